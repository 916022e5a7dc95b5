"""The directed update cases of tests/update_cases.py on the device (yrwi_add_postings /
yrwi_remove_postings): after every step the call's stats are the seven the case computed by
construction, every list of the case -- bystanders included -- equals the expected one byte for byte,
the url dictionary is consistent, the index statistics are the expected totals and six queries over the
case's terms equal the oracle on the expected lists; after a case's last step the hits also equal those
of a fresh index built in full.  Add cases run under every policy they name, remove cases at
YRWI_RM_CHUNK unset, 256 and 4096.  (tests/test_update_cases_ref.py checks the same expectations
against tests/update_ref.py on the CPU, and the edges the cases claim to reach.)"""

import numpy as np
import pytest

import index_util as iu
import update_cases as uc
from yacy_search_server_amd._lib import YrwiError

pytestmark = pytest.mark.gpu

LIGHT = ("jobs_4097", "jobs_65537", "three_pieces")
ADDS = [(n, p) for n, ps in uc.names() for p in ps if not n.startswith(("rm_", "atomic_")) and n not in LIGHT]
REMOVES = [n for n, _ in uc.names() if n.startswith("rm_")]
ATOMIC = [n for n, _ in uc.names() if n.startswith("atomic_")]


def _stats(st):
    return {k: st[k] for k in iu.STAT_KEYS}


def _totals(lists):
    return (len(lists), sum(len(r) for r in lists.values()))


def _do(ix, s):
    """one step on the device; -> its stats"""
    if s.op == "add":
        st = ix.add_postings(s.terms, s.rows, s.policy)
        assert st["added"] + st["replaced"] + st["dropped"] == len(s.rows), (st, len(s.rows))
        return st
    if s.op == "remove":
        return ix.remove_postings(s.urls, s.names)
    before = ix.stats()
    with pytest.raises(YrwiError) as e:
        ix.add_postings(s.terms, s.rows, s.policy)
    assert e.value.rc == s.rc, (e.value.rc, s.rc)
    assert ix.stats() == before
    return None


def _run(c, monkeypatch, after=None):
    qs = c.queries()
    ix = iu.open_index(c.lists)
    try:
        ix.build_url_ids()
        for k, s in enumerate(c.steps):
            st = _do(ix, s)
            if st is not None:
                assert _stats(st) == s.stats, (c.name, k, st, s.stats)
            iu.same_lists(ix, s.lists, c.watch)
            ix.build_url_ids()
            bad = ix.check_url_ids()[0]
            assert bad == 0, (c.name, k, bad)
            assert ix.stats()[:2] == _totals(s.lists), (ix.stats(), _totals(s.lists))
            got, exp = iu.hits(ix, qs), iu.oracle_hits(s.lists, qs)
            assert got == exp, (c.name, k) + iu._first_difference(got, exp)
            if after:
                after(ix, s, st)
        iu.verify_step(ix, c.steps[-1].lists, c.watch, qs, monkeypatch)
    finally:
        ix.close()


@pytest.mark.parametrize("name,policy", ADDS, ids=["%s-%s" % a for a in ADDS])
def test_add(name, policy, monkeypatch):
    c = uc.build(name, policy)

    def joins(ix, s, st):
        """near_keys: a mis-ordered list shows in a join as well, on the probe path and on the merge path"""
        for ratio in ("1", "1000000000"):
            monkeypatch.setenv("YRWI_PROBE_RATIO", ratio)
            jq = [(inc, []) for inc in c.facts["joins"]]
            got, exp = iu.hits(ix, jq), iu.oracle_hits(s.lists, jq)
            assert all(len(e) >= 30 for e in exp)
            assert got == exp, (ratio,) + iu._first_difference(got, exp)
        monkeypatch.delenv("YRWI_PROBE_RATIO")

    _run(c, monkeypatch, joins if name == "near_keys" else None)


@pytest.mark.parametrize("chunk", [None, 256, 4096])
@pytest.mark.parametrize("name", REMOVES)
def test_remove(name, chunk, monkeypatch):
    iu.set_rm_chunk(monkeypatch, chunk)

    def no_chunk(ix, s, st):
        """rm_everything: an emptied list needs no compaction, so the call is its marking pass alone (the
        upload, the memset, k_rm_count, the read-back) and its two waits, whatever the chunk size"""
        assert (st["launches"], st["syncs"]) == (4, 2), st

    _run(uc.build(name), monkeypatch, no_chunk if name == "rm_everything" else None)


@pytest.mark.parametrize("name", ATOMIC)
def test_errors_are_atomic(name, monkeypatch):
    _run(uc.build(name), monkeypatch)


@pytest.mark.parametrize("name", LIGHT)
def test_many_lists(name):
    """too many lists, or rows, for a fresh build and queries: the stats, the index statistics, the size of
    every list, the bytes of the lists that were there before and of up to 517 sampled ones, the url ids"""
    c = uc.build(name)
    s = c.steps[0]
    ix = iu.open_index(c.lists)  # (jobs_*: five lists)
    try:
        st = ix.add_postings(s.terms, s.rows, s.policy)
        assert _stats(st) == s.stats, (st, s.stats)
        assert st["added"] + st["replaced"] + st["dropped"] == len(s.rows)
        assert ix.stats()[:2] == _totals(s.lists)
        terms = [bytes(t) for t in c.facts["terms"]]
        assert set(terms) == set(s.lists)
        sizes = np.array([ix.get_size(t) for t in terms])
        want = np.array([len(s.lists[t]) for t in terms])
        assert (sizes == want).all(), np.flatnonzero(sizes != want)[:8]
        iu.same_lists(ix, s.lists, c.facts["prebuilt"] + c.sample)
        bad = ix.check_url_ids()[0]
        assert bad == 0, bad
    finally:
        ix.close()
