"""The streaming passes of the maintenance calls past a workgroup's first tile: the host calls, the census,
retention and the url references on the one large index of tests/span_cases.py (2^21 + 1 + 4096 postings: every
workgroup's span is two tiles), each against the expectation computed from the arrays the index was made
from.  tests/test_span_cases_ref.py checks those expectations against the references and that the hits lie
where the cases say: in a second tile only, in a first tile only, in both."""

import ctypes

import numpy as np
import pytest

import index_util as iu
import refs_ref as rr
import retention_ref as tr
import span_cases as sc
from yacy_search_server_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus():
    c = sc.corpus()
    return c, c.lists()


@pytest.fixture(scope="module")
def index(corpus):
    """the context of the calls that change nothing"""
    c, lists = corpus
    ix = iu.open_index(lists)
    yield ix
    ix.close()


def _unchanged(ix, c):
    assert ix.stats()[:2] == (len(c.terms), c.n)


# ------------------------------------------------------------------ hosts
@pytest.mark.parametrize("n", [64, 2049])
def test_count_hosts(corpus, index, n):
    """64 hosts are searched and counted in LDS, 2049 in global memory"""
    c, lists = corpus
    keys = sc.host_set(n)
    exp, lists_hit, _ = sc.expect_count_hosts(c, keys)
    counts, hit = index.count_hosts(sc.host_hashes(keys), c.terms)
    assert list(counts) == exp and hit == lists_hit
    _unchanged(index, c)


@pytest.mark.parametrize("n", [64, 2049])
def test_remove_hosts(corpus, n, monkeypatch):
    c, lists = corpus
    iu.set_rm_chunk(monkeypatch, None)
    keys = sc.host_set(n)
    new, exp = sc.expect_remove_hosts(c, keys)
    ix = iu.open_index(lists)
    try:
        st = ix.remove_hosts(sc.host_hashes(keys), c.terms)
        assert {k: st[k] for k in iu.STAT_KEYS} == exp, (st, exp)
        assert ix.stats()[:2] == (len(new), c.n - exp["removed"])
        iu.same_lists(ix, new, c.terms)
    finally:
        ix.close()


# ------------------------------------------------------------------ census
@pytest.mark.parametrize("lds_slots", [None, 64])
def test_host_census(corpus, index, lds_slots, monkeypatch):
    """64 slots of LDS hold the hosts of a span's first tile: those of its second tile go past it"""
    c, lists = corpus
    if lds_slots is None:
        monkeypatch.delenv("YRWI_CENSUS_LDS_SLOTS", raising=False)
    else:
        monkeypatch.setenv("YRWI_CENSUS_LDS_SLOTS", str(lds_slots))
    monkeypatch.delenv("YRWI_CENSUS_SLOTS", raising=False)
    for order in ("host", "count"):
        for minp in (1, sc.CENSUS_CUT):
            hosts, counts, exp = sc.expect_census(c, order, minp)
            got_h, got_c, st = index.host_census(c.terms, order, minp)
            assert got_h == hosts and list(got_c) == counts, (order, minp)
            assert {k: st[k] for k in exp} == exp, (st, exp)
            if lds_slots == 64:  # the hosts of a first tile fill the table: those of the second find no place
                floor = sc.census_bypass_floor(c, 64)
                assert st["lds_bypass"] >= floor > 1000 * sc.SPAN_TILE - 16 * 4096, (st["lds_bypass"], floor)
    _unchanged(index, c)


# ------------------------------------------------------------------ retention
def test_retention_count(corpus, index):
    c, lists = corpus
    _, _, exp, hist, _ = sc.expect_retention(c, sc.MIN_DAY, sc.MAX_REFS)
    st, h = index.retention_count(sc.MIN_DAY, sc.MAX_REFS, c.terms, hist=True)
    assert {k: st[k] for k in tr.COUNT_KEYS} == exp, (st, exp)
    assert (h == hist).all()
    assert st["hist_bypass"] == sc.expect_hist_bypass(c) == 1050624
    _unchanged(index, c)


def test_retain(corpus, monkeypatch):
    """the age rule and a cap of two rows: the cap cuts the 8192-row list on a tied day, and three-row lists"""
    c, lists = corpus
    iu.set_rm_chunk(monkeypatch, None)
    new, exp, rexp, _, _ = sc.expect_retention(c, sc.MIN_DAY, sc.MAX_REFS)
    ix = iu.open_index(lists)
    try:
        st, rst = ix.retain(sc.MIN_DAY, sc.MAX_REFS, c.terms)
        assert {k: st[k] for k in iu.STAT_KEYS} == exp, (st, exp)
        assert {k: rst[k] for k in tr.COUNT_KEYS} == rexp, (rst, rexp)
        assert ix.stats()[:2] == (len(new), c.n - exp["removed"])
        iu.same_lists(ix, new, c.terms)
    finally:
        ix.close()


# ------------------------------------------------------------------ references
@pytest.mark.parametrize("n", [2047, 2049])
def test_url_references(corpus, index, n, monkeypatch):
    """2047 urls are searched in LDS, 2049 in global memory; the streaming path, named"""
    c, lists = corpus
    monkeypatch.setenv("YRWI_REFS_PATH", "stream")
    uhi, uhost = sc.url_set(c, n)
    urls = sc.url_hashes(uhi, uhost)
    counts, exp, by, _ = sc.expect_refs(c, uhi, uhost)
    got, _, _, st = index.url_references(urls, c.terms, fetch=False)
    assert (got == counts).all() and {k: st[k] for k in exp} == exp, (st, exp)
    assert st["path"] == _lib.REFS_STREAM
    refs = exp["refs"]
    pinned = np.ctypeslib.as_array(index.host_array(ctypes.c_uint8, 40 * refs))
    for order in rr.ORDERS:
        for kind, buf, direct in (("pinned", pinned, 1), ("pageable", np.zeros(40 * refs, dtype=np.uint8), 0)):
            buf[:] = 0xA5
            got, terms, rows, st = index.url_references(urls, c.terms, order, rows_out=buf)
            assert (got == counts).all() and {k: st[k] for k in exp} == exp, (order, kind, st, exp)
            assert (st["path"], st["direct"]) == (_lib.REFS_STREAM, direct), (order, kind)
            assert terms.tobytes() == by[order][0].tobytes(), (order, kind)
            assert rows.tobytes() == by[order][1].tobytes(), (order, kind)
    _unchanged(index, c)
