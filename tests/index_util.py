"""Shared helpers of the tests that open a device index: hand-made hashes and rows, the 40-query
batch of the maintenance tests with its oracle, the checks every maintenance step ends with, and the
threads that drive the shard contexts of one process over the loopback transport.

A plain module (no fixtures, no tests): pytest does not rewrite its asserts, so each one carries its
operands in its message.  It imports without the built library (tests/dump_ref.py takes its hashes and
rows from here), so nothing at module level calls into it: the C5 profile is parsed where it is used."""

import os
import threading

import numpy as np

import oracle as orc
import update_ref as ur
from yacy_search_server_amd import Query, RankingProfile, RWIIndex

NOW = 20741 * 86400000 + 4242
C5 = "date=15,domlength=15,authority=13,tf=10"  # the authority profile: every second query of batch()
B64 = ur._B64
STAT_KEYS = ("terms", "new_terms", "emptied_terms", "added", "replaced", "dropped", "removed")
EMPTY = np.zeros((0, 40), np.uint8)


# ------------------------------------------------------------------ hashes and rows
def enc(i, width):
    out = bytearray()
    for _ in range(width):
        out.append(B64[i & 63])
        i >>= 6
    return bytes(reversed(out))


def url(i, prefix=b"__"):
    """url hashes the synthetic index does not have (the fixtures check), ascending in i"""
    return prefix + enc(i, 10)


def term(i, prefix=b"-t"):
    return prefix + enc(i, 10)


def rows(idx, urls, lm=None, start=0):
    """hand-made rows: rows of the synthetic index as templates, the url hash (and lastModified) set"""
    r = idx.rows[(start + 13 * np.arange(len(urls))) % len(idx.rows)].copy()
    for i, u in enumerate(urls):
        r[i, :12] = np.frombuffer(u, dtype=np.uint8)
    if lm is not None:
        lm = np.broadcast_to(np.asarray(lm), (len(urls),))
        r[:, 12], r[:, 13] = lm >> 8, lm & 255
    return r


# ------------------------------------------------------------------ one index
def open_index(lists, url_ids=False):
    ix = RWIIndex(0)
    for h, r in lists.items():
        ix.add(h, r)
    if url_ids:
        ix.build_url_ids()
    return ix


def batch(qs):
    """default and authority profiles alternating"""
    c5 = RankingProfile("", C5)
    return [Query(inc, exc, now_ms=NOW, k=50, profile=(c5 if i % 2 else None)) for i, (inc, exc) in enumerate(qs)]


def hits(ix, qs):
    return [[(h.urlhash, h.score, h.tiebreak) for h in r] for r in ix.search_batch(batch(qs))]


def oracle_hits(lists, qs):
    out, c5 = [], orc.profile_from(RankingProfile("", C5))
    for qi, (inc, exc) in enumerate(qs):
        d = {h: lists[h] for h in inc + exc if h in lists}
        out.append(orc.search(d, inc, exc, profile=(c5 if qi % 2 else None), now_ms=NOW, k=50))
    return out


def _first_difference(got, exp):
    """the first query whose hits differ, for an assert's message"""
    qi = next((i for i, (g, e) in enumerate(zip(got, exp)) if g != e), min(len(got), len(exp)))
    return ("query", qi, len(got), len(exp), got[qi:qi + 1], exp[qi:qi + 1])


def same_lists(ix, lists, touched):
    for t in touched:
        exp = lists.get(t, EMPTY)
        assert ix.get_size(t) == len(exp), (t, ix.get_size(t), len(exp))
        assert ix.get_list(t).tobytes() == exp.tobytes(), t


def verify_step(ix, lists, touched, qs, monkeypatch):
    """the four checks of a step: the touched lists byte for byte, a consistent url dictionary, the index
    statistics, and the hits of the batch equal to the oracle's and to those of a fresh index built in full"""
    same_lists(ix, lists, touched)
    bad = ix.check_url_ids()[0]
    assert bad == 0, bad
    nterms, npost, _ = ix.stats()
    want = (len(lists), sum(len(r) for r in lists.values()))
    assert (nterms, npost) == want, ((nterms, npost), want)
    got = hits(ix, qs)
    exp = oracle_hits(lists, qs)
    assert got == exp, _first_difference(got, exp)
    monkeypatch.setenv("YRWI_DICT_FULL", "1")
    fresh = open_index(lists)
    try:
        bad = fresh.check_url_ids()[0]
        assert bad == 0, ("fresh", bad)
        again = hits(fresh, qs)
        assert got == again, ("fresh",) + _first_difference(got, again)
    finally:
        fresh.close()
        monkeypatch.delenv("YRWI_DICT_FULL")


def checked_add(ix, lists, terms, rows, policy="replace"):
    """add on the device and on the reference; the stats must agree"""
    st = ix.add_postings(terms, rows, policy)
    new, exp = ur.apply_add(lists, terms, rows, policy)
    assert {k: st[k] for k in STAT_KEYS} == exp, (st, exp)
    assert st["added"] + st["replaced"] + st["dropped"] == len(rows), (st, len(rows))
    return new, st


def checked_remove(ix, lists, urls, terms=None):
    st = ix.remove_postings(urls, terms)
    new, exp = ur.apply_remove(lists, urls, terms)
    assert {k: st[k] for k in STAT_KEYS} == exp, (st, exp)
    return new, st


def set_rm_chunk(monkeypatch, chunk):
    """rows compacted at a time (None: the default, one chunk on the `tiny` corpus)"""
    if chunk is None:
        monkeypatch.delenv("YRWI_RM_CHUNK", raising=False)
    else:
        monkeypatch.setenv("YRWI_RM_CHUNK", str(chunk))


# ------------------------------------------------------------------ shards of one process
def loop_id():
    return b"YRWI-LOOPBACK\0" + os.urandom(114)


def split_by_rank(lists, world):
    """per-rank {term hash: the rows of the rank's url-hash range}, empty parts dropped
    (Distribution.verticalDHTPosition, world 2: the top bit of the first character)"""
    assert world == 2, world
    rank_of = lambda l: np.array([ur.url_key(bytes(r[:12]))[0] >> 5 for r in l])
    parts = [{t: l[rank_of(l) == r] for t, l in lists.items()} for r in range(world)]
    return [{t: l for t, l in p.items() if len(l)} for p in parts]


def _open_shard(r, world, uid):
    return RWIIndex(0, shard=(r, world, uid))


def run_parts(parts, world, fn, timeout=300, open_rank=None):
    """parts: per-rank {term hash: rows}; fn(rank, index) runs on every rank's own thread (the same call
    sequence on every rank); -> the per-rank results.  Both phases, opening and fn, fail the call when a
    rank raises or is still running `timeout` seconds after its join began.  Once every thread has ended,
    every context that was opened is closed, whatever failed; under a running thread nothing is closed.
    open_rank(rank, world, uid) -> the rank's context (default: a shard over the loopback transport)."""
    uid = loop_id()
    open_rank = open_rank or _open_shard
    ixs, out, errs = [None] * world, [None] * world, []

    def opening(r):
        ixs[r] = open_rank(r, world, uid)
        for h, rows_ in parts[r].items():
            ixs[r].add(h, rows_)

    def running(r):
        out[r] = fn(r, ixs[r])

    def guarded(phase, r):
        try:
            phase(r)
        except BaseException as e:  # reported below, with its rank
            errs.append((r, phase.__name__, repr(e)))

    alive = []
    try:
        for phase in (opening, running):
            ths = [threading.Thread(target=guarded, args=(phase, r)) for r in range(world)]
            for t in ths:
                t.start()
            for t in ths:
                t.join(timeout=timeout)
            alive = [r for r, t in enumerate(ths) if t.is_alive()]
            assert not alive, ("ranks still %s after %s s" % (phase.__name__, timeout), alive)
            assert not errs, sorted(errs)
    finally:
        if not alive:
            for ix in ixs:
                if ix is not None:
                    ix.close()
    return out
