"""GPU parity (MI355X) of yrwi_term_search_batch: the joined and excluded containers of many
TermSearch descriptors in one pass, compacted on the device into one packed image.

Every comparison of rows is byte equality against both oracle.term_search and the existing
per-query path (RWIIndex.term_search: yrwi_join_exclude / yrwi_term_search).  The inputs are
those of term_batch_cases.py, whose lengths and removal positions
tests/test_term_batch_cases_ref.py asserts on the oracle."""

import ctypes
import os

import numpy as np
import pytest

import event_local_cases as E
import term_batch_cases as C
from index_util import open_index, run_parts
from yacy_search_server_amd import Query
from yacy_search_server_amd._lib import YrwiError, lib

pytestmark = pytest.mark.gpu

NOW, INF = C.NOW, C.INF
E_ARG, E_HASH, E_UNSUPPORTED = -1, -2, -8


@pytest.fixture(scope="module")
def ix():
    x = open_index(C.index_dict(), url_ids=True)
    yield x
    x.close()


@pytest.fixture(scope="module")
def tiny():
    x = open_index(E.corpus("tiny")[2], url_ids=True)
    yield x
    x.close()


def _query(q):
    inc, exc, maxd, now, sel = q
    return Query(list(inc), list(exc), maxd, now_ms=now, urlselection=None if sel is None else list(sel))


_single_cache = {}


def _per_query(index, q):
    """what the existing per-query call returns for the descriptor (once per index, query and fold mode)"""
    key = (id(index), q, os.environ.get("YRWI_NO_CHAIN"))
    if key not in _single_cache:
        inc, exc, maxd, now, sel = q
        _single_cache[key] = index.term_search(list(inc), list(exc), maxd, now,
                                               urlselection=None if sel is None else list(sel))
    return _single_cache[key]


def _check_batch(index, qs, pinned=False, preset=None):
    """one batch call; every range equal to the oracle and to the per-query call"""
    got, st = index.term_search_batch([_query(q) for q in qs], pinned=pinned)
    assert len(got) == len(qs)
    for i, (q, g) in enumerate(zip(qs, got)):
        exp = C.expected(q, preset)
        assert g.shape == exp.shape and np.array_equal(g, exp), (i, q[:2], "vs oracle")
        one = _per_query(index, q)
        assert g.shape == one.shape and np.array_equal(g, one), (i, q[:2], "vs yrwi_term_search")
    assert st.rows_out == sum(len(g) for g in got) and st.rows_joined >= st.rows_out
    assert st.direct == (1 if pinned and st.rows_joined > 0 else 0)
    return got, st


def _raw(index, qs, rows, cap, fill=-7):
    off = np.full(len(qs) + 1, fill, dtype=np.int64)
    rc, st = index.term_search_batch_raw([_query(q) for q in qs], rows, cap, off)
    return rc, st, off


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("pinned", [False, True])
def test_tile_edges(ix, pinned):
    qs = C.tile_edge_queries()
    for q in qs:  # each alone
        got, _ = _check_batch(ix, [q], pinned)
        assert len(got[0]) in C.EDGES
    _check_batch(ix, C.shuffled(qs, 3), pinned)  # and all in one batch


# ------------------------------------------------------------------ 2
def test_empties_and_offsets(ix):
    qs = C.empties_batch()
    _check_batch(ix, qs)
    rows = np.zeros((770, 40), dtype=np.uint8)
    rc, st, off = _raw(ix, qs, rows, 770)
    assert rc == 0 and list(off) == [0, 0, 257, 257, 257, 770, 770]
    # (a chained fold applies its exclusion within the join: the all-excluded container may be gone already)
    assert st.rows_out == 770 and st.rows_joined in (770, 770 + C.N)
    for name, q in C.EMPTIES.items():  # alone, and a batch of nothing but empties
        got, st = _check_batch(ix, [q])
        assert len(got[0]) == 0 and st.rows_out == 0, name
    got, st = _check_batch(ix, list(C.EMPTIES.values()) * 2)
    assert all(len(g) == 0 for g in got)


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("chain", [True, False])
@pytest.mark.parametrize("pinned", [False, True])
def test_removal_positions(ix, pinned, chain, monkeypatch):
    """chain=False (YRWI_NO_CHAIN=1, read per call): the two-term folds run step by step and
    their exclusions leave marks for the compaction, as a single list's always does; chained,
    a fold drops its excluded rows within the join"""
    if not chain:
        monkeypatch.setenv("YRWI_NO_CHAIN", "1")
    qs = C.removal_queries()
    got, st = _check_batch(ix, qs, pinned)
    assert [len(g) for g in got] == [C.N - len(C.REMOVALS[n]) for n in C.REMOVALS for _ in range(2)]
    assert st.rows_joined >= len(qs) // 2 * C.N + st.rows_out // 2  # every single list arrives whole
    if not chain:
        assert st.rows_joined == len(qs) * C.N
    for q in qs:
        _check_batch(ix, [q], pinned)


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("mixed", [False, True])
def test_past_one_scan_block(ix, mixed):
    qs = C.past_scan_block(mixed)
    got, st = _check_batch(ix, qs, pinned=mixed)
    assert st.rows_out == 300 * 257 + (6400 if mixed else 0)
    assert len({g.ctypes.data for g in got}) == len(qs)  # identical descriptors, each its own range


# ------------------------------------------------------------------ 5
def test_per_job_state(ix):
    qs = C.per_job_batch()
    got, _ = _check_batch(ix, qs)
    assert not np.array_equal(got[0], got[1])  # the same join at two request times
    reps = [i for i, q in enumerate(qs) if q == qs[2]]
    assert len(reps) == 3 and all(np.array_equal(got[i], got[2]) for i in reps)
    _check_batch(ix, qs, pinned=True)
    # a quoted fold with a url selection is refused as yrwi_term_search refuses it, and named
    bad = C.Q(C.SEL2[0], (), 1, NOW, C.SEL2[4])
    rows = np.full((4000, 40), 0xA5, dtype=np.uint8)
    rc, _, off = _raw(ix, [C.joined(257), C.SEL1, bad], rows, 4000)
    assert rc == E_UNSUPPORTED and (off == -7).all() and (rows == 0xA5).all()
    assert lib().yrwi_last_error(ix._h).decode().startswith("query 2: ")


# ------------------------------------------------------------------ 6
def test_random_sweep(tiny):
    qs = C.sweep_queries()
    _check_batch(tiny, qs, preset="tiny")
    _check_batch(tiny, qs, pinned=True, preset="tiny")


# ------------------------------------------------------------------ 7
def test_capacity_and_count_only(ix):
    qs = C.removal_queries() + [C.EMPTIES["empty_join"], C.joined(513)]
    exp = np.concatenate([C.expected(q) for q in qs])
    total = len(exp)
    want = np.cumsum([0] + [len(C.expected(q)) for q in qs])
    assert total >= 64
    pin = ix.host_array(ctypes.c_uint8, 40 * (total + 8))
    for name in ("numpy", "pinned"):
        buf = np.zeros(40 * (total + 8), dtype=np.uint8) if name == "numpy" else np.ctypeslib.as_array(pin)
        buf[:] = 0xA5
        rc, st, off = _raw(ix, qs, buf, total - 1)
        assert rc == E_ARG and (off == want).all(), name  # the offsets say what a retry needs
        assert (buf == 0xA5).all(), name
        assert st.rows_out == total and st.bytes_d2h < 40 * st.rows_out and st.direct == 0
        rc, st, off = _raw(ix, qs, buf, total)
        assert rc == 0 and (off == want).all() and st.direct == (name == "pinned")
        assert np.array_equal(buf[:40 * total].reshape(-1, 40), exp), name
        assert (buf[40 * total:] == 0xA5).all(), name
    rc, st, off = _raw(ix, qs, None, 0)  # count only
    assert rc == 0 and (off == want).all()
    assert st.rows_out == total and st.bytes_d2h < 40 * st.rows_out and st.direct == 0
    rc, st, off = _raw(ix, qs, None, -3)  # ... whatever cap_rows says
    assert rc == 0 and (off == want).all()


# ------------------------------------------------------------------ 8
def test_buffers(ix):
    qs = C.shuffled(C.tile_edge_queries(), 5) + [C.joined(C.N, (C.xterm("middle_tile"),))]
    exp = np.concatenate([C.expected(q) for q in qs])
    total = len(exp)
    pin = np.ctypeslib.as_array(ix.host_array(ctypes.c_uint8, 40 * total + 8))
    assert pin.ctypes.data % 8 == 0
    outs = {}
    for name, buf, direct in (("pinned", pin, 1), ("numpy", np.zeros(40 * total + 8, dtype=np.uint8), 0),
                              ("pinned+4", pin[4:], 0)):
        buf[:] = 0xA5
        rc, st, off = _raw(ix, qs, buf, total)
        assert rc == 0 and off[-1] == total and st.direct == direct, name
        outs[name] = buf[:40 * total].copy()
        assert np.array_equal(outs[name].reshape(-1, 40), exp), name
        assert (buf[40 * total:] == 0xA5).all(), name
    assert np.array_equal(outs["pinned"], outs["numpy"]) and np.array_equal(outs["pinned"], outs["pinned+4"])


# ------------------------------------------------------------------ 9
def _dense_queries():
    h = C.dense_terms
    """four kinds of fold, each with rows left: 3 terms and an exclusion, 2 terms, 2 terms and an
    exclusion, one list and an exclusion"""
    return [C.Q(h((0, 1, 2)), h((3,))), C.Q(h((0, 1))), C.Q(h((0, 1)), h((3,))), C.Q(h((4,)), h((5,)))]


def _shape(index, qs, n, pinned):
    batch = [_query(qs[i % len(qs)]) for i in range(n)]
    rows, st = index.term_search_batch(batch, pinned=pinned)
    assert st.rows_out == sum(len(r) for r in rows) > 0
    return st


def test_shape_of_the_call(ix):
    """the library's own counters (no times): launches and host waits do not depend on the
    number of queries or on the list lengths, the bytes over PCIe beyond the rows themselves
    not on the list lengths, and a call allocates nothing on the device (measured after a
    first call has sized the lane's scratch and staging, as for every other entry point)"""
    qs = _dense_queries()
    kinds = [[q] for q in qs] + [qs]  # like with like: each kind of query alone, and the four together
    for pinned in (False, True):  # the largest batches first: scratch and staging reach their size
        for kind in kinds:
            _shape(ix, kind, 64, pinned)
    assert lib().yrwi_settle_scratch(ix._h) == 0
    tenth = open_index({h: rows[:max(1, len(rows) // 10)] for h, rows in E.corpus("dense")[2].items()},
                       url_ids=True)
    try:
        for pinned in (False, True):
            for kind in kinds:
                s1, s64 = _shape(ix, kind, len(kind), pinned), _shape(ix, kind, 64, pinned)
                print("pinned", pinned, "nq", len(kind), "/ 64: launches_tail", s1.launches_tail, s64.launches_tail,
                      "syncs", s1.syncs, s64.syncs, "allocs", s1.device_allocs, s64.device_allocs)
                assert s1.direct == s64.direct == int(pinned)
                assert s1.launches_tail == s64.launches_tail and s1.syncs == s64.syncs
                assert s1.device_allocs == 0 and s64.device_allocs == 0
            # the same terms with every list cut to its first tenth: fewer rows, the same shape
            _shape(tenth, qs, 4, pinned)
            l4, t4 = _shape(ix, qs, 4, pinned), _shape(tenth, qs, 4, pinned)
            print("dense / tenth: rows joined", l4.rows_joined, t4.rows_joined, "h2d", l4.bytes_h2d, t4.bytes_h2d,
                  "d2h beyond the rows", l4.bytes_d2h - 40 * l4.rows_out, t4.bytes_d2h - 40 * t4.rows_out)
            assert t4.rows_joined < l4.rows_joined // 5
            assert t4.launches_tail == l4.launches_tail == s64.launches_tail and t4.syncs == l4.syncs == s64.syncs
            assert t4.bytes_h2d == l4.bytes_h2d
            assert t4.bytes_d2h - 40 * t4.rows_out == l4.bytes_d2h - 40 * l4.rows_out
        # the pageable path waits once more than the direct one, for its one copy
        p, d = _shape(ix, qs, 4, False), _shape(ix, qs, 4, True)
        assert p.syncs == d.syncs + 1 and p.launches_tail == d.launches_tail + 1
    finally:
        tenth.close()


# ------------------------------------------------------------------ 10
def test_errors(ix):
    qs = [C.joined(257)] * 5 + [C.Q((b"not*base64!!",))] + [C.single(255)] * 2
    rows = np.full((8 * 257, 40), 0xA5, dtype=np.uint8)
    rc, _, off = _raw(ix, qs, rows, 8 * 257)
    assert rc == E_HASH and (off == -7).all() and (rows == 0xA5).all()
    assert "query 5" in lib().yrwi_last_error(ix._h).decode()
    off = np.full(1, -7, dtype=np.int64)
    assert lib().yrwi_term_search_batch(ix._h, None, 0, None, 0, off.ctypes.data, None) == 0 and off[0] == 0
    assert ix.term_search_batch([])[0] == []
    assert lib().yrwi_term_search_batch(ix._h, None, -1, None, 0, off.ctypes.data, None) == E_ARG
    cq = ix._marshal([_query(C.joined(1))], 1)
    assert lib().yrwi_term_search_batch(ix._h, cq[0], 1, None, 0, None, None) == E_ARG  # no row_off
    assert lib().yrwi_term_search_batch(ix._h, None, 1, None, 0, off.ctypes.data, None) == E_ARG  # no queries
    _check_batch(ix, [C.joined(257)])  # and the context still answers


def test_sharded_context_is_refused():
    def fn(r, x):
        if r:
            return
        with pytest.raises(YrwiError) as e:
            x.term_search_batch([Query([C.ABSENT], now_ms=NOW)])
        assert e.value.rc == E_UNSUPPORTED

    run_parts([{}, {}], 2, fn, timeout=120)


# ------------------------------------------------------------------ 11
def test_nothing_else_moved(ix):
    h = C.dense_terms
    batch = [Query(h((0, 1)), now_ms=NOW), Query(h((0, 1, 2)), h((3,)), now_ms=NOW), Query(h((4,)), now_ms=NOW)]
    hits = lambda: [[(x.urlhash, x.score, x.tiebreak) for x in g] for g in ix.search_batch(batch)]
    before, stats = hits(), ix.stats()
    one = ix.term_search(h((0, 1)), h((2,)), INF, NOW)
    assert all(before)
    _check_batch(ix, C.per_job_batch())
    _check_batch(ix, C.removal_queries(), pinned=True)
    assert hits() == before and ix.stats() == stats
    assert np.array_equal(ix.term_search(h((0, 1)), h((2,)), INF, NOW), one)
    assert np.array_equal(one, C.expected(C.Q(h((0, 1)), h((2,)))))
