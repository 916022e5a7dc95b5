"""Batched term search (yrwi_term_search_batch), the part that runs without a GPU.

The library exports the entry point, the Python class carries it, and the argument errors
that need no device are answered.  The rest is reference-only: with oracle.term_search alone,
every input of tests/test_gpu_term_batch.py (term_batch_cases.py) has the lengths and the
removal positions it claims -- containers of exactly 1 .. 513 rows, exclusions that remove the
first or last row of every k_local_count tile, a whole tile, all rows but one, the two rows on
a tile edge; empty containers of three kinds; more than 256 tiles and more than 256 jobs."""

import ctypes

import numpy as np

import term_batch_cases as C
from yacy_search_server_amd import _lib, rwi

LR_TILE = C.LR_TILE


def test_symbol_struct_and_null_arguments():
    L = _lib.lib()
    assert hasattr(L, "yrwi_term_search_batch") and "yrwi_term_search_batch" in _lib.SIGNATURES
    assert callable(getattr(rwi.RWIIndex, "term_search_batch", None))
    assert callable(getattr(rwi.RWIIndex, "term_search_batch_raw", None))
    # the struct layout of include/yrwi.h
    S = _lib.CTsbStats
    assert ctypes.sizeof(S) == 72 and S.launches_tail.offset == 32 and S.direct.offset == 40
    assert S.device_allocs.offset == 48 and S.t_total_ns.offset == 64
    st = S()
    st.syncs = 7
    off = np.full(2, -5, dtype=np.int64)
    assert L.yrwi_term_search_batch(None, None, 1, None, 0, off.ctypes.data, ctypes.byref(st)) == -1  # YRWI_E_ARG
    assert st.syncs == 0 and (off == -5).all()  # the statistics are cleared even then
    assert L.yrwi_term_search_batch(None, None, 0, None, 0, off.ctypes.data, None) == -1


def _urls(rows):
    return [bytes(r[:12]) for r in rows]


def test_tile_edge_containers_have_their_lengths():
    uni = C.universe()[1]
    assert len(uni) == C.N == 3 * LR_TILE and uni == sorted(set(uni), key=uni.index)
    assert set(C.EDGES) == {1, LR_TILE - 1, LR_TILE, LR_TILE + 1, 2 * LR_TILE - 1, 2 * LR_TILE, 2 * LR_TILE + 1}
    d = C.universe()[0]
    for n in C.EDGES:
        j, s = C.expected(C.joined(n)), C.expected(C.single(n))
        assert len(j) == len(s) == n and _urls(j) == _urls(s) == uni[:n], n
        assert (s == d[C.prefix(n)]).all()  # one include term: the rows as stored ...
        assert s[:, 28].all() and s[:, 39].all()
        assert not j[:, 28].any() and not j[:, 39].any()  # ... a joined record is re-encoded
        assert (j[:, 12:] != s[:, 12:]).any(axis=1).all()
    assert sorted(C.tile_edge_queries()) == sorted(set(C.tile_edge_queries())) and len(C.tile_edge_queries()) == 14
    assert C.shuffled(C.tile_edge_queries(), 3) != C.tile_edge_queries()


def test_empty_containers_are_empty_for_three_reasons():
    d = C.index_dict()
    assert C.ABSENT not in d
    assert not set(_urls(d[C.LOW])) & set(_urls(d[C.HIGH]))
    assert _urls(d[C.XALL]) == C.universe()[1]
    for name, q in C.EMPTIES.items():
        assert len(C.expected(q)) == 0, name
    assert len(C.expected(C.Q(*C.EMPTIES["all_excluded"][:1]))) == C.N  # ... which has N rows before its exclusion
    b = C.empties_batch()
    lens = [len(C.expected(q)) for q in b]
    assert lens == [0, 257, 0, 0, 513, 0]


def test_removal_positions():
    uni = C.universe()[1]
    tiles = lambda pos: {p // LR_TILE for p in pos}
    R = C.REMOVALS
    assert R["first_of_tile"] == [t * LR_TILE for t in range(3)]
    assert R["last_of_tile"] == [t * LR_TILE + LR_TILE - 1 for t in range(3)]
    assert R["middle_tile"] == list(range(LR_TILE, 2 * LR_TILE))
    assert len(R["all_but_one"]) == C.N - 1 and tiles(R["all_but_one"]) == {0, 1, 2}
    assert R["rows_255_256"] == [LR_TILE - 1, LR_TILE]
    for name, pos in R.items():
        keep = [u for i, u in enumerate(uni) if i not in set(pos)]
        for f in (C.joined, C.single):
            assert len(C.expected(f(C.N))) == C.N
            assert _urls(C.expected(f(C.N, (C.xterm(name),)))) == keep, (name, f.__name__)
    assert len(C.removal_queries()) == 10


def test_past_one_scan_block():
    qs = C.past_scan_block(False)
    assert len(qs) == 300 > 256 and {len(C.expected(q)) for q in qs} == {257}
    assert sum((257 + LR_TILE - 1) // LR_TILE for _ in qs) == 600
    a, b = C.expected(qs[0]), C.expected(qs[1])  # the request times alternate: freshUntil differs
    assert qs[0] != qs[1] and qs[0] == qs[2] and (a[:, :12] == b[:, :12]).all() and (a != b).any()
    mixed = C.past_scan_block(True)
    assert len(mixed) == 301 and mixed[150] == C.DENSE_INC2 and len(C.expected(C.DENSE_INC2)) == 6400


def test_per_job_state_queries():
    b = C.per_job_batch()
    a0, a1 = C.expected(b[0]), C.expected(b[1])
    assert len(a0) == len(a1) == 513 and (a0 != a1).any()
    assert b.count(b[2]) == 3 and len(C.expected(b[2])) == 511 - 2  # first rows of tiles 0 and 1 removed
    q3 = C.expected(C.QUOTED3)
    unq = C.expected(C.Q(C.QUOTED3[0]))
    assert C.QUOTED3[2] == 2 and len(C.QUOTED3[0]) == 3 and 0 < len(q3) < len(unq)
    sel = C.urls(C.SEL)
    assert len(sel) == 100 and _urls(C.expected(C.SEL2)) == sel and _urls(C.expected(C.SEL1)) == sel
    stored = C.universe()[0][C.prefix(C.N)]
    assert (C.expected(C.SEL1) == stored[C.SEL]).all()  # a single list under a selection: as stored
    assert not C.expected(C.SEL2)[:, 39].any()
    assert all(len(C.expected(q)) > 0 for q in b)


def test_random_sweep_covers_its_shapes():
    qs = C.sweep_queries()
    assert len(qs) == 64
    assert {len(set(q[0])) for q in qs} >= {1, 2, 3} and {len(q[1]) for q in qs} == {0, 1}
    lens = [len(C.expected(q, "tiny")) for q in qs]
    assert sum(1 for n in lens if n == 0) < 32 and max(lens) > LR_TILE
