"""Inputs shared by test_term_batch_cases_ref.py (CPU: the oracle alone shows that these inputs
have the lengths and removal positions they claim) and test_gpu_term_batch.py (GPU:
yrwi_term_search_batch against the oracle and the per-query yrwi_term_search).

Exact-length containers come from one sorted universe of N urls: a list over the first n
urls joined with the list over all of them has exactly n rows, and an exclude list over
chosen positions removes exactly those rows.  Every list carries its own adversarial cells
(adv_rows: nonzero reserved bytes, so a row as stored differs from its re-encoding).  The
index of the GPU tests holds these lists next to the `dense` preset of event_local_cases.py.

A query is a hashable tuple (include, exclude, max_distance, now_ms, urlselection or None)."""

import functools

import numpy as np

import adv_rows as A
import event_local_cases as E
import oracle as orc
from yacy_search_server_amd import synth

LR_TILE = 256  # csrc/yrwi_internal.h
NOW, NOWS, INF, ABSENT = E.NOW, E.NOWS, E.INF, E.ABSENT
N = 3 * LR_TILE                             # the universe: three tiles
EDGES = (1, 255, 256, 257, 511, 512, 513)   # container lengths around one and two tiles
FULL = b"TSBfull_____"
LOW, HIGH = b"TSBlow______", b"TSBhigh_____"   # urls 0..99 and 400..499: an empty join
XALL = b"TSBxall_____"                          # excludes every url

# name: positions (of the universe, and so of a 768-row container) that an exclusion removes
REMOVALS = {
    "first_of_tile": [0, 256, 512],
    "last_of_tile": [255, 511, 767],
    "middle_tile": list(range(256, 512)),
    "all_but_one": [i for i in range(N) if i != 300],
    "rows_255_256": [255, 256],
}
SEL = list(range(100, 400, 3))  # the url selection: 100 urls, all within the first 513


def prefix(n):
    return b"TSBp%04d____" % n


def xterm(name):
    return b"TSBx%02d______" % list(REMOVALS).index(name)


def Q(inc, exc=(), maxd=INF, now=NOW, sel=None):
    return (tuple(inc), tuple(exc), maxd, now, None if sel is None else tuple(sel))


@functools.lru_cache(maxsize=None)
def universe():
    """{term: rows} of the hand-built lists and the universe's url hashes"""
    uni = A.adv_rows(N, 4100)

    def over(pos, seed):
        r = A.adv_rows(N, seed)
        r[:, :12] = uni[:, :12]
        return r[np.asarray(list(pos), dtype=np.int64)].copy()

    d = {FULL: over(range(N), 4101), LOW: over(range(100), 4102), HIGH: over(range(400, 500), 4103),
         XALL: over(range(N), 4104)}
    for j, n in enumerate(EDGES + (N,)):
        d[prefix(n)] = over(range(n), 4110 + j)
    for j, (name, pos) in enumerate(REMOVALS.items()):
        d[xterm(name)] = over(pos, 4130 + j)
    return d, [bytes(u) for u in uni[:, :12]]


def urls(pos):
    u = universe()[1]
    return [u[i] for i in pos]


def selection():
    """the selected urls and two the index does not hold"""
    return urls(SEL) + [b"AAAAAAAAAAAA", b"AAAAAAAAAAAB"]


@functools.lru_cache(maxsize=None)
def index_dict():
    """what the GPU tests' index holds: the dense preset and the hand-built lists"""
    d = dict(E.corpus("dense")[2])
    assert not set(d) & set(universe()[0])
    d.update(universe()[0])
    return d


def dense_terms(ranks):
    _, idx, _, order = E.corpus("dense")
    return [idx.hashes[order[r]] for r in ranks]


def joined(n, exc=(), now=NOW):
    """a two-term query whose joined container has exactly n rows"""
    return Q((prefix(n), FULL), exc, INF, now)


def single(n, exc=(), now=NOW):
    """a one-term query: the n rows as stored"""
    return Q((prefix(n),), exc, INF, now)


DENSE_INC2 = Q(dense_terms((0, 1)))                    # 6400 joined rows
QUOTED3 = Q(dense_terms((0, 1, 2)), (), 2)             # a three-term quoted query
SEL2 = Q((prefix(513), FULL), (), INF, NOW, selection())
SEL1 = Q((prefix(N),), (), INF, NOW, selection())
EMPTIES = {
    "absent_include": Q((FULL, ABSENT)),
    "empty_join": Q((LOW, HIGH)),
    "all_excluded": Q((prefix(N), FULL), (XALL,)),
}


def _restrict(d, terms, sel):
    """ReferenceContainerCache.get(key, urlselection) for the lists of `terms`: the rows whose
    url hash is selected, in their order; an emptied list is absent to searchConjunction"""
    s = set(sel)
    out = {}
    for h in terms:
        rows = d.get(h)
        if rows is None:
            continue
        r = rows[np.fromiter((bytes(x[:12]) in s for x in rows), dtype=bool, count=len(rows))]
        if len(r):
            out[h] = r
    return out


@functools.lru_cache(maxsize=None)
def expected(q, preset=None):
    """the oracle's joined and excluded container of the query, (m, 40) uint8; preset: a synth
    preset's index instead of index_dict()"""
    inc, exc, maxd, now, sel = q
    d = E.corpus(preset)[2] if preset else index_dict()
    if sel is not None:
        d = _restrict(d, inc + exc, sel)
    return orc.term_search(d, list(inc), list(exc), maxd, now)


# ---------------------------------------------------------------- the batches
def tile_edge_queries():
    return [f(n) for n in EDGES for f in (joined, single)]


def shuffled(qs, seed):
    rng = np.random.default_rng(seed)
    return [qs[i] for i in rng.permutation(len(qs))]


def empties_batch():
    """an empty container first, twice in a row in the middle, and last"""
    e = EMPTIES
    return [e["absent_include"], joined(257), e["empty_join"], e["all_excluded"], single(513), e["absent_include"]]


def removal_queries():
    return [f(N, (xterm(name),)) for name in REMOVALS for f in (joined, single)]


def past_scan_block(mixed):
    """300 descriptors of 257 joined rows: 600 tiles and 300 jobs, the request times alternating;
    mixed: the 6400-row dense container between them"""
    qs = [joined(257, (), NOWS[i % 2]) for i in range(300)]
    return qs[:150] + [DENSE_INC2] + qs[150:] if mixed else qs


def per_job_batch():
    rep = joined(511, (xterm("first_of_tile"),))
    return [joined(513, (), NOWS[0]), joined(513, (), NOWS[1]), rep, QUOTED3, joined(257, (), NOWS[1]), SEL2,
            joined(257, (), NOWS[0]), rep, SEL1, single(255), rep, DENSE_INC2]


@functools.lru_cache(maxsize=None)
def sweep_queries():
    """64 random queries on the tiny preset, 1 to 3 include terms and 0 or 1 exclude terms"""
    cfg, idx, _, _ = E.corpus("tiny")
    drawn = synth.queries(cfg, 64, 1, 3, 1, qseed=4242)  # (the stream gives every query its exclude term)
    return [Q([idx.hashes[t] for t in inc], [idx.hashes[t] for t in exc[:i % 2]])
            for i, (inc, exc) in enumerate(drawn)]
