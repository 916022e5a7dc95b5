"""Directed inputs of the host facet tests (tests/test_facet_cases_ref.py checks them on the CPU
against facets_ref over the oracle, tests/test_gpu_host_facets.py feeds them to the device).  A
plain module: no tests, no import of a test file or of the built library's device side.

Every list is a set of positions of a url universe whose hosts are designed: url i of universe
`tag` is tag + enc(i, 4) + hosts[i], so the urls ascend with i whatever their hosts are, and the
hosts of a container in url order are whatever the case wants (one host, all distinct, ABAB...).
A list over positions P joined with the list over the whole universe is exactly P; an exclusion
list over positions X removes exactly X.  So every case states its facets by construction, from
the host and url arrays alone: Uni.facets(kept positions).

A query is the hashable tuple of term_batch_cases.py: (include, exclude, max_distance, now_ms,
urlselection or None).  A facet is (host, count, smallest url); a case lists, per query, its
facets in ascending host order (None: no designed hosts -- the numpy group-by over the oracle's
rows is the expectation) and the max_hosts values it is asked with."""

import functools
from typing import List, NamedTuple, Tuple

import numpy as np

import adv_rows as A
import facets_ref as R
import index_util as iu
import oracle as orc
import term_batch_cases as C

LR_TILE = C.LR_TILE
NOW, NOWS, INF, ABSENT = C.NOW, C.NOWS, C.INF, C.ABSENT
Q = C.Q

LENGTHS = (1, 255, 256, 257, 512, 513, 1025)   # one host over containers around one, two and four tiles
NDIST = 3 * LR_TILE                             # all-distinct hosts: 768 rows
DIST_MAX_HOSTS = (1, 255, 256, 257, 768, 769, 0)
ONE_HOST = b"0nlyh0"
TIES = ((b"tieAAA", 3), (b"tieBBB", 5), (b"tieCCC", 3), (b"tieDDD", 5), (b"tieEEE", 1), (b"tieFFF", 3))
TIE_MAX_HOSTS = (1, 2, 3, 4, 5, 0)              # 1 cuts the tie of the fives, 3 and 4 the tie of the threes
H_ZERO, H_TOP = b"AAAAAA", b"______"            # the hosts of key 0 and key 2^36 - 1
EXTREMES = ((H_ZERO, 2), (H_TOP, 3), (b"BAAAAA", 1), (b"AAAAAB", 4), (b"_____-", 2), (b"-_____", 1))
NEX = 3 * LR_TILE                               # the exclusion universe: hosts X0 X1 X2 X0 X1 X2 ...
XHOSTS = (b"xh0st0", b"Xh0st1", b"-h0st2")      # (not in host order: X1 < x0 < -2)
ONE_LEFT = 301                                  # the one row of XHOSTS[1] that "all_but_one" keeps
REMOVALS = {
    "whole_host": [i for i in range(NEX) if i % 3 == 1],
    "all_but_one": [i for i in range(NEX) if i % 3 == 1 and i != ONE_LEFT],
    "smallest_url": [0],
    "tile_edges": [0, 255, 256, 511, 512, 767],
}


class Uni:
    """one url universe: hosts[i] is the host of its i-th url"""

    def __init__(self, tag: bytes, hosts):
        assert len(tag) == 2
        self.tag, self.hosts = tag, [bytes(h) for h in hosts]
        self.urls = [tag + iu.enc(i, 4) + h for i, h in enumerate(self.hosts)]
        keys = [R.host_key(u) for u in self.urls]  # (any length: six bits per character)
        assert all(a < b for a, b in zip(keys, keys[1:]))

    def term(self, name: str) -> bytes:
        t = b"FC" + self.tag + name.encode()
        assert len(t) <= 12
        return t + b"_" * (12 - len(t))

    def rows(self, pos, seed) -> np.ndarray:
        r = A.adv_rows(len(pos), seed)
        for k, i in enumerate(pos):
            r[k, :12] = np.frombuffer(self.urls[i], dtype=np.uint8)
        return r

    def facets(self, kept):
        """the facets of the container over the positions `kept`, in ascending host order"""
        by = {}
        for i in sorted(kept):
            h = self.hosts[i]
            if h in by:
                by[h][0] += 1
            else:
                by[h] = [1, self.urls[i]]  # ascending positions: the first is the smallest url
        return [(h, c, u) for h, (c, u) in sorted(by.items(), key=lambda kv: R.host_key(kv[0]))]


class Case(NamedTuple):
    name: str
    queries: Tuple
    facets: Tuple            # per query: its facets in host order, or None (facets_of(query))
    max_hosts: Tuple[int, ...] = (0,)


def _interleaved(counts):
    """hosts round-robin until every host has its count: no two neighbours share a host while
    two hosts are left, so only the sort forms the runs"""
    left, out = [c for _, c in counts], []
    while any(left):
        for j, (h, _) in enumerate(counts):
            if left[j]:
                out.append(h)
                left[j] -= 1
    return out


def _scrambled(i: int) -> bytes:
    """768 distinct hosts whose order is not the url order (an odd multiplier permutes 2^36)"""
    return iu.enc((i * 0x9E3779B1 + 0x2545F491) & ((1 << 36) - 1), 6)


class _Build:
    def __init__(self):
        self.spec = {}    # term -> (universe, positions)
        self.cases = []

    def lst(self, uni: Uni, name: str, pos) -> bytes:
        t = uni.term(name)
        assert t not in self.spec
        self.spec[t] = (uni, tuple(pos))
        return t

    def both(self, uni, pos, name, full, exc=(), removed=()):
        """the container over `pos` as a single stored list and as a two-term join, and its facets"""
        t = uni.term(name) if uni.term(name) in self.spec else self.lst(uni, name, pos)
        f = uni.facets(set(pos) - set(removed))
        return [Q((t,), exc), Q((t, full), exc)], [f, f]

    def case(self, name, queries, facets, max_hosts=(0,)):
        assert len(queries) == len(facets)
        self.cases.append(Case(name, tuple(queries), tuple(None if f is None else tuple(f) for f in facets),
                               tuple(max_hosts)))


@functools.lru_cache(maxsize=None)
def _built() -> _Build:
    b = _Build()
    # ---- one host over containers of every length
    le = Uni(b"le", [ONE_HOST] * max(LENGTHS))
    le_full = b.lst(le, "full", range(max(LENGTHS)))
    qs, fs = [], []
    for n in LENGTHS:
        q, f = b.both(le, range(n), "p%04d" % n, le_full)
        assert f[0] == [(ONE_HOST, n, le.urls[0])]
        qs, fs = qs + q, fs + f
    b.case("lengths", qs, fs)
    # ---- every row its own host
    di = Uni(b"di", [_scrambled(i) for i in range(NDIST)])
    assert len(set(di.hosts)) == NDIST
    q, f = b.both(di, range(NDIST), "all", b.lst(di, "full", range(NDIST)))
    b.case("distinct", q, f, DIST_MAX_HOSTS)
    # ---- hosts alternating row by row
    for tag, hosts, n in ((b"a2", (b"zzalt2", b"AAalt2"), 2 * LR_TILE + 1),
                          (b"a3", (b"mmalt3", b"zzalt3", b"AAalt3"), 3 * LR_TILE + 1)):
        u = Uni(tag, [hosts[i % len(hosts)] for i in range(n)])
        q, f = b.both(u, range(n), "all", b.lst(u, "full", range(n)))
        assert sorted(c for _, c, _ in f[0]) == sorted(len(range(j, n, len(hosts))) for j in range(len(hosts)))
        b.case("alternating_" + tag.decode(), q, f, (0, 1))
    # ---- ties in the count, extreme host keys
    for name, tag, counts, mh in (("ties", b"ti", TIES, TIE_MAX_HOSTS), ("extremes", b"xt", EXTREMES, (0, 2))):
        hosts = _interleaved(counts)
        u = Uni(tag, hosts)
        q, f = b.both(u, range(len(hosts)), "all", b.lst(u, "full", range(len(hosts))))
        assert {h: c for h, c, _ in f[0]} == dict(counts)
        b.case(name, q, f, mh)
    # ---- exclusions
    ex = Uni(b"ex", [XHOSTS[i % 3] for i in range(NEX)])
    ex_full = b.lst(ex, "full", range(NEX))
    b.lst(ex, "all", range(NEX))
    qs, fs = [], []
    for name, pos in REMOVALS.items():
        x = b.lst(ex, "x" + name[:7], pos)
        q, f = b.both(ex, range(NEX), "all", ex_full, (x,), pos)
        qs, fs = qs + q, fs + f
    b.case("exclusions", qs, fs, (0, 2))
    # ---- batches: one host in every query, identical descriptors
    j257, s513 = Q((le.term("p0257"), le_full)), Q((le.term("p0513"),))
    f257, f513, f1 = ([(ONE_HOST, n, le.urls[0])] for n in (257, 513, 1))
    b.case("same_host_batch", [j257, j257, s513, j257, Q((le.term("p0001"),)), s513],
           [f257, f257, f513, f257, f1, f513])
    # ---- empties
    low, high = b.lst(ex, "low", range(100)), b.lst(ex, "high", range(400, 500))
    xall = b.lst(ex, "xall", range(NEX))
    empties = {"absent_include": Q((ex_full, ABSENT)), "empty_join": Q((low, high)),
               "all_excluded": Q((ex.term("all"), ex_full), (xall,))}
    qa, fa = Q((low, ex_full)), ex.facets(range(100))
    qb, fb = Q((high,)), ex.facets(range(400, 500))
    for name, e in empties.items():  # first, in the middle and last
        b.case("empty_" + name, [e, qa, e, qb, e], [[], fa, [], fb, []])
    b.case("all_empties", list(empties.values()) * 2, [[]] * 6)
    qs, fs = [], []
    kinds = list(empties.values())
    pool = [(j257, f257), (qa, fa), (s513, f513), (qb, fb), (Q((le.term("p0001"), le_full)), f1)]
    for i in range(300):
        if i % 7 in (0, 3) or i >= 297:
            qs.append(kinds[i % 3])
            fs.append([])
        else:
            q, f = pool[i % len(pool)]
            qs.append(q)
            fs.append(f)
    b.case("scattered_300", qs, fs, (0, 1))
    # ---- other query shapes: no designed hosts, the group-by over the oracle's rows
    h = C.dense_terms
    shapes = [Q(h((0, 1, 2))), C.QUOTED3, C.SEL2, C.SEL1, C.DENSE_INC2]
    b.case("shapes", shapes, [None] * len(shapes), (0, 10))
    return b


def cases() -> List[Case]:
    return list(_built().cases)


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def lists():
    """{term: rows} of the hand-built lists"""
    return {t: u.rows(pos, 5200 + k) for k, (t, (u, pos)) in enumerate(_built().spec.items())}


@functools.lru_cache(maxsize=None)
def index_dict():
    """what the GPU tests' index holds: the index of term_batch_cases.py and the hand-built lists"""
    d = dict(C.index_dict())
    assert not set(d) & set(lists())
    d.update(lists())
    return d


@functools.lru_cache(maxsize=None)
def rows_of(q) -> np.ndarray:
    """the oracle's joined and excluded container of the query over index_dict()"""
    inc, exc, maxd, now, sel = q
    d = index_dict()
    if sel is not None:
        d = C._restrict(d, inc + exc, sel)
    return orc.term_search(d, list(inc), list(exc), maxd, now)


@functools.lru_cache(maxsize=None)
def facets_of(q):
    """the reference's facets of the query, in ascending host order"""
    return tuple(R.group(rows_of(q)))


def expected(c: Case, i: int, order: str, max_hosts: int):
    """what the call writes for query i of the case"""
    f = c.facets[i] if c.facets[i] is not None else facets_of(c.queries[i])
    return R.ordered(list(f), order, max_hosts)
