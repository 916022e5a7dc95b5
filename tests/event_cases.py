"""Directed inputs of the search-event path (k_event_add and what surrounds it): a helper, no tests.

A Case is a named script of steps over one event:
    ("add", rows, local)               an arrival the event applies (rows may be empty)
    ("bad", rows, local, expected_rc)  an arrival the library must reject; the oracle never sees it
    ("pull", n, skip_double_dom)       pullOneRWI n times
with the stack bound k, profile fields, QueryFilter kwargs and `facts`: what the case claims about
itself.  tests/test_event_cases_ref.py checks the facts on the literal oracle alone (so an input
cannot drift away from the point it was built for), tests/test_gpu_event_arrivals.py runs every
script through the library and compares with run_oracle() after every step.  Everything is built
with numpy and java_literal and is the same on every run.

The points the groups are aimed at (constants of yrwi_internal.h / k_event_add):
  EV_CH = 1024 rows a chunk, EV_THREADS = 256 (4 rows a thread), 64-lane rounds of the
  max-distance fold, the double-buffered stack merged once per chunk, the (epoch << 32 | row)
  word of the doublecheck set.

"Plain" rows (plain_rows) are equal in every feature byte but wordsintext, with hitcount 0 (so
the term frequency is 0 everywhere): under one frozen normalisation (a row with w = 0 and one with
w = W_TOP = 256 in the first arrival, everything later inside) cardinal is base + (w << coeff), a
function of the row alone, and ties are decided by ByteArray.hashCode."""

import functools
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

import adv_rows as ar
import java_literal as jl

NOW = 20741 * 86400000 + 31337
NOW_DAY = 20741
EV_CH = 1024
EV_THREADS = 256
ROUND = 64
E_HASH = -2            # YRWI_E_HASH
E_NULL_LANGUAGE = -7   # YRWI_E_NULL_LANGUAGE
W_TOP = 256
_ALPHA = np.frombuffer(jl.ALPHA, dtype=np.uint8)
EMPTY = np.zeros((0, 40), dtype=np.uint8)


@dataclass
class Case:
    name: str
    steps: List[tuple]
    k: int = 100
    profile: Dict[str, int] = field(default_factory=dict)
    kw: Optional[dict] = None          # QueryFilter kwargs (None: no filter)
    language: str = "en"
    facts: Dict[str, object] = field(default_factory=dict)

    def total_rows(self) -> int:
        return sum(len(s[1]) for s in self.steps if s[0] in ("add", "bad"))


# ------------------------------------------------------------------ rows
def urls(n: int, salt: int, host: Optional[bytes] = None, last: int = ord("A")) -> np.ndarray:
    """(n, 12) distinct well-formed url hashes, distinct between salts (n < 2^20): characters 0..5
    are a bijective mix of salt << 20 | i, 6..10 another mix (the host), character 11 (the
    dom-length class) is `last`; `host` (6 bytes) replaces characters 6..11."""
    assert n < (1 << 20) and salt < (1 << 16)
    i = np.arange(n, dtype=np.int64) + (salt << 20)
    a = (i * 2654435761) & ((1 << 36) - 1)
    b = (i * 40503 + 977) & ((1 << 30) - 1)
    out = np.empty((n, 12), dtype=np.uint8)
    for j in range(6):
        out[:, j] = _ALPHA[(a >> (6 * (5 - j))) & 63]
    for j in range(5):
        out[:, 6 + j] = _ALPHA[(b >> (6 * (4 - j))) & 63]
    out[:, 11] = last
    if host is not None:
        out[:, 6:12] = np.frombuffer(host, dtype=np.uint8)
    return out


def plain_rows(h: np.ndarray, w=0, **cols) -> np.ndarray:
    """rows under the url hashes h: lastModified 15000, doctype 't', language "en", posintext 1,
    wordsintext w, every other cell 0; cols (column letter = value or array) override"""
    h = np.asarray(h, dtype=np.uint8).reshape(-1, 12)
    r = np.zeros((len(h), 40), dtype=np.uint8)
    r[:, :12] = h
    if len(h) == 0:
        return r
    ar._put(r, "a", 15000)
    r[:, 21] = ord("t")
    r[:, 22:24] = np.frombuffer(b"en", dtype=np.uint8)
    ar._put(r, "t", 1)
    ar._put(r, "w", w)
    for c, v in cols.items():
        if c == "l":
            r[:, 22:24] = np.frombuffer(v, dtype=np.uint8).reshape(-1, 2)
        elif c == "z":
            v = np.broadcast_to(np.asarray(v, dtype=np.int64), (len(r),))
            for j in range(4):  # Bitfield bit p is bit p % 8 of byte p >> 3
                r[:, 29 + j] = (v >> (8 * j)) & 0xFF
        else:
            ar._put(r, c, v)
    return r


def keys(rows) -> List[bytes]:
    return [bytes(x) for x in np.asarray(rows, dtype=np.uint8).reshape(-1, 40)[:, :12]]


def family(f: int) -> np.ndarray:
    """32 well-formed url hashes with one ByteArray.hashCode and one dom-length class: five
    two-character blocks at 0, 2, 4, 6, 8, each (x, y) or (x + 1, y - 31) -- equal 31 x + y --,
    characters 10..11 fixed.  x in A..Y, y in a..y: both variants stay inside the alphabet."""
    base = [(65 + (f * 5 + j * 3) % 25, 97 + (f * 7 + j * 11) % 25) for j in range(5)]
    out = np.empty((32, 12), dtype=np.uint8)
    for m in range(32):
        for j, (x, y) in enumerate(base):
            out[m, 2 * j:2 * j + 2] = (x + 1, y - 31) if (m >> j) & 1 else (x, y)
    out[:, 10:12] = (ord("A") + f % 26, ord("A"))
    return out


def _shuffled(rows: np.ndarray, seed: int) -> np.ndarray:
    return rows[np.random.default_rng(seed).permutation(len(rows))]


def _by_hashcode(h: np.ndarray) -> np.ndarray:
    """url hashes with distinct hashCodes, ascending in hashCode"""
    hc = ar.hashcodes(h)
    _, first = np.unique(hc, return_index=True)
    return h[first]


def spans(salt: int) -> np.ndarray:
    """the two rows that freeze the normalisation of plain rows: w = 0 and w = W_TOP"""
    return plain_rows(urls(2, salt), w=np.array([0, W_TOP]))


# ------------------------------------------------------------------ the fold, restated
def fold_distances(arrivals: List[np.ndarray]) -> List[int]:
    """max.distance() after each arrival, from WordReferenceVars.max (:420-455) restated over two
    numbers: P (the running maximum of posintext) and A (the one position max holds, or None).
    The event's first row is the clone: its stored distance does not count."""
    out, P, A, started = [], 0, None, False

    def dist():
        return abs(P - A) if (A is not None and P > 0) else 0

    for rows in arrivals:
        p = ar.col_values(rows, "t")
        od = ar.col_values(rows, "i")
        for i in range(len(rows)):
            if not started:
                P, started = int(p[i]), True
                continue
            P = max(P, int(p[i]))
            o = int(od[i])
            if o > 0 and o > dist():
                A = P + o
        out.append(dist())
    return out


def new_maxima(arrivals: List[np.ndarray]) -> List[List[int]]:
    """per arrival, the number of new running maxima of posintext in each 64-row round (the
    event's first row sets P and is none)"""
    out, P, started = [], 0, False
    for rows in arrivals:
        p = [int(x) for x in ar.col_values(rows, "t")]
        per = [0] * ((len(p) + ROUND - 1) // ROUND)
        for i, v in enumerate(p):
            if not started:
                P, started = v, True
            elif v > P:
                P = v
                per[i // ROUND] += 1
        out.append(per)
    return out


# ------------------------------------------------------------------ sizes
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3073)


def _dup_rows(n: int) -> List[Tuple[int, ...]]:
    """the groups of rows that share one url (n = 1025: rows 0, 1023 and 1024 are one group)"""
    if n - 1 == EV_CH:
        return [(0, EV_CH - 1, EV_CH)]
    d = [(0, n - 1)] if n > 1 else []
    if n > EV_CH:
        d.append((EV_CH - 1, EV_CH))
    return d


@functools.lru_cache(maxsize=None)
def sizes() -> List[Case]:
    out = []
    for n in SIZES:
        loc = ar.adv_rows(n, 1000 + n, "edge")
        rem = ar.adv_rows(n, 9000 + n, "edge", first_char_min=1)
        for g in _dup_rows(n):   # the same url, other features
            loc[list(g[1:]), :12] = loc[g[0], :12]
            rem[list(g[1:]), :12] = rem[g[0], :12]
        first = _dup_rows(n)[0] if n > 1 else (0,)
        rem[list(first), :12] = loc[n // 2, :12]  # the remote arrival's first duplicate repeats a local url
        for k in (3000, 100):
            out.append(Case(f"n{n}_k{k}", [("add", loc, True), ("add", rem, False)], k=k,
                            facts={"weights": ["coeff_posintext", "coeff_date"], "lengths": [n, n],
                                   "dups": [(0, r) for r in _dup_rows(n)] + [(1, r) for r in _dup_rows(n)],
                                   "repeats": (1, 0, 0, n // 2)}))
    return out


# ------------------------------------------------------------------ fold
FOLD_PROFILE = {"coeff_worddistance": 15}
LEAD_P = 5


def _lead(salt: int) -> np.ndarray:
    """three rows that start the event: P = LEAD_P, a stored distance on the second"""
    return plain_rows(urls(3, salt), w=[3, 9, 6], t=[LEAD_P, 2, LEAD_P], i=[9, 4, 0], c=[1, 2, 3])


def _pos_patterns() -> Dict[str, np.ndarray]:
    P, n = LEAD_P, 130
    i = np.arange(n)

    def single(lane):
        p = np.full(n, P)
        p[lane] = P + 10
        return p

    big = np.full(1100, P)
    big[EV_CH - 1], big[EV_CH] = P + 5, P + 9
    return {"rising": P + 1 + i, "flat": np.full(n, P), "falling": P + 200 - i, "zero": np.zeros(n, dtype=np.int64),
            "lane0": single(0), "lane63": single(63), "lane64": single(64), "second": P + 1 + i // 2,
            "rows1023_1024": big, "step8": P + 1 + np.arange(200) // 8}


def _dist_patterns(p: np.ndarray, P0: int) -> Dict[str, np.ndarray]:
    n = len(p)
    run = np.maximum.accumulate(np.concatenate([[P0], p]))
    start = run[1:] > run[:-1]                  # a new maximum: the first row of a segment
    end = np.concatenate([start[1:], [True]])   # the last row of a segment
    i = np.arange(n)
    return {"mixed": np.where(i % 3 == 0, 0, (i * 7) % 40), "d0": np.zeros(n, dtype=np.int64),
            "d255": np.full(n, 255), "seg_last": np.where(end, 1 + i % 200, 0),
            "seg_first": np.where(start | (i == 0), 1 + i % 200, 0)}


def _fold_case(name: str, arrivals: List[np.ndarray], extra: Optional[dict] = None) -> Case:
    facts = {"weights": ["coeff_worddistance"], "newmax": new_maxima(arrivals), "distance": fold_distances(arrivals)}
    facts.update(extra or {})
    return Case("fold_" + name, [("add", a, j == 0) for j, a in enumerate(arrivals)], k=3000, profile=FOLD_PROFILE,
                facts=facts)


@functools.lru_cache(maxsize=None)
def fold() -> List[Case]:
    out = []
    salt = 100
    for pn, p in _pos_patterns().items():
        for dn, d in _dist_patterns(p, LEAD_P).items():
            salt += 1
            n = len(p)
            rows = plain_rows(urls(n, salt), w=1 + np.arange(n) % 50, t=p, i=d, c=1 + np.arange(n) % 7)
            extra = {}
            if pn == "rising":
                extra["newmax_is"] = (1, [64, 64, 2])
            if pn == "flat" or pn == "zero":
                extra["newmax_is"] = (1, [0, 0, 0])
            if pn in ("lane0", "lane63", "lane64"):
                extra["newmax_is"] = (1, {"lane0": [1, 0, 0], "lane63": [1, 0, 0], "lane64": [0, 1, 0]}[pn])
            if pn == "second":
                extra["newmax_is"] = (1, [32, 32, 1])
            if pn == "rows1023_1024":
                extra["newmax_is"] = (1, [0] * 15 + [1, 1, 0])
            out.append(_fold_case(f"{pn}_{dn}", [_lead(salt + 500), rows], extra))
            if dn == "mixed":  # the same pattern as the event's first arrival (row 0 is the clone)
                out.append(_fold_case(f"{pn}_{dn}_first", [rows]))
    # a second arrival whose largest posintext is below, equal to and above the event's P.  (Cutting
    # a run of one P into several pieces folds to the same value -- within one P the fold keeps the
    # largest stored distance, or for P = 0 the last one --, so a kernel that started a segment at
    # an equal posintext would still be right; what the fold cases pin is which segment a row
    # belongs to, the carry of P and A across rounds, chunks and arrivals, and index 64.)
    for name, top, cnt in (("below_P", 299, 0), ("equal_P", 300, 0), ("above_P", 301, 1)):
        salt += 1
        a = plain_rows(urls(70, salt), w=1 + np.arange(70) % 9, t=np.minimum(300, 100 + 3 * np.arange(70)),
                       i=(np.arange(70) * 5) % 30, c=2)
        p2 = np.full(70, 50)
        p2[[0, 40, 69]] = top
        b = plain_rows(urls(70, salt + 500), w=1 + np.arange(70) % 11, t=p2, i=(np.arange(70) * 11) % 90, c=3)
        out.append(_fold_case(name, [a, b], {"newmax_is": (1, [cnt, 0]), "P": 300}))
    # adv_rows.distance_fold_rows as an arrival (70 rows: the last row lies in the second round)
    for D in (0, 1, 255, 256, 511, 512, 65534):
        rows = ar.distance_fold_rows(max(D, 1), 70)
        if D == 0:  # the helper starts at 1: the last posintext moves onto the position the fold holds
            ar._put(rows[69:], "t", 256)
        out.append(_fold_case(f"D{D}", [rows], {"distance_is": [D]}))
    return out


# ------------------------------------------------------------------ first row
FIRST_PROFILE = {"coeff_worddistance": 15, "coeff_date": 15}


def _first_rows() -> np.ndarray:
    n = 80
    i = np.arange(n)
    p = 10 + (i * 13) % 300
    p[0] = 5000                                  # the clone holds the largest posintext,
    d = (i * 7) % 60
    d[0] = 200                                   # a stored distance (the clone drops it)
    a = 15000 + (i * 37) % 4000
    a[0] = NOW_DAY + 500                         # and a date in the future (the clone clamps it)
    return plain_rows(urls(n, 300), w=1 + i % 40, t=p, i=d, a=a, c=1 + i % 5)


@functools.lru_cache(maxsize=None)
def first_row() -> List[Case]:
    rows = _first_rows()
    swapped = rows[[1, 0] + list(range(2, len(rows)))]
    flawed = plain_rows(urls(40, 301), w=60000, t=9000, i=250)
    flawed[11, 3] = ord("*")
    w = ["coeff_worddistance", "coeff_date"]
    return [Case("first_largest", [("add", rows, True)], k=3000, profile=FIRST_PROFILE, facts={"weights": w}),
            Case("first_swapped", [("add", swapped, True)], k=3000, profile=FIRST_PROFILE,
                 facts={"weights": w, "differs_from": "first_largest"}),
            Case("first_after_empty", [("add", EMPTY, True), ("add", rows, True)], k=3000, profile=FIRST_PROFILE,
                 facts={"weights": w, "equals": "first_largest"}),
            Case("first_after_rejected", [("bad", flawed, True, E_HASH), ("add", rows, True)], k=3000,
                 profile=FIRST_PROFILE, facts={"weights": w, "equals": "first_largest", "discriminates": [0]})]


# ------------------------------------------------------------------ stack
STACK_KS = (1, 2, 64, 255, 256, 257, 1024, 3000)


def _full_stack(K: int, salt: int, mid_w) -> Tuple[np.ndarray, np.ndarray]:
    """-> (first arrival, spare url hashes ascending in hashCode).  The arrival has K + 1 plain
    rows: the top (w = W_TOP, the lowest hashCode of all urls of the case), K - 1 middle rows
    (w = mid_w(i), 101..200) and the bottom (w = 0), which the bound K cuts off again."""
    pool = _by_hashcode(urls(5 * K + 2200, salt))
    assert len(pool) >= 5 * K + 2100
    top, rest = pool[:1], pool[1:]
    mids = rest[0:2 * (K - 1):2]          # every second url: the others alternate with them in hashCode
    arrival = np.concatenate([plain_rows(top, w=W_TOP), plain_rows(mids, w=mid_w(np.arange(len(mids)))),
                              plain_rows(rest[-1:], w=0)])
    perm = np.random.default_rng(salt).permutation(len(arrival))
    spare = np.concatenate([rest[1:2 * (K - 1):2], rest[2 * (K - 1):-1]])
    return arrival[perm], spare


@functools.lru_cache(maxsize=None)
def stack() -> List[Case]:
    out = []
    w = ["coeff_wordsintext"]
    for K in STACK_KS:
        for delta in (-1, 0, 1):  # one arrival that admits K - 1, K, K + 1 distinct classes
            n = K + delta
            h = _by_hashcode(urls(n + 50, 400 + K))[:n]
            rows = _shuffled(plain_rows(h, w=1 + (np.arange(n) * 37) % 200), K)
            out.append(Case(f"K{K}_admits{delta:+d}", [("add", rows, True)], k=K,
                            facts={"weights": w, "classes": {0: n}, "stack_after": {0: min(n, K)}}))
        if K == 1:
            continue
        varied = lambda i: 101 + i % 100  # noqa: E731
        first, spare = _full_stack(K, 500 + K, varied)
        below = _shuffled(plain_rows(spare[:300], w=1 + np.arange(300) % 100), K + 1)
        above = _shuffled(plain_rows(spare[:K + 3], w=W_TOP), K + 2)
        late = plain_rows(spare[:EV_CH + 1], w=1 + np.arange(EV_CH + 1) % 100)
        ar._put(late[EV_CH:], "w", 201)
        full = {"weights": w, "stack_before": (1, K)}
        out.append(Case(f"K{K}_below", [("add", first, True), ("add", below, False)], k=K,
                        facts=dict(full, unchanged=[1])))
        out.append(Case(f"K{K}_above", [("add", first, True), ("add", above, False)], k=K,
                        facts=dict(full, disjoint=[1])))
        out.append(Case(f"K{K}_row1024", [("add", first, True), ("add", late, False)], k=K,
                        facts=dict(full, entered={1: keys(late[EV_CH:])})))
        # every middle row at one score: the stack order is the hashCode order, and the second
        # arrival's urls lie between the stack's one for one
        first, spare = _full_stack(K, 600 + K, lambda i: 150 + 0 * i)
        alt = _shuffled(plain_rows(spare[:K - 1], w=150), K + 3)
        out.append(Case(f"K{K}_alternate", [("add", first, True), ("add", alt, False)], k=K,
                        facts=dict(full, alternates=[1])))
    # K = 1, the best row last: in the first arrival by score, in the second by hashCode at the top score
    pool = _by_hashcode(urls(400, 700))
    a = plain_rows(pool[1:301], w=np.concatenate([[0], 1 + np.arange(298) % 200, [W_TOP]]))
    b = plain_rows(np.concatenate([pool[301:370], pool[:1], pool[399:]]), w=np.concatenate([1 + np.arange(70), [W_TOP]]))
    b[69, 17:19] = (W_TOP >> 8, W_TOP & 255)  # the top score under a lower hashCode than the entry: it stays out
    out.append(Case("K1_best_last", [("add", a, True), ("add", b, False)], k=1,
                    facts={"weights": w, "stack_before": (1, 1), "entered": {0: keys(a[-1:]), 1: keys(b[-1:])}}))
    return out


# ------------------------------------------------------------------ ties
def _singles(n: int, salt: int, lo: int = 1, hi: int = 255) -> np.ndarray:
    h = _by_hashcode(urls(n + 20, salt))[:n]
    return _shuffled(plain_rows(h, w=lo + (np.arange(n) * 29) % (hi - lo + 1)), salt)


@functools.lru_cache(maxsize=None)
def ties() -> List[Case]:
    out = []
    w = ["coeff_wordsintext"]
    fam = family(3)
    # 32 twins in one chunk, among other rows
    rows = np.concatenate([spans(800), _singles(40, 801)])
    rows = np.insert(rows, np.arange(2, 34), plain_rows(fam, w=100), axis=0)
    out.append(Case("twins32_one_chunk", [("add", rows, True)], k=3000,
                    facts={"weights": w, "rejected_twins": {0: 31}, "entered": {0: keys(rows[2:3])}}))
    # twins at rows 1023 and 1024
    rows = np.concatenate([spans(810), _singles(1098, 811)])
    rows[EV_CH - 1] = plain_rows(fam[5:6], w=77)[0]
    rows[EV_CH] = plain_rows(fam[9:10], w=77)[0]
    out.append(Case("twins_rows_1023_1024", [("add", rows, True)], k=3000,
                    facts={"weights": w, "rejected_twins": {0: 1}, "entered": {0: keys(rows[EV_CH - 1:EV_CH])},
                           "stays_out": {0: keys(rows[EV_CH:EV_CH + 1])}}))
    # twins in two arrivals under a frozen normalisation
    a = np.concatenate([spans(820), plain_rows(fam[:16], w=120), _singles(30, 821)])
    b = np.concatenate([_singles(30, 822), plain_rows(fam[16:], w=120)])
    out.append(Case("twins_two_arrivals", [("add", a, True), ("add", b, False)], k=3000,
                    facts={"weights": w, "rejected_twins": {0: 15, 1: 16}, "entered": {0: keys(a[2:3])}}))
    # a twin of the K-th (last) entry arrives at a full stack.  (The merge would copy the entry
    # itself to the very slot a twin let in were written to, and after it: at the last slot a merge
    # without the tie rule is right by accident.  twin_of_second_last is the case that tells.)
    a = np.concatenate([spans(830), plain_rows(_by_hashcode(urls(9, 831))[:6], w=200 + np.arange(6)),
                        plain_rows(fam[:1], w=50)])
    b = plain_rows(fam[1:2], w=50)
    c = np.concatenate([plain_rows(urls(1, 832), w=220), plain_rows(fam[2:3], w=50)])  # a better row and a twin
    out.append(Case("twin_of_kth", [("add", a, True), ("add", b, False), ("add", c, False)], k=8,
                    facts={"weights": w, "stack_before": (1, 8), "last_is": (1, keys(a[-1:])[0]), "unchanged": [1],
                           "rejected_twins": {1: 1, 2: 1}, "entered": {2: keys(c[:1])}}))
    # the same with one entry below the twin's class: a twin let in would shift that entry
    a = np.concatenate([spans(835), plain_rows(_by_hashcode(urls(9, 836))[:5], w=200 + np.arange(5)),
                        plain_rows(fam[:1], w=50), plain_rows(urls(1, 837), w=30)])
    out.append(Case("twin_of_second_last", [("add", a, True), ("add", plain_rows(fam[1:2], w=50), False)], k=8,
                    facts={"weights": w, "stack_before": (1, 8), "last_is": (1, keys(a[-1:])[0]), "unchanged": [1],
                           "rejected_twins": {1: 1}}))
    # a twin of an entry that a pull has removed: the class is free again
    a = np.concatenate([spans(840), plain_rows(fam[:1], w=250), _singles(20, 841, 1, 200)])
    b = plain_rows(fam[1:2], w=250)
    out.append(Case("twin_after_pull", [("add", a, True), ("pull", 2, False), ("add", b, False)], k=100,
                    facts={"weights": w, "pulled": {1: [keys(a[1:2])[0], keys(a[2:3])[0]]}, "entered": {2: keys(b)}}))
    # the url of a stack entry arrives again with a higher score: dropped, the old score stays
    a = np.concatenate([spans(850), _singles(20, 851, 1, 100)])
    b = a[5:6].copy()
    ar._put(b, "w", 200)
    out.append(Case("same_url_higher", [("add", a, True), ("add", b, False)], k=100,
                    facts={"weights": w, "unchanged": [1], "admits": {1: 0}, "would_score_higher": (1, 0)}))
    return out


# ------------------------------------------------------------------ doublecheck / filter / flags
DE = {"language": "de"}


def _lang(passes) -> np.ndarray:
    return np.frombuffer(b"".join(b"de" if p else b"en" for p in passes), dtype=np.uint8).reshape(-1, 2)


def _filler(n: int, salt: int) -> np.ndarray:
    """n rows of distinct urls: two of three are "de" (pass the language filter); flag words walk
    one bit at a time over bits 8..31"""
    i = np.arange(n)
    return plain_rows(urls(n, salt), w=1 + (i * 31) % 250, l=_lang(i % 3 != 0), z=1 << (8 + i % 24),
                      t=1 + i % 20, c=1 + i % 3)


def _is_de(r) -> bool:
    return bytes(r[22:24]) == b"de"


def _stated_sources(arrivals, ok, seeded=()) -> Dict[bytes, Tuple[int, int]]:
    """(arrival, row) of every url of the case, from the case's own rule `ok` (which rows pass its
    filter): the first passing row of a url that is not in the set yet; never passing: (-1, -1)"""
    out = {bytes(u): (0, 0) for u in seeded}
    for a, rows in enumerate(arrivals):
        for i, r in enumerate(rows):
            if ok(r):
                out.setdefault(bytes(r[:12]), (a + 1, i))
    for rows in arrivals:
        for r in rows:
            out.setdefault(bytes(r[:12]), (-1, -1))
    return out


THRICE = {"stride": (5, 5 + EV_THREADS, 5 + 2 * EV_THREADS), "chunk_edge": (EV_CH - 1, EV_CH, EV_CH + 6)}
VARIANTS = {"first_passes": (True, False, True), "second_passes": (False, True, True), "none_passes": (False,) * 3}


@functools.lru_cache(maxsize=None)
def doublecheck() -> List[Case]:
    out = []
    w = ["coeff_wordsintext", "coeff_language"]
    salt = 900
    for ln, at in THRICE.items():
        for vn, passes in VARIANTS.items():
            salt += 1
            rows = _filler(1100, salt)
            u = urls(1, salt + 50)
            rows[list(at)] = plain_rows(np.repeat(u, 3, axis=0), w=[90, 180, 240], l=_lang(passes), z=[1, 2, 4])
            rows[700, :12] = rows[50, :12]  # both pass: the second is dropped uncounted in every variant
            win = [r for r, p in zip(at, passes) if p][:1]
            out.append(Case(f"thrice_{ln}_{vn}", [("add", rows, False)], k=3000, kw=DE,
                            facts={"weights": w, "flag_rule": True,
                                   "sources": {bytes(u[0]): (1, win[0]) if win else (-1, -1)},
                                   "sources_all": _stated_sources([rows], _is_de),
                                   "flagcount_bits": {j: int(not win or at[j] <= win[0]) for j in range(3)}}))
    # a url that fails the filter in arrival 1 and passes in arrival 2
    a, b = _filler(300, 950), _filler(300, 951)
    u = urls(1, 952)
    a[100] = plain_rows(u, w=33, l=_lang([False]), z=1)[0]
    b[[40, 296]] = plain_rows(np.repeat(u, 2, axis=0), w=[66, 99], l=_lang([True, True]), z=[2, 4])
    out.append(Case("fails_then_passes", [("add", a, True), ("add", b, False)], k=3000, kw=DE,
                    facts={"weights": w, "flag_rule": True, "sources": {bytes(u[0]): (2, 40)},
                           "sources_all": _stated_sources([a, b], _is_de),
                           "flagcount_bits": {0: 1, 1: 1, 2: 0}}))
    # urls seeded by the filter that then arrive: dropped uncounted
    rows = _filler(300, 960)
    rows[:, 29:33] |= np.array([1, 0, 0, 0], dtype=np.uint8)  # bit 0 on every row
    seeded = keys(rows[[0, 1, 255, 256, 299]])
    passing = int((rows[:, 22] == ord("d")).sum())
    out.append(Case("seeded_urls_arrive", [("add", rows, False)], k=3000, kw=dict(DE, urlhashes=seeded),
                    facts={"weights": w, "flag_rule": True, "sources": {u: (0, 0) for u in seeded},
                           "sources_all": _stated_sources([rows], _is_de, seeded),
                           "flagcount_bits": {0: 295}, "admits": {0: passing - sum(r[22] == ord("d") for r in
                                                                                 rows[[0, 1, 255, 256, 299]])}}))
    # all 32 flag bits, and none, under a constraint (any of bits 1, 9): rows without flags fail it
    i = np.arange(400)
    z = np.where(i % 2 == 0, 0xFFFFFFFF, np.where(i % 4 == 1, 0xFFFFFFFF & ~0x202, 0))  # all; all but 1, 9; none
    rows = plain_rows(urls(400, 970), w=1 + (i * 17) % 250, z=z, t=1 + i % 9)
    rows[[8, 264, 398], :12] = rows[6, :12]    # a url under all flags (row 6), again at rows 8, 264, 398
    rows[[10, 266], :12] = rows[3, :12]        # a url without flags (row 3, fails), with flags at row 10, again at 266
    out.append(Case("flags_all_and_none", [("add", rows, True)], k=3000, kw={"constraint": b"\x02\x02\0\0"},
                    facts={"weights": w, "flag_rule": True,
                           "sources": {keys(rows[6:7])[0]: (1, 6), keys(rows[3:4])[0]: (1, 10)},
                           "sources_all": _stated_sources([rows], lambda r: bool(r[29] & 2 or r[30] & 2))}))
    return out


# ------------------------------------------------------------------ authority
AUTH_PROFILE = {"coeff_authority": 14}


@functools.lru_cache(maxsize=None)
def authority() -> List[Case]:
    w = ["coeff_authority"]
    i = np.arange(300)
    one = plain_rows(urls(300, 1000, host=b"hostAA"), w=1 + i % 200, t=1 + i % 30, c=1 + i % 4)
    own = plain_rows(urls(300, 1001), w=1 + i % 200, t=1 + i % 30, c=1 + i % 4)
    grow = []
    for j, (nh, no) in enumerate(((10, 60), (40, 30), (100, 1200))):
        rows = np.concatenate([plain_rows(urls(nh, 1010 + j, host=b"growAA"), w=50 + np.arange(nh) % 100),
                               plain_rows(urls(no, 1020 + j), w=1 + np.arange(no) % 250)])
        rows[nh + no // 2:nh + no // 2 + 12, 6:12] = np.frombuffer(b"otherA", dtype=np.uint8)  # 12 a time: the largest at first
        grow.append(_shuffled(rows, 1030 + j))
    return [Case("one_host", [("add", one, True)], k=3000, profile=AUTH_PROFILE,
                 facts={"weights": w, "maxdomcount": [300], "hosts": 1}),
            Case("own_hosts", [("add", own, True)], k=3000, profile=AUTH_PROFILE,
                 facts={"weights": w, "maxdomcount": [1], "hosts": 300}),
            Case("growing_host", [("add", g, j == 0) for j, g in enumerate(grow)], k=3000, profile=AUTH_PROFILE,
                 facts={"weights": w, "maxdomcount": [12, 50, 150], "keeps_scores": True})]


# ------------------------------------------------------------------ rejects
@functools.lru_cache(maxsize=None)
def rejects() -> List[Case]:
    out = []
    good = [ar.adv_rows(90, 1100 + j, "edge") for j in range(3)]
    for kind, rc in (("hash", E_HASH), ("language", E_NULL_LANGUAGE)):
        for pos in ("first", "middle", "last"):
            # the flawed arrival would move every maximum and top the stack; in the middle it is
            # 1,025 rows long and the flaw sits at its last row
            n, at = (EV_CH + 1, EV_CH) if pos == "middle" else (60, 17)
            bad = plain_rows(urls(n, 1110 + len(out)), w=65535, t=65535, i=255, c=255, u=255, z=0xFFFFFFFF)
            if kind == "hash":
                bad[at, 4] = ord("*")
            else:
                bad[at, 22:24] = 0
            steps = [("add", g, j == 0) for j, g in enumerate(good)]
            steps.insert({"first": 0, "middle": 2, "last": 3}[pos], ("bad", bad, False, rc))
            out.append(Case(f"{kind}_{pos}", steps, k=100, profile={"coeff_worddistance": 12},
                            facts={"weights": ["coeff_wordsintext"],
                                   "discriminates": [j for j, s in enumerate(steps) if s[0] == "bad"]}))
    return out


# ------------------------------------------------------------------ pulls
@functools.lru_cache(maxsize=None)
def pulls() -> List[Case]:
    out = []
    w = ["coeff_wordsintext"]
    for m in (10, 11):  # the m best entries are one host's: the poll loop stops at 10
        rows = np.concatenate([spans(1200 + m), plain_rows(urls(m, 1210 + m, host=b"sameAA"), w=255 - np.arange(m)),
                               _singles(40, 1220 + m, 1, 200)])
        rows = rows[[1] + list(range(2, len(rows))) + [0]]  # the top (w = W_TOP, a host of its own) comes first
        out.append(Case(f"one_host_top{m}", [("add", rows, True), ("pull", 1, True), ("pull", 1, True), ("pull", 1, True),
                                             ("pull", 4, True)], k=100,
                        facts={"weights": w, "top_one_host": m, "third_pull_same_host": m == 11}))
    a, b = _singles(20, 1230), _singles(30, 1231)
    out.append(Case("pull_empties_then_arrival", [("add", a, True), ("pull", 50, True), ("add", b, False),
                                                  ("pull", 0, True), ("pull", 3, False), ("pull", 100, True)], k=25,
                    facts={"weights": w, "empty_after": [1, 5], "pulled_count": {1: 20, 3: 0, 4: 3, 5: 22}}))
    return out


GROUPS: Dict[str, Callable[[], List[Case]]] = {
    "sizes": sizes, "fold": fold, "first_row": first_row, "stack": stack, "ties": ties, "doublecheck": doublecheck,
    "authority": authority, "rejects": rejects, "pulls": pulls}


def case(group: str, name: str) -> Case:
    return next(c for c in GROUPS[group]() if c.name == name)


def names(group: str) -> List[str]:
    return [c.name for c in GROUPS[group]()]


# ------------------------------------------------------------------ the oracle, step by step
INFO_FIELDS = ("flagcount", "postings_in", "admitted_local", "admitted_remote", "remote_arrivals", "max_distance",
               "stack_size", "maxdomcount")


def profile_of(c: Case, cls=jl.RankingProfile):
    p = cls()
    for f, v in c.profile.items():
        setattr(p, f, v)
    return p


def _row_list(rows) -> List[bytes]:
    return [bytes(r) for r in np.asarray(rows, dtype=np.uint8).reshape(-1, 40)]


def _snapshot(ref: jl.SearchEventRWI, nin: int) -> dict:
    mx = ref.order.max
    return {"stack": [(h, w, jl.bytearray_hashcode(h)) for h, w in ref.stack()],
            "info": {"flagcount": list(ref.filt.flagcount), "postings_in": nin, "admitted_local": ref.local_available,
                     "admitted_remote": ref.remote_available, "remote_arrivals": ref.remote_peers,
                     "max_distance": mx.distance() if mx is not None else 0, "stack_size": len(ref.q.items),
                     "maxdomcount": ref.order.maxdomcount}}


def run_oracle(c: Case, feed_bad: bool = False):
    """java_literal.SearchEventRWI over the script -> (one record per step, sources, the oracle).  A record
    holds the oracle's stack as (urlhash, score, hashCode), the yrwi_event_info fields, and for a
    pull the pulled (urlhash, score) list.  sources: url -> (arrival, row) of the posting that
    admitted it, arrivals numbered from 1 over the applied, non-empty arrivals; (0, 0) for a url
    the filter seeded.  feed_bad gives the rejected arrivals to the oracle as well (what the
    event would be had they been applied; a JavaNPE on the way is swallowed)."""
    kw = dict(c.kw or {})
    ref = jl.SearchEventRWI(profile_of(c), c.language, NOW, filt=jl.QueryFilter(**kw), maxsize=c.k)
    plain = dict(kw)
    plain.pop("urlhashes", None)
    sources = {bytes(u): (0, 0) for u in kw.get("urlhashes", ())}
    out, nin, epoch = [], 0, 0
    for s in c.steps:
        rec = {"kind": s[0]}
        if s[0] == "add" or (s[0] == "bad" and feed_bad):
            rows = _row_list(s[1])
            before = set(ref.filt.urlhashes)
            try:
                rec["admitted"] = ref.add_rwis(rows, s[2])
            except jl.JavaNPE:
                rec["admitted"] = None
            if rows:
                epoch += 1
                nin += len(rows)
                new = set(ref.filt.urlhashes) - before
                for i, r in enumerate(rows):
                    u = r[:12]
                    if u in new and u not in sources and jl.QueryFilter(**plain).admit(jl.Vars.from_row(r, NOW)):
                        sources[u] = (epoch, i)
        elif s[0] == "pull":
            rec["pulled"] = ref.pull(s[1], s[2])
        rec.update(_snapshot(ref, nin))
        out.append(rec)
    return out, sources, ref


def all_urls(c: Case) -> List[bytes]:
    seen = dict.fromkeys(u for s in c.steps if s[0] in ("add", "bad") for u in keys(s[1]) if jl.wellformed(u))
    seen.update(dict.fromkeys(bytes(u) for u in (c.kw or {}).get("urlhashes", ())))
    return list(seen)
