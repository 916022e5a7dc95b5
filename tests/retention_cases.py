"""The directed inputs of the retention tests (tests/test_retention_ref.py on the reference,
tests/test_gpu_retention.py on the device): hand-made lists over template rows, with their lastModified
days set, and the facts each case claims, as functions that assert them on a (before, after) pair."""

import numpy as np

import retention_ref as rr
import update_ref as ur

B64 = ur._B64

# the re-dated corpus: eight days, the newest the most frequent, within a band narrower than half an LDS
# window of the histogram pass, so that the histogram of the corpus takes the LDS path alone
CORPUS_DAYS = (20700, 20650, 20500, 20200, 19800, 19000, 18000, 17500)
CORPUS_WEIGHTS = tuple(1.0 / (1 + j) for j in range(len(CORPUS_DAYS)))


def enc(i, width):
    out = bytearray()
    for _ in range(width):
        out.append(B64[i & 63])
        i >>= 6
    return bytes(reversed(out))


def term(i):
    return b"-r" + enc(i, 10)


def url(i):
    """url i of the hand-made lists: the lists share their urls, so joins of two of them are not empty"""
    return enc(7 * i, 6) + b"r3t41n"


def make(base, n, days, start=0):
    """n hand-made rows: rows of `base` as templates, urls url(0 .. n-1), the days set"""
    r = base[(start + 13 * np.arange(n)) % len(base)].copy()
    for i in range(n):
        r[i, :12] = np.frombuffer(url(i), dtype=np.uint8)
    return rr.set_days(r, days)


# ------------------------------------------------------------------ edges
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)
PATTERNS = {
    "all_equal": lambda i, n: 20000,
    "ascending": lambda i, n: 1000 + i,
    "descending": lambda i, n: 3000 - i,
    "alternating": lambda i, n: 20000 + i % 2,
    "old_first": lambda i, n: 100 if i == 0 else 20000,
    "old_last": lambda i, n: 100 if i == n - 1 else 20000,
    "extremes": lambda i, n: 65535 if i % 2 else 0,
    "straddle": lambda i, n: 0x4EFE + i % 4,  # ..FE, ..FF | ..00, ..01: the cut day on either side of a high-byte edge
}
# every cap of 1, n - 1, n, n + 1 over the sizes (0 is "no cap")
EDGE_CAPS = tuple(sorted({1} | {n + d for n in SIZES for d in (-1, 0, 1)} - {0}))


def edge_lists(base):
    """-> ({term: rows}, {term: (size, pattern)}): every size under every pattern"""
    lists, what = {}, {}
    for k, (n, (name, day)) in enumerate((n, p) for n in SIZES for p in PATTERNS.items()):
        lists[term(k)] = make(base, n, [day(i, n) for i in range(n)], start=k)
        what[term(k)] = (n, name)
    return lists, what


def check_edges(lists, what, new, cap):
    """the claims of the edge case for one cap, on the lists before and after"""
    for t, (n, name) in what.items():
        got = new.get(t)
        if cap >= n:  # caps n and n + 1 (and every larger one) remove nothing
            assert got is lists[t], (name, n, cap)
            continue
        assert len(got) == cap, (name, n, cap)
        if cap == n - 1:  # exactly the oldest row goes; among equal oldest rows the last in url order
            a = rr.days_of(lists[t])
            gone = max(i for i in range(n) if a[i] == a.min())
            assert got.tobytes() == np.delete(lists[t], gone, axis=0).tobytes(), (name, n)
        if cap == 1:  # the newest row stays; among equal newest rows the first in url order
            a = rr.days_of(lists[t])
            assert got.tobytes() == lists[t][int(np.argmax(a))][None].tobytes(), (name, n)


# ------------------------------------------------------------------ ties at the cut
TIE_CAPS = (63, 64, 65, 255, 256, 257, 1024)


def tie_lists(base):
    """two lists of 1025 rows of one single day each"""
    return {term(100): make(base, 1025, [20000] * 1025, start=3), term(101): make(base, 1025, [7] * 1025, start=5)}


SCATTER_ENDS = (63, 64, 255, 256, 1023, 1024)
SCATTER_N, SCATTER_CAP = 1100, 600
NEWER, CUT, OLDER = 9000, 5000, 1000


def scatter_lists(base):
    """One list of SCATTER_N rows per end position P: its cut-day rows (day CUT) are scattered, and the
    last of them that the quota of cap SCATTER_CAP admits sits at position P of the list -- of the chunk,
    when the list is a chunk of its own (YRWI_RM_CHUNK below its length).  -> ({term: rows}, {term: P})"""
    lists, ends = {}, {}
    for k, P in enumerate(SCATTER_ENDS):
        tie = {p for p in range(SCATTER_N) if p % 5 in (1, 2) or p == P}
        q = sum(1 for p in tie if p <= P)
        free = [p for p in range(SCATTER_N) if p not in tie]
        m = SCATTER_CAP - q  # cap = newer rows + quota; the newer rows are spread over the whole list
        newer = {free[i * len(free) // m] for i in range(m)}
        assert len(newer) == m > 0 and q < len(tie)
        days = [CUT if p in tie else NEWER if p in newer else OLDER for p in range(SCATTER_N)]
        lists[term(200 + k)] = make(base, SCATTER_N, days, start=7 * k)
        ends[term(200 + k)] = P
    return lists, ends


def check_scatter(lists, ends, new):
    for t, P in ends.items():
        a, kept = rr.days_of(lists[t]), {bytes(r[:12]) for r in new[t]}
        at = [i for i in range(len(a)) if a[i] == CUT and bytes(lists[t][i, :12]) in kept]
        assert len(new[t]) == SCATTER_CAP and max(at) == P, (P, max(at))
        assert all(bytes(lists[t][i, :12]) in kept for i in range(P) if a[i] >= CUT)  # nothing kept is skipped
        assert not any(bytes(lists[t][i, :12]) in kept for i in range(P + 1, len(a)) if a[i] <= CUT)


# ------------------------------------------------------------------ age meets cap
AGE_MIN_DAY, AGE_CAP = 200, 60


def age_cap_lists(base):
    """exact: the age rule leaves AGE_CAP rows; plus_one: AGE_CAP + 1; emptied: none"""
    mix = lambda new, old: [100 if i % 7 == 3 and i // 7 < old else 20000 + i % 3 for i in range(new + old)]
    exact, plus = mix(AGE_CAP, 8), mix(AGE_CAP + 1, 8)
    assert sum(d >= AGE_MIN_DAY for d in exact) == AGE_CAP and sum(d >= AGE_MIN_DAY for d in plus) == AGE_CAP + 1
    return {term(300): make(base, len(exact), exact, start=1), term(301): make(base, len(plus), plus, start=2),
            term(302): make(base, 40, [150 - i for i in range(40)], start=3)}


# ------------------------------------------------------------------ many small lists
def small_lists(base, count):
    """`count` lists of 1-3 rows, days 100 (old) and 20000 .. 20002"""
    lists = {}
    for k in range(count):
        n = 1 + k % 3
        lists[term(1000 + k)] = make(base, n, [(100, 20000, 20001, 20002, 20000)[(k + i) % 5] for i in range(n)], start=k)
    return lists


# ------------------------------------------------------------------ hot list
HOT_N, HOT_CAP = 20000, 5000


def hot_list(base):
    """20,000 rows over three days in turn: the cap of 5,000 cuts inside the newest day's 6,666 rows"""
    return make(base, HOT_N, [20000 + i % 3 for i in range(HOT_N)], start=11)


# ------------------------------------------------------------------ histogram paths
def band_lists(base):
    """days within a band of 3,000: inside every workgroup's LDS window"""
    return {term(400 + k): make(base, 700, [18000 + (37 * i + 501 * k) % 3000 for i in range(700)], start=k)
            for k in range(4)}


def spread_lists(base):
    """days over 0 .. 65535, both ends included: most of them outside any one window"""
    out = {term(410 + k): make(base, 700, [(9973 * i + 4099 * k) % 65536 for i in range(700)], start=k)
           for k in range(4)}
    out[term(414)] = make(base, 4, [0, 65535, 0, 65535])
    return out
