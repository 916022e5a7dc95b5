"""The directed inputs of the url-reference tests (tests/test_refs_cases_ref.py on the reference,
tests/test_gpu_url_refs.py on the device): named cases of yrwi_url_references.

A case is its lists {term: rows}, the urls and terms of the call, and the numbers it must give, stated
by construction where the case is built (how many references, hit lists, covered lists, found urls): no
case is vacuous, and tests/refs_ref.py is not called here.  The positions a case claims to reach are
positions of the postings flattened in term order, the domain of the streaming path (a wave's step is 64
neighbours, a tile 1024), and of the (list, url) pairs, list-major, the domain of the probe path (a tile
is 256 pairs); both paths scan their tile counts 1024 at a time (SCAN_STEP), so a case that needs the
scan's carry has hits beyond tile 1024.

A plain module: no tests, no import of a test file or of the built library.

names()        the case names, in a fixed order
build(name)    the Case (cached; the arrays are shared and must be left unchanged)"""

import functools

import numpy as np

import split_keys as sk
import update_cases as uc

REF_LDS_MAX = 2048   # YRWI_REF_LDS_MAX
STREAM_TILE = 1024   # postings per tile of the streaming path
PAIR_TILE = 256      # (list, url) pairs per tile of the probe path
SCAN_STEP = 1024     # tile counts k_ref_scan takes per step of its carry
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)
SET_SIZES = (1, 2, REF_LDS_MAX - 1, REF_LDS_MAX, REF_LDS_MAX + 1, 8192)


class Case:
    """lists, urls (as given: unsorted, maybe with duplicates), terms (None: every list), and `expect`: the
    stated numbers (refs, lists_hit, lists_covered, urls_found; lists / postings / urls where the case says)"""

    def __init__(self, name, lists, urls, terms, expect, facts=None):
        self.name, self.lists, self.urls, self.terms, self.expect, self.facts = name, lists, urls, terms, expect, facts or {}


# ------------------------------------------------------------------ hashes and rows
def universe(n, seed, first=None):
    """n distinct url hashes ascending in the 72-bit key, as (n, 12) uint8; first: every hash begins with it
    (universes with different first characters are disjoint)"""
    rng = np.random.default_rng([seed, n])
    idx = rng.integers(0, 64, (n + n // 8 + 8, 12), dtype=np.int64)
    if first is not None:
        idx[:, 0] = first
    h = uc._ALPHA[idx]
    khi, klo = uc.split_keys(h)
    o = np.lexsort((klo, khi))
    h, khi, klo = h[o], khi[o], klo[o]
    keep = np.ones(len(h), dtype=bool)
    keep[1:] = (khi[1:] != khi[:-1]) | (klo[1:] != klo[:-1])
    h = h[keep]
    assert len(h) >= n
    pick = np.sort(rng.choice(len(h), n, replace=False))
    return h[pick]


def rows_of(h, seed):
    return uc.make_rows(h, 1000 + seed % 7, np.random.default_rng([seed, len(h)]))


def blist(a):
    """(n, 12) uint8 -> [bytes]"""
    return [bytes(x) for x in np.asarray(a, dtype=np.uint8).reshape(-1, 12)]


def flat(lists):
    """the non-empty lists in term order and the flattened position of each one's first row"""
    names = sorted((t for t in lists if len(lists[t])), key=uc.key72)
    off = np.concatenate([[0], np.cumsum([len(lists[t]) for t in names])])
    return names, off


def at(lists, g):
    """flattened position g -> (term, row index)"""
    names, off = flat(lists)
    j = int(np.searchsorted(off, g, "right")) - 1
    return names[j], int(g - off[j])


def shuffled(urls, seed, dups=0):
    """the urls in a random order, the first `dups` of them given once more"""
    urls = list(urls)
    rng = np.random.default_rng([seed, len(urls)])
    out = urls + urls[:dups]
    return [out[int(i)] for i in rng.permutation(len(out))]


def _length_lists(seed):
    """one list per LENGTHS entry, every list with url hashes of its own (first character = its number)"""
    return {uc.term(100 + j): rows_of(universe(n, seed + j, first=j), seed + j) for j, n in enumerate(LENGTHS)}


# ------------------------------------------------------------------ the cases
def _edges():
    """hits at the first and last row of every list, at both sides of list positions 64, 256 and 1024, and at
    both sides of the flattened positions 64, 256, 1024 and 2048 and the very first and last posting"""
    lists = _length_lists(11)
    names, off = flat(lists)
    total = int(off[-1])
    assert names == [uc.term(100 + j) for j in range(1, len(LENGTHS))] and total == sum(LENGTHS)
    picks = set()
    for t in names:
        n = len(lists[t])
        picks |= {(t, k) for k in (0, n - 1, 63, 64, 255, 256, 1023, 1024) if k < n}
    for g in (0, 63, 64, 255, 256, 1023, 1024, 2047, 2048, total - 1):
        picks.add(at(lists, g))
    urls = [bytes(lists[t][k, :12]) for t, k in sorted(picks)]
    hit = {t for t, _ in picks}
    covered = [t for t in names if all((t, k) in picks for k in range(len(lists[t])))]
    assert len(hit) == len(names) and covered == [uc.term(101)]  # (the one-row list)
    exp = dict(lists=len(names), postings=total, urls=len(picks), urls_found=len(picks), refs=len(picks),
               lists_hit=len(hit), lists_covered=1)
    return Case("edges", lists, shuffled(urls, 1, dups=3), None, exp)


def _runs():
    """a whole wave (64 neighbours from a flattened multiple of 64), a whole tile (flattened [2048, 3072), which
    a list boundary crosses), every row of two lists (lists_covered) and no row of the others"""
    lists = _length_lists(12)
    names, off = flat(lists)
    picks = {at(lists, g) for g in range(1152, 1216)} | {at(lists, g) for g in range(2048, 3072)}
    assert len({t for t, _ in picks}) == 3  # the wave in one list, the tile over the next two
    full = [uc.term(100 + LENGTHS.index(63)), uc.term(100 + LENGTHS.index(257))]
    for t in full:
        assert not any(p[0] == t for p in picks)
        picks |= {(t, k) for k in range(len(lists[t]))}
    urls = [bytes(lists[t][k, :12]) for t, k in sorted(picks)]
    n = 64 + 1024 + 63 + 257
    assert len(picks) == n
    exp = dict(lists=len(names), postings=int(off[-1]), urls=n, urls_found=n, refs=n, lists_hit=5, lists_covered=2)
    return Case("runs", lists, shuffled(urls, 2), None, exp)


def _one_row_lists():
    """300 one-row lists: many lists share one tile and one wave; list i holds url i"""
    u = universe(300, 13)
    lists = {uc.term(1000 + i): rows_of(u[i:i + 1], 13 + i) for i in range(300)}
    chosen = sorted({0, 1, 62, 63, 64, 65, 127, 128, 255, 256, 257, 298, 299} | set(range(5, 300, 7)))
    urls = blist(u[chosen])
    n = len(chosen)
    exp = dict(lists=300, postings=300, urls=n, urls_found=n, refs=n, lists_hit=n, lists_covered=n)
    return Case("one_row_lists", lists, shuffled(urls, 3, dups=2), None, exp)


def _url_set(n):
    """n distinct urls, half of them (rounded up) drawn from a universe of 10,000 of which list A holds every
    second, B every third and C those numbered 5000..5299; the others are in no list"""
    u = universe(10000, 14, first=3)
    ghosts = universe(8192, 15, first=40)
    lists = {uc.term(2000): rows_of(u[::2], 21), uc.term(2001): rows_of(u[::3], 22), uc.term(2002): rows_of(u[5000:5300], 23)}
    rng = np.random.default_rng([16, n])
    nin = (n + 1) // 2
    idx = np.sort(rng.choice(10000, nin, replace=False))
    per = (idx % 2 == 0).astype(np.int64) + (idx % 3 == 0) + ((idx >= 5000) & (idx < 5300))
    urls = blist(u[idx]) + blist(ghosts[:n - nin])
    a, b, c = int((idx % 2 == 0).sum()), int((idx % 3 == 0).sum()), int(((idx >= 5000) & (idx < 5300)).sum())
    exp = dict(lists=3, postings=5000 + 3334 + 300, urls=n, urls_found=int((per > 0).sum()), refs=int(per.sum()),
               lists_hit=(a > 0) + (b > 0) + (c > 0), lists_covered=int(c == 300))
    return Case("url_set_%d" % n, lists, shuffled(urls, 4, dups=min(n, 5)), None, exp,
                {"counts": dict(zip(blist(u[idx]), (int(p) for p in per)))})


def _near_misses():
    """families of url hashes equal in their first 64 key bits (tests/split_keys.py): list X holds of every
    family the members at even places, list Y every member (both siblings present).  The set: the odd-placed
    members (each a near miss of X and a hit of Y), the first member (a hit of both) and, for every family
    that has one to spare, a sibling no list holds"""
    hs = sk.families(17, 40)
    fams = sk.by_family(hs)
    known = set(hs)
    even = [h for f in fams for h in f[0::2]]
    odd = [h for f in fams for h in f[1::2]]
    first = [f[0] for f in fams]
    ghosts = []
    for f in fams:
        khi = sk.blind_key(f[0])
        ghosts.append(next(sk.join(khi, k) for k in range(256) if sk.join(khi, k) not in known))
    lists = {uc.term(3000): rows_of(sk.hash_array(even), 31), uc.term(3001): rows_of(sk.hash_array(hs), 32)}
    assert uc.ascending(lists[uc.term(3000)]) and uc.ascending(lists[uc.term(3001)])
    urls = odd + first + ghosts
    assert len(set(urls)) == len(urls) and all(len(f) >= 8 for f in fams)
    # a compare of the first 64 key bits alone would find every url of the set in both lists
    assert all(sk.lookup(even, urls, sk.blind_key))
    exp = dict(lists=2, postings=len(even) + len(hs), urls=len(urls), urls_found=len(odd) + len(first),
               refs=len(odd) + 2 * len(first), lists_hit=2, lists_covered=0)
    return Case("near_misses", lists, shuffled(urls, 5, dups=4), None, exp)


def _named(all_lists):
    """lists a..d over one universe of 400 urls (a: all, b: first half, c: second half, d: every fourth); the
    set is urls 0..99; named: a, b, a again and a term nobody has -- against nterms == 0"""
    u = universe(400, 18)
    a, b, c, d = (uc.term(4000 + j) for j in range(4))
    lists = {a: rows_of(u, 41), b: rows_of(u[:200], 42), c: rows_of(u[200:], 43), d: rows_of(u[::4], 44)}
    urls = blist(u[:100])
    if all_lists:
        exp = dict(lists=4, postings=400 + 200 + 200 + 100, urls=100, urls_found=100, refs=100 + 100 + 0 + 25,
                   lists_hit=3, lists_covered=0)
        return Case("named_none", lists, shuffled(urls, 6, dups=2), None, exp)
    exp = dict(lists=2, postings=600, urls=100, urls_found=100, refs=200, lists_hit=2, lists_covered=0)
    return Case("named_some", lists, shuffled(urls, 6, dups=2), [a, b, a, uc.term(4999)], exp)


def _everywhere_nowhere():
    """a url present in every one of 20 lists and a url present in none"""
    u = universe(1001, 19)
    e, rest = u[500], np.delete(u, 500, axis=0)
    ghost = universe(1, 20, first=50)
    lists = {}
    for j in range(20):
        own = rest[50 * j:50 * j + 50]
        h = np.concatenate([own, e[None]])
        khi, klo = uc.split_keys(h)
        lists[uc.term(5000 + j)] = rows_of(h[np.lexsort((klo, khi))], 50 + j)
    urls = [bytes(e), bytes(ghost[0])]
    exp = dict(lists=20, postings=20 * 51, urls=2, urls_found=1, refs=20, lists_hit=20, lists_covered=0)
    return Case("everywhere_nowhere", lists, urls, None, exp, {"counts": {urls[0]: 20, urls[1]: 0}})


def _carry_stream():
    """three lists of 360,000 rows: more than SCAN_STEP tiles of postings, every 1009th posting a reference,
    so the tiles beyond the scan's first step have hits and start at its carry"""
    u = universe(3 * 360000, 21)
    lists = {uc.term(6000 + j): rows_of(u[j::3], 60 + j) for j in range(3)}
    names, off = flat(lists)
    total = int(off[-1])
    tiles = -(-total // STREAM_TILE)
    gs = np.arange(7, total, 1009)
    assert tiles > SCAN_STEP and gs[-1] // STREAM_TILE == tiles - 1 and len(set(gs // STREAM_TILE)) > SCAN_STEP
    j = np.searchsorted(off, gs, "right") - 1
    urls = [bytes(lists[names[a]][g - off[a], :12]) for a, g in zip(j, gs)]
    assert len(set(urls)) == len(urls)  # (the three lists share no url)
    exp = dict(lists=3, postings=total, urls=len(gs), urls_found=len(gs), refs=len(gs), lists_hit=3, lists_covered=0)
    return Case("carry_stream", lists, shuffled(urls, 7), None, exp)


def _carry_probe():
    """600 lists by 500 urls: more than SCAN_STEP tiles of pairs; list i holds url j of a universe of 2000
    where a drawn matrix says so (about 1 in 100), the set is every fourth url"""
    u = universe(2000, 22)
    rng = np.random.default_rng(23)
    m = rng.random((600, 2000)) < 0.01
    m[:, 0] |= ~m.any(axis=1)  # (no empty list)
    lists = {uc.term(7000 + i): rows_of(u[m[i]], 70 + i) for i in range(600)}
    sel = np.arange(0, 2000, 4)
    hits = m[:, sel]
    pairs_tiles = -(-600 * len(sel) // PAIR_TILE)
    hit_tiles = set((np.flatnonzero(hits.ravel()) // PAIR_TILE).tolist())  # (lists in term order = in i)
    assert pairs_tiles > SCAN_STEP and max(hit_tiles) >= SCAN_STEP and len(hit_tiles) > PAIR_TILE
    exp = dict(lists=600, postings=int(m.sum()), urls=500, urls_found=int(hits.any(axis=0).sum()), refs=int(hits.sum()),
               lists_hit=int(hits.any(axis=1).sum()), lists_covered=int((hits.sum(axis=1) == m.sum(axis=1)).sum()))
    return Case("carry_probe", lists, shuffled(blist(u[sel]), 8), None, exp)


def _document():
    """one document against many lists, the common call: 200 lists of about 2000 rows over a universe of 4000
    urls; the url is in the lists a drawn vector says.  facts: 5000 urls (the universe and 1000 more) and one
    list's name, for the tests of the call's shape"""
    u = universe(4000, 24)
    rng = np.random.default_rng(25)
    m = rng.random((200, 4000)) < 0.5
    doc = 1234
    lists = {uc.term(8000 + i): rows_of(u[m[i]], 80 + i) for i in range(200)}
    n = int(m[:, doc].sum())
    assert 50 < n < 150
    exp = dict(lists=200, postings=int(m.sum()), urls=1, urls_found=1, refs=n, lists_hit=n, lists_covered=0)
    many = blist(u) + blist(universe(1000, 26, first=60))
    return Case("document", lists, [bytes(u[doc])], None, exp,
                {"urls5000": many, "refs5000": int(m.sum()), "one_list": uc.term(8000), "one_list_refs": int(m[0, doc])})


_BUILDERS = {"edges": _edges, "runs": _runs, "one_row_lists": _one_row_lists, "near_misses": _near_misses,
             "named_some": lambda: _named(False), "named_none": lambda: _named(True),
             "everywhere_nowhere": _everywhere_nowhere, "carry_stream": _carry_stream, "carry_probe": _carry_probe,
             "document": _document}
_BUILDERS.update({"url_set_%d" % n: functools.partial(_url_set, n) for n in SET_SIZES})


def names():
    return list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def build(name) -> Case:
    c = _BUILDERS[name]()
    assert c.expect["refs"] > 0, name  # no case is vacuous
    for t, l in c.lists.items():  # strictly ascending in the 72-bit key
        khi, klo = uc.split_keys(l)
        assert ((khi[1:] > khi[:-1]) | ((khi[1:] == khi[:-1]) & (klo[1:] > klo[:-1]))).all(), (name, t)
    return c
