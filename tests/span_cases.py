"""The one large index of the span-walk tests (tests/test_span_cases_ref.py on the references,
tests/test_gpu_span_walk.py on the device) and what every maintenance call must give on it.

The streaming passes of yrwi_update.hip (host marking, census, retention, url references) give each of at
most SPAN_BLOCKS workgroups a contiguous span of the flattened postings, whole tiles of SPAN_TILE.  Only
above SPAN_BLOCKS * SPAN_TILE postings does a workgroup walk a second tile, and only then does the state it
carries from tile to tile matter: the list cursor, the per-list sum of a wave, the LDS tables that collect
over a span.  This index holds SPAN_BLOCKS * SPAN_TILE + 1 + 4096 postings, so a span is two tiles.

Every posting is described by arrays (its list, the high and the low 36 bits of its url key -- the low
bits are the host --, its lastModified day), the rows are made from them, and every expectation is computed
from the arrays in vectorised numpy: no reference module is called here.  thin() gives a small corpus of
the same shape on which the references run in seconds.

A plain module: no tests, no import of a test file or of the built library.

corpus()        the Corpus (cached; its arrays are shared and must be left unchanged)
thin(c)         every marked posting and every 64th other one
expect_*(c, .)  what the calls must give"""

import functools

import numpy as np

import update_ref as ur

SPAN_TILE = 1024     # postings a workgroup takes per step
SPAN_BLOCKS = 2048   # the grid cap of the streaming passes
HOST_LDS_MAX = 2048  # YRWI_HOST_LDS_MAX
REF_LDS_MAX = 2048   # YRWI_REF_LDS_MAX
RET_WIN = 8192       # days of a workgroup's LDS histogram window
DAYS = 65536
TOTAL = SPAN_BLOCKS * SPAN_TILE + 1 + 4096
PER = 2 * SPAN_TILE  # the span of a workgroup at TOTAL postings (span_of() says so)

ONE_ROW_LISTS = 300
BIG = 8192           # the list that covers four whole spans
BG_HOSTS = 1500      # hosts of the unmarked postings: 16 neighbours share one, 128 hosts per span
N_H64, N_G = 64, 1985
KEY_BG, KEY_H64, KEY_G, KEY_NOBODY = 0x100000, 0x200000, 0x300000, 0x400000
MIN_DAY, MAX_REFS = 20003, 2
CENSUS_CUT = 10      # min_postings that cuts: the G hosts have one or two postings, the H64 hosts more

_ALPHA = np.frombuffer(ur._B64, dtype=np.uint8)
UPDATE_KEYS = ("terms", "new_terms", "emptied_terms", "added", "replaced", "dropped", "removed")


# ------------------------------------------------------------------ the span, as the kernels compute it
def span_of(total):
    """-> (workgroups launched, postings per workgroup)"""
    grid = min(-(-total // SPAN_TILE), SPAN_BLOCKS)
    per = -(-(-(-total // grid)) // SPAN_TILE) * SPAN_TILE
    return grid, per


# ------------------------------------------------------------------ hashes and rows
def chars6(v):
    """36-bit values -> (n, 6) uint8 Base64 characters, ascending as the values"""
    v = np.asarray(v, dtype=np.int64)
    return np.stack([_ALPHA[(v >> (6 * (5 - j))) & 63] for j in range(6)], axis=1)


def host_hashes(keys):
    return [bytes(h) for h in chars6(keys)]


def url_hashes(hi, host):
    return [bytes(h) for h in np.concatenate([chars6(hi), chars6(host)], axis=1)]


def term(j):
    return b"-s" + bytes(chars6([0])[0, :4]) + bytes(chars6([j])[0])


def _rows(hi, host, day, seed):
    """valid rows: the url hash and the day set, a non-empty language, every other byte drawn"""
    r = np.random.default_rng(seed).integers(0, 256, (len(hi), 40), dtype=np.uint8)
    r[:, 0:6], r[:, 6:12] = chars6(hi), chars6(host)
    r[:, 12], r[:, 13] = day >> 8, day & 255
    nolang = (r[:, 22] == 0) & (r[:, 23] == 0)
    r[nolang, 22:24] = np.frombuffer(b"en", dtype=np.uint8)
    return r


class Corpus:
    """terms[j]: list j's term hash (ascending: the flattened order is the term order and the order
    named); off[j]: its first posting; per posting: lst, hi, host, day, rows; marked / marked2: the
    postings of the H64 hosts and of the G hosts; facts: what the layout claims"""

    def __init__(self, terms, off, hi, host, day, rows, marked, marked2, facts):
        self.terms, self.off, self.hi, self.host, self.day, self.rows = terms, off, hi, host, day, rows
        self.marked, self.marked2, self.facts = marked, marked2, facts
        self.n = int(off[-1])
        self.lens = np.diff(off)
        self.lst = np.repeat(np.arange(len(terms)), self.lens)
        self.key = (hi << 36) | host  # the 72-bit key's order in 60 bits

    def lists(self):
        return {t: self.rows[self.off[j]:self.off[j + 1]] for j, t in enumerate(self.terms)}


def _lengths():
    """the list lengths, in flattened order, and the places the layout is about"""
    rng = np.random.default_rng(20260)
    lens = [BIG, SPAN_TILE]                    # [0, 8192): four whole spans; [8192, 9216): ends on span 4's tile edge
    edge = 5 * PER + SPAN_TILE                 # the tile edge inside span 5
    lens.append(edge - ONE_ROW_LISTS // 2 - sum(lens))
    one_row_first = len(lens)
    lens += [1] * ONE_ROW_LISTS                # 150 on each side of that edge
    lens.append(6 * PER - sum(lens))           # ends on the edge of span 6
    run_first = len(lens)
    while sum(lens) < 6 * PER + SPAN_TILE:     # lists of 1, 2, 3, 1, ... rows fill span 6's first tile
        lens.append(min((len(lens) - run_first) % 3 + 1, 6 * PER + SPAN_TILE - sum(lens)))
    run_end = len(lens)
    left = TOTAL - sum(lens)
    while left >= 11000:                       # fillers of 3000 .. 5000 rows up to the total
        lens.append(int(rng.integers(3000, 5001)))
        left -= lens[-1]
    parts = 2 if left <= 10000 else 3
    lens += [left // parts + (i < left % parts) for i in range(parts)]
    return np.array(lens, dtype=np.int64), dict(one_row=(one_row_first, one_row_first + ONE_ROW_LISTS),
                                                 run=(run_first, run_end), filler_first=run_end, edge=edge)


@functools.lru_cache(maxsize=None)
def corpus() -> Corpus:
    lens, f = _lengths()
    assert lens.sum() == TOTAL and len(lens) < 2048 and (lens[f["filler_first"]:] >= 3000).all()
    assert (lens[f["filler_first"]:] <= 5000).all()
    off = np.concatenate([[0], np.cumsum(lens)])
    nl = len(lens)
    g = np.arange(TOTAL, dtype=np.int64)
    lst = np.repeat(np.arange(nl), lens)
    k = g - off[lst]
    hi = k * 2048 + lst  # ascending in a list, unique in the index, not ascending across lists
    # ---- three quiet spans: each inside one filler list, no list begins in them
    starts = np.zeros(TOTAL // PER + 1, dtype=bool)
    starts[off[:-1] // PER] = True
    quiet = [int(w) for w in np.flatnonzero(~starts[:TOTAL // PER]) if w >= 8][:3]
    w_second, w_first, w_both = quiet
    in_quiet = np.isin(g // PER, quiet)
    # ---- marked: the postings of the H64 hosts and of every url set
    marked = np.zeros(TOTAL, dtype=bool)
    marked[off[:-1][lens >= 4]] = True                       # the first row of every list of 4 rows or more
    marked[off[f["one_row"][0]]:off[f["one_row"][1]]] = True  # every one-row list
    run = np.arange(f["run"][0], f["run"][1])
    marked[off[run[::3] + 1] - 1] = True                     # the last row of every third list of the run
    marked[np.arange(1000, BIG, 1000)] = True                # the big list: hits in many tiles of four spans
    marked[w_second * PER + SPAN_TILE + np.array([0, 63, 64, 500, 1023])] = True  # hits only in the second tile
    marked[w_first * PER + np.array([1, 255, 256, 1023])] = True                  # only in the first
    marked[w_both * PER + np.array([10, 700, 1023, 1024, 1500, 2047])] = True     # in both, of one list
    # ---- marked2: the postings of the G hosts: every 1021st elsewhere, none in the quiet spans
    marked2 = (g % 1021 == 5) & ~marked & ~in_quiet & (lens[lst] >= 4)
    host = KEY_BG + (g // 16) % BG_HOSTS
    m, m2 = np.flatnonzero(marked), np.flatnonzero(marked2)
    host[m] = KEY_H64 + np.arange(len(m)) % N_H64
    host[m2] = KEY_G + np.arange(len(m2)) % N_G
    assert len(m2) >= N_G
    # ---- days: a span's second tile lies 5000 days after its first, outside any window around the first
    day = 20000 + (g // SPAN_TILE) % 2 * 5000 + g % 7
    facts = dict(f, w_second=w_second, w_first=w_first, w_both=w_both)
    return Corpus([term(j) for j in range(nl)], off, hi, host, day, _rows(hi, host, day, 7), marked, marked2, facts)


def thin(c: Corpus) -> Corpus:
    """every marked posting and every 64th other one; a list left without a posting is dropped"""
    keep = c.marked | c.marked2 | (np.arange(c.n) % 64 == 0)
    lens = np.bincount(c.lst[keep], minlength=len(c.terms))
    have = lens > 0
    off = np.concatenate([[0], np.cumsum(lens[have])])
    return Corpus([t for t, h in zip(c.terms, have) if h], off, c.hi[keep], c.host[keep], c.day[keep], c.rows[keep],
                  c.marked[keep], c.marked2[keep], {})


# ------------------------------------------------------------------ the arguments of the calls
def host_set(n):
    """64: the H64 hosts (searched in LDS); 2049: they and the G hosts (one more than LDS holds, searched
    in global memory); as keys, given unsorted, the first one twice"""
    assert n in (N_H64, N_H64 + N_G)
    keys = np.concatenate([KEY_H64 + np.arange(N_H64), KEY_G + np.arange(N_G if n > N_H64 else 0)])
    keys = keys[np.random.default_rng(n).permutation(len(keys))]
    return np.concatenate([keys, keys[:1]])


def host_set_bytes(n):
    return host_hashes(host_set(n))


def url_set(c: Corpus, n):
    """n distinct urls as keys (hi, host): every marked posting's, marked2 postings' up to n - 8, and 8 no
    list holds; given unsorted, the first three twice"""
    m, m2 = np.flatnonzero(c.marked), np.flatnonzero(c.marked2)
    pos = np.concatenate([m, m2[:n - 8 - len(m)]])
    assert len(pos) == n - 8
    hi = np.concatenate([c.hi[pos], (1 << 30) + np.arange(8)])
    host = np.concatenate([c.host[pos], np.full(8, KEY_NOBODY)])
    o = np.random.default_rng(n).permutation(n)
    o = np.concatenate([o, o[:3]])
    return hi[o], host[o]


# ------------------------------------------------------------------ expectations, from the arrays
def _split(c: Corpus, keep):
    """-> ({term: the list's kept rows}, the update statistics of removing the others)"""
    left = np.bincount(c.lst[keep], minlength=len(c.terms))
    lost = c.lens - left
    kept = c.rows[keep]
    o = np.concatenate([[0], np.cumsum(left)])
    lists = {t: kept[o[j]:o[j + 1]] for j, t in enumerate(c.terms) if left[j]}
    st = dict.fromkeys(UPDATE_KEYS, 0)
    st.update(terms=int((lost > 0).sum()), emptied_terms=int(((lost > 0) & (left == 0)).sum()), removed=int(lost.sum()))
    return lists, st


def expect_count_hosts(c: Corpus, keys):
    """-> (postings of keys[i], selected lists with a posting of any of them)"""
    u, n = np.unique(c.host, return_counts=True)
    at = np.minimum(np.searchsorted(u, keys), len(u) - 1)
    counts = np.where(u[at] == keys, n[at], 0)
    hit = np.isin(c.host, keys)
    return [int(x) for x in counts], len(np.unique(c.lst[hit])), hit


def expect_remove_hosts(c: Corpus, keys):
    return _split(c, ~np.isin(c.host, keys))


def expect_census(c: Corpus, order, min_postings):
    u, n = np.unique(c.host, return_counts=True)
    keep = n >= max(min_postings, 1)
    st = dict(lists=len(c.terms), postings=c.n, hosts=len(u), hosts_passing=int(keep.sum()))
    u, n = u[keep], n[keep]
    if order == "count":
        o = np.lexsort((u, -n))
        u, n = u[o], n[o]
    return host_hashes(u), [int(x) for x in n], st


def census_bypass_floor(c: Corpus, slots):
    """the least number of postings that go past a workgroup's LDS table of `slots` hosts, whatever the order
    they arrive in: a span with D hosts leaves D - slots of them without a slot, its smallest at best"""
    _, per = span_of(c.n)
    pair, n = np.unique((np.arange(c.n) // per << 36) | c.host, return_counts=True)
    span = pair >> 36
    o = np.lexsort((n, span))
    span, n = span[o], n[o]
    hosts = np.bincount(span)
    rank = np.arange(len(span)) - (np.cumsum(hosts) - hosts)[span]
    return int(n[rank < hosts[span] - slots].sum())


def expect_hist_bypass(c: Corpus):
    """postings whose day lies outside the window around the day of their span's first posting"""
    _, per = span_of(c.n)
    first = c.day[np.arange(c.n) // per * per]
    wlo = np.clip(first - RET_WIN // 2, 0, DAYS - RET_WIN)
    return int(((c.day < wlo) | (c.day >= wlo + RET_WIN)).sum())


def expect_retention(c: Corpus, min_day, max_refs):
    """-> (lists after retain, update statistics, retention statistics, the day histogram before any rule)"""
    surv = c.day >= min_day
    keep = surv.copy()
    if max_refs > 0:  # of a list's survivors the max_refs newest, equal days in list order
        pos = np.flatnonzero(surv)
        o = pos[np.lexsort((pos, -c.day[pos], c.lst[pos]))]
        first = np.concatenate([[0], np.cumsum(np.bincount(c.lst[pos], minlength=len(c.terms)))])[c.lst[o]]
        keep[o[np.arange(len(o)) - first >= max_refs]] = False
    nsurv = np.bincount(c.lst[surv], minlength=len(c.terms))
    nkeep = np.bincount(c.lst[keep], minlength=len(c.terms))
    age, cap = c.lens - nsurv, nsurv - nkeep
    rs = dict(lists=len(c.terms), postings=c.n, removed_age=int(age.sum()), removed_cap=int(cap.sum()),
              lists_age=int((age > 0).sum()), lists_cap=int((cap > 0).sum()), emptied_terms=int((nsurv == 0).sum()),
              day_min=int(c.day.min()), day_max=int(c.day.max()))
    lists, st = _split(c, keep)
    return lists, st, rs, np.bincount(c.day, minlength=DAYS).astype(np.int64), keep


def expect_refs(c: Corpus, uhi, uhost):
    """-> (counts per url given, statistics, {order: (terms (n, 12), rows (n, 40))})"""
    ukey = (np.asarray(uhi) << 36) | np.asarray(uhost)
    hit = np.isin(c.key, ukey)
    pos = np.flatnonzero(hit)
    found = np.sort(c.key[pos])
    counts = np.searchsorted(found, ukey, "right") - np.searchsorted(found, ukey, "left")
    per_list = np.bincount(c.lst[pos], minlength=len(c.terms))
    st = dict(lists=len(c.terms), postings=c.n, urls=len(np.unique(ukey)), urls_found=len(np.unique(found)),
              refs=len(pos), lists_hit=int((per_list > 0).sum()), lists_covered=int((per_list == c.lens).sum()))
    tarr = np.frombuffer(b"".join(c.terms), dtype=np.uint8).reshape(-1, 12)
    by_url = pos[np.argsort(c.key[pos], kind="stable")]
    return counts.astype(np.int64), st, {"term": (tarr[c.lst[pos]], c.rows[pos]),
                                         "url": (tarr[c.lst[by_url]], c.rows[by_url])}, hit
