"""The directed inputs of the index-update tests (tests/test_update_cases_ref.py on the reference,
tests/test_gpu_update_cases.py on the device): named cases of yrwi_add_postings / yrwi_remove_postings.

A case is its starting lists {term: rows} and a script of steps; every step carries the lists and the
seven STAT_KEYS it must leave, computed here by construction (construct_add / construct_remove: one
stable sort of the list's rows and the batch's on the 72-bit key, and masks) -- a second statement of
the rule of include/yrwi.h beside the sequential fold of tests/update_ref.py, which is not called here.
The edges a case claims to reach (a run across sorted positions 255 | 256, keys equal in 64 of 72 bits,
...) are asserted where the case is built, through sorted_order() where they concern the sorted batch.

A plain module: no tests, no import of a test file or of the built library.

names()                  [(case name, policies)], in a fixed order
build(name, policy)      the Case (cached; the arrays are shared and must be left unchanged)
sorted_order(terms, rows)   the device's order of a batch: job by first appearance, 72-bit key, arrival"""

import functools

import numpy as np

B64 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"
_ALPHA = np.frombuffer(B64, dtype=np.uint8)
_RANK = np.full(256, 255, dtype=np.uint8)
_RANK[_ALPHA] = np.arange(64, dtype=np.uint8)

POLICIES = ("replace", "keep", "recent")
STAT_KEYS = ("terms", "new_terms", "emptied_terms", "added", "replaced", "dropped", "removed")
EMPTY = np.zeros((0, 40), np.uint8)
PIECE = 16 << 20  # one pinned staging piece of stage_rows
M36 = (1 << 36) - 1


# ------------------------------------------------------------------ hashes and keys
def enc(i, width):
    out = bytearray()
    for _ in range(width):
        out.append(B64[i & 63])
        i >>= 6
    return bytes(reversed(out))


def term(i):
    return b"-u" + enc(i, 10)


def key72(h):
    k = 0
    for b in bytes(h[:12]):
        k = (k << 6) | int(_RANK[b])
    return k


def hashes(keys):
    """72-bit keys (Python ints) -> (n, 12) uint8 url hashes"""
    ks = [int(k) for k in keys]
    assert all(0 <= k < 1 << 72 for k in ks)
    hi = np.array([k >> 36 for k in ks], dtype=np.int64)
    lo = np.array([k & M36 for k in ks], dtype=np.int64)
    out = np.empty((len(ks), 12), dtype=np.uint8)
    for j in range(6):
        out[:, j] = _ALPHA[(hi >> (6 * (5 - j))) & 63]
        out[:, 6 + j] = _ALPHA[(lo >> (6 * (5 - j))) & 63]
    return out


def split_keys(h):
    """(n, >= 12) uint8 -> (khi, klo) as the device stores a key: its top 64 bits and its low 8"""
    idx = _RANK[np.asarray(h, dtype=np.uint8)[:, :12]].astype(np.uint64)
    assert len(idx) == 0 or idx.max() < 64, "malformed hash"
    khi = np.zeros(len(idx), dtype=np.uint64)
    for j in range(10):
        khi = (khi << np.uint64(6)) | idx[:, j]
    khi = (khi << np.uint64(4)) | (idx[:, 10] >> np.uint64(2))
    klo = ((idx[:, 10] & np.uint64(3)) << np.uint64(6)) | idx[:, 11]
    return khi, klo


def s12(a):
    """(n, >= 12) uint8 -> the hashes as (n,) S12 (no hash holds a NUL)"""
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint8)[:, :12]).view("S12").ravel()


def tarr(terms):
    """terms as an (n, 12) uint8 array"""
    if isinstance(terms, np.ndarray):
        return terms.reshape(-1, 12)
    return np.frombuffer(b"".join(bytes(t) for t in terms), dtype=np.uint8).reshape(-1, 12)


def days_of(rows):
    return (rows[:, 12].astype(np.int64) << 8) | rows[:, 13]


def jobs_of(terms):
    """-> (job of every posting, [term of job j]): jobs numbered by first appearance in the batch"""
    t = s12(tarr(terms))
    uniq, first, inv = np.unique(t, return_index=True, return_inverse=True)
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(uniq))
    names = [None] * len(uniq)
    for u, r in zip(uniq, rank):
        names[r] = bytes(u)
    return rank[inv.ravel()], names


def sorted_order(terms, rows):
    """the batch positions in the device's sort order: job, then the 72-bit url key, then arrival"""
    job, _ = jobs_of(terms)
    khi, klo = split_keys(rows)
    return np.lexsort((np.arange(len(job)), klo, khi, job))


def ascending(rows):
    """strictly ascending in the 72-bit key"""
    khi, klo = split_keys(rows)
    k = [(int(a) << 8) | int(b) for a, b in zip(khi, klo)]
    return all(x < y for x, y in zip(k, k[1:]))


# ------------------------------------------------------------------ rows
def make_rows(hs, lm, rng):
    """valid rows under the hashes hs: lastModified lm (scalar or one per row), a non-empty language,
    every other byte random"""
    hs = np.asarray(hs, dtype=np.uint8).reshape(-1, 12)
    r = rng.integers(0, 256, (len(hs), 40), dtype=np.uint8)
    r[:, :12] = hs
    lm = np.broadcast_to(np.asarray(lm, dtype=np.int64), (len(hs),))
    assert len(hs) == 0 or (0 <= lm.min() and lm.max() <= 65535)
    r[:, 12], r[:, 13] = lm >> 8, lm & 255
    nolang = (r[:, 22] == 0) & (r[:, 23] == 0)
    r[nolang, 22:24] = np.frombuffer(b"en", dtype=np.uint8)
    return r


def _tails(rows):
    """bytes 14..39 of every row as four uint64 columns"""
    t = np.zeros((len(rows), 32), dtype=np.uint8)
    t[:, :26] = rows[:, 14:40]
    return t.view(np.uint64)


# ------------------------------------------------------------------ the rule, by construction
def _candidates(lists, terms, rows):
    """the candidates of every touched (term, url): the list's row, then the batch's rows in batch order,
    as one stable sort.  -> (names, job, src, allrows, order, gstart): `order` sorts the candidates by
    (job, key, list row first, arrival); gstart: the sorted positions that begin a (job, key) group"""
    job, names = jobs_of(terms)
    parts, pj = [], []
    for j, t in enumerate(names):
        l = lists.get(t)
        if l is not None and len(l):
            parts.append(l)
            pj.append(np.full(len(l), j, dtype=np.int64))
    old = np.concatenate(parts) if parts else EMPTY
    allrows = np.concatenate([old, rows])
    cj = np.concatenate(pj + [job]) if pj else job
    src = np.concatenate([np.zeros(len(old), np.int64), np.ones(len(rows), np.int64)])
    khi, klo = split_keys(allrows)
    order = np.lexsort((np.arange(len(cj)), src, klo, khi, cj))  # (stable; arrival = the position)
    sj, sh, sl = cj[order], khi[order], klo[order]
    new = np.ones(len(order), dtype=bool)
    new[1:] = (sj[1:] != sj[:-1]) | (sh[1:] != sh[:-1]) | (sl[1:] != sl[:-1])
    return names, cj, src, allrows, order, np.flatnonzero(new)


def construct_add(lists, terms, rows, policy):
    """-> (lists after the add, the seven stats); `lists` and its arrays are left as they are, and a
    list that no batch row enters is the same object afterwards"""
    assert policy in POLICIES
    rows = np.asarray(rows, dtype=np.uint8).reshape(-1, 40)
    n = len(rows)
    names, cj, src, allrows, order, gstart = _candidates(lists, terms, rows)
    m = len(order)
    gend = np.append(gstart[1:], m) - 1
    if policy == "replace":  # the last candidate
        win = gend
    elif policy == "keep":  # the first: the list's row if there is one
        win = gstart
    else:  # the last of the largest lastModified, the list's row among them
        score = (days_of(allrows[order]) << 32) | np.arange(m, dtype=np.int64)
        win = np.maximum.reduceat(score, gstart) & 0xFFFFFFFF
    wsrc = src[order[win]]
    had = src[order[gstart]] == 0
    gj = cj[order[gstart]]
    nj = len(names)
    added = np.bincount(gj, weights=(wsrc == 1) & ~had, minlength=nj).astype(np.int64)
    replaced = np.bincount(gj, weights=(wsrc == 1) & had, minlength=nj).astype(np.int64)
    out = dict(lists)
    st = dict.fromkeys(STAT_KEYS, 0)
    lo = np.searchsorted(gj, np.arange(nj), "left")
    hi = np.searchsorted(gj, np.arange(nj), "right")
    winners = allrows[order[win]]
    for j in np.flatnonzero(added + replaced):
        out[names[j]] = winners[lo[j]:hi[j]]
        st["terms"] += 1
        st["new_terms"] += names[j] not in lists
    st["added"], st["replaced"] = int(added.sum()), int(replaced.sum())
    st["dropped"] = n - st["added"] - st["replaced"]
    return out, st


def candidates_differ(lists, terms, rows):
    """any two candidates of one (term, url) differ in bytes 14..39: a wrong winner shows in the bytes"""
    names, cj, src, allrows, order, gstart = _candidates(lists, terms, rows)
    gid = np.zeros(len(order), dtype=np.int64)
    gid[gstart] = 1
    gid = np.cumsum(gid)
    t = _tails(allrows[order])
    o = np.lexsort((t[:, 3], t[:, 2], t[:, 1], t[:, 0], gid))
    same = (gid[o][1:] == gid[o][:-1]) & (t[o][1:] == t[o][:-1]).all(axis=1)
    return not same.any()


def construct_remove(lists, urls, names=None):
    """-> (lists after the removal, the seven stats); names=None: every list"""
    gone = np.unique(s12(tarr(urls))) if len(urls) else np.zeros(0, "S12")
    sel = list(lists) if names is None else [t for t in dict.fromkeys(bytes(x) for x in names) if t in lists]
    out = dict(lists)
    st = dict.fromkeys(STAT_KEYS, 0)
    for t in sel:
        hit = np.isin(s12(lists[t]), gone)
        k = int(hit.sum())
        if k == 0:
            continue
        st["removed"] += k
        st["terms"] += 1
        if k == len(hit):
            st["emptied_terms"] += 1
            del out[t]
        else:
            out[t] = lists[t][~hit]
    return out, st


# ------------------------------------------------------------------ cases
class Step:
    """op "add": terms (n, 12), rows, policy; op "remove": urls [bytes], names ([bytes] or None);
    op "error": an add that must fail with rc and change nothing.  lists / stats: what the step leaves"""

    def __init__(self, op, lists, stats, terms=None, rows=None, policy=None, urls=None, names=None, rc=0):
        self.op, self.lists, self.stats = op, lists, stats
        self.terms, self.rows, self.policy, self.urls, self.names, self.rc = terms, rows, policy, urls, names, rc


class Case:
    def __init__(self, name, lists):
        self.name, self.lists, self.steps = name, lists, []
        self.cur = lists
        self.watch = list(lists)  # every term whose list is compared after every step, bystanders included
        self.qterms = None        # the terms of the six queries (default: the first of `watch`)
        self.light = False        # too many lists for a fresh build and queries: sizes and samples instead
        self.sample = []          # light: the terms whose bytes are compared
        self.facts = {}           # what the case claims, for the tests to state once more

    def _see(self, ts):
        seen = set(self.watch)
        for t in ts:
            if t not in seen:
                seen.add(t)
                self.watch.append(t)

    def add(self, terms, rows, policy="replace", differ=True):
        terms = tarr(terms)
        if differ:
            assert candidates_differ(self.cur, terms, rows), self.name
        new, st = construct_add(self.cur, terms, rows, policy)
        self.steps.append(Step("add", new, st, terms=terms, rows=rows, policy=policy))
        if not self.light:
            self._see(jobs_of(terms)[1])
        self.cur = new
        return st

    def remove(self, urls, names=None):
        urls = [bytes(u) for u in urls]
        new, st = construct_remove(self.cur, urls, names)
        self.steps.append(Step("remove", new, st, urls=urls, names=names))
        self._see([t for t in (names or []) if t in self.cur])
        self.cur = new
        return st

    def error(self, terms, rows, policy, rc):
        self.steps.append(Step("error", self.cur, dict.fromkeys(STAT_KEYS, 0), terms=tarr(terms), rows=rows,
                               policy=policy, rc=rc))
        self._see(jobs_of(terms)[1])

    def queries(self):
        """six queries over the case's terms: single, pair, triple with an exclude"""
        t = list(self.qterms or self.watch)
        a, b, c, d = (t[i % len(t)] for i in range(4))
        pair = lambda x, y: [x] + ([y] if y != x else [])
        tri = pair(a, b) + ([c] if c not in (a, b) else [])
        exc = [d] if d not in (a, b, c) else []
        return [([a], []), ([b], []), (pair(a, b), []), (pair(b, c), []), (tri, exc), (tri[::-1], exc)]


_BUILDERS = {}


def _case(name, policies=("replace",)):
    def reg(fn):
        _BUILDERS[name] = (fn, policies)
        return fn
    return reg


def names():
    return [(n, p) for n, (_, p) in _BUILDERS.items()]


@functools.lru_cache(maxsize=None)
def build(name, policy="replace"):
    fn, policies = _BUILDERS[name]
    assert policy in policies, (name, policy)
    c = fn(policy)
    c.name = name
    return c


def _rng(*seed):
    return np.random.default_rng([2024] + [int(s) for s in seed])


def _shuffled(rng, terms, rows):
    """a batch with its postings interleaved"""
    p = rng.permutation(len(rows))
    return tarr(terms)[p], rows[p]


def _batch(rng, parts, lm=None):
    """parts: [(term, keys)] -> (terms, rows), interleaved; lastModified random over a few values (ties)"""
    ts = [t for t, ks in parts for _ in ks]
    ks = [k for _, kk in parts for k in kk]
    days = rng.integers(100, 108, len(ks)) if lm is None else lm
    return _shuffled(rng, ts, make_rows(hashes(ks), days, rng))


# The hand universe.  BASE: character 0 is 'M', the top two bits of character 1 are 0.  Row r of every
# geometry list is R(r): 148 apart, so about four of ten neighbours agree in khi and differ in klo alone
# (as the groups of _universe() in tests/test_gpu_updates.py do); the gap in the middle of a list takes 300 keys.
BASE = key72(b"MAAAAAAAAAAA") + (1 << 30)
LENS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)
BY1, BY2 = term(900), term(901)  # bystanders: lists no step names


def R(r, an):
    return BASE + 148 * r + (1000 if r >= max(1, an // 2) else 0)


def _list(an, rng, lm=None):
    return make_rows(hashes([R(r, an) for r in range(an)]), rng.integers(100, 108, an) if lm is None else lm, rng)


def _bystanders(rng):
    return {BY1: _list(70, rng), BY2: make_rows(hashes([BASE + (1 << 40) + 5 * i for i in range(300)]), 7, rng)}


def near(k, kind, j):
    """neighbour j (1, 2) of key k that differs from it (a) only in character 0, (b) only in the top two
    bits of character 1 -- both: only in khi >> 56 -- or (c) only in klo (character 11, two bits of 10)"""
    if kind == "a":
        return k ^ (j * 5 << 66)
    if kind == "b":
        return k ^ (j << 64)
    return (k & ~0xFF) | ((k + 67 * j) & 0xFF)


def _check_near(k, kind):
    ks = [k, near(k, kind, 1), near(k, kind, 2)]
    assert len(set(ks)) == 3
    if kind == "c":
        assert len({x >> 8 for x in ks}) == 1  # equal in khi
        assert len({hashes([x])[0, :10].tobytes() for x in ks}) == 1
    else:
        assert len({x & ((1 << 64) - 1) for x in ks}) == 1 and len({x >> 64 for x in ks}) == 3  # only khi >> 56
        h = hashes(ks)
        assert len({r[2:].tobytes() for r in h}) == 1
        assert len({r[1:].tobytes() for r in h}) == (1 if kind == "a" else 3) and (kind == "a" or len(set(h[:, 0])) == 1)
    return ks


# ------------------------------------------------------------------ A. add, geometry
def _placement(what, an, k, rng):
    """the url keys one list of `an` rows receives"""
    rows = [R(r, an) for r in range(an)]
    last = rows[-1] if an else BASE
    if what == "front":
        return [BASE - 1000 + 37 * i for i in range(5)]
    if what == "back":
        return [last + 2000 + 37 * i for i in range(5)]
    if what == "every_gap":
        return [x - 74 for x in rows] + [last + 74]
    if what == "one_gap":
        g = rows[max(1, an // 2) - 1] + 149 if an else BASE
        return [g + 3 * i for i in range(300)]
    if what == "on_rows_all":
        return rows
    if what == "on_rows_first":
        return rows[:1]
    if what == "on_rows_last":
        return rows[-1:]
    if what == "on_rows_second":
        return rows[::2]
    assert what == "mixed"
    ks = [BASE - 500, BASE - 463, last + 3000, last + 3037] + [x - 74 for x in rows[::3]] + rows[1::4]
    return ks + [ks[-1], BASE - 500]  # two keys twice


PLACEMENTS = ("front", "back", "every_gap", "one_gap", "on_rows_all", "on_rows_first", "on_rows_last",
              "on_rows_second", "mixed")


def _geometry(what):
    def fn(policy):
        rng = _rng(1, PLACEMENTS.index(what))
        lists = {term(100 + k): _list(an, rng) for k, an in enumerate(LENS) if an}
        c = Case("", {**lists, **_bystanders(rng)})
        parts = [(term(100 + k), _placement(what, an, k, rng)) for k, an in enumerate(LENS)]
        parts = [(t, ks) for t, ks in parts if ks]
        st = c.add(*_batch(rng, parts), policy)
        n = sum(len(ks) for _, ks in parts)
        if what in ("front", "back", "every_gap", "one_gap"):
            assert (st["added"], st["replaced"], st["dropped"]) == (n, 0, 0)
            assert st["new_terms"] == 1 and st["terms"] == len(LENS)
        if what.startswith("on_rows"):  # (the new term has no row to be on)
            assert (st["added"], st["dropped"]) == (0, 0) and st["replaced"] == n and st["terms"] == len(LENS) - 1
        if what == "on_rows_all":  # whole waves of k_upd_old without a destination
            assert all(c.cur[t].tobytes() != lists[t].tobytes() and len(c.cur[t]) == len(lists[t]) for t in lists)
        if what == "mixed":
            assert st["dropped"] == 2 * len(LENS) and st["added"] and st["replaced"]
        c.qterms = [term(100 + k) for k in (8, 6, 3, 1)]
        return c
    return fn


for _w in PLACEMENTS:
    _case("geom_" + _w)(_geometry(_w))

SIX = ("front", "back", "every_gap", "one_gap", "on_rows", "mixed")


@_case("geom_all_54")
def _geom_all(policy):
    """every placement of every length, 54 distinct terms in one call"""
    rng = _rng(2)
    variants = ("on_rows_all", "on_rows_first", "on_rows_last", "on_rows_second")
    lists, parts = {}, []
    for p, what in enumerate(SIX):
        for k, an in enumerate(LENS):
            t = term(200 + 10 * p + k)
            if an:
                lists[t] = _list(an, rng)
            w = variants[k % 4] if what == "on_rows" else what
            ks = _placement(w, an, k, rng) or [BASE]  # (on_rows of the new term: one new key)
            parts.append((t, ks))
    c = Case("", {**lists, **_bystanders(rng)})
    st = c.add(*_batch(rng, parts))
    assert len(parts) == 54 == st["terms"] and st["new_terms"] == 6
    c.qterms = [term(200 + 10 * 2 + 8), term(200 + 10 * 5 + 8), term(200 + 10 * 3 + 6), term(200 + 7)]
    return c


@_case("tiny_lists")
def _tiny_lists(policy):
    """700 lists of one row and three of 64: a list boundary at every lane of the flattened k_upd_old"""
    rng = _rng(3)
    lists, parts = {}, []
    for i in range(703):
        t = term(1000 + i)
        own = BASE + 148 * (i % 50)
        if i < 700:
            lists[t] = make_rows(hashes([own]), 100 + i % 5, rng)
            ks = []
            if i % 2:
                ks.append(own)       # the row replaced
            if i % 4 == 0:
                ks.append(own - 9)   # a key before the row
            if i % 4 == 2:
                ks.append(own + 9)   # a key after it
        else:
            lists[t] = _list(64, rng)
            ks = [R(31, 64) + 5, R(63, 64)]
        parts.append((t, ks))
    assert all(ks for _, ks in parts)  # every list is touched
    c = Case("", {**lists, **_bystanders(rng)})
    st = c.add(*_batch(rng, parts))
    assert st["terms"] == 703 and st["replaced"] == 350 + 3 and st["added"] == 350 + 3 and st["dropped"] == 0
    for i in range(700):
        got, old = c.cur[term(1000 + i)], lists[term(1000 + i)]
        assert len(got) == 1 + (i % 2 == 0)
        if i % 2 == 0:
            assert got[(i % 4 == 0) * 1].tobytes() == old[0].tobytes()
    c.qterms = [term(1000), term(1050), term(1701), term(1002)]
    return c


@_case("unchanged_among_changed", ("keep",))
def _unchanged(policy):
    """keep: every odd job (by first appearance) offers existing keys only and loses everything, every
    even job gains rows; then existing keys only to every job: nothing changes"""
    rng = _rng(4)
    ts = [term(1800 + j) for j in range(40)]
    lists = {t: _list(20 + 7 * j, rng) for j, t in enumerate(ts) if j % 4}  # jobs 0 mod 4: new terms
    c = Case("", {**lists, **_bystanders(rng)})
    parts = []
    for j, t in enumerate(ts):
        an = 20 + 7 * j
        own = [R(r, an) for r in range(an)]
        parts.append((t, own[::3] if j % 2 else [x - 74 for x in own[:6]] + (own[:4] if j % 4 else [])))
    bt, rows = _batch(rng, parts)
    head = tarr(ts)  # job j is ts[j]: every job's first posting stands in front, in turn
    first = [int(np.flatnonzero(s12(bt) == t)[0]) for t in ts]
    rest = np.setdiff1d(np.arange(len(bt)), first)
    bt, rows = np.concatenate([bt[first], bt[rest]]), np.concatenate([rows[first], rows[rest]])
    assert jobs_of(bt)[1] == ts and (bt[:40] == head).all()
    st = c.add(bt, rows, "keep")
    assert st["terms"] == 20 and st["new_terms"] == 10 and st["replaced"] == 0 and st["added"] == 20 * 6
    assert all(c.cur[t] is lists[t] for j, t in enumerate(ts) if j % 2)
    before = c.cur
    bt, rows = _batch(rng, [(t, [key72(r) for r in c.cur[t][::2]]) for t in ts])
    st = c.add(bt, rows, "keep")
    assert st == dict(dict.fromkeys(STAT_KEYS, 0), dropped=len(rows)) and all(c.cur[t] is before[t] for t in before)
    c.qterms = [ts[39], ts[38], ts[37], ts[36]]
    return c


@_case("only_new_terms")
def _only_new(policy):
    """every job is a new term: no old row is placed (atotal == 0)"""
    rng = _rng(5)
    c = Case("", _bystanders(rng))
    parts = [(term(1900 + j), [BASE + 148 * i for i in range(1 + j % 5)] + [BASE]) for j in range(30)]
    st = c.add(*_batch(rng, parts))
    assert st["new_terms"] == st["terms"] == 30 and st["replaced"] == 0 and st["dropped"] == 30
    return c


def _jobs_small(nj):
    def fn(policy):
        """nj jobs of one or two rows; a third of them have a list; a job's two keys differ in the top 8 key
        bits alone (job << 8 | khi >> 56, the second sort's key, orders them)"""
        rng = _rng(6, nj)
        ts = [term(3000 + j) for j in range(nj)]
        own = [BASE, BASE + 148, BASE + 296]
        lists = {t: make_rows(hashes(own), 100, rng) for j, t in enumerate(ts) if j % 3 == 0}
        c = Case("", {**lists, **_bystanders(rng)})
        parts = []
        for j, t in enumerate(ts):
            k = (own[j % 3] if j % 2 else BASE + 74 + j)
            parts.append((t, [near(k, "ab"[j % 2], 1), k] if j % 4 < 2 or nj <= 3 else [k]))
        c.add(*_batch(rng, parts), policy)
        assert len(jobs_of(c.steps[0].terms)[1]) == nj
        jbits = 1
        while (1 << jbits) < nj:
            jbits += 1
        c.facts["jbits"] = jbits
        c.qterms = [ts[0], ts[-1], ts[nj // 2], ts[min(3, nj - 1)]]
        return c
    return fn


for _n in (1, 2, 3, 255, 256, 257):
    _case("jobs_%d" % _n)(_jobs_small(_n))


def _jobs_many(nj):
    def fn(policy):
        """nj jobs of one row each, job i = posting i; all new terms but five lists of three rows"""
        rng = _rng(7, nj)
        at = (0, 255, 256, nj - 2, nj - 1)
        i = np.arange(nj, dtype=np.int64)
        tb = np.empty((nj, 12), dtype=np.uint8)
        tb[:, 0], tb[:, 1] = ord("-"), ord("v")
        for j in range(10):
            tb[:, 2 + j] = _ALPHA[(i >> (6 * (9 - j))) & 63]
        keys = [BASE + 148 * int(x) for x in rng.integers(0, 5000, nj)]
        own = [BASE + 148 * 6000, BASE + 148 * 6001, BASE + 148 * 6002]
        lists = {}
        for n_, j in enumerate(at):
            lists[bytes(tb[j])] = make_rows(hashes(own), 100, rng)
            keys[j] = own[n_ % 3] if n_ % 2 == 0 else own[0] - 74  # on a row, or a new key in front
        rows = make_rows(hashes(keys), 101, rng)
        c = Case("", lists)
        c.light = True
        st = c.add(tb, rows)
        assert (jobs_of(tb)[0] == i).all()
        assert st == dict(terms=nj, new_terms=nj - 5, emptied_terms=0, added=nj - 3, replaced=3, dropped=0, removed=0)
        pick = rng.choice(nj, 512, replace=False)
        c.sample = [bytes(tb[j]) for j in at] + [bytes(tb[j]) for j in pick]
        c.facts["prebuilt"] = [bytes(tb[j]) for j in at]
        c.facts["terms"] = tb
        return c
    return fn


_case("jobs_4097")(_jobs_many(4097))
_case("jobs_65537")(_jobs_many(65537))


def _batch_n(n):
    def fn(policy):
        """n postings, new keys and existing ones, into one list of 300 rows"""
        rng = _rng(8, n)
        t = term(1950)
        c = Case("", {t: _list(300, rng), **_bystanders(rng)})
        own = [R(r, 300) for r in range(300)]
        pool = own[::2] + [x - 74 for x in own] + [own[-1] + 74 * (i + 1) for i in range(600)]
        ks = [pool[int(i)] for i in rng.choice(len(pool), n, replace=False)]
        st = c.add(*_batch(rng, [(t, ks)]))
        assert st["added"] + st["replaced"] == n
        c.qterms = [t, BY1]
        return c
    return fn


for _n in (1, 255, 256, 257, 1025):
    _case("batch_%d" % _n)(_batch_n(_n))


# ------------------------------------------------------------------ B. add, duplicates and policies
LM_PATTERNS = ("ascending", "descending", "all_equal", "max_twice_then_smaller", "max_first", "zero_only",
               "top_among_smaller")


def lm_pattern(name, L):
    """lastModified of a run's copies, in arrival order"""
    i = np.arange(L, dtype=np.int64)
    if name == "ascending":
        return 1000 + i
    if name == "descending":
        return 3000 - i
    if name == "all_equal" or (name == "max_twice_then_smaller" and L < 3):
        return np.full(L, 2000)
    if name == "max_twice_then_smaller":  # ... M ... M, smaller
        v = 500 + i % 7
        v[0], v[L - 2], v[L - 1] = 900, 900, 899
        return v
    if name == "max_first":
        return np.where(i == 0, 4000, 3000 + i % 9)
    if name == "zero_only":
        return np.zeros(L, dtype=np.int64)
    assert name == "top_among_smaller"
    return np.where(i == L // 2, 65535, 60000 + i % 11)


def _own_day(mx, rel):
    """the list's own row below, equal to or above the run's maximum (where the 16 bits allow)"""
    return int(np.clip(mx + {"below": -1, "equal": 0, "above": 1}[rel], 0, 65535))


def _runs_case(plan, seed, policy, fill=200):
    """plan: [(L, pattern, rel)]: a run of L copies of one (term, url) with the pattern's days; rel None:
    the url is new to the list, else the list's own row lies below / equal / above the run's maximum.
    The copies are scattered through the batch among `fill` single postings"""
    rng = _rng(9, seed)
    t, t2 = term(2000), term(2001)
    key = lambda i: BASE + 148 * 3 * i
    own_k, own_d, bk, rid, pats = [BASE - 5000], [50], [], [], []
    for i, (L, pat, rel) in enumerate(plan):
        d = lm_pattern(pat, L)
        if rel is not None:
            own_k.append(key(i))
            own_d.append(_own_day(int(d.max()), rel))
        bk += [key(i)] * L
        rid += [i] * L
        pats.append(d)
    fk = [key(len(plan) + i) for i in range(fill)]
    o = np.argsort(own_k)
    lists = {t: make_rows(hashes([own_k[i] for i in o]), [own_d[i] for i in o], rng), t2: _list(40, rng)}
    c = Case("", {**lists, **_bystanders(rng)})
    p = rng.permutation(len(bk) + fill + 20)
    bt = tarr([t] * (len(bk) + fill) + [t2] * 20)[p]
    rid = np.array(rid + [-1] * (fill + 20))[p]
    days = np.full(len(p), 77, dtype=np.int64)
    for i, d in enumerate(pats):  # the pattern runs in arrival order
        days[np.flatnonzero(rid == i)] = d
    rows = make_rows(hashes(bk + fk + fk[:20])[p], days, rng)
    # scattered: no run of two or more stands as one block in arrival order
    pos = {}
    for p, h in enumerate(s12(rows)):
        pos.setdefault(bytes(h) + bt[p].tobytes(), []).append(p)
    assert all(ps[-1] - ps[0] >= len(ps) for ps in pos.values() if 2 <= len(ps))
    c.add(bt, rows, policy)
    c.qterms = [t, t2, BY1]
    return c


@_case("runs_lengths", POLICIES)
def _runs_lengths(policy):
    """runs of 1, 2, 3, 64, 257 and 1000 copies, each for a url new to the list and for one it has"""
    plan = []
    for i, L in enumerate((1, 2, 3, 64, 257, 1000)):
        for v in range(2):
            plan.append((L, LM_PATTERNS[(2 * i + v) % 7], None if v == 0 else ("below", "equal", "above")[i % 3]))
    plan.append((1000, "max_twice_then_smaller", "equal"))
    plan.append((257, "all_equal", "equal"))
    c = _runs_case(plan, 1, policy)
    c.facts["run_lengths"] = sorted({L for L, _, _ in plan})
    return c


@_case("runs_last_modified", POLICIES)
def _runs_lm(policy):
    """every pattern of days over a run of 5 (and of 3), against no row and a row below / equal / above"""
    plan = [(L, p, rel) for L in (5, 3) for p in LM_PATTERNS for rel in (None, "below", "equal", "above")]
    c = _runs_case(plan, 2, policy)
    if policy == "recent":  # the ties decide rows: `>` in place of `>=` on either side would change the result
        t = term(2000)
        bt, rows = c.steps[0].terms, c.steps[0].rows
        mine = rows[s12(bt) == t]
        got = {bytes(r[:12]): bytes(r) for r in c.cur[t]}
        key = lambda i: bytes(hashes([BASE + 148 * 3 * i])[0])
        for i, (L, p, rel) in enumerate(plan):
            run = mine[s12(mine) == key(i)]
            d = days_of(run)
            assert len(run) == L
            last_max = int(np.flatnonzero(d == d.max())[-1])
            if rel == "above" and d.max() < 65535:
                assert got[key(i)] == bytes(c.lists[t][list(s12(c.lists[t])).index(key(i))])
            else:  # below, equal (the arrival wins a tie) and new: the last of the largest
                assert got[key(i)] == bytes(run[last_max]), (L, p, rel)
            if p == "max_twice_then_smaller" and L >= 3:
                assert last_max == L - 2 and d[0] == d.max() and d[-1] < d.max()
    return c


@_case("run_at_block_edge", POLICIES)
def _block_edge(policy):
    """one job: a run at sorted positions 0..2, a run whose head is at 255 and whose tail is 256..554 (two
    more block edges inside it), a run that ends at n - 1"""
    rng = _rng(10)
    t = term(2100)
    nk = 255 - 3 + 1 + 1 + 40 + 1   # distinct keys: run A, 252 singles, run B, 40 singles, run C
    ks = [BASE + 100 * i for i in range(nk)]
    count = [3] + [1] * 252 + [300] + [1] * 40 + [3]
    assert len(count) == nk
    bk = [k for k, m in zip(ks, count) for _ in range(m)]
    n = len(bk)
    lists = {t: make_rows(hashes([ks[0], ks[100], ks[253]]), [6, 6, 6], rng)}  # runs A and B meet a row, C none
    c = Case("", {**lists, **_bystanders(rng)})
    bt, rows = _shuffled(rng, [t] * n, make_rows(hashes(bk), rng.integers(5, 8, n), rng))
    o = sorted_order(bt, rows)
    sk = s12(rows)[o]
    run = lambda k: np.flatnonzero(sk == bytes(hashes([k])[0]))
    a, b, z = run(ks[0]), run(ks[253]), run(ks[-1])
    assert list(a) == [0, 1, 2]
    assert b[0] == 255 and list(b[1:]) == list(range(256, 555))
    assert list(z) == [n - 3, n - 2, n - 1]
    assert (np.diff(o[b]) > 0).all() and o[b].max() - o[b].min() > 300  # arrival order inside the run, scattered
    c.add(bt, rows, policy)
    c.facts["runs"] = {"head0": (ks[0], 0, 2), "edge": (ks[253], 255, 554), "tail": (ks[-1], n - 3, n - 1)}
    c.qterms = [t, BY1]
    return c


@_case("same_url_neighbour_jobs", POLICIES)
def _neighbour_jobs(policy):
    """url u_j is the largest batch key of job j and the smallest of job j + 1: neighbours in the sorted
    batch, and two runs"""
    rng = _rng(11)
    nj = 8
    ts = [term(2200 + j) for j in range(nj)]
    u = [BASE + 10000 * (j + 1) for j in range(nj)]  # u[j] shared by jobs j and j + 1
    lists = {ts[j]: make_rows(hashes(sorted({u[j], u[j] - 148} | ({u[j - 1]} if j % 3 == 0 and j else set()))),
                              6, rng) for j in range(nj) if j % 2 == 0}
    c = Case("", {**lists, **_bystanders(rng)})
    bt, bk = list(ts), [u[j] - 50 for j in range(nj)]  # every job's first posting, in turn: job j is ts[j]
    for j in range(nj):
        ks = [u[j]] * (1 + j % 3) + [u[j] - 74, u[j] - 148]
        if j:
            ks += [u[j - 1]] * (1 + (j + 1) % 2)
        bt += [ts[j]] * len(ks)
        bk += ks
    rows = make_rows(hashes(bk), rng.integers(5, 8, len(bk)), rng)
    p = np.concatenate([np.arange(nj), nj + rng.permutation(len(bk) - nj)])
    bt, rows = tarr(bt)[p], rows[p]
    job, names_ = jobs_of(bt)
    assert names_ == ts
    o = sorted_order(bt, rows)
    sj, sk = job[o], s12(rows)[o]
    pairs = []
    for j in range(nj - 1):
        h = bytes(hashes([u[j]])[0])
        last = int(np.flatnonzero((sj == j) & (sk == h))[-1])
        first = int(np.flatnonzero((sj == j + 1) & (sk == h))[0])
        assert first == last + 1, (j, last, first)  # adjacent: the job alone parts the two runs
        assert last == np.flatnonzero(sj == j)[-1] and first == np.flatnonzero(sj == j + 1)[0]
        pairs.append((last, first))
    st = c.add(bt, rows, policy)
    assert st["terms"] == nj  # every job gains u_j - 74
    assert all(len(c.cur[ts[j]]) == len({key72(r) for r in c.cur[ts[j]]}) for j in range(nj))
    c.facts["pairs"] = pairs
    c.qterms = [ts[1], ts[2], ts[0], ts[3]]
    return c


@_case("near_keys", POLICIES)
def _near_keys(policy):
    """triples of keys equal in 64 of their 72 bits, batch row against batch row in one job and batch row
    against list row; none is a duplicate: every posting is added under every policy"""
    rng = _rng(12)
    ta, tb = term(2300), term(2301)
    base = [(kind, BASE + 148 * 7 * i + 3) for i, kind in enumerate("abc" * 40)]
    tri = [_check_near(k, kind) for kind, k in base]
    allk = [k for t3 in tri for k in t3]
    assert len(set(allk)) == len(allk)
    plain = [BASE - 148 * (i + 1) for i in range(30)]
    la = make_rows(hashes(sorted([t3[0] for t3 in tri] + plain)), 6, rng)   # ta holds member 0 of every triple
    lb = make_rows(hashes(sorted([t3[1] for t3 in tri] + plain[::2])), 6, rng)
    tc = term(2302)                                                          # tc: all three from the batch
    c = Case("", {ta: la, tb: lb, **_bystanders(rng)})
    parts = [(ta, [k for t3 in tri for k in t3[1:]]), (tb, [k for t3 in tri for k in (t3[0], t3[2])]), (tc, allk)]
    bt, rows = _batch(rng, parts)
    st = c.add(bt, rows, policy)
    n = len(rows)
    assert st == dict(terms=3, new_terms=1, emptied_terms=0, added=n, replaced=0, dropped=0, removed=0)
    for t in (ta, tb, tc):  # the result in the full 72-bit order
        assert ascending(c.cur[t]) and {key72(r) for r in c.cur[t]} >= set(allk)
    c.qterms = [ta, tb, tc, BY1]
    c.facts["joins"] = [[ta, tb], [tb, ta], [tc, ta], [ta, tb, tc]]
    return c


# ------------------------------------------------------------------ C. remove
RM_SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)
RM_PATTERNS = {
    "first": lambda i, n: i == 0,
    "last": lambda i, n: i == n - 1,
    "all": lambda i, n: i >= 0,
    "all_but_first": lambda i, n: i > 0,
    "all_but_last": lambda i, n: i < n - 1,
    "even": lambda i, n: i % 2 == 0,
    "odd": lambda i, n: i % 2 == 1,
    "fifth_0": lambda i, n: i % 5 == 0,
    "fifth_1": lambda i, n: i % 5 == 1,
    "fifth_2": lambda i, n: i % 5 == 2,
    "fifth_3": lambda i, n: i % 5 == 3,
    "fifth_4": lambda i, n: i % 5 == 4,
    "wave_64_127": lambda i, n: (i >= 64) & (i < 128),
    "block_0_255": lambda i, n: i < 256,
    "keep_lane_0": lambda i, n: i % 64 != 0,
    "keep_lane_63": lambda i, n: i % 64 != 63,
}
RM_TERMS = [term(2400 + k) for k in range(len(RM_SIZES))]
UNKNOWN = term(2499)


def _rm_key(k, r):
    """row r of removal list k: the lists share no url, so a position is removed in one list alone"""
    return BASE + ((k + 1) << 24) + 148 * r


def _rm_lists(rng):
    lists = {t: make_rows(hashes([_rm_key(k, r) for r in range(n)]), 100 + k, rng)
             for k, (t, n) in enumerate(zip(RM_TERMS, RM_SIZES))}
    return {**lists, **_bystanders(rng)}


def _remove_pattern(pat, named):
    def fn(policy):
        rng = _rng(13)
        lists = _rm_lists(rng)
        c = Case("", lists)
        masks = {t: np.asarray(RM_PATTERNS[pat](np.arange(n), n), dtype=bool) & np.ones(n, dtype=bool)
                 for t, n in zip(RM_TERMS, RM_SIZES)}
        urls = [bytes(r[:12]) for t in RM_TERMS for r in lists[t][masks[t]]]
        urls = [urls[int(i)] for i in rng.permutation(len(urls))] + urls[:3] + [bytes(hashes([BASE - 7])[0])]
        who = [RM_TERMS[int(i)] for i in rng.permutation(len(RM_TERMS))]
        who = who[:4] + [UNKNOWN, who[1]] + who[4:] + [who[0]] if named else None
        st = c.remove(urls, who)
        for t in RM_TERMS:  # by position
            left = lists[t][~masks[t]]
            assert c.cur.get(t, EMPTY).tobytes() == left.tobytes() and (len(left) > 0) == (t in c.cur)
            if not masks[t].any():
                assert c.cur[t] is lists[t]
        assert c.cur[BY1] is lists[BY1] and c.cur[BY2] is lists[BY2]
        hit = [t for t in RM_TERMS if masks[t].any()]
        assert st == dict(dict.fromkeys(STAT_KEYS, 0), terms=len(hit), removed=sum(int(m.sum()) for m in masks.values()),
                          emptied_terms=sum(1 for t in hit if masks[t].all()))
        c.qterms = [RM_TERMS[7], RM_TERMS[6], RM_TERMS[4], BY1]
        return c
    return fn


for _p in RM_PATTERNS:
    _case("rm_%s_named" % _p)(_remove_pattern(_p, True))
    _case("rm_%s_all" % _p)(_remove_pattern(_p, False))


@_case("rm_near_miss")
def _near_miss(policy):
    """for 200 rows the set holds their (a), (b) and (c) neighbours and not the rows: nothing goes; then the
    true urls of 20 of them join the set: exactly those go"""
    rng = _rng(14)
    lists = _rm_lists(rng)
    c = Case("", lists)
    have = {key72(r) for l in lists.values() for r in l}
    where = [(t, int(i)) for t in RM_TERMS for i in range(len(lists[t]))]
    where = [where[int(i)] for i in rng.choice(len(where), 200, replace=False)]
    assert len({t for t, _ in where}) >= 5
    urls = []
    for t, i in where:
        k = key72(lists[t][i])
        for kind in "abc":
            ks = _check_near(k, kind)[1:]
            assert not set(ks) & have
            urls += ks
    miss = [bytes(h) for h in hashes(urls)]
    st = c.remove([miss[int(i)] for i in rng.permutation(len(miss))], None)
    assert st == dict.fromkeys(STAT_KEYS, 0) and all(c.cur[t] is lists[t] for t in lists)
    true = [bytes(lists[t][i, :12]) for t, i in where[:20]]
    st = c.remove(miss + true, None)
    assert st["removed"] == 20 and st["emptied_terms"] == 0
    for t in RM_TERMS:
        gone = sorted(i for tt, i in where[:20] if tt == t)
        assert c.cur[t].tobytes() == np.delete(lists[t], gone, axis=0).tobytes()
    c.facts["near_sets"] = (miss, true)
    c.qterms = [RM_TERMS[7], RM_TERMS[6], RM_TERMS[4], BY1]
    return c


def _rm_set(size):
    def fn(policy):
        """a url set of `size`, unsorted and with duplicates, most of it absent from every list"""
        rng = _rng(15, size)
        lists = _rm_lists(rng)
        c = Case("", lists)
        present = [bytes(lists[RM_TERMS[7]][700, :12]), bytes(lists[BY1][3, :12])] + \
                  [bytes(r[:12]) for r in lists[RM_TERMS[6]][::9]]
        absent = [bytes(h) for h in hashes([BASE + (99 << 24) + 11 * i for i in range(size)])]
        urls = (present[:max(1, size // 40)] + absent)[:size]
        assert len(set(urls)) == size
        urls = urls + urls[: 1 + size // 8]  # duplicates
        st = c.remove([urls[int(i)] for i in rng.permutation(len(urls))], None)
        assert st["removed"] == min(len(present), max(1, size // 40)) and st["emptied_terms"] == 0
        c.qterms = [RM_TERMS[7], RM_TERMS[6], BY1]
        return c
    return fn


for _n in (1, 2, 4097):
    _case("rm_set_%d" % _n)(_rm_set(_n))


@_case("rm_everything")
def _rm_everything(policy):
    """the set holds every url of every list: every list is emptied and none is compacted"""
    rng = _rng(16)
    lists = _rm_lists(rng)
    c = Case("", lists)
    urls = [bytes(r[:12]) for l in lists.values() for r in l]
    st = c.remove([urls[int(i)] for i in rng.permutation(len(urls))], None)
    assert not c.cur and st["emptied_terms"] == st["terms"] == len(lists) and st["removed"] == len(urls)
    return c


@_case("rm_round_trip")
def _round_trip(policy):
    """new urls only are added, then exactly those are removed under the touched terms: every starting list
    is back byte for byte and the terms the add created are gone"""
    rng = _rng(17)
    lists = _rm_lists(rng)
    c = Case("", lists)
    fresh = [term(2480), term(2481)]
    parts = [(t, [_rm_key(k, r) - 74 for r in range(0, n + 1, 2)]) for k, (t, n) in enumerate(zip(RM_TERMS, RM_SIZES))]
    parts += [(fresh[0], [BASE + 5]), (fresh[1], [BASE + 148 * i + 5 for i in range(100)])]
    bt, rows = _batch(rng, parts)
    st = c.add(bt, rows)
    assert st["added"] == len(rows) and st["new_terms"] == 2
    st = c.remove([bytes(r[:12]) for r in rows], RM_TERMS + fresh)
    assert st["removed"] == len(rows) and st["emptied_terms"] == 2 and st["terms"] == len(RM_TERMS) + 2
    assert set(c.cur) == set(lists) and all(c.cur[t].tobytes() == lists[t].tobytes() for t in lists)
    c.qterms = [RM_TERMS[7], RM_TERMS[6], RM_TERMS[4], fresh[1]]
    return c


# ------------------------------------------------------------------ D. more than two staging pieces
THREE_N = 850_000


@_case("three_pieces")
def _three_pieces(policy):
    """850,000 rows (34,000,000 B) of distinct urls in random order to three new terms: stage_rows uses its
    first pinned piece a second time"""
    rng = _rng(18)
    n = THREE_N
    assert n * 40 > 2 * PIECE
    a = np.unique(rng.integers(0, 1 << 60, n + n // 50, dtype=np.int64))  # characters 0..9, ascending
    assert len(a) >= n
    a = a[:n]
    b = rng.integers(0, 1 << 12, n, dtype=np.int64)                      # characters 10, 11
    rows = rng.integers(0, 256, (n, 40), dtype=np.uint8)
    for j in range(10):
        rows[:, j] = _ALPHA[(a >> (6 * (9 - j))) & 63]
    rows[:, 10], rows[:, 11] = _ALPHA[b >> 6], _ALPHA[b & 63]
    nolang = (rows[:, 22] == 0) & (rows[:, 23] == 0)
    rows[nolang, 22:24] = np.frombuffer(b"en", dtype=np.uint8)
    ts = [term(2500 + j) for j in range(3)]
    which = rng.integers(0, 3, n)
    which[:3] = (0, 1, 2)
    exp = {ts[j]: rows[which == j] for j in range(3)}  # (rows is ascending: a is, and every a is there once)
    p = rng.permutation(n)
    c = Case("", {})
    c.light = True
    c.steps.append(Step("add", exp, dict(dict.fromkeys(STAT_KEYS, 0), terms=3, new_terms=3, added=n),
                        terms=tarr(ts)[which][p], rows=rows[p], policy="replace"))
    c.cur = exp
    c.sample = list(ts)
    c.facts["prebuilt"] = []
    c.facts["terms"] = tarr(ts)
    return c


# ------------------------------------------------------------------ atomicity
def _atomic(bad, where):
    def fn(policy):
        """a malformed url hash (-2) or an empty language cell (-7), as the last row of a batch of 257 or as a
        losing copy inside a run under keep: the call fails and nothing has changed"""
        rng = _rng(19, bad == "hash", where == "last")
        t, t2 = term(2600), term(2601)
        lists = {t: _list(100, rng), **_bystanders(rng)}
        c = Case("", lists)
        if where == "last":
            ks = [R(r, 100) - 74 for r in range(200)] + [R(r, 100) for r in range(57)]
            bt = [t] * 200 + [t2] * 57
            rows = make_rows(hashes(ks), 9, rng)
            at, pol = 256, "replace"
            assert len(rows) == 257
        else:
            ks = [R(5, 100)] * 6 + [R(7, 100) - 74] * 6 + [R(r, 100) - 74 for r in range(20, 60)]
            bt = [t] * len(ks)
            bt, rows = _shuffled(rng, bt, make_rows(hashes(ks), 9, rng))
            at, pol = int(np.flatnonzero(s12(rows) == bytes(hashes([R(7, 100) - 74])[0]))[3]), "keep"
        if bad == "hash":
            rows[at, 4] = ord("!")
            rc = -2
        else:
            rows[at, 22:24] = 0
            rc = -7
        c.error(bt, rows, pol, rc)
        c.qterms = [t, BY1]
        return c
    return fn


for _b in ("hash", "language"):
    for _w in ("last", "in_run"):
        _case("atomic_%s_%s" % (_b, _w))(_atomic(_b, _w))
