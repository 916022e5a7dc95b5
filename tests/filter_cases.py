"""Directed inputs of the query filters (admit / passes fused into k_score, the flag counts, the
per-query threshold under a filter) and of the doubledom pull (k_pull): a helper, no tests.

A Case is one query over hand-made lists: include and exclude terms, QueryFilter keyword arguments,
k, the ranking language, a profile, environment variables, and two expectations that are computed
here BY CONSTRUCTION -- with numpy, from the arrays the rows were generated from (Gen: the flag
words, doctypes, languages and hosts), never by decoding rows through java_literal:
    admitted    the url hashes addRWIs puts on the stack (SearchEvent.java:736-806)
    flagcount   SearchEvent.flagcount: one count per flag bit over the rows that pass the doublecheck
A doubledom case also carries the hosts of the stack in rank order (stack_hosts; as letters in
`pattern` when the hosts have letters) and, where it is short enough, the pulled order written
down by hand (`pulled`).  tests/test_filter_cases_ref.py checks every expectation against the
literal oracle on the CPU (two independent statements of the rules), tests/test_gpu_filters_directed.py
runs every case through the library and compares hits and flag counts with java_literal.search.

The families (one device index serves a family):
    flags, contentdom, language, site, doublecheck   the predicates of `passes` and the doublecheck
    counting     flag counts once per posting on every path of k_score / k_score_full
    threshold    the published k-th score (Tq) must come from admitted postings only
    norm         a rejected row that holds a column's extreme still normalises the admitted rows
    joins        filters over a joined container (url keys through the url ids), an authority profile
    doubledom    the pull order on designed host patterns
    batch        300 queries of one call, each filter object with its own counts

Designed scores.  A normalised term has 257 levels, so no single cell gives thousands of distinct
scores: score_profile() is adv_rows.single("wordsintext", 13) with phrasesintext at 5, and a row of
designed rank value r stores wordsintext = r >> 8 and phrasesintext = r & 255; the row of the
largest r stores 256 in both, so both spans are 256 and cardinal is const + (r >> 8 << 13) +
(r & 255 << 5) + (256 - domlength), strictly rising in r (the domlength classes differ by < 32)."""

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

import adv_rows as ar
import java_literal as jl

NOW = 20741 * 86400000 + 4242
MAX_K = 3000            # YRWI_MAX_K == SearchEvent.max_results_rwi
CHUNK = 2048            # rows a k_score workgroup scores
SCORE_SMALL = 256       # k above it: k_score only counts, k_score_full scores
DD_SLOTS = 8192         # k_pull's host table
H_ZERO, H_TOP = b"AAAAAA", b"______"   # host keys 0 and 2^36 - 1
_ALPHA = np.frombuffer(jl.ALPHA, dtype=np.uint8)
_Z = ar._off("z")


# ------------------------------------------------------------------ small helpers
def enc(v: int, width: int) -> bytes:
    return bytes(jl.ALPHA[(v >> (6 * (width - 1 - j))) & 63] for j in range(width))


def host_key(h: bytes) -> int:
    k = 0
    for b in h:
        k = (k << 6) | jl.AHPLA[b]
    return k


def term(family: str, j: int) -> bytes:
    return b"F" + family.encode()[:8].ljust(8, b"-") + b"-" + enc(j, 2)


def bits(*js) -> bytes:
    """a 4-byte Bitfield with the bits js: bit p is bit p % 8 of byte p >> 3"""
    b = bytearray(4)
    for j in js:
        b[j >> 3] |= 1 << (j & 7)
    return bytes(b)


def score_profile() -> jl.RankingProfile:
    p = ar.single("wordsintext", 13)
    p.coeff_phrasesintext = 5
    return p


@dataclass
class Gen:
    """rows and the arrays they were generated from"""
    rows: np.ndarray
    z: np.ndarray      # int64: the 32 flag bits, bit j = flag j
    d: np.ndarray      # uint8 doctypes
    l: np.ndarray      # (n, 2) uint8 languages
    host: np.ndarray   # (n, 6) uint8 host hashes

    @property
    def urls(self) -> List[bytes]:
        return [bytes(x) for x in self.rows[:, :12]]

    def take(self, keep: np.ndarray) -> "Gen":
        return Gen(self.rows[keep], self.z[keep], self.d[keep], self.l[keep], self.host[keep])


def _as_hosts(hosts, n) -> np.ndarray:
    if isinstance(hosts, np.ndarray):
        return hosts
    return np.frombuffer(b"".join(hosts), dtype=np.uint8).reshape(n, 6)


def _stamp(rows, z, d, l, host) -> Gen:
    """write the generating arrays into the rows' cells"""
    n = len(rows)
    z = np.broadcast_to(np.asarray(z, dtype=np.int64), (n,)).copy()
    d = np.broadcast_to(np.asarray(d, dtype=np.uint8), (n,)).copy()
    l = np.broadcast_to(np.asarray(l, dtype=np.uint8), (n, 2)).copy()
    host = _as_hosts(host, n).copy()
    for j in range(4):
        rows[:, _Z + j] = (z >> (8 * j)) & 0xFF
    rows[:, ar._off("d")] = d
    rows[:, ar._off("l"):ar._off("l") + 2] = l
    rows[:, 6:12] = host
    return Gen(rows, z, d, l, host)


def _lang(b: bytes) -> np.ndarray:
    return np.frombuffer(b, dtype=np.uint8)


def hostile(n, seed, z=None, d=None, l=None, host=None) -> Gen:
    """adv_rows' edge rows (every cell hostile) with the four filtered cells drawn here"""
    rng = np.random.default_rng([seed, n, 77])
    rows = ar.adv_rows(n, seed, "edge")
    if z is None:
        z = rng.integers(0, 1 << 32, n, dtype=np.int64)
    if d is None:
        d = _lang(b"tiam")[rng.integers(0, 4, n)]
    if l is None:
        l = _lang(b"".join(ar.LANGS)).reshape(-1, 2)[rng.integers(0, len(ar.LANGS), n)]
    if host is None:
        pool = _lang(b"hostAAhostABsiteXy").reshape(3, 6)
        host = pool[rng.integers(0, 3, n)]
    return _stamp(rows, z, d, l, host)


def plain(n, host, /, z=0, l=b"en", d=ord("t"), salt=0, **cols) -> Gen:
    """rows equal in every feature cell (lastModified 15000, posintext 1, else 0) but `cols`;
    url hashes ascending in the row index"""
    rows = np.zeros((n, 40), dtype=np.uint8)
    v = (np.arange(n, dtype=np.int64) + 1) * 9973 + (salt << 28)
    assert n == 0 or v[-1] < (1 << 36)
    for j in range(6):
        rows[:, j] = _ALPHA[(v >> (6 * (5 - j))) & 63]
    ar._put(rows, "a", 15000)
    ar._put(rows, "t", 1)
    for c, val in cols.items():
        ar._put(rows, c, val)
    return _stamp(rows, z, d, _lang(l) if isinstance(l, bytes) else l, host)


def designed(r: np.ndarray, host, z=0, l=b"en", salt=0) -> Gen:
    """plain rows whose score under score_profile() rises strictly with r (a permutation of
    0..n-1 over the list positions); see the module docstring"""
    r = np.asarray(r, dtype=np.int64)
    assert sorted(r.tolist()) == list(range(len(r))) and len(r) < (1 << 16)
    w, p = r >> 8, r & 255
    top = int(np.argmax(r))
    w[top], p[top] = 256, 256
    return plain(len(r), host, z=z, l=l, salt=salt, w=w, p=p)


# ------------------------------------------------------------------ the rules, by construction
def expect(g: Gen, kw: dict, keep: Optional[np.ndarray] = None):
    """(admitted url hashes, 32 flag counts) of the container g (its rows `keep`) under the
    filter kw, from the generating arrays"""
    n = len(g.rows)
    keep = np.ones(n, dtype=bool) if keep is None else keep
    urls = g.urls
    seen = {bytes(u) for u in kw.get("urlhashes", ())}
    dc = np.fromiter((u in seen for u in urls), dtype=bool, count=n)
    counted = keep & ~dc                       # the doublecheck comes first, then the counts
    fc = [int(((g.z[counted] >> j) & 1).sum()) for j in range(32)]
    ok = counted.copy()
    if kw.get("constraint") is not None:
        c = int.from_bytes(kw["constraint"], "little")
        ok &= ((g.z & c) == c) if kw.get("all_of_constraint") else ((g.z & c) != 0)
    cd = kw.get("contentdom", 0)
    if 1 <= cd <= 4:                           # IMAGE, AUDIO, VIDEO, APP; TEXT and the others filter nothing
        if kw.get("strict_contentdom") and cd != 4:
            ok &= g.d == ord("iam"[cd - 1])
        else:
            ok &= ((g.z >> (19 + cd)) & 1) == 1
    lang = kw.get("language", "")
    if lang:
        lb = lang.encode()
        ok &= np.fromiter((bytes(x) == lb for x in g.l), dtype=bool, count=n)
    hosts = [bytes(h) for h in g.host]
    if kw.get("sitehash") is not None:         # siteexcludes are not consulted then
        acc = {bytes(kw["sitehash"])}
        if kw.get("alt_sitehash") is not None:
            acc.add(bytes(kw["alt_sitehash"]))
        ok &= np.fromiter((h in acc for h in hosts), dtype=bool, count=n)
    else:
        ex = {bytes(h) for h in kw.get("siteexcludes", ())}
        ok &= np.fromiter((h not in ex for h in hosts), dtype=bool, count=n)
    return frozenset(u for u, a in zip(urls, ok) if a), fc


@dataclass
class Case:
    name: str
    lists: Dict[bytes, np.ndarray]
    include: List[bytes]
    exclude: List[bytes]
    kw: Optional[dict]                 # QueryFilter kwargs; None: no filter
    k: int
    admitted: frozenset
    flagcount: Optional[List[int]]
    container: int                     # rows of the joined container
    language: str = "en"
    profile: Optional[jl.RankingProfile] = None
    env: Dict[str, str] = field(default_factory=dict)
    vacuous: str = ""                  # "nothing" / "everything": the case is meant to admit that
    twin: Optional["Case"] = None      # norm: the same query without the rejected extremes
    stack_hosts: Optional[List[bytes]] = None   # doubledom: hosts of the stack, rank order
    pattern: Optional[str] = None      # the same as letters
    pulled: Optional[str] = None       # the pulled order as letters, written by hand

    def literal_profile(self) -> jl.RankingProfile:
        return self.profile if self.profile is not None else jl.RankingProfile()


@dataclass
class Batch:
    name: str
    lists: Dict[bytes, np.ndarray]
    queries: List[Case]


def _case(name, lists, inc, exc, kw, g, k=100, keep=None, **more) -> Case:
    adm, fc = expect(g, kw, keep)
    n = len(g.rows) if keep is None else int(keep.sum())
    if more.get("vacuous"):
        name += " (admits %s)" % more["vacuous"]
    return Case(name, lists, inc, exc, kw, k, adm, fc, n, **more)


def literal_lists(lists) -> Dict[bytes, List[bytes]]:
    return {h: [bytes(r) for r in rows] for h, rows in lists.items()}


# ------------------------------------------------------------------ flags
@functools.lru_cache(maxsize=None)
def flag_cases() -> List[Case]:
    """one row per single bit 0..31, all ones, zero, repeated to 600 rows"""
    n = 600
    z = np.array([1 << j for j in range(32)] + [0xFFFFFFFF, 0], dtype=np.int64)[np.arange(n) % 34]
    g = hostile(n, 11, z=z)
    t = term("flags", 0)
    lists = {t: g.rows}
    out = []

    def add(name, k=100, **kw):
        vac = kw.pop("vacuous", "")
        out.append(_case("flags/" + name, lists, [t], [], kw, g, k, vacuous=vac))

    for j in (0, 7, 8, 15, 16, 20, 21, 22, 23, 24, 31):
        add("any_bit%d" % j, k=20, constraint=bits(j))
    for a, b in ((7, 8), (15, 16), (23, 24), (0, 31)):
        add("any_bits%d_%d" % (a, b), constraint=bits(a, b))
        add("all_bits%d_%d" % (a, b), constraint=bits(a, b), all_of_constraint=True)
    add("all_bit31", constraint=bits(31), all_of_constraint=True)
    add("all_bit0", k=10, constraint=bits(0), all_of_constraint=True)
    add("empty_any", constraint=bits(), vacuous="nothing")
    add("empty_all", constraint=bits(), all_of_constraint=True, vacuous="everything")
    return out


# ------------------------------------------------------------------ contentdom
@functools.lru_cache(maxsize=None)
def contentdom_cases() -> List[Case]:
    """every doctype of t i a m crossed with flags 20..23 set and clear; codes 0..5 and -1"""
    n = 320
    i = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(12)
    z = (rng.integers(0, 1 << 32, n, dtype=np.int64) & ~(0xF << 20)) | (((i // 4) % 16) << 20)
    g = hostile(n, 12, z=z, d=_lang(b"tiam")[i % 4])
    t = term("contentd", 0)
    lists = {t: g.rows}
    out = []
    for code in (0, 1, 2, 3, 4, 5, -1):
        for strict in (False, True):
            vac = "" if 1 <= code <= 4 else "everything"
            out.append(_case("contentdom/code%d%s" % (code, "_strict" if strict else ""), lists, [t], [],
                             dict(contentdom=code, strict_contentdom=strict), g, 50, vacuous=vac))
    return out


# ------------------------------------------------------------------ language
@functools.lru_cache(maxsize=None)
def language_cases() -> List[Case]:
    n = 350
    langs = _lang(b"".join(ar.LANGS)).reshape(-1, 2)
    g = hostile(n, 13, l=langs[np.arange(n) % len(ar.LANGS)])
    t = term("language", 0)
    lists = {t: g.rows}
    out = []
    for f, vac in (("", "everything"), ("e", "nothing"), ("en", ""), ("EN", ""), ("de", ""), ("eng", "nothing"),
                   ("english", "nothing")):
        out.append(_case("language/%r" % f, lists, [t], [], dict(language=f), g, 30, vacuous=vac))
    return out


# ------------------------------------------------------------------ site
SITE_POOL = [H_ZERO, H_TOP, b"hostAA", b"hostAB", b"siteXy", b"0-_9zZ", b"B_____", b"_____-", b"AAAAAB", b"mmmmmm",
             b"Zz09-_", b"qwerty"]
ABSENT_HOST = b"absent"


def _fillers(m: int, seed: int) -> List[bytes]:
    """m distinct host hashes outside SITE_POOL, strictly between keys 0 and 2^36 - 1"""
    rng = np.random.default_rng(seed)
    pool = {host_key(h) for h in SITE_POOL + [ABSENT_HOST]}
    ks = [int(x) for x in np.unique(rng.integers(1, (1 << 36) - 1, 2 * m, dtype=np.int64)) if int(x) not in pool]
    assert len(ks) >= m
    ks = [ks[j] for j in rng.permutation(len(ks))[:m]]
    return [enc(x, 6) for x in ks]


def _unsorted(hs: List[bytes], dupes: int, seed: int) -> List[bytes]:
    """descending by key (a binary search over it as given fails), then `dupes` repeats"""
    rng = np.random.default_rng(seed)
    out = sorted(hs, key=host_key, reverse=True)
    return out + [out[int(j)] for j in rng.integers(0, len(out), dupes)]


@functools.lru_cache(maxsize=None)
def site_cases() -> List[Case]:
    n = 420
    rng = np.random.default_rng(14)
    pool = _lang(b"".join(SITE_POOL)).reshape(-1, 6)
    g = hostile(n, 14, host=pool[rng.permutation(n) % len(SITE_POOL)])
    t = term("site", 0)
    lists = {t: g.rows}
    P = SITE_POOL
    fill = _fillers(4096, 15)
    out = []

    def add(name, k=100, vacuous="", **kw):
        out.append(_case("site/" + name, lists, [t], [], kw, g, k, vacuous=vacuous))

    add("site_zero", sitehash=H_ZERO)
    add("site_top", sitehash=H_TOP)
    add("site_plain", k=10, sitehash=P[2])
    add("site_alt", sitehash=P[2], alt_sitehash=P[3])
    add("site_alt_zero", sitehash=P[4], alt_sitehash=H_ZERO)
    add("site_absent_alt_top", sitehash=ABSENT_HOST, alt_sitehash=H_TOP)
    add("alt_alone", alt_sitehash=P[3], vacuous="everything")
    add("site_and_excludes_ignored", sitehash=P[2], siteexcludes=[P[2], P[3], H_ZERO])
    add("site_alt_and_excludes_ignored", sitehash=P[5], alt_sitehash=P[6], siteexcludes=_unsorted(P, 3, 1))
    add("ex1", siteexcludes=[P[5]])
    add("ex1_zero", siteexcludes=[H_ZERO])
    add("ex1_top", siteexcludes=[H_TOP])
    add("ex2_unsorted", siteexcludes=[H_TOP, H_ZERO])
    add("ex2_dupes", siteexcludes=[P[6], P[5], P[6], P[5], P[6]])
    add("ex_pool_but_one", siteexcludes=_unsorted(P[:9] + P[10:], 5, 2))
    add("ex4097_first", siteexcludes=_unsorted(fill + [H_ZERO], 40, 3))
    add("ex4097_last", siteexcludes=_unsorted(fill + [H_TOP], 40, 4))
    add("ex4097_inside", siteexcludes=_unsorted(fill[:4094] + [P[2], P[7], P[8]], 40, 5))
    add("ex4097_none", siteexcludes=_unsorted(fill + [ABSENT_HOST], 40, 6), vacuous="everything")
    add("ex_outside_alphabet", siteexcludes=[b"host!A", P[5], b"\xffAAAAA", b"AAAAA\0", P[9]])
    add("site_malformed", sitehash=b"hostA!", vacuous="nothing")
    add("site_malformed_alt", sitehash=b"\xffAAAAA", alt_sitehash=P[3])
    add("alt_malformed", sitehash=P[2], alt_sitehash=b"host!B")
    return out


# ------------------------------------------------------------------ doublecheck
def _near_absent(urls: List[bytes], held: set) -> List[bytes]:
    """hashes that share their first six characters, their last six, or all but the last one with
    a url of the container and are not in it"""
    out = ([u[:6] + bytes(reversed(u[6:])) for u in urls] + [u[:6] + b"zzzzzz" for u in urls] +
           [bytes(reversed(u[:6])) + u[6:] for u in urls] +
           [u[:11] + bytes([jl.ALPHA[(jl.AHPLA[u[11]] + 1) % 64]]) for u in urls])
    return sorted({u for u in out if u not in held})


@functools.lru_cache(maxsize=None)
def doublecheck_cases() -> List[Case]:
    n = 500
    g = hostile(n, 16)
    urls = g.urls
    held = set(urls)
    t = term("doublech", 0)
    lists = {t: g.rows}
    rng = np.random.default_rng(16)
    absent = [bytes(x[:12]) for x in ar.adv_rows(4100, 17, "edge")]
    absent = [u for u in absent if u not in held] + _near_absent(urls[:150], held)
    some = [urls[0], urls[-1]] + [urls[int(j)] for j in rng.choice(np.arange(1, n - 1), 248, replace=False)]
    many = absent + some
    many = many + [many[int(j)] for j in rng.integers(0, len(many), 5000 - len(many))]   # duplicates
    many = [many[int(j)] for j in rng.permutation(5000)]
    out = []

    def add(name, k=100, vacuous="", **kw):
        out.append(_case("doublecheck/" + name, lists, [t], [], kw, g, k, vacuous=vacuous))

    add("first", urlhashes=[urls[0]])
    add("last", urlhashes=[urls[-1]])
    add("absent", urlhashes=[absent[0]], vacuous="everything")
    add("many5000", urlhashes=many)
    add("every_url", urlhashes=list(reversed(urls)), vacuous="nothing")
    add("malformed", urlhashes=[b"AAAAAA!AAAAA", urls[3], b"\xff" + urls[4][1:], urls[5][:11] + b"\0"])
    add("then_language", k=30, urlhashes=[urls[j] for j in range(0, n, 3)], language="en")
    add("then_constraint", urlhashes=[urls[j] for j in range(n - 1, 0, -2)], constraint=bits(8, 31))
    return out


# ------------------------------------------------------------------ counting once
COUNT_KS = (1, 100, 256, 257, 3000)


@functools.lru_cache(maxsize=None)
def counting_cases() -> List[Case]:
    """3 * 2048 + 1 rows under a site filter admitting a third, at every k around SCORE_SMALL; and
    600 rows of one score under a constraint (more than SCORE_SMALL keys tie at the cut)"""
    n = 3 * CHUNK + 1
    g = hostile(n, 18)     # three hosts, drawn uniformly
    t = term("counting", 0)
    lists = {t: g.rows}
    out = [_case("counting/k%d" % k, lists, [t], [], dict(sitehash=b"hostAB"), g, k) for k in COUNT_KS]
    rng = np.random.default_rng(19)
    z = rng.choice(np.array([0, 1 << 3, (1 << 3) | (1 << 7), (1 << 3) | (1 << 8), (1 << 7) | (1 << 8)], dtype=np.int64), 600)
    tied = plain(600, [b"tiedAA"] * 600, z=z, salt=1)     # flags 3, 7, 8 are not scored
    t2 = term("counting", 1)
    zero = jl.RankingProfile()
    zero.all_zero()
    out.append(_case("counting/tied_cut", {t2: tied.rows}, [t2], [], dict(constraint=bits(3)), tied, 100, profile=zero))
    return out


# ------------------------------------------------------------------ threshold under a filter
REJ, ADM = b"reject", b"admitA"


def _threshold_gen(admit_from: int, every: int, seed: int, salt: int) -> Gen:
    """6145 rows: the first 2048 in list order score highest, every `every`-th row from position
    admit_from on is on the admitted host and these score lowest of all"""
    n = 3 * CHUNK + 1
    rng = np.random.default_rng(seed)
    pos = np.arange(n)
    adm = (pos >= admit_from) & ((pos - admit_from) % every == 0)
    adm[n - 1] = True                          # the one-row tail chunk holds an admitted row too
    r = np.empty(n, dtype=np.int64)
    r[:CHUNK] = n - 1 - pos[:CHUNK]
    na = int(adm.sum())
    r[adm] = rng.permutation(na)
    rest = ~adm & (pos >= CHUNK)
    r[rest] = na + rng.permutation(int(rest.sum()))
    host = np.where(adm[:, None], _lang(ADM), _lang(REJ))
    return designed(r, host.astype(np.uint8), salt=salt)


@functools.lru_cache(maxsize=None)
def threshold_cases() -> List[Case]:
    out = []
    for j, (name, start, every) in enumerate((("spread", CHUNK, 13), ("last_chunk", 2 * CHUNK, 7))):
        g = _threshold_gen(start, every, 20 + j, 2 + j)
        t = term("threshol", j)
        for k in (10, 100):
            out.append(_case("threshold/%s_k%d" % (name, k), {t: g.rows}, [t], [], dict(sitehash=ADM), g, k,
                             profile=score_profile()))
    return out


# ------------------------------------------------------------------ normalisation
NORM_RULES = ("doublecheck", "constraint", "site")


@functools.lru_cache(maxsize=None)
def norm_cases() -> List[Case]:
    """per min/max column: values 10..20 on the admitted rows, 0 and 200 on two rows only, which
    the rule rejects; `twin` is the query over the list without the two"""
    n, lo, hi = 60, 17, 41
    out = []
    j = 0
    for col in ar.MINMAX_COLS:
        v = 10 + (np.arange(n, dtype=np.int64) * 7) % 11
        v[lo], v[hi] = 0, 200
        z = np.full(n, (1 << 5) | (1 << 24), dtype=np.int64)
        z[[lo, hi]] = 1 << 24
        hosts = [b"normAA", b"normAB", b"normAC"]
        host = [hosts[i % 3] for i in range(n)]
        host[lo] = host[hi] = b"extrem"
        g = plain(n, host, z=z, salt=4, **{col: v})
        urls = g.urls
        keep = np.ones(n, dtype=bool)
        keep[[lo, hi]] = False
        g2 = g.take(keep)
        for rule in NORM_RULES:
            kw = {"doublecheck": dict(urlhashes=[urls[hi], urls[lo]]), "constraint": dict(constraint=bits(5)),
                  "site": dict(siteexcludes=[b"extrem"])}[rule]
            t, t2 = term("norm", 2 * j), term("norm", 2 * j + 1)
            j += 1
            twin = _case("norm/%s_%s_without" % (col, rule), {t2: g2.rows}, [t2], [], kw, g2, 100,
                         vacuous="everything")
            out.append(_case("norm/%s_%s" % (col, rule), {t: g.rows}, [t], [], kw, g, 100, twin=twin))
    return out


# ------------------------------------------------------------------ joins
def _universe(n, seed, fracs, family, hosts):
    """lists over one universe of n urls; a url carries other cells in each list but the same
    flags, doctype and language (whichever side a join keeps, the filters see the same)"""
    rng = np.random.default_rng(seed)
    pool = _lang(b"".join(hosts)).reshape(-1, 6)
    uni = hostile(n, seed, host=pool[rng.integers(0, len(pool), n)])
    lists, sels = {}, []
    for j, frac in enumerate(fracs):
        r = ar.adv_rows(n, seed + 100 + j, "edge")
        r[:, :12] = uni.rows[:, :12]
        r = _stamp(r, uni.z, uni.d, uni.l, uni.host).rows
        sel = rng.random(n) < frac
        sels.append(sel)
        lists[term(family, j)] = r[sel]
    return uni, lists, sels


@functools.lru_cache(maxsize=None)
def join_cases() -> List[Case]:
    hosts = [b"joinAA", b"joinAB", H_ZERO, H_TOP, b"joinAC"]
    uni, lists, (sa, sb, sc) = _universe(400, 21, (0.9, 0.5, 0.3), "joins", hosts)
    ta, tb, tc = (term("joins", j) for j in range(3))
    urls = uni.urls
    kw = dict(constraint=bits(20, 24, 31), siteexcludes=[H_TOP, b"joinAB", H_TOP],
              urlhashes=[urls[j] for j in range(0, 400, 5)])
    keep = sa & sb & ~sc
    out = [_case("joins/probe_ratio_%s" % pr, lists, [ta, tb], [tc], kw, uni, 50, keep=keep,
                 env={"YRWI_PROBE_RATIO": pr}) for pr in ("1", "1000000000")]
    c5 = jl.RankingProfile.parse("", "date=15,domlength=15,authority=13,tf=10")
    out.append(_case("joins/authority_site", lists, [ta], [], dict(sitehash=b"joinAA", alt_sitehash=H_ZERO), uni, 100,
                     keep=sa, profile=c5))
    out.append(_case("joins/authority_join_excludes", lists, [tb, ta], [], dict(siteexcludes=[b"joinAC", H_ZERO]), uni,
                     100, keep=sa & sb, profile=c5))
    return out


# ------------------------------------------------------------------ one batch of 300 queries
@functools.lru_cache(maxsize=None)
def batch_case() -> Batch:
    hosts = [b"batcAA", b"batcAB", H_ZERO, H_TOP, b"batcAC", b"batcAD"]
    n = 120
    uni, lists, (sa, sb, sc) = _universe(n, 22, (0.9, 0.6, 0.3), "batch", hosts)
    ta, tb, tc = (term("batch", j) for j in range(3))
    urls = uni.urls
    shapes = [([ta], [], sa), ([tb], [], sb), ([ta, tb], [], sa & sb), ([ta], [tc], sa & ~sc),
              ([tb, ta], [tc], sa & sb & ~sc)]
    pool = ([dict(constraint=bits(j)) for j in (0, 7, 8, 23, 31)] +
            [dict(constraint=bits(7, 8), all_of_constraint=True), dict(constraint=bits()),
             dict(constraint=bits(), all_of_constraint=True)] +
            [dict(contentdom=c, strict_contentdom=s) for c in (1, 2, 3, 4) for s in (False, True)] +
            [dict(language=f) for f in ("en", "EN", "eng")] +
            [dict(sitehash=H_ZERO), dict(sitehash=b"batcAA", alt_sitehash=H_TOP), dict(alt_sitehash=b"batcAB"),
             dict(sitehash=b"batcAC", siteexcludes=[b"batcAC"]), dict(siteexcludes=[H_TOP, b"batcAD", H_ZERO]),
             dict(siteexcludes=_unsorted(_fillers(300, 23) + [b"batcAB"], 9, 7)), dict(sitehash=b"batc!A")] +
            [dict(urlhashes=[urls[0], urls[-1]]), dict(urlhashes=list(reversed(urls))),
             dict(urlhashes=urls[::2], language="en", constraint=bits(20, 21, 22)),
             dict(urlhashes=urls[1::3], siteexcludes=[b"batcAA"], contentdom=1)])
    qs = []
    for i in range(300):
        inc, exc, keep = shapes[i % len(shapes)]
        k = (10, 100, 37, 300)[(i // 3) % 4]
        if i % 3 == 0:
            adm = frozenset(u for u, a in zip(urls, keep) if a)
            qs.append(Case("batch/%d_plain" % i, lists, inc, exc, None, k, adm, None, int(keep.sum())))
            continue
        kw = dict(pool[(i - i // 3) % len(pool)])
        if i == 101:                               # the same filtered query twice, side by side
            inc, exc, keep = shapes[100 % len(shapes)]
            kw, k = dict(qs[100].kw), qs[100].k
        qs.append(_case("batch/%d" % i, lists, inc, exc, kw, uni, k, keep=keep))
    return Batch("batch/300", lists, qs)


# ------------------------------------------------------------------ doubledom
def letter_host(c: str) -> bytes:
    return b"ddh" + c.encode() * 2 + b"A"


def _mix64(z: int) -> int:
    m = (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def slot_zero_host() -> bytes:
    """a host whose 36-bit key, hashed as it is, falls on k_pull's slot 0 -- where key 0 (host
    AAAAAA) would sit, unclaimed, if the table did not store key + 1"""
    k = next(k for k in range(1 << 20, 1 << 21) if _mix64(k) & (DD_SLOTS - 1) == 0)
    assert _mix64(0) == 0
    return enc(k, 6)


def _dd(name, rank_hosts: List[bytes], k, seed, pattern=None, pulled=None, kw=None, lang_by_rank=None,
        family_j=0) -> Case:
    """rows in a shuffled list order whose stack order (rank 0 first) carries rank_hosts"""
    n = len(rank_hosts)
    rng = np.random.default_rng([seed, n])
    perm = rng.permutation(n)                  # list position of rank i
    r = np.empty(n, dtype=np.int64)
    r[perm] = n - 1 - np.arange(n)
    host = np.empty((n, 6), dtype=np.uint8)
    host[perm] = _as_hosts(rank_hosts, n)
    l = np.empty((n, 2), dtype=np.uint8)
    l[perm] = _lang(b"en") if lang_by_rank is None else lang_by_rank
    z = rng.integers(0, 1 << 17, n, dtype=np.int64) << 1    # flags 1..17: counted, not scored
    g = designed(r, host, z=z, l=l, salt=5)
    t = term("doubledo", family_j)
    kw = dict(kw or {}, skip_double_dom=True)
    c = _case("doubledom/" + name, {t: g.rows}, [t], [], kw, g, k, profile=score_profile(), pattern=pattern,
              pulled=pulled)
    byrank = [bytes(h) for h, u in zip(_as_hosts(rank_hosts, n), g.rows[perm][:, :12]) if bytes(u) in c.admitted]
    c.stack_hosts = byrank
    return c


def _pat(name, pattern, k, j, pulled=None, hosts=None) -> Case:
    hosts = hosts or {}
    rank_hosts = [hosts.get(ch, letter_host(ch)) for ch in pattern]
    return _dd(name, rank_hosts, k, 30 + j, pattern=pattern, pulled=pulled, family_j=j)


@functools.lru_cache(maxsize=None)
def doubledom_cases() -> List[Case]:
    out = []
    js = {}

    def pat(name, pattern, k, pulled=None, hosts=None):
        j = js.setdefault((pattern, id(hosts)), len(js))   # one list per pattern, whatever the k
        out.append(_pat(name, pattern, k, j, pulled, hosts))

    # SearchEvent.java:1297-1394 by hand.  A round polls up to 10 entries and returns the first of
    # a fresh host; a round without one returns the head of the FIFO of queued doubles.
    pat("AABACB", "AABACB", 6, "ABCAAB")
    pat("AABACB_short_stack", "AABACB", 10, "ABCAAB")
    pat("AABACB_k1", "AABACB", 1, "A")
    pat("twelve_A_then_B", "A" * 12 + "B", 13, "AAB" + "A" * 10)
    # 9 doubles: B is the round's 10th poll and comes out ahead of every queued A
    pat("run9", "A" + "A" * 9 + "B", 11, "AB" + "A" * 9)
    # 10 doubles fill a round: one queued A comes out, the next round reaches B
    pat("run10", "A" + "A" * 10 + "B", 12, "AAB" + "A" * 9)
    pat("run11", "A" + "A" * 11 + "B", 13, "AAB" + "A" * 10)
    # A's only double leaves the FIFO after ten B doubles: A drains, leaves the cache, and the A
    # at rank 13 is fresh again (ahead of the queued Bs); the last A is a double once more
    pat("returning_host", "AAB" + "B" * 10 + "AA", 15, "ABAA" + "B" * 10 + "A")
    pat("run9_10_11_chained", "A" + "A" * 9 + "B" + "B" * 10 + "C" + "C" * 11 + "D" + "AD", 40)
    # host keys 0 and 2^36 - 1; X hashes to slot 0 of the host table as an unshifted key 0 would
    special = {"A": H_ZERO, "Z": H_TOP, "X": slot_zero_host()}
    pat("zero_key_and_slot_zero_host", "A" + "A" * 9 + "X", 11, "AX" + "A" * 9, special)
    pat("zero_top_slot_zero_mixed", "AXZAZXBAXZZAB" * 3, 39, None, special)
    rng = np.random.default_rng(31)
    few = "".join("ABCDEFGH"[int(x)] for x in np.minimum(rng.integers(0, 12, MAX_K), 7))   # uneven
    for k in (1, 10, MAX_K):
        pat("eight_hosts_3000_k%d" % k, few, k)
    pat("one_host_3000", "A" * MAX_K, MAX_K)
    pat("one_host_3000_k10", "A" * MAX_K, 10)
    distinct = [enc(7 + 5 * i, 5) + b"A" for i in range(MAX_K)]
    distinct[3], distinct[1500], distinct[2999], distinct[40] = H_ZERO, H_TOP, slot_zero_host(), enc(1, 6)
    assert len(set(distinct)) == MAX_K
    out.append(_dd("distinct_hosts_3000", distinct, MAX_K, 32, family_j=20))
    out.append(_dd("distinct_hosts_3000_k10", distinct, 10, 32, family_j=20))
    over = "".join("ABCDE"[int(x)] for x in rng.integers(0, 5, 3500))
    out.append(_pat("stack_cut_3500", over, MAX_K, 21))
    out.append(_pat("stack_cut_3500_k100", over, 100, 21))
    # with a language filter: every third rank is "de" and never reaches the stack
    n = 400
    hosts = [letter_host("ABCDE"[int(x)]) for x in np.minimum(rng.integers(0, 8, n), 4)]
    langs = np.where((np.arange(n) % 3 == 2)[:, None], _lang(b"de"), _lang(b"en")).astype(np.uint8)
    c = _dd("language_filter", hosts, 100, 33, kw=dict(language="en"), lang_by_rank=langs, family_j=22)
    c.pattern = "".join(chr(h[3]) for h in c.stack_hosts)
    out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def doubledom_batch() -> Batch:
    """a doubledom query and a plain query with k = 10 in one call (the stacks are then MAX_K deep)"""
    dd = next(c for c in doubledom_cases() if c.name == "doubledom/eight_hosts_3000_k10")
    plain_q = Case("doubledom/plain_k10_beside", dd.lists, dd.include, [], None, 10, dd.admitted, None, dd.container,
                   profile=dd.profile)
    filt = Case("doubledom/site_k10_beside", dd.lists, dd.include, [],
                dict(sitehash=letter_host("C")), 10,
                frozenset(u for u in dd.admitted if u[6:12] == letter_host("C")), dd.flagcount, dd.container,
                profile=dd.profile)
    return Batch("doubledom/with_plain", dd.lists, [dd, plain_q, filt, dd])


FAMILIES = {"flags": flag_cases, "contentdom": contentdom_cases, "language": language_cases, "site": site_cases,
            "doublecheck": doublecheck_cases, "counting": counting_cases, "threshold": threshold_cases,
            "norm": norm_cases, "joins": join_cases, "doubledom": doubledom_cases}
BATCHES = {"batch": batch_case, "doubledom_batch": doubledom_batch}


def names(family: str) -> List[str]:
    return [c.name for c in FAMILIES[family]()]


def case(family: str, name: str) -> Case:
    return next(c for c in FAMILIES[family]() if c.name == name)


def family_lists(family: str) -> Dict[bytes, np.ndarray]:
    """every list of the family's cases (and of their twins): what one device index holds"""
    out = {}
    for c in FAMILIES[family]():
        for x in (c, c.twin):
            if x is not None:
                for h, rows in x.lists.items():
                    assert h not in out or np.array_equal(out[h], rows), (family, h)
                    out[h] = rows
    return out
