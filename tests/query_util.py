"""Shared helpers of the GPU parity tests of the query path: profiles and raw query descriptors, hits
as raw records from the library and from the oracle, and the comparison of hits and of their rows.

A plain module (no fixtures, no tests): pytest does not rewrite its asserts, so each one carries its
operands in its message."""

import ctypes

import numpy as np

import java_literal as jl
import oracle as orc
from adv_rows import adv_rows
from yacy_search_server_amd import RankingProfile
from yacy_search_server_amd._lib import CQuery

DAY = 86400000
NOW = 20741 * DAY + 4242
INF = 2147483647
HIT = 24  # sizeof(yrwi_hit) == sizeof(YoHit): urlhash[12], int32 tiebreak, int64 score


# ------------------------------------------------------------------ inputs
def profiles():
    c5 = jl.RankingProfile.parse("", "date=15,domlength=15,authority=13,tf=10")
    date = jl.RankingProfile()
    date.all_zero()
    date.coeff_date = 15
    rng = np.random.default_rng(3)
    rnd = jl.RankingProfile()
    for _, f in jl.PROFILE_FIELDS:
        setattr(rnd, f, int(rng.integers(0, 16)))
    rnd.coeff_urlcomps = 27
    return [("default", jl.RankingProfile()), ("c5", c5), ("date", date), ("rand", rnd)]


def collision_family(base, n_blocks=6):
    """64 url hashes with one Java hashCode: 6 two-char blocks, each either
    (x, y) or (x + 1, y - 31) -- equal 31 * x + y."""
    out = []
    for m in range(1 << n_blocks):
        h = bytearray(base[:12 - 2 * n_blocks])
        for j in range(n_blocks):
            x, y = base[12 - 2 * n_blocks + 2 * j], base[12 - 2 * n_blocks + 2 * j + 1]
            h += bytes([x + 1, y - 31]) if (m >> j) & 1 else bytes([x, y])
        out.append(bytes(h))
    return out


def restrict(d, sel):
    """ReferenceContainerCache.get(key, urlselection) (ReferenceContainerCache.java:448-470) for
    every list: the rows whose url hash is in the selection, in their order; an emptied list is
    what searchConjunction treats as absent (AbstractIndex.java:118-121)."""
    s = set(sel)
    out = {}
    for h, rows in d.items():
        r = rows[np.fromiter((bytes(x[:12]) in s for x in rows), dtype=bool, count=len(rows))]
        if len(r):
            out[h] = r
    return out


def hand_list(n, seed, hashes=None):
    """n rows with nonzero typeofword (g) and reserve (k) bytes and a freshUntil (s) that is
    not lastModified + 2 (today - lastModified)."""
    rows = adv_rows(n, seed, "edge")
    if hashes is not None:
        rows[:, :12] = hashes
    a = (rows[:, 12].astype(np.int64) << 8) | rows[:, 13]
    today = NOW // DAY
    fresh = np.maximum(a + 2 * (today - a), 0) & 0xFFFF
    s = (fresh + 1 + (np.arange(n) % 7)) & 0xFFFF  # never the recomputed value
    rows[:, 14], rows[:, 15] = s >> 8, s & 0xFF
    assert (rows[:, 28] != 0).all() and (rows[:, 39] != 0).all(), (n, seed, "a zero typeofword or reserve byte")
    stored = (rows[:, 14].astype(np.int64) << 8) | rows[:, 15]
    assert (stored != fresh).all(), (n, seed, int((stored == fresh).sum()), "rows hold the recomputed freshUntil")
    return rows


def cqueries(batch):
    """the queries as an array of yrwi_query_desc, for the raw entry points; keep `keep` alive with it"""
    arr = (CQuery * len(batch))()
    keep = []
    for i, q in enumerate(batch):
        ib = ctypes.create_string_buffer(b"".join(q.include), max(1, 12 * len(q.include)))
        eb = ctypes.create_string_buffer(b"".join(q.exclude), max(1, 12 * len(q.exclude)))
        prof = RankingProfile()
        keep += [ib, eb, prof]
        arr[i].incl = ctypes.cast(ib, ctypes.c_void_p)
        arr[i].nincl = len(q.include)
        arr[i].excl = ctypes.cast(eb, ctypes.c_void_p)
        arr[i].nexcl = len(q.exclude)
        arr[i].max_distance = q.max_distance
        arr[i].k = q.k
        arr[i].profile = ctypes.pointer(prof.c)
        arr[i].language = b"en"
        arr[i].now_ms = q.now_ms
    return arr, keep


# ------------------------------------------------------------------ hits as raw records
def decode(raw):
    a = np.frombuffer(raw, dtype=np.dtype([("h", "S12"), ("t", "<i4"), ("s", "<i8")]))
    return [(bytes(x["h"]).ljust(12, b"\0"), int(x["s"]), int(x["t"])) for x in a]


def orc_raw(d, inc, exc, prof, lang, now, k, md=INF):
    """orc.search's hits as the raw 24-byte records (no per-hit Python objects)."""
    lib = orc.load()
    ip, k1 = orc._lists([(h, d.get(h)) for h in inc])
    ep, k2 = orc._lists([(h, d.get(h)) for h in exc])
    out = (orc.YoHit * max(1, k))()
    n = ctypes.c_int32(0)
    rc = lib.yo_search(ip, len(inc), ep, len(exc), md, ctypes.byref(prof), lang.encode(), now, k, out,
                       ctypes.byref(n), None, None)
    assert rc == 0, ("yo_search", rc)
    return bytes(memoryview(out).cast("B")[:n.value * HIT])


def gpu_raw(ix, queries, stats=None):
    """search_batch's hits as raw records, one bytes object per query."""
    arr, keep, hits, nout, kmax = ix._marshal(queries, None)
    ix.search_batch_raw(arr, len(queries), kmax, hits, nout, stats)
    mv = memoryview(hits).cast("B")
    return [bytes(mv[i * kmax * HIT:(i * kmax + nout[i]) * HIT]) for i in range(len(queries))]


def same_hits(got, exp, ctx):
    if got == exp:
        return
    g, e = decode(got), decode(exp)
    i = next((j for j, (a, b) in enumerate(zip(g, e)) if a != b), min(len(g), len(e)))
    assert False, (ctx, "hits", len(g), len(e), "first difference at", i, g[i:i + 2], e[i:i + 2])


# ------------------------------------------------------------------ hits with their rows
def row_map(rows):
    m = {bytes(r[:12]): bytes(r) for r in rows}
    assert len(m) == len(rows), ("a url hash twice among the rows", len(m), len(rows))
    return m


def same_rows(got, exp_hits, exp_rows, ctx):
    """got: Hits with rows; exp_hits: [(urlhash, score, tiebreak)]; exp_rows: the oracle's joined container"""
    assert [(h.urlhash, h.score, h.tiebreak) for h in got] == list(exp_hits), (ctx, "hits")
    m = row_map(exp_rows)
    for i, h in enumerate(got):
        assert h.row is not None and len(h.row) == 40, (ctx, i)
        assert h.row == m[h.urlhash], (ctx, "row of hit", i, h.urlhash)
