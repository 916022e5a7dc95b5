"""Inputs shared by test_event_local_ref.py (CPU: the oracle alone shows that these inputs
exercise the cases) and test_gpu_event_local.py (GPU: yrwi_event_add_local / yrwi_event_rows
against the host path and the oracle).

A shape names a preset, include and exclude terms by size rank, and the rows its container
has before and after the exclusion (asserted against the oracle by the CPU test).

arrivals() and check_event() are the random arrival sequences and the event check of
tests/test_events.py, kept here for the other tests that feed events."""

import functools

import numpy as np

import java_literal as jl
import oracle as orc
from yacy_search_server_amd import QueryFilter, RankingProfile, synth

DAY = 86400000
NOW = 20741 * DAY + 31337
NOWS = (NOW, 15500 * DAY + 7)  # two request times: the re-encoded freshUntil differs
INF = 2147483647
ABSENT = b"ABSENTterm__"       # a well-formed term hash no preset has

# name: (preset, include ranks, exclude ranks, joined rows, rows after exclusion)
SHAPES = {
    "dense_inc3_exc1": ("dense", (0, 1, 2), (3,), 6400, 667),   # heavy removal over every tile, > 1 EV_CH chunk
    "dense_inc2": ("dense", (0, 1), (), 6400, 6400),            # 7 chunks of k_event_add
    "tiny_inc1_exc1": ("tiny", (0,), (1,), 5984, 5835),         # rows as stored, scattered removal
    "tiny_inc2": ("tiny", (0, 1), (), 149, 149),                # under one tile
}
EMPTY_SHAPES = {
    "dense_all_excluded": ("dense", (0, 1), (2,), 6400, 0),
    "dense_absent_include": ("dense", (0, None), (), 0, 0),
}
PROFILES = {
    "default": {},
    "authority": {"coeff_authority": 14, "coeff_worddistance": 15},
    "date": None,  # the "/date" modifier: every coefficient 0, coeff_date 15
}
KS = (10, 100, 3000)


@functools.lru_cache(maxsize=None)
def corpus(preset):
    cfg = synth.preset(preset)
    idx = synth.build_index(cfg)
    order = [int(t) for t in np.argsort(-idx.sizes, kind="stable")]
    return cfg, idx, idx.as_dict(), order


def terms(shape):
    preset, inc, exc, _, _ = {**SHAPES, **EMPTY_SHAPES}[shape]
    _, idx, _, order = corpus(preset)
    h = lambda r: ABSENT if r is None else idx.hashes[order[r]]
    return preset, [h(r) for r in inc], [h(r) for r in exc]


@functools.lru_cache(maxsize=None)
def container(shape, now=NOW):
    """the oracle's joined and excluded container of the shape, (m, 40) uint8"""
    preset, inc, exc = terms(shape)
    return orc.term_search(corpus(preset)[2], inc, exc, INF, now)


def jl_profile(pname):
    p = jl.RankingProfile()
    if PROFILES[pname] is None:
        p.all_zero()
        p.coeff_date = 15
    else:
        for f, v in PROFILES[pname].items():
            setattr(p, f, v)
    return p


def rows_list(a):
    return [bytes(r) for r in np.asarray(a, dtype=np.uint8).reshape(-1, 40)]


def arrivals(idx, rng, n_remote, local_term=None, zero_pos=False, big=False):
    """local container (a whole posting list, sorted) + remote containers built
    from random rows of random lists (same url under other words: different
    features), shuffled (arrival order), with duplicates inside an arrival."""
    out = []
    if local_term is not None:
        out.append((np.array(idx.list_rows(local_term)), True))
    all_rows = np.asarray(idx.rows, dtype=np.uint8)
    for _ in range(n_remote):
        m = int(rng.integers(0, 3000 if big else 200))
        take = rng.integers(0, len(all_rows), m)
        if m > 4:
            take[: m // 4] = take[rng.integers(0, m, m // 4)]  # duplicates inside the arrival
        r = all_rows[take].copy()
        if m:  # word distances (the 'i' column), so the max-distance fold has work
            d = rng.random(m) < 0.5
            r[d, 38] = rng.integers(0, 40, int(d.sum()))
        if zero_pos and m:
            z = rng.random(m) < 0.3
            r[z, 34] = 0
            r[z, 35] = 0
        out.append((r, False))
    return out


def remote_arrivals(preset, seed, n_remote=6):
    """n_remote remote containers built as arrivals() builds them (big)"""
    return [r for r, _ in arrivals(corpus(preset)[1], np.random.default_rng(seed), n_remote, big=True)]


def check_event(ix, arrivals, profile_fields=None, kw=None, k=100, language="en"):
    """the arrivals into one event of the index and into java_literal.SearchEventRWI: the stack, the
    tiebreaks and every yrwi_event_info field must agree (a plain module: every assert names its operands)"""
    lp = jl.RankingProfile()
    gp = RankingProfile()
    for f, v in (profile_fields or {}).items():
        setattr(lp, f, v)
        setattr(gp, f, v)
    lf = jl.QueryFilter(**(kw or {}))
    gf = QueryFilter(**(kw or {})) if kw is not None else None
    ref = jl.SearchEventRWI(lp, language, NOW, filt=lf)
    total = sum(len(r) for r, _ in arrivals)
    with ix.event(gp, language, NOW, k=k, filter=gf, max_postings=total + 16) as ev:
        for rows, local in arrivals:
            ref.add_rwis(rows_list(rows), local)
            ev.add_rwis(rows, local)
        hits, info = ev.results()
    exp = ref.stack()[:k]
    got = [(h.urlhash, h.score) for h in hits]
    i = next((j for j, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
    assert got == exp, ("stack", len(got), len(exp), "first difference at", i, got[i:i + 2], exp[i:i + 2])
    ties = [h.tiebreak for h in hits]
    want = [jl.bytearray_hashcode(u) for u, _ in exp]
    assert ties == want, ("tiebreaks", [(j, a, b) for j, (a, b) in enumerate(zip(ties, want)) if a != b][:4])
    assert list(info.flagcount) == lf.flagcount, (list(info.flagcount), lf.flagcount)
    assert info.postings_in == total, (info.postings_in, total)
    assert info.admitted_remote == ref.remote_available, (info.admitted_remote, ref.remote_available)
    assert info.admitted_local == ref.local_available, (info.admitted_local, ref.local_available)
    assert info.remote_arrivals == ref.remote_peers, (info.remote_arrivals, ref.remote_peers)
    mx = ref.order.max
    assert info.max_distance == (mx.distance() if mx is not None else 0), (info.max_distance, mx and mx.distance())
    if lp.coeff_authority > 12:
        assert info.maxdomcount == ref.order.maxdomcount, (info.maxdomcount, ref.order.maxdomcount)


def info_of(ref, total):
    """the yrwi_event_info fields of a java_literal.SearchEventRWI that received `total` rows"""
    mx = ref.order.max
    return {"flagcount": list(ref.filt.flagcount), "postings_in": total, "admitted_local": ref.local_available,
            "admitted_remote": ref.remote_available, "remote_arrivals": ref.remote_peers,
            "max_distance": mx.distance() if mx is not None else 0, "maxdomcount": ref.order.maxdomcount,
            "err": 0, "stack_size": len(ref.stack())}


def info_dict(info, authority):
    d = {"flagcount": list(info.flagcount), "postings_in": info.postings_in, "admitted_local": info.admitted_local,
         "admitted_remote": info.admitted_remote, "remote_arrivals": info.remote_arrivals,
         "max_distance": info.max_distance, "maxdomcount": info.maxdomcount, "err": info.err,
         "stack_size": info.stack_size}
    if not authority:  # ReferenceOrder counts hosts for every profile; the device only when authority reads them
        d.pop("maxdomcount")
    return d
