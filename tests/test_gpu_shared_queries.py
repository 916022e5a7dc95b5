"""GPU parity (MI355X) of shared queries: identical queries of one pass of a batch part run
once and every copy gets the first occurrence's hits and rows (csrc/yrwi_share.h).

One batch of 64 queries per preset holds repeats of every kind (reordered and duplicated terms,
a missing term, one, two and three include terms, an exclusion, a quoted query) next to
near-copies that must not share (k, profile, language, now_ms, max_distance, exclude list,
a filter).  Expected hits come from the oracle alone; YRWI_SHARE=0 runs every query and must
give the same bytes; the number of shared queries is counted here from the queries themselves.

`dense`: its two largest lists join to 6400 rows (4 rank chunks: the multi-chunk score and
k_topq paths); `tiny`: its largest pairs join to 149 and 65 rows (n > k and n <= k, one chunk)."""

import os

import numpy as np
import pytest

import java_literal as jl
import oracle as orc
from index_util import run_parts
from yacy_search_server_amd import Query, QueryFilter, RankingProfile, RWIIndex, synth
from yacy_search_server_amd._lib import CStats

pytestmark = pytest.mark.gpu

DAY = 86400000
NOW = 20741 * DAY + 777
INF = 2147483647
MISSING = b"NOSUCHTERM__"
FILTER_KW = dict(constraint=b"\0\0\x10\x01")
NQ = 64


class _Env:
    """an environment variable for the length of a with block (the library reads both per call)"""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        os.environ[self.name] = self.value

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


def _make_batch(idx):
    """-> [Query]; every call builds its own filter objects (their flag counts are outputs)"""
    order = [int(t) for t in np.argsort(-idx.sizes, kind="stable")]
    a, b, c, d, e = (idx.hashes[t] for t in order[:5])
    alt = RankingProfile("", "date=15,domlength=15,tf=10")

    def q(inc, exc=(), **kw):
        kw.setdefault("k", 100)
        kw.setdefault("now_ms", NOW)
        return Query(list(inc), list(exc), **kw)

    head = [
        q([a, b]),                                    # 0: the first occurrence
        q([a, b], k=99),                              # near-copies of it: each differs in one field
        q([a, b], profile=alt),
        q([a, b], language="de"),
        q([a, b], now_ms=NOW + DAY),
        q([a, b], max_distance=1),
        q([a, b], [e]),
        q([a, b], max_distance=1),                    # repeats of the quoted one and of the exclusion
        q([b, a], [e]),
        q([b, c], filter=QueryFilter(**FILTER_KW)),   # a pair with a filter: never shared
        q([b, c], filter=QueryFilter(**FILTER_KW)),
        q([b, c]),                                    # the same terms without one: shared among themselves
        q([c, b]),
        q([a, MISSING]),                              # a missing term: 0 hits, repeated
        q([MISSING, a]),
        q([a, b, c]),                                 # three terms, repeated in another order
        q([c, a, b]),
        q([a]),                                       # one list (its stored rows), repeated
        q([a, a]),
    ]
    rest = [q([idx.hashes[t] for t in inc], [idx.hashes[t] for t in exc])
            for inc, exc in synth.queries(idx.cfg, NQ - len(head) - 2, 1, 4, 1, qseed=911)]
    mid = len(rest) // 2
    batch = head + rest[:mid] + [q([b, a])] + rest[mid:] + [q([a, b, a])]  # ... a middle and the last one
    assert len(batch) == NQ
    return batch


def _key(q):
    """what makes two queries one (None: never shared)"""
    if q.filter is not None or q.urlselection is not None:
        return None
    p = q.profile or RankingProfile()
    return (frozenset(q.include), frozenset(q.exclude), q.max_distance, q.k,
            tuple(getattr(p, f) for _, f in jl.PROFILE_FIELDS), q.language, q.now_ms)


def _shared(batch, parts=1):
    """queries with an identical earlier one in their batch part (parts: the lanes a
    synchronous call splits the batch over, contiguous and equal in count)"""
    nq = len(batch)
    nl = min(parts, nq)
    n = 0
    for l in range(nl):
        seen = set()
        for q in batch[nq * l // nl:nq * (l + 1) // nl]:
            k = _key(q)
            if k is not None and k in seen:
                n += 1
            elif k is not None:
                seen.add(k)
    return n


def _lanes():
    return max(1, min(16, int(os.environ.get("YRWI_LANES", "8"))))


def _triples(hits):
    return [(h.urlhash, h.score, h.tiebreak) for h in hits]


def _submit(ix, batch, stats=True, rows=False):
    """the whole batch as one part on one lane (yrwi_query_batch[_rows]_submit + wait)
    -> (hits per query, CStats or None)"""
    nq = len(batch)
    arr, keep, hits, nout, kmax = ix._marshal(batch, None)
    st = CStats() if stats else None
    rbuf = np.full((nq * kmax, 40), 0xA5, dtype=np.uint8) if rows else None
    t = ix.submit_rows_raw(arr, nq, kmax, hits, rbuf, nout, st) if rows else ix.submit_raw(arr, nq, kmax, hits, nout, st)
    ix.wait(t)
    return RWIIndex._unmarshal(nq, kmax, hits, nout, rbuf), st


@pytest.fixture(scope="module", params=["dense", "tiny"])
def corpus(request):
    """the index, one context holding it, and the oracle's hits of the batch (computed once)"""
    idx = synth.build_index(synth.preset(request.param))
    d = idx.as_dict()
    ix = RWIIndex(0)
    for h, rows in d.items():
        ix.add(h, rows)
    batch = _make_batch(idx)
    lit = None
    exp, flags = [], []
    for q in batch:
        if q.filter is None:
            prof = orc.profile_from(q.profile) if q.profile is not None else None
            exp.append(orc.search(d, q.include, q.exclude, prof, q.language, q.max_distance, q.now_ms, q.k))
            flags.append(None)
        else:
            lit = lit or {h: [bytes(x) for x in rows] for h, rows in d.items()}
            lf = jl.QueryFilter(**FILTER_KW)
            e = jl.search(lit, q.include, q.exclude, jl.RankingProfile(), q.language, q.max_distance, q.now_ms, q.k, lf)
            exp.append(e)
            flags.append(lf.flagcount)
    yield request.param, idx, d, ix, exp, flags
    ix.close()


def _check(batch, got, exp, flags, ctx):
    for qi, (q, g, e) in enumerate(zip(batch, got, exp)):
        if q.filter is None:
            assert _triples(g) == e, (ctx, qi)
        else:
            assert [(h.urlhash, h.score) for h in g] == e, (ctx, qi)
            assert q.filter.flagcount == flags[qi], (ctx, qi, "flagcount")


def test_batch_layout(corpus):
    """the batch holds what the module's text promises, at the sizes that take each path"""
    name, idx, d, ix, exp, flags = corpus
    batch = _make_batch(idx)
    n0 = len(orc.term_search(d, batch[0].include, [], INF, NOW))
    n1 = len(orc.term_search(d, batch[11].include, [], INF, NOW))
    assert (n0, n1) == {"dense": (6400, 6400), "tiny": (149, 65)}[name]
    assert _key(batch[0]) == _key(batch[NQ - 1]) and sum(_key(q) == _key(batch[0]) for q in batch) == 3
    assert sum(_key(q) == _key(batch[0]) for q in batch[20:NQ - 1]) == 1  # the middle one
    assert len({_key(q) for q in batch[:7]}) == 7  # the near-copies: seven different queries
    assert len(exp[13]) == 0 and len(exp[14]) == 0 and len(exp[0]) == 100 and len(exp[1]) == 99
    assert len(exp[9]) > 0 and exp[9] == exp[10] and sum(flags[9]) > 0
    assert _shared(batch) >= 8  # the eight repeats written out in _make_batch


def test_submit_shares_and_matches_oracle(corpus):
    """One part on one lane: every query bit-exact against the oracle and against the same batch
    with YRWI_SHARE=0; postings_in and joined equal between the two; queries_shared as counted."""
    name, idx, d, ix, exp, flags = corpus
    on_b, off_b = _make_batch(idx), _make_batch(idx)
    on, st_on = _submit(ix, on_b)
    with _Env("YRWI_SHARE", "0"):
        off, st_off = _submit(ix, off_b)
    _check(on_b, on, exp, flags, (name, "share"))
    _check(off_b, off, exp, flags, (name, "no share"))
    assert [_triples(g) for g in on] == [_triples(g) for g in off]
    want = _shared(on_b)
    assert st_on.queries_shared == want and st_off.queries_shared == 0
    assert st_on.postings_in == st_off.postings_in > 0 and st_on.joined == st_off.joined > 0
    assert st_off.postings_shared == 0 and st_off.joined_shared == 0
    # the shared queries' own postings (their lists' lengths) and joined rows (each query's, alone)
    seen, post, rows = set(), 0, 0
    for q in on_b:
        k = _key(q)
        if k is not None and k in seen:
            post += sum(len(d.get(t, ())) for t in set(q.include)) + sum(len(d.get(t, ())) for t in set(q.exclude))
            one = CStats()
            ix.search_batch([q], stats=one)
            assert one.postings_in == sum(len(d.get(t, ())) for t in set(q.include)) + \
                sum(len(d.get(t, ())) for t in set(q.exclude))
            rows += one.joined
        elif k is not None:
            seen.add(k)
    assert rows > 0
    assert st_on.postings_shared == post and st_on.joined_shared == rows
    # executed work only: a batch with repeats moves fewer bytes than the same batch run in full
    assert st_on.bytes_alg < st_off.bytes_alg and st_on.bytes_score < st_off.bytes_score


def test_submit_without_statistics(corpus):
    """the production call: submit / wait with yrwi_stats NULL"""
    name, idx, d, ix, exp, flags = corpus
    batch = _make_batch(idx)
    got, _ = _submit(ix, batch, stats=False)
    _check(batch, got, exp, flags, (name, "stats NULL"))


def test_synchronous_batch_splits_over_lanes(corpus):
    """yrwi_query_batch cuts the batch into one part per lane: only a part's own repeats share"""
    name, idx, d, ix, exp, flags = corpus
    batch = _make_batch(idx)
    st = CStats()
    got = ix.search_batch(batch, stats=st)
    _check(batch, got, exp, flags, (name, "lanes"))
    assert st.queries_shared == _shared(batch, _lanes()) > 0
    if _lanes() > 1:  # the first, the middle and the last query lie in different parts
        assert st.queries_shared < _shared(batch)


def test_rows_of_repeats(corpus):
    """yrwi_query_batch_rows(_submit): a repeat's rows are its first occurrence's, and the oracle's"""
    name, idx, d, ix, exp, flags = corpus
    batch = _make_batch(idx)
    got, st = _submit(ix, batch, rows=True)
    _check(batch, got, exp, flags, (name, "rows"))
    assert st.queries_shared == _shared(batch)
    with _Env("YRWI_SHARE", "0"):
        off, _ = _submit(ix, _make_batch(idx), rows=True)
    assert [[h.row for h in g] for g in got] == [[h.row for h in g] for g in off]
    first = {}
    nrep = 0
    for qi, q in enumerate(batch):
        k = _key(q)
        if k is None:
            continue
        if k in first:
            assert [h.row for h in got[qi]] == [h.row for h in got[first[k]]], (name, qi)
            nrep += 1
            continue
        first[k] = qi
        m = {bytes(r[:12]): bytes(r) for r in orc.term_search(d, q.include, q.exclude, q.max_distance, q.now_ms)}
        for h in got[qi]:
            assert h.row == m[h.urlhash], (name, qi)
    assert nrep == _shared(batch)
    sync = ix.search_batch(_make_batch(idx), rows=True)  # the synchronous entry point, parts per lane
    assert [[h.row for h in g] for g in sync] == [[h.row for h in g] for g in got]


def test_pass_split_between_repeats(corpus):
    """A scratch budget of 1 MiB cuts the part into passes (every query with a result is
    estimated at 64 KiB or more, so no pass holds more than 16 of them): the first and the last
    query, identical, fall into different passes and the last one runs again.  Results unchanged."""
    name, idx, d, ix, exp, flags = corpus
    batch = _make_batch(idx)
    with _Env("YRWI_SCRATCH_GB", "0.001"):
        got, st = _submit(ix, batch)
        rows, _ = _submit(ix, _make_batch(idx), rows=True)
    _check(batch, got, exp, flags, (name, "passes"))
    assert 0 < st.queries_shared < _shared(batch)
    full, _ = _submit(ix, _make_batch(idx), rows=True)
    assert [[(h.urlhash, h.score, h.tiebreak, h.row) for h in g] for g in rows] == \
           [[(h.urlhash, h.score, h.tiebreak, h.row) for h in g] for g in full]


def test_sharded_loopback_does_not_share():
    """world 2 over the loopback transport: the same batch, results as the whole index's, nothing shared"""
    world = 2
    full = synth.preset("tiny")
    whole_idx = synth.build_index(full)
    whole = whole_idx.as_dict()
    lit = {h: [bytes(x) for x in rows] for h, rows in whole.items()}
    shards = [synth.build_index(full.shard(r, world)) for r in range(world)]

    def fn(r, ix):
        batch = _make_batch(whole_idx)  # (term hashes and sizes of the whole index: the same batch on every rank)
        st = CStats()
        return batch, ix.search_batch(batch, stats=st), st

    out = run_parts([p.as_dict() for p in shards], world, fn)
    for r, (batch, got, st) in enumerate(out):
        assert st.queries_shared == 0 and st.postings_shared == 0 and st.joined_shared == 0
        for qi, (q, g) in enumerate(zip(batch, got)):
            if q.filter is None:
                prof = orc.profile_from(q.profile) if q.profile is not None else None
                e = orc.search(whole, q.include, q.exclude, prof, q.language, q.max_distance, q.now_ms, q.k)
                assert _triples(g) == e, (r, qi)
            else:
                lf = jl.QueryFilter(**FILTER_KW)
                e = jl.search(lit, q.include, q.exclude, jl.RankingProfile(), q.language, q.max_distance, q.now_ms,
                              q.k, lf)
                assert [(h.urlhash, h.score) for h in g] == e, (r, qi)
                assert q.filter.flagcount == lf.flagcount, (r, qi)
