"""GPU parity (MI355X) of device-local arrivals: yrwi_event_add_local feeds a search event the
joined and excluded container of a query straight from the device index, yrwi_event_rows
returns the retained row of an admitted posting.

The event must end in exactly the state the host path leaves (yrwi_term_search rows through
yrwi_event_add, local = 1) and the literal oracle computes (oracle.term_search rows into
java_literal.SearchEventRWI).  Every comparison is equality.  The inputs are those of
event_local_cases.py, whose coverage tests/test_event_local_ref.py asserts on the oracle."""

import numpy as np
import pytest

import event_local_cases as C
import java_literal as jl
import oracle as orc
from index_util import open_index, run_parts
from query_util import hand_list
from yacy_search_server_amd import Query, QueryFilter, RankingProfile, synth
from yacy_search_server_amd._lib import CLocalStats, YrwiError, lib

pytestmark = pytest.mark.gpu

NOW, INF = C.NOW, C.INF
E_ARG, E_HASH, E_UNSUPPORTED, E_CAPACITY = -1, -2, -8, -10


@pytest.fixture(scope="module")
def indexes():
    ixs = {p: open_index(C.corpus(p)[2], url_ids=True) for p in ("dense", "tiny")}
    yield ixs
    for ix in ixs.values():
        ix.close()


def _gpu_profile(pname):
    jp = C.jl_profile(pname)
    rp = RankingProfile()
    for _, f in jl.PROFILE_FIELDS:
        setattr(rp, f, getattr(jp, f))
    return rp


_oracle_cache = {}


def _oracle_event(shape, pname, remote_seed=None, filt_kw=None):
    """java_literal.SearchEventRWI (stack bound 3000: a smaller bound keeps a prefix) after the
    shape's container as the local arrival and, with remote_seed, six remote arrivals"""
    key = (shape, pname, remote_seed, repr(filt_kw))
    if key not in _oracle_cache:
        ref = jl.SearchEventRWI(C.jl_profile(pname), "en", NOW, filt=jl.QueryFilter(**filt_kw) if filt_kw else None)
        total = len(C.container(shape))
        ref.add_rwis(C.rows_list(C.container(shape)), True)
        if remote_seed is not None:
            for r in C.remote_arrivals(C.terms(shape)[0], remote_seed):
                ref.add_rwis(C.rows_list(r), False)
                total += len(r)
        _oracle_cache[key] = (ref, total)
    return _oracle_cache[key]


def _state(ev, authority):
    """(stack as the oracle states it, every yrwi_event_info field, the hits' tiebreaks)"""
    hits, info = ev.results()
    return [(h.urlhash, h.score) for h in hits], C.info_dict(info, authority), [h.tiebreak for h in hits]


def _expect(ref, total, k, authority):
    info = C.info_of(ref, total)
    info["stack_size"] = min(k, info["stack_size"])
    if not authority:
        info.pop("maxdomcount")
    return ref.stack()[:k], info


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("pname", list(C.PROFILES))
@pytest.mark.parametrize("shape", list(C.SHAPES) + list(C.EMPTY_SHAPES))
def test_same_state_as_host_path_and_oracle(indexes, shape, pname):
    preset, inc, exc = C.terms(shape)
    ix = indexes[preset]
    ref, total = _oracle_event(shape, pname)
    authority = C.jl_profile(pname).coeff_authority > 12
    exp_m = len(orc.term_search(C.corpus(preset)[2], inc, exc, INF, NOW))
    for k in C.KS:
        with ix.event(_gpu_profile(pname), "en", NOW, k=k, max_postings=6400 + 16) as A, \
                ix.event(_gpu_profile(pname), "en", NOW, k=k, max_postings=6400 + 16) as B:
            m = A.add_local(inc, exc, now_ms=NOW)
            assert m == exp_m, (shape, k)
            rows = ix.term_search(inc, exc, now_ms=NOW)
            assert len(rows) == exp_m
            B.add_rwis(rows, True)
            sa, sb = _state(A, authority), _state(B, authority)
            assert sa == sb, (shape, pname, k, "device-local vs host path")
            assert sa[:2] == _expect(ref, total, k, authority), (shape, pname, k, "vs oracle")
            urls = [h for h, _ in sa[0]]
            assert A.source(urls) == B.source(urls)
            if exp_m:
                assert all(a == 1 for a, _ in A.source(urls))
            else:  # the event is unchanged: no arrival number was used up
                again = ix.term_search(*C.terms("dense_inc2")[1:], now_ms=NOW)
                A.add_rwis(again, True)
                assert {a for a, _ in A.source([bytes(r[:12]) for r in again[:50]])} == {1}


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("shape", list(C.SHAPES))
def test_remote_arrivals_continue_from_the_local_state(indexes, shape, filtered):
    preset, inc, exc = C.terms(shape)
    ix = indexes[preset]
    idx = C.corpus(preset)[1]
    rng = np.random.default_rng(5)
    kw = None
    if filtered:
        kw = dict(siteexcludes=sorted({bytes(r[6:12]) for r in np.asarray(idx.rows)[rng.integers(0, len(idx.rows), 80)]}))
    ref, total = _oracle_event(shape, "authority", remote_seed=11, filt_kw=kw)
    remote = C.remote_arrivals(preset, 11)
    assert len(remote) == 6
    for k in (100, 3000):
        fa, fb = (QueryFilter(**kw) if kw else None for _ in range(2))
        with ix.event(_gpu_profile("authority"), "en", NOW, k=k, filter=fa, max_postings=total + 16) as A, \
                ix.event(_gpu_profile("authority"), "en", NOW, k=k, filter=fb, max_postings=total + 16) as B:
            A.add_local(inc, exc, now_ms=NOW)
            B.add_rwis(ix.term_search(inc, exc, now_ms=NOW), True)
            ix.add_rwis([(A, r, False) for r in remote])
            ix.add_rwis([(B, r, False) for r in remote])
            sa, sb = _state(A, True), _state(B, True)
            assert sa == sb, (shape, filtered, k)
            assert sa[:2] == _expect(ref, total, k, True), (shape, filtered, k)
            urls = [h for h, _ in sa[0]]
            assert A.source(urls) == B.source(urls)


# ------------------------------------------------------------------ 3
def test_many_events_one_call(indexes):
    ix = indexes["dense"]
    cfg, idx, d, _ = C.corpus("dense")
    qs = [([idx.hashes[t] for t in inc], [idx.hashes[t] for t in exc])
          for inc, exc in synth.queries(cfg, 40, 1, 4, 1, qseed=700)]
    assert {len(set(inc)) for inc, _ in qs} >= {1, 2, 3, 4}
    K = 100
    evs = [ix.event(None, "en", NOW, k=K, max_postings=2 * 6400 + 16) for _ in qs]
    try:
        batch, exp = [], []
        for e, (inc, exc) in enumerate(qs):
            batch.append((evs[e], Query(inc, exc, now_ms=NOW)))
            if e % 7 == 0:  # a second local container in the same call, as the sitehost retry adds one
                inc2, exc2 = qs[(e + 1) % len(qs)]
                batch.append((evs[e], Query(inc2, exc2, now_ms=NOW)))
                ref = jl.SearchEventRWI(jl.RankingProfile(), "en", NOW, maxsize=K)
                for i, x in ((inc, exc), (inc2, exc2)):
                    ref.add_rwis(C.rows_list(orc.term_search(d, i, x, INF, NOW)), True)
                exp.append(ref.stack())
            else:  # one local arrival: the canonical single-container query
                exp.append([(h, s) for h, s, _ in orc.search(d, inc, exc, now_ms=NOW, k=K)])
        st = CLocalStats()
        ms = ix.add_local_rwis(batch, st)
        assert ms == [len(orc.term_search(d, q.include, q.exclude, INF, NOW)) for _, q in batch]
        assert st.rows_arrived == sum(ms) and st.rows_joined >= st.rows_arrived
        assert sum(1 for m in ms if m == 0) < len(ms) // 2
        for e, ev in enumerate(evs):
            hits, _ = ev.results()
            assert [(h.urlhash, h.score) for h in hits] == exp[e], e
    finally:
        for ev in evs:
            ev.close()


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("shape", list(C.SHAPES))
def test_rows_of_hits_and_of_pulled_hits(indexes, shape):
    preset, inc, exc = C.terms(shape)
    ix = indexes[preset]
    for now in C.NOWS:
        exp = {bytes(r[:12]): bytes(r) for r in C.container(shape, now)}
        with ix.event(None, "en", NOW, k=3000, max_postings=6400 + 16) as ev:
            assert ev.add_local(inc, exc, now_ms=now) == len(exp)
            hits, _ = ev.results()
            assert len(hits) == min(3000, len(exp))
            urls = [h.urlhash for h in hits]
            assert ev.rows(urls) == [exp[u] for u in urls], (shape, now)
            pulled = [h.urlhash for h in ev.pull(60, skip_double_dom=True)]
            assert pulled and ev.rows(pulled) == [exp[u] for u in pulled]
            while ev.pull(3000, skip_double_dom=False):
                pass
            assert ev.results()[0] == []
            assert ev.rows(urls[:200] + pulled) == [exp[u] for u in urls[:200] + pulled]  # still in the doublecheck set
            unknown = [b"AAAAAAAAAAAA", b"zzzzzzzzzzzz"]
            assert all(u not in exp for u in unknown) and ev.rows(unknown) == [None, None]
    # the 40 bytes of a url that is not found are zero
    with ix.event(None, "en", NOW, k=10, max_postings=1024) as ev:
        out = np.full((2, 40), 0xAB, dtype=np.uint8)
        found = np.full(2, 7, dtype=np.uint8)
        assert lib().yrwi_event_rows(ix._h, ev._e, b"AAAAAAAAAAAA" + b"zzzzzzzzzzzz", 2, out.ctypes.data,
                                     found.ctypes.data) == 0
        assert not out.any() and not found.any()


def test_single_include_rows_come_back_as_stored():
    """hand-built lists with nonzero typeofword / reserve bytes and a freshUntil that is not the
    recomputed one: a single-include arrival keeps all 40 bytes, a two-term one re-encodes"""
    A, B = b"TERMrowsA___", b"TERMrowsB___"
    a = hand_list(700, 5)
    b = hand_list(700, 6, a[:, :12])[::2].copy()
    d = {A: a, B: b}
    ix = open_index(d, url_ids=True)
    try:
        with ix.event(None, "en", NOW, k=3000, max_postings=1024) as ev:
            assert ev.add_local([A], now_ms=NOW) == 700
            urls = [bytes(r[:12]) for r in a]
            assert ev.rows(urls) == [bytes(r) for r in a]
        with ix.event(None, "en", NOW, k=3000, max_postings=1024) as ev:
            exp = orc.term_search(d, [A, B], [], INF, NOW)
            assert ev.add_local([A, B], now_ms=NOW) == len(exp) == 350
            got = ev.rows([bytes(r[:12]) for r in exp])
            assert got == [bytes(r) for r in exp]
            assert all(g[28] == 0 and g[39] == 0 for g in got)
    finally:
        ix.close()


def test_found_pattern_of_a_mixed_event(indexes):
    """remote, local, remote into one event (tests/test_event_local_ref.py): a url is found only
    when the local container brought its admitted posting"""
    ix = indexes["tiny"]
    _, inc, exc = C.terms("tiny_inc1_exc1")
    first, second = C.remote_arrivals("tiny", 77, 2)
    local = C.container("tiny_inc1_exc1")
    u = lambda a: {bytes(r[:12]) for r in a}
    exp = {bytes(r[:12]): bytes(r) for r in local}
    with ix.event(None, "en", NOW, k=3000, max_postings=len(first) + len(local) + len(second) + 16) as ev:
        ev.add_rwis(first, False)
        assert ev.add_local(inc, exc, now_ms=NOW) == len(local)
        ev.add_rwis(second, False)
        shared = sorted(u(first) & u(local))
        only_local = sorted(u(local) - u(first))
        only_remote = sorted((u(first) | u(second)) - u(local))
        assert shared and only_local and only_remote
        assert ev.rows(shared) == [None] * len(shared)          # admitted from the first remote arrival
        assert ev.rows(only_remote) == [None] * len(only_remote)
        assert ev.rows(only_local) == [exp[x] for x in only_local]
        assert {a for a, _ in ev.source(only_local)} == {2} and {a for a, _ in ev.source(shared)} == {1}
    # a url the filter seeded is in the set from the start: not found, though the local container has it
    seeds = [bytes(r[:12]) for r in local[:40]]
    with ix.event(None, "en", NOW, k=100, filter=QueryFilter(urlhashes=seeds), max_postings=6400) as ev:
        ev.add_local(inc, exc, now_ms=NOW)
        assert ev.rows(seeds) == [None] * len(seeds)
        rest = [bytes(r[:12]) for r in local[40:80]]
        assert ev.rows(rest) == [exp[x] for x in rest]


# ------------------------------------------------------------------ 5
def _dense_queries():
    idx, order = C.corpus("dense")[1], C.corpus("dense")[3]
    h = lambda r: idx.hashes[order[r]]
    return [Query([h(0), h(1), h(2)], [h(3)], now_ms=NOW), Query([h(0), h(1)], now_ms=NOW),
            Query([h(0), h(1)], [h(2)], now_ms=NOW), Query([h(4)], [h(5)], now_ms=NOW)]


def _call(ix, queries, nev):
    evs = [ix.event(None, "en", NOW, k=100, max_postings=6400 + 16) for _ in range(nev)]
    try:
        st = CLocalStats()
        r0 = lib().yrwi_realloc_events()
        ms = ix.add_local_rwis([(evs[i], queries[i % len(queries)]) for i in range(nev)], st)
        return st, ms, lib().yrwi_realloc_events() - r0
    finally:
        for ev in evs:
            ev.close()


def test_cost_contract(indexes):
    """the library's own counters (no times): the tail of the call and its host waits do not
    depend on the number of arrivals, the bytes over PCIe not on the list lengths, and a call
    makes at most one device allocation (measured after a first call has sized the lane's
    scratch and staging, as for every other entry point)"""
    ix = indexes["dense"]
    qs = _dense_queries()
    _call(ix, qs, 40)  # scratch and staging reach their size
    s4, m4, r4 = _call(ix, qs, 4)
    s40, m40, r40 = _call(ix, qs, 40)
    print("arrivals 4 / 40: launches_tail", s4.launches_tail, s40.launches_tail, "syncs", s4.syncs, s40.syncs,
          "bytes", s4.bytes_h2d + s4.bytes_d2h, s40.bytes_h2d + s40.bytes_d2h, "allocs", s4.device_allocs,
          s40.device_allocs, r4, r40)
    assert m40 == m4 * 10 and s40.rows_arrived == 10 * s4.rows_arrived
    assert s4.launches_tail == s40.launches_tail and s4.syncs == s40.syncs
    assert 0 <= r4 <= 1 and 0 <= r40 <= 1 and s4.device_allocs <= 1 and s40.device_allocs <= 1
    # the same terms with every list cut to its first tenth: fewer rows, the same bytes
    tenth = open_index({h: rows[:max(1, len(rows) // 10)] for h, rows in C.corpus("dense")[2].items()},
                       url_ids=True)
    try:
        _call(tenth, qs, 4)
        t4, mt, _ = _call(tenth, qs, 4)
        print("dense / tenth: rows joined", s4.rows_joined, t4.rows_joined, "bytes h2d", s4.bytes_h2d, t4.bytes_h2d,
              "d2h", s4.bytes_d2h, t4.bytes_d2h)
        assert t4.rows_joined < s4.rows_joined // 5
        assert t4.bytes_h2d + t4.bytes_d2h == s4.bytes_h2d + s4.bytes_d2h
        assert t4.launches_tail == s4.launches_tail
    finally:
        tenth.close()
    # no row crosses: the bytes of the call are far below one row per arrived posting
    assert 10 * (s40.bytes_h2d + s40.bytes_d2h) < 40 * s40.rows_arrived


# ------------------------------------------------------------------ 6
def test_errors_leave_the_events_alone(indexes):
    ix = indexes["tiny"]
    _, inc, exc = C.terms("tiny_inc1_exc1")
    with ix.reference_order(None, "en", NOW) as ro, ix.event(None, "en", NOW, k=50, max_postings=6400) as ev:
        ev.add_local(*C.terms("tiny_inc2")[1:], now_ms=NOW)
        before = _state(ev, False)
        with pytest.raises(YrwiError) as e:
            ix.add_local_rwis([(ev, Query(inc, exc, now_ms=NOW)), (ro, Query(inc, exc, now_ms=NOW))])
        assert e.value.rc == E_ARG
        with pytest.raises(YrwiError) as e:  # an ill-formed term hash in another arrival of the call
            ix.add_local_rwis([(ev, Query(inc, exc, now_ms=NOW)), (ev, Query([b"not*base64!!"], now_ms=NOW))])
        assert e.value.rc == E_HASH
        assert _state(ev, False) == before
    # max_postings too small: the event's own capacity flag, per arrival
    order = C.corpus("tiny")[3]
    idx = C.corpus("tiny")[1]
    with ix.event(None, "en", NOW, k=20, max_postings=0) as ev:
        with pytest.raises(YrwiError) as e:
            ix.add_local_rwis([(ev, Query([idx.hashes[t]], now_ms=NOW)) for t in order[:24]])
        assert e.value.rc == E_CAPACITY
        codes = e.value.codes
        assert E_CAPACITY in codes and codes[0] == 0
        assert all(c == 0 for c in codes[:codes.index(E_CAPACITY)])
        assert all(c == E_CAPACITY for c in codes[codes.index(E_CAPACITY):])
        assert ev.results()[1].err == E_CAPACITY


def test_sharded_context_is_refused():
    def fn(r, ix):
        if r:
            return
        with ix.event(None, "en", NOW, k=10, max_postings=64) as ev:
            with pytest.raises(YrwiError) as e:
                ev.add_local([C.ABSENT], now_ms=NOW)
            assert e.value.rc == E_UNSUPPORTED
            assert ev.results()[0] == []

    run_parts([{}, {}], 2, fn, timeout=120)


def test_retained_rows_are_freed_with_the_last_event():
    d = C.corpus("dense")[2]
    ix = open_index(d, url_ids=True)
    try:
        qs = _dense_queries()
        _call(ix, qs, 5)
        base = ix.stats()[2]
        evs = [ix.event(None, "en", NOW, k=100, max_postings=2 * 6400 + 16) for _ in range(5)]
        s1, s2 = CLocalStats(), CLocalStats()
        ms = ix.add_local_rwis([(evs[0], qs[0]), (evs[1], qs[1]), (evs[2], qs[3])], s1)
        ms += ix.add_local_rwis([(evs[2], qs[1]), (evs[3], qs[3]), (evs[4], qs[0])], s2)
        assert all(m > 0 for m in ms)  # every event holds rows in the block of its call
        assert ix.stats()[2] == base + 40 * (s1.rows_joined + s2.rows_joined)
        for i in (3, 0, 4):
            evs[i].close()
        assert ix.stats()[2] == base + 40 * (s1.rows_joined + s2.rows_joined)  # events 1 and 2 hold both blocks
        evs[2].close()
        assert ix.stats()[2] == base + 40 * s1.rows_joined
        evs[1].close()
        assert ix.stats()[2] == base
        # a context closed under an open event frees the event's retained rows itself
        ev = ix.event(None, "en", NOW, k=100, max_postings=6400 + 16)
        assert ev.add_local(qs[1].include, now_ms=NOW) == 6400
        assert ix.stats()[2] == base + 40 * 6400
    finally:
        ix.close()
