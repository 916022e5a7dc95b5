"""GPU parity (MI355X) on url hashes that share their first 64 key bits.

The device stores a 72-bit url key as khi (64 bits) and klo (8 bits); every key compare has a
second branch, `ah == bh && al < bl`, that runs only when two keys agree in khi.  The lists here
come from tests/split_keys.py: families of 8 to 16 hashes with one khi, at the edge values of khi
and klo, so that at least half of the adjacent rows of every list agree in khi (asserted).
tests/test_split_keys_ref.py shows on the CPU that a khi-only compare gives another answer on
every input used here.  Expected values come from oracle.search / oracle.term_search,
oracle/heap.py, oracle/abstracts.py, java_literal and tests/update_ref.py's key order; every
comparison is equality.

What each test reaches (kernel: compare site):
  test_put_list_order            k_validate: the "strictly ascending" check (siblings swapped, a
                                 sibling twice, inside a block and across rows 255 / 256); the
                                 host's stable sort of sorted = 0
  test_dictionary_full_build     full_rebuild (yrwi_dict.hip): radix sort by klo, then stably by
                                 khi; k_dict_flags reads kl[pos[j]] through the permutation;
                                 k_heads' two head levels (a list of more than 1,024 rows)
  test_dictionary_incremental    k_dict_lookup and k_uid_assign, both through lb_key: new keys
                                 below, between and above their family's present members, and
                                 a list of known keys only
  test_joins_and_rank            the join kernels on url ids (id probe and merge tiles on an index
                                 without bitmaps, the bitmap probe on the shared one, chained and
                                 stepwise folds) over ids that the dictionary gave to siblings;
                                 the authority host counts through key_host36, whose low 8 bits
                                 are klo (siblings are different hosts)
  test_selection_and_doublecheck k_sel_lookup (url selections); the doublecheck search in admit
                                 (QueryFilter.urlhashes)
  test_hit_rows_doubledom        k_hit_rows in its HR_HITS mode: the binary search by key
  test_event_arrivals            the event url set: uset_slot / uset_insert / uset_find, which
                                 store hi >> 1 and pick a sub-table from the other 9 bits
                                 (h / h + 1 neighbour families with equal klo)
  test_event_local_rows          uset_find behind yrwi_event_rows and yrwi_event_source after a
                                 device-local arrival
  test_heap_loader               k_union_b / k_union_a / k_union_bs through the shared lb_key,
                                 k_validate on every record
  test_index_abstracts           k_ca_keys' exclusion search
  test_secondary_search          same_url in the secondary-search kernels (the low byte travels
                                 in k2 >> 40, next to the word and abstract numbers)

Left out on purpose: k_dht_bounds compares only the top e bits of khi; k_dump_pack compares no
keys; the removal, count and census kernels see hosts that differ in klo only through
host_ref.host_name (tests/test_gpu_hosts.py, tests/test_gpu_census.py); the update kernels have
_universe() in tests/test_gpu_updates.py."""

import numpy as np
import pytest

import abstracts as ab
import event_local_cases as C
import heap
import index_util as iu
import java_literal as jl
import oracle as orc
import query_util as qu
import split_keys as sk
from abstract_cases import oracle_plan
from yacy_search_server_amd import Query, QueryFilter, RankingProfile, RWIIndex
from yacy_search_server_amd._lib import YrwiError

pytestmark = pytest.mark.gpu

DAY = 86400000
NOW = 20741 * DAY + 4242
INF = 2147483647
E_UNSORTED = -3
C5_STR = "date=15,domlength=15,authority=13,tf=10"  # the C5 profile of the update tests
A, B, CC, D = sk.TERMS
E = sk.T257


def _hashes(r):
    return [bytes(x) for x in r[:, :12]]


def _profiles():
    return [("default", None, None), ("c5", RankingProfile("", C5_STR), jl.RankingProfile.parse("", C5_STR))]


def _check_hits(ix, lists, qs, k, ctx, **kw):
    """search_batch of the queries under the default and the authority profile against orc.search"""
    for name, rp, lp in _profiles():
        op = orc.profile_from(lp if lp is not None else jl.RankingProfile())
        got = qu.gpu_raw(ix, [Query(inc, exc, k=k, profile=rp, now_ms=NOW, **kw) for inc, exc in qs])
        for qi, ((inc, exc), g) in enumerate(zip(qs, got)):
            qu.same_hits(g, qu.orc_raw(lists, inc, exc, op, "en", NOW, k), (ctx, name, qi))
    return got


@pytest.fixture(scope="module")
def shared():
    """one index over split_keys.corpus(): lists A..D over a universe of about 6,000 urls (A holds
    all of them: both head levels of k_heads), a run of exactly 257 rows, the exclusion list"""
    d = sk.corpus()
    for h, r in d.items():
        sk.check_list(r, h)
    assert len(d[A]) > 1024 and len(d[E]) == 257 and max(len(r) for r in d.values()) <= 8000
    ix = iu.open_index(d)
    ix.build_url_ids()
    yield ix, d
    ix.close()


# ------------------------------------------------------------------ a
def test_put_list_order():
    uni = sk.universe()
    run, bad = sk.order_input()
    s = uni.index(bytes(run[0, :12]))
    T, U = b"TERMspkord1_", b"TERMspkord2_"
    ix = RWIIndex(0)
    try:
        for i, swapped, twice in bad:  # inside a block of k_validate, and across rows 255 / 256
            hs = _hashes(swapped)
            # the only disorder: equal khi, descending klo
            assert sk.split(hs[i])[0] == sk.split(hs[i + 1])[0] and sk.split(hs[i])[1] > sk.split(hs[i + 1])[1]
            assert sorted(hs, key=sk.true_key) == _hashes(run)
            assert bytes(twice[i, :12]) == bytes(twice[i + 1, :12]) and sk.blind_key(twice[i - 1]) == sk.blind_key(twice[i])
            for rows in (swapped, twice):
                with pytest.raises(YrwiError) as e:
                    ix.add(T, rows)
                assert e.value.rc == E_UNSORTED, i
                assert ix.get_size(T) == 0
        ix.add(T, run)  # the rows in order are accepted
        assert np.array_equal(ix.get_list(T), run)
        # sorted = 0: the same rows and second rows (other cells) of 100 of the hashes, shuffled
        more = sk.rows(uni[s + 200:s + 300], 42)
        both = np.concatenate([run, more])
        both = both[np.random.default_rng(43).permutation(len(both))]
        exp = heap.sort_unique(both)  # the first of two equal hashes is kept
        first = {}
        for r in both:
            first.setdefault(bytes(r[:12]), bytes(r))
        assert [bytes(r) for r in exp] == [first[h] for h in _hashes(run)]
        assert any(first[h] == bytes(r) for h, r in zip(_hashes(more), more))  # both ways round
        assert any(first[h] != bytes(r) for h, r in zip(_hashes(more), more))
        ix.add(U, both, sorted=False)
        assert np.array_equal(ix.get_list(U), exp)
        assert ix.check_url_ids() == (0, 600)
    finally:
        ix.close()


# ------------------------------------------------------------------ b
DICT_QS = [([A, B], []), ([A, B, CC], [D]), ([CC, D], []), ([A], [B]), ([B, E], []), ([A, B, CC, D], [])]


def test_dictionary_full_build(shared, monkeypatch):
    ix, d = shared
    n = sk.distinct(h for r in d.values() for h in _hashes(r))
    assert n > len(sk.universe())  # the exclusion list names siblings that no other list has
    assert ix.check_url_ids() == (0, n)
    monkeypatch.setenv("YRWI_DICT_FULL", "1")
    fresh = iu.open_index(d)
    try:
        assert fresh.check_url_ids() == (0, n)
        assert fresh.index_info()["incremental_updates"] == 0
        _check_hits(fresh, d, DICT_QS, 100, "full")
    finally:
        fresh.close()


def test_dictionary_incremental(monkeypatch):
    uni = sk.universe()
    base, sibl, known, where = sk.dictionary_input()
    assert min(where.values()) > 50, where
    present = _hashes(base[A])
    S, K = b"TERMspksibl_", b"TERMspkknow_"
    # sibl: only siblings of keys the dictionary has; known: only keys it has
    assert not set(_hashes(sibl)) & set(present) and set(_hashes(known)) <= set(present)
    assert {sk.blind_key(h) for h in _hashes(sibl)} <= {sk.blind_key(h) for h in present}
    assert len(present) + len(sibl) == len(uni)
    qs = DICT_QS[:4] + [([A, S], []), ([S], []), ([A], [S]), ([K, B], []), ([A, K], [S]), ([S, K], [])]
    ix = iu.open_index(base)
    try:
        _check_hits(ix, base, DICT_QS[:4], 100, "first query")  # the full build
        assert ix.check_url_ids() == (0, len(present))
        ix.add(S, sibl)
        ix.add(K, known)
        lists = {**base, S: sibl, K: known}
        total = sum(len(r) for r in lists.values())
        assert 4 * (len(sibl) + len(known)) < total  # the precondition of an incremental update
        before = ix.index_info()
        assert ix.check_url_ids() == (0, len(uni))
        after = ix.index_info()
        assert after["incremental_updates"] == before["incremental_updates"] + 1, after
        assert after["full_rebuilds"] == before["full_rebuilds"] == 1, after
        got = _check_hits(ix, lists, qs, 100, "incremental")
        # siblings are other urls: a list of siblings alone joins with nothing and excludes nothing
        assert len(orc.term_search(lists, [A, S], [], INF, NOW)) == 0
        assert len(orc.term_search(lists, [A], [S], INF, NOW)) == len(base[A])
        assert np.array_equal(ix.term_search([A, S], [], INF, NOW), np.zeros((0, 40), np.uint8))
        assert np.array_equal(ix.term_search([A], [S], INF, NOW), base[A])
        monkeypatch.setenv("YRWI_DICT_FULL", "1")
        fresh = iu.open_index(lists)
        try:
            assert fresh.check_url_ids() == (0, len(uni))
            assert fresh.index_info()["incremental_updates"] == 0
            assert _check_hits(fresh, lists, qs, 100, "fresh") == got  # the same hits under both settings
        finally:
            fresh.close()
    finally:
        ix.close()


# ------------------------------------------------------------------ c
JOIN_QS = [([A, B], []), ([CC, D], []), ([B, E], []), ([A, B, CC], []), ([A, B, CC, D], []), ([A, B], [D]),
           ([CC, B, A], [D]), ([A, CC, D], [E]), ([A, B, CC, D], [E])]


@pytest.fixture(scope="module")
def plain():
    """the same lists on an index built without url-id bitmaps (YRWI_BM_DIV = 0, read when the
    dictionary is built): a list with a bitmap is probed at any YRWI_PROBE_RATIO (layout_jobs), so
    only here do the id probe and the merge tiles meet every query"""
    d = sk.corpus()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("YRWI_BM_DIV", "0")
        ix = iu.open_index(d)
        ix.build_url_ids()
    yield ix, d
    ix.close()


@pytest.mark.parametrize("chain", ["chained", "stepwise"])
@pytest.mark.parametrize("algo", ["probe", "merge"])
@pytest.mark.parametrize("index", ["plain", "bitmaps"])
def test_joins_and_rank(shared, plain, index, algo, chain, monkeypatch):
    """two-, three- and four-term queries with and without an exclude: the rows of term_search
    and the hits at k = 3000 under the default and the authority profile, under the four
    combinations of YRWI_PROBE_RATIO and YRWI_NO_CHAIN.  On the index without bitmaps these are the
    id probe and the merge tiles; on the shared index lists A and B (more than 4,096 urls) have
    bitmaps, and YRWI_PROBE_RATIO = 1 there is the bitmap probe."""
    from yacy_search_server_amd._lib import CStats
    monkeypatch.setenv("YRWI_PROBE_RATIO", "1" if algo == "probe" else "1000000000")
    monkeypatch.setenv("YRWI_NO_CHAIN", "1" if chain == "stepwise" else "0")
    ix, d = plain if index == "plain" else shared
    nbm = ix.index_info()["bitmap_lists"]
    assert nbm == 0 if index == "plain" else nbm >= 2, nbm
    for qi, (inc, exc) in enumerate(JOIN_QS):
        exp = orc.term_search(d, inc, exc, INF, NOW)
        got = ix.term_search(inc, exc, INF, NOW)
        assert got.shape == exp.shape and np.array_equal(got, exp), (index, algo, chain, qi)
        if not exc:  # the joined urls include siblings
            assert len(exp) > 100 and sk.equal_khi_fraction(exp) > 0.25, (qi, sk.equal_khi_fraction(exp))
    _check_hits(ix, d, JOIN_QS, 3000, (index, algo, chain))
    # the library's own counters: the setting took the path it names
    st = CStats()
    qu.gpu_raw(ix, [Query(inc, exc, k=3000, now_ms=NOW) for inc, exc in JOIN_QS], stats=st)
    assert (st.n_chain_launches == 0) == (chain == "stepwise"), st.n_chain_launches
    # (probe tiles: a job whose larger side has a bitmap, or is more than YRWI_PROBE_RATIO times the smaller)
    assert (st.n_probe_dispatches == 0) == (index == "plain" and algo == "merge"), st.n_probe_dispatches


# ------------------------------------------------------------------ d
def test_selection_and_doublecheck(shared):
    ix, d = shared
    uni = sk.universe()
    sel, left, ghosts = sk.selection(uni, sk.SEED + 3)
    assert ghosts and not set(ghosts) & set(uni)
    rd = qu.restrict(d, sel)
    qs = [([A], []), ([A, B], []), ([A, B, CC], [D]), ([B, E], []), ([A], [D]), ([CC, D], [])]
    for qi, (inc, exc) in enumerate(qs):
        exp = orc.term_search(rd, inc, exc, INF, NOW)
        got = ix.term_search(inc, exc, INF, NOW, urlselection=sel)
        assert got.shape == exp.shape and np.array_equal(got, exp), qi
        assert len(got) > 20 and not set(_hashes(got)) & set(left)  # siblings outside the selection are absent
    got = _check_hits(ix, rd, qs, 3000, "selection", urlselection=sel)
    for g in got:
        assert len(g) and not {h for h, _, _ in qu.decode(g)} & (set(left) | set(ghosts))
    # the doublecheck set of a filter, built the same way
    dc, left2, ghosts2 = sk.selection(uni, sk.SEED + 4)
    lit = {h: [bytes(x) for x in d[h]] for h in (B, CC, D)}
    for inc in ([CC], [B, D]):
        gf, lf = QueryFilter(urlhashes=dc), jl.QueryFilter(urlhashes=dc)
        got = ix.search(inc, [], now_ms=NOW, k=3000, filter=gf)
        exp = jl.search(lit, inc, [], jl.RankingProfile(), "en", now_ms=NOW, k=3000, filt=lf)
        assert [(h.urlhash, h.score) for h in got] == exp, inc
        assert gf.flagcount == lf.flagcount, inc
        urls = {h.urlhash for h in got}
        joined = set(_hashes(orc.term_search(d, inc, [], INF, NOW)))
        assert urls <= joined - set(dc) and len(urls & set(left2)) > 50 and joined & set(dc)


# ------------------------------------------------------------------ e
def test_hit_rows_doubledom(shared):
    """search(rows=True) under the doubledom pull order: the hits are looked up by key among the
    joined rows (k_hit_rows, HR_HITS); every hit's row is its own url's, never a sibling's"""
    ix, d = shared
    lit = {h: [bytes(x) for x in d[h]] for h in (B, CC, D)}
    for inc in ([CC], [B, D]):
        joined = orc.term_search(d, inc, [], INF, NOW)
        assert sk.sibling_bytes_differ(joined) and sk.equal_khi_fraction(joined) > 0.25
        m = qu.row_map(joined)
        full = jl.search(lit, inc, [], jl.RankingProfile(), "en", now_ms=NOW, k=3000,
                         filt=jl.QueryFilter(skip_double_dom=True))
        for k in (100, 3000):
            got = ix.search(inc, [], k=k, now_ms=NOW, filter=QueryFilter(skip_double_dom=True), rows=True)
            assert [(h.urlhash, h.score) for h in got] == full[:k], (inc, k)  # (the pulls are sequential)
            assert len(got) >= 100 and all(h.row == m[h.urlhash] for h in got), (inc, k)
        fams = sk.by_family(sorted((h.urlhash for h in got), key=sk.true_key))
        assert sum(len(f) > 1 for f in fams) > 50  # siblings among the hits


# ------------------------------------------------------------------ f
def test_event_arrivals():
    arrivals, never, pairs = sk.event_input()
    total = sum(len(r) for r, _ in arrivals)
    ix = RWIIndex(0)
    try:
        C.check_event(ix, arrivals, k=3000)
        C.check_event(ix, arrivals, {"coeff_authority": 14, "coeff_worddistance": 15}, k=3000)
        # where every url was admitted: the literal oracle's doublecheck set, arrival by arrival
        ref = jl.SearchEventRWI(jl.RankingProfile(), "en", C.NOW)
        admitted = {}
        with ix.event(None, "en", C.NOW, k=3000, max_postings=total + 16) as ev:
            for j, (rows, local) in enumerate(arrivals, 1):
                before = set(ref.filt.urlhashes)
                ref.add_rwis(C.rows_list(rows), local)
                for h in ref.filt.urlhashes - before:
                    admitted[h] = j
                ev.add_rwis(rows, local)
            arrived = {h for r, _ in arrivals for h in _hashes(r)}
            assert set(admitted) == arrived and set(admitted.values()) == {1, 2, 3}
            urls = sorted(admitted, key=sk.true_key)
            src = ev.source(urls)
            assert [a for a, _ in src] == [admitted[u] for u in urls]
            assert all(bytes(arrivals[a - 1][0][r, :12]) == u for u, (a, r) in zip(urls, src))
            assert ev.source(never) == [(-1, -1)] * len(never)
            for a, b in pairs:  # khi apart in bit 0 only, equal klo: the same stored word, another sub-table
                (aa, ra), (ab_, rb) = ev.source([a, b])
                assert aa == admitted[a] == admitted[b] == ab_ and ra != rb
            hits, _ = ev.results()
            assert [(h.urlhash, h.score) for h in hits] == ref.stack()[:3000]
    finally:
        ix.close()


def test_event_local_rows(shared):
    """add_local against add_rwis(term_search(...), True) and the literal oracle; rows() returns each
    admitted url's own row and None for its absent siblings"""
    ix, d = shared
    uni = sk.universe()
    for inc, exc in (([D], []), ([B, D], []), ([CC, D], [E])):
        exp = orc.term_search(d, inc, exc, INF, NOW)
        m = {bytes(r[:12]): bytes(r) for r in exp}
        khis = {sk.blind_key(u) for u in m}
        absent = [u for u in uni if u not in m and sk.blind_key(u) in khis]
        assert len(m) > 200 and len(absent) > 200
        ref = jl.SearchEventRWI(jl.RankingProfile(), "en", NOW)
        ref.add_rwis(C.rows_list(exp), True)
        with ix.event(None, "en", NOW, k=3000, max_postings=len(exp) + 16) as X, \
                ix.event(None, "en", NOW, k=3000, max_postings=len(exp) + 16) as Y:
            assert X.add_local(inc, exc, now_ms=NOW) == len(exp)
            Y.add_rwis(ix.term_search(inc, exc, now_ms=NOW), True)
            (hx, ix_), (hy, iy) = X.results(), Y.results()
            assert [(h.urlhash, h.score, h.tiebreak) for h in hx] == [(h.urlhash, h.score, h.tiebreak) for h in hy]
            assert C.info_dict(ix_, False) == C.info_dict(iy, False)
            assert [(h.urlhash, h.score) for h in hx] == ref.stack()[:3000]
            want = C.info_of(ref, len(exp))
            want.pop("maxdomcount")
            assert C.info_dict(ix_, False) == want
            urls = list(m)
            assert X.rows(urls) == [m[u] for u in urls], (inc, exc)
            assert X.rows(absent) == [None] * len(absent)
            assert X.source(urls) == Y.source(urls) and {a for a, _ in X.source(urls)} == {1}
            assert X.source(absent) == [(-1, -1)] * len(absent)


# ------------------------------------------------------------------ g
def test_heap_loader(tmp_path):
    files, ram = sk.heap_input()
    paths = []
    for f, recs in enumerate(files):
        p = str(tmp_path / f"text.index.2024010100000{f}000.blob")
        heap.write_heap(p, [(t, heap.export_collection(r)) for t, r in recs])
        paths.append(p)
    exp = heap.index_get(heap.order_files(paths), ram)
    t = sorted(exp)
    assert len(t) == 4 and [len(exp[x]) for x in t[1:]] == [511, 257, 3]
    for x in t:
        sk.check_list(exp[x], x)
    ix = RWIIndex(0)
    try:
        for h, r in ram.items():
            ix.add(h, r)
        st = ix.load_heaps(list(reversed(paths)), order_by_name=True)
        assert st.files == 3 and st.dropped_terms == 0
        assert st.terms == len(exp) and st.postings == sum(len(v) for v in exp.values())
        for h, rows in exp.items():
            assert ix.get_size(h) == len(rows)
            assert np.array_equal(ix.term_search([h], now_ms=NOW), rows), h
        assert ix.check_url_ids() == (0, sk.distinct(h for r in exp.values() for h in _hashes(r)))
        qs = [([t[0]], []), ([t[0], t[1]], []), ([t[0]], [t[2]]), ([t[2], t[0]], [t[3]]), ([t[1], t[2]], []),
              ([t[3]], []), ([t[0], t[3]], [])]
        assert all(len(orc.term_search(exp, inc, exc, INF, NOW)) for inc, exc in qs)
        _check_hits(ix, exp, qs, 3000, "heap")
    finally:
        ix.close()


# ------------------------------------------------------------------ h
def test_index_abstracts(shared):
    ix, d = shared
    ex = [bytes(r) for r in d[sk.TEXCL]]
    for terms in ([A, B], [CC, D], [E]):
        got = ix.index_abstracts(terms, exclude=sk.TEXCL)
        exp = [ab.compress_index([bytes(r) for r in d[t]], ex) for t in terms]
        assert got == exp, terms
        assert exp != [ab.compress_index([bytes(r) for r in d[t]]) for t in terms]
    assert ix.index_abstracts([A, D]) == [ab.compress_index([bytes(r) for r in d[t]]) for t in (A, D)]


def test_secondary_search():
    words, base, abstracts, peers = sk.abstract_input()
    ix = RWIIndex(0)
    try:
        for mypeer, checked in ((peers[0], ()), (b"notapeer____", peers[1:3])):
            join, wl, plan = ix.secondary_search(abstracts, len(words), mypeer, checked)
            ejoin, eplan = oracle_plan(abstracts, words, mypeer, checked)
            assert wl == words
            assert join == [(u, next(iter(ejoin[u]))) for u in sorted(ejoin)]
            assert plan == eplan and len(plan) >= 5
            fams = sk.by_family(sorted((u for u, _ in join), key=sk.true_key))
            assert sum(len(f) > 1 for f in fams) > 50  # siblings are joined as separate urls
    finally:
        ix.close()
