"""GPU parity (MI355X) of the hits' rows: yrwi_query_rows / yrwi_query_batch_rows /
yrwi_query_batch_rows_submit return, next to every hit, the 40-byte row of the joined
and excluded container the hit was ranked from.

Expected values come from the oracle alone: the hits of a query are orc.search's (the
literal java_literal.search where a filter decides them), and the row of a hit is the one
row of orc.term_search under the same descriptor whose first 12 bytes are the hit's url
hash.  Every comparison is equality of all 40 bytes."""

import ctypes

import numpy as np
import pytest

import index_util as iu
import java_literal as jl
import oracle as orc
import query_util as qu
from adv_rows import adv_rows, hashcodes, shard_of, sort_rows, universe_lists
from yacy_search_server_amd import Query, QueryFilter, RankingProfile, synth
from yacy_search_server_amd._lib import CHit, CStats

pytestmark = pytest.mark.gpu

DAY = 86400000
NOW = 20741 * DAY + 4242
NOWS = (NOW, 15500 * DAY + 7)
INF = 2147483647
QSEED = 700  # synth.queries(cfg, 20, 1, 4, 1, qseed=700): the coverage test_parity_presets asserts holds on every preset


def _rp(jlprof):
    rp = RankingProfile()
    for _, f in jl.PROFILE_FIELDS:
        setattr(rp, f, getattr(jlprof, f))
    return rp


@pytest.fixture(scope="module", params=["dense", "tiny", "small"])
def corpus(request):
    cfg = synth.preset(request.param)
    idx = synth.build_index(cfg)
    ix = iu.open_index(idx.as_dict())
    yield cfg, idx, ix
    ix.close()


def _queries(cfg, idx, n, qseed, nexc=1):
    return [([idx.hashes[t] for t in inc], [idx.hashes[t] for t in exc])
            for inc, exc in synth.queries(cfg, n, 1, 4, nexc, qseed=qseed)]


# ------------------------------------------------------------------ 1
def test_parity_presets(corpus):
    """1-4 include terms, 0-1 exclude terms, four profiles, two request times, k = 100: the
    hits equal search_batch without rows and the oracle, the rows the oracle's."""
    cfg, idx, ix = corpus
    d = idx.as_dict()
    qs = _queries(cfg, idx, 20, QSEED)
    assert {len(inc) for inc, _ in qs} >= {1, 2, 3, 4}
    assert {len(set(inc)) for inc, _ in qs} >= {1, 2, 3, 4}
    assert any(exc and len(orc.term_search(d, inc, exc, INF, NOW)) < len(orc.term_search(d, inc, [], INF, NOW))
               for inc, exc in qs)  # an exclusion that removes a row
    for now in NOWS:
        exp_rows = [orc.term_search(d, inc, exc, INF, now) for inc, exc in qs]
        for pname, prof in qu.profiles():
            batch = [Query(inc, exc, k=100, profile=_rp(prof), now_ms=now) for inc, exc in qs]
            got = ix.search_batch(batch, rows=True)
            plain = ix.search_batch(batch)
            for qi, (q, g, p) in enumerate(zip(batch, got, plain)):
                assert [(h.urlhash, h.score, h.tiebreak) for h in g] == [(h.urlhash, h.score, h.tiebreak) for h in p]
                assert all(h.row is None for h in p)
                exp = orc.search(d, q.include, q.exclude, orc.profile_from(prof), "en", now_ms=now, k=100)
                qu.same_rows(g, exp, exp_rows[qi], (pname, now, qi))


# ------------------------------------------------------------------ 2
def test_single_list_returns_stored_row():
    """One include term: the list's row as stored, all 40 bytes.  The same urls in a two-term
    query: the re-encoded record (typeofword and reserve 0, freshUntil from now_ms)."""
    A, B = b"TERMrowsA___", b"TERMrowsB___"
    a = qu.hand_list(700, 5)
    b = qu.hand_list(700, 6, a[:, :12])[::2].copy()
    d = {A: a, B: b}
    ix = iu.open_index(d)
    try:
        for k in (100, 3000):
            g = ix.search([A], k=k, now_ms=NOW, rows=True)
            qu.same_rows(g, orc.search(d, [A], [], now_ms=NOW, k=k), orc.term_search(d, [A], [], INF, NOW), ("single", k))
            stored = qu.row_map(a)
            assert len(g) > 50 and all(h.row == stored[h.urlhash] for h in g)
            g2 = ix.search([A, B], k=k, now_ms=NOW, rows=True)
            qu.same_rows(g2, orc.search(d, [A, B], [], now_ms=NOW, k=k), orc.term_search(d, [A, B], [], INF, NOW), ("two", k))
            assert len(g2) > 50
            today = NOW // DAY
            for h in g2:
                r = h.row
                am = (r[12] << 8) | r[13]
                assert r[28] == 0 and r[39] == 0 and ((r[14] << 8) | r[15]) == max(am + 2 * (today - am), 0) & 0xFFFF
                assert r != stored[h.urlhash]
    finally:
        ix.close()


# ------------------------------------------------------------------ 3
def test_k_edges_and_batch_layout(corpus):
    """k from 0 to 3000 in one batch of stride 3000, a missing term, fewer joined rows than k:
    nout as without rows, every query's rows at its own stride; each query alone the same."""
    cfg, idx, ix = corpus
    d = idx.as_dict()
    ks = [1, 5, 100, 3000, 0, 77, 2048, 2049]
    qs = _queries(cfg, idx, len(ks), 14)
    big = idx.hashes[int(np.argmax(idx.sizes))]
    small = idx.hashes[int(np.argmin(np.where(idx.sizes > 0, idx.sizes, 1 << 60)))]
    assert 0 < len(d[small]) < 3000
    qs += [([b"NOSUCHTERM__"], []), ([big, b"NOSUCHTERM__"], []), ([big], []), ([small], [])]
    ks += [100, 100, 3000, 3000]
    batch = [Query(inc, exc, k=k, now_ms=NOW) for (inc, exc), k in zip(qs, ks)]
    kmax = 3000
    arr, keep, hits, nout, _ = ix._marshal(batch, kmax)
    rbuf = np.full((len(batch) * kmax, 40), 0xA5, dtype=np.uint8)
    ix.search_batch_rows_raw(arr, len(batch), kmax, hits, rbuf, nout, CStats())
    plain = ix.search_batch(batch, kmax=kmax)
    got = ix.search_batch(batch, kmax=kmax, rows=True)
    assert [nout[i] for i in range(len(batch))] == [len(p) for p in plain] == [len(g) for g in got]
    assert nout[8] == 0 and nout[9] == 0 and nout[4] == 0
    short = 0
    for qi, (q, g) in enumerate(zip(batch, got)):
        exp_rows = orc.term_search(d, q.include, q.exclude, INF, NOW)
        exp = orc.search(d, q.include, q.exclude, now_ms=NOW, k=q.k) if q.k else []
        qu.same_rows(g, exp, exp_rows, ("batch", qi))
        short += 0 < len(exp_rows) < q.k
        for i, h in enumerate(g):  # the raw buffer: row i of query qi at (qi * kmax + i) * 40
            assert rbuf[qi * kmax + i].tobytes() == h.row, (qi, i)
        alone = ix.search(q.include, q.exclude, k=q.k, now_ms=NOW, rows=True)  # yrwi_query_rows
        assert alone == g, ("alone", qi)
    assert short >= 1


# ------------------------------------------------------------------ 4
def _few_hosts(idx):
    import heap
    hosts = [b"hst%03d" % i for i in range(8)]
    sel = np.frombuffer(b"".join(hosts), np.uint8).reshape(8, 6)
    d = {}
    for h, rows in idx.as_dict().items():
        r = rows.copy()
        r[:, 6:12] = sel[r[:, 3] % 8]
        d[h] = heap.sort_unique(r)
    return d


def test_doubledom_order_rows():
    """pullOneRWI(skipDoubleDom) order on a corpus of eight hosts: the rows follow the hits."""
    idx = synth.build_index(synth.preset("dense"))
    d = _few_hosts(idx)
    lit = {h: [bytes(x) for x in rows] for h, rows in d.items()}
    big = [h for h, _ in sorted(d.items(), key=lambda kv: -len(kv[1]))[:3]]
    ix = iu.open_index(d)
    try:
        cases = [(inc, k) for inc in ([big[0]], [big[1], big[2]]) for k in (10, 100, 3000)]
        batch = [Query(inc, [], k=k, now_ms=NOW, filter=QueryFilter(skip_double_dom=True)) for inc, k in cases]
        batch.insert(2, Query([big[0]], [], k=50, now_ms=NOW))  # a plain neighbour in the same batch
        got = ix.search_batch(batch, rows=True)
        changed = 0
        for q, g in zip(batch, got):
            lf = jl.QueryFilter(skip_double_dom=True) if q.filter is not None else None
            e = jl.search(lit, q.include, [], jl.RankingProfile(), "en", now_ms=NOW, k=q.k, filt=lf)
            assert [(h.urlhash, h.score) for h in g] == e
            m = qu.row_map(orc.term_search(d, q.include, [], INF, NOW))
            assert all(h.row == m[h.urlhash] for h in g)
            changed += lf is not None and e != jl.search(lit, q.include, [], jl.RankingProfile(), "en", now_ms=NOW, k=q.k)
            alone = ix.search(q.include, [], k=q.k, now_ms=NOW, filter=q.filter, rows=True)
            assert alone == g
        assert changed >= 2  # the pull order did differ from the rank order
    finally:
        ix.close()


def test_filter_quoted_urlselection_rows(corpus):
    """A filter with constraint, language, sitehash and a seeded doublecheck set; a quoted query
    (max_distance = nincl - 1); a urlselection query (rows of the index restricted to the selection)."""
    cfg, idx, ix = corpus
    d = idx.as_dict()
    rng = np.random.default_rng(9)
    big = [idx.hashes[int(t)] for t in np.argsort(-idx.sizes)[:3]]
    lit = {h: [bytes(x) for x in d[h]] for h in big}
    joined = orc.term_search(d, big[:2], [], INF, NOW)
    assert len(joined) > 20
    host = bytes(joined[len(joined) // 2][6:12])
    seeds = [bytes(r[:12]) for r in joined[::3]]
    kws = [dict(constraint=b"\0\0\x10\x01"), dict(language="de"), dict(sitehash=host),
           dict(urlhashes=seeds), dict(constraint=b"\0\0\x10\x01", language="en", urlhashes=seeds[::2])]
    nhit = 0
    for kw in kws:
        for inc in ([big[2]], big[:2]):
            g = ix.search(inc, [], k=100, now_ms=NOW, filter=QueryFilter(**kw), rows=True)
            e = jl.search(lit, inc, [], jl.RankingProfile(), "en", now_ms=NOW, k=100, filt=jl.QueryFilter(**kw))
            assert [(h.urlhash, h.score) for h in g] == e, kw
            m = qu.row_map(orc.term_search(d, inc, [], INF, NOW))
            assert all(h.row == m[h.urlhash] for h in g), kw
            nhit += len(g)
    assert nhit > 0
    # quoted queries
    qs = [q for q in _queries(cfg, idx, 30, 15, 0) if len(q[0]) >= 2][:6] + [(big[:2], []), (big, [])]
    batch = [Query(inc, exc, max_distance=len(inc) - 1, k=100, now_ms=NOW) for inc, exc in qs]
    for q, g in zip(batch, ix.search_batch(batch, rows=True)):
        qu.same_rows(g, orc.search(d, q.include, q.exclude, max_distance=q.max_distance, now_ms=NOW, k=100),
              orc.term_search(d, q.include, q.exclude, q.max_distance, NOW), ("quoted", q.include))
    # url selection
    urls = np.unique(np.asarray(idx.rows)[:, :12].copy().view("S12").ravel())
    nsel = 0
    for frac in (0.05, 0.4):
        sel = [bytes(u) for u in rng.choice(urls, max(1, int(frac * len(urls))), replace=False)]
        sel += [b"AAAAAAAAAAA" + bytes([65 + i]) for i in range(3)]  # not in the index
        rd = qu.restrict(d, sel)
        sq = _queries(cfg, idx, 12, 808, 2) + [([big[0]], []), (big[:2], [])]
        batch = [Query(inc, exc, now_ms=NOW, urlselection=sel) for inc, exc in sq]
        for q, g in zip(batch, ix.search_batch(batch, rows=True)):
            qu.same_rows(g, orc.search(rd, q.include, q.exclude, now_ms=NOW, k=100),
                  orc.term_search(rd, q.include, q.exclude, INF, NOW), ("selection", frac, q.include))
            nsel += len(g)
    assert nsel > 0


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("gb", ["0.000001", "0.002"])
def test_rows_over_several_passes(corpus, gb, monkeypatch):
    """A batch that runs as consecutive passes: every pass's rows leave before its arena is
    reused, at their queries' own positions."""
    monkeypatch.setenv("YRWI_SCRATCH_GB", gb)
    cfg, idx, ix = corpus
    d = idx.as_dict()
    qs = _queries(cfg, idx, 24, 41)
    batch = [Query(inc, exc, k=k, now_ms=NOW) for (inc, exc), k in zip(qs, [100, 7, 3000, 1] * 6)]
    got = ix.search_batch(batch, rows=True)
    for qi, (q, g) in enumerate(zip(batch, got)):
        qu.same_rows(g, orc.search(d, q.include, q.exclude, now_ms=NOW, k=q.k),
              orc.term_search(d, q.include, q.exclude, INF, NOW), (gb, qi))


# ------------------------------------------------------------------ 6
def test_async_pinned_and_landing(corpus):
    """Eight batches submitted before any wait: four with pinned buffers (written by the GPU
    directly), four with pageable ones (the landing path); one pinned rows buffer offset by 4
    bytes, which must land."""
    cfg, idx, ix = corpus
    d = idx.as_dict()
    kmax = 50
    tickets = []
    for s in range(8):
        b = [Query(inc, exc, k=50, now_ms=NOW) for inc, exc in _queries(cfg, idx, 7 + s, 60 + s, s % 2)]
        arr, keep = qu.cqueries(b)
        n = len(b)
        if s % 2:
            hits, nout = ix.host_array(CHit, n * kmax), ix.host_array(ctypes.c_int32, n)
            raw = ix.host_array(ctypes.c_uint8, n * kmax * 40 + 8)
            off = 4 if s == 3 else 0
            assert ctypes.addressof(raw) % 8 == 0
            rows = ctypes.addressof(raw) + off
            view = np.frombuffer(raw, dtype=np.uint8)[off:off + n * kmax * 40].reshape(-1, 40)
        else:
            hits, nout = (CHit * (n * kmax))(), (ctypes.c_int32 * n)()
            view = np.zeros((n * kmax, 40), dtype=np.uint8)
            rows = view
            raw = None
        view[:] = 0x5A
        st = CStats()
        t = ix.submit_rows_raw(arr, n, kmax, hits, rows, nout, st)
        tickets.append((t, b, hits, nout, view, (st, keep, arr, raw)))
    for t, b, hits, nout, view, _ in tickets:
        ix.wait(t)
        for i, q in enumerate(b):
            got = [(bytes(hits[i * kmax + j].urlhash), hits[i * kmax + j].score, hits[i * kmax + j].tiebreak)
                   for j in range(nout[i])]
            assert got == orc.search(d, q.include, q.exclude, now_ms=NOW, k=q.k), (t, i)
            m = qu.row_map(orc.term_search(d, q.include, q.exclude, INF, NOW))
            for j, (u, _, _) in enumerate(got):
                assert view[i * kmax + j].tobytes() == m[u], (t, i, j)
    # the same through submit(rows=True) / PendingBatch.result
    b = tickets[1][1]
    pend = [ix.submit(b, kmax=kmax, rows=True), ix.submit(b, kmax=kmax)]
    with_rows, without = pend[0].result(), pend[1].result()
    assert with_rows == ix.search_batch(b, kmax=kmax, rows=True)
    assert without == ix.search_batch(b, kmax=kmax) and all(h.row is None for g in without for h in g)


# ------------------------------------------------------------------ 7
def test_null_rows_is_the_old_call(corpus):
    """rows40_out == NULL through the new entry points: hits and nout of the old ones."""
    from yacy_search_server_amd import _lib
    cfg, idx, ix = corpus
    b = [Query(inc, exc, k=k, now_ms=NOW)
         for (inc, exc), k in zip(_queries(cfg, idx, 12, 77), [100, 3, 3000, 0, 50, 1] * 2)]
    kmax, n = 3000, 12
    arr, keep = qu.cqueries(b)

    def bufs():
        return (CHit * (n * kmax))(), (ctypes.c_int32 * n)()

    def dec(hits, nout):
        return [[(bytes(hits[i * kmax + j].urlhash), hits[i * kmax + j].score, hits[i * kmax + j].tiebreak)
                 for j in range(nout[i])] for i in range(n)]

    h0, n0 = bufs()
    ix.search_batch_raw(arr, n, kmax, h0, n0, None)
    old = dec(h0, n0)
    assert sum(len(x) for x in old) > 0
    h1, n1 = bufs()
    ix.search_batch_rows_raw(arr, n, kmax, h1, None, n1, None)
    assert dec(h1, n1) == old
    h2, n2 = bufs()
    ix.wait(ix.submit_rows_raw(arr, n, kmax, h2, None, n2, None))
    assert dec(h2, n2) == old
    h3, n3 = bufs()
    ix.wait(ix.submit_raw(arr, n, kmax, h3, n3, None))
    assert dec(h3, n3) == old
    L = _lib.lib()
    for i, q in enumerate(b):
        one, cnt = (CHit * max(1, q.k))(), ctypes.c_int32()
        assert L.yrwi_query_rows(ix._h, ctypes.byref(arr[i]), one, None, ctypes.byref(cnt), None) == 0
        assert [(bytes(one[j].urlhash), one[j].score, one[j].tiebreak) for j in range(cnt.value)] == old[i][:q.k]
        assert cnt.value == len(old[i])


# ------------------------------------------------------------------ 8
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_rows_loopback(world):
    """Url-hash shards over the loopback transport: every rank ends with the oracle's hits; the
    rank owning a hit's url-hash range returns the oracle's row, every other rank 40 zero bytes."""
    cfg = synth.preset("tiny")
    idx = synth.build_index(cfg)
    whole = idx.as_dict()
    lit = {h: [bytes(x) for x in rows] for h, rows in whole.items()}
    parts = [{h: shard_of(r, rk, world) for h, r in whole.items() if len(shard_of(r, rk, world))}
             for rk in range(world)]
    c5 = jl.RankingProfile.parse("", "date=15,domlength=15,authority=13,tf=10")
    qs = _queries(cfg, idx, 16, QSEED)
    big = [idx.hashes[int(t)] for t in np.argsort(-idx.sizes)[:2]]
    cases = [(inc, exc, c5 if i % 2 else jl.RankingProfile(), False) for i, (inc, exc) in enumerate(qs)]
    cases += [([big[0]], [], jl.RankingProfile(), True), (big, [], jl.RankingProfile(), False)]

    def run(rk, ix):
        batch = [Query(inc, exc, k=100, profile=_rp(prof), now_ms=NOW,
                       filter=QueryFilter(skip_double_dom=True) if dd else None) for inc, exc, prof, dd in cases]
        return ix.search_batch(batch, rows=True)

    res = iu.run_parts(parts, world, run)
    sh = 6 - (world.bit_length() - 1)
    zero = bytes(40)
    spread = 0
    for ci, (inc, exc, prof, dd) in enumerate(cases):
        if dd:
            exp = [(u, s) for u, s in jl.search(lit, inc, exc, prof, "en", now_ms=NOW, k=100,
                                                filt=jl.QueryFilter(skip_double_dom=True))]
        else:
            exp = [(u, s) for u, s, _ in orc.search(whole, inc, exc, orc.profile_from(prof), "en", now_ms=NOW, k=100)]
        m = qu.row_map(orc.term_search(whole, inc, exc, INF, NOW))
        for rk in range(world):
            assert [(h.urlhash, h.score) for h in res[rk][ci]] == exp, (world, rk, ci)
        owners = set()
        for i, (u, _) in enumerate(exp):
            owner = jl.AHPLA[u[0]] >> sh
            owners.add(owner)
            for rk in range(world):
                assert res[rk][ci][i].row == (m[u] if rk == owner else zero), (world, rk, ci, i)
        spread += len(owners) > 1
    assert spread >= 1  # a query whose hits belong to more than one rank


# ------------------------------------------------------------------ 9
def test_adversarial_rows_returned():
    """Cells at their extremes (nonzero reserved bytes, any doctype and flag byte) in single
    lists of several chunks and in joins of one universe: the rows of the surviving hits."""
    d = universe_lists(11, 5000)
    A, B, C, D = d
    d[b"TERMadvFEW__"] = adv_rows(6200, 52, "few")
    d[b"TERMadvTIGHT"] = adv_rows(6200, 53, "tight")
    qs = [([h], []) for h in d] + [([A, B], []), ([A, B, C], []), ([A, B, C, D], []), ([A, B], [D]), ([A], [C])]
    ix = iu.open_index(d)
    try:
        for now in NOWS:
            for k in (100, 3000):
                batch = [Query(inc, exc, k=k, now_ms=now) for inc, exc in qs]
                for q, g in zip(batch, ix.search_batch(batch, rows=True)):
                    qu.same_rows(g, orc.search(d, q.include, q.exclude, now_ms=now, k=k),
                          orc.term_search(d, q.include, q.exclude, INF, now), (now, k, q.include, q.exclude))
    finally:
        ix.close()


def test_tying_twins_across_chunks():
    """Postings that tie on score and ByteArray.hashCode, spread over several 2048-posting
    chunks: the TreeSet keeps the first of each class, and the row returned with it is its own,
    not the rejected twin's (the twins' rows differ in their reserved bytes)."""
    rng = np.random.default_rng(23)
    alpha = np.frombuffer(jl.ALPHA, dtype=np.uint8)
    fams, seen = [], set()
    for f in range(100):
        base = bytes(rng.choice(alpha[:26], 2)) + b"".join(
            bytes([int(rng.integers(65, 90)), int(rng.integers(97 + 6, 97 + 25))]) for _ in range(5))
        hs = [h for h in qu.collision_family(base, 5) if h not in seen]
        seen.update(hs)
        fams.append(hs)
    filler = set()
    while len(filler) < 4000:
        h = bytes(rng.choice(alpha, 12))
        if h not in seen:
            filler.add(h)
    allh = [h for hs in fams for h in hs] + sorted(filler)
    fam_of = {h: f for f, hs in enumerate(fams) for h in hs}
    n = len(allh)
    rows = np.zeros((n, 40), dtype=np.uint8)
    for i, h in enumerate(allh):
        rows[i, :12] = np.frombuffer(h, dtype=np.uint8)
        f = fam_of.get(h)
        day = 20000 + f if f is not None else 15000 + int(rng.integers(0, 300))  # the families rank first
        rows[i, 12:14] = np.frombuffer(day.to_bytes(2, "big"), dtype=np.uint8)
        rows[i, 17:19] = np.frombuffer((40 + (f or 0) % 7).to_bytes(2, "big"), dtype=np.uint8)
        rows[i, 21] = ord("t")
        rows[i, 22:24] = np.frombuffer(b"en", dtype=np.uint8)
        rows[i, 33] = 9 if f is not None else int(rng.integers(1, 9))
        p = 3 if f is not None else int(rng.integers(1, 400))
        rows[i, 34], rows[i, 35] = p >> 8, p & 0xFF
    rows[:, 28] = 1 + np.arange(n) % 251  # typeofword and reserve: no two twins' stored rows agree
    rows[:, 39] = 1 + np.arange(n) % 241
    rows = sort_rows(rows)
    assert n > 2 * 2048
    T, U = b"TERMtwins___", b"TERMtwinsB__"
    d = {T: rows, U: rows[::2].copy()}
    hc = dict(zip((bytes(r[:12]) for r in rows), hashcodes(rows)))
    ix = iu.open_index(d)
    try:
        for inc in ([T], [T, U]):
            joined = orc.term_search(d, inc, [], INF, NOW)
            for k in (100, 3000):
                g = ix.search(inc, k=k, now_ms=NOW, rows=True)
                exp = orc.search(d, inc, [], now_ms=NOW, k=k)
                qu.same_rows(g, exp, joined, (len(inc), k))
                assert all(h.row[:12] == h.urlhash for h in g)
            # the dedupe did reject twins: fewer (score, hashCode) classes among the hits' families than postings
            kept = {u for u, _, _ in exp}
            rejected = [bytes(r[:12]) for r in joined if bytes(r[:12]) in fam_of and bytes(r[:12]) not in kept]
            assert rejected and any(hc[u] in {hc[v] for v in kept} for u in rejected)
    finally:
        ix.close()
