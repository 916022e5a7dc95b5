"""GPU parity (MI355X) of the pair cache (csrc/yrwi_pair_cache.h): the joined
container of a two-term query is kept across calls and a later query of the pair is ranked from
the kept container instead of joining again.

Every comparison is bit-exact against the oracle on the index as it stands at that moment; the
counters of yrwi_pair_cache_info_get tell whether a query filled an entry, hit one or went
around the cache.  The admission minimum is 1 row here (YRWI_PAIR_CACHE_MIN_ROWS), so the
small presets fill the cache."""

import numpy as np
import pytest

import host_ref as hr
import index_util as iu
import oracle as orc
import query_util as qu
import retention_ref as rr
import update_ref as ur
from adv_rows import adv_rows
from yacy_search_server_amd import Query, RankingProfile, synth

pytestmark = pytest.mark.gpu

DAY = 86400000
NOW = 20741 * DAY + 777
INF = 2147483647


@pytest.fixture(autouse=True)
def _admit_every_pair(monkeypatch):
    monkeypatch.setenv("YRWI_PAIR_CACHE_MIN_ROWS", "1")
    monkeypatch.setenv("YRWI_PAIR_CACHE", "1")
    monkeypatch.delenv("YRWI_PAIR_CACHE_MB", raising=False)


def _triples(hits):
    return [(h.urlhash, h.score, h.tiebreak) for h in hits]


def _oracle(d, q):
    prof = orc.profile_from(q.profile) if q.profile is not None else None
    return orc.search(d, q.include, q.exclude, prof, q.language, q.max_distance, q.now_ms, q.k)


def _one_lane(ix, batch, rows=False):
    """the whole batch as one part on one lane"""
    return ix.submit(batch, rows=rows).result()


def _delta(ix, before):
    now = ix.pair_cache_info()
    return {k: now[k] - before[k] for k in ("hits", "misses", "fills", "dropped", "evictions", "invalidations",
                                            "rows_served")}


def _q(inc, exc=(), **kw):
    kw.setdefault("now_ms", NOW)
    return Query(list(inc), list(exc), **kw)


@pytest.fixture(scope="module")
def dense():
    """the `dense` preset, one context holding it, a batch of two-term queries beside queries the
    cache does not serve, and the oracle's hits of the batch (computed once)"""
    idx = synth.build_index(synth.preset("dense"))
    d = idx.as_dict()
    ix = iu.open_index(d, url_ids=True)  # (the cache's block is reserved with the url ids)
    order = [int(t) for t in np.argsort(-idx.sizes, kind="stable")]
    a, b, c = (idx.hashes[t] for t in order[:3])
    pairs = [[idx.hashes[t] for t in inc] for inc, _ in synth.queries(idx.cfg, 20, 2, 2, 0, qseed=77)]
    batch = [_q(p) for p in pairs] + [
        _q([a, b]), _q([b, a]),                      # one pair in both orders (one query to the batch: shared)
        _q([a, b, c]), _q([a]), _q([a, b], [c]),     # three terms, one term, an exclusion: not served
        _q([a, b], max_distance=1),                  # a quoted query: not served
        _q([a, c], k=7), _q([b, c], language="de"),
    ]
    exp = [_oracle(d, q) for q in batch]
    yield idx, d, ix, batch, exp, (a, b, c)
    ix.close()


def _served(d, q):
    """the cache serves q (the default profile has no authority counts) and its join is not empty"""
    inc = set(q.include)
    return (len(inc) == 2 and not q.exclude and q.max_distance == INF and q.filter is None and
            all(t in d for t in inc) and len(orc.term_search(d, sorted(inc), [], INF, q.now_ms)) > 0)


# ------------------------------------------------------------------ 1: the same batch twice
def test_same_batch_twice(dense, monkeypatch):
    idx, d, ix, batch, exp, _ = dense
    info = ix.pair_cache_info()
    assert info["enabled"] == 1 and info["capacity_bytes"] == 2048 << 20 and info["min_rows"] == 1, info
    keys = {(frozenset(q.include), q.k, q.language) for q in batch if _served(d, q)}
    npairs = len({k[0] for k in keys})
    assert npairs >= 5, npairs
    first = _one_lane(ix, batch)
    d1 = _delta(ix, info)
    assert [_triples(g) for g in first] == exp
    # one fill per pair; a pair asked twice in the pass with another k or language fills once and
    # its second query finds the key taken
    assert d1["fills"] == npairs and d1["hits"] == 0 and d1["evictions"] == 0, d1
    assert d1["dropped"] == len(keys) - npairs, (d1, len(keys), npairs)
    assert ix.pair_cache_info()["entries"] == info["entries"] + npairs
    mid = ix.pair_cache_info()
    second = _one_lane(ix, batch)
    d2 = _delta(ix, mid)
    assert [_triples(g) for g in second] == exp
    assert d2["hits"] == len(keys) and d2["fills"] == 0 and d2["rows_served"] > 0, d2
    served_rows = sum(len(orc.term_search(d, sorted(k[0]), [], INF, NOW)) for k in keys)
    assert d2["rows_served"] == served_rows, (d2, served_rows)
    monkeypatch.setenv("YRWI_PAIR_CACHE", "0")
    off_info = ix.pair_cache_info()
    assert off_info["enabled"] == 0
    off = _one_lane(ix, batch)
    assert [_triples(g) for g in off] == exp
    d3 = _delta(ix, off_info)
    assert d3["hits"] == 0 and d3["misses"] == 0 and d3["fills"] == 0, d3
    monkeypatch.setenv("YRWI_PAIR_CACHE", "1")
    sync = ix.search_batch(batch)  # the synchronous entry point: one part per lane
    assert [_triples(g) for g in sync] == exp


# ------------------------------------------------------------------ 2: one cached pair, asked in every way
def test_cached_pair_variants(dense):
    idx, d, ix, batch, exp, (a, b, c) = dense
    ix.search_batch([_q([a, b])])  # filled here, if no earlier test did
    custom = RankingProfile("", "date=15,domlength=15,tf=10")
    variants = [dict(k=1), dict(k=100), dict(k=3000), dict(profile=None), dict(profile=custom),
                dict(profile=RankingProfile.date()), dict(language="de"), dict(language="zz", k=17)]
    for kw in variants:
        q = _q([b, a], **kw)
        info = ix.pair_cache_info()
        got = ix.search_batch([q])[0]
        assert _triples(got) == _oracle(d, q), kw
        dl = _delta(ix, info)
        assert dl["hits"] == 1 and dl["fills"] == 0 and dl["misses"] == 0, (kw, dl)
    # the authority profile counts hosts over the container: around the cache
    q = _q([a, b], profile=RankingProfile("", iu.C5))
    info = ix.pair_cache_info()
    got = ix.search_batch([q])[0]
    assert _triples(got) == _oracle(d, q)
    dl = _delta(ix, info)
    assert dl["hits"] == 0 and dl["misses"] == 0 and dl["fills"] == 0, dl
    # (the first authority batch stamped host ids into the records: every entry went)
    assert dl["invalidations"] >= 1 and ix.pair_cache_info()["entries"] == 0


# ------------------------------------------------------------------ 3: many tiles, several piece groups
def _rising_lists():
    """two lists of about 80 k urls of one universe of 100 k whose posintext rises along the url
    order: the smaller side's 1024-id tiles make more than 64 pieces (two piece groups), and every
    group of pieces overflows its SEGC segments, so k_shard_fin walks the run again"""
    n = 100_000
    rng = np.random.default_rng(41)
    uni = adv_rows(n, 5, "few")
    out = {}
    for j, (name, frac) in enumerate(((b"TERMriseA___", 0.85), (b"TERMriseB___", 0.80))):
        r = adv_rows(n, 6 + j, "few")
        r[:, :12] = uni[:, :12]
        p = np.minimum(65535, (np.arange(n) * 13) // 20 + 1 + j)
        r[:, 34], r[:, 35] = p >> 8, p & 255
        r[:, 38] = rng.integers(0, 256, n) * (rng.random(n) < 0.5)
        out[name] = r[rng.random(n) < frac]
    return out


def test_many_tiles_cold_against_hit():
    d = _rising_lists()
    A, B = list(d)
    assert min(len(d[A]), len(d[B])) > 64 * 1024
    ix = iu.open_index(d)
    try:
        date = RankingProfile.date()
        for prof in (None, date):
            q = _q([A, B], profile=prof, k=100)
            e = _oracle(d, q)
            info = ix.pair_cache_info()
            got = ix.search_batch([q])[0]
            dl = _delta(ix, info)
            assert _triples(got) == e, ("cold" if prof is None else "hit", dl)
            assert (dl["fills"], dl["hits"]) == ((1, 0) if prof is None else (0, 1)), dl
        info = ix.pair_cache_info()
        hit = ix.search_batch([_q([A, B], k=100)])[0]
        assert _delta(ix, info)["hits"] == 1
        assert _triples(hit) == _oracle(d, _q([A, B], k=100))
        joined = orc.term_search(d, [A, B], [], INF, NOW)
        e = ix.pair_cache_info()
        assert e["entries"] == 1 and e["rows_served"] >= 2 * len(joined)
        # the one entry holds more than 64 pieces: k_piece_merge folds it in two groups or more
        assert e["pieces"] > 64, e
        # and a tile's run of the fold overflows: the fold keeps a record per rise of posintext, SEGC = 32
        # of them per piece, and every 64 consecutive joined rows here rise more than 32 times
        p = (joined[:, 34].astype(np.int64) << 8) | joined[:, 35]
        rises = np.add.reduceat((np.diff(p) > 0).astype(np.int64), np.arange(0, len(p) - 1, 64))
        assert rises[:-1].min() > 32, int(rises[:-1].min())
    finally:
        ix.close()


# ------------------------------------------------------------------ 4: invalidation
def test_every_index_change_invalidates():
    idx = synth.build_index(synth.preset("tiny"))
    lists = idx.as_dict()
    order = [int(t) for t in np.argsort(-idx.sizes, kind="stable")]
    a, b, c = (idx.hashes[t] for t in order[:3])
    ix = iu.open_index(lists)
    state = {"lists": lists}

    def ask(what, expect):
        """the pair's query: equal to the oracle on the index as it stands, and a fill or a hit"""
        q = _q([a, b])
        info = ix.pair_cache_info()
        got = ix.search_batch([q])[0]
        dl = _delta(ix, info)
        assert _triples(got) == _oracle(state["lists"], q), (what, dl)
        assert (dl["fills"], dl["hits"]) == ((1, 0) if expect == "fill" else (0, 1)), (what, dl)
        return dl

    def changed(what, fn):
        info = ix.pair_cache_info()
        fn()
        dl = _delta(ix, info)
        assert dl["invalidations"] >= 1, (what, dl)
        assert ix.pair_cache_info()["entries"] == 0, what
        ask(what, "fill")
        ask(what + ", again", "hit")

    try:
        ask("cold", "fill")
        ask("warm", "hit")
        joined = orc.term_search(lists, [a, b], [], INF, NOW)
        assert len(joined) > 8

        def add_first():  # a new url that sorts before every other, in both lists: every url id shifts
            u = iu.url(1, prefix=b"AA")
            assert all(ur.url_key(u) < ur.url_key(r[:12]) for l in state["lists"].values() for r in l[:1])
            state["lists"], _ = iu.checked_add(ix, state["lists"], [a, b], iu.rows(idx, [u, u]))

        def add_unrelated():
            state["lists"], _ = iu.checked_add(ix, state["lists"], [c], iu.rows(idx, [iu.url(7)]))

        def remove_some():
            urls = [bytes(r[:12]) for r in joined[2:6]]
            state["lists"], _ = iu.checked_remove(ix, state["lists"], urls)

        def retention():
            days = np.sort(rr.days_of(state["lists"][a]))
            cut = int(days[len(days) // 3])
            new, _, _ = rr.apply_retention(state["lists"], cut, 0, [a])
            st, _ = ix.retain(min_day=cut, terms=[a])
            assert st["removed"] > 0
            state["lists"] = {t: l for t, l in new.items() if len(l)}

        def remove_host():
            now = orc.term_search(state["lists"], [a, b], [], INF, NOW)
            host = hr.host_of(bytes(now[len(now) // 2][:12]))
            new, _ = hr.apply_remove_hosts(state["lists"], [host])
            st = ix.remove_hosts([host])
            assert st["removed"] > 0
            state["lists"] = {t: l for t, l in new.items() if len(l)}

        def authority():  # the first authority batch stamps host ids into every record
            q = _q([a, c], profile=RankingProfile("", iu.C5))
            assert _triples(ix.search_batch([q])[0]) == _oracle(state["lists"], q)

        changed("add_postings, a url sorting first", add_first)
        assert bytes(orc.term_search(state["lists"], [a, b], [], INF, NOW)[0][:12]) == iu.url(1, prefix=b"AA")
        changed("an unrelated list", add_unrelated)
        changed("remove_postings", remove_some)
        changed("retention", retention)
        changed("removal by host", remove_host)
        changed("host-id stamping", authority)
        ask("authority again: nothing stamped", "hit")
        q = _q([a, c], profile=RankingProfile("", iu.C5))
        info = ix.pair_cache_info()
        assert _triples(ix.search_batch([q])[0]) == _oracle(state["lists"], q)
        assert _delta(ix, info)["invalidations"] == 0
        ask("after the second authority batch", "hit")
    finally:
        ix.close()


# ------------------------------------------------------------------ 5: the clamp day
def test_clamp_day_is_part_of_the_key():
    idx = synth.build_index(synth.preset("dense"))
    day = NOW // DAY
    urls = [iu.url(i) for i in range(600)]
    lm = day - 2 + (np.arange(600) % 7)  # lastModified from two days before "now" to four days after
    d = {b"TERMdayA____": iu.rows(idx, urls[:500], lm=lm[:500]),
         b"TERMdayB____": iu.rows(idx, urls[100:], lm=lm[100:][::-1].copy(), start=3)}
    A, B = list(d)
    date = RankingProfile.date()
    ix = iu.open_index(d)
    try:
        hits = {}
        for now, want in ((NOW, (1, 0)), (NOW + 2 * DAY, (1, 0)), (NOW + 5000, (0, 1)), (NOW + 2 * DAY + 5000, (0, 1))):
            for prof in (None, date):
                q = _q([A, B], now_ms=now, profile=prof, k=400)
                info = ix.pair_cache_info()
                got = ix.search_batch([q], rows=True)[0]
                dl = _delta(ix, info)
                e = _oracle(d, q)
                qu.same_rows(got, e, orc.term_search(d, [A, B], [], INF, now), (now - NOW, prof is date))
                assert (dl["fills"], dl["hits"]) == (want if prof is None else (0, 1)), (now - NOW, dl)
                hits[now, prof is date] = _triples(got)
        assert ix.pair_cache_info()["entries"] == 2
        assert hits[NOW, True] != hits[NOW + 2 * DAY, True]  # the clamp shows in the date term
    finally:
        ix.close()


# ------------------------------------------------------------------ 6: eviction with batches in flight
def _three_lists(n=16_000, frac=0.9):
    rng = np.random.default_rng(9)
    uni = adv_rows(n, 21, "edge")
    out = {}
    for j, name in enumerate((b"TERMevA_____", b"TERMevB_____", b"TERMevC_____")):
        r = adv_rows(n, 22 + j, "edge")
        r[:, :12] = uni[:, :12]
        out[name] = r[rng.random(n) < frac]
    return out


def test_eviction_in_flight(monkeypatch):
    monkeypatch.setenv("YRWI_PAIR_CACHE_MB", "1")
    d = _three_lists()
    A, B, C = list(d)
    pairs = [[A, B], [A, C], [B, C]]
    rows = [len(orc.term_search(d, p, [], INF, NOW)) for p in pairs]
    # an entry takes 36 B per row and more: any two fit the 1 MiB, the three do not
    assert all(36 * (r0 + r1) < (1 << 20) - 65536 for r0 in rows for r1 in rows) and 36 * sum(rows) > 1 << 20, rows
    exp = [_oracle(d, _q(p)) for p in pairs]
    ix = iu.open_index(d)
    try:
        assert ix.search_batch([_q([A])])  # (builds the url ids: the block is reserved)
        info = ix.pair_cache_info()
        assert info["capacity_bytes"] == 1 << 20 and info["enabled"] == 1, info
        for rnd in range(2):
            pend = [ix.submit([_q(pairs[(i + rnd) % 3])]) for i in range(8)]
            for i, p in enumerate(pend):
                assert _triples(p.result()[0]) == exp[(i + rnd) % 3], (rnd, i)
        for rnd in range(2):  # one at a time: nothing pinned, so the absent pair displaces another
            for i in range(3):
                assert _triples(ix.search_batch([_q(pairs[i])])[0]) == exp[i], ("alone", rnd, i)
        end = ix.pair_cache_info()
        assert end["evictions"] > 0 and end["entries"] <= 2 and end["bytes"] <= 1 << 20, end
        assert end["hits"] + end["fills"] > 0 and end["fills"] - end["evictions"] == end["entries"], end
    finally:
        ix.close()


# ------------------------------------------------------------------ 7: one cold batch, eight times in flight
def test_cold_batch_in_flight(dense):
    idx, d, _, batch, exp, _ = dense
    ix = iu.open_index(d)
    try:
        pend = [ix.submit(batch) for _ in range(8)]
        for i, p in enumerate(pend):
            assert [_triples(g) for g in p.result()] == exp, i
        npairs = len({frozenset(q.include) for q in batch if _served(d, q)})
        info = ix.pair_cache_info()
        # two lanes that miss a key together both join it; one entry stays
        assert info["entries"] == npairs and info["fills"] == npairs and info["evictions"] == 0, (info, npairs)
        assert info["hits"] + info["dropped"] > 0, info
        again = ix.submit(batch).result()
        assert [_triples(g) for g in again] == exp
        assert ix.pair_cache_info()["fills"] == npairs
    finally:
        ix.close()


# ------------------------------------------------------------------ 8: the rows of the hits
def test_rows_on_a_hit(dense, monkeypatch):
    idx, d, ix, batch, exp, (a, b, c) = dense
    monkeypatch.setenv("YRWI_PAIR_CACHE", "0")
    cold = _one_lane(ix, batch, rows=True)
    monkeypatch.setenv("YRWI_PAIR_CACHE", "1")
    _one_lane(ix, batch, rows=True)  # fills what is not there yet
    info = ix.pair_cache_info()
    hit = _one_lane(ix, batch, rows=True)
    dl = _delta(ix, info)
    assert dl["hits"] > 0 and dl["fills"] == 0, dl
    assert [[(h.urlhash, h.score, h.tiebreak, h.row) for h in g] for g in hit] == \
           [[(h.urlhash, h.score, h.tiebreak, h.row) for h in g] for g in cold]
    for qi, (q, g) in enumerate(zip(batch, hit)):
        if _served(d, q):
            qu.same_rows(g, exp[qi], orc.term_search(d, q.include, [], INF, q.now_ms), ("hit", qi))


# ------------------------------------------------------------------ 9: a sharded context has no pair cache
def test_sharded_context_reports_the_cache_off():
    world = 2
    full = synth.preset("tiny")
    whole_idx = synth.build_index(full)
    whole = whole_idx.as_dict()
    order = [int(t) for t in np.argsort(-whole_idx.sizes, kind="stable")]
    a, b = (whole_idx.hashes[t] for t in order[:2])
    shards = [synth.build_index(full.shard(r, world)) for r in range(world)]

    def fn(r, ix):
        q = _q([a, b])
        return [_triples(ix.search_batch([q])[0]) for _ in range(2)], ix.pair_cache_info()

    e = _oracle(whole, _q([a, b]))
    for r, (got, info) in enumerate(iu.run_parts([p.as_dict() for p in shards], world, fn)):
        assert got == [e, e], r
        assert info["enabled"] == 0 and info["capacity_bytes"] == 0 and info["entries"] == 0, (r, info)
        assert info["hits"] == info["misses"] == info["fills"] == 0, (r, info)
