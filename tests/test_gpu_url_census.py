"""The url census on the device (yrwi_url_census / yrwi_host_url_census) against
tests/url_census_ref.py: on the `tiny` corpus as generated (48,200 urls of 1 .. 5 references, 36,406
hosts) and re-hosted (64 hosts), on the hand-made lists of tests/url_census_cases.py and on the large
index of tests/span_cases.py.  Urls, hosts, counts and the counters of the call's statistics are
compared exactly, in both orders and both forms; wherever the path is not the subject, on both forced
paths (YRWI_UCENSUS_PATH)."""

import ctypes

import numpy as np
import pytest

import host_ref as hr
import index_util as iu
import span_cases as sc
import update_ref as ur
import url_census_cases as ucc
import url_census_ref as ucr
from yacy_search_server_amd import _lib, synth
from yacy_search_server_amd._lib import YrwiError

pytestmark = pytest.mark.gpu

PATHS = ("hist", "sort")
KNOB = "YRWI_UCENSUS_PATH"


@pytest.fixture(scope="module")
def tiny():
    """(synthetic index, {"raw": lists, "rehosted": lists}, {corpus: url -> references}); the facts the
    cases rely on (tests/test_url_census_ref.py checks them without a GPU)"""
    idx = synth.build_index(synth.preset("tiny"))
    raw = idx.as_dict()
    corp = {"raw": raw, "rehosted": hr.rehost(raw)}
    have = {name: ucr.tally(lists) for name, lists in corp.items()}
    for name in corp:
        assert len(corp[name]) == 200 and sum(have[name].values()) == 60050 and len(have[name]) == 48200
    return idx, corp, have


@pytest.fixture(scope="module")
def opened(tiny):
    """one context per corpus for the cases that change nothing"""
    idx, corp, have = tiny
    ixs = {name: iu.open_index(lists) for name, lists in corp.items()}
    yield ixs
    for ix in ixs.values():
        ix.close()


@pytest.fixture(scope="module")
def bound():
    b = ucc.boundary()
    ix = iu.open_index(b.lists)
    yield b, ix
    ix.close()


@pytest.fixture(autouse=True)
def _default_path(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)


def _urls(ix, exp, terms=None, hosts=None, order="refs", min_refs=1, top=None):
    """the url form; urls and references must equal exp = (urls, refs, counters)"""
    urls, refs, st = ix.url_census(terms, hosts, order, min_refs, top)
    assert refs.dtype == np.int64 and len(urls) == len(refs)
    assert urls == list(exp[0]) and list(refs) == list(exp[1]), (order, min_refs, st)
    for k, v in exp[2].items():
        assert st[k] == v, (k, st, exp[2])
    return st


def _hosts(ix, exp, terms=None, order="count", min_urls=1, top=None):
    """the host form; exp = (hosts, urls, postings, counters)"""
    hosts, nurls, posts, st = ix.host_url_census(terms, order, min_urls, top)
    assert nurls.dtype == posts.dtype == np.int64
    assert hosts == list(exp[0]) and list(nurls) == list(exp[1]) and list(posts) == list(exp[2]), (order, min_urls, st)
    for k, v in exp[3].items():
        assert st[k] == v, (k, st, exp[3])
    return st


def _both(monkeypatch, fn):
    """fn(path) on both forced paths -> their results"""
    out = []
    for p in PATHS:
        monkeypatch.setenv(KNOB, p)
        out.append(fn(p))
    monkeypatch.delenv(KNOB)
    return out


def _ran(st, path):
    assert st["path"] == _lib.UCENSUS_PATHS[path], (st, path)


def _raw_urls(ix, terms, hosts, order, min_refs, cap, urls, refs, st=True, nout=True):
    """yrwi_url_census as it is: -> (rc, nout, stats)"""
    tb = np.frombuffer(b"".join(terms or ()), dtype=np.uint8)
    hb = np.frombuffer(b"".join(hosts or ()), dtype=np.uint8)
    n, s = ctypes.c_int64(-7), _lib.CUCensusStats()
    rc = _lib.lib().yrwi_url_census(ix._h, tb.ctypes.data if len(tb) else None, len(tb) // 12,
                                    hb.ctypes.data if len(hb) else None, len(hb) // 6, order, min_refs,
                                    None if urls is None else urls.ctypes.data,
                                    None if refs is None else refs.ctypes.data, cap,
                                    ctypes.byref(n) if nout else None, ctypes.byref(s) if st else None)
    return rc, n.value, s


def _raw_hosts(ix, terms, order, min_urls, cap, hosts, nurls, posts, st=True, nout=True):
    """yrwi_host_url_census as it is: -> (rc, nout, stats)"""
    tb = np.frombuffer(b"".join(terms or ()), dtype=np.uint8)
    n, s = ctypes.c_int64(-7), _lib.CUCensusStats()
    rc = _lib.lib().yrwi_host_url_census(ix._h, tb.ctypes.data if len(tb) else None, len(tb) // 12, order, min_urls,
                                         None if hosts is None else hosts.ctypes.data,
                                         None if nurls is None else nurls.ctypes.data,
                                         None if posts is None else posts.ctypes.data, cap,
                                         ctypes.byref(n) if nout else None, ctypes.byref(s) if st else None)
    return rc, n.value, s


# ------------------------------------------------------------------ 1: both corpora, every list
@pytest.mark.parametrize("name", ["raw", "rehosted"])
def test_every_list(tiny, opened, monkeypatch, name):
    idx, corp, have = tiny
    ix = opened[name]
    bad, dict_urls = ix.check_url_ids()
    assert bad == 0 and dict_urls == 48200

    def run(path):
        for order in ucr.ORDERS:
            exp = ucr.census(corp[name], order=order, have=have[name])
            st = _urls(ix, exp, order=order)
            _ran(st, path)
            assert sum(exp[1]) == st["postings"] == 60050 and st["urls"] == 48200 and st["dict_urls"] == dict_urls
            assert st["max_refs"] == 5 and st["t_count_ns"] > 0 and st["t_total_ns"] >= st["t_count_ns"]
        for order in ucr.HOST_ORDERS:
            exp = ucr.host_census(corp[name], order=order, have=have[name])
            st = _hosts(ix, exp, order=order)
            _ran(st, path)
            assert sum(exp[1]) == st["urls"] == 48200 and sum(exp[2]) == 60050 and st["dict_urls"] == dict_urls

    _both(monkeypatch, run)


# ------------------------------------------------------------------ 2: named lists
def test_named_lists(tiny, opened, monkeypatch):
    idx, corp, have = tiny
    lists, ix = corp["raw"], opened["raw"]
    named = sorted(lists)[::7][:28]
    terms = named + [named[3], iu.term(77, b"-u")]  # 30 terms named: one of them twice, one nobody has
    assert len(set(terms)) == 29 and len(terms) == 30
    h = ucr.tally(lists, terms)
    one = named[5]

    def run(path):
        got = []
        for order in ucr.ORDERS:
            exp = ucr.census(lists, terms, order=order, have=h)
            assert exp[2]["lists"] == 28 and exp[2]["postings"] < 60050
            _urls(ix, exp, terms, order=order)
            got.append(ix.url_census(terms, None, order)[:2])
        for order in ucr.HOST_ORDERS:
            _hosts(ix, ucr.host_census(lists, terms, order, have=h), terms, order)
            got.append(ix.host_url_census(terms, order)[:3])
        # one list alone: its urls, one reference each
        exp = ucr.census({one: lists[one]}, order="url")
        assert exp[1] == [1] * len(lists[one])
        st = _urls(ix, exp, [one], order="url")
        if path:
            _ran(st, path)
        _hosts(ix, ucr.host_census({one: lists[one]}, order="host"), [one], "host")
        return [(a, [list(x) for x in rest]) for a, *rest in got]

    forced = _both(monkeypatch, run)
    assert forced[0] == forced[1]
    assert run(None) == forced[0]  # the path the call chooses itself returns the same
    urls, refs, st = ix.url_census([], None, "refs")
    assert urls == [] and len(refs) == 0 and st["postings"] == 0
    hosts, nurls, posts, st = ix.host_url_census([], "count")
    assert hosts == [] and len(nurls) == len(posts) == 0 and st["postings"] == 0
    urls, refs, st = ix.url_census([iu.term(77, b"-u")], None, "refs")
    assert urls == [] and (st["lists"], st["postings"], st["urls"], st["launches"], st["syncs"]) == (0, 0, 0, 0, 0)


# ------------------------------------------------------------------ 3: boundaries
def test_boundaries(bound, monkeypatch):
    b, ix = bound
    have = ucr.tally(b.lists)
    bad, dict_urls = ix.check_url_ids()
    assert bad == 0 and dict_urls == len(b.hashes) + len(ucc.RUNS)

    def run(path):
        for order in ucr.ORDERS:
            st = _urls(ix, ucr.census(b.lists, order=order, have=have), order=order)
            _ran(st, path)
            assert st["max_refs"] == 1025 and st["dict_urls"] == dict_urls
        urls, refs, _ = ix.url_census(None, None, "url")
        assert (urls[0], urls[-1]) == (ucc.FIRST_URL, ucc.LAST_URL)  # dictionary id 0 and id dict_urls - 1
        assert set(b.hashes) <= set(urls)  # urls that differ only in the last 8 key bits stay distinct
        for order in ucr.HOST_ORDERS:
            _hosts(ix, ucr.host_census(b.lists, order=order, have=have), order=order)
        hosts, nurls, posts, _ = ix.host_url_census(None, "host")
        assert (hosts[0], hosts[-1]) == (ucc.FIRST_HOST, ucc.LAST_HOST)  # the hosts of key 0 and key 2^36 - 1
        for L in ucc.RUNS:  # one url in each of L one-row lists
            exp = ([ucc.run_url(L)], [L], dict(lists=L, postings=L, urls=1, urls_hosted=1, urls_passing=1, max_refs=L))
            _urls(ix, exp, b.runs[L], order="refs")
            _hosts(ix, ([ucc.RUN_HOST], [1], [L], dict(hosts=1, hosts_passing=1)), b.runs[L], "count")
        for n in ucc.SELECTIONS:  # 1023, 1024 and 1025 postings
            terms = ucc.selection(b, n)
            for order in ucr.ORDERS:
                st = _urls(ix, ucr.census(b.lists, terms, order=order), terms, order=order)
                assert st["postings"] == n
            _hosts(ix, ucr.host_census(b.lists, terms, "count"), terms, "count")
        # the two edge hosts as a host set
        _urls(ix, ucr.census(b.lists, None, [ucc.LAST_HOST, ucc.FIRST_HOST], "url", have=have), None,
              [ucc.LAST_HOST, ucc.FIRST_HOST], "url")

    _both(monkeypatch, run)


# ------------------------------------------------------------------ 4: dead ids and shifted ids
def test_dead_and_shifted_ids(tiny, monkeypatch):
    idx, corp, have = tiny
    lists = corp["raw"]
    # a few urls of two references whose lists are small: the lists that change hold less than a quarter of the
    # postings, so the dictionary is updated incrementally and keeps the keys of the removed postings
    small = set(sorted(lists, key=lambda t: (len(lists[t]), t))[:60])
    where = {}
    for t, l in lists.items():
        for r in l:
            where.setdefault(bytes(r[:12]), []).append(t)
    gone = sorted(u for u, ts in where.items() if len(ts) >= 2 and set(ts) <= small)[:8]
    assert len(gone) == 8 and 4 * sum(len(lists[t]) for t in {t for u in gone for t in where[u]}) < 60050
    ix = iu.open_index(lists, url_ids=True)
    try:
        left, _ = iu.checked_remove(ix, lists, gone)
        bad, dict_urls = ix.check_url_ids()
        assert bad == 0 and dict_urls == 48200  # the keys of the removed postings stay in the dictionary
        h = ucr.tally(left)
        assert len(h) == 48200 - 8

        def dead(path):
            for order in ucr.ORDERS:
                st = _urls(ix, ucr.census(left, order=order, have=h), order=order)
                assert (st["dict_urls"], st["urls"], st["max_refs"]) == (48200, 48192, 5)
            urls = ix.url_census(None, None, "url")[0]
            assert not set(gone) & set(urls)
            _hosts(ix, ucr.host_census(left, order="count", have=h), order="count")

        _both(monkeypatch, dead)
        # urls new to the dictionary, below, between and above the old ones: the ids behind them shift
        new = [b"AAAAAAAAAAAB"] + [iu.url(i) for i in range(40)] + [b"___________-"]
        new = sorted(new, key=ur.url_key)
        assert not set(new) & set(have["raw"])
        some = sorted(left, key=lambda t: (len(left[t]), t))[:6]
        terms = [t for t in some for _ in new]
        rows = np.concatenate([iu.rows(idx, new, start=j) for j in range(len(some))])
        after, _ = iu.checked_add(ix, left, terms, rows)
        h2 = ucr.tally(after)
        assert len(h2) == len(h) + len(new) and h2[new[0]] == 6

        def shifted(path):
            for order in ucr.ORDERS:
                st = _urls(ix, ucr.census(after, order=order, have=h2), order=order)
                assert st["max_refs"] == 6
            _hosts(ix, ucr.host_census(after, order="host", have=h2), order="host")

        _both(monkeypatch, shifted)
        assert ix.check_url_ids()[0] == 0
    finally:
        ix.close()


# ------------------------------------------------------------------ 5: host set
def test_host_set(tiny, opened, monkeypatch):
    idx, corp, have = tiny
    lists, ix, h = corp["raw"], opened["raw"], have["raw"]
    all_hosts = sorted({hr.host_of(u) for u in h})
    assert len(all_hosts) == 36406

    def run(path):
        for n in (1, _lib.HOST_LDS_MAX, _lib.HOST_LDS_MAX + 1):
            hs = ucc.host_set(all_hosts, n)
            for order in ucr.ORDERS:
                exp = ucr.census(lists, None, hs, order, have=h)
                assert 0 < exp[2]["urls_hosted"] < 48200
                _urls(ix, exp, None, hs, order)
            exp = ucr.census(lists, None, hs, "refs", 2, have=h)
            _urls(ix, exp, None, hs, "refs", 2)
        exp = ucr.census(lists, None, [ucc.NOBODY], "refs", have=h)
        assert exp[:2] == ([], []) and exp[2]["urls_hosted"] == 0
        st = _urls(ix, exp, None, [ucc.NOBODY], "refs")
        assert st["urls"] == 48200

    _both(monkeypatch, run)
    # no host named equals every host named (sort path alone: the set is searched in global memory)
    monkeypatch.setenv(KNOB, "sort")
    a = ix.url_census(None, None, "refs", top=500)
    b = ix.url_census(None, all_hosts, "refs", top=500)
    assert (a[0], list(a[1])) == (b[0], list(b[1]))
    assert b[2]["urls_hosted"] == a[2]["urls_hosted"] == a[2]["urls"] == 48200


# ------------------------------------------------------------------ 6: minimum and top
def test_minimum_and_top(tiny, opened, monkeypatch):
    idx, corp, have = tiny
    lists, ix, h = corp["raw"], opened["raw"], have["raw"]
    full = ucr.census(lists, order="refs", have=h)
    rl, rh = corp["rehosted"], have["rehosted"]
    hfull = ucr.host_census(rl, order="count", have=rh)

    def run(path):
        for cap in (10, 100, 48200, 50000):  # a prefix of the full order: the tie-break by url holds inside it
            _urls(ix, (full[0][:cap], full[1][:cap], full[2]), order="refs", top=cap)
        by_url = ucr.census(lists, order="url", have=h)
        _urls(ix, (by_url[0][:100], by_url[1][:100], by_url[2]), order="url", top=100)
        for m in (2, 3, 4, 5):
            for order in ucr.ORDERS:
                exp = ucr.census(lists, order=order, min_refs=m, have=h)
                assert 0 < exp[2]["urls_passing"] < 48200
                _urls(ix, exp, order=order, min_refs=m)
        st = _urls(ix, ucr.census(lists, min_refs=6, have=h), min_refs=6)  # above every count
        assert st["urls_passing"] == 0 and st["urls"] == 48200
        for m in (0, -5):  # a minimum below 1 is 1; cap 0 with NULL buffers fills the statistics alone
            rc, n, st = _raw_urls(ix, None, None, _lib.UCENSUS_BY_REFS, m, 0, None, None)
            assert (rc, n) == (0, 0)
            assert (st.lists, st.postings, st.urls, st.urls_passing, st.max_refs) == (200, 60050, 48200, 48200, 5)
            rc, n, st = _raw_hosts(opened["rehosted"], None, _lib.CENSUS_BY_COUNT, m, 0, None, None, None)
            assert (rc, n, st.hosts, st.hosts_passing, st.urls) == (0, 0, 64, 64, 48200)
        # the host form, on the re-hosted corpus
        hx = opened["rehosted"]
        for cap in (10, 64, 100):
            _hosts(hx, (hfull[0][:cap], hfull[1][:cap], hfull[2][:cap], hfull[3]), order="count", top=cap)
        for m in (149, 1000, 10235):
            for order in ucr.HOST_ORDERS:
                exp = ucr.host_census(rl, order=order, min_urls=m, have=rh)
                assert 0 < exp[3]["hosts_passing"] < 64
                _hosts(hx, exp, order=order, min_urls=m)
        st = _hosts(hx, ucr.host_census(rl, min_urls=10236, have=rh), min_urls=10236)
        assert st["hosts_passing"] == 0 and st["hosts"] == 64
        # st and nout may be NULL
        urls, refs = np.zeros((3, 12), np.uint8), np.zeros(3, np.int64)
        assert _raw_urls(ix, None, None, _lib.UCENSUS_BY_REFS, 1, 3, urls, refs, st=False, nout=False)[0] == 0
        assert [bytes(u) for u in urls] == full[0][:3] and list(refs) == full[1][:3]
        hosts, nurls, posts = np.zeros((3, 6), np.uint8), np.zeros(3, np.int64), np.zeros(3, np.int64)
        assert _raw_hosts(hx, None, _lib.CENSUS_BY_COUNT, 1, 3, hosts, nurls, posts, st=False, nout=False)[0] == 0
        assert ([bytes(x) for x in hosts], list(nurls), list(posts)) == (hfull[0][:3], hfull[1][:3], hfull[2][:3])

    _both(monkeypatch, run)


# ------------------------------------------------------------------ 7: agreement with the neighbours
def test_agrees_with_its_neighbours(tiny, monkeypatch):
    idx, corp, have = tiny
    lists = corp["rehosted"]
    ix = iu.open_index(lists)
    try:
        named = sorted(lists)[:40]

        def run(path):
            for terms in (None, named):
                urls, refs, _ = ix.url_census(terms, None, "refs", top=3000)
                assert list(ix.url_references(urls, terms, fetch=False)[0]) == list(refs)
                hosts, nurls, posts, _ = ix.host_url_census(terms, "host")
                ch, cc, _ = ix.host_census(terms, "host")
                assert (hosts, list(posts)) == (ch, list(cc))

        _both(monkeypatch, run)
        # without the largest host: its urls are gone, every other count is unchanged
        full = ucr.host_census(lists, order="count", have=have["rehosted"])
        big = full[0][0]
        rm = ix.remove_hosts([big], None)
        assert rm["removed"] == full[2][0]

        def after(path):
            st = _hosts(ix, (full[0][1:], full[1][1:], full[2][1:], dict(hosts=63, urls=48200 - full[1][0])), order="count")
            assert st["dict_urls"] == 48200 - full[1][0]  # (every list changed: the dictionary was rebuilt in full)
            urls = ix.url_census(None, None, "url")[0]
            assert len(urls) == 48200 - full[1][0] and not any(hr.host_of(u) == big for u in urls)

        _both(monkeypatch, after)
    finally:
        ix.close()


# ------------------------------------------------------------------ 8: more than one tile per workgroup
@pytest.fixture(scope="module")
def span_index():
    c = sc.corpus()
    ix = iu.open_index(c.lists())
    yield c, ix
    ix.close()


@pytest.mark.parametrize("path", PATHS)
def test_two_tiles_per_workgroup(span_index, monkeypatch, path):
    """the index of tests/span_cases.py: a workgroup's span is two tiles.  Every url lies in one list"""
    c, ix = span_index
    monkeypatch.setenv(KNOB, path)
    o = np.argsort(c.key, kind="stable")[:100]
    urls, refs, st = ix.url_census(None, None, "url", top=100)
    assert urls == sc.url_hashes(c.hi[o], c.host[o]) and list(refs) == [1] * 100
    _ran(st, path)
    want = dict(lists=len(c.terms), postings=c.n, dict_urls=c.n, urls=c.n, urls_hosted=c.n, urls_passing=c.n, max_refs=1)
    assert {k: st[k] for k in want} == want, st
    hk, hn = np.unique(c.host, return_counts=True)
    hosts, nurls, posts, st = ix.host_url_census(None, "host", top=100)
    assert hosts == sc.host_hashes(hk[:100]) and list(nurls) == list(posts) == [int(x) for x in hn[:100]]
    assert (st["hosts"], st["hosts_passing"], st["urls"]) == (len(hk), len(hk), c.n)
    keys = sc.host_set(sc.N_H64)
    st = ix.url_census(None, sc.host_hashes(keys), "url", top=0)[2]
    assert st["urls_hosted"] == int(np.isin(c.host, keys).sum()) == int(c.marked.sum())


# ------------------------------------------------------------------ 9: changes nothing, allocates once
def test_changes_nothing_and_allocates_once(tiny, monkeypatch):
    idx, corp, have = tiny
    lists, h = corp["rehosted"], have["rehosted"]
    ix = iu.open_index(lists)
    try:
        ix.build_url_ids()
        info, stats = ix.index_info(), ix.stats()
        one = [sorted(lists)[0]]
        for path in PATHS:
            monkeypatch.setenv(KNOB, path)
            _urls(ix, ucr.census(lists, order="refs", have=h))
            r0 = _lib.lib().yrwi_realloc_events()
            sts = {}
            for order in ("url", "refs", "url"):
                sts[order, None] = _urls(ix, ucr.census(lists, order=order, have=h), order=order)
                sts[order, 1] = ix.url_census(one, None, order)[2]
            for order in ucr.HOST_ORDERS:
                sts[order, None] = _hosts(ix, ucr.host_census(lists, order=order, have=h), order=order)
                sts[order, 1] = ix.host_url_census(one, order)[3]
            assert _lib.lib().yrwi_realloc_events() - r0 == 0
            # one named list and every list: equal launches and syncs on the same path, order and form
            for order in ucr.ORDERS + ucr.HOST_ORDERS:
                a, b = sts[order, 1], sts[order, None]
                assert a["lists"] == 1 and b["lists"] == 200 and a["path"] == b["path"] == _lib.UCENSUS_PATHS[path]
                assert (a["launches"], a["syncs"]) == (b["launches"], b["syncs"]) and a["launches"] > 0 < a["syncs"]
        assert ix.index_info() == info and ix.stats() == stats
        for t, l in lists.items():
            assert ix.get_size(t) == len(l), t
            assert ix.get_list(t).tobytes() == l.tobytes(), t
        assert ix.index_info() == info and ix.check_url_ids()[0] == 0
    finally:
        ix.close()


# ------------------------------------------------------------------ 10: errors write nothing
def test_errors_write_nothing(tiny, opened, monkeypatch):
    idx, corp, have = tiny
    ix, lists, h = opened["rehosted"], corp["rehosted"], have["rehosted"]
    some = sorted(lists)[:3]
    good = ucr.census(lists, order="url", have=h, top=50)
    hgood = ucr.host_census(lists, order="host", have=h)
    bad_term, bad_host = [some[0], b"bad#term_ash"], [hr.host_name(0), b"b#dhst"]
    ucases = [(bad_term, None, _lib.UCENSUS_BY_REFS, 8, -2), (None, bad_host, _lib.UCENSUS_BY_REFS, 8, -2),
              (None, None, 2, 8, -1), (None, None, -1, 8, -1), (None, None, _lib.UCENSUS_BY_URL, -1, -1)]
    hcases = [(bad_term, _lib.CENSUS_BY_COUNT, 8, -2), (None, 2, 8, -1), (None, -1, 8, -1),
              (None, _lib.CENSUS_BY_HOST, -1, -1)]

    def run(path):
        for terms, hosts, order, cap, want in ucases:
            urls, refs = np.full((8, 12), 0xA5, np.uint8), np.full(8, -0x5A5A, np.int64)
            rc, n, _ = _raw_urls(ix, terms, hosts, order, 1, cap, urls, refs)
            assert rc == want, (terms, hosts, order, cap, rc)
            assert (urls == 0xA5).all() and (refs == -0x5A5A).all() and n == -7
            assert _lib.lib().yrwi_last_error(ix._h)
            _urls(ix, good, order="url", top=50)  # a following good call is right
        for terms, order, cap, want in hcases:
            hosts, nurls, posts = np.full((8, 6), 0xA5, np.uint8), np.full(8, -0x5A5A, np.int64), np.full(8, -3, np.int64)
            rc, n, _ = _raw_hosts(ix, terms, order, 1, cap, hosts, nurls, posts)
            assert rc == want, (terms, order, cap, rc)
            assert (hosts == 0xA5).all() and (nurls == -0x5A5A).all() and (posts == -3).all() and n == -7
            assert _lib.lib().yrwi_last_error(ix._h)
            _hosts(ix, hgood, order="host")
        # a capacity without a buffer
        for urls, refs in ((None, np.zeros(8, np.int64)), (np.zeros((8, 12), np.uint8), None), (None, None)):
            rc, n, _ = _raw_urls(ix, None, None, _lib.UCENSUS_BY_REFS, 1, 8, urls, refs)
            assert (rc, n) == (-1, -7)
            assert (urls is None or not urls.any()) and (refs is None or not refs.any())
        for k in range(3):
            bufs = [np.zeros((8, 6), np.uint8), np.zeros(8, np.int64), np.zeros(8, np.int64)]
            bufs[k] = None
            rc, n, _ = _raw_hosts(ix, None, _lib.CENSUS_BY_COUNT, 1, 8, *bufs)
            assert (rc, n) == (-1, -7) and not any(x.any() for x in bufs if x is not None)

    _both(monkeypatch, run)
    with pytest.raises(YrwiError) as e:
        ix.url_census([b"bad#term_ash"], None, "refs")
    assert e.value.rc == -2
    with pytest.raises(YrwiError) as e:
        ix.url_census(None, [b"b#dhst"], "refs")
    assert e.value.rc == -2
    with pytest.raises(KeyError):
        ix.url_census(None, None, "size")
    with pytest.raises(KeyError):
        ix.host_url_census(None, "refs")
    _urls(ix, good, order="url", top=50)


# ------------------------------------------------------------------ 11: two shards in one process
def test_two_shards(tiny, monkeypatch):
    """world 2 over the loopback transport: each shard holds its url-hash range of the lists and is asked the
    same thing; its census is the reference on its range, the ranks' urls are disjoint and together the whole
    corpus's, and a host's counts add up"""
    idx, corp, have = tiny
    lists = corp["rehosted"]
    world = 2
    parts = iu.split_by_rank(lists, world)

    def fn(r, ix):
        return ([ix.url_census(None, None, o) for o in ucr.ORDERS],
                [ix.host_url_census(None, o) for o in ucr.HOST_ORDERS])

    for path in PATHS:
        monkeypatch.setenv(KNOB, path)
        out = iu.run_parts(parts, world, fn)
        seen, nurls, posts = {}, {}, {}
        for r in range(world):
            ph = ucr.tally(parts[r])
            assert len(ph) > 0
            for (urls, refs, st), o in zip(out[r][0], ucr.ORDERS):
                eu, er, est = ucr.census(parts[r], order=o, have=ph)
                assert (urls, list(refs)) == (eu, er), (r, o, path)
                assert {k: st[k] for k in est} == est and st["path"] == _lib.UCENSUS_PATHS[path], (r, o, st)
            for (hosts, hn, hp, st), o in zip(out[r][1], ucr.HOST_ORDERS):
                eh, en, ep, est = ucr.host_census(parts[r], order=o, have=ph)
                assert (hosts, list(hn), list(hp)) == (eh, en, ep), (r, o, path)
                assert {k: st[k] for k in est} == est, (r, o, st)
            urls, refs, _ = out[r][0][0]
            assert not set(urls) & set(seen)
            seen.update(zip(urls, (int(x) for x in refs)))
            for hh, n, p in zip(*out[r][1][0][:3]):
                nurls[hh] = nurls.get(hh, 0) + int(n)
                posts[hh] = posts.get(hh, 0) + int(p)
        assert seen == dict(have["rehosted"])
        eh, en, ep, _ = ucr.host_census(lists, order="host", have=have["rehosted"])
        assert nurls == dict(zip(eh, en)) and posts == dict(zip(eh, ep))
