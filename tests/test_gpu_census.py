"""The host census on the device (yrwi_host_census) against tests/census_ref.py: on the re-hosted
`tiny` corpus (64 hosts, skewed), on `tiny` as generated (36,406 hosts of at most 16 postings: ties
everywhere, more hosts than any LDS table and than a small device table) and on hand-made lists.
Hosts, counts and the counters of the call's statistics are compared exactly, in both orders; the
overflow paths of both tables are reached with YRWI_CENSUS_LDS_SLOTS and YRWI_CENSUS_SLOTS."""

import ctypes

import numpy as np
import pytest

import census_ref as cr
import host_ref as hr
import index_util as iu
import update_ref as ur
from yacy_search_server_amd import _lib, synth
from yacy_search_server_amd._lib import YrwiError

pytestmark = pytest.mark.gpu

FIRST, LAST, OTHER = b"AAAAAA", b"______", b"keepme"
KNOBS = ("YRWI_CENSUS_SLOTS", "YRWI_CENSUS_LDS_SLOTS")


def _term(i):
    return iu.term(i, b"-h")


@pytest.fixture(scope="module")
def tiny():
    """(synthetic index, {"rehosted": lists, "raw": lists}, {corpus: postings per host}); the facts about
    both corpora the cases rely on (tests/test_census_ref.py checks them without a GPU)"""
    idx = synth.build_index(synth.preset("tiny"))
    raw = idx.as_dict()
    corp = {"rehosted": hr.rehost(raw), "raw": raw}
    have = {name: cr.tally(lists) for name, lists in corp.items()}
    for name, lists in corp.items():
        assert sum(len(l) for l in lists.values()) == 60050 and len(lists) == 200
        assert not any(t.startswith(b"-h") for t in lists)
    assert sorted(have["rehosted"]) == sorted(hr.host_name(i) for i in range(64))
    counts = sorted(have["rehosted"].values(), reverse=True)
    assert counts[0] == 12719 and counts[-1] == 183
    assert sum(1 for c in set(counts) if counts.count(c) == 2) == 4 and len(set(counts)) == 60
    assert len(have["raw"]) == 36406 and max(have["raw"].values()) == 16
    assert not {FIRST, LAST, OTHER} & (set(have["raw"]) | set(have["rehosted"]))
    return idx, corp, have


@pytest.fixture(scope="module")
def refs(tiny):
    """the reference of every list of either corpus in either order, computed once"""
    idx, corp, have = tiny
    return {(name, order): cr.ordered(have[name], order) for name in corp for order in cr.ORDERS}


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def opened(tiny):
    """one context per corpus for the cases that change nothing"""
    idx, corp, have = tiny
    ixs = {name: iu.open_index(lists) for name, lists in corp.items()}
    yield ixs
    for ix in ixs.values():
        ix.close()


def _census(ix, exp, terms=None, order="count", min_postings=1, top=None, st_exp=None):
    """the census on the device; hosts and counts must equal exp = (hosts, counts), the counters st_exp"""
    hosts, counts, st = ix.host_census(terms, order, min_postings, top)
    assert counts.dtype == np.int64 and len(hosts) == len(counts)
    assert hosts == list(exp[0]) and list(counts) == list(exp[1]), (order, st)
    for k, v in (st_exp or {}).items():
        assert st[k] == v, (k, st)
    return st


def _whole(n_hosts, passing=None):
    return dict(lists=200, postings=60050, hosts=n_hosts, hosts_passing=n_hosts if passing is None else passing)


def _raw_call(ix, terms, order, min_postings, cap, hosts, counts):
    """yrwi_host_census as it is: -> (rc, nout, stats); hosts / counts: numpy arrays or None"""
    tb = np.frombuffer(b"".join(terms or ()), dtype=np.uint8)
    n = ctypes.c_int64(-7)
    st = _lib.CCensusStats()
    rc = _lib.lib().yrwi_host_census(ix._h, tb.ctypes.data if len(tb) else None, len(tb) // 12, order, min_postings,
                                     None if hosts is None else hosts.ctypes.data,
                                     None if counts is None else counts.ctypes.data, cap, ctypes.byref(n),
                                     ctypes.byref(st))
    return rc, n.value, st


HOSTS_OF = {"rehosted": 64, "raw": 36406}


# ------------------------------------------------------------------ 1: both corpora, every list, both orders
@pytest.mark.parametrize("name", ["rehosted", "raw"])
@pytest.mark.parametrize("order", cr.ORDERS)
def test_every_list(tiny, refs, opened, name, order):
    """at the defaults nothing bypasses the LDS table (a workgroup sees at most 1024 postings, its table has
    2048 slots) and the device table (131,072 slots for 60,050 postings) is not enlarged"""
    st = _census(opened[name], refs[name, order], order=order, st_exp=_whole(HOSTS_OF[name]))
    assert sum(refs[name, order][1]) == st["postings"] == 60050
    assert (st["passes"], st["lds_bypass"], st["table_slots"]) == (1, 0, 131072), st
    assert st["t_count_ns"] > 0 and st["t_total_ns"] >= st["t_count_ns"]


# ------------------------------------------------------------------ 2: the LDS table too small
@pytest.mark.parametrize("order", cr.ORDERS)
def test_lds_table_too_small(tiny, refs, opened, monkeypatch, order):
    monkeypatch.setenv("YRWI_CENSUS_LDS_SLOTS", "64")
    st = _census(opened["raw"], refs["raw", order], order=order, st_exp=_whole(36406))
    assert st["lds_bypass"] > 0 and st["passes"] == 1, st
    assert st["lds_bypass"] <= 60050
    _census(opened["rehosted"], refs["rehosted", order], order=order, st_exp=_whole(64))


# ------------------------------------------------------------------ 3: the device table too small
def test_device_table_too_small(tiny, refs, opened, monkeypatch):
    idx, corp, have = tiny
    base = {name: _census(opened[name], refs[name, "count"], st_exp=_whole(HOSTS_OF[name])) for name in corp}
    monkeypatch.setenv("YRWI_CENSUS_SLOTS", "1024")
    for order in cr.ORDERS:
        st = _census(opened["raw"], refs["raw", order], order=order, st_exp=_whole(36406))
        assert st["passes"] >= 2 and st["table_slots"] >= st["hosts"], st
        assert st["table_slots"] == 1024 * 4 ** (st["passes"] - 1), st
    assert st["launches"] > base["raw"]["launches"] and st["syncs"] > base["raw"]["syncs"], (st, base["raw"])
    # 64 hosts into 64 slots: exactly full or enlarged, and either is right
    monkeypatch.setenv("YRWI_CENSUS_SLOTS", "64")
    for order in cr.ORDERS:
        st = _census(opened["rehosted"], refs["rehosted", order], order=order, st_exp=_whole(64))
        assert st["table_slots"] == 64 * 4 ** (st["passes"] - 1), st
    # both tables too small at once
    monkeypatch.setenv("YRWI_CENSUS_LDS_SLOTS", "64")
    st = _census(opened["raw"], refs["raw", "count"], st_exp=_whole(36406))
    assert st["passes"] >= 2 and st["lds_bypass"] > 0, st


def test_launches_and_syncs_are_a_function_of_the_passes(tiny, refs, opened):
    """one named list against every list, at the defaults: equal passes, equal launches and syncs"""
    idx, corp, have = tiny
    one = sorted(corp["rehosted"])[0]
    a = opened["rehosted"].host_census([one], "count")[2]
    b = opened["rehosted"].host_census(None, "count")[2]
    c = opened["raw"].host_census(None, "count")[2]
    assert a["lists"] == 1 and b["lists"] == c["lists"] == 200
    assert a["passes"] == b["passes"] == c["passes"] == 1
    assert len({(s["launches"], s["syncs"]) for s in (a, b, c)}) == 1, (a, b, c)
    assert a["launches"] > 0 and a["syncs"] > 0


# ------------------------------------------------------------------ 4: named lists
@pytest.mark.parametrize("name", ["rehosted", "raw"])
def test_named_lists(tiny, opened, name):
    idx, corp, have = tiny
    lists = corp[name]
    order = sorted(lists)
    named = order[::7][:28]
    terms = named + [named[3], _term(77)]  # 30 terms named: one of them twice, one nobody has
    assert len(set(terms)) == 29 and len(terms) == 30
    for o in cr.ORDERS:
        eh, ec, est = cr.census(lists, terms, o)
        assert est["lists"] == 28 and est["postings"] == sum(len(lists[t]) for t in named) < 60050
        _census(opened[name], (eh, ec), terms, o, st_exp=est)
    # lists that were not named contribute nothing: one list's census is that list's hosts
    t = named[5]
    eh, ec, est = cr.census({t: lists[t]}, None, "host")
    assert sum(ec) == len(lists[t])
    _census(opened[name], (eh, ec), [t], "host", st_exp=est)
    hosts, counts, st = opened[name].host_census([], "count")
    assert hosts == [] and len(counts) == 0 and st["postings"] == 0
    hosts, counts, st = opened[name].host_census([_term(77)], "count")
    assert hosts == [] and len(counts) == 0 and (st["lists"], st["postings"], st["hosts"], st["passes"]) == (0, 0, 0, 0)


# ------------------------------------------------------------------ 5: boundaries
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)
PATTERNS = {
    "alternating": lambda i, n: i % 2 == 0,
    "all_but_first": lambda i, n: i > 0,
    "all_but_last": lambda i, n: i < n - 1,
    "first_and_last": lambda i, n: i in (0, n - 1),
    "every_row": lambda i, n: True,
    "no_row": lambda i, n: False,
}


def test_boundaries(tiny, monkeypatch):
    """lists of 1 .. 1025 rows in which two hosts alternate or sit at the edges, next to the re-hosted corpus:
    the runs of a host cross wave (64), block (256), tile (1024) and list edges of the flattened index; one more
    list holds the host of key 0 (not an empty slot) and the host of key 2^36 - 1"""
    idx, corp, have = tiny
    gone, stay = b"g0ne__", b"st4y__"
    hand, k = {}, 0
    for n in SIZES:
        for name, member in PATTERNS.items():
            urls = [iu.enc(1000 * k + i, 6) + (gone if member(i, n) else stay) for i in range(n)]
            assert urls == sorted(urls, key=ur.url_key)
            hand[_term(k)] = iu.rows(idx, urls, start=k)
            k += 1
    edge = _term(500)
    hand[edge] = iu.rows(idx, [iu.enc(i, 6) + (FIRST, LAST, OTHER)[i % 3] for i in range(300)])
    all_lists = {**corp["rehosted"], **hand}
    exp = have["rehosted"] + cr.tally(hand)
    assert exp[FIRST] == exp[LAST] == exp[OTHER] == 100 and exp[gone] > exp[stay] > 0 and len(exp) == 69
    ix = iu.open_index(all_lists)
    try:
        for lds in (None, "64"):
            if lds:
                monkeypatch.setenv("YRWI_CENSUS_LDS_SLOTS", lds)
            for order in cr.ORDERS:
                st = _census(ix, cr.ordered(exp, order), order=order)
                assert (st["lists"], st["postings"], st["hosts"]) == (len(all_lists), sum(exp.values()), 69)
        monkeypatch.delenv("YRWI_CENSUS_LDS_SLOTS")
        # the hand-made lists alone, each one alone at the edge sizes, and the edge list
        for order in cr.ORDERS:
            eh, ec, est = cr.census(hand, None, order)
            _census(ix, (eh, ec), list(hand), order, st_exp=est)
        for t in list(hand)[:12] + list(hand)[-7:]:
            eh, ec, est = cr.census({t: hand[t]}, None, "count")
            _census(ix, (eh, ec), [t], "count", st_exp=est)
        hosts, counts, _ = ix.host_census([edge], "host")
        assert hosts == [FIRST, OTHER, LAST] and list(counts) == [100, 100, 100]
    finally:
        ix.close()


# ------------------------------------------------------------------ 6: hot spot
def test_hot_spot(tiny, monkeypatch):
    """one host owns a list of 20,000 rows, next to three 300-row lists"""
    idx, corp, have = tiny
    lists = corp["rehosted"]
    hot = b"h0t___"
    big = _term(900)
    three = [t for t in sorted(lists) if len(lists[t]) >= 300][:3]
    small = {t: lists[t][:300] for t in three}
    small[big] = iu.rows(idx, [iu.enc(i, 6) + hot for i in range(20000)])
    exp = cr.tally(small)
    assert exp[hot] == 20000 and sum(exp.values()) == 20900
    ix = iu.open_index(small)
    try:
        for lds in (None, "64"):
            if lds:
                monkeypatch.setenv("YRWI_CENSUS_LDS_SLOTS", lds)
            for order in cr.ORDERS:
                _census(ix, cr.ordered(exp, order), order=order,
                        st_exp=dict(lists=4, postings=20900, hosts=len(exp), hosts_passing=len(exp)))
            hosts, counts, _ = ix.host_census(None, "count")
            assert hosts[0] == hot and counts[0] == 20000
    finally:
        ix.close()


# ------------------------------------------------------------------ 7: top and min_postings
def test_top_and_min_postings(tiny, refs, opened):
    idx, corp, have = tiny
    ix = opened["raw"]
    full_h, full_c = refs["raw", "count"]
    for cap in (10, 100, 36406, 40000):  # a prefix of the full order: the tie-break by host holds inside it
        st = _census(ix, (full_h[:cap], full_c[:cap]), order="count", top=cap, st_exp=_whole(36406))
    by_host = refs["raw", "host"]
    _census(ix, (by_host[0][:100], by_host[1][:100]), order="host", top=100, st_exp=_whole(36406))
    for order in cr.ORDERS:
        eh, ec = cr.ordered(have["raw"], order, 16)
        assert len(eh) >= 1 and set(ec) == {16}
        _census(ix, (eh, ec), order=order, min_postings=16, st_exp=_whole(36406, len(eh)))
        eh, ec = cr.ordered(have["raw"], order, 10)
        assert len(eh) > len(set(ec)) > 1  # ties among them
        _census(ix, (eh, ec), order=order, min_postings=10, st_exp=_whole(36406, len(eh)))
        eh, ec = cr.ordered(have["raw"], order, 3)
        _census(ix, (eh, ec), order=order, min_postings=3, st_exp=_whole(36406, len(eh)))
        _census(ix, (eh[:7], ec[:7]), order=order, min_postings=3, top=7, st_exp=_whole(36406, len(eh)))
    st = _census(ix, ([], []), min_postings=17, st_exp=_whole(36406, 0))  # above every count
    rc, n, cst = _raw_call(ix, None, _lib.CENSUS_BY_COUNT, 17, 5, np.zeros((5, 6), np.uint8), np.zeros(5, np.int64))
    assert (rc, n, cst.hosts_passing, cst.hosts) == (0, 0, 0, 36406)
    # min_postings below 1 is 1; cap 0 with NULL buffers fills the statistics alone
    for mp in (0, -5):
        rc, n, cst = _raw_call(ix, None, _lib.CENSUS_BY_COUNT, mp, 0, None, None)
        assert (rc, n) == (0, 0)
        assert (cst.lists, cst.postings, cst.hosts, cst.hosts_passing, cst.passes) == (200, 60050, 36406, 36406, 1)
    L = _lib.lib()  # st and nout may be NULL
    hosts, counts = np.zeros((3, 6), np.uint8), np.zeros(3, np.int64)
    assert L.yrwi_host_census(ix._h, None, 0, _lib.CENSUS_BY_COUNT, 1, hosts.ctypes.data, counts.ctypes.data, 3, None,
                              None) == 0
    assert [bytes(h) for h in hosts] == full_h[:3] and list(counts) == full_c[:3]


# ------------------------------------------------------------------ 8: agreement with its neighbours
def test_agrees_with_count_hosts_and_remove_hosts(tiny, refs):
    idx, corp, have = tiny
    for name, top in (("rehosted", None), ("raw", 3000)):  # (3000 hosts: count_hosts searches them in global memory)
        ix = iu.open_index(corp[name])
        try:
            hosts, counts, st = ix.host_census(None, "count", top=top)
            assert len(hosts) == (top or 64)
            got, _ = ix.count_hosts(hosts, None)
            assert list(got) == list(counts)
            named = sorted(corp[name])[:40]
            hosts, counts, _ = ix.host_census(named, "host")
            assert list(ix.count_hosts(hosts, named)[0]) == list(counts)
            # without the largest host: its postings are gone, every other count is unchanged
            full_h, full_c = refs[name, "count"]
            rm = ix.remove_hosts([full_h[0]], None)
            assert rm["removed"] == full_c[0]
            _census(ix, (full_h[1:], full_c[1:]), order="count",
                    st_exp=dict(postings=60050 - full_c[0], hosts=len(full_h) - 1, hosts_passing=len(full_h) - 1))
        finally:
            ix.close()


# ------------------------------------------------------------------ 9: changes nothing, allocates once
def test_changes_nothing_and_allocates_once(tiny, refs):
    idx, corp, have = tiny
    lists = corp["rehosted"]
    ix = iu.open_index(lists)
    try:
        ix.build_url_ids()
        info, stats = ix.index_info(), ix.stats()
        _census(ix, refs["rehosted", "count"])
        r0 = _lib.lib().yrwi_realloc_events()
        for order in ("host", "count", "host"):
            _census(ix, refs["rehosted", order], order=order)
        assert _lib.lib().yrwi_realloc_events() - r0 == 0
        _census(ix, cr.census(lists, sorted(lists)[:20], "host")[:2], sorted(lists)[:20], "host")
        assert ix.index_info() == info and ix.stats() == stats
        for t, l in lists.items():
            assert ix.get_size(t) == len(l), t
            assert ix.get_list(t).tobytes() == l.tobytes(), t
        assert ix.index_info() == info and ix.check_url_ids()[0] == 0
    finally:
        ix.close()


# ------------------------------------------------------------------ 10: errors write nothing
def test_errors_write_nothing(tiny, refs, opened):
    idx, corp, have = tiny
    ix = opened["rehosted"]
    some = sorted(corp["rehosted"])[:3]
    cases = [([some[0], b"bad#term_ash"], _lib.CENSUS_BY_COUNT, 8, -2),  # a character outside the alphabet
             (None, 2, 8, -1), (None, -1, 8, -1),                        # no such order
             (None, _lib.CENSUS_BY_HOST, -1, -1)]                        # a negative capacity
    for terms, order, cap, want in cases:
        hosts, counts = np.full((8, 6), 0xA5, np.uint8), np.full(8, -0x5A5A, np.int64)
        rc, n, st = _raw_call(ix, terms, order, 1, cap, hosts, counts)
        assert rc == want, (terms, order, cap, rc)
        assert (hosts == 0xA5).all() and (counts == -0x5A5A).all() and n == -7
        assert _lib.lib().yrwi_last_error(ix._h)
        _census(ix, refs["rehosted", "host"], order="host", st_exp=_whole(64))  # a following good call is right
    for hosts, counts in ((None, np.zeros(8, np.int64)), (np.zeros((8, 6), np.uint8), None), (None, None)):
        keep = None if counts is None else counts.copy()
        assert _raw_call(ix, None, _lib.CENSUS_BY_COUNT, 1, 8, hosts, counts)[0] == -1  # a capacity without a buffer
        assert keep is None or (counts == keep).all()
    with pytest.raises(YrwiError) as e:
        ix.host_census([b"bad#term_ash"], "count")
    assert e.value.rc == -2
    with pytest.raises(KeyError):
        ix.host_census(None, "size")
    _census(ix, refs["rehosted", "count"], st_exp=_whole(64))


# ------------------------------------------------------------------ 11: two shards in one process
def test_two_shards(tiny, refs):
    """world 2 over the loopback transport: each shard holds its url-hash range of the lists and is asked
    the same thing; its census is the reference on its range, and the two merged by host are the whole corpus's"""
    idx, corp, have = tiny
    lists = corp["rehosted"]
    world = 2
    parts = iu.split_by_rank(lists, world)

    def fn(r, ix):
        return [ix.host_census(None, o) for o in cr.ORDERS]

    out = iu.run_parts(parts, world, fn)
    merged = {}
    for r in range(world):
        assert sum(len(l) for l in parts[r].values()) > 0
        for (hosts, counts, st), o in zip(out[r], cr.ORDERS):
            eh, ec, est = cr.census(parts[r], None, o)
            assert (hosts, list(counts)) == (eh, ec), (r, o)
            assert {k: st[k] for k in est} == est, (r, o, st)
        for h, c in zip(out[r][0][0], out[r][0][1]):
            merged[h] = merged.get(h, 0) + int(c)
    assert merged == dict(have["rehosted"])
