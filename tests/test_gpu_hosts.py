"""Removal and counting by host on the device (yrwi_remove_hosts / yrwi_count_hosts) against
tests/host_ref.py on the re-hosted `tiny` corpus and on hand-made lists: after every removal
the lists equal the reference byte for byte, the url dictionary is consistent, the index
statistics and the call's statistics equal the reference's, and a 40-query batch (default and
authority profiles alternating, with excludes) equals the oracle on the reference's lists and a
fresh index built in full from them."""

import numpy as np
import pytest

import host_ref as hr
import index_util as iu
import update_ref as ur
from yacy_search_server_amd import _lib, synth
from yacy_search_server_amd._lib import YrwiError

pytestmark = pytest.mark.gpu

B64 = iu.B64
B = _lib.HOST_LDS_MAX
NOBODY = b"n0b0dy"
H0, H5, H40, H63 = (hr.host_name(i) for i in (0, 5, 40, 63))


def _term(i):
    return iu.term(i, b"-h")


@pytest.fixture(scope="module")
def tiny():
    cfg = synth.preset("tiny")
    idx = synth.build_index(cfg)
    lists = hr.rehost(idx.as_dict())
    # the facts about the re-hosted corpus the cases rely on
    assert sum(len(l) for l in lists.values()) == 60050 and len(lists) == 200
    holds = lambda h: sum(1 for l in lists.values() if (l[:, 6:12] == np.frombuffer(h, np.uint8)).all(axis=1).any())
    assert holds(H0) == 200 and 50 <= holds(H63) <= 150 and holds(NOBODY) == 0
    assert not any(t.startswith(b"-h") for t in lists)
    qs = [([idx.hashes[t] for t in inc], [idx.hashes[t] for t in exc]) for inc, exc in synth.queries(cfg, 40, 2, 3, 1)]
    return cfg, idx, lists, qs


@pytest.fixture(scope="module")
def every_list(tiny):
    """case 1's reference, shared with the chunk cases: hosts {0, 5, 40} and one nobody has, from every list"""
    cfg, idx, lists, qs = tiny
    hosts = [H0, H5, NOBODY, H40]
    new, exp = hr.apply_remove_hosts(lists, hosts)
    assert exp["removed"] == 15128 and exp["emptied_terms"] == 0 and exp["terms"] == 200
    return hosts, new, exp, hr.count_hosts(lists, hosts)


def _count(ix, lists, hosts, terms=None, ref=None):
    counts, hit = ix.count_hosts(hosts, terms)
    exp = ref or hr.count_hosts(lists, hosts, terms)
    assert (counts.dtype, list(counts), hit) == (np.int64, exp[0], exp[1])
    return list(counts)


def _remove(ix, lists, hosts, terms=None, ref=None):
    """remove on the device and on the reference; the stats must agree"""
    st = ix.remove_hosts(hosts, terms)
    new, exp = ref or hr.apply_remove_hosts(lists, hosts, terms)
    assert {k: st[k] for k in iu.STAT_KEYS} == exp, (st, exp)
    return new, st


# ------------------------------------------------------------------ 1 and 6: every list, at three chunk sizes
@pytest.mark.parametrize("chunk", [None, 256, 4096])
def test_every_list(tiny, every_list, monkeypatch, chunk):
    """chunk 256 / 4096: YRWI_RM_CHUNK forces many chunks (a list longer than the chunk is one of its
    own); lists and stats are those of the default"""
    cfg, idx, lists, qs = tiny
    hosts, new, exp, cexp = every_list
    iu.set_rm_chunk(monkeypatch, chunk)
    if chunk is not None:
        assert max(len(l) for l in lists.values()) > 256
    ix = iu.open_index(lists)
    try:
        ix.build_url_ids()
        counts = _count(ix, lists, hosts, ref=cexp)
        cur, st = _remove(ix, lists, hosts, ref=(new, exp))
        assert sum(dict(zip(hosts, counts)).values()) == st["removed"] == 15128  # over the unique hosts
        iu.verify_step(ix, cur, list(lists), qs, monkeypatch)
        _, st = _remove(ix, cur, hosts)  # nothing left to remove: nothing changes
        assert st["removed"] == 0 and st["terms"] == 0
    finally:
        ix.close()


def test_more_chunks_more_launches(tiny, every_list, monkeypatch):
    cfg, idx, lists, qs = tiny
    hosts, new, exp, _ = every_list
    st = {}
    for chunk in (None, 256):
        iu.set_rm_chunk(monkeypatch, chunk)
        ix = iu.open_index(lists)
        try:
            _, st[chunk] = _remove(ix, lists, hosts, ref=(new, exp))
        finally:
            ix.close()
    assert st[256]["launches"] > st[None]["launches"], st
    assert st[256]["syncs"] == st[None]["syncs"], st  # no host wait per chunk


# ------------------------------------------------------------------ 2: named lists
def test_named_lists(tiny, monkeypatch):
    cfg, idx, lists, qs = tiny
    has = lambda t: (lists[t][:, 6:12] == np.frombuffer(H63, np.uint8)).all(axis=1).any()
    order = sorted(lists)
    named = order[::7][:28]
    terms = named + [named[3], _term(77)]  # 30 terms named: one of them twice, one nobody has
    assert len(set(terms)) == 29 and len(terms) == 30
    with_host = [t for t in named if has(t)]
    assert 0 < len(with_host) < len(named) and any(has(t) for t in order if t not in named)
    ix = iu.open_index(lists)
    try:
        ix.build_url_ids()
        _count(ix, lists, [H63, H63], terms)
        cur, st = _remove(ix, lists, [H63, H63], terms)
        assert st["terms"] == len(with_host) and st["removed"] > 0
        for t in order:  # lists not named, and named lists without the host, keep their bytes
            if t not in with_host:
                assert cur[t] is lists[t]
        iu.verify_step(ix, cur, order, qs, monkeypatch)
    finally:
        ix.close()


# ------------------------------------------------------------------ 3: boundaries
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
    """lists of 1 .. 1025 rows under six membership patterns, all in one call over every list: the
    removed runs cross wave (64), block (256) and list edges of the flattened index"""
    cfg, idx, lists, qs = tiny
    gone, stay = b"g0ne__", b"st4y__"
    hand, k = {}, 0
    for n in SIZES:
        for name, member in PATTERNS.items():
            urls = [iu.enc(1000 * k + i, 6) + (gone if member(i, n) else stay) for i in range(n)]
            assert urls == sorted(urls, key=ur.url_key)
            hand[_term(k)] = iu.rows(idx, urls, start=k)
            k += 1
    terms = list(hand)
    all_lists = {**lists, **hand}
    is_gone = lambda l: (l[:, 6:12] == np.frombuffer(gone, np.uint8)).all(axis=1)
    emptied = sum(1 for l in hand.values() if is_gone(l).all())
    losing = sum(1 for l in hand.values() if is_gone(l).any())
    assert emptied == len(SIZES) + 2  # every_row at each size; the 1-row lists of two more patterns
    assert losing == len(hand) - len(SIZES) - 2  # all but no_row at each size and two more 1-row lists
    qs = qs[:34] + [([terms[6], terms[12]], []), ([terms[18]], [terms[24]]), ([terms[30], terms[36]], []),
                    ([terms[42], terms[43]], [terms[44]]), ([terms[45]], []), ([terms[7], terms[8]], [])]
    ix = iu.open_index(all_lists)
    try:
        ix.build_url_ids()
        _count(ix, all_lists, [gone, stay, NOBODY])
        cur, st = _remove(ix, all_lists, [gone, NOBODY])
        assert st["emptied_terms"] == emptied and st["terms"] == losing
        iu.verify_step(ix, cur, terms + list(lists)[:10], qs, monkeypatch)
    finally:
        ix.close()


# ------------------------------------------------------------------ 4: the host set across the LDS bound
FIRST, LAST, OTHER = b"AAAAAA", b"______", b"keepme"
REAL = [FIRST, H0, H5, H40, H63, LAST]


def _host_set(n):
    """n hosts: REAL among hosts nobody has ('B....' below and 'y....' above the corpus's), so that the
    hosts with postings sit at the first, the middle and the last positions of the sorted set"""
    fill = [bytes([B64[1 + i % 2 * 49]]) + iu.enc(i, 5) for i in range(n - len(REAL))]
    hs = fill[: len(fill) // 2] + REAL + fill[len(fill) // 2:]
    key = sorted(hs, key=ur.url_key)
    assert len(set(hs)) == n and key[0] == FIRST and key[-1] == LAST and abs(key.index(H0) - n // 2) <= 3
    return hs


@pytest.fixture(scope="module")
def across(tiny):
    """the corpus plus one list of hosts that sort first and last; the reference for REAL, which is the
    reference of every set of _host_set: the hosts it adds have no posting (checked)"""
    cfg, idx, lists, qs = tiny
    extra = _term(500)
    urls = [iu.enc(i, 6) + (FIRST, LAST, OTHER)[i % 3] for i in range(300)]
    lists = {**lists, extra: iu.rows(idx, urls)}
    have = {bytes(r[6:12]) for l in lists.values() for r in l}
    assert not have & (set(_host_set(4 * B)) - set(REAL)) and set(REAL) <= have
    qs = qs[:38] + [([extra], []), ([extra, list(lists)[0]], [])]
    counts, hit = hr.count_hosts(lists, REAL)
    return lists, qs, hr.apply_remove_hosts(lists, REAL), dict(zip(REAL, counts)), hit


@pytest.mark.parametrize("n", [1, B, B + 1, 4 * B])
def test_set_sizes_across_the_lds_bound(across, monkeypatch, n):
    """sets of 1, B, B + 1 and 4 B hosts: a set of B or fewer is searched in LDS, a larger one in global
    memory; B, B + 1 and 4 B give one reference's lists, counts and stats, so the same as each other"""
    lists, qs, ref, cref, hit = across
    hosts = [H0] if n == 1 else _host_set(n)
    ix = iu.open_index(lists)
    try:
        ix.build_url_ids()
        if n == 1:
            counts = _count(ix, lists, hosts)
            cur, st = _remove(ix, lists, hosts)
        else:
            counts = _count(ix, lists, hosts, ref=([cref.get(h, 0) for h in hosts], hit))
            cur, st = _remove(ix, lists, hosts, ref=ref)
        assert st["removed"] == sum(counts) > 0
        iu.verify_step(ix, cur, list(lists), qs, monkeypatch)
    finally:
        ix.close()


# ------------------------------------------------------------------ 5: hot spot
def test_hot_spot(tiny, monkeypatch):
    """one host owns a list of 20,000 rows: its count is exact, and the removal leaves the other hosts' rows"""
    cfg, idx, lists, qs = tiny
    hot = b"h0t___"
    big = _term(900)
    three = [t for t in sorted(lists) if len(lists[t]) >= 300][:3]
    small = {t: lists[t][:300] for t in three}
    small[big] = iu.rows(idx, [iu.enc(i, 6) + hot for i in range(20000)])
    qs = [([big], []), ([three[0]], [big]), ([three[0], three[1]], []), ([three[2]], [three[0]]), ([three[1]], []),
          ([three[2], three[1]], [])]
    ix = iu.open_index(small)
    try:
        ix.build_url_ids()
        counts = _count(ix, small, [hot, H0, NOBODY])
        assert counts[0] == 20000 and counts[1] > 0
        cur, st = _remove(ix, small, [hot, H0])
        assert st["removed"] == counts[0] + counts[1] and st["emptied_terms"] == 1 and big not in cur
        for t in three:
            assert cur[t].tobytes() == small[t][(small[t][:, 6:12] != np.frombuffer(H0, np.uint8)).any(axis=1)].tobytes()
        iu.verify_step(ix, cur, list(small), qs, monkeypatch)
    finally:
        ix.close()


# ------------------------------------------------------------------ 7: launches, syncs, allocations
def test_launches_and_syncs_are_a_function_of_the_chunks(tiny, monkeypatch):
    cfg, idx, lists, qs = tiny
    monkeypatch.delenv("YRWI_RM_CHUNK", raising=False)
    fill = [b"B" + iu.enc(i, 5) for i in range(4 * B - 1)]
    one = sorted(lists)[0]
    st = []
    for hosts, terms in (([H0], [one]), ([H0], None), ([H0] + fill, None)):
        ix = iu.open_index(lists)
        try:
            st.append(_remove(ix, lists, hosts, terms)[1])
        finally:
            ix.close()
    assert st[0]["terms"] == 1 and st[1]["terms"] == st[2]["terms"] == 200
    assert len({(s["launches"], s["syncs"]) for s in st}) == 1, st
    # a steady sequence of calls makes no device-wide allocation after the first
    ix = iu.open_index(lists)
    try:
        ix.count_hosts([H0, H5], None)
        ix.remove_hosts([H63], None)
        r0 = _lib.lib().yrwi_realloc_events()
        for h in (H5, H40):
            ix.count_hosts([H0, h], None)
            assert ix.remove_hosts([h], None)["removed"] > 0
        assert _lib.lib().yrwi_realloc_events() - r0 == 0
    finally:
        ix.close()


# ------------------------------------------------------------------ 8: count_hosts changes nothing
def test_count_changes_nothing(tiny):
    cfg, idx, lists, qs = tiny
    ix = iu.open_index(lists)
    try:
        ix.build_url_ids()
        info, stats = ix.index_info(), ix.stats()
        _count(ix, lists, [H0, H5, NOBODY, H0])
        _count(ix, lists, [H40], sorted(lists)[:20])
        assert ix.count_hosts([H0], [])[1] == 0 and list(ix.count_hosts([], None)[0]) == []
        assert ix.index_info() == info and ix.stats() == stats
        iu.same_lists(ix, lists, list(lists))
        assert ix.index_info() == info
    finally:
        ix.close()


# ------------------------------------------------------------------ 9: errors are atomic
def test_errors_are_atomic(tiny):
    cfg, idx, lists, qs = tiny
    ix = iu.open_index(lists)
    try:
        ix.build_url_ids()
        before = ix.stats()
        some = sorted(lists)[:3]
        for call in (ix.remove_hosts, ix.count_hosts):
            with pytest.raises(YrwiError) as e:
                call([H0, b"h0s!AA"], None)
            assert e.value.rc == -2
            with pytest.raises(YrwiError) as e:
                call([H0], [some[0], b"bad#term_ash"])
            assert e.value.rc == -2
        assert ix.stats() == before
        iu.same_lists(ix, lists, some)
        st = ix.remove_hosts([], None)
        assert all(v == 0 for v in st.values()) and set(iu.STAT_KEYS) <= set(st)
        assert all(v == 0 for v in ix.remove_hosts([H0], []).values())
        assert ix.stats() == before
        assert ix.check_url_ids()[0] == 0
    finally:
        ix.close()


# ------------------------------------------------------------------ 10: two shards in one process
def test_two_shards(tiny, every_list):
    """world 2 over the loopback transport: each shard holds its url-hash range of the lists and gets
    the same call; the shards' lists together are the reference's, their counts and `removed` add up"""
    cfg, idx, lists, qs = tiny
    hosts, whole, exp, (cexp, _) = every_list
    world = 2
    parts = iu.split_by_rank(lists, world)

    def fn(r, ix):
        counts, _ = ix.count_hosts(hosts, None)
        st = ix.remove_hosts(hosts, None)
        assert ix.check_url_ids()[0] == 0
        return list(counts), st, {t: ix.get_list(t) for t in lists}

    out = iu.run_parts(parts, world, fn)
    assert [a + b for a, b in zip(out[0][0], out[1][0])] == cexp
    assert out[0][1]["removed"] + out[1][1]["removed"] == exp["removed"]
    assert out[0][1]["removed"] > 0 and out[1][1]["removed"] > 0
    for t in lists:
        got = np.concatenate([out[0][2][t], out[1][2][t]])
        assert got.tobytes() == whole.get(t, iu.EMPTY).tobytes(), t
