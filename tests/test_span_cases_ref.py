"""The large index of tests/span_cases.py, the part that runs without a GPU: the layout reaches the places
it claims (two tiles per workgroup, list boundaries on tile and span edges, hits on one side of a tile edge
only), the expectations computed from the arrays equal tests/host_ref.py, tests/census_ref.py,
tests/retention_ref.py and tests/refs_ref.py on the thinned corpus, and the constants the cases carry are
the library's."""

import numpy as np
import pytest

import census_ref as cr
import host_ref as hr
import refs_ref as rr
import retention_ref as tr
import span_cases as sc
import update_ref as ur
from yacy_search_server_amd import _lib


@pytest.fixture(scope="module")
def c():
    return sc.corpus()


@pytest.fixture(scope="module")
def small(c):
    t = sc.thin(c)
    assert t.n < c.n // 40 and t.marked.sum() == c.marked.sum() and t.marked2.sum() == c.marked2.sum()
    return t, t.lists()


def test_constants_are_the_librarys():
    """the LDS limits the set sizes of the cases sit around: tests/host_ref.py carries no such constant, so the
    binding's, which tests/test_host_ref.py ties to include/yrwi.h, are the ones compared"""
    assert _lib.HOST_LDS_MAX == sc.HOST_LDS_MAX and _lib.REF_LDS_MAX == sc.REF_LDS_MAX
    assert _lib.RETENTION_DAYS == sc.DAYS == tr.DAYS


def test_geometry(c):
    f = c.facts
    assert c.n == sc.TOTAL == 2097153 + 4096
    grid, per = sc.span_of(c.n)
    assert (grid, per) == (2048, 2048) and per == sc.PER
    assert sc.span_of(sc.SPAN_BLOCKS * sc.SPAN_TILE) == (2048, 1024)  # one posting fewer than 2^21 + 1: one tile
    nonempty = -(-c.n // per)
    assert nonempty == 1027 and c.n - 1026 * per == 1  # workgroups 0 .. 1025 walk two tiles, 1026 one posting
    second = np.arange(1026) * per + sc.SPAN_TILE  # the postings that start a second tile
    assert second[-1] < c.n
    assert (np.diff(c.off) == c.lens).all() and len(c.terms) == len(set(c.terms)) == len(c.lens)
    assert c.terms == sorted(c.terms, key=ur.url_key)
    # the list that covers whole spans; a boundary on a tile edge inside a span; boundaries on span edges
    assert c.lens[0] == 8192 and c.off[1] == 4 * per
    assert c.off[2] == 4 * per + sc.SPAN_TILE
    assert 6 * per in c.off and 4 * per in c.off
    # 300 one-row lists, 150 on each side of the tile edge inside span 5
    a, b = f["one_row"]
    assert b - a == 300 and (c.lens[a:b] == 1).all() and f["edge"] == 5 * per + sc.SPAN_TILE
    assert c.off[a] == f["edge"] - 150 and c.off[b] == f["edge"] + 150
    # lists of 1 .. 3 rows fill the first tile of span 6
    a, b = f["run"]
    assert c.off[a] == 6 * per and c.off[b] == 6 * per + sc.SPAN_TILE and set(c.lens[a:b]) == {1, 2, 3}
    assert ((c.lens[f["filler_first"]:] >= 3000) & (c.lens[f["filler_first"]:] <= 5000)).all()
    # every list ascends strictly in the 72-bit key; no url twice in the index
    same = c.lst[1:] == c.lst[:-1]
    assert (c.key[1:][same] > c.key[:-1][same]).all() and len(np.unique(c.key)) == c.n
    assert (np.diff(c.key) < 0).any()  # (the url order is not the flattened order)


def _tiles(c, mask, w):
    """hits of span w in its first and in its second tile, and the lists they are of"""
    a = w * sc.PER
    return (int(mask[a:a + sc.SPAN_TILE].sum()), int(mask[a + sc.SPAN_TILE:a + sc.PER].sum()),
            set(c.lst[a:a + sc.PER][mask[a:a + sc.PER]]))


@pytest.mark.parametrize("n", [64, 2049])
def test_host_hits_are_where_the_cases_say(c, n):
    f = c.facts
    keys = sc.host_set(n)
    assert len(set(keys)) == n and len(keys) == n + 1 and (n <= sc.HOST_LDS_MAX) == (n == 64)
    counts, lists_hit, hit = sc.expect_count_hosts(c, keys)
    assert (hit == (c.marked | (c.marked2 if n > 64 else False))).all() and min(counts) > 0
    assert _tiles(c, hit, f["w_second"])[:2] == (0, 5)      # hits only in the second tile
    assert _tiles(c, hit, f["w_first"])[:2] == (4, 0)       # only in the first
    t1, t2, of = _tiles(c, hit, f["w_both"])
    assert (t1, t2) == (3, 3) and len(of) == 1              # of one list in both tiles
    t1, t2, of = _tiles(c, hit, 0)
    assert t1 > 0 and t2 > 0 and of == {0}                  # and of the list over four spans
    a, b = f["one_row"]
    assert hit[c.off[a]:c.off[b]].all()                     # every one-row list holds one hit
    # the compaction after the removal walks second tiles too: the lists that lose some rows, not all
    part = np.bincount(c.lst[hit], minlength=len(c.lens))
    assert c.lens[(part > 0) & (part < c.lens)].sum() > sc.SPAN_BLOCKS * sc.SPAN_TILE


def test_url_hits_are_where_the_cases_say(c):
    f = c.facts
    for n in (2047, 2049):
        uhi, uhost = sc.url_set(c, n)
        assert len(uhi) == n + 3 and (n <= sc.REF_LDS_MAX) == (n == 2047)
        counts, st, by, hit = sc.expect_refs(c, uhi, uhost)
        assert st["urls"] == n and st["urls_found"] == st["refs"] == n - 8 and set(counts) == {0, 1}
        assert (hit & c.marked).sum() == c.marked.sum()
        assert _tiles(c, hit, f["w_first"])[:2] == (4, 0)   # a first tile with hits, a second without
        assert _tiles(c, hit, f["w_second"])[:2] == (0, 5)  # the reverse
        assert _tiles(c, hit, f["w_both"])[:2] == (3, 3)    # both: the pack pass uses its wave counts twice
        tt, rows = by["term"]
        ut, urows = by["url"]
        assert len(tt) == len(rows) == n - 8 and tt.tobytes() != ut.tobytes() and rows.tobytes() != urows.tobytes()


def test_retention_reaches_what_it_claims(c):
    f = c.facts
    lists, st, rs, hist, keep = sc.expect_retention(c, sc.MIN_DAY, sc.MAX_REFS)
    # a span's second tile lies outside the window around its first posting: it goes past LDS whole
    bypass = sc.expect_hist_bypass(c)
    assert bypass == 1026 * sc.SPAN_TILE == 1050624 and hist.sum() == c.n
    # the cap cuts the big list on a tied day, and some three-row lists
    surv = c.day[:8192][c.day[:8192] >= sc.MIN_DAY]
    cut = np.sort(surv)[-sc.MAX_REFS]
    assert (surv == cut).sum() > sc.MAX_REFS and keep[:8192].sum() == sc.MAX_REFS
    assert (c.day[:8192][keep[:8192]] == cut).all()
    a, b = f["run"]
    nsurv = np.bincount(c.lst[c.day >= sc.MIN_DAY], minlength=len(c.lens))[a:b]
    assert (nsurv == 3).any() and (nsurv == 0).any() and rs["removed_age"] > 0 and rs["removed_cap"] > 0
    assert rs["lists_cap"] > len(c.lens) - f["filler_first"] and rs["emptied_terms"] > 0  # every filler and more
    # the cut-day search walks second tiles: the lists over the cap
    assert c.lens[np.bincount(c.lst[c.day >= sc.MIN_DAY], minlength=len(c.lens)) > sc.MAX_REFS].sum() > 2 ** 21


def test_census_reaches_what_it_claims(c):
    hosts, counts, st = sc.expect_census(c, "count", 1)
    assert st["hosts"] == sc.BG_HOSTS + sc.N_H64 + sc.N_G and st["hosts_passing"] == st["hosts"]
    _, cut, st = sc.expect_census(c, "host", sc.CENSUS_CUT)
    assert st["hosts_passing"] == sc.BG_HOSTS + sc.N_H64
    # 128 hosts in every whole span: with 64 LDS slots a second tile's hosts find the table full
    g = np.arange(c.n)
    plain = ~(c.marked | c.marked2)
    w = 100
    assert len(np.unique(c.host[(g // sc.PER == w) & plain])) == 128
    assert len(np.unique(c.host[(g // sc.PER == w) & plain & (g % sc.PER < sc.SPAN_TILE)])) == 64
    floor = sc.census_bypass_floor(c, 64)
    assert 1000 * sc.SPAN_TILE - 16 * 4096 < floor < c.n and sc.census_bypass_floor(c, 4096) == 0


# ------------------------------------------------------------------ the expectations against the references
def _same(got, exp):
    assert list(got) == list(exp), (sorted(set(got) ^ set(exp))[:5], len(got), len(exp))
    for t in exp:
        assert got[t].tobytes() == exp[t].tobytes(), t


@pytest.mark.parametrize("n", [64, 2049])
def test_hosts_against_host_ref(small, n):
    t, lists = small
    keys = sc.host_set(n)
    hosts = sc.host_hashes(keys)
    counts, lists_hit, _ = sc.expect_count_hosts(t, keys)
    assert (counts, lists_hit) == hr.count_hosts(lists, hosts, t.terms)
    new, st = sc.expect_remove_hosts(t, keys)
    rnew, rst = hr.apply_remove_hosts(lists, hosts, t.terms)
    assert st == rst and st["removed"] == sum(counts[:-1])
    _same(new, rnew)


def test_census_against_census_ref(small):
    t, lists = small
    for order in cr.ORDERS:
        for minp in (1, 3):
            hosts, counts, st = sc.expect_census(t, order, minp)
            assert (hosts, counts, st) == cr.census(lists, t.terms, order, minp)


def test_retention_against_retention_ref(small):
    t, lists = small
    for min_day, max_refs in ((sc.MIN_DAY, sc.MAX_REFS), (sc.MIN_DAY, 0), (0, 1), (25003, 5)):
        new, st, rs, hist, _ = sc.expect_retention(t, min_day, max_refs)
        rnew, rst, rrs = tr.apply_retention(lists, min_day, max_refs, t.terms)
        assert st == rst and rs == rrs, (min_day, max_refs, st, rst, rs, rrs)
        _same(new, rnew)
        assert (hist == tr.day_hist(lists, t.terms)).all()


@pytest.mark.parametrize("n", [2047, 2049])
def test_refs_against_refs_ref(c, small, n):
    t, lists = small
    uhi, uhost = sc.url_set(c, n)
    counts, st, by, _ = sc.expect_refs(t, uhi, uhost)
    r = rr.references(lists, sc.url_hashes(uhi, uhost), t.terms)
    assert (counts == r.counts).all() and st == {k: r.stats[k] for k in st}
    for order in rr.ORDERS:
        assert by[order][0].tobytes() == r.by[order][0].tobytes(), order
        assert by[order][1].tobytes() == r.by[order][1].tobytes(), order
