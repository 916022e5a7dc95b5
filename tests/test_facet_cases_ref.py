"""Host facets (yrwi_host_facets_batch), reference only: every case of facet_cases.py states its
facets by construction, from the host and url arrays its lists are made from; here the numpy
group-by of facets_ref over the oracle's rows gives the same facets for every query of every
case, and the cases have the shapes they claim."""

import numpy as np

import facet_cases as F
import facets_ref as R

LR_TILE = F.LR_TILE


def test_stated_facets_equal_the_reference():
    seen = set()
    for c in F.cases():
        for i, q in enumerate(c.queries):
            if c.facets[i] is None or q in seen:
                continue
            seen.add(q)
            assert list(F.facets_of(q)) == list(c.facets[i]), (c.name, i)
            rows = F.rows_of(q)
            assert sum(n for _, n, _ in c.facets[i]) == len(rows), (c.name, i)
    assert len(seen) >= 14 + 2 + 4 + 4 + 8  # lengths, distinct, alternating, ties and extremes, exclusions


def test_group_and_order():
    rows = F.rows_of(F.case("ties").queries[1])
    g = R.group(rows)
    assert [h for h, _, _ in g] == sorted(h for h, _ in F.TIES)  # (these hosts: byte order is key order)
    assert {h: n for h, n, _ in g} == dict(F.TIES)
    for h, n, u in g:
        mine = [bytes(r[:12]) for r in rows if bytes(r[6:12]) == h]
        assert len(mine) == n and u == mine[0] == min(mine)
    by_count = [h for h, _, _ in R.ordered(g, "count", 0)]
    assert by_count == [b"tieBBB", b"tieDDD", b"tieAAA", b"tieCCC", b"tieFFF", b"tieEEE"]
    assert [h for h, _, _ in R.ordered(g, "count", 1)] == [b"tieBBB"]      # the cut splits the fives
    assert [h for h, _, _ in R.ordered(g, "count", 3)] == by_count[:3]     # ... and the threes
    assert [h for h, _, _ in R.ordered(g, "host", 2)] == [b"tieAAA", b"tieBBB"]
    assert R.group(np.zeros((0, 40), dtype=np.uint8)) == []
    assert R.host_key(F.H_ZERO) == 0 and R.host_key(F.H_TOP) == (1 << 36) - 1
    assert R.host_key(b"AAAAAB") == 1 and R.host_key(b"BAAAAA") == 1 << 30


def test_lengths_and_runs():
    c = F.case("lengths")
    assert set(F.LENGTHS) >= {1, LR_TILE - 1, LR_TILE, LR_TILE + 1, 2 * LR_TILE, 2 * LR_TILE + 1, 4 * LR_TILE + 1}
    assert [len(F.rows_of(q)) for q in c.queries] == [n for n in F.LENGTHS for _ in range(2)]
    assert all(len(f) == 1 for f in c.facets)
    d = F.case("distinct")
    assert all(len(f) == F.NDIST == len(F.rows_of(q)) for q, f in zip(d.queries, d.facets))
    assert set(d.max_hosts) == {1, 255, 256, 257, 768, 769, 0}
    url_order = [bytes(r[6:12]) for r in F.rows_of(d.queries[0])]
    assert url_order != [h for h, _, _ in d.facets[0]]  # the host order is not the url order
    for name, k in (("alternating_a2", 2), ("alternating_a3", 3)):
        a = F.case(name)
        hosts = [bytes(r[6:12]) for r in F.rows_of(a.queries[1])]
        assert len(set(hosts)) == k and all(x != y for x, y in zip(hosts, hosts[1:]))  # no run before the sort
        assert len(hosts) > k * LR_TILE
    x = F.case("extremes")
    hs = [h for h, _, _ in x.facets[0]]
    assert hs[0] == F.H_ZERO and hs[1] == b"AAAAAB" and hs[-1] == F.H_TOP and hs[-2] == b"_____-"
    assert {b"BAAAAA", b"-_____"} < set(hs)  # differ from the extremes in their first character only


def test_exclusions_and_empties():
    c = F.case("exclusions")
    names = [n for n in F.REMOVALS for _ in range(2)]
    full = {h: F.NEX // 3 for h in F.XHOSTS}
    for name, q, f in zip(names, c.queries, c.facets):
        got = {h: n for h, n, _ in f}
        urls = {h: u for h, _, u in f}
        if name == "whole_host":
            assert F.XHOSTS[1] not in got and len(got) == 2
        elif name == "all_but_one":
            assert got[F.XHOSTS[1]] == 1 and urls[F.XHOSTS[1]][2:6] == F.iu.enc(F.ONE_LEFT, 4)
        elif name == "smallest_url":
            assert got[F.XHOSTS[0]] == full[F.XHOSTS[0]] - 1 and urls[F.XHOSTS[0]][2:6] == F.iu.enc(3, 4)
        else:
            assert sorted(p // LR_TILE for p in F.REMOVALS[name]) == [0, 0, 1, 1, 2, 2]
            assert sum(got.values()) == F.NEX - 6
        assert len(q[1]) == 1 and len(F.rows_of((q[0], (), q[2], q[3], q[4]))) == F.NEX
    for c in F.cases():
        if c.name.startswith("empty_"):
            assert [len(F.rows_of(q)) for q in c.queries] == [0, 100, 0, 100, 0], c.name
    assert all(len(F.rows_of(q)) == 0 for q in F.case("all_empties").queries)
    assert len({q for q in F.case("all_empties").queries}) == 3
    s = F.case("scattered_300")
    empty = [len(f) == 0 for f in s.facets]
    assert len(s.queries) == 300 and empty[0] and empty[-1] and 60 < sum(empty) < 150
    b = F.case("same_host_batch")
    assert b.queries[0] == b.queries[1] and all(f[0][0] == F.ONE_HOST for f in b.facets)
    sh = F.case("shapes")
    lens = [len(F.rows_of(q)) for q in sh.queries]
    assert lens[-1] == 6400 and all(lens) and all(f is None for f in sh.facets)
    assert len(sh.queries[0][0]) == 3 and sh.queries[1][2] == 2 and sh.queries[2][4] is not None
