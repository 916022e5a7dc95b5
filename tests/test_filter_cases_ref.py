"""The directed filter and doubledom inputs of tests/filter_cases.py, checked on the CPU: what each
case claims by construction (the admitted urls and the flag counts from the generating arrays, the
stack's hosts, the pulled order written by hand) against java_literal (QueryFilter.admit over the
joined container, search, pull_double_dom) -- two independent statements of SearchEvent.java:736-806
and :1297-1394 -- and the properties a case was built for (scores distinct, scores moved, a tie at
the cut), so that an input cannot drift away from its point.  tests/test_gpu_filters_directed.py
runs the same cases through the library."""

import functools

import pytest

import filter_cases as fc
import java_literal as jl

ALL = [(f, n) for f in fc.FAMILIES for n in fc.names(f)]


@functools.lru_cache(maxsize=None)
def _lit(family):
    return fc.literal_lists(fc.family_lists(family))


def _container(lit, c):
    return jl.term_search(lit, c.include, c.exclude, 2147483647, fc.NOW)


def _admit(lit, c):
    """QueryFilter.admit over the case's joined container: (admitted urls, the counts)"""
    f = jl.QueryFilter(**c.kw)
    rows = _container(lit, c)
    adm = frozenset(r[:12] for r in rows if f.admit(jl.Vars.from_row(r, fc.NOW)))
    return adm, f.flagcount, len(rows)


def _stack(lit, c, doubledom=False, k=fc.MAX_K):
    kw = dict(c.kw or {}, skip_double_dom=doubledom)
    return jl.search(lit, c.include, c.exclude, c.literal_profile(), c.language, now_ms=fc.NOW, k=k,
                     filt=jl.QueryFilter(**kw))


@pytest.mark.parametrize("family,name", ALL, ids=[n for _, n in ALL])
def test_construction_agrees_with_the_literal(family, name):
    c = fc.case(family, name)
    for x in (c, c.twin):
        if x is None:
            continue
        adm, counts, n = _admit(_lit(family), x)
        assert n == x.container, (x.name, n, x.container)
        assert adm == x.admitted, (x.name, len(adm), len(x.admitted), sorted(adm ^ x.admitted)[:3])
        assert counts == x.flagcount, (x.name, counts, x.flagcount)


@pytest.mark.parametrize("family,name", ALL, ids=[n for _, n in ALL])
def test_no_case_is_vacuous(family, name):
    c = fc.case(family, name)
    assert ("admits nothing" in name) == (c.vacuous == "nothing") and \
           ("admits everything" in name) == (c.vacuous == "everything"), name
    if c.vacuous == "nothing":
        assert len(c.admitted) == 0 and c.container > 0, name
    elif c.vacuous == "everything":
        assert len(c.admitted) == c.container > 0, name
    elif family != "doubledom":   # a doubledom case is about the order; only one of them filters
        assert 0 < len(c.admitted) < c.container, (name, len(c.admitted), c.container)


def test_families_cover_what_they_name():
    """the points of the cases that a loose edit of the module could lose"""
    by = {n: fc.case(f, n) for f, n in ALL}
    bit = lambda j: by["flags/any_bit%d" % j]
    assert len({bit(j).admitted for j in (0, 7, 8, 15, 16, 20, 21, 22, 23, 24, 31)}) == 11
    assert any(v for v in by["language/'eng' (admits nothing)"].flagcount)   # rejects all, counts all
    assert by["doublecheck/every_url (admits nothing)"].flagcount == [0] * 32
    dc = by["doublecheck/then_language"]
    assert 0 < sum(dc.flagcount) < sum(by["doublecheck/absent (admits everything)"].flagcount)
    many = by["doublecheck/many5000"].kw["urlhashes"]
    assert len(many) == 5000 and len(set(many)) < 5000 and many != sorted(many)
    for n in ("first", "last", "inside", "none"):
        ex = next(c for k, c in by.items() if k.startswith("site/ex4097_" + n)).kw["siteexcludes"]
        keys = [fc.host_key(h) for h in ex]
        assert len(set(keys)) == 4097 and len(keys) > 4097 and keys != sorted(keys), n
        assert (min(keys) == 0) == (n == "first") and (max(keys) == (1 << 36) - 1) == (n == "last"), n
    counts = [by["counting/k%d" % k] for k in fc.COUNT_KS]
    assert all(c.container == 3 * fc.CHUNK + 1 and c.flagcount == counts[0].flagcount for c in counts)
    assert [c.k for c in counts] == [1, 100, fc.SCORE_SMALL, fc.SCORE_SMALL + 1, fc.MAX_K]
    assert 0.25 < len(counts[0].admitted) / counts[0].container < 0.42


def test_tied_cut_case_ties():
    c = fc.case("counting", "counting/tied_cut")
    st = _stack(_lit("counting"), c)
    assert len(st) == len(c.admitted) > fc.SCORE_SMALL > c.k and len({s for _, s in st}) == 1


@pytest.mark.parametrize("name", fc.names("threshold"))
def test_threshold_cases_are_aimed(name):
    """distinct scores; the first 2048 rows in list order are rejected and score above everything
    else; every admitted row scores below every rejected one"""
    c = fc.case("threshold", name)
    lit = _lit("threshold")
    (t, rows), = c.lists.items()
    full = dict(jl.search(lit, c.include, [], c.literal_profile(), "en", now_ms=fc.NOW, k=fc.MAX_K * 3,
                          filt=None))   # the first MAX_K of the whole list
    order = jl.ReferenceOrder(c.literal_profile(), "en")
    scores = {e.urlHash: order.cardinal(e) for e in order.normalize_with(lit[t], fc.NOW)}
    assert len(set(scores.values())) == len(rows) == 3 * fc.CHUNK + 1
    assert all(scores[u] == s for u, s in full.items())
    first = [bytes(r[:12]) for r in rows[:fc.CHUNK]]
    assert not set(first) & c.admitted
    rest = [bytes(r[:12]) for r in rows[fc.CHUNK:]]
    assert min(scores[u] for u in first) > max(scores[u] for u in rest)
    assert max(scores[u] for u in c.admitted) < min(s for u, s in scores.items() if u not in c.admitted)
    where = {i // fc.CHUNK for i, r in enumerate(rows) if bytes(r[:12]) in c.admitted}
    assert where == ({1, 2, 3} if "spread" in name else {2, 3}), where
    assert len(c.admitted) > c.k


@pytest.mark.parametrize("name", fc.names("norm"))
def test_norm_cases_move_a_score(name):
    c = fc.case("norm", name)
    lit = _lit("norm")
    with_, without = dict(_stack(lit, c)), dict(_stack(lit, c.twin))
    assert set(with_) == set(without) == c.admitted == c.twin.admitted
    assert c.container == c.twin.container + 2
    assert any(with_[u] != without[u] for u in with_), name


DD = [n for n in fc.names("doubledom")]


@pytest.mark.parametrize("name", DD)
def test_doubledom_stack_and_pull(name):
    c = fc.case("doubledom", name)
    lit = _lit("doubledom")
    st = _stack(lit, c)                                   # without doubledom: the stack, cut at MAX_K
    assert [u[6:12] for u, _ in st] == c.stack_hosts[:fc.MAX_K], name
    assert len({s for _, s in st}) == len(st), name       # distinct scores: the order is designed
    if c.pattern is not None:
        letters = {fc.letter_host(ch): ch for ch in c.pattern}
        letters.update({fc.H_ZERO: "A", fc.H_TOP: "Z", fc.slot_zero_host(): "X"} if "zero" in name else {})
        assert "".join(letters[h] for h in c.stack_hosts) == c.pattern, name
        pulled = jl.pull_double_dom(st, c.k)
        if c.pulled is not None:
            assert "".join(letters[u[6:12]] for u, _ in pulled) == c.pulled, name
    assert _stack(lit, c, doubledom=True, k=c.k) == jl.pull_double_dom(st, c.k)


def test_doubledom_family_holds_the_named_shapes():
    by = {n: fc.case("doubledom", n) for n in DD}
    assert by["doubledom/AABACB_short_stack"].k > len(by["doubledom/AABACB_short_stack"].stack_hosts)
    assert {by[n].k for n in DD} >= {1, 10, fc.MAX_K}
    assert len(set(by["doubledom/one_host_3000"].stack_hosts)) == 1
    d = by["doubledom/distinct_hosts_3000"].stack_hosts
    assert len(set(d)) == len(d) == fc.MAX_K and {fc.H_ZERO, fc.H_TOP, fc.slot_zero_host()} <= set(d)
    assert len(by["doubledom/stack_cut_3500"].stack_hosts) == 3500
    lf = by["doubledom/language_filter"]
    assert 0 < len(lf.admitted) < lf.container and any(lf.flagcount)
    hand = [n for n in DD if by[n].pulled is not None]
    assert len(hand) >= 8
    assert fc._mix64(fc.host_key(fc.slot_zero_host())) % fc.DD_SLOTS == 0


def test_batch_case_shape():
    b = fc.batch_case()
    q = b.queries
    assert len(q) == 300 and all((x.kw is None) == (i % 3 == 0) for i, x in enumerate(q))
    bare = [x for x in q if x.kw is not None and not x.kw.get("siteexcludes") and not x.kw.get("urlhashes")]
    assert len(bare) >= 2
    a, c = q[100], q[101]
    assert a.kw is not None and a.kw is not c.kw and (a.kw, a.include, a.exclude, a.k) == (c.kw, c.include, c.exclude, c.k)
    lit = fc.literal_lists(b.lists)
    for x in q:
        if x.kw is None:
            assert frozenset(r[:12] for r in _container(lit, x)) == x.admitted, x.name
        else:
            adm, counts, n = _admit(lit, x)
            assert (adm, counts, n) == (x.admitted, x.flagcount, x.container), x.name
    d = fc.doubledom_batch().queries
    assert d[0].kw["skip_double_dom"] and d[1].kw is None and d[1].k == 10
    lit = fc.literal_lists(d[0].lists)
    adm, counts, _ = _admit(lit, d[2])
    assert (adm, counts) == (d[2].admitted, d[2].flagcount) and 0 < len(adm) < d[2].container
