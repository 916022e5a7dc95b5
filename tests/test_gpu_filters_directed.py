"""The query filters (admit / passes in k_score and k_score_full, the flag counts, the per-query
threshold) and the doubledom pull (k_pull) on the directed inputs of tests/filter_cases.py against
java_literal.search over the same lists: url hashes, scores, tiebreaks and their order, and
QueryFilter.flagcount against the literal filter's counts.  Every comparison is equality.

  test_case[<family>/<name>]   one case through RWIIndex.search; one device index per family
  test_counts_do_not_depend_on_k  the 6145-row list at k = 1, 100, 256, 257, 3000 in one call
  test_threshold_in_a_crowded_call  8192 threshold queries in one call: later chunks meet a threshold
  test_batch_300               300 queries of one search_batch, every third without a filter, each
                               filter object with its own counts
  test_doubledom_beside_plain  a doubledom query, a plain and a filtered one with k = 10, one call

tests/test_filter_cases_ref.py holds the CPU checks of the inputs."""

import pytest

import filter_cases as fc
import java_literal as jl
from index_util import open_index

pytestmark = pytest.mark.gpu

ALL = [(f, n) for f in fc.FAMILIES for n in fc.names(f)]
_LIT = {}


def _rp(p):
    from yacy_search_server_amd import RankingProfile
    if p is None:
        return None
    rp = RankingProfile()
    for _, f in jl.PROFILE_FIELDS:
        setattr(rp, f, getattr(p, f))
    return rp


def _literal(key, lists):
    if key not in _LIT:
        _LIT[key] = fc.literal_lists(lists)
    return _LIT[key]


@pytest.fixture(scope="module")
def indexes():
    """key -> the device index with the family's lists; one is open at a time (the tests come
    family by family)"""
    held = {}

    def get(key, lists=None):
        if key not in held:
            for ix in held.values():
                ix.close()
            held.clear()
            held[key] = open_index(lists if lists is not None else fc.family_lists(key))
        return held[key]

    yield get
    for ix in held.values():
        ix.close()


def _expected(lit, c):
    """(hits as (urlhash, score, tiebreak), the literal filter's counts or None)"""
    lf = jl.QueryFilter(**c.kw) if c.kw is not None else None
    e = jl.search(lit, c.include, c.exclude, c.literal_profile(), c.language, now_ms=fc.NOW, k=c.k, filt=lf)
    return [(u, s, jl.bytearray_hashcode(u)) for u, s in e], (lf.flagcount if lf is not None else None)


def _query(c):
    from yacy_search_server_amd import Query, QueryFilter
    gf = QueryFilter(**c.kw) if c.kw is not None else None
    return Query(c.include, c.exclude, k=c.k, profile=_rp(c.profile), language=c.language, now_ms=fc.NOW, filter=gf)


def _same(got, q, exp, counts, c):
    g = [(h.urlhash, h.score, h.tiebreak) for h in got]
    i = next((j for j, (a, b) in enumerate(zip(g, exp)) if a != b), min(len(g), len(exp)))
    assert g == exp, (c.name, "hits", len(g), len(exp), "first difference at", i, g[i:i + 2], exp[i:i + 2])
    if counts is not None:
        assert q.filter.flagcount == counts, (c.name, "flagcount", q.filter.flagcount, counts)
        assert counts == c.flagcount, (c.name, "the literal's counts against the construction")
    if not (c.kw or {}).get("skip_double_dom"):
        assert {u for u, _, _ in g} <= c.admitted, (c.name, "a hit outside the admitted set")


def _run(ix, lit, c, monkeypatch):
    for name, value in c.env.items():
        monkeypatch.setenv(name, value)
    exp, counts = _expected(lit, c)
    q = _query(c)
    got = ix.search(q.include, q.exclude, q.profile, q.language, now_ms=q.now_ms, k=q.k, filter=q.filter)
    _same(got, q, exp, counts, c)


@pytest.mark.parametrize("family,name", ALL, ids=[n for _, n in ALL])
def test_case(indexes, monkeypatch, family, name):
    c = fc.case(family, name)
    lit = _literal(family, fc.family_lists(family))
    ix = indexes(family)
    _run(ix, lit, c, monkeypatch)
    if c.twin is not None:
        _run(ix, lit, c.twin, monkeypatch)


def _run_batch(ix, lit, cases):
    qs = [_query(c) for c in cases]
    got = ix.search_batch(qs)
    assert len(got) == len(cases)
    memo = {}
    for c, q, g in zip(cases, qs, got):
        key = (tuple(c.include), tuple(c.exclude), c.k, repr(sorted((c.kw or {"": 0}).items())), c.kw is None)
        if key not in memo:
            memo[key] = _expected(lit, c)
        exp, counts = memo[key]
        _same(g, q, exp, counts, c)


def test_counts_do_not_depend_on_k(indexes):
    """one call: k_score counts alone for k > SCORE_SMALL and scores as well below; the counts of
    the five filter objects are the same and exact"""
    cases = [fc.case("counting", "counting/k%d" % k) for k in fc.COUNT_KS]
    _run_batch(indexes("counting"), _literal("counting", fc.family_lists("counting")), cases)


def test_threshold_in_a_crowded_call(indexes):
    """A query alone has its four chunks scored side by side, each before any threshold exists
    (as have 2048 such queries: measured on an MI355X, a threshold published from the unfiltered
    chunk changed nothing below 8192).  2048 copies of the four threshold queries in one call are
    32768 chunks, first chunks first: the later chunks of a query start after its first chunk,
    all rejected and scoring highest, is done, and a threshold that counted rejected postings
    cuts every admitted one."""
    cases = [fc.case("threshold", n) for n in fc.names("threshold")] * 2048
    _run_batch(indexes("threshold"), _literal("threshold", fc.family_lists("threshold")), cases)


def test_batch_300(indexes):
    b = fc.batch_case()
    _run_batch(indexes(b.name, b.lists), _literal(b.name, b.lists), b.queries)


def test_doubledom_beside_plain(indexes):
    b = fc.doubledom_batch()
    _run_batch(indexes("doubledom"), _literal("doubledom", fc.family_lists("doubledom")), b.queries)
