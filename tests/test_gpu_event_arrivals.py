"""The search-event path on the device (k_event_add, the url set and host table around it,
yrwi_event_pull / result / source / order / authority) on the directed inputs of
tests/event_cases.py against java_literal.SearchEventRWI: every comparison is equality, and it
is made after every step of a case, not only at its end.

  test_<group>              every case of the group: hits as (urlhash, score, tiebreak), the info
                            fields, the pulled hits, a rejected arrival's code and the untouched
                            event after it, and at the end the (arrival, row) of every url
  test_one_call_many_events the small `sizes` cases and every `fold` case as separate events of one
                            yrwi_event_add call (both arrivals of an event in the call: its jobs
                            run in one workgroup with the state in LDS), then split over two calls
  test_order_only           fold, first-row and authority cases through yrwi_event_order /
                            yrwi_event_authority against ReferenceOrder.normalize_with + cardinal

tests/test_event_cases_ref.py holds the CPU checks of the inputs."""

import numpy as np
import pytest

import event_cases as ec
import java_literal as jl

pytestmark = pytest.mark.gpu

UNSEEN = b"zzzzzzzzzzzA"
_ORACLE = {}


def _oracle(group, name):
    if (group, name) not in _ORACLE:
        _ORACLE[(group, name)] = ec.run_oracle(ec.case(group, name))[:2]
    return _ORACLE[(group, name)]


@pytest.fixture(scope="module")
def ix():
    from yacy_search_server_amd import RWIIndex
    x = RWIIndex(0)
    yield x
    x.close()


def _open(ix, c):
    from yacy_search_server_amd import QueryFilter, RankingProfile
    gf = QueryFilter(**c.kw) if c.kw is not None else None
    return ix.event(ec.profile_of(c, RankingProfile), c.language, ec.NOW, k=c.k, filter=gf,
                    max_postings=c.total_rows() + 16)


def _fields(c):
    return [f for f in ec.INFO_FIELDS if f != "maxdomcount" or c.profile.get("coeff_authority", 0) > 12]


def _state(ev, c):
    hits, info = ev.results()
    d = {f: (list(info.flagcount) if f == "flagcount" else int(getattr(info, f))) for f in _fields(c)}
    return [(h.urlhash, h.score, h.tiebreak) for h in hits], d


def _expected(rec, c):
    return rec["stack"][:c.k], {f: rec["info"][f] for f in _fields(c)}


def _check_sources(ev, c, sources):
    us = ec.all_urls(c) + [UNSEEN]
    assert ev.source(us) == [sources.get(u, (-1, -1)) for u in us]


def _run_case(ix, group, name):
    from yacy_search_server_amd._lib import YrwiError
    c = ec.case(group, name)
    recs, sources = _oracle(group, name)
    with _open(ix, c) as ev:
        for j, (s, rec) in enumerate(zip(c.steps, recs)):
            if s[0] == "add":
                ev.add_rwis(s[1], s[2])
            elif s[0] == "bad":
                before = _state(ev, c)
                with pytest.raises(YrwiError) as e:
                    ev.add_rwis(s[1], s[2])
                assert e.value.rc == s[3], (name, j)
                assert _state(ev, c) == before, (name, j)
            else:
                got = [(h.urlhash, h.score, h.tiebreak) for h in ev.pull(s[1], s[2])]
                assert got == [(u, w, jl.bytearray_hashcode(u)) for u, w in rec["pulled"]], (name, j)
            hits, info = _state(ev, c)
            ehits, einfo = _expected(rec, c)
            assert info == einfo, (name, j)
            assert hits == ehits, (name, j)
        _check_sources(ev, c, sources)


def _group_test(group):
    @pytest.mark.parametrize("name", ec.names(group))
    def test(ix, name):
        _run_case(ix, group, name)
    test.__name__ = test.__qualname__ = "test_" + group
    return test


test_sizes = _group_test("sizes")
test_fold = _group_test("fold")
test_first_row = _group_test("first_row")
test_stack = _group_test("stack")
test_ties = _group_test("ties")
test_doublecheck = _group_test("doublecheck")
test_authority = _group_test("authority")
test_rejects = _group_test("rejects")
test_pulls = _group_test("pulls")


def _many(ix, cases, calls):
    """every case an event of its own; calls = 1: all arrivals in one yrwi_event_add call (an
    event's arrivals one after the other), 2: the first arrivals in one call, the rest in a second"""
    evs = [_open(ix, c) for _, c in cases]
    try:
        if calls == 1:
            ix.add_rwis([(ev, s[1], s[2]) for ev, (_, c) in zip(evs, cases) for s in c.steps])
        else:
            ix.add_rwis([(ev, c.steps[0][1], c.steps[0][2]) for ev, (_, c) in zip(evs, cases)])
            ix.add_rwis([(ev, s[1], s[2]) for ev, (_, c) in zip(evs, cases) for s in c.steps[1:]])
        out = []
        for ev, (g, c) in zip(evs, cases):
            recs, sources = _oracle(g, c.name)
            st = _state(ev, c)
            assert st[1] == _expected(recs[-1], c)[1], c.name
            assert st[0] == _expected(recs[-1], c)[0], c.name
            _check_sources(ev, c, sources)
            out.append(st)
        return out
    finally:
        for ev in evs:
            ev.close()


def test_one_call_many_events(ix):
    cases = [("sizes", c) for c in ec.sizes() if len(c.steps[0][1]) <= 257] + [("fold", c) for c in ec.fold()]
    assert all(s[0] == "add" for _, c in cases for s in c.steps)
    assert sum(len(c.steps) == 2 for _, c in cases) > 50
    one = _many(ix, cases, 1)
    two = _many(ix, cases, 2)
    assert one == two


def _order_cases():
    return [(g, n) for g in ("fold", "first_row", "authority") for n in ec.names(g)]


@pytest.mark.parametrize("group,name", _order_cases(), ids=[n for _, n in _order_cases()])
def test_order_only(ix, group, name):
    from yacy_search_server_amd import RankingProfile
    c = ec.case(group, name)
    lp = ec.profile_of(c)
    order = jl.ReferenceOrder(lp, c.language)
    hosts = {}
    with ix.reference_order(ec.profile_of(c, RankingProfile), c.language, ec.NOW) as ro:
        for j, s in enumerate(c.steps):
            if s[0] != "add":  # the oracle never sees a rejected arrival; its parity is test_first_row's
                continue
            got = ro.order(s[1], s[2])
            rows = [bytes(r) for r in s[1]]
            exp = [order.cardinal(e) for e in order.normalize_with(rows, ec.NOW)]
            assert [int(x) for x in got] == exp, (name, j)
            hosts.update(dict.fromkeys(r[6:12] for r in rows))
            if lp.coeff_authority > 12:  # the host counts exist for authority profiles only (yrwi.h)
                hs = list(hosts) + [UNSEEN[6:12]]
                assert ro.authority(hs) == [order.authority(h) for h in hs], (name, j)
