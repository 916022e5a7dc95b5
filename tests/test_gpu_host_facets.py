"""GPU parity (MI355X) of yrwi_host_facets_batch: per query of a batch the hosts of its joined
container, their postings and each host's smallest url hash.

Every comparison is equality.  The inputs are those of facet_cases.py, whose stated facets
tests/test_facet_cases_ref.py checks against the numpy group-by over the oracle's rows; here
the device's answer equals them in both orders, with and without the urls, for every max_hosts
of the case, and agrees with yrwi_term_search_batch and yrwi_count_hosts on the same index."""

import numpy as np
import pytest

import facet_cases as F
from index_util import open_index, run_parts
from yacy_search_server_amd import Query, RankingProfile
from yacy_search_server_amd._lib import FACETS_ORDERS, YrwiError, lib

pytestmark = pytest.mark.gpu

E_ARG, E_HASH, E_UNSUPPORTED = -1, -2, -8
ORDERS = ("host", "count")
C5 = "date=15,domlength=15,authority=13,tf=10"  # an authority profile: the rank phase counts hosts itself


@pytest.fixture(scope="module")
def ix():
    x = open_index(F.index_dict(), url_ids=True)
    yield x
    x.close()


def _query(q):
    inc, exc, maxd, now, sel = q
    return Query(list(inc), list(exc), maxd, now_ms=now, urlselection=None if sel is None else list(sel))


class Out:
    """one raw call into caller buffers filled with 0xA5"""

    def __init__(self, index, qs, order, max_hosts, urls, cap, count_only=False):
        nq = len(qs)
        self.h6 = np.full(6 * max(cap, 1) + 6, 0xA5, dtype=np.uint8)
        self.cnt = np.full(max(cap, 1) + 1, -0x5A5A5A5A5A5A5A5B, dtype=np.int64)
        self.u12 = np.full(12 * max(cap, 1) + 12, 0xA5, dtype=np.uint8)
        self.off = np.full(nq + 1, -7, dtype=np.int64)
        self.nhosts = np.full(max(nq, 1), -7, dtype=np.int64)
        self.nrows = np.full(max(nq, 1), -7, dtype=np.int64)
        self.urls = urls
        self.rc, self.st = index.host_facets_batch_raw(
            [_query(q) for q in qs], FACETS_ORDERS[order], max_hosts, None if count_only else self.h6,
            None if count_only else self.cnt, self.u12 if urls and not count_only else None, cap, self.off,
            self.nhosts, self.nrows)

    def untouched(self):
        return (self.h6 == 0xA5).all() and (self.cnt == self.cnt[-1]).all() and (self.u12 == 0xA5).all()

    def facets(self, i):
        """query i's range as (host, count, url or None) triples"""
        a, b = int(self.off[i]), int(self.off[i + 1])
        hb, ub = self.h6.tobytes(), self.u12.tobytes()
        return [(hb[6 * j:6 * j + 6], int(self.cnt[j]), ub[12 * j:12 * j + 12] if self.urls else None)
                for j in range(a, b)]


def _expected(c, i, order, max_hosts, urls):
    return [(h, n, u if urls else None) for h, n, u in F.expected(c, i, order, max_hosts)]


def _check_case(index, c, sub=None):
    """the case's batch (or the queries `sub` of it) in both orders, with and without urls, for every
    max_hosts of the case"""
    sel = list(range(len(c.queries))) if sub is None else list(sub)
    qs = [c.queries[i] for i in sel]
    for order in ORDERS:
        for urls in (True, False):
            for mh in c.max_hosts:
                want = [_expected(c, i, order, mh, urls) for i in sel]
                total = sum(len(w) for w in want)
                o = Out(index, qs, order, mh, urls, total)  # the exact capacity
                tag = (c.name, order, urls, mh)
                assert o.rc == 0, (tag, lib().yrwi_last_error(index._h))
                assert list(o.off) == list(np.cumsum([0] + [len(w) for w in want])), tag
                for k, i in enumerate(sel):
                    assert o.facets(k) == want[k], (tag, i)
                    full = F.expected(c, i, "host", 0)
                    assert o.nhosts[k] == len(full) and o.nrows[k] == sum(n for _, n, _ in full), (tag, i)
                # nothing behind the last entry, and no url without being asked
                assert (o.h6[6 * total:] == 0xA5).all() and (o.u12[12 * total if urls else 0:] == 0xA5).all(), tag
                assert (o.cnt[total:] == o.cnt[-1]).all(), tag
                assert o.st.hosts_out == total and o.st.hosts == int(o.nhosts[:len(sel)].sum()), tag
                assert o.st.rows_kept == int(o.nrows[:len(sel)].sum()) <= o.st.rows_joined, tag


SMALL = [c.name for c in F.cases() if c.name not in ("exclusions", "scattered_300", "shapes")]


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", SMALL)
def test_case(ix, name):
    c = F.case(name)
    _check_case(ix, c)
    if name in ("lengths", "same_host_batch"):  # each query alone as well
        for i in range(len(c.queries)):
            _check_case(ix, c, [i])


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("chain", [True, False])
def test_exclusions(ix, chain, monkeypatch):
    """chain=False (YRWI_NO_CHAIN=1, read per call): the two-term folds run step by step and their
    exclusions leave marks, as a single list's always does -- those rows get the sentinel key;
    chained, a fold drops its excluded rows within the join"""
    if not chain:
        monkeypatch.setenv("YRWI_NO_CHAIN", "1")
    c = F.case("exclusions")
    _check_case(ix, c)
    for i in range(len(c.queries)):
        _check_case(ix, c, [i])
    o = Out(ix, c.queries, "host", 0, False, 64)
    assert o.rc == 0 and o.st.rows_kept < o.st.rows_joined  # every single list arrives whole, marks and all
    if not chain:
        assert o.st.rows_joined == len(c.queries) * F.NEX


# ------------------------------------------------------------------ 3
def test_300_queries_with_empties(ix):
    _check_case(ix, F.case("scattered_300"))


# ------------------------------------------------------------------ 4
def test_other_query_shapes(ix):
    _check_case(ix, F.case("shapes"))


# ------------------------------------------------------------------ 5
def test_agrees_with_term_search_batch_and_count_hosts(ix):
    for name in ("lengths", "exclusions", "empty_all_excluded", "shapes", "ties"):
        c = F.case(name)
        rows, _ = ix.term_search_batch([_query(q) for q in c.queries])
        facets, nhosts, nrows, st = ix.host_facets_batch([_query(q) for q in c.queries], order="count", max_hosts=0)
        for i, (hosts, counts, urls) in enumerate(facets):
            assert int(counts.sum()) == nrows[i] == len(rows[i]), (name, i)
            assert len(hosts) == nhosts[i] == len(urls), (name, i)
            assert all(u[6:] == h for h, u in zip(hosts, urls)), (name, i)
    # a single-term query: its counts are yrwi_count_hosts' of that term
    for name in ("distinct", "ties", "extremes", "alternating_a3"):
        q = F.case(name).queries[0]
        assert len(q[0]) == 1 and not q[1]
        facets, _, _, _ = ix.host_facets_batch([_query(q)], order="host", urls=False)
        hosts, counts, urls = facets[0]
        assert urls is None and len(hosts) > 0
        got, _ = ix.count_hosts(hosts, [q[0][0]])
        assert (got == counts).all(), name


# ------------------------------------------------------------------ 6
def test_capacity_and_count_only(ix):
    c = F.case("exclusions")
    qs = list(c.queries) + [F.case("all_empties").queries[1]] + list(F.case("ties").queries)
    for order, mh in (("count", 0), ("host", 2)):
        want = np.cumsum([0] + [len(F.R.ordered(list(F.facets_of(q)), order, mh)) for q in qs])
        total = int(want[-1])
        assert total >= 20
        exact = Out(ix, qs, order, mh, True, total)
        assert exact.rc == 0 and (exact.off == want).all()
        short = Out(ix, qs, order, mh, True, total - 1)
        assert short.rc == E_ARG and (short.off == want).all()  # the offsets say what a retry needs
        assert short.untouched()
        assert (short.nhosts == exact.nhosts).all() and (short.nrows == exact.nrows).all()
        assert short.st.syncs == 1 and short.st.bytes_d2h == 8 * (3 * len(qs) + 2)
        only = Out(ix, qs, order, mh, False, -0, count_only=True)
        assert only.rc == 0 and (only.off == want).all() and only.untouched()
        assert (only.nhosts == exact.nhosts).all() and (only.nrows == exact.nrows).all()
        assert only.st.syncs == 1 and only.st.bytes_d2h == 8 * (3 * len(qs) + 2)
        roomy = Out(ix, qs, order, mh, True, total + 5)
        assert roomy.rc == 0 and [roomy.facets(i) for i in range(len(qs))] == [exact.facets(i) for i in range(len(qs))]


# ------------------------------------------------------------------ 7
def test_errors(ix):
    good = F.case("lengths").queries[3]
    qs = [good] * 7 + [F.Q((b"not*base64!!",))] + [good] * 4
    o = Out(ix, qs, "count", 0, True, 64)
    assert o.rc == E_HASH and (o.off == -7).all() and (o.nhosts == -7).all() and (o.nrows == -7).all()
    assert o.untouched()
    assert lib().yrwi_last_error(ix._h).decode().startswith("query 7: ")
    L, off = lib(), np.full(2, -7, dtype=np.int64)
    call = lambda cq, nq, order, mh, h6, cnt, cap, offp: L.yrwi_host_facets_batch(
        ix._h, cq, nq, order, mh, h6, cnt, None, cap, offp, None, None, None)
    assert call(None, 0, 1, 0, None, None, 0, off.ctypes.data) == 0 and off[0] == 0
    assert ix.host_facets_batch([])[0] == []
    cq = ix._marshal([_query(good)], 1)
    h6, cnt = np.zeros(64, dtype=np.uint8), np.zeros(8, dtype=np.int64)
    assert call(cq[0], 1, 2, 0, h6.ctypes.data, cnt.ctypes.data, 8, off.ctypes.data) == E_ARG   # the order
    assert call(cq[0], 1, -1, 0, h6.ctypes.data, cnt.ctypes.data, 8, off.ctypes.data) == E_ARG
    assert call(cq[0], 1, 0, -1, h6.ctypes.data, cnt.ctypes.data, 8, off.ctypes.data) == E_ARG  # max_hosts < 0
    assert call(cq[0], 1, 0, 0, h6.ctypes.data, cnt.ctypes.data, -1, off.ctypes.data) == E_ARG  # cap < 0
    assert call(cq[0], -1, 0, 0, h6.ctypes.data, cnt.ctypes.data, 8, off.ctypes.data) == E_ARG  # nq < 0
    assert call(None, 1, 0, 0, h6.ctypes.data, cnt.ctypes.data, 8, off.ctypes.data) == E_ARG    # no queries
    assert call(cq[0], 1, 0, 0, h6.ctypes.data, cnt.ctypes.data, 8, None) == E_ARG              # no host_off
    assert call(cq[0], 1, 0, 0, h6.ctypes.data, None, 8, off.ctypes.data) == E_ARG              # half a result
    assert (off == [0, -7]).all()
    _check_case(ix, F.case("ties"))  # and the context still answers


def test_sharded_context_is_refused():
    def fn(r, x):
        if r:
            return
        with pytest.raises(YrwiError) as e:
            x.host_facets_batch([Query([F.ABSENT], now_ms=F.NOW)])
        assert e.value.rc == E_UNSUPPORTED

    run_parts([{}, {}], 2, fn, timeout=120)


# ------------------------------------------------------------------ 8
# include/yrwi.h, "Shape of the call"
def _header_launches(order, urls, count_only):
    return 12 if count_only else 15 + (1 if urls else 0) + (2 if order == "count" else 0)


def test_shape_of_the_call(ix):
    """the library's own counters (no times): launches and host waits after the join phase depend on
    the form of the call alone, never on the number of queries or on the lists; what crosses PCIe
    towards the host is the triples and 3 nq + 2 words; the second call allocates nothing"""
    kinds = [F.case("exclusions").queries[1], F.case("ties").queries[0], F.case("shapes").queries[4]]
    for order in ORDERS:
        for urls in (True, False):
            for count_only in (False, True):
                if count_only and urls:
                    continue
                seen = set()
                for kind in kinds:
                    for nq in (300, 1):  # the largest first: scratch and staging reach their size
                        cap = nq * len(F.facets_of(kind))
                        if nq == 300:  # a first call may grow the lane's scratch, the next one folds it into one block
                            Out(ix, [kind] * nq, order, 0, urls, cap, count_only)
                        Out(ix, [kind] * nq, order, 0, urls, cap, count_only)
                        o = Out(ix, [kind] * nq, order, 0, urls, cap, count_only)
                        print(order, "urls", urls, "count_only", count_only, "nq", nq, "launches_tail",
                              o.st.launches_tail, "syncs", o.st.syncs, "d2h", o.st.bytes_d2h, "hosts_out",
                              o.st.hosts_out, "allocs", o.st.device_allocs)
                        assert o.rc == 0 and o.st.device_allocs == 0
                        assert o.st.launches_tail == _header_launches(order, urls, count_only)
                        assert o.st.syncs == (1 if count_only else 2)
                        if not count_only:
                            assert o.st.hosts_out == cap
                            assert o.st.bytes_d2h <= 26 * o.st.hosts_out + 8 * (3 * nq + 2)
                            assert o.st.bytes_d2h == (26 if urls else 14) * o.st.hosts_out + 8 * (3 * nq + 2)
                        seen.add((o.st.launches_tail, o.st.syncs))
                assert len(seen) == 1


# ------------------------------------------------------------------ 9
def test_context_untouched(ix):
    h = F.C.dense_terms
    c5 = RankingProfile("", C5)
    batch = [Query(h((0, 1)), now_ms=F.NOW, profile=c5), Query(h((0, 1, 2)), h((3,)), now_ms=F.NOW),
             Query(h((4,)), now_ms=F.NOW, profile=c5)]
    hits = lambda: [[(x.urlhash, x.score, x.tiebreak) for x in g] for g in ix.search_batch(batch)]
    before, info, stats = hits(), ix.index_info(), ix.stats()
    assert all(before)
    _check_case(ix, F.case("shapes"))
    _check_case(ix, F.case("exclusions"))
    assert ix.index_info() == info and ix.stats() == stats and hits() == before
