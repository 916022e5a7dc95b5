"""GPU parity (MI355X) of yrwi_abstract.hip on the directed inputs of tests/abstract_cases.py.

Serving side: yrwi_index_abstracts (compressIndex).  Asking side: yrwi_secondary_search
(decompressIndex, addAbstract, joinConstructive, prepareSecondarySearch).  Expected values come from
oracle/abstracts.py; every comparison is equality of bytes: the abstract texts, the join's urls and
peers, the words, and the plan's peers, urls and words.  tests/test_abstract_cases_ref.py shows on the
CPU that every input is what its name says.

What each test reaches:
  test_index_abstracts_case      k_ca_keys / k_ca_heads / k_ca_write at 1, 255, 256, 257 and 1,025
                                 postings with G = 1 and G = n; the 48-bit raw host sort against the
                                 list's Base64Order (384 hosts); the exclusion search and the
                                 excluded key 1 << 48 (none, all, all but one, one whole host, every
                                 second, a larger exclude list)
  test_index_abstracts_multi     one term twice in a call; an absent last term
  test_secondary_search_case     k_ss_bad's stop rules as the middle abstract of three; the parser
                                 at every residue of 16 and across the 4,096-byte blocks; the 72-bit
                                 key's characters 10 and 11; addAbstract's newest peer; the fold
                                 order and the word mask up to bit 31; the plan for 1..257 peers
  test_alignment_variants_agree  the 17 shifted texts give one result
  test_refusals                  YRWI_E_ARG for texts decompressIndex would misparse and for 33
                                 words; the context answers the next call
  test_int_wrap                  2,147,484 urls in one map: `size * 1000` wraps and the big map
                                 folds first
  test_capacity_*                the C ABI with exact and too small buffers, NULL outputs
  test_abstracts_after_maintenance   the list table after add_postings, remove_postings, remove_hosts"""

import ctypes
import time

import pytest

import abstract_cases as AC
import abstracts as ab
from yacy_search_server_amd import RWIIndex, _lib
from yacy_search_server_amd._lib import YrwiError

pytestmark = pytest.mark.gpu

E_ARG, E_HASH = -1, -2
CCASES = AC.compress_cases()
JCASES = AC.join_cases()
ABSENT = b"ABSabsent___"


def _term(i):
    return b"ABScase%03d__" % i


def _exterm(i):
    return b"ABSexcl%03d__" % i


@pytest.fixture(scope="module")
def cindex():
    """every compressIndex case under a term of its own, its exclude rows under another"""
    ix = RWIIndex(0)
    for i, c in enumerate(CCASES):
        ix.add(_term(i), c.rows)
        if c.ex_mode == "list":
            ix.add(_exterm(i), c.ex_rows)
    lists, _ = AC.multi_term()
    for t, r in lists.items():
        ix.add(t, r)
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def ix():
    x = RWIIndex(0)
    yield x
    x.close()


def _exclude_arg(i, c):
    return {None: None, "absent": ABSENT, "self": _term(i), "list": _exterm(i)}[c.ex_mode]


# ------------------------------------------------------------------ compressIndex
@pytest.mark.parametrize("i", range(len(CCASES)), ids=[c.name for c in CCASES])
def test_index_abstracts_case(cindex, i):
    c = CCASES[i]
    assert cindex.index_abstracts([_term(i)], exclude=_exclude_arg(i, c)) == [AC.compress_expected(c)]


def test_index_abstracts_multi(cindex):
    lists, calls = AC.multi_term()
    exp = {t: ab.compress_index(AC.row_list(r)) for t, r in lists.items()}
    (_, twice), (_, absent) = calls
    assert cindex.index_abstracts(twice) == [exp[t] for t in twice]
    assert cindex.index_abstracts(absent) == []
    assert cindex.index_abstracts(twice, exclude=AC.MT2) == [
        ab.compress_index(AC.row_list(lists[t]), AC.row_list(lists[AC.MT2])) for t in twice]
    # every case in one call, in reverse order: the texts lie back to back in one buffer
    terms = [_term(i) for i in reversed(range(len(CCASES)))]
    assert cindex.index_abstracts(terms) == [ab.compress_index(AC.row_list(c.rows)) for c in reversed(CCASES)]


# ------------------------------------------------------------------ decompressIndex, join, plan
def _search(ix, c):
    return ix.secondary_search(c.abstracts, c.nwords, c.mypeer, c.checked)


@pytest.mark.parametrize("i", range(len(JCASES)), ids=[c.name for c in JCASES])
def test_secondary_search_case(ix, i):
    c = JCASES[i]
    join, words, plan = _search(ix, c)
    ejoin, ewords, eplan = AC.expected(c)
    assert words == ewords
    assert join == ejoin
    assert plan == eplan


def test_alignment_variants_agree(ix):
    got = [_search(ix, c) for c in AC.alignment_cases()]
    assert len(got) == AC.NALIGN and len(got[0][0]) == 2460
    assert all(g == got[0] for g in got)


REFUSALS = AC.refusal_cases()


@pytest.mark.parametrize("i", range(len(REFUSALS)), ids=[c.name for c in REFUSALS])
def test_refusals(ix, i):
    with pytest.raises(YrwiError) as e:
        _search(ix, REFUSALS[i])
    assert e.value.rc == E_ARG
    good = AC.well_formed_case()
    assert _search(ix, good) == AC.expected(good)  # the same context answers the next call


def test_int_wrap(ix):
    """word X's map has 2,147,484 urls: 2,147,484 * 1000 is negative as a Java int, X folds first and
    the join carries X's peer (without the wrap: Y's).  The one large case of this file: 12.9 MB of
    text, 7.3 s on an MI355X (one host's run is scanned by one thread)"""
    c = AC.wrap_case()
    t0 = time.perf_counter()
    got = _search(ix, c)
    print("int wrap: %.2f s for %d bytes of abstracts" % (time.perf_counter() - t0, sum(len(t) for _, _, t in c.abstracts)))
    join, words, plan = AC.wrap_expected()
    assert {p for _, p in join} == {AC.P(1)} and len(join) == 30
    assert got == (join, words, plan)
    small = AC.well_formed_case()
    assert _search(ix, small) == AC.expected(small)


# ------------------------------------------------------------------ the C ABI's capacities
def _raw_abstracts(ix, terms, cap, exclude=None):
    """yrwi_index_abstracts with a buffer of exactly cap bytes (guard bytes behind it stay untouched)"""
    out = ctypes.create_string_buffer(b"\xA5" * (cap + 64), cap + 64)
    offs = (ctypes.c_int64 * (len(terms) + 1))()
    nout = ctypes.c_int32(-7)
    rc = _lib.lib().yrwi_index_abstracts(ix._h, b"".join(terms), len(terms), exclude, out, cap, offs, ctypes.byref(nout))
    raw = out.raw
    assert raw[cap:] == b"\xA5" * 64
    return rc, raw[:cap], list(offs), nout.value


def test_capacity_index_abstracts(cindex):
    terms = [AC.MT1, AC.MT2]
    exp = cindex.index_abstracts(terms)
    need = [len(exp[0]), len(exp[0]) + len(exp[1])]
    rc, raw, offs, nout = _raw_abstracts(cindex, terms, need[1])
    assert rc == 0 and nout == 2 and offs == [0] + need and raw == exp[0] + exp[1]
    rc, raw, offs, nout = _raw_abstracts(cindex, terms, need[1] - 1)
    assert rc == E_ARG and nout == 0 and offs == [0] + need  # offsets[t + 1]: the end that was needed
    rc, raw, offs, nout = _raw_abstracts(cindex, terms, need[0] - 1)
    assert rc == E_ARG and nout == 0 and offs[1] == need[0]
    rc, raw, offs, nout = _raw_abstracts(cindex, terms, need[1])  # the next call is right
    assert rc == 0 and nout == 2 and raw == exp[0] + exp[1]
    # an exclusion that leaves "{}": 2 bytes are enough, 1 is not
    rc, raw, offs, nout = _raw_abstracts(cindex, [AC.MT1], 2, exclude=AC.MT1)
    assert rc == 0 and raw == b"{}" and offs == [0, 2]
    rc, raw, offs, nout = _raw_abstracts(cindex, [AC.MT1], 1, exclude=AC.MT1)
    assert rc == E_ARG and offs == [0, 2]
    rc, _, _, nout = _raw_abstracts(cindex, terms, need[1], exclude=b"not a hash!!")
    assert rc == E_HASH and nout == 0
    assert cindex.index_abstracts(terms) == exp


def _raw_search(ix, c, cap, plan_cap, null=()):
    """yrwi_secondary_search with the given capacities; buffers are full size behind them"""
    n = len(c.abstracts)
    arr = (_lib.CAbstract * n)()
    keep = []
    for i, (w, p, t) in enumerate(c.abstracts):
        b = ctypes.create_string_buffer(bytes(t), max(1, len(t)))
        keep.append(b)
        arr[i].word[:] = list(w)
        arr[i].peer[:] = list(p)
        arr[i].text = ctypes.cast(b, ctypes.c_void_p)
        arr[i].len = len(t)
    full = sum(len(t) for _, _, t in c.abstracts) // 6 + 1
    bufs = {k: ctypes.create_string_buffer(b"\xA5" * (12 * full), 12 * full) for k in ("join_urls", "join_peers", "plan_urls")}
    bufs["words_out"] = ctypes.create_string_buffer(12 * 32)
    arg = {k: (None if k in null else v) for k, v in bufs.items()}
    plan = (_lib.CPeerRequest * max(1, n))()
    nj, npl, nw = ctypes.c_int64(-7), ctypes.c_int32(-7), ctypes.c_int32(-7)
    rc = _lib.lib().yrwi_secondary_search(ix._h, arr, n, c.nwords, c.mypeer, None, 0, arg["join_urls"], arg["join_peers"],
                                          cap, ctypes.byref(nj), plan, plan_cap, ctypes.byref(npl), arg["plan_urls"],
                                          arg["words_out"], ctypes.byref(nw))
    reqs = [(bytes(plan[i].peer), plan[i].words, plan[i].url_off, plan[i].url_n) for i in range(max(npl.value, 0))]
    return rc, nj.value, npl.value, nw.value, {k: v.raw for k, v in bufs.items()}, reqs


def test_capacity_secondary_search(ix):
    c = next(c for c in JCASES if c.name == "plan_skip_mypeer_and_checked")._replace(mypeer=AC.NOBODY, checked=())
    ejoin, ewords, eplan = AC.expected(c)
    J, NP = len(ejoin), len(eplan)
    assert J == 15 and NP == 5
    urls, peers = b"".join(u for u, _ in ejoin), b"".join(p for _, p in ejoin)
    purls = b"".join(u for _, us, _ in eplan for u in us)
    rc, nj, npl, nw, out, reqs = _raw_search(ix, c, J, NP)
    assert (rc, nj, npl, nw) == (0, J, NP, 1)
    assert out["join_urls"][:12 * J] == urls and out["join_peers"][:12 * J] == peers and out["plan_urls"][:12 * J] == purls
    assert out["words_out"][:12] == ewords[0]
    assert [r[0] for r in reqs] == [p for p, _, _ in eplan] and all(r[1] == 1 and r[3] == 3 for r in reqs)
    for k in ("join_urls", "join_peers", "plan_urls"):
        assert out[k][12 * J:] == b"\xA5" * (len(out[k]) - 12 * J)  # nothing behind the J-th entry
    rc, nj, npl, nw, out, reqs = _raw_search(ix, c, J - 1, NP)
    assert rc == E_ARG and nj == J  # *njoin says what was needed
    assert out["join_urls"] == b"\xA5" * len(out["join_urls"])
    rc, nj, npl, nw, out, reqs = _raw_search(ix, c, J, NP - 1)
    assert rc == E_ARG
    rc, nj, npl, nw, out, reqs = _raw_search(ix, c, J, NP)  # the next call is right
    assert (rc, nj, npl) == (0, J, NP) and out["join_urls"][:12 * J] == urls
    # NULL outputs are accepted; the others are filled as before
    rc, nj, npl, nw, out, reqs2 = _raw_search(ix, c, J, NP, null=("join_urls", "join_peers", "plan_urls", "words_out"))
    assert (rc, nj, npl, nw) == (0, J, NP, 1) and reqs2 == reqs
    rc, nj, npl, nw, out, _ = _raw_search(ix, c, J, NP, null=("join_urls",))
    assert rc == 0 and out["join_peers"][:12 * J] == peers and out["plan_urls"][:12 * J] == purls


# ------------------------------------------------------------------ after index maintenance
def test_abstracts_after_maintenance():
    """the abstract of a list after each maintenance call equals compress_index of get_list, and of
    the rows the call should have left (a stale list pointer would give the old abstract)"""
    T, X, O = b"ABSmaint1___", b"ABSmaintx___", b"ABSmainto___"
    base = AC.exclusion_base()
    own = AC.hashes(base)
    hosts = sorted({u[6:] for u in own})
    x = RWIIndex(0)
    try:
        x.add(O, AC.make_rows(AC.own_host_urls(500)))  # a neighbour in the index: T moves when it grows
        x.add(T, base)
        x.add(X, base[::4])

        def check(want_urls, ctx):
            rows = x.get_list(T)
            assert AC.hashes(rows) == sorted(want_urls, key=AC.b64key), ctx
            assert x.index_abstracts([T]) == [ab.compress_index(AC.row_list(rows))], ctx
            ex = x.get_list(X)
            assert x.index_abstracts([T, O], exclude=X)[0] == ab.compress_index(AC.row_list(rows), AC.row_list(ex)), ctx

        check(own, "put")
        new = [AC.enc6(AC.scr(i, 0xC2B2AE35)) + hosts[i % 5] for i in range(400)] + [AC.U(i, b"newHST") for i in range(40)]
        new = [u for u in new if u not in set(own)]
        st = x.add_postings([T] * len(new), AC.make_rows(new))
        assert st["added"] == len(set(new))
        have = set(own) | set(new)
        check(have, "add_postings")
        gone = sorted(have)[::3]
        assert x.remove_postings(gone, [T])["removed"] == len(gone)
        have -= set(gone)
        check(have, "remove_postings")
        x.remove_postings(AC.hashes(base[::8]), [X])  # the exclude list changes too
        check(have, "remove_postings on the exclude list")
        h = hosts[len(hosts) // 2]
        lost = {u for u in have if u[6:] == h}
        assert len(lost) >= 3 and x.remove_hosts([h], [T])["removed"] == len(lost)
        have -= lost
        check(have, "remove_hosts")
        assert h + b":" not in x.index_abstracts([T])[0]
    finally:
        x.close()
