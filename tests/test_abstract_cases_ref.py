"""The inputs of tests/abstract_cases.py are what their names say -- shown with oracle/abstracts.py
alone, on the CPU.  tests/test_gpu_abstracts_adversarial.py feeds the same inputs to the device; a
case that lost its point (a stop rule that no longer stops, a fold whose first word is the first
word anyway) would make that parity test pass for nothing, and fails here first."""

import time

import pytest

import abstract_cases as AC
import abstracts as ab


def _maps(case):
    """word -> url -> peer as addAbstract leaves them"""
    s = ab.SecondarySearch()
    for w, p, t in case.abstracts:
        s.add_abstract(w, ab.decompress_index(t, p))
    return {w: {u: next(iter(ps)) for u, ps in m.items()} for w, m in s.cache.items()}


def _case(name):
    return next(c for c in AC.join_cases() if c.name == name)


# ------------------------------------------------------------------ the oracle itself
def test_decompress_index_is_strict_where_it_parses():
    p = b"p" * 12
    for t in (b"{ab,cde:AAAAAA}", b"{host00:AAA:AA}", b"{host00:AAAAAAA}", b"{host00:AAAAAA,h st01:BBBBBB}"):
        with pytest.raises(ValueError):
            ab.decompress_index(t, p)
    # behind the stop nothing is looked at
    assert ab.decompress_index(b"{host00:AAAAAA,host01xBB BBB,ho,t02:CC:CCC}", p) == {AC.A0: {p}}
    assert ab.decompress_index(b"{host00:AAAAAA,h st01}", p) == {AC.A0: {p}}  # shorter than 13


def test_decompress_index_is_linear():
    """the text is not copied per url: 20,000 and 160,000 urls differ by a factor of 8 in length; a
    linear parse takes 8 times as long (12 with the larger dict's cache misses), a quadratic one 64
    times.  The bound lies between the two."""
    def run(n):
        t = b"{" + AC.WRAP_HOST + b":" + b"".join(AC.enc6(i) for i in range(n)) + b"}"
        t0 = time.perf_counter()
        m = ab.decompress_index(t, b"p" * 12)
        dt = time.perf_counter() - t0
        assert len(m) == n
        return dt
    run(1000)
    small, big = min(run(20000) for _ in range(3)), min(run(160000) for _ in range(3))
    assert big < 32 * small, (small, big)


def test_join_order():
    assert ab.join_order([3, 2]) == [1, 0]
    assert ab.join_order([2, 2, 1]) == [2, 0, 1]  # equal sizes: the lower count first
    assert ab.join_order([5]) == [0] and ab.join_order([]) == [] and ab.join_order([4, 0, 2]) == []
    # 2,147,483 * 1000 = 2,147,483,000 < 2^31; 2,147,484 * 1000 wraps to -2,147,483,296
    assert 2147483 * 1000 < 2 ** 31 <= 2147484 * 1000
    assert ab.join_order([2147483, 50]) == [1, 0]
    assert ab.join_order([2147484, 50]) == [0, 1]
    assert ab.join_order([50, 2147484]) == [1, 0]
    assert ab.join_order([4294968, 50]) == [0, 1]  # 4,294,968 * 1000 wraps past zero again: 704 < 50,001
    assert ab.join_order([4294968, 50, 1]) == [0, 2, 1]
    # join_constructive folds in that order: the first map's peer sets stay
    a, b = {b"u1": {b"pA"}, b"u2": {b"pA"}, b"u3": {b"pA"}}, {b"u1": {b"pB"}, b"u3": {b"pB"}}
    assert ab.SecondarySearch.join_constructive([a, b]) == {b"u1": {b"pB"}, b"u3": {b"pB"}}
    assert ab.SecondarySearch.join_constructive([b, a]) == {b"u1": {b"pB"}, b"u3": {b"pB"}}
    assert ab.SecondarySearch.join_constructive([a, {}]) == {}


# ------------------------------------------------------------------ compressIndex cases
def test_compress_cases_sizes_and_hosts():
    cases = {c.name: c for c in AC.compress_cases()}
    for n in AC.SIZES:
        for kind, hosts in (("one_host", 1), ("own_host", n)):
            c = cases["%s_%d" % (kind, n)]
            hs = AC.hashes(c.rows)
            assert len(hs) == n and hs == sorted(set(hs), key=AC.b64key)
            assert len({h[6:] for h in hs}) == hosts
            t = AC.compress_expected(c)
            assert len(t) == 8 * hosts + 6 * n + 1
            assert sorted(ab.decompress_index(t, b"p" * 12)) == sorted(hs)
    assert all(bytes(c.rows[0, 22:24]) == b"ee" and c.rows.shape[1] == 40 for c in cases.values())


def test_compress_case_host_order():
    c = next(c for c in AC.compress_cases() if c.name == "host_order")
    hosts = AC.host_order_hosts()
    assert len(set(hosts)) == 384
    for p in range(6):
        assert {h[p] for h in hosts} >= set(AC.B64)
    assert {h[:1] for h in hosts} >= {b"-", b"_", b"0", b"z"}
    assert sum(a[:5] == b[:5] and a != b for a in hosts for b in hosts) >= 64 * 63  # differ in the last byte only
    t = AC.compress_expected(c)
    in_text = [t[s:s + 6] for s in AC.segment_starts(t)]
    assert in_text == sorted(hosts)  # raw-byte order ...
    container = list(dict.fromkeys(h[6:] for h in AC.hashes(c.rows)))
    assert in_text != container and sorted(in_text) == sorted(container)  # ... which is not the container's
    assert in_text != sorted(hosts, key=AC.b64key)


def test_compress_cases_exclusion():
    cases = {c.name: c for c in AC.compress_cases()}
    base = AC.hashes(cases["ex_absent"].rows)
    p = b"p" * 12

    def left(name):
        c = cases[name]
        assert AC.hashes(c.rows) == base
        return c, sorted(ab.decompress_index(AC.compress_expected(c), p))

    assert left("ex_absent")[1] == sorted(base) and cases["ex_absent"].ex_rows is None
    assert AC.compress_expected(cases["ex_self"]) == b"{}"
    assert left("ex_all_but_first")[1] == [base[0]]
    assert left("ex_all_but_last")[1] == [base[-1]]
    c, rest = left("ex_one_host")
    gone = {h[6:] for h in AC.hashes(c.ex_rows)}
    assert len(gone) == 1 and len(c.ex_rows) >= 3
    assert rest == sorted(h for h in base if h[6:] not in gone)
    g_all = len(AC.segment_starts(AC.compress_expected(cases["ex_absent"])))
    assert len(AC.segment_starts(AC.compress_expected(c))) == g_all - 1 == 22
    assert left("ex_every_second")[1] == sorted(base[0::2])
    c, rest = left("ex_larger")
    ex = AC.hashes(c.ex_rows)
    assert len(ex) > len(base) and ex == sorted(set(ex), key=AC.b64key)
    assert AC.b64key(ex[0]) < AC.b64key(base[0]) and AC.b64key(ex[-1]) > AC.b64key(base[-1])
    assert rest == sorted(set(base) - set(base[::3])) and len(set(ex) - set(base)) > len(base)
    c = cases["ex_every_second_257"]
    assert len(c.rows) == 257 and len(ab.decompress_index(AC.compress_expected(c), p)) == 128


def test_multi_term_calls():
    lists, calls = AC.multi_term()
    assert calls[0][1].count(AC.MT1) == 2 and calls[1][1][-1] == AC.MT_ABSENT and AC.MT_ABSENT not in lists
    assert all(len(r) for r in lists.values())


# ------------------------------------------------------------------ decompressIndex / join cases
def test_alphabet_case_round_trips():
    urls = AC.alphabet_urls()
    assert len(set(urls)) == 768
    for p in range(12):
        assert {u[p] for u in urls} >= set(AC.B64)
    for p in (10, 11):  # pairs that differ in that character only
        assert sum(a[:p] == b[:p] and a[p + 1:] == b[p + 1:] and a != b for a in urls for b in urls) >= 64 * 63
    t = ab.compress_index(AC.row_list(AC.make_rows(urls)))
    assert sorted(ab.decompress_index(t, b"p" * 12)) == sorted(urls)
    assert ab.compress_index(AC.row_list(AC.make_rows(ab.decompress_index(t, b"p" * 12)))) == t
    join, words, plan = AC.expected(AC.alphabet_case())
    assert [u for u, _ in join] == sorted(set(urls[0::2]) | set(urls[0::5])) and len(words) == 2
    assert dict(join)[urls[10]] == AC.P(5) and dict(join)[urls[2]] == AC.P(4)  # the later abstract's peer
    assert {p for _, p in join} == {AC.P(4), AC.P(5)} and len(plan) == 2


def test_alignment_cases():
    body = AC.alignment_body()
    assert len(body) >= 12300 and body == AC.alignment_cases()[3].abstracts[1][2]
    runs = [(len(s) - 7) // 6 for s in body[1:-1].split(b",")]
    assert sorted(runs) == sorted(list(range(1, 41)) * 3)
    cases = AC.alignment_cases()
    assert [len(c.abstracts[0][2]) for c in cases] == list(range(17))
    starts = [s for c in cases for s in AC.alignment_starts(c)]
    assert {s % 16 for s in starts} == set(range(16))
    assert {s % 4096 for s in starts} >= {4095, 0, 1}
    # the prefixes contribute nothing, and every variant gives the one result
    assert all(ab.decompress_index(c.abstracts[0][2], b"p" * 12) == {} for c in cases)
    exp = [AC.expected(c) for c in cases]
    assert all(e == exp[0] for e in exp)
    join = exp[0][0]
    assert [u for u, _ in join] == sorted(ab.decompress_index(body, b"p" * 12)) and {p for _, p in join} == {AC.P(2)}
    assert len(join) == sum(runs)


def test_stop_cases():
    first, last = AC.stop_neighbours()
    for (name, mid, urls), case in zip(AC.STOPS, AC.stop_cases()):
        assert case.name == "stop_" + name and case.abstracts[1][2] == mid
        assert ab.decompress_index(mid, AC.P(2)) == {u: {AC.P(2)} for u in urls}, name
        join, words, plan = AC.expected(case)
        want = [(u, AC.P(1)) for u in first] + [(u, AC.P(2)) for u in urls] + [(u, AC.P(3)) for u in last]
        assert join == sorted(want), name  # the neighbours are whole
    listed = {"{}": [], "{": [], "}": [], "": [], "{host00:}": [], "{host00:,host01:BBBBBB}": [AC.B1],
              "{host00:AAAAAA,}": [AC.A0], "{,host00:AAAAAA}": [], "{host00:AAAAAA,,host01:BBBBBB}": [AC.A0],
              "{host00:AAAAAA,host01:BBBBB}": [AC.A0], "{host00:AAAAAA": [],
              "{host00:AAAAAA,host01xBBBBBB,host02:CCCCCC}": [AC.A0],
              "{host00:AAAAAA,host01xBBBBBB,host02:CCCCCCC}": [AC.A0],
              "{host00:AAAAAAAAAAAA}": [AC.A0], "{host00:AAAAAA,host00:AAAAAA}": [AC.A0]}
    have = {mid.decode(): urls for _, mid, urls in AC.STOPS}
    assert all(have[t] == u for t, u in listed.items())
    # the run of 7 behind the stop would be refused in front of it
    with pytest.raises(ValueError):
        ab.decompress_index(b"{host00:AAAAAA,host02:CCCCCCC}", AC.P(2))


def test_refusal_cases():
    cases = AC.refusal_cases()
    for c in cases[:-1]:
        with pytest.raises(ValueError):
            AC.expected(c)
    bad = {c.name: [i for i, (w, p, t) in enumerate(c.abstracts) if _raises(t)] for c in cases[:-1]}
    assert bad["refuse_run_of_7_first_abstract"] == [0] and bad["refuse_run_of_7_last_abstract"] == [2]
    assert all(len(v) == 1 for v in bad.values())
    assert len({w for w, _, _ in cases[-1].abstracts}) == 33 == cases[-1].nwords
    join, words, plan = AC.expected(AC.well_formed_case())
    assert len(join) == 9 + 3 + 2 + 7 + 4 and len(plan) == 3


def _raises(t):
    try:
        ab.decompress_index(t, b"p" * 12)
    except ValueError:
        return True
    return False


def test_add_abstract_cases():
    newest, twice = AC.add_abstract_cases()
    assert [p for _, p, _ in newest.abstracts] == [AC.P(3), AC.P(2), AC.P(1)]  # arrival against peer order
    assert _maps(newest)[AC.W(0)][AC.U(0)] == AC.P(1)
    assert dict(AC.expected(newest)[0])[AC.U(0)] == AC.P(1)
    m = _maps(twice)[AC.W(0)]
    assert [m[AC.U(i)] for i in range(12)] == [AC.P(1)] * 4 + [AC.P(2)] * 2 + [AC.P(1)] * 4 + [AC.P(2)] * 2


def test_fold_cases():
    def first_word(case):
        m = _maps(case)
        words = sorted(m)
        return words, ab.join_order([len(m[w]) for w in words])

    c = _case("fold_smallest_is_last_word")
    words, order = first_word(c)
    assert order[0] == 2 and words[2] == AC.W(2)
    join, _, plan = AC.expected(c)
    assert join == sorted([(AC.U(0), AC.P(3)), (AC.U(1), AC.P(3))]) and [p for p, _, _ in plan] == [AC.P(3)]
    assert plan[0][2] == [AC.W(2)] and len({p for _, p, _ in c.abstracts}) == 3

    c = _case("fold_equal_sizes")
    m = _maps(c)
    assert len(m[AC.W(0)]) == len(m[AC.W(1)]) and first_word(c)[1] == [0, 1]
    assert {p for _, p in AC.expected(c)[0]} == {AC.P(1)}

    join, words, plan = AC.expected(_case("fold_single_word"))
    assert words == [AC.W(5)] and len(join) == 6 and [u for u, _ in join] != sorted((u for u, _ in join), key=AC.b64key)

    c = _case("fold_32_words_bit_31")
    words, order = first_word(c)
    assert len(words) == 32 and order[0] == 31
    join, _, plan = AC.expected(c)
    assert join == [(AC.U(0), AC.P(2))] and plan == [(AC.P(2), [AC.U(0)], [AC.W(31)])]  # the mask is 1 << 31

    for name in ("fold_one_word_all_empty", "fold_all_texts_zero_length", "fold_disjoint_words"):
        join, words, plan = AC.expected(_case(name))
        assert join == [] and plan == [] and words == [AC.W(0), AC.W(1)], name
    assert _maps(_case("fold_one_word_all_empty")) == {AC.W(0): {AC.U(0): AC.P(1), AC.U(1): AC.P(1)}, AC.W(1): {}}
    assert all(len(m) for m in _maps(_case("fold_disjoint_words")).values())

    c = _case("fold_nwords_one_too_large")
    assert c.nwords == len(_maps(c)) + 1 and AC.expected(c)[0] == [] and AC.expected(c)[2] == []
    assert AC.expected(c._replace(nwords=3))[0] != []


def test_plan_cases():
    c = _case("plan_skip_mypeer_and_checked")
    join, _, plan = AC.expected(c)
    assert {p for _, p in join} == {AC.P(i) for i in range(1, 6)}
    assert [p for p, _, _ in plan] == [AC.P(1), AC.P(3), AC.P(5)] and c.mypeer == AC.P(2) and c.checked == (AC.P(4),)
    for n in AC.PEER_COUNTS:
        c = _case("plan_%d_peers" % n)
        join, _, plan = AC.expected(c)
        peers = [p for _, p, _ in c.abstracts]
        assert len(set(peers)) == n == len(plan) and len(join) == 2 * n
        assert [p for p, _, _ in plan] == sorted(peers) and (n < 3 or peers != sorted(peers))
        assert all(len(u) == 2 for _, u, _ in plan)
    join, _, plan = AC.expected(_case("plan_urls_in_string_order"))
    urls = plan[0][1]
    assert len(urls) == 128 and urls == sorted(urls) and urls != sorted(urls, key=AC.b64key)
    join, _, plan = AC.expected(_case("plan_peer_with_some_words"))
    assert join == sorted([(AC.U(1), AC.P(2)), (AC.U(2), AC.P(1))])
    assert plan == [(AC.P(1), [AC.U(2)], [AC.W(0), AC.W(1)]), (AC.P(2), [AC.U(1)], [AC.W(1)])]


def test_wrap_case():
    t0 = time.perf_counter()
    c = AC.wrap_case()
    built = time.perf_counter() - t0
    (wy, py, ty), (wx, px, tx) = c.abstracts
    n = AC.NWRAP
    assert len(tx) == 6 * n + 9 and tx[:8] == b"{wrapHS:" and tx[-1:] == b"}" and (wx, wy) == (AC.W(0), AC.W(1))
    assert tx[8:14] == AC.enc6(0) and tx[-7:-1] == AC.enc6(n - 1) and tx[8 + 6 * 4095:14 + 6 * 4095] == AC.enc6(4095)
    assert built < 5.0, built  # numpy builds the text; no per-url Python work
    y = ab.decompress_index(ty, py)
    inside, outside = AC.wrap_y_urls()
    assert len(y) == 50 and len(inside) == 30 and set(y) == set(inside) | set(outside)
    # the same shape at a size the oracle handles shows that wrap_expected is expected(): no wrap there,
    # Y folds first and the join carries Y's peer
    small = 2200
    assert AC.expected(AC.wrap_case(small)) == AC.wrap_expected(small)
    assert {p for _, p in AC.wrap_expected(small)[0]} == {py}
    join, words, plan = AC.wrap_expected()
    assert {p for _, p in join} == {px} and len(join) == 30 and plan == [(px, [u for u, _ in join], [wx])]
    assert ab.join_order([n - 1, 50]) == [1, 0] and ab.join_order([n, 50]) == [0, 1]
