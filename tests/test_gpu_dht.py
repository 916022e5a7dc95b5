"""The DHT send path on the device (yrwi_dht_select): the selected terms, the partition-major
offsets and every row byte equal the restatement (tests/dht_ref.py) whatever the window size and
wherever the rows land; the selection rules; removal and putting back; capacities and errors;
cost by windows, not by terms; url-hash shards."""

import ctypes

import numpy as np
import pytest

import dht_ref as dr
import index_util as iu
from yacy_search_server_amd import RWIIndex, _lib, synth

pytestmark = pytest.mark.gpu

NOW = iu.NOW
B64 = iu.B64
LAST = dr.LAST
BIG = (1 << 31) - 1
E_ARG, E_HASH = -1, -2
STAT_KEYS = ("terms", "postings", "skipped_private", "wrapped")


def _u(c0, c1, i):
    """a url hash whose first two characters have the alphabet indices c0, c1: partition
    c0 >> 2 at e = 4, c0 * 4 + (c1 >> 4) at e = 8"""
    return bytes([B64[c0], B64[c1]]) + iu.enc(i, 10)


def _private(i):
    return dr.PRIVATE + iu.enc(i, 10)


def _late(i):
    return b"_z" + iu.enc(i, 10)  # sorts after the private terms


def _spread(rng, n, lo, hi, base):
    """n distinct urls with first characters in [lo, hi), ascending"""
    c = rng.integers(lo, hi, n), rng.integers(0, 64, n)
    return sorted({_u(int(a), int(b), base + k) for k, (a, b) in enumerate(zip(*c))}, key=dr.key)


@pytest.fixture(scope="module")
def tiny():
    return synth.build_index(synth.preset("tiny"))


def _fixture_urls():
    rng = np.random.default_rng(72)
    L = {}
    # rows in all 16 partitions at e = 4, 1 .. 5 of them each
    L[iu.term(10)] = [_u(4 * p + k % 4, (11 * k) % 64, 100 * p + k) for p in range(16) for k in range(1 + (p * 7) % 5)]
    L[iu.term(20)] = [_u(k % 4, (5 * k) % 64, k) for k in range(33)]       # wholly in partition 0
    L[iu.term(30)] = [_u(60 + k % 4, (9 * k) % 64, k) for k in range(20)]  # wholly in partition 15
    L[iu.term(40)] = [_u(30, 7, 1)]                                        # one row
    # partition boundaries right after the first row and right before the last
    L[iu.term(50)] = [_u(8, 1, 0)] + [_u(20 + k % 4, k, k) for k in range(9)] + [_u(44, 2, 0)]
    # two urls that share their first character and differ at e = 8
    L[iu.term(60)] = [_u(20, 3, 0), _u(20, 40, 0), _u(33, 0, 0), _u(33, 63, 0), _u(50, 16, 0), _u(50, 17, 0)]
    # the middle one's single row in partition 3 is wedged between its neighbours' rows there
    L[iu.term(70)] = [_u(12 + k % 4, k, k) for k in range(5)]
    L[iu.term(80)] = [_u(13, 9, 0), _u(36, 0, 0), _u(37, 0, 0)]
    L[iu.term(90)] = [_u(12 + k % 4, 20 + k, k) for k in range(4)] + [_u(38, 5, 0), _u(39, 5, 0)]
    big = _spread(rng, 300, 0, 64, 1000)
    L[iu.term(100)] = big
    L[iu.term(110)] = sorted(set(big[::3]) | set(_spread(rng, 120, 0, 64, 5000)), key=dr.key)  # joins with it
    L[iu.term(120)] = _spread(rng, 150, 32, 64, 9000)
    L[_private(1)] = _spread(rng, 7, 0, 64, 20000)
    L[_private(2)] = _spread(rng, 12, 0, 64, 21000)
    L[_late(1)] = _spread(rng, 40, 0, 64, 30000)
    L[_late(2)] = _spread(rng, 9, 0, 64, 31000)
    for t, us in L.items():
        assert sorted(us, key=dr.key) == sorted(set(us), key=dr.key), t
    return {t: sorted(us, key=dr.key) for t, us in L.items()}


def _runs_of_empty(cnt):
    best = run = 0
    for c in cnt:
        run = run + 1 if c == 0 else 0
        best = max(best, run)
    return best


@pytest.fixture(scope="module")
def hand(tiny):
    """the hand-made index on the device, its lists, and the reference of the whole selection
    (rotated: from the middle of the term order) for every tested exponent"""
    urls = _fixture_urls()
    lists = {t: iu.rows(tiny, us, start=17 * i) for i, (t, us) in enumerate(urls.items())}
    assert 14 <= len(lists) <= 16 and sum(map(len, lists.values())) <= 1200
    e4 = {t: [dr.partition(u, 4) for u in us] for t, us in urls.items()}
    assert set(e4[iu.term(10)]) == set(range(16))
    assert set(e4[iu.term(20)]) == {0} and set(e4[iu.term(30)]) == {15} and len(urls[iu.term(40)]) == 1
    p50 = e4[iu.term(50)]
    assert p50[0] < p50[1] == p50[-2] < p50[-1]
    a, b = urls[iu.term(60)][:2]
    assert a[0] == b[0] and dr.partition(a, 8) != dr.partition(b, 8) and dr.partition(a, 6) == dr.partition(b, 6)
    assert sum(t[:2] == dr.PRIVATE for t in lists) == 2
    start = iu.term(45)
    ref = {e: dr.expected(lists, start, LAST, BIG, BIG, e) for e in (0, 1, 4, 6, 8)}
    # the edge cases, through the reference at e = 4
    terms, off, rows, st = ref[4]
    assert st["wrapped"] == 1 and st["skipped_private"] == 2 and len(terms) == len(lists) - 2
    cnt = np.diff(off)
    src = dr.source_starts(lists, terms, 4)
    assert {(int(src[c]) & 1, int(off[c]) & 1) for c in range(len(cnt)) if cnt[c]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert _runs_of_empty(cnt) >= 3
    assert any(cnt[c] == 1 and cnt[c - 1] > 0 and cnt[c + 1] > 0 and (c - 1) // len(terms) == (c + 1) // len(terms)
               for c in range(1, len(cnt) - 1))
    ix = iu.open_index(lists)
    yield ix, lists, start, ref
    ix.close()


def _window(monkeypatch, w):
    if w is None:
        monkeypatch.delenv("YRWI_DHT_WINDOW_ROWS", raising=False)
    else:
        monkeypatch.setenv("YRWI_DHT_WINDOW_ROWS", str(w))


def _same(sel, exp):
    terms, off, rows, st = exp
    assert sel.terms == terms
    assert sel.part_off.tolist() == off.tolist()
    assert sel.rows.shape == rows.shape and sel.rows.tobytes() == rows.tobytes()
    assert {k: sel.stats[k] for k in STAT_KEYS} == st, (sel.stats, st)
    assert sel.part_off[-1] == sel.stats["postings"] == len(rows)


def _unchanged(ix, lists):
    for t, r in lists.items():
        assert ix.get_list(t).tobytes() == r.tobytes(), t
    assert ix.stats()[:2] == (len(lists), sum(map(len, lists.values())))


# ------------------------------------------------------------------ 1: the image is exact
@pytest.mark.parametrize("pinned", [True, False])
def test_image_is_exact(hand, monkeypatch, pinned):
    ix, lists, start, ref = hand
    _window(monkeypatch, 64)  # several windows, cells and rows across their boundaries
    n = ref[4][3]["postings"]
    for e in (0, 1, 4, 6, 8):
        buf = ix.host_array(ctypes.c_uint8, 40 * n) if pinned else None
        sel = ix.dht_select(start, LAST, BIG, BIG, e, rows_out=buf)
        _same(sel, ref[e])
        assert sel.partitions == 1 << e and sel.stats["removed"] == 0
        T = len(sel.terms)
        for p in (0, (1 << e) - 1):
            for j in (0, T - 1):
                full = lists[sel.terms[j]]
                mask = np.array([dr.partition(r[:12].tobytes(), e) == p for r in full], dtype=bool)
                assert sel.cell(p, j).tobytes() == full[mask].tobytes()
    # a pageable buffer at an odd address lands through the pinned window
    if not pinned:
        raw = np.zeros(40 * n + 8, dtype=np.uint8)
        _same(ix.dht_select(start, LAST, BIG, BIG, 4, rows_out=raw[3:]), ref[4])
    _unchanged(ix, lists)


# ------------------------------------------------------------------ 2: window independence
def test_window_independence(hand, monkeypatch):
    ix, lists, start, ref = hand
    n = ref[4][3]["postings"]
    for w in (16, 17, 64, None):
        _window(monkeypatch, w)
        sel = ix.dht_select(start, LAST, BIG, BIG, 4)
        _same(sel, ref[4])
        assert sel.stats["windows"] == -(-n // (w or _lib.DHT_WINDOW_ROWS_DEFAULT)), (w, sel.stats)


# ------------------------------------------------------------------ 3: selection rules
def test_selection_rules(hand, monkeypatch):
    ix, lists, start, ref = hand
    _window(monkeypatch, None)
    order = sorted(lists, key=dr.key)
    public = [t for t in order if t[:2] != dr.PRIVATE]
    size = {t: len(r) for t, r in lists.items()}

    def run(*a, **kw):
        sel = ix.dht_select(*a, **kw)
        _same(sel, dr.expected(lists, a[0], a[1], a[2], a[3], a[4] if len(a) > 4 else 4, kw.get("rot", True),
                               kw.get("skip_private", True)))
        return sel

    # start between two terms
    assert run(iu.term(45), LAST, 3, BIG, 4).terms == [iu.term(50), iu.term(60), iu.term(70)]
    # start past the last term, with and without rot
    past = _late(3)
    sel = run(past, LAST, 2, BIG, 4)
    assert sel.terms == order[:2] and sel.stats["wrapped"] == 1
    sel = run(past, LAST, 2, BIG, 4, rot=False)
    assert sel.terms == [] and sel.part_off.tolist() == [0] and sel.stats["wrapped"] == 0
    # stop at limit; the first container is taken even when it is >= limit
    assert run(iu.term(30), iu.term(60), BIG, BIG, 4).terms == [iu.term(30), iu.term(40), iu.term(50)]
    assert run(iu.term(70), iu.term(60), BIG, BIG, 4).terms == [iu.term(70)]
    # after a wrap the comparison is still the plain one
    assert run(_late(2), iu.term(30), BIG, BIG, 4).terms == [_late(2), iu.term(10), iu.term(20)]
    # the max_containers cut, and max_refs overshot by the last container
    assert run(iu.term(10), LAST, 4, BIG, 4).terms == order[:4]
    cut = size[order[0]] + 1
    sel = run(iu.term(10), LAST, BIG, cut, 4)
    assert sel.terms == order[:2] and sel.stats["postings"] == size[order[0]] + size[order[1]] > cut
    # private terms are passed over without counting
    sel = run(iu.term(120), LAST, 3, BIG, 4, rot=False)
    assert sel.terms == [iu.term(120), _late(1), _late(2)] and sel.stats["skipped_private"] == 2
    sel = run(iu.term(120), LAST, 3, BIG, 4, rot=False, skip_private=False)
    assert sel.terms == [iu.term(120), _private(1), _private(2)] and sel.stats["skipped_private"] == 0
    # a full cycle: every non-private term once, in rotated order
    sel = run(iu.term(95), LAST, BIG, BIG, 4)
    k = public.index(iu.term(100))
    assert sel.terms == public[k:] + public[:k] and sel.stats["wrapped"] == 1
    assert sel.stats["postings"] == sum(size[t] for t in public)
    # nothing to select: an empty result, rc 0
    for mc, mr in ((0, BIG), (5, 0)):
        sel = run(iu.term(10), LAST, mc, mr, 4)
        assert sel.terms == [] and sel.part_off.tolist() == [0] and sel.rows.shape == (0, 40)
        assert sel.stats["windows"] == 0
    _unchanged(ix, lists)


# ------------------------------------------------------------------ 4: removal, and putting back
def test_remove_and_put_back(hand, tiny, monkeypatch):
    _, lists, _, _ = hand
    _window(monkeypatch, 64)
    ix = iu.open_index(lists)
    try:
        ix.build_url_ids()
        sel = ix.dht_select(iu.term(30), iu.term(100), BIG, BIG, 4, remove=True)
        _same(sel, dr.expected(lists, iu.term(30), iu.term(100), BIG, BIG, 4))
        gone = [iu.term(i) for i in (30, 40, 50, 60, 70, 80, 90)]
        assert sel.terms == gone
        assert sel.stats["removed"] == sel.stats["postings"] == sum(len(lists[t]) for t in gone)
        left = dr.after_removal(lists, gone)
        for t in gone:
            assert ix.get_size(t) == 0 and ix.get_list(t).shape == (0, 40)
        _unchanged(ix, left)
        assert ix.check_url_ids()[0] == 0
        qs = [([iu.term(100), iu.term(110)], []), ([iu.term(110), iu.term(120)], [iu.term(100)])]
        got = iu.hits(ix, qs)
        assert got == iu.oracle_hits(left, qs) and len(got[0]) > 0
        # what could not be sent goes back: term j for every row of its cells
        T = len(sel.terms)
        per_row = [sel.terms[c % T] for c in range(len(sel.part_off) - 1)
                   for _ in range(sel.part_off[c + 1] - sel.part_off[c])]
        st = ix.add_postings(per_row, sel.rows, policy="keep")
        assert (st["added"], st["new_terms"]) == (sel.stats["postings"], T)
        _unchanged(ix, lists)
        assert ix.check_url_ids()[0] == 0
    finally:
        ix.close()


# ------------------------------------------------------------------ 5: capacities and errors
def test_capacity_and_errors(hand, monkeypatch):
    ix, lists, start, ref = hand
    _window(monkeypatch, 64)
    terms, off, rows, st = ref[4]
    T, n = len(terms), len(rows)
    ROT_SKIP = _lib.DHT_ROT | _lib.DHT_SKIP_PRIVATE

    def bufs():
        return (np.full((T + 1, 12), 0xAB, np.uint8), np.full(16 * (T + 1) + 1, -7, np.int64),
                np.full((n + 1, 40), 0xCD, np.uint8))

    def untouched(b):
        return (b[0] == 0xAB).all() and (b[1] == -7).all() and (b[2] == 0xCD).all()

    # one row, one term short, REMOVE set: the needed sizes, nothing written, nothing removed
    for ct, cr in ((T, n - 1), (T - 1, n)):
        b = bufs()
        rc, s = ix.dht_select_raw(start, LAST, BIG, BIG, 4, ROT_SKIP | _lib.DHT_REMOVE, b[0], ct, b[1], b[2], cr)
        assert rc == E_ARG and (s["terms"], s["postings"], s["removed"]) == (T, n, 0)
        assert untouched(b)
        _unchanged(ix, lists)
    # a bad hash, an exponent out of range, an unknown flag
    for args, want in (((b"bad!hash#xyz", LAST, BIG, BIG, 4, ROT_SKIP), E_HASH),
                       ((start, b"bad!hash#xyz", BIG, BIG, 4, ROT_SKIP), E_HASH),
                       ((start, LAST, BIG, BIG, -1, ROT_SKIP), E_ARG), ((start, LAST, BIG, BIG, 9, ROT_SKIP), E_ARG),
                       ((start, LAST, BIG, BIG, 4, ROT_SKIP | 16), E_ARG)):
        b = bufs()
        rc, s = ix.dht_select_raw(*args, b[0], T, b[1], b[2], n)
        assert rc == want, (args, rc)
        assert untouched(b)
    _unchanged(ix, lists)
    # the dry run says what the real call selects; it writes no buffer and changes nothing
    b = bufs()
    rc, dry = ix.dht_select_raw(start, LAST, BIG, BIG, 4, ROT_SKIP | _lib.DHT_REMOVE | _lib.DHT_COUNT_ONLY,
                                b[0], T, b[1], b[2], n)
    assert rc == 0 and untouched(b) and (dry["removed"], dry["windows"]) == (0, 0)
    rc, dry0 = ix.dht_select_raw(start, LAST, BIG, BIG, 4, ROT_SKIP | _lib.DHT_COUNT_ONLY, None, 0, None, None, 0)
    assert rc == 0 and {k: dry0[k] for k in STAT_KEYS} == {k: dry[k] for k in STAT_KEYS} == st
    _unchanged(ix, lists)
    rc, real = ix.dht_select_raw(start, LAST, BIG, BIG, 4, ROT_SKIP, b[0], T, b[1], b[2], n)
    assert rc == 0 and {k: real[k] for k in STAT_KEYS} == st
    assert [b[0][j].tobytes() for j in range(T)] == terms and (b[0][T] == 0xAB).all()
    assert b[1][:16 * T + 1].tolist() == off.tolist() and (b[1][16 * T + 1:] == -7).all()
    assert b[2][:n].tobytes() == rows.tobytes() and (b[2][n] == 0xCD).all()
    sel = ix.dht_select(start, LAST, BIG, BIG, 4, count_only=True)
    assert {k: sel.stats[k] for k in STAT_KEYS} == st and sel.rows.shape == (0, 40)


# ------------------------------------------------------------------ 6: cost does not follow the term count
def test_cost_does_not_follow_term_count(tiny, monkeypatch):
    _window(monkeypatch, 64)
    one = {iu.term(1): iu.rows(tiny, sorted((_u(k % 64, (7 * k) % 64, k) for k in range(1000)), key=dr.key))}
    many = {iu.term(100 + i): iu.rows(tiny, sorted((_u((i + 16 * k) % 64, i % 64, i) for k in range(4)), key=dr.key),
                                        start=i) for i in range(250)}
    lists = {**one, **many}
    ix = iu.open_index(lists)
    try:
        a = ix.dht_select(iu.term(1), iu.term(2), BIG, BIG, 4)
        b = ix.dht_select(iu.term(100), LAST, BIG, BIG, 4, rot=False)
        _same(a, dr.expected(lists, iu.term(1), iu.term(2), BIG, BIG, 4))
        _same(b, dr.expected(lists, iu.term(100), LAST, BIG, BIG, 4, rot=False))
        assert (len(a.terms), len(b.terms)) == (1, 250) and a.stats["postings"] == b.stats["postings"] == 1000
        assert a.stats["windows"] == b.stats["windows"] == 16
        assert (a.stats["launches"], a.stats["syncs"]) == (b.stats["launches"], b.stats["syncs"]), (a.stats, b.stats)
    finally:
        ix.close()


# ------------------------------------------------------------------ 7: url-hash shards
def test_shards_loopback(hand, monkeypatch):
    _, lists, _, _ = hand
    _window(monkeypatch, 64)
    world = 2
    half = {t: np.array([dr.partition(r[:12].tobytes(), 1) for r in rows]) for t, rows in lists.items()}
    both = {t: rows for t, rows in lists.items() if set(half[t]) == {0, 1} and t[:2] != dr.PRIVATE}
    assert len(both) >= 5
    parts = [{t: rows[half[t] == r] for t, rows in both.items()} for r in range(world)]
    first = min(both, key=dr.key)

    def fn(r, ix):
        sel = ix.dht_select(first, LAST, BIG, BIG, 4)
        return sel.terms, sel.part_off, sel.rows.copy(), sel.stats

    res = iu.run_parts(parts, world, fn)
    whole = iu.open_index(both)
    try:
        ref = whole.dht_select(first, LAST, BIG, BIG, 4)
    finally:
        whole.close()
    _same(ref, dr.expected(both, first, LAST, BIG, BIG, 4))
    T = len(ref.terms)
    for r in range(world):
        terms, off, rows, st = res[r]
        assert terms == ref.terms
        _same(type(ref)(terms, off, rows, 16, st), dr.expected(parts[r], first, LAST, BIG, BIG, 4))
        cnt = np.diff(off).reshape(16, T)
        assert not cnt[:8].any() if r == 1 else not cnt[8:].any()
    for p in range(16):
        for j in range(T):
            c = p * T + j
            got = b"".join(res[r][2][res[r][1][c]:res[r][1][c + 1]].tobytes() for r in range(world))
            assert got == ref.cell(p, j).tobytes(), (p, j)
