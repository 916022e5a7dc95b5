"""GPU parity (MI355X) on adversarial rows: libyrwi's rank path against the C++
oracle (java_literal where only it has the operation), bit-exact, on value
ranges no synthetic corpus reaches -- tests/adv_rows.py; tests/test_adv_oracle.py
licenses the oracle on these rows.

What the sizes reach (yrwi_kernels.hip, yrwi_internal.h):
  normalize_score        k_score_all: cardinal() without term tables, any n
  search, k > 256        k_score only counts flags and hands every chunk to k_score_full
                         (SCORE_SMALL = 256), which builds a CardTab of its own in LDS for
                         every chunk, whatever n is, and scores every posting through it
  search, k <= 256       k_score scores the chunk itself: a chunk of at most 512 postings
                         (YRWI_CARD_TAB_MIN) without tables, a longer one through the
                         CardTab that k_qtabs built for a query of more than 512 postings
                         and copy_card_tab brought into LDS; only here are the published
                         threshold, score_bound and prune_chunk at work (n > 2048)
  joins with > 64 tiles  several 64-piece groups of k_piece_merge, folded by k_shard_fin
So the table tests run every container at k = 3000 (every row comes back: build_card_tab's
arithmetic entry by entry, in k_score_full) and at k = 256 and 100 (the top of the same
ranking: k_qtabs -> copy_card_tab -> k_score, and k_score without tables at 512 rows)."""

import numpy as np
import pytest

import index_util as iu
import java_literal as jl
import oracle as orc
import query_util as qu
from adv_rows import (CONST_COLS, adv_profiles, adv_rows, col_values, distance_fold_rows, flag_profiles,
                      flag_walk_rows, hashcodes, palette_profile, shard_of, single, sort_rows, span_rows,
                      universe_lists)
from event_local_cases import check_event
from yacy_search_server_amd import Query, QueryFilter, RankingProfile, RWIIndex
from yacy_search_server_amd._lib import CStats

pytestmark = pytest.mark.gpu

DAY = 86400000
NOW = 20741 * DAY + 4242
NOWS = [NOW, 15500 * DAY + 7, 70000 * DAY + 1]  # day 15500: most dates in the future; day 70000: none
INF = 2147483647
MODES = ["edge", "few"] + ["const:" + c for c in CONST_COLS]
HIT = qu.HIT


def _rp(jlprof):
    rp = RankingProfile()
    for _, f in jl.PROFILE_FIELDS:
        setattr(rp, f, getattr(jlprof, f))
    return rp


def _same_scores(got, exp, ctx):
    if np.array_equal(got, exp):
        return
    i = int(np.flatnonzero(got != exp)[0])
    assert False, (ctx, "row", i, "gpu", int(got[i]), "oracle", int(exp[i]), int((got != exp).sum()), "rows differ")


KS = (3000, 256, 100)  # k_score_full; k_score at its largest k; k_score at the usual k


def _check_lists(ix, d, rp, op, lang, now, ctx):
    """Every list of d as a one-term query, one batch per k of KS, against the oracle's
    ranking of the whole list (its first k entries are the oracle's top-k)."""
    exp = {h: qu.orc_raw(d, [h], [], op, lang, now, 3000) for h in d}
    for k in KS:
        got = qu.gpu_raw(ix, [Query([h], [], k=k, profile=rp, language=lang, now_ms=now) for h in d])
        for h, g in zip(d, got):
            qu.same_hits(g, exp[h][:k * HIT], (h, k) + tuple(ctx))


@pytest.fixture(scope="module")
def ctx():
    ix = RWIIndex(0)
    yield ix
    ix.close()


def _schedule(ci):
    """(name, profile, language, now) runs of one container: default, c5, /date and the
    three palettes at every `now`, the single-field profiles at a rotating one."""
    out = []
    for pi, (name, prof) in enumerate(adv_profiles()):
        if not name.startswith("single"):
            out += [(name, prof, ("en", "zz")[(pi + ci + ni) % 2], now) for ni, now in enumerate(NOWS)]
        else:
            out.append((name, prof, ("en", "zz")[(pi + ci) % 2], NOWS[(pi + ci) % 3]))
    return out


# ------------------------------------------------------------------ a
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 2048, 2049, 4500])
def test_all_scores_direct(ctx, n):
    """cardinal() of every row without term tables (k_score_all), one wave, two waves,
    one chunk, one posting more, three chunks; every mode, profile, language, now."""
    for ci, mode in enumerate(MODES):
        rows = adv_rows(n, 20 + ci, mode)
        for name, prof, lang, now in _schedule(ci):
            exp, _ = orc.normalize_score(rows, orc.profile_from(prof), lang, now)
            got = ctx.normalize_score(rows, _rp(prof), lang, now)
            _same_scores(got, exp, (n, mode, name, lang, now))


# ------------------------------------------------------------------ b
@pytest.mark.parametrize("sizes", [(512, 513), (2047, 3000)])
def test_all_scores_through_tables(sizes):
    """The same containers through search.  k = 3000 returns every row, all scored by
    k_score_full through the CardTab it builds per chunk.  k = 256 and k = 100 are
    scored by k_score: at 512 rows it computes the terms, from 513 on every one-byte
    term and the flag subsets come from the CardTab k_qtabs built.  One batch holds a
    query per container, so k_qtabs builds tables for some queries (513) and not
    for others (512), and k_score must read them for exactly those."""
    d = {}
    for ci, mode in enumerate(MODES):
        for n in sizes:
            d[b"TERM%04d%02d__" % (n, ci)] = adv_rows(n, 20 + ci, mode)
    ix = RWIIndex(0)
    try:
        for h, r in d.items():
            ix.add(h, r)
        for name, prof, lang, now in _schedule(0):
            _check_lists(ix, d, _rp(prof), orc.profile_from(prof), lang, now, (name, lang, now))
    finally:
        ix.close()


# ------------------------------------------------------------------ c
BYTE_FIELDS = [("u", "wordsintitle"), ("x", "llocal"), ("y", "lother"), ("m", "urllength"), ("n", "urlcomps"),
               ("c", "hitcount"), ("r", "posinphrase"), ("o", "posofphrase")]


def _byte_spans():
    return [(lo, d) for d in range(1, 256) for lo in ([0, 255 - d] if d % 2 else [0])]


def test_division_exhaustive_byte_fields_direct(ctx):
    """Every (numerator, divisor) pair a one-byte min/max field can produce: for each
    span d = 1..255 a container whose one-byte cells take every value lo..lo + d
    (lo = 0; lo = 255 - d for odd d), scored under single(f, 15) for each field.  The
    min/max fold has eight one-byte fields; the ninth one-byte term of CardTab, the
    distance, has the fold's D as divisor: test_division_distance_fold."""
    profs = [(f, _rp(single(f, 15)), orc.profile_from(single(f, 15))) for _, f in BYTE_FIELDS]
    cols = "".join(c for c, _ in BYTE_FIELDS)
    for lo, d in _byte_spans():
        rows = span_rows(cols, lo, d)
        assert all(set(col_values(rows, c)) == set(range(lo, lo + d + 1)) for c in cols)
        for f, rp, op in profs:
            exp, _ = orc.normalize_score(rows, op, "en", NOW)
            _same_scores(ctx.normalize_score(rows, rp, "en", NOW), exp, (lo, d, f))


def test_division_exhaustive_byte_fields_tables():
    """The same spans padded to 513 rows, through search: at k = 3000 every entry of
    the eight min/max term tables for every divisor, as k_score_full builds them; at
    k = 256 and 100 the best rows of each span through the tables k_qtabs built and
    k_score copied (383 containers in one batch: every query's own QTab)."""
    cols = "".join(c for c, _ in BYTE_FIELDS)
    d = {b"TERMsp%03d%03d" % (lo, dd): span_rows(cols, lo, dd, pad_to=513) for lo, dd in _byte_spans()}
    ix = RWIIndex(0)
    try:
        for h, r in d.items():
            ix.add(h, r)
        for _, f in BYTE_FIELDS:
            _check_lists(ix, d, _rp(single(f, 15)), orc.profile_from(single(f, 15)), "en", NOW, (f,))
    finally:
        ix.close()


def test_division_distance_fold(ctx):
    """The distance term's divisor is the fold's D: containers of 2, 3 and 300 rows
    whose fold ends at D in {1, 2, 3, 127, 254, 255, 256, 65534}, stored distances
    over 0..255 (above D: the negative term, at D = 1 and coefficient 15 next to the
    int range's end); direct, and padded to 600 rows through the distance table of
    k_score_full (k = 3000) and of k_qtabs / k_score (k = 256, 100)."""
    want = {1, 2, 3, 127, 254, 255, 256, 65534}
    seen = set()
    d = {}
    for D in sorted(want):
        for n in (2, 3, 300):
            if n == 2 and D > 255:
                continue
            rows = distance_fold_rows(D, n)
            for c in (15, 7, 0):
                exp, nm = orc.normalize_score(rows, orc.profile_from(single("worddistance", c)), "en", NOW)
                assert nm.max_distance_D == D
                _same_scores(ctx.normalize_score(rows, _rp(single("worddistance", c)), "en", NOW), exp, (D, n, c))
            seen.add(D)
            if n == 300:
                assert (col_values(rows, "i") > D).any() or D >= 255
                d[b"TERMdf%06d" % D] = distance_fold_rows(D, n, pad_to=600)
    assert seen == want
    ix = RWIIndex(0)
    try:
        for h, r in d.items():
            ix.add(h, r)
        for name, prof in [("wd15", single("worddistance", 15)), ("wd7", single("worddistance", 7)),
                           ("default", jl.RankingProfile())]:
            op = orc.profile_from(prof)
            for h in d:
                _, nm = orc.normalize_score(d[h], op, "en", NOW)
                assert nm.max_distance_D == int(h[6:])
            _check_lists(ix, d, _rp(prof), op, "en", NOW, (name,))
    finally:
        ix.close()


# ------------------------------------------------------------------ d
SPANS16 = [1, 2, 3, 5, 7, 255, 256, 257, 511, 513, 4095, 4097, 21845, 32767, 32768, 32769, 43691, 65521, 65534,
           65535]


@pytest.mark.parametrize("col,field", [("t", "posintext"), ("w", "wordsintext"), ("p", "phrasesintext"),
                                       ("a", "date")])
def test_division_16bit_spans(ctx, col, field):
    """qdiv on the two-byte fields: every value of a span of d + 1 values, d up to
    65535, so every numerator (v << 8) meets the divisor d -- the exact quotients
    (v = 0, v = d, and the multiples of d / gcd(d, 256) between) with the values next
    to them.  Dates at now = day 70000 (no date is clamped), plus containers whose
    first row is the only one in the future: the clone is clamped to today, later
    rows lift the maximum again, and the first row's own date lies above it."""
    now = NOWS[2] if col == "a" else NOW
    profs = [(c, _rp(single(field, c)), orc.profile_from(single(field, c))) for c in (15, 7)]
    for d in SPANS16:
        for lo in sorted({0, 65535 - d, (65535 - d) // 2}):
            rows = span_rows(col, lo, d)
            v = col_values(rows, col) - lo
            assert np.array_equal(np.sort(v), np.arange(d + 1))  # every numerator v << 8, v = 0..d
            exact = np.flatnonzero((np.arange(d + 1) << 8) % d == 0)  # with v - 1 and v + 1 in the span too
            assert {0, d} <= set(exact.tolist()) and len(exact) == 1 + np.gcd(d, 256)
            for c, rp, op in profs[:2 if d < 1000 or lo == 0 else 1]:
                exp, _ = orc.normalize_score(rows, op, "en", now)
                _same_scores(ctx.normalize_score(rows, rp, "en", now), exp, (col, lo, d, c))
    if col == "a":
        for d in (2, 255, 256, 4097, 32768):
            lo = 20000
            rows = span_rows(col, lo, d)
            rows[:, 12:] = rows[::-1, 12:].copy()  # the largest date first
            today = lo + d // 2
            for c, rp, op in profs:
                exp, nm = orc.normalize_score(rows, op, "en", today * DAY + 5)
                _same_scores(ctx.normalize_score(rows, rp, "en", today * DAY + 5), exp, ("future first", d, c))


# ------------------------------------------------------------------ e
K_RANGES = ((2, 12), (13, 128), (129, 256), (257, 2048), (2049, 3000))  # k_score prunes up to 256


def _tie_cuts(rows, op, lang, now):
    """k values (2..12, 13..128, 129..256, 257..2048, > 2048) at which the k-th and the
    (k+1)-th distinct (score, hashCode) class of the reference have the same score."""
    sc, _ = orc.normalize_score(rows, op, lang, now)
    cls = np.unique(np.stack([sc, hashcodes(rows)], axis=1), axis=0)[::-1]  # best class first
    tie = np.flatnonzero(cls[:-1, 0] == cls[1:, 0]) + 1                   # k: class k and k + 1 tie
    ks = []
    for lo, hi in K_RANGES:
        t = tie[(tie >= lo) & (tie <= hi)]
        if len(t):
            ks.append(int(t[len(t) // 2]))
    return sc, ks


def _prune_profiles():
    date = single("date", 15)
    return [("default", jl.RankingProfile()),
            ("c5", jl.RankingProfile.parse("", "date=15,domlength=15,authority=13,tf=10")), ("date", date),
            ("tf", single("termfrequency", 15)),                # the score is the long-accumulated tf term
            ("low", palette_profile((0, 1, 7, 15), 104)),       # every bound valid
            ("wrap", palette_profile((23, 24, 27, 31), 105))]   # terms can wrap: PruneP.ok == 0


@pytest.mark.parametrize("mode", ["few", "edge", "tight"])
@pytest.mark.parametrize("n", [6200, 10300, 18500])
def test_pruning_with_ties_at_k(n, mode):
    """Containers of 3, 5 and 9 chunks; k cut through a run of equal scores, so the
    published threshold equals the k-th score and `bound < T` must stay strict.  The
    best rows last in url order (early chunks publish a low threshold, late ones
    raise it) and first; each query alone and in a batch of 8 copies (threshold
    publication under contention).  In mode "tight" score_bound equals the score, so
    the rows that tie with the threshold are the ones whose bound equals it.

    k_score reads the threshold when a chunk's workgroup starts, and one launch holds
    every chunk of the batch, chunk 0 of every query first: a query's later chunks
    see a threshold only when the batch has more chunks than the device runs at once.
    So the cuts of at most 256 (k_score prunes up to SCORE_SMALL = 256) also run as
    2048 copies in one batch, 6,144 to 18,432 chunks."""
    base = adv_rows(n, 50 + n % 7, mode)
    d, cases, dropped = {}, [], 0
    for pi, (name, prof) in enumerate(_prune_profiles()):
        op = orc.profile_from(prof)
        sc, _ = orc.normalize_score(base, op, "en", NOW)
        for oi, order in enumerate((np.argsort(sc, kind="stable"), np.argsort(-sc, kind="stable"))):
            rows = base.copy()
            rows[:, 12:] = base[order, 12:]  # features re-dealt along the url order by their score
            sc2, ks = _tie_cuts(rows, op, "en", NOW)
            if not ks:
                dropped += 1
                continue
            # precondition, from the reference alone: the cut at each k goes through a tie run
            cls = np.unique(np.stack([sc2, hashcodes(rows)], axis=1), axis=0)[::-1]
            assert all(cls[k - 1, 0] == cls[k, 0] for k in ks)
            h = b"TERMpr%02d%02d__" % (pi, oi)
            d[h] = rows
            cases.append((h, name, prof, ks))
    assert dropped * 4 <= 12, dropped
    allk = [k for _, _, _, ks in cases for k in ks]

    for lo, hi in K_RANGES:  # every range has a cut, and some container has one in each
        assert any(lo <= k <= hi for k in allk), (lo, hi)
    assert any(len(ks) == len(K_RANGES) for _, _, _, ks in cases)
    ix = RWIIndex(0)
    try:
        for h, r in d.items():
            ix.add(h, r)
        for h, name, prof, ks in cases:
            rp, op = _rp(prof), orc.profile_from(prof)
            exp = [qu.orc_raw(d, [h], [], op, "en", NOW, k) for k in ks]
            got = qu.gpu_raw(ix, [Query([h], [], k=k, profile=rp, now_ms=NOW) for k in ks])
            for k, g, e in zip(ks, got, exp):
                qu.same_hits(g, e, (h, name, k, "alone"))
            got = qu.gpu_raw(ix, [Query([h], [], k=k, profile=rp, now_ms=NOW) for k in ks for _ in range(8)])
            for j, g in enumerate(got):
                qu.same_hits(g, exp[j // 8], (h, name, ks[j // 8], "copy", j % 8))
            small = [j for j, k in enumerate(ks) if k <= 256]
            if not small:
                continue
            got = qu.gpu_raw(ix, [Query([h], [], k=ks[small[c % len(small)]], profile=rp, now_ms=NOW)
                                for c in range(2048)])
            for c, g in enumerate(got):
                j = small[c % len(small)]
                qu.same_hits(g, exp[j], (h, name, ks[j], "of 2048 copies", c))
    finally:
        ix.close()


LADDER = ((700, 100), (4000, 100), (8200, 3000), (16500, 3000))  # (rows, k): 1, 2, 5 and 9 chunks of 2048


def test_topk_pass_ladder():
    """The top-k passes over the chunks' candidate lists (run_rank_phase, yrwi_rank.cpp), one
    batch of single-term queries whose lists take different numbers of passes:
      a missing term       no chunk: the count is the pass's zero word
      700 rows, k = 100    one chunk: final as k_score left it, never in a pass
      4000 rows, k = 100   two chunks, merged in pass 1; it sits out the later passes, so its
                           final list stays pass 1's output while the others' inputs move on
      8200 rows, k = 3000  five chunks: 5 -> 2 -> 1 lists
      16500 rows, k = 3000 nine chunks: 9 -> 3 -> 2 -> 1 lists
    The batch's largest k is 3000: chunk lists of stride 2048, 8192 candidates per group, so
    pass 1 merges 4 lists a group and the later passes (stride 3000) 2.  Rows of few values:
    ties cross the list boundaries.  The batch in this order and reversed (other group bases),
    through search_batch and through the call that returns the hits' rows."""
    assert [-(-n // 2048) for n, _ in LADDER] == [1, 2, 5, 9]
    d = {b"TERMladder%d_" % i: adv_rows(n, 80 + i, "few") for i, (n, _) in enumerate(LADDER)}
    assert [len(r) for r in d.values()] == [n for n, _ in LADDER]
    prof = jl.RankingProfile()
    rp, op = _rp(prof), orc.profile_from(prof)
    cases = [(b"TERMladderNO", 100, b"", [])]
    for (h, rows), (_, k) in zip(d.items(), LADDER):
        exp = qu.orc_raw(d, [h], [], op, "en", NOW, k)
        assert len(exp) == k * HIT  # precondition, from the reference alone: every list fills its k
        cases.append((h, k, exp, orc.term_search(d, [h], [], INF, NOW)))
    ix = RWIIndex(0)
    try:
        for h, rows in d.items():
            ix.add(h, rows)
        for order in (cases, cases[::-1]):
            batch = [Query([h], [], k=k, profile=rp, now_ms=NOW) for h, k, _, _ in order]
            for (h, k, exp, _), g in zip(order, qu.gpu_raw(ix, batch)):
                qu.same_hits(g, exp, (h, k, order is cases))
            for (h, k, exp, joined), g in zip(order, ix.search_batch(batch, rows=True)):
                qu.same_rows(g, qu.decode(exp), joined, (h, k, order is cases, "rows"))
    finally:
        ix.close()


# ------------------------------------------------------------------ f
def test_flag_bits_outside_tables():
    """Flag words of one bit each (0..31), all ones and none, 600 rows (CardTab path, in
    k_score_full at k = 3000 and in k_score at k = 256 and 100):
    bits 20-23 and 24-29 index the two subset tables, bit 0 is added apart, every
    other bit must change nothing.  Query languages that are no two-letter code.
    The same rows through a QueryFilter: all 32 flag counts."""
    rows = flag_walk_rows(600, 4)
    T = b"TERMflags___"
    d = {T: rows}
    ix = RWIIndex(0)
    try:
        ix.add(T, rows)
        for name, prof in flag_profiles() + [("high", palette_profile((15, 16, 22, 23, 24, 31), 102))]:
            rp, op = _rp(prof), orc.profile_from(prof)
            for lang in ("en", "e", "", "eng"):
                _check_lists(ix, d, rp, op, lang, NOW, (name, lang))
                exp, _ = orc.normalize_score(rows, op, lang, NOW)
                _same_scores(ix.normalize_score(rows, rp, lang, NOW), exp, (name, lang))
        lit = {T: [bytes(r) for r in rows]}
        for kw in (dict(), dict(constraint=b"\0\0\x10\x01"), dict(constraint=b"\x01\0\0\x80", all_of_constraint=True)):
            gf, lf = QueryFilter(**kw), jl.QueryFilter(**kw)
            got = ix.search([T], [], now_ms=NOW, k=3000, filter=gf)
            exp = jl.search(lit, [T], [], jl.RankingProfile(), "en", now_ms=NOW, k=3000, filt=lf)
            assert [(h.urlhash, h.score) for h in got] == exp, kw
            assert gf.flagcount == lf.flagcount, kw
            assert all(c >= 600 // 34 for c in lf.flagcount)
    finally:
        ix.close()


# ------------------------------------------------------------------ g
@pytest.fixture(scope="module")
def join_lists():
    d = universe_lists(7, 3000)
    A, B = list(d)[:2]
    a, b = d[A], d[B]
    hb = {bytes(x) for x in b[:, :12]}
    both = a[[bytes(x) in hb for x in a[:, :12]]]
    ha = {bytes(x) for x in both[:, :12]}
    bb = b[[bytes(x) in ha for x in b[:, :12]]]
    pa, pb = col_values(both, "t"), col_values(bb, "t")
    # J5's corners are present among the joined pairs (from the generated rows alone)
    assert ((pa == 0) & (pb > 0)).any() and ((pb == 0) & (pa > 0)).any() and ((pa == 0) & (pb == 0)).any()
    assert ((pa == 65535) & (pb == 65535)).any()
    assert (col_values(both, "o") == col_values(bb, "o")).any()
    assert (np.maximum(col_values(both, "c"), col_values(bb, "c")) == 255).any()
    assert (np.maximum(col_values(both, "u"), col_values(bb, "u")) == 255).any()
    return d


@pytest.mark.parametrize("chain", ["chained", "stepwise"])
@pytest.mark.parametrize("algo", ["probe", "merge"])
def test_adversarial_joins(join_lists, algo, chain, monkeypatch):
    """joinConstructive (J5) on packed cells at their extremes over one universe of
    3000 urls: posintext 0 on either side or both, both 65535, equal posofphrase,
    hitcount / wordsintitle at 255, joined distances cut to one byte; rows at
    max_distance inf / 300 / 1 and the top-k, probe and merge tiles, chained and
    stepwise folds."""
    monkeypatch.setenv("YRWI_PROBE_RATIO", "1" if algo == "probe" else "1000000000")
    monkeypatch.setenv("YRWI_NO_CHAIN", "1" if chain == "stepwise" else "0")
    d = join_lists
    A, B, C, D = d
    qs = [([A, B], []), ([B, C], []), ([A, B, C], []), ([A, B, C, D], []), ([A, B], [D]), ([C, B, A], [D])]
    profs = adv_profiles(singles=False) + [("near", single("worddistance", 15)), ("tf", single("termfrequency", 15)),
                                          ("posinphrase", single("posinphrase", 15))]
    ix = RWIIndex(0)
    try:
        for h, r in d.items():
            ix.add(h, r)
        for qi, (inc, exc) in enumerate(qs):
            for md in (INF, 300, 1):
                for now in NOWS[:2]:
                    exp = orc.term_search(d, inc, exc, md, now)
                    got = ix.term_search(inc, exc, md, now)
                    assert got.shape == exp.shape and np.array_equal(got, exp), (qi, md, now)
        for pi, (name, prof) in enumerate(profs):
            rp, op = _rp(prof), orc.profile_from(prof)
            for md in (INF, 300):
                now = NOWS[(pi + (md == 300)) % 3]
                got = qu.gpu_raw(ix, [Query(inc, exc, max_distance=md, k=3000, profile=rp, now_ms=now)
                                    for inc, exc in qs])
                for qi, ((inc, exc), g) in enumerate(zip(qs, got)):
                    qu.same_hits(g, qu.orc_raw(d, inc, exc, op, "en", now, 3000, md), (qi, name, md, now))
    finally:
        ix.close()


# ------------------------------------------------------------------ h
def _keyed(keys, seed, pmode):
    """Valid rows for ascending integer keys (vectorised); posintext by pmode."""
    rng = np.random.default_rng(seed)
    n = len(keys)
    rows = np.zeros((n, 40), dtype=np.uint8)
    alpha = np.frombuffer(jl.ALPHA, dtype=np.uint8)
    k = keys.astype(np.int64) * 977 + 13
    for j in range(12):
        rows[:, 11 - j] = alpha[(k >> (6 * j)) & 63]
    rows[:, 12:14] = np.frombuffer((15000).to_bytes(2, "big"), dtype=np.uint8)
    rows[:, 18] = 50
    rows[:, 21] = ord("t")
    rows[:, 22:24] = np.frombuffer(b"en", dtype=np.uint8)
    if pmode == "rise":
        p = 1 + (keys * 65000) // (keys.max() + 1)
    elif pmode == "zero":
        # posintext 0 over the first two 64-piece groups and into the third; the last positive
        # stored distance lies inside the second group (keys up to 200,000), which is no record
        # group: the fold takes it from that group's L_rest.  Then posintext 300 without stored
        # distances, so that D = |300 - that distance| and every distance term depends on it
        p = np.where(keys < 275000, 0, 300)
    elif pmode == "runs":
        p = 1 + (keys * 65000) // (keys.max() + 1)
        p[(keys // 9000) % 4 == 1] = 0       # runs of 0 over whole tiles
        p[(keys >= 100000) & (keys < 190000)] = 0  # and over whole 64-piece groups
    else:
        p = rng.integers(0, 65536, n)
    rows[:, 34] = (p >> 8) & 0xFF
    rows[:, 35] = p & 0xFF
    rows[:, 38] = rng.integers(0, 256, n) * (rng.random(n) < 0.5)
    if pmode == "zero":
        rows[:, 38] = rng.integers(40, 256, n)
        rows[(keys >= 199000) & (keys < 200000), 38] = 60  # the last positive one: D = |300 - 60|
        rows[keys >= 200000, 38] = 0
        # the rows with a stored distance are the newer ones, so they fill the top-k
        # and the top-k's distance terms (40..255 over D) depend on D
        rows[keys < 200000, 12:14] = np.frombuffer((20000).to_bytes(2, "big"), dtype=np.uint8)
    rows[:, 33] = rng.integers(1, 20, n)
    return rows


@pytest.mark.parametrize("algo", ["probe", "merge", "bitmap"])
def test_pieces_many_groups(algo, monkeypatch):
    """Joins whose compaction writes more than 64 and more than 128 pieces per query
    (one per tile: PROBE_TILE 256 over a small side of 25,000 / 42,000 ids, JOIN_TILE
    4096 over 300,000 + 4,000 / 285,000, BM_TILE 1024 over 75,000 / 150,000), so k_piece_merge
    makes two and three 64-piece groups and k_shard_fin folds them: posintext rising
    along the url order (every group overflows SEGC and is rewalked across group
    boundaries), rising with runs of 0 over whole tiles and whole groups, random;
    posintext 0 over the first 11/12 of both lists (more than 128 pieces: the first two
    groups fold stored distances alone, and the second hands on its last positive
    one, L_rest, from a piece that is not its first); nonzero stored distances; a query
    whose matches all lie in the last groups;
    profiles without authority beside authority and exclusions in one batch."""
    monkeypatch.setenv("YRWI_PROBE_RATIO", "1000000000" if algo == "merge" else "1")
    if algo == "probe":
        monkeypatch.setenv("YRWI_BM_DIV", "0")  # no url-id bitmaps: the id probe
    n = 300000
    keys = np.arange(n)
    rng = np.random.default_rng(23)
    pick = lambda frac: keys[rng.random(n) < frac]
    # (small side S, mid side M, the keys of L: the matches of S x L lie in S's last tiles only)
    fs, fm, l0 = {"merge": (0.95, 0.94, 296000), "probe": (0.14, 0.083, 250000), "bitmap": (0.5, 0.25, 140000)}[algo]
    spec = [("A", keys, "rise"), ("S", pick(fs), "runs"), ("M", pick(fm), "rise"), ("R", pick(fs), "rand"),
            ("L", keys[keys >= l0], "rise"), ("E", pick(0.3), "rand"), ("Z", keys, "zero"), ("Y", pick(fs), "zero")]
    size = {nm: len(ks) for nm, ks, _ in spec}
    if algo == "merge":    # tiles of JOIN_TILE over both lists
        assert size["A"] + size["S"] > 128 * 4096 and size["S"] >= 280000 and size["A"] + size["L"] > 64 * 4096
    elif algo == "probe":  # tiles of PROBE_TILE over the small side
        assert size["S"] >= 40000 > 128 * 256 and 128 * 256 > size["M"] > 64 * 256 and size["L"] > size["S"]
    else:                  # tiles of BM_TILE over the small side
        assert size["S"] >= 140000 > 128 * 1024 and 128 * 1024 > size["M"] > 64 * 1024 and size["L"] > size["S"]
    d = {b"TERMpg%s_____" % nm.encode(): _keyed(ks, 3 + i, pm) for i, (nm, ks, pm) in enumerate(spec)}
    t = lambda names: [b"TERMpg%s_____" % x.encode() for x in names]
    c5 = jl.RankingProfile.parse("", "date=15,domlength=15,authority=13,tf=10")
    default, near = jl.RankingProfile(), single("worddistance", 15)
    plan = [(default, "AS", ""), (default, "SA", "E"), (default, "AM", ""), (default, "AR", ""), (default, "ASR", ""),
            (default, "SL" if algo != "merge" else "AL", ""), (near, "AS", ""), (near, "ASR", "E"), (near, "SR", ""),
            (c5, "AM", ""), (c5, "SL" if algo != "merge" else "AL", ""), (default, "ZY", ""), (default, "YZ", "")]
    ix = RWIIndex(0)
    try:
        for h, r in d.items():
            ix.add(h, r)
        batch = [Query(t(q), t(exc), k=100, profile=_rp(prof), now_ms=NOW) for prof, q, exc in plan]
        meta = [(pi, prof, q, exc) for pi, (prof, q, exc) in enumerate(plan)]
        st = CStats()
        got = qu.gpu_raw(ix, batch, stats=st)
        assert st.t_compact_ns > 0 and st.joined > 0
        for (pname, prof, q, exc), g in zip(meta, got):
            exp = qu.orc_raw(d, t(q), t(exc), orc.profile_from(prof), "en", NOW, 100)
            assert len(exp) == 100 * HIT
            if q in ("ZY", "YZ"):  # from the reference alone: the best hit's distance term depends on D
                _, nm = orc.search(d, t(q), [], orc.profile_from(prof), "en", now_ms=NOW, k=1, with_norm=True)
                zr = d[t("Z")[0]]
                best = zr[(zr[:, :12] == np.frombuffer(exp[:12], dtype=np.uint8)).all(axis=1)]
                assert nm.max_distance_D == 240 and len(best) == 1 and best[0, 38] >= 40
            qu.same_hits(g, exp, (algo, pname, q, exc))
    finally:
        ix.close()


# ------------------------------------------------------------------ i
@pytest.mark.parametrize("world", [2, 8])
def test_adversarial_shards(world):
    """Url-hash shards over the loopback transport: every url hash starts at or above
    char index 24, so with 8 shards the shards 0..2 are empty and the first valid
    shard is not shard 0 (k_combine's s == gf branch takes the clone clamp).  The
    first row of every list lies in the future; in list F it is the only one beside
    the first row of the last shard, whose date must stay unclamped."""
    full = universe_lists(31, 3000, fracs=(1.0, 0.6))
    full = {h: r for h, r in zip((b"TERMshA_____", b"TERMshB_____"), full.values())}
    uni = adv_rows(3000, 31, "edge", first_char_min=24)
    for h in full:  # the universe's hashes lie anywhere: take those of the shifted one
        sel = np.sort(np.random.default_rng(len(full[h])).choice(3000, len(full[h]), replace=False))
        full[h][:, :12] = uni[sel, :12]
        full[h][0, 12:14] = 255  # lastModified 65535: the clone is clamped to today
    few = adv_rows(2500, 32, "few", first_char_min=24)
    few[:, 12:14] = np.frombuffer((15000).to_bytes(2, "big"), dtype=np.uint8)
    few[0, 12:14] = np.frombuffer((40000).to_bytes(2, "big"), dtype=np.uint8)
    last = np.flatnonzero((np.array(jl.AHPLA)[few[:, 0]] >> (6 - (world.bit_length() - 1))) == world - 1)[0]
    assert last > 0
    few[last, 12:14] = np.frombuffer((50000).to_bytes(2, "big"), dtype=np.uint8)
    full[b"TERMshF_____"] = few
    A, B, F = full
    parts = [{h: shard_of(r, rk, world) for h, r in full.items() if len(shard_of(r, rk, world))} for rk in range(world)]
    if world == 8:
        assert [len(p) for p in parts[:3]] == [0, 0, 0] and all(len(p) for p in parts[3:])
    c5 = jl.RankingProfile.parse("", "date=15,domlength=15,authority=13,tf=10")
    cases = [(inc, exc, name, prof) for inc, exc in (([A], []), ([B], []), ([F], []), ([A, B], []), ([F, A], []))
             for name, prof in (("default", jl.RankingProfile()), ("c5", c5), ("date", single("date", 15)))]

    def run(rk, ix):
        return qu.gpu_raw(ix, [Query(inc, exc, k=100, profile=_rp(prof), now_ms=NOW) for inc, exc, _, prof in cases])

    res = iu.run_parts(parts, world, run)
    for rk, got in enumerate(res):
        for (inc, exc, name, prof), g in zip(cases, got):
            qu.same_hits(g, qu.orc_raw(full, inc, exc, orc.profile_from(prof), "en", NOW, 100), (world, rk, inc, name))


# ------------------------------------------------------------------ j
def test_adversarial_events(ctx):
    """SearchEvent arrivals drawn from an adversarial pool of 1,200 rows: duplicates
    inside and across arrivals, one arrival of more than 2,048 rows; the stack, the
    flag counts, the max-distance fold and maxdomcount against java_literal."""
    pool = adv_rows(1200, 9, "edge")
    rng = np.random.default_rng(9)
    arrivals = [(pool[:300], True)]
    for m in (40, 700, 2500, 1, 300):
        take = rng.integers(0, 1200, m)
        take[: m // 4] = take[rng.integers(0, m, m // 4)]
        arrivals.append((pool[take], False))
    high = palette_profile((15, 16, 22, 23, 24, 31), 102)
    check_event(ctx, arrivals, k=3000)
    check_event(ctx, arrivals, {"coeff_authority": 14, "coeff_worddistance": 15}, k=3000)
    check_event(ctx, arrivals[1:], {f: getattr(high, f) for _, f in jl.PROFILE_FIELDS}, k=200)


# ------------------------------------------------------------------ k
def test_bytes_survive_storage(tmp_path):
    """All 40 bytes of a row come back: nonzero reserved bytes and `s` column through
    put_list / get_list, through add_postings(keep) of a disjoint batch, and in the
    heap dump's image."""
    import dump_ref as dr
    T = b"TERMbytes___"
    rows = adv_rows(700, 61, "edge")
    more = adv_rows(300, 62, "edge")
    assert not {bytes(x) for x in rows[:, :12]} & {bytes(x) for x in more[:, :12]}
    assert (rows[:, [14, 15, 28, 39]] != 0).any(axis=0).all()
    ix = RWIIndex(0)
    try:
        ix.add(T, rows)
        assert np.array_equal(ix.get_list(T), rows)
        ix.add_postings([T] * len(more), more, policy="keep")
        merged = sort_rows(np.concatenate([rows, more]))
        assert np.array_equal(ix.get_list(T), merged)
        path = tmp_path / "adv.blob"
        ix.dump_heap(str(path), None, now_ms=NOW)
        assert path.read_bytes() == dr.expected_image({T: merged}, now_ms=NOW)
    finally:
        ix.close()
