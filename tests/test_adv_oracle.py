"""The two CPU restatements on adversarial rows (tests/adv_rows.py): the literal
object-level one (java_literal) against the flat C++ oracle.  The GPU tests of
test_gpu_adversarial.py compare libyrwi with the C++ oracle alone; this file is
what licenses that on rows no synthetic corpus produces (cells at 0 / 255 / 65535,
dates in the future, wordsintext = wordsintitle = 0, any doctype, flag and
language byte, nonzero reserved bytes, coefficients outside 0..15)."""

import numpy as np
import pytest

import java_literal as jl
import oracle as orc
from adv_rows import (CONST_COLS, adv_profiles, adv_rows, col_values, flag_walk_rows, hashcodes, shard_of, single,
                      sort_rows, span_rows, universe_lists, flag_profiles)

DAY = 86400000
NOW = 20741 * DAY + 4242
NOWS = [NOW, 15500 * DAY + 7, 70000 * DAY + 1]


def _rows(a):
    return [bytes(r) for r in a]


def test_generators_are_valid_and_deterministic():
    for mode in ["edge", "few"] + ["const:" + c for c in CONST_COLS]:
        r = adv_rows(700, 3, mode)
        assert r.shape == (700, 40) and np.array_equal(r, adv_rows(700, 3, mode))
        keys = [jl.key72(bytes(x[:12])) for x in r]
        assert all(jl.wellformed(bytes(x[:12])) for x in r)
        assert all(a < b for a, b in zip(keys, keys[1:]))
        assert not ((r[:, 22] == 0) & (r[:, 23] == 0)).any()
        if mode.startswith("const:") and mode != "const:all":
            for c in mode[6:]:
                assert len(set(col_values(r, c))) == 1, mode
    e = adv_rows(700, 3, "edge")
    assert (e[:, 28] != 0).all() and (e[:, 39] != 0).all() and len(set(e[:, 21])) > 50
    assert {0, 255} <= set(col_values(e, "c")) and {0, 65535} <= set(col_values(e, "w"))
    assert ((col_values(e, "w") == 0) & (col_values(e, "u") == 0)).any()  # tf = c / 1
    assert len(np.unique(adv_rows(700, 3, "few")[:, 12:], axis=0)) <= 3
    s = span_rows("uxymncro", 5, 250, pad_to=513)
    for c in "uxymncro":
        assert set(col_values(s, c)) == set(range(5, 256))
    assert not np.array_equal(col_values(s, "u"), col_values(s, "x"))
    w8 = adv_rows(400, 1, "edge", first_char_min=24)
    assert [len(shard_of(w8, r, 8)) for r in range(3)] == [0, 0, 0]
    assert sum(len(shard_of(w8, r, 8)) for r in range(8)) == 400
    assert sum(len(shard_of(e, r, 2)) for r in range(2)) == 700 and len(shard_of(e, 0, 2)) > 0


@pytest.mark.parametrize("n", [1, 2, 3, 300, 700])
def test_single_lists(n):
    profs = adv_profiles()
    for mi, mode in enumerate(["edge", "few", "const:a", "const:cwu", "const:t", "const:all"]):
        rows = adv_rows(n, 11 + mi, mode)
        cont = _rows(rows)
        # every profile on the small lists, a rotating sample of them on the long ones
        pick = profs if n <= 3 else profs[:6] + profs[6 + mi::6]
        for pi, (pname, prof) in enumerate(pick):
            now = NOWS[(pi + mi) % 3]
            lang = ("en", "zz")[pi % 2]
            order = jl.ReferenceOrder(prof, lang)
            exp = [order.cardinal(e) for e in order.normalize_with(cont, now)]
            got, nm = orc.normalize_score(rows, orc.profile_from(prof), lang, now)
            assert got.tolist() == exp, (mode, pname, now)
            assert nm.max_distance_D == order.max.distance()
            a = jl.rank(cont, prof, lang, now)
            b = [(h, s) for h, s, _ in orc.search({b"TERMadv_____": rows}, [b"TERMadv_____"], [],
                                                  orc.profile_from(prof), lang, now_ms=now, k=3000)]
            assert a == b, (mode, pname, now)


@pytest.mark.parametrize("mode", ["edge", "few"])
def test_joins_and_exclusion(mode):
    d = universe_lists(5, 500, mode)
    dl = {h: _rows(r) for h, r in d.items()}
    A, B, C, D = d
    profs = [p for p in adv_profiles(singles=False)] + [("near", single("worddistance", 15))]
    for qi, (inc, exc) in enumerate([([A, B], []), ([B, C], []), ([A, B, C], []), ([A, B, C, D], []),
                                     ([A, B], [D]), ([C, B, A], [D])]):
        for md in (2147483647, 300, 1):
            for now in NOWS[:2]:
                a = jl.term_search(dl, inc, exc, md, now)
                b = orc.term_search(d, inc, exc, md, now)
                assert b"".join(a) == b.tobytes(), (qi, md, now)
        for pi, (pname, prof) in enumerate(profs):
            now = NOWS[(pi + qi) % 3]
            a = jl.search(dl, inc, exc, prof, "en", now_ms=now, k=3000)
            b = [(h, s) for h, s, _ in orc.search(d, inc, exc, orc.profile_from(prof), "en", now_ms=now, k=3000)]
            assert a == b and (len(a) > 0 or exc or len(inc) > 2), (qi, pname)


def test_flag_walk_and_query_languages():
    """Every flag bit alone, all and none, under profiles with distinct coefficients on
    the 11 flag terms; query languages that are no two-letter code match no row."""
    rows = flag_walk_rows(140, 2)
    assert hashcodes(rows).tolist() == [jl.bytearray_hashcode(bytes(r[:12])) for r in rows]
    assert np.array_equal(sort_rows(rows[::-1]), rows)
    cont = _rows(rows)
    for name, prof in flag_profiles():
        for lang in ("en", "e", "", "eng"):
            order = jl.ReferenceOrder(prof, lang)
            exp = [order.cardinal(e) for e in order.normalize_with(cont, NOW)]
            got, _ = orc.normalize_score(rows, orc.profile_from(prof), lang, NOW)
            assert got.tolist() == exp, (name, lang)
    assert len({bytes(r[29:33]) for r in rows}) == 34


def test_event_sequence():
    """SearchEventRWI on an adversarial pool, the reference of test_adversarial_events.
    The C++ oracle has no events, so only the first arrival is compared across the
    two restatements (jl.rank and orc.search of that container).  After the second
    arrival java_literal is checked against itself alone: entries keep the score
    they arrived with, and new urls were admitted."""
    pool = adv_rows(1200, 9, "edge")
    rng = np.random.default_rng(9)
    prof = adv_profiles(singles=False)[4][1]
    ev = jl.SearchEventRWI(prof, "en", NOW)
    first = _rows(pool[:400])
    ev.add_rwis(first, True)
    assert ev.stack() == jl.rank(first, prof, "en", NOW)
    T = b"TERMadv_____"
    hits, nm = orc.search({T: pool[:400]}, [T], [], orc.profile_from(prof), "en", now_ms=NOW, k=3000, with_norm=True)
    assert ev.stack() == [(h, s) for h, s, _ in hits]
    assert nm.max_distance_D == ev.order.max.distance()
    before = dict(ev.stack())
    ev.add_rwis(_rows(pool[rng.integers(0, 1200, 500)]), False)
    after = dict(ev.stack())
    assert all(after[h] == w for h, w in before.items() if h in after)
    assert ev.remote_available > 0 and len(after) > len(before)
