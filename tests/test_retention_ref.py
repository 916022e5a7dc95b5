"""The retention reference (tests/retention_ref.py) against an independent cut-day restatement on every
directed case of tests/retention_cases.py and on the re-dated `tiny` corpus, the facts the cases claim,
and the presence of yrwi_retain / yrwi_retention_count in the library, its ctypes table and the header.
No GPU."""

import ctypes
import os
import re

import numpy as np
import pytest

import retention_cases as rc
import retention_ref as rr
from yacy_search_server_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def corpus():
    idx = synth.build_index(synth.preset("tiny"))
    lists = rr.redate(idx.as_dict(), rc.CORPUS_DAYS, rc.CORPUS_WEIGHTS)
    return idx.rows, lists


def _cut_day_form(lists, min_day, max_refs, terms=None):
    """the rules in the form the device applies them: per list the cut day d* = the max_refs-th largest day
    of the survivors and the quota q; keep a > d*, and of a == d* the first q"""
    out, removed_age, removed_cap = dict(lists), 0, 0
    for t in rr.selected(lists, terms):
        rows = lists[t]
        a = [int(x) for x in rr.days_of(rows)]
        surv = [i for i in range(len(a)) if a[i] >= min_day]
        keep = surv
        if max_refs > 0 and len(surv) > max_refs:
            d = sorted((a[i] for i in surv), reverse=True)[max_refs - 1]
            q = max_refs - sum(1 for i in surv if a[i] > d)
            keep, rank = [], 0
            for i in surv:
                if a[i] > d or (a[i] == d and rank < q):
                    keep.append(i)
                rank += a[i] == d
        removed_age += len(a) - len(surv)
        removed_cap += len(surv) - len(keep)
        if len(keep) == len(a):
            continue
        if keep:
            out[t] = rows[keep]
        else:
            del out[t]
    return out, removed_age, removed_cap


def _same(a, b):
    return set(a) == set(b) and all(a[t].tobytes() == b[t].tobytes() for t in a)


def _check(lists, min_day, max_refs, terms=None):
    """the reference against the restatement; its own invariants; idempotence"""
    new, st, rs = rr.apply_retention(lists, min_day, max_refs, terms)
    alt, age, cap = _cut_day_form(lists, min_day, max_refs, terms)
    assert _same(new, alt), (min_day, max_refs)
    if min_day or max_refs:
        assert (rs["removed_age"], rs["removed_cap"]) == (age, cap)
    assert st["removed"] == rs["removed_age"] + rs["removed_cap"]
    assert st["removed"] == sum(len(l) for l in lists.values()) - sum(len(l) for l in new.values())
    assert st["emptied_terms"] == rs["emptied_terms"] == len(lists) - len(new)
    for t, l in new.items():  # kept rows keep their bytes and their order: a subsequence of the list
        if l is not lists[t]:
            have = {bytes(r) for r in l}
            assert [bytes(r) for r in lists[t] if bytes(r) in have] == [bytes(r) for r in l]
            if max_refs and (terms is None or t in terms):
                assert len(l) <= max_refs
    again, st2, rs2 = rr.apply_retention(new, min_day, max_refs, terms)
    assert _same(again, new) and st2["removed"] == 0 and st2["terms"] == 0
    assert all(again[t] is new[t] for t in new)
    return new, st, rs


def test_corpus_has_what_the_cases_rely_on(corpus):
    base, lists = corpus
    assert sum(len(l) for l in lists.values()) == 60050 and len(lists) == 200
    h = rr.day_hist(lists)
    assert h.sum() == 60050 and set(np.flatnonzero(h)) == set(rc.CORPUS_DAYS)
    assert max(rc.CORPUS_DAYS) - min(rc.CORPUS_DAYS) < _lib.RETENTION_LDS_WINDOW // 2  # one LDS window holds them
    median = int(np.searchsorted(np.cumsum(h), (h.sum() + 1) // 2))
    assert 0.3 < h[:median].sum() / h.sum() < 0.7  # the age case removes 30-70 % of the rows
    cap = int(np.median([len(l) for l in lists.values()])) // 2
    assert sum(len(l) > cap for l in lists.values()) > len(lists) // 2
    assert max(len(l) for l in lists.values()) > 256  # a list longer than the smallest chunk
    assert not any(t.startswith(b"-r") for t in lists)
    # the same corpus every time
    assert _same(lists, rr.redate(lists, rc.CORPUS_DAYS, rc.CORPUS_WEIGHTS))


def test_every_list_three_ways(corpus):
    base, lists = corpus
    h = rr.day_hist(lists)
    median = int(np.searchsorted(np.cumsum(h), (h.sum() + 1) // 2))
    cap = int(np.median([len(l) for l in lists.values()])) // 2
    _, st, rs = _check(lists, median, 0)
    assert rs["removed_cap"] == 0 and rs["removed_age"] == h[:median].sum() and rs["lists_cap"] == 0
    _, st, rs = _check(lists, 0, cap)
    assert rs["removed_age"] == 0 and rs["lists_cap"] > 100 and rs["emptied_terms"] == 0
    _, st, rs = _check(lists, median, cap)
    assert rs["removed_age"] == h[:median].sum() and rs["removed_cap"] > 0
    assert (rs["day_min"], rs["day_max"]) == (min(rc.CORPUS_DAYS), max(rc.CORPUS_DAYS))
    assert (rs["lists"], rs["postings"]) == (200, 60050)


def test_edges(corpus):
    base, _ = corpus
    lists, what = rc.edge_lists(base)
    assert len(lists) == len(rc.SIZES) * len(rc.PATTERNS) == 64
    assert {1, 62, 63, 64, 65, 66, 1024, 1025, 1026} <= set(rc.EDGE_CAPS) and 0 not in rc.EDGE_CAPS
    straddle = [rr.days_of(l) for t, l in lists.items() if what[t][1] == "straddle" and len(l) >= 63]
    assert all({int(x) >> 8 for x in a} == {0x4E, 0x4F} and {int(x) & 255 for x in a} == {0xFE, 0xFF, 0, 1} for a in straddle)
    for cap in rc.EDGE_CAPS:
        new, st, rs = _check(lists, 0, cap)
        rc.check_edges(lists, what, new, cap)
        assert rs["lists_cap"] == sum(1 for n, _ in what.values() if n > cap)
    # the cut day of a straddling list falls on the last day of one bucket and on the first of the next
    for cap, day in ((17, 0x4F00), (40, 0x4EFF)):
        t = next(t for t, w in what.items() if w == (65, "straddle"))
        new, _, _ = rr.apply_retention(lists, 0, cap, [t])
        assert int(rr.days_of(new[t]).min()) == day


def test_ties(corpus):
    base, _ = corpus
    lists = rc.tie_lists(base)
    for cap in rc.TIE_CAPS:
        new, st, rs = _check(lists, 0, cap)
        for t in lists:  # exactly the first `cap` rows in url order stay
            assert new[t].tobytes() == lists[t][:cap].tobytes()
    lists, ends = rc.scatter_lists(base)
    assert sorted(ends.values()) == [63, 64, 255, 256, 1023, 1024]
    new, st, rs = _check(lists, 0, rc.SCATTER_CAP)
    rc.check_scatter(lists, ends, new)
    assert rs["lists_cap"] == len(lists)


def test_age_meets_cap(corpus):
    base, _ = corpus
    lists = rc.age_cap_lists(base)
    exact, plus, emptied = list(lists)
    new, st, rs = _check(lists, rc.AGE_MIN_DAY, rc.AGE_CAP)
    assert len(new[exact]) == len(new[plus]) == rc.AGE_CAP and emptied not in new
    assert (rs["lists_age"], rs["lists_cap"], rs["removed_cap"], rs["emptied_terms"]) == (3, 1, 1, 1)
    new, st, rs = _check(lists, 65536, 0, [plus, emptied])
    assert set(new) == {exact} and st["emptied_terms"] == 2 and rs["removed_age"] == len(lists[plus]) + 40


def test_small_hot_and_histogram_cases(corpus):
    base, _ = corpus
    for count in (30, 3000):
        lists = rc.small_lists(base, count)
        assert len(lists) == count and {len(l) for l in lists.values()} == {1, 2, 3}
        new, st, rs = _check(lists, 150, 1)
        assert rs["lists_age"] > 0 and rs["lists_cap"] > 0 and rs["emptied_terms"] > 0
    hot = {rc.term(900): rc.hot_list(base)}
    new, st, rs = _check(hot, 0, rc.HOT_CAP)
    a = rr.days_of(new[rc.term(900)])
    assert len(a) == rc.HOT_CAP and set(a) == {20002}  # the cut is inside the newest day: a tie
    assert (rr.days_of(hot[rc.term(900)]) == 20002).sum() > rc.HOT_CAP
    band, spread = rr.day_hist(rc.band_lists(base)), rr.day_hist(rc.spread_lists(base))
    nz = np.flatnonzero(band)
    assert nz.max() - nz.min() < _lib.RETENTION_LDS_WINDOW // 2 and band.sum() == 2800
    assert spread[0] > 0 and spread[65535] > 0 and spread.sum() == 2804
    assert (np.flatnonzero(spread) // _lib.RETENTION_LDS_WINDOW).max() == 7  # no window holds them all


def test_selection_and_noop(corpus):
    base, lists = corpus
    order = sorted(lists)
    named = order[::9][:10]
    terms = named + [named[2], rc.term(77)]
    new, st, rs = _check(lists, 20600, 50, terms)
    assert rs["lists"] == 10 and all(new[t] is lists[t] for t in order if t not in named)
    new, st, rs = rr.apply_retention(lists, 0, 0)
    assert all(new[t] is lists[t] for t in lists) and (st, rs) == rr.noop_stats()
    assert rr.apply_retention(lists, 5, 5, [])[1:] == rr.noop_stats()
    _, _, rs = rr.apply_retention(lists, 0, 0, dry_hist=True)
    assert (rs["lists"], rs["postings"], rs["day_min"], rs["removed_age"]) == (200, 60050, min(rc.CORPUS_DAYS), 0)
    assert (rr.day_hist(lists, terms) == rr.day_hist({t: lists[t] for t in named})).all()


def test_library_exports_and_header():
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "yrwi.h")).read()
    for name in ("yrwi_retain", "yrwi_retention_count"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint %s\(" % name, header)
    assert "UNVERIFIED against a reference line: the reference has no method that drops" in header
    # the ctypes struct has the header's layout: 7 x int64, 4 x int32, 4 x int64
    body = re.search(r"typedef struct yrwi_retention_stats \{(.*?)\} yrwi_retention_stats;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for typ, names in re.findall(r"(int64_t|int32_t)\s+([^;]+);", body):
        fields += [(n.strip(), typ) for n in names.split(",")]
    ct = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    assert [(n, ct[t]) for n, t in fields] == list(_lib.CRetentionStats._fields_)
    assert ctypes.sizeof(_lib.CRetentionStats) == 7 * 8 + 4 * 4 + 4 * 8
