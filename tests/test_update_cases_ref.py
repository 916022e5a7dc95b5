"""The directed update cases (tests/update_cases.py) on the CPU: for every case and step the sequential
fold of tests/update_ref.py returns exactly the lists and the seven stats the case computed by
construction -- two independent statements of the rule of include/yrwi.h -- every list is strictly
ascending in the 72-bit key, and the edges the cases claim to reach are stated once more here, those
about the sorted batch through sorted_order().  No GPU."""

import numpy as np
import pytest

import update_cases as uc
import update_ref as ur

CASES = [(n, p) for n, ps in uc.names() for p in ps]
IDS = ["%s-%s" % np_ if len(dict(uc.names())[np_[0]]) > 1 else np_[0] for np_ in CASES]


def _same(a, b):
    assert set(a) == set(b), (sorted(set(a) ^ set(b))[:4])
    for t in a:
        assert a[t].tobytes() == b[t].tobytes(), t


@pytest.mark.parametrize("name,policy", [c for c in CASES if c[0] != "three_pieces"],
                         ids=[i for i, c in zip(IDS, CASES) if c[0] != "three_pieces"])
def test_reference_agrees(name, policy):
    c = uc.build(name, policy)
    cur = c.lists
    assert all(uc.ascending(l) and len(l) for l in cur.values())
    for s in c.steps:
        if s.op == "add":
            new, st = ur.apply_add(cur, s.terms, s.rows, s.policy)
            assert len(s.rows) == st["added"] + st["replaced"] + st["dropped"]
        elif s.op == "remove":
            new, st = ur.apply_remove(cur, s.urls, s.names)
        else:  # an add that fails leaves everything as it is; its bad row is the only one
            new, st = cur, dict.fromkeys(uc.STAT_KEYS, 0)
            bad_hash = (uc._RANK[s.rows[:, :12]] > 63).any(axis=1)
            no_lang = (s.rows[:, 22] == 0) & (s.rows[:, 23] == 0)
            assert (int(bad_hash.sum()), int(no_lang.sum())) == ((1, 0) if s.rc == -2 else (0, 1))
        assert st == s.stats, (name, st, s.stats)
        _same(new, s.lists)
        changed = [t for t in new if new[t] is not cur.get(t)]
        assert all(uc.ascending(new[t]) and len(new[t]) for t in changed)
        assert all(s.lists[t] is cur[t] for t in s.lists if t in cur and t not in changed)  # untouched: the same object
        cur = s.lists
    assert set(c.watch) >= set(c.lists) or c.light
    qs = c.queries()
    assert len(qs) == 6 and all(inc for inc, _ in qs)


def test_names_cover_the_issue():
    have = dict(uc.names())
    for w in uc.PLACEMENTS:
        assert have["geom_" + w] == ("replace",)
    for n in ("runs_lengths", "runs_last_modified", "run_at_block_edge", "same_url_neighbour_jobs", "near_keys"):
        assert have[n] == uc.POLICIES
    assert have["unchanged_among_changed"] == ("keep",)
    for p in uc.RM_PATTERNS:
        assert "rm_%s_named" % p in have and "rm_%s_all" % p in have
    assert len(uc.RM_PATTERNS) == 16 and uc.RM_SIZES == (1, 63, 64, 65, 255, 256, 257, 1025)
    assert uc.LENS == (0, 1, 63, 64, 65, 255, 256, 257, 1025)
    for n in (1, 2, 3, 255, 256, 257, 4097, 65537):
        assert "jobs_%d" % n in have


def test_jbits_edges():
    """255, 256 -> 8 bits; 257 -> 9; 65,537 -> 17: 8 + jbits = 25 bits, a fourth 8-bit radix pass"""
    assert [uc.build("jobs_%d" % n).facts["jbits"] for n in (1, 2, 3, 255, 256, 257)] == [1, 1, 2, 8, 8, 9]
    c = uc.build("jobs_65537")
    job, names = uc.jobs_of(c.steps[0].terms)
    assert len(names) == 65537 > 1 << 16 and (job == np.arange(65537)).all()
    pre = c.facts["prebuilt"]
    assert [names.index(t) for t in pre] == [0, 255, 256, 65535, 65536] and set(pre) == set(c.lists)
    assert all(len(c.lists[t]) == 3 for t in pre)
    c = uc.build("jobs_4097")
    assert [uc.jobs_of(c.steps[0].terms)[1].index(t) for t in c.facts["prebuilt"]] == [0, 255, 256, 4095, 4096]


@pytest.mark.parametrize("policy", uc.POLICIES)
def test_block_edge_positions(policy):
    c = uc.build("run_at_block_edge", policy)
    s = c.steps[0]
    o = uc.sorted_order(s.terms, s.rows)
    sk = [uc.key72(r) for r in s.rows[o]]
    n = len(sk)
    for k, lo, hi in c.facts["runs"].values():
        assert [i for i in range(n) if sk[i] == k] == list(range(lo, hi + 1))
    runs = c.facts["runs"]
    assert runs["head0"][1] == 0 and runs["tail"][2] == n - 1
    assert runs["edge"][1] == 255 and runs["edge"][2] >= 512  # head in block 0, tail in blocks 1 and 2


@pytest.mark.parametrize("policy", uc.POLICIES)
def test_neighbour_jobs_adjacent(policy):
    c = uc.build("same_url_neighbour_jobs", policy)
    s = c.steps[0]
    o = uc.sorted_order(s.terms, s.rows)
    job = uc.jobs_of(s.terms)[0][o]
    sk = [uc.key72(r) for r in s.rows[o]]
    assert len(c.facts["pairs"]) == 7
    for last, first in c.facts["pairs"]:
        assert first == last + 1 and sk[last] == sk[first] and job[first] == job[last] + 1
        assert all(sk[i] < sk[last] for i in range(len(sk)) if job[i] == job[last] and sk[i] != sk[last])
        assert all(sk[i] > sk[first] for i in range(len(sk)) if job[i] == job[first] and sk[i] != sk[first])
    # two runs: the url is in both jobs' lists afterwards
    for j in range(7):
        u = sk[c.facts["pairs"][j][0]]
        for t in (uc.term(2200 + j), uc.term(2200 + j + 1)):
            assert u in {uc.key72(r) for r in s.lists[t]}


def test_runs_reach_their_lengths():
    c = uc.build("runs_lengths", "recent")
    s = c.steps[0]
    _, counts = np.unique(uc.s12(s.rows[uc.s12(s.terms) == uc.term(2000)]), return_counts=True)
    assert set(c.facts["run_lengths"]) == {1, 2, 3, 64, 257, 1000} <= set(int(x) for x in counts)
    for L in (1, 2, 3, 64, 257, 1000):  # for a url new to the list and for one it has
        assert sum(1 for x in counts if x == L) >= 2
    # the three policies give three different lists
    got = {p: uc.build("runs_lengths", p).steps[0].lists[uc.term(2000)].tobytes() for p in uc.POLICIES}
    assert len(set(got.values())) == 3
    got = {p: uc.build("runs_last_modified", p).steps[0].lists[uc.term(2000)].tobytes() for p in uc.POLICIES}
    assert len(set(got.values())) == 3


def test_recent_ties_separate_the_comparisons():
    """RECENT with `>` in place of `>=` inside a run, or against the list's row, gives other lists on
    runs_last_modified: a kernel with either slip cannot pass that case"""
    c = uc.build("runs_last_modified", "recent")
    s = c.steps[0]
    t = uc.term(2000)

    def fold(in_run_strict, row_strict):
        cell = {bytes(r[:12]): (bytes(r), True) for r in c.lists[t]}
        for tt, r in zip(uc.s12(s.terms), s.rows):
            if tt != t:
                continue
            u, d = bytes(r[:12]), int(uc.days_of(r[None])[0])
            if u in cell:
                hd = int(uc.days_of(np.frombuffer(cell[u][0], np.uint8)[None])[0])
                strict = row_strict if cell[u][1] else in_run_strict
                if d < hd or (strict and d == hd):
                    continue
            cell[u] = (bytes(r), False)
        return b"".join(cell[u][0] for u in sorted(cell, key=ur.url_key))

    right = fold(False, False)
    assert right == s.lists[t].tobytes()
    assert fold(True, False) != right and fold(False, True) != right


def test_near_keys_agree_in_64_bits():
    c = uc.build("near_keys", "replace")
    s = c.steps[0]
    for t in (uc.term(2300), uc.term(2301), uc.term(2302)):
        khi, klo = uc.split_keys(s.lists[t])
        low64 = (khi << np.uint64(8)) | klo  # the first sort's key
        assert int((khi[1:] == khi[:-1]).sum()) >= 80       # neighbours told apart by klo alone
        assert len(set(low64.tolist())) <= len(low64) - 80   # and rows told apart by khi >> 56 alone
    # a compare blind to klo, or to the top 8 bits, would take postings of the batch for duplicates
    bk, bl = uc.split_keys(s.rows)
    job = uc.jobs_of(s.terms)[0]
    full = len({(j, int(h), int(l)) for j, h, l in zip(job, bk, bl)})
    assert full == len(s.rows)
    assert len({(j, int(h)) for j, h in zip(job, bk)}) < full
    assert len({(j, int(h) & ((1 << 56) - 1), int(l)) for j, h, l in zip(job, bk, bl)}) < full


def test_near_miss_set():
    c = uc.build("rm_near_miss")
    miss, true = c.facts["near_sets"]
    have = {bytes(r[:12]) for l in c.lists.values() for r in l}
    assert len(miss) == 1200 and not set(miss) & have and len(true) == 20 and set(true) <= have
    hk = {uc.key72(h) >> 8 for h in have}
    assert sum(1 for u in miss if uc.key72(u) >> 8 in hk) >= 400  # (c): khi of a row that stays
    low = {uc.key72(h) & ((1 << 64) - 1) for h in have}
    assert sum(1 for u in miss if uc.key72(u) & ((1 << 64) - 1) in low) >= 800  # (a), (b)
    assert c.steps[0].stats["removed"] == 0 and c.steps[1].stats["removed"] == 20


def test_tiny_lists_boundaries():
    c = uc.build("tiny_lists")
    assert [len(l) for l in c.lists.values()][:703] == [1] * 700 + [64] * 3
    job, names = uc.jobs_of(c.steps[0].terms)
    assert len(names) == 703 and set(names) == set(list(c.lists)[:703])


def test_three_pieces():
    c = uc.build("three_pieces")
    s = c.steps[0]
    n = len(s.rows)
    assert n == 850_000 and n * 40 == 34_000_000 and n * 40 > 2 * (16 << 20)
    assert sum(len(l) for l in s.lists.values()) == n == s.stats["added"] and len(s.lists) == 3
    for l in s.lists.values():
        khi, klo = uc.split_keys(l)
        assert (khi[1:] > khi[:-1]).all()  # (distinct in their first ten characters)
    assert len(np.unique(uc.s12(s.rows))) == n
    o = uc.sorted_order(s.terms, s.rows)
    assert (np.diff(o) < 0).sum() > n // 3  # given in random order
    job, names = uc.jobs_of(s.terms)
    for j, t in enumerate(names):
        assert s.rows[o][job[o] == j].tobytes() == s.lists[t].tobytes()
