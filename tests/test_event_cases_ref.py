"""CPU checks of tests/event_cases.py: every case through java_literal.SearchEventRWI, and the
conditions the case claims about itself (Case.facts) asserted on the oracle alone.  These are
conditions, not measurements: they keep every input at the point of k_event_add it was built for
(a chunk edge, a round of the fold, a tie, the cut of the bounded stack, ...), whatever the library
does with it.  tests/test_gpu_event_arrivals.py runs the same cases on the device."""

import numpy as np
import pytest

import adv_rows as ar
import event_cases as ec
import java_literal as jl


def _params():
    return [pytest.param(g, n, id=f"{g}-{n}") for g in ec.GROUPS for n in ec.names(g)]


_RUNS = {}


def _run(group, name):
    if (group, name) not in _RUNS:
        _RUNS[(group, name)] = ec.run_oracle(ec.case(group, name))
    return _RUNS[(group, name)]


def _urls_of(rec):
    return [h for h, _, _ in rec["stack"]]


def _before(recs, j):
    return recs[j - 1]["stack"] if j else []


def _flag_counts(rows_list):
    out = [0] * 32
    for r in rows_list:
        f = jl.Bitfield(r[29:33])
        for b in range(32):
            out[b] += f.get(b)
    return out


def test_groups_and_limits():
    assert list(ec.GROUPS) == ["sizes", "fold", "first_row", "stack", "ties", "doublecheck", "authority", "rejects",
                               "pulls"]
    seen = set()
    for g in ec.GROUPS:
        for c in ec.GROUPS[g]():
            assert c.name not in seen, c.name
            seen.add(c.name)
            assert c.total_rows() <= 7100, (c.name, c.total_rows())
            assert all(len(s[1]) <= 3073 for s in c.steps if s[0] in ("add", "bad")), c.name
            assert 1 <= c.k <= jl.MAX_RESULTS_RWI
    assert [n for n in ec.SIZES] == [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3073]
    assert {c.k for c in ec.sizes()} == {3000, 100}
    assert ec.STACK_KS == (1, 2, 64, 255, 256, 257, 1024, 3000)


def test_family_is_one_class():
    """32 well-formed urls, one hashCode, one dom-length class, 4 hosts; with identical feature
    bytes one arrival of all of them leaves a stack of 1 and admits 32"""
    for f in (0, 3, 17):
        fam = ec.family(f)
        ks = ec.keys(ec.plain_rows(fam))
        assert len(set(ks)) == 32 and all(jl.wellformed(k) for k in ks)
        assert len({jl.bytearray_hashcode(k) for k in ks}) == 1
        assert len({jl.dom_length_normalized(k) for k in ks}) == 1
        assert len({k[6:12] for k in ks}) == 4  # blocks 6 and 8 lie in the host hash
        ev = jl.SearchEventRWI(jl.RankingProfile(), "en", ec.NOW)
        assert ev.add_rwis([bytes(r) for r in ec.plain_rows(fam, w=5)], True) == 32
        assert len(ev.stack()) == 1 and ev.stack()[0][0] == ks[0]


def test_fold_restatement_equals_the_oracle():
    """event_cases.fold_distances (the value the fold cases state) on random arrivals"""
    rng = np.random.default_rng(9)
    for trial in range(30):
        arrs = []
        for a in range(int(rng.integers(1, 4))):
            n = int(rng.integers(1, 150))
            arrs.append(ec.plain_rows(ec.urls(n, 2000 + 4 * trial + a), t=rng.integers(0, 40, n) * rng.integers(0, 2, n),
                                      i=rng.integers(0, 30, n) * rng.integers(0, 2, n)))
        order = jl.ReferenceOrder(jl.RankingProfile(), "en")
        got = []
        for r in arrs:
            order.normalize_with([bytes(x) for x in r], ec.NOW)
            got.append(order.max.distance())
        assert got == ec.fold_distances(arrs), trial


@pytest.mark.parametrize("group,name", _params())
def test_case_facts(group, name):
    c = ec.case(group, name)
    recs, sources, ref = _run(group, name)
    f = c.facts
    assert len(recs) == len(c.steps)
    # every case: the feature under test carries weight
    prof = ec.profile_of(c)
    assert f["weights"] and all(getattr(prof, x) != 0 for x in f["weights"])
    if group in ("fold", "first_row"):
        assert prof.coeff_worddistance == 15
    if group == "authority":
        assert prof.coeff_authority > 12
    adds = [j for j, s in enumerate(c.steps) if s[0] == "add"]

    if "lengths" in f:
        assert [len(c.steps[j][1]) for j in adds] == f["lengths"]
    for j, rows_at in f.get("dups", ()):
        ks = ec.keys(c.steps[j][1])
        assert len({ks[r] for r in rows_at}) == 1
        assert len({bytes(c.steps[j][1][r]) for r in rows_at}) == len(rows_at)  # other features
    if "repeats" in f:
        j, r, j0, r0 = f["repeats"]
        assert ec.keys(c.steps[j][1])[r] == ec.keys(c.steps[j0][1])[r0]
        shared = set(ec.keys(c.steps[j][1])) & set(ec.keys(c.steps[j0][1]))
        assert shared == {ec.keys(c.steps[j0][1])[r0]}  # n other rows, but for the planted url
    if group == "sizes":
        n = f["lengths"][0]
        assert recs[-1]["info"]["postings_in"] == 2 * n
        pairs = sum(len(g) - 1 for j, g in f["dups"] if j == 0)  # rows per arrival that repeat a url of it
        assert recs[0]["info"]["admitted_local"] == n - pairs
        assert recs[1]["info"]["admitted_remote"] == n - pairs - 1

    if "newmax" in f:
        arrs = [c.steps[j][1] for j in adds]
        assert ec.new_maxima(arrs) == f["newmax"]
        # the same count, straight from the columns: a row above everything before it in the event
        flat = np.concatenate([ar.col_values(a, "t") for a in arrs])
        run = np.maximum.accumulate(flat)
        rec = np.concatenate([[False], flat[1:] > run[:-1]])
        off = 0
        for a, per in zip(arrs, f["newmax"]):
            assert [int(rec[off + s:off + min(s + ec.ROUND, len(a))].sum()) for s in range(0, len(a), ec.ROUND)] == per
            off += len(a)
    if "newmax_is" in f:
        j, per = f["newmax_is"]
        assert f["newmax"][j] == per
    if "distance" in f:
        assert [recs[j]["info"]["max_distance"] for j in adds] == f["distance"]
    if "distance_is" in f:
        assert f["distance"] == f["distance_is"]
    if "P" in f:
        assert int(ar.col_values(c.steps[0][1], "t").max()) == f["P"]  # the event's P when the second arrival comes
        assert ref.order.max.posintext == f["P"] + f["newmax_is"][1][0]

    if "differs_from" in f:
        other = _run(group, f["differs_from"])[0][-1]
        assert (other["stack"], other["info"]["max_distance"]) != (recs[-1]["stack"], recs[-1]["info"]["max_distance"])
        assert other["info"]["max_distance"] != recs[-1]["info"]["max_distance"]
    if "equals" in f:
        other = _run(group, f["equals"])[0][-1]
        assert other["stack"] == recs[-1]["stack"] and recs[-1]["stack"]
        assert other["info"] == recs[-1]["info"]

    if "stack_before" in f:
        j, K = f["stack_before"]
        assert len(_before(recs, j)) == K == c.k
    for j in f.get("unchanged", ()):
        assert recs[j]["stack"] == _before(recs, j) and recs[j]["stack"]
    for j in f.get("disjoint", ()):
        assert not set(_urls_of(recs[j])) & {h for h, _, _ in _before(recs, j)}
        assert len(recs[j]["stack"]) == c.k
    for j in f.get("alternates", ()):
        old = {h for h, _, _ in _before(recs, j)}
        pattern = [h in old for h in _urls_of(recs[j])]
        assert pattern == [True] + [i % 2 == 1 for i in range(len(pattern) - 1)]
        assert len({w for _, w, _ in recs[j]["stack"][1:]}) == 1  # one score: the order is the hashCode order
    for j, n in f.get("classes", {}).items():
        rows = [bytes(r) for r in c.steps[j][1]]
        ev = jl.SearchEventRWI(prof, c.language, ec.NOW, maxsize=len(rows) + 1)
        ev.add_rwis(rows, True)
        assert len(ev.stack()) == n == len({(w, jl.bytearray_hashcode(h)) for h, w in ev.stack()})
    for j, n in f.get("stack_after", {}).items():
        assert len(recs[j]["stack"]) == n
    for j, us in f.get("entered", {}).items():
        old = {h for h, _, _ in _before(recs, j)}
        assert all(u in _urls_of(recs[j]) and u not in old for u in us)
    for j, us in f.get("stays_out", {}).items():
        assert not set(us) & set(_urls_of(recs[j]))
    if "last_is" in f:
        j, u = f["last_is"]
        assert _before(recs, j)[-1][0] == u

    for j, n in f.get("rejected_twins", {}).items():
        old = {h for h, _, _ in _before(recs, j)}
        entered = [h for h in _urls_of(recs[j]) if h not in old]
        cut = len(old) + len(entered) - len(recs[j]["stack"])  # pushed out by the bound, not by a twin
        assert recs[j]["admitted"] - len(entered) - (0 if name.startswith("twin_of_") else cut) == n > 0
    for j, n in f.get("admits", {}).items():
        assert recs[j]["admitted"] == n
    for j, us in f.get("pulled", {}).items():
        assert [h for h, _ in recs[j]["pulled"]] == us
    if "would_score_higher" in f:
        j, r = f["would_score_higher"]
        row = bytes(c.steps[j][1][r])
        old = dict((h, w) for h, w, _ in recs[j]["stack"])[row[:12]]
        assert ref.order.cardinal(jl.Vars.from_row(row, ec.NOW)) > old

    if f.get("flag_rule"):
        rows = [bytes(r) for j in adds for r in c.steps[j][1]]
        admitted = [bytes(c.steps[adds[a - 1]][1][r]) for (a, r) in sources.values() if a > 0]
        got = recs[-1]["info"]["flagcount"]
        assert got != _flag_counts(rows) and got != _flag_counts(admitted)
    for u, where in f.get("sources", {}).items():
        assert sources.get(u, (-1, -1)) == where, (u, sources.get(u))
    if group == "doublecheck":
        assert f["sources_all"] == {u: sources.get(u, (-1, -1)) for u in ec.all_urls(c)}
    for b, n in f.get("flagcount_bits", {}).items():
        assert recs[-1]["info"]["flagcount"][b] == n, b

    if "maxdomcount" in f:
        assert [recs[j]["info"]["maxdomcount"] for j in adds] == f["maxdomcount"]
    if "hosts" in f:
        assert len(ref.order.doms) == f["hosts"]
    if f.get("keeps_scores"):
        grown = 0
        for j in adds[1:]:
            old = {h: w for h, w, _ in _before(recs, j)}
            now = {h: w for h, w, _ in recs[j]["stack"]}
            assert all(now[h] == w for h, w in old.items() if h in now)
            # ... although the same rows scored again now would get another score
            rows = {bytes(r[:12]): bytes(r) for s in c.steps[:j] for r in s[1]}
            grown += sum(ref.order.cardinal(jl.Vars.from_row(rows[h], ec.NOW)) != w for h, w in old.items())
        assert grown > 0

    for j in f.get("discriminates", ()):
        fed = ec.run_oracle(c, feed_bad=True)[0]
        assert (fed[-1]["stack"], fed[-1]["info"]["max_distance"]) != (recs[-1]["stack"], recs[-1]["info"]["max_distance"])
        assert fed[j]["info"]["postings_in"] == recs[j]["info"]["postings_in"] + len(c.steps[j][1])
        assert recs[j]["stack"] == _before(recs, j)  # the oracle of the case never saw it

    if "top_one_host" in f:
        m = f["top_one_host"]
        st = _urls_of(recs[0])
        assert len({u[6:12] for u in st[1:m + 1]}) == 1 and st[0][6:12] != st[1][6:12] != st[m + 1][6:12]
        third = recs[3]["pulled"][0][0]
        assert (third[6:12] == st[1][6:12]) == f["third_pull_same_host"]
    for j in f.get("empty_after", ()):
        assert recs[j]["stack"] == []
    for j, n in f.get("pulled_count", {}).items():
        assert len(recs[j]["pulled"]) == n
