"""CPU checks behind tests/test_gpu_heap_loader.py: the directed inputs of tests/heap_cases.py are
what they claim to be (a case that is not of its class tests nothing), and the loader's rules as
oracle/heap.py states them (validate=True, scan_stats, load_reference) give hand-derived
results.  No GPU."""

import struct

import numpy as np
import pytest

import heap
import heap_cases as hc
import oracle as orc

NOW = 20741 * 86400000 + 4242
INF = 2147483647


def _ref(load, tmp_path, shard=(0, 1), ram=None):
    paths = hc.write_files(load, tmp_path)
    return heap.load_reference(paths, load.ram if ram is None else ram, shard)


def _tags(r):
    return [int(x) for x in r[:, 33]]


# ------------------------------------------------------------------ union_pairs
def test_union_cases_are_of_their_class():
    cases = hc.union_pairs().info["cases"]
    c = {name: hc.pair_class(a, b) for name, _, a, b in cases}
    assert len({t for _, t, _, _ in cases}) == len(cases) == 11 + len(hc.SIZE_PAIRS) + 1
    x = c["below"]
    assert x["shared"] == 0 and x["below"] == x["nb"] == 40 and x["above"] == 0
    x = c["above"]
    assert x["shared"] == 0 and x["above"] == x["nb"] == 40 and x["below"] == 0
    x = c["alternate"]  # a b a b ... a b
    assert x["shared"] == 0 and x["na"] == x["nb"] == 40 and (x["below"], x["above"]) == (0, 1)
    _, _, a, b = next(k for k in cases if k[0] == "alternate")
    merged = sorted([(heap.key_order(bytes(h)), 0) for h in a] + [(heap.key_order(bytes(h)), 1) for h in b])
    assert [s for _, s in merged] == [0, 1] * 40
    x = c["b_in_a"]  # kept == 0
    assert x["shared"] == x["nb"] == 20 and x["na"] == 60
    x = c["a_in_b"]
    assert x["shared"] == x["na"] == 20 and x["nb"] == 60
    x = c["equal"]
    assert x["shared"] == x["na"] == x["nb"] == 50 and x["slots_a"] == x["slots_b"] == list(range(50))
    assert (c["one_equal"]["na"], c["one_equal"]["nb"], c["one_equal"]["shared"]) == (1, 1, 1)
    assert (c["one_above"]["na"], c["one_above"]["nb"], c["one_above"]["shared"], c["one_above"]["above"]) == (1, 1, 0, 1)
    assert (c["one_below"]["na"], c["one_below"]["nb"], c["one_below"]["shared"], c["one_below"]["below"]) == (1, 1, 0, 1)
    x = c["dup_first"]
    assert x["slots_a"] == x["slots_b"] == [0] and x["na"] == x["nb"] == 40
    x = c["dup_last"]
    assert x["slots_a"] == [x["na"] - 1] and x["slots_b"] == [x["nb"] - 1] and x["na"] == x["nb"] == 40
    for na, nb in hc.SIZE_PAIRS:
        x = c["size_%d_%d" % (na, nb)]
        assert (x["na"], x["nb"], x["shared"]) == (na, nb, (min(na, nb) + 1) // 2)
        if min(na, nb) > 1:  # interleaved: neither list lies to one side, shared rows at both ends
            assert x["below"] < 40 and x["above"] < 40
            assert min(x["slots_b"]) < nb // 4 and max(x["slots_b"]) > 3 * nb // 4
    # each of the three kernels has its grid edge (256 threads) on one side at least once
    assert {na for na, _ in hc.SIZE_PAIRS} >= {1, 255, 256, 257, 512, 513}
    assert {nb for _, nb in hc.SIZE_PAIRS} >= {1, 255, 256, 257, 512, 513}


def test_union_last_two_characters():
    _, _, a, b = next(k for k in hc.union_pairs().info["cases"] if k[0] == "last_two")
    ka, kb = [bytes(h) for h in a], [bytes(h) for h in b]
    shared = sorted(set(ka) & set(kb), key=heap.key_order)
    assert len(shared) == 80 and len(ka) == 220 and len(kb) == 160
    both = sorted(set(ka) | set(kb), key=heap.key_order)
    for h in shared:
        i = both.index(h)
        lo, hi = both[i - 1], both[i + 1]
        assert lo[:10] == h[:10] == hi[:10] and lo != h != hi
        assert {lo in ka and lo not in kb, hi in ka and hi not in kb} == {True, False}  # one neighbour in each list alone
    # some shared hashes differ from a neighbour in the key's low byte alone, some in the high part
    lut = heap._LUT
    khi = lambda h: tuple(lut[list(h[:10])]) + (lut[h[10]] >> 2,)
    same_hi = [khi(h) == khi(both[both.index(h) + d]) for h in shared for d in (-1, 1)]
    assert any(same_hi) and not all(same_hi)


# ------------------------------------------------------------------ precedence
def test_precedence_owner_sets(tmp_path):
    load = hc.precedence()
    sets = [hc.owners(i) for i in range(hc.PREC_URLS)]
    count = {}
    for s in sets:
        count[s] = count.get(s, 0) + 1
    assert len(count) == 31 and all(v >= 20 for v in count.values()) and () not in count
    # the files and RAM hold exactly what the owner sets say
    held = [set(hc.keys(f[hc.PREC])) for f in hc.file_rowsets(load)] + [set(hc.keys(load.ram[hc.PREC]))]
    uni = hc.keys(hc.rows(np.arange(hc.PREC_URLS), 0))
    for i, h in enumerate(uni):
        assert tuple(s for s in range(hc.SOURCES) if h in held[s]) == sets[i]
    lists, st, rep = _ref(load, tmp_path)
    got = lists[hc.PREC]
    assert hc.keys(got) == uni and _tags(got) == load.info["tags"]
    assert set(load.info["tags"]) == {1, 2, 3, 4, hc.RAM_TAG}
    assert rep["dropped"] == {} and st["terms"] == 2


# ------------------------------------------------------------------ unsorted tails
def test_unsorted_tails(tmp_path):
    load = hc.unsorted_tails()
    lists, st, rep = _ref(load, tmp_path)
    assert rep["dropped"] == {} and len(load.info["expect"]) == 6 == st["terms"]
    for t, (h, tags) in load.info["expect"].items():
        assert hc.keys(lists[t]) == [bytes(x) for x in h], t
        assert _tags(lists[t]) == list(tags), t
    # the inputs are what they say: orderbound below size, the tail really out of order
    f1 = dict(load.files[1])
    for t, blob in f1.items():
        size, ob = struct.unpack_from(">i", blob, 0)[0], struct.unpack_from(">i", blob, 10)[0]
        r = np.frombuffer(blob, np.uint8, offset=14).reshape(-1, 40)
        assert ob < size == len(r) and hc.ascending(r[:ob]) and not hc.ascending(r), t
    size = lambda t: struct.unpack_from(">i", f1[hc.tail_term(t)], 0)[0]
    ob = lambda t: struct.unpack_from(">i", f1[hc.tail_term(t)], 10)[0]
    assert ob(b"ob0") == 0 and size(b"one") - ob(b"one") == 1 and size(b"desc300") - ob(b"desc300") == 300
    # without the validation the same lists come out (no rowset here has a fault)
    assert {t: v.tobytes() for t, v in heap.index_get(hc.write_files(load, tmp_path), load.ram).items()} == \
        {t: v.tobytes() for t, v in lists.items()}


# ------------------------------------------------------------------ rejects
def test_reject_cases_trip_their_own_cause(tmp_path):
    load = hc.rejects()
    causes, where = load.info["causes"], load.info["where"]
    assert sorted(set(causes.values())) == ["hash", "language", "order", "space"] and len(causes) == 10
    for f, recs in enumerate(load.files):
        for t, blob in recs:
            faults = heap.rowset_faults(blob)
            if t in causes and where[t] == f:
                assert faults == (causes[t],), (t, f, faults)
            else:
                assert faults == (), (t, f, faults)
    lists, st, rep = _ref(load, tmp_path)
    assert rep["dropped"] == {t: (c,) for t, c in causes.items()}
    assert st["dropped_terms"] == 10 and st["terms"] == 1 and rep["stored"] == [hc.HEALTHY]
    for t in causes:
        assert lists[t].tobytes() == load.ram[t].tobytes(), t
    got = lists[hc.HEALTHY]
    assert set(_tags(got)) == {1, 2, 3, hc.RAM_TAG} and st["postings"] == len(got)
    # the placement the issue names: first row, last row, character 11 alone, a middle row
    rs = hc.file_rowsets(load)
    bad = lambda t: np.argwhere(heap._LUT[rs[where[hc.rej_term(t)]][hc.rej_term(t)][:, :12]] < 0).tolist()
    assert bad(b"hashfirst")[0][0] == 0 and len(bad(b"hashfirst")) == 1
    assert bad(b"hashlast") == [[39, 0]] and bad(b"hash11") == [[17, 11]]
    r = rs[1][hc.rej_term(b"lang")]
    assert np.argwhere((r[:, 22] == 0) & (r[:, 23] == 0)).tolist() == [[20]] and len(r) == 40
    assert where[hc.rej_term(b"newest")] == 2 and where[hc.rej_term(b"space")] == 1
    for t in (b"newest", b"space"):
        assert [hc.rej_term(t) in f for f in rs] == [True, True, True]


def test_drop_rule_by_hand(tmp_path):
    """the rules of validate=True one by one, as test_heap.test_import_rules does for the import"""
    ar = np.arange
    ok = hc.rows(ar(5), 1)
    assert heap.row_faults(ok, True) == () and heap.row_faults(ok[::-1], False) == ()
    assert heap.row_faults(ok[::-1], True) == ("order",)
    assert heap.row_faults(ok[[0, 1, 1, 2]], True) == ("order",) and heap.row_faults(ok[[0, 1, 1, 2]], False) == ()
    z = ok.copy()
    z[2, 22:24] = 0
    assert heap.row_faults(z, True) == heap.row_faults(z, False) == ("language",)
    z[2, 23] = 1  # one zero byte is a language
    assert heap.row_faults(z, True) == ()
    h = ok.copy()
    h[4, 11] = ord("=")
    assert heap.row_faults(h, True) == heap.row_faults(h, False) == ("hash",)
    h[0, 22:24] = 0
    assert heap.row_faults(h[::-1], True) == ("hash", "language", "order")
    assert heap.rowset_faults(heap.export_collection(ok, size=6)) == ("space",)
    assert heap.rowset_faults(b"short") == () == heap.rowset_faults(heap.export_collection(ok[::-1], size=-1 & 0xFFFFFFFF))
    # orderbound >= size claims sorted; below it the rows are sorted, not rejected
    assert heap.rowset_faults(heap.export_collection(ok[::-1], orderbound=9)) == ("order",)
    assert heap.rowset_faults(heap.export_collection(ok[::-1], orderbound=4)) == ()
    # through index_get: the faulty term keeps its RAM list, validate off keeps today's result
    T1, T2 = b"termAAAAAAAA", b"termBBBBBBBB"
    p0, p1 = hc.path_of(tmp_path, 0), hc.path_of(tmp_path, 1)
    heap.write_heap(p0, [(T1, heap.export_collection(ok)), (T2, heap.export_collection(ok))])
    heap.write_heap(p1, [(T1, heap.export_collection(hc.rows(ar(9, 3, -1), 2)))])
    ram = {T1: hc.rows([2, 20], hc.RAM_TAG)}
    rep = {}
    got = heap.index_get([p0, p1], ram, validate=True, report=rep)
    assert got[T1].tobytes() == ram[T1].tobytes() and got[T2].tobytes() == ok.tobytes()
    assert rep == {"dropped": {T1: ("order",)}, "stored": [T2]}
    rep = {}
    off = heap.index_get([p0, p1], ram, report=rep)
    assert rep == {"dropped": {}, "stored": [T1, T2]}
    assert _tags(off[T1]) == [1] * 5 + [2] * 5 + [hc.RAM_TAG] and off[T1].tobytes() == heap.index_get([p0, p1], ram)[T1].tobytes()
    lists, st, _ = heap.load_reference([p0, p1], ram)
    assert st == {"files": 2, "records": 3, "free_records": 0, "bad_keys": 0, "terms": 1, "postings": 5, "dropped_terms": 1}


# ------------------------------------------------------------------ records
def test_record_image(tmp_path):
    load = hc.records()
    paths = hc.write_files(load, tmp_path)
    assert [len(open(p, "rb").read()) for p in paths[:2]] == [0, 15]
    assert heap.scan_stats(paths) == load.info["counters"]
    per_file = [heap.scan_stats([p]) for p in paths]
    assert [s["records"] for s in per_file] == [0, 0, 9, 2, 2]
    # not cut short by accident: the record before each file's ending is accepted
    T = hc.rec_term
    assert T(b"after") in heap.scan_heap(paths[2]) and T(b"space") in heap.scan_heap(paths[4])
    assert sorted(heap.scan_heap(paths[3])) == sorted([T(b"small"), T(b"space")])
    assert T(b"unseen") not in heap.scan_heap(paths[4]) and T(b"unseen") in load.files[4]
    lists, st, rep = heap.load_reference(paths, load.ram)
    assert {t: _tags(r) for t, r in lists.items()} == load.info["lists"]
    assert not any(t in lists for t in load.info["absent"])
    assert sorted(rep["dropped"]) == load.info["dropped"] and rep["dropped"][T(b"space")] == ("space",)
    assert st["terms"] == load.info["stored"] == 5 and st["postings"] == 9 + 4 * 6 and st["dropped_terms"] == 1
    assert heap.order_files(list(reversed(paths))) == paths


# ------------------------------------------------------------------ reload, big list
def test_reload_inputs(tmp_path):
    for n in (300, 4200):
        first, second = hc.reload(n)
        da, db = tmp_path / ("a%d" % n), tmp_path / ("b%d" % n)
        da.mkdir()
        db.mkdir()
        l1, st1, _ = _ref(first, da)
        p2 = hc.write_files(second, db)
        l2, st2, _ = heap.load_reference(p2, l1)
        assert sorted(l1) == hc.REL[:2] and sorted(l2) == hc.REL and st2["terms"] == 3
        for t in hc.REL[:2]:
            k1, k2 = hc.keys(l1[t]), hc.keys(l2[t])
            new = dict(second.files[0])
            file2 = set(hc.keys(np.frombuffer(new[t], np.uint8, offset=14).reshape(-1, 40)))
            assert set(k1) < set(k2) and file2 & set(k1) and file2 - set(k1)  # overlaps and adds
            won = [int(r[33]) for r in l2[t] if bytes(r[:12]) in file2]
            assert won and set(won) == {3}  # the newer file wins over what was loaded before
            assert {1, 2, hc.RAM_TAG} <= set(_tags(l1[t]))
            assert hc.ascending(l2[t])
        assert len(l1[hc.REL[0]]) >= n


def test_big_list_spans_three_pieces():
    piece = 16 << 20
    assert piece % 40 != 0 and hc.BIG_ROWS * 40 > 2 * piece and (hc.BIG_ROWS * 40 - 1) // piece == 2
    r = hc.big_rows()
    assert r.shape == (hc.BIG_ROWS, 40)
    k0, k1 = heap._keys(r)
    assert ((k0[:-1] < k0[1:]) | ((k0[:-1] == k0[1:]) & (k1[:-1] < k1[1:]))).all()
    assert heap.row_faults(r, True) == ()


# ------------------------------------------------------------------ shard input
@pytest.mark.parametrize("world", [2, 4])
def test_shard_input_conditions(world, tmp_path):
    load = hc.shard_input()
    rs = hc.file_rowsets(load)
    for f in rs:
        for t, r in f.items():
            assert heap.row_faults(r, True) == (), t
    firsts = {bytes([c]) for f in rs for r in f.values() for c in r[:, 0]} | \
        {bytes([c]) for r in load.ram.values() for c in r[:, 0]}
    assert firsts == {bytes([c]) for c in hc.FIRST_CHARS}
    part = lambda r: sorted({int(x) for x in heap._LUT[r[:, 0]] >> (6 - (world.bit_length() - 1))})
    every = list(range(world))
    # 0: wholly inside one quarter
    a = [r for f in rs for t, r in f.items() if t == hc.SH[0]] + [load.ram[hc.SH[0]]]
    assert all(part(r) == [1 if world == 4 else 0] for r in a)
    # 1: rows in every quarter, in every file and in RAM
    assert all(part(f[hc.SH[1]]) == every for f in rs) and part(load.ram[hc.SH[1]]) == every
    # 2: the files hold nothing in the last rank's range, RAM does
    assert all(world - 1 not in part(f[hc.SH[2]]) for f in rs if hc.SH[2] in f)
    assert world - 1 in part(load.ram[hc.SH[2]])
    # 3: for the last rank the range is the whole rowset (row 0 to row n), for 0 it is empty
    assert all(part(f[hc.SH[3]]) == [world - 1] for f in rs if hc.SH[3] in f)
    # the shards' expectations together are the unsharded one, and the cut RAM changes nothing
    paths = hc.write_files(load, tmp_path)
    whole, _, _ = heap.load_reference(paths, load.ram)
    parts = []
    for rank in range(world):
        ram = {t: hc.shard_of(r, rank, world) for t, r in load.ram.items()}
        lists, st, rep = heap.load_reference(paths, ram, (rank, world))
        assert {t: v.tobytes() for t, v in lists.items()} == \
            {t: v.tobytes() for t, v in heap.index_get(paths, load.ram, (rank, world)).items()}
        assert rep["dropped"] == {}
        parts.append(lists)
        if rank == world - 1:
            assert hc.SH[2] in lists and hc.SH[2] not in rep["stored"]  # RAM rows only: not a stored list
            assert _tags(lists[hc.SH[2]]) == [hc.RAM_TAG] * 14
        if rank == 0:
            assert hc.SH[3] not in lists
    for t, r in whole.items():
        got = np.concatenate([p[t] for p in parts if t in p])
        assert got.tobytes() == r.tobytes(), t


# ------------------------------------------------------------------ every expected list, and the queries
def test_expected_lists_ascend_and_queries_hit(tmp_path):
    loads = {"union": hc.union_pairs(), "precedence": hc.precedence(), "tails": hc.unsorted_tails(),
             "rejects": hc.rejects(), "records": hc.records(), "shard": hc.shard_input()}
    for name, load in loads.items():
        d = tmp_path / name
        d.mkdir()
        lists, st, _ = _ref(load, d)
        assert lists, name
        for t, r in lists.items():
            assert hc.ascending(r), (name, t)
        assert st["postings"] <= sum(len(r) for r in lists.values())
        if name in ("union", "precedence"):
            terms = [t for _, t, _, _ in load.info["cases"]] if name == "union" else [hc.PREC, hc.PREC_MATE]
            qs = hc.query_pairs(lists, terms)
            assert len(qs) == 2 * len(terms)
            for inc, exc in qs:
                assert len(inc) + len(exc) == 2
                assert len(orc.search(lists, inc, exc, now_ms=NOW, k=50)) > 0, (inc, exc)


def test_union_expectations(tmp_path):
    """the reference on the union cases against plain set arithmetic: A's row on shared hashes"""
    load = hc.union_pairs()
    lists, st, _ = _ref(load, tmp_path)
    for name, t, a, b in load.info["cases"]:
        ka, kb = {bytes(h) for h in a}, {bytes(h) for h in b}
        exp = sorted(ka | kb, key=heap.key_order)
        assert hc.keys(lists[t]) == exp, name
        assert _tags(lists[t]) == [1 if h in ka else 2 for h in exp], name
    assert st["terms"] == len(load.info["cases"]) and st["files"] == 2
