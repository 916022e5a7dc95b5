"""CPU side of the split-key parity tests (tests/split_keys.py, tests/test_gpu_split_keys.py).

Generator properties: families of url hashes that agree in their first 64 key bits (khi) and
differ in the last 8 (klo), at the edge values of both.

Discrimination: for every input the GPU module feeds to a key-comparing path, the operation done
with keys compared on khi alone (split_keys.blind_key) gives another answer than the true one.
A kernel whose low-byte compare were wrong could therefore not pass on that input -- shown here
without ever running wrong device code."""

import numpy as np

import abstracts as ab
import adv_rows
import java_literal as jl
import split_keys as sk
import update_ref as ur


def test_generator_properties():
    for seed, nfam in ((1, 128), (sk.SEED, sk.N // 12)):
        table = sk.family_table(seed, nfam)
        hashes = sk.families(seed, nfam)
        assert sk.families(seed, nfam) == hashes  # deterministic
        sk.check_families(table, hashes)
        khis = [khi for khi, _ in table]
        assert len(khis) == nfam
        for e in (0, 1, 2, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 2, 2 ** 64 - 1):
            assert e in khis
        assert hashes[0] == b"AAAAAAAAAAAA" and hashes[-1] == b"____________"
        pairs = sk.neighbour_pairs(table)
        drawn = [k for k in khis if k not in sk.KHI_EDGES]
        assert 4 * sum(1 for k in drawn if (k & ~1) in set(pairs)) >= len(drawn)
        assert all(h % 2 == 0 and (h >> 1) == ((h + 1) >> 1) for h in pairs)
        for khi, ks in table:
            assert {0, 63, 64, 127, 128, 191, 192, 255} <= set(ks) and 8 <= len(ks) <= 16
        assert max(khis) > 2 ** 63 > min(k for k in khis if k > 2)  # Python ints: no int64 wrap
        # character 10 carries both: its upper four bits belong to khi, its lower two to klo
        fam = sk.by_family(hashes)[3]
        assert len({h[:10] for h in fam}) == 1 and len({h[10:] for h in fam}) == len(fam)
        assert len({jl.AHPLA[h[10]] >> 2 for h in fam}) == 1 and len({jl.AHPLA[h[10]] & 3 for h in fam}) == 4
        # the three orders of the suite agree on them
        assert sorted(hashes, key=ur.url_key) == hashes
        k72 = [jl.key72(h) for h in hashes]
        assert all(a < b for a, b in zip(k72, k72[1:]))
        r = sk.rows(hashes, 5)
        hi, lo = adv_rows.url_keys(r)
        assert [(int(a) << 36) | int(b) for a, b in zip(hi, lo)] == k72
        assert np.array_equal(adv_rows.sort_rows(r[::-1]), r)
        assert [sk.split(h) for h in hashes] == [(khi, k) for khi, ks in table for k in ks]


def test_rows_and_lists():
    d = sk.corpus()
    uni = sk.universe()
    assert list(d)[:4] == sk.TERMS and len(d[sk.TERMS[0]]) == len(uni) > 1024 and len(d[sk.T257]) == 257
    for h, r in d.items():
        sk.check_list(r, h)
        assert sk.equal_khi_fraction(r) >= 0.5
        assert (r[:, 22:24] != 0).any(axis=1).all()  # a language: the rows are valid
    # the same url carries different cells in different lists
    a, b = d[sk.TERMS[0]], d[sk.TERMS[1]]
    pos = {bytes(x[:12]): i for i, x in enumerate(a)}
    assert sum(bytes(a[pos[bytes(x[:12])], 12:]) != bytes(x[12:]) for x in b) > 0.99 * len(b)
    # siblings differ in their feature bytes: a row returned for a sibling would be seen
    for t in sk.TERMS:
        assert sk.sibling_bytes_differ(d[t])
    # a list that is not family-dense fails the condition (the check can fail)
    sparse = adv_rows.adv_rows(300, 1)
    assert sk.equal_khi_fraction(sparse) == 0.0


def test_blind_references_on_a_hand_case():
    a, b, c = sk.join(5, 1), sk.join(5, 2), sk.join(6, 1)
    assert sk.union([[a, c], [b]]) == [a, b, c] and sk.union([[a, c], [b]], sk.blind_key) == [a, c]
    assert sk.lookup([a], [a, b, c]) == [True, False, False]
    assert sk.lookup([a], [a, b, c], sk.blind_key) == [True, True, False]
    assert sk.distinct([a, b, c]) == 3 and sk.distinct([a, b, c], sk.blind_key) == 2


def _hashes(r):
    return [bytes(x) for x in r[:, :12]]


def test_discrimination_heap_records():
    files, ram = sk.heap_input()
    terms = sorted({t for f in files for t, _ in f})
    assert len(terms) == 4
    for t in terms:
        sources = [_hashes(r) for f in files for tt, r in f if tt == t] + ([_hashes(ram[t])] if t in ram else [])
        true, blind = sk.union(sources), sk.union(sources, sk.blind_key)
        assert len(blind) < len(true), t
    # term 0: even against odd members; term 1: one side below the other inside a family
    (_, even), (_, low) = files[0][0], files[0][1]
    (_, odd), (_, high) = files[1][0], files[1][1]
    assert set(map(sk.blind_key, _hashes(even))) & set(map(sk.blind_key, _hashes(odd)))
    shared = set(map(sk.blind_key, _hashes(low))) & set(map(sk.blind_key, _hashes(high)))
    assert len(shared) > 10
    for khi in shared:
        assert max(sk.true_key(h) for h in _hashes(low) if sk.blind_key(h) == khi) < \
            min(sk.true_key(h) for h in _hashes(high) if sk.blind_key(h) == khi)
    # the file that is read first wins: an overlap whose telling byte differs
    over = dict(zip(_hashes(files[2][0][1]), files[2][0][1][:, 33]))
    first = dict(zip(_hashes(even) + _hashes(odd), list(even[:, 33]) + list(odd[:, 33])))
    assert all(h in first for h in over) and all(first[h] != v for h, v in over.items())


def test_discrimination_selections():
    uni = sk.universe()
    d = sk.corpus()
    for seed in (sk.SEED + 3, sk.SEED + 4):  # the url selection and the doublecheck set of the GPU module
        sel, left, ghosts = sk.selection(uni, seed)
        assert left and ghosts and not set(ghosts) & set(uni) and not set(left) & set(sel)
        for t in sk.TERMS + [sk.T257]:
            hs = _hashes(d[t])
            true, blind = sk.lookup(sel, hs), sk.lookup(sel, hs, sk.blind_key)
            assert true != blind and sum(blind) > sum(true) > 0, t
        # the absent siblings: found by a khi-only search, not by the true one
        assert not any(sk.lookup(uni, ghosts)) and all(sk.lookup(uni, ghosts, sk.blind_key))
    # the abstracts' exclusion list
    ex = _hashes(d[sk.TEXCL])
    for t in sk.TERMS[:2]:
        hs = _hashes(d[t])
        assert sum(sk.lookup(ex, hs, sk.blind_key)) > sum(sk.lookup(ex, hs)) > 0


def test_discrimination_abstract_texts():
    words, base, abstracts, peers = sk.abstract_input()
    assert len(words) == 3 and len(peers) == 9
    held = {}
    for w, p, text in abstracts:
        urls = list(ab.decompress_index(text, p))
        held.setdefault(w, {})[p] = urls
        assert sk.distinct(urls, sk.blind_key) < sk.distinct(urls) == len(urls)
    for w in words:
        every = [u for p in held[w] for u in held[w][p]]
        assert sk.distinct(every, sk.blind_key) < sk.distinct(every) < len(every)  # several peers hold one url
        a, b = held[w][peers[0]], held[w][peers[1]]
        assert sk.lookup(a, b) != sk.lookup(a, b, sk.blind_key)  # peers hold different siblings
    # the join over the words: larger when siblings count as one url
    u = [[u for p in held[w] for u in held[w][p]] for w in words]
    true = set(map(sk.true_key, u[0])) & set(map(sk.true_key, u[1])) & set(map(sk.true_key, u[2]))
    blind = set(map(sk.blind_key, u[0])) & set(map(sk.blind_key, u[1])) & set(map(sk.blind_key, u[2]))
    assert len(true) > len(blind) > 0 and any(sk.distinct(f) > 1 for f in sk.by_family(sorted(
        (jl.key_to_hash(k) for k in true), key=sk.true_key)))


def test_discrimination_event_arrivals():
    arrivals, never, pairs = sk.event_input()
    assert arrivals[0][1] and not any(local for _, local in arrivals[1:])
    sk.check_list(arrivals[0][0], b"local")
    total = sum(len(r) for r, _ in arrivals)
    assert 1500 <= total <= 2500
    sets = [_hashes(r) for r, _ in arrivals]
    every = [h for s in sets for h in s]
    assert sk.distinct(every, sk.blind_key) < sk.distinct(every)
    # siblings arrive in different arrivals: a khi-only url set would refuse the later ones
    for later in (1, 2):
        before = [h for s in sets[:later] for h in s]
        true, blind = sk.lookup(before, sets[later]), sk.lookup(before, sets[later], sk.blind_key)
        assert not any(true) and sum(blind) > len(blind) // 2
    # the same hash twice in one arrival, and again in a later one
    assert len(set(sets[1])) < len(sets[1])
    assert set(sets[3]) <= set(sets[0] + sets[1] + sets[2]) and len(set(sets[3])) < len(sets[3])
    # siblings that never arrive: in no arrival, though a khi-only search finds them
    assert never and not any(sk.lookup(every, never)) and all(sk.lookup(every, never, sk.blind_key))
    # h / h + 1 neighbours with equal klo both arrive: equal in khi >> 1 and in klo
    assert len(pairs) >= 3
    for a, b in pairs:
        (ha, la), (hb, lb) = sk.split(a), sk.split(b)
        assert ha + 1 == hb and ha % 2 == 0 and la == lb and a in every and b in every


def test_discrimination_order_and_dictionary():
    """put_list's ordering check and the incremental dictionary's lookups"""
    run, bad = sk.order_input()
    strictly = lambda hs, key: all(key(a) < key(b) for a, b in zip(hs, hs[1:]))
    rising = lambda hs, key: all(key(a) <= key(b) for a, b in zip(hs, hs[1:]))
    assert strictly(_hashes(run), sk.true_key) and not strictly(_hashes(run), sk.blind_key)
    assert [i for i, _, _ in bad] == [100, 255]
    for i, swapped, twice in bad:
        # by khi alone the swapped list still rises (and a strict check would refuse the rows in order)
        assert not rising(_hashes(swapped), sk.true_key) and rising(_hashes(swapped), sk.blind_key)
        assert rising(_hashes(twice), sk.true_key) and not strictly(_hashes(twice), sk.true_key)
        assert len(twice) == len(run) + 1 and len(swapped) == len(run)
    base, sibl, known, where = sk.dictionary_input()
    present = _hashes(base[sk.TERMS[0]])
    assert min(where.values()) > 50 and sum(where.values()) == len(sibl)
    assert not any(sk.lookup(present, _hashes(sibl))) and all(sk.lookup(present, _hashes(sibl), sk.blind_key))
    assert all(sk.lookup(present, _hashes(known)))
    assert sk.distinct(present + _hashes(sibl), sk.blind_key) == sk.distinct(present, sk.blind_key)
    assert sk.distinct(present + _hashes(sibl)) == len(present) + len(sibl) == len(sk.universe())
    sk.check_list(sibl, b"sibl")
    sk.check_list(known, b"known")
