"""Url hashes that share their first 64 key bits (a helper, no tests).

A url hash is a 72-bit key in Base64Order; the device stores it split: khi, the top 64 bits
(characters 0..9 and the upper four bits of character 10), and klo, the low 8 bits (the lower
two bits of character 10, and character 11).  Two keys that agree in khi are told apart by klo
alone -- the `ah == bh && al < bl` branch of every key compare on the device.  Every other
generator of the suite draws hashes whose first six characters differ, so that branch never
runs on them.  Here hashes come in *families*: one khi, 8 to 16 distinct klo.

families()          the hashes, ascending; the properties are asserted as they are built
rows()              valid rows (adv_rows "edge" cells) under given hashes
lists()             universe_lists over a family universe; in every list at least half of
                    the adjacent row pairs agree in khi (asserted)
union / lookup / distinct   the operations the device does on keys, with the key function as
                    a parameter: true_key (72 bits) or blind_key (khi only).  A test shows
                    on the CPU that an input separates the two; a kernel that compared khi
                    alone could then not pass on that input.
corpus() and the *_input functions: what tests/test_gpu_split_keys.py feeds the device, so that
tests/test_split_keys_ref.py can show the separation on exactly those inputs."""

import functools

import numpy as np

import java_literal as jl
from abstract_cases import peer_abstracts
from adv_rows import adv_rows, url_keys

KHI_EDGES = (0, 1, 2, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 2, (1 << 64) - 1)
KLO_EDGES = (0, 63, 64, 127, 128, 191, 192, 255)  # 0, 255 and both sides of character 10's two bits

SEED, N, FRACS = 72, 6000, (1.0, 0.7, 0.5, 0.3)
TERMS = [b"TERMspk%s____" % bytes([65 + j]) for j in range(len(FRACS))]  # A (every url) .. D
T257 = b"TERMspka____"   # a run of exactly 257 rows
TEXCL = b"TERMspkx____"  # of every second family some members, and siblings no other list has (the abstracts' exclusion list)


# ------------------------------------------------------------------ keys
def true_key(h) -> int:
    return jl.key72(bytes(h[:12]))


def blind_key(h) -> int:
    """what a compare of khi alone sees"""
    return jl.key72(bytes(h[:12])) >> 8


def split(h):
    k = true_key(h)
    return k >> 8, k & 255


def join(khi: int, klo: int) -> bytes:
    return jl.key_to_hash((khi << 8) | klo)


def by_family(hashes):
    """ascending hashes -> [[members of one khi]], in order"""
    out = []
    for h in hashes:
        if out and blind_key(out[-1][0]) == blind_key(h):
            out[-1].append(h)
        else:
            out.append([h])
    return out


# ------------------------------------------------------------------ the blind references
def union(sets, key=true_key):
    """the merged ascending set; of equal keys the first source's element is kept"""
    seen = {}
    for s in sets:
        for h in s:
            seen.setdefault(key(h), bytes(h[:12]))
    return [seen[k] for k in sorted(seen)]


def lookup(table, probes, key=true_key):
    """for every probe: is its key in the table"""
    t = {key(h) for h in table}
    return [key(p) in t for p in probes]


def distinct(hashes, key=true_key) -> int:
    return len({key(h) for h in hashes})


# ------------------------------------------------------------------ families
def family_table(seed: int, nfam: int):
    """[(khi, (klo, ...))] ascending by khi, Python ints throughout: the eight edge khi, then
    drawn ones over the whole 64-bit range, at least a quarter of them as pairs h, h + 1 with h
    even (equal in khi >> 1); every klo set holds KLO_EDGES and 0 to 8 random values more"""
    rng = np.random.default_rng([seed, nfam])
    ndrawn = nfam - len(KHI_EDGES)
    assert ndrawn >= 8
    draw = lambda: int.from_bytes(rng.bytes(8), "big")
    khis = set(KHI_EDGES)
    npair = -(-ndrawn // 6)
    while npair:
        h = draw() & ~1
        if h not in khis and h + 1 not in khis:
            khis |= {h, h + 1}
            npair -= 1
    while len(khis) < nfam:
        khis.add(draw())
    rest = np.array([k for k in range(256) if k not in KLO_EDGES])
    table = []
    for khi in sorted(khis):
        extra = rng.choice(rest, int(rng.integers(0, 9)), replace=False)
        table.append((khi, tuple(sorted(set(KLO_EDGES) | {int(k) for k in extra}))))
    return table


def neighbour_pairs(table):
    """the even khi h whose h + 1 has a family too"""
    have = {khi for khi, _ in table}
    return [khi for khi in sorted(have) if khi % 2 == 0 and khi + 1 in have]


def check_families(table, hashes):
    """the generator's properties (tests/test_split_keys_ref.py states them once more)"""
    khis = [khi for khi, _ in table]
    assert khis == sorted(set(khis)) and set(KHI_EDGES) <= set(khis)
    assert all(0 <= khi < 1 << 64 for khi in khis)
    ndrawn = len(khis) - len(KHI_EDGES)
    pairs = neighbour_pairs(table)
    drawn_in_pairs = sum(1 for khi in khis if khi not in KHI_EDGES and ((khi & ~1) in pairs))
    assert 4 * drawn_in_pairs >= ndrawn, (drawn_in_pairs, ndrawn)
    klos = dict(table)
    for h in pairs:  # the pairs share klo values: hi >> 1 equal, klo equal, bit 0 of khi apart
        assert len(set(klos[h]) & set(klos[h + 1])) >= 2
    for khi, ks in table:
        assert set(KLO_EDGES) <= set(ks) and 8 <= len(ks) <= 16 and len(set(ks)) == len(ks)
        assert all(0 <= k < 256 for k in ks)
    assert len(hashes) == sum(len(ks) for _, ks in table) == len(set(hashes))
    assert hashes == sorted(hashes, key=true_key)
    assert b"AAAAAAAAAAAA" in hashes and b"____________" in hashes
    assert all(split(h) == (khi, k) for h, (khi, k) in zip(hashes, ((khi, k) for khi, ks in table for k in ks)))
    if ndrawn >= 64:  # drawn over the whole range, not a corner of it
        assert {khi >> 61 for khi in khis} == set(range(8))


def families(seed: int, nfam: int):
    """ascending url hashes of nfam families (about 12 each)"""
    table = family_table(seed, nfam)
    hashes = [join(khi, k) for khi, ks in table for k in ks]
    check_families(table, hashes)
    return hashes


def hash_array(hashes) -> np.ndarray:
    return np.frombuffer(b"".join(bytes(h) for h in hashes), dtype=np.uint8).reshape(-1, 12)


def rows(hashes, seed: int) -> np.ndarray:
    """adv_rows' "edge" cells copied in under the given hashes: the same url carries different
    cells under different seeds"""
    r = adv_rows(len(hashes), seed, "edge")
    if len(hashes):
        r[:, :12] = hash_array(hashes)
    return r


def equal_khi_fraction(r: np.ndarray) -> float:
    """share of the adjacent row pairs that agree in khi"""
    if len(r) < 2:
        return 0.0
    hi, lo = url_keys(r)
    same = (hi[1:] == hi[:-1]) & ((lo[1:] >> 8) == (lo[:-1] >> 8))
    return float(same.mean())


def check_list(r: np.ndarray, name=b""):
    """the condition every list of the GPU module meets: ascending, and at least half of the adjacent
    pairs equal in khi -- without it a test could pass while exercising nothing"""
    hs = [bytes(x) for x in r[:, :12]]
    assert hs == sorted(set(hs), key=true_key), name
    assert equal_khi_fraction(r) >= 0.5, (name, equal_khi_fraction(r))


def lists(seed: int, n: int, fracs=FRACS, runs=()):
    """as adv_rows.universe_lists, over a universe of about n family hashes: list j keeps a url
    with probability fracs[j] and gives it cells of its own.  runs: for every length m a further
    list, a run of m consecutive urls of the universe."""
    uni = families(seed, max(16, n // 12))
    rng = np.random.default_rng([seed, n, 1])
    d = {}
    for j, frac in enumerate(fracs):
        d[b"TERMspk%s____" % bytes([65 + j])] = rows(uni, seed + 100 + j)[rng.random(len(uni)) < frac]
    for j, m in enumerate(runs):
        start = int(rng.integers(0, len(uni) - m))
        d[b"TERMspk%s____" % bytes([97 + j])] = rows(uni, seed + 200 + j)[start:start + m].copy()
    for h, r in d.items():
        check_list(r, h)
    return d


# ------------------------------------------------------------------ what the GPU module feeds the device
def selection(hashes, seed: int, known=()):
    """of every second family some members but not their siblings, and for every eighth family a
    sibling that `known` (and the family) does not hold -> (the selection, shuffled; the left-out
    siblings; the absent ones)"""
    rng = np.random.default_rng([seed, len(hashes)])
    known = set(known) | set(hashes)
    sel, left, ghosts = [], [], []
    for i, fam in enumerate(by_family(hashes)):
        if i % 2 or len(fam) < 2:
            continue
        m = rng.random(len(fam)) < 0.5
        j = int(rng.integers(len(fam)))
        m[j], m[(j + 1) % len(fam)] = True, False
        sel += [h for h, x in zip(fam, m) if x]
        left += [h for h, x in zip(fam, m) if not x]
        if i % 8 == 0:
            khi = blind_key(fam[0])
            g = next(join(khi, int(k)) for k in rng.permutation(256) if join(khi, int(k)) not in known)
            ghosts.append(g)
    out = sel + ghosts
    return [out[int(i)] for i in rng.permutation(len(out))], left, ghosts


@functools.lru_cache(maxsize=None)
def corpus():
    """the lists of the GPU module's shared index: A..D over one universe (A holds every url,
    more than 1,024 rows), a run of 257 rows, and the abstracts' exclusion list"""
    d = lists(SEED, N, FRACS, runs=(257,))
    uni = [bytes(x) for x in d[TERMS[0]][:, :12]]
    assert len(d[TERMS[0]]) > 1024 and len(d[T257]) == 257 and len(d[TERMS[0]]) <= 8000
    sel, _, _ = selection(uni, SEED + 2)
    d[TEXCL] = rows(sorted(sel, key=true_key), SEED + 300)
    check_list(d[TEXCL], TEXCL)
    return d


def universe():
    return [bytes(x) for x in corpus()[TERMS[0]][:, :12]]


def sibling_bytes_differ(r: np.ndarray) -> bool:
    """no two siblings of the list carry the same 28 feature bytes"""
    feats = {}
    for x in r:
        feats.setdefault(blind_key(x), []).append(bytes(x[12:]))
    return len(r) > 0 and all(len(set(v)) == len(v) for v in feats.values())


def heap_input(seed: int = SEED + 7):
    """-> (files: three lists of (term, rows), ram: {term: rows}).  Term 0, per family: the even
    members in file 1, the odd ones in file 2, a random overlap of both in file 3, a random subset
    in RAM; byte 33 tells the sources apart.  Term 1: in every family all of file 1's members below
    all of file 2's.  Term 2: file 2's record has no rows.  Term 3: records of one row, siblings
    of one another.  Records of 255, 256, 257 and 1 rows."""
    uni = universe()
    fams = by_family(uni)
    rng = np.random.default_rng(seed)
    base = rows(uni, seed)
    pos = {h: i for i, h in enumerate(uni)}

    def take(hs, tag):
        hs = sorted(hs, key=true_key)
        r = base[[pos[h] for h in hs]].copy()
        r[:, 33] = (r[:, 33].astype(int) + tag) % 256
        return r

    t = [b"TERMheap%d___" % i for i in range(4)]
    even = [h for fam in fams for h in fam[0::2]][:255]
    odd = [h for fam in fams for h in fam[1::2]][:256]
    both = even + odd
    over = [both[int(i)] for i in rng.choice(len(both), 257, replace=False)]
    inram = [h for h in uni[:700] if rng.random() < 0.3]
    f2 = fams[20:]  # (the terms overlap: their joins are not empty)
    low = [h for fam in f2 for h in fam[:len(fam) // 2]][:256]
    high = [h for fam in f2 for h in fam[len(fam) // 2:]][:255]
    run = uni[300:557]
    one = fams[7]
    files = [[(t[0], take(even, 1)), (t[1], take(low, 1)), (t[2], take(run, 1)), (t[3], take(one[:1], 1))],
             [(t[0], take(odd, 2)), (t[1], take(high, 2)), (t[2], take([], 2)), (t[3], take(one[1:2], 2))],
             [(t[0], take(over, 3)), (t[3], take(one[:1], 3))]]
    ram = {t[0]: take(inram, 0), t[3]: take(one[2:3], 0)}
    assert sorted(len(r) for f in files for _, r in f) == [0, 1, 1, 1, 255, 255, 256, 256, 257, 257]
    return files, ram


def abstract_input(seed: int = SEED + 11, npeers: int = 9):
    """-> (words, base, abstracts (word, peer, text) in shuffled arrival order, peers): three words
    over the urls of every fourth family; every peer holds a random 40 % of each word's urls
    (abstract_cases.peer_abstracts), so peers hold different siblings and several peers one url"""
    rng = np.random.default_rng(seed)
    urls = [h for fam in by_family(universe())[::4] for h in fam]
    words = sorted(b"WORDspk%d____" % i for i in range(3))
    base = {w: sorted(u for u in urls if rng.random() < 0.8) for w in words}
    abstracts, peers = peer_abstracts(rng, words, npeers, base)
    return words, base, abstracts, peers


def event_input(seed: int = SEED + 13, nfam: int = 150):
    """-> (arrivals [(rows, local)], never: siblings that arrive nowhere, pairs: [(a, b)] hashes
    of h / h + 1 neighbour families with equal klo that both arrive).  Over the first nfam families:
    every member goes to the local list, to remote arrival 1 or 2, or nowhere; arrival 1 repeats
    some of its own rows, arrival 3 draws from everything that arrived before (with repeats)."""
    uni = universe()
    fams = by_family(uni)[:nfam]
    rng = np.random.default_rng(seed)
    cls = {}
    for fam in fams:
        c = rng.integers(0, 4, len(fam))
        c[:4] = rng.permutation(4)  # every family: all three arrivals, and a member that never arrives
        for h, x in zip(fam, c):
            cls[h] = int(x)
    have = {blind_key(f[0]) for f in fams}
    pairs = []
    for khi in sorted(have):
        if khi % 2 == 0 and khi + 1 in have:
            for c, klo in ((0, 0), (1, 255), (2, 64)):  # equal klo on both sides, in each arrival
                a, b = join(khi, klo), join(khi + 1, klo)
                cls[a] = cls[b] = c
                pairs.append((a, b))
    for fam in fams:  # (the overrides may have taken a family's only absent member)
        if not any(cls[h] == 3 for h in fam):
            free = [h for h in fam if split(h)[1] not in (0, 255, 64)]
            cls[free[0]] = 3
    members = [h for fam in fams for h in fam]
    part = lambda c: [h for h in members if cls[h] == c]
    local = rows(part(0), seed + 1)
    r1 = rows(part(1), seed + 2)
    take = rng.permutation(len(r1))
    take = np.concatenate([take, take[rng.integers(0, len(take), len(take) // 4)]])  # twice in one arrival
    r1 = r1[take[rng.permutation(len(take))]]
    r2 = rows(part(2), seed + 3)
    r2 = r2[rng.permutation(len(r2))]
    seen = part(0) + part(1) + part(2)
    again = rows(seen, seed + 4)[rng.integers(0, len(seen), 400)]  # once more, later, other cells
    arrivals = [(local, True), (r1, False), (r2, False), (again, False)]
    assert 1500 <= sum(len(r) for r, _ in arrivals) <= 2500
    return arrivals, part(3), pairs


def order_input(seed: int = SEED + 17):
    """-> (run: 600 consecutive rows of the universe whose rows 100 / 101 and 255 / 256 are siblings,
    [(i, the run with rows i and i + 1 swapped, the run with row i twice)] for i = 100 and 255)"""
    uni = universe()
    sib = lambda i, j: blind_key(uni[i]) == blind_key(uni[j])
    s = next(s for s in range(100, 1000) if sib(s + 100, s + 101) and sib(s + 255, s + 256))
    run = rows(uni[s:s + 600], seed)
    check_list(run)
    bad = []
    for i in (100, 255):
        swapped = run.copy()
        swapped[[i, i + 1]] = swapped[[i + 1, i]]
        bad.append((i, swapped, np.concatenate([run[:i + 1], run[i:]])))
    return run, bad


def dictionary_input(seed: int = SEED + 19):
    """-> (base: the lists A..D without the held-out urls, sibl: a list of the held-out urls alone --
    siblings of keys the base has, below, between and above their family's present members --,
    known: a list of urls the base has, where: how many of each position)"""
    d = corpus()
    held, where = set(), {"below": 0, "between": 0, "above": 0}
    for i, fam in enumerate(by_family(universe())):
        if i % 2:
            continue
        n = len(fam)
        take = ([0, 1], [n - 2, n - 1], [n // 2, n // 2 + 1], [0, 1, n // 2, n - 1])[(i // 2) % 4]
        held |= {fam[j] for j in take}
        rest = [true_key(h) for j, h in enumerate(fam) if j not in take]
        for j in take:  # from the keys alone: where the new key lies among its family's present members
            k = true_key(fam[j])
            where["below" if k < min(rest) else "above" if k > max(rest) else "between"] += 1
    base = {t: d[t][[bytes(x) not in held for x in d[t][:, :12]]] for t in TERMS}
    for t, r in base.items():
        check_list(r, t)
    present = [bytes(x) for x in base[TERMS[0]][:, :12]]
    sibl = rows(sorted(held, key=true_key), seed)
    known = rows([h for fam in by_family(present)[::9] for h in fam], seed + 1)
    return base, sibl, known, where
