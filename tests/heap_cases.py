"""Directed inputs of the heap loader (yrwi_load_heaps): a helper, no tests.

Every function returns a Load: heap files oldest first (a list of (term, exported rowset)
records that heap.write_heap writes, or a file image as bytes), the lists the context holds
before the call (the RAM cache), and what the case claims about itself.  tests/
test_heap_cases_ref.py checks those claims on the CPU, tests/test_gpu_heap_loader.py runs every
Load through the library against oracle/heap.py.  Everything is built with numpy alone and is
the same on every run.  Byte 33 of a row tells its source: file f writes tag f + 1 (or what the
case says), RAM writes RAM_TAG; the language cell is "en" unless the case says otherwise."""

import functools
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Tuple, Union

import numpy as np

import heap

ROW = heap.ROW
RAM_TAG = 9
SOURCES = 5  # precedence(): four files and RAM
_ALPHA = np.frombuffer(heap.ALPHA, dtype=np.uint8)
FIRST_CHARS = b"APQfgvw_"  # alphabet indices 0 15 | 16 31 | 32 47 | 48 63: the edges of the halves and quarters


@dataclass
class Load:
    files: List[Union[bytes, List[Tuple[bytes, bytes]]]]
    ram: Dict[bytes, np.ndarray] = field(default_factory=dict)
    info: dict = field(default_factory=dict)


def path_of(directory, f: int) -> str:
    return str(directory) + "/text.index.%017d.blob" % (20240101000000000 + 1000 * f)


def write_files(load: Load, directory) -> List[str]:
    """the Load's files under `directory`, stamped in their order -> paths, oldest first"""
    paths = []
    for f, spec in enumerate(load.files):
        p = path_of(directory, f)
        if isinstance(spec, bytes):
            with open(p, "wb") as fh:
                fh.write(spec)
        else:
            heap.write_heap(p, spec)
        paths.append(p)
    return paths


# ------------------------------------------------------------------ rows
def hashes(idx, first=None) -> np.ndarray:
    """(n, 12) url hashes, ascending in idx (< 2^30): characters 0..5 spell idx, 6..11 a mix of
    it; `first` (a byte or n bytes) replaces character 0, which is 'A' otherwise"""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    lo = (idx * 2654435761 + 12345) & ((1 << 36) - 1)
    out = np.empty((len(idx), 12), dtype=np.uint8)
    for j in range(6):
        out[:, j] = _ALPHA[(idx >> (6 * (5 - j))) & 63]
        out[:, 6 + j] = _ALPHA[(lo >> (6 * (5 - j))) & 63]
    if first is not None:
        out[:, 0] = first
    return out


def rows_of(h: np.ndarray, tag: int, lang: bytes = b"en") -> np.ndarray:
    """rows under the hashes h: the cells a mix of hash, tag and column, so that the same url
    differs between sources in every cell; language and tag as given"""
    h = np.asarray(h, dtype=np.uint8).reshape(-1, 12)
    r = np.zeros((len(h), ROW), dtype=np.uint8)
    r[:, :12] = h
    k = (h.astype(np.int64) * np.arange(1, 13, dtype=np.int64)).sum(axis=1)
    cols = np.arange(12, ROW, dtype=np.int64)
    r[:, 12:] = (((k[:, None] * 31 + tag * 7 + cols[None, :] * 13) * 2654435761) >> 16) & 255
    r[:, 22:24] = np.frombuffer(lang, dtype=np.uint8)
    r[:, 33] = tag
    return r


def rows(idx, tag: int, lang: bytes = b"en", first=None) -> np.ndarray:
    return rows_of(hashes(idx, first), tag, lang)


def keys(r: np.ndarray) -> List[bytes]:
    return [bytes(x) for x in np.asarray(r).reshape(-1, ROW)[:, :12]]


def ascending(r: np.ndarray) -> bool:
    k = [heap.key_order(h) for h in keys(r)]
    return all(a < b for a, b in zip(k, k[1:]))


def export(r: np.ndarray, **kw) -> bytes:
    return heap.export_collection(r, **kw)


# ------------------------------------------------------------------ union_pairs
SIZE_PAIRS = ((1, 257), (257, 1), (256, 256), (255, 513), (513, 255), (512, 512))


def _half_shared(na: int, nb: int, seed: int):
    """index sets of na and nb urls, (min + 1) // 2 of them shared, interleaved at random"""
    s = (min(na, nb) + 1) // 2
    rng = np.random.default_rng([20, na, nb, seed])
    pool = rng.permutation(2 * (na + nb))[:na + nb - s]
    a = np.sort(pool[:na])
    b = np.sort(np.concatenate([pool[:s], pool[na:]]))
    return a, b


def _last_two():
    """families that agree in characters 0..9; the last two characters count 0, 1, 63, 64, 255,
    256, 4095 (both sides of character 10 and of the key's low byte).  A holds members 0 1 3 4 6,
    B holds 1 2 4 5: the shared ones (1, 4) have a neighbour in A and one in B that differ from
    them in the last two characters only"""
    vals = np.array([0, 1, 63, 64, 255, 256, 4095])
    fam = hashes(np.arange(40) * 17 + 3)
    h = np.repeat(fam, len(vals), axis=0)
    v = np.tile(vals, len(fam))
    h[:, 10] = _ALPHA[v >> 6]
    h[:, 11] = _ALPHA[v & 63]
    m = np.tile(np.arange(len(vals)), len(fam))
    plain = hashes(np.arange(1000, 1020))  # above every family: urls that other terms hold too (queries)
    return np.concatenate([h[np.isin(m, (0, 1, 3, 4, 6))], plain]), h[np.isin(m, (1, 2, 4, 5))]


def union_term(j: int) -> bytes:
    return b"UNIONpair%02d_" % j


@functools.lru_cache(maxsize=None)
def union_pairs() -> Load:
    """two files, one term per case: the older file's list A (tag 1), the newer one's B (tag 2).
    info["cases"]: (name, term, A's hashes, B's hashes)"""
    ar = np.arange
    ev, od = ar(0, 80, 2), ar(1, 80, 2)
    named = [
        ("below", ar(100, 140), ar(0, 40)),
        ("above", ar(0, 40), ar(100, 140)),
        ("alternate", ev, od),
        ("b_in_a", ar(0, 60), ar(0, 60, 3)),
        ("a_in_b", ar(1, 60, 3), ar(0, 60)),
        ("equal", ar(10, 60), ar(10, 60)),
        ("one_equal", ar(5, 6), ar(5, 6)),
        ("one_above", ar(5, 6), ar(6, 7)),
        ("one_below", ar(5, 6), ar(4, 5)),
        ("dup_first", ev, np.concatenate([[0], od[1:]])),
        ("dup_last", ev, np.concatenate([od[:-1], [78]])),
    ]
    pairs = [(n, hashes(a), hashes(b)) for n, a, b in named]
    for k, (na, nb) in enumerate(SIZE_PAIRS):
        a, b = _half_shared(na, nb, k)
        pairs.append(("size_%d_%d" % (na, nb), hashes(a), hashes(b)))
    pairs.append(("last_two",) + _last_two())
    cases = [(n, union_term(j), a, b) for j, (n, a, b) in enumerate(pairs)]
    fa = [(t, export(rows_of(a, 1))) for _, t, a, _ in cases]
    fb = [(t, export(rows_of(b, 2))) for _, t, _, b in cases]
    return Load([fa, fb[::-1]], {}, {"cases": cases})


def pair_class(a: np.ndarray, b: np.ndarray) -> dict:
    """counts that name the geometry of a pair: rows, shared hashes, B's rows below A's first and
    above A's last row, and where the shared hashes sit in A and in B"""
    ka = [heap.key_order(h) for h in keys(rows_of(a, 0))]
    kb = [heap.key_order(h) for h in keys(rows_of(b, 0))]
    sa = set(ka)
    shared = [k for k in kb if k in sa]
    return {"na": len(ka), "nb": len(kb), "shared": len(shared),
            "below": sum(k < ka[0] for k in kb), "above": sum(k > ka[-1] for k in kb),
            "slots_a": [ka.index(k) for k in shared], "slots_b": [kb.index(k) for k in shared]}


# ------------------------------------------------------------------ precedence
PREC, PREC_MATE = b"PRECEDENCE__", b"PRECEDENmate"
PREC_URLS = 31 * 20


def owners(i: int) -> Tuple[int, ...]:
    """the sources (files 0..3, RAM = 4) that hold url i: the (i mod 31)-th non-empty subset"""
    mask = i % 31 + 1
    return tuple(s for s in range(SOURCES) if mask >> s & 1)


def owner_tag(i: int) -> int:
    o = owners(i)[0]  # the oldest file wins; RAM loses to every file
    return RAM_TAG if o == 4 else o + 1


@functools.lru_cache(maxsize=None)
def precedence() -> Load:
    """one term over four files and RAM, every owner set 20 times; PREC_MATE (every third url and
    some urls beyond, in the oldest file) gives the queries a second list"""
    own = [owners(i) for i in range(PREC_URLS)]
    files = []
    for f in range(4):
        idx = [i for i in range(PREC_URLS) if f in own[i]]
        files.append([(PREC, export(rows(idx, f + 1)))])
    files[0].append((PREC_MATE, export(rows(np.arange(0, PREC_URLS + 60, 3), 1))))
    ram = {PREC: rows([i for i in range(PREC_URLS) if 4 in own[i]], RAM_TAG)}
    return Load(files, ram, {"tags": [owner_tag(i) for i in range(PREC_URLS)]})


# ------------------------------------------------------------------ unsorted_tails
def tail_term(name: bytes) -> bytes:
    return (b"TAIL" + name + b"_" * 12)[:12]


@functools.lru_cache(maxsize=None)
def unsorted_tails() -> Load:
    """rowsets whose orderbound is the length of their sorted prefix (file 1; file 0 is older).
    info["expect"]: term -> (hashes, tags) the load must leave, derived by hand here"""
    ar = np.arange
    cat = np.concatenate
    rng = np.random.default_rng(21)
    f0, f1, ram, expect = [], [], {}, {}

    def case(name, parts, orderbound, exp_idx, exp_tags):
        r = cat([rows(i, t) for i, t in parts])
        f1.append((tail_term(name), export(r, orderbound=orderbound)))
        expect[tail_term(name)] = (hashes(exp_idx), np.asarray(exp_tags))

    # orderbound == 0: nothing is claimed sorted
    p = rng.permutation(50)
    case(b"ob0", [(p, 2)], 0, ar(50), [2] * 50)
    # a tail of one row that belongs in the middle
    case(b"one", [(cat([ar(0, 20), ar(21, 41)]), 2), ([20], 3)], 40, ar(41), [2] * 20 + [3] + [2] * 20)
    # the tail repeats prefix hashes (the prefix row stays) and adds new ones
    case(b"dupprefix", [(ar(0, 80, 2), 2), ([10, 7, 78, 0, 3], 3)], 40,
         sorted(set(range(0, 80, 2)) | {7, 3}), [3 if i in (3, 7) else 2 for i in sorted(set(range(0, 80, 2)) | {7, 3})])
    # equal hashes inside the tail: the first one stays
    case(b"duptail", [(ar(0, 30), 2), ([50, 40, 45], 3), ([40, 50, 60], 4)], 30,
         list(range(30)) + [40, 45, 50, 60], [2] * 30 + [3, 3, 3, 4])
    # a long tail in descending order
    case(b"desc300", [(ar(1000, 1020), 2), (ar(300)[::-1], 3)], 20,
         list(range(300)) + list(range(1000, 1020)), [3] * 300 + [2] * 20)
    # the same term in an older sorted file and in RAM as well
    t = tail_term(b"mixed")
    f0.append((t, export(rows(ar(0, 60, 2), 1))))
    f1.append((t, export(cat([rows(ar(0, 30), 2), rows([45, 31, 44, 31], 3)]), orderbound=30)))
    ram[t] = rows(ar(25, 65, 5), RAM_TAG)
    exp = {}
    for i in ar(25, 65, 5):
        exp[int(i)] = RAM_TAG
    for i in [44, 45, 31]:
        exp[i] = 3
    for i in range(30):
        exp[i] = 2
    for i in range(0, 60, 2):
        exp[i] = 1
    expect[t] = (hashes(sorted(exp)), np.array([exp[i] for i in sorted(exp)]))
    return Load([f0, f1], ram, {"expect": expect})


# ------------------------------------------------------------------ rejects
BAD = ord("!")
HEALTHY = b"REJhealthy__"


def rej_term(name: bytes) -> bytes:
    return (b"REJ" + name + b"_" * 12)[:12]


@functools.lru_cache(maxsize=None)
def rejects() -> Load:
    """three files; every term but HEALTHY has one fault in one rowset and a RAM list that must
    stay as it is.  info["causes"]: term -> the one cause; info["where"]: term -> file"""
    ar = np.arange
    files = [[], [], []]
    ram, causes, where = {}, {}, {}
    good = ar(0, 40)

    def case(name, cause, f, blob, others=()):
        t = rej_term(name)
        files[f].append((t, blob))
        for g in others:  # healthy rowsets of the same term in other files
            files[g].append((t, export(rows(good + 3 * g, g + 1))))
        ram[t] = rows(ar(5, 45, 4), RAM_TAG)
        causes[t], where[t] = cause, f

    def hurt(tag, at, col, n=40):
        r = rows(ar(n) * 2, tag)
        r[at, col] = BAD
        return r

    case(b"hashfirst", "hash", 0, export(hurt(1, 0, 3)), others=(1,))
    case(b"hashlast", "hash", 1, export(hurt(2, 39, 0)), others=(0,))
    case(b"hash11", "hash", 0, export(hurt(1, 17, 11)))
    r = rows(ar(40) * 2, 2)
    r[20, 22:24] = 0
    case(b"lang", "language", 1, export(r), others=(0, 2))
    case(b"desc", "order", 0, export(rows(ar(40)[::-1], 1)))
    case(b"equal", "order", 2, export(rows([0, 1, 2, 3, 3, 4, 5], 3)), others=(0,))
    r = np.concatenate([rows(ar(20), 1), hurt(1, 4, 6, n=10)])
    case(b"tailhash", "hash", 0, export(r, orderbound=20), others=(2,))
    # a tail row with an empty language cell that "first of equal hashes" would remove
    r = np.concatenate([rows(ar(20), 2), rows([30], 2), rows([7], 2, lang=b"\0\0")])
    case(b"taillang", "language", 1, export(r, orderbound=20))
    case(b"newest", "language", 2, export(rows(ar(30), 3, lang=b"\0\0")), others=(0, 1))
    case(b"space", "space", 1, export(rows(good, 2), size=41), others=(0, 2))
    for f in range(3):
        files[f].insert(f, (HEALTHY, export(rows(good * 2 + f, f + 1))))
    ram[HEALTHY] = rows(ar(0, 90, 9), RAM_TAG)
    return Load(files, ram, {"causes": causes, "where": where})


# ------------------------------------------------------------------ records
def rec_term(name: bytes) -> bytes:
    return (b"REC" + name + b"_" * 12)[:12]


def _rec(key: bytes, blob: bytes, reclen=None) -> bytes:
    return struct.pack(">i", 12 + len(blob) if reclen is None else reclen) + key + blob


@functools.lru_cache(maxsize=None)
def records() -> Load:
    """file images written record by record.  info["counters"]: the scan's counters as counted
    by hand; info["lists"]: term -> tags the load must leave; info["absent"]: terms it must not"""
    ar = np.arange
    T = rec_term
    good = lambda tag, n=6: export(rows(ar(n), tag))
    # file 2: the main image
    cut = _rec(T(b"kept"), good(7, 30))
    main = b"".join([
        _rec(T(b"twice"), good(1)),                                  # replaced below
        _rec(b"\0" + T(b"free")[1:], b"x" * 25),                     # free record
        _rec(T(b"kept"), good(2)),                                   # a later copy runs past the end
        _rec(b"REC bad key!", good(3)),                              # key outside the alphabet
        _rec(T(b"twice"), good(4, 9)),                               # the last record of a key wins
        _rec(T(b"negsize"), export(rows(ar(6), 3), size=-1 & 0xFFFFFFFF)),    # size < 0: empty set
        _rec(T(b"negbound"), export(rows(ar(6), 3), orderbound=-2 & 0xFFFFFFFF)),  # orderbound < 0
        _rec(T(b"short"), b"y" * 13),                                # blob shorter than the header
        _rec(T(b"shortram"), b"y" * 5),                              # the same over a RAM list
        _rec(T(b"space"), good(3)),                                  # one of three files, see below
        _rec(T(b"after"), good(5)),                                  # the scan reaches this one
        cut[:-7],                                                    # record past the end of the file
    ])
    # file 3: the middle file of "space"; ends with reclen < 12 under a good key
    f3 = b"".join([
        _rec(T(b"small"), good(1)),
        _rec(T(b"space"), export(rows(ar(6), 4), size=5)),           # SpaceExceeded
        _rec(T(b"small"), b"", reclen=8),                            # must not replace the first copy
    ])
    # file 4: ends with a negative reclen; what follows is never read
    f4 = b"".join([
        _rec(T(b"neg"), good(1)),
        _rec(T(b"space"), good(5)),
        _rec(T(b"neg"), good(2), reclen=-20),
        _rec(T(b"unseen"), good(3)),
    ])
    files = [b"", b"fifteen bytes!!", main, f3, f4]
    assert len(files[1]) == 15
    ram = {T(b"space"): rows(ar(2, 5), RAM_TAG), T(b"shortram"): rows(ar(3), RAM_TAG)}
    lists = {T(b"twice"): [4] * 9, T(b"kept"): [2] * 6, T(b"after"): [5] * 6, T(b"small"): [1] * 6,
             T(b"neg"): [1] * 6, T(b"space"): [RAM_TAG] * 3, T(b"shortram"): [RAM_TAG] * 3}
    absent = [T(b"negsize"), T(b"negbound"), T(b"short"), T(b"unseen"), T(b"free")]
    # accepted records: main 9 (twice x2, kept, negsize, negbound, short, shortram, space, after),
    # file 3: 2, file 4: 2
    counters = {"files": 5, "records": 13, "free_records": 1, "bad_keys": 1}
    return Load(files, ram, {"counters": counters, "lists": lists, "absent": absent,
                             "stored": 5, "dropped": [T(b"space")]})


# ------------------------------------------------------------------ reload
REL = [b"RELOADterm_a", b"RELOADterm_b", b"RELOADterm_c"]


@functools.lru_cache(maxsize=None)
def reload(n: int = 300) -> Tuple[Load, Load]:
    """-> (first, second): `first` is two files and RAM lists; `second` one newer file that holds
    some of the first load's urls under another tag, urls new to both terms, and a new term.
    n: rows of term a's oldest record (4096 and more: a list that gets a bitmap)"""
    ar = np.arange
    first = Load([[(REL[0], export(rows(ar(0, 2 * n, 2), 1))), (REL[1], export(rows(ar(0, 300, 3), 1)))],
                  [(REL[0], export(rows(ar(0, 2 * n, 5), 2))), (REL[1], export(rows(ar(100, 200), 2)))]],
                 {REL[0]: rows(ar(1, 2 * n, 14), RAM_TAG), REL[1]: rows(ar(150, 260), RAM_TAG)})
    second = Load([[(REL[0], export(rows(np.concatenate([ar(0, 2 * n, 7), ar(2 * n, 2 * n + 50)]), 3))),
                    (REL[1], export(rows(ar(90, 330, 2), 3))),
                    (REL[2], export(rows(ar(0, 2 * n, 9), 3)))]])
    return first, second


# ------------------------------------------------------------------ big_list
BIG = b"BIGlist_____"
BIG_ROWS = 840_000  # 33,600,000 bytes: the third 16 MiB piece reuses the first staging buffer


@functools.lru_cache(maxsize=None)
def big_rows() -> np.ndarray:
    return rows(np.arange(BIG_ROWS) * 3 + 1, 1)


def big_list() -> Load:
    return Load([[(BIG, export(big_rows()))]])


# ------------------------------------------------------------------ shard_input
SH = [b"SHARDquarter", b"SHARDevery__", b"SHARDramonly", b"SHARDtopend_"]


def _chars(cs: bytes, n: int, start: int = 0, step: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """n urls under each first character of cs, in key order -> (idx, first)"""
    cs = bytes(sorted(cs, key=heap.ALPHA.index))
    idx = np.tile(start + step * np.arange(n), len(cs))
    return idx, np.repeat(np.frombuffer(cs, dtype=np.uint8), n)


@functools.lru_cache(maxsize=None)
def shard_input() -> Load:
    """three files and RAM, every rowset claimed sorted and well formed; first characters from
    FIRST_CHARS.  SH[0]: inside quarter 1 (Q, f).  SH[1]: every quarter, every file.  SH[2]: the
    files hold A and P only, RAM holds w and _.  SH[3]: inside the last quarter (w, _)"""
    def rs(cs, n, tag, start=0, step=1):
        idx, first = _chars(cs, n, start, step)
        return rows(idx, tag, first=first)

    files = [[(SH[0], export(rs(b"Qf", 20, 1))), (SH[1], export(rs(FIRST_CHARS, 12, 1, step=2))),
              (SH[2], export(rs(b"AP", 15, 1))), (SH[3], export(rs(b"w_", 9, 1)))],
             [(SH[1], export(rs(FIRST_CHARS, 12, 2, start=1, step=3))), (SH[0], export(rs(b"Q", 30, 2, step=2))),
              (SH[3], export(rs(b"_", 20, 2)))],
             [(SH[2], export(rs(b"A", 25, 3))), (SH[1], export(rs(b"APfgw", 8, 3, start=5)))]]
    ram = {SH[0]: rs(b"f", 25, RAM_TAG, step=3), SH[1]: rs(b"PQvw_", 10, RAM_TAG, start=2),
           SH[2]: rs(b"w_", 7, RAM_TAG), SH[3]: rs(b"w", 12, RAM_TAG, start=4)}
    return Load(files, ram)


def shard_of(r: np.ndarray, rank: int, world: int) -> np.ndarray:
    """the rows of a context's url-hash range (Distribution.verticalDHTPosition)"""
    r = np.asarray(r).reshape(-1, ROW)
    bits = world.bit_length() - 1
    return r[(heap._LUT[r[:, 0]] >> (6 - bits)) == rank]


def file_rowsets(load: Load) -> List[Dict[bytes, np.ndarray]]:
    """per file: term -> rows as exported (record lists only)"""
    return [{t: np.frombuffer(b, np.uint8, offset=heap.EXPORT_OVERHEAD).reshape(-1, ROW) for t, b in f}
            for f in load.files]


# ------------------------------------------------------------------ queries
def query_pairs(lists: Dict[bytes, np.ndarray], terms) -> List[Tuple[List[bytes], List[bytes]]]:
    """for every term t a two-term AND with the next term (cyclically) that shares a url with it,
    and an AND-NOT with the next one that leaves a url of t: (include, exclude) pairs"""
    terms = list(terms)
    sets = {t: set(keys(lists[t])) for t in terms}
    out = []
    for i, t in enumerate(terms):
        rest = terms[i + 1:] + terms[:i]
        u = next(u for u in rest if sets[t] & sets[u])
        out.append(([t, u], []))
        u = next(u for u in rest if sets[t] - sets[u])
        out.append(([t], [u]))
    return out
