"""Directed inputs of the url census tests (tests/test_url_census_ref.py checks their numbers on the
CPU, tests/test_gpu_url_census.py feeds them to the device).  A plain module: no tests, no import of
a test file or of the built library.

boundary()      hand-made lists: for every L of RUNS one url that is the only row of L one-row lists
                (L references: every lane of a wave adds to one id on the HIST path, and its run
                crosses wave, block and 1024-tile edges on the SORT path), and three lists over
                families of url hashes that differ only in the last 8 key bits (tests/split_keys.py),
                among them AAAAAAAAAAAA and ____________: the smallest and the largest key there
                is, so dictionary id 0 and id dict_urls - 1, of the hosts of key 0 and key 2^36 - 1
selection(b, n) terms of boundary() that select exactly n postings
host_set(h, n)  n distinct hosts, one of them nobody's, given unsorted, two of them twice"""

import functools

import numpy as np

import index_util as iu
import split_keys as sk

RUNS = (1, 63, 64, 65, 256, 257, 1025)
RUN_HOST = b"runh0s"
FIRST_URL, LAST_URL = b"AAAAAAAAAAAA", b"____________"
FIRST_HOST, LAST_HOST = b"AAAAAA", b"______"
NOBODY = b"n0b0dy"
SEED, NFAM = 91, 16
SELECTIONS = (1023, 1024, 1025)


def run_url(L: int) -> bytes:
    return b"-r" + iu.enc(L, 4) + RUN_HOST


def _term(k: int) -> bytes:
    return iu.term(k, b"-u")


class Boundary:
    """lists: {term: rows}; runs: {L: the L terms of its one-row lists}; pool: every one-row term, by L;
    fam: the three family lists' terms (every hash, every second, every third from the second);
    hashes: the family hashes, ascending"""

    def __init__(self, lists, runs, fam, hashes):
        self.lists, self.runs, self.fam, self.hashes = lists, runs, fam, hashes
        self.pool = [t for L in RUNS for t in runs[L]]


@functools.lru_cache(maxsize=None)
def boundary() -> Boundary:
    hashes = sk.families(SEED, NFAM)
    assert hashes[0] == FIRST_URL and hashes[-1] == LAST_URL
    lists, runs, k = {}, {}, 0
    for L in RUNS:
        row = sk.rows([run_url(L)], SEED + L)
        runs[L] = []
        for _ in range(L):
            lists[_term(k)] = row.copy()
            runs[L].append(_term(k))
            k += 1
    fam = [_term(5000), _term(5001), _term(5002)]
    for j, (t, hs) in enumerate(zip(fam, (hashes, hashes[0::2], hashes[1::3]))):
        lists[t] = sk.rows(hs, SEED + 1000 + j)
    return Boundary(lists, runs, fam, hashes)


def selection(b: Boundary, n: int):
    """the first two family lists and as many one-row lists, in pool order, as make n postings"""
    base = len(b.lists[b.fam[0]]) + len(b.lists[b.fam[1]])
    assert base < n <= base + len(b.pool)
    return b.fam[:2] + b.pool[:n - base]


def host_set(hosts, n: int):
    """n distinct hosts: n - 1 of `hosts` (drawn without order) and one nobody has (n == 1: one of `hosts`
    alone); unsorted, the first two once more"""
    hosts = sorted(bytes(h) for h in hosts)
    assert NOBODY not in hosts and 1 <= n <= len(hosts) + 1
    rng = np.random.default_rng(n)
    pick = [hosts[int(i)] for i in rng.permutation(len(hosts))[:max(n - 1, 1)]] + ([NOBODY] if n > 1 else [])
    pick = [pick[int(i)] for i in rng.permutation(n)]
    return pick + pick[:2]
