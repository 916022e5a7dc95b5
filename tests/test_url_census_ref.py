"""The url census reference (tests/url_census_ref.py) on hand-made lists whose references are counted
by hand, against tests/census_ref.py for the postings of a host, the numbers of every directed case
of tests/url_census_cases.py by construction, the facts about the `tiny` corpus
the GPU tests rely on, and the presence of the two entry points in the library, its ctypes table and
the header.  No GPU."""

import ctypes
import os
import re
from collections import Counter

import numpy as np
import pytest

import census_ref as cr
import host_ref as hr
import span_cases as sc
import split_keys as sk
import update_ref as ur
import url_census_cases as ucc
import url_census_ref as ucr
from yacy_search_server_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _row(url, fill):
    r = np.full(40, fill, dtype=np.uint8)
    r[:12] = np.frombuffer(url, dtype=np.uint8)
    return r


def _hand():
    """three lists over six urls of three hosts"""
    ha, hb = b"hostAA", b"hostBB"
    a, b, c, d, e, f = (b"AAAAAA" + ha, b"AAAAAB" + hb, b"AAAAAC" + ha, b"BAAAAA" + hb, b"CAAAAA" + b"______",
                        b"______" + hb)
    urls = {b"t0__________": [a, b, c, d], b"t1__________": [a, b, e], b"t2__________": [a, c, f]}
    lists = {}
    for k, (t, us) in enumerate(urls.items()):
        us = sorted(us, key=ur.url_key)
        lists[t] = np.array([_row(u, 10 * k + i + 1) for i, u in enumerate(us)], dtype=np.uint8)
    return lists, (a, b, c, d, e, f), (ha, hb)


def test_hand_lists():
    lists, (a, b, c, d, e, f), (ha, hb) = _hand()
    t0, t1, t2 = list(lists)
    assert ucr.tally(lists) == Counter({a: 3, b: 2, c: 2, d: 1, e: 1, f: 1})
    urls, refs, st = ucr.census(lists, order="url")
    assert urls == [a, b, c, d, e, f] and refs == [3, 2, 2, 1, 1, 1]
    assert st == dict(lists=3, postings=10, urls=6, urls_hosted=6, urls_passing=6, max_refs=3)
    urls, refs, st = ucr.census(lists, order="refs")
    assert urls == [a, b, c, d, e, f] and sum(refs) == st["postings"]  # ties by ascending url hash
    assert ucr.census(lists, order="refs", min_refs=2)[:2] == ([a, b, c], [3, 2, 2])
    assert ucr.census(lists, order="refs", min_refs=2)[2]["urls_passing"] == 3
    assert ucr.census(lists, order="refs", min_refs=0)[:2] == ucr.census(lists, order="refs", min_refs=-3)[:2] == (urls, refs)
    assert ucr.census(lists, order="refs", min_refs=4)[2] == dict(lists=3, postings=10, urls=6, urls_hosted=6,
                                                                 urls_passing=0, max_refs=3)
    assert ucr.census(lists, order="refs", top=2)[:2] == ([a, b], [3, 2])
    assert ucr.census(lists, order="refs", top=2)[2]["urls_passing"] == 6
    # the host set: given twice and with a host nobody has
    urls, refs, st = ucr.census(lists, hosts=[hb, hb, b"nobody"], order="refs")
    assert (urls, refs) == ([b, d, f], [2, 1, 1])
    assert st == dict(lists=3, postings=10, urls=6, urls_hosted=3, urls_passing=3, max_refs=2)
    assert ucr.census(lists, hosts=[], order="url")[:2] == ucr.census(lists, order="url")[:2]
    # a duplicate and an unknown term: each selected list once
    urls, refs, st = ucr.census(lists, [t1, t0, t1, b"nosuchterm__"], order="url")
    assert (urls, refs) == ([a, b, c, d, e], [2, 2, 1, 1, 1])
    assert st == dict(lists=2, postings=7, urls=5, urls_hosted=5, urls_passing=5, max_refs=2)
    assert ucr.census(lists, [])[:2] == ([], []) and ucr.census(lists, [b"nosuchterm__"])[2]["lists"] == 0
    # the host form: urls and postings per host; the postings are the host census's
    hosts, nurls, posts, st = ucr.host_census(lists, order="host")
    assert (hosts, nurls, posts) == ([ha, hb, b"______"], [2, 3, 1], [5, 4, 1])
    assert st == dict(lists=3, postings=10, urls=6, urls_hosted=6, urls_passing=6, max_refs=3, hosts=3, hosts_passing=3)
    hosts, nurls, posts, st = ucr.host_census(lists, order="count")
    assert (hosts, nurls, posts) == ([hb, ha, b"______"], [3, 2, 1], [4, 5, 1])
    assert ucr.host_census(lists, order="count", min_urls=2)[:3] == ([hb, ha], [3, 2], [4, 5])
    assert ucr.host_census(lists, order="count", min_urls=4)[3]["hosts_passing"] == 0
    for terms in (None, [t2], [t1, t0, t1]):
        hosts, nurls, posts, st = ucr.host_census(lists, terms, "host")
        assert (hosts, posts) == cr.census(lists, terms, "host")[:2]
        assert sum(nurls) == st["urls"] and sum(posts) == st["postings"]


@pytest.fixture(scope="module")
def corpora():
    raw = synth.build_index(synth.preset("tiny")).as_dict()
    return raw, hr.rehost(raw)


def test_tiny_facts(corpora):
    """the facts of `tiny` the GPU cases rely on"""
    raw, reh = corpora
    have = ucr.tally(raw)
    assert len(raw) == 200 and sum(have.values()) == 60050 and len(have) == 48200
    by_refs = Counter(have.values())
    assert [by_refs[k] for k in (1, 2, 3, 4, 5)] == [38005, 8693, 1358, 135, 9] and max(have.values()) == 5
    passing = [ucr.census(raw, min_refs=m, have=have)[2]["urls_passing"] for m in (2, 3, 4, 5, 6)]
    assert passing == [10195, 1502, 144, 9, 0]  # every minimum cuts differently
    hosts, nurls, posts, st = ucr.host_census(raw, order="count", have=have)
    assert st["hosts"] == 36406 and (min(nurls), max(nurls)) == (1, 12) and sum(nurls) == 48200
    assert sorted(zip(hosts, posts)) == sorted(zip(*cr.census(raw, None, "host")[:2]))
    rhave = ucr.tally(reh)
    assert len(rhave) == 48200 and sum(rhave.values()) == 60050  # re-hosting merges no urls here
    hosts, nurls, posts, st = ucr.host_census(reh, order="count", have=rhave)
    assert st["hosts"] == 64 and (nurls[-1], nurls[0]) == (148, 10235) and len(set(nurls)) == 59  # ties
    assert nurls == sorted(nurls, reverse=True)
    for i in range(63):  # equal url counts by ascending host hash
        assert nurls[i] > nurls[i + 1] or cr.host_key(hosts[i]) < cr.host_key(hosts[i + 1])
    assert sorted(zip(hosts, posts)) == sorted(zip(*cr.census(reh, None, "host")[:2]))
    # named lists: 30 terms, one twice, one nobody has
    named = sorted(raw)[::7][:28]
    urls, refs, st = ucr.census(raw, named + [named[3], b"-u" + b"A" * 10], order="refs")
    assert st["lists"] == 28 and sum(refs) == st["postings"] < 60050 and st["urls"] == len(urls) < 48200


def test_boundary_numbers_by_construction():
    b = ucc.boundary()
    nh = len(b.hashes)
    assert len(b.pool) == sum(ucc.RUNS) == 1731 and len(b.lists) == 1731 + 3
    assert all(len(b.lists[t]) == 1 for t in b.pool)
    assert [len(b.lists[t]) for t in b.fam] == [nh, (nh + 1) // 2, len(b.hashes[1::3])]
    # the families: members differ only in the last 8 key bits, and a compare of khi alone merges them
    assert sk.distinct(b.hashes) == nh and sk.distinct(b.hashes, sk.blind_key) == ucc.NFAM < nh
    have = ucr.tally(b.lists)
    assert len(have) == nh + len(ucc.RUNS)
    for L in ucc.RUNS:
        assert have[ucc.run_url(L)] == L
    want = {h: 1 + (i % 2 == 0) + (i % 3 == 1) for i, h in enumerate(b.hashes)}
    assert all(have[h] == c for h, c in want.items())
    urls, refs, st = ucr.census(b.lists, order="refs", have=have)
    assert urls[:4] == [ucc.run_url(L) for L in (1025, 257, 256, 65)] and refs[:4] == [1025, 257, 256, 65]
    assert st == dict(lists=1734, postings=1731 + sum(want.values()), urls=nh + 7, urls_hosted=nh + 7,
                      urls_passing=nh + 7, max_refs=1025)
    by_url = ucr.census(b.lists, order="url", have=have)[0]
    assert by_url[0] == ucc.FIRST_URL and by_url[-1] == ucc.LAST_URL  # dictionary id 0 and id dict_urls - 1
    assert ur.url_key(ucc.FIRST_URL) == bytes(12) and ur.url_key(ucc.LAST_URL) == bytes([63]) * 12
    hosts, nurls, posts, hst = ucr.host_census(b.lists, order="host", have=have)
    assert hosts[0] == ucc.FIRST_HOST and hosts[-1] == ucc.LAST_HOST  # the hosts of key 0 and key 2^36 - 1
    at = hosts.index(ucc.RUN_HOST)
    assert (nurls[at], posts[at]) == (7, 1731)
    assert hr.host_of(ucc.FIRST_URL) == ucc.FIRST_HOST and hr.host_of(ucc.LAST_URL) == ucc.LAST_HOST
    # one run alone: one url, L references, L postings
    for L in ucc.RUNS:
        urls, refs, st = ucr.census(b.lists, b.runs[L], order="refs")
        assert (urls, refs) == ([ucc.run_url(L)], [L])
        assert st == dict(lists=L, postings=L, urls=1, urls_hosted=1, urls_passing=1, max_refs=L)
    for n in ucc.SELECTIONS:
        terms = ucc.selection(b, n)
        st = ucr.census(b.lists, terms)[2]
        assert st["postings"] == n and st["lists"] == len(terms) == len(set(terms))


def test_host_sets():
    hosts = [sc.host_hashes([i])[0] for i in range(1, 4000)]
    for n in (1, 2048, 2049):
        hs = ucc.host_set(hosts, n)
        assert len(hs) == n + min(n, 2) and len(set(hs)) == n
        assert n == 1 or hs[:n] != sorted(hs[:n], key=cr.host_key)
        assert (ucc.NOBODY in hs) == (n > 1)


def test_span_corpus_numbers():
    """the large index of tests/span_cases.py: every url in one list, so every url has one reference"""
    c = sc.corpus()
    assert len(np.unique(c.key)) == c.n == sc.TOTAL
    u, n = np.unique(c.host, return_counts=True)
    assert n.sum() == c.n and len(u) == sc.BG_HOSTS + sc.N_H64 + sc.N_G


def test_entry_points_exported():
    for name in ("yrwi_url_census", "yrwi_host_url_census"):
        assert hasattr(_lib.lib(), name) and name in _lib.SIGNATURES


def test_constants_and_struct_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "yrwi.h")).read()
    for name, val in (("BY_URL", _lib.UCENSUS_BY_URL), ("BY_REFS", _lib.UCENSUS_BY_REFS), ("HIST", _lib.UCENSUS_HIST),
                      ("SORT", _lib.UCENSUS_SORT)):
        assert int(re.search(r"#define YRWI_UCENSUS_%s\s+(\d+)" % name, hdr).group(1)) == val
    body = re.search(r"typedef struct yrwi_ucensus_stats \{(.*?)\} yrwi_ucensus_stats;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            fields += [(n.strip(), {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}[typ]) for n in names.split(",")]
    assert fields == list(_lib.CUCensusStats._fields_)
