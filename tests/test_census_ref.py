"""The census reference (tests/census_ref.py) against host_ref.count_hosts on the re-hosted `tiny`
corpus and on three hand-made lists that hold the hosts AAAAAA and ______, the facts about both
corpora the GPU tests rely on, and the presence of yrwi_host_census in the library, its ctypes
table and the header.  No GPU."""

import ctypes
import os
import re

import numpy as np
import pytest

import census_ref as cr
import host_ref as hr
import update_ref as ur
from yacy_search_server_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST, LAST = b"AAAAAA", b"______"


def _row(url, fill):
    r = np.full(40, fill, dtype=np.uint8)
    r[:12] = np.frombuffer(url, dtype=np.uint8)
    return r


def _hand():
    """three lists over five hosts, among them the first and the last of the order"""
    ha, hb = b"hostAA", b"hostBB"
    urls = {
        b"t0__________": [b"AAAAAA" + FIRST, b"AAAAAB" + hb, b"AAAAAC" + ha, b"BAAAAA" + LAST, b"CAAAAA" + LAST],
        b"t1__________": [b"AAAAAA" + FIRST, b"AAAAAD" + LAST, b"DAAAAA" + b"h0st-_"],
        b"t2__________": [b"AAAAAB" + hb, b"AAAAAC" + ha, b"EAAAAA" + hb, b"______" + LAST],
    }
    lists = {}
    for k, (t, us) in enumerate(urls.items()):
        us = sorted(us, key=ur.url_key)
        lists[t] = np.array([_row(u, 10 * k + i + 1) for i, u in enumerate(us)], dtype=np.uint8)
    return lists, (ha, hb)


@pytest.fixture(scope="module")
def corpora():
    raw = synth.build_index(synth.preset("tiny")).as_dict()
    return raw, hr.rehost(raw)


def test_hand_lists():
    lists, (ha, hb) = _hand()
    t0, t1, t2 = list(lists)
    hosts, counts, st = cr.census(lists, order="host")
    assert hosts == [FIRST, ha, hb, b"h0st-_", LAST] and counts == [2, 2, 3, 1, 4]
    assert st == dict(lists=3, postings=12, hosts=5, hosts_passing=5)
    hosts, counts, st = cr.census(lists, order="count")
    assert hosts == [LAST, hb, FIRST, ha, b"h0st-_"] and counts == [4, 3, 2, 2, 1]  # the tie: AAAAAA before hostAA
    assert cr.census(lists, order="count", min_postings=2)[:2] == ([LAST, hb, FIRST, ha], [4, 3, 2, 2])
    assert cr.census(lists, order="count", min_postings=2)[2]["hosts_passing"] == 4
    assert cr.census(lists, order="count", min_postings=0)[0] == hosts  # as min_postings = 1
    assert cr.census(lists, order="count", top=2)[:2] == ([LAST, hb], [4, 3])
    assert cr.census(lists, order="count", top=2)[2]["hosts_passing"] == 5
    # a duplicate and an unknown term: each selected list once
    hosts, counts, st = cr.census(lists, [t1, t0, t1, b"nosuchterm__"], order="host")
    assert (hosts, counts) == ([FIRST, ha, hb, b"h0st-_", LAST], [2, 1, 1, 1, 3])
    assert st == dict(lists=2, postings=8, hosts=5, hosts_passing=5)
    assert cr.census(lists, [])[:2] == ([], []) and cr.census(lists, [b"nosuchterm__"])[2]["lists"] == 0
    assert cr.census(lists, order="count", min_postings=5)[2] == dict(lists=3, postings=12, hosts=5, hosts_passing=0)
    for terms in (None, [t2], [t1, t0, t1]):
        hosts, counts, _ = cr.census(lists, terms)
        assert hr.count_hosts(lists, hosts, terms)[0] == counts


def test_against_count_hosts_on_rehosted_tiny(corpora):
    """and the facts about the re-hosted corpus the GPU tests rely on"""
    raw, lists = corpora
    for order in cr.ORDERS:
        hosts, counts, st = cr.census(lists, order=order)
        assert st == dict(lists=200, postings=60050, hosts=64, hosts_passing=64)
        assert sorted(hosts) == sorted(hr.host_name(i) for i in range(64))  # every host is present
        assert hr.count_hosts(lists, hosts)[0] == counts and sum(counts) == 60050
    assert counts[0] == 12719 and counts[-1] == 183 and hosts[0] == hr.host_name(0)
    shared = [c for c in set(counts) if counts.count(c) > 1]
    assert len(shared) == 4 and all(counts.count(c) == 2 for c in shared)  # four count values, two hosts each
    for c in shared:  # equal counts by ascending host hash
        i = counts.index(c)
        assert cr.host_key(hosts[i]) < cr.host_key(hosts[i + 1])
    assert counts == sorted(counts, reverse=True)
    by_host = cr.census(lists, order="host")[0]
    assert by_host == sorted(by_host, key=cr.host_key)
    named = sorted(lists)[::7][:28]
    hosts, counts, st = cr.census(lists, named + [named[3]], order="count", min_postings=20)
    assert st["lists"] == 28 and 0 < st["hosts_passing"] < st["hosts"] and min(counts) >= 20
    assert hr.count_hosts(lists, hosts, named)[0] == counts


def test_raw_tiny_facts(corpora):
    """`tiny` as generated: the same postings over very many hosts of a few postings each"""
    raw, _ = corpora
    hosts, counts, st = cr.census(raw, order="count")
    assert st == dict(lists=200, postings=60050, hosts=36406, hosts_passing=36406)
    assert max(counts) == 16 and sum(counts) == 60050
    assert cr.census(raw, order="count", min_postings=17)[2]["hosts_passing"] == 0


def test_census_entry_point_exported():
    assert hasattr(_lib.lib(), "yrwi_host_census")
    assert "yrwi_host_census" in _lib.SIGNATURES


def test_constants_and_struct_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "yrwi.h")).read()
    assert int(re.search(r"#define YRWI_CENSUS_BY_HOST (\d+)", hdr).group(1)) == _lib.CENSUS_BY_HOST
    assert int(re.search(r"#define YRWI_CENSUS_BY_COUNT (\d+)", hdr).group(1)) == _lib.CENSUS_BY_COUNT
    body = re.search(r"typedef struct yrwi_census_stats \{(.*?)\} yrwi_census_stats;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            fields += [(n.strip(), {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}[typ]) for n in names.split(",")]
    assert fields == list(_lib.CCensusStats._fields_)
