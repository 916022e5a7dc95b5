"""The host reference (tests/host_ref.py) against a brute-force restatement on a hand case,
rehost() on the `tiny` corpus, and the presence of yrwi_remove_hosts / yrwi_count_hosts in the
library, its ctypes table and the header.  No GPU."""

import os
import re

import numpy as np

import host_ref as hr
import update_ref as ur
from yacy_search_server_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _row(url, fill):
    r = np.full(40, fill, dtype=np.uint8)
    r[:12] = np.frombuffer(url, dtype=np.uint8)
    return r


def _hand():
    """three lists over four hosts; list t2 holds hosts a and b only"""
    ha, hb, hc, hd = b"hostAA", b"hostBB", b"hostCC", b"hostDD"
    urls = {
        b"t0__________": [b"AAAAAA" + ha, b"AAAAAB" + hb, b"AAAAAC" + ha, b"BAAAAA" + hc, b"CAAAAA" + hd],
        b"t1__________": [b"AAAAAA" + ha, b"AAAAAD" + hc, b"DAAAAA" + hc],
        b"t2__________": [b"AAAAAB" + hb, b"AAAAAC" + ha, b"EAAAAA" + hb],
    }
    lists = {}
    for k, (t, us) in enumerate(urls.items()):
        us = sorted(us, key=ur.url_key)
        lists[t] = np.array([_row(u, 10 * k + i + 1) for i, u in enumerate(us)], dtype=np.uint8)
    return lists, (ha, hb, hc, hd)


def _brute(lists, hosts, terms):
    """every selected list without the rows whose characters 6..11 are in the set"""
    hs = {bytes(h) for h in hosts}
    names = set(lists) if terms is None else {bytes(t) for t in terms}
    out, removed, changed, emptied = {}, 0, 0, 0
    for t, l in lists.items():
        if t not in names:
            out[t] = l
            continue
        keep = [r for r in l if bytes(r[6:12]) not in hs]
        removed += len(l) - len(keep)
        changed += len(keep) != len(l)
        if keep:
            out[t] = np.array(keep, dtype=np.uint8) if len(keep) != len(l) else l
        else:
            emptied += 1
    return out, dict(terms=changed, new_terms=0, emptied_terms=emptied, added=0, replaced=0, dropped=0, removed=removed)


def _same(a, b):
    return set(a) == set(b) and all(a[t].tobytes() == b[t].tobytes() for t in a)


def test_reference_against_brute_force():
    lists, (ha, hb, hc, hd) = _hand()
    t0, t1, t2 = list(lists)
    cases = [([ha, hb, ha, b"nobody"], None),                       # duplicate and absent hosts; t2 is emptied
             ([hc], [t1, t0, t1, b"nosuchterm__"]),                 # a duplicate and an unknown term
             ([ha, hb], [t2]), ([hd], [t1]), ([], None), ([b"nobody"], None)]
    for hosts, terms in cases:
        got, st = hr.apply_remove_hosts(lists, hosts, terms)
        exp, est = _brute(lists, hosts, terms)
        assert _same(got, exp), (hosts, terms)
        assert st == est, (hosts, terms, st, est)
        counts, hit = hr.count_hosts(lists, hosts, terms)
        assert sum(dict(zip(hosts, counts)).values()) == est["removed"]  # over the unique hosts
        assert hit == est["terms"]
    got, st = hr.apply_remove_hosts(lists, [ha, hb, ha, b"nobody"], None)
    assert t2 not in got and st["emptied_terms"] == 1 and st["removed"] == 3 + 1 + 3
    assert hr.count_hosts(lists, [ha, hb, ha, b"nobody"], None) == ([4, 3, 4, 0], 3)
    assert hr.count_hosts(lists, [hc], [t1, t0, t1, b"nosuchterm__"]) == ([3], 2)
    assert sorted(hr.urls_of_hosts(lists, [hb], None)) == [b"AAAAAB" + hb, b"EAAAAA" + hb]


def test_rehost_tiny():
    """the facts the GPU tests rely on"""
    lists = synth.build_index(synth.preset("tiny")).as_dict()
    re_ = hr.rehost(lists)
    assert set(re_) == set(lists)
    assert sum(len(l) for l in re_.values()) == sum(len(l) for l in lists.values()) == 60050
    for t, l in re_.items():
        keys = [ur.url_key(bytes(r[:12])) for r in l]
        assert all(a < b for a, b in zip(keys, keys[1:])), t
        assert sorted(map(bytes, l[:, 12:])) == sorted(map(bytes, lists[t][:, 12:])), t  # only the hosts changed
        assert all(bytes(r[6:10]) == b"h0st" for r in l), t
    hosts = [hr.host_name(i) for i in (0, 5, 40, 63)]
    counts, _ = hr.count_hosts(re_, hosts)
    assert counts == [12719, 2095, 314, 183]
    in_lists = [sum(1 for l in re_.values() if any(bytes(r[6:12]) == h for r in l)) for h in hosts]
    assert in_lists == [200, 198, 116, 91]
    got, st = hr.apply_remove_hosts(re_, hosts[:3])
    assert st["removed"] == 15128 and st["emptied_terms"] == 0 and st["terms"] == 200


def test_timing_tool_rehosts_as_the_reference():
    """tools/index_hosts.py re-hosts the concatenated lists with numpy: the same lists as rehost()"""
    import importlib.util
    import zlib
    spec = importlib.util.spec_from_file_location("index_hosts", os.path.join(ROOT, "tools", "index_hosts.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    idx = synth.build_index(synth.preset("tiny"))
    some = idx.rows[::997, :12]
    assert list(tool.crc32_rows(some)) == [zlib.crc32(bytes(r)) for r in some]
    assert [bytes(n) for n in tool.host_names(64)] == [hr.host_name(i) for i in range(64)]
    big = [bytes(n) for n in tool.host_names(8192)]
    assert len(set(big)) == 8192 and big == sorted(big, key=ur.url_key)
    exp = hr.rehost(idx.as_dict())
    # a list with rows that share their first six characters: re-sorted, a duplicate dropped
    rows = np.concatenate([idx.rows, idx.rows[:3]])
    rows[-3:, :6] = np.frombuffer(b"zzzzzz", dtype=np.uint8)
    rows[-1, :12] = rows[-2, :12]
    last = b"last________"
    exp.update(hr.rehost({last: rows[-3:]}))
    assert 1 <= len(exp[last]) <= 2
    got, sizes, rank = tool.rehost(rows.copy(), np.append(idx.sizes, 3), 64)
    assert len(got) == sizes.sum() == len(rank) == sum(len(l) for l in exp.values())
    off = np.concatenate([[0], np.cumsum(sizes)])
    for t, h in enumerate(idx.hashes + [last]):
        assert got[off[t]:off[t + 1]].tobytes() == exp.get(h, np.zeros((0, 40), np.uint8)).tobytes(), t
    assert [bytes(r[6:12]) for r in got[::101]] == [hr.host_name(int(i)) for i in rank[::101]]


def test_host_entry_points_exported():
    for name in ("yrwi_remove_hosts", "yrwi_count_hosts"):
        assert hasattr(_lib.lib(), name), name
        assert name in _lib.SIGNATURES, name


def test_lds_bound_mirrors_header():
    hdr = open(os.path.join(ROOT, "include", "yrwi.h")).read()
    assert int(re.search(r"#define YRWI_HOST_LDS_MAX (\d+)", hdr).group(1)) == _lib.HOST_LDS_MAX
