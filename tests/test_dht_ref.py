"""The restatement of the DHT send path (tests/dht_ref.py) against expectations written out by
hand on a 6-term fixture: wrap, the first container >= limit, max_refs overshoot, private skip,
and the split at e = 0, 4 and 8.  No GPU."""

import numpy as np

import dht_ref as dr

T0, T1, T2, T3, T4, T5 = (b"AAAAAAAAAAAA", b"Mterm0000000", b"aterm0000000", b"5term0000000", b"_Cprivate000",
                          b"_zlast000000")  # in Base64Order: A < M < a < 5 < _C < _z
URLS = {
    T0: [b"AAurl0000001", b"gAurl0000002", b"_zurl0000003"],                   # e = 4: partitions 0, 8, 15
    T1: [b"BAurl0000004", b"BQurl0000005"],                                    # e = 8: partitions 4, 5
    T2: [b"CAurl0000006", b"Jxurl0000007", b"wAurl0000008", b"9Aurl0000009"],  # e = 4: 0, 2, 12, 15
    T3: [b"hAurl000000a"],
    T4: [b"DAurl000000b", b"EAurl000000c"],
    T5: [b"AAurl0000001", b"QAurl000000d", b"-Aurl000000e"],                   # e = 4: 0, 4, 15
}


def _row(term, url):
    return np.frombuffer(url + (term[:4] + url[-4:]) * 3 + b"fill", dtype=np.uint8)


LISTS = {t: np.stack([_row(t, u) for u in us]) for t, us in URLS.items()}
LISTS[b"emptyterm000"] = np.zeros((0, 40), dtype=np.uint8)  # an empty list is no container


def test_dht_entry_point_exported():
    from yacy_search_server_amd import RWIIndex, _lib
    assert hasattr(_lib.lib(), "yrwi_dht_select") and "yrwi_dht_select" in _lib.SIGNATURES
    assert callable(RWIIndex.dht_select)


def test_dht_stats_mirror_matches_header(tmp_path):
    """_lib.CDhtStats and the flag values against the C compiler's reading of include/yrwi.h"""
    import ctypes
    import os
    import shutil
    import subprocess
    from yacy_search_server_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cls = _lib.CDhtStats
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "yrwi.h"', "int main(void) {",
             '  printf("%zu\\n", sizeof(yrwi_dht_stats));']
    want = [str(ctypes.sizeof(cls))]
    for name, _ in cls._fields_:
        lines.append(f'  printf("%zu\\n", offsetof(yrwi_dht_stats, {name}));')
        want.append(str(getattr(cls, name).offset))
    lines += ['  printf("%d %d %d %d %d %c%c\\n", YRWI_DHT_ROT, YRWI_DHT_REMOVE, YRWI_DHT_SKIP_PRIVATE, '
              'YRWI_DHT_COUNT_ONLY, YRWI_DHT_MAX_EXPONENT, YRWI_DHT_PRIVATE0, YRWI_DHT_PRIVATE1);', "  return 0;", "}"]
    want.append(f"{_lib.DHT_ROT} {_lib.DHT_REMOVE} {_lib.DHT_SKIP_PRIVATE} {_lib.DHT_COUNT_ONLY} "
                f"{_lib.DHT_MAX_EXPONENT} {dr.PRIVATE.decode()}")
    assert (_lib.DHT_MAX_EXPONENT, dr.PRIVATE) == (dr.MAX_EXPONENT, b"_C")
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "abi"
    subprocess.run([shutil.which("gcc") or "cc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert [g for g in got if g] == want


def test_fixture_order():
    assert sorted(URLS, key=dr.key) == [T0, T1, T2, T3, T4, T5]
    for t, us in URLS.items():
        assert sorted(us, key=dr.key) == us and LISTS[t].shape == (len(us), 40)


def test_wrap():
    terms, st = dr.select(LISTS, b"bbbbbbbbbbbb", dr.LAST, 10, 100)
    assert terms == [T3, T5, T0, T1, T2]
    assert st == dict(terms=5, postings=13, skipped_private=1, wrapped=1)
    terms, st = dr.select(LISTS, b"bbbbbbbbbbbb", dr.LAST, 10, 100, rot=False)
    assert terms == [T3, T5] and st == dict(terms=2, postings=4, skipped_private=1, wrapped=0)
    # from the smallest term: a full cycle without a wrap; past the largest: nothing without rot
    terms, st = dr.select(LISTS, T0, dr.LAST, 10, 100)
    assert terms == [T0, T1, T2, T3, T5] and st["wrapped"] == 0
    assert dr.select(LISTS, b"_zlast000001", dr.LAST, 10, 100, rot=False)[0] == []
    terms, st = dr.select(LISTS, b"_zlast000001", dr.LAST, 10, 100)
    assert terms == [T0, T1, T2, T3, T5] and st["wrapped"] == 1


def test_first_container_at_or_past_limit():
    terms, st = dr.select(LISTS, T2, T1, 10, 100)
    assert terms == [T2] and st == dict(terms=1, postings=4, skipped_private=0, wrapped=0)
    # after a wrap the comparison is the plain one: T0 < limit is taken, T1 is not
    terms, st = dr.select(LISTS, T5, T1, 10, 100)
    assert terms == [T5, T0] and st == dict(terms=2, postings=6, skipped_private=0, wrapped=1)


def test_max_refs_overshoot_and_container_cut():
    terms, st = dr.select(LISTS, T0, dr.LAST, 10, 4)
    assert terms == [T0, T1] and st["postings"] == 5
    terms, st = dr.select(LISTS, T0, dr.LAST, 1, 100)
    assert terms == [T0] and st["postings"] == 3
    for mc, mr in ((0, 100), (10, 0), (-1, 100)):
        assert dr.select(LISTS, T0, dr.LAST, mc, mr) == ([], dict(terms=0, postings=0, skipped_private=0, wrapped=0))


def test_private_skip():
    terms, st = dr.select(LISTS, T3, dr.LAST, 10, 100, rot=False)
    assert terms == [T3, T5] and st == dict(terms=2, postings=4, skipped_private=1, wrapped=0)
    terms, st = dr.select(LISTS, T3, dr.LAST, 10, 100, rot=False, skip_private=False)
    assert terms == [T3, T4, T5] and st == dict(terms=3, postings=6, skipped_private=0, wrapped=0)
    # a private term does not use up a container slot
    assert dr.select(LISTS, T3, dr.LAST, 2, 100, rot=False)[0] == [T3, T5]


def test_split_e0_and_e8():
    off, rows = dr.split(LISTS, [T0, T2], 0)
    assert off.tolist() == [0, 3, 7]
    assert rows.tobytes() == LISTS[T0].tobytes() + LISTS[T2].tobytes()
    off, rows = dr.split(LISTS, [T1], 8)
    cnt = np.zeros(256, dtype=np.int64)
    cnt[4] = cnt[5] = 1  # "BA": 1 * 4 + 0, "BQ": 1 * 4 + 1
    assert off.tolist() == [0] + np.cumsum(cnt).tolist()
    assert rows.tobytes() == LISTS[T1].tobytes()
    off, rows = dr.split(LISTS, [], 4)
    assert off.tolist() == [0] and rows.shape == (0, 40)


def test_split_partition_major_layout():
    a, b, c = LISTS[T0], LISTS[T2], LISTS[T5]
    off, rows = dr.split(LISTS, [T0, T2, T5], 4)
    cnt = np.zeros(48, dtype=np.int64)
    for p, j in ((0, 0), (0, 1), (0, 2), (2, 1), (4, 2), (8, 0), (12, 1), (15, 0), (15, 1), (15, 2)):
        cnt[p * 3 + j] = 1
    assert off.tolist() == [0] + np.cumsum(cnt).tolist()
    assert rows.tobytes() == b"".join(x.tobytes() for x in (a[0], b[0], c[0], b[1], c[1], a[1], b[2], a[2], b[3], c[2]))
    assert dr.source_starts(LISTS, [T0, T2, T5], 4)[[0, 8 * 3, 15 * 3, 2 * 3 + 1, 15 * 3 + 2]].tolist() == [0, 1, 2, 1, 2]
    assert [dr.partition(u, 4) for u in URLS[T2]] == [0, 2, 12, 15]
    assert [dr.partition(u, 8) for u in URLS[T2]] == [8, 39, 192, 244]
