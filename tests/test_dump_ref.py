"""The heap dump's reference (tests/dump_ref.py) against the oracle's heap reader, the
preconditions of the list-size fixture of tests/test_gpu_dump.py, and the presence of
yrwi_dump_heap in the library and its ctypes table.  No GPU."""

import pytest

import dump_ref as dr
import heap
from yacy_search_server_amd import _lib, synth

NOW = 20741 * 86400000 + 4242


@pytest.fixture(scope="module")
def hand():
    lists = dr.fixture_lists(synth.build_index(synth.preset("tiny")))
    return lists, dr.expected_image(lists, now_ms=NOW)


def test_dump_entry_point_exported():
    assert hasattr(_lib.lib(), "yrwi_dump_heap")
    assert "yrwi_dump_heap" in _lib.SIGNATURES


def test_dump_stats_mirror_matches_header(tmp_path):
    """_lib.CDumpStats against the C compiler's layout of yrwi_dump_stats; YRWI_E_IO"""
    import ctypes
    import os
    import shutil
    import subprocess
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cls = _lib.CDumpStats
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "yrwi.h"', "int main(void) {",
             '  printf("%zu\\n", sizeof(yrwi_dump_stats));']
    want = [str(ctypes.sizeof(cls))]
    for name, _ in cls._fields_:
        lines.append(f'  printf("%zu\\n", offsetof(yrwi_dump_stats, {name}));')
        want.append(str(getattr(cls, name).offset))
    lines += ['  printf("%d %c%c %lld\\n", YRWI_E_IO, YRWI_DUMP_ORDERKEY0, YRWI_DUMP_ORDERKEY1, YRWI_DUMP_EPOCH_MS);',
              "  return 0;", "}"]
    want.append(f"-11 Be {dr.MS_2000}")
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert [g for g in got if g] == want
    assert _lib.E_IO == -11 and _lib.ERRORS[-11] == "YRWI_E_IO"


def test_expected_image_round_trips(hand, tmp_path):
    lists, image = hand
    p = tmp_path / "x.blob"
    p.write_bytes(image)
    scan = heap.scan_heap(str(p))
    assert set(scan) == set(lists)
    for t, rows in lists.items():
        assert heap.import_rowset(scan[t]).tobytes() == rows.tobytes(), t
    # the records are in Base64Order of the term hashes, the header cells as yrwi.h states them
    keys = [image[o + 4:o + 16] for o, _ in dr.layout(image)]
    assert keys == sorted(lists, key=heap.key_order)
    o, n = dr.layout(image)[0]
    d = (20741 - 10957).to_bytes(2, "big")
    assert image[o + 16:o + 30] == n.to_bytes(4, "big") + d + d + b"Be" + n.to_bytes(4, "big")
    assert len(image) == sum(30 + 40 * len(r) for r in lists.values())


def test_selection_of_expected_image(hand):
    lists, image = hand
    some = sorted(lists)[3:40:5]
    sub = dr.expected_image(lists, list(reversed(some)) + [some[0], b"nosuchterm__"], now_ms=NOW)
    assert sub == dr.expected_image({t: lists[t] for t in some}, now_ms=NOW)
    assert dr.expected_image(lists, [b"nosuchterm__"], now_ms=NOW) == b""


def test_fixture_sizes_meet_their_preconditions(hand):
    lists, image = hand
    sizes = sorted(len(r) for r in lists.values())
    assert len(sizes) == 200 and sizes.count(1) >= 40 and max(sizes) == 1000
    assert all(s in sizes for s in (2, 3, 5, 7, 11, 13, 64, 65))
    assert [n for _, n in dr.layout(image)] == [len(lists[t]) for t in sorted(lists, key=heap.key_order)]
    # at W = 256 a window boundary falls inside a reclen, a key and an export header, strictly
    # inside a row and exactly at a row start
    assert dr.boundary_classes(image, 256) == dr.BOUNDARY_CLASSES
    # the row areas start at all eight even residues mod 16
    assert dr.row_area_residues(image) == {0, 2, 4, 6, 8, 10, 12, 14}
