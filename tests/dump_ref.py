"""Reference of the heap dump (yrwi_dump_heap, include/yrwi.h): the bytes the file must hold,
built with the oracle's heap writer (oracle/heap.py: export_collection, write_heap), and the
hand-made list-size fixture of tests/test_gpu_dump.py with the checks of its preconditions.
A helper for the tests."""

import os
import struct
import tempfile
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import heap
import index_util as iu

MS_2000 = 946684800000  # 2000-01-01T00:00:00Z
REC_HDR = 4 + heap.KEYLEN + heap.EXPORT_OVERHEAD  # reclen, key, export header: 30 bytes


def days2000(now_ms: int) -> int:
    """the lastread / lastwrote cell: whole days from 2000-01-01 to now_ms, as an int16 cell"""
    return ((now_ms - MS_2000) // 86400000) & 0xFFFF


def expected_image(lists: Dict[bytes, np.ndarray], terms: Optional[Sequence[bytes]] = None, *, now_ms: int) -> bytes:
    """the file of yrwi_dump_heap(terms, now_ms) over `lists`: one record per non-empty list in
    Base64Order of the term hashes (terms=None: every list; unknown terms ignored)"""
    d = days2000(now_ms)
    names = set(lists) if terms is None else {bytes(t) for t in terms}
    recs = []
    for t in sorted(names, key=heap.key_order):
        rows = lists.get(t)
        if rows is None or len(rows) == 0:
            continue
        recs.append((t, heap.export_collection(rows, lastread=d, lastwrote=d, orderkey=b"Be")))
    fd, path = tempfile.mkstemp(suffix=".blob")
    os.close(fd)
    try:
        heap.write_heap(path, recs)
        with open(path, "rb") as f:
            return f.read()
    finally:
        os.unlink(path)


def layout(image: bytes) -> List[Tuple[int, int]]:
    """(file offset, rows) of every record, read from the image alone"""
    out, seek = [], 0
    while seek < len(image):
        reclen = struct.unpack_from(">i", image, seek)[0]
        n = struct.unpack_from(">i", image, seek + 4 + heap.KEYLEN)[0]
        assert reclen == heap.KEYLEN + heap.EXPORT_OVERHEAD + heap.ROW * n
        out.append((seek, n))
        seek += 4 + reclen
    assert seek == len(image)
    return out


def boundary_classes(image: bytes, window: int) -> set:
    """where the window boundaries (multiples of `window` inside the file) fall"""
    recs = layout(image)
    offs = np.array([o for o, _ in recs], dtype=np.int64)
    seen = set()
    for b in range(window, len(image), window):
        r = b - int(offs[np.searchsorted(offs, b, side="right") - 1])
        if 0 < r < 4:
            seen.add("reclen")
        elif 4 < r < 4 + heap.KEYLEN:
            seen.add("key")
        elif 4 + heap.KEYLEN < r < REC_HDR:
            seen.add("header")
        elif r >= REC_HDR and (r - REC_HDR) % heap.ROW == 0:
            seen.add("row start")
        elif r > REC_HDR:
            seen.add("inside row")
    return seen


BOUNDARY_CLASSES = {"reclen", "key", "header", "row start", "inside row"}


def row_area_residues(image: bytes) -> set:
    """file offsets of the records' row areas mod 16 (row storage is 256-byte aligned on the
    device, so this is the misalignment between source and destination)"""
    return {(o + REC_HDR) % 16 for o, _ in layout(image)}


def _sizes() -> List[int]:
    rng = np.random.default_rng(20)
    s = [1] * 40 + [2, 3, 5, 7, 11, 13, 64, 65, 1000] + [int(x) for x in rng.integers(1, 401, 151)]
    return [s[int(i)] for i in rng.permutation(len(s))]


SIZES = _sizes()  # list sizes of the hand-made fixture, in term order


def fixture_lists(idx) -> Dict[bytes, np.ndarray]:
    """len(SIZES) hand-made lists: rows of the synthetic index `idx` as templates, url hashes set
    as index_util.rows does"""
    return {iu.term(5000 + 7 * i): iu.rows(idx, [iu.url(k) for k in range(n)], start=i)
            for i, n in enumerate(SIZES)}
