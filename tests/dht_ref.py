"""Reference of the DHT send path (yrwi_dht_select, include/yrwi.h), restated in plain Python /
numpy over a dict {term hash: (n, 40) uint8 rows ascending by url hash}: the selection
(Dispatcher.selectContainers), the split (splitContainer by Distribution.verticalDHTPosition) and
the partition-major layout of the output.  A helper for the tests."""

from typing import Dict, List, Sequence, Tuple

import numpy as np

_B64 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"
_RANK = bytes.maketrans(_B64, bytes(range(64)))
PRIVATE = b"_C"  # Word.isPrivate: the first two bytes of the term hash
MAX_EXPONENT = 8
LAST = b"_" * 12  # the largest hash


def key(h: bytes) -> bytes:
    """sort key of a 12-character hash in Base64Order"""
    return bytes(h[:12]).translate(_RANK)


def partition(urlhash: bytes, e: int) -> int:
    """the top e bits of the url key, e <= 8: they lie in the first two characters (12 bits)"""
    k = key(urlhash)
    return ((k[0] << 6) | k[1]) >> (12 - e)


def select(lists: Dict[bytes, np.ndarray], start: bytes, limit: bytes, max_containers: int, max_refs: int,
           rot: bool = True, skip_private: bool = True) -> Tuple[List[bytes], dict]:
    """-> (the selected terms in selection order, {terms, postings, skipped_private, wrapped})"""
    order = sorted((t for t in lists if len(lists[t])), key=key)
    ahead = [t for t in order if key(t) >= key(start)]
    behind = [t for t in order if key(t) < key(start)]
    # referenceContainerIterator(start, rot): the terms from `start` on, then (rot) the ones before it
    walk = [(t, 0) for t in ahead] + ([(t, 1) for t in behind] if rot else [])
    out: List[bytes] = []
    st = dict(terms=0, postings=0, skipped_private=0, wrapped=0)
    for t, after_wrap in walk:
        if not (len(out) < max_containers and st["postings"] < max_refs):
            break
        st["wrapped"] |= after_wrap
        if skip_private and t[:2] == PRIVATE:
            st["skipped_private"] += 1
            continue
        if out and not key(t) < key(limit):
            break
        out.append(t)
        st["postings"] += len(lists[t])
    st["terms"] = len(out)
    return out, st


def split(lists: Dict[bytes, np.ndarray], terms: Sequence[bytes], e: int) -> Tuple[np.ndarray, np.ndarray]:
    """-> (part_off: 2^e * T + 1 row offsets, partition-major; rows: the cells one after another)"""
    assert 0 <= e <= MAX_EXPONENT
    P, T = 1 << e, len(terms)
    off = np.zeros(P * T + 1, dtype=np.int64)
    cells = []
    parts = [[partition(r[:12].tobytes(), e) for r in lists[t]] for t in terms]
    for p in range(P):
        for j, t in enumerate(terms):
            rows = lists[t]
            mine = [i for i, q in enumerate(parts[j]) if q == p]
            assert mine == list(range(mine[0], mine[0] + len(mine))) if mine else True  # a contiguous row range
            cells.append(rows[mine].reshape(-1, 40))
            off[p * T + j + 1] = off[p * T + j] + len(mine)
    rows = np.concatenate(cells) if cells else np.zeros((0, 40), dtype=np.uint8)
    return off, rows.reshape(-1, 40)


def expected(lists, start, limit, max_containers, max_refs, e, rot=True, skip_private=True):
    """-> (terms, part_off, rows, stats) of yrwi_dht_select over `lists`"""
    terms, st = select(lists, start, limit, max_containers, max_refs, rot, skip_private)
    off, rows = split(lists, terms, e)
    return terms, off, rows, st


def source_starts(lists: Dict[bytes, np.ndarray], terms: Sequence[bytes], e: int) -> np.ndarray:
    """the first row, within its list, of every cell (partition-major, as part_off)"""
    P, T = 1 << e, len(terms)
    out = np.zeros(P * T, dtype=np.int64)
    for j, t in enumerate(terms):
        parts = np.array([partition(r[:12].tobytes(), e) for r in lists[t]], dtype=np.int64)
        for p in range(P):
            out[p * T + j] = int(np.searchsorted(parts, p, side="left"))
    return out


def after_removal(lists: Dict[bytes, np.ndarray], terms: Sequence[bytes]) -> Dict[bytes, np.ndarray]:
    return {t: r for t, r in lists.items() if t not in set(terms)}
