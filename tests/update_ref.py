"""Reference of the index-update semantics (yrwi_add_postings / yrwi_remove_postings,
include/yrwi.h), written as the literal sequential fold: one posting at a time, in batch
order, into a dict {term hash: (n, 40) uint8 rows ascending by url hash}.  A helper for the
tests, not an oracle of the query path.

add, for each posting (term, row) in batch order: the holder of (term, url hash) is the
list's row if it has one, else whatever an earlier posting of the batch left there.
  replace  (RowSet.put / IndexCell.add(termHash, entry)): the arrival takes the place;
  keep     (RowSet.mergeEnum): the holder stays;
  recent   (ReferenceContainer.putAllRecent): the arrival takes the place unless its
           lastModified (column a) is strictly smaller than the holder's.
Stats describe the end state: a batch posting that ends as the survivor of its (term, url)
is `added` when the url was new to the list and `replaced` when it took an existing row's
place; every other batch posting is `dropped`."""

from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

import java_literal as jl

_B64 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"
_RANK = bytes.maketrans(_B64, bytes(range(64)))

POLICIES = ("replace", "keep", "recent")


def url_key(h: bytes) -> bytes:
    """sort key of a 12-character hash in Base64Order"""
    return bytes(h[:12]).translate(_RANK)


def last_modified(row) -> int:
    return jl.col_long(bytes(row), "a")


def _rows(entries: List[bytes]) -> np.ndarray:
    return np.frombuffer(b"".join(entries), dtype=np.uint8).reshape(-1, 40).copy()


def apply_add(lists: Dict[bytes, np.ndarray], terms: Sequence[bytes], rows: np.ndarray,
              policy: str) -> Tuple[Dict[bytes, np.ndarray], dict]:
    """-> (new lists, expected stats); `lists` is left unchanged."""
    assert policy in POLICIES
    rows = np.asarray(rows, dtype=np.uint8).reshape(-1, 40)
    assert len(terms) == len(rows)
    # per touched term: url hash -> [row bytes, source]; source -1 = the list's row, else batch index
    work: Dict[bytes, Dict[bytes, list]] = {}
    for i, t in enumerate(terms):
        t = bytes(t)
        if t not in work:
            work[t] = {bytes(r[:12]): [bytes(r), -1] for r in lists.get(t, np.zeros((0, 40), np.uint8))}
        cell = work[t]
        row = bytes(rows[i])
        u = row[:12]
        holder = cell.get(u)
        if holder is None:
            cell[u] = [row, i]
        elif policy == "replace":
            cell[u] = [row, i]
        elif policy == "keep":
            pass
        elif not last_modified(row) < last_modified(holder[0]):
            cell[u] = [row, i]
    out = dict(lists)
    st = dict(terms=0, new_terms=0, emptied_terms=0, added=0, replaced=0, dropped=0, removed=0)
    for t, cell in work.items():
        had = {bytes(r[:12]) for r in lists.get(t, np.zeros((0, 40), np.uint8))}
        add = sum(1 for u, (_, s) in cell.items() if s >= 0 and u not in had)
        rep = sum(1 for u, (_, s) in cell.items() if s >= 0 and u in had)
        st["added"] += add
        st["replaced"] += rep
        if add + rep:
            st["terms"] += 1
            st["new_terms"] += t not in lists
            out[t] = _rows([cell[u][0] for u in sorted(cell, key=url_key)])
    st["dropped"] = len(rows) - st["added"] - st["replaced"]
    return out, st


def apply_remove(lists: Dict[bytes, np.ndarray], urls: Iterable[bytes],
                 terms: Optional[Sequence[bytes]] = None) -> Tuple[Dict[bytes, np.ndarray], dict]:
    """-> (new lists, expected stats); terms=None: every list."""
    out = dict(lists)
    st = dict(terms=0, new_terms=0, emptied_terms=0, added=0, replaced=0, dropped=0, removed=0)
    names = list(lists) if terms is None else [bytes(t) for t in terms]
    urls = [bytes(u) for u in urls]
    for t in names:  # a term named twice finds nothing left the second time
        if t not in out:
            continue
        cell = {bytes(r[:12]): bytes(r) for r in out[t]}  # (dicts keep the list's order)
        for u in urls:  # one url at a time; a url given twice is gone the second time
            if u in cell:
                del cell[u]
                st["removed"] += 1
        if len(cell) == len(out[t]):
            continue
        if cell:
            out[t] = _rows(list(cell.values()))
        else:
            del out[t]
    for t in set(names):
        if t in lists and (t not in out or len(out[t]) != len(lists[t])):
            st["terms"] += 1
            st["emptied_terms"] += t not in out
    return out, st
