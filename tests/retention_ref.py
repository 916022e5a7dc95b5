"""Reference of index retention (yrwi_retain / yrwi_retention_count, include/yrwi.h), written from the
definition "stable-sort the survivors of the age rule by lastModified descending, keep the first
max_refs, restore url-hash order", not from the cut-day form the device uses.  Also day_hist(), the
histogram of the selected rows' days, and redate(), which gives a corpus a small, skewed set of days so
that ties at the cut are the rule (what host_ref.rehost does for hosts).  A helper for the tests."""

import zlib
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

DAYS = 65536
UPDATE_KEYS = ("terms", "new_terms", "emptied_terms", "added", "replaced", "dropped", "removed")
COUNT_KEYS = ("lists", "postings", "removed_age", "removed_cap", "lists_age", "lists_cap", "emptied_terms",
              "day_min", "day_max")


def days_of(rows: np.ndarray) -> np.ndarray:
    """the `a` cell of every row: bytes 12-13, big endian, the raw unsigned value"""
    rows = np.asarray(rows, dtype=np.uint8).reshape(-1, 40)
    return (rows[:, 12].astype(np.int64) << 8) | rows[:, 13].astype(np.int64)


def set_days(rows: np.ndarray, days) -> np.ndarray:
    """a copy of the rows with their `a` cells set"""
    rows = np.array(rows, dtype=np.uint8).reshape(-1, 40)
    d = np.asarray(days, dtype=np.int64)
    assert len(d) == len(rows) and ((0 <= d) & (d < DAYS)).all()
    rows[:, 12] = d >> 8
    rows[:, 13] = d & 255
    return rows


def selected(lists: Dict[bytes, np.ndarray], terms: Optional[Sequence[bytes]] = None):
    """the selection of yrwi_remove_hosts: every list, or the named ones, each once, unknown terms ignored"""
    names = list(lists) if terms is None else [bytes(t) for t in terms]
    return [t for t in dict.fromkeys(names) if t in lists and len(lists[t])]


def day_hist(lists: Dict[bytes, np.ndarray], terms: Optional[Sequence[bytes]] = None) -> np.ndarray:
    """hist[d] = selected rows with a == d, before any rule"""
    h = np.zeros(DAYS, dtype=np.int64)
    for t in selected(lists, terms):
        h += np.bincount(days_of(lists[t]), minlength=DAYS)
    return h


def noop_stats() -> Tuple[dict, dict]:
    rs = {k: 0 for k in COUNT_KEYS}
    rs["day_min"] = rs["day_max"] = -1
    return {k: 0 for k in UPDATE_KEYS}, rs


def apply_retention(lists: Dict[bytes, np.ndarray], min_day: int, max_refs: int,
                    terms: Optional[Sequence[bytes]] = None,
                    dry_hist: bool = False) -> Tuple[Dict[bytes, np.ndarray], dict, dict]:
    """-> (new lists, expected yrwi_update_stats, expected yrwi_retention_stats counts); `lists` is left
    unchanged and a list that loses nothing stays the same object.  dry_hist: the statistics of the dry run
    with a histogram, whose pass runs without a rule too."""
    assert 0 <= min_day <= DAYS and max_refs >= 0
    sel = selected(lists, terms)
    st, rs = noop_stats()
    out = dict(lists)
    if not sel or (min_day == 0 and max_refs == 0 and not dry_hist):
        return out, st, rs
    lo, hi = DAYS, -1
    for t in sel:
        rows = lists[t]
        a = days_of(rows)
        lo, hi = min(lo, int(a.min())), max(hi, int(a.max()))
        surv = np.flatnonzero(a >= min_day)  # the age rule
        keep = surv
        if max_refs > 0 and len(surv) > max_refs:  # the cap: newest first, stable, the first max_refs
            newest_first = surv[np.argsort(-a[surv], kind="stable")]
            keep = np.sort(newest_first[:max_refs])
        age, cap = len(rows) - len(surv), len(surv) - len(keep)
        rs["lists"] += 1
        rs["postings"] += len(rows)
        rs["removed_age"] += age
        rs["removed_cap"] += cap
        rs["lists_age"] += age > 0
        rs["lists_cap"] += cap > 0
        rs["emptied_terms"] += len(surv) == 0
        if age + cap == 0:
            continue
        st["terms"] += 1
        st["removed"] += age + cap
        if len(keep):
            out[t] = rows[keep]
        else:
            del out[t]
            st["emptied_terms"] += 1
    rs["day_min"], rs["day_max"] = lo, hi
    return out, st, rs


def redate(lists: Dict[bytes, np.ndarray], days: Sequence[int], weights: Sequence[float]) -> Dict[bytes, np.ndarray]:
    """Every row gets a day of `days`, drawn with `weights` by the crc32 of (term hash, url hash): the same
    posting gets the same day whenever the corpus is built.  The url hashes, and so the order, stay."""
    assert len(days) == len(weights) and all(0 <= d < DAYS for d in days)
    w = np.asarray(weights, dtype=np.float64)
    cdf = np.cumsum(w / w.sum())
    dd = np.asarray(days, dtype=np.int64)
    out = {}
    for t, rows in lists.items():
        rows = np.asarray(rows, dtype=np.uint8).reshape(-1, 40)
        x = np.array([(zlib.crc32(bytes(t) + bytes(r[:12])) & 0xFFFFFF) / 2.0 ** 24 for r in rows])
        i = np.minimum(np.searchsorted(cdf, x, side="right"), len(dd) - 1)
        out[bytes(t)] = set_days(rows, dd[i])
    return out
