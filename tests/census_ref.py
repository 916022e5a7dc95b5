"""Reference of the host census (yrwi_host_census, include/yrwi.h), built on tests/host_ref.py:
a Counter over the host hash of every row of the selected lists, each selected list once,
filtered by min_postings and ordered by the Base64 order of the host or by (-count, that
order).  A helper for the tests."""

from collections import Counter
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import host_ref as hr
import update_ref as ur

ORDERS = ("host", "count")


def host_key(h: bytes) -> bytes:
    """sort key of a 6-character host hash in Base64Order (update_ref.url_key's rule)"""
    return ur.url_key(bytes(h))


def selected(lists: Dict[bytes, np.ndarray], terms: Optional[Sequence[bytes]] = None) -> List[np.ndarray]:
    """the non-empty selected lists, each once (terms=None: every list; unknown terms ignored)"""
    return [lists[t] for t in dict.fromkeys(hr._names(lists, terms)) if t in lists and len(lists[t])]


def tally(lists: Dict[bytes, np.ndarray], terms: Optional[Sequence[bytes]] = None) -> Counter:
    """postings per host over the selected lists"""
    return Counter(hr.host_of(r[:12]) for l in selected(lists, terms) for r in l)


def ordered(have: Counter, order: str = "count", min_postings: int = 1) -> Tuple[List[bytes], List[int]]:
    """the hosts of `have` with at least max(min_postings, 1) postings, in `order`, and their counts"""
    assert order in ORDERS
    keep = [(h, c) for h, c in have.items() if c >= max(min_postings, 1)]
    if order == "host":
        keep.sort(key=lambda hc: host_key(hc[0]))
    else:
        keep.sort(key=lambda hc: (-hc[1], host_key(hc[0])))
    return [h for h, _ in keep], [c for _, c in keep]


def census(lists: Dict[bytes, np.ndarray], terms: Optional[Sequence[bytes]] = None, order: str = "count",
           min_postings: int = 1, top: Optional[int] = None) -> Tuple[List[bytes], List[int], dict]:
    """-> (hosts, counts, expected stats: lists, postings, hosts, hosts_passing)"""
    have = tally(lists, terms)
    hosts, counts = ordered(have, order, min_postings)
    sel = selected(lists, terms)
    st = dict(lists=len(sel), postings=sum(len(l) for l in sel), hosts=len(have), hosts_passing=len(hosts))
    if top is not None:
        hosts, counts = hosts[:top], counts[:top]
    return hosts, counts, st
