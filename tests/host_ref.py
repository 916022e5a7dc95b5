"""Reference of removal and counting by host (yrwi_remove_hosts / yrwi_count_hosts,
include/yrwi.h), built on tests/update_ref.py: removing hosts is removing the url hashes of
the selected lists whose characters 6..11 are in the host set.  Also rehost(), which gives a
synthetic corpus a small, skewed set of hosts (the corpora spread their postings over tens of
thousands of host parts with a handful of postings each).  A helper for the tests."""

import zlib
from collections import Counter
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import update_ref as ur

B64 = ur._B64


def host_of(url) -> bytes:
    """the host hash of a url hash: characters 6..11"""
    return bytes(url[6:12])


def _names(lists, terms):
    return list(lists) if terms is None else [bytes(t) for t in terms]


def urls_of_hosts(lists: Dict[bytes, np.ndarray], hosts: Sequence[bytes],
                  terms: Optional[Sequence[bytes]] = None) -> List[bytes]:
    """the url hashes in the selected lists (terms=None: every list) whose host is in `hosts`, each once"""
    hs = {bytes(h) for h in hosts}
    out = {}
    for t in _names(lists, terms):
        for r in lists.get(t, ()):
            u = bytes(r[:12])
            if host_of(u) in hs:
                out[u] = None
    return list(out)


def apply_remove_hosts(lists: Dict[bytes, np.ndarray], hosts: Sequence[bytes],
                       terms: Optional[Sequence[bytes]] = None) -> Tuple[Dict[bytes, np.ndarray], dict]:
    """-> (new lists, expected stats), as update_ref.apply_remove of those url hashes"""
    return ur.apply_remove(lists, urls_of_hosts(lists, hosts, terms), terms)


def count_hosts(lists: Dict[bytes, np.ndarray], hosts: Sequence[bytes],
                terms: Optional[Sequence[bytes]] = None) -> Tuple[List[int], int]:
    """-> (postings of hosts[i] in the selected lists, each selected list once; selected lists with a
    posting of any of the hosts)"""
    sel = [lists[t] for t in dict.fromkeys(_names(lists, terms)) if t in lists]
    per = [[host_of(r[:12]) for r in l] for l in sel]
    have = Counter(x for p in per for x in p)
    hs = {bytes(h) for h in hosts}
    return [have[bytes(h)] for h in hosts], sum(1 for p in per if any(x in hs for x in p))


def host_name(i: int) -> bytes:
    """host i of a re-hosted corpus"""
    return b"h0st" + bytes([B64[i >> 6], B64[i & 63]])


def rehost(lists: Dict[bytes, np.ndarray], H: int = 64) -> Dict[bytes, np.ndarray]:
    """Every row gets host host_name(i) in bytes 6..11, i drawn by the crc32 of its url hash
    from H hosts with weights 1 / (1 + j): the same url gets the same host in every list.
    Each list is sorted again; of rows that now share a url hash the first stays."""
    w = 1.0 / (1.0 + np.arange(H))
    cdf = np.cumsum(w / w.sum())
    names = np.array([np.frombuffer(host_name(i), dtype=np.uint8) for i in range(H)])
    out = {}
    for t, rows in lists.items():
        rows = np.array(rows, dtype=np.uint8).reshape(-1, 40)
        x = np.array([(zlib.crc32(bytes(r[:12])) & 0xFFFFFF) / 2.0 ** 24 for r in rows])
        i = np.minimum(np.searchsorted(cdf, x, side="right"), H - 1)
        rows[:, 6:12] = names[i]
        order = sorted(range(len(rows)), key=lambda k: ur.url_key(bytes(rows[k, :12])))  # stable
        keep, last = [], None
        for k in order:
            u = bytes(rows[k, :12])
            if u != last:
                keep.append(k)
            last = u
        out[t] = rows[keep]
    return out
