"""Reference of yrwi_host_facets_batch: a numpy group-by over the rows oracle.term_search returns.

A facet is a triple (host, count, url): the six characters 6..11 of the url hashes of one host,
how many rows of the container carry them, and the smallest url hash among those rows.  A plain
module: no tests, no import of a test file or of the built library."""

import numpy as np

import java_literal as jl

_IDX = np.full(256, -1, dtype=np.int64)
_IDX[np.frombuffer(jl.ALPHA, dtype=np.uint8)] = np.arange(64)


def host_key(h: bytes) -> int:
    """the 36-bit key of a host hash: Base64Order.enhancedCoder's order is the order of its integers"""
    k = 0
    for c in bytes(h):
        assert _IDX[c] >= 0, h
        k = (k << 6) | int(_IDX[c])
    return k


def group(rows: np.ndarray):
    """the facets of a container's (m, 40) rows (ascending url hashes), in ascending host order"""
    rows = np.asarray(rows, dtype=np.uint8).reshape(-1, 40)
    if len(rows) == 0:
        return []
    idx = _IDX[rows[:, 6:12]]
    assert (idx >= 0).all()
    keys = (idx << (6 * np.arange(5, -1, -1))).sum(axis=1)
    _, first, counts = np.unique(keys, return_index=True, return_counts=True)  # first: the smallest url
    return [(bytes(rows[f, 6:12]), int(c), bytes(rows[f, :12])) for f, c in zip(first, counts)]


def ordered(facets, order: str, max_hosts: int):
    """facets in ascending host order -> the ones the call writes: order "host", or "count"
    (postings descending, equal counts by ascending host), the first max_hosts (0: all)"""
    f = sorted(facets, key=lambda t: host_key(t[0]))
    if order == "count":
        f = sorted(f, key=lambda t: -t[1])  # stable
    else:
        assert order == "host", order
    return f[:max_hosts] if max_hosts > 0 else f
