"""Reference of the url census (yrwi_url_census / yrwi_host_url_census, include/yrwi.h): a Counter
over the url hash of every row of the selected lists, each selected list once -- a url's references
are the selected lists that hold it --, filtered by the host set and min_refs and ordered by the
Base64 order of the url or by (-references, that order); the host form groups those urls by their
characters 6..11.  Each call returns the expected counters of the call's statistics too.  A helper
for the tests."""

from collections import Counter
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import census_ref as cr
import host_ref as hr
import update_ref as ur

ORDERS = ("url", "refs")
HOST_ORDERS = cr.ORDERS  # "host", "count"
URL_KEYS = ("lists", "postings", "urls", "urls_hosted", "urls_passing", "max_refs")
HOST_KEYS = URL_KEYS + ("hosts", "hosts_passing")


def tally(lists: Dict[bytes, np.ndarray], terms: Optional[Sequence[bytes]] = None) -> Counter:
    """url -> references over the selected lists (a list holds a url once)"""
    have = Counter()
    for l in cr.selected(lists, terms):
        urls = [bytes(r[:12]) for r in l]
        assert len(set(urls)) == len(urls)
        have.update(urls)
    return have


def _frame(lists, terms, have) -> dict:
    sel = cr.selected(lists, terms)
    return dict(lists=len(sel), postings=sum(len(l) for l in sel), urls=len(have))


def ordered(have: Counter, order: str = "refs", min_refs: int = 1, hosts: Optional[Sequence[bytes]] = None):
    """-> (urls, refs, urls_hosted, max_refs): the urls of `have` of the hosts (None or empty: of every
    host) with at least max(min_refs, 1) references, in `order`"""
    assert order in ORDERS
    hs = {bytes(h) for h in hosts or ()}
    hosted = [(u, c) for u, c in have.items() if not hs or hr.host_of(u) in hs]
    keep = [(u, c) for u, c in hosted if c >= max(min_refs, 1)]
    if order == "url":
        keep.sort(key=lambda uc: ur.url_key(uc[0]))
    else:
        keep.sort(key=lambda uc: (-uc[1], ur.url_key(uc[0])))
    return [u for u, _ in keep], [c for _, c in keep], len(hosted), max((c for _, c in hosted), default=0)


def census(lists: Dict[bytes, np.ndarray], terms: Optional[Sequence[bytes]] = None,
           hosts: Optional[Sequence[bytes]] = None, order: str = "refs", min_refs: int = 1,
           top: Optional[int] = None, have: Optional[Counter] = None) -> Tuple[List[bytes], List[int], dict]:
    """-> (urls, references, expected stats: URL_KEYS).  have: tally(lists, terms), when the caller has it"""
    have = tally(lists, terms) if have is None else have
    urls, refs, hosted, most = ordered(have, order, min_refs, hosts)
    st = dict(_frame(lists, terms, have), urls_hosted=hosted, urls_passing=len(urls), max_refs=most)
    if top is not None:
        urls, refs = urls[:top], refs[:top]
    return urls, refs, st


def host_census(lists: Dict[bytes, np.ndarray], terms: Optional[Sequence[bytes]] = None, order: str = "count",
                min_urls: int = 1, top: Optional[int] = None,
                have: Optional[Counter] = None) -> Tuple[List[bytes], List[int], List[int], dict]:
    """-> (hosts, distinct urls, postings, expected stats: HOST_KEYS)"""
    assert order in HOST_ORDERS
    have = tally(lists, terms) if have is None else have
    nurls, posts = Counter(), Counter()
    for u, c in have.items():
        nurls[hr.host_of(u)] += 1
        posts[hr.host_of(u)] += c
    keep = [(h, n) for h, n in nurls.items() if n >= max(min_urls, 1)]
    if order == "host":
        keep.sort(key=lambda hn: cr.host_key(hn[0]))
    else:
        keep.sort(key=lambda hn: (-hn[1], cr.host_key(hn[0])))
    st = dict(_frame(lists, terms, have), urls_hosted=len(have), urls_passing=len(have),
              max_refs=max(have.values(), default=0), hosts=len(nurls), hosts_passing=len(keep))
    if top is not None:
        keep = keep[:top]
    return [h for h, _ in keep], [n for _, n in keep], [posts[h] for h, _ in keep], st
