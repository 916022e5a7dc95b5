"""Host-side mirror of YaCy's RWI query API over libyrwi (MI355X).

Mirrors the reference interface of the hot path so a caller written against
YaCy's classes finds the same names, argument meanings and "empty means no
result" behaviour (paths relative to /root/reference/source/net/yacy):

  RankingProfile           search/ranking/RankingProfile.java (defaults, external
                           string form, allZero)
  RWIIndex.add / get_size  kelondro/rwi/IndexCell.add (:289) / count
  RWIIndex.term_search     kelondro/rwi/TermSearch (:42-70) ->
                           ReferenceContainer.joinExcludeContainers (:310-326)
  ReferenceOrder           search/ranking/ReferenceOrder.normalizeWith (:70) +
                           cardinal (:223); settled (deterministic) min/max
  RWIIndex.search          SearchEvent.RWIProcess.run (:601-631) -> addRWIs
                           (:673-836) -> rwiStack top-k

All posting work runs in libyrwi's HIP kernels; this module only marshals.
"""

from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import CFilter, CHit, CProfile, CQuery, CStats, YrwiError

INTEGER_MAX = 2147483647
MAX_RESULTS_RWI = 3000  # SearchEvent.java:118

# external attribute names (RankingProfile.java:42-75) -> coefficient field
_EXTERNAL = {
    "domlength": "coeff_domlength", "date": "coeff_date", "wordsintitle": "coeff_wordsintitle",
    "wordsintext": "coeff_wordsintext", "phrasesintext": "coeff_phrasesintext", "llocal": "coeff_llocal",
    "lother": "coeff_lother", "urllength": "coeff_urllength", "urlcomps": "coeff_urlcomps",
    "hitcount": "coeff_hitcount", "posintext": "coeff_posintext", "posofphrase": "coeff_posofphrase",
    "posinphrase": "coeff_posinphrase", "authority": "coeff_authority", "worddistance": "coeff_worddistance",
    "appurl": "coeff_appurl", "appdescr": "coeff_app_dc_title", "appauthor": "coeff_app_dc_creator",
    "apptags": "coeff_app_dc_subject", "appref": "coeff_app_dc_description", "appemph": "coeff_appemph",
    "catindexof": "coeff_catindexof", "cathasimage": "coeff_cathasimage", "cathasaudio": "coeff_cathasaudio",
    "cathasvideo": "coeff_cathasvideo", "cathasapp": "coeff_cathasapp", "tf": "coeff_termfrequency",
    "urlcompintoplist": "coeff_urlcompintoplist", "descrcompintoplist": "coeff_descrcompintoplist",
    "prefer": "coeff_prefer", "language": "coeff_language", "citation": "coeff_citation",
}


class RankingProfile:
    """search/ranking/RankingProfile.java.  Default = RankingProfile(ContentDomain.TEXT)."""

    COEFF_MIN = 0
    COEFF_MAX = 15

    def __init__(self, prefix: Optional[str] = None, profile: Optional[str] = None):
        self._c = CProfile()
        if profile:
            _lib.lib().yrwi_profile_parse((prefix or "").encode(), profile.encode(), ctypes.byref(self._c))
        else:
            _lib.lib().yrwi_profile_default(ctypes.byref(self._c))

    def __getattr__(self, name):
        if name.startswith("coeff_"):
            return getattr(self._c, name)
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if name.startswith("coeff_"):
            setattr(self._c, name, int(value))
        else:
            object.__setattr__(self, name, value)

    def all_zero(self) -> "RankingProfile":  # allZero() :200-233
        _lib.lib().yrwi_profile_all_zero(ctypes.byref(self._c))
        return self

    @classmethod
    def date(cls) -> "RankingProfile":  # "/date" modifier, htroot/yacysearch.java:495-499
        p = cls().all_zero()
        p.coeff_date = cls.COEFF_MAX
        return p

    @classmethod
    def near(cls) -> "RankingProfile":  # "/near" modifier, htroot/yacysearch.java:489-494
        p = cls().all_zero()
        p.coeff_worddistance = cls.COEFF_MAX
        return p

    def to_external_map(self) -> dict:
        return {k: getattr(self._c, v) for k, v in _EXTERNAL.items()}

    @property
    def c(self) -> CProfile:
        return self._c


@dataclass
class Hit:
    urlhash: bytes
    score: int      # ReferenceOrder.cardinal
    tiebreak: int   # ByteArray.hashCode(urlhash)
    # the 40-byte row of the joined container the hit was ranked from (searches with rows=True;
    # a sharded context: 40 zero bytes when another rank owns the url hash), else None
    row: Optional[bytes] = None


class QueryFilter:
    """SearchEvent.addRWIs constraints (SearchEvent.java:736-806) and the doubledom
    pull order (pullOneRWI, :1297-1394); see yrwi_filter in include/yrwi.h.
    After a search, `flagcount` holds SearchEvent.flagcount (32 counters)."""

    def __init__(self, constraint: Optional[bytes] = None, all_of_constraint: bool = False, contentdom: int = 0,
                 strict_contentdom: bool = False, language: str = "", sitehash: Optional[bytes] = None,
                 alt_sitehash: Optional[bytes] = None, siteexcludes: Sequence[bytes] = (),
                 urlhashes: Sequence[bytes] = (), skip_double_dom: bool = False):
        c = CFilter()
        if constraint is not None:
            c.constraint[:] = list(bytes(constraint)[:4].ljust(4, b"\0"))
            c.has_constraint = 1
        c.all_of_constraint = int(all_of_constraint)
        c.contentdom = contentdom
        c.strict_contentdom = int(strict_contentdom)
        c.language = language.encode()[:7]
        if sitehash is not None:
            c.sitehash[:] = list(bytes(sitehash)[:6])
            c.has_sitehash = 1
        if alt_sitehash is not None:
            c.alt_sitehash[:] = list(bytes(alt_sitehash)[:6])
            c.has_alt_sitehash = 1
        sx = b"".join(bytes(h) for h in siteexcludes)
        uh = b"".join(bytes(h) for h in urlhashes)
        self._sx = ctypes.create_string_buffer(sx, max(1, len(sx)))
        self._uh = ctypes.create_string_buffer(uh, max(1, len(uh)))
        c.siteexcludes = ctypes.cast(self._sx, ctypes.c_void_p)
        c.nsiteexcludes = len(siteexcludes)
        c.urlhashes = ctypes.cast(self._uh, ctypes.c_void_p)
        c.nurlhashes = len(urlhashes)
        c.skip_double_dom = int(skip_double_dom)
        self._flags = (ctypes.c_int32 * 32)()
        c.flagcount = ctypes.cast(self._flags, ctypes.POINTER(ctypes.c_int32))
        self.c = c

    @property
    def flagcount(self) -> List[int]:
        return list(self._flags)


class SearchEvent:
    """One SearchEvent's RWI side (SearchEvent.addRWIs, SearchEvent.java:673-836):
    the local container and remote peers' containers (Protocol.java:802) arrive
    one after another; normalisation, doublecheck set, flag counts and the
    rwiStack persist on the GPU between arrivals (yrwi_event_* in include/yrwi.h)."""

    def __init__(self, index: "RWIIndex", profile: Optional[RankingProfile], language: str, now_ms: int, k: int,
                 filter: Optional[QueryFilter], max_postings: int, order_only_hosts: Optional[int] = None):
        self._ix = index
        self.k = k
        prof = profile or RankingProfile()
        e = ctypes.c_void_p()
        if order_only_hosts is not None:  # yrwi_event_open_order: order() / authority() only
            _check(index._h, _lib.lib().yrwi_event_open_order(index._h, ctypes.byref(prof._c), language.encode(),
                                                              now_ms, order_only_hosts, ctypes.byref(e)))
        else:
            fp = ctypes.byref(filter.c) if filter is not None else None
            _check(index._h, _lib.lib().yrwi_event_open(index._h, ctypes.byref(prof._c), language.encode(), now_ms, k,
                                                        fp, max_postings, ctypes.byref(e)))
        self._e = e

    def add_rwis(self, rows: np.ndarray, local: bool = False) -> int:
        return self._ix.add_rwis([(self, rows, local)])[0]

    def add_local(self, include: Sequence[bytes], exclude: Sequence[bytes] = (), max_distance: int = INTEGER_MAX,
                  now_ms: int = 0, urlselection: Optional[Sequence[bytes]] = None) -> int:
        """The local container of the event straight from the device index
        (yrwi_event_add_local): what add_rwis(index.term_search(...), True) leaves, without
        the rows crossing to the host.  Returns the rows that arrived."""
        return self._ix.add_local_rwis([(self, Query(include, exclude, max_distance, 1, None, "en", now_ms, None,
                                                     urlselection))])[0]

    def rows(self, urlhashes: Sequence[bytes]) -> List[Optional[bytes]]:
        """The 40-byte row of each url's admitted posting when it arrived through add_local
        (yrwi_event_rows); None for a url that was not admitted, was seeded by the filter, or
        came from an add_rwis arrival (the caller holds those rows, see source())."""
        n = len(urlhashes)
        out = np.zeros((max(1, n), 40), dtype=np.uint8)
        found = np.zeros(max(1, n), dtype=np.uint8)
        if n:
            _check(self._ix._h, _lib.lib().yrwi_event_rows(self._ix._h, self._e, _hashes(urlhashes), n,
                                                           out.ctypes.data, found.ctypes.data))
        return [out[i].tobytes() if found[i] else None for i in range(n)]

    def order(self, rows: np.ndarray, local: bool = False) -> np.ndarray:
        """ReferenceOrder.normalizeWith(container, local) + cardinal of every row
        (yrwi_event_order): the container continues the event's ReferenceOrder
        (min/max, max-distance fold, host counts over every container so far); the
        scores are under the state after it.  The stack is not touched: the
        drop-in's SearchEvent.addRWIs keeps its own (GpuReferenceOrder)."""
        r = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, 40)
        out = np.zeros(len(r), dtype=np.int64)
        if len(r):
            _check(self._ix._h, _lib.lib().yrwi_event_order(self._ix._h, self._e, r.ctypes.data, len(r),
                                                            int(bool(local)), out.ctypes.data))
        return out

    def authority(self, hosthashes: Sequence[bytes]) -> List[int]:
        """ReferenceOrder.authority(hostHash) against the accumulated host counts."""
        buf = b"".join(bytes(h)[:6] for h in hosthashes)
        out = (ctypes.c_int32 * max(1, len(hosthashes)))()
        if hosthashes:
            _check(self._ix._h, _lib.lib().yrwi_event_authority(self._ix._h, self._e, buf, len(hosthashes), out))
        return [int(out[i]) for i in range(len(hosthashes))]

    def source(self, urlhashes: Sequence[bytes]) -> List[Tuple[int, int]]:
        """(arrival, row) of each url's admitted posting (yrwi_event_source): arrival 1 is
        the event's first applied add_rwis arrival (empty and rejected arrivals are not
        counted), 0 a seeded doublecheck url, -1 not admitted."""
        n = len(urlhashes)
        a = np.zeros(max(1, n), dtype=np.int32)
        r = np.zeros(max(1, n), dtype=np.int32)
        if n:
            _check(self._ix._h, _lib.lib().yrwi_event_source(self._ix._h, self._e, b"".join(bytes(u) for u in urlhashes),
                                                             n, a.ctypes.data, r.ctypes.data))
        return [(int(a[i]), int(r[i])) for i in range(n)]

    def results(self) -> Tuple[List["Hit"], "CEventInfo"]:
        out = (_lib.CHit * max(1, self.k))()
        n = ctypes.c_int32()
        info = _lib.CEventInfo()
        _check(self._ix._h, _lib.lib().yrwi_event_result(self._ix._h, self._e, out, self.k, ctypes.byref(n),
                                                         ctypes.byref(info)))
        return [Hit(bytes(out[i].urlhash), out[i].score, out[i].tiebreak) for i in range(n.value)], info

    def pull(self, n: int, skip_double_dom: bool = True) -> List["Hit"]:
        """SearchEvent.pullOneRWI(skipDoubleDom) up to n times (SearchEvent.java:1297-1394):
        the entries leave the stack; the doubleDomCache persists across calls."""
        out = (_lib.CHit * max(1, n))()
        got = ctypes.c_int32()
        _check(self._ix._h, _lib.lib().yrwi_event_pull(self._ix._h, self._e, 1 if skip_double_dom else 0, out, n,
                                                       ctypes.byref(got)))
        return [Hit(bytes(out[i].urlhash), out[i].score, out[i].tiebreak) for i in range(got.value)]

    def close(self):
        if self._e and self._ix._h:
            _lib.lib().yrwi_event_close(self._ix._h, self._e)
        self._e = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


@dataclass
class Query:
    include: Sequence[bytes]
    exclude: Sequence[bytes] = ()
    max_distance: int = INTEGER_MAX
    k: int = 100
    profile: Optional[RankingProfile] = None
    language: str = "en"
    now_ms: int = 0
    filter: Optional[QueryFilter] = None
    urlselection: Optional[Sequence[bytes]] = None  # TermSearch's urlselection (url hashes)


def _check(ctx, rc: int):
    if rc != 0:
        # ctx None: an open failed, and yrwi_last_error(NULL) holds this thread's reason
        msg = _lib.lib().yrwi_last_error(ctx)
        raise YrwiError(rc, (msg or b"").decode(errors="replace"))


def _address(buf) -> Optional[int]:
    """address of a ctypes array / numpy array, an int address as it is, None as NULL"""
    if buf is None or isinstance(buf, int):
        return buf
    if isinstance(buf, np.ndarray):
        return buf.ctypes.data
    return ctypes.addressof(buf)


def _hashes(hs: Sequence[bytes]) -> bytes:
    out = b"".join(bytes(h) for h in hs)
    if len(out) != 12 * len(hs):
        raise ValueError("term hashes must be 12 bytes")
    return out


class DhtSelection:
    """What RWIIndex.dht_select returns: terms (the T selected term hashes in selection order),
    part_off (P * T + 1 row offsets, partition-major), rows (every selected posting as one
    (n, 40) uint8 array, cell after cell), partitions (P) and stats (yrwi_dht_stats as a dict)."""

    def __init__(self, terms: List[bytes], part_off: np.ndarray, rows: np.ndarray, partitions: int, stats: dict):
        self.terms, self.part_off, self.rows, self.partitions, self.stats = terms, part_off, rows, partitions, stats

    def cell(self, p: int, j: int) -> np.ndarray:
        """the rows of term j that go to partition p, in url-hash order"""
        if not (0 <= p < self.partitions and 0 <= j < len(self.terms)):
            raise IndexError("no such cell")
        c = p * len(self.terms) + j
        return self.rows[self.part_off[c]:self.part_off[c + 1]]


class RWIIndex:
    """A device-resident reverse word index (one GPU, or one URL-hash shard).

    rows: numpy uint8 arrays of shape (n, 40) -- WordReferenceRow rows, i.e. the
    bytes of a RowSet chunkcache (RowCollection.java:68)."""

    def __init__(self, device: int = 0, shard: Optional[Tuple[int, int, bytes]] = None):
        L = _lib.lib()
        h = ctypes.c_void_p()
        if shard is None:
            _check(None, L.yrwi_open(device, ctypes.byref(h)))
        else:
            rank, world, uid = shard
            _check(None, L.yrwi_open_shard(device, rank, world, uid, ctypes.byref(h)))
        self._h = h
        self.device = device

    def shard_info(self) -> dict:
        """How this context's collectives travel (yrwi_shard_info): transport ("rccl",
        "host-staged", "loopback", "none"), RCCL communicator rank count, lanes, lanes
        with their own communicator, other ranks on this device, mailbox, PCI bus id."""
        info = _lib.CTransportInfo()
        _check(self._h, _lib.lib().yrwi_shard_info(self._h, ctypes.byref(info)))
        d = {f: getattr(info, f) for f, _ in _lib.CTransportInfo._fields_}
        d["transport"] = _lib.TRANSPORTS.get(d["transport"], str(d["transport"]))
        d["pci_bus_id"] = d["pci_bus_id"].decode(errors="replace")
        return d

    def close(self):
        if self._h:
            for p in getattr(self, "_pinned", []):
                _lib.lib().yrwi_host_free(self._h, p)
            self._pinned = []
            self._tsb_buf, self._tsb_cap = None, -1  # term_search_batch's pinned landing buffer went with them
            _lib.lib().yrwi_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- index maintenance (IndexCell) ----
    def add(self, term: bytes, rows: np.ndarray, sorted: bool = True) -> None:
        rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, 40)
        _check(self._h, _lib.lib().yrwi_put_list(self._h, bytes(term), rows.ctypes.data, len(rows), 1 if sorted else 0))

    def add_postings(self, terms: Sequence[bytes], rows: np.ndarray, policy: str = "replace") -> dict:
        """IndexCell.add in bulk (yrwi_add_postings): posting i, rows[i], goes into the list of
        terms[i]; only the batch crosses to the device.  policy: "replace" (RowSet.put: the
        newest of a (term, url) pair stays), "keep" (RowSet.mergeEnum: the first stays) or
        "recent" (ReferenceContainer.putAllRecent: the newest unless its lastModified is
        smaller).  Returns the call's yrwi_update_stats as a dict."""
        rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, 40)
        if isinstance(terms, np.ndarray):
            tb = np.ascontiguousarray(terms, dtype=np.uint8).reshape(-1, 12)
        else:
            tb = np.frombuffer(_hashes(terms), dtype=np.uint8).reshape(-1, 12)
        if len(tb) != len(rows):
            raise ValueError("one term hash per posting")
        st = _lib.CUpdateStats()
        _check(self._h, _lib.lib().yrwi_add_postings(self._h, tb.ctypes.data, rows.ctypes.data, len(rows),
                                                     _lib.ADD_POLICIES[policy], ctypes.byref(st)))
        return {f: getattr(st, f) for f, _ in _lib.CUpdateStats._fields_}

    def remove_postings(self, urls: Sequence[bytes], terms: Optional[Sequence[bytes]] = None) -> dict:
        """IndexCell.remove(termHash, urlHashes) for every term of `terms`, or with terms=None
        Segment.removeAllUrlReferences over every list (yrwi_remove_postings).  Returns the
        call's yrwi_update_stats as a dict ("removed": rows removed)."""
        ub = np.frombuffer(_hashes(urls), dtype=np.uint8)
        tb = np.frombuffer(_hashes(terms or ()), dtype=np.uint8)
        if terms is not None and len(terms) == 0:
            return {f: 0 for f, _ in _lib.CUpdateStats._fields_}  # no term named: nothing to do
        st = _lib.CUpdateStats()
        _check(self._h, _lib.lib().yrwi_remove_postings(self._h, tb.ctypes.data if len(tb) else None, len(tb) // 12,
                                                        ub.ctypes.data if len(ub) else None, len(ub) // 12,
                                                        ctypes.byref(st)))
        return {f: getattr(st, f) for f, _ in _lib.CUpdateStats._fields_}

    @staticmethod
    def _host_args(hosts: Sequence[bytes], terms: Optional[Sequence[bytes]]):
        hb = b"".join(bytes(h) for h in hosts)
        if len(hb) != 6 * len(hosts):
            raise ValueError("host hashes must be 6 bytes")
        return np.frombuffer(hb, dtype=np.uint8), np.frombuffer(_hashes(terms or ()), dtype=np.uint8)

    def remove_hosts(self, hosts: Sequence[bytes], terms: Optional[Sequence[bytes]] = None) -> dict:
        """Removes every posting of the hosts (6-byte host hashes: url-hash characters 6..11, as
        QueryFilter's sitehash) from the lists of `terms`, or with terms=None from every list
        (yrwi_remove_hosts); no list leaves the device.  Returns the call's yrwi_update_stats as
        a dict, as remove_postings does for the url hashes of those hosts."""
        hb, tb = self._host_args(hosts, terms)
        if terms is not None and len(terms) == 0:
            return {f: 0 for f, _ in _lib.CUpdateStats._fields_}  # no term named: nothing to do
        st = _lib.CUpdateStats()
        _check(self._h, _lib.lib().yrwi_remove_hosts(self._h, tb.ctypes.data if len(tb) else None, len(tb) // 12,
                                                     hb.ctypes.data if len(hb) else None, len(hb) // 6,
                                                     ctypes.byref(st)))
        return {f: getattr(st, f) for f, _ in _lib.CUpdateStats._fields_}

    def count_hosts(self, hosts: Sequence[bytes], terms: Optional[Sequence[bytes]] = None) -> Tuple[np.ndarray, int]:
        """What remove_hosts(hosts, terms) would remove, the index unchanged (yrwi_count_hosts):
        (postings of each host in the selected lists, int64, in the order given; selected lists
        with at least one of them)."""
        hb, tb = self._host_args(hosts, terms)
        counts = np.zeros(len(hosts), dtype=np.int64)
        if terms is not None and len(terms) == 0:
            return counts, 0
        hit = ctypes.c_int64()
        _check(self._h, _lib.lib().yrwi_count_hosts(self._h, tb.ctypes.data if len(tb) else None, len(tb) // 12,
                                                    hb.ctypes.data if len(hb) else None, len(hb) // 6,
                                                    counts.ctypes.data if len(counts) else None, ctypes.byref(hit)))
        return counts, hit.value

    def url_references_raw(self, urls, terms, order: int, counts, terms_out, rows_out,
                           cap_refs: int) -> Tuple[int, "_lib.CRefStats"]:
        """yrwi_url_references as it is: urls and terms are the hashes' bytes (terms empty or None:
        every list), counts / terms_out / rows_out ctypes arrays, numpy arrays, addresses or None.
        Returns (rc, the call's yrwi_ref_stats) and raises nothing."""
        st = _lib.CRefStats()
        ub = np.frombuffer(bytes(urls or b""), dtype=np.uint8)
        tb = np.frombuffer(bytes(terms or b""), dtype=np.uint8)
        rc = _lib.lib().yrwi_url_references(self._h, tb.ctypes.data if len(tb) else None, len(tb) // 12,
                                            ub.ctypes.data if len(ub) else None, len(ub) // 12, order,
                                            _address(counts), _address(terms_out), _address(rows_out), cap_refs,
                                            ctypes.byref(st))
        return rc, st

    def url_references(self, urls: Sequence[bytes], terms: Optional[Sequence[bytes]] = None, order: str = "term",
                       fetch: bool = True, rows_out=None):
        """What remove_postings(urls, terms) would remove, the index unchanged (yrwi_url_references):
        (counts, terms, rows, stats) -- the references of each url as int64 in the order given, and
        with fetch=True every reference in `order` ("term": by term hash, then url hash; "url": by
        url hash, then term hash) as an (n, 12) uint8 array of term hashes and an (n, 40) uint8
        array of rows as get_list returns them; fetch=False: terms and rows are None.  stats is the
        yrwi_ref_stats of the last call as a dict.  rows_out: a uint8 buffer for the rows (a numpy
        array or, for rows written by the kernel itself, a host_array); the call then fetches at once
        into its 40-byte capacity and raises YRWI_E_ARG when that is too small (rows is a view of
        it).  Without rows_out a counting call sizes the buffers first."""
        o = _lib.REFS_ORDERS[order]
        ub = _hashes(urls)
        tb = _hashes(terms or ())
        counts = np.zeros(len(urls), dtype=np.int64)
        as_dict = lambda st: {f: getattr(st, f) for f, _ in _lib.CRefStats._fields_}
        cptr = counts if len(counts) else None
        if terms is not None and len(terms) == 0:  # no term named (nterms == 0 would mean every list)
            none = (np.zeros((0, 12), np.uint8), np.zeros((0, 40), np.uint8)) if fetch else (None, None)
            return (counts,) + none + (as_dict(_lib.CRefStats()),)
        if not fetch or rows_out is None:
            rc, st = self.url_references_raw(ub, tb, o, cptr, None, None, 0)
            _check(self._h, rc)
            if not fetch or st.refs == 0:
                none = (np.zeros((0, 12), np.uint8), np.zeros((0, 40), np.uint8)) if fetch else (None, None)
                return (counts,) + none + (as_dict(st),)
            buf = np.zeros(40 * st.refs, dtype=np.uint8)
        else:
            buf = rows_out if isinstance(rows_out, np.ndarray) else np.ctypeslib.as_array(rows_out)
            buf = buf.reshape(-1).view(np.uint8)
        cap = len(buf) // 40
        tout = np.zeros((max(cap, 1), 12), dtype=np.uint8)
        rc, st = self.url_references_raw(ub, tb, o, cptr, tout if cap else None, buf if cap else None, cap)
        _check(self._h, rc)
        n = st.refs if cap else 0
        return counts, tout[:n], buf[:40 * n].reshape(-1, 40), as_dict(st)

    def host_census(self, terms: Optional[Sequence[bytes]] = None, order: str = "count", min_postings: int = 1,
                    top: Optional[int] = None) -> Tuple[List[bytes], np.ndarray, dict]:
        """Which hosts have postings in the lists of `terms`, or with terms=None in every list, and
        how many each (yrwi_host_census): the hosts with at least min_postings postings, by
        order="count" (postings descending, equal counts by host hash) or "host" (ascending host
        hash), all of them or the first `top`.  Returns (6-byte host hashes, their postings as
        int64 -- what count_hosts gives for them --, the call's yrwi_census_stats as a dict).  No
        list leaves the device; with top=None a first call asks how many hosts pass (cap 0) and a
        second one fetches them."""
        o = _lib.CENSUS_ORDERS[order]
        if top is not None and top < 0:
            raise ValueError("top must not be negative")
        tb = np.frombuffer(_hashes(terms or ()), dtype=np.uint8)
        st = _lib.CCensusStats()
        if terms is not None and len(terms) == 0:  # no term named (nterms == 0 would mean every list)
            return [], np.zeros(0, dtype=np.int64), {f: 0 for f, _ in _lib.CCensusStats._fields_}
        call = lambda hosts, counts, cap, n: _check(self._h, _lib.lib().yrwi_host_census(
            self._h, tb.ctypes.data if len(tb) else None, len(tb) // 12, o, min_postings, hosts, counts, cap, n,
            ctypes.byref(st)))
        if top is None:
            call(None, None, 0, None)
            top = st.hosts_passing
        hosts = np.zeros((top, 6), dtype=np.uint8)
        counts = np.zeros(top, dtype=np.int64)
        n = ctypes.c_int64()
        call(hosts.ctypes.data if top else None, counts.ctypes.data if top else None, top, ctypes.byref(n))
        return ([bytes(h) for h in hosts[:n.value]], counts[:n.value].copy(),
                {f: getattr(st, f) for f, _ in _lib.CCensusStats._fields_})

    def url_census(self, terms: Optional[Sequence[bytes]] = None, hosts: Optional[Sequence[bytes]] = None,
                   order: str = "refs", min_refs: int = 1,
                   top: Optional[int] = None) -> Tuple[List[bytes], np.ndarray, dict]:
        """Which urls have postings in the lists of `terms`, or with terms=None in every list, and in
        how many of those lists each (yrwi_url_census): the urls with at least min_refs references
        and, with `hosts` (6-byte host hashes), of those hosts only, by order="refs" (references
        descending, equal references by url hash) or "url" (ascending url hash), all of them or the
        first `top`.  Returns (12-byte url hashes, their references as int64 -- the counts
        url_references gives for them --, the call's yrwi_ucensus_stats as a dict).  No list leaves
        the device; with top=None a first call asks how many urls pass (cap 0) and a second one
        fetches them."""
        o = _lib.UCENSUS_ORDERS[order]
        if top is not None and top < 0:
            raise ValueError("top must not be negative")
        hb, tb = self._host_args(hosts or (), terms)
        st = _lib.CUCensusStats()
        if terms is not None and len(terms) == 0:  # no term named (nterms == 0 would mean every list)
            return [], np.zeros(0, dtype=np.int64), {f: 0 for f, _ in _lib.CUCensusStats._fields_}
        call = lambda urls, refs, cap, n: _check(self._h, _lib.lib().yrwi_url_census(
            self._h, tb.ctypes.data if len(tb) else None, len(tb) // 12, hb.ctypes.data if len(hb) else None,
            len(hb) // 6, o, min_refs, urls, refs, cap, n, ctypes.byref(st)))
        if top is None:
            call(None, None, 0, None)
            top = st.urls_passing
        urls = np.zeros((top, 12), dtype=np.uint8)
        refs = np.zeros(top, dtype=np.int64)
        n = ctypes.c_int64()
        call(urls.ctypes.data if top else None, refs.ctypes.data if top else None, top, ctypes.byref(n))
        return ([bytes(u) for u in urls[:n.value]], refs[:n.value].copy(),
                {f: getattr(st, f) for f, _ in _lib.CUCensusStats._fields_})

    def host_url_census(self, terms: Optional[Sequence[bytes]] = None, order: str = "count", min_urls: int = 1,
                        top: Optional[int] = None) -> Tuple[List[bytes], np.ndarray, np.ndarray, dict]:
        """Which hosts have urls in the lists of `terms`, or with terms=None in every list, how many
        distinct urls and how many postings each (yrwi_host_url_census): the hosts with at least
        min_urls urls, by order="count" (urls descending, equal counts by host hash) or "host"
        (ascending host hash), all of them or the first `top`.  Returns (6-byte host hashes, their
        distinct urls as int64, their postings as int64 -- what host_census gives for them --, the
        call's yrwi_ucensus_stats as a dict).  With top=None a first call asks how many hosts pass."""
        o = _lib.CENSUS_ORDERS[order]
        if top is not None and top < 0:
            raise ValueError("top must not be negative")
        tb = np.frombuffer(_hashes(terms or ()), dtype=np.uint8)
        st = _lib.CUCensusStats()
        if terms is not None and len(terms) == 0:  # no term named (nterms == 0 would mean every list)
            none = np.zeros(0, dtype=np.int64)
            return [], none, none.copy(), {f: 0 for f, _ in _lib.CUCensusStats._fields_}
        call = lambda hosts, urls, posts, cap, n: _check(self._h, _lib.lib().yrwi_host_url_census(
            self._h, tb.ctypes.data if len(tb) else None, len(tb) // 12, o, min_urls, hosts, urls, posts, cap, n,
            ctypes.byref(st)))
        if top is None:
            call(None, None, None, 0, None)
            top = st.hosts_passing
        hosts = np.zeros((top, 6), dtype=np.uint8)
        urls = np.zeros(top, dtype=np.int64)
        posts = np.zeros(top, dtype=np.int64)
        n = ctypes.c_int64()
        call(hosts.ctypes.data if top else None, urls.ctypes.data if top else None,
             posts.ctypes.data if top else None, top, ctypes.byref(n))
        return ([bytes(h) for h in hosts[:n.value]], urls[:n.value].copy(), posts[:n.value].copy(),
                {f: getattr(st, f) for f, _ in _lib.CUCensusStats._fields_})

    @staticmethod
    def _retention_noop() -> dict:
        st = {f: 0 for f, _ in _lib.CRetentionStats._fields_}
        st["day_min"] = st["day_max"] = -1
        return st

    def retention_count(self, min_day: int = 0, max_refs: int = 0, terms: Optional[Sequence[bytes]] = None,
                        hist: bool = False) -> Tuple[dict, Optional[np.ndarray]]:
        """What retain(min_day, max_refs, terms) would remove, the index unchanged
        (yrwi_retention_count): the call's yrwi_retention_stats as a dict and, with hist=True, the
        65,536-entry int64 histogram of the selected rows' lastModified days before any rule (else
        None): what a caller picks the min_day from that reaches a target size."""
        tb = np.frombuffer(_hashes(terms or ()), dtype=np.uint8)
        h = np.zeros(_lib.RETENTION_DAYS, dtype=np.int64) if hist else None
        if terms is not None and len(terms) == 0:
            return self._retention_noop(), h  # no term named (nterms == 0 would mean every list)
        st = _lib.CRetentionStats()
        _check(self._h, _lib.lib().yrwi_retention_count(self._h, tb.ctypes.data if len(tb) else None, len(tb) // 12,
                                                        min_day, max_refs, h.ctypes.data if hist else None,
                                                        ctypes.byref(st)))
        return {f: getattr(st, f) for f, _ in _lib.CRetentionStats._fields_}, h

    def retain(self, min_day: int = 0, max_refs: int = 0,
               terms: Optional[Sequence[bytes]] = None) -> Tuple[dict, dict]:
        """Retention on the device (yrwi_retain): from the lists of `terms`, or with terms=None from
        every list, removes every posting whose lastModified day is below min_day (0: no age rule),
        then leaves a list that still has more than max_refs rows (0: no cap) its max_refs newest,
        equal days at the cut kept in url-hash order.  No list leaves the device.  Returns the
        call's yrwi_update_stats and yrwi_retention_stats as dicts."""
        tb = np.frombuffer(_hashes(terms or ()), dtype=np.uint8)
        if terms is not None and len(terms) == 0:
            return {f: 0 for f, _ in _lib.CUpdateStats._fields_}, self._retention_noop()  # no term named
        st, rst = _lib.CUpdateStats(), _lib.CRetentionStats()
        _check(self._h, _lib.lib().yrwi_retain(self._h, tb.ctypes.data if len(tb) else None, len(tb) // 12,
                                               min_day, max_refs, ctypes.byref(st), ctypes.byref(rst)))
        return ({f: getattr(st, f) for f, _ in _lib.CUpdateStats._fields_},
                {f: getattr(rst, f) for f, _ in _lib.CRetentionStats._fields_})

    def load_heaps(self, paths: Sequence[str], order_by_name: bool = False) -> "_lib.CLoadStats":
        """Load YaCy BLOB heap files (IndexCell's ReferenceContainerArray) into the index;
        lists already present act as the RAM cache (the files' rows win)."""
        arr = (ctypes.c_char_p * max(1, len(paths)))(*[p.encode() for p in paths])
        st = _lib.CLoadStats()
        _check(self._h, _lib.lib().yrwi_load_heaps(self._h, arr, len(paths), 1 if order_by_name else 0,
                                                   ctypes.byref(st)))
        return st

    def dump_heap(self, path: str, terms: Optional[Sequence[bytes]] = None, now_ms: int = 0) -> dict:
        """The IndexCell dump (yrwi_dump_heap): the lists of `terms`, or with terms=None every
        list, written to one BLOB heap file at `path` in term-hash order, as load_heaps reads
        it.  The file image is packed on the device window by window (YRWI_DUMP_WINDOW bytes);
        the context is unchanged.  Returns the call's yrwi_dump_stats as a dict."""
        st = _lib.CDumpStats()
        if terms is not None and len(terms) == 0:  # no term named (nterms == 0 would mean every list)
            with open(os.fspath(path) + ".prt", "wb"):
                pass
            os.replace(os.fspath(path) + ".prt", path)
            return {f: 0 for f, _ in _lib.CDumpStats._fields_}
        tb =np.frombuffer(_hashes(terms or ()), dtype=np.uint8)
        _check(self._h, _lib.lib().yrwi_dump_heap(self._h, os.fsencode(path), tb.ctypes.data if len(tb) else None,
                                                  len(tb) // 12, now_ms, ctypes.byref(st)))
        return {f: getattr(st, f) for f, _ in _lib.CDumpStats._fields_}

    def dht_select_raw(self, start: bytes, limit: bytes, max_containers: int, max_refs: int, partition_exponent: int,
                       flags: int, terms_out, cap_terms: int, part_off, rows_out, cap_rows: int) -> Tuple[int, dict]:
        """yrwi_dht_select as it is: the buffers are ctypes arrays, numpy arrays, addresses or
        None.  Returns (rc, the call's yrwi_dht_stats as a dict) and raises nothing."""
        st = _lib.CDhtStats()
        rc = _lib.lib().yrwi_dht_select(self._h, bytes(start), bytes(limit), max_containers, max_refs,
                                        partition_exponent, flags, _address(terms_out), cap_terms, _address(part_off),
                                        _address(rows_out), cap_rows, ctypes.byref(st))
        return rc, {f: getattr(st, f) for f, _ in _lib.CDhtStats._fields_}

    def dht_select(self, start: bytes, limit: bytes, max_containers: int, max_refs: int, partition_exponent: int = 4,
                   rot: bool = True, remove: bool = False, skip_private: bool = True, count_only: bool = False,
                   rows_out=None) -> "DhtSelection":
        """The DHT send path (yrwi_dht_select; Dispatcher.selectContainersEnqueueToBuffer): whole
        containers in term order from the first term >= start, up to max_containers containers
        and max_refs references, while their terms are < limit (the first one whatever it is);
        each split by the top partition_exponent bits of the url key; with remove=True taken out
        of the index.  A dry run sizes the buffers.  rows_out: a buffer for the rows (a
        host_array(ctypes.c_uint8, n) lands them without a staging copy) of at least 40 bytes per
        selected posting; None: a numpy array.  count_only=True: the stats of the dry run alone."""
        flags = (_lib.DHT_ROT if rot else 0) | (_lib.DHT_SKIP_PRIVATE if skip_private else 0)
        rc, st = self.dht_select_raw(start, limit, max_containers, max_refs, partition_exponent,
                                     flags | _lib.DHT_COUNT_ONLY, None, 0, None, None, 0)
        _check(self._h, rc)
        T, n, P = st["terms"], st["postings"], 1 << partition_exponent
        if count_only:
            return DhtSelection([], np.zeros(1, dtype=np.int64), np.zeros((0, 40), dtype=np.uint8), P, st)
        terms = np.zeros((max(1, T), 12), dtype=np.uint8)
        part_off = np.zeros(P * T + 1, dtype=np.int64)
        if rows_out is None:
            rows = np.zeros((max(1, n), 40), dtype=np.uint8)
        else:
            rows = np.ctypeslib.as_array(rows_out) if not isinstance(rows_out, np.ndarray) else rows_out
            rows = rows.reshape(-1).view(np.uint8)
            if rows.size < 40 * n:
                raise ValueError("rows_out is smaller than the selection")
            rows = rows[:40 * n].reshape(-1, 40)
        rc, st = self.dht_select_raw(start, limit, max_containers, max_refs, partition_exponent,
                                     flags | (_lib.DHT_REMOVE if remove else 0), terms, T, part_off, rows, n)
        _check(self._h, rc)
        return DhtSelection([terms[j].tobytes() for j in range(T)], part_off, rows[:n], P, st)

    def build_url_ids(self) -> None:
        """Bring the url dictionary up to date now (else the next query does)."""
        _check(self._h, _lib.lib().yrwi_build_url_ids(self._h))

    def check_url_ids(self) -> Tuple[int, int]:
        """(inconsistent postings / dictionary entries, dictionary size) after bringing
        the url ids up to date (diagnostic; 0 inconsistencies expected)."""
        bad, nurls = ctypes.c_int64(), ctypes.c_int64()
        _check(self._h, _lib.lib().yrwi_check_url_ids(self._h, ctypes.byref(bad), ctypes.byref(nurls)))
        return bad.value, nurls.value

    def index_info(self) -> dict:
        """Index maintenance counters (yrwi_index_info_get): dictionary full rebuilds /
        incremental updates, memory repacks, index arena bytes, bitmap lists."""
        info = _lib.CIndexInfo()
        _check(self._h, _lib.lib().yrwi_index_info_get(self._h, ctypes.byref(info)))
        return {f: getattr(info, f) for f, _ in _lib.CIndexInfo._fields_}

    def pair_cache_info(self) -> dict:
        """The pair cache's state and counters (yrwi_pair_cache_info_get): enabled, block and
        budget bytes, admission minimum, entries, their pieces, bytes, hits, misses, fills, dropped fills,
        evictions, invalidations, rows served."""
        info = _lib.CPairCacheInfo()
        _check(self._h, _lib.lib().yrwi_pair_cache_info_get(self._h, ctypes.byref(info)))
        return {f: getattr(info, f) for f, _ in _lib.CPairCacheInfo._fields_}

    def get_size(self, term: bytes) -> int:
        n = ctypes.c_int64()
        _check(self._h, _lib.lib().yrwi_list_size(self._h, bytes(term), ctypes.byref(n)))
        return n.value

    def get_list(self, term: bytes) -> np.ndarray:
        """Index.get(termHash) (AbstractIndex.java:116): the list's (n, 40) uint8 rows
        in url-hash order, (0, 40) when the term has no list (yrwi_get_list)."""
        n = self.get_size(term)
        out = np.zeros((max(n, 1), 40), dtype=np.uint8)
        m = ctypes.c_int64()
        _check(self._h, _lib.lib().yrwi_get_list(self._h, bytes(term), out.ctypes.data, n, ctypes.byref(m)))
        return out[:m.value]

    def stats(self) -> Tuple[int, int, int]:
        a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _check(self._h, _lib.lib().yrwi_index_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    # ---- TermSearch / joinExcludeContainers ----
    def term_search(self, include: Sequence[bytes], exclude: Sequence[bytes] = (),
                    max_distance: int = INTEGER_MAX, now_ms: int = 0,
                    urlselection: Optional[Sequence[bytes]] = None) -> np.ndarray:
        """The joined (and excluded) ReferenceContainer as (m, 40) uint8 rows
        (TermSearch.joined(); with `urlselection`, every list restricted to those urls)."""
        cap = 0
        for t in include:
            cap = max(cap, self.get_size(t))
        out = np.zeros((max(cap, 1), 40), dtype=np.uint8)
        m = ctypes.c_int64()
        if urlselection is None:
            _check(self._h, _lib.lib().yrwi_join_exclude(self._h, _hashes(include), len(include), _hashes(exclude),
                                                         len(exclude), max_distance, now_ms, out.ctypes.data, cap,
                                                         ctypes.byref(m)))
        else:
            arr, keep, _, _, _ = self._marshal([Query(include, exclude, max_distance, 1, None, "en", now_ms, None,
                                                      urlselection)], 1)
            _check(self._h, _lib.lib().yrwi_term_search(self._h, arr, out.ctypes.data, cap, ctypes.byref(m)))
        return out[:m.value].copy()

    def term_search_batch_raw(self, queries: Sequence[Query], rows_out, cap_rows: int,
                              row_off) -> Tuple[int, "_lib.CTsbStats"]:
        """yrwi_term_search_batch as it is: rows_out and row_off are ctypes arrays, numpy arrays,
        addresses or None (rows_out None: the count-only form).  Returns (rc, the call's
        yrwi_tsb_stats) and raises nothing."""
        st = _lib.CTsbStats()
        cq, keep = (self._marshal(queries, 1)[:2]) if len(queries) else (None, None)
        rc = _lib.lib().yrwi_term_search_batch(self._h, cq, len(queries), _address(rows_out), cap_rows,
                                               _address(row_off), ctypes.byref(st))
        return rc, st

    def term_search_batch(self, queries: Sequence[Query],
                          pinned: bool = False) -> Tuple[List[np.ndarray], "_lib.CTsbStats"]:
        """TermSearch.joined() of every query in one pass (yrwi_term_search_batch): the joined
        and excluded container of queries[i] as an (m_i, 40) uint8 view into one buffer, what
        term_search(...) of that query returns, and the call's yrwi_tsb_stats.  The buffer is
        sized by the sum of each query's smallest include list (no counting call first).
        pinned=True lands the rows in the index's pinned buffer without a staging copy: those
        views are valid until the next pinned call or close()."""
        cap = 0
        for q in queries:
            cap += min((self.get_size(t) for t in q.include), default=0)
        row_off = np.zeros(len(queries) + 1, dtype=np.int64)
        if pinned:
            if getattr(self, "_tsb_cap", -1) < cap:
                old = ctypes.addressof(self._tsb_buf) if getattr(self, "_tsb_buf", None) is not None else None
                if old is not None:  # the grown buffer replaces it
                    self._tsb_buf = None
                    self._pinned.remove(old)
                    _check(self._h, _lib.lib().yrwi_host_free(self._h, old))
                self._tsb_buf = self.host_array(ctypes.c_uint8, 40 * max(cap, 1))
                self._tsb_cap = cap
            buf = np.ctypeslib.as_array(self._tsb_buf)
        else:
            buf = np.zeros(40 * max(cap, 1), dtype=np.uint8)
        rc, st = self.term_search_batch_raw(queries, buf, cap, row_off)
        _check(self._h, rc)
        rows = buf[:40 * int(row_off[-1])].reshape(-1, 40)
        return [rows[row_off[i]:row_off[i + 1]] for i in range(len(queries))], st

    def host_facets_batch_raw(self, queries: Sequence[Query], order: int, max_hosts: int, hosts6_out, counts_out,
                              urls12_out, cap: int, host_off, nhosts=None,
                              nrows=None) -> Tuple[int, "_lib.CFacetStats"]:
        """yrwi_host_facets_batch as it is: the buffers are ctypes arrays, numpy arrays, addresses
        or None (hosts6_out and counts_out None: the count-only form).  Returns (rc, the call's
        yrwi_facet_stats) and raises nothing."""
        st = _lib.CFacetStats()
        cq, keep = (self._marshal(queries, 1)[:2]) if len(queries) else (None, None)
        rc = _lib.lib().yrwi_host_facets_batch(self._h, cq, len(queries), order, max_hosts, _address(hosts6_out),
                                               _address(counts_out), _address(urls12_out), cap, _address(host_off),
                                               _address(nhosts), _address(nrows), ctypes.byref(st))
        return rc, st

    def host_facets_batch(self, queries: Sequence[Query], order: str = "count", max_hosts: int = 0,
                          urls: bool = True):
        """The hosts of every query's joined container (yrwi_host_facets_batch): per query
        (hosts, counts, urls) -- the six-character host hashes as a list of bytes, their postings
        as an int64 array and, with urls=True, each host's smallest url hash as a list of bytes
        (else None) -- in `order` ("count": postings descending, ties by host; "host": ascending
        host hash), the first max_hosts of them (0: all).  Returns (facets, nhosts, nrows, stats):
        nhosts[i] the distinct hosts and nrows[i] the rows of query i's container, and the
        call's yrwi_facet_stats.  The buffers are sized by the sum of each query's smallest
        include list (no counting call first)."""
        nq = len(queries)
        cap = 0
        for q in queries:
            m = min((self.get_size(t) for t in q.include), default=0)
            cap += min(m, max_hosts) if max_hosts > 0 else m
        h6 = np.zeros(6 * max(cap, 1), dtype=np.uint8)
        cnt = np.zeros(max(cap, 1), dtype=np.int64)
        u12 = np.zeros(12 * max(cap, 1), dtype=np.uint8) if urls else None
        off = np.zeros(nq + 1, dtype=np.int64)
        nhosts = np.zeros(max(nq, 1), dtype=np.int64)
        nrows = np.zeros(max(nq, 1), dtype=np.int64)
        rc, st = self.host_facets_batch_raw(queries, _lib.FACETS_ORDERS[order], max_hosts, h6, cnt, u12, cap, off,
                                            nhosts, nrows)
        _check(self._h, rc)
        hb = h6.tobytes()
        ub = u12.tobytes() if urls else b""
        out = []
        for i in range(nq):
            a, b = int(off[i]), int(off[i + 1])
            out.append(([hb[6 * j:6 * j + 6] for j in range(a, b)], cnt[a:b],
                        [ub[12 * j:12 * j + 12] for j in range(a, b)] if urls else None))
        return out, nhosts[:nq], nrows[:nq], st

    # ---- ReferenceOrder.normalizeWith + cardinal ----
    def normalize_score(self, rows: np.ndarray, profile: Optional[RankingProfile] = None, language: str = "en",
                        now_ms: int = 0) -> np.ndarray:
        rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, 40)
        out = np.zeros(len(rows), dtype=np.int64)
        prof = profile or RankingProfile()
        _check(self._h, _lib.lib().yrwi_normalize_score(self._h, rows.ctypes.data, len(rows), ctypes.byref(prof.c),
                                                        language.encode(), now_ms, out.ctypes.data))
        return out

    # ---- search events: containers arriving one after another ----
    def event(self, profile: Optional[RankingProfile] = None, language: str = "en", now_ms: int = 0, k: int = 100,
              filter: Optional[QueryFilter] = None, max_postings: int = 1 << 16) -> "SearchEvent":
        return SearchEvent(self, profile, language, now_ms, k, filter, max_postings)

    def reference_order(self, profile: Optional[RankingProfile] = None, language: str = "en", now_ms: int = 0,
                        max_hosts: int = 1 << 16) -> "SearchEvent":
        """A SearchEvent's ReferenceOrder alone (yrwi_event_open_order, what
        GpuReferenceOrder holds): order() and authority(); no url set, no stack."""
        return SearchEvent(self, profile, language, now_ms, 1, None, 0, order_only_hosts=max_hosts)

    def add_rwis(self, arrivals: Sequence[Tuple["SearchEvent", np.ndarray, bool]]) -> List[int]:
        """Applies (event, rows (n, 40) uint8, local) arrivals in order, events in
        parallel (yrwi_event_add); returns the per-arrival codes (raises on the first
        error)."""
        arr = (_lib.CArrival * max(1, len(arrivals)))()
        keep = []
        for i, (ev, rows, local) in enumerate(arrivals):
            r = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, 40)
            keep.append(r)
            arr[i].ev = ev._e
            arr[i].rows40 = r.ctypes.data if len(r) else None
            arr[i].n = len(r)
            arr[i].local = int(bool(local))
        rc = _lib.lib().yrwi_event_add(self._h, arr, len(arrivals))
        codes = [arr[i].rc for i in range(len(arrivals))]
        _check(self._h, rc)
        return codes

    def add_local_rwis(self, arrivals: Sequence[Tuple["SearchEvent", "Query"]],
                       stats: Optional["_lib.CLocalStats"] = None) -> List[int]:
        """Applies (event, Query) device-local arrivals in order, events in parallel
        (yrwi_event_add_local): each event receives the joined and excluded container of its
        query (include, exclude, max_distance, now_ms, urlselection) as its local arrival.
        Returns the rows that arrived per arrival; raises on the first error, the exception
        carrying the per-arrival codes as `codes`.  stats: a CLocalStats to fill."""
        n = len(arrivals)
        if n == 0:
            return []
        cq, keep, _, _, _ = self._marshal([q for _, q in arrivals], 1)
        arr = (_lib.CLocalArrival * n)()
        for i, (ev, _) in enumerate(arrivals):
            arr[i].ev = ev._e
            arr[i].q = ctypes.pointer(cq[i])
        rc = _lib.lib().yrwi_event_add_local(self._h, arr, n, ctypes.byref(stats) if stats is not None else None)
        try:
            _check(self._h, rc)
        except YrwiError as e:
            e.codes = [arr[i].rc for i in range(n)]
            raise
        return [arr[i].m for i in range(n)]

    # ---- index abstracts (compressIndex) and the secondary search ----
    def index_abstracts(self, terms: Sequence[bytes], exclude: Optional[bytes] = None) -> List[bytes]:
        """searchConjunction + WordReferenceFactory.compressIndex per term; [] when
        a term has no list."""
        L = _lib.lib()
        sizes = [self.get_size(t) for t in terms]
        cap = sum(14 * n + 2 for n in sizes) + 2
        out = ctypes.create_string_buffer(max(1, cap))
        offs = (ctypes.c_int64 * (len(terms) + 1))()
        nout = ctypes.c_int32()
        _check(self._h, L.yrwi_index_abstracts(self._h, _hashes(terms), len(terms), exclude, out, cap, offs,
                                               ctypes.byref(nout)))
        raw = out.raw
        return [raw[offs[i]:offs[i + 1]] for i in range(nout.value)]

    def secondary_search(self, abstracts: Sequence[Tuple[bytes, bytes, bytes]], nwords_query: int, mypeer: bytes,
                         checked: Sequence[bytes] = (), decode: bool = True):
        """abstracts: (word, peer, text) in arrival order.  Returns (join [(url, peer)],
        words, plan [(peer, urls, words)]); with decode=False only (njoin, nplan)."""
        L = _lib.lib()
        arr = (_lib.CAbstract * max(1, len(abstracts)))()
        bufs = []
        total = 0
        for i, (w, p, t) in enumerate(abstracts):
            b = ctypes.create_string_buffer(bytes(t), max(1, len(t)))
            bufs.append(b)
            arr[i].word[:] = list(bytes(w))
            arr[i].peer[:] = list(bytes(p))
            arr[i].text = ctypes.cast(b, ctypes.c_void_p)
            arr[i].len = len(t)
            total += len(t)
        cap = total // 6 + 1
        ju = ctypes.create_string_buffer(12 * cap)
        jp = ctypes.create_string_buffer(12 * cap)
        pu = ctypes.create_string_buffer(12 * cap)
        plan = (_lib.CPeerRequest * max(1, len(abstracts)))()
        wo = ctypes.create_string_buffer(12 * 32)
        nj = ctypes.c_int64()
        npl = ctypes.c_int32()
        nw = ctypes.c_int32()
        _check(self._h, L.yrwi_secondary_search(self._h, arr, len(abstracts), nwords_query, bytes(mypeer),
                                                b"".join(bytes(c) for c in checked) or None, len(checked),
                                                ju, jp, cap, ctypes.byref(nj), plan, len(plan), ctypes.byref(npl),
                                                pu, wo, ctypes.byref(nw)))
        if not decode:
            return nj.value, npl.value
        wr, jur, jpr, pur = wo.raw, ju.raw, jp.raw, pu.raw  # each .raw is a copy: take them once
        words = [wr[12 * i:12 * i + 12] for i in range(nw.value)]
        join = [(jur[12 * i:12 * i + 12], jpr[12 * i:12 * i + 12]) for i in range(nj.value)]
        reqs = []
        for i in range(npl.value):
            r = plan[i]
            urls = [pur[12 * j:12 * j + 12] for j in range(r.url_off, r.url_off + r.url_n)]
            reqs.append((bytes(r.peer), urls, [words[b] for b in range(nw.value) if (r.words >> b) & 1]))
        return join, words, reqs

    # ---- ReferenceOrder.cardinal(URIMetadataNode): the Solr node stack ----
    def score_nodes(self, nodes: Sequence[dict], profile: Optional[RankingProfile] = None, language: str = "en",
                    maxdomcount: int = 0) -> np.ndarray:
        """nodes: dicts with urlhash, virtual_age, wordsintitle, wordcount, llocal, lother,
        flags (4 bytes), host_count, language (str or None) -- the URIMetadataNode fields
        cardinal reads (ReferenceOrder.java:267-296)."""
        n = len(nodes)
        arr = (_lib.CNode * max(1, n))()
        for i, d in enumerate(nodes):
            arr[i].urlhash[:] = list(bytes(d["urlhash"]))
            for f in ("virtual_age", "wordsintitle", "wordcount", "llocal", "lother", "host_count"):
                setattr(arr[i], f, int(d.get(f, 0)))
            arr[i].flags[:] = list(bytes(d.get("flags", b"\0\0\0\0"))[:4])
            arr[i].language = (d.get("language") or "").encode()[:7]
        out = np.zeros(max(1, n), dtype=np.int64)
        prof = profile or RankingProfile()
        _check(self._h, _lib.lib().yrwi_score_nodes(self._h, arr, n, ctypes.byref(prof._c), language.encode(),
                                                    maxdomcount, out.ctypes.data))
        return out[:n]

    # ---- full query: TermSearch -> normalise -> cardinal -> top-k ----
    def search(self, include: Sequence[bytes], exclude: Sequence[bytes] = (), profile: Optional[RankingProfile] = None,
               language: str = "en", max_distance: int = INTEGER_MAX, now_ms: int = 0, k: int = 100,
               stats: Optional[CStats] = None, filter: Optional[QueryFilter] = None, rows: bool = False) -> List[Hit]:
        """rows=True: every Hit carries its joined posting's 40-byte row (yrwi_query_rows)."""
        q = Query(include, exclude, max_distance, k, profile, language, now_ms, filter)
        if not rows:
            return self.search_batch([q], stats=stats)[0]
        arr, keep, hits, nout, kmax = self._marshal([q], None)
        st = stats if stats is not None else CStats()
        rbuf = np.zeros((kmax, 40), dtype=np.uint8)
        _check(self._h, _lib.lib().yrwi_query_rows(self._h, arr, hits, rbuf.ctypes.data, nout, ctypes.byref(st)))
        return self._unmarshal(1, kmax, hits, nout, rbuf)[0]

    def _marshal(self, queries: Sequence[Query], kmax: Optional[int]):
        nq = len(queries)
        kmax = kmax or max(1, min(MAX_RESULTS_RWI, max(q.k for q in queries)))
        arr = (CQuery * nq)()
        keep = []
        for i, q in enumerate(queries):
            inc = _hashes(q.include)
            exc = _hashes(q.exclude)
            ib = ctypes.create_string_buffer(inc, max(1, len(inc)))
            eb = ctypes.create_string_buffer(exc, max(1, len(exc)))
            prof = q.profile or RankingProfile()
            keep += [ib, eb, prof]
            arr[i].incl = ctypes.cast(ib, ctypes.c_void_p)
            arr[i].nincl = len(q.include)
            arr[i].excl = ctypes.cast(eb, ctypes.c_void_p)
            arr[i].nexcl = len(q.exclude)
            arr[i].max_distance = q.max_distance
            arr[i].k = q.k
            arr[i].profile = ctypes.pointer(prof.c)
            arr[i].language = q.language.encode()[:7]
            arr[i].now_ms = q.now_ms
            if q.filter is not None:
                keep.append(q.filter)
                arr[i].filter = ctypes.pointer(q.filter.c)
            if q.urlselection is not None:
                sb = ctypes.create_string_buffer(_hashes(q.urlselection), max(1, 12 * len(q.urlselection)))
                keep.append(sb)
                arr[i].urlselection = ctypes.cast(sb, ctypes.c_void_p)
                arr[i].nurlselection = len(q.urlselection)
        hits = (CHit * (nq * kmax))()
        nout = (ctypes.c_int32 * nq)()
        return arr, keep, hits, nout, kmax

    @staticmethod
    def _unmarshal(nq: int, kmax: int, hits, nout, rows: Optional[np.ndarray] = None) -> List[List[Hit]]:
        """rows: the (nq * kmax, 40) uint8 rows buffer of a search with rows, or None"""
        if rows is None:
            return [[Hit(bytes(hits[i * kmax + j].urlhash), hits[i * kmax + j].score, hits[i * kmax + j].tiebreak)
                     for j in range(nout[i])] for i in range(nq)]
        return [[Hit(bytes(hits[i * kmax + j].urlhash), hits[i * kmax + j].score, hits[i * kmax + j].tiebreak,
                     rows[i * kmax + j].tobytes()) for j in range(nout[i])] for i in range(nq)]

    def search_batch(self, queries: Sequence[Query], stats: Optional[CStats] = None,
                     kmax: Optional[int] = None, rows: bool = False) -> List[List[Hit]]:
        """rows=True: every Hit carries its joined posting's 40-byte row (yrwi_query_batch_rows)."""
        nq = len(queries)
        if nq == 0:
            return []
        arr, keep, hits, nout, kmax = self._marshal(queries, kmax)
        st = stats if stats is not None else CStats()
        if not rows:
            _check(self._h, _lib.lib().yrwi_query_batch(self._h, arr, nq, kmax, hits, nout, ctypes.byref(st)))
            return self._unmarshal(nq, kmax, hits, nout)
        rbuf = np.zeros((nq * kmax, 40), dtype=np.uint8)
        self.search_batch_rows_raw(arr, nq, kmax, hits, rbuf.ctypes.data, nout, st)
        return self._unmarshal(nq, kmax, hits, nout, rbuf)

    def submit(self, queries: Sequence[Query], kmax: Optional[int] = None, rows: bool = False) -> "PendingBatch":
        """Start a batch asynchronously (yrwi_query_batch_submit); .result() waits for it.
        Batches run on the context's lanes in submission order (ticket t on lane t % lanes).
        rows=True: the result's Hits carry their rows (yrwi_query_batch_rows_submit)."""
        nq = len(queries)
        arr, keep, hits, nout, kmax = self._marshal(queries, kmax) if nq else ((CQuery * 1)(), [], (CHit * 1)(),
                                                                               (ctypes.c_int32 * 1)(), 1)
        st = CStats()
        if not rows:
            ticket = self.submit_raw(arr, nq, kmax, hits, nout, st)
            return PendingBatch(self, ticket, nq, kmax, (arr, keep, hits, nout, st))
        rbuf = np.zeros((max(1, nq) * kmax, 40), dtype=np.uint8)
        ticket = self.submit_rows_raw(arr, nq, kmax, hits, rbuf.ctypes.data, nout, st)
        return PendingBatch(self, ticket, nq, kmax, (arr, keep, hits, nout, st), rbuf)

    def search_batch_raw(self, cq, nq: int, kmax: int, hits, nout, st) -> None:
        """Zero-marshalling batch call for benchmarks (pre-built ctypes arrays).
        st None: no statistics (yrwi_stats* NULL, no HIP events: the production call)."""
        _check(self._h, _lib.lib().yrwi_query_batch(self._h, cq, nq, kmax, hits, nout,
                                                    ctypes.byref(st) if st is not None else None))

    def search_batch_rows_raw(self, cq, nq: int, kmax: int, hits, rows, nout, st) -> None:
        """search_batch_raw with the hits' rows (yrwi_query_batch_rows).  rows: a buffer of
        nq * kmax * 40 bytes -- a ctypes array (host_array(ctypes.c_uint8, n): pinned, written
        by the GPU directly when 8-byte aligned) or an address; None: no rows."""
        _check(self._h, _lib.lib().yrwi_query_batch_rows(self._h, cq, nq, kmax, hits, _address(rows), nout,
                                                         ctypes.byref(st) if st is not None else None))

    def submit_rows_raw(self, cq, nq: int, kmax: int, hits, rows, nout, st) -> int:
        """submit_raw with the hits' rows (yrwi_query_batch_rows_submit); `rows` as in
        search_batch_rows_raw, alive until wait(ticket)."""
        t = ctypes.c_int64()
        _check(self._h, _lib.lib().yrwi_query_batch_rows_submit(self._h, cq, nq, kmax, hits, _address(rows), nout,
                                                                ctypes.byref(st) if st is not None else None,
                                                                ctypes.byref(t)))
        return t.value

    # ---- asynchronous batches (yrwi_query_batch_submit / _wait) ----
    def submit_raw(self, cq, nq: int, kmax: int, hits, nout, st) -> int:
        """Start a batch; the ctypes buffers must stay alive until wait(ticket)."""
        t = ctypes.c_int64()
        _check(self._h, _lib.lib().yrwi_query_batch_submit(self._h, cq, nq, kmax, hits, nout,
                                                           ctypes.byref(st) if st is not None else None,
                                                           ctypes.byref(t)))
        return t.value

    def wait(self, ticket: int) -> None:
        _check(self._h, _lib.lib().yrwi_query_batch_wait(self._h, ticket))

    def host_array(self, ctype, n: int):
        """A ctypes array of n `ctype` in pinned host memory (GPU writes results into it directly)."""
        p = ctypes.c_void_p()
        _check(self._h, _lib.lib().yrwi_host_alloc(self._h, ctypes.sizeof(ctype) * max(1, n), ctypes.byref(p)))
        arr = (ctype * max(1, n)).from_address(p.value)
        self._pinned = getattr(self, "_pinned", []) + [p.value]
        return arr


class PendingBatch:
    """A submitted batch: its ctypes buffers stay alive until result() collects it."""

    def __init__(self, index: RWIIndex, ticket: int, nq: int, kmax: int, bufs, rows: Optional[np.ndarray] = None):
        self.index, self.ticket, self.nq, self.kmax, self._bufs = index, ticket, nq, kmax, bufs
        self._rows = rows  # the rows buffer of submit(rows=True)

    def result(self) -> List[List[Hit]]:
        self.index.wait(self.ticket)
        _, _, hits, nout, _ = self._bufs
        return RWIIndex._unmarshal(self.nq, self.kmax, hits, nout, self._rows)


def unique_id() -> bytes:
    buf = ctypes.create_string_buffer(128)
    _check(None, _lib.lib().yrwi_get_unique_id(buf))
    return buf.raw
