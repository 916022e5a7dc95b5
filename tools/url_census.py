"""Time the url census on the C2 index (one GPU): yrwi_url_census in both orders and
yrwi_host_url_census, each path forced (YRWI_UCENSUS_PATH = hist | sort) and as the call chooses, over
selections of 1, 16, 256 and 4096 terms and of every list, on two indexes: C2 as generated and C2
re-hosted to URL_CENSUS_H hosts (default 4096; tools/index_hosts.py's rehost()).  Against

  (a) get_list of every selected term (40 B per posting to the host) and a numpy group-by on the
      url hash: the only route without the call.  Run once per selection; the device results of both
      forced paths, both orders and the host form must equal it before a time is printed;
  (b) host_census over the same selection: the same postings through the 9 B per posting pass.

The C calls are timed as they are (ctypes, buffers allocated before): the call with cap 0 that sizes
the result and the call that fetches all of it, URL_CENSUS_REPS times (default 3), median and
min-max range, and the counting kernels alone (t_count_ns).  The statistics of a call are printed as
they come.  One JSON line to stdout (URL_CENSUS_OUT: also to that file); the rows of the table for
DESIGN.md section 8 go to stderr."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import index_hosts as ih  # noqa: E402  (rehost, key_of, ms, summary)

STAT_KEYS = ("lists", "postings", "dict_urls", "urls", "urls_hosted", "urls_passing", "max_refs", "hosts",
             "hosts_passing", "path", "launches", "syncs", "t_count_ns", "t_total_ns")
SELECTIONS = (1, 16, 256, 4096, None)
PATHS = ("hist", "sort", None)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def keys72(chars):
    """(n, 12) url-hash characters -> (high 36 bits, low 36 bits = the host) of the 72-bit key"""
    return ih.key_of(chars[:, :6]), ih.key_of(chars[:, 6:12])


class Census:
    """the two C calls on one index and one selection, into buffers of `cap` results"""

    def __init__(self, ix, terms, cap_urls, cap_hosts):
        from yacy_search_server_amd import _lib
        self.L, self.lib, self.ix = _lib, _lib.lib(), ix
        self.tb = np.frombuffer(b"".join(terms), dtype=np.uint8) if terms else np.zeros(0, np.uint8)
        self.urls, self.refs = np.zeros((max(cap_urls, 1), 12), np.uint8), np.zeros(max(cap_urls, 1), np.int64)
        self.hosts = np.zeros((max(cap_hosts, 1), 6), np.uint8)
        self.hurls, self.hposts = np.zeros(max(cap_hosts, 1), np.int64), np.zeros(max(cap_hosts, 1), np.int64)

    def _done(self, rc, n, st):
        assert rc == 0, (rc, self.lib.yrwi_last_error(self.ix._h))
        return n.value, {k: getattr(st, k) for k in STAT_KEYS}

    def url(self, order, cap):
        n, st = ctypes.c_int64(), self.L.CUCensusStats()
        rc = self.lib.yrwi_url_census(self.ix._h, self.tb.ctypes.data if len(self.tb) else None, len(self.tb) // 12,
                                      None, 0, order, 1, self.urls.ctypes.data if cap else None,
                                      self.refs.ctypes.data if cap else None, cap, ctypes.byref(n), ctypes.byref(st))
        return self._done(rc, n, st)

    def host(self, order, cap):
        n, st = ctypes.c_int64(), self.L.CUCensusStats()
        rc = self.lib.yrwi_host_url_census(self.ix._h, self.tb.ctypes.data if len(self.tb) else None,
                                           len(self.tb) // 12, order, 1, self.hosts.ctypes.data if cap else None,
                                           self.hurls.ctypes.data if cap else None,
                                           self.hposts.ctypes.data if cap else None, cap, ctypes.byref(n),
                                           ctypes.byref(st))
        return self._done(rc, n, st)


def route_a(ix, terms):
    """get_list of every term and the group-by on the host -> (times, the expected results)"""
    t_get = t_np = 0.0
    hi, lo = [], []
    for t in terms:
        dt, r = ih.ms(lambda: ix.get_list(t))
        t_get += dt
        dt, (h, l) = ih.ms(lambda: keys72(r[:, :12]))
        t_np += dt
        hi.append(h)
        lo.append(l)

    def group():
        h, l = np.concatenate(hi), np.concatenate(lo)
        o = np.lexsort((l, h))
        h, l = h[o], l[o]
        head = np.ones(len(h), dtype=bool)
        head[1:] = (h[1:] != h[:-1]) | (l[1:] != l[:-1])
        at = np.flatnonzero(head)
        return h[at], l[at], np.diff(np.concatenate([at, [len(h)]])).astype(np.int64)

    dt, (uh, ul, uc) = ih.ms(group)
    t_np += dt
    by_refs = np.lexsort((ul, uh, -uc))
    hk, inv = np.unique(ul, return_inverse=True)
    hn = np.bincount(inv).astype(np.int64)
    hp = np.bincount(inv, weights=uc).astype(np.int64)
    by_count = np.lexsort((hk, -hn))
    exp = {"url": (uh, ul, uc), "refs": (uh[by_refs], ul[by_refs], uc[by_refs]), "host": (hk, hn, hp),
           "count": (hk[by_count], hn[by_count], hp[by_count])}
    return {"ms": round(t_get + t_np, 3), "get_list_ms": round(t_get, 3), "numpy_ms": round(t_np, 3)}, exp


def check(c, form, order_name, order, exp, n):
    if form == "url":
        h, l = keys72(c.urls[:n])
        eh, el, ec = exp[order_name]
        assert n == len(eh) and (h == eh).all() and (l == el).all() and (c.refs[:n] == ec).all(), (form, order_name)
    else:
        k = ih.key_of(c.hosts[:n])
        ek, en, ep = exp[order_name]
        assert n == len(ek) and (k == ek).all() and (c.hurls[:n] == en).all() and (c.hposts[:n] == ep).all(), order_name


def measure(label, hashes, rows, sizes, reps):
    """one index: resident, every selection checked and timed -> the record of `label`"""
    from yacy_search_server_amd import RWIIndex, _lib
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    ids = [t for t in range(len(sizes)) if sizes[t]]
    ix = RWIIndex(0)
    for t in ids:
        ix.add(hashes[t], rows[offsets[t]:offsets[t] + sizes[t]])
    ix.build_url_ids()
    log(label, "resident:", int(sizes.sum()), "postings in", len(ids), "lists")
    forms = (("url", "url", _lib.UCENSUS_BY_URL), ("url", "refs", _lib.UCENSUS_BY_REFS),
             ("host", "count", _lib.CENSUS_BY_COUNT))
    out = {}
    for nsel in SELECTIONS:
        if nsel is not None and nsel > len(ids):
            continue
        pick = ids if nsel is None else [ids[(i * len(ids)) // nsel] for i in range(nsel)]
        terms = [bytes(hashes[t]) for t in pick]
        ta, exp = route_a(ix, terms)
        npost, nurl, nhost = int(sum(sizes[t] for t in pick)), len(exp["url"][0]), len(exp["host"][0])
        rec = {"terms": len(terms), "postings": npost, "urls": nurl, "hosts": nhost, "route_a": ta}
        c = Census(ix, None if nsel is None else terms, nurl, nhost)
        calls = []
        for _ in range(reps):
            dt, _ = ih.ms(lambda: ix.host_census(None if nsel is None else terms, "count", top=0))
            calls.append(dt)
        rec["host_census_cap0"] = ih.summary(calls)
        for path in PATHS:
            if path:
                os.environ["YRWI_UCENSUS_PATH"] = path
            else:
                os.environ.pop("YRWI_UCENSUS_PATH", None)
            for form, oname, order in forms:
                fn = c.url if form == "url" else c.host
                full = nurl if form == "url" else nhost
                n, st = fn(order, full)
                check(c, form, oname, order, exp, n)
                if form == "host":
                    check(c, form, "host", _lib.CENSUS_BY_HOST, exp, c.host(_lib.CENSUS_BY_HOST, full)[0])
                two, stats = [], []
                for _ in range(reps):
                    d0, _ = ih.ms(lambda: fn(order, 0))
                    d1, (_, st) = ih.ms(lambda: fn(order, full))
                    two.append(d0 + d1)
                    stats.append(st)
                top, _ = ih.ms(lambda: fn(order, min(100, full)))
                r = {"two_calls": ih.summary(two), "top_100_one_call_ms": round(top, 3),
                     "count_ms": ih.summary([s["t_count_ns"] / 1e6 for s in stats]),
                     "last_call_ms": ih.summary([s["t_total_ns"] / 1e6 for s in stats]),
                     "stats": stats[-1], "faster_than_route_a": ta["ms"] > float(np.median(two))}
                rec["%s_%s_%s" % (path or "auto", form, oname)] = r
                log("| %s | %s | %s | %s/%s | %s | %.3f (%.3f-%.3f) | %.3f | %d / %d | %.3f | %.1f |" % (
                    label, len(terms), npost, form, oname, (path or "auto") + ("=" + ("sort" if st["path"] else "hist")),
                    r["two_calls"]["median_ms"], r["two_calls"]["min_ms"], r["two_calls"]["max_ms"],
                    r["count_ms"]["median_ms"], st["launches"], st["syncs"], rec["host_census_cap0"]["median_ms"],
                    ta["ms"]))
        os.environ.pop("YRWI_UCENSUS_PATH", None)
        out["all" if nsel is None else str(nsel)] = rec
        log(label, nsel, json.dumps(rec))
    ix.close()
    return out


def main():
    from yacy_search_server_amd import synth
    name = os.environ.get("URL_CENSUS_CONFIG", "C2")
    cfg = synth.preset(name)
    reps = max(1, int(os.environ.get("URL_CENSUS_REPS", "3")))
    H = int(os.environ.get("URL_CENSUS_H", "4096"))
    idx = synth.build_index(cfg)
    log("index built")
    log("| index | terms | postings | form/order | path | two calls, ms | counting kernels, ms | launches / syncs | "
        "host_census cap 0, ms | get_list + numpy, ms |")
    out = {"config": name, "repeats": reps}
    try:
        import bench
        out.update(bench.source_identity())
    except Exception:  # the identity is a label only
        pass
    out["as_generated"] = measure("as generated", idx.hashes, idx.rows, idx.sizes, reps)
    rows, sizes, rank = ih.rehost(idx.rows, idx.sizes.copy(), H)  # (in place where it can: the raw index is done with)
    del rank
    out["rehosted_%d" % H] = measure("re-hosted to %d" % H, idx.hashes, rows, sizes, reps)
    line = json.dumps(out)
    print(line)
    if os.environ.get("URL_CENSUS_OUT"):
        with open(os.environ["URL_CENSUS_OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
