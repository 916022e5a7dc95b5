"""What the host facets of many queries cost on the C2 corpus (one GPU), two ways in one process
over one resident index.  QUERY_FACETS_N (default 256) two-term queries of the C2 stream:

  baseline   the only way to this answer before yrwi_host_facets_batch: one
             yrwi_term_search_batch into a pinned buffer (every kept row crosses PCIe, 40 bytes
             each) and a numpy group-by over the bytes 6..11 of the rows of every query;
  facets     one yrwi_host_facets_batch: the group-by on the device, only the (host, count, url)
             triples cross.

  python tools/query_facets.py [--src LABEL]

The facets arm runs in both orders, with max_hosts 0 and 10, with and without urls; the baseline
orders and cuts its groups on the host to the same form.  ms per cell is the wall time of the C
call (the baseline: the C call and the numpy group-by), the median of QUERY_FACETS_REPS (default
5) timed repeats after QUERY_FACETS_WARMUP (default 1) untimed ones, with the min-max range; the
arms alternate.  Every result of the facets arm is compared with the baseline's for equality.
The call's yrwi_facet_stats are printed per cell.  No speed-up is asserted.  One JSON line to
stdout and to profiles/query_facets_<src>.json (QUERY_FACETS_CONFIG: another preset;
QUERY_FACETS_OUT: another file)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from yacy_search_server_amd import RWIIndex, _lib, synth  # noqa: E402
from yacy_search_server_amd._lib import CFacetStats, CQuery, CTsbStats  # noqa: E402

NOW_MS = 20741 * 86400000
ALPHA = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"


def summary(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=None, help="label of the output file (default: the source identity)")
    args = ap.parse_args()
    name = os.environ.get("QUERY_FACETS_CONFIG", "C2")
    N = max(1, int(os.environ.get("QUERY_FACETS_N", "256")))
    reps = max(1, int(os.environ.get("QUERY_FACETS_REPS", "5")))
    warmup = max(1, int(os.environ.get("QUERY_FACETS_WARMUP", "1")))
    import bench
    cfg = synth.preset(name)
    idx = synth.build_index(cfg)
    ix = RWIIndex(0)
    for t in range(cfg.n_terms):
        if idx.sizes[t]:
            ix.add(idx.hashes[t], idx.list_rows(t))
    ix.build_url_ids()
    print("index resident", file=sys.stderr, flush=True)
    L = _lib.lib()
    qs = bench.draws(cfg, N, 2, 2, 0, None, 1)[0]
    keep = []
    cq = (CQuery * N)()
    for i, (inc, exc) in enumerate(qs):
        ib = ctypes.create_string_buffer(b"".join(idx.hashes[t] for t in inc), 12 * max(1, len(inc)))
        keep.append(ib)
        cq[i].incl = ctypes.cast(ib, ctypes.c_void_p)
        cq[i].nincl = len(inc)
        cq[i].max_distance = 2147483647
        cq[i].k = 1
        cq[i].language = b"en"
        cq[i].now_ms = NOW_MS

    def check(rc, what):
        if rc:
            raise RuntimeError(f"{what}: {rc} {(L.yrwi_last_error(ix._h) or b'').decode(errors='replace')}")

    cap = sum(int(min(idx.sizes[t] for t in inc)) for inc, _ in qs)  # rows, and so hosts, at most
    pinned = np.ctypeslib.as_array(ix.host_array(ctypes.c_uint8, 40 * max(cap, 1)))
    pinned[:] = 0
    row_off = np.zeros(N + 1, dtype=np.int64)
    h6 = np.zeros(6 * max(cap, 1), dtype=np.uint8)
    cnt = np.zeros(max(cap, 1), dtype=np.int64)
    u12 = np.zeros(12 * max(cap, 1), dtype=np.uint8)
    host_off, nhosts, nrows = (np.zeros(N + 1, dtype=np.int64) for _ in range(3))
    lut = np.full(256, -1, dtype=np.int64)
    lut[np.frombuffer(ALPHA, dtype=np.uint8)] = np.arange(64)
    shifts = 6 * np.arange(5, -1, -1)

    def baseline(order, mh):
        """-> ms, per query (hosts (m, 6) uint8, counts, urls (m, 12) uint8), stats"""
        st = CTsbStats()
        t0 = time.perf_counter()
        check(L.yrwi_term_search_batch(ix._h, cq, N, pinned.ctypes.data, cap, row_off.ctypes.data, ctypes.byref(st)),
              "yrwi_term_search_batch")
        rows = pinned[:40 * int(row_off[N])].reshape(-1, 40)
        out = []
        for i in range(N):
            r = rows[row_off[i]:row_off[i + 1]]
            keys = (lut[r[:, 6:12]] << shifts).sum(axis=1)
            _, first, counts = np.unique(keys, return_index=True, return_counts=True)
            if order == 1:
                o = np.argsort(-counts, kind="stable")
                first, counts = first[o], counts[o]
            if mh:
                first, counts = first[:mh], counts[:mh]
            out.append((r[first, 6:12], counts, r[first, :12]))
        return (time.perf_counter() - t0) * 1e3, out, st

    def facets(order, mh, urls):
        st = CFacetStats()
        t0 = time.perf_counter()
        check(L.yrwi_host_facets_batch(ix._h, cq, N, order, mh, h6.ctypes.data, cnt.ctypes.data,
                                       u12.ctypes.data if urls else None, cap, host_off.ctypes.data,
                                       nhosts.ctypes.data, nrows.ctypes.data, ctypes.byref(st)),
              "yrwi_host_facets_batch")
        return (time.perf_counter() - t0) * 1e3, st

    fields = [f for f, _ in CFacetStats._fields_]
    cells = []
    for order, oname in ((0, "host"), (1, "count")):
        for mh in (0, 10):
            for urls in (True, False):
                ms_b, ms_f, st, base = [], [], None, None
                for r in range(warmup + reps):
                    tb, base, tst = baseline(order, mh)
                    tf, st = facets(order, mh, urls)
                    if r >= warmup:
                        ms_b.append(tb)
                        ms_f.append(tf)
                equal = True
                for i in range(N):
                    a, b = int(host_off[i]), int(host_off[i + 1])
                    bh, bc, bu = base[i]
                    equal &= b - a == len(bc) and np.array_equal(h6[6 * a:6 * b].reshape(-1, 6), bh)
                    equal &= np.array_equal(cnt[a:b], bc) and nrows[i] == row_off[i + 1] - row_off[i]
                    if urls:
                        equal &= np.array_equal(u12[12 * a:12 * b].reshape(-1, 12), bu)
                assert equal, ("the facets differ from the baseline's", oname, mh, urls)
                sd = {f: int(getattr(st, f)) for f in fields}
                assert sd["device_allocs"] == 0 and sd["rows_kept"] == int(row_off[N]), sd
                cell = {"order": oname, "max_hosts": mh, "urls": urls, "baseline": summary(ms_b),
                        "facets": summary(ms_f), "baseline_over_facets": round(
                            float(np.median(ms_b)) / float(np.median(ms_f)), 3),
                        "baseline_bytes_d2h": int(tst.bytes_d2h), "equal": bool(equal), "facet_stats": sd}
                cells.append(cell)
                print(oname, "max_hosts", mh, "urls", urls, "baseline", cell["baseline"], "facets", cell["facets"],
                      "stats", sd, file=sys.stderr, flush=True)
    res = {"config": name, "queries": N, "repeats": reps, "warmup": warmup, "cells": cells}
    try:
        res.update(bench.source_identity())
    except Exception:  # the identity is a label only
        pass
    ix.close()
    line = json.dumps(res)
    print(line)
    src = args.src or res.get("src") or res.get("source") or "local"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.environ.get("QUERY_FACETS_OUT") or os.path.join(ROOT, "profiles", f"query_facets_{src}.json"),
              "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
