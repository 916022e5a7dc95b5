"""What feeding a search event's local container costs on the C2 corpus (one GPU), two ways in
one process over one resident index.  EVENT_LOCAL_N events (default 256) each receive the
joined container of one of the C2 two-term queries as their local arrival:

  host_path     the path before yrwi_event_add_local: yrwi_term_search per query (every joined
                row crosses to the host), then one yrwi_event_add of all arrivals (every row
                crosses back);
  device_local  one yrwi_event_add_local: the rows never leave the device.

  python tools/event_local.py [--src LABEL]

ms per call is the wall time of the C calls alone (each ends in a device synchronise) on freshly
opened events, the median of EVENT_LOCAL_REPS (default 5) timed repeats after EVENT_LOCAL_WARMUP
(default 1) untimed ones, with the min-max range; the two arms alternate, so drift of the box
falls on both.  Events are opened and closed outside the timed regions, and term_search writes
into buffers allocated before.  The stacks of a 32-event sample are compared between the arms
and against the oracle.  The structural contract is asserted from the library's own counters
(yrwi_local_stats): launches_tail and syncs are the same for N and N / 2 arrivals, and the bytes
the call moves over PCIe stay under 2 KiB per arrival (its descriptors), however many rows
arrive.  No speed-up is asserted.  One JSON line to stdout and to profiles/event_local_<src>.json (EVENT_LOCAL_CONFIG:
another preset; EVENT_LOCAL_K: another stack bound; EVENT_LOCAL_OUT: another file)."""
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
from yacy_search_server_amd._lib import CArrival, CLocalArrival, CLocalStats, CQuery  # noqa: E402

NOW_MS = 20741 * 86400000
SAMPLE = 32


def summary(ms):
    return {"median_ms_per_call": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=None, help="label of the output file (default: the source identity)")
    args = ap.parse_args()
    name = os.environ.get("EVENT_LOCAL_CONFIG", "C2")
    N = max(2, int(os.environ.get("EVENT_LOCAL_N", "256")))
    reps = max(1, int(os.environ.get("EVENT_LOCAL_REPS", "5")))
    warmup = max(1, int(os.environ.get("EVENT_LOCAL_WARMUP", "1")))
    k = int(os.environ.get("EVENT_LOCAL_K", "100"))
    import bench
    import oracle as orc
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

    # sizing pass: the rows of every query's container (a buffer per query, sized before the timed regions)
    m = ctypes.c_int64()
    bufs = []
    for i, (inc, _) in enumerate(qs):
        cap = int(min(idx.sizes[t] for t in inc))
        b = np.zeros((max(cap, 1), 40), dtype=np.uint8)
        check(L.yrwi_term_search(ix._h, ctypes.byref(cq[i]), b.ctypes.data, cap, ctypes.byref(m)), "yrwi_term_search")
        bufs.append(b[:max(m.value, 1)].copy())

    def open_events(n):
        return [ix.event(None, "en", NOW_MS, k=k, max_postings=len(bufs[i]) + 16) for i in range(n)]

    def host_path(evs):
        n = len(evs)
        arr = (CArrival * n)()
        t0 = time.perf_counter()
        for i in range(n):
            check(L.yrwi_term_search(ix._h, ctypes.byref(cq[i]), bufs[i].ctypes.data, len(bufs[i]), ctypes.byref(m)),
                  "yrwi_term_search")
            arr[i].ev = evs[i]._e
            arr[i].rows40 = bufs[i].ctypes.data if m.value else None
            arr[i].n = m.value
            arr[i].local = 1
        check(L.yrwi_event_add(ix._h, arr, n), "yrwi_event_add")
        dt = time.perf_counter() - t0
        return dt * 1e3, [arr[i].n for i in range(n)], None

    def device_local(evs):
        n = len(evs)
        arr = (CLocalArrival * n)()
        for i in range(n):
            arr[i].ev = evs[i]._e
            arr[i].q = ctypes.pointer(cq[i])
        st = CLocalStats()
        t0 = time.perf_counter()
        check(L.yrwi_event_add_local(ix._h, arr, n, ctypes.byref(st)), "yrwi_event_add_local")
        dt = time.perf_counter() - t0
        return dt * 1e3, [arr[i].m for i in range(n)], st

    def stacks(evs):
        out = []
        for ev in evs[:SAMPLE]:
            hits, info = ev.results()
            out.append(([(h.urlhash, h.score, h.tiebreak) for h in hits], info.postings_in, info.admitted_local))
        return out

    arms = (("host_path", host_path), ("device_local", device_local))
    ms = {a: [] for a, _ in arms}
    seen = {}
    stats = None
    for r in range(warmup + reps):
        for aname, fn in arms:
            evs = open_events(N)
            t, rows, st = fn(evs)
            if r >= warmup:
                ms[aname].append(t)
                print(aname, round(t, 3), "ms", file=sys.stderr, flush=True)
            if r == warmup + reps - 1:
                seen[aname] = (stacks(evs), rows)
                stats = st or stats
            for ev in evs:
                ev.close()
    rows_q = seen["device_local"][1]
    same_between_arms = seen["host_path"] == seen["device_local"]
    d = idx.as_dict()
    same_as_oracle = all(
        seen["device_local"][0][i][0] == orc.search(d, [idx.hashes[t] for t in qs[i][0]], [], now_ms=NOW_MS, k=k)
        for i in range(min(SAMPLE, N)))
    # the structural contract, from the library's counters: half the arrivals, the same tail and waits
    evs = open_events(N // 2)
    _, _, half = device_local(evs)
    for ev in evs:
        ev.close()
    fields = [f for f, _ in CLocalStats._fields_]
    sd = {f: int(getattr(stats, f)) for f in fields}
    hd = {f: int(getattr(half, f)) for f in fields}
    pcie = sd["bytes_h2d"] + sd["bytes_d2h"]
    assert same_between_arms, "the two arms left different stacks"
    assert same_as_oracle, "the device-local stacks differ from the oracle's"
    assert sd["launches_tail"] == hd["launches_tail"] and sd["syncs"] == hd["syncs"], (sd, hd)
    # no row among the bytes: what crosses is each arrival's descriptors (EvDev, EvJob, LocalJob, the
    # JoinQ and tile bases of its join; about 1 KiB for a two-term query), whatever its container holds
    assert sd["rows_arrived"] == sum(rows_q) and pcie <= 2048 * N, sd
    assert sd["device_allocs"] <= 1, sd
    a, b = summary(ms["host_path"]), summary(ms["device_local"])
    res = {"config": name, "events": N, "k": k, "repeats": reps, "warmup": warmup,
           "rows_arrived": sd["rows_arrived"], "row_bytes": 40 * sd["rows_arrived"],
           "host_path": dict(a, pcie_row_bytes_per_call=2 * 40 * sd["rows_arrived"]),
           "device_local": dict(b, pcie_row_bytes_per_call=0, pcie_bytes_per_call=pcie),
           "host_over_device": round(a["median_ms_per_call"] / b["median_ms_per_call"], 3),
           "device_local_is_faster": b["median_ms_per_call"] < a["median_ms_per_call"],
           "local_stats": sd, "local_stats_half_the_events": hd,
           "sample_events": min(SAMPLE, N), "stacks_equal_between_arms": same_between_arms,
           "stacks_equal_oracle": same_as_oracle}
    try:
        res.update(bench.source_identity())
    except Exception:  # the identity is a label only
        pass
    ix.close()
    line = json.dumps(res)
    print(line)
    src = args.src or res.get("src") or res.get("source") or "local"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.environ.get("EVENT_LOCAL_OUT") or os.path.join(ROOT, "profiles", f"event_local_{src}.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
