"""What the pair cache does on the C2 corpus (one GPU): the benchmark's batches (1000 two-term
queries, k = 100, 8 distinct batches cycled, 8 in flight, pinned result buffers, no statistics)
timed in one process over one resident index with the cache on and off (YRWI_PAIR_CACHE is read
per call), regions alternating so that drift of the box falls on both.

  python tools/pair_cache.py [--src LABEL]

ms/step is the wall time of PAIR_CACHE_STEPS (default 200) steps after PAIR_CACHE_WARMUP (default
20), PAIR_CACHE_REPS (default 3) regions each way, every region's figure kept.  The first "on"
region starts cold: its warm-up fills the cache.  For every "on" region the counters of
yrwi_pair_cache_info_get over the timed steps (hits, misses, fills, evictions, rows served) and the
share of the steps' joined rows that came from entries.  isolated: one batch in flight with
statistics, each of the 8 batches once each way -- the device time of the batch's kernels, of
its probe and of its compaction (HIP events of yrwi_stats), and its joined rows.  The limits: a
warm cache, and an index that does not change during the run.  One JSON line to stdout and to
profiles/pair_cache_<src>.json."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yacy_search_server_amd import RankingProfile, RWIIndex, _lib, synth  # noqa: E402
from yacy_search_server_amd._lib import CHit, CQuery, CStats  # noqa: E402

NOW_MS = 20741 * 86400000
INFLIGHT = 8
COUNTERS = ("hits", "misses", "fills", "dropped", "evictions", "invalidations", "rows_served")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=None, help="label of the output file (default: the source identity)")
    args = ap.parse_args()
    name = os.environ.get("PAIR_CACHE_CONFIG", "C2")
    steps = max(INFLIGHT, int(os.environ.get("PAIR_CACHE_STEPS", "200")))
    warmup = int(os.environ.get("PAIR_CACHE_WARMUP", "20"))
    reps = max(1, int(os.environ.get("PAIR_CACHE_REPS", "3")))
    nq, k = 1000, 100
    import bench
    cfg = synth.preset(name)
    idx = synth.build_index(cfg)
    ix = RWIIndex(0)
    for t in range(cfg.n_terms):
        if idx.sizes[t]:
            ix.add(idx.hashes[t], idx.list_rows(t))
    ix.build_url_ids()
    print("index resident", file=sys.stderr, flush=True)
    prof = RankingProfile()
    keep = [prof]
    arrs = []
    for qs in bench.draws(cfg, nq, 2, 2, 0, None, INFLIGHT):
        arr = (CQuery * nq)()
        for i, (inc, exc) in enumerate(qs):
            ib = ctypes.create_string_buffer(b"".join(idx.hashes[t] for t in inc), 12 * max(1, len(inc)))
            keep.append(ib)
            arr[i].incl = ctypes.cast(ib, ctypes.c_void_p)
            arr[i].nincl = len(inc)
            arr[i].max_distance = 2147483647
            arr[i].k = k
            arr[i].profile = ctypes.pointer(prof.c)
            arr[i].language = b"en"
            arr[i].now_ms = NOW_MS
        arrs.append(arr)
    D = len(arrs)
    bufs = [(ix.host_array(CHit, nq * k), ix.host_array(ctypes.c_int32, nq)) for _ in range(INFLIGHT)]

    def run_steps(n):
        pending = []
        for i in range(n):
            b = bufs[i % INFLIGHT]
            if len(pending) == INFLIGHT:
                ix.wait(pending.pop(0))
            pending.append(ix.submit_raw(arrs[i % D], nq, k, b[0], b[1], None))
        for t in pending:
            ix.wait(t)

    def switch(on):
        os.environ["YRWI_PAIR_CACHE"] = "1" if on else "0"

    def results():
        run_steps(D)
        out = []
        for b in bufs:  # every query's hits, as many as it has
            mv, n = memoryview(b[0]).cast("B"), list(b[1])
            out.append([bytes(mv[24 * q * k:24 * (q * k + n[q])]) for q in range(nq)])
        return out

    def isolated():
        st = CStats()
        out = []
        for bi in range(D):
            ix.wait(ix.submit_raw(arrs[bi], nq, k, bufs[0][0], bufs[0][1], st))
            out.append({"kernels_us": st.t_kernels_ns / 1e3, "probe_us": st.t_probe_ns / 1e3,
                        "compact_us": st.t_compact_ns / 1e3, "score_us": st.t_scorek_ns / 1e3, "joined": st.joined})
        return {f: round(float(np.mean([o[f] for o in out])), 1) for f in out[0]}

    # both ways once, then every lane's scratch and staging settled (as the benchmark does)
    switch(False)
    ref = results()
    rc = _lib.lib().yrwi_settle_scratch(ix._h)
    if rc:
        raise RuntimeError(f"yrwi_settle_scratch: {rc}")
    regions = {"on": [], "off": []}
    realloc = 0
    for _ in range(reps):
        for mode in ("off", "on"):
            switch(mode == "on")
            run_steps(warmup)
            i0 = ix.pair_cache_info()
            r0 = _lib.lib().yrwi_realloc_events()
            t0 = time.perf_counter()
            run_steps(steps)
            dt = time.perf_counter() - t0
            realloc += int(_lib.lib().yrwi_realloc_events() - r0)
            i1 = ix.pair_cache_info()
            reg = {"ms_per_step": round(dt / steps * 1e3, 4)}
            if mode == "on":
                reg.update({c: i1[c] - i0[c] for c in COUNTERS})
                reg.update(entries=i1["entries"], bytes=i1["bytes"])
            regions[mode].append(reg)
            print(mode, reg, file=sys.stderr, flush=True)
    switch(True)
    same = results() == ref  # the warm cache's hits, byte for byte, against the run without it
    iso_on = isolated()
    switch(False)
    iso_off = isolated()
    info = ix.pair_cache_info()
    joined_per_cycle = iso_off["joined"] * D
    served = [r["rows_served"] / (steps / D * joined_per_cycle) for r in regions["on"]]
    res = {"config": name, "nq": nq, "k": k, "inflight": INFLIGHT, "batches": D, "steps": steps, "warmup": warmup,
           "repeats": reps, "regions": regions, "realloc_events_in_timed_regions": realloc,
           "results_equal_on_off": same, "rows_served_share_of_joined": [round(s, 4) for s in served],
           "isolated_mean_per_batch": {"on": iso_on, "off": iso_off},
           "cache": {c: info[c] for c in ("capacity_bytes", "budget_bytes", "min_rows", "entries", "bytes") + COUNTERS},
           "limits": "warm cache; index unchanged during the run"}
    try:
        res.update(bench.source_identity())
    except Exception:  # the identity is a label only
        pass
    ix.close()
    line = json.dumps(res)
    print(line)
    src = args.src or res.get("src") or res.get("source") or "local"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.environ.get("PAIR_CACHE_OUT") or os.path.join(ROOT, "profiles", f"pair_cache_{src}.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
