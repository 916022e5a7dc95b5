"""What the hits' rows cost on the C2 corpus (one GPU): the benchmark's batches (1000 two-term
queries, k = 100, 8 batches in flight, pinned result buffers, no statistics) timed three ways in
one process over one resident index:

  hits       yrwi_query_batch_submit -- the headline path, hits only;
  hits_rows  yrwi_query_batch_rows_submit -- the same batches with the 40-byte row of every hit;
  term_search  yrwi_term_search per query -- the only way to the postings before: the whole
             joined container of every query crosses to the host (and no ranking is done).

  python tools/hit_rows.py [--src LABEL]

ms/step is the wall time of HIT_ROWS_STEPS (default 200) steps after HIT_ROWS_WARMUP (default
20), the median of HIT_ROWS_REPS (default 3) regions with the min-max range; hits and hits_rows
regions alternate, so drift of the box falls on both.  term_search runs HIT_ROWS_TS_STEPS
(default 2) steps: it is two to three orders slower.  isolated_kernels_us: the device time of one
batch's kernels (yrwi_stats.t_kernels_ns of a submitted batch that is waited for at once: one lane,
nothing else in flight) without and with rows; the difference is k_hit_rows alone.  The PCIe bytes are what each path moves to
the host per step: 24 B per hit (+ 40 B per row), 4 B per query count; the whole container for
term_search.  One JSON line to stdout and to profiles/hit_rows_<src>.json (HIT_ROWS_CONFIG:
another preset; HIT_ROWS_NQ, HIT_ROWS_K: another batch shape)."""
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


def summary(ms):
    return {"median_ms_per_step": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=None, help="label of the output file (default: the source identity)")
    args = ap.parse_args()
    name = os.environ.get("HIT_ROWS_CONFIG", "C2")
    steps = max(INFLIGHT, int(os.environ.get("HIT_ROWS_STEPS", "200")))
    warmup = int(os.environ.get("HIT_ROWS_WARMUP", "20"))
    reps = max(1, int(os.environ.get("HIT_ROWS_REPS", "3")))
    ts_steps = max(1, int(os.environ.get("HIT_ROWS_TS_STEPS", "2")))
    nq = int(os.environ.get("HIT_ROWS_NQ", "1000"))
    k = int(os.environ.get("HIT_ROWS_K", "100"))
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
    batches = bench.draws(cfg, nq, 2, 2, 0, None, INFLIGHT)
    for qs in batches:
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
    bufs = [(ix.host_array(CHit, nq * k), ix.host_array(ctypes.c_int32, nq), ix.host_array(ctypes.c_uint8, nq * k * 40))
            for _ in range(INFLIGHT)]

    def run_steps(n, rows):
        pending = []
        for i in range(n):
            b = bufs[i % INFLIGHT]
            if len(pending) == INFLIGHT:
                ix.wait(pending.pop(0))
            if rows:
                pending.append(ix.submit_rows_raw(arrs[i % D], nq, k, b[0], b[2], b[1], None))
            else:
                pending.append(ix.submit_raw(arrs[i % D], nq, k, b[0], b[1], None))
        for t in pending:
            ix.wait(t)

    def region(rows):
        run_steps(warmup, rows)
        r0 = _lib.lib().yrwi_realloc_events()
        t0 = time.perf_counter()
        run_steps(steps, rows)
        dt = time.perf_counter() - t0
        return dt / steps * 1e3, int(_lib.lib().yrwi_realloc_events() - r0)

    # both paths once, then every lane's scratch and staging settled (as the benchmark does)
    run_steps(D, True)
    run_steps(D, False)
    rc = _lib.lib().yrwi_settle_scratch(ix._h)
    if rc:
        raise RuntimeError(f"yrwi_settle_scratch: {rc}")
    ms = {"hits": [], "hits_rows": []}
    realloc = 0
    for _ in range(reps):
        for mode, rows in (("hits", False), ("hits_rows", True)):
            m, r = region(rows)
            ms[mode].append(m)
            realloc += r
            print(mode, round(m, 4), "ms/step", file=sys.stderr, flush=True)
    # isolated (one batch in flight, with statistics): the device time of the batch's kernels with and
    # without k_hit_rows -- their difference is the kernel alone, nothing of it hidden behind other lanes
    iso = {"hits": [], "hits_rows": []}
    st = CStats()
    for i in range(2 * INFLIGHT):
        b = bufs[0]
        ix.wait(ix.submit_raw(arrs[i % D], nq, k, b[0], b[1], st))  # the whole batch on one lane
        iso["hits"].append(st.t_kernels_ns / 1e3)
        ix.wait(ix.submit_rows_raw(arrs[i % D], nq, k, b[0], b[2], b[1], st))
        iso["hits_rows"].append(st.t_kernels_ns / 1e3)
    iso_us = {m: round(float(np.median(v)), 1) for m, v in iso.items()}
    # what the last rows step returned, against the hits: every row carries its hit's url hash
    hits_per_step = int(sum(bufs[0][1][:nq]))
    h = np.frombuffer(bufs[0][0], dtype=np.uint8).reshape(nq * k, 24)
    r = np.frombuffer(bufs[0][2], dtype=np.uint8).reshape(nq * k, 40)
    live = (np.arange(k)[None, :] < np.asarray(bufs[0][1][:nq])[:, None]).ravel()
    rows_match = bool((h[live, :12] == r[live, :12]).all())
    # term_search per query: the whole joined container to the host
    cap = int(idx.sizes.max())
    out = np.zeros((cap, 40), dtype=np.uint8)
    m = ctypes.c_int64()
    L = _lib.lib()
    ts_ms, ts_rows = [], 0
    for s in range(ts_steps):
        arr = arrs[s % D]
        t0 = time.perf_counter()
        n_rows = 0
        for i in range(nq):
            rc = L.yrwi_term_search(ix._h, ctypes.byref(arr[i]), out.ctypes.data, cap, ctypes.byref(m))
            if rc:
                raise RuntimeError(f"yrwi_term_search: {rc}")
            n_rows += m.value
        ts_ms.append((time.perf_counter() - t0) * 1e3)
        ts_rows = n_rows
    res = {"config": name, "nq": nq, "k": k, "inflight": INFLIGHT, "steps": steps, "warmup": warmup, "repeats": reps,
           "hits_per_step": hits_per_step, "rows_carry_their_hits_url_hash": rows_match,
           "realloc_events_in_timed_regions": realloc,
           "hits": dict(summary(ms["hits"]), pcie_bytes_per_step=24 * hits_per_step + 4 * nq),
           "hits_rows": dict(summary(ms["hits_rows"]), pcie_bytes_per_step=64 * hits_per_step + 4 * nq),
           "term_search_per_query": dict(summary(ts_ms), steps=ts_steps, joined_rows_per_step=ts_rows,
                                         pcie_bytes_per_step=40 * ts_rows)}
    res["rows_cost_ms_per_step"] = round(res["hits_rows"]["median_ms_per_step"] - res["hits"]["median_ms_per_step"], 4)
    res["isolated_kernels_us"] = dict(iso_us, k_hit_rows=round(iso_us["hits_rows"] - iso_us["hits"], 1))
    try:
        res.update(bench.source_identity())
    except Exception:  # the identity is a label only
        pass
    ix.close()
    line = json.dumps(res)
    print(line)
    src = args.src or res.get("src") or res.get("source") or "local"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.environ.get("HIT_ROWS_OUT") or os.path.join(ROOT, "profiles", f"hit_rows_{src}.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
