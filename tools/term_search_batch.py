"""What the joined containers of many queries cost on the C2 corpus (one GPU), three ways in one
process over one resident index.  TERM_BATCH_N (default 256) two-term queries of the C2 stream:

  per_query       yrwi_term_search once per query, the only way to the rows before: each call
                  plans and joins one descriptor, copies the whole container and its exclusion
                  marks to pageable memory, waits, and compacts on the host;
  batch_pageable  one yrwi_term_search_batch into a numpy buffer: one join pass, the rows
                  packed on the device, one copy of exactly the kept rows;
  batch_pinned    the same call into yrwi_host_alloc memory: the pack kernel stores the rows
                  into the buffer itself.

  python tools/term_search_batch.py [--src LABEL]

ms per arm is the wall time of the C calls alone (each ends in a device synchronise), the median
of TERM_BATCH_REPS (default 5) timed repeats after TERM_BATCH_WARMUP (default 1) untimed ones,
with the min-max range; the arms alternate, so drift of the box falls on all three.  Every
buffer is allocated before the timed regions, sized by the smallest include list of each query
(no counting call).  The rows of the three arms are compared byte for byte, and a sample against
the oracle.  The structural contract is asserted from the library's own counters
(yrwi_tsb_stats): launches_tail and syncs are the same for N and N / 2 queries, and what crosses
PCIe beyond the rows themselves stays under 2 KiB per query.  No speed-up is asserted.  One JSON
line to stdout and to profiles/term_search_batch_<src>.json (TERM_BATCH_CONFIG: another preset;
TERM_BATCH_OUT: another file)."""
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
from yacy_search_server_amd._lib import CQuery, CTsbStats  # noqa: E402

NOW_MS = 20741 * 86400000
SAMPLE = 32


def summary(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=None, help="label of the output file (default: the source identity)")
    args = ap.parse_args()
    name = os.environ.get("TERM_BATCH_CONFIG", "C2")
    N = max(2, int(os.environ.get("TERM_BATCH_N", "256")))
    reps = max(1, int(os.environ.get("TERM_BATCH_REPS", "5")))
    warmup = max(1, int(os.environ.get("TERM_BATCH_WARMUP", "1")))
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

    # the buffers, before any timed region: the smallest include list bounds a conjunction
    caps = [int(min(idx.sizes[t] for t in inc)) for inc, _ in qs]
    cap = sum(caps)
    per_bufs = [np.zeros((max(c, 1), 40), dtype=np.uint8) for c in caps]
    pageable = np.zeros(40 * max(cap, 1), dtype=np.uint8)
    pinned = np.ctypeslib.as_array(ix.host_array(ctypes.c_uint8, 40 * max(cap, 1)))
    pinned[:] = 0  # the pages are touched before the first timed call, as the numpy buffer's are
    off = np.zeros(N + 1, dtype=np.int64)
    m = ctypes.c_int64()

    def per_query(n):
        ms_rows = []
        t0 = time.perf_counter()
        for i in range(n):
            check(L.yrwi_term_search(ix._h, ctypes.byref(cq[i]), per_bufs[i].ctypes.data, caps[i], ctypes.byref(m)),
                  "yrwi_term_search")
            ms_rows.append(m.value)
        dt = time.perf_counter() - t0
        return dt * 1e3, np.concatenate([per_bufs[i][:ms_rows[i]] for i in range(n)]), np.cumsum([0] + ms_rows), None

    def batch(buf):
        def run(n):
            st = CTsbStats()
            t0 = time.perf_counter()
            check(L.yrwi_term_search_batch(ix._h, cq, n, buf.ctypes.data, cap, off.ctypes.data, ctypes.byref(st)),
                  "yrwi_term_search_batch")
            dt = time.perf_counter() - t0
            return dt * 1e3, buf[:40 * int(off[n])].reshape(-1, 40).copy(), off[:n + 1].copy(), st
        return run

    arms = (("per_query", per_query), ("batch_pageable", batch(pageable)), ("batch_pinned", batch(pinned)))
    ms = {a: [] for a, _ in arms}
    seen, stats = {}, {}
    for r in range(warmup + reps):
        for aname, fn in arms:
            t, rows, offs, st = fn(N)
            if r >= warmup:
                ms[aname].append(t)
                print(aname, round(t, 3), "ms", file=sys.stderr, flush=True)
            if r == warmup + reps - 1:
                seen[aname] = (rows, offs)
                stats[aname] = st
    ref_rows, ref_off = seen["per_query"]
    same_between_arms = all(np.array_equal(seen[a][0], ref_rows) and np.array_equal(seen[a][1], ref_off)
                            for a in ("batch_pageable", "batch_pinned"))
    d = idx.as_dict()
    same_as_oracle = all(
        np.array_equal(ref_rows[ref_off[i]:ref_off[i + 1]],
                       orc.term_search(d, [idx.hashes[t] for t in qs[i][0]], [], 2147483647, NOW_MS))
        for i in range(min(SAMPLE, N)))
    # the structural contract, from the library's counters: half the queries, the same tail and waits
    fields = [f for f, _ in CTsbStats._fields_]
    sd = {a: {f: int(getattr(stats[a], f)) for f in fields} for a in ("batch_pageable", "batch_pinned")}
    hd = {a: {f: int(getattr(fn(N // 2)[3], f)) for f in fields} for a, fn in arms[1:]}
    assert same_between_arms, "the three arms returned different rows"
    assert same_as_oracle, "the rows differ from the oracle's"
    for a in sd:
        assert sd[a]["launches_tail"] == hd[a]["launches_tail"] and sd[a]["syncs"] == hd[a]["syncs"], (sd, hd)
        assert sd[a]["rows_out"] == len(ref_rows) and sd[a]["device_allocs"] == 0, sd
        beyond = sd[a]["bytes_h2d"] + sd[a]["bytes_d2h"] - 40 * sd[a]["rows_out"]
        assert 0 <= beyond <= 2048 * N, sd
    assert sd["batch_pinned"]["direct"] == 1 and sd["batch_pageable"]["direct"] == 0
    t = {a: summary(ms[a]) for a, _ in arms}
    res = {"config": name, "queries": N, "repeats": reps, "warmup": warmup, "rows_out": int(len(ref_rows)),
           "row_bytes": 40 * int(len(ref_rows)), "rows_joined": sd["batch_pinned"]["rows_joined"],
           "per_query": t["per_query"], "batch_pageable": t["batch_pageable"], "batch_pinned": t["batch_pinned"],
           "per_query_over_batch_pageable": round(t["per_query"]["median_ms"] / t["batch_pageable"]["median_ms"], 3),
           "per_query_over_batch_pinned": round(t["per_query"]["median_ms"] / t["batch_pinned"]["median_ms"], 3),
           "tsb_stats": sd, "tsb_stats_half_the_queries": hd, "sample_queries": min(SAMPLE, N),
           "rows_equal_between_arms": same_between_arms, "rows_equal_oracle": same_as_oracle}
    try:
        res.update(bench.source_identity())
    except Exception:  # the identity is a label only
        pass
    ix.close()
    line = json.dumps(res)
    print(line)
    src = args.src or res.get("src") or res.get("source") or "local"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.environ.get("TERM_BATCH_OUT") or os.path.join(ROOT, "profiles", f"term_search_batch_{src}.json"),
              "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
