"""Time the DHT send path on the C2 index (one GPU): yrwi_dht_select of up to 1,000 containers /
10 M references at e = 4 from the smallest term, without and with removal, against the only way
out the library had before it: a get_list per term (one copy and one device wait each), the
split in numpy, and for the removal a put_list(n = 0) per term (product code only, no oracle).

  python tools/index_dht.py [--src LABEL]

Between repeats the removed containers are put back with add_postings(policy="keep"), outside
the timed region.  Every figure is the median of INDEX_DHT_REPS (default 5) repeats in one
process with the min-max range, in ms and GB/s of row bytes; the pack kernels' device time
(t_pack_ns) stands beside the call's wall time (t_total_ns), with the windows, launches and syncs
of the call.  One JSON line to stdout and to profiles/index_dht_<src>.json (INDEX_DHT_CONFIG:
another preset; INDEX_DHT_CONTAINERS, INDEX_DHT_REFS: other caps)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yacy_search_server_amd import RWIIndex, _lib, synth  # noqa: E402

B64 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"
RANK = np.frombuffer(bytes.maketrans(B64, bytes(range(64))), dtype=np.uint8)
E = 4
FIRST, LAST = b"A" * 12, b"_" * 12


def summary(ms, nbytes):
    med = float(np.median(ms))
    return {"median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "gb_per_s": round(nbytes / med / 1e6, 3)}


def per_term(ix, terms, remove):
    """the parent's way: get_list per term, the partition boundaries by numpy, the cells put
    together partition-major on the host; with `remove` a put_list(n = 0) per term"""
    P, T = 1 << E, len(terms)
    lists, bounds = [], np.zeros((T, P + 1), dtype=np.int64)
    for j, t in enumerate(terms):
        rows = ix.get_list(t)
        part = ((RANK[rows[:, 0]].astype(np.int64) << 6) | RANK[rows[:, 1]]) >> (12 - E)
        bounds[j] = np.searchsorted(part, np.arange(P + 1), side="left")
        lists.append(rows)
    cnt = (bounds[:, 1:] - bounds[:, :-1]).T.reshape(-1)  # partition-major
    off = np.concatenate([[0], np.cumsum(cnt)])
    out = np.concatenate([lists[j][bounds[j, p]:bounds[j, p + 1]] for p in range(P) for j in range(T)])
    if remove:
        for t in terms:
            ix.add(t, np.zeros((0, 40), dtype=np.uint8))
    return off, out


def put_back(ix, terms, off, rows):
    T = len(terms)
    tb = np.frombuffer(b"".join(terms), dtype=np.uint8).reshape(T, 12)
    per_row = np.repeat(tb[np.arange(len(off) - 1) % T], np.diff(off), axis=0)
    st = ix.add_postings(per_row, rows, policy="keep")
    assert st["added"] == len(rows) and st["new_terms"] == T, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=None, help="label of the output file (default: the source identity)")
    args = ap.parse_args()
    name = os.environ.get("INDEX_DHT_CONFIG", "C2")
    reps = max(1, int(os.environ.get("INDEX_DHT_REPS", "5")))
    maxc = int(os.environ.get("INDEX_DHT_CONTAINERS", "1000"))
    maxr = int(os.environ.get("INDEX_DHT_REFS", "10000000"))
    cfg = synth.preset(name)
    print("building", name, file=sys.stderr, flush=True)
    idx = synth.build_index(cfg)
    ix = RWIIndex(0)
    for t in range(cfg.n_terms):
        if idx.sizes[t]:
            ix.add(idx.hashes[t], idx.list_rows(t))
        if t % 2000 == 1999:
            print("uploaded", t + 1, "terms", file=sys.stderr, flush=True)
    del idx
    print("index resident", file=sys.stderr, flush=True)
    os.environ.pop("YRWI_DHT_WINDOW_ROWS", None)
    dry = ix.dht_select(FIRST, LAST, maxc, maxr, E, count_only=True).stats
    n, nbytes = dry["postings"], 40 * dry["postings"]
    out = {"config": name, "index_postings": ix.stats()[1], "index_terms": ix.stats()[0], "repeats": reps,
           "max_containers": maxc, "max_refs": maxr, "partition_exponent": E, "terms": dry["terms"], "postings": n,
           "row_bytes": nbytes, "window_rows": _lib.DHT_WINDOW_ROWS_DEFAULT}
    try:
        import bench
        out.update(bench.source_identity())
    except Exception:  # the identity is a label only
        pass
    pinned = ix.host_array(ctypes.c_uint8, nbytes)
    ref = ix.dht_select(FIRST, LAST, maxc, maxr, E, rows_out=pinned)  # the windows are allocated here, untimed
    terms, ref_off, ref_rows = ref.terms, ref.part_off.copy(), ref.rows.copy()

    def run(remove, rows_out):
        wall, sts = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            sel = ix.dht_select(FIRST, LAST, maxc, maxr, E, remove=remove, rows_out=rows_out)
            wall.append((time.perf_counter() - t0) * 1e3)
            sts.append(sel.stats)
            assert sel.terms == terms and np.array_equal(sel.part_off, ref_off)
            if remove:
                assert sel.stats["removed"] == n and ix.get_size(terms[0]) == 0
                put_back(ix, terms, sel.part_off, sel.rows)
        assert np.array_equal(sel.rows, ref_rows)
        return {"wall_with_dry_run": summary(wall, nbytes),
                "t_total": summary([s["t_total_ns"] / 1e6 for s in sts], nbytes),
                "t_pack": summary([s["t_pack_ns"] / 1e6 for s in sts], nbytes),
                "pack_share_of_total": round(float(np.median([s["t_pack_ns"] / max(s["t_total_ns"], 1) for s in sts])), 4),
                "windows": sts[0]["windows"], "launches": sts[0]["launches"], "syncs": sts[0]["syncs"]}

    for key, remove, buf in (("select_pinned", False, pinned), ("select_remove_pinned", True, pinned),
                             ("select_pageable", False, None), ("select_remove_pageable", True, None)):
        out[key] = run(remove, buf)
        print(key, json.dumps(out[key]), file=sys.stderr, flush=True)
    # the parent's alternative
    for key, remove in (("get_list_per_term", False), ("get_list_per_term_remove", True)):
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            off, rows = per_term(ix, terms, remove)
            wall.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(off, ref_off) and np.array_equal(rows, ref_rows)
            if remove:
                put_back(ix, terms, off, rows)
        out[key] = summary(wall, nbytes)
        # library calls that wait for the device per term: a get_list (copy and wait) and, with `remove`,
        # a put_list(n = 0) (the batches in flight only)
        out[key]["device_waits"] = len(terms) * (2 if remove else 1)
        print(key, json.dumps(out[key]), file=sys.stderr, flush=True)
    for a, b in (("select_pinned", "get_list_per_term"), ("select_remove_pinned", "get_list_per_term_remove"),
                 ("select_pageable", "get_list_per_term"), ("select_remove_pageable", "get_list_per_term_remove")):
        out[f"ratio_{b}_over_{a}"] = round(out[b]["median_ms"] / max(out[a]["wall_with_dry_run"]["median_ms"], 1e-6), 2)
    out["check_bad"] = ix.check_url_ids()[0]  # after the put-backs the index is consistent
    out["index_postings_after"] = ix.stats()[1]
    ix.close()
    line = json.dumps(out)
    print(line)
    src = args.src or out.get("src") or out.get("source") or "local"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.environ.get("INDEX_DHT_OUT") or os.path.join(ROOT, "profiles", f"index_dht_{src}.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
