"""Time the heap dump of the C2 index (one GPU): yrwi_dump_heap of the whole index into a
directory given on the command line, at the default window size and at a few others, against
the only way out the library had before it: a get_list per term, the same record bytes
written from Python (product code only, no oracle).

  python tools/index_dump.py <directory> [--src LABEL]

Every figure is the median of INDEX_DUMP_REPS (default 5) repeats in one process, with the
min-max range, in ms and GB/s of file bytes; the pack kernels' device time (t_pack_ns) stands
beside the call's wall time (t_total_ns), with the launches, syncs and windows of the call.
State the directory's file system with the numbers: tmpfs and disk differ.  One JSON line to
stdout and to profiles/index_dump_<src>.json (INDEX_DUMP_CONFIG: another preset)."""
import argparse
import filecmp
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yacy_search_server_amd import RWIIndex, _lib, synth  # noqa: E402

WINDOWS_MB = (1, 8, 32, 128)
B64 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"
RANK = bytes.maketrans(B64, bytes(range(64)))


def fs_type(path):
    """file system of `path` by the longest mount point in /proc/mounts"""
    best, kind = "", "unknown"
    try:
        real = os.path.realpath(path)
        with open("/proc/mounts") as f:
            for line in f:
                _, mnt, typ = line.split()[:3]
                if (real == mnt or real.startswith(mnt.rstrip("/") + "/")) and len(mnt) > len(best):
                    best, kind = mnt, typ
    except OSError:
        pass
    return kind


def summary(ms, nbytes):
    med = float(np.median(ms))
    return {"median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "gb_per_s": round(nbytes / med / 1e6, 3)}


def per_term_dump(ix, terms, path, days):
    """the parent's way: one get_list per term (one copy and one device wait each), the record
    framed in Python"""
    cell = struct.pack(">H", days)
    with open(path + ".prt", "wb") as f:
        for t in terms:
            rows = ix.get_list(t)
            n = len(rows)
            if n == 0:
                continue
            f.write(struct.pack(">i", 26 + 40 * n) + t + struct.pack(">i", n) + cell + cell + b"Be" +
                    struct.pack(">i", n))
            f.write(rows.tobytes())
        f.flush()
        os.fsync(f.fileno())
    os.replace(path + ".prt", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("directory")
    ap.add_argument("--src", default=None, help="label of the output file (default: the source identity)")
    args = ap.parse_args()
    name = os.environ.get("INDEX_DUMP_CONFIG", "C2")
    reps = max(1, int(os.environ.get("INDEX_DUMP_REPS", "5")))
    cfg = synth.preset(name)
    idx = synth.build_index(cfg)
    ix = RWIIndex(0)
    for t in range(cfg.n_terms):
        if idx.sizes[t]:
            ix.add(idx.hashes[t], idx.list_rows(t))
    ix.build_url_ids()
    print("index resident", file=sys.stderr, flush=True)
    now = 20741 * 86400000
    days = (now - 946684800000) // 86400000
    terms = sorted((idx.hashes[t] for t in range(cfg.n_terms) if idx.sizes[t]), key=lambda h: h.translate(RANK))
    out = {"config": name, "postings": int(idx.sizes.sum()), "terms": len(terms), "repeats": reps,
           "directory_fs": fs_type(args.directory), "default_window_mb": _lib.DUMP_WINDOW_DEFAULT >> 20}
    try:
        import bench
        out.update(bench.source_identity())
    except Exception:  # the identity is a label only
        pass
    path = os.path.join(args.directory, "index_dump.blob")
    os.environ.pop("YRWI_DUMP_WINDOW", None)
    ix.dump_heap(path, now_ms=now)  # the staging windows are allocated here, outside the timed runs

    def run(window_mb):
        if window_mb is None:
            os.environ.pop("YRWI_DUMP_WINDOW", None)
        else:
            os.environ["YRWI_DUMP_WINDOW"] = str(window_mb << 20)
        wall, sts = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            st = ix.dump_heap(path, now_ms=now)
            wall.append((time.perf_counter() - t0) * 1e3)
            sts.append(st)
        nbytes = sts[0]["bytes"]
        c = {"wall": summary(wall, nbytes),
             "t_total": summary([s["t_total_ns"] / 1e6 for s in sts], nbytes),
             "t_pack": summary([s["t_pack_ns"] / 1e6 for s in sts], nbytes),
             "pack_share_of_total": round(float(np.median([s["t_pack_ns"] / max(s["t_total_ns"], 1) for s in sts])), 4),
             "bytes": nbytes, "windows": sts[0]["windows"], "launches": sts[0]["launches"], "syncs": sts[0]["syncs"]}
        return c

    # the largest window first: the staging memory grows once, before its timed runs
    for mb in sorted(WINDOWS_MB, reverse=True):
        os.environ["YRWI_DUMP_WINDOW"] = str(mb << 20)
        if mb == max(WINDOWS_MB):
            ix.dump_heap(path, now_ms=now)
        out[f"window_{mb}mb"] = run(mb)
        print(f"window {mb} MiB", json.dumps(out[f"window_{mb}mb"]), file=sys.stderr, flush=True)
    out["dump_heap"] = run(None)
    print("dump_heap", json.dumps(out["dump_heap"]), file=sys.stderr, flush=True)
    nbytes = out["dump_heap"]["bytes"]
    # the parent's alternative
    ppath = os.path.join(args.directory, "index_dump_per_term.blob")
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        per_term_dump(ix, terms, ppath, days)
        wall.append((time.perf_counter() - t0) * 1e3)
    out["per_term_image_equal"] = filecmp.cmp(path, ppath, shallow=False)
    out["get_list_per_term"] = summary(wall, nbytes)
    out["get_list_per_term"]["device_waits"] = len(terms)
    out["speedup_over_get_list_per_term"] = round(out["get_list_per_term"]["median_ms"] /
                                                  max(out["dump_heap"]["wall"]["median_ms"], 1e-6), 2)
    print("get_list per term", json.dumps(out["get_list_per_term"]), file=sys.stderr, flush=True)
    # the file loads back into an equal index
    back = RWIIndex(0)
    ls = back.load_heaps([path])
    out["reload"] = {"terms": ls.terms, "postings": ls.postings, "check_bad": back.check_url_ids()[0]}
    back.close()
    ix.close()
    for p in (path, ppath):
        os.unlink(p)
    line = json.dumps(out)
    print(line)
    src = args.src or out.get("src") or out.get("source") or "local"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.environ.get("INDEX_DUMP_OUT") or os.path.join(ROOT, "profiles", f"index_dump_{src}.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
