"""Time index retention on the C2 index (one GPU): the device route (yrwi_retention_count / yrwi_retain:
nothing but the arguments and the per-list counts cross PCIe) against the route a caller had before it:
get_list of every term (40 B per posting to the host), the same selection in numpy, and
yrwi_remove_postings of the losers, term by term.

Five things are timed, each once (a removal cannot be repeated on the index it has changed): the dry run
with the histogram of the days; retain with an age cutoff at the histogram's median day; retain with a cap
at a tenth of the longest list; both rules together; and the get_list route for both rules together.
Every removal has a context of its own holding the same index, and the device route and the get_list route
of both rules must leave the same statistics.  count_hosts with one host runs over the same selection: it
is the 9-byte-per-posting marking pass, which gives the age pass's t_mark_ns (40 B per posting: the day
cell sits inside the row) something to be read against.  One JSON line to stdout (INDEX_RETENTION_OUT:
also to that file).  No threshold is set here."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ms(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def days_of(rows):
    return (rows[:, 12].astype(np.int64) << 8) | rows[:, 13]


def losers(rows, min_day, max_refs):
    """the url hashes the rules remove from one list (tests/retention_ref.py's definition)"""
    a = days_of(rows)
    surv = np.flatnonzero(a >= min_day)
    keep = surv
    if max_refs > 0 and len(surv) > max_refs:
        keep = surv[np.argsort(-a[surv], kind="stable")[:max_refs]]
    gone = np.ones(len(rows), dtype=bool)
    gone[keep] = False
    return np.ascontiguousarray(rows[gone, :12])


def main():
    from yacy_search_server_amd import RWIIndex, _lib, synth
    name = os.environ.get("INDEX_RETENTION_CONFIG", "C2")
    cfg = synth.preset(name)
    idx = synth.build_index(cfg)
    print("index built", file=sys.stderr, flush=True)
    rows, sizes, hashes = idx.rows, idx.sizes, idx.hashes
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    terms = [t for t in range(cfg.n_terms) if sizes[t]]
    ixs = {}
    for k in ("age", "cap", "both", "get_list"):
        ix = RWIIndex(0)
        for t in terms:
            ix.add(hashes[t], rows[offsets[t]:offsets[t] + sizes[t]])
        ix.build_url_ids()
        ixs[k] = ix
        print("context resident:", k, file=sys.stderr, flush=True)
    host = bytes(rows[0, 6:12])
    # every kernel of the calls runs once on a small context first: the code objects are loaded before anything
    # is timed (a timed context's own first-call costs, its lane's scratch among them, stay in its figure)
    warm = RWIIndex(0)
    for t in terms[:8]:
        warm.add(hashes[t], rows[offsets[t]:offsets[t] + min(sizes[t], 4096)])
    warm.retention_count(0, 0, None, hist=True)
    warm.retain(int(np.median(days_of(rows[:4096]))), 100, None)
    warm.close()
    del rows
    L = _lib.lib()
    out = {"config": name, "postings": int(sizes.sum()), "terms": len(terms), "longest_list": int(sizes.max())}
    try:
        import bench
        out.update(bench.source_identity())
    except Exception:  # the identity is a label only
        pass

    # ---- the dry run with the histogram (twice: the first call sizes the lane's buffers), and the marking pass
    dev = ixs["age"]
    dev.retention_count(0, 0, None, hist=True)
    t_count, (st, hist) = ms(lambda: dev.retention_count(0, 0, None, hist=True))
    assert int(hist.sum()) == st["postings"] == out["postings"], (hist.sum(), st)
    median = int(np.searchsorted(np.cumsum(hist), (hist.sum() + 1) // 2))
    cap = max(1, out["longest_list"] // 10)
    dev.count_hosts([host], None)
    t_hosts, _ = ms(lambda: dev.count_hosts([host], None))
    out["retention_count_hist"] = {"call_ms": round(t_count, 3), "t_mark_ms": round(st["t_mark_ns"] / 1e6, 3),
                                   "hist_bypass": st["hist_bypass"], "distinct_days": int((hist > 0).sum()),
                                   "day_min": st["day_min"], "day_max": st["day_max"], "launches": st["launches"],
                                   "syncs": st["syncs"],
                                   "row_gbytes_per_s": round(40 * st["postings"] / max(st["t_mark_ns"], 1), 1)}
    out["count_hosts_1_host_call_ms"] = round(t_hosts, 3)
    out["median_day"], out["cap"] = median, cap
    print(json.dumps(out), file=sys.stderr, flush=True)

    # ---- the three removals on the device
    for k, (d, m) in (("age", (median, 0)), ("cap", (0, cap)), ("both", (median, cap))):
        ix = ixs[k]
        t_dry, (dry, _) = ms(lambda: ix.retention_count(d, m, None))
        t_rm, (ust, rst) = ms(lambda: ix.retain(d, m, None))
        assert all(dry[f] == rst[f] for f in ("removed_age", "removed_cap", "lists_age", "lists_cap", "emptied_terms"))
        assert ust["removed"] == rst["removed_age"] + rst["removed_cap"]
        assert ix.stats()[1] == out["postings"] - ust["removed"] and ix.check_url_ids()[0] == 0
        out["retain_" + k] = {"min_day": d, "max_refs": m, "call_ms": round(t_rm, 3), "dry_run_call_ms": round(t_dry, 3),
                              "t_mark_ms": round(rst["t_mark_ns"] / 1e6, 3),
                              "t_select_ms": round(rst["t_select_ns"] / 1e6, 3),
                              "row_gbytes_per_s_mark": round(40 * rst["postings"] / max(rst["t_mark_ns"], 1), 1),
                              "removed_age": rst["removed_age"], "removed_cap": rst["removed_cap"],
                              "lists_age": rst["lists_age"], "lists_cap": rst["lists_cap"],
                              "emptied_terms": rst["emptied_terms"], "launches": ust["launches"], "syncs": ust["syncs"]}
        print(k, json.dumps(out["retain_" + k]), file=sys.stderr, flush=True)

    # ---- the route there was: every list to the host, the selection in numpy, the losers removed per term
    old = ixs["get_list"]
    t_get = t_np = t_rm = 0.0
    removed = changed = 0
    st = _lib.CUpdateStats()
    for t in terms:
        dt, r = ms(lambda: old.get_list(hashes[t]))
        t_get += dt
        dt, u = ms(lambda: losers(r, median, cap))
        t_np += dt
        if not len(u):
            continue
        tb = np.frombuffer(bytes(hashes[t]), dtype=np.uint8)

        def call():
            rc = L.yrwi_remove_postings(old._h, tb.ctypes.data, 1, u.ctypes.data, len(u), ctypes.byref(st))
            assert rc == 0, rc
        dt, _ = ms(call)
        t_rm += dt
        removed += st.removed
        changed += 1
    both = out["retain_both"]
    assert removed == both["removed_age"] + both["removed_cap"], (removed, both)
    assert old.stats()[:2] == ixs["both"].stats()[:2]
    out["get_list_route_both"] = {"total_ms": round(t_get + t_np + t_rm, 3), "get_list_ms": round(t_get, 3),
                                  "numpy_ms": round(t_np, 3), "remove_postings_ms": round(t_rm, 3),
                                  "removed": removed, "lists_changed": changed,
                                  "bytes_to_host": 40 * out["postings"], "bytes_to_device": 12 * removed}
    out["speedup_both"] = round(out["get_list_route_both"]["total_ms"] / max(both["call_ms"], 1e-6), 1)
    out["t_mark_over_count_hosts"] = round(out["retention_count_hist"]["t_mark_ms"] / max(t_hosts, 1e-6), 2)
    out["check_bad"] = [ix.check_url_ids()[0] for ix in ixs.values()]
    for ix in ixs.values():
        ix.close()
    line = json.dumps(out)
    print(line)
    if os.environ.get("INDEX_RETENTION_OUT"):
        with open(os.environ["INDEX_RETENTION_OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
