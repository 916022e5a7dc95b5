"""Time the host census on the C2 index (one GPU): yrwi_host_census (one pass over the 9 key bytes
of every posting, only the result crosses PCIe) against the pass it is measured by and the route a
caller had before it, on two indexes: C2 as generated (very many hosts of a few postings each) and
C2 re-hosted to HOST_CENSUS_H hosts (default 4096) with weights 1 / (1 + rank) (few hosts, skewed;
tools/index_hosts.py's rehost()).  On each index:

  host_census   in both orders, every list, every host (two calls each: how many pass, then all);
  count_hosts   with one host over every list: the same 9 B per posting through k_host_mark, a
                lookup in a given set instead of a group-by -- the yardstick of the counting pass;
  get_list      of every term (40 B per posting to the host) and numpy.unique over bytes 6..11:
                the only route without the census.  Run once; the others HOST_CENSUS_REPS times
                (default 3), median and min-max range.

The census is checked against the numpy result, hosts and counts in both orders, before a time is
printed.  The statistics of a census call (yrwi_census_stats) are printed as they come, with the
achieved key bytes per second of the counting pass, 9 x postings / t_count_ns.  One JSON line to
stdout (HOST_CENSUS_OUT: also to that file)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import index_hosts as ih  # noqa: E402  (rehost, key_of, ms, summary)

STAT_KEYS = ("lists", "postings", "hosts", "hosts_passing", "table_slots", "passes", "lds_bypass", "launches", "syncs",
             "t_count_ns", "t_total_ns")


def measure(label, hashes, rows, sizes, reps):
    """one index: resident, checked, timed -> the record of `label`"""
    from yacy_search_server_amd import RWIIndex
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    terms = [t for t in range(len(sizes)) if sizes[t]]
    ix = RWIIndex(0)
    for t in terms:
        ix.add(hashes[t], rows[offsets[t]:offsets[t] + sizes[t]])
    print(label, "resident:", int(sizes.sum()), "postings", file=sys.stderr, flush=True)
    # ---- the route without the census: every list to the host, a group-by there
    t_get = t_np = 0.0
    keys = []
    for t in terms:
        dt, r = ih.ms(lambda: ix.get_list(hashes[t]))
        t_get += dt
        dt, k = ih.ms(lambda: ih.key_of(r[:, 6:12]))
        t_np += dt
        keys.append(k)
    dt, (uk, uc) = ih.ms(lambda: np.unique(np.concatenate(keys), return_counts=True))
    t_np += dt
    del keys
    uc = uc.astype(np.int64)
    by_count = np.lexsort((uk, -uc))
    expect = {"host": (uk, uc), "count": (uk[by_count], uc[by_count])}
    # ---- the census, checked before it is timed
    out = {"postings": int(sizes.sum()), "terms": len(terms), "hosts": int(len(uk)), "largest_host": int(uc.max()),
           "get_list_route_ms": round(t_get + t_np, 3), "get_list_route_get_list_ms": round(t_get, 3),
           "get_list_route_numpy_ms": round(t_np, 3), "bytes_to_host_get_list_route": 40 * int(sizes.sum())}
    for order in ("host", "count"):
        hosts, counts, st = ix.host_census(None, order)
        got = ih.key_of(np.frombuffer(b"".join(hosts), dtype=np.uint8).reshape(-1, 6))
        assert len(got) == len(uk) and (got == expect[order][0]).all() and (counts == expect[order][1]).all(), order
        assert st["postings"] == counts.sum() == sizes.sum() and st["hosts"] == st["hosts_passing"] == len(uk), st
        calls, stats = [], []
        for _ in range(reps):
            dt, (_, _, st) = ih.ms(lambda: ix.host_census(None, order))
            calls.append(dt)
            stats.append(st)
        top, _ = ih.ms(lambda: ix.host_census(None, order, top=100))
        st = stats[-1]
        rec = {"two_calls": ih.summary(calls), "top_100_one_call_ms": round(top, 3),
               "count_pass_ms": ih.summary([s["t_count_ns"] / 1e6 for s in stats]),
               "last_call_ms": ih.summary([s["t_total_ns"] / 1e6 for s in stats]),
               "count_pass_key_gbytes_per_s": round(float(np.median([9 * s["postings"] / s["t_count_ns"] for s in stats])), 1),
               "stats": {k: st[k] for k in STAT_KEYS},
               "lds_bypass_share": round(st["lds_bypass"] / max(st["postings"], 1), 4),
               "bytes_to_host": 14 * st["hosts_passing"]}
        out["host_census_by_" + order] = rec
        print(label, order, json.dumps(rec), file=sys.stderr, flush=True)
    # ---- the yardstick: the marking pass with one host over every list
    big = bytes(ih.B64[(int(uk[by_count[0]]) >> (6 * np.arange(5, -1, -1))) & 63])
    calls = []
    for _ in range(reps):
        dt, (c, _) = ih.ms(lambda: ix.count_hosts([big], None))
        calls.append(dt)
        assert int(c[0]) == int(uc.max())
    out["count_hosts_one_host"] = ih.summary(calls)
    out["count_hosts_key_gbytes_per_s"] = round(9 * int(sizes.sum()) / np.median(calls) / 1e6, 1)  # the whole call
    ix.close()
    print(label, json.dumps(out), file=sys.stderr, flush=True)
    return out


def main():
    from yacy_search_server_amd import synth
    name = os.environ.get("HOST_CENSUS_CONFIG", "C2")
    cfg = synth.preset(name)
    reps = max(1, int(os.environ.get("HOST_CENSUS_REPS", "3")))
    H = int(os.environ.get("HOST_CENSUS_H", "4096"))
    idx = synth.build_index(cfg)
    print("index built", file=sys.stderr, flush=True)
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
    if os.environ.get("HOST_CENSUS_OUT"):
        with open(os.environ["HOST_CENSUS_OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
