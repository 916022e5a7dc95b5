#!/usr/bin/env python3
"""What the pair cache (csrc/yrwi_pair_cache.h) can hold of the benchmark's C2
stream, from the generator alone (CPU only).

For the 8 batches bench.py cycles: every distinct two-term query's joined rows, estimated as
|a| |b| / n_urls from the generated list lengths (synth.counts); how the rows concentrate in
the largest queries; the share of a batch's rows in pairs of at least the admission minimum
(YRWI_PAIR_CACHE_MIN_ROWS), and of those the share another of the 8 batches asks too; the
distinct pairs of that size over all batches and the bytes that hold them (36 B per row: a
32-byte record and a url id).

  python3 tools/pair_cache_estimate.py [--min-rows 16384] [--json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from yacy_search_server_amd import synth  # noqa: E402
from batch_repeats import NBATCH, draws  # noqa: E402

ROW_BYTES = 36


def estimate(min_rows):
    cfg = synth.preset("C2")
    n = synth.counts(cfg)
    batches = []
    for qs in draws(cfg, 1000, 2, 2, 0, None, NBATCH):
        pairs = {}
        for inc, _ in qs:
            t = tuple(sorted(set(inc)))
            if len(t) == 2:
                pairs[t] = float(n[t[0]]) * float(n[t[1]]) / cfg.n_urls
        batches.append(pairs)
    out = {"min_rows": min_rows, "batches": []}
    for b, pairs in enumerate(batches):
        rows = sorted(pairs.values(), reverse=True)
        total = sum(rows)
        others = set().union(*(set(p) for i, p in enumerate(batches) if i != b))
        big = {t: r for t, r in pairs.items() if r >= min_rows}
        out["batches"].append({
            "batch": b, "queries": len(pairs), "rows": total,
            "top10": sum(rows[:10]) / total, "top50": sum(rows[:50]) / total, "top200": sum(rows[:200]) / total,
            "median_rows": rows[len(rows) // 2],
            "small_queries": sum(r <= 2048 for r in rows), "small_share": sum(r for r in rows if r <= 2048) / total,
            "admitted_pairs": len(big), "admitted_share": sum(big.values()) / total,
            "recurring_share": sum(r for t, r in big.items() if t in others) / total})
    allbig = {}
    for pairs in batches:
        allbig.update({t: r for t, r in pairs.items() if r >= min_rows})
    out["pairs"] = len(allbig)
    out["pair_rows"] = sum(allbig.values())
    out["pair_bytes"] = ROW_BYTES * sum(allbig.values())
    out["largest"] = max(allbig.items(), key=lambda kv: kv[1]) if allbig else None
    if out["largest"]:
        (a, b), r = out["largest"]
        out["largest"] = {"lists": [int(n[a]), int(n[b])], "rows": r}
    return out


def main(argv):
    min_rows = int(argv[argv.index("--min-rows") + 1]) if "--min-rows" in argv else 16384
    e = estimate(min_rows)
    if "--json" in argv:
        print(json.dumps(e))
        return 0
    print(f"C2, {NBATCH} batches of 1000 two-term queries; rows per distinct query = |a| |b| / n_urls; "
          f"admission minimum {min_rows} rows")
    print("batch  queries  rows(M)  top10  top50  top200  median  <=2048 rows: queries, share   "
          "pairs >= min: n, share, also in another batch")
    for t in e["batches"]:
        print(f"{t['batch']:5d}  {t['queries']:7d}  {t['rows'] / 1e6:7.2f}  {100 * t['top10']:4.0f}%  "
              f"{100 * t['top50']:4.0f}%  {100 * t['top200']:5.0f}%  {t['median_rows']:6.0f}  "
              f"{t['small_queries']:5d}, {100 * t['small_share']:4.1f}%                  "
              f"{t['admitted_pairs']:4d}, {100 * t['admitted_share']:4.1f}%, {100 * t['recurring_share']:4.1f}%")
    print(f"all batches: {e['pairs']} distinct pairs of at least {min_rows} rows, {e['pair_rows'] / 1e6:.1f} M rows, "
          f"{e['pair_bytes'] / 1e9:.2f} GB at {ROW_BYTES} B per row")
    if e["largest"]:
        la = e["largest"]
        print(f"largest pair: {la['lists'][0] / 1e6:.2f} M x {la['lists'][1] / 1e6:.2f} M postings, "
              f"about {la['rows'] / 1e3:.0f} k rows")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
