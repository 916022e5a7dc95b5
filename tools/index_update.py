"""Time index updates on the C2 index (one GPU): the device path (yrwi_add_postings /
yrwi_remove_postings, only the change crosses PCIe) against the same change made through
the whole-list interface (put_list of the host-merged lists).  Both are followed by
build_url_ids(); the host merge is timed separately and is not part of the baseline.

  (a) one document: 512 terms drawn in proportion to df, one posting each;
  (b) one posting into the largest list;
  (c) 100 k postings over 1000 terms (100 documents);
  (d) 1000 urls removed from every list.

Every figure is the median of INDEX_UPDATE_REPS (default 5) repeats on distinct fresh urls in
one process, with the min-max range; a case's device-path repeats run first, then its put_list
repeats (changes of the same shape, other urls), on one context.  One JSON line to stdout (INDEX_UPDATE_OUT: also to
that file)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yacy_search_server_amd import RWIIndex, synth  # noqa: E402

B64 = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_", dtype=np.uint8)
RANK = np.zeros(256, dtype=np.uint64)
RANK[B64] = np.arange(64, dtype=np.uint64)


def key60(rows):
    """order-preserving key of the first 10 url-hash characters (ties are settled on the bytes)"""
    k = np.zeros(len(rows), dtype=np.uint64)
    for j in range(10):
        k = (k << np.uint64(6)) | RANK[rows[:, j]]
    return k


class HostCopy:
    """what a caller of the whole-list interface has to keep: every list, and its sort keys"""

    def __init__(self, idx):
        self.rows = {t: idx.list_rows(t) for t in range(len(idx.hashes)) if idx.sizes[t]}
        self.keys = {t: key60(r) for t, r in self.rows.items()}

    def add(self, t, new):
        """RowSet.put of every row of `new` (fresh urls: no equal key expected, checked)"""
        nk = key60(new)
        o = np.argsort(nk, kind="stable")
        new, nk = new[o], nk[o]
        assert len(nk) < 2 or (nk[1:] != nk[:-1]).all()
        rows, keys = self.rows.get(t), self.keys.get(t)
        if rows is None or len(rows) == 0:
            self.rows[t], self.keys[t] = new, nk
            return
        pos = np.searchsorted(keys, nk)
        assert not (keys[np.minimum(pos, len(keys) - 1)] == nk).any(), "fresh url equal to a stored one in 60 bits"
        self.rows[t] = np.insert(rows, pos, new, axis=0)
        self.keys[t] = np.insert(keys, pos, nk)

    def remove(self, t, urls, uk):
        """-> rows removed from list t (urls sorted by uk)"""
        rows, keys = self.rows[t], self.keys[t]
        pos = np.searchsorted(keys, uk)
        ok = pos < len(keys)
        cand = np.flatnonzero(ok)
        hit = cand[keys[pos[cand]] == uk[cand]]
        hit = hit[(rows[pos[hit], :12] == urls[hit]).all(axis=1)]
        if len(hit) == 0:
            return 0
        self.rows[t] = np.delete(rows, pos[hit], axis=0)
        self.keys[t] = np.delete(keys, pos[hit])
        return len(hit)


def ms(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def ids(ix):
    """build_url_ids timed, with what it did: (ms, full rebuilds, incremental updates, repacks)"""
    a = ix.index_info()
    t, _ = ms(ix.build_url_ids)
    b = ix.index_info()
    return t, tuple(b[k] - a[k] for k in ("full_rebuilds", "incremental_updates", "repacks"))


def summary(v):
    return {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def main():
    cfg = synth.preset(os.environ.get("INDEX_UPDATE_CONFIG", "C2"))
    reps = max(5, int(os.environ.get("INDEX_UPDATE_REPS", "5")))
    scale = cfg.n_terms / 10_000.0  # the smaller presets (smoke runs of this tool) keep the proportions
    idx = synth.build_index(cfg)
    hashes = idx.hashes
    ix = RWIIndex(0)
    for t in range(cfg.n_terms):
        if idx.sizes[t]:
            ix.add(hashes[t], idx.list_rows(t))
    ix.build_url_ids()
    host = HostCopy(idx)
    print("index resident", file=sys.stderr, flush=True)
    rng = np.random.default_rng(2)
    df = idx.sizes / idx.sizes.sum()
    big = int(np.argmax(idx.sizes))
    tarr = np.frombuffer(b"".join(hashes), dtype=np.uint8).reshape(-1, 12)

    def fresh_rows(n):
        r = idx.rows[rng.integers(0, len(idx.rows), n)].copy()
        r[:, :12] = B64[rng.integers(0, 64, (n, 12))]
        return r

    def add_case(nterms, per_term):
        def make():
            terms = [big] if nterms == 1 else [int(t) for t in rng.choice(cfg.n_terms, nterms, replace=False, p=df)]
            docs = fresh_rows(per_term)  # per_term documents, each with every one of the terms
            tix = np.repeat(np.asarray(terms), per_term)
            rows = np.tile(docs, (len(terms), 1))
            return terms, tix, rows
        return make

    def run_add(make, device):
        terms, tix, rows = make()
        if device:  # the device path
            t_call, st = ms(lambda: ix.add_postings(tarr[tix], rows))
            t_ids, did = ids(ix)
            assert st["added"] == len(rows), st
            for t in terms:
                host.add(t, rows[tix == t])
            return dict(call=t_call, ids=t_ids, did=did, launches=st["launches"], syncs=st["syncs"],
                        bytes=len(rows) * 52)
        # the same change through put_list of the host-merged lists
        t_merge, _ = ms(lambda: [host.add(t, rows[tix == t]) for t in terms])
        t_put, _ = ms(lambda: [ix.add(hashes[t], host.rows[t]) for t in terms])
        t_ids, did = ids(ix)
        return dict(call=t_put, ids=t_ids, did=did, merge=t_merge, bytes=sum(len(host.rows[t]) for t in terms) * 40)

    def run_remove(device):
        nu = max(1, int(1000 * min(1.0, scale * 10)))
        u = np.unique(idx.rows[rng.integers(0, len(idx.rows), nu), :12], axis=0)
        uk = key60(u)
        o = np.argsort(uk, kind="stable")
        u, uk = u[o], uk[o]
        if device:
            t_call, st = ms(lambda: ix.remove_postings([bytes(x) for x in u], None))
            t_ids, did = ids(ix)
            removed = sum(host.remove(t, u, uk) for t in list(host.rows))
            assert removed == st["removed"], (removed, st)
            return dict(call=t_call, ids=t_ids, did=did, launches=st["launches"], syncs=st["syncs"],
                        bytes=len(u) * 12, lists_changed=st["terms"])
        changed = []

        def merge():
            for t in list(host.rows):
                if host.remove(t, u, uk):
                    changed.append(t)
        t_merge, _ = ms(merge)
        t_put, _ = ms(lambda: [ix.add(hashes[t], host.rows[t]) for t in changed])
        t_ids, did = ids(ix)
        return dict(call=t_put, ids=t_ids, did=did, merge=t_merge, bytes=sum(len(host.rows[t]) for t in changed) * 40,
                    lists_changed=len(changed))

    n_a = max(2, int(512 * min(1.0, scale * 10)))
    n_c = max(2, int(1000 * min(1.0, scale * 10)))
    cases = [("a_one_document", lambda dev: run_add(add_case(n_a, 1), dev)),
             ("b_one_posting_largest_list", lambda dev: run_add(add_case(1, 1), dev)),
             ("c_100k_postings_1000_terms", lambda dev: run_add(add_case(n_c, 100), dev)),
             ("d_remove_1000_urls_everywhere", run_remove)]
    out = {"config": os.environ.get("INDEX_UPDATE_CONFIG", "C2"), "postings": int(idx.sizes.sum()),
           "terms": int((idx.sizes > 0).sum()), "largest_list": int(idx.sizes[big]), "repeats": reps}
    try:
        import bench
        out.update(bench.source_identity())
    except Exception:  # the identity is a label only
        pass
    for name, run in cases:
        # the repeats of one path in a row, then the other's (alternating them on one context
        # would put every index repack, due once the dead bytes pass the live ones, on one path's turn)
        d = [run(True) for _ in range(reps)]
        b = [run(False) for _ in range(reps)]
        c = {"device_call": summary([x["call"] for x in d]),
             "device_call_plus_url_ids": summary([x["call"] + x["ids"] for x in d]),
             "put_list": summary([x["call"] for x in b]),
             "put_list_plus_url_ids": summary([x["call"] + x["ids"] for x in b]),
             "host_merge_excluded": summary([x["merge"] for x in b]),
             # build_url_ids alone after either path, and what it did in each repeat:
             # [full rebuilds, incremental updates, index repacks]
             "url_ids_after_device_call": summary([x["ids"] for x in d]),
             "url_ids_after_put_list": summary([x["ids"] for x in b]),
             "url_ids_did_after_device_call": [list(x["did"]) for x in d],
             "url_ids_did_after_put_list": [list(x["did"]) for x in b],
             "launches": sorted({x["launches"] for x in d}), "syncs": sorted({x["syncs"] for x in d}),
             "bytes_device_path": int(np.median([x["bytes"] for x in d])),
             "bytes_put_list": int(np.median([x["bytes"] for x in b]))}
        if "lists_changed" in d[0]:
            c["lists_changed"] = int(np.median([x["lists_changed"] for x in b]))
        c["speedup_call"] = round(c["put_list"]["median_ms"] / max(c["device_call"]["median_ms"], 1e-6), 1)
        c["speedup_with_url_ids"] = round(c["put_list_plus_url_ids"]["median_ms"] /
                                          max(c["device_call_plus_url_ids"]["median_ms"], 1e-6), 2)
        out[name] = c
        print(name, json.dumps(c), file=sys.stderr, flush=True)
    bad, _ = ix.check_url_ids()
    out["check_bad"] = bad
    out["index_info"] = ix.index_info()
    ix.close()
    line = json.dumps(out)
    print(line)
    if os.environ.get("INDEX_UPDATE_OUT"):
        with open(os.environ["INDEX_UPDATE_OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
