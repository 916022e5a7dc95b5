"""Time removal and counting by host on the C2 index (one GPU): the device route
(yrwi_count_hosts / yrwi_remove_hosts: only the host hashes cross PCIe) against the route a
caller had before them: get_list of every term (40 B per posting to the host), a numpy test of
the host part of every url hash, then yrwi_remove_postings with the url hashes found.

The synthetic corpora spread their postings over very many host parts with a handful of
postings each, so the index is re-hosted first (rehost(), the vectorised form of
tests/host_ref.py's): INDEX_HOSTS_H hosts (default 16384) with weights 1 / (1 + rank).  The host
sets are runs of ranks: 1 host from rank 10, 64 hosts from rank 100, 4096 hosts from rank 1000;
repeat r takes the run after repeat r - 1's, so every repeat removes hosts that are still there
(about 0.9 %, 4.8 % and 15 % of the postings in the first repeat).  Two contexts hold the same
index; one takes the device route, the other the get_list route, with the same sets, and the
`removed` of both must agree.  Every figure is the median of INDEX_HOSTS_REPS (default 3) repeats
with the min-max range.  count_hosts runs before the removal, over every list, and its call time
gives the marking pass's key bytes per second (9 B per selected posting; the call's host work and
waits included, so a lower bound of the kernel's rate).  One JSON line to stdout
(INDEX_HOSTS_OUT: also to that file)."""
import ctypes
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B64 = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_", dtype=np.uint8)
RANK = np.zeros(256, dtype=np.uint64)
RANK[B64] = np.arange(64, dtype=np.uint64)


def key_of(chars):
    """order-preserving key of (n, w) url-hash characters, w <= 10"""
    k = np.zeros(len(chars), dtype=np.uint64)
    for j in range(chars.shape[1]):
        k = (k << np.uint64(6)) | RANK[chars[:, j]]
    return k


def crc32_rows(b):
    """zlib.crc32 of every row of the (n, w) uint8 array"""
    t = np.arange(256, dtype=np.uint32)
    for _ in range(8):
        t = np.where(t & 1, (t >> 1) ^ np.uint32(0xEDB88320), t >> 1).astype(np.uint32)
    c = np.full(len(b), 0xFFFFFFFF, dtype=np.uint32)
    for j in range(b.shape[1]):
        c = t[(c ^ b[:, j]) & np.uint32(0xFF)] ^ (c >> np.uint32(8))
    return c ^ np.uint32(0xFFFFFFFF)


def host_names(H):
    """(H, 6) uint8, ascending in Base64Order: tests/host_ref.py's names up to 4096 hosts, one more digit above"""
    i = np.arange(H)
    n = np.empty((H, 6), dtype=np.uint8)
    if H <= 4096:
        n[:, :4] = np.frombuffer(b"h0st", dtype=np.uint8)
    else:
        n[:, :3] = np.frombuffer(b"h0s", dtype=np.uint8)
        n[:, 3] = B64[i >> 12]
    n[:, 4] = B64[(i >> 6) & 63]
    n[:, 5] = B64[i & 63]
    return n


def rehost(rows, sizes, H):
    """tests/host_ref.py rehost() on the concatenated lists, in place where it can: -> (rows, sizes, host
    rank of every row).  A list stays ascending except where rows share their first six characters:
    those runs are sorted again, and of rows that now share a url hash the first stays."""
    w = 1.0 / (1.0 + np.arange(H))
    cdf = np.cumsum(w / w.sum())
    x = (crc32_rows(rows[:, :12]) & np.uint32(0xFFFFFF)) / 2.0 ** 24
    rank = np.minimum(np.searchsorted(cdf, x, side="right"), H - 1).astype(np.int32)
    del x
    rows[:, 6:12] = host_names(H)[rank]
    k36 = key_of(rows[:, :6])
    lid = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    tie = np.flatnonzero((k36[1:] == k36[:-1]) & (lid[1:] == lid[:-1]))
    del k36
    drop = []
    p = 0
    while p < len(tie):  # maximal runs of rows with equal first six characters
        q = p
        while q + 1 < len(tie) and tie[q + 1] == tie[q] + 1:
            q += 1
        a, b = int(tie[p]), int(tie[q]) + 2
        o = a + np.argsort(rank[a:b], kind="stable")
        rows[a:b], rank[a:b] = rows[o], rank[o]
        drop += [a + 1 + int(d) for d in np.flatnonzero(rank[a + 1:b] == rank[a:b - 1])]
        p = q + 1
    if drop:
        keep = np.ones(len(rows), dtype=bool)
        keep[drop] = False
        sizes = sizes - np.bincount(lid[drop], minlength=len(sizes))
        rows, rank = rows[keep], rank[keep]
    return rows, sizes, rank


def ms(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def summary(v):
    return {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def main():
    from yacy_search_server_amd import RWIIndex, _lib, synth
    name = os.environ.get("INDEX_HOSTS_CONFIG", "C2")
    cfg = synth.preset(name)
    reps = max(1, int(os.environ.get("INDEX_HOSTS_REPS", "3")))
    H = int(os.environ.get("INDEX_HOSTS_H", "16384"))
    idx = synth.build_index(cfg)
    print("index built", file=sys.stderr, flush=True)
    rows, sizes, rank = rehost(idx.rows, idx.sizes.copy(), H)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    per_rank = np.bincount(rank, minlength=H)
    del rank
    terms = [t for t in range(cfg.n_terms) if sizes[t]]
    hashes = idx.hashes
    names = host_names(H)
    print("index re-hosted:", len(rows), "postings", file=sys.stderr, flush=True)
    ixs = []
    for _ in range(2):  # [0]: the device route, [1]: the get_list route
        ix = RWIIndex(0)
        for t in terms:
            ix.add(hashes[t], rows[offsets[t]:offsets[t] + sizes[t]])
        ix.build_url_ids()
        ixs.append(ix)
    dev, old = ixs
    del rows
    print("two contexts resident", file=sys.stderr, flush=True)
    L = _lib.lib()

    def device_route(hosts):
        hl = [bytes(h) for h in hosts]
        selected = dev.stats()[1]
        t_count, (counts, lists_hit) = ms(lambda: dev.count_hosts(hl, None))
        t_rm, st = ms(lambda: dev.remove_hosts(hl, None))
        assert int(counts.sum()) == st["removed"] and lists_hit == st["terms"], (counts.sum(), lists_hit, st)
        return dict(count=t_count, remove=t_rm, removed=st["removed"], lists=st["terms"], launches=st["launches"],
                    syncs=st["syncs"], key_bytes=9 * selected, emptied=st["emptied_terms"])

    def get_list_route(hosts):
        hk = np.sort(key_of(hosts))
        t_get = t_np = 0.0
        found = []
        for t in terms:
            dt, r = ms(lambda: old.get_list(hashes[t]))
            t_get += dt
            dt, u = ms(lambda: r[np.isin(key_of(r[:, 6:12]), hk), :12])
            t_np += dt
            if len(u):
                found.append(u)
        dt, urls = ms(lambda: np.unique(np.concatenate(found), axis=0) if found else np.zeros((0, 12), np.uint8))
        t_np += dt
        urls = np.ascontiguousarray(urls)
        st = _lib.CUpdateStats()

        def call():
            rc = L.yrwi_remove_postings(old._h, None, 0, urls.ctypes.data if len(urls) else None, len(urls),
                                        ctypes.byref(st))
            assert rc == 0, rc
        t_rm, _ = ms(call)
        return dict(get_list=t_get, numpy=t_np, remove_postings=t_rm, removed=st.removed, urls=len(urls),
                    bytes_to_host=40 * old.stats()[1] + 40 * st.removed)

    out = {"config": name, "hosts_in_index": H, "postings": int(per_rank.sum()), "terms": len(terms), "repeats": reps}
    try:
        import bench
        out.update(bench.source_identity())
    except Exception:  # the identity is a label only
        pass
    for n, first in ((1, 10), (64, 100), (4096, 1000)):
        d, b = [], []
        for r in range(reps):
            lo = min(first + r * n, H - n)
            hosts = names[lo:lo + n]
            d.append(device_route(hosts))
            b.append(get_list_route(hosts))
            assert d[-1]["removed"] == b[-1]["removed"] == int(per_rank[lo:lo + n].sum()), (d[-1], b[-1])
        c = {"count_hosts": summary([x["count"] for x in d]),
             "remove_hosts": summary([x["remove"] for x in d]),
             "get_list_route": summary([x["get_list"] + x["numpy"] + x["remove_postings"] for x in b]),
             "get_list_route_get_list": summary([x["get_list"] for x in b]),
             "get_list_route_numpy": summary([x["numpy"] for x in b]),
             "get_list_route_remove_postings": summary([x["remove_postings"] for x in b]),
             "removed": [x["removed"] for x in d], "lists_changed": [x["lists"] for x in d],
             "lists_emptied": [x["emptied"] for x in d], "urls_get_list_route": [x["urls"] for x in b],
             "launches": sorted({x["launches"] for x in d}), "syncs": sorted({x["syncs"] for x in d}),
             # the marking pass: 9 key bytes per selected posting over the whole count_hosts call
             "mark_key_gbytes_per_s": round(float(np.median([x["key_bytes"] / x["count"] / 1e6 for x in d])), 1),
             "bytes_to_host_get_list_route": int(np.median([x["bytes_to_host"] for x in b])),
             "bytes_to_device_device_route": 6 * n}
        c["speedup_remove"] = round(c["get_list_route"]["median_ms"] / max(c["remove_hosts"]["median_ms"], 1e-6), 1)
        out["hosts_%d" % n] = c
        print(n, json.dumps(c), file=sys.stderr, flush=True)
    out["check_bad"] = [ix.check_url_ids()[0] for ix in ixs]
    out["stats_equal"] = dev.stats()[:2] == old.stats()[:2]
    for ix in ixs:
        ix.close()
    line = json.dumps(out)
    print(line)
    if os.environ.get("INDEX_HOSTS_OUT"):
        with open(os.environ["INDEX_HOSTS_OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
