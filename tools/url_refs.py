"""Time yrwi_url_references on the C2 index (one GPU), every list selected, for url sets of 1, 16, 256,
4096 and 65,536 urls drawn from the index: counting, fetching into a pinned buffer and fetching into a
pageable one, with each path forced (YRWI_REFS_PATH = stream | probe) and with the call's own choice,
against the only route there was before the call: get_list of every term (40 B per posting to the host)
and numpy.isin on bytes 0..11 of every row.  The tool runs that route itself (every list fetched once and
tested against every set; a set's figure is that transfer plus its own numpy time), and its
references -- the rows in term order and the count of every url -- must equal the call's.

Every figure is the median of URL_REFS_REPS (default 5) repeats with the min-max range, after one
unmeasured call of each kind; `find` is the call's t_find_ns (the finding kernel alone), `call` the wall
time of the whole call.  `crossover` gives, per set, which forced path counted faster: the dispatch
constant REF_PROBE_STEP_KEYS (yrwi_update.hip) is set between the largest set PROBE wins and the smallest
STREAM wins, as `step_keys_*` says.  One JSON line to stdout (URL_REFS_OUT: also to that file)."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = (1, 16, 256, 4096, 65536)
B64 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"
RANK = bytes.maketrans(B64, bytes(range(64)))


def s12(a):
    return np.ascontiguousarray(a[:, :12]).view("S12").ravel()


def ms(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def summary(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    from yacy_search_server_amd import RWIIndex, _lib, synth
    name = os.environ.get("URL_REFS_CONFIG", "C2")
    reps = max(1, int(os.environ.get("URL_REFS_REPS", "5")))
    sets = [int(x) for x in os.environ.get("URL_REFS_SETS", ",".join(map(str, SETS))).split(",")]
    cfg = synth.preset(name)
    idx = synth.build_index(cfg)
    print("index built", file=sys.stderr, flush=True)
    terms = [t for t in range(cfg.n_terms) if idx.sizes[t]]
    ix = RWIIndex(0)
    for t in terms:
        ix.add(idx.hashes[t], idx.list_rows(t))
    by_key = sorted(terms, key=lambda t: bytes(idx.hashes[t]).translate(RANK))  # the order of YRWI_REFS_BY_TERM
    nrows = len(idx.rows)
    rng = np.random.default_rng(20741)
    print("index resident:", nrows, "postings", file=sys.stderr, flush=True)

    def call(urls, cap, rows_out, terms_out, counts):
        rc, st = ix.url_references_raw(urls, None, _lib.REFS_BY_TERM, counts, terms_out, rows_out, cap)
        assert rc == 0, rc
        return st

    def get_list_route(usets):
        """every list fetched once and tested against every set -> (ms of get_list, per set: ms of numpy, per set:
        the references' rows in term order)"""
        t_get, t_np, found = 0.0, [0.0] * len(usets), [[] for _ in usets]
        for t in by_key:
            dt, r = ms(lambda: ix.get_list(idx.hashes[t]))
            t_get += dt
            h = s12(r)
            for k, uset in enumerate(usets):
                dt, hit = ms(lambda: r[np.isin(h, uset)])
                t_np[k] += dt
                if len(hit):
                    found[k].append(hit)
        return t_get, t_np, [np.concatenate(f) if f else np.zeros((0, 40), np.uint8) for f in found]

    out = {"config": name, "postings": nrows, "lists": len(terms), "repeats": reps, "ref_lds_max": _lib.REF_LDS_MAX}
    try:
        import bench
        out.update(bench.source_identity())
    except Exception:  # the identity is a label only
        pass
    crossover, usets = {}, []
    for n in sets:
        pick = np.unique(s12(idx.rows[rng.choice(nrows, 2 * n + 64, replace=False)]))
        usets.append(rng.permutation(pick)[:n])
        assert len(usets[-1]) == n
    t_get, t_nps, old = get_list_route([np.sort(u) for u in usets])
    print("get_list route done: get_list %.0f ms" % t_get, file=sys.stderr, flush=True)
    for n, uset, t_np, old_rows in zip(sets, usets, t_nps, old):
        urls = uset.tobytes()
        counts = np.zeros(n, dtype=np.int64)
        os.environ.pop("YRWI_REFS_PATH", None)
        st = call(urls, 0, None, None, counts)
        refs = st.refs
        pinned = np.ctypeslib.as_array(ix.host_array(ctypes.c_uint8, 40 * max(refs, 1)))
        pageable = np.zeros(40 * max(refs, 1), dtype=np.uint8)
        tout = np.zeros((max(refs, 1), 12), dtype=np.uint8)
        c = {"refs": int(refs), "urls_found": int(st.urls_found), "lists_hit": int(st.lists_hit)}
        # the route there was, and the equality of what both routes find
        c["get_list_route"] = {"get_list_ms": round(t_get, 1), "numpy_ms": round(t_np, 1), "total_ms": round(t_get + t_np, 1),
                               "bytes_to_host": 40 * nrows}
        st = call(urls, refs, pageable, tout, counts)
        assert len(old_rows) == refs and pageable[:40 * refs].tobytes() == old_rows.tobytes(), (n, len(old_rows), refs)
        found, per = np.unique(s12(old_rows), return_counts=True)
        want = dict(zip(found.tolist(), per.tolist()))
        assert [want.get(u, 0) for u in uset.tolist()] == counts.tolist(), n
        c["equal_to_get_list_route"] = True
        for path in ("auto", "stream", "probe"):
            if path == "auto":
                os.environ.pop("YRWI_REFS_PATH", None)
            else:
                os.environ["YRWI_REFS_PATH"] = path
            kinds = {"count": (0, None, None), "fetch_pinned": (refs, pinned, tout), "fetch_pageable": (refs, pageable, tout)}
            p = {}
            for kind, (cap, rows_out, terms_out) in kinds.items():
                if cap == 0 and kind != "count":
                    continue
                st = call(urls, cap, rows_out, terms_out, counts)  # unmeasured: scratch and staging reach their size
                walls, finds = [], []
                for _ in range(reps):
                    dt, st = ms(lambda: call(urls, cap, rows_out, terms_out, counts))
                    walls.append(dt)
                    finds.append(st.t_find_ns / 1e6)
                assert st.refs == refs
                if kind != "count":
                    assert rows_out[:40 * refs].tobytes() == old_rows.tobytes(), (n, path, kind)
                p[kind] = {"call": summary(walls), "find": summary(finds)}
                p["stats"] = {f: getattr(st, f) for f, _ in _lib.CRefStats._fields_}
            p["path_taken"] = "probe" if p["stats"]["path"] == _lib.REFS_PROBE else "stream"
            c[path] = p
            print(n, path, json.dumps(p), file=sys.stderr, flush=True)
        os.environ.pop("YRWI_REFS_PATH", None)
        s_ms, p_ms = c["stream"]["count"]["find"]["median_ms"], c["probe"]["count"]["find"]["median_ms"]
        steps = 1
        while (1 << steps) < nrows // len(terms) + 1:
            steps += 1
        # PROBE is taken when lists * urls * steps * REF_PROBE_STEP_KEYS <= postings: the constant at which this set tips
        c["step_keys_tip"] = round(nrows / (len(terms) * n * steps), 3)
        c["faster_count"] = "probe" if p_ms < s_ms else "stream"
        c["speedup_fetch_vs_get_list"] = round(c["get_list_route"]["total_ms"] /
                                               max(c["auto"].get("fetch_pageable", c["auto"]["count"])["call"]["median_ms"], 1e-6), 1)
        crossover[n] = c["faster_count"]
        out["urls_%d" % n] = c
        ix._pinned.remove(pinned.ctypes.data)
        _lib.lib().yrwi_host_free(ix._h, pinned.ctypes.data)
    out["crossover"] = crossover
    probe_wins = [out["urls_%d" % n]["step_keys_tip"] for n in sets if crossover[n] == "probe"]
    stream_wins = [out["urls_%d" % n]["step_keys_tip"] for n in sets if crossover[n] == "stream"]
    out["step_keys_at_most"] = min(probe_wins) if probe_wins else None    # PROBE still wins at this tip ...
    out["step_keys_at_least"] = max(stream_wins) if stream_wins else None  # ... and STREAM already at this one
    out["check_bad"] = ix.check_url_ids()[0]
    ix.close()
    line = json.dumps(out)
    print(line)
    if os.environ.get("URL_REFS_OUT"):
        with open(os.environ["URL_REFS_OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
