"""bench.py's launcher: `--gpus N` starts N rank processes itself (RANK /
LOCAL_RANK / WORLD_SIZE / MASTER_* set, before anything touches a GPU); checked
on the CPU with the --dry-run rendezvous over gloo."""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args, env=None):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout  # only rank 0 prints
    return lines[0]


def test_gpus_2_launches_two_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = _run("--gpus", "2", "--dry-run", "--steps", "3", "--warmup", "1", env=env)
    assert out["n_gpus"] == 2 and out["ranks_sum"] == 3.0 and out["steps"] == 3


def test_gpus_1_single_process():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = _run("--dry-run", env=env)
    assert out["n_gpus"] == 1


def test_compact_line_fits_the_driver_tail():
    """The stdout line stays a few KB (round 4's 20 KB line overflowed the driver's
    tail): rebuilt from round 4's full record, it keeps the contract's fields, the
    roofline, the CPU baseline, parity, latency and one summary per leg."""
    sys.path.insert(0, ROOT)
    import bench
    with open(os.path.join(ROOT, "profiles", "archive", "r04_bench.json")) as f:
        full = json.load(f)
    full["build"] = bench.source_identity()
    line = bench.compact_line(full, "profiles/bench_detail_x.json")
    s = json.dumps(line)
    assert len(s) <= 6000, len(s)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype", "config",
              "roofline", "cpu_baseline", "parity_sample", "latency_ms", "legs", "detail"):
        assert k in line, k
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in line["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in line["cpu_baseline"], k
    assert set(line["legs"]) == {"C3", "C4", "C5_custom", "C5_date"}
    assert all("ms_per_step" in v and "frac" in v for v in line["legs"].values())


def test_line_reports_the_shard_transport():
    """world > 1: the line names how the shards' collectives travelled and the RCCL
    communicators' rank counts (min / max over the ranks, from yrwi_shard_info), so
    an 8-GPU record shows that RCCL saw 8 ranks -- or that it did not."""
    sys.path.insert(0, ROOT)
    import bench
    with open(os.path.join(ROOT, "profiles", "archive", "r04_bench.json")) as f:
        full = json.load(f)
    info = lambda r, t, n, peers: {"transport": t, "rank": r, "world": 8, "rccl_ranks": n, "lanes": 8,
                                   "lanes_own_comm": 8 if n else 0, "device_peers": peers, "mailbox": 1,
                                   "pci_bus_id": f"0000:{r:02x}:00.0"}
    full["shard_transport"] = bench.transport_summary([info(r, "rccl", 8, 0) for r in range(8)])
    line = bench.compact_line(full, "profiles/bench_detail_x.json")
    assert len(json.dumps(line)) <= 6000
    assert line["transport"] == "rccl" and line["rccl_ranks"] == {"min": 8, "max": 8}
    assert "k_compact" in line["roofline_kernels"] and "frac" in line["roofline_kernels"]["k_compact"]
    mixed = bench.transport_summary([info(0, "rccl", 2, 0), info(1, "host-staged", 0, 1)])
    assert mixed["transport"] == ["rccl", "host-staged"] and mixed["rccl_ranks"] == {"min": 0, "max": 2}
    assert mixed["ranks_sharing_a_device"] == 1
    assert bench.transport_summary([None, None]) is None
    # one GPU: no transport keys
    full.pop("shard_transport")
    assert "transport" not in bench.compact_line(full, "x")


def test_plain_run_is_the_default_and_its_line_keeps_the_contract():
    """Without --full the bench times the headline alone: the line still carries the
    contract's fields, and what --full measures is absent (null), not invented."""
    sys.path.insert(0, ROOT)
    import bench
    assert bench.parse_args([]).full is False and bench.parse_args(["--full"]).full is True
    with open(os.path.join(ROOT, "profiles", "archive", "r04_bench.json")) as f:
        full = json.load(f)
    for k in ("roofline", "roofline_kernels", "cpu_baseline", "cpu_baseline_1thread", "parity_sample", "latency_ms",
              "legs", "phase_ms", "identical_batch"):
        full[k] = None
    line = bench.compact_line(full, None)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert line[k] == full[k], k
    assert line["roofline"] is None and line["cpu_baseline"] is None and "legs" not in line and line["detail"] is None


def _fake_last_step(nq, k, seed=7):
    import ctypes
    import numpy as np
    from yacy_search_server_amd._lib import CHit
    rng = np.random.default_rng(seed)
    nout = rng.integers(0, k + 1, nq)
    nout[0], nout[-1] = k, 0
    hits = (CHit * (nq * k))()
    raw = np.frombuffer(hits, dtype=np.uint8)
    raw[:] = rng.integers(0, 256, raw.size, dtype=np.uint8)  # rows past nout hold garbage, as stale buffers do
    for i in range(nq * k):
        hits[i].score = int(rng.integers(-(1 << 40), 1 << 40))
    return hits, nout, {"last_out": {"batch": 3, "hits": bytes(memoryview(hits).cast("B")), "nout": [int(x) for x in nout]}}


def test_dump_outputs_writes_the_last_steps_hits(tmp_path):
    """--dump-outputs: every array is float32 / float64 and holds the caller's hits
    exactly (rank order, zero past each query's count), the same from call to call."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    nq, k = 37, 5
    hits, nout, M = _fake_last_step(nq, k)
    bench.dump_outputs(str(tmp_path / "a"), M, k)
    bench.dump_outputs(str(tmp_path / "b"), M, k)
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("nout", "score", "tiebreak", "urlhash", "query", "step")}
    for n, a in got.items():
        assert a.dtype in (np.float32, np.float64), n
        assert np.array_equal(a, np.load(tmp_path / "b" / (n + ".npy"))), n
    assert got["score"].shape == (nq, k) and got["urlhash"].shape == (nq, k, 12)
    assert got["nout"].tolist() == nout.tolist() and got["query"].tolist() == list(range(nq))
    assert got["step"].tolist() == [3, nq]
    for q in range(nq):
        for j in range(k):
            h = hits[q * k + j]
            want = (h.score, h.tiebreak, list(h.urlhash)) if j < nout[q] else (0, 0, [0] * 12)
            assert (got["score"][q, j], got["tiebreak"][q, j], got["urlhash"][q, j].tolist()) == want, (q, j)


def test_dump_outputs_samples_a_large_batch(tmp_path, monkeypatch):
    """Past the size cap a fixed, seeded sample of the queries is written (ascending,
    named in query.npy), within the cap."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    nq, k = 64, 4
    hits, nout, M = _fake_last_step(nq, k)
    per_query = 16 + k * 64
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 16 + 10 * per_query + 5)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), M, k)
    files = sorted(os.listdir(tmp_path / "a"))
    arrs = {f: np.load(tmp_path / "a" / f) for f in files}
    assert sum(a.nbytes for a in arrs.values()) <= bench.DUMP_MAX_BYTES
    sel = arrs["query.npy"].astype(int)
    assert len(sel) == 10 and list(sel) == sorted(set(sel)) and sel.max() < nq
    assert all(np.array_equal(arrs[f], np.load(tmp_path / "b" / f)) for f in files)
    assert arrs["nout.npy"].tolist() == nout[sel].tolist()
    for r, q in enumerate(sel):
        assert arrs["score.npy"][r].tolist() == [hits[q * k + j].score if j < nout[q] else 0 for j in range(k)]


@pytest.mark.gpu
def test_plain_bench_dumps_what_the_last_timed_step_returned(tmp_path):
    """A plain run on a small corpus: --steps sets the timed steps, the line has
    ms_per_step and nothing of --full, and the dumped hits of the last step (step
    2: distinct batch 2) are the oracle's, hash for hash and score for score."""
    import numpy as np
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import bench
    import oracle as orc
    from yacy_search_server_amd import synth
    nq, k = 16, 100
    env = {k_: v for k_, v in os.environ.items() if k_ not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = _run("--gpus", "1", "--config", "dense", "--nq", str(nq), "--steps", "3", "--warmup", "1",
               "--dump-outputs", str(tmp_path / "o"), env=env)
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
    assert out["value"] == pytest.approx(out["config"]["postings_per_step"] / (out["ms_per_step"] * 1e-3))
    assert out["roofline"] is None and out["cpu_baseline"] is None and out["parity_sample"] is None
    assert out["latency_ms"] is None and "legs" not in out and out["detail"] is None
    a = {n: np.load(tmp_path / "o" / (n + ".npy")) for n in ("nout", "score", "urlhash", "query", "step")}
    assert a["step"].tolist() == [2, nq] and a["query"].tolist() == list(range(nq))
    cfg = synth.preset("dense")
    idx = synth.build_index(cfg)
    d = idx.as_dict()
    qs = bench.draws(cfg, nq, 2, 2, 0, None, 8)[2]
    for qi, (inc, exc) in enumerate(qs):
        exp = orc.search(d, [idx.hashes[t] for t in inc], [idx.hashes[t] for t in exc], now_ms=bench.NOW_MS, k=k)
        n = int(a["nout"][qi])
        assert n == len(exp), qi
        got = [(bytes(a["urlhash"][qi, j].astype(np.uint8)), int(a["score"][qi, j])) for j in range(n)]
        assert got == [(h, s) for h, s, _ in exp], qi
