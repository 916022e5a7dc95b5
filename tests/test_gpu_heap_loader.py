"""The heap loader on the device (yrwi_load_heaps) on the directed inputs of tests/heap_cases.py
against oracle/heap.py's load_reference: exact bytes of every list, exact counters.

  test_cases_through_library   every Load twice, by file name with shuffled paths and in plain
                               oldest-first order: the rank merge's geometry (k_union_b, k_union_a,
                               k_union_bs: one list beside, inside or equal to the other, one-row
                               lists, duplicates at the ends, the 256-thread grid edges), the 31
                               owner sets of four files and RAM, unsorted tails through the host
                               sort, the three row faults and SpaceExceeded, the record rules;
                               then two-term queries over the union and precedence terms
  test_reload                  a second load over a context whose url ids (and bitmaps) are built:
                               the newer file wins over what was loaded before
  test_big_list                840,000 rows: three pieces through the two staging buffers, every
                               piece edge inside a row; loaded, read back and dumped
  test_sharded_load_and_dump   world 2 and 4 on one GPU: every rank loads the same files, keeps
                               its url-hash range and dumps it; the dumps together are the index

tests/test_heap_cases_ref.py holds the CPU checks of the inputs and of the reference."""

import os
import sys

import numpy as np
import pytest

import dump_ref
import heap
import heap_cases as hc
import index_util as iu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOW = 20741 * 86400000 + 4242
STAT_KEYS = ("files", "records", "free_records", "bad_keys", "terms", "postings", "dropped_terms")
EMPTY = np.zeros((0, 40), np.uint8)


def _stats(st):
    return {k: getattr(st, k) for k in STAT_KEYS}


def _distinct(lists):
    return len({h for r in lists.values() for h in hc.keys(r)})


def _check_lists(ix, exp, absent=()):
    for t, rows in exp.items():
        assert ix.get_size(t) == len(rows), t
        assert ix.get_list(t).tobytes() == rows.tobytes(), t
    for t in absent:
        assert ix.get_size(t) == 0, t


def _check_queries(ix, lists, qs):
    exp = iu.oracle_hits(lists, qs)
    assert all(exp), "a query without hits checks nothing"
    assert iu.hits(ix, qs) == exp  # url hash, score and tiebreak


LOADS = {"union": hc.union_pairs, "precedence": hc.precedence, "tails": hc.unsorted_tails, "rejects": hc.rejects,
         "records": hc.records, "shard_input": hc.shard_input}


@pytest.mark.parametrize("by_name", [True, False], ids=["by_name", "oldest_first"])
@pytest.mark.parametrize("name", list(LOADS))
def test_cases_through_library(name, by_name, tmp_path):
    from yacy_search_server_amd import RWIIndex
    load = LOADS[name]()
    paths = hc.write_files(load, tmp_path)
    exp, st_exp, rep = heap.load_reference(paths, load.ram)
    if name == "rejects":
        assert sorted(rep["dropped"]) == sorted(load.info["causes"])
    ix = RWIIndex(0)
    try:
        for t, r in load.ram.items():
            ix.add(t, r)
        if by_name:
            given = paths[1::2] + paths[0::2][::-1]  # not oldest first
            st = ix.load_heaps(given, order_by_name=True)
        else:
            st = ix.load_heaps(paths)
        seen = {t for f in load.files if not isinstance(f, bytes) for t, _ in f} | set(load.info.get("absent", ()))
        _check_lists(ix, exp, absent=[t for t in seen if t not in exp])
        for t in rep["dropped"]:  # a dropped term keeps exactly its RAM rows
            assert ix.get_list(t).tobytes() == load.ram.get(t, EMPTY).tobytes(), t
        assert _stats(st) == st_exp
        assert ix.check_url_ids() == (0, _distinct(exp))
        assert ix.stats()[:2] == (len(exp), sum(len(r) for r in exp.values()))
        if name in ("union", "precedence"):
            terms = [t for _, t, _, _ in load.info["cases"]] if name == "union" else [hc.PREC, hc.PREC_MATE]
            _check_queries(ix, exp, hc.query_pairs(exp, terms))
    finally:
        ix.close()


@pytest.mark.parametrize("n", [300, 4200], ids=["plain", "bitmap"])
def test_reload(n, tmp_path):
    """lists loaded earlier are the RAM cache of the next load; the context's url dictionary, side
    arrays and (n = 4200: a list of more than 4,096 rows) bitmaps are built in between"""
    from yacy_search_server_amd import RWIIndex
    first, second = hc.reload(n)
    d1, d2 = tmp_path / "one", tmp_path / "two"
    d1.mkdir()
    d2.mkdir()
    p1, p2 = hc.write_files(first, d1), hc.write_files(second, d2)
    exp1, st1, _ = heap.load_reference(p1, first.ram)
    exp2, st2, rep2 = heap.load_reference(p2, exp1)
    assert rep2["dropped"] == {} and sorted(rep2["stored"]) == hc.REL
    ix = RWIIndex(0)
    try:
        for t, r in first.ram.items():
            ix.add(t, r)
        assert _stats(ix.load_heaps(p1)) == st1
        ix.build_url_ids()
        _check_lists(ix, exp1, absent=[hc.REL[2]])
        _check_queries(ix, exp1, hc.query_pairs(exp1, hc.REL[:2]))
        before = ix.index_info()
        if n >= 4096:
            assert before["bitmap_lists"] > 0, before
        assert _stats(ix.load_heaps(p2)) == st2
        _check_lists(ix, exp2)
        assert ix.check_url_ids() == (0, _distinct(exp2))
        after = ix.index_info()
        assert after["full_rebuilds"] + after["incremental_updates"] == \
            before["full_rebuilds"] + before["incremental_updates"] + 1, (before, after)
        assert ix.stats()[:2] == (3, sum(len(r) for r in exp2.values()))
        if n >= 4096:
            assert after["bitmap_lists"] > 0, after
        _check_queries(ix, exp2, hc.query_pairs(exp2, hc.REL))
    finally:
        ix.close()


def test_big_list(tmp_path):
    from yacy_search_server_amd import RWIIndex
    rows = hc.big_rows()
    (path,) = hc.write_files(hc.big_list(), tmp_path)
    ix = RWIIndex(0)
    try:
        st = ix.load_heaps([path])
        assert _stats(st) == {"files": 1, "records": 1, "free_records": 0, "bad_keys": 0, "terms": 1,
                              "postings": hc.BIG_ROWS, "dropped_terms": 0}
        assert ix.get_size(hc.BIG) == hc.BIG_ROWS
        assert ix.get_list(hc.BIG).tobytes() == rows.tobytes()
        out = str(tmp_path / "big.dump.blob")
        ds = ix.dump_heap(out, now_ms=NOW)
        with open(out, "rb") as f:
            image = f.read()
        assert (ds["terms"], ds["postings"], ds["bytes"]) == (1, hc.BIG_ROWS, len(image))
        assert image == dump_ref.expected_image({hc.BIG: rows}, now_ms=NOW)
    finally:
        ix.close()


# ------------------------------------------------------------------ sharded load and dump
def _rank_main(rank, world, uid, directory, out_q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import heap as hp
        import heap_cases as cases
        from yacy_search_server_amd import RWIIndex
        load = cases.shard_input()
        paths = [cases.path_of(directory, f) for f in range(len(load.files))]
        ram = {t: cases.shard_of(r, rank, world) for t, r in load.ram.items()}  # put_list does not shard
        exp, st_exp, _ = hp.load_reference(paths, ram, (rank, world))
        ix = RWIIndex(0, shard=(rank, world, uid))
        try:
            for t, r in ram.items():
                if len(r):
                    ix.add(t, r)
            st = ix.load_heaps(paths)
            bad = [t for t in cases.SH if ix.get_list(t).tobytes() != exp.get(t, EMPTY).tobytes()]
            if _stats(st) != st_exp:
                bad.append((_stats(st), st_exp))
            out = os.path.join(directory, "dump.%d.of.%d.blob" % (rank, world))
            ix.dump_heap(out, now_ms=NOW)
        finally:
            ix.close()
        out_q.put((rank, "ok", (bad, out)))
    except Exception as e:  # report, never hang the parent
        out_q.put((rank, "error", repr(e)))


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_load_and_dump(world, tmp_path, monkeypatch):
    import queue
    import time
    import torch.multiprocessing as mp
    # a rank that fails must not leave its peers waiting out the default 300 s
    monkeypatch.setenv("YRWI_HOSTX_TIMEOUT_S", "30")
    load = hc.shard_input()
    paths = hc.write_files(load, tmp_path)
    whole, _, _ = heap.load_reference(paths, load.ram)
    uid = b"YRWI-HOSTSTAGE\0" + os.urandom(113)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, world, uid, str(tmp_path), q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    deadline = time.time() + 90
    try:
        for _ in procs:
            res.append(q.get(timeout=max(1.0, deadline - time.time())))
    except queue.Empty:
        pass
    for p in procs:
        p.join(timeout=max(1.0, deadline + 10 - time.time()))
        if p.is_alive():
            p.kill()
    assert len(res) == world, ("ranks that never reported", res)
    dumps = {}
    for rank, status, info in res:
        assert status == "ok", (rank, info)
        bad, out = info
        assert bad == [], (rank, bad)
        dumps[rank] = out
    for rank in range(world):
        ram = {t: hc.shard_of(r, rank, world) for t, r in load.ram.items()}
        exp = heap.index_get(paths, ram, (rank, world))
        assert exp, rank
        with open(dumps[rank], "rb") as f:
            assert f.read() == dump_ref.expected_image(exp, now_ms=NOW), rank
    back = heap.index_get([dumps[r] for r in range(world)])
    assert {t: r.tobytes() for t, r in back.items()} == {t: r.tobytes() for t, r in whole.items()}
