"""The heap dump on the device (yrwi_dump_heap): the file equals the reference writer's bytes
(tests/dump_ref.py over oracle/heap.py) whatever the window size, loads back into an equal
index, follows the update path's changes, honours a term selection, lands atomically, and
costs launches and waits by the bytes, not by the number of terms."""

import os

import numpy as np
import pytest

import dump_ref as dr
import heap
import index_util as iu
import update_ref as ur
from yacy_search_server_amd import RWIIndex, _lib, synth
from yacy_search_server_amd._lib import YrwiError

pytestmark = pytest.mark.gpu

NOW = iu.NOW


@pytest.fixture(scope="module")
def tiny():
    cfg = synth.preset("tiny")
    idx = synth.build_index(cfg)
    lists = idx.as_dict()
    qs = [([idx.hashes[t] for t in inc], [idx.hashes[t] for t in exc]) for inc, exc in synth.queries(cfg, 40, 2, 3, 1)]
    return cfg, idx, lists, qs


@pytest.fixture(scope="module")
def hand(tiny):
    """the hand-made lists (dump_ref.SIZES) on the device, and their expected image"""
    lists = dr.fixture_lists(tiny[1])
    ix = iu.open_index(lists)
    yield ix, lists, dr.expected_image(lists, now_ms=NOW)
    ix.close()


def _dump(ix, path, terms=None, window=None, monkeypatch=None):
    if monkeypatch is not None:
        if window is None:
            monkeypatch.delenv("YRWI_DUMP_WINDOW", raising=False)
        else:
            monkeypatch.setenv("YRWI_DUMP_WINDOW", str(window))
    st = ix.dump_heap(str(path), terms, now_ms=NOW)
    assert not os.path.exists(str(path) + ".prt")
    with open(path, "rb") as f:
        return f.read(), st


# ------------------------------------------------------------------ 1: the image is exact
def test_image_is_exact(hand, tmp_path, monkeypatch):
    ix, lists, image = hand
    # preconditions (CPU, from the expected image): every kind of window boundary at W = 256,
    # every even misalignment between the 256-B aligned rows and their place in the file
    assert dr.boundary_classes(image, 256) == dr.BOUNDARY_CLASSES
    assert dr.row_area_residues(image) == {0, 2, 4, 6, 8, 10, 12, 14}
    got, st = _dump(ix, tmp_path / "a.blob", window=256, monkeypatch=monkeypatch)
    assert len(got) == len(image)
    assert got == image
    assert (st["terms"], st["postings"], st["bytes"]) == (len(lists), sum(dr.SIZES), len(image))


# ------------------------------------------------------------------ 2: window independence
def test_window_independence(hand, tmp_path, monkeypatch):
    ix, lists, image = hand
    for w in (256, 4096, 4096 + 256, None):
        got, st = _dump(ix, tmp_path / f"w{w}.blob", window=w, monkeypatch=monkeypatch)
        assert got == image, w
        eff = w or _lib.DUMP_WINDOW_DEFAULT
        assert st["windows"] == -(-len(image) // eff), (w, st)


# ------------------------------------------------------------------ 3: round trip
def test_round_trip(tiny, tmp_path):
    cfg, idx, lists, qs = tiny
    src = iu.open_index(lists)
    back = RWIIndex(0)
    try:
        before = iu.hits(src, qs)
        path = tmp_path / "tiny.blob"
        got, st = _dump(src, path)
        assert got == dr.expected_image(lists, now_ms=NOW)
        ls = back.load_heaps([str(path)])
        assert (ls.terms, ls.postings) == (st["terms"], st["postings"]) == (len(lists), sum(map(len, lists.values())))
        for t in lists:
            assert back.get_list(t).tobytes() == src.get_list(t).tobytes(), t
        assert back.stats()[:2] == src.stats()[:2]
        assert back.check_url_ids()[0] == 0
        assert iu.hits(back, qs) == before == iu.oracle_hits(lists, qs)
        # the dump changed nothing in the source context
        assert src.check_url_ids()[0] == 0
        assert iu.hits(src, qs) == before
    finally:
        src.close()
        back.close()


# ------------------------------------------------------------------ 4: after updates
def test_after_updates(tiny, tmp_path, monkeypatch):
    cfg, idx, lists, qs = tiny
    a, b, c, d = sorted(lists, key=lambda h: -len(lists[h]))[:4]
    cur = {h: lists[h] for h in (a, b, c, d)}
    new_term = iu.term(9)
    ix = iu.open_index(cur)
    try:
        ix.build_url_ids()

        def step(cur, k):
            # a new term, a replaced row and a new url; then a list emptied
            terms = [new_term, a, b]
            rows = iu.rows(idx, [iu.url(700 + k), bytes(cur[a][5, :12]), iu.url(800 + k)], start=k)
            cur, st = iu.checked_add(ix, cur, terms, rows)
            assert st["replaced"] == 1 and st["added"] == 2
            cur, st = iu.checked_remove(ix, cur, [bytes(r[:12]) for r in cur[new_term]], [new_term])
            assert st["emptied_terms"] == 1
            return cur

        def check(cur, name):
            got, st = _dump(ix, tmp_path / name)
            assert got == dr.expected_image(cur, now_ms=NOW)
            # the emptied term has no record, and no dead copy of a re-written list appears
            assert [got[o + 4:o + 16] for o, _ in dr.layout(got)] == sorted(cur, key=heap.key_order)
            assert new_term not in cur and st["terms"] == len(cur) == 4
            assert ix.check_url_ids()[0] == 0

        cur = step(cur, 0)
        check(cur, "u0.blob")
        # again, with the index memory repacked in between
        monkeypatch.setenv("YRWI_REPACK_MIN_MB", "0.05")
        first = ix.index_info()
        for i in range(16):
            cur, _ = iu.checked_add(ix, cur, [a] * 3, iu.rows(idx, [iu.url(1000 + 3 * i + k) for k in range(3)], start=i))
            ix.build_url_ids()
        assert ix.index_info()["repacks"] > first["repacks"], ix.index_info()
        cur = step(cur, 1)
        check(cur, "u1.blob")
    finally:
        ix.close()


# ------------------------------------------------------------------ 5: selection
def test_selection(hand, tmp_path, monkeypatch):
    ix, lists, image = hand
    some = sorted(lists, key=heap.key_order)[5:120:9]
    sel = list(reversed(some)) + [some[2], iu.term(3)]  # out of order, one twice, one unknown
    got, st = _dump(ix, tmp_path / "s.blob", terms=sel, window=4096, monkeypatch=monkeypatch)
    assert got == dr.expected_image(lists, sel, now_ms=NOW)
    assert [got[o + 4:o + 16] for o, _ in dr.layout(got)] == some
    assert st["terms"] == len(some) and st["postings"] == sum(len(lists[t]) for t in some)
    # only unknown terms: an empty selection, a 0-byte file
    got, st = _dump(ix, tmp_path / "none.blob", terms=[iu.term(3)])
    assert got == b"" and st["windows"] == 0
    bad = tmp_path / "bad.blob"
    with pytest.raises(YrwiError) as e:
        ix.dump_heap(str(bad), some[:3] + [b"bad!term#ash"], now_ms=NOW)
    assert e.value.rc == -2
    assert not bad.exists() and not os.path.exists(str(bad) + ".prt")


# ------------------------------------------------------------------ 6: files
def test_files(hand, tmp_path):
    ix, lists, image = hand
    old = tmp_path / "old.blob"
    old.write_bytes(b"old bytes")
    # a missing directory
    missing = tmp_path / "nodir" / "x.blob"
    with pytest.raises(YrwiError) as e:
        ix.dump_heap(str(missing), now_ms=NOW)
    assert e.value.rc == _lib.E_IO and "nodir" in str(e.value)
    assert not (tmp_path / "nodir").exists()
    assert old.read_bytes() == b"old bytes" and [p.name for p in tmp_path.iterdir()] == ["old.blob"]
    # failures onto an existing file leave it alone and no temporary file behind
    blocker = tmp_path / "old.blob.prt"
    blocker.mkdir()  # the temporary file cannot be created
    with pytest.raises(YrwiError) as e:
        ix.dump_heap(str(old), now_ms=NOW)
    assert e.value.rc == _lib.E_IO
    assert old.read_bytes() == b"old bytes" and blocker.is_dir()
    blocker.rmdir()
    with pytest.raises(YrwiError) as e:
        ix.dump_heap(str(old), [b"bad!term#ash"], now_ms=NOW)
    assert e.value.rc == -2
    assert old.read_bytes() == b"old bytes" and not blocker.exists()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["old.blob"]
    # a successful dump replaces it
    got, _ = _dump(ix, old)
    assert got == image
    # an index without lists: a 0-byte file, also over an existing one
    empty = RWIIndex(0)
    try:
        got, st = _dump(empty, old)
        assert got == b"" and (st["terms"], st["bytes"], st["windows"]) == (0, 0, 0)
    finally:
        empty.close()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["old.blob"]


# ------------------------------------------------------------------ 7: cost does not follow the term count
def test_cost_does_not_follow_term_count(tiny, tmp_path, monkeypatch):
    cfg, idx, lists, qs = tiny
    one = {iu.term(1): iu.rows(idx, [iu.url(k) for k in range(1000)])}
    many = {iu.term(100 + i): iu.rows(idx, [iu.url(k) for k in range(3)], start=i) for i in range(250)}
    ix = iu.open_index({**one, **many})
    try:
        a, sa = _dump(ix, tmp_path / "one.blob", terms=list(one), window=4096, monkeypatch=monkeypatch)
        b, sb = _dump(ix, tmp_path / "many.blob", terms=list(many), window=4096, monkeypatch=monkeypatch)
        assert (len(a), len(b)) == (40030, 37500)
        assert a == dr.expected_image(one, now_ms=NOW) and b == dr.expected_image(many, now_ms=NOW)
        assert sa["windows"] == sb["windows"] == 10
        assert (sa["launches"], sa["syncs"]) == (sb["launches"], sb["syncs"]), (sa, sb)
        assert (sa["terms"], sb["terms"]) == (1, 250)
    finally:
        ix.close()
