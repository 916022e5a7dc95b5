"""tests/index_util.py without a GPU: same_lists on a stub index, run_parts over stub contexts (the
threads, the per-rank errors and the closing of what was opened)."""

import numpy as np
import pytest

import index_util as iu

A, B, GONE = b"TERMstubA___", b"TERMstubB___", b"TERMstubGone"


class StubIndex:
    def __init__(self, lists):
        self.lists = dict(lists)

    def get_size(self, t):
        return len(self.lists.get(t, iu.EMPTY))

    def get_list(self, t):
        return self.lists.get(t, iu.EMPTY)


def _lists():
    rng = np.random.default_rng(1)
    return {A: rng.integers(0, 256, (5, 40)).astype(np.uint8), B: rng.integers(0, 256, (3, 40)).astype(np.uint8)}


def test_same_lists_passes_on_equal_input():
    lists = _lists()
    iu.same_lists(StubIndex(lists), lists, [A, B, GONE])  # GONE: empty on both sides


def test_same_lists_sees_a_flipped_byte():
    lists = _lists()
    held = {t: r.copy() for t, r in lists.items()}
    held[B][2, 39] ^= 1
    iu.same_lists(StubIndex(held), lists, [A])
    with pytest.raises(AssertionError, match="TERMstubB"):
        iu.same_lists(StubIndex(held), lists, [A, B])


def test_same_lists_sees_a_missing_row():
    lists = _lists()
    held = {**lists, A: lists[A][:-1]}
    with pytest.raises(AssertionError, match="TERMstubA.*4, 5"):
        iu.same_lists(StubIndex(held), lists, [B, A])


def test_same_lists_sees_rows_the_reference_has_not():
    lists = _lists()
    held = {**lists, GONE: lists[B][:1]}
    with pytest.raises(AssertionError, match="TERMstubGone.*1, 0"):
        iu.same_lists(StubIndex(held), lists, [GONE])


class StubContext:
    def __init__(self, rank, log):
        self.rank, self.added, self.log = rank, [], log
        log["opened"] += 1

    def add(self, h, rows):
        self.added.append(h)

    def close(self):
        self.log["closed"] += 1


def _opener(log, fail_on=None):
    def open_rank(r, world, uid):
        assert world == 3 and len(uid) == 128
        if r == fail_on:
            raise RuntimeError("no context for rank %d" % r)
        return StubContext(r, log)
    return open_rank


PARTS = [{A: None}, {}, {A: None, B: None}]


def test_run_parts_returns_results_in_rank_order():
    log = {"opened": 0, "closed": 0}
    out = iu.run_parts(PARTS, 3, lambda r, ix: (r, ix.rank, ix.added), open_rank=_opener(log))
    assert out == [(0, 0, [A]), (1, 1, []), (2, 2, [A, B])]
    assert log == {"opened": 3, "closed": 3}


def test_run_parts_reports_the_rank_that_raised():
    log = {"opened": 0, "closed": 0}

    def fn(r, ix):
        if r == 1:
            raise ValueError("rank one is unwell")
        return r

    with pytest.raises(AssertionError, match=r"1, 'running', .*rank one is unwell"):
        iu.run_parts(PARTS, 3, fn, open_rank=_opener(log))
    assert log == {"opened": 3, "closed": 3}


def test_run_parts_reports_a_rank_that_did_not_open():
    log = {"opened": 0, "closed": 0}
    ran = []
    with pytest.raises(AssertionError, match=r"2, 'opening', .*no context for rank 2"):
        iu.run_parts(PARTS, 3, lambda r, ix: ran.append(r), open_rank=_opener(log, fail_on=2))
    assert log == {"opened": 2, "closed": 2} and ran == []
