"""The hits' rows interface without a GPU: the ctypes prototypes of yrwi_query_rows,
yrwi_query_batch_rows and yrwi_query_batch_rows_submit as include/yrwi.h documents them,
and Hit's optional row."""

import ctypes
import os
import re

from yacy_search_server_amd import _lib
from yacy_search_server_amd.rwi import Hit, PendingBatch, RWIIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prototypes_match_the_header():
    text = open(os.path.join(ROOT, "include", "yrwi.h")).read()
    # each rows entry point takes its counterpart's arguments plus rows40_out right after `out`
    for name, old, nargs in (("yrwi_query_rows", "yrwi_query", 6), ("yrwi_query_batch_rows", "yrwi_query_batch", 8),
                             ("yrwi_query_batch_rows_submit", "yrwi_query_batch_submit", 9)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == nargs, (name, params)
        assert "uint8_t* rows40_out" in params
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
        _, old_args = _lib.SIGNATURES[old]
        at = params.index("uint8_t* rows40_out")
        assert params[at - 1].endswith("out") and args[at] is ctypes.c_void_p
        assert args[:at] + args[at + 1:] == old_args


def test_library_exports_the_entry_points():
    L = _lib.lib()  # resolves every symbol of SIGNATURES
    for name in ("yrwi_query_rows", "yrwi_query_batch_rows", "yrwi_query_batch_rows_submit"):
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]


def test_hit_without_row_is_todays_hit():
    h = Hit(b"AAAAAAAAAAAA", 17, -3)
    assert h.row is None
    assert h == Hit(urlhash=b"AAAAAAAAAAAA", score=17, tiebreak=-3)
    assert h == Hit(b"AAAAAAAAAAAA", 17, -3, None)
    assert h != Hit(b"AAAAAAAAAAAA", 17, -3, bytes(40))
    assert (h.urlhash, h.score, h.tiebreak) == (b"AAAAAAAAAAAA", 17, -3)


def test_python_keywords_default_to_no_rows():
    import inspect
    for fn in (RWIIndex.search, RWIIndex.search_batch, RWIIndex.submit):
        p = inspect.signature(fn).parameters["rows"]
        assert p.default is False
    assert inspect.signature(PendingBatch.__init__).parameters["rows"].default is None
    for fn in (RWIIndex.search_batch_rows_raw, RWIIndex.submit_rows_raw):
        assert list(inspect.signature(fn).parameters)[5] == "rows"
    hits = (_lib.CHit * 2)()
    hits[0].urlhash[:] = list(b"BBBBBBBBBBBB")
    hits[0].score, hits[0].tiebreak = 5, 6
    nout = (ctypes.c_int32 * 1)(1)
    assert RWIIndex._unmarshal(1, 2, hits, nout) == [[Hit(b"BBBBBBBBBBBB", 5, 6)]]
