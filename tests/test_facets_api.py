"""Host facets (yrwi_host_facets_batch), the part that runs without a GPU: the library exports the
entry point, the ctypes mirror has the header's layout, the Python class carries the call, and
the argument errors that need no device are answered."""

import ctypes
import os
import re

import numpy as np

from yacy_search_server_amd import _lib, rwi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "yrwi.h")


def test_symbol_and_argtypes():
    L = _lib.lib()
    assert hasattr(L, "yrwi_host_facets_batch") and "yrwi_host_facets_batch" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["yrwi_host_facets_batch"]
    assert res is ctypes.c_int and len(args) == 13
    assert args[2:5] == [ctypes.c_int32] * 3 and args[8] is ctypes.c_int64
    assert args[12] == ctypes.POINTER(_lib.CFacetStats)
    assert callable(getattr(rwi.RWIIndex, "host_facets_batch", None))
    assert callable(getattr(rwi.RWIIndex, "host_facets_batch_raw", None))
    assert _lib.FACETS_ORDERS == {"host": 0, "count": 1}


def test_struct_layout():
    S = _lib.CFacetStats
    # nine int64 and two int32 (include/yrwi.h): 6 * 8, 2 * 4, 3 * 8
    assert ctypes.sizeof(S) == 80
    assert S.hosts.offset == 16 and S.bytes_d2h.offset == 40 and S.launches_tail.offset == 48
    assert S.syncs.offset == 52 and S.device_allocs.offset == 56 and S.t_total_ns.offset == 72


def test_header_declares_the_call():
    src = open(HEADER).read()
    assert re.search(r"#define\s+YRWI_FACETS_BY_HOST\s+0\b", src)
    assert re.search(r"#define\s+YRWI_FACETS_BY_COUNT\s+1\b", src)
    assert re.search(r"\bint\s+yrwi_host_facets_batch\s*\(\s*yrwi_ctx\s*\*", src)
    m = re.search(r"typedef struct yrwi_facet_stats \{(.*?)\} yrwi_facet_stats;", src, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [(t, [n.strip() for n in names.split(",")]) for t, names in re.findall(r"(int64_t|int32_t)\s+([^;]+);", body)]
    flat = [(n, ctypes.c_int64 if t == "int64_t" else ctypes.c_int32) for t, ns in fields for n in ns]
    assert flat == [(n, t) for n, t in _lib.CFacetStats._fields_]


def test_null_arguments():
    L = _lib.lib()
    st = _lib.CFacetStats()
    st.syncs = 7
    off = np.full(2, -5, dtype=np.int64)
    E_ARG = -1
    assert L.yrwi_host_facets_batch(None, None, 1, 0, 0, None, None, None, 0, off.ctypes.data, None, None,
                                    ctypes.byref(st)) == E_ARG
    assert st.syncs == 0 and (off == -5).all()  # the statistics are cleared even then
    assert L.yrwi_host_facets_batch(None, None, 0, 0, 0, None, None, None, 0, off.ctypes.data, None, None,
                                    None) == E_ARG
