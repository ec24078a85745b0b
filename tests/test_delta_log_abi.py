"""CPU: the logged delta merge's entry points exist in every layer: exported by
libcrdtgpu.so, declared in include/crdtgpu.h, bound in crdtgpu/abi.py with the
header's argument counts, wrapped by Engine and by the Go binding; and the kernel
file shares the log's pieces with join_log.hip rather than copying them.
"""

import os
import re

import pytest

import crdtgpu
from crdtgpu import abi
from helpers import PKG

ENTRY_POINTS = [("crdt_awset_delta_join_log_async", 7), ("crdt_awset_delta_exchange_log_async", 10)]


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(abi.HEADER_PATH).read(), flags=re.S)


@pytest.mark.parametrize("name,n_args", ENTRY_POINTS)
def test_header_library_and_bindings_have_the_entry_points(name, n_args):
    assert name in crdtgpu.header_functions()
    assert getattr(abi.lib(), name) is not None  # exported by libcrdtgpu.so
    args = re.search(name + r"\s*\((.*?)\)\s*;", _header_text(), flags=re.S).group(1)
    assert len(args.split(",")) == n_args
    restype, argtypes = abi.signatures()[name]
    assert len(argtypes) == n_args


def test_engine_has_the_methods():
    for m in ("delta_join_log_async", "delta_exchange_log_async", "delta_exchange_log"):
        assert hasattr(crdtgpu.Engine, m), m


def test_go_binding_has_the_wrappers():
    go = open(os.path.join(PKG, "..", "go", "crdtgpu", "crdtgpu.go")).read()
    for fn, sym in (("DeltaJoin", "crdt_awset_delta_join_async"), ("DeltaExchange", "crdt_awset_delta_exchange_async"),
                    ("DeltaJoinLog", "crdt_awset_delta_join_log_async"),
                    ("DeltaExchangeLog", "crdt_awset_delta_exchange_log_async")):
        assert re.search(r"func \(\w+ \*?\w+\) %s\(" % fn, go), fn
        assert "C.%s(" % sym in go, sym


def test_the_kernels_share_the_logs_pieces():
    csrc = os.path.join(PKG, "csrc")
    log = open(os.path.join(csrc, "delta_pair_log.hip")).read()
    join = open(os.path.join(csrc, "join_log.hip")).read()
    shared = open(os.path.join(csrc, "merge_log.hpp")).read()
    for piece in ("struct LogSums", "struct LogSink", "void sums_add(", "void sums_flush(", "uint32_t log_flags("):
        assert piece in shared and piece not in log and piece not in join, piece
    # one rule, one walk: decide() and merge_walk are called, not restated
    assert "decide(" in log and "merge_walk<" in log and "for_each_work(" in log and "wave_place(" in log
    mk = open(os.path.join(csrc, "Makefile")).read()
    for var in ("SRC", "RU_SRC"):
        assert re.search(r"^%s := .*\bdelta_pair_log\.hip\b" % var, mk, flags=re.M), var
