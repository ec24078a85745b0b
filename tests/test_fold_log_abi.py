"""CPU: the logged fold's entry point exists in every layer: exported by
libcrdtgpu.so, declared in include/crdtgpu.h, bound in crdtgpu/abi.py with the
header's argument count, wrapped by Engine and by the Go binding; and the kernel
file calls the shared rule, walk and log pieces rather than copying them.
"""

import glob
import os
import re

import crdtgpu
from crdtgpu import abi
from helpers import PKG

NAME, N_ARGS = "crdt_awset_fold_log_async", 7
CSRC = os.path.join(PKG, "csrc")


def test_header_library_and_binding_have_the_entry_point():
    assert NAME in crdtgpu.header_functions()
    assert getattr(abi.lib(), NAME) is not None  # exported by libcrdtgpu.so
    header = re.sub(r"/\*.*?\*/", "", open(abi.HEADER_PATH).read(), flags=re.S)
    args = re.search(NAME + r"\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
    assert len(args.split(",")) == N_ARGS
    restype, argtypes = abi.signatures()[NAME]
    assert len(argtypes) == N_ARGS
    assert abi.lib().crdt_abi_version() == 1  # crdt_merge_log as it stands: no new struct


def test_engine_has_the_methods():
    for m in ("fold_log_async", "fold_log"):
        assert hasattr(crdtgpu.Engine, m), m


def test_go_binding_has_the_wrapper():
    go = open(os.path.join(PKG, "..", "go", "crdtgpu", "crdtgpu.go")).read()
    assert re.search(r"func \(\w+ \*?\w+\) FoldLog\(", go)
    assert "C.%s(" % NAME in go


def test_the_kernels_share_the_rule_the_walk_and_the_logs_pieces():
    log = open(os.path.join(CSRC, "fold_log.hip")).read()
    for call in ("decide(", "for_each_work(", "wave_lookup(", "wave_place(", "pair_wave_kind(", "log_flags(", "sums_add("):
        assert call in log, call
    # fold_block_kernel's step loop (block_merge< per step) lives in one header both files include
    shared = open(os.path.join(CSRC, "merge_block.hpp")).read()
    fold = open(os.path.join(CSRC, "fold.hip")).read()
    assert "block_merge<" in shared and "fold_block_doc(" in shared
    assert "fold_block_doc<" in log and "fold_block_doc<" in fold and "block_merge<" not in fold
    for piece in ("struct LogSums", "struct LogSink", "struct DiffSink", "uint32_t log_flags("):
        where = [os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(p)
                 and piece in open(p, errors="replace").read()]
        assert where == ["merge_log.hpp"], (piece, where)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for var in ("SRC", "RU_SRC"):
        assert re.search(r"^%s := .*\bfold_log\.hip\b" % var, mk, flags=re.M), var
