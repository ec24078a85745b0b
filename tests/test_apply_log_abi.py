"""CPU: the logged local ops' entry point exists in every layer: exported by
libcrdtgpu.so, declared in include/crdtgpu.h, bound in crdtgpu/abi.py with the
header's argument count, wrapped by Engine and by the Go binding; the resolve of
the op lists exists once, in the header both kernel files include; and the logged
kernel file uses the shared log pieces rather than its own.
"""

import glob
import os
import re

import crdtgpu
from crdtgpu import abi
from helpers import PKG

NAME, N_ARGS = "crdt_awset_apply_log_async", 8
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
    for m in ("apply_log_async", "apply_log"):
        assert hasattr(crdtgpu.Engine, m), m


def test_go_binding_has_the_wrapper():
    go = open(os.path.join(PKG, "..", "go", "crdtgpu", "crdtgpu.go")).read()
    assert re.search(r"func \(\w+ \*?\w+\) ApplyLog\(", go)
    assert "C.%s(" % NAME in go


def test_the_resolve_exists_once_and_the_log_pieces_are_the_shared_ones():
    def where(piece):
        return sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(p)
                      and piece in open(p, errors="replace").read())

    for piece in ("struct ApplyWaveSmem", "scan_last_marked<EPL>(mk", "scan_last_marked<EPL>(hd", "flag_prefix<EPL>(rem"):
        assert where(piece) == ["apply_wave.hpp"], (piece, where(piece))
    plain = open(os.path.join(CSRC, "apply.hip")).read()
    log = open(os.path.join(CSRC, "apply_log.hip")).read()
    shared = open(os.path.join(CSRC, "apply_wave.hpp")).read()
    for text in (plain, log):
        assert '#include "apply_wave.hpp"' in text and "scan_last_marked<" not in text
    assert "apply_kernel<kApplyWaves, false>" in plain and "apply_kernel<kApplyWaves, true>" in log
    # the log's flags and summary go through merge_log.hpp's pieces, in the one kernel body
    assert '#include "merge_log.hpp"' in shared
    for call in ("log_flags(", "sums_add(", "sums_flush("):
        assert call in shared, call
    for call in ("launch_log_zero(", "launch_log_summary("):
        assert call in log, call
    for piece in ("struct LogSums", "uint32_t log_flags(", "void sums_add(", "void sums_flush("):
        assert where(piece) == ["merge_log.hpp"], (piece, where(piece))
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for var in ("SRC", "RU_SRC"):
        assert re.search(r"^%s := .*\bapply_log\.hip\b" % var, mk, flags=re.M), var
