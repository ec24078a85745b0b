"""CPU: the worklist digest's entry point exists in every layer: exported by
libcrdtgpu.so, declared in include/crdtgpu.h with its two mode constants, bound
in crdtgpu/abi.py with the header's argument count, wrapped by Engine and by the
Go binding; its kernels are a translation unit of their own that leaves
digest.hip alone and shares the hash terms with it.
"""

import os
import re

import crdtgpu
from crdtgpu import abi
from helpers import PKG

NAME, N_ARGS = "crdt_awset_digest_idx_async", 10
CSRC = os.path.join(PKG, "csrc")


def test_header_library_and_binding_have_the_entry_point():
    assert NAME in crdtgpu.header_functions()
    assert getattr(abi.lib(), NAME) is not None  # exported by libcrdtgpu.so
    text = open(abi.HEADER_PATH).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = re.search(NAME + r"\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
    assert len(args.split(",")) == N_ARGS
    restype, argtypes = abi.signatures()[NAME]
    assert len(argtypes) == N_ARGS
    # the argument order of the header: ctx, state, tombs, idx, n_idx, n_max, n_digest_docs, mode, digest, stream
    names = [a.split()[-1].lstrip("*") for a in args.split(",")]
    assert names == ["ctx", "state", "tombs", "idx", "n_idx", "n_max", "n_digest_docs", "mode", "digest", "stream"]
    import ctypes

    assert [t is ctypes.c_uint32 for t in argtypes] == [False] * 5 + [True] * 3 + [False] * 2
    assert abi.lib().crdt_abi_version() == 1  # additive: no struct changed


def test_mode_constants_match_the_header():
    text = open(abi.HEADER_PATH).read()
    for name, value in (("CRDT_DIGEST_GATHER", 0), ("CRDT_DIGEST_PLACE", 1)):
        m = re.search(r"#define\s+%s\s+(\d+)u\b" % name, text)
        assert m and int(m.group(1)) == value, name
        assert getattr(abi, name) == value and getattr(crdtgpu, name) == value


def test_engine_has_the_methods():
    for m in ("digest_idx_async", "digest_idx"):
        assert hasattr(crdtgpu.Engine, m), m


def test_go_binding_has_the_wrapper():
    go = open(os.path.join(PKG, "..", "go", "crdtgpu", "crdtgpu.go")).read()
    assert re.search(r"func \(\w+ \*?\w+\) DigestIdx\(", go)
    assert "C.%s(" % NAME in go
    for const in ("CRDT_DIGEST_GATHER", "CRDT_DIGEST_PLACE"):
        assert "C.%s" % const in go


def test_the_kernels_are_their_own_translation_unit():
    src = open(os.path.join(CSRC, "digest_idx.hip")).read()
    assert '#include "digest_hash.hpp"' in src  # the definition as it stands
    for fn in ("dig_fmix", "dig_key", "dig_dot", "dig_clock"):
        assert fn + "(" in src and not re.search(r"uint64_t\s+%s\s*\(" % fn, src), fn
    assert "digest_idx" not in open(os.path.join(CSRC, "digest.hip")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for var in ("SRC", "RU_SRC"):
        assert re.search(r"^%s := .*\bdigest_idx\.hip\b" % var, mk, flags=re.M), var
    assert "check_digest_idx(" in open(os.path.join(CSRC, "api_args.hpp")).read()
    assert "check_digest_idx(" in open(os.path.join(CSRC, "api.cpp")).read()
