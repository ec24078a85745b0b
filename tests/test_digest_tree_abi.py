"""CPU: the digest tree's entry points exist in every layer: exported by
libcrdtgpu.so, declared in include/crdtgpu.h with the fan-out constant, bound in
crdtgpu/abi.py with the header's argument counts, wrapped by Engine and by the Go
binding; the kernels are a translation unit of their own that leaves digest.hip,
digest_idx.hip and compare.hip alone and takes its terms from digest_hash.hpp, the
one place K_P is written down.
"""

import ctypes
import os
import re

import crdtgpu
from crdtgpu import abi
from helpers import PKG

CSRC = os.path.join(PKG, "csrc")
ENTRY = {
    "crdt_digest_tree_layout": ["n_docs", "level_nodes", "level_off"],
    "crdt_digest_tree_host": ["digest", "n_docs", "tree"],
    "crdt_digest_tree_async": ["ctx", "digest", "n_docs", "tree", "stream"],
    "crdt_digest_tree_children_async": ["ctx", "level", "n_level", "parents", "n_parents", "n_max", "out", "stream"],
    "crdt_digest_tree_diff_async": ["ctx", "mine_level", "n_level", "theirs", "parents", "n_parents", "n_max", "leaf",
                                    "mask", "idx_out", "flags_out", "n_out", "out_max", "summary", "stream"],
}
U32_ARGS = {"n_docs", "n_level", "n_max", "leaf", "mask", "out_max"}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(abi.HEADER_PATH).read(), flags=re.S)


def test_header_library_and_binding_have_the_entry_points():
    header = _header()
    for name, want in ENTRY.items():
        assert name in crdtgpu.header_functions(), name
        assert getattr(abi.lib(), name) is not None, name  # exported by libcrdtgpu.so
        args = re.search(name + r"\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
        names = [re.sub(r"\[\d+\]", "", a.split()[-1]).lstrip("*") for a in args.split(",")]
        assert names == want, name
        restype, argtypes = abi.signatures()[name]
        assert restype is ctypes.c_int and len(argtypes) == len(want), name
        assert [t is ctypes.c_uint32 for t in argtypes] == [a in U32_ARGS for a in want], name
    assert abi.lib().crdt_abi_version() == 1  # additive: no struct changed


def test_fanout_constant_matches_the_header():
    m = re.search(r"#define\s+CRDT_DIGEST_TREE_FANOUT\s+(\d+)u\b", open(abi.HEADER_PATH).read())
    assert m and int(m.group(1)) == 16
    assert abi.CRDT_DIGEST_TREE_FANOUT == 16 and crdtgpu.CRDT_DIGEST_TREE_FANOUT == 16
    assert re.search(r"kDigTreeFanout = 16;", open(os.path.join(CSRC, "digest_hash.hpp")).read())


def test_engine_and_package_have_the_methods():
    for m in ("digest_tree_async", "digest_tree", "digest_tree_children_async", "digest_tree_diff_async",
              "digest_tree_descend"):
        assert hasattr(crdtgpu.Engine, m), m
    for f in ("digest_tree_host", "digest_tree_layout", "DigestTreeBuffers"):
        assert hasattr(crdtgpu, f), f
    t = crdtgpu.DigestTreeBuffers(4097, cap=100)
    assert (t.L, t.nodes[:5], t.off[1:5], t.n_nodes) == (4, [4097, 257, 17, 2, 1], [0, 257, 274, 276], 277)
    assert t.tree.shape == (554,) and t.packed.shape == (3200,) and t.idx[0].shape == (100,)
    assert t.level(2, None)[0].shape == (34,) and t.level(2, None)[1] == 17
    # buffers without a descent's lists are refused by the driver, with 0 docs too (before any device call)
    import pytest

    for n in (4097, 0):
        with pytest.raises(ValueError, match="cap"):
            crdtgpu.Engine.digest_tree_descend(None, None, crdtgpu.DigestTreeBuffers(n), None)


def test_go_binding_has_the_wrappers():
    go = open(os.path.join(PKG, "..", "go", "crdtgpu", "crdtgpu.go")).read()
    for fn, c in (("DigestTree", "crdt_digest_tree_async"), ("DigestTreeChildren", "crdt_digest_tree_children_async"),
                  ("DigestTreeDiff", "crdt_digest_tree_diff_async")):
        assert re.search(r"func \(\w+ \*?\w+\) %s\(" % fn, go), fn
        assert "C.%s(" % c in go, c
    assert "C.crdt_digest_tree_layout(" in go and "C.crdt_digest_tree_host(" in go
    assert "C.CRDT_DIGEST_TREE_FANOUT" in go


def test_the_kernels_are_their_own_translation_unit():
    src = open(os.path.join(CSRC, "digest_tree.hip")).read()
    assert '#include "digest_hash.hpp"' in src  # the definition as it stands
    for fn in ("dig_tree_term", "dig_tree_node", "dig_tree_layout"):
        assert fn + "(" in src and not re.search(r"\b%s\s*\([^)]*\)\s*\{" % fn, src), fn
    for other in ("digest.hip", "digest_idx.hip", "compare.hip"):
        assert "tree" not in open(os.path.join(CSRC, other)).read().lower(), other
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for var in ("SRC", "RU_SRC"):
        assert re.search(r"^%s := .*\bdigest_tree\.hip\b" % var, mk, flags=re.M), var
    args, api = (open(os.path.join(CSRC, f)).read() for f in ("api_args.hpp", "api.cpp"))
    for check in ("check_digest_tree(", "check_digest_tree_children(", "check_digest_tree_diff("):
        assert check in args and check in api, check


def test_k_p_is_written_down_once():
    hits = []
    for f in sorted(os.listdir(CSRC)):
        p = os.path.join(CSRC, f)
        if os.path.isfile(p) and f.endswith((".hip", ".hpp", ".cpp", ".h")):
            hits += [f] * len(re.findall(r"2545F4914F6CDD1D", open(p, errors="replace").read(), flags=re.I))
    assert hits == ["digest_hash.hpp"]
    assert "0x2545F4914F6CDD1D" in open(abi.HEADER_PATH).read()  # the ABI's statement of it
