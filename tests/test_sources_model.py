"""CPU: crdt_awset_sources_async restated with numpy (tests/sources_cases.py,
sources_ref), the expectation of tests/test_gpu_sources.py.

sources_ref is pinned here by the host builder the call replaces: the packed
source batch of P resident replicas equals SrcBatch.from_lists of each replica's
live documents, in every resident layout, and folds to the same result in both
fold modes (C oracle).  The entry point itself (header, library, bindings) is
checked for its arity, which fails on a tree without it.
"""

import os
import random
import re

import numpy as np
import pytest

import crdtgpu
from crdtgpu import CRDT_FOLD_AWSET, CRDT_FOLD_DELTA, abi
from helpers import PKG, ROOT, batch_of, out_doc, outs_equal
from oracle import oracle
from test_abi import _go_calls, _header_api
from sources_cases import (K_GATHER, K_PART, K_RUN, K_SCAN, LAYOUTS, host_built, make_replica, rand_docs,
                           rand_replicas, same_sources, sources_ref, tiny_replicas)


# ------------------------------------------------- 1. against the host builder

@pytest.mark.parametrize("R", [1, 3, 64])
@pytest.mark.parametrize("P", [1, 2, 3, 16])
def test_equals_the_host_builder(P, R):
    """Mixed layouts (rand_replicas): slack 0 and 3, counts given and NULL, stale
    non-zero slack, replica 1 without tombstones, scalar and per-document actors."""
    reps_docs, reps = rand_replicas(7000 + 17 * P + R, 120, P, R)
    ref = sources_ref(reps)
    want = host_built(R, reps_docs, reps)
    assert same_sources(ref.msg, want) and not ref.capacity
    assert ref.n_e == int(want.entry_off[-1]) and ref.n_t == int(want.tomb_off[-1])
    assert crdtgpu.validate_src(ref.msg) == 0
    assert ref.msg.doc_srcs.tolist() == [d * P for d in range(121)]
    if P > 1:  # replica 1 has no tombstones: its ranges are empty
        t = ref.msg.tomb_off
        assert (t[2::P][: 120] == t[1::P][: 120]).all() and int(t[-1]) > 0


@pytest.mark.parametrize("lay", range(len(LAYOUTS)))
def test_every_layout_alone(lay):
    rng = random.Random(7100 + lay)
    R = 3
    docs = rand_docs(rng, R, 200)
    kw = dict(LAYOUTS[lay])
    if kw.pop("garbage", False):
        kw["garbage"] = np.random.default_rng(lay)
    for lead in (0, 1):
        rep = make_replica(R, docs, actor=2, lead=lead, **kw)
        assert same_sources(sources_ref([rep]).msg, host_built(R, [docs], [rep]))
    if "garbage" in kw:  # the slack really holds stale values
        s = rep.state
        assert int(s.keys[int(s.offsets[0]) + int(s.counts[0])]) != 0


def test_vectorised_reference_handles_a_million_tiny_sources():
    import time

    reps = tiny_replicas(7200, (1 << 20) + 1, 1)
    t0 = time.perf_counter()
    ref = sources_ref(reps)
    assert time.perf_counter() - t0 < 5.0
    s = reps[0].state
    assert ref.msg.n_srcs == (1 << 20) + 1 and ref.n_e == int(s.counts.astype(np.int64).sum())
    assert (np.diff(ref.msg.entry_off.astype(np.int64)) == s.counts).all()


# --------------------------------------------------- 2. through the fold oracle

@pytest.mark.parametrize("mode", [CRDT_FOLD_AWSET, CRDT_FOLD_DELTA])
def test_folds_like_the_host_built_sources(mode):
    R, n, P = 4, 150, 3
    reps_docs, reps = rand_replicas(7300 + mode, n, P, R, max_e=10, max_t=3)
    rng = random.Random(7301)
    dst = batch_of(R, [(e, v) for e, _, v in rand_docs(rng, R, n)], slack=1)
    rc1, got = oracle.fold(mode, dst, sources_ref(reps).msg)
    rc2, want = oracle.fold(mode, dst, host_built(R, reps_docs, reps))
    assert rc1 == 0 and rc2 == 0
    assert outs_equal(got, want, n, R) is None
    assert sum(out_doc(want, d, R) != dst.doc(d) for d in range(n)) > n // 2  # the sources changed the documents


# ------------------------------------------------------------ 3. error paths

def test_count_above_slots_is_clamped():
    R = 2
    rng = random.Random(7400)
    docs = rand_docs(rng, R, 30, max_e=5, max_t=2)
    for which in ("entries", "tombstones"):
        rep = make_replica(R, docs, slack=1, garbage=np.random.default_rng(1))
        cols = rep.state if which == "entries" else rep.tombs
        d = 4
        slots = int(cols.offsets[d + 1]) - int(cols.offsets[d])
        cols.counts[d] = slots + 9
        ref = sources_ref([rep])
        assert ref.capacity
        off = ref.msg.entry_off if which == "entries" else ref.msg.tomb_off
        assert int(off[d + 1]) - int(off[d]) == slots  # the slack slot included, nothing of document 5
        k = ref.msg.keys if which == "entries" else ref.msg.tkeys
        assert int(k[int(off[d + 1]) - 1]) == int(cols.keys[int(cols.offsets[d + 1]) - 1])


def test_total_above_its_slots_writes_nothing_past_them():
    R = 2
    _, reps = rand_replicas(7500, 50, 2, R)
    full = sources_ref(reps)
    te, tt = int(full.msg.entry_off[-1]), int(full.msg.tomb_off[-1])
    assert te > 5 and tt > 5 and not full.capacity
    cut = sources_ref(reps, entry_slots=te - 1, tomb_slots=tt)
    assert cut.capacity and cut.n_e == te - 1 and cut.n_t == tt
    cut = sources_ref(reps, entry_slots=te, tomb_slots=tt - 3)
    assert cut.capacity and cut.n_e == te and cut.n_t == tt - 3
    assert same_sources(cut.msg, full.msg)  # the offsets are the whole scan's either way
    roomy = sources_ref(reps, entry_slots=te + 7, tomb_slots=tt)
    assert not roomy.capacity and roomy.n_e == te


# ------------------------------------------- 4. the entry point, in every layer

def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(abi.HEADER_PATH).read(), flags=re.S)


def test_header_library_and_bindings_have_the_entry_point():
    name = "crdt_awset_sources_async"
    assert name in crdtgpu.header_functions()
    assert getattr(abi.lib(), name) is not None  # exported by libcrdtgpu.so
    args = re.search(name + r"\s*\((.*?)\)\s*;", _header_text(), flags=re.S).group(1)
    assert len(args.split(",")) == 7
    restype, argtypes = abi.signatures()[name]
    assert len(argtypes) == 7
    go = open(os.path.join(ROOT, "go", "crdtgpu", "crdtgpu.go")).read()
    calls = dict(_go_calls(re.sub(r'//[^\n]*|"(?:[^"\\]|\\.)*"', "", go)))
    assert calls.get(name) == 7
    assert hasattr(crdtgpu.Engine, "sources_async") and hasattr(crdtgpu.Engine, "sources")
    assert hasattr(crdtgpu, "Replica") and crdtgpu.CRDT_MAX_REPLICAS == 16
    assert re.search(r"#define\s+CRDT_MAX_REPLICAS\s+16\b", _header_text())


def test_replica_struct_matches_the_header():
    import ctypes

    fields = _header_api()[1]["crdt_replica"]
    assert fields == [f for f, _ in abi.CReplica._fields_] == ["state", "tombs", "doc_actor", "actor"]
    assert ctypes.sizeof(abi.CReplica) == 32 and abi.CReplica.actor.offset == 24


def test_kernel_chunk_constants_are_the_ones_the_gpu_tests_mirror():
    src = open(os.path.join(PKG, "csrc", "sources.hip")).read()

    def const(name):
        expr = re.search(r"constexpr \w+ %s = ([^;]+);" % name, src).group(1)
        for _ in range(4):  # constants defined through earlier ones
            expr = re.sub(r"k\w+", lambda m: "(%s)" % re.search(r"constexpr \w+ %s = ([^;]+);" % m.group(0),
                                                                 src).group(1), expr)
        return eval(expr, {"__builtins__": {}})

    assert const("kSrcScanChunk") == K_SCAN and const("kSrcPartStep") == K_PART
    assert const("kSrcGatherChunk") == K_GATHER and const("kSrcRun") == K_RUN
