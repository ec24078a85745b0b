"""CPU: the expectation of tests/test_gpu_delta_pair.py (tests/delta_pair_cases.py,
delta_pair_ref) and the conditions on its case sets.

delta_pair_ref is the C oracle's delta fold of one source per document.  It is
pinned here against the pure-Python restatement of the reference
(oracle/awset_ref.py, AWSetDelta.Merge), on reachable replicas (random
histories) and on the arbitrary states of the GPU case sets, so the kernels are
not checked against a single restatement.  The census shows that the case sets
hold every kind in each direction on each path, and the delta cases the contract
singles out; the entry points (header, library, bindings) are checked for their
arity, which fails on a tree without them.
"""

import os
import random
import re

import numpy as np
import pytest

import crdtgpu
from crdtgpu import CRDT_DELTA_DELTA, CRDT_DELTA_FULL, CRDT_DELTA_NONE, abi
from delta_pair_cases import (BLOCK_WINDOW, EDGE_SIZES, EDGE_TOMBS, FEATURES, KINDS, LOOP_ENTRIES, MAX_C, PAIR_WAVES,
                              WAVE_MAX, _doc_lists, census, delta_pair_ref, edge_pair, on_wave_path, phase2_doc,
                              random_pair, replica_of_ref)
from helpers import PKG, intern, out_doc, random_history, ref_entries, ref_state
from oracle import awset_ref as ref
from sources_cases import make_replica


def _merge_by_ref(dst_rep, src_rep, d):
    """AWSetDelta.Merge of document d through oracle/awset_ref.py: (entries, vv, kind)."""
    R = dst_rep.state.R
    de, dt, dv, da = _doc_lists(dst_rep, d)
    se, st, sv, sa = _doc_lists(src_rep, d)
    D = ref_state(de, dv, da, cls=ref.AWSetDelta, deleted=dt)
    S = ref_state(se, sv, sa, cls=ref.AWSetDelta, deleted=st)
    if D.VersionVector.Counter(S.Actor) <= 0:
        kind = CRDT_DELTA_FULL
    else:
        ch, dl = S.MakeDeltaMergeData(D.VersionVector)
        kind = CRDT_DELTA_NONE if ch is None and dl is None else CRDT_DELTA_DELTA
    D.Merge(S)
    return ref_entries(D), list(D.VersionVector) + [0] * (R - len(D.VersionVector)), kind


def _check_against_ref(a, b):
    want = delta_pair_ref(a, b)
    assert want.rc_ab == 0 and want.rc_ba == 0
    R = a.state.R
    for d in range(a.n_docs):
        e, vv, k = _merge_by_ref(a, b, d)
        assert out_doc(want.ab, d, R) == (e, vv), ("ab", d)
        assert int(want.kind_ab[d]) == k, ("kind ab", d)
        e, vv, k = _merge_by_ref(b, a, d)
        assert out_doc(want.ba, d, R) == (e, vv), ("ba", d)
        assert int(want.kind_ba[d]) == k, ("kind ba", d)
    return want


# ------------------------------------------- 1. against the pure-Python reference

def test_reachable_pairs_equal_the_python_reference():
    """300 random histories of three AWSetDelta replicas (Add, AWSetDelta.Del, Merge);
    document d is history d, replicas (x, y) of it.  Expected by the reference's own
    Merge on clones of the map states, not through the batch layout."""
    rng = random.Random(5100)
    R = 3
    hist = [random_history(rng, R, rng.randint(4, 40), 12, delta=True) for _ in range(300)]
    seen = set()
    for x, y in ((0, 1), (2, 0)):
        ids = intern([s for h in hist for s in h])
        a = replica_of_ref([h[x] for h in hist], ids, R, actor=x)
        b = replica_of_ref([h[y] for h in hist], ids, R, actor=y)
        want = delta_pair_ref(a, b)
        assert want.rc_ab == 0 and want.rc_ba == 0
        inv = {v: k for k, v in ids.items()}
        for d, h in enumerate(hist):
            for got, kinds, dst, src in ((want.ab, want.kind_ab, h[x], h[y]), (want.ba, want.kind_ba, h[y], h[x])):
                D = dst.Clone()
                before = list(D.VersionVector)
                D.Merge(src)
                e, vv = out_doc(got, d, R)
                assert sorted((inv[k], ac, c) for k, ac, c in e) == sorted(
                    (k, dot.actor, dot.counter) for k, dot in D.Entries.items()), d
                assert vv == list(D.VersionVector), d
                if int(kinds[d]) == CRDT_DELTA_NONE:
                    assert vv == before
                seen.add(int(kinds[d]))
    assert seen == set(KINDS)


@pytest.mark.parametrize("R", [1, 2, 5, 64])
def test_random_case_set_equals_the_python_reference(R):
    a, b = random_pair(5200 + R, 400, R)
    _check_against_ref(a, b)


def test_edge_case_set_equals_the_python_reference():
    da, db = edge_pair(big=False)
    a, b = make_replica(2, da, actor=0), make_replica(2, db, actor=1)
    _check_against_ref(a, b)


# ------------------------------------------------------------------ 2. census

def _assert_census(kinds, feats, paths):
    for path in paths:
        for direction in ("ab", "ba"):
            for k in KINDS:
                assert (path, direction, k) in kinds, (path, direction, k)
        for f in FEATURES:
            assert (path, f) in feats, (path, f)


def test_edge_cases_hold_every_kind_and_feature_on_both_paths():
    da, db = edge_pair()
    a, b = make_replica(2, da, actor=0), make_replica(2, db, actor=1)
    kinds, feats = census(a, b)
    _assert_census(kinds, feats, ("wave", "block"))
    assert a.n_docs % PAIR_WAVES != 0
    sizes = {(len(x[0]), len(y[0])) for x, y in zip(da, db)}
    assert {(p, q) for p in EDGE_SIZES for q in EDGE_SIZES} <= sizes
    tombs = {(len(x[1]), len(y[1])) for x, y in zip(da, db) if len(x[0]) <= WAVE_MAX and len(y[0]) <= WAVE_MAX}
    assert {(p, q) for p in EDGE_TOMBS for q in EDGE_TOMBS} <= tombs  # tombstones alone change the path
    assert sum(not on_wave_path(a, b, d) for d in range(a.n_docs)) > 100
    assert 2 * LOOP_ENTRIES - 77 > 2 * BLOCK_WINDOW  # the big documents step the block path's window
    assert max(len(x[0]) for x in da) == LOOP_ENTRIES


@pytest.mark.parametrize("R", [1, 2, 5, 64])
def test_random_cases_hold_every_kind_and_feature(R):
    a, b = random_pair(6000 + R, 3000, R)  # the seed and size tests/test_gpu_delta_pair.py uses
    kinds, feats = census(a, b)
    need = [f for f in FEATURES if not (R == 1 and f == "none_src_ahead")]  # one component: the clocks are equal
    for direction in ("ab", "ba"):
        for k in KINDS:
            assert ("wave", direction, k) in kinds, (direction, k)
    for f in need:
        assert ("wave", f) in feats, f
    assert all(on_wave_path(a, b, d) for d in range(a.n_docs))


def test_phase2_document_does_what_it_says():
    for R in (1, 2, 5):
        x, y = phase2_doc(R)
        a, b = make_replica(R, [x], actor=0), make_replica(R, [y], actor=1 % R)
        want = _check_against_ref(a, b)
        assert int(want.kind_ab[0]) == CRDT_DELTA_DELTA and int(want.kind_ba[0]) == CRDT_DELTA_NONE
        e, vv = out_doc(want.ab, 0, R)
        assert [k for k, _, _ in e] == [10, 70] and (70, 1 % R, 6) in e  # 40 added, then removed; 70 updated
        assert vv == [8] * R
        assert out_doc(want.ba, 0, R) == (y[0], y[2])


def test_none_keeps_the_destination_clock():
    """A NONE document whose src clock is ahead: the output clock is dst's (the oracle's
    delta step returns before its clock merge)."""
    R = 2
    a, b = random_pair(6002, 3000, R)
    want = delta_pair_ref(a, b)
    n = 0
    for d in range(a.n_docs):
        _, _, va, _ = _doc_lists(a, d)
        _, _, vb, _ = _doc_lists(b, d)
        if int(want.kind_ab[d]) == CRDT_DELTA_NONE and any(s > v for s, v in zip(vb, va)):
            assert out_doc(want.ab, d, R) == (a.state.doc(d)[0], va)
            n += 1
    assert n > 50


def test_counters_fit_the_counter_maps():
    a, b = random_pair(6005, 500, 5)
    for r in (a, b):
        assert int(r.state.counters.max()) <= MAX_C and int(r.state.vv.max()) <= MAX_C
        assert int(r.tombs.counters.max()) <= MAX_C


# ---------------------------------------------------------- 3. dispatch constants

def test_dispatch_constants_are_the_ones_the_case_sets_mirror():
    src = open(os.path.join(PKG, "csrc", "delta_pair.hip")).read()

    def const(name):
        return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))

    assert const("kPairWaveMax") == WAVE_MAX and const("kPairWaves") == PAIR_WAVES
    assert const("kPairBlockNT") * const("kPairBlockIPT") == BLOCK_WINDOW
    # one rule: the kernels call merge_block.hpp's decide, they do not restate it
    assert "decide(" in src and "block_merge<" in src


# ------------------------------------------- 4. the entry points, in every layer

def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(abi.HEADER_PATH).read(), flags=re.S)


@pytest.mark.parametrize("name,n_args", [("crdt_awset_delta_join_async", 6), ("crdt_awset_delta_exchange_async", 8)])
def test_header_library_and_bindings_have_the_entry_points(name, n_args):
    assert name in crdtgpu.header_functions()
    assert getattr(abi.lib(), name) is not None  # exported by libcrdtgpu.so
    args = re.search(name + r"\s*\((.*?)\)\s*;", _header_text(), flags=re.S).group(1)
    assert len(args.split(",")) == n_args
    restype, argtypes = abi.signatures()[name]
    assert len(argtypes) == n_args


def test_engine_has_the_methods():
    for m in ("delta_join_async", "delta_exchange_async", "delta_exchange"):
        assert hasattr(crdtgpu.Engine, m), m
    text = open(abi.HEADER_PATH).read()
    assert "crdt_awset_delta_join_async / crdt_awset_delta_exchange_async" in text  # the list of replaced methods
