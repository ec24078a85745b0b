"""CPU: the order-preserving counter maps of tests/counter_maps.py and the
metamorphic property the wide-counter GPU tests rest on,

    oracle(f(x)) == f(oracle(x))    bit for bit, error verdicts included,

shown on the oracles themselves: the C oracle's join, both fold modes (panic
documents included), the delta-extraction restatement and the tombstone GC,
over a few hundred random documents each, every batch mixing all six maps.
The cases come from the generators the GPU tests use.
"""

import random

import numpy as np
import pytest

import counter_maps as cm
import test_delta_extract_model as model
from counter_maps import C, MAPS, TOP
from crdtgpu import CRDT_FOLD_AWSET, CRDT_FOLD_DELTA
from crdtgpu.batch import TombBatch
from helpers import batch_of, src_batch_of
from oracle import oracle
from test_gpu_delta_extract import expected, parity_case
from test_gpu_gc import gc_case
from test_gpu_parity import PANIC_R, assert_same_all, fold_case, join_case, panic_cases

U64 = np.uint64


# ---------------------------------------------------------------- the tables

def test_tables_strictly_increasing_from_zero():
    assert [m.name for m in MAPS] == ["hi_only", "across_2_32", "across_2_31", "across_2_63", "top", "scattered"]
    for m in MAPS:
        t = [int(x) for x in m.table]
        assert len(t) == C + 1 and m.table.dtype == U64
        assert t[0] == 0 and t[1] > 0
        assert all(a < b for a, b in zip(t, t[1:])), m.name
        assert t[-1] <= TOP and t[-1] >= m.edge
    t = {m.name: [int(x) for x in m.table] for m in MAPS}
    assert all(x & 0xFFFFFFFF == 0 for x in t["hi_only"])
    assert t["across_2_32"][32] == (1 << 32) and t["across_2_31"][32] == (1 << 31)
    assert t["across_2_63"][32] == (1 << 63) and t["top"][C] == TOP
    assert t["across_2_31"][C] < (1 << 32)  # (by construction no high word: its edge is bit 31)
    lo = [x & 0xFFFFFFFF for x in t["scattered"][1:]]
    hi = [x >> 32 for x in t["scattered"][1:]]
    assert lo != sorted(lo) and len(set(hi)) == C and all(hi)  # the low halves alone do not carry the order


@pytest.mark.parametrize("max_c", [6, 8, 9, 12, 20, 40, 50, 64])
def test_stretch_keeps_order_and_reaches_both_sides(max_c):
    for m in MAPS:
        t = [int(x) for x in cm.stretch(m, max_c)]
        assert len(t) == max_c + 1 and t[0] == 0 and t[-1] == int(m.table[-1])
        assert all(a < b for a, b in zip(t, t[1:]))
        assert t[1] < m.edge or not m.name.startswith("across")
    assert cm.stretch(MAPS[0], max_c) is cm.stretch(MAPS[0], max_c)


def test_appliers_leave_everything_but_counters_alone():
    rng = random.Random(1)
    R = 3
    dst, _ = join_case(rng, 60, R, lambda: rng.randint(0, 9), 40, 9)
    tod = cm.mixed(9)
    m = cm.map_batch(dst, tod)
    assert m.offsets is dst.offsets and m.keys is dst.keys and m.actors is dst.actors and m.counts is dst.counts
    for d in range(dst.n_docs):
        t = tod(d)
        e, vv = dst.doc(d)
        assert m.doc(d) == (cm.map_entries(e, t), cm.map_clock(vv, t))
    # slack slots (beyond a document's count) are not entries and stay as they are
    docs = [dst.doc(d) for d in range(dst.n_docs)]
    sl = batch_of(R, docs, slack=2)
    sl.counters[int(sl.offsets[1]) - 1] = 999  # a dead slot with a value outside every table
    ms = cm.map_batch(sl, tod)
    assert int(ms.counters[int(sl.offsets[1]) - 1]) == 999
    assert all(ms.doc(d) == m.doc(d) for d in range(dst.n_docs))
    # a live value outside its table is refused
    bad = batch_of(R, [([(1, 0, 10)], [0, 0, 0])])
    with pytest.raises(AssertionError):
        cm.map_batch(bad, tod)
    # the batch form and the list form of a source batch agree
    _, srcs = fold_case(rng, 60, R, lambda: 3, lambda: rng.randint(0, 4), lambda: rng.randint(0, 5),
                        lambda: rng.randint(0, 3), 40, 9, True)
    per_doc = _source_lists(srcs)
    a, b = cm.map_srcs(srcs, tod), src_batch_of(R, cm.map_source_lists(per_doc, tod))
    for f, _dt in type(srcs)._FIELDS:
        assert (np.asarray(getattr(a, f)) == np.asarray(getattr(b, f))).all(), f


def _source_lists(srcs):
    per_doc = []
    for d in range(srcs.n_docs):
        lst = []
        for s in range(int(srcs.doc_srcs[d]), int(srcs.doc_srcs[d + 1])):
            def col(off, k, a, c):
                lo, hi = int(off[s]), int(off[s + 1])
                return list(zip(k[lo:hi].tolist(), a[lo:hi].tolist(), c[lo:hi].tolist()))
            lst.append((int(srcs.src_actor[s]), srcs.vv[s * srcs.R:(s + 1) * srcs.R].tolist(),
                        col(srcs.entry_off, srcs.keys, srcs.actors, srcs.counters),
                        col(srcs.tomb_off, srcs.tkeys, srcs.tactors, srcs.tcounters)))
        per_doc.append(lst)
    return per_doc


# ---------------------------------------------------------------- the property, per operation

@pytest.mark.parametrize("R,maxn,max_c", [(2, 64, 9), (3, 200, 20), (64, 40, 64)])
def test_join_commutes_with_the_maps(R, maxn, max_c):
    rng = random.Random(R)
    dst, src = join_case(rng, 300, R, lambda: rng.randint(0, maxn), 3 * maxn, max_c)
    tod = cm.mixed(max_c)
    rc0, small = oracle.join(dst, src)
    rc1, wide = oracle.join(cm.map_batch(dst, tod), cm.map_batch(src, tod))
    assert rc0 == rc1 == 0
    assert_same_all(wide, cm.map_out(small, tod), dst.n_docs, R)
    cm.assert_mixes(wide, tod, "join")


@pytest.mark.parametrize("mode", [CRDT_FOLD_AWSET, CRDT_FOLD_DELTA])
def test_fold_commutes_with_the_maps(mode):
    rng = random.Random(7 + mode)
    R = 4
    dst, srcs = fold_case(rng, 400, R, lambda: rng.randint(0, 64), lambda: rng.randint(0, 10),
                          lambda: rng.randint(0, 8), lambda: rng.randint(0, 3), 120, 8, mode == CRDT_FOLD_DELTA)
    # first contact: every map keeps the clock entry 0 at 0
    z = np.asarray(srcs.src_actor)[np.asarray(srcs.doc_srcs)[:-1][np.diff(srcs.doc_srcs) > 0]]
    docs = np.nonzero(np.diff(srcs.doc_srcs) > 0)[0]
    dst.vv[docs[::3] * R + z[::3]] = 0
    tod = cm.mixed(8)
    rc0, small = oracle.fold(mode, dst, srcs)
    rc1, wide = oracle.fold(mode, cm.map_batch(dst, tod), cm.map_srcs(srcs, tod))
    assert rc0 == rc1 == 0
    assert_same_all(wide, cm.map_out(small, tod), dst.n_docs, R)
    cm.assert_mixes(wide, tod, "fold")


@pytest.mark.parametrize("mode", [CRDT_FOLD_AWSET, CRDT_FOLD_DELTA])
def test_fold_panic_verdicts_commute_with_the_maps(mode):
    """One document per call, so the rc is that document's verdict."""
    R = PANIC_R
    err = ok = 0
    for i, (e, vv, chain) in enumerate(panic_cases(mode)):
        tod = cm.single(MAPS[i % len(MAPS)], 6)
        dst, srcs = batch_of(R, [(e, vv)]), src_batch_of(R, [chain])
        rc0, small = oracle.fold(mode, dst, srcs)
        rc1, wide = oracle.fold(mode, cm.map_batch(dst, tod), cm.map_srcs(srcs, tod))
        assert rc0 == rc1, (i, e, vv, chain)
        if rc0 == 0:
            assert_same_all(wide, cm.map_out(small, tod), 1, R)
            ok += 1
        else:
            err += 1
    assert err > 10 and ok > 10


@pytest.mark.parametrize("R", [2, 16])
def test_delta_extract_commutes_with_the_maps(R):
    per_doc, peers = parity_case(R, 300, 1000 + R)
    tod = cm.mixed(15)  # (counters up to 12, a tombstone's up to 3 above its entry's)
    kinds0, msgs0 = expected(R, per_doc, peers)
    wide_peers = [cm.map_clock(p, tod(d)) for d, p in enumerate(peers)]
    kinds1, msgs1 = expected(R, cm.map_source_lists(per_doc, tod), wide_peers)
    assert (kinds0 == kinds1).all() and {int(k) for k in kinds0} == {model.NONE, model.DELTA, model.FULL}
    assert msgs1 == cm.map_source_lists(msgs0, tod)
    assert any(0 in p for p in wide_peers)  # peer clock 0 (ships the full state) stays 0
    cm.assert_mixes(src_batch_of(R, msgs1), tod, "extract")


@pytest.mark.parametrize("R", [2, 8])
def test_tombstone_gc_commutes_with_the_maps(R):
    per_doc, stable = gc_case(R, 400)
    tb = TombBatch.from_lists(per_doc)
    tod = cm.mixed(50)
    rc0, small = oracle.tomb_gc(tb, R, stable)
    rc1, wide = oracle.tomb_gc(cm.map_batch(tb, tod), R, cm.map_clocks(stable, R, tod))
    assert rc0 == rc1 == 0
    want = cm.map_out(small, tod)
    assert (wide.offsets == want.offsets).all() and (wide.counts == want.counts).all()
    for d in range(tb.n_docs):
        assert wide.doc(d) == want.doc(d), d
    cm.assert_mixes(wide, tod, "gc")

