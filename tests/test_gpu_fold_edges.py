"""GPU: the fold kernels on every dispatch edge of csrc/fold.hip, bit-exact against
the C oracle.

The cases are the deterministic builders of tests/fold_edge_cases.py;
tests/test_fold_paths_model.py shows on the CPU which path each document takes
(tests/fold_paths.py) and that every class is populated.  Every case runs with
the lean pass first and with the general kernel alone (fold_lean_first 1 / 0:
for AWSet folds the latter is the general kernel over whole batches, which no
other test launches).  On top: dst with counts and adversarial slack, a delta
source batch without tombstone arrays, the capacity and workspace reports,
guard bands around all six output arrays, and the source ladder at 64-bit
counters."""

import random

import numpy as np
import pytest

import counter_maps as cm
import crdtgpu
import fold_edge_cases as fe
import fold_paths as fp
from crdtgpu import CRDT_FOLD_AWSET, CRDT_FOLD_DELTA
from crdtgpu.batch import AWSetBatch, OutBuffers
from helpers import batch_of, src_batch_of
from oracle import oracle
from test_gpu_parity import assert_same, fold_case, host_out, wide_key_case
from test_gpu_wide_counters import check_fold, wide_fold

pytestmark = pytest.mark.gpu

AWSET, DELTA = CRDT_FOLD_AWSET, CRDT_FOLD_DELTA


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "GPU tests need a HIP device"
    return t


@pytest.fixture(scope="module")
def eng(torch):
    e = crdtgpu.Engine(0)
    yield e
    e.close()


_wants = {}


def want_of(key, mode, dst, srcs):
    """The oracle's output of a batch, computed once and shared (never modified)."""
    if key not in _wants:
        rc, want = oracle.fold(mode, dst, srcs)
        assert rc == 0
        _wants[key] = want
    return _wants[key]


class lean_first:
    """fold_lean_first set for the block, restored to the default afterwards."""

    def __init__(self, eng, value):
        self.eng, self.value = eng, value

    def __enter__(self):
        self.eng.set_option("fold_lean_first", self.value)

    def __exit__(self, *a):
        self.eng.set_option("fold_lean_first", 1)


def fold_dev(eng, torch, mode, dst, srcs, out=None, reserve=True):
    """fold_async on device copies of host batches; the output downloaded."""
    dev = torch.device("cuda:0")
    slots = srcs.out_slots(dst)
    out = out or OutBuffers(dst.n_docs, dst.R, slots, device=dev)
    if reserve:
        eng.reserve(dst.n_docs, slots)
    eng.fold_async(mode, dst.to(dev), srcs.to(dev), out)
    eng.sync()
    return host_out(out, torch)


# ---------------------------------------------------------------- every builder, both passes

CASES = sorted(fe.all_cases())


@pytest.mark.parametrize("lean", [1, 0])
@pytest.mark.parametrize("name", CASES)
def test_edge_case(eng, name, lean):
    c = fe.all_cases()[name]
    with lean_first(eng, lean):
        for i, (dst, srcs) in enumerate(c.batches):
            want = want_of((name, i), c.mode, dst, srcs)
            assert_same(eng.fold(c.mode, dst, srcs), want, dst.n_docs, dst.R)


def parity_awset_batches():
    """The AWSet batches of test_gpu_parity.py's fold tests (its builders, its arguments)."""
    out = {}
    rng = random.Random(20 + AWSET)
    out["wave"] = fold_case(rng, 3000, 4, lambda: rng.randint(0, 64), lambda: rng.randint(0, 10),
                            lambda: rng.randint(0, 8), lambda: rng.randint(0, 3), 120, 8, False)
    for universe, max_src in [(16, 4), (40, 15), (64, 15), (64, 16), (65, 8)]:
        r2 = random.Random(universe * 100 + max_src + AWSET)
        out["dense_%d_%d" % (universe, max_src)] = fold_case(
            r2, 1500, 4, lambda: r2.randint(0, min(universe, 60)), lambda: r2.randint(0, max_src),
            lambda: r2.randint(0, min(universe, 12)), lambda: r2.randint(0, 3), universe, 9, False)
    r3 = random.Random(30 + AWSET)
    out["block"] = fold_case(r3, 200, 3, lambda: r3.choice([10, 100, 127, 128, 129, 600]), lambda: r3.randint(0, 6),
                             lambda: r3.choice([5, 40, 64, 65, 300]), lambda: r3.choice([0, 2, 64, 65, 200]), 5000, 50,
                             False)
    R, dsts, per_doc = wide_key_case(AWSET)
    out["wide_keys"] = (batch_of(R, dsts), src_batch_of(R, per_doc))
    return out


PARITY = ["wave", "dense_16_4", "dense_40_15", "dense_64_15", "dense_64_16", "dense_65_8", "block", "wide_keys"]
_parity = {}


@pytest.mark.parametrize("which", PARITY)
def test_parity_awset_cases_on_the_general_kernel(eng, which):
    if not _parity:
        _parity.update(parity_awset_batches())
    dst, srcs = _parity[which]
    want = want_of(("parity", which), AWSET, dst, srcs)
    with lean_first(eng, 0):
        assert_same(eng.fold(AWSET, dst, srcs), want, dst.n_docs, dst.R)


# ---------------------------------------------------------------- slack, no tombstone arrays

@pytest.mark.parametrize("lean", [1, 0])
@pytest.mark.parametrize("mode", [AWSET, DELTA])
def test_dst_counts_and_slack(eng, torch, mode, lean):
    case, compact = fe.slack_case(mode)
    dst, srcs = case.batches[0]
    want = want_of((case.name, 0), mode, dst, srcs)
    with lean_first(eng, lean):
        batch = eng.fold(mode, dst, srcs)
        dev = fold_dev(eng, torch, mode, dst, srcs)
        plain = eng.fold(mode, compact, srcs)
    assert_same(batch, want, dst.n_docs, dst.R)
    assert_same(dev, want, dst.n_docs, dst.R)
    # counts == NULL over the same live documents: the same live output (other slot bounds)
    assert fp.arrays_equal_live(plain, want, dst.n_docs, dst.R) is None


@pytest.mark.parametrize("lean", [1, 0])
def test_delta_fold_without_tombstone_arrays(eng, torch, lean):
    case, twin = fe.no_tomb_case()
    dst, bare = case.batches[0]
    want = want_of((case.name, 0), DELTA, dst, bare)
    with lean_first(eng, lean):
        for srcs in (bare, twin):
            assert_same(eng.fold(DELTA, dst, srcs), want, dst.n_docs, dst.R)
            assert_same(fold_dev(eng, torch, DELTA, dst, srcs), want, dst.n_docs, dst.R)


# ---------------------------------------------------------------- capacity and workspace reports

def report_batch(mode, big):
    """(dst with counts and one slack slot a document, srcs, p): 40 small documents;
    document p is a block-path one when `big`."""
    delta = mode == DELTA
    R = 3
    rng = random.Random(9800 + mode + 10 * big)
    docs = [fe.make_doc(rng, R, delta, rng.randint(0, 9), rng.randint(1, 12), list(range(100 * d, 100 * d + 40)))
            for d in range(40)]
    p = 17
    if big:
        docs[p] = fe.sized_doc(rng, R, delta, 300, 60, 12 if delta else 0, 3, list(range(100000, 100600)))
    dst = batch_of(R, [(e, vv) for e, vv, _ in docs], slack=1)
    s = int(dst.offsets[p + 1]) - 1  # p's slack slot continues its keys: clamped to its slots, p is still a sorted document
    dst.keys[s], dst.actors[s], dst.counters[s] = int(dst.keys[s - 1]) + 1, 0, 1
    return dst, src_batch_of(R, [c for _, _, c in docs]), p


def same_but(got, want, n_docs, R, skip):
    for d in range(n_docs):
        if d != skip:
            assert fp.arrays_equal_live(_one(got, d), _one(want, d), 1, R) is None, "doc %d" % d
    assert list(got.offsets[: n_docs + 1]) == list(want.offsets[: n_docs + 1])


class _one:
    """Document d of an output as a one-document output."""

    def __init__(self, o, d):
        self.offsets, self.counts = o.offsets[d:d + 2], o.counts[d:d + 1]
        self.keys, self.actors, self.counters = o.keys, o.actors, o.counters
        self.vv = o.vv[d * o.R:(d + 1) * o.R]


@pytest.mark.parametrize("big", [0, 1], ids=["pipe", "block"])
@pytest.mark.parametrize("mode", [AWSET, DELTA])
def test_live_count_above_slots_is_clamped_and_reported(eng, torch, mode, big):
    dst, srcs, p = report_batch(mode, big)
    slots_p = int(dst.offsets[p + 1]) - int(dst.offsets[p])
    want = want_of(("report", mode, big), mode, dst, srcs)  # (every count within its slots)
    counts = dst.counts.copy()
    counts[p] = slots_p + 2
    over = AWSetBatch(dst.R, dst.offsets, dst.keys, dst.actors, dst.counters, dst.vv, counts)
    dev = torch.device("cuda:0")
    out = OutBuffers(dst.n_docs, dst.R, srcs.out_slots(dst), device=dev)
    eng.reserve(dst.n_docs, out.slots)
    eng.fold_async(mode, over.to(dev), srcs.to(dev), out)
    with pytest.raises(crdtgpu.CrdtError) as ei:
        eng.sync()
    assert ei.value.code == crdtgpu.CRDT_E_CAPACITY
    same_but(host_out(out, torch), want, dst.n_docs, dst.R, skip=p)
    eng.sync()  # the report was cleared


@pytest.mark.parametrize("mode", [AWSET, DELTA])
def test_block_kernel_without_scratch_reports_workspace(torch, mode):
    dst, srcs, p = report_batch(mode, 1)
    want = want_of(("report", mode, 1), mode, dst, srcs)
    dev = torch.device("cuda:0")
    fresh = crdtgpu.Engine(0)
    try:
        out = OutBuffers(dst.n_docs, dst.R, srcs.out_slots(dst), device=dev)
        fresh.fold_async(mode, dst.to(dev), srcs.to(dev), out)  # never reserved: one scratch slot
        with pytest.raises(crdtgpu.CrdtError) as ei:
            fresh.sync()
        assert ei.value.code == crdtgpu.CRDT_E_WORKSPACE
        same_but(host_out(out, torch), want, dst.n_docs, dst.R, skip=p)
        assert_same(fold_dev(fresh, torch, mode, dst, srcs), want, dst.n_docs, dst.R)
    finally:
        fresh.close()


# ---------------------------------------------------------------- guard bands

GUARD = 64
PAT64, PAT32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A


class GuardedOut:
    """Output arrays that are views GUARD elements inside pattern-filled tensors."""

    def __init__(self, torch, n_docs, R, slots):
        dev = torch.device("cuda:0")
        self.n_docs, self.R, self.slots = n_docs, R, slots
        self.big = {}
        sizes = dict(offsets=(n_docs + 1, torch.int32), counts=(n_docs, torch.int32), keys=(slots, torch.int64),
                     actors=(slots, torch.int32), counters=(slots, torch.int64), vv=(n_docs * R, torch.int64))
        for f, (n, dt) in sizes.items():
            b = torch.full((n + 2 * GUARD,), PAT64 if dt == torch.int64 else PAT32, dtype=dt, device=dev)
            self.big[f] = (b, n)
            setattr(self, f, b[GUARD:GUARD + n])

    def c(self):
        return OutBuffers.c(self)

    def assert_bands(self):
        for f, (b, n) in self.big.items():
            h = b.cpu().numpy()
            pat = np.array(PAT64 if h.dtype == np.int64 else PAT32, dtype=h.dtype)
            assert (h[:GUARD] == pat).all(), "%s: written before its first element" % f
            assert (h[GUARD + n:] == pat).all(), "%s: written past its last element" % f


def guard_batches(mode):
    yield "source ladder", fe.source_ladder(mode, fe.LADDER_R[mode][0]).batches[0]
    for n in fe.DOC_COUNTS[mode][-4:]:
        yield "%d documents" % n, fe.doc_count_batch(mode, n, 0, True)


@pytest.mark.parametrize("lean", [1, 0])
@pytest.mark.parametrize("mode", [AWSET, DELTA])
def test_outputs_stay_inside_their_arrays(eng, torch, mode, lean):
    with lean_first(eng, lean):
        for what, (dst, srcs) in guard_batches(mode):
            want = want_of(("guard", mode, what), mode, dst, srcs)
            out = GuardedOut(torch, dst.n_docs, dst.R, srcs.out_slots(dst))
            assert_same(fold_dev(eng, torch, mode, dst, srcs, out=out), want, dst.n_docs, dst.R)
            out.assert_bands()


# ---------------------------------------------------------------- 64-bit counters

@pytest.mark.parametrize("mode", [AWSET, DELTA])
def test_source_ladder_wide_counters(eng, mode):
    """The source ladder through the order-preserving counter maps (all six mixed per
    document): against the oracle on the mapped inputs, and against the mapped
    result of the small-counter run."""
    dst, srcs = fe.source_ladder(mode, fe.LADDER_R[mode][0]).batches[0]
    check_fold(eng, wide_fold(mode, dst, srcs, cm.mixed(fe.CMAX), "source ladder mode %d" % mode))
