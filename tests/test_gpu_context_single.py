"""GPU: the causal-context summary (csrc/reduce.hip: per-workgroup partial rows
in the engine's workspace, then one workgroup folds them).  Checked against
numpy.max over the u64 view of the clocks, never against another GPU run: sizes
round the per-workgroup 256 documents and the cap of 1,024 workgroups, values
with the top bit set (a signed compare picks the wrong maximum), repeated calls
and graph replays on one engine (whatever the summary keeps in the engine's
workspace between its kernels must be fit for the next call), and a
large-document join between two summaries (its reset kernel zeroes the engine's
per-call counters).
"""

import random

import numpy as np
import pytest

from crdtgpu.batch import OutBuffers
from helpers import batch_of, random_state
from oracle import oracle
from test_gpu_parity import assert_same_all, host_out

pytestmark = pytest.mark.gpu

N_DOCS = [1, 2, 255, 256, 257, 4097, 1024 * 256 + 1]  # the last: 1,025 workgroups wanted, 1,024 launched
RS = [1, 2, 3, 8, 16, 64]
TOP = np.uint64(1) << np.uint64(63)


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "GPU tests need a HIP device"
    return t


@pytest.fixture(scope="module")
def eng(torch):
    import crdtgpu

    e = crdtgpu.Engine(0)
    yield e
    e.close()


def clocks(seed, n, R):
    """n * R u64 clocks: about half with the top bit set, the rest below 2^62; one
    column's maximum in the last document, another's in the first."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 1 << 62, size=n * R, dtype=np.uint64)
    v |= np.where(rng.random(n * R) < 0.5, TOP, np.uint64(0))
    v = v.reshape(n, R)
    v[n - 1, 0] = np.uint64(0xFFFFFFFFFFFFFFFF)
    v[0, R - 1] = np.uint64(0xFFFFFFFFFFFFFFFE)
    return v


def want_of(v):
    w = v.max(axis=0)
    assert w.dtype == np.uint64 and w[0] & TOP and w[-1] & TOP  # a signed maximum would have the top bit clear
    return w


def on_device(torch, v):
    return torch.from_numpy(v.view(np.int64).reshape(-1).copy()).to("cuda:0")


def got_of(out):
    return out.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("n", N_DOCS)
def test_summary_is_the_unsigned_columnwise_maximum(eng, torch, n, R):
    v = clocks(n * 131 + R, n, R)
    out = torch.full((R,), -1, dtype=torch.int64, device="cuda:0")
    eng.causal_context_async(on_device(torch, v), n, R, out)
    eng.sync()
    assert (got_of(out) == want_of(v)).all()


def test_no_top_bit_anywhere(eng, torch):
    """All clocks below 2^63, and a column that is zero in every document."""
    n, R = 4097, 3
    v = clocks(5, n, R) & ~TOP
    v[:, 1] = 0
    out = torch.full((R,), -1, dtype=torch.int64, device="cuda:0")
    eng.causal_context_async(on_device(torch, v), n, R, out)
    eng.sync()
    assert (got_of(out) == v.max(axis=0)).all()


def test_five_calls_in_a_row_on_one_engine(eng, torch):
    """Different inputs and sizes back to back, no sync in between: no call may
    see a partial row or a counter of the call before it."""
    cases = [(4097, 3), (257, 64), (1024 * 256 + 1, 2), (2, 8), (70000, 16)]
    vs = [clocks(40 + i, n, R) for i, (n, R) in enumerate(cases)]
    dvs = [on_device(torch, v) for v in vs]
    outs = [torch.full((R,), -1, dtype=torch.int64, device="cuda:0") for _, R in cases]
    torch.cuda.synchronize()
    for (n, R), dv, out in zip(cases, dvs, outs):
        eng.causal_context_async(dv, n, R, out)
    eng.sync()
    for v, out in zip(vs, outs):
        assert (got_of(out) == want_of(v)).all()


def test_captured_and_replayed_with_changed_input(eng, torch):
    n, R = 70000, 2
    vs = [clocks(60 + i, n, R) for i in range(4)]
    dv = on_device(torch, vs[0])
    out = torch.full((R,), -1, dtype=torch.int64, device="cuda:0")
    eng.causal_context_async(dv, n, R, out)  # eager first, as a caller warms up before a capture
    eng.sync()
    assert (got_of(out) == want_of(vs[0])).all()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.causal_context_async(dv, n, R, out, stream=torch.cuda.current_stream())
    for v in vs[1:]:
        dv.copy_(on_device(torch, v))
        out.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert (got_of(out) == want_of(v)).all()


def test_large_document_join_between_two_summaries(eng, torch):
    """summary, join with documents above 64 entries (its reset kernel and its
    worklist counters), summary of the join's clocks -- one stream, no sync in
    between; the join equals the oracle's and both summaries numpy's."""
    rng = random.Random(77)
    R, n = 3, 40
    sz = lambda d: rng.choice([70, 300, 1500]) if d % 7 == 0 else rng.randint(0, 64)  # noqa: E731
    dsts = [random_state(rng, R, sz(d), 6000, 25) for d in range(n)]
    srcs = [random_state(rng, R, sz(d), 6000, 25) for d in range(n)]
    a, b = batch_of(R, dsts), batch_of(R, srcs)
    rc, want = oracle.join(a, b)
    assert rc == 0
    dev = torch.device("cuda:0")
    da, db = a.to(dev), b.to(dev)
    o = OutBuffers(n, R, int(a.offsets[-1]) + int(b.offsets[-1]), device=dev)
    for t in (o.offsets, o.counts, o.keys, o.actors, o.counters, o.vv):
        t.fill_(-1)
    v = clocks(9, 4097, R)
    dv = on_device(torch, v)
    out1 = torch.full((R,), -1, dtype=torch.int64, device="cuda:0")
    out2 = torch.full((R,), -1, dtype=torch.int64, device="cuda:0")
    s = torch.cuda.current_stream()
    torch.cuda.synchronize()
    eng.causal_context_async(dv, 4097, R, out1, stream=s)
    eng.join_async(da, db, o, stream=s)
    eng.causal_context_async(o.vv, n, R, out2, stream=s)
    eng.sync(s)
    assert (got_of(out1) == want_of(v)).all()
    assert_same_all(host_out(o, torch), want, n, R)
    assert (got_of(out2) == np.asarray(want.vv[: n * R]).reshape(n, R).max(axis=0)).all()
