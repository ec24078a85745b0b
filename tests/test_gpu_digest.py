"""GPU: the per-document state digests (crdt_awset_digest_async) against
digest_ref (tests/test_digest_model.py), bit-exact, and their comparison
(crdt_digest_diff_async) against a numpy restatement.

Every output buffer is pre-filled with poison (digest words all-ones, flags 77),
so each word read back was written by the call.  The kernels (csrc/digest.hip)
work in these units, and the edge cases below are sized around them:
  kDigChunk  = 1,024 slot positions per workgroup step (256 threads x 2 pairs
               of positions); a document whose live entries lie in one chunk has
               one owner (plain add), one that straddles a boundary uses atomics,
  kDigRun    = 512 documents of a chunk staged in LDS at most (beyond: lanes
               search the offsets in global memory and add with global atomics),
  a wave     = 128 positions per pair step (one document under a whole wave
               takes the butterfly path, otherwise the run reduction),
  kScanChunk = 8,192 documents per step of the worklist scan (compare.hip).
"""

import ctypes
import random

import numpy as np
import pytest

import crdtgpu
from crdtgpu import abi
from crdtgpu.batch import AWSetBatch, CompareBuffers, OutBuffers, TombBatch
from crdtgpu.engine import zipf_sizes
from test_compare_model import select_ref
from test_digest_model import M64, batch_of, digest_ref, known_batches, with_slack

pytestmark = pytest.mark.gpu

U8, U32, U64 = np.uint8, np.uint32, np.uint64
ONES32 = 2 ** 32 - 1
K_CHUNK = 1024
K_RUN = 512
K_SCAN = 8192


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


def dev_of(torch):
    return torch.device("cuda:0")


def poisoned_digest(torch, n_docs):
    return torch.full((max(2 * n_docs, 1),), -1, dtype=torch.int64, device=dev_of(torch))


def host_digest(t, n_docs):
    return t.cpu().numpy().view(U64)[: 2 * n_docs].reshape(n_docs, 2)


def digest_on_device(eng, torch, b, tombs=None, stream=None, engine=None):
    out = poisoned_digest(torch, b.n_docs)
    dev = dev_of(torch)
    bd, td = b.to(dev), tombs.to(dev) if tombs is not None else None
    (engine or eng).digest_async(bd, out, td, stream=stream)
    (engine or eng).sync(stream)
    return host_digest(out, b.n_docs)


def assert_digest(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    if not (got == want).all():
        d, w = [int(x[0]) for x in np.nonzero(got != want)]
        raise AssertionError("document %d word %d: gpu %#x, expected %#x (%d documents differ)"
                             % (d, w, int(got[d, w]), int(want[d, w]), int((got != want).any(axis=1).sum())))


def rand_entries(rng, R, n):
    ks = set()
    if n and rng.random() < 0.3:
        ks.add(0)
    if n > 1 and rng.random() < 0.3:
        ks.add(M64)
    while len(ks) < n:
        ks.add(rng.getrandbits(64))
    return [(k, rng.randrange(R), rng.randint(1, 2 ** 64 - 1)) for k in sorted(ks)]


# live sizes around the units, in slot order (no slack: the boundaries fall as the comments say)
SIZES = ([0, 1, 63, 64, 65, K_CHUNK - 193,          # ... the last ends exactly at the first chunk boundary
          K_CHUNK - 1, 2,                           # ends one before the second boundary; ends one past it
          K_CHUNK - 1 - 40, 7, 0, 33,               # small ones up to the third boundary
          2 * K_CHUNK + K_CHUNK // 2 + 37,          # ~2.5 chunks between small ones: the straddler path
          5, 0, 0, 128, 129, 127, 256]              # one and two waves of one document
         + [0] * (K_RUN + 90) + [1]                 # more empty documents in a row than the staging holds
         + [1] * (K_RUN + 200)                      # ... and more one-entry documents than it holds
         + [3, 0, 700, 2])
_cases = {}


def sized_case(R=2):
    """(batch, tombs, digest_ref with tombs, digest_ref without), built once."""
    if R not in _cases:
        rng = random.Random(9300 + R)
        docs, tombs = [], []
        for i, n in enumerate(SIZES):
            docs.append((rand_entries(rng, R, n), [rng.choice([0, rng.getrandbits(64)]) for _ in range(R)]))
            tombs.append(rand_entries(rng, R, 1500 if i == 3 else rng.choice([0, 0, 1, 3])))  # one tomb straddler
        b, t = batch_of(R, docs), TombBatch.from_lists(tombs)
        _cases[R] = (b, t, digest_ref(b, t), digest_ref(b))
    return _cases[R]


# ------------------------------------------------------------------ 1. known answers

def test_known_answers(eng, torch):
    for b, t, want in known_batches():
        assert_digest(digest_on_device(eng, torch, b, t), want)


# ------------------------------------------------------------------ 2. sizes, layouts, tombstones

@pytest.mark.parametrize("tombs", ["present", "null", "empty"])
@pytest.mark.parametrize("layout", ["packed", "counts", "slack"])
def test_sizes_layouts_tombstones(eng, torch, layout, tombs):
    b, t, want_t, want = sized_case()
    rng = random.Random(9400)
    if layout == "counts":  # counts given, equal to the slots
        b = AWSetBatch(b.R, b.offsets, b.keys, b.actors, b.counters, b.vv,
                       counts=np.diff(b.offsets.astype(np.int64)).astype(U32))
    elif layout == "slack":  # counts below the slots, the slack holding garbage keys
        b, t = with_slack(b, 3, rng), with_slack(t, 2, rng)
    if tombs == "null":
        t = None
    elif tombs == "empty":
        t = TombBatch.from_lists([[] for _ in range(b.n_docs)])
    want = want_t if tombs == "present" else want
    got = digest_on_device(eng, torch, b, t)
    assert_digest(got, want)
    assert (digest_on_device(eng, torch, b, t) == got).all()  # the same bits on every run


@pytest.mark.parametrize("R", [1, 2, 64])
def test_clock_widths(eng, torch, R):
    """Clock words >= 2^63, zero words in the middle, documents with no entry."""
    rng = random.Random(9500 + R)
    docs = []
    for d in range(300):
        vv = [rng.choice([0, 0, 1, 2 ** 63, 2 ** 64 - 1, rng.getrandbits(64)]) for _ in range(R)]
        if R > 2:
            vv[R // 2] = 0
        docs.append((rand_entries(rng, R, rng.choice([0, 0, 1, 5])), vv))
    docs[7] = ([], [0] * R)
    b = batch_of(R, docs)
    want = digest_ref(b)
    assert (want[7] == 0).all()
    assert_digest(digest_on_device(eng, torch, b), want)


def test_no_documents(eng, torch):
    b = batch_of(2, [])
    out = poisoned_digest(torch, 4)
    eng.digest_async(b.to(dev_of(torch)), out)
    eng.sync()
    assert (out.cpu().numpy().view(U64) == M64).all()


def test_exchange_output_is_a_state_as_it_stands(eng, torch):
    rng = random.Random(9600)
    R, n = 3, 200
    mk = lambda: batch_of(R, [(rand_entries(rng, R, rng.choice([0, 1, 9, 70, 200])),  # noqa: E731
                               [rng.randint(0, 2 ** 40) for _ in range(R)]) for _ in range(n)])
    a, b = mk(), mk()
    dev = dev_of(torch)
    slots = int(a.offsets[-1]) + int(b.offsets[-1])
    o1 = OutBuffers(n, R, slots, device=dev)
    o2 = OutBuffers(n, R, slots, device=dev, shared_keys=o1)
    d1, d2 = poisoned_digest(torch, n), poisoned_digest(torch, n)
    eng.exchange_async(a.to(dev), b.to(dev), o1, o2)
    eng.digest_async(o1.as_batch(), d1)
    eng.digest_async(o2.as_batch(), d2)
    eng.sync()
    h1, h2 = o1.as_batch().numpy(), o2.as_batch().numpy()
    assert int(h1.counts.sum()) < slots  # documents at capacity offsets, slack behind them
    g1, g2 = host_digest(d1, n), host_digest(d2, n)
    assert_digest(g1, digest_ref(h1))
    assert_digest(g2, digest_ref(h2))
    assert (g1[:, 0] == g2[:, 0]).all()  # both directions hold the same elements


# ------------------------------------------------------------------ 3. errors

def test_capacity_clamp(eng, torch):
    b, t, _, _ = sized_case()
    rng = random.Random(9700)
    b, t = with_slack(b, 1, rng), with_slack(t, 1, rng)
    b.counts[4] += 5   # above the slots: clamped to them (the garbage slot becomes live)
    assert b.counts[4] > b.offsets[5] - b.offsets[4]
    want = digest_ref(b, t)  # (clamps too)
    out = poisoned_digest(torch, b.n_docs)
    dev = dev_of(torch)
    bd, td = b.to(dev), t.to(dev)
    eng.digest_async(bd, out, td)
    with pytest.raises(crdtgpu.CrdtError) as e:
        eng.sync()
    assert e.value.code == crdtgpu.CRDT_E_CAPACITY
    assert_digest(host_digest(out, b.n_docs), want)
    eng.sync()  # cleared
    t.counts[9] = int(t.offsets[10] - t.offsets[9]) + 1  # the same for a tombstone count
    td = t.to(dev)
    eng.digest_async(bd, out, td)
    with pytest.raises(crdtgpu.CrdtError) as e:
        eng.sync()
    assert e.value.code == crdtgpu.CRDT_E_CAPACITY
    assert_digest(host_digest(out, b.n_docs), digest_ref(b, t))


def test_invalid_arguments(eng, torch):
    b, t, _, _ = sized_case()
    dev = dev_of(torch)
    bd, td = b.to(dev), t.to(dev)
    out = poisoned_digest(torch, b.n_docs)
    lib, ctx = abi.lib(), eng._ctx
    cb, ct = bd.c(), td.c()

    def rc(state, tombs, digest):
        return lib.crdt_awset_digest_async(ctx, ctypes.byref(state) if state is not None else None,
                                           ctypes.byref(tombs) if tombs is not None else None, digest, None)

    assert rc(None, None, out.data_ptr()) == crdtgpu.CRDT_E_INVALID
    assert rc(cb, None, None) == crdtgpu.CRDT_E_INVALID
    for R in (0, 65):
        wide = bd.c()
        wide.R = R
        assert rc(wide, None, out.data_ptr()) == crdtgpu.CRDT_E_INVALID
    for arr in (bd.offsets, bd.keys, bd.actors, bd.counters, bd.vv, td.offsets, td.keys, td.actors, td.counters):
        assert rc(cb, ct, arr.data_ptr()) == crdtgpu.CRDT_E_INVALID  # digest starts where an input starts
    no_off = td.c()
    no_off.offsets = None
    assert rc(cb, no_off, out.data_ptr()) == crdtgpu.CRDT_E_INVALID
    eng.sync()
    assert (out.cpu().numpy().view(U64) == M64).all()  # none of them launched anything
    # diff: NULL arrays, one of worklist / n_work, mask bits above 15
    res = CompareBuffers(8, device=dev)
    m = poisoned_digest(torch, 8)
    with pytest.raises(crdtgpu.CrdtError):
        eng.digest_diff_async(None, m, 8, res)
    with pytest.raises(crdtgpu.CrdtError):
        eng.digest_diff_async(m, None, 8, res)
    with pytest.raises(crdtgpu.CrdtError):
        eng.digest_diff_async(m, m, 8, res, mask=16)
    half = CompareBuffers(8, device=dev)
    half.n_work = None
    with pytest.raises(crdtgpu.CrdtError):
        eng.digest_diff_async(m, m, 8, half)
    noflags = CompareBuffers(8, device=dev)
    noflags.flags = None
    with pytest.raises(crdtgpu.CrdtError):
        eng.digest_diff_async(m, m, 8, noflags)


# ------------------------------------------------------------------ 4. streams, capture

def test_other_stream_and_captured_on_an_unreserved_context(eng, torch):
    b, t, want, _ = sized_case()
    assert_digest(digest_on_device(eng, torch, b, t, stream=torch.cuda.Stream()), want)
    dev = dev_of(torch)
    bd, td = b.to(dev), t.to(dev)
    e = crdtgpu.Engine(0)  # fresh: nothing reserved, no call made on it yet
    try:
        out = poisoned_digest(torch, b.n_docs)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.digest_async(bd, out, td, stream=torch.cuda.current_stream())
        for _ in range(2):
            out.fill_(-1)
            g.replay()
            e.sync(torch.cuda.current_stream())
            assert_digest(host_digest(out, b.n_docs), want)
    finally:
        e.close()


# ------------------------------------------------------------------ 5. diff

def diff_ref(mine, theirs, mask):
    flags = np.where(mine[:, 0] != theirs[:, 0], 1, np.where(mine[:, 1] != theirs[:, 1], 2, 0)).astype(U8)
    work = np.nonzero(flags & U8(mask))[0].astype(U32)
    summary = np.array([int((flags == 1).sum()), int((flags == 2).sum()), 0, 0, len(work)], U32)
    return flags, summary, work


def poisoned_cmp(torch, n_docs):
    out = CompareBuffers(n_docs, device=dev_of(torch))
    out.flags.fill_(77)
    for t in (out.summary, out.worklist, out.n_work):
        t.fill_(-1)
    return out


def read_cmp(out):
    flags, summary, work = out.numpy()
    tail = out.worklist.cpu().numpy().view(U32)[len(work):]
    assert (tail == ONES32).all(), "worklist written at or past n_work"
    return flags, summary, work


def diff_digests(n, seed):
    """Two digest arrays: a third of the documents equal, a third differing in word 1
    only, the rest in word 0 (half of those in word 1 too)."""
    rng = np.random.default_rng(seed)
    mine = rng.integers(0, 2 ** 63, (n, 2), dtype=np.int64).view(U64) * U64(2) + U64(1)
    theirs = mine.copy()
    kind = rng.integers(0, 4, n)
    theirs[kind == 1, 1] ^= U64(1)
    theirs[kind == 2, 0] ^= U64(2 ** 63)
    theirs[kind == 3] ^= U64(4)
    return mine, theirs


@pytest.mark.parametrize("mask", [0, 1, 2, 3])
def test_diff_flags_summary_worklist(eng, torch, mask):
    n = 2 * K_SCAN + 1  # one above a multiple of the scan chunk
    mine, theirs = diff_digests(n, 9800)
    dev = dev_of(torch)
    md = torch.from_numpy(mine.view(np.int64).reshape(-1).copy()).to(dev)
    td = torch.from_numpy(theirs.view(np.int64).reshape(-1).copy()).to(dev)
    res = poisoned_cmp(torch, n)
    eng.digest_diff_async(md, td, n, res, mask=mask)
    eng.sync()
    want = diff_ref(mine, theirs, mask)
    assert want[1][0] > 0 and want[1][1] > 0
    for name, g, w in zip(("flags", "summary", "worklist"), read_cmp(res), want):
        assert g.shape == w.shape and (g == w).all(), name
    # no documents: summary and n_work are still written
    res = poisoned_cmp(torch, 1)
    eng.digest_diff_async(None, None, 0, res, mask=mask)
    eng.sync()
    assert not res.summary.cpu().numpy().any() and int(res.n_work.cpu().numpy()[0]) == 0
    assert int(res.flags.cpu().numpy()[0]) == 77


def test_digest_diff_select_on_device(eng, torch):
    """digest both replicas, diff, select the differing documents: no host round trip."""
    b, t, _, _ = sized_case()
    rng = random.Random(9900)
    other = with_slack(b, 2, rng)  # the same live state in another layout ...
    changed = sorted(set(rng.sample(range(b.n_docs), 40)) | {12})
    for d in changed:  # ... except here: a dot, or the last clock word
        o = int(other.offsets[d])
        if other.counts[d] and d % 2:
            other.counters[o + int(other.counts[d]) - 1] ^= U64(1)
        else:
            other.vv[d * b.R + b.R - 1] ^= U64(2 ** 63)
    dev = dev_of(torch)
    bd, od = b.to(dev), other.to(dev)
    n = b.n_docs
    dm, dt = poisoned_digest(torch, n), poisoned_digest(torch, n)
    res = poisoned_cmp(torch, n)
    want_sel = select_ref(b, np.array(changed, U32), n_idx=len(changed), n_out=len(changed))
    out = OutBuffers(len(changed), b.R, int(want_sel.offsets[-1]) + 4, device=dev)
    eng.digest_async(bd, dm)
    eng.digest_async(od, dt)
    eng.digest_diff_async(dm, dt, n, res)
    eng.select_async(bd, out, idx=res.worklist, n_idx=res.n_work)
    eng.sync()
    flags, summary, work = read_cmp(res)
    assert work.tolist() == changed and summary.tolist() == [0, len(changed), 0, 0, len(changed)]
    assert (flags[changed] == crdtgpu.CRDT_DIG_STATE).all() and int(flags.sum()) == 2 * len(changed)
    h = out.as_batch().numpy()
    for j in range(len(changed)):
        assert h.doc(j) == want_sel.doc(j), j


# ------------------------------------------------------------------ 6. mid-size parity

def _host_batch(o):
    return o.as_batch().numpy()


def test_parity_zipf(eng, torch):
    dev = dev_of(torch)
    n = 4096  # Zipf sizes: documents of several hundred chunks beside documents of one entry
    sizes = zipf_sizes(0xD16E57, n)
    assert int(sizes.max()) > 3 * K_CHUNK
    offs = np.zeros(n + 1, dtype=U32)
    np.cumsum(sizes, out=offs[1:])
    total = int(offs[-1])
    A, B = OutBuffers(n, 2, total, device=dev), OutBuffers(n, 2, total, device=dev)
    eng.gen_zipf_async(0xD16E57, n, torch.from_numpy(offs.view(np.int32).copy()).to(dev), A, B)
    da, db = poisoned_digest(torch, n), poisoned_digest(torch, n)
    eng.digest_async(A.as_batch(), da)
    eng.digest_async(B.as_batch(), db)
    eng.sync()
    ga, gb = host_digest(da, n), host_digest(db, n)
    assert_digest(ga, crdtgpu.digest_host(_host_batch(A)))
    del A
    assert_digest(gb, crdtgpu.digest_host(_host_batch(B)))
    assert (ga != gb).any(axis=1).sum() > n // 2


def test_parity_pair(eng, torch):
    dev = dev_of(torch)
    n = 65536  # 64 entries in 64 slots per document
    A, B = OutBuffers(n, 2, n * 64, device=dev), OutBuffers(n, 2, n * 64, device=dev)
    eng.gen_pair_async(0xD16E57, n, A, B)
    da, db = poisoned_digest(torch, n), poisoned_digest(torch, n)
    eng.digest_async(A.as_batch(), da)
    eng.digest_async(B.as_batch(), db)
    eng.sync()
    ga, gb = host_digest(da, n), host_digest(db, n)
    assert_digest(ga, crdtgpu.digest_host(_host_batch(A)))
    assert_digest(gb, crdtgpu.digest_host(_host_batch(B)))
    assert (ga != gb).any(axis=1).all()  # every pair of replicas differs
