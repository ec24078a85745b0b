"""GPU: the convergence check (crdt_awset_compare_async / _batch) and the
sub-batch selection (crdt_awset_select_async) against compare_ref / select_ref
(tests/test_compare_model.py), bit-exact.

Every output buffer is pre-filled with poison (flags 77, words all-ones), so each
word read back was written by the call; worklist words at or past n_work and
entry slots at or past offsets[n_out] must still hold it.  The kernels
(csrc/compare.hip) work in these units, and the edge cases below are sized
around them:
  kCmpChunk   = 2,048 slot positions of `a` per compare workgroup step
                (256 threads x 4 pairs of positions),
  kCmpRun     = 1,024 documents of a chunk staged in LDS at most (beyond: lanes
                search the offsets in global memory),
  kCmpVvChunk = 1,024 clock words per workgroup step,
  kSelChunk   = 2,048 output positions per gather step, kSelRun = 1,024,
  kScanChunk  = 8,192 documents per step of the single-workgroup scans
                (worklist, select offsets).
"""

import ctypes
import random

import numpy as np
import pytest

import crdtgpu
from crdtgpu import abi
from crdtgpu.batch import AWSetBatch, CompareBuffers, OutBuffers
from helpers import batch_of, random_state
from oracle import oracle
from test_compare_model import A_AHEAD, B_AHEAD, DOTS, KEYS, compare_ref, golden_pairs, select_ref

pytestmark = pytest.mark.gpu

U8, U32, U64 = np.uint8, np.uint32, np.uint64
MAXK = 2 ** 64 - 1
ONES32 = 2 ** 32 - 1
K_CHUNK = 2048
K_RUN = 1024
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


def poisoned_cmp(torch, n_docs, worklist=True, summary=True):
    out = CompareBuffers(n_docs, device=dev_of(torch), worklist=worklist, summary=summary)
    out.flags.fill_(77)
    for t in (out.summary, out.worklist, out.n_work):
        if t is not None:
            t.fill_(-1)
    return out


def read_cmp(out):
    """(flags, summary, worklist) of a poisoned CompareBuffers after the call; the
    worklist's tail must be untouched."""
    flags, summary, work = out.numpy()
    if out.worklist is not None:
        tail = out.worklist.cpu().numpy().view(U32)[len(work):]
        assert (tail == ONES32).all(), "worklist written at or past n_work"
    return flags, summary, work


def assert_cmp(got, want):
    for name, g, w in zip(("flags", "summary", "worklist"), got, want):
        if g is None:
            continue
        assert g.shape == w.shape, (name, g.shape, w.shape)
        if not (g == w).all():
            i = int(np.nonzero(g != w)[0][0])
            raise AssertionError("%s differs first at %d: gpu %d, expected %d" % (name, i, g[i], w[i]))


def cmp_on_device(eng, torch, a, b, mask=15, worklist=True, summary=True, stream=None):
    out = poisoned_cmp(torch, a.n_docs, worklist, summary)
    eng.compare_async(a.to(dev_of(torch)), b.to(dev_of(torch)), out, mask=mask, stream=stream)
    eng.sync(stream)
    return read_cmp(out)


def poisoned_out(torch, n_docs, R, slots):
    out = OutBuffers(n_docs, R, slots, device=dev_of(torch))
    for t in (out.offsets, out.counts, out.keys, out.actors, out.counters, out.vv):
        t.fill_(-1)
    return out


def host_out(out):
    h = OutBuffers(out.n_docs, out.R, 0)
    for f in ("offsets", "counts", "keys", "actors", "counters", "vv"):
        a = getattr(out, f).cpu().numpy()
        setattr(h, f, a.view(U32 if a.dtype == np.int32 else U64))
    h.slots = out.slots
    return h


def assert_packed(out, want, n_out=None, check_tail=True):
    """A select output (device OutBuffers, poisoned before the call) equals the
    packed batch `want`; entry slots at or past offsets[n_out] hold the poison."""
    h = host_out(out)
    n = want.n_docs if n_out is None else n_out
    R = want.R
    assert (h.offsets[: n + 1] == want.offsets).all(), "offsets"
    assert (h.counts[:n] == want.counts).all(), "counts"
    assert (h.vv[: n * R] == want.vv).all(), "vv"
    total = int(want.offsets[-1])
    for f in ("keys", "actors", "counters"):
        assert (getattr(h, f)[:total] == getattr(want, f)).all(), f
    if check_tail:
        assert (h.keys[total:out.slots] == MAXK).all() and (h.counters[total:out.slots] == MAXK).all()
        assert (h.actors[total:out.slots] == ONES32).all()
    return h


def pack(R, docs, slack=0, with_counts=False, garbage=None):
    """docs: [(keys, actors, counters, vv)] -> AWSetBatch; slack slots filled from
    the `garbage` rng (so two sides hold different stale entries)."""
    n = len(docs)
    counts = np.array([len(d[0]) for d in docs], U32)
    offsets = np.zeros(n + 1, U32)
    np.cumsum(counts + U32(slack), out=offsets[1:])
    total = int(offsets[-1])
    if garbage is not None:
        keys = garbage.integers(0, 2 ** 63, max(total, 1), dtype=np.int64).view(U64).copy()
        actors = garbage.integers(0, 2 ** 31, max(total, 1), dtype=np.int64).astype(U32)
        counters = garbage.integers(0, 2 ** 63, max(total, 1), dtype=np.int64).view(U64).copy()
    else:
        keys, actors, counters = np.zeros(max(total, 1), U64), np.zeros(max(total, 1), U32), np.zeros(max(total, 1), U64)
    vv = np.zeros(max(n * R, 1), U64)
    for d, (k, a, c, v) in enumerate(docs):
        o, m = int(offsets[d]), len(k)
        keys[o:o + m] = np.asarray(k, dtype=U64)
        actors[o:o + m] = np.asarray(a, dtype=U32)
        counters[o:o + m] = np.asarray(c, dtype=U64)
        vv[d * R:(d + 1) * R] = v
    return AWSetBatch(R, offsets, keys, actors, counters, vv[: n * R],
                      counts=counts if (slack or with_counts) else None)


# ------------------------------------------------------------------ 1. golden

def test_golden_snapshots_all_pairs(eng, torch):
    import itertools

    n = 0
    for R, docs, snaps in golden_pairs():
        pairs = list(itertools.product(range(len(snaps)), repeat=2))
        a = batch_of(R, [docs[i] for i, _ in pairs])
        b = batch_of(R, [docs[j] for _, j in pairs], slack=1)
        want = compare_ref(a, b)
        assert_cmp(cmp_on_device(eng, torch, a, b), want)
        for p, (i, j) in enumerate(pairs):  # assertEntries, straight from the fixture
            same = sorted(e[0] for e in snaps[i]["entries"]) == sorted(e[0] for e in snaps[j]["entries"])
            assert bool(want[0][p] & KEYS) == (not same)
        n += len(pairs)
    assert n >= 23 * 23


# ------------------------------------------------------------ 2. random small

LIVE = (0, 1, 2, 63, 64, 65, 200)
KINDS = ("first_key", "last_key", "last_counter", "last_actor", "clock", "counts")
_small = {}


def _rand_doc(rng, R, n):
    ks = set()
    if n and rng.random() < 0.3:
        ks.add(0)
    if n > 1 and rng.random() < 0.3:
        ks.add(MAXK)
    while len(ks) < n:
        ks.add(rng.getrandbits(64))
    ks = sorted(ks)
    return (ks, [rng.randrange(R) for _ in ks], [rng.randint(1, 2 ** 40) for _ in ks],
            [rng.randint(0, 2 ** 40) for _ in range(R)])


def small_case(slack, with_counts, n_docs=2000):
    """(a, b, compare_ref(a, b), kinds seen) built once per layout.  About half the
    documents identical; each of the rest differs in exactly one place."""
    key = (slack, with_counts)
    if key in _small:
        return _small[key]
    rng = random.Random(9000 + 10 * slack + with_counts)
    R = 2
    da, db, seen = [], [], {k: 0 for k in KINDS}
    for _ in range(n_docs):
        k, a, c, v = _rand_doc(rng, R, rng.choice(LIVE))
        da.append((k, a, c, v))
        k, a, c, v = list(k), list(a), list(c), list(v)
        if rng.random() < 0.5:
            db.append((k, a, c, v))
            continue
        kind = rng.choice(KINDS)
        if kind != "counts" and not k:
            kind = "clock"
        if kind == "first_key":
            nk = k[0] - 1 if k[0] > 0 else 1
            kind = "clock" if (len(k) > 1 and nk >= k[1]) else kind
            if kind == "first_key":
                k[0] = nk
        if kind == "last_key":
            k[-1] = k[-1] + 1 if k[-1] < MAXK else MAXK - 1
            if len(k) > 1 and k[-1] <= k[-2]:
                k[-1], kind = MAXK, "clock"
        if kind == "last_counter":
            c[-1] += 1
        elif kind == "last_actor":
            a[-1] ^= 1
        elif kind == "counts":  # this side's count drawn on its own
            k, a, c, _ = _rand_doc(rng, R, rng.choice(LIVE))
        if kind == "clock":
            r = rng.randrange(R)
            v[r] += 1 if (v[r] == 0 or rng.random() < 0.5) else -1
        seen[kind] += 1
        db.append((k, a, c, v))
    ga, gb = np.random.default_rng(1), np.random.default_rng(2)
    a = pack(R, da, slack, with_counts, ga)
    b = pack(R, db, slack, with_counts, gb)
    _small[key] = (a, b, compare_ref(a, b), seen)
    return _small[key]


LAYOUTS = [(0, 0), (0, 1), (3, 1)]  # (slack, counts given); counts == NULL only at zero slack


@pytest.mark.parametrize("slack,with_counts", LAYOUTS)
def test_random_small(eng, torch, slack, with_counts):
    a, b, want, seen = small_case(slack, with_counts)
    assert (a.counts is None) == (not slack and not with_counts)
    assert all(v > 20 for v in seen.values()), seen
    flags = want[0]
    assert 800 < int((flags == 0).sum()) < 1200
    assert (flags & KEYS).any() and (flags & DOTS).any() and (flags & A_AHEAD).any() and (flags & B_AHEAD).any()
    assert_cmp(cmp_on_device(eng, torch, a, b), want)
    assert_cmp(cmp_on_device(eng, torch, b, a), compare_ref(b, a))


def test_identical_batches_with_different_slack_contents(eng, torch):
    a, _, _, _ = small_case(3, 1)
    b = AWSetBatch(a.R, a.offsets, a.keys.copy(), a.actors.copy(), a.counters.copy(), a.vv, counts=a.counts)
    for d in range(a.n_docs):  # every slack slot differs between the sides
        o = int(a.offsets[d]) + int(a.counts[d])
        b.keys[o:o + 3] ^= U64(0x5555)
        b.actors[o:o + 3] ^= U32(1)
        b.counters[o:o + 3] += U64(1)
    flags, summary, work = cmp_on_device(eng, torch, a, b)
    assert not flags.any() and not summary.any() and len(work) == 0


# ------------------------------------------------------------- 3. chunk edges

def _seq_doc(start, n, R=2):
    k = (np.arange(n, dtype=U64) * U64(3) + U64(start)).tolist()
    return (k, [i % R for i in range(n)], [i + 1 for i in range(n)], [5] * R)


def _edge_docs():
    """Documents laid out so that, at zero slack, `a`'s slot space has: a document
    one below a chunk (2,047); one of 2,050 entries that starts on a chunk's last
    slot and so spans three chunks, differing only in its very last entry; a
    filler; another such document differing only in its very first entry; a filler
    that ends on a chunk boundary; documents of exactly one chunk and one above;
    then 1,500 one-entry documents (more per chunk than kCmpRun stages), empty
    documents among them."""
    sizes = [K_CHUNK - 1, K_CHUNK + 2, K_CHUNK - 2, K_CHUNK + 2, K_CHUNK - 1, K_CHUNK, K_CHUNK + 1]
    assert sum(sizes[:1]) % K_CHUNK == K_CHUNK - 1 and sum(sizes[:3]) % K_CHUNK == K_CHUNK - 1
    assert sum(sizes[:5]) % K_CHUNK == 0
    da = [_seq_doc(1000 * i, n) for i, n in enumerate(sizes)]
    db = [tuple(list(x) for x in d) for d in da]
    db[1][0][-1] += 1          # the three-chunk document's very last key
    db[3][0][0] -= 1           # ... very first key
    db[5][2][K_CHUNK - 1] += 7  # exactly one chunk: last counter
    db[6][1][0] ^= 1           # one above: first actor
    want = {1: KEYS, 3: KEYS, 5: DOTS, 6: DOTS}
    rng = random.Random(9100)
    for i in range(1500):
        d = len(da)
        if i % 7 == 3:
            da.append(([], [], [], [5, 5]))
            db.append(([], [], [], [5, 5]))
            continue
        doc = ([10 * i + 1], [i % 2], [i + 1], [5, 5])
        da.append(doc)
        other = tuple(list(x) for x in doc)
        r = rng.randrange(6)
        if r == 0:
            other[0][0] += 1
            want[d] = KEYS
        elif r == 1:
            other[2][0] += 1
            want[d] = DOTS
        elif r == 2:
            other = ([], [], [], [5, 5])
            want[d] = KEYS
        db.append(other)
    return da, db, want


@pytest.mark.parametrize("b_slack", [0, 1])
def test_chunk_edges(eng, torch, b_slack):
    """b_slack 0: both sides share the layout (pairs of neighbouring entries read
    with 16 B loads); 1: every other document of b starts at an odd slot."""
    da, db, marked = _edge_docs()
    a = pack(2, da)
    b = pack(2, db, slack=b_slack, garbage=np.random.default_rng(3))
    want = compare_ref(a, b)
    for d in range(a.n_docs):
        assert int(want[0][d]) == marked.get(d, 0), d
    assert_cmp(cmp_on_device(eng, torch, a, b), want)
    assert_cmp(cmp_on_device(eng, torch, b, a), compare_ref(b, a))  # the partition runs over b's slots now


@pytest.mark.parametrize("n_docs", [K_SCAN - 1, K_SCAN, K_SCAN + 1])
def test_scan_chunk_edges(eng, torch, n_docs):
    """Tiny documents around one step of the single-workgroup worklist scan."""
    rng = np.random.default_rng(9200 + n_docs)
    cnt = rng.integers(0, 2, n_docs).astype(U32)
    off = np.zeros(n_docs + 1, U32)
    np.cumsum(cnt, out=off[1:])
    tot = int(off[-1])
    keys = np.arange(tot, dtype=U64) * U64(2)
    vv = np.ones(2 * n_docs, U64)
    a = AWSetBatch(2, off, keys, np.zeros(tot, U32), np.ones(tot, U64), vv)
    bk, bvv = keys.copy(), vv.copy()
    bk[rng.integers(0, tot, 300)] += U64(1)
    bvv[rng.integers(0, 2 * n_docs, 300)] += U64(1)
    bvv[2 * (n_docs - 1) + 1] += U64(1)  # the very last clock word
    b = AWSetBatch(2, off, bk, a.actors, a.counters, bvv)
    want = compare_ref(a, b)
    assert want[0][-1] & B_AHEAD
    assert_cmp(cmp_on_device(eng, torch, a, b), want)


# ------------------------------------------------------------------ 4. clocks

@pytest.mark.parametrize("R", [1, 3, 64])
def test_clock_widths(eng, torch, R):
    rng = random.Random(9300 + R)
    n = 300
    da, db = [], []
    for d in range(n):
        doc = _rand_doc(rng, R, rng.choice((0, 1, 5)))
        va, vb = list(doc[3]), list(doc[3])
        m = d % 4
        if m == 1:  # differ only in word R-1
            vb[R - 1] += 1
        elif m == 2:
            va[R - 1] += 1
        elif m == 3 and R > 1:  # concurrent: each side ahead in one word
            va[0] += 1
            vb[R - 1] += 1
        da.append((doc[0], doc[1], doc[2], va))
        db.append((doc[0], doc[1], doc[2], vb))
    a, b = pack(R, da), pack(R, db, slack=1)
    want = compare_ref(a, b)
    assert (want[0] & KEYS).sum() == 0
    assert set(want[0].tolist()) == ({0, A_AHEAD, B_AHEAD, A_AHEAD | B_AHEAD} if R > 1 else {0, A_AHEAD, B_AHEAD})
    assert_cmp(cmp_on_device(eng, torch, a, b), want)


# ------------------------------------------------------------------- 5. masks

@pytest.mark.parametrize("mask", [0, 1, 2, 4, 8, 15])
def test_masks(eng, torch, mask):
    a, b, want15, _ = small_case(3, 1)
    want = compare_ref(a, b, mask)
    assert (want[0] == want15[0]).all()
    got = cmp_on_device(eng, torch, a, b, mask=mask)
    assert_cmp(got, want)
    flags, summary, work = got
    assert int(summary[4]) == len(work) == int(((flags & mask) != 0).sum())
    assert (np.diff(work.astype(np.int64)) > 0).all()
    assert (len(work) == 0) == (mask == 0)


def test_optional_outputs(eng, torch):
    a, b, want, _ = small_case(0, 1)
    got = cmp_on_device(eng, torch, a, b, worklist=False)
    assert got[2] is None
    assert_cmp(got, want)
    got = cmp_on_device(eng, torch, a, b, summary=False)
    assert got[1] is None
    assert_cmp(got, want)
    got = cmp_on_device(eng, torch, a, b, worklist=False, summary=False)
    assert got[1] is None and got[2] is None
    assert_cmp(got, want)


# ------------------------------------------------- 6. an exchange's two outputs

_xchg = {}


def xchg_case():
    if not _xchg:
        rng = random.Random(9400)
        R, n, universe = 3, 600, 50
        a = batch_of(R, [random_state(rng, R, rng.randint(0, 40), universe, 30) for _ in range(n)])
        b = batch_of(R, [random_state(rng, R, rng.randint(0, 40), universe, 30) for _ in range(n)])
        rc1, ab = oracle.join(a, b)
        rc2, ba = oracle.join(b, a)
        assert rc1 == 0 and rc2 == 0
        _xchg.update(R=R, n=n, a=a, b=b, ab=ab, ba=ba, slots=int(a.offsets[-1]) + int(b.offsets[-1]))
    return _xchg


def test_exchange_outputs_compared_in_place(eng, torch):
    """out_ab against out_ba straight from the crdt_awset_out arrays (capacity
    offsets, zero-padded slack), no host round trip between the two calls."""
    c = xchg_case()
    dev = dev_of(torch)
    o1 = OutBuffers(c["n"], c["R"], c["slots"], device=dev)
    o2 = OutBuffers(c["n"], c["R"], c["slots"], device=dev)
    res = poisoned_cmp(torch, c["n"])
    eng.exchange_async(c["a"].to(dev), c["b"].to(dev), o1, o2)
    eng.compare_async(o1.as_batch(), o2.as_batch(), res)
    eng.sync()
    want = compare_ref(c["ab"].as_batch(), c["ba"].as_batch())
    assert not (want[0] & KEYS).any() and (want[0] & DOTS).any()
    assert_cmp(read_cmp(res), want)


# ------------------------------------------------------------------ 7. select

def test_identity_select_compacts_a_join_output(eng, torch):
    c = xchg_case()
    dev = dev_of(torch)
    n, R = c["n"], c["R"]
    joined = OutBuffers(n, R, c["slots"], device=dev)
    want = select_ref(c["ab"].as_batch())
    total = int(want.offsets[-1])
    assert 0 < total < c["slots"]
    packed = poisoned_out(torch, n, R, total + 9)
    res = poisoned_cmp(torch, n)
    eng.join_async(c["a"].to(dev), c["b"].to(dev), joined)
    eng.select_async(joined.as_batch(), packed)
    eng.compare_async(packed.as_batch(), joined.as_batch(), res)
    eng.sync()
    assert_packed(packed, want)
    flags, summary, work = read_cmp(res)
    assert not flags.any() and not summary.any() and len(work) == 0


@pytest.mark.parametrize("extra", [0, 5])
def test_worklist_feeds_select_on_the_device(eng, torch, extra):
    """compare -> select with the worklist and n_work left on the device; n_out is
    the worklist's length (extra 0) or more (trailing documents empty, VV zero)."""
    a, b, want, _ = small_case(3, 1)
    dev = dev_of(torch)
    ad = a.to(dev)
    n_out = len(want[2]) + extra
    sel_want = select_ref(a, want[2], n_idx=len(want[2]), n_out=n_out)
    res = poisoned_cmp(torch, a.n_docs)
    out = poisoned_out(torch, n_out, a.R, int(sel_want.offsets[-1]) + 4)
    eng.compare_async(ad, b.to(dev), res)
    eng.select_async(ad, out, idx=res.worklist, n_idx=res.n_work)
    eng.sync()
    assert_cmp(read_cmp(res), want)
    h = assert_packed(out, sel_want)
    if extra:
        assert not h.counts[n_out - extra:n_out].any() and not h.vv[(n_out - extra) * a.R:n_out * a.R].any()


def test_select_any_order_and_repeats(eng, torch):
    a, _, _, _ = small_case(3, 1)
    dev = dev_of(torch)
    rng = np.random.default_rng(9500)
    idx = np.concatenate([np.arange(a.n_docs - 1, a.n_docs - 400, -1), rng.integers(0, a.n_docs, 300),
                          np.array([7, 7, 7, 0, a.n_docs - 1])]).astype(U32)
    want = select_ref(a, idx, n_out=len(idx))
    out = poisoned_out(torch, len(idx), a.R, int(want.offsets[-1]) + 3)
    eng.select_async(a.to(dev), out, idx=torch.from_numpy(idx.view(np.int32)).to(dev))
    eng.sync()
    assert_packed(out, want)


def test_select_gather_chunk_edges(eng, torch):
    """2,047 one-entry documents (more than kSelRun stages), then a document of
    2,050 entries that starts on a gather chunk's last output position and spans
    three chunks, then one-entry documents again; the state holds them in another
    order and with slack, so source runs start at odd slots."""
    big = _seq_doc(7, K_CHUNK + 2)
    docs = [big] + [([10 * i + 1], [i % 2], [i + 1], [i, 1]) for i in range(K_CHUNK + 40)]
    state = pack(2, docs, slack=1, garbage=np.random.default_rng(4))
    idx = np.array(list(range(1, K_CHUNK)) + [0] + list(range(K_CHUNK, K_CHUNK + 41)), U32)
    want = select_ref(state, idx, n_out=len(idx))
    assert int(want.offsets[K_CHUNK - 1]) == K_CHUNK - 1 and int(want.counts[K_CHUNK - 1]) == K_CHUNK + 2
    dev = dev_of(torch)
    out = poisoned_out(torch, len(idx), 2, int(want.offsets[-1]) + 5)
    eng.select_async(state.to(dev), out, idx=torch.from_numpy(idx.view(np.int32)).to(dev))
    eng.sync()
    assert_packed(out, want)
    # the same at zero slack, identity: aligned pairs on both sides
    st0 = pack(2, [docs[i] for i in idx.tolist()])
    out = poisoned_out(torch, st0.n_docs, 2, int(want.offsets[-1]))
    eng.select_async(st0.to(dev), out)
    eng.sync()
    assert_packed(out, want)


@pytest.mark.parametrize("n_docs", [K_SCAN - 1, K_SCAN + 1])
def test_select_scan_chunk_edges(eng, torch, n_docs):
    rng = np.random.default_rng(9600 + n_docs)
    cnt = rng.integers(0, 3, n_docs).astype(U32)
    off = np.zeros(n_docs + 1, U32)
    np.cumsum(cnt + U32(1), out=off[1:])
    tot = int(off[-1])
    state = AWSetBatch(2, off, rng.integers(0, 2 ** 63, tot, dtype=np.int64).view(U64),
                       rng.integers(0, 2, tot, dtype=np.int64).astype(U32),
                       rng.integers(1, 2 ** 40, tot, dtype=np.int64).view(U64),
                       rng.integers(0, 99, 2 * n_docs, dtype=np.int64).view(U64), counts=cnt)
    want = select_ref(state)
    out = poisoned_out(torch, n_docs, 2, int(want.offsets[-1]) + 2)
    eng.select_async(state.to(dev_of(torch)), out)
    eng.sync()
    assert_packed(out, want)


def test_select_output_is_a_join_input(eng, torch):
    c = xchg_case()
    dev = dev_of(torch)
    n, R = c["n"], c["R"]
    rng = np.random.default_rng(9700)
    idx = rng.permutation(n)[:250].astype(U32)
    sub_a, sub_b = select_ref(c["a"], idx, n_out=250), select_ref(c["b"], idx, n_out=250)
    rc, want = oracle.join(sub_a, sub_b)
    assert rc == 0
    d_idx = torch.from_numpy(idx.view(np.int32)).to(dev)
    sa = OutBuffers(250, R, int(sub_a.offsets[-1]), device=dev)
    sb = OutBuffers(250, R, int(sub_b.offsets[-1]), device=dev)
    joined = OutBuffers(250, R, sa.slots + sb.slots, device=dev)
    eng.select_async(c["a"].to(dev), sa, idx=d_idx)
    eng.select_async(c["b"].to(dev), sb, idx=d_idx)
    eng.join_async(sa.as_batch(), sb.as_batch(), joined)
    eng.sync()
    got = host_out(joined)
    assert (got.offsets[:251] == want.offsets[:251]).all() and (got.counts[:250] == want.counts[:250]).all()
    assert (got.vv[:250 * R] == want.vv[:250 * R]).all()
    assert not compare_ref(got.as_batch(), want.as_batch())[0].any()


# ------------------------------------------------------------------ 8. errors

def _code(fn):
    with pytest.raises(crdtgpu.CrdtError) as ei:
        fn()
    return ei.value.code


def test_compare_argument_errors(eng, torch):
    """Every one of these is refused on the host: nothing is launched."""
    dev = dev_of(torch)
    a = batch_of(2, [([(1, 0, 1), (4, 1, 2)], [1, 2]), ([(3, 0, 1)], [1, 0])]).to(dev)
    a3 = batch_of(2, [([(1, 0, 1)], [1, 2])] * 3).to(dev)
    aR = batch_of(3, [([(1, 0, 1), (4, 1, 2)], [1, 2, 0]), ([(3, 0, 1)], [1, 0, 0])]).to(dev)
    out = poisoned_cmp(torch, 2)
    lib, ctx, ref = abi.lib(), eng._ctx, ctypes.byref

    def call(ca, cb, co, mask=15):
        return lib.crdt_awset_compare_async(ctx, ref(ca) if ca else None, ref(cb) if cb else None, mask,
                                            ref(co) if co else None, None)

    assert call(None, a.c(), out.c()) == crdtgpu.CRDT_E_INVALID
    assert call(a.c(), None, out.c()) == crdtgpu.CRDT_E_INVALID
    assert call(a.c(), a.c(), None) == crdtgpu.CRDT_E_INVALID
    assert call(a.c(), a3.c(), out.c()) == crdtgpu.CRDT_E_INVALID  # n_docs
    assert call(a.c(), aR.c(), out.c()) == crdtgpu.CRDT_E_INVALID  # R
    assert call(a.c(), a.c(), out.c(), 16) == crdtgpu.CRDT_E_INVALID
    for field in ("flags", "worklist", "n_work"):
        co = out.c()
        setattr(co, field, None)
        assert call(a.c(), a.c(), co) == crdtgpu.CRDT_E_INVALID, field
    ca = a.c()
    ca.R = 65
    assert call(ca, ca, out.c()) == crdtgpu.CRDT_E_INVALID
    eng.sync()
    assert (out.flags.cpu().numpy() == 77).all() and (out.summary.cpu().numpy().view(U32) == ONES32).all()
    assert (out.worklist.cpu().numpy().view(U32) == ONES32).all() and int(out.n_work.cpu().numpy().view(U32)[0]) == ONES32
    eng.compare_async(a, a, out)  # and the call still works
    eng.sync()
    assert_cmp(read_cmp(out), (np.zeros(2, U8), np.zeros(5, U32), np.zeros(0, U32)))


def test_count_above_slots_is_clamped(eng, torch):
    a = batch_of(2, [([(1, 0, 1), (4, 1, 2)], [1, 2]), ([(3, 0, 1)], [1, 0]), ([(9, 0, 1)], [0, 0])], slack=1)
    b = batch_of(2, [([(1, 0, 1), (4, 1, 2)], [1, 2]), ([(3, 0, 1)], [1, 0]), ([(9, 0, 1)], [0, 0])], slack=1)
    a.keys[int(a.offsets[1]) + 1] = 77  # doc 1's slack slot: live once the count says 2
    b.keys[int(b.offsets[1]) + 1] = 78
    a.counts[1] = 9
    b.counts[1] = 9
    out = poisoned_cmp(torch, 3)
    eng.compare_async(a.to(dev_of(torch)), b.to(dev_of(torch)), out)
    assert _code(eng.sync) == crdtgpu.CRDT_E_CAPACITY
    flags, summary, work = read_cmp(out)  # clamped to the two slots: the second differs
    assert flags.tolist() == [0, KEYS, 0] and work.tolist() == [1] and summary.tolist() == [1, 0, 0, 0, 1]
    eng.sync()  # cleared


def test_select_errors(eng, torch):
    dev = dev_of(torch)
    a, _, _, _ = small_case(3, 1)
    ad = a.to(dev)
    n = a.n_docs
    # an index that is no document: CRDT_E_INVALID at sync, that document empty, the others exact
    idx = np.array([4, n, 6, 2 ** 32 - 1, 8], U32)
    want = select_ref(a, idx, n_out=5)
    assert int(want.counts[1]) == 0 and int(want.counts[3]) == 0
    out = poisoned_out(torch, 5, a.R, int(want.offsets[-1]) + 3)
    eng.select_async(ad, out, idx=torch.from_numpy(idx.view(np.int32)).to(dev))
    assert _code(eng.sync) == crdtgpu.CRDT_E_INVALID
    assert_packed(out, want)
    # *n_idx > n_out: clamped, CRDT_E_CAPACITY
    idx = np.arange(10, 30, dtype=U32)
    want = select_ref(a, idx, n_out=8)
    out = poisoned_out(torch, 8, a.R, int(want.offsets[-1]) + 3)
    eng.select_async(ad, out, idx=torch.from_numpy(idx.view(np.int32)).to(dev),
                     n_idx=torch.tensor([20], dtype=torch.int32, device=dev))
    assert _code(eng.sync) == crdtgpu.CRDT_E_CAPACITY
    assert_packed(out, want)
    # more live entries than out_slots: CRDT_E_CAPACITY, nothing at or past out_slots
    want = select_ref(a)
    total = int(want.offsets[-1])
    out = poisoned_out(torch, n, a.R, total)
    cut = total - 777
    eng.select_async(ad, out, out_slots=cut)
    assert _code(eng.sync) == crdtgpu.CRDT_E_CAPACITY
    h = host_out(out)
    assert (h.keys[cut:total] == MAXK).all() and (h.counters[cut:total] == MAXK).all()
    assert (h.actors[cut:total] == ONES32).all()
    assert (h.keys[:cut] == want.keys[:cut]).all()
    # a count above its slots: clamped, CRDT_E_CAPACITY
    over = batch_of(2, [([(1, 0, 1)], [1, 0]), ([(3, 0, 1)], [1, 0])], slack=1)
    over.counts[1] = 5
    out = poisoned_out(torch, 2, 2, 8)
    eng.select_async(over.to(dev), out)
    assert _code(eng.sync) == crdtgpu.CRDT_E_CAPACITY
    h = host_out(out)
    assert h.offsets[:3].tolist() == [0, 1, 3] and h.counts[:2].tolist() == [1, 2] and (h.keys[3:8] == MAXK).all()
    # aliasing and NULL arguments: refused by the call
    co = out.c()
    co.keys = ad.keys.data_ptr()
    lib, ref = abi.lib(), ctypes.byref
    cs = ad.c()
    assert lib.crdt_awset_select_async(eng._ctx, ref(cs), None, None, 2, 8, ref(co), None) == crdtgpu.CRDT_E_INVALID
    assert lib.crdt_awset_select_async(eng._ctx, None, None, None, 2, 8, ref(out.c()), None) == crdtgpu.CRDT_E_INVALID
    assert lib.crdt_awset_select_async(eng._ctx, ref(cs), None, None, 2, 8, None, None) == crdtgpu.CRDT_E_INVALID
    eng.sync()


def test_host_form(eng, torch):
    for slack, with_counts in LAYOUTS:
        a, b, want, _ = small_case(slack, with_counts)
        assert_cmp(eng.compare(a, b), want)
    a, b, _, _ = small_case(3, 1)
    assert_cmp(eng.compare(a, b, mask=DOTS), compare_ref(a, b, DOTS))
    good = batch_of(2, [([(1, 0, 1), (4, 1, 2)], [1, 2]), ([(3, 0, 1)], [1, 0]), ([], [0, 0])])
    unsorted = batch_of(2, [([(4, 0, 1), (1, 1, 2)], [1, 2]), ([(3, 0, 1)], [1, 0]), ([], [0, 0])])
    out = CompareBuffers(3)
    out.flags[:] = 77
    out.summary[:] = ONES32
    out.worklist[:] = ONES32
    out.n_work[:] = ONES32
    ca, cb, co = good.c(), unsorted.c(), out.c()
    rc = abi.lib().crdt_awset_compare_batch(eng._ctx, ctypes.byref(ca), ctypes.byref(cb), 15, ctypes.byref(co))
    assert rc == crdtgpu.CRDT_E_UNSORTED
    assert (out.flags == 77).all() and (out.summary == ONES32).all() and (out.worklist == ONES32).all()
    assert int(out.n_work[0]) == ONES32  # outputs untouched
    over = batch_of(2, [([(1, 0, 1)], [1, 0]), ([(3, 0, 1)], [1, 0]), ([], [0, 0])], slack=1)
    over.counts[1] = 5
    assert _code(lambda: eng.compare(good, over)) == crdtgpu.CRDT_E_CAPACITY
    assert _code(lambda: eng.compare(good, batch_of(2, [([], [0, 0])]))) == crdtgpu.CRDT_E_INVALID
    flags, summary, work = eng.compare(good, good)  # the context is still usable
    assert not flags.any() and not summary.any() and len(work) == 0


# ---------------------------------------------------------------- 9. plumbing

def test_no_documents(eng, torch):
    dev = dev_of(torch)
    z = lambda dt: torch.zeros(1, dtype=dt, device=dev)  # noqa: E731
    e = AWSetBatch(2, z(torch.int32), z(torch.int64), z(torch.int32), z(torch.int64), z(torch.int64))
    assert e.n_docs == 0
    out = poisoned_cmp(torch, 0)
    eng.compare_async(e, e, out)
    eng.sync()
    assert (out.summary.cpu().numpy() == 0).all() and int(out.n_work.cpu().numpy()[0]) == 0
    assert int(out.flags.cpu().numpy()[0]) == 77 and int(out.worklist.cpu().numpy().view(U32)[0]) == ONES32
    sel = poisoned_out(torch, 1, 2, 4)
    eng.select_async(e, sel, n_out=0)
    eng.sync()
    assert int(sel.offsets.cpu().numpy()[0]) == 0 and (sel.keys.cpu().numpy().view(U64) == MAXK).all()
    flags, summary, work = eng.compare(e.numpy(), e.numpy())
    assert len(flags) == 0 and not summary.any() and len(work) == 0


def test_ordered_after_an_exchange_on_another_stream(eng, torch):
    c = xchg_case()
    dev = dev_of(torch)
    o1 = OutBuffers(c["n"], c["R"], c["slots"], device=dev)
    o2 = OutBuffers(c["n"], c["R"], c["slots"], device=dev)
    for o in (o1, o2):
        for t in (o.offsets, o.counts, o.keys, o.actors, o.counters, o.vv):
            t.zero_()  # a compare that ran before the exchange would see two empty batches
    da, db = c["a"].to(dev), c["b"].to(dev)
    res = poisoned_cmp(torch, c["n"])
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.exchange_async(da, db, o1, o2, stream=sa)
    eng.compare_async(o1.as_batch(), o2.as_batch(), res, stream=sb)
    eng.sync(sb)
    assert_cmp(read_cmp(res), compare_ref(c["ab"].as_batch(), c["ba"].as_batch()))


def test_graph_capture(torch):
    """compare + select captured on a reserved context, replayed twice with the
    inputs changed in between, equal to eager; on an unreserved context the
    capture is refused with CRDT_E_WORKSPACE and launches nothing."""
    a, b, want, _ = small_case(3, 1)
    b2 = AWSetBatch(b.R, b.offsets, b.keys.copy(), b.actors.copy(), b.counters.copy(), b.vv.copy(), counts=b.counts)
    for d in range(0, b.n_docs, 5):  # other documents differ now
        o, n = int(b.offsets[d]), int(b.counts[d])
        ao = int(a.offsets[d])
        if int(a.counts[d]) == n:
            b2.keys[o:o + n], b2.actors[o:o + n], b2.counters[o:o + n] = (
                a.keys[ao:ao + n], a.actors[ao:ao + n], a.counters[ao:ao + n])
        b2.vv[d * b.R:(d + 1) * b.R] = a.vv[d * a.R:(d + 1) * a.R]
    want2 = compare_ref(a, b2)
    assert len(want2[2]) != len(want[2])
    dev = dev_of(torch)
    n = a.n_docs
    assert n > 1024  # (a fresh context's workspace holds 1,024 documents)
    e = crdtgpu.Engine(0)
    try:
        ad, bd = a.to(dev), b.to(dev)
        res = poisoned_cmp(torch, n)
        sel = poisoned_out(torch, n, a.R, int(a.offsets[-1]))
        g0 = torch.cuda.CUDAGraph()
        with pytest.raises(crdtgpu.CrdtError) as ei:
            with torch.cuda.graph(g0):
                e.compare_async(ad, bd, res, stream=torch.cuda.current_stream())
        assert ei.value.code == crdtgpu.CRDT_E_WORKSPACE
        torch.cuda.synchronize()
        assert (res.flags.cpu().numpy() == 77).all() and int(res.n_work.cpu().numpy().view(U32)[0]) == ONES32
        e.reserve(n)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.compare_async(ad, bd, res, stream=torch.cuda.current_stream())
            e.select_async(ad, sel, idx=res.worklist, n_idx=res.n_work, stream=torch.cuda.current_stream())
        for src, w in ((b, want), (b2, want2), (b, want)):
            for f in ("keys", "actors", "counters", "vv"):
                getattr(bd, f).copy_(getattr(src.to(dev), f))
            res.flags.fill_(77)
            for t in (res.summary, res.worklist, res.n_work, sel.offsets, sel.counts, sel.keys, sel.actors,
                      sel.counters, sel.vv):
                t.fill_(-1)
            g.replay()
            e.sync(torch.cuda.current_stream())
            assert_cmp(read_cmp(res), w)
            assert_packed(sel, select_ref(a, w[2], n_idx=len(w[2]), n_out=n))
    finally:
        e.close()
