"""GPU: the opt-in tombstone GC (crdt_tombstone_gc_async; the reference's
gcDeleted is an empty stub, awset-delta_test.go:67-77) and the elementwise
u64 min that computes a causally stable clock (crdt_vv_min_async), against the
C oracle (oracle_tomb_gc) and numpy.  The rule has no reference output to pin
it: parity here is with the restated rule (keep (k, x) unless
stable.HasDot(x), actor >= R kept)."""

import random

import numpy as np
import pytest

import crdtgpu
from apply_cases import tomb_batch
from crdtgpu.batch import TombBatch, TombBuffers
from oracle import oracle

pytestmark = pytest.mark.gpu


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


def _i64(a, torch, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)


def test_vv_min(eng, torch):
    rng = np.random.default_rng(1)
    a = rng.integers(0, 2**64 - 1, 100_003, dtype=np.uint64)
    b = rng.integers(0, 2**64 - 1, 100_003, dtype=np.uint64)
    a[5], b[5] = np.uint64(2**63), np.uint64(2**63 - 1)  # unsigned order, not signed
    dev = torch.device("cuda:0")
    da, db = _i64(a, torch, dev), _i64(b, torch, dev)
    eng.vv_min_async(da, db, a.size)
    eng.sync()
    assert (da.cpu().numpy().view(np.uint64) == np.minimum(a, b)).all()


def gc_case(R, n=4000):
    """(tombstones per doc, stable clocks [n * R]): lists of 0 ... 300 tombstones, actors up to R + 1."""
    rng = random.Random(R)
    per_doc = []
    for _ in range(n):
        keys = sorted(rng.sample(range(10 ** 6), rng.choice([0, 1, 3, 63, 64, 65, 300])))
        per_doc.append([(k, rng.randrange(R + 2), rng.randint(1, 50)) for k in keys])  # actors >= R kept
    stable = np.array([rng.randint(0, 50) for _ in range(n * R)], dtype=np.uint64)
    return per_doc, stable


def gc_on_gpu(eng, torch, tb, R, stable):
    """crdt_tombstone_gc_async on device copies; the output as a host TombBatch."""
    dev = torch.device("cuda:0")
    n = tb.n_docs
    out = TombBuffers(n, int(tb.offsets[-1]), device=dev)
    eng.tombstone_gc_async(tb.to(dev), R, _i64(stable, torch, dev), out)
    eng.sync()
    return TombBatch(*(t.cpu().numpy().view(np.uint32 if t.dtype == torch.int32 else np.uint64)
                       for t in (out.offsets, out.keys, out.actors, out.counters)),
                     counts=out.counts.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("R", [2, 8, 64])
def test_tombstone_gc_matches_oracle(eng, torch, R):
    n = 4000
    per_doc, stable = gc_case(R, n)
    tb = TombBatch.from_lists(per_doc)
    rc, want = oracle.tomb_gc(tb, R, stable)
    assert rc == 0
    got = gc_on_gpu(eng, torch, tb, R, stable)
    assert (got.offsets == want.offsets).all()
    for d in range(n):
        assert got.doc(d) == want.doc(d), d
    # the rule itself, restated in numpy for a few docs
    for d in range(0, n, 397):
        keep = [(k, a, c) for k, a, c in per_doc[d] if not (a < R and stable[d * R + a] >= c)]
        assert want.doc(d) == keep


# ---- deterministic lists on the kernel's edges (tomb_gc_kernel, csrc/apply.hip: one
# wavefront per document, 64 tombstones per step, four documents per workgroup), into
# poisoned outputs

GC_LENGTHS = (0, 1, 63, 64, 65, 128, 129)
GC_VARIANTS = ("all_kept", "all_dropped", "alternating", "first_kept", "last_kept")
P32, P64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


def gc_stable(R):
    return [10 + a for a in range(R)]


def gc_list(R, n, variant):
    """(tombstones, the ones kept) of one document under the clock gc_stable(R).  A dropped
    tombstone has actor a < R and counter stable[a] (covered at equality) or below it; a kept
    one has counter stable[a] + 1, or actor R or R + 1 under a counter any clock would cover."""
    stable = gc_stable(R)
    keep = {"all_kept": lambda i: True, "all_dropped": lambda i: False, "alternating": lambda i: i % 2 == 0,
            "first_kept": lambda i: i == 0, "last_kept": lambda i: i == n - 1}[variant]
    tombs, kept = [], []
    for i in range(n):
        a = i % R
        if keep(i):
            t = ((7 * i + 3, a, stable[a] + 1), (7 * i + 3, R, 1), (7 * i + 3, R + 1, 1))[(i // 2) % 3]
            kept.append(t)
        else:
            t = (7 * i + 3, a, stable[a] - 3 * (i % 4 == 1))
        tombs.append(t)
    return tombs, kept


def gc_into_poison(eng, torch, lists, R, stable, slack=0):
    """GC on the device into poisoned buffers: offsets and counts whole, the kept prefix of
    every document equal to the oracle's, every slot past counts[d] still poison."""
    tb = tomb_batch(lists, slack)
    n, slots = tb.n_docs, int(tb.offsets[-1])
    rc, want = oracle.tomb_gc(tb, R, stable)
    assert rc == 0
    dev = torch.device("cuda:0")
    out = TombBuffers(n, slots, device=dev)
    for t in (out.offsets, out.counts, out.keys, out.actors, out.counters):
        t.fill_(P32 if t.dtype == torch.int32 else P64)
    eng.tombstone_gc_async(tb.to(dev), R, _i64(stable, torch, dev), out)
    eng.sync()
    got = {f: getattr(out, f).cpu().numpy() for f in ("offsets", "counts", "keys", "actors", "counters")}
    got = {f: a.view(np.uint32 if a.dtype == np.int32 else np.uint64) for f, a in got.items()}
    assert (got["offsets"][: n + 1] == tb.offsets).all() and (got["counts"][:n] == want.counts).all()
    live = np.zeros(slots, bool)
    for d in range(n):
        o = int(tb.offsets[d])
        live[o:o + int(want.counts[d])] = True
    for f, p in (("keys", P64), ("actors", P32), ("counters", P64)):
        exp = np.where(live, getattr(want, f)[:slots], p)
        bad = np.flatnonzero(got[f][:slots] != exp)
        assert bad.size == 0, (f, int(bad[0]))
    return want


@pytest.mark.parametrize("slack", [0, 2])
@pytest.mark.parametrize("R", [2, 8])
def test_tombstone_gc_edge_lists(eng, torch, R, slack):
    """Every length in every variant in one batch, packed and with counts and stale slack."""
    made = [gc_list(R, n, v) for n in GC_LENGTHS for v in GC_VARIANTS]
    lists, kept = [m[0] for m in made], [m[1] for m in made]
    for (n, v), k in zip(((n, v) for n in GC_LENGTHS for v in GC_VARIANTS), kept):
        assert len(k) == {"all_kept": n, "all_dropped": 0, "alternating": (n + 1) // 2}.get(v, min(n, 1)), (n, v)
    actors = {t[1] for k in kept for t in k}
    assert {R, R + 1} <= actors and min(actors) < R
    stable = np.array(gc_stable(R) * len(lists), dtype=np.uint64)
    want = gc_into_poison(eng, torch, lists, R, stable, slack)
    for d, k in enumerate(kept):  # the oracle keeps what the lists were built to keep
        assert want.doc(d) == k, d


@pytest.mark.parametrize("n_docs", [1, 5])
def test_tombstone_gc_document_counts(eng, torch, n_docs):
    R = 3
    made = [gc_list(R, 65, "alternating")] if n_docs == 1 else [gc_list(R, 129, v) for v in GC_VARIANTS]
    stable = np.array(gc_stable(R) * n_docs, dtype=np.uint64)
    want = gc_into_poison(eng, torch, [m[0] for m in made], R, stable, slack=1)
    assert [want.doc(d) for d in range(n_docs)] == [m[1] for m in made]


def test_tombstone_gc_more_documents_than_waves(eng, torch):
    """More than 4 * 16 * CUs tiny documents: every wavefront takes a second document."""
    R = 2
    n = 4 * 16 * torch.cuda.get_device_properties(0).multi_processor_count + 5
    shapes = [gc_list(R, m, v) for m in (0, 1, 2, 3) for v in ("all_kept", "alternating", "last_kept", "all_dropped")]
    made = [shapes[(d * 5) % len(shapes)] for d in range(n)]
    stable = np.array(gc_stable(R) * n, dtype=np.uint64)
    want = gc_into_poison(eng, torch, [m[0] for m in made], R, stable)
    for d in range(0, n, 97):
        assert want.doc(d) == made[d][1], d
    assert (np.asarray(want.counts) == np.array([len(m[1]) for m in made], np.uint32)).all()
