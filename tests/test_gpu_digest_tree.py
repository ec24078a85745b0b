"""GPU: the digest tree (csrc/digest_tree.hip) against crdt_digest_tree_host and the
numpy restatement of tests/test_digest_tree_model.py, bit-exact.

Build: every layout of the model file into a sentinel tree array with guard words,
aligned and one u64 past a 16 B boundary.  Children and diff: the list forms, the
error table, the scan's chunk edges.  Descent: whole descents chained on the device
with nothing downloaded between levels, against crdt_digest_diff_async, feeding
crdt_awset_select_async.  Then run-to-run identity, graph capture and replay, the
workspace refusal and two streams.
"""

import numpy as np
import pytest

import crdtgpu
from crdtgpu import CRDT_E_CAPACITY, CRDT_E_INVALID, CRDT_E_WORKSPACE, abi
from crdtgpu.batch import AWSetBatch, CompareBuffers, DigestTreeBuffers, OutBuffers, _np
from test_digest_tree_model import (LAYOUTS, children_ref, diff_ref, differing, flat_ref, levels_of, random_digest,
                                    tree_ref)

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64
GUARD = 6
CHUNK = 64  # listed parents per scan chunk (digest_tree.hip, kTreeChunk)


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


def sentinel(n_words):
    """A different value in every word, none of them a plausible hash of the test data."""
    return (np.arange(n_words, dtype=U64) * U64(0x9E3779B1) + U64(0x5EAD00000000BEEF))


def guarded(torch, values, shift=False):
    """(view, whole): `values` (u64) on the device between GUARD sentinel words on each
    side; shift: the view starts one u64 past a 16 B boundary."""
    values = np.ascontiguousarray(values, U64).reshape(-1)
    before = GUARD + (1 if shift else 0)
    whole = sentinel(before + len(values) + GUARD) ^ U64(0xFFFF)
    whole[before: before + len(values)] = values
    t = torch.from_numpy(whole.view(np.int64).copy()).to(dev_of(torch))
    view = t[before: before + len(values)]
    assert t.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (8 if shift else 0)
    return view, t, whole, before


def guards_intact(t, whole, before, n):
    h = _np(t, U64)
    return (h[:before] == whole[:before]).all() and (h[before + n:] == whole[before + n:]).all()


def dev64(torch, a, shift=False):
    return guarded(torch, a, shift)[0]


def dev32(torch, a):
    a = np.ascontiguousarray(a, U32).reshape(-1)
    t = torch.from_numpy(a.view(np.int32).copy()).to(dev_of(torch))
    return t if t.numel() else torch.zeros(1, dtype=torch.int32, device=dev_of(torch))


def code_of(fn):
    with pytest.raises(crdtgpu.CrdtError) as ei:
        fn()
    return ei.value.code


# ------------------------------------------------------------------- 1. build

@pytest.mark.parametrize("shift", (False, True))
@pytest.mark.parametrize("n", LAYOUTS)
def test_build(eng, torch, n, shift):
    digest = random_digest(n, 7 + n)
    want = crdtgpu.digest_tree_host(digest)
    assert (want == tree_ref(digest)).all()
    d = dev64(torch, digest if n else np.zeros(2, U64), shift)
    n_words = max(2 * len(want), 2)
    tree, whole, host, before = guarded(torch, sentinel(n_words), shift)
    eng.digest_tree_async(d, n, tree)
    eng.sync()
    got = _np(whole, U64)[before: before + n_words]
    if n == 0:
        assert (got == sentinel(n_words)).all()  # nothing launched
    else:
        got = got.reshape(-1, 2)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, "node %d of %d: gpu %s, host %s" % (bad[0], len(want), got[bad[0]], want[bad[0]])
    assert guards_intact(whole, host, before, n_words)


def test_build_unfused_is_the_same_tree(torch):
    """crdt_ctx_set_option("digest_tree_fuse", 0): one launch per level up to the root."""
    e = crdtgpu.Engine(0)
    try:
        e.set_option("digest_tree_fuse", 0)
        for n in (1, 17, 4097, 65537):
            digest = random_digest(n, n)
            assert (e.digest_tree(digest) == crdtgpu.digest_tree_host(digest)).all()
    finally:
        e.close()


# ---------------------------------------------------------------- 2. children

N = 4097
_cache = {}


def pair(n=N, docs=None, seed=41):
    """(mine, theirs, mine levels, their levels) of two digest arrays, computed once."""
    key = (n, tuple(docs) if docs is not None else None, seed)
    if key not in _cache:
        if docs is None:
            rng = np.random.default_rng(seed)
            docs = sorted(rng.choice(n, size=max(1, n // 7), replace=False).tolist())
        mine, theirs = differing(n, docs, seed)
        _cache[key] = (mine, theirs, levels_of(mine, tree_ref(mine)), levels_of(theirs, tree_ref(theirs)))
    return _cache[key]


def run_children(eng, torch, level, parents, n_parents, n_max, shift=False):
    """(packed [16 * n_max, 2], tail words past it) after one call into a sentinel array."""
    n_words = 32 * n_max + 8
    out, whole, host, before = guarded(torch, sentinel(n_words), shift)
    lv = dev64(torch, level, shift)
    eng.digest_tree_children_async(lv, len(level), out, parents=None if parents is None else dev32(torch, parents),
                                   n_parents=None if n_parents is None else dev32(torch, [n_parents]), n_max=n_max)
    return out, whole, host, before, n_words


CHILD_LISTS = {
    "empty": ([3, 4, 5, 6], 0, 4),
    "one": ([7], None, 1),
    "partial_last": ([256], None, 1),
    "identity": (None, None, 257),
    "identity_prefix": (None, 5, 257),
    "any_order": ([5, 0, 256, 3, 3, 200], None, 6),
    "fewer_than_room": ([9, 8, 7, 6], 2, 4),
}


@pytest.mark.parametrize("shift", (False, True))
@pytest.mark.parametrize("name", sorted(CHILD_LISTS))
def test_children_lists(eng, torch, name, shift):
    parents, n_parents, n_max = CHILD_LISTS[name]
    level = pair()[2][0]
    out, whole, host, before, n_words = run_children(eng, torch, level, parents, n_parents, n_max, shift)
    eng.sync()
    got = _np(whole, U64)[before: before + n_words]
    k = n_max if n_parents is None else min(n_parents, n_max)
    plist = np.arange(n_max, dtype=U32) if parents is None else np.array(parents, U32)
    assert (got[: 32 * k].reshape(-1, 2) == children_ref(level, plist[:k])).all()
    assert (got[32 * k:] == sentinel(n_words)[32 * k:]).all()  # past the list: untouched
    assert guards_intact(whole, host, before, n_words)


def test_children_of_an_upper_level(eng, torch):
    level = pair()[2][2]  # 17 nodes: parent 1 has one child
    out, whole, host, before, n_words = run_children(eng, torch, level, None, None, 2)
    eng.sync()
    got = _np(whole, U64)[before: before + 64].reshape(-1, 2)
    assert (got == children_ref(level, [0, 1])).all() and (got[17:] == 0).all()


def test_children_errors_reported_at_sync(eng, torch):
    level = pair()[2][0]
    # *n_parents above n_max: clamped
    out, whole, host, before, n_words = run_children(eng, torch, level, [1, 2, 3, 4, 5, 6, 7, 8, 9], 9, 3)
    assert code_of(eng.sync) == CRDT_E_CAPACITY
    got = _np(whole, U64)[before: before + n_words]
    assert (got[:96].reshape(-1, 2) == children_ref(level, [1, 2, 3])).all()
    assert (got[96:] == sentinel(n_words)[96:]).all()
    # a parent that is no node, in the middle: its slots zero, the others exact
    out, whole, host, before, n_words = run_children(eng, torch, level, [1, 257, 2, 0xFFFFFFFF, 256], None, 5)
    assert code_of(eng.sync) == CRDT_E_INVALID
    got = _np(whole, U64)[before: before + n_words]
    want = children_ref(level, [1, 0, 2, 0, 256])
    want[16:32] = 0
    want[48:64] = 0
    assert (got[:160].reshape(-1, 2) == want).all() and guards_intact(whole, host, before, n_words)
    eng.sync()  # the status word was cleared


# -------------------------------------------------------------------- 3. diff

class DiffOut:
    def __init__(self, torch, room, out_max=None):
        dev = dev_of(torch)
        self.room = room
        self.out_max = room if out_max is None else out_max
        self.idx = torch.full((room + 4,), -7, dtype=torch.int32, device=dev)
        self.flags = torch.full((room + 4,), 99, dtype=torch.uint8, device=dev)
        self.n_out = torch.full((1,), -1, dtype=torch.int32, device=dev)
        self.summary = torch.full((5,), -1, dtype=torch.int32, device=dev)

    def read(self):
        n = int(_np(self.n_out, U32)[0])
        return n, _np(self.idx, U32), _np(self.flags, np.uint8), _np(self.summary, U32).tolist()


def run_diff(eng, torch, mine_level, packed, parents, n_parents, n_max, leaf, mask, out, shift=False, stream=None):
    eng.digest_tree_diff_async(dev64(torch, mine_level, shift), len(mine_level), dev64(torch, packed, shift),
                               out.idx, out.n_out, parents=None if parents is None else dev32(torch, parents),
                               n_parents=None if n_parents is None else dev32(torch, [n_parents]), n_max=n_max,
                               leaf=leaf, mask=mask, flags_out=out.flags, out_max=out.out_max, summary=out.summary,
                               stream=stream)


def check_diff(out, want):
    idx, flags, summary = want
    n, gi, gf, gs = out.read()
    assert n == len(idx) and gs == summary, (n, len(idx), gs, summary)
    k = min(n, out.out_max)
    assert (gi[:k] == idx[:k]).all() and (gf[:k] == flags[:k]).all()
    assert (gi[k:] == U32(0xFFFFFFF9)).all() and (gf[k:] == 99).all()  # nothing past the list, nor past out_max


@pytest.mark.parametrize("shift", (False, True))
@pytest.mark.parametrize("mask", (1, 2, 3))
@pytest.mark.parametrize("lvl", (1, 2, 3, 4))
def test_diff_every_level(eng, torch, lvl, mask, shift):
    """Level lvl's nodes as parents, their children diffed: the ancestors of the docs that
    differ (first and last child of the first and last parent among them), and every node."""
    docs = [0, 15, 16, 31, 2048, 4080, 4095, 4096]
    mine, theirs, ml, tl = pair(N, docs, 43)
    assert len(ml) == 5
    ancestors = sorted({d // 16 ** lvl for d in docs})
    for parents in (ancestors, None):
        plist = np.arange(len(ml[lvl]), dtype=U32) if parents is None else np.array(parents, U32)
        packed = children_ref(tl[lvl - 1], plist)
        out = DiffOut(torch, 16 * len(plist))
        run_diff(eng, torch, ml[lvl - 1], packed, parents, None, len(plist), lvl == 1, mask, out, shift)
        eng.sync()
        want = diff_ref(ml[lvl - 1], packed, plist, lvl == 1, mask)
        check_diff(out, want)
        if lvl == 1:
            fw, ff = flat_ref(mine, theirs, mask)
            assert (want[0] == fw).all() and (want[1] == ff).all()


@pytest.mark.parametrize("k", (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1))
def test_diff_at_the_scan_chunk_edges(eng, torch, k):
    mine, theirs, ml, tl = pair()
    plist = np.arange(257 - k, 257, dtype=U32)  # the last k parents, the partial one among them
    packed = children_ref(tl[0], plist)
    for mask in (1, 2, 3):
        out = DiffOut(torch, 16 * k)
        run_diff(eng, torch, ml[0], packed, plist, k, k + 3, True, mask, out)  # (room for more than listed)
        eng.sync()
        check_diff(out, diff_ref(ml[0], packed, plist, True, mask))


def test_diff_out_max_one_short(eng, torch):
    mine, theirs, ml, tl = pair()
    plist = np.arange(257, dtype=U32)
    packed = children_ref(tl[0], plist)
    want = diff_ref(ml[0], packed, plist, True, 3)
    out = DiffOut(torch, len(want[0]), out_max=len(want[0]) - 1)
    run_diff(eng, torch, ml[0], packed, None, None, 257, True, 3, out)
    assert code_of(eng.sync) == CRDT_E_CAPACITY
    check_diff(out, want)  # exact *n_out and summary, nothing at or past out_max
    out = DiffOut(torch, len(want[0]))
    run_diff(eng, torch, ml[0], packed, None, None, 257, True, 3, out)
    eng.sync()
    check_diff(out, want)


def test_diff_list_errors(eng, torch):
    mine, theirs, ml, tl = pair()
    for plist in ([3, 2, 5], [3, 3, 5], [1, 2, 300]):
        packed = children_ref(tl[0], [min(p, 256) for p in plist])
        out = DiffOut(torch, 48)
        run_diff(eng, torch, ml[0], packed, plist, None, 3, True, 3, out)
        assert code_of(eng.sync) == CRDT_E_INVALID, plist
        n, gi, gf, gs = out.read()
        assert n <= 48 and (gi[48:] == U32(0xFFFFFFF9)).all()
    # *n_parents above n_max: clamped
    packed = children_ref(tl[0], [0, 1])
    out = DiffOut(torch, 32)
    run_diff(eng, torch, ml[0], packed, [0, 1, 2, 3], 4, 2, True, 3, out)
    assert code_of(eng.sync) == CRDT_E_CAPACITY
    check_diff(out, diff_ref(ml[0], packed, [0, 1], True, 3))


def test_diff_with_no_parents_still_writes_the_counts(eng, torch):
    mine, theirs, ml, tl = pair()
    for n_parents, n_max in ((None, 0), (0, 5)):
        out = DiffOut(torch, 16)
        run_diff(eng, torch, ml[0], np.zeros(32 * 5, U64), [1, 2, 3, 4, 5], n_parents, n_max, True, 3, out)
        eng.sync()
        check_diff(out, (np.zeros(0, U32), np.zeros(0, np.uint8), [0, 0, 0, 0, 0]))


def test_argument_refusals(eng, torch):
    """Refused on the host: nothing is launched."""
    lib, ctx = abi.lib(), eng._ctx
    dev = dev_of(torch)
    a = torch.zeros(64, dtype=torch.int64, device=dev)
    b = torch.zeros(64, dtype=torch.int64, device=dev)
    i = torch.arange(64, dtype=torch.int32, device=dev)
    j = torch.zeros(64, dtype=torch.int32, device=dev)
    w = torch.zeros(8, dtype=torch.int32, device=dev)
    f = torch.zeros(64, dtype=torch.uint8, device=dev)
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    tree = lambda *x: lib.crdt_digest_tree_async(*x)  # noqa: E731
    assert tree(ctx, P(a), 20, P(b), None) == 0
    assert tree(None, P(a), 20, P(b), None) == CRDT_E_INVALID
    assert tree(ctx, None, 20, P(b), None) == CRDT_E_INVALID
    assert tree(ctx, P(a), 20, None, None) == CRDT_E_INVALID
    assert tree(ctx, P(a), 20, P(a), None) == CRDT_E_INVALID
    assert tree(ctx, None, 0, None, None) == 0
    ch = lambda *x: lib.crdt_digest_tree_children_async(*x)  # noqa: E731
    assert ch(ctx, P(a), 20, P(i), P(w), 2, P(b), None) == 0
    assert ch(ctx, P(a), 20, P(i), P(w), 2, None, None) == CRDT_E_INVALID
    assert ch(ctx, None, 20, P(i), P(w), 2, P(b), None) == CRDT_E_INVALID
    assert ch(ctx, P(a), 20, P(i), P(w), 2, P(a), None) == CRDT_E_INVALID
    assert ch(ctx, P(a), 20, P(i), P(w), 2, P(i), None) == CRDT_E_INVALID
    assert ch(ctx, P(a), 20, P(i), P(w), 2, P(w), None) == CRDT_E_INVALID
    assert ch(ctx, P(a), 20, None, None, 2, P(b), None) == 0
    assert ch(ctx, P(a), 20, None, None, 3, P(b), None) == CRDT_E_INVALID  # identity: 2 nodes
    df = lambda *x: lib.crdt_digest_tree_diff_async(*x)  # noqa: E731
    ok = [ctx, P(a), 20, P(b), P(i), P(w), 2, 1, 3, P(j), P(f), P(w[2:]), 32, P(w[3:]), None]
    assert df(*ok) == 0

    def bad(pos, v):
        x = list(ok)
        x[pos] = v
        return df(*x)

    for pos in (0, 1, 3, 9, 11):  # ctx, mine_level, theirs, idx_out, n_out
        assert bad(pos, None) == CRDT_E_INVALID, pos
    for pos in (10, 13, 4, 5):  # flags_out, summary, parents (with n_max in range), n_parents: optional
        assert bad(pos, None) == 0, pos
    for mask in (0, 4, 7):
        assert bad(8, mask) == CRDT_E_INVALID
    assert bad(9, P(i)) == CRDT_E_INVALID  # idx_out on parents
    assert bad(9, P(a)) == CRDT_E_INVALID and bad(9, P(b)) == CRDT_E_INVALID
    assert bad(11, P(w)) == CRDT_E_INVALID  # n_out on n_parents
    assert bad(11, P(w[3:])) == CRDT_E_INVALID  # n_out on summary
    assert bad(13, P(w[1:])) == CRDT_E_INVALID  # summary's five words over n_out
    x = list(ok)
    x[4], x[6] = None, 3
    assert df(*x) == CRDT_E_INVALID  # identity: 2 nodes
    eng.sync()


# ----------------------------------------------------------------- 4. descent

def states(torch, n, docs, seed):
    """Two device replicas of n one-entry docs that differ in `docs`: even ones in the
    key (ELEMENTS), odd ones in the dot's counter (STATE)."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(1, 1 << 40, size=n, dtype=U64)
    counters = rng.integers(1, 1 << 30, size=n, dtype=U64)
    a = AWSetBatch(1, np.arange(n + 1, dtype=U32), keys, np.zeros(n, U32), counters, counters.copy())
    k2, c2 = keys.copy(), counters.copy()
    d = np.array(docs, np.int64)
    k2[d[d % 2 == 0]] += U64(1)
    c2[d[d % 2 == 1]] += U64(1)
    b = AWSetBatch(1, a.offsets, k2, a.actors, c2, a.vv)
    return a, b, a.to(dev_of(torch)), b.to(dev_of(torch))


def device_descent(eng, torch, dm, dt, tm, tt, mask, stream=None):
    """The whole descent from the root on the device: each level's idx_out / n_out are the
    next level's parents / n_parents; no download, no sync in between."""
    lvl = tm.L
    parents, n_parents, n_max, k = None, None, 1, 0
    while lvl >= 1:
        peer, n_level = tt.level(lvl - 1, dt)
        eng.digest_tree_children_async(peer, n_level, tm.packed, parents=parents, n_parents=n_parents, n_max=n_max,
                                       stream=stream)
        mine, _ = tm.level(lvl - 1, dm)
        eng.digest_tree_diff_async(mine, n_level, tm.packed, tm.idx[k], tm.n_out[k], parents=parents,
                                   n_parents=n_parents, n_max=n_max, leaf=lvl == 1, mask=mask, flags_out=tm.flags,
                                   out_max=tm.cap, summary=tm.summary, stream=stream)
        parents, n_parents, n_max, k, lvl = tm.idx[k], tm.n_out[k], min(tm.cap, tm.nodes[lvl - 1]), k ^ 1, lvl - 1
    return parents, n_parents


@pytest.mark.parametrize("n,share", (((1 << 20) + 1, None), (70001, 0.05)))
def test_descent_equals_the_flat_diff_and_feeds_select(eng, torch, n, share):
    rng = np.random.default_rng(n)
    if share is None:
        docs = [0, 15, 16, 70000, 1 << 19, (1 << 20) - 1, 1 << 20]  # seven, the last one alone under its parents
    else:
        docs = sorted(rng.choice(n, size=int(n * share), replace=False).tolist())
    a, b, da, db = states(torch, n, docs, n)
    dev = dev_of(torch)
    eng.reserve(n)
    dm = torch.empty(2 * n, dtype=torch.int64, device=dev)
    dt = torch.empty(2 * n, dtype=torch.int64, device=dev)
    eng.digest_async(da, dm)
    eng.digest_async(db, dt)
    cap = 8192
    tm, tt = DigestTreeBuffers(n, dev, cap=cap), DigestTreeBuffers(n, dev)
    eng.digest_tree_async(dm, n, tm.tree)
    eng.digest_tree_async(dt, n, tt.tree)
    flat = CompareBuffers(n, device=dev)
    for mask in (1, 2, 3):
        eng.digest_diff_async(dm, dt, n, flat, mask=mask)
        work, n_work = device_descent(eng, torch, dm, dt, tm, tt, mask)
        eng.sync()
        fflags, fsum, fwork = flat.numpy()
        want = [d for d in docs if (1 if d % 2 == 0 else 2) & mask]
        assert fwork.tolist() == want
        k = int(_np(n_work, U32)[0])
        assert k == len(want) and _np(work, U32)[:k].tolist() == want
        assert (_np(tm.flags, np.uint8)[:k] == fflags[want]).all()
        assert _np(tm.summary, U32).tolist()[4] == k
    # mask 3's worklist, still on the device, selects the docs
    out = OutBuffers(len(docs), 1, len(docs) + 4, device=dev)
    eng.select_async(da, out, idx=work, n_idx=n_work, n_out=len(docs))
    eng.sync()
    h = out.as_batch().numpy()
    d = np.array(docs, np.int64)
    assert (h.counts == 1).all() and (h.keys[: len(docs)] == a.keys[d]).all()
    assert (h.counters[: len(docs)] == a.counters[d]).all() and (h.vv[: len(docs)] == a.vv[d]).all()
    # the Engine's driver: the same list, one 4-byte read per level, the model's bytes
    asked = []

    def fetch(level, parents, k):
        asked.append(k)
        peer, n_level = tt.level(level - 1, dt)
        eng.digest_tree_children_async(peer, n_level, tt_packed, parents=parents, n_max=k)
        return tt_packed

    tt_packed = torch.empty(32 * cap, dtype=torch.int64, device=dev)
    w, f, k, fetched = eng.digest_tree_descend(dm, tm, fetch, mask=3)
    assert _np(w, U32).tolist() == docs and k == len(docs)
    levels = [np.unique(np.array(docs) // 16 ** l) for l in range(tm.L, 0, -1)]
    assert asked == [len(x) for x in levels] and fetched == 256 * sum(asked)
    if share is None:
        assert fetched < 16 * n // 1000


def test_descent_of_converged_replicas_asks_for_the_root_only(eng, torch):
    n = 70001
    dev = dev_of(torch)
    digest = dev64(torch, random_digest(n, 3))
    t = DigestTreeBuffers(n, dev, cap=64)
    eng.digest_tree_async(digest, n, t.tree)
    asked = []

    def fetch(level, parents, k):
        asked.append((level, k))
        lv, n_level = t.level(level - 1, digest)
        eng.digest_tree_children_async(lv, n_level, t.packed, parents=parents, n_max=k)
        return t.packed

    w, f, k, fetched = eng.digest_tree_descend(digest, t, fetch)
    assert k == 0 and fetched == 256 and asked == [(t.L, 1)]


# ------------------------------------------------------------------- 5. also

def test_run_to_run_identity(eng, torch):
    n = 70001
    mine, theirs = differing(n, list(range(0, n, 13)), 5)
    dm, dt = dev64(torch, mine), dev64(torch, theirs)
    dev = dev_of(torch)
    runs = []
    for r in range(3):
        tm, tt = DigestTreeBuffers(n, dev, cap=8192), DigestTreeBuffers(n, dev)
        eng.digest_tree_async(dm, n, tm.tree)
        eng.digest_tree_async(dt, n, tt.tree)
        work, n_work = device_descent(eng, torch, dm, dt, tm, tt, 3)
        eng.sync()
        k = int(_np(n_work, U32)[0])
        runs.append((_np(tm.tree, U64).copy(), _np(work, U32)[:k].copy(), _np(tm.flags, np.uint8)[:k].copy()))
    assert (runs[0][0].reshape(-1, 2) == crdtgpu.digest_tree_host(mine)).all()
    assert runs[0][1].tolist() == list(range(0, n, 13))
    for r in runs[1:]:
        assert all((x == y).all() for x, y in zip(r, runs[0]))


def test_graph_capture_build_and_diff(torch):
    """A build and a leaf diff over the whole level captured on a reserved context and
    replayed after both digest arrays changed; on an unreserved context the diff's capture
    is refused with CRDT_E_WORKSPACE and nothing is launched."""
    n = (1 << 20) + 1
    dev = dev_of(torch)
    docs1, docs2 = [3, 70000, 1 << 20], [0, 99, 65536, 1000000]
    m1, t1 = differing(n, docs1, 61)
    m2, t2 = differing(n, docs2, 62)
    dm = dev64(torch, m1)
    packed = torch.zeros(32 * (-(-n // 16)), dtype=torch.int64, device=dev)  # the peer's level 0, padded
    packed[: 2 * n].copy_(dev64(torch, t1))
    tm = DigestTreeBuffers(n, dev)
    out = DiffOut(torch, 64)
    n_parents = tm.nodes[1]
    e = crdtgpu.Engine(0)
    try:
        g0 = torch.cuda.CUDAGraph()
        with pytest.raises(crdtgpu.CrdtError) as ei:
            with torch.cuda.graph(g0):
                s = torch.cuda.current_stream()
                e.digest_tree_async(dm, n, tm.tree, stream=s)  # (no workspace: captured)
                e.digest_tree_diff_async(dm, n, packed, out.idx, out.n_out, n_max=n_parents, leaf=True,
                                         flags_out=out.flags, out_max=64, summary=out.summary, stream=s)
        assert ei.value.code == CRDT_E_WORKSPACE
        torch.cuda.synchronize()
        assert int(_np(out.n_out, U32)[0]) == 0xFFFFFFFF and (_np(out.idx, U32) == U32(0xFFFFFFF9)).all()
        e.reserve(n)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            s = torch.cuda.current_stream()
            e.digest_tree_async(dm, n, tm.tree, stream=s)
            e.digest_tree_diff_async(dm, n, packed, out.idx, out.n_out, n_max=n_parents, leaf=True,
                                     flags_out=out.flags, out_max=64, summary=out.summary, stream=s)
        for mine, theirs, docs in ((m1, t1, docs1), (m2, t2, docs2)):
            dm.copy_(dev64(torch, mine))
            packed[: 2 * n].copy_(dev64(torch, theirs))
            tm.tree.zero_()
            g.replay()
            e.sync(torch.cuda.current_stream())
            fw, ff = flat_ref(mine, theirs, 3)
            assert fw.tolist() == docs
            k, gi, gf, gs = out.read()
            assert k == len(docs) and gi[:k].tolist() == docs and (gf[:k] == ff).all() and gs[4] == k
            assert (_np(tm.tree, U64).reshape(-1, 2) == crdtgpu.digest_tree_host(mine)).all()
    finally:
        e.close()


def test_two_streams_are_ordered_by_the_context(eng, torch):
    """The build on one stream, the children and the diff that read its tree on another,
    with no event of the caller's between them."""
    n = 70001
    docs = list(range(5, n, 997))
    mine, theirs = differing(n, docs, 71)
    dm, dt = dev64(torch, mine), dev64(torch, theirs)
    dev = dev_of(torch)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    tm, tt = DigestTreeBuffers(n, dev, cap=8192), DigestTreeBuffers(n, dev)
    torch.cuda.synchronize()
    eng.digest_tree_async(dm, n, tm.tree, stream=sa)
    eng.digest_tree_async(dt, n, tt.tree, stream=sa)
    work, n_work = device_descent(eng, torch, dm, dt, tm, tt, 3, stream=sb)
    eng.sync(sb)
    k = int(_np(n_work, U32)[0])
    assert _np(work, U32)[:k].tolist() == docs
