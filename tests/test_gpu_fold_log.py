"""GPU: crdt_awset_fold_log_async (csrc/fold_log.hip) against fold_log_ref
(tests/fold_log_cases.py, pinned by tests/test_fold_log_model.py): the merged state
bit-equal to crdt_awset_fold_async and to the C oracle, and both lists of every
document, flags, counts, offsets and summary equal to the reference.

Every written buffer is over-allocated and pre-filled with poison, so each word
compared was written by the call; every list slot outside a document's live prefix
and every output slot past the batch's last must still hold the poison afterwards.
The wave path takes a document while dst, every source's entries and tombstones and
the state after every step hold at most 64; the rest goes through the worklist to
the block path.  No test provokes a fault: the error cases are the clamped, reported
ones of the contract, which the fold's own tests exercise too.
"""

import ctypes

import numpy as np
import pytest

import crdtgpu
import fold_edge_cases as fe
from counter_maps import map_batch, map_srcs, mixed
from crdtgpu import CRDT_E_ACTOR_RANGE, CRDT_E_CAPACITY, CRDT_E_INVALID, CRDT_E_WORKSPACE, abi
from crdtgpu.batch import AWSetBatch, DiffBuffers, MergeLogBuffers, OutBuffers, SrcBatch
from fold_log_cases import (AWSET, CLOCK, DELTA, LOG_DOCS, LOG_WAVES, MAX_C, WAVE_MAX, all_cases, batches, big_doc,
                            fold_log_ref, path_of, seq)
from helpers import out_doc
from join_log_cases import assert_log, assert_state, doc_lists
from oracle import oracle
from test_gpu_compare import _code, dev_of, host_out, poisoned_out

pytestmark = pytest.mark.gpu

U8, U32, U64 = np.uint8, np.uint32, np.uint64
POISON8 = 77
PAD = 40  # slots every entry array is over-allocated by
LIST_FIELDS = ("rem_keys", "rem_actors", "rem_counters", "ups_keys", "ups_actors", "ups_counters", "ups_kind")


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


_refs = {}


def ref_of(key, mode, dst, srcs):
    """The reference of a batch, computed once and shared (never modified)."""
    if key not in _refs:
        _refs[key] = fold_log_ref(mode, dst, srcs)
    return _refs[key]


# ------------------------------------------------------------------- helpers

def slots_of(dst, srcs):
    return int(np.asarray(dst.offsets)[-1]), int(np.asarray(srcs.entry_off)[-1])


def poison(log):
    for f in log.FIELDS:
        t = getattr(log, f)
        if t is not None:
            t.fill_(POISON8 if f in ("flags", "ups_kind") else -1)
    return log


def run(eng, torch, mode, dst, srcs, stream=None, reserve=True, d_dst=None, d_srcs=None, **kw):
    """(out, log) on the device after one fold_log_async into poisoned buffers; not synced."""
    dev = dev_of(torch)
    ds, es = slots_of(dst, srcs)
    out = poisoned_out(torch, dst.n_docs, dst.R, ds + es + PAD)
    log = poison(MergeLogBuffers(dst.n_docs, ds + PAD, es + PAD, device=dev, **kw))
    if reserve:
        eng.reserve(max(dst.n_docs, 1), ds + es)
    eng.fold_log_async(mode, d_dst or dst.to(dev), d_srcs or srcs.to(dev), out, log, stream=stream)
    return out, log


def assert_poison_kept(h, g, want, ds, es):
    for f in LIST_FIELDS:
        if g[f] is None:
            continue
        keep = np.ones(len(g[f]), bool)
        keep[want.rem_idx if f.startswith("rem") else want.ups_idx] = False
        bad = POISON8 if f == "ups_kind" else (2 ** 64 - 1 if g[f].dtype == U64 else 2 ** 32 - 1)
        assert (g[f][keep] == bad).all(), "%s: a slot outside the live prefixes was written" % f
    for f in ("keys", "actors", "counters"):
        a = getattr(h, f)
        assert (a[ds + es:] == (2 ** 64 - 1 if a.dtype == U64 else 2 ** 32 - 1)).all(), "%s: written past the last slot" % f


def assert_result(out, log, dst, srcs, want, what=""):
    assert want.rc == 0
    h, g = host_out(out), log.numpy()
    assert_state(h, want.out, dst.n_docs, dst.R, what)
    assert_log(g, want, what)
    assert_poison_kept(h, g, want, *slots_of(dst, srcs))
    return h, g


def check(eng, torch, mode, dst, srcs, want=None, plain=True, **kw):
    want = want or fold_log_ref(mode, dst, srcs)
    dev = dev_of(torch)
    d_dst, d_srcs = dst.to(dev), srcs.to(dev)
    out, log = run(eng, torch, mode, dst, srcs, d_dst=d_dst, d_srcs=d_srcs, **kw)
    if plain:  # the plain fold of the same device inputs
        p = poisoned_out(torch, dst.n_docs, dst.R, sum(slots_of(dst, srcs)))
        eng.fold_async(mode, d_dst, d_srcs, p)
    eng.sync()
    h, g = assert_result(out, log, dst, srcs, want)
    if plain:
        hp = host_out(p)
        n, R = dst.n_docs, dst.R
        assert (hp.offsets[: n + 1] == h.offsets[: n + 1]).all() and (hp.counts[:n] == h.counts[:n]).all()
        assert (hp.vv[: n * R] == h.vv[: n * R]).all()
        for d in range(n):
            assert out_doc(hp, d, R) == out_doc(h, d, R), d
    return h, g, want


# --------------------------------------------------------- 1. the case table

@pytest.mark.parametrize("name", sorted(all_cases()))
def test_case(eng, torch, name):
    c = all_cases()[name]
    dst, srcs = batches(c)
    check(eng, torch, c.mode, dst, srcs, ref_of(name, c.mode, dst, srcs))


@pytest.mark.parametrize("name", sorted(fe.all_cases()))
def test_fold_edge_case(eng, torch, name):
    """Every case of tests/fold_edge_cases.py in its mode: the documents that sit on the
    dispatch edges of the plain fold's kernels."""
    c = fe.all_cases()[name]
    for i, (dst, srcs) in enumerate(c.batches):
        check(eng, torch, c.mode, dst, srcs, ref_of((name, i), c.mode, dst, srcs))


def test_paths_are_the_ones_the_cases_name(eng, torch):
    """A given-up document and the small one after it share a wavefront; the many-documents
    case spans more workgroups than one and ends inside one."""
    c = all_cases()["stale_lds_awset"]
    assert len(c.docs) <= LOG_DOCS and c.paths[0] == ("bail", 1) and c.paths[1] == "wave"
    m = all_cases()["many_docs_delta"]
    assert len(m.docs) > 2 * LOG_WAVES * LOG_DOCS and len(m.docs) % (LOG_WAVES * LOG_DOCS) != 0
    assert sum(path_of(m.mode, *d) == "block" for d in m.docs) >= 3
    assert WAVE_MAX == 64


# ------------------------------------------------------------------ 2. shapes

@pytest.mark.parametrize("name", ["shapes_awset", "shapes_delta", "state_grows_delta", "width_R3_delta", "block_awset"])
def test_counts_with_slack(eng, torch, name):
    """counts given and three spare slots a document, stale values in them; the same live
    documents as with counts == NULL (test_case), other slot bounds."""
    c = all_cases()[name]
    dst, srcs = batches(c, slack=3)
    assert dst.counts is not None
    rng = np.random.default_rng(5)
    live = np.zeros(len(dst.keys), bool)
    for d in range(dst.n_docs):
        live[int(dst.offsets[d]):int(dst.offsets[d]) + int(dst.counts[d])] = True
    dst.keys[~live] = rng.integers(0, 2 ** 63, int((~live).sum()), dtype=np.int64).view(U64)
    dst.actors[~live] = c.R
    dst.counters[~live] = MAX_C
    h, g, want = check(eng, torch, c.mode, dst, srcs)
    tight = ref_of(name, c.mode, *batches(c))
    for d in range(dst.n_docs):
        assert out_doc(h, d, c.R) == out_doc(tight.out, d, c.R), d
        assert doc_lists(g, d) == doc_lists(tight.log, d), d


@pytest.mark.parametrize("name", ["shapes_delta", "width_R2_delta", "block_delta"])
def test_delta_fold_without_tombstone_arrays(eng, torch, name):
    c = all_cases()[name]
    docs = [(e, vv, [(a, v, s, []) for a, v, s, _ in chain]) for e, vv, chain in c.docs]
    dst, twin = batches(c._replace(docs=docs))
    bare = SrcBatch(c.R, twin.doc_srcs, twin.src_actor, twin.vv, twin.entry_off, twin.keys, twin.actors, twin.counters)
    want = fold_log_ref(DELTA, dst, twin)
    check(eng, torch, DELTA, dst, bare, want)


@pytest.mark.parametrize("kw", [dict(summary=False), dict(kind=False), dict(summary=False, kind=False)])
def test_optional_outputs(eng, torch, kw):
    c = all_cases()["width_R3_delta"]
    dst, srcs = batches(c)
    out, log = run(eng, torch, c.mode, dst, srcs, **kw)
    eng.sync()
    assert_result(out, log, dst, srcs, ref_of(c.name, c.mode, dst, srcs))


@pytest.mark.parametrize("summary", [True, False])
def test_no_documents(eng, torch, summary):
    dev = dev_of(torch)
    z = lambda dt: torch.zeros(1, dtype=dt, device=dev)  # noqa: E731
    dst = AWSetBatch(2, z(torch.int32), z(torch.int64), z(torch.int32), z(torch.int64), z(torch.int64))
    srcs = SrcBatch(2, z(torch.int32), z(torch.int32), z(torch.int64), z(torch.int32), z(torch.int64), z(torch.int32),
                    z(torch.int64))
    assert dst.n_docs == 0 and srcs.n_docs == 0
    out = poisoned_out(torch, 1, 2, 4)
    log = poison(MergeLogBuffers(0, 4, 4, device=dev, summary=summary))
    for mode in (AWSET, DELTA):
        eng.fold_log_async(mode, dst, srcs, out, log)
        eng.sync()
        assert (out.keys.cpu().numpy().view(U64) == 2 ** 64 - 1).all()
        assert int(out.counts.cpu().numpy().view(U32)[0]) == 2 ** 32 - 1 and int(out.offsets.cpu().numpy().view(U32)[0]) == 2 ** 32 - 1
        if summary:
            assert not log.summary.cpu().numpy().any()  # zeroed
        assert int(log.flags.cpu().numpy()[0]) == POISON8 and int(log.rem_offsets.cpu().numpy().view(U32)[0]) == 2 ** 32 - 1
        assert (log.ups_keys.cpu().numpy().view(U64) == 2 ** 64 - 1).all()


# ------------------------------------------------------------ 3. wide counters

@pytest.mark.parametrize("name", ["width_R2_awset", "width_R3_delta", "many_docs_delta", "block_delta"])
def test_wide_counters(eng, torch, name):
    """The same documents with every counter and clock value through the order-preserving
    maps of tests/counter_maps.py (up to 2^32, 2^63, 2^64 - 1): equal to the reference on
    the mapped inputs, with the flags and counts of the unmapped run."""
    c = all_cases()[name]
    dst, srcs = batches(c)
    plain = ref_of(name, c.mode, dst, srcs)
    cmax = fe.CMAX if name.startswith("width") else MAX_C
    tab = mixed(cmax, 3)
    _, g, want = check(eng, torch, c.mode, map_batch(dst, tab), map_srcs(srcs, tab))
    big = np.concatenate([want.log["rem_counters"], want.log["ups_counters"], np.asarray(want.out.vv)])
    assert (big >= 2 ** 32).any()
    if dst.n_docs >= 12:  # every map of the six is met
        assert ((big >= 2 ** 63) & (big < 2 ** 63 + 64)).any() and (big >= 2 ** 64 - 1 - 64).any()
    for f in ("flags", "summary", "rem_counts", "ups_counts"):
        assert (g[f] == plain.log[f]).all(), f


# ------------------------------------------------------- 4. parity with the diff

@pytest.mark.parametrize("name", ["width_R2_awset", "width_R64_delta", "block_delta", "state_grows_awset"])
def test_log_equals_the_device_diff_of_dst_and_out(eng, torch, name):
    """flags, per-document counts and summary equal crdt_awset_diff_async(dst, out)'s, and
    its packed lists equal the log's lists read document by document."""
    c = all_cases()[name]
    dst, srcs = batches(c)
    want = ref_of(name, c.mode, dst, srcs)
    dev = dev_of(torch)
    d_dst = dst.to(dev)
    out, log = run(eng, torch, c.mode, dst, srcs, d_dst=d_dst)
    diff = DiffBuffers(dst.n_docs, log.rem_slots, log.ups_slots, device=dev)
    eng.diff_async(d_dst, out.as_batch(), diff)
    eng.sync()
    g, df = log.numpy(), diff.numpy()
    assert (g["flags"] == df["flags"]).all() and (g["summary"] == df["summary"]).all()
    assert (g["rem_counts"] == np.diff(df["rem_off"])).all() and (g["ups_counts"] == np.diff(df["ups_off"])).all()
    for f in LIST_FIELDS:
        idx = want.rem_idx if f.startswith("rem") else want.ups_idx
        assert (g[f][idx] == df[f][: len(idx)]).all(), f


# --------------------------------------------------------------- 5. errors

def error_docs(mode, size, actor):
    """Four small documents, the second holding a source-only key under a dot of `actor`
    that the step asks dst's clock about; size "block": that document has 70 dst entries."""
    small = lambda d: ([(10 * d, 0, 1), (10 * d + 1, 1, 2)], [5, 5], [(1, [0, 7], [(10 * d + 2, 1, 7)], [])])  # noqa: E731
    docs = [small(d) for d in range(4)]
    docs[1] = (seq(70 if size == "block" else 5, 1000), [5, 5], [(1, [0, 7], [(999, actor, 7)], [])])
    return docs


@pytest.mark.parametrize("size", ["wave", "block"])
@pytest.mark.parametrize("mode", [AWSET, DELTA])
def test_actor_range_on_each_path(eng, torch, mode, size):
    """HasDot at actor == R is the reference's panic; actor > R is "never seen".  The clean
    documents around it are exact."""
    case = all_cases()["shapes_awset"]._replace(mode=mode, docs=error_docs(mode, size, 2))
    assert path_of(mode, *error_docs(mode, size, 3)[1]) == ("block" if size == "block" else "wave")
    dst, srcs = batches(case)
    assert oracle.fold(mode, dst, srcs)[0] == CRDT_E_ACTOR_RANGE
    out, log = run(eng, torch, mode, dst, srcs)
    assert _code(eng.sync) == CRDT_E_ACTOR_RANGE
    eng.sync()  # cleared
    ok = case._replace(docs=error_docs(mode, size, 3))
    h2, g2, want = check(eng, torch, mode, *batches(ok))
    h, g = host_out(out), log.numpy()
    for d in (0, 2, 3):
        assert out_doc(h, d, 2) == out_doc(want.out, d, 2), d
        assert doc_lists(g, d) == doc_lists(want.log, d) and int(g["flags"][d]) == int(want.log["flags"][d]), d


@pytest.mark.parametrize("size", ["wave", "block"])
def test_actor_range_on_the_path_select(eng, torch, size):
    """Counter(src.Actor) at actor == R (delta folds)."""
    docs = error_docs(DELTA, size, 1)
    e, vv, chain = docs[1]
    docs[1] = (e, vv, [(2,) + chain[0][1:]])
    dst, srcs = batches(all_cases()["shapes_delta"]._replace(docs=docs))
    run(eng, torch, DELTA, dst, srcs)
    assert _code(eng.sync) == CRDT_E_ACTOR_RANGE
    eng.sync()


@pytest.mark.parametrize("size", ["wave", "block"])
@pytest.mark.parametrize("mode", [AWSET, DELTA])
def test_live_count_above_slots_is_clamped(eng, torch, mode, size):
    case = all_cases()["shapes_awset"]._replace(mode=mode, docs=error_docs(mode, size, 1))
    dst, srcs = batches(case, slack=1)
    s = int(dst.offsets[2]) - 1  # the slack slot continues the document's keys: clamped, it is still sorted
    dst.keys[s], dst.actors[s], dst.counters[s] = int(dst.keys[s - 1]) + 1, 0, 1
    want = fold_log_ref(mode, dst, srcs)  # (every count within its slots)
    counts = dst.counts.copy()
    counts[1] = int(dst.offsets[2]) - int(dst.offsets[1]) + 2
    over = AWSetBatch(dst.R, dst.offsets, dst.keys, dst.actors, dst.counters, dst.vv, counts)
    out, log = run(eng, torch, mode, over, srcs)
    assert _code(eng.sync) == CRDT_E_CAPACITY
    eng.sync()  # cleared
    h, g = host_out(out), log.numpy()
    for d in (0, 2, 3):
        assert out_doc(h, d, 2) == out_doc(want.out, d, 2), d
        assert doc_lists(g, d) == doc_lists(want.log, d) and int(g["flags"][d]) == int(want.log["flags"][d]), d


@pytest.mark.parametrize("mode", [AWSET, DELTA])
def test_block_path_without_fold_slots_reports_workspace(torch, mode):
    case = all_cases()["block_awset" if mode == AWSET else "block_delta"]
    dst, srcs = batches(case)
    want = ref_of(case.name, mode, dst, srcs)
    fresh = crdtgpu.Engine(0)
    try:
        out, log = run(fresh, torch, mode, dst, srcs, reserve=False)  # never reserved: one scratch slot
        assert _code(fresh.sync) == CRDT_E_WORKSPACE
        fresh.sync()
        h, g = host_out(out), log.numpy()
        assert out_doc(h, 1, 2) == out_doc(want.out, 1, 2) and doc_lists(g, 1) == doc_lists(want.log, 1)
        check(fresh, torch, mode, dst, srcs, want)  # reserved now
    finally:
        fresh.close()


def test_argument_errors(eng, torch):
    """Every one of these is refused on the host: nothing is launched."""
    c = all_cases()["shapes_delta"]
    dst, srcs = batches(c)
    dev = dev_of(torch)
    d, s = dst.to(dev), srcs.to(dev)
    n, R = dst.n_docs, 2
    out, out2 = poisoned_out(torch, n, R, 64), poisoned_out(torch, n, R, 64)
    log = poison(MergeLogBuffers(n, 64, 64, device=dev))
    lib, ctx, ref = abi.lib(), eng._ctx, ctypes.byref
    r = lambda x: ref(x) if x is not None else None  # noqa: E731

    def call(cd, cs, co, cl, mode=DELTA, c=ctx):
        return lib.crdt_awset_fold_log_async(c, mode, r(cd), r(cs), r(co), r(cl), None)

    args = [d.c(), s.c(), out.c(), log.c()]
    for i in range(4):  # any NULL among the arguments
        bad = list(args)
        bad[i] = None
        assert call(*bad) == CRDT_E_INVALID, i
    assert call(*args, c=None) == CRDT_E_INVALID
    for mode in (-1, 2, 7):
        assert call(*args, mode=mode) == CRDT_E_INVALID, mode
    few = batches(c._replace(docs=c.docs[:3]))
    assert call(few[0].to(dev).c(), args[1], args[2], args[3]) == CRDT_E_INVALID  # n_docs
    assert call(args[0], few[1].to(dev).c(), args[2], args[3]) == CRDT_E_INVALID
    wide = d.c()
    wide.R = 3
    assert call(wide, args[1], args[2], args[3]) == CRDT_E_INVALID  # R mismatch
    w1, w2 = d.c(), s.c()
    w1.R = w2.R = 65
    assert call(w1, w2, args[2], args[3]) == CRDT_E_INVALID  # R out of range
    for f in ("offsets", "counts", "keys", "actors", "counters", "vv"):  # a required field NULL
        co = out.c()
        setattr(co, f, None)
        assert call(args[0], args[1], co, args[3]) == CRDT_E_INVALID, f
    for f in ("doc_srcs", "src_actor", "entry_off"):
        cs = s.c()
        setattr(cs, f, None)
        assert call(args[0], cs, args[2], args[3]) == CRDT_E_INVALID, f
    for f in MergeLogBuffers.FIELDS:
        if f not in ("summary", "ups_kind"):
            g = log.c()
            setattr(g, f, None)
            assert call(args[0], args[1], args[2], g) == CRDT_E_INVALID, f
    for f, g_ in (("rem_keys", "ups_keys"), ("rem_counts", "ups_counts"), ("rem_keys", "rem_counters"),
                  ("flags", "ups_kind"), ("rem_offsets", "ups_offsets")):  # two written arrays at one address
        g = log.c()
        setattr(g, f, getattr(log.c(), g_))
        assert call(args[0], args[1], args[2], g) == CRDT_E_INVALID, (f, g_)
    for f, of in (("rem_keys", "keys"), ("ups_counters", "counters"), ("rem_actors", "actors"), ("rem_counts", "counts"),
                  ("ups_offsets", "offsets"), ("ups_keys", "vv")):  # a log array against an output array
        g = log.c()
        setattr(g, f, getattr(out.c(), of))
        assert call(args[0], args[1], args[2], g) == CRDT_E_INVALID, (f, of)
    # a written array starting where an input array of the same kind starts
    for f, src in (("keys", d.keys), ("counters", s.keys), ("vv", s.vv), ("actors", s.actors), ("offsets", s.doc_srcs),
                   ("counts", s.entry_off), ("keys", s.tkeys), ("counters", s.tcounters), ("actors", s.tactors),
                   ("offsets", s.tomb_off), ("vv", d.vv), ("counts", s.src_actor)):
        co = out.c()
        setattr(co, f, src.data_ptr())
        assert call(args[0], args[1], co, args[3]) == CRDT_E_INVALID, f
    for f, src in (("rem_keys", d.keys), ("ups_keys", s.keys), ("rem_counters", d.vv), ("ups_actors", s.actors),
                   ("rem_offsets", d.offsets), ("ups_offsets", s.entry_off), ("summary", s.doc_srcs),
                   ("ups_counters", s.tcounters), ("rem_counts", s.tactors)):
        g = log.c()
        setattr(g, f, src.data_ptr())
        assert call(args[0], args[1], args[2], g) == CRDT_E_INVALID, f
    eng.sync()
    for t in (out.offsets, out.counts, out.actors):
        assert (t.cpu().numpy().view(U32) == 2 ** 32 - 1).all()
    for t in (out.keys, out.counters, out.vv):
        assert (t.cpu().numpy().view(U64) == 2 ** 64 - 1).all()
    assert (log.flags.cpu().numpy() == POISON8).all() and (log.rem_counts.cpu().numpy().view(U32) == 2 ** 32 - 1).all()
    assert (log.summary.cpu().numpy().view(U32) == 2 ** 32 - 1).all()
    assert call(*args) == 0  # and the same arguments as they stand are accepted
    eng.sync()
    del out2


# ------------------------------------------------------------ 6. repeatability

def _bits(out, log):
    return [getattr(out, f).cpu().numpy().copy() for f in ("offsets", "counts", "keys", "actors", "counters", "vv")] + \
           [getattr(log, f).cpu().numpy().copy() for f in log.FIELDS]


@pytest.mark.parametrize("name", ["many_docs_delta", "block_awset"])
def test_two_runs_write_the_same_bits(eng, torch, name):
    c = all_cases()[name]
    dst, srcs = batches(c)
    runs = []
    for _ in range(2):
        out, log = run(eng, torch, c.mode, dst, srcs)
        eng.sync()
        runs.append(_bits(out, log))
    for a, b in zip(*runs):
        assert (a == b).all()


def test_graph_capture(torch):
    """Captured on a reserved context and replayed with the sources' clocks changed in
    between, equal to eager; on an unreserved context the capture is refused with
    CRDT_E_WORKSPACE and launches nothing."""
    c = all_cases()["many_docs_delta"]
    reps = 1100 // len(c.docs) + 1
    c = c._replace(docs=c.docs * reps)
    dst, srcs = batches(c)
    n = dst.n_docs
    assert n > 1024  # (a fresh context's workspace holds 1,024 documents)
    dev = dev_of(torch)
    ds, es = slots_of(dst, srcs)
    e = crdtgpu.Engine(0)
    try:
        d_dst, d_srcs = dst.to(dev), srcs.to(dev)
        out = poisoned_out(torch, n, 2, ds + es + PAD)
        log = poison(MergeLogBuffers(n, ds + PAD, es + PAD, device=dev))
        g0 = torch.cuda.CUDAGraph()
        with pytest.raises(crdtgpu.CrdtError) as ei:
            with torch.cuda.graph(g0):
                e.fold_log_async(DELTA, d_dst, d_srcs, out, log, stream=torch.cuda.current_stream())
        assert ei.value.code == CRDT_E_WORKSPACE
        torch.cuda.synchronize()
        assert (log.flags.cpu().numpy() == POISON8).all() and (out.counts.cpu().numpy().view(U32) == 2 ** 32 - 1).all()
        e.reserve(n, ds + es)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.fold_log_async(DELTA, d_dst, d_srcs, out, log, stream=torch.cuda.current_stream())
        for bump in (0, 1):  # the sources' clocks change between replays: other flags
            vv = srcs.vv.copy()
            vv[::2] += U64(bump)
            hs = SrcBatch(2, srcs.doc_srcs, srcs.src_actor, vv, srcs.entry_off, srcs.keys, srcs.actors, srcs.counters,
                          srcs.tomb_off, srcs.tkeys, srcs.tactors, srcs.tcounters)
            d_srcs.vv.copy_(hs.to(dev).vv)
            for t in (out.offsets, out.counts, out.keys, out.actors, out.counters, out.vv):
                t.fill_(-1)
            poison(log)
            g.replay()
            e.sync(torch.cuda.current_stream())
            want = fold_log_ref(DELTA, dst, hs)
            assert_result(out, log, dst, hs, want)
            replayed = _bits(out, log)
            eo, el = run(e, torch, DELTA, dst, hs)
            e.sync()
            for a, b in zip(replayed, _bits(eo, el)):
                assert (a == b).all()
        assert (want.log["flags"] & CLOCK).any()
    finally:
        e.close()
