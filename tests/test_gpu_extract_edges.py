"""GPU: extract_kernel (csrc/extract.hip) on every case of tests/extract_edge_cases.py (pinned by
tests/test_extract_edges_model.py), bit-exact against the restatement of
tests/test_delta_extract_model.py.

Every output array is allocated MARGIN elements longer than the call may use and filled with a
pattern no case holds.  After the call the live prefix is compared bit-exactly and every word
outside it must still be the pattern: the entry columns past entry_off[n_srcs], the tombstone
columns past tomb_off[n_srcs], kind and src_actor past n_srcs, vv past n_srcs * R, the offset
arrays past n_srcs + 1 and doc_srcs past n_docs + 1.  No test provokes a fault: the error
cases are the reported ones of the contract (include/crdtgpu.h).
"""

import ctypes

import numpy as np
import pytest

import crdtgpu
import test_delta_extract_model as model
from crdtgpu import CRDT_E_ACTOR_RANGE, CRDT_E_INVALID, CRDT_MAX_R, abi
from crdtgpu.batch import SrcBatch
from extract_edge_cases import BY_NAME, CASES, Case, clock, expected, flat_peers, full_src, geo_doc, small_src
from helpers import src_batch_of
from test_delta_extract_model import DELTA, FULL, NONE
from test_gpu_compare import _code, dev_of
from test_gpu_delta_extract import assert_message, to_dev

pytestmark = pytest.mark.gpu

U8, U32, U64 = np.uint8, np.uint32, np.uint64
MARGIN = 128
P8, P32, P64 = 0x5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A  # no case holds these as a key, an actor, a counter, a clock or a kind
TOMB_F = ("tomb_off", "tkeys", "tactors", "tcounters")


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


# ------------------------------------------------------------------- helpers

_prepared = {}


def prepared(case):
    """(host sources with tombstone arrays, expected kinds, expected messages, flat peer clocks),
    computed once per case and left unchanged."""
    if case.name not in _prepared:
        kinds, msgs = expected(case)
        _prepared[case.name] = (src_batch_of(case.R, case.per_doc), np.array(kinds, U8), msgs,
                                np.array(flat_peers(case), dtype=U64))
    return _prepared[case.name]


def live_sizes(srcs):
    """Elements of each output array the call may write: the input's capacity."""
    ns, nd = srcs.n_srcs, srcs.n_docs
    ne, nt = int(srcs.entry_off[ns]), int(srcs.tomb_off[ns])
    return dict(doc_srcs=nd + 1, src_actor=ns, vv=ns * srcs.R, entry_off=ns + 1, keys=ne, actors=ne, counters=ne,
                tomb_off=ns + 1, tkeys=nt, tactors=nt, tcounters=nt)


def poison(torch, t):
    return t.fill_({torch.uint8: P8, torch.int32: P32, torch.int64: P64}[t.dtype])


def poisoned_out(torch, srcs, tombs="given"):
    """(output SrcBatch of device tensors, kind tensor): every array MARGIN longer than the input's
    capacity and poisoned; tombs "out_null": no tombstone arrays at all."""
    dev = dev_of(torch)
    arrays = {}
    for (f, dt), n in zip(SrcBatch._FIELDS, live_sizes(srcs).values()):
        tdt = torch.int32 if dt == U32 else torch.int64
        arrays[f] = None if tombs == "out_null" and f in TOMB_F else poison(torch, torch.empty(n + MARGIN, dtype=tdt, device=dev))
    kind = poison(torch, torch.empty(srcs.n_srcs + MARGIN, dtype=torch.uint8, device=dev))
    return SrcBatch(srcs.R, *(arrays[f] for f, _ in SrcBatch._FIELDS)), kind


def repoison(torch, out, kind):
    for f, _ in SrcBatch._FIELDS:
        if getattr(out, f) is not None:
            poison(torch, getattr(out, f))
    poison(torch, kind)


def device_input(torch, srcs, tombs="given"):
    if tombs != "given":  # srcs->tomb_off == NULL
        srcs = SrcBatch(srcs.R, srcs.doc_srcs, srcs.src_actor, srcs.vv, srcs.entry_off, srcs.keys, srcs.actors, srcs.counters)
    return srcs.to(dev_of(torch))


def download(out, kind):
    raw = {}
    for f, dt in SrcBatch._FIELDS:
        t = getattr(out, f)
        raw[f] = None if t is None else t.cpu().numpy().view(dt)
    raw["kind"] = kind.cpu().numpy()
    return raw


def check_whole_buffers(raw, srcs, want_kinds, want_msgs, tombs="given", kind_given=True, what=""):
    """The live prefix against the restatement (assert_message), then every word outside it."""
    ns, nd, R = srcs.n_srcs, srcs.n_docs, srcs.R
    n = live_sizes(srcs)
    cut = lambda f: None if raw[f] is None else raw[f][: n[f]]  # noqa: E731
    got = SrcBatch(R, *(cut(f) for f, _ in SrcBatch._FIELDS))
    assert_message(got, raw["kind"][:ns] if kind_given else None, srcs, want_kinds, want_msgs, tombs=tombs != "out_null")
    te = int(got.entry_off[ns])
    tt = int(got.tomb_off[ns]) if got.tomb_off is not None else 0
    if tombs != "given":
        assert tt == 0 and (tombs == "out_null" or (got.tomb_off == 0).all()), "a tomb_off passed without tombstones is zeroed"
    first_free = dict(n, keys=te, actors=te, counters=te, tkeys=tt, tactors=tt, tcounters=tt)
    for (f, dt), lo in zip(SrcBatch._FIELDS, first_free.values()):
        if raw[f] is None:
            continue
        tail = raw[f][lo:]
        assert len(tail) >= MARGIN
        bad = np.flatnonzero(tail != (P32 if dt == U32 else P64))
        assert bad.size == 0, "%s %s[%d] = %#x was written (live prefix: %d)" % (what, f, lo + bad[0], int(tail[bad[0]]), lo)
    lo = ns if kind_given else 0
    bad = np.flatnonzero(raw["kind"][lo:] != P8)
    assert bad.size == 0, "%s kind[%d] was written" % (what, lo + bad[0])


def run_async(eng, torch, srcs, peer, tombs="given", kind_given=True, stream=None):
    out, kind = poisoned_out(torch, srcs, tombs)
    out.inputs = (device_input(torch, srcs, tombs), to_dev(torch, peer))  # (alive as long as the output is)
    eng.delta_extract_async(out.inputs[0], out.inputs[1], out, kind=kind if kind_given else None, stream=stream)
    return out, kind


def run_case(eng, torch, case):
    srcs, kinds, msgs, peer = prepared(case)
    out, kind = run_async(eng, torch, srcs, peer, case.tombs, not case.kind_null)
    eng.sync()
    torch.cuda.synchronize()
    return download(out, kind)


# ------------------------------------------------------------- 1. the case table

@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_into_poisoned_buffers(eng, torch, case):
    srcs, kinds, msgs, _ = prepared(case)
    raw = run_case(eng, torch, case)
    check_whole_buffers(raw, srcs, kinds, msgs, case.tombs, not case.kind_null, case.name)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_on_the_host_path(eng, torch, case):
    """crdt_awset_delta_extract_batch: bit-equal to the asynchronous result, trimmed to the totals."""
    srcs, kinds, msgs, peer = prepared(case)
    raw = run_case(eng, torch, case)
    host_in = srcs if case.tombs == "given" else SrcBatch(srcs.R, srcs.doc_srcs, srcs.src_actor, srcs.vv, srcs.entry_off,
                                                           srcs.keys, srcs.actors, srcs.counters)
    msg, kind = eng.delta_extract(host_in, peer)
    assert_message(msg, kind, srcs, kinds, msgs)
    ns = srcs.n_srcs
    assert kind.dtype == U8 and len(kind) == ns
    if not case.kind_null:
        assert (kind == raw["kind"][:ns]).all()
    te, tt = int(raw["entry_off"][ns]), int(msg.tomb_off[ns])
    assert len(msg.keys) == len(msg.actors) == len(msg.counters) == te
    assert len(msg.tkeys) == len(msg.tactors) == len(msg.tcounters) == tt
    sizes = dict(live_sizes(srcs), keys=te, actors=te, counters=te, tkeys=tt, tactors=tt, tcounters=tt)
    for f, n in sizes.items():
        if raw[f] is not None:
            assert len(getattr(msg, f)) == n and (getattr(msg, f) == raw[f][:n]).all(), f


# ------------------------------------------------ 2. stale LDS across the grid stride

def test_second_turn_of_a_wavefront_after_a_heavy_first(eng, torch):
    """More groups than the launch has wavefronts, at R = 64 (a group is one document).  The
    launch has W = min(ceil(n_groups / 4), n_cu * 8) * 4 wavefronts (launch_extract) and
    wavefront i takes groups i, i + W, i + 2 W.  A heavy first group for every wavefront would be
    W x 129 sources x 64 clock words (half a gigabyte at 256 CUs), so every 64th wavefront's
    first document is heavy -- 129 sources with entries and tombstones, everything kept, which
    leaves all 129 slots of the staged arrays and both runs behind -- and the others' hold one
    source.  The documents of the second turn hold four sources: an empty one first and last, one
    the peer covers entirely, one that keeps an entry and a tombstone, under another clock than
    the first turn's.  Five documents make a third turn."""
    R = 64
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    W = n_cu * 8 * 4
    n_docs = 2 * W + 5
    assert min((n_docs + 3) // 4, n_cu * 8) * 4 == W
    assert W % 64 == 0
    Ph, Pl, P2, P3 = clock(R, 0), clock(R, 2), clock(R, 3), clock(R, 5)  # (the second turn sees the actors the first did not)
    heavy = [full_src(Ph, 2, [(3, i % R, 1 + i % 7)], key0=1, step=4, i=i) for i in range(129)]
    templates = {
        "heavy": (heavy, Ph),
        "light": ([small_src(Pl, 0, 0)], Pl),
        "second": ([small_src(P2, 1, 4), small_src(P2, 2, 3), small_src(P2, 3, 0), small_src(P2, 4, 4)], P2),
        "second_b": ([small_src(P3, 1, 4), small_src(P3, 2, 0), small_src(P3, 3, 3), small_src(P3, 4, 4)], P3),
        "third": ([small_src(Pl, 5, 5), small_src(Pl, 6, 4)], Pl),
    }
    done = {k: model.extract_doc_ref(s, P) for k, (s, P) in templates.items()}
    assert done["heavy"][0] == [FULL] * 129 and all(len(m[2]) == 2 and len(m[3]) == 1 for m in done["heavy"][1])
    assert done["second"][0] == [NONE, NONE, DELTA, NONE] and done["second_b"][0] == [NONE, DELTA, NONE, NONE]
    names = [("heavy" if d % 64 == 0 else "light") if d < W else
             ("second" if d % 64 == 0 else "second_b") if d < 2 * W else "third" for d in range(n_docs)]
    per_doc = [templates[k][0] for k in names]
    peer = np.array([x for k in names for x in templates[k][1]], dtype=U64)
    kinds = np.array([x for k in names for x in done[k][0]], U8)
    msgs = [done[k][1] for k in names]
    srcs = src_batch_of(R, per_doc)
    out, kind = run_async(eng, torch, srcs, peer)
    eng.sync()
    torch.cuda.synchronize()
    check_whole_buffers(download(out, kind), srcs, kinds, msgs, what="stride")


# ------------------------------------------------ 3. an error among clean neighbours

@pytest.mark.parametrize("what", ["src_actor_R", "delta_entry_at_R"])
def test_error_among_neighbours(torch, what):
    """A source with src_actor == R, or a DELTA entry dot at actor R, in the middle one of three
    groups: crdt_ctx_sync reports CRDT_E_ACTOR_RANGE (the message of a failed call is not defined
    and not looked at), and the next call on the same engine is exact."""
    R = 4
    n = 3 * (64 // R)
    per_doc = [geo_doc(R, d) for d in range(n)]
    P = clock(R, 20)
    assert P[1] > 0
    bad = (R, [1] * R, [(5, 0, 1)], []) if what == "src_actor_R" else (1, [1] * R, [(5, R, 1)], [])
    per_doc[20] = per_doc[20][:1] + [bad] + per_doc[20][1:]
    peers = [clock(R, d) for d in range(n)]
    with pytest.raises(model.ref.GoPanic):
        expected(Case("bad", R, per_doc, peers))
    e = crdtgpu.Engine(0)
    try:
        held = run_async(e, torch, src_batch_of(R, per_doc), np.array(peers, dtype=U64).reshape(-1))
        assert _code(e.sync) == CRDT_E_ACTOR_RANGE and held
        e.sync()  # cleared
        case = BY_NAME["geo_R3_docs42"]
        srcs, kinds, msgs, _ = prepared(case)
        check_whole_buffers(run_case(e, torch, case), srcs, kinds, msgs, what="after " + what)
    finally:
        e.close()


# ------------------------------------------------ 4. two eager runs are bit-identical

@pytest.mark.parametrize("name", ["run_257", "run_of_128_empties", "e_masks", "t_masks", "geo_R1_docs128", "kinds"])
def test_two_eager_runs_are_bit_identical(eng, torch, name):
    """No atomic decides a position: two runs agree in every word of every array, kinds included."""
    a, b = run_case(eng, torch, BY_NAME[name]), run_case(eng, torch, BY_NAME[name])
    for f in a:
        assert (a[f] == b[f]).all(), f


# ------------------------------------------------ 5. graph capture

def test_graph_capture_of_a_table_case(torch):
    """A case with 257 sources in one group (three staged runs), captured on a reserved context
    and replayed twice into re-poisoned buffers."""
    case = BY_NAME["run_257"]
    srcs, kinds, msgs, peer = prepared(case)
    e = crdtgpu.Engine(0)
    try:
        e.reserve(srcs.n_docs)
        ds, dp = device_input(torch, srcs), to_dev(torch, peer)
        out, kind = poisoned_out(torch, srcs)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.delta_extract_async(ds, dp, out, kind=kind, stream=torch.cuda.current_stream())
        for turn in range(2):
            repoison(torch, out, kind)
            g.replay()
            e.sync(torch.cuda.current_stream())
            torch.cuda.synchronize()
            check_whole_buffers(download(out, kind), srcs, kinds, msgs, what="replay %d" % turn)
    finally:
        e.close()


# ------------------------------------------------ 6. argument errors

def test_argument_errors(eng, torch):
    """Every one of these is refused on the host: nothing is launched, the poisoned output is
    untouched, the call returns CRDT_E_INVALID.  (srcs->vv and the entry columns are not among
    the pointers the call checks: it cannot tell a batch without sources or entries, where they
    may be anything, from one that has some.)"""
    case = BY_NAME["geo_R5_docs13"]
    srcs, kinds, msgs, peer = prepared(case)
    ds, dp = device_input(torch, srcs), to_dev(torch, peer)
    out, kind = poisoned_out(torch, srcs)
    lib, ctx, ref = abi.lib(), eng._ctx, ctypes.byref
    p = dp.data_ptr()

    def call(c, cs, cp, co):
        return lib.crdt_awset_delta_extract_async(c, ref(cs) if cs else None, cp, ref(co) if co else None, None)

    cs, co = ds.c, lambda: out.c_delta_out(kind)
    assert call(None, cs(), p, co()) == CRDT_E_INVALID
    assert call(ctx, None, p, co()) == CRDT_E_INVALID
    assert call(ctx, cs(), p, None) == CRDT_E_INVALID
    assert call(ctx, cs(), None, co()) == CRDT_E_INVALID  # n_docs > 0 without peer clocks
    for field in ("doc_srcs", "src_actor", "entry_off", "tkeys", "tactors", "tcounters"):  # (tomb_off is given)
        s = cs()
        setattr(s, field, None)
        assert call(ctx, s, p, co()) == CRDT_E_INVALID, field
    for R in (0, CRDT_MAX_R + 1):
        s = cs()
        s.R = R
        assert call(ctx, s, p, co()) == CRDT_E_INVALID, R
    for field in ("doc_srcs", "src_actor", "vv", "entry_off", "keys", "actors", "counters",
                  "tomb_off", "tkeys", "tactors", "tcounters"):  # the last four: required because srcs->tomb_off is given
        o = co()
        setattr(o, field, None)
        assert call(ctx, cs(), p, o) == CRDT_E_INVALID, field
    eng.sync()
    torch.cuda.synchronize()
    raw = download(out, kind)
    for f, dt in SrcBatch._FIELDS:
        assert (raw[f] == (P32 if dt == U32 else P64)).all(), f
    assert (raw["kind"] == P8).all()
    # accepted: no documents and no peer clocks -- the three words of an empty message are written
    s = cs()
    s.n_docs = 0
    zero = torch.zeros(1, dtype=torch.int32, device=dev_of(torch))
    s.doc_srcs = zero.data_ptr()
    assert call(ctx, s, None, co()) == 0
    eng.sync()
    torch.cuda.synchronize()
    raw = download(out, kind)
    assert raw["doc_srcs"][0] == 0 and raw["entry_off"][0] == 0 and raw["tomb_off"][0] == 0
    for f, dt in SrcBatch._FIELDS:
        assert (raw[f][1:] == (P32 if dt == U32 else P64)).all(), f
        assert f in ("doc_srcs", "entry_off", "tomb_off") or raw[f][0] == (P32 if dt == U32 else P64), f
    assert (raw["kind"] == P8).all()
    # accepted: kind == NULL
    repoison(torch, out, kind)
    o = co()
    o.kind = None
    assert call(ctx, cs(), p, o) == 0
    eng.sync()
    torch.cuda.synchronize()
    check_whole_buffers(download(out, kind), srcs, kinds, msgs, kind_given=False, what="kind NULL")
