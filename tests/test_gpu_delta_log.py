"""GPU: crdt_awset_delta_join_log_async / crdt_awset_delta_exchange_log_async
(csrc/delta_pair_log.hip) against delta_log_ref (tests/delta_log_cases.py, pinned by
tests/test_delta_log_model.py): the merged state, the kinds and both lists of every
document, flags, counts, offsets and summary, bit-exact, in both directions.

Every written buffer is pre-filled with poison, so each word compared was written by
the call, and every list slot outside a document's live prefix must still hold the
poison afterwards.  The wave path takes a document whose two sides hold at most 64
live entries and 64 live tombstones each, four documents per workgroup; the rest goes
through the worklist to the block path, which steps a window of 1,024 merged
positions.  No test provokes a fault: the error cases are the clamped, reported ones
of the contract.
"""

import ctypes
import random

import numpy as np
import pytest

import crdtgpu
from counter_maps import assert_mixes, map_batch, mixed
from crdtgpu import (CRDT_DELTA_DELTA, CRDT_DELTA_FULL, CRDT_DELTA_NONE, CRDT_E_ACTOR_RANGE, CRDT_E_CAPACITY,
                     CRDT_E_INVALID, CRDT_E_WORKSPACE, abi)
from crdtgpu.batch import AWSetBatch, DiffBuffers, MergeLogBuffers, QueryBatch, QueryBuffers, Replica, TombBatch
from delta_log_cases import at_block_size, case_sets, delta_log_ref, feature_docs, feature_list, feature_pair
from delta_pair_cases import (BLOCK_WINDOW, MAX_C, PAIR_WAVES, assert_direction, on_wave_path, pair_docs, phase2_doc,
                              random_pair)
from helpers import out_doc
from join_log_cases import assert_log, doc_lists, merged_position
from sources_cases import LAYOUTS, make_replica
from test_diff_model import ADDED, CLOCK, REMOVED, UPDATED
from test_gpu_compare import _code, dev_of, host_out, poisoned_out

pytestmark = pytest.mark.gpu

U8, U32, U64 = np.uint8, np.uint32, np.uint64
POISON8 = 77
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


@pytest.fixture(scope="module")
def sets():
    return case_sets()


@pytest.fixture(scope="module")
def random2(sets):
    a, b = sets["random2"]
    return a, b, delta_log_ref(a, b)


# ------------------------------------------------------------------- helpers

def slots_of(state):
    return int(np.asarray(state.offsets)[-1])


def poison(log):
    for f in log.FIELDS:
        t = getattr(log, f)
        if t is not None:
            t.fill_(POISON8 if f in ("flags", "ups_kind") else -1)
    return log


def poisoned_log(torch, n, rem_slots, ups_slots, **kw):
    return poison(MergeLogBuffers(n, rem_slots, ups_slots, device=dev_of(torch), **kw))


def kind_buf(torch, n):
    return torch.full((max(n, 1),), POISON8, dtype=torch.uint8, device=dev_of(torch))


def kinds_host(t, n):
    return t.cpu().numpy().view(U8)[:n]


def exchange_on_device(eng, torch, a, b, da=None, db=None, stream=None, kinds=True, **kw):
    """(o1, o2, k1, k2, l1, l2) on the device after one delta_exchange_log_async; not synced."""
    n, R = a.n_docs, a.state.R
    dev = dev_of(torch)
    sa, sb = slots_of(a.state), slots_of(b.state)
    o1, o2 = poisoned_out(torch, n, R, sa + sb), poisoned_out(torch, n, R, sa + sb)
    k1, k2 = (kind_buf(torch, n), kind_buf(torch, n)) if kinds else (None, None)
    l1, l2 = poisoned_log(torch, n, sa, sb, **kw), poisoned_log(torch, n, sb, sa, **kw)
    eng.delta_exchange_log_async(da or a.to(dev), db or b.to(dev), o1, o2, l1, l2, k1, k2, stream=stream)
    return o1, o2, k1, k2, l1, l2


def join_on_device(eng, torch, dst, src, kinds=True, **kw):
    """(out, kind, log) after one delta_join_log_async of dst.state <- src; not synced."""
    n, R = dst.n_docs, dst.state.R
    dev = dev_of(torch)
    sd, ss = slots_of(dst.state), slots_of(src.state)
    o, k = poisoned_out(torch, n, R, sd + ss), (kind_buf(torch, n) if kinds else None)
    lg = poisoned_log(torch, n, sd, ss, **kw)
    eng.delta_join_log_async(dst.to(dev).state, src.to(dev), o, lg, k)
    return o, k, lg


def assert_poison_kept(g, want, what=""):
    """Every list slot that holds no record still holds the poison."""
    for f in LIST_FIELDS:
        if g[f] is None:
            continue
        keep = np.ones(len(g[f]), bool)
        keep[want.rem_idx if f.startswith("rem") else want.ups_idx] = False
        bad = POISON8 if f == "ups_kind" else (2 ** 64 - 1 if g[f].dtype == U64 else 2 ** 32 - 1)
        assert (g[f][keep] == bad).all(), "%s %s: a slot outside the live prefixes was written" % (what, f)


def assert_dir(out, kind, log, dst, src, lref, kinds_want, a, b, what):
    assert lref.rc == 0
    h = host_out(out)
    assert_direction(h, lref.out, a.state, b.state, what)
    n = dst.n_docs
    if kind is not None:
        g = kinds_host(kind, n)
        if not (g == kinds_want).all():
            d = int(np.nonzero(g != kinds_want)[0][0])
            raise AssertionError("%s kind differs first at document %d: gpu %d, expected %d" % (what, d, g[d], kinds_want[d]))
    g = log.numpy()
    assert_log(g, lref, what)
    assert_poison_kept(g, lref, what)
    return h, g


def assert_exchange(got, a, b, want=None):
    want = want or delta_log_ref(a, b)
    o1, o2, k1, k2, l1, l2 = got
    r1 = assert_dir(o1, k1, l1, a, b, want.ab, want.pair.kind_ab, a, b, "a <- b")
    r2 = assert_dir(o2, k2, l2, b, a, want.ba, want.pair.kind_ba, a, b, "b <- a")
    return r1, r2, want


def check_exchange(eng, torch, a, b, want=None, **kw):
    got = exchange_on_device(eng, torch, a, b, **kw)
    eng.sync()
    return assert_exchange(got, a, b, want)


def same_docs(x, y, n, R):
    for d in range(n):
        assert out_doc(x, d, R) == out_doc(y, d, R), d


def same_records(g1, g2, lref):
    for f in ("flags", "summary", "rem_offsets", "rem_counts", "ups_offsets", "ups_counts"):
        if g1[f] is not None and g2[f] is not None:
            assert (g1[f] == g2[f]).all(), f
    for f in LIST_FIELDS:
        if g1[f] is not None and g2[f] is not None:
            idx = lref.rem_idx if f.startswith("rem") else lref.ups_idx
            assert (g1[f][idx] == g2[f][idx]).all(), f


def host_state(out):
    h = host_out(out)
    return AWSetBatch(out.R, h.offsets, h.keys, h.actors, h.counters, h.vv, counts=h.counts)


# ------------------------------------------------------------ 1. random parity

@pytest.mark.parametrize("R", [1, 2, 5, 64])
def test_random_parity(eng, torch, sets, R):
    """300 small documents in the three kinds: the exchange, and each direction's join
    equal to its half of the exchange."""
    a, b = sets["random%d" % R]
    n = a.n_docs
    assert n % PAIR_WAVES == 0 and n > PAIR_WAVES
    (h1, g1), (h2, g2), want = check_exchange(eng, torch, a, b)
    assert {int(k) for k in want.pair.kind_ab} == {CRDT_DELTA_NONE, CRDT_DELTA_DELTA, CRDT_DELTA_FULL}
    for dst, src, lref, kw, h, g, what in ((a, b, want.ab, want.pair.kind_ab, h1, g1, "join a <- b"),
                                           (b, a, want.ba, want.pair.kind_ba, h2, g2, "join b <- a")):
        o, k, lg = join_on_device(eng, torch, dst, src)
        eng.sync()
        hj, gj = assert_dir(o, k, lg, dst, src, lref, kw, a, b, what)
        same_docs(hj, h, n, R)
        same_records(gj, g, lref)


# ------------------------------------------------------------ 2. dispatch edges

@pytest.fixture(scope="module")
def edges(sets):
    a, b = sets["edges"]
    return a, b, delta_log_ref(a, b)


def test_dispatch_edges_and_features(eng, torch, edges):
    """0 / 1 / 63 / 64 / 65 / 129 entries a side, 0 / 1 / 64 / 65 tombstones, three modes,
    documents of 3,000 entries a side (three windows of 1,024), every feature document at
    both sizes among them; n_docs is no multiple of the workgroup's four."""
    a, b, want = edges
    assert a.n_docs % PAIR_WAVES != 0
    assert max(len(a.state.doc(d)[0]) for d in range(a.n_docs - 40, a.n_docs)) >= 2 * BLOCK_WINDOW
    check_exchange(eng, torch, a, b, want)


def _straddle_doc(shift):
    """A DELTA document on the block path: the common key X1 (moved to b's dot in phase 1,
    removed by b's tombstone in phase 2) has its dst entry at merged position
    WINDOW - 1 + shift and its src entry at WINDOW + shift; the common key X2 (UPDATED)
    sits likewise at 2 * WINDOW - 1 + shift / 2 * WINDOW + shift."""
    W = BLOCK_WINDOW
    ea, eb, key = [], [], 1

    def fill(count):
        nonlocal key
        for i in range(count):
            (ea if i % 2 == 0 else eb).append((key, 0, 1) if i % 2 == 0 else (key, 1, 6))
            key += 3

    fill(W - 1 + shift)
    x1 = key
    key += 3
    ea.append((x1, 1, 2))
    eb.append((x1, 1, 7))
    fill(W - 2)
    x2 = key
    key += 3
    ea.append((x2, 1, 2))
    eb.append((x2, 1, 7))
    fill(41)
    return (ea, [], [3, 4]), (eb, [(x1, 1, 8)], [8, 8]), x1, x2


def test_a_window_boundary_splits_the_update_then_remove_key(eng, torch):
    W = BLOCK_WINDOW
    docs = [_straddle_doc(s) for s in (-1, 0, 1)]
    a = make_replica(2, [d[0] for d in docs], actor=0)
    b = make_replica(2, [d[1] for d in docs], actor=1)
    for i, (s, (_, _, x1, x2)) in enumerate(zip((-1, 0, 1), docs)):
        assert merged_position(a.state, b.state, i, x1, "d") == W - 1 + s
        assert merged_position(a.state, b.state, i, x1, "s") == W + s
        assert merged_position(a.state, b.state, i, x2, "d") == 2 * W - 1 + s
        assert merged_position(a.state, b.state, i, x2, "s") == 2 * W + s
        assert not on_wave_path(a, b, i)
    (_, g1), _, want = check_exchange(eng, torch, a, b)
    assert (want.pair.kind_ab == CRDT_DELTA_DELTA).all()
    for i, (_, _, x1, x2) in enumerate(docs):
        rem, ups = doc_lists(g1, i)
        assert rem == [(x1, 1, 2)]  # with the dot it had in dst, and no upsert record
        assert [u for u in ups if u[3] == UPDATED] == [(x2, 1, 7, UPDATED)] and x1 not in [u[0] for u in ups]


# -------------------------------------------------------- 3. feature documents

def test_each_feature_document_alone(eng, torch):
    for name, size, x, y in feature_list(2):
        a, b = make_replica(2, [x], actor=0), make_replica(2, [y], actor=1)
        (_, g1), _, want = check_exchange(eng, torch, a, b)
        rem, ups = doc_lists(g1, 0)
        if name == "p1_update_p2_remove":
            assert rem == [(40, 1, 2)] and ups == [] and int(g1["flags"][0]) == REMOVED | CLOCK, size
        if name == "none_src_ahead":
            assert int(g1["flags"][0]) == 0 and not g1["summary"].any(), size
        if name == "tomb_absent_key":
            assert int(g1["flags"][0]) == CLOCK and g1["summary"].tolist() == [0, 0, 0, 0, 1], size


def test_feature_documents_among_neighbours(eng, torch, sets):
    a, b = sets["features"]
    check_exchange(eng, torch, a, b)
    a, b = feature_pair(2, slack=2, with_counts=True, garbage=np.random.default_rng(3))
    check_exchange(eng, torch, a, b)


@pytest.mark.parametrize("n_docs", [1, 3, 5, 4 * 300 + 1])
def test_grid_edges(eng, torch, n_docs):
    """n_docs no multiple of the four documents of a workgroup; more documents than one
    workgroup covers, the block path's among them."""
    a, b = random_pair(8200 + n_docs, n_docs, 3, max_e=(70 if n_docs > 5 else 10), max_t=3)
    check_exchange(eng, torch, a, b)


# ------------------------------------------------------------------ 4. layouts

def _layout(i, seed):
    lay = dict(LAYOUTS[i])
    if lay.pop("garbage", False):
        lay["garbage"] = np.random.default_rng(seed)
    return lay


@pytest.mark.parametrize("la,lb", [(3, 0), (1, 2), (2, 3), (0, 1)])
def test_slot_layouts(eng, torch, la, lb):
    """Slack with stale values behind the live prefixes, zero slack, counts given and NULL,
    the two replicas laid out independently, a lead before the first document."""
    a, b = random_pair(8300 + la, 300, 3, max_e=70, max_t=70, lay_a=dict(_layout(la, 1), lead=la),
                       lay_b=dict(_layout(lb, 2), lead=2 * lb))
    assert sum(not on_wave_path(a, b, d) for d in range(a.n_docs)) > 5
    check_exchange(eng, torch, a, b)


@pytest.mark.parametrize("ta,tb", [(False, True), (True, False), (False, False)])
def test_without_tombstones(eng, torch, ta, tb):
    a, b = random_pair(8400, 300, 2, max_e=70, tombs_a=ta, tombs_b=tb)
    assert (a.tombs is None) == (not ta) and (b.tombs is None) == (not tb)
    check_exchange(eng, torch, a, b)


def test_actor_per_document_and_scalar(eng, torch):
    a, b = random_pair(8500, 300, 5, max_e=70, doc_actors=True)
    assert a.doc_actor is not None and len(set(a.doc_actor.tolist())) == 5
    check_exchange(eng, torch, a, b)
    for r in (a, b):
        r.doc_actor[:] = 3
    (h1, g1), (h2, g2), want = check_exchange(eng, torch, a, b)
    sa, sb = Replica(a.state, a.tombs, actor=3), Replica(b.state, b.tombs, actor=3)
    (s1, q1), (s2, q2), _ = check_exchange(eng, torch, sa, sb)
    same_docs(s1, h1, a.n_docs, 5)
    same_records(q1, g1, want.ab)
    same_records(q2, g2, want.ba)


# ------------------------------------------ 5. agreement with the existing calls

def test_state_and_kinds_equal_the_plain_delta_exchange(eng, torch, random2):
    a, b, want = random2
    dev = dev_of(torch)
    da, db = a.to(dev), b.to(dev)
    o1, o2, k1, k2, _, _ = exchange_on_device(eng, torch, a, b, da, db)
    n, R = a.n_docs, 2
    s = slots_of(a.state) + slots_of(b.state)
    p1, p2, q1, q2 = poisoned_out(torch, n, R, s), poisoned_out(torch, n, R, s), kind_buf(torch, n), kind_buf(torch, n)
    eng.delta_exchange_async(da, db, p1, p2, q1, q2)
    eng.sync()
    for x, y in ((o1, p1), (o2, p2)):
        hx, hy = host_out(x), host_out(y)
        same_docs(hx, hy, n, R)
        assert (hx.offsets[: n + 1] == hy.offsets[: n + 1]).all() and (hx.counts[:n] == hy.counts[:n]).all()
        assert (hx.vv[: n * R] == hy.vv[: n * R]).all()
    assert (kinds_host(k1, n) == kinds_host(q1, n)).all() and (kinds_host(k2, n) == kinds_host(q2, n)).all()


def test_log_equals_the_device_diff_of_dst_and_out(eng, torch, edges):
    """flags, per-document counts and summary equal crdt_awset_diff_async(dst, out)'s, and
    its packed lists equal the log's lists read document by document."""
    a, b, want = edges
    dev = dev_of(torch)
    da, db = a.to(dev), b.to(dev)
    o1, o2, _, _, l1, l2 = exchange_on_device(eng, torch, a, b, da, db)
    for dst, out, log, lref in ((da.state, o1, l1, want.ab), (db.state, o2, l2, want.ba)):
        diff = DiffBuffers(a.n_docs, log.rem_slots, log.ups_slots, device=dev)
        eng.diff_async(dst, out.as_batch(), diff)
        eng.sync()
        g, df = log.numpy(), diff.numpy()
        assert (g["flags"] == df["flags"]).all() and (g["summary"] == df["summary"]).all()
        assert (g["rem_counts"] == np.diff(df["rem_off"])).all() and (g["ups_counts"] == np.diff(df["ups_off"])).all()
        for f in LIST_FIELDS:
            idx = lref.rem_idx if f.startswith("rem") else lref.ups_idx
            assert (g[f][idx] == df[f][: len(idx)]).all(), f


def test_optional_outputs(eng, torch, random2):
    """summary, ups_kind and the kinds passed as NULL leave the rest equal."""
    a, b, want = random2
    got = exchange_on_device(eng, torch, a, b, kinds=False, kind=False, summary=False)
    eng.sync()
    assert_exchange(got, a, b, want)
    o, k, lg = join_on_device(eng, torch, a, b, kinds=False, summary=False)
    eng.sync()
    assert_dir(o, k, lg, a, b, want.ab, want.pair.kind_ab, a, b, "join")


# -------------------------------------------------------------- 6. composition

def test_exchange_output_is_the_next_calls_state(eng, torch):
    """Documents at capacity offsets with slack behind the live prefixes: the outputs of
    one logged exchange, on the device, are the states of the next."""
    a, b = random_pair(8600, 300, 3, max_e=70, max_t=70)
    dev = dev_of(torch)
    da, db = a.to(dev), b.to(dev)
    o1, o2, _, _, _, _ = exchange_on_device(eng, torch, a, b, da, db)
    a2d, b2d = Replica(o1.as_batch(), da.tombs, actor=a.actor), Replica(o2.as_batch(), db.tombs, actor=b.actor)
    eng.sync()
    a2, b2 = Replica(host_state(o1), a.tombs, actor=a.actor), Replica(host_state(o2), b.tombs, actor=b.actor)
    assert int(a2.state.offsets[-1]) > int(a2.state.counts.sum())
    (_, g1), _, want = check_exchange(eng, torch, a2, b2, da=a2d, db=b2d)
    assert len(set(want.pair.kind_ab.tolist())) >= 2 and not (g1["flags"] & ADDED).all()


def test_a_removed_list_is_a_tomb_batch(eng, torch, edges):
    """The removed list, wrapped as a TombBatch as it stands, answers crdt_tomb_has_async:
    every removed key is found with its dot, a key the merge kept is not."""
    a, b, want = edges
    o, k, lg = join_on_device(eng, torch, a, b)
    per_doc, exp = [], []
    for d in range(a.n_docs):
        rem, _ = doc_lists(want.ab.log, d)
        kept = [e[0] for e in out_doc(want.ab.out, d, 2)[0][:2]]
        per_doc.append([r[0] for r in rem] + kept)
        exp += [(1, r[1], r[2]) for r in rem] + [(0, 0, 0)] * len(kept)
    q = QueryBatch.from_lists(per_doc)
    res = QueryBuffers(q.n_queries, device=dev_of(torch))
    eng.tomb_has_async(lg.removed(), q.to(dev_of(torch)), res)
    eng.sync()
    found, actors, counters = res.numpy()
    assert found.tolist() == [w[0] for w in exp] and sum(found.tolist()) > 100
    hit = found.astype(bool)
    assert actors[hit].tolist() == [w[1] for w in exp if w[0]] and counters[hit].tolist() == [w[2] for w in exp if w[0]]


# ------------------------------------------------------------ 7. wide counters

def _mapped(rep, tab):
    return Replica(map_batch(rep.state, tab), map_batch(rep.tombs, tab) if rep.tombs is not None else None,
                   actor=rep.actor, doc_actor=rep.doc_actor)


@pytest.mark.parametrize("case", ["features", "random5"])
def test_wide_counters(eng, torch, sets, case):
    """The same documents with every counter and clock value through the order-preserving
    maps of tests/counter_maps.py (up to 2^32, 2^63, 2^64 - 1): equal to the reference on
    the mapped inputs, with the kinds, flags and counts of the unmapped run."""
    a, b = sets[case]
    plain = delta_log_ref(a, b)
    tab = mixed(MAX_C, 3)
    am, bm = _mapped(a, tab), _mapped(b, tab)
    (_, g1), (_, g2), want = check_exchange(eng, torch, am, bm)
    if case == "random5":
        assert_mixes(want.pair.ab, tab, "a <- b")
        assert_mixes(want.pair.ba, tab, "b <- a")
    big = np.concatenate([want.ab.log["rem_counters"], want.ab.log["ups_counters"], np.asarray(want.pair.ab.vv)])
    assert (big >= 2 ** 32).any()
    assert (want.pair.kind_ab == plain.pair.kind_ab).all() and (want.pair.kind_ba == plain.pair.kind_ba).all()
    for g, p in ((g1, plain.ab), (g2, plain.ba)):
        for f in ("flags", "summary", "rem_counts", "ups_counts"):
            assert (g[f] == p.log[f]).all(), f


# ------------------------------------------------------- 8. errors and ordering

def small_pair(R=2):
    x, y = phase2_doc(R)
    rng = random.Random(8700)
    docs = [pair_docs(rng, R, 4, 5, 1, 2, m) for m in (0, 1, 2)] + [(x, y)]
    return [p[0] for p in docs], [p[1] for p in docs]


@pytest.mark.parametrize("size", ["wave", "block"])
def test_actor_range_on_the_path_select(eng, torch, size):
    """Counter(s) at s == R is the reference's panic; s > R is "never seen": FULL."""
    da, db = small_pair()
    if size == "block":
        da, db = zip(*(at_block_size(x, y) for x, y in zip(da, db)))
        da, db = list(da), list(db)
    a, b = make_replica(2, da, actor=0), make_replica(2, db, actor=2)
    assert on_wave_path(a, b, 0) == (size == "wave")
    exchange_on_device(eng, torch, a, b)
    assert _code(eng.sync) == CRDT_E_ACTOR_RANGE
    eng.sync()  # cleared
    a, b = make_replica(2, da, actor=0), make_replica(2, db, actor=3)
    _, _, want = check_exchange(eng, torch, a, b)
    assert (want.pair.kind_ab == CRDT_DELTA_FULL).all()


@pytest.mark.parametrize("size", [3, 80])
def test_actor_range_on_a_has_dot(eng, torch, size):
    """A src entry dot with actor == R on the DELTA path (HasDot against dst's clock), at
    wave and at block size; the oracle reports the same.  actor > R is "never seen"."""
    rng = random.Random(8800 + size)
    x, y = pair_docs(rng, 2, size, size, 0, 0, 1)
    y = ([(k, 2, c) if i == 1 else (k, a_, c) for i, (k, a_, c) in enumerate(y[0])], y[1], y[2])
    a, b = make_replica(2, [x], actor=0), make_replica(2, [y], actor=1)
    want = delta_log_ref(a, b)
    assert want.ab.rc == CRDT_E_ACTOR_RANGE and int(want.pair.kind_ab[0]) != CRDT_DELTA_FULL
    join_on_device(eng, torch, a, b)
    assert _code(eng.sync) == CRDT_E_ACTOR_RANGE
    eng.sync()  # cleared
    y2 = ([(k_, 3, c) if a_ == 2 else (k_, a_, c) for k_, a_, c in y[0]], y[1], y[2])
    check_exchange(eng, torch, a, make_replica(2, [y2], actor=1))


@pytest.mark.parametrize("size", ["wave", "block"])
@pytest.mark.parametrize("which", ["entries", "tombstones"])
def test_count_above_slots_is_clamped(eng, torch, which, size):
    if size == "wave":
        da, db = small_pair()
    else:
        rng = random.Random(8900)
        docs = [pair_docs(rng, 2, 70, 70, 70, 70, m) for m in (0, 1, 2, 1)]
        da, db = [p[0] for p in docs], [p[1] for p in docs]
    a = make_replica(2, da, actor=0, slack=1, with_counts=True)
    b = make_replica(2, db, actor=1, slack=1, with_counts=True)
    assert on_wave_path(a, b, 1) == (size == "wave")
    cols = b.state if which == "entries" else b.tombs
    cols.counts[1] = int(cols.offsets[2]) - int(cols.offsets[1]) + 9
    got = exchange_on_device(eng, torch, a, b)
    assert _code(eng.sync) == CRDT_E_CAPACITY
    eng.sync()  # cleared
    # the other documents are what they would be without the bad count
    cols.counts[1] = int(cols.offsets[2]) - int(cols.offsets[1]) - 1
    want = delta_log_ref(a, b)
    for out, log, lref in ((got[0], got[4], want.ab), (got[1], got[5], want.ba)):
        h, g = host_out(out), log.numpy()
        for d in (0, 2, 3):
            assert out_doc(h, d, 2) == out_doc(lref.out, d, 2), d
            assert doc_lists(g, d) == doc_lists(lref.log, d) and int(g["flags"][d]) == int(lref.log["flags"][d]), d


def test_argument_errors(eng, torch):
    """Every one of these is refused on the host: nothing is launched."""
    da, db = small_pair()
    dev = dev_of(torch)
    a, b = make_replica(2, da, actor=0).to(dev), make_replica(2, db, actor=1).to(dev)
    b3 = make_replica(2, db[:3], actor=1).to(dev)
    bR = make_replica(3, small_pair(3)[1], actor=1).to(dev)
    n, R, slots = 4, 2, 64
    o1, o2 = poisoned_out(torch, n, R, slots), poisoned_out(torch, n, R, slots)
    l1, l2 = poisoned_log(torch, n, slots, slots), poisoned_log(torch, n, slots, slots)
    k1, k2 = kind_buf(torch, n), kind_buf(torch, n)
    lib, ctx, ref = abi.lib(), eng._ctx, ctypes.byref
    r = lambda x: ref(x) if x is not None else None  # noqa: E731

    def xchg(ca, cb, c1, c2, g1, g2, p1=None, p2=None):
        return lib.crdt_awset_delta_exchange_log_async(ctx, r(ca), r(cb), r(c1), r(c2), p1, p2, r(g1), r(g2), None)

    def join(cd, cs, co, g, p=None):
        return lib.crdt_awset_delta_join_log_async(ctx, r(cd), r(cs), r(co), p, r(g), None)

    ca, cb, cst = a.c(), b.c(), a.state.c()
    args = [ca, cb, o1.c(), o2.c(), l1.c(), l2.c()]
    for i in range(6):  # any NULL among the arguments
        bad = list(args)
        bad[i] = None
        assert xchg(*bad) == CRDT_E_INVALID, i
    for i, bad in enumerate(([None, cb, o1.c(), l1.c()], [cst, None, o1.c(), l1.c()], [cst, cb, None, l1.c()],
                             [cst, cb, o1.c(), None])):
        assert join(*bad) == CRDT_E_INVALID, i
    assert lib.crdt_awset_delta_join_log_async(None, ref(cst), ref(cb), ref(args[2]), None, ref(args[4]), None) == CRDT_E_INVALID
    assert xchg(ca, b3.c(), *args[2:]) == CRDT_E_INVALID  # n_docs
    assert xchg(ca, bR.c(), *args[2:]) == CRDT_E_INVALID  # R
    assert join(cst, bR.c(), o1.c(), l1.c()) == CRDT_E_INVALID
    no_state = b.c()
    no_state.state = None
    assert xchg(ca, no_state, *args[2:]) == CRDT_E_INVALID
    wide_state = a.state.c()
    wide_state.R = 65
    wide = abi.CReplica(ctypes.addressof(wide_state), None, None, 0)
    assert xchg(wide, wide, *args[2:]) == CRDT_E_INVALID  # R out of range
    no_off = b.tombs.c()
    no_off.offsets = None
    cs = b.state.c()
    bad_t = abi.CReplica(ctypes.addressof(cs), ctypes.addressof(no_off), None, 1)
    assert xchg(ca, bad_t, *args[2:]) == CRDT_E_INVALID  # a tomb batch without offsets
    assert join(cst, bad_t, o1.c(), l1.c()) == CRDT_E_INVALID
    for f in ("offsets", "counts", "keys", "actors", "counters", "vv"):  # a required field NULL
        c = o1.c()
        setattr(c, f, None)
        assert xchg(ca, cb, c, o2.c(), l1.c(), l2.c()) == CRDT_E_INVALID, f
        assert xchg(ca, cb, o2.c(), c, l1.c(), l2.c()) == CRDT_E_INVALID, f
        assert join(cst, cb, c, l1.c()) == CRDT_E_INVALID, f
        c = o2.c()  # the two directions share no array
        setattr(c, f, getattr(o1.c(), f))
        assert xchg(ca, cb, o1.c(), c, l1.c(), l2.c()) == CRDT_E_INVALID, f
    for f in MergeLogBuffers.FIELDS:
        if f not in ("summary", "ups_kind"):
            g = l1.c()
            setattr(g, f, None)
            assert join(cst, cb, o1.c(), g) == CRDT_E_INVALID, f
            assert xchg(ca, cb, o1.c(), o2.c(), g, l2.c()) == CRDT_E_INVALID, f
            assert xchg(ca, cb, o1.c(), o2.c(), l2.c(), g) == CRDT_E_INVALID, f
        g = l2.c()  # two written arrays starting at one address, across the logs
        setattr(g, f, getattr(l1.c(), f))
        assert xchg(ca, cb, o1.c(), o2.c(), l1.c(), g) == CRDT_E_INVALID, f
    for f, g_ in (("rem_keys", "ups_keys"), ("rem_counts", "ups_counts"), ("rem_keys", "rem_counters"),
                  ("flags", "ups_kind"), ("rem_offsets", "ups_offsets")):  # within one log
        g = l1.c()
        setattr(g, f, getattr(l1.c(), g_))
        assert join(cst, cb, o1.c(), g) == CRDT_E_INVALID, (f, g_)
    for f, of in (("rem_keys", "keys"), ("ups_counters", "counters"), ("rem_actors", "actors"), ("rem_counts", "counts"),
                  ("ups_offsets", "offsets"), ("ups_keys", "vv")):  # a log array against a state array
        g = l1.c()
        setattr(g, f, getattr(o1.c(), of))
        assert join(cst, cb, o1.c(), g) == CRDT_E_INVALID, (f, of)
    # the kinds are written arrays too
    assert xchg(*args, k1.data_ptr(), k1.data_ptr()) == CRDT_E_INVALID
    assert xchg(*args, l1.flags.data_ptr(), k2.data_ptr()) == CRDT_E_INVALID
    assert join(cst, cb, o1.c(), l1.c(), l1.ups_kind.data_ptr()) == CRDT_E_INVALID
    # a written array starting where an input array of the same kind starts
    for f, src in (("keys", a.state.keys), ("counters", b.state.keys), ("vv", b.state.vv), ("actors", a.state.actors),
                   ("offsets", b.state.offsets), ("keys", b.tombs.keys), ("counters", a.tombs.counters),
                   ("actors", b.tombs.actors), ("counts", b.tombs.offsets)):
        c = o1.c()
        setattr(c, f, src.data_ptr())
        assert xchg(ca, cb, c, o2.c(), l1.c(), l2.c()) == CRDT_E_INVALID, f
        assert xchg(ca, cb, o2.c(), c, l1.c(), l2.c()) == CRDT_E_INVALID, f
    # (the join reads nothing of a beyond its state: only the exchange refuses a's tombstones)
    for f, src, join_too in (("rem_keys", a.state.keys, True), ("ups_keys", b.tombs.keys, True),
                             ("rem_counters", a.state.vv, True), ("ups_actors", b.state.actors, True),
                             ("rem_offsets", a.state.offsets, True), ("ups_offsets", b.tombs.offsets, True),
                             ("rem_counts", a.tombs.actors, False), ("summary", b.state.offsets, True),
                             ("ups_counters", a.tombs.counters, False)):
        g = l1.c()
        setattr(g, f, src.data_ptr())
        assert xchg(ca, cb, o1.c(), o2.c(), l2.c(), g) == CRDT_E_INVALID, f
        if join_too:
            assert join(cst, cb, o1.c(), g) == CRDT_E_INVALID, f
    eng.sync()
    for o in (o1, o2):
        for t in (o.offsets, o.counts, o.actors):
            assert (t.cpu().numpy().view(U32) == 2 ** 32 - 1).all()
        for t in (o.keys, o.counters, o.vv):
            assert (t.cpu().numpy().view(U64) == 2 ** 64 - 1).all()
    for lg in (l1, l2):
        assert (lg.flags.cpu().numpy() == POISON8).all() and (lg.rem_counts.cpu().numpy().view(U32) == 2 ** 32 - 1).all()
        assert (lg.summary.cpu().numpy().view(U32) == 2 ** 32 - 1).all()
    assert (kinds_host(k1, n) == POISON8).all() and (kinds_host(k2, n) == POISON8).all()


@pytest.mark.parametrize("summary", [True, False])
def test_no_documents(eng, torch, summary):
    dev = dev_of(torch)
    z = lambda dt: torch.zeros(1, dtype=dt, device=dev)  # noqa: E731
    st = AWSetBatch(2, z(torch.int32), z(torch.int64), z(torch.int32), z(torch.int64), z(torch.int64))
    e = Replica(st, TombBatch(z(torch.int32), z(torch.int64), z(torch.int32), z(torch.int64)), actor=1)
    assert e.n_docs == 0
    o1, o2 = poisoned_out(torch, 1, 2, 4), poisoned_out(torch, 1, 2, 4)
    l1, l2 = poisoned_log(torch, 0, 4, 4, summary=summary), poisoned_log(torch, 0, 4, 4, summary=summary)
    k = kind_buf(torch, 0)
    eng.delta_exchange_log_async(e, e, o1, o2, l1, l2, k, None)
    eng.sync()
    for o, lg in ((o1, l1), (o2, l2)):
        assert (o.keys.cpu().numpy().view(U64) == 2 ** 64 - 1).all() and int(o.counts.cpu().numpy().view(U32)[0]) == 2 ** 32 - 1
        if summary:
            assert not lg.summary.cpu().numpy().any()  # zeroed
        assert int(lg.flags.cpu().numpy()[0]) == POISON8 and int(lg.rem_offsets.cpu().numpy().view(U32)[0]) == 2 ** 32 - 1
    assert int(k.cpu().numpy()[0]) == POISON8
    poison(l1)
    eng.delta_join_log_async(st, e, o1, l1, k)
    eng.sync()
    if summary:
        assert not l1.summary.cpu().numpy().any()
    assert (l1.rem_keys.cpu().numpy().view(U64) == 2 ** 64 - 1).all()


def test_graph_capture(torch):
    """Captured on a reserved context, replayed with b's clocks changed in between, equal to
    eager; on an unreserved context the capture is refused with CRDT_E_WORKSPACE and
    launches nothing."""
    a, b = random_pair(9000, 1100, 2, max_e=70, max_t=3)
    n, R = a.n_docs, 2
    assert n > 1024  # (a fresh context's workspace holds 1,024 documents)
    assert sum(not on_wave_path(a, b, d) for d in range(n)) > 20
    dev = dev_of(torch)
    sa, sb = slots_of(a.state), slots_of(b.state)
    e = crdtgpu.Engine(0)
    try:
        da, db = a.to(dev), b.to(dev)
        o1, o2 = poisoned_out(torch, n, R, sa + sb), poisoned_out(torch, n, R, sa + sb)
        l1, l2 = poisoned_log(torch, n, sa, sb), poisoned_log(torch, n, sb, sa)
        k1, k2 = kind_buf(torch, n), kind_buf(torch, n)
        g0 = torch.cuda.CUDAGraph()
        with pytest.raises(crdtgpu.CrdtError) as ei:
            with torch.cuda.graph(g0):
                e.delta_exchange_log_async(da, db, o1, o2, l1, l2, k1, k2, stream=torch.cuda.current_stream())
        assert ei.value.code == CRDT_E_WORKSPACE
        torch.cuda.synchronize()
        assert (l1.flags.cpu().numpy() == POISON8).all() and (o1.counts.cpu().numpy().view(U32) == 2 ** 32 - 1).all()
        assert (l1.summary.cpu().numpy().view(U32) == 2 ** 32 - 1).all() and (kinds_host(k1, n) == POISON8).all()
        e.reserve(n)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.delta_exchange_log_async(da, db, o1, o2, l1, l2, k1, k2, stream=torch.cuda.current_stream())
        for vv_src in (a, b):  # b's clocks change between replays: other kinds, other records
            db.state.vv.copy_(vv_src.state.to(dev).vv)
            hb = Replica(AWSetBatch(R, b.state.offsets, b.state.keys, b.state.actors, b.state.counters, vv_src.state.vv),
                         b.tombs, actor=b.actor)
            for o in (o1, o2):
                for t in (o.offsets, o.counts, o.keys, o.actors, o.counters, o.vv):
                    t.fill_(-1)
            for x in (l1, l2):
                poison(x)
            k1.fill_(POISON8)
            k2.fill_(POISON8)
            g.replay()
            e.sync(torch.cuda.current_stream())
            (h1, g1), _, want = assert_exchange((o1, o2, k1, k2, l1, l2), a, hb)
            eager = exchange_on_device(e, torch, a, hb)
            e.sync()
            same_docs(host_out(eager[0]), h1, n, R)
            same_records(eager[4].numpy(), g1, want.ab)
    finally:
        e.close()


def test_ordered_after_a_call_on_another_stream(eng, torch, random2):
    """The logged exchange reads the outputs of a plain delta exchange issued on another stream."""
    a, b, want = random2
    dev = dev_of(torch)
    n, R = a.n_docs, 2
    s = slots_of(a.state) + slots_of(b.state)
    da, db = a.to(dev), b.to(dev)
    from crdtgpu.batch import OutBuffers

    o1, o2 = OutBuffers(n, R, s, device=dev), OutBuffers(n, R, s, device=dev)
    for o in (o1, o2):
        for t in (o.offsets, o.counts, o.keys, o.actors, o.counters, o.vv):
            t.zero_()  # a logged exchange that ran first would see two empty batches
    p1, p2 = poisoned_out(torch, n, R, 2 * s), poisoned_out(torch, n, R, 2 * s)
    l1, l2 = poisoned_log(torch, n, s, s), poisoned_log(torch, n, s, s)
    k1, k2 = kind_buf(torch, n), kind_buf(torch, n)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.delta_exchange_async(da, db, o1, o2, stream=s1)
    eng.delta_exchange_log_async(Replica(o1.as_batch(), da.tombs, actor=a.actor),
                                 Replica(o2.as_batch(), db.tombs, actor=b.actor), p1, p2, l1, l2, k1, k2, stream=s2)
    eng.sync(s2)
    a2, b2 = Replica(host_state(o1), a.tombs, actor=a.actor), Replica(host_state(o2), b.tombs, actor=b.actor)
    assert int(a2.state.counts.sum()) > 0
    assert_exchange((p1, p2, k1, k2, l1, l2), a2, b2)
