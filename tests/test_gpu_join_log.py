"""GPU: crdt_awset_join_log_async / crdt_awset_exchange_log_async (csrc/join_log.hip)
against join_log_ref (tests/join_log_cases.py, pinned by tests/test_join_log_model.py):
the merged state and both lists of every document, flags, counts, offsets and summary,
bit-exact, in both directions.

Every written buffer is pre-filled with poison, so each word compared was written by the
call.  The wave path takes a document whose two sides hold at most 64 live entries
(kLogWaveMax), 32 documents per workgroup (kLogWaves x kLogDocs); the rest goes through
the worklist to the block path, which steps a window of 1,024 merged positions.  No test
provokes a fault: the error cases are the clamped, reported ones of the contract.
"""

import ctypes
import random

import numpy as np
import pytest

import crdtgpu
from counter_maps import assert_mixes, map_batch, map_out, mixed
from crdtgpu import CRDT_E_ACTOR_RANGE, CRDT_E_CAPACITY, CRDT_E_INVALID, CRDT_E_WORKSPACE, abi
from crdtgpu.batch import AWSetBatch, DiffBuffers, MergeLogBuffers, OutBuffers, QueryBatch, QueryBuffers
from join_log_cases import (LOG_DOCS, LOG_WAVES, MAX_C, WAVE_MAX, WINDOW, assert_log, assert_state, doc_lists,
                            join_log_ref, on_wave_path, pack, pair_doc, random_pair, seq_batch, straddle_pair)
from test_diff_model import ADDED, CLOCK, REMOVED, UPDATED
from test_gpu_compare import _code, dev_of, host_out, poisoned_out

pytestmark = pytest.mark.gpu

U8, U32, U64 = np.uint8, np.uint32, np.uint64
POISON8 = 77


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

def slots_of(x):
    return int(np.asarray(x.offsets)[-1])


def poison(log):
    for f in log.FIELDS:
        t = getattr(log, f)
        if t is not None:
            t.fill_(POISON8 if f in ("flags", "ups_kind") else -1)
    return log


def poisoned_log(torch, n, rem_slots, ups_slots, **kw):
    return poison(MergeLogBuffers(n, rem_slots, ups_slots, device=dev_of(torch), **kw))


def join_on_device(eng, torch, dst, src, dd=None, ds=None, stream=None, **kw):
    """(out, log) on the device after one join_log_async; not synced."""
    n, R = dst.n_docs, dst.R
    dev = dev_of(torch)
    out = poisoned_out(torch, n, R, slots_of(dst) + slots_of(src))
    log = poisoned_log(torch, n, slots_of(dst), slots_of(src), **kw)
    eng.join_log_async(dd or dst.to(dev), ds or src.to(dev), out, log, stream=stream)
    return out, log


def exchange_on_device(eng, torch, a, b, da=None, db=None, stream=None):
    """(out_ab, out_ba, log_ab, log_ba) on the device after one exchange_log_async; not synced."""
    n, R = a.n_docs, a.R
    dev = dev_of(torch)
    sa, sb = slots_of(a), slots_of(b)
    o1, o2 = poisoned_out(torch, n, R, sa + sb), poisoned_out(torch, n, R, sa + sb)
    l1, l2 = poisoned_log(torch, n, sa, sb), poisoned_log(torch, n, sb, sa)
    eng.exchange_log_async(da or a.to(dev), db or b.to(dev), o1, o2, l1, l2, stream=stream)
    return o1, o2, l1, l2


def assert_join(got, dst, src, want=None, what="dst <- src"):
    want = want or join_log_ref(dst, src)
    assert want.rc == 0
    out, log = got
    h = host_out(out)
    assert_state(h, want.out, dst.n_docs, dst.R, what)
    g = log.numpy()
    assert_log(g, want, what)
    return h, g, want


def check_join(eng, torch, dst, src, want=None):
    got = join_on_device(eng, torch, dst, src)
    eng.sync()
    return assert_join(got, dst, src, want)


def check_exchange(eng, torch, a, b, want_ab=None, want_ba=None):
    o1, o2, l1, l2 = exchange_on_device(eng, torch, a, b)
    eng.sync()
    r1 = assert_join((o1, l1), a, b, want_ab, "a <- b")
    r2 = assert_join((o2, l2), b, a, want_ba, "b <- a")
    return r1, r2


def same_records(g1, g2, want):
    """Two downloaded logs hold the same bits at every word the contract specifies."""
    for f in ("flags", "summary", "rem_offsets", "rem_counts", "ups_offsets", "ups_counts"):
        assert (g1[f] == g2[f]).all(), f
    for f in ("rem_keys", "rem_actors", "rem_counters"):
        assert (g1[f][want.rem_idx] == g2[f][want.rem_idx]).all(), f
    for f in ("ups_keys", "ups_actors", "ups_counters", "ups_kind"):
        assert (g1[f][want.ups_idx] == g2[f][want.ups_idx]).all(), f


# ------------------------------------------------------- 1. parity and shapes

LAYOUTS = {1: (dict(), dict(slack=2, stale=1)), 2: (dict(slack=3, stale=2), dict()),
           5: (dict(slack=1), dict(slack=2, stale=3)), 64: (dict(with_counts=True), dict())}


def _lay(lay):
    lay = dict(lay)
    if "stale" in lay:
        lay["stale"] = np.random.default_rng(lay["stale"])
    return lay


@pytest.fixture(scope="module")
def parity2():
    a, b = random_pair(9000 + 2, 3000, 2, lay_d=_lay(LAYOUTS[2][0]), lay_s=_lay(LAYOUTS[2][1]))
    return a, b, join_log_ref(a, b), join_log_ref(b, a)


@pytest.mark.parametrize("R", [1, 2, 5, 64])
def test_random_parity(eng, torch, R):
    """The 3,000 documents tests/test_join_log_model.py takes the census of, with stale and
    zero slack and counts NULL on either side; exchange_log equals the two join_logs."""
    a, b = random_pair(9000 + R, 3000, R, lay_d=_lay(LAYOUTS[R][0]), lay_s=_lay(LAYOUTS[R][1]))
    assert (a.counts is None) != (b.counts is None) or R == 5
    (h1, g1, w1), (h2, g2, w2) = check_exchange(eng, torch, a, b)
    for dst, src, h, g, w in ((a, b, h1, g1, w1), (b, a, h2, g2, w2)):
        hj, gj, _ = check_join(eng, torch, dst, src, w)
        assert_state(hj, h, a.n_docs, R, "join_log against exchange_log")
        same_records(gj, g, w)


@pytest.mark.parametrize("n_docs", [1, 3, 4, 5, LOG_WAVES * LOG_DOCS - 1, LOG_WAVES * LOG_DOCS, LOG_WAVES * LOG_DOCS + 1])
def test_grid_edges(eng, torch, n_docs):
    a, b = random_pair(9100 + n_docs, n_docs, 3, big_every=3, lay_d=dict(slack=1))
    check_exchange(eng, torch, a, b)


def test_handoff_sizes(eng, torch):
    """63 / 64 / 65 live entries on either side, each in the three modes of pair_doc."""
    rng = random.Random(9200)
    dd, sd = [], []
    for nd in (WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1):
        for ns in (WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1):
            for mode in range(3):
                x, y = pair_doc(rng, 2, nd, ns, mode)
                dd.append(x)
                sd.append(y)
    a, b = pack(2, dd, slack=2, stale=np.random.default_rng(5)), pack(2, sd)
    paths = [on_wave_path(a, b, d) for d in range(a.n_docs)]
    assert any(paths) and not all(paths)
    check_exchange(eng, torch, a, b)


def test_large_documents(eng, torch):
    """About 300 documents of 65..3,000 entries a side: the worklist, several windows."""
    rng = random.Random(9300)
    dd, sd = [], []
    for d in range(300):
        hi = 3000 if d % 10 == 0 else 400
        x, y = pair_doc(rng, 3, rng.randint(65, hi), rng.randint(65, hi), (0, 0, 1, 2)[d % 4])
        dd.append(x)
        sd.append(y)
    a, b = pack(3, dd, slack=1, stale=np.random.default_rng(6)), pack(3, sd)
    assert max(int(x) for x in a.counts) > 2 * WINDOW
    (_, _, w1), _ = check_exchange(eng, torch, a, b)
    assert int(w1.log["summary"][0]) > 1000 and int(w1.log["summary"][2]) > 1000


# ------------------------------------------- 2. block-path window boundaries

def _uniform_doc(rng, keys, R=2):
    n = len(keys)
    return (np.asarray(keys, U64), rng.integers(0, R, n).astype(U32), rng.integers(1, MAX_C, n).astype(U64),
            rng.integers(0, MAX_C + 1, R).astype(U64))


def test_window_boundaries(eng, torch):
    """A common pair straddling merged positions 1,023 / 1,024 / 1,025 and 2,047 / 2,048 /
    2,049; identical key sets; disjoint key ranges, either side below the other."""
    rng = np.random.default_rng(9400)
    ds, ss = [], []
    for pos in (WINDOW - 1, WINDOW, WINDOW + 1, 2 * WINDOW - 1, 2 * WINDOW, 2 * WINDOW + 1):
        x, y = straddle_pair(pos)
        ds.append(x)
        ss.append(y)
    same = np.arange(1, 2501, dtype=U64) * U64(7)
    ds.append(_uniform_doc(rng, same))
    ss.append(_uniform_doc(rng, same))
    lo, hi = np.arange(1, 1301, dtype=U64), np.arange(5000, 6500, dtype=U64)
    for x, y in ((lo, hi), (hi, lo)):
        ds.append(_uniform_doc(rng, x))
        ss.append(_uniform_doc(rng, y))
    a, b = seq_batch(2, ds), seq_batch(2, ss)
    (_, _, w1), (_, _, w2) = check_exchange(eng, torch, a, b)
    for d in range(6):  # exactly one UPDATED record per straddling pair, in either direction
        for w in (w1, w2):
            assert sum(x[3] == UPDATED for x in doc_lists(w.log, d)[1]) == 1
    assert int(w1.log["flags"][6]) & (REMOVED | ADDED) == 0 and int(w1.log["flags"][6]) & UPDATED


def test_one_document_of_2_17_plus_1_entries_a_side(eng, torch):
    rng = np.random.default_rng(9500)
    n = 2 ** 17 + 1
    universe = np.arange(1, 3 * n // 2 + 3, dtype=U64) * U64(3)
    ka, kb = np.sort(rng.choice(universe, n, replace=False)), np.sort(rng.choice(universe, n, replace=False))
    a, b = seq_batch(2, [_uniform_doc(rng, ka)]), seq_batch(2, [_uniform_doc(rng, kb)])
    (_, _, w1), _ = check_exchange(eng, torch, a, b)
    assert int(w1.log["flags"][0]) & 7 == REMOVED | ADDED | UPDATED


# ------------------------------------------------ 3. one change per document

def one_change_docs(R=2):
    """Per size (wave: 1, 7, 64; block: 65, 1,100): a single removed, added or updated
    key placed first, last or only; everything removed; everything added; converged."""
    dd, sd, want = [], [], []
    for n in (1, 7, WAVE_MAX, WAVE_MAX + 1, 1100):
        keys = [10 * (i + 1) for i in range(n)]
        base = [(k, 0, 2) for k in keys]
        vv = [5] * R
        for where in ((0,) if n == 1 else (0, n - 1)):
            k = keys[where]
            # removed: dst has k, src does not and its clock covers the dot
            dd.append((base, vv))
            sd.append(([e for e in base if e[0] != k], vv))
            want.append(REMOVED)
            # added: src has a key dst lacks, under a dot dst's clock has not seen
            new = (k - 5 if where == 0 else k + 5, 1 % R, 9)
            dd.append((base, vv))
            sd.append((sorted(base + [new]), vv))
            want.append(ADDED)
            # updated: the common key under another dot
            dd.append((base, vv))
            sd.append(([(kk, a, 3) if kk == k else (kk, a, c) for kk, a, c in base], vv))
            want.append(UPDATED)
        dd.append((base, vv))  # everything removed: src empty, its clock covers dst
        sd.append(([], [6] * R))
        want.append(REMOVED | CLOCK)
        dd.append(([], [0] * R))  # everything added
        sd.append((base, vv))
        want.append(ADDED | CLOCK)
        dd.append((base, vv))  # converged
        sd.append((list(base), list(vv)))
        want.append(0)
    return pack(R, dd, slack=1), pack(R, sd), np.array(want, U8)


def test_one_change_per_document(eng, torch):
    a, b, flags = one_change_docs()
    (h, g, w), _ = check_exchange(eng, torch, a, b)
    assert (g["flags"] == flags).all()
    single = np.isin(flags, [REMOVED, ADDED, UPDATED])
    assert ((g["rem_counts"] + g["ups_counts"])[single] == 1).all()
    conv = flags == 0
    assert (g["rem_counts"][conv] == 0).all() and (g["ups_counts"][conv] == 0).all()
    gone = flags == (REMOVED | CLOCK)
    assert (h.counts[: a.n_docs][gone] == 0).all() and (g["rem_counts"][gone] == np.asarray(a.counts)[gone]).all()


def test_a_converged_batch(eng, torch):
    """flags 0, counts 0, summary zeros, in both directions."""
    rng = random.Random(9600)
    docs = [pair_doc(rng, 3, rng.choice([0, 5, 64, 70, 1500]), 0, 1)[0] for _ in range(200)]
    a, b = pack(3, docs, slack=2, stale=np.random.default_rng(7)), pack(3, docs)
    (_, g1, _), (_, g2, _) = check_exchange(eng, torch, a, b)
    for g in (g1, g2):
        assert not g["flags"].any() and not g["summary"].any() and not g["rem_counts"].any() and not g["ups_counts"].any()


# ------------------------------------------------------------------- 4. dots

def test_dots_differing_in_one_field(eng, torch):
    """Common keys whose dots differ only in the actor, or only in the counter by one step,
    with every counter through the maps of tests/counter_maps.py: the step is then a
    difference in the high half alone (hi_only), across 2^32, 2^31, 2^63, and at 2^64 - 1."""
    rng = random.Random(9700)
    R = 3
    dd, sd = [], []
    for d in range(240):
        n = (5, 64, 90)[d % 3]
        keys = [3 * i + 1 for i in range(n)]
        ed = [(k, rng.randrange(R), rng.randint(1, MAX_C - 1)) for k in keys]
        es = []
        for k, a, c in ed:
            how = rng.randrange(3)
            es.append((k, a, c) if how == 0 else (k, (a + 1) % R, c) if how == 1 else (k, a, c + 1))
        dd.append((ed, [rng.randint(0, MAX_C) for _ in range(R)]))
        sd.append((es, [rng.randint(0, MAX_C) for _ in range(R)]))
    a, b = pack(R, dd), pack(R, sd, slack=1)
    tab = mixed(MAX_C, 3)
    am, bm = map_batch(a, tab), map_batch(b, tab)
    (h1, g1, w1), _ = check_exchange(eng, torch, am, bm)
    assert_mixes(w1.out, tab, "a <- b")
    plain = join_log_ref(a, b)
    assert (g1["flags"] == plain.log["flags"]).all() and (g1["ups_counts"] == plain.log["ups_counts"]).all()
    assert int(plain.log["summary"][2]) > 3000 and int(plain.log["summary"][0]) == 0
    assert_state(h1, map_out(plain.out, tab), a.n_docs, R, "mapped result of the unmapped run")


# ------------------------------------------ 5. consistency with existing calls

def test_merged_states_equal_the_plain_exchange(eng, torch, parity2):
    a, b, w1, w2 = parity2
    dev = dev_of(torch)
    da, db = a.to(dev), b.to(dev)
    o1, o2, _, _ = exchange_on_device(eng, torch, a, b, da, db)
    slots = slots_of(a) + slots_of(b)
    p1, p2 = poisoned_out(torch, a.n_docs, 2, slots), poisoned_out(torch, a.n_docs, 2, slots)
    eng.exchange_async(da, db, p1, p2)
    eng.sync()
    assert_state(host_out(o1), host_out(p1), a.n_docs, 2, "a <- b")
    assert_state(host_out(o2), host_out(p2), a.n_docs, 2, "b <- a")


def test_log_equals_the_device_diff_of_dst_and_out(eng, torch, parity2):
    """flags, per-document counts and summary equal crdt_awset_diff_async(dst, out)'s, and
    its packed lists equal the log's lists read document by document."""
    a, b, w1, w2 = parity2
    dev = dev_of(torch)
    da, db = a.to(dev), b.to(dev)
    o1, o2, l1, l2 = exchange_on_device(eng, torch, a, b, da, db)
    for dst, out, log, want in ((da, o1, l1, w1), (db, o2, l2, w2)):
        diff = DiffBuffers(a.n_docs, log.rem_slots, log.ups_slots, device=dev)
        eng.diff_async(dst, out.as_batch(), diff)
        eng.sync()
        g, df = log.numpy(), diff.numpy()
        assert (g["flags"] == df["flags"]).all() and (g["summary"] == df["summary"]).all()
        assert (g["rem_counts"] == np.diff(df["rem_off"])).all() and (g["ups_counts"] == np.diff(df["ups_off"])).all()
        for f, idx in (("rem_keys", want.rem_idx), ("rem_actors", want.rem_idx), ("rem_counters", want.rem_idx),
                       ("ups_keys", want.ups_idx), ("ups_actors", want.ups_idx), ("ups_counters", want.ups_idx),
                       ("ups_kind", want.ups_idx)):
            assert (g[f][idx] == df[f]).all(), f


# -------------------------------------------------------------- 6. composition

def test_exchange_output_is_an_input_as_it_stands(eng, torch, parity2):
    """Documents at capacity offsets with slack behind the live prefixes: the outputs of
    one logged exchange, on the device, are the inputs of the next."""
    a, b, w1, w2 = parity2
    o1, o2, _, _ = exchange_on_device(eng, torch, a, b)
    n, R = a.n_docs, 2
    s = o1.slots
    p1, p2 = poisoned_out(torch, n, R, 2 * s), poisoned_out(torch, n, R, 2 * s)
    l1, l2 = poisoned_log(torch, n, s, s), poisoned_log(torch, n, s, s)
    eng.exchange_log_async(o1.as_batch(), o2.as_batch(), p1, p2, l1, l2)
    eng.sync()
    a2, b2 = w1.out.as_batch(), w2.out.as_batch()
    assert slots_of(a2) > int(np.asarray(a2.counts).sum())
    assert_join((p1, l1), a2, b2, what="a2 <- b2")
    _, g, _ = assert_join((p2, l2), b2, a2, what="b2 <- a2")
    assert not (g["flags"] & (REMOVED | ADDED)).any()  # after one exchange the element sets agree


def test_a_log_list_is_a_tomb_batch(eng, torch, parity2):
    """The removed list, wrapped as a TombBatch as it stands, answers crdt_tomb_has_async:
    every removed key is found with its dot, a key the merge kept is not."""
    a, b, w1, _ = parity2
    out, log = join_on_device(eng, torch, a, b)
    per_doc, want = [], []
    merged = w1.out.as_batch()
    for d in range(a.n_docs):
        rem, _ = doc_lists(w1.log, d)
        kept = [e[0] for e in merged.doc(d)[0][:2]]
        per_doc.append([r[0] for r in rem] + kept)
        want += [(1, r[1], r[2]) for r in rem] + [(0, 0, 0)] * len(kept)
    q = QueryBatch.from_lists(per_doc)
    res = QueryBuffers(q.n_queries, device=dev_of(torch))
    eng.tomb_has_async(log.removed(), q.to(dev_of(torch)), res)
    eng.sync()
    found, actors, counters = res.numpy()
    assert found.tolist() == [w[0] for w in want] and sum(found.tolist()) > 100
    hit = found.astype(bool)
    assert actors[hit].tolist() == [w[1] for w in want if w[0]] and counters[hit].tolist() == [w[2] for w in want if w[0]]


# ------------------------------------------------------ 7. errors and ordering

def small_pair(R=2, n=6, size=5):
    rng = random.Random(9800 + size)
    docs = [pair_doc(rng, R, size, size, 0) for _ in range(n)]
    return [p[0] for p in docs], [p[1] for p in docs]


@pytest.mark.parametrize("size", [5, 80])
def test_actor_range(eng, torch, size):
    """A dst-only entry whose dot has actor == R (HasDot against src's clock), at wave and at
    block size; the oracle reports the same.  actor > R in the same place is "never seen"."""
    dd, sd = small_pair(size=size)
    e, v = dd[2]
    top = max(k for k, _, _ in e + sd[2][0]) + 1
    dd[2] = (e + [(top, 2, 1)], v)
    a, b = pack(2, dd), pack(2, sd)
    assert on_wave_path(a, b, 2) == (size <= WAVE_MAX)
    assert join_log_ref(a, b).rc == CRDT_E_ACTOR_RANGE
    join_on_device(eng, torch, a, b)
    assert _code(eng.sync) == CRDT_E_ACTOR_RANGE
    eng.sync()  # cleared
    dd[2] = (e + [(top, 3, 1)], v)
    a = pack(2, dd)
    check_exchange(eng, torch, a, b)


def test_count_above_slots_is_clamped(eng, torch):
    dd, sd = small_pair()
    a, b = pack(2, dd, slack=1), pack(2, sd, slack=1)
    b.counts[1] = int(b.offsets[2]) - int(b.offsets[1]) + 9
    out, log = join_on_device(eng, torch, a, b)
    assert _code(eng.sync) == CRDT_E_CAPACITY
    eng.sync()  # cleared
    # the other documents are what they would be without the bad count
    b.counts[1] = int(b.offsets[2]) - int(b.offsets[1]) - 1
    want = join_log_ref(a, b)
    h, g = host_out(out), log.numpy()
    hw = want.out.as_batch()
    for d in (0, 2, 3, 4, 5):
        o, m = int(h.offsets[d]), int(h.counts[d])
        got = list(zip(h.keys[o:o + m].tolist(), h.actors[o:o + m].tolist(), h.counters[o:o + m].tolist()))
        assert got == hw.doc(d)[0], d
        assert doc_lists(g, d) == doc_lists(want.log, d) and int(g["flags"][d]) == int(want.log["flags"][d]), d


def test_count_above_slots_is_clamped_at_block_size(eng, torch):
    """The same with 80 entries a side and the exchange: the document is the block path's,
    which clamps the count again, as dst of one direction and as src of the other."""
    dd, sd = small_pair(size=80)
    a, b = pack(2, dd, slack=1), pack(2, sd, slack=1)
    assert not on_wave_path(a, b, 1)
    b.counts[1] = int(b.offsets[2]) - int(b.offsets[1]) + 9
    o1, o2, l1, l2 = exchange_on_device(eng, torch, a, b)
    assert _code(eng.sync) == CRDT_E_CAPACITY
    eng.sync()  # cleared
    b.counts[1] = int(b.offsets[2]) - int(b.offsets[1]) - 1
    for (out, log), want in zip(((o1, l1), (o2, l2)), (join_log_ref(a, b), join_log_ref(b, a))):
        h, g, hw = host_out(out), log.numpy(), want.out.as_batch()
        for d in (0, 2, 3, 4, 5):
            o, m = int(h.offsets[d]), int(h.counts[d])
            live = list(zip(h.keys[o:o + m].tolist(), h.actors[o:o + m].tolist(), h.counters[o:o + m].tolist()))
            assert live == hw.doc(d)[0], d
            assert doc_lists(g, d) == doc_lists(want.log, d) and int(g["flags"][d]) == int(want.log["flags"][d]), d


def test_argument_errors(eng, torch):
    """Every one of these is refused on the host: nothing is launched."""
    dd, sd = small_pair()
    dev = dev_of(torch)
    a, b = pack(2, dd).to(dev), pack(2, sd).to(dev)
    b5 = pack(2, sd[:5]).to(dev)
    d3, s3 = small_pair(3)
    bR = pack(3, s3).to(dev)
    n, R, slots = 6, 2, 64
    o1, o2 = poisoned_out(torch, n, R, slots), poisoned_out(torch, n, R, slots)
    l1, l2 = poisoned_log(torch, n, slots, slots), poisoned_log(torch, n, slots, slots)
    lib, ctx, ref = abi.lib(), eng._ctx, ctypes.byref

    def xchg(ca, cb, c1, c2, g1, g2):
        r = lambda x: ref(x) if x is not None else None  # noqa: E731
        return lib.crdt_awset_exchange_log_async(ctx, r(ca), r(cb), r(c1), r(c2), r(g1), r(g2), None)

    def join(cd, cs, co, g):
        r = lambda x: ref(x) if x is not None else None  # noqa: E731
        return lib.crdt_awset_join_log_async(ctx, r(cd), r(cs), r(co), r(g), None)

    ca, cb = a.c(), b.c()
    args = [ca, cb, o1.c(), o2.c(), l1.c(), l2.c()]
    for i in range(6):  # any NULL among the arguments
        bad = list(args)
        bad[i] = None
        assert xchg(*bad) == CRDT_E_INVALID, i
    for i, bad in enumerate(([None, cb, o1.c(), l1.c()], [ca, None, o1.c(), l1.c()], [ca, cb, None, l1.c()],
                             [ca, cb, o1.c(), None])):
        assert join(*bad) == CRDT_E_INVALID, i
    assert lib.crdt_awset_join_log_async(None, ref(ca), ref(cb), ref(args[2]), ref(args[4]), None) == CRDT_E_INVALID
    assert xchg(ca, b5.c(), *args[2:]) == CRDT_E_INVALID  # n_docs
    assert xchg(ca, bR.c(), *args[2:]) == CRDT_E_INVALID  # R
    assert join(ca, bR.c(), o1.c(), l1.c()) == CRDT_E_INVALID
    wide_a, wide_b = a.c(), b.c()
    wide_a.R = wide_b.R = 65
    assert xchg(wide_a, wide_b, *args[2:]) == CRDT_E_INVALID  # R out of range
    wide_a.R = wide_b.R = 0
    assert join(wide_a, wide_b, o1.c(), l1.c()) == CRDT_E_INVALID
    for f in ("offsets", "counts", "keys", "actors", "counters", "vv"):  # a required field NULL
        c = o1.c()
        setattr(c, f, None)
        assert xchg(ca, cb, c, o2.c(), l1.c(), l2.c()) == CRDT_E_INVALID, f
        assert xchg(ca, cb, o2.c(), c, l1.c(), l2.c()) == CRDT_E_INVALID, f
        assert join(ca, cb, c, l1.c()) == CRDT_E_INVALID, f
        # the two directions share no array: the shared key column is the plain exchange's
        c = o2.c()
        setattr(c, f, getattr(o1.c(), f))
        assert xchg(ca, cb, o1.c(), c, l1.c(), l2.c()) == CRDT_E_INVALID, f
    for f in MergeLogBuffers.FIELDS:
        g = l1.c()
        setattr(g, f, None)
        rc = CRDT_E_INVALID if f not in ("summary", "ups_kind") else 0
        assert join(ca, cb, o1.c(), g) == rc, f
        if rc:
            assert xchg(ca, cb, o1.c(), o2.c(), g, l2.c()) == rc and xchg(ca, cb, o1.c(), o2.c(), l2.c(), g) == rc, f
        # two written arrays starting at one address: across the logs, and log against state
        g = l2.c()
        setattr(g, f, getattr(l1.c(), f))
        assert xchg(ca, cb, o1.c(), o2.c(), l1.c(), g) == CRDT_E_INVALID, f
    eng.sync()  # (the two calls without summary / ups_kind ran)
    poison(l1)
    for t in (o1.offsets, o1.counts, o1.keys, o1.actors, o1.counters, o1.vv):
        t.fill_(-1)
    for f, g_ in (("rem_keys", "ups_keys"), ("rem_counts", "ups_counts"), ("rem_keys", "rem_counters"),
                  ("flags", "ups_kind"), ("rem_offsets", "ups_offsets")):
        g = l1.c()
        setattr(g, f, getattr(l1.c(), g_))
        assert join(ca, cb, o1.c(), g) == CRDT_E_INVALID, (f, g_)
    for f, of in (("rem_keys", "keys"), ("ups_counters", "counters"), ("rem_actors", "actors"), ("rem_counts", "counts"),
                  ("ups_offsets", "offsets"), ("ups_keys", "vv")):
        g = l1.c()
        setattr(g, f, getattr(o1.c(), of))
        assert join(ca, cb, o1.c(), g) == CRDT_E_INVALID, (f, of)
    # a written array starting where an input array of the same kind starts
    for f, src in (("keys", a.keys), ("counters", b.keys), ("vv", b.vv), ("actors", a.actors), ("offsets", b.offsets),
                   ("counts", a.offsets), ("keys", b.counters)):
        c = o1.c()
        setattr(c, f, src.data_ptr())
        assert join(ca, cb, c, l1.c()) == CRDT_E_INVALID, f
        assert xchg(ca, cb, o2.c(), c, l1.c(), l2.c()) == CRDT_E_INVALID, f
    for f, src in (("rem_keys", a.keys), ("ups_keys", b.keys), ("rem_counters", a.vv), ("ups_actors", b.actors),
                   ("rem_offsets", a.offsets), ("ups_offsets", b.offsets), ("rem_counts", a.actors),
                   ("summary", b.offsets), ("ups_counters", a.counters)):
        g = l1.c()
        setattr(g, f, src.data_ptr())
        assert join(ca, cb, o1.c(), g) == CRDT_E_INVALID, f
        assert xchg(ca, cb, o1.c(), o2.c(), l2.c(), g) == CRDT_E_INVALID, f
    eng.sync()
    for o in (o1, o2):
        for t in (o.offsets, o.counts, o.actors):
            assert (t.cpu().numpy().view(U32) == 2 ** 32 - 1).all()
        for t in (o.keys, o.counters, o.vv):
            assert (t.cpu().numpy().view(U64) == 2 ** 64 - 1).all()
    assert (l1.flags.cpu().numpy() == POISON8).all() and (l1.rem_counts.cpu().numpy().view(U32) == 2 ** 32 - 1).all()


def test_optional_columns(eng, torch):
    """summary and ups_kind are optional, and the call writes the rest as ever."""
    dd, sd = small_pair(n=40, size=30)
    a, b = pack(2, dd), pack(2, sd)
    want = join_log_ref(a, b)
    got = join_on_device(eng, torch, a, b, kind=False, summary=False)
    eng.sync()
    assert_join(got, a, b, want)


def test_no_documents(eng, torch):
    dev = dev_of(torch)
    z = lambda dt: torch.zeros(1, dtype=dt, device=dev)  # noqa: E731
    e = AWSetBatch(2, z(torch.int32), z(torch.int64), z(torch.int32), z(torch.int64), z(torch.int64))
    assert e.n_docs == 0
    o1, o2 = poisoned_out(torch, 1, 2, 4), poisoned_out(torch, 1, 2, 4)
    l1, l2 = poisoned_log(torch, 0, 4, 4), poisoned_log(torch, 0, 4, 4)
    eng.exchange_log_async(e, e, o1, o2, l1, l2)
    eng.sync()
    for o, lg in ((o1, l1), (o2, l2)):
        assert (o.keys.cpu().numpy().view(U64) == 2 ** 64 - 1).all() and int(o.counts.cpu().numpy().view(U32)[0]) == 2 ** 32 - 1
        assert not lg.summary.cpu().numpy().any()  # zeroed
        assert int(lg.flags.cpu().numpy()[0]) == POISON8 and int(lg.rem_offsets.cpu().numpy().view(U32)[0]) == 2 ** 32 - 1
    poison(l1)
    eng.join_log_async(e, e, o1, l1)
    eng.sync()
    assert not l1.summary.cpu().numpy().any() and (l1.rem_keys.cpu().numpy().view(U64) == 2 ** 64 - 1).all()


def test_graph_capture(torch):
    """Captured on a reserved context, replayed with the inputs' clocks changed in between,
    equal to eager; on an unreserved context the capture is refused with CRDT_E_WORKSPACE
    and launches nothing."""
    a, b = random_pair(9900, 1500, 2, max_e=70, big_every=20)
    n, R = a.n_docs, 2
    assert n > 1024  # (a fresh context's workspace holds 1,024 documents)
    assert sum(not on_wave_path(a, b, d) for d in range(n)) > 20
    dev = dev_of(torch)
    sa, sb = slots_of(a), slots_of(b)
    e = crdtgpu.Engine(0)
    try:
        da, db = a.to(dev), b.to(dev)
        o1, o2 = poisoned_out(torch, n, R, sa + sb), poisoned_out(torch, n, R, sa + sb)
        l1, l2 = poisoned_log(torch, n, sa, sb), poisoned_log(torch, n, sb, sa)
        g0 = torch.cuda.CUDAGraph()
        with pytest.raises(crdtgpu.CrdtError) as ei:
            with torch.cuda.graph(g0):
                e.exchange_log_async(da, db, o1, o2, l1, l2, stream=torch.cuda.current_stream())
        assert ei.value.code == CRDT_E_WORKSPACE
        torch.cuda.synchronize()
        assert (l1.flags.cpu().numpy() == POISON8).all() and (o1.counts.cpu().numpy().view(U32) == 2 ** 32 - 1).all()
        assert (l1.summary.cpu().numpy().view(U32) == 2 ** 32 - 1).all()
        e.reserve(n)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.exchange_log_async(da, db, o1, o2, l1, l2, stream=torch.cuda.current_stream())
        b_swapped = AWSetBatch(R, b.offsets, b.keys, b.actors, b.counters, np.asarray(a.vv).copy(), counts=b.counts)
        for hb in (b_swapped, b):  # b's clocks change between replays: other removes, other adds
            db.vv.copy_(hb.to(dev).vv)
            for o in (o1, o2):
                for t in (o.offsets, o.counts, o.keys, o.actors, o.counters, o.vv):
                    t.fill_(-1)
            poison(l1)
            poison(l2)
            g.replay()
            e.sync(torch.cuda.current_stream())
            _, g1, w1 = assert_join((o1, l1), a, hb, what="a <- b")
            assert_join((o2, l2), hb, a, what="b <- a")
            eager = exchange_on_device(e, torch, a, hb)
            e.sync()
            assert_state(host_out(eager[0]), host_out(o1), n, R, "eager")
            same_records(eager[2].numpy(), g1, w1)
    finally:
        e.close()


def test_ordered_after_a_call_on_another_stream(eng, torch, parity2):
    """The logged exchange reads the outputs of a plain exchange issued on another stream."""
    a, b, w1, w2 = parity2
    dev = dev_of(torch)
    n, R = a.n_docs, 2
    s = slots_of(a) + slots_of(b)
    o1, o2 = OutBuffers(n, R, s, device=dev), OutBuffers(n, R, s, device=dev)
    for o in (o1, o2):
        for t in (o.offsets, o.counts, o.keys, o.actors, o.counters, o.vv):
            t.zero_()  # a logged exchange that ran first would see two empty batches
    da, db = a.to(dev), b.to(dev)
    p1, p2 = poisoned_out(torch, n, R, 2 * s), poisoned_out(torch, n, R, 2 * s)
    l1, l2 = poisoned_log(torch, n, s, s), poisoned_log(torch, n, s, s)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.exchange_async(da, db, o1, o2, stream=sa)
    eng.exchange_log_async(o1.as_batch(), o2.as_batch(), p1, p2, l1, l2, stream=sb)
    eng.sync(sb)
    assert_join((p1, l1), w1.out.as_batch(), w2.out.as_batch(), what="a2 <- b2")


def test_two_eager_runs_are_bit_identical(eng, torch, parity2):
    a, b, w1, _ = parity2
    runs = []
    for _ in range(2):
        out, log = join_on_device(eng, torch, a, b)
        eng.sync()
        runs.append((host_out(out), log.numpy()))
    assert_state(runs[0][0], runs[1][0], a.n_docs, 2)
    same_records(runs[0][1], runs[1][1], w1)
