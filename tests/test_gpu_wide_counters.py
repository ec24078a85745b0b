"""GPU: the merge path at full 64-bit dot counters and clocks.

Every other merge-path test draws counters below 51, so every high half the
kernels move between lanes (wave_sort.hpp readlane64 / lane_xor / from_next_lane,
fold.hip wave_or64 / lane_put / the clock replay, extract.hip shfl64, join.hip's
__shfl of a dot counter) is zero there.  Here the same small-counter cases, built
by the generators of those tests, go through the order-preserving maps of
tests/counter_maps.py -- one batch mixing all six, per document -- and each case
asserts both

  (a) kernel(f(inputs)) == oracle(f(inputs))
  (b) kernel(f(inputs)) == f(kernel(inputs))

bit for bit.  tests/test_counter_maps_model.py shows on the oracles that (b) is
a sound expectation.  The local ops (apply.hip) add to the clock and are checked
against oracle.apply only, with the acting actor's clock started just below
2^31, 2^32, 2^63 and 2^64 - 1.  Every case first asserts, on the oracle's
output, that it really mixes the maps and reaches each map's edge.
"""

import random
from types import SimpleNamespace

import numpy as np
import pytest

import counter_maps as cm
import crdtgpu
import test_delta_extract_model as model
from apply_cases import doc_of, encode, random_calls, random_doc
from counter_maps import MAPS, TOP
from crdtgpu import CRDT_FOLD_AWSET, CRDT_FOLD_DELTA, CRDT_OP_ADD, CRDT_OP_DELTA_DEL
from crdtgpu.batch import AWSetBatch, OpBatch, OutBuffers, TombBatch
from helpers import batch_of, out_doc, outs_equal, random_state, src_batch_of
from oracle import oracle
from test_gpu_delta_extract import assert_message, case as extract_case, expected, extract
from test_gpu_gc import gc_case, gc_on_gpu
from test_gpu_parity import (NOOP_FC_DST, NOOP_FC_SRCS, NOOP_FC_WANT, PANIC_R, fold_case, host_out, join_case,
                             lean_defer_case, panic_cases, wide_key_case)
from test_gpu_tiles import TILE, disjoint_key_docs, equal_key_docs, interleaved, shaped  # noqa: F401  (shaped: fixture)

pytestmark = pytest.mark.gpu

U64 = np.uint64


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


# ---------------------------------------------------------------- helpers

_cache = {}


def cached(key, build):
    """Inputs and oracle outputs of a case, made once and shared (never modified)."""
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def same(got, want, n, R, tod, what):
    bad = outs_equal(got, want, n, R)
    if bad is None:
        return
    if bad < 0:
        raise AssertionError("%s: slot bounds differ" % what)
    raise AssertionError("%s: doc %d (map %s) differs:\n got  %.600s\n want %.600s" % (
        what, bad, cm.map_name(tod(bad)), out_doc(got, bad, R), out_doc(want, bad, R)))


def wide_join(dst, src, tod, what):
    """A join case: the small inputs, the mapped ones, the oracle on the mapped ones in both directions."""
    wd, ws = cm.map_batch(dst, tod), cm.map_batch(src, tod)
    rc, want = oracle.join(wd, ws)
    assert rc == 0
    rc, want_ba = oracle.join(ws, wd)
    assert rc == 0
    cm.assert_mixes(want, tod, what)
    return SimpleNamespace(dst=dst, src=src, wd=wd, ws=ws, want=want, want_ba=want_ba, tod=tod, R=dst.R,
                           n=dst.n_docs, what=what)


def check_join(eng, c):
    got = eng.join(c.wd, c.ws)
    same(got, c.want, c.n, c.R, c.tod, c.what + " (a) vs oracle")
    same(got, cm.map_out(eng.join(c.dst, c.src), c.tod), c.n, c.R, c.tod, c.what + " (b) vs mapped small run")


def check_exchange(eng, c, run=None):
    run = run or (lambda a, b: eng.exchange(a, b))
    g1, g2 = run(c.wd, c.ws)
    same(g1, c.want, c.n, c.R, c.tod, c.what + " exchange a<-b (a)")
    same(g2, c.want_ba, c.n, c.R, c.tod, c.what + " exchange b<-a (a)")
    s1, s2 = run(c.dst, c.src)
    same(g1, cm.map_out(s1, c.tod), c.n, c.R, c.tod, c.what + " exchange a<-b (b)")
    same(g2, cm.map_out(s2, c.tod), c.n, c.R, c.tod, c.what + " exchange b<-a (b)")


def wide_fold(mode, dst, srcs, tod, what):
    wd, ws = cm.map_batch(dst, tod), cm.map_srcs(srcs, tod)
    rc, want = oracle.fold(mode, wd, ws)
    assert rc == 0
    cm.assert_mixes(want, tod, what)
    return SimpleNamespace(mode=mode, dst=dst, srcs=srcs, wd=wd, ws=ws, want=want, tod=tod, R=dst.R, n=dst.n_docs,
                           what=what)


def check_fold(eng, c):
    got = eng.fold(c.mode, c.wd, c.ws)
    same(got, c.want, c.n, c.R, c.tod, c.what + " (a) vs oracle")
    small = eng.fold(c.mode, c.dst, c.srcs)
    same(got, cm.map_out(small, c.tod), c.n, c.R, c.tod, c.what + " (b) vs mapped small run")


# ---------------------------------------------------------------- join: wave path

@pytest.mark.parametrize("R", [2, 64])
def test_join_wave_path(eng, R):
    def build():
        rng = random.Random(R * 1000 + 64)
        dst, src = join_case(rng, 3000, R, lambda: rng.randint(0, 64), 100 if R == 2 else 128, 9)
        return wide_join(dst, src, cm.mixed(9), "join wave R=%d" % R)
    check_join(eng, cached(("jw", R), build))


def test_join_wave_block_handoff_sizes(eng):
    """63 / 64 / 65 entries a side, every pair of sizes under every map."""
    def build():
        rng = random.Random(11)
        R = 2
        sizes = [(a, b) for a in (63, 64, 65) for b in (63, 64, 65)] * len(MAPS)
        dst = batch_of(R, [random_state(rng, R, a, 12000, 20) for a, _ in sizes])
        src = batch_of(R, [random_state(rng, R, b, 12000, 20) for _, b in sizes])
        return wide_join(dst, src, lambda d: cm.stretch(MAPS[d // 9], 20), "join 63/64/65")
    c = cached("jh", build)
    check_join(eng, c)
    check_exchange(eng, c)


# ---------------------------------------------------------------- join: block path

@pytest.mark.parametrize("tiles", [0, 1], ids=["block_kernel", "default"])
def test_join_block_path(eng, tiles):
    """Documents of 65 ... 2500 entries: through the per-document block kernel
    (join_tiles = 0), and as the engine routes them by default."""
    def build():
        rng = random.Random(12)
        R = 4
        dst, src = join_case(rng, 64, R, lambda: rng.choice([65, 300, 1023, 1024, 1025, 2500]), 20000, 30)
        return wide_join(dst, src, cm.mixed(30), "join block")
    c = cached("jb", build)
    try:
        eng.set_option("join_tiles", tiles)
        check_join(eng, c)
        check_exchange(eng, c)
    finally:
        eng.set_option("join_tiles", 1)


# ---------------------------------------------------------------- join and exchange: tile path

@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 3 * TILE + 7])
def test_tile_boundaries(shaped, n):
    def build():
        rng = random.Random(n)
        R = 3
        docs = [interleaved(rng, n, R, rng.choice([0.3, 0.9, 1.0])) for _ in range(6)]
        return wide_join(batch_of(R, [d for d, _ in docs]), batch_of(R, [s for _, s in docs]), cm.mixed(40),
                         "tile n=%d" % n)
    c = cached(("tb", n), build)
    check_join(shaped, c)
    check_exchange(shaped, c)


@pytest.mark.parametrize("keys", ["equal", "disjoint"])
def test_tile_equal_and_disjoint_keys(shaped, keys):
    """The documents of test_tile_equal_key_sets / test_tile_disjoint_key_ranges, cycled to six so that each map has one."""
    def build():
        R, dd, ds = equal_key_docs() if keys == "equal" else disjoint_key_docs()
        six = lambda docs: [docs[d % len(docs)] for d in range(len(MAPS))]  # noqa: E731
        return wide_join(batch_of(R, six(dd)), batch_of(R, six(ds)), cm.mixed(9), "tile %s keys" % keys)
    c = cached(("tk", keys), build)
    check_join(shaped, c)
    check_exchange(shaped, c)


# ---------------------------------------------------------------- exchange

@pytest.mark.parametrize("sizes", ["small", "mixed"])
def test_exchange_equals_two_joins(eng, sizes):
    def build():
        rng = random.Random(40 if sizes == "small" else 41)
        R = 3
        pick = (lambda: rng.randint(0, 64)) if sizes == "small" else (lambda: rng.choice([0, 5, 64, 65, 300, 2000]))
        a, b = join_case(rng, 1500 if sizes == "small" else 300, R, pick, 5000, 9)
        return wide_join(a, b, cm.mixed(9), "exchange " + sizes)
    check_exchange(eng, cached(("x", sizes), build))


@pytest.mark.parametrize("stage,shared", [(1, 0), (1, 1), (0, 0), (0, 1)])
@pytest.mark.parametrize("sizes", ["wave64", "mixed"])
def test_exchange_staging_and_shared_key_column(eng, torch, sizes, stage, shared):
    """Device buffers: LDS-staged and lane-scattered stores, each with two key
    columns and with one shared; wave64: 3,000 documents of at most 64 entries
    under the max_doc_entries promise (the kernel config 2 runs); mixed: wave,
    tile and block paths in one batch."""
    def build():
        if sizes == "wave64":
            rng = random.Random(2064)
            a, b = join_case(rng, 3000, 2, lambda: rng.randint(0, 64), 100, 9)
        else:
            rng = random.Random(43)
            a, b = join_case(rng, 300, 3, lambda: rng.choice([0, 5, 63, 64, 65, 300, 2000]), 5000, 9)
        return wide_join(a, b, cm.mixed(9), "exchange device " + sizes)
    c = cached(("xd", sizes), build)
    dev = torch.device("cuda:0")

    def run(a, b):
        slots = int(a.offsets[-1]) + int(b.offsets[-1])
        o1 = OutBuffers(c.n, c.R, slots, device=dev)
        o2 = OutBuffers(c.n, c.R, slots, device=dev, shared_keys=o1 if shared else None)
        eng.exchange_async(a.to(dev), b.to(dev), o1, o2)
        eng.sync()
        return host_out(o1, torch), host_out(o2, torch)

    try:
        eng.set_option("join_stage_stores", stage)
        if sizes == "wave64":
            eng.set_max_doc_entries(64)
        check_exchange(eng, c, run)
    finally:
        eng.set_option("join_stage_stores", 1)
        eng.set_max_doc_entries()


# ---------------------------------------------------------------- fold, both modes

MODES = [CRDT_FOLD_AWSET, CRDT_FOLD_DELTA]


@pytest.mark.parametrize("mode", MODES)
def test_fold_wave_path(eng, mode):
    def build():
        rng = random.Random(20 + mode)
        dst, srcs = fold_case(rng, 3000, 4, lambda: rng.randint(0, 64), lambda: rng.randint(0, 10),
                              lambda: rng.randint(0, 8), lambda: rng.randint(0, 3), 120, 8, mode == CRDT_FOLD_DELTA)
        return wide_fold(mode, dst, srcs, cm.mixed(8), "fold wave mode %d" % mode)
    check_fold(eng, cached(("fw", mode), build))


@pytest.mark.parametrize("universe,max_src", [(40, 15), (64, 16), (65, 8)])
@pytest.mark.parametrize("mode", MODES)
def test_fold_dense_key_spans(eng, mode, universe, max_src):
    """The per-slot walk (span < 64, <= 15 sources), the counting sort (span < 256) and the fall-back."""
    def build():
        rng = random.Random(universe * 100 + max_src + mode)
        dst, srcs = fold_case(rng, 3000, 4, lambda: rng.randint(0, min(universe, 60)),
                              lambda: rng.randint(0, max_src), lambda: rng.randint(0, min(universe, 12)),
                              lambda: rng.randint(0, 3), universe, 9, mode == CRDT_FOLD_DELTA)
        return wide_fold(mode, dst, srcs, cm.mixed(9), "fold dense (%d, %d) mode %d" % (universe, max_src, mode))
    check_fold(eng, cached(("fd", mode, universe, max_src), build))


@pytest.mark.parametrize("mode", MODES)
def test_fold_wide_keys_and_wide_counters(eng, mode):
    """All three sort tiers (32-, 64- and 80-bit tuples): wide keys and wide counters in one tuple."""
    def build():
        R, dsts, per_doc = wide_key_case(mode)
        return wide_fold(mode, batch_of(R, dsts), src_batch_of(R, per_doc), cm.mixed(8, period=12),
                         "fold wide keys mode %d" % mode)
    check_fold(eng, cached(("fk", mode), build))


@pytest.mark.parametrize("mode", MODES)
def test_fold_block_path_and_overflow(eng, mode):
    def build():
        rng = random.Random(30 + mode)
        dst, srcs = fold_case(rng, 200, 3, lambda: rng.choice([10, 100, 127, 128, 129, 600]),
                              lambda: rng.randint(0, 6), lambda: rng.choice([5, 40, 64, 65, 300]),
                              lambda: rng.choice([0, 2, 64, 65, 200]), 5000, 50, mode == CRDT_FOLD_DELTA)
        return wide_fold(mode, dst, srcs, cm.mixed(50), "fold block mode %d" % mode)
    check_fold(eng, cached(("fb", mode), build))


# ---------------------------------------------------------------- no-op steps and first contact

def noop_and_first_contact_docs(rng, R, n, max_c, universe):
    """3 n documents, counters up to max_c - 1 except where said:
    kind 0  every step a no-op: the dst clock [max_c - 1] * R covers every source
            entry, no tombstones, the source clocks [max_c] * R (a merge would raise
            the dst clock; the no-op must not) -- 1 to 13 steps;
    kind 1  the same with one step in the middle that carries tombstones (effective);
    kind 2  first contact: the dst clock max_c everywhere but 0 at the first source's actor."""
    dsts, per_doc = [], []
    for i in range(3 * n):
        kind = i % 3
        e, _ = random_state(rng, R, rng.randint(0, 40), universe, max_c - 1)
        chain = []
        for _ in range(rng.randint(1, 13)):
            se, svv = random_state(rng, R, rng.randint(0, 8), universe, max_c - 1)
            if kind == 2:
                chain.append((rng.randrange(R), svv, se, random_state(rng, R, rng.randint(0, 3), universe, max_c)[0]))
            else:
                chain.append((rng.randrange(R), [max_c] * R, se, []))
        if kind == 1:
            a, vv, se, _ = chain[len(chain) // 2]
            chain[len(chain) // 2] = (a, vv, se, random_state(rng, R, rng.randint(1, 3), universe, max_c)[0])
        vv = [max_c - 1] * R
        if kind == 2:
            vv = [max_c] * R
            vv[chain[0][0]] = 0
        dsts.append((e, vv))
        per_doc.append(chain)
    return dsts, per_doc


@pytest.mark.parametrize("lean", [1, 0])
def test_delta_fold_lean_pass_defers(eng, lean):
    """The six kinds of test_delta_fold_lean_pass_defers (each kind under each
    map), followed by documents whose steps are no-ops -- the clock broadcast
    of the no-op replay is the densest 64-bit lane traffic of the fold -- and
    first contacts, with the lean pass first and with the general kernel alone."""
    def build():
        R, dsts, per_doc = lean_defer_case(1800)
        nd, npd = noop_and_first_contact_docs(random.Random(78), R, 60, 9, 150)
        dst, srcs = batch_of(R, dsts + nd), src_batch_of(R, per_doc + npd)
        c = wide_fold(CRDT_FOLD_DELTA, dst, srcs, cm.mixed(9, period=6), "delta fold lean")
        for d in range(1800, 1980, 3):  # the pure no-op documents come out as they went in
            assert out_doc(c.want, d, R) == c.wd.doc(d), d
        return c
    c = cached("fl", build)
    try:
        eng.set_option("fold_lean_first", lean)
        check_fold(eng, c)
    finally:
        eng.set_option("fold_lean_first", 1)


@pytest.mark.parametrize("mode", MODES)
def test_fold_noop_and_first_contact_docs(eng, mode):
    """R = 4 (the general wave kernel's usual shape): no-op steps and first contacts only."""
    def build():
        dsts, per_doc = noop_and_first_contact_docs(random.Random(79 + mode), 4, 200, 8, 120)
        if mode == CRDT_FOLD_AWSET:
            per_doc = [[(a, vv, e, []) for a, vv, e, _ in ch] for ch in per_doc]
        c = wide_fold(mode, batch_of(4, dsts), src_batch_of(4, per_doc), cm.mixed(8, period=6),
                      "fold no-op / first contact mode %d" % mode)
        if mode == CRDT_FOLD_DELTA:
            for d in range(0, 600, 3):
                assert out_doc(c.want, d, 4) == c.wd.doc(d), d
        return c
    check_fold(eng, cached(("fn", mode), build))


def test_delta_fold_noop_and_first_contact_literals(eng):
    """The three documents of test_delta_fold_noop_and_first_contact under each map, the expected literals mapped."""
    R = 2
    tod = lambda d: cm.stretch(MAPS[d // 3], 9)  # noqa: E731
    n = 3 * len(MAPS)
    dst = batch_of(R, NOOP_FC_DST * len(MAPS))
    srcs = src_batch_of(R, NOOP_FC_SRCS * len(MAPS))
    c = wide_fold(CRDT_FOLD_DELTA, dst, srcs, tod, "no-op / first contact literals")
    check_fold(eng, c)
    got = eng.fold(CRDT_FOLD_DELTA, c.wd, c.ws)
    for d in range(n):
        e, vv = NOOP_FC_WANT[d % 3]
        assert out_doc(got, d, R) == (cm.map_entries(e, tod(d)), cm.map_clock(vv, tod(d))), (d, MAPS[d // 3].name)


# ---------------------------------------------------------------- panic parity

@pytest.mark.parametrize("mode", MODES)
def test_fold_panic_parity(eng, mode):
    """60 single documents of test_fold_panic_parity_per_doc's generator, ten per
    map: the oracle's verdict on the mapped document is the kernel's, and where
    there is none the same bits -- as the oracle, and as the mapped small run."""
    R = PANIC_R
    err = ok = 0
    for i, (e, vv, chain) in enumerate(panic_cases(mode, 60)):
        tod = cm.single(MAPS[i % len(MAPS)], 6)
        dst, srcs = batch_of(R, [(e, vv)]), src_batch_of(R, [chain])
        wd, ws = cm.map_batch(dst, tod), cm.map_srcs(srcs, tod)
        rc, want = oracle.fold(mode, wd, ws)
        if rc != 0:
            for a, b in ((wd, ws), (dst, srcs)):
                with pytest.raises(crdtgpu.CrdtError) as ei:
                    eng.fold(mode, a, b)
                assert ei.value.code == crdtgpu.CRDT_E_ACTOR_RANGE, (i, e, vv, chain)
            err += 1
        else:
            got = eng.fold(mode, wd, ws)
            same(got, want, 1, R, tod, "panic parity %d (a)" % i)
            same(got, cm.map_out(eng.fold(mode, dst, srcs), tod), 1, R, tod, "panic parity %d (b)" % i)
            ok += 1
    assert err > 5 and ok > 5


# ---------------------------------------------------------------- delta extract

@pytest.mark.parametrize("R", [2, 16])
def test_delta_extract(eng, torch, R):
    """parity_case (3,000 documents, sources of 0 ... 130 entries) with states,
    tombstones and peer clocks mapped; a peer clock entry 0 (FULL) stays 0."""
    def build():
        per_doc, peers, srcs, kinds, _ = extract_case(R)
        tod = cm.mixed(15)  # (counters up to 12, a tombstone's up to 3 above its entry's)
        wide_peers = [cm.map_clock(p, tod(d)) for d, p in enumerate(peers)]
        wkinds, wmsgs = expected(R, cm.map_source_lists(per_doc, tod), wide_peers)
        assert (wkinds == kinds).all() and {int(k) for k in kinds} == {model.NONE, model.DELTA, model.FULL}
        cm.assert_mixes(src_batch_of(R, wmsgs), tod, "extract R=%d" % R)
        return SimpleNamespace(srcs=srcs, peers=np.array(peers, dtype=U64).reshape(-1), tod=tod,
                               ws=cm.map_srcs(srcs, tod), wpeers=np.array(wide_peers, dtype=U64).reshape(-1),
                               kinds=wkinds, msgs=wmsgs)
    c = cached(("ex", R), build)
    assert ((c.wpeers == 0) == (c.peers == 0)).all() and (c.peers == 0).any()
    got, kind = extract(eng, torch, c.ws, c.wpeers)
    assert_message(got, kind, c.ws, c.kinds, c.msgs)  # (a)
    small, skind = extract(eng, torch, c.srcs, c.peers)
    want = cm.map_out(small, c.tod)  # (b)
    assert (kind == skind).all()
    ns = c.srcs.n_srcs
    te, tt = int(want.entry_off[ns]), int(want.tomb_off[ns])
    for f, n in (("doc_srcs", None), ("src_actor", ns), ("vv", ns * R), ("entry_off", None), ("tomb_off", None),
                 ("keys", te), ("actors", te), ("counters", te), ("tkeys", tt), ("tactors", tt), ("tcounters", tt)):
        g, w = np.asarray(getattr(got, f))[:n], np.asarray(getattr(want, f))[:n]
        assert (g == w).all(), (f, np.nonzero(g != w)[0][:8])


# ---------------------------------------------------------------- tombstone GC

@pytest.mark.parametrize("R", [2, 64])
def test_tombstone_gc(eng, torch, R):
    def build():
        per_doc, stable = gc_case(R, 1500)
        tb = TombBatch.from_lists(per_doc)
        tod = cm.mixed(50)
        wt, ws = cm.map_batch(tb, tod), cm.map_clocks(stable, R, tod)
        rc, want = oracle.tomb_gc(wt, R, ws)
        assert rc == 0
        cm.assert_mixes(want, tod, "gc R=%d" % R)
        return SimpleNamespace(tb=tb, stable=stable, wt=wt, ws=ws, want=want, tod=tod)
    c = cached(("gc", R), build)
    got = gc_on_gpu(eng, torch, c.wt, R, c.ws)
    small = cm.map_out(gc_on_gpu(eng, torch, c.tb, R, c.stable), c.tod)
    assert (got.offsets == c.want.offsets).all() and (got.offsets == small.offsets).all()
    for d in range(c.tb.n_docs):
        assert got.doc(d) == c.want.doc(d), (d, cm.map_name(c.tod(d)), "(a)")
        assert got.doc(d) == small.doc(d), (d, cm.map_name(c.tod(d)), "(b)")


# ---------------------------------------------------------------- apply (arithmetic: oracle only)

def test_apply_clock_carries_across_the_edges(eng):
    """Local ops bump the acting actor's clock once per ADD and per DELTA_DEL
    (awset.go:89-94, awset-delta_test.go:14-33), so apply is not map-invariant:
    against oracle.apply only.  State and tombstone counters go through the
    maps; the acting clock starts at 2^31 - 3, 2^32 - 3, 2^32 - 1, 2^32,
    2^63 - 3, or so that it lands exactly on 2^64 - 1 (a wrap past that is out
    of scope), and the document's 1 / 64 / 65 / 256 ops carry it across.  The
    dots of added entries, the DELTA_DEL tombstone dots and the output clocks
    are compared per document."""
    rng = random.Random(2064)
    R, n = 4, 240
    starts = [(1 << 31) - 3, (1 << 32) - 3, (1 << 32) - 1, 1 << 32, (1 << 63) - 3, None]
    docs, tombs, per_ops, actors = [], [], [], []
    for d in range(n):
        ents, tb, vv = random_doc(rng, R, rng.randint(0, 64), rng.randint(0, 3), 300, 40)
        n_ops = [1, 64, 65, 256][(d // len(starts)) % 4]
        ops = encode(random_calls(rng, n_ops, 300, [k for k, _, _ in ents]))
        ops += [(CRDT_OP_ADD, rng.randrange(300)) for _ in range(n_ops - len(ops))]  # exactly n_ops
        docs.append((ents, vv))
        tombs.append(tb)
        per_ops.append(ops)
        actors.append(rng.randrange(R))
    tod = cm.mixed(40, period=24)
    st = cm.map_batch(AWSetBatch.from_docs(R, docs), tod)
    tb = cm.map_batch(TombBatch.from_lists(tombs), tod)
    op = OpBatch.from_lists(per_ops, actors)
    bumps = [sum(1 for k, _ in ops if k in (CRDT_OP_ADD, CRDT_OP_DELTA_DEL)) for ops in per_ops]
    clock0 = [starts[d % len(starts)] if starts[d % len(starts)] is not None else TOP - bumps[d] for d in range(n)]
    for d in range(n):
        assert len(per_ops[d]) == [1, 64, 65, 256][(d // len(starts)) % 4] and clock0[d] + bumps[d] <= TOP
        st.vv[d * R + actors[d]] = clock0[d]
    rc, wo, wt = oracle.apply(st, op, tb)
    assert rc == 0
    # the case: the maps are mixed, every start has documents whose clock crossed its edge, and one lands on the top
    cm.assert_mixes(wo, tod, "apply")
    after = [int(wo.vv[d * R + actors[d]]) for d in range(n)]
    assert after == [clock0[d] + bumps[d] for d in range(n)]
    for i, edge in enumerate([1 << 31, 1 << 32, 1 << 32, (1 << 32) + 1, 1 << 63, TOP]):
        assert any(clock0[d] < edge <= after[d] for d in range(i, n, len(starts))), i
    go, gt = eng.apply(st, op, tb)
    assert (go.offsets == wo.offsets).all() and (gt.offsets == wt.offsets).all()
    for d in range(n):
        assert doc_of(go, gt, d, R) == doc_of(wo, wt, d, R), (d, cm.map_name(tod(d)), clock0[d], bumps[d])
