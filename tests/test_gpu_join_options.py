"""GPU parity of every kernel the join options can select
(crdt_ctx_set_option: "performance only, never results").  Each option value
picks another instantiation of the wave kernel (join.hip, launch_wave_ks /
launch_wave_k), of the tile kernels (tile.hip, launch_tile_pass), or another
grid or plan; this file runs them: the wave kernel's plain-store arm at every
K, every tile shape with both store kinds on sizes at the edges of that
shape's own tile, passes and the block-kernel fallback at every shape, the
one-word dispenser and the plan's grid at their ends, worklists on the edges
of a count run, the slab block order on its C == G, padding and S = 3 cases
at every K, and 24 option sets drawn from the whole product.

Every expectation is the C oracle's join (oracle/awset_oracle.c) in both
directions, never another GPU run; device outputs start filled with -1, so a
document that nothing wrote shows in its count, clock and slot bounds.  The
cases and the conditions that make them mean something are in
tests/join_option_cases.py, checked on the CPU by
tests/test_join_option_cases_model.py.
"""

import contextlib
import random

import pytest

import join_option_cases as jc
from crdtgpu import CRDT_E_INVALID, CrdtError
from crdtgpu.batch import OutBuffers
from join_option_cases import PIPE_SHAPES, T_OF_SHAPE
from test_gpu_join_meta import KS, WAVES, case, lane_edge_case
from test_gpu_parity import assert_same_all, host_out

pytestmark = pytest.mark.gpu

SHAPES = sorted(T_OF_SHAPE)

# name: (default, accepted values at the ends of the range, rejected values just outside it); a 0|1 option
# takes any nonzero value as 1 (api.cpp), so it has no value outside its range
OPTIONS = {
    "join_docs_per_wave": (8, (1, 2, 4, 8, 16), (0, 3, 17, 32, -1)),
    "join_nt_stores": (1, (0, 1), ()),
    "join_stage_stores": (1, (0, 1), ()),
    "join_slab_blocks_per_cu": (0, (0, 64), (-1, 65)),
    "join_tiles": (1, (0, 1), ()),
    "join_tile_capacity": (1 << 22, (1, 1 << 28), (0, (1 << 28) + 1)),
    "join_tile_max_passes": (256, (1, 65536), (0, 65537)),
    "join_tile_shape": (9, (0, 10), (-1, 11)),
    "join_tile_nt_stores": (1, (0, 1), ()),
    "join_tile_split_blocks_per_cu": (4, (1, 64), (0, 65)),
    "join_tile_dispensers": (8, (1, 8), (0, 2, 7, 9)),
    "fold_lean_first": (1, (0, 1), ()),
    "probe_blocks_per_cu": (16, (1, 64), (0, 65)),
    "probe_slab": (0, (0, 1), ()),
    "pack_batch_outputs": (0, (0, 1), ()),
    "span_staging": (1, (0, 1), ()),
}


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


@contextlib.contextmanager
def options(eng, max_doc_entries=None, **values):
    """Set the options (and the small-document promise) for the block; back to
    the defaults after it, whatever happened inside."""
    try:
        for name, v in values.items():
            eng.set_option(name, v)
        if max_doc_entries is not None:
            eng.set_max_doc_entries(max_doc_entries)
        yield
    finally:
        for name in values:
            eng.set_option(name, OPTIONS[name][0])
        eng.set_max_doc_entries()


def poisoned(torch, n, R, slots, shared_keys=None):
    o = OutBuffers(n, R, slots, device=torch.device("cuda:0"), shared_keys=shared_keys)
    for t in (o.offsets, o.counts, o.keys, o.actors, o.counters, o.vv):
        t.fill_(-1)
    return o


def check_device(eng, torch, c, shared=(False,), join=True):
    """Device-resident through the async ABI into poisoned outputs: the join, and
    the exchange with its own (False) or a shared (True) key column."""
    a, b, ab, ba = c
    n, R = a.n_docs, a.R
    dev = torch.device("cuda:0")
    da, db = a.to(dev), b.to(dev)
    slots = int(a.offsets[-1]) + int(b.offsets[-1])
    if join:
        o = poisoned(torch, n, R, slots)
        eng.join_async(da, db, o)
        eng.sync()
        assert_same_all(host_out(o, torch), ab, n, R)
    for sh in shared:
        o1 = poisoned(torch, n, R, slots)
        o2 = poisoned(torch, n, R, slots, shared_keys=o1 if sh else None)
        eng.exchange_async(da, db, o1, o2)
        eng.sync()
        assert_same_all(host_out(o1, torch), ab, n, R)
        assert_same_all(host_out(o2, torch), ba, n, R)


def check_host(eng, c):
    """The host path (the *_batch calls): tiles counted on the host, exactly the
    passes they need, no block-kernel fallback behind them (api.cpp, plan_tiles)."""
    a, b, ab, ba = c
    n, R = a.n_docs, a.R
    assert_same_all(eng.join(a, b), ab, n, R)
    o1, o2 = eng.exchange(a, b)
    assert_same_all(o1, ab, n, R)
    assert_same_all(o2, ba, n, R)


# ---------------------------------------------------------------- a. wave kernel, plain stores

@pytest.mark.parametrize("stage", [0, 1], ids=["scattered", "staged"])
@pytest.mark.parametrize("K", KS, ids=lambda k: "K%d" % k)
def test_wave_plain_stores(eng, torch, K, stage):
    """join_nt_stores = 0 (join_wave_kernel's AUX = 0 arm) at every K, staged and
    lane-scattered: 1, 9 and 65 workgroups' worth of documents at the default K
    with partly filled waves, inputs with and without `counts`; the join, and the
    exchange with an own and a shared key column."""
    with options(eng, 64, join_nt_stores=0, join_docs_per_wave=K, join_stage_stores=stage):
        for n in (3, 33, 257):
            for slack in (0, 3):
                check_device(eng, torch, case(n, slack), shared=(False, True))


@pytest.mark.parametrize("K", KS, ids=lambda k: "K%d" % k)
def test_wave_plain_stores_with_large_documents(eng, torch, K):
    """The same arm without the promise of small documents: documents above 64
    entries at the wave's lane edges leave for the worklist, the rest is written
    with plain stores around them."""
    with options(eng, join_nt_stores=0, join_docs_per_wave=K):
        check_device(eng, torch, lane_edge_case(K), shared=(False, True))


# ---------------------------------------------------------------- b. tile kernels, every shape x store kind

@pytest.mark.parametrize("nts", [0, 1], ids=["plain", "nt"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "shape%d" % s)
def test_tile_shapes_on_their_own_tile_edges(eng, torch, shape, nts):
    """Documents of T k - 1, T k and T k + 1 merged positions (k = 1, 2, 3, 5; T
    this shape's tile), split evenly and 70 / 65 against the rest, with both store
    kinds.  The host path launches the passes the host's own tile count needs and
    no fallback behind them; with a workspace of exactly that many tiles, one
    tile more on the device (tile_count_kernel) would find neither a pass nor the
    block kernel and leave its document unwritten: this pins api.cpp's host_tiles
    to the device's count at this T.  Device-resident the bound comes from the
    batch size and the fallback's gate is live."""
    c = jc.boundary_case(T_OF_SHAPE[shape])
    with options(eng, join_tile_shape=shape, join_tile_nt_stores=nts):
        check_host(eng, c)
        check_device(eng, torch, c)
    with options(eng, join_tile_shape=shape, join_tile_nt_stores=nts,
                 join_tile_capacity=jc.host_tiles(c[0], c[1], shape)):
        check_host(eng, c)


# ---------------------------------------------------------------- c. passes at every shape

@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "shape%d" % s)
def test_tile_passes_at_every_shape(eng, torch, shape, cap):
    """A workspace of 1 or 3 tiles at every shape: the carry word across a pass
    boundary inside a document, the pipelined shapes' later-pass kernel
    (join_tile_pipe_later_kernel) and join_tile_kernel at pass > 0.  Cap 1 on the
    pipelined shapes runs with plain stores, the later-pass kernel's other arm."""
    c = jc.mixed_case()
    assert jc.host_tiles(c[0], c[1], shape) >= 2 * cap + 1
    nts = 0 if cap == 1 and shape in PIPE_SHAPES else 1
    with options(eng, join_tile_shape=shape, join_tile_capacity=cap, join_tile_max_passes=4096,
                 join_tile_nt_stores=nts):
        check_host(eng, c)
        check_device(eng, torch, c, join=False)


# ---------------------------------------------------------------- d. fallback at every T

@pytest.mark.parametrize("shape", [10, 9, 0], ids=lambda s: "T%d" % T_OF_SHAPE[s])
def test_tile_fallback_at_every_tile_size(eng, torch, shape):
    """More tiles than one pass of three: the plan sets the fallback word and the
    block kernel takes the worklist, at one shape of each tile size."""
    c = jc.mixed_case()
    assert jc.host_tiles(c[0], c[1], shape) > 3
    with options(eng, join_tile_shape=shape, join_tile_capacity=3, join_tile_max_passes=1):
        check_host(eng, c)
        check_device(eng, torch, c)


# ---------------------------------------------------------------- e. dispensers x shapes

@pytest.mark.parametrize("shape", [0, 4, 10])
def test_tile_one_dispenser_at_other_shapes(eng, torch, shape):
    """The one-word dispenser under join_tile_kernel (shape 0), the pipelined
    kernel (4) and the smallest tile (10)."""
    c = jc.mixed_case()
    with options(eng, join_tile_shape=shape, join_tile_dispensers=1):
        check_host(eng, c)
        check_device(eng, torch, c, join=False)


# ---------------------------------------------------------------- f. plan grid

@pytest.mark.parametrize("bpc", [1, 64])
def test_tile_split_grid(eng, torch, bpc):
    """tile_split_kernel's grid-stride loop at the smallest and the largest grid."""
    with options(eng, join_tile_split_blocks_per_cu=bpc):
        for c in (jc.mixed_case(), jc.boundary_case(1024)):
            check_host(eng, c)
            check_device(eng, torch, c, join=False)


# ---------------------------------------------------------------- g. worklist run edges

@pytest.mark.parametrize("cap", [1 << 22, 1024], ids=["one_pass", "cap1024"])
@pytest.mark.parametrize("n_large", [1023, 1024, 1025, 2049])
def test_worklist_on_run_edges(eng, torch, n_large, cap):
    """A worklist one short of, exactly, one past one count run of 1,024 slots
    (tile_count_kernel, tile_scan_kernel) and one past two; at a workspace of
    1,024 tiles a pass boundary falls on each run boundary."""
    c = jc.many_large_case(n_large)
    with options(eng, join_tile_capacity=cap):
        check_host(eng, c)
        check_device(eng, torch, c)


# ---------------------------------------------------------------- h. slab order

@pytest.mark.parametrize("large", [False, True], ids=["promise64", "large_docs"])
@pytest.mark.parametrize("extra", ["G", "G+1", "2G+1"])
@pytest.mark.parametrize("v", [1, 2])
@pytest.mark.parametrize("K", KS, ids=lambda k: "K%d" % k)
def test_slab_order(eng, torch, K, v, extra, large):
    """The wave kernel's slab block order with C == G workgroups (in order),
    G + 1 (S = 2, G - 1 padding blocks) and 2 G + 1 (S = 3), the last workgroup a
    document short, at every K; under the promise of small documents, and without
    it with five documents bound for the worklist from the first and last
    document and the first and last slab."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count  # (api.cpp: ctx->n_cu, the same property)
    G = v * n_cu
    extra_blocks = {"G": 0, "G+1": 1, "2G+1": G + 1}[extra]
    n_docs, C, _ = jc.slab_geometry(K, v, n_cu, extra_blocks)
    m = jc.slab_map(C, G)
    if extra_blocks:
        assert C > G and jc.slab_grid(m) > C and m[1] == (2 if extra_blocks == 1 else 3)
    else:
        assert C == G and m[0] == 0
    c = jc.slab_case(K, v, n_cu, extra_blocks, large)
    assert c[0].n_docs == n_docs == WAVES * K * C - 1
    with options(eng, None if large else 64, join_slab_blocks_per_cu=v, join_docs_per_wave=K):
        check_device(eng, torch, c, shared=(True,))


# ---------------------------------------------------------------- i. combinations

def _option_sets(n):
    rng = random.Random(0x0B7)
    sets = []
    for _ in range(n):
        sets.append((("join_docs_per_wave", rng.choice(KS)),
                     ("join_nt_stores", rng.randint(0, 1)),
                     ("join_stage_stores", rng.randint(0, 1)),
                     ("join_slab_blocks_per_cu", rng.randint(0, 1)),
                     ("join_tiles", rng.randint(0, 1)),
                     ("join_tile_capacity", rng.choice([1, 7, 1 << 22])),
                     ("join_tile_max_passes", rng.choice([1, 256, 4096])),
                     ("join_tile_shape", rng.randint(0, 10)),
                     ("join_tile_nt_stores", rng.randint(0, 1)),
                     ("join_tile_split_blocks_per_cu", rng.randint(1, 64)),
                     ("join_tile_dispensers", rng.choice([1, 8]))))
    return sets


def _set_id(s):
    short = {"join_docs_per_wave": "K", "join_nt_stores": "nt", "join_stage_stores": "stage",
             "join_slab_blocks_per_cu": "slab", "join_tiles": "tiles", "join_tile_capacity": "cap",
             "join_tile_max_passes": "passes", "join_tile_shape": "shape", "join_tile_nt_stores": "tnt",
             "join_tile_split_blocks_per_cu": "split", "join_tile_dispensers": "disp"}
    return "-".join("%s%d" % (short[k], v) for k, v in s)


@pytest.mark.parametrize("opts", _option_sets(24), ids=_set_id)
def test_option_combinations(eng, torch, opts):
    """24 option sets drawn from the product of every join and tile option's
    values, device-resident on the mixed batch: whatever the set selects -- tiles
    in one pass or many, the block kernel behind a closed or an open gate, or no
    tile path at all -- the bits are the oracle's."""
    with options(eng, **dict(opts)):
        check_device(eng, torch, jc.mixed_case())


# ---------------------------------------------------------------- j. the validation table

def test_option_validation_table(eng):
    """Every option accepts both ends of its range and rejects the values just
    outside it with CRDT_E_INVALID, keeping its value; an unknown name is
    rejected."""
    for name, (default, good, bad) in OPTIONS.items():
        try:
            for v in good:
                eng.set_option(name, v)
            for v in bad:
                with pytest.raises(CrdtError) as e:
                    eng.set_option(name, v)
                assert e.value.code == CRDT_E_INVALID, (name, v)
        finally:
            eng.set_option(name, default)
    for name in ("join_tile_shapes", "", "JOIN_TILES"):
        with pytest.raises(CrdtError) as e:
            eng.set_option(name, 1)
        assert e.value.code == CRDT_E_INVALID

