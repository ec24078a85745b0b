"""GPU: the plain join and exchange (crdt_awset_join_async, crdt_awset_exchange_async) on every
case of tests/join_edge_cases.py (pinned by tests/test_join_edges_model.py), bit-exact against
the C oracle's join, under every option that selects other code.

Inputs are device-resident.  All six output arrays are allocated GUARD elements longer than
the call may use and filled with a pattern no case holds.  After the call every document's
live entries, count, clock and the n_docs + 1 slot bounds are compared bit-exactly; every
word past an array's end must still be the pattern; and every slot no document holds live --
which is some document's slack inside its own capacity -- must hold the pattern or the zeros
the whole-sector stores pad with, so a survivor or a stray store outside a document's live
prefix shows.  No test provokes a fault: the over-count inputs stay inside their arrays even
for a kernel that does not clamp (test_over_count_cases_stay_inside_the_arrays).
"""

import contextlib

import numpy as np
import pytest

import crdtgpu
import join_option_cases as jc
from crdtgpu import CRDT_E_CAPACITY
from crdtgpu.batch import OutBuffers
from join_edge_cases import FILLS, OVER_CASES, SLACKS, TABLE, R, batches, concat
from oracle import oracle
from test_gpu_compare import _code, dev_of
from test_gpu_join_options import OPTIONS

pytestmark = pytest.mark.gpu

GUARD = 64
S32, S64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A  # no key, actor, counter or clock word of the table
FIELDS = ("offsets", "counts", "keys", "actors", "counters", "vv")
MODES = ("join_ab", "join_ba", "exchange", "exchange_shared_keys")
LOOK_BACK_PER_TILE = 1  # join_tile_kernel, T = 1024 (shapes 0-3 look back once per tile; 4-10 are pipelined)
PASSES = 512  # most passes a call of this file launches: with a workspace of one tile, one pass a tile

# the options that select different code, each against the defaults
OPTION_SETS = {
    "defaults": {},
    "scattered_stores": dict(join_stage_stores=0),
    "plain_stores": dict(join_nt_stores=0),
    "scattered_plain_stores": dict(join_stage_stores=0, join_nt_stores=0),
    "K1": dict(join_docs_per_wave=1),
    "K16": dict(join_docs_per_wave=16),
    "shape10": dict(join_tile_shape=10),
    "look_back_per_tile": dict(join_tile_shape=LOOK_BACK_PER_TILE),
    "block_kernel": dict(join_tiles=0),
    "capacity1": dict(join_tile_capacity=1, join_tile_max_passes=PASSES),
    "capacity1_shape10": dict(join_tile_capacity=1, join_tile_max_passes=PASSES, join_tile_shape=10),
    "capacity1_look_back_per_tile": dict(join_tile_capacity=1, join_tile_max_passes=PASSES,
                                         join_tile_shape=LOOK_BACK_PER_TILE),
    "one_dispenser": dict(join_tile_dispensers=1),
    "one_dispenser_shape10": dict(join_tile_dispensers=1, join_tile_shape=10),
}
# the three paths of a large document, at a tile shape
PATHS = {
    "tiles": lambda shape: dict(join_tile_shape=shape),
    "block_kernel": lambda shape: dict(join_tiles=0),
    "capacity1": lambda shape: dict(join_tile_shape=shape, join_tile_capacity=1, join_tile_max_passes=PASSES),
}


def tiles_of(a, b, opts):
    """Tiles of the call in either direction at the options' shape (api.cpp, host_tiles)."""
    shape = opts.get("join_tile_shape", OPTIONS["join_tile_shape"][0])
    return max(jc.host_tiles(a, b, shape), jc.host_tiles(b, a, shape), 1)


def with_passes(a, b, opts):
    """opts with exactly the passes a workspace of one tile needs for this batch (a device-resident
    call launches every pass it is allowed; the ones past its tiles return at once)."""
    if opts.get("join_tile_capacity") != 1:
        return opts
    assert tiles_of(a, b, opts) <= PASSES  # every tile gets its pass: no fallback to the block kernel
    return dict(opts, join_tile_max_passes=tiles_of(a, b, opts))


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


@contextlib.contextmanager
def options(eng, **values):
    """Set the options for the block; back to the defaults after it, whatever happened inside."""
    try:
        for name, v in values.items():
            eng.set_option(name, v)
        yield
    finally:
        for name in values:
            eng.set_option(name, OPTIONS[name][0])


# ------------------------------------------------------------------- helpers

def poisoned(torch, n, slots, shared_keys=None):
    """Output buffers for n documents and `slots` entries, every array GUARD longer and filled
    with the pattern; shared_keys: the other output of an exchange, whose key column this one uses."""
    dev = dev_of(torch)
    o = OutBuffers(n, R, slots + GUARD, device=dev, shared_keys=shared_keys)
    full = lambda m, dt, v: torch.full((m + GUARD,), v, dtype=dt, device=dev)  # noqa: E731
    o.offsets, o.counts, o.vv = full(n + 1, torch.int32, S32), full(n, torch.int32, S32), full(n * R, torch.int64, S64)
    o.actors.fill_(S32)
    o.counters.fill_(S64)
    if shared_keys is None:
        o.keys.fill_(S64)
    return o


def download(o):
    return {f: getattr(o, f).cpu().numpy().view(np.uint32 if f in ("offsets", "counts", "actors") else np.uint64)
            for f in FIELDS}


def check(raw, want, n, slots, what):
    """raw (download) against the oracle's `want` for n documents of `slots` entry slots in all."""
    sizes = dict(offsets=n + 1, counts=n, vv=n * R, keys=slots, actors=slots, counters=slots)
    for f, m in sizes.items():
        tail = raw[f][m:]
        assert len(tail) == GUARD
        bad = np.flatnonzero(tail != (S32 if tail.dtype == np.uint32 else S64))
        assert bad.size == 0, "%s: %s[%d] past the array's end was written" % (what, f, m + bad[0])
    assert (raw["offsets"][: n + 1] == want.offsets[: n + 1]).all(), (what, "offsets")
    bad = np.flatnonzero(raw["counts"][:n] != want.counts[:n])
    assert bad.size == 0, "%s: counts[%d] = %d, oracle %d" % (what, bad[0], raw["counts"][bad[0]], want.counts[bad[0]])
    bad = np.flatnonzero(raw["vv"][: n * R] != want.vv[: n * R])
    assert bad.size == 0, "%s: clock of document %d" % (what, bad[0] // R if bad.size else -1)
    cnt = want.counts[:n].astype(np.int64)
    start = want.offsets[:n].astype(np.int64)
    idx = np.repeat(start, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    dead = np.ones(slots, dtype=bool)
    dead[idx] = False
    doc_at = lambda i: int(np.searchsorted(want.offsets[: n + 1].astype(np.int64), i, side="right")) - 1  # noqa: E731
    for f in ("keys", "actors", "counters"):
        g, w = raw[f][:slots], np.asarray(getattr(want, f))
        bad = np.flatnonzero(g[idx] != w[idx])
        assert bad.size == 0, "%s: %s of document %d differ (slot %d: %#x, oracle %#x)" % (
            what, f, doc_at(idx[bad[0]]), idx[bad[0]], int(g[idx[bad[0]]]), int(w[idx[bad[0]]]))
        rest = g[dead]
        bad = np.flatnonzero((rest != (S32 if g.dtype == np.uint32 else S64)) & (rest != 0))
        if bad.size:
            i = int(np.flatnonzero(dead)[bad[0]])
            raise AssertionError("%s: %s[%d] = %#x was written past the live entries of document %d"
                                 % (what, f, i, int(g[i]), doc_at(i)))


_wants = {}


def expected(key, a, b):
    """(a <- b, b <- a) by the C oracle, once per key, never modified."""
    if key not in _wants:
        rc1, ab = oracle.join(a, b)
        rc2, ba = oracle.join(b, a)
        assert rc1 == 0 and rc2 == 0
        _wants[key] = (ab, ba)
    return _wants[key]


def launch(eng, torch, mode, da, db, n, slots):
    """One call of `mode` into poisoned outputs: [(output, which direction it holds)]."""
    if mode == "join_ab":
        o = poisoned(torch, n, slots)
        eng.join_async(da, db, o)
        return [(o, 0)]
    if mode == "join_ba":
        o = poisoned(torch, n, slots)
        eng.join_async(db, da, o)
        return [(o, 1)]
    o1 = poisoned(torch, n, slots)
    o2 = poisoned(torch, n, slots, shared_keys=o1 if mode == "exchange_shared_keys" else None)
    eng.exchange_async(da, db, o1, o2)
    return [(o1, 0), (o2, 1)]


def run_clean(eng, torch, a, b, wants, what, modes=MODES):
    n, slots = a.n_docs, int(a.offsets[-1]) + int(b.offsets[-1])
    da, db = a.to(dev_of(torch)), b.to(dev_of(torch))
    for mode in modes:
        outs = launch(eng, torch, mode, da, db, n, slots)
        eng.sync()
        torch.cuda.synchronize()
        for o, direction in outs:
            check(download(o), wants[direction], n, slots, "%s %s %s" % (what, mode, "ab" if direction == 0 else "ba"))


_tables = {}


def table(extra=(0, 0), fill="zeros"):
    """The clean cases as one batch pair (tests/test_join_edges_model.py checks that each case's
    documents come out of it as they do alone), with its expectations; built once per build."""
    key = (extra, fill)
    if key not in _tables:
        a, b, _ = concat(TABLE, extra, fill)
        _tables[key] = (a, b, expected(("table", extra), a, b))  # (the oracle never reads the slack: one per layout)
    return _tables[key]


def large(case):
    return any(max(len(d[0]), len(s[0])) > jc.WAVE_MAX for d, s in zip(case.dst_docs, case.src_docs))


# ------------------------------------------------------------- 1. every case alone

@pytest.mark.parametrize("case", TABLE, ids=lambda c: c.name)
def test_case_alone(eng, torch, case):
    """The case as its own batch: its first document is the batch's first, its last the one
    that alone writes offsets[n_docs], and a one-document case a batch of exactly one.  A case
    with a large document runs on the tile path at the shape it was built around, through the
    block kernel, and with a workspace of one tile (every later tile of a document then takes
    its placed count from the carry word)."""
    a, b = batches(case)
    wants = expected(case.name, a, b)
    if not large(case):
        run_clean(eng, torch, a, b, wants, case.name)
        return
    shape = case.shape if case.shape is not None else OPTIONS["join_tile_shape"][0]
    for path, opts in PATHS.items():
        with options(eng, **with_passes(a, b, opts(shape))):
            run_clean(eng, torch, a, b, wants, "%s [%s]" % (case.name, path), modes=("join_ab", "join_ba", "exchange"))


# ------------------------------------------------------------- 2. the table under every option

@pytest.mark.parametrize("name", OPTION_SETS, ids=str)
def test_table_under_options(eng, torch, name):
    a, b, wants = table()
    with options(eng, **with_passes(a, b, OPTION_SETS[name])):
        run_clean(eng, torch, a, b, wants, name)


# ------------------------------------------------------------- 3. slack is never read

@pytest.mark.parametrize("name", ["defaults", "scattered_stores", "shape10", "block_kernel", "capacity1_shape10",
                                  "look_back_per_tile"])
@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("extra", SLACKS, ids=lambda s: "slack_%d_%d" % s)
def test_slack_is_never_read(eng, torch, extra, fill, name):
    """Every case with 1 and 9 (9 and 1) spare slots a document on dst and src, the slack zeros,
    all-ones, or entries that continue the document -- keys ascending past its last live key,
    among them keys the other side holds live, under dots the other side's clock has not seen:
    the result is the oracle's of the live prefixes."""
    a, b, wants = table(extra, fill)
    with options(eng, **with_passes(a, b, OPTION_SETS[name])):
        run_clean(eng, torch, a, b, wants, "%s %s %s" % (name, fill, extra), modes=("join_ab", "join_ba", "exchange_shared_keys"))


# ------------------------------------------------------------- 4. counts above the slots

OVER_RUNS = [(c, p) for c in OVER_CASES for p in PATHS if p == "tiles" or large(c)]  # (a wave-path case has one path)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case,path", OVER_RUNS, ids=lambda x: x if isinstance(x, str) else x.name)
def test_count_above_slots_is_clamped(eng, torch, case, path, mode):
    """One document's count is its slots + 9 (10), as dst or as src of the call: crdt_ctx_sync
    returns CRDT_E_CAPACITY and a second sync is clean; the bad document is the join of its
    clamped prefix, chosen for the wave kernel or the worklist by its clamped sizes; every other
    document is bit-exact; nothing outside the live prefixes holds anything but the pattern or
    padding zeros -- the neighbours' regions are untouched."""
    a, b = batches(case)
    ca, cb = batches(case, clamped=True)
    wants = expected(case.name, ca, cb)
    n, slots = a.n_docs, int(a.offsets[-1]) + int(b.offsets[-1])
    da, db = a.to(dev_of(torch)), b.to(dev_of(torch))
    shape = case.shape if case.shape is not None else OPTIONS["join_tile_shape"][0]
    with options(eng, **with_passes(ca, cb, PATHS[path](shape))):
        outs = launch(eng, torch, mode, da, db, n, slots)
        assert _code(eng.sync) == CRDT_E_CAPACITY
        eng.sync()  # cleared
        torch.cuda.synchronize()
        for o, direction in outs:
            check(download(o), wants[direction], n, slots, "%s [%s] %s %d" % (case.name, path, mode, direction))
