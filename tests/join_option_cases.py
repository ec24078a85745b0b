"""Host batches for the join option tests (tests/test_gpu_join_options.py), each
with the C oracle's join in both directions, built once and never modified --
and the conditions under which those tests mean something (a size on every
tile edge of every tile shape, more tiles than two passes hold, a launch with
more blocks than one slab front), restated here so that
tests/test_join_option_cases_model.py can check them without a GPU.

No GPU is touched in this module.
"""

import functools
import random

import numpy as np

from crdtgpu.batch import AWSetBatch
from helpers import batch_of, random_state
from oracle import oracle
from test_gpu_join_meta import R as SLAB_R
from test_gpu_join_meta import WAVES, _docs
from test_gpu_tiles import _sub, interleaved

# merged positions per tile of each join_tile_shape (tile.hip, tile_positions)
T_OF_SHAPE = {0: 2048, 1: 1024, 2: 2048, 3: 2048, 4: 1024, 5: 1024, 6: 2048, 7: 1024, 8: 1024, 9: 1024, 10: 512}
PIPE_SHAPES = (4, 5, 6, 7, 8, 9, 10)  # join_tile_pipe_kernel and its later-pass kernel (tile.hip, launch_tile_pass)
WAVE_MAX = 64  # a document above this on either side leaves the wave kernel for the worklist
K_RUN = 1024  # worklist slots per run of the tile count and scan (tile.hip, kRun)

BOUNDARY_KS = (1, 2, 3, 5)
MIXED_R = BOUNDARY_R = 3


def live_sizes(a, b):
    nd = np.array([a.live(d) for d in range(a.n_docs)], dtype=np.int64)
    ns = np.array([b.live(d) for d in range(b.n_docs)], dtype=np.int64)
    return nd, ns


def large_docs(a, b):
    nd, ns = live_sizes(a, b)
    return (nd > WAVE_MAX) | (ns > WAVE_MAX)


def doc_tiles(a, b, shape):
    """Tiles of each document of a <- b at a tile shape: ceil((nd + ns) / T) where
    a side has more than 64 live entries, else 0 (api.cpp, host_tiles)."""
    T = T_OF_SHAPE[shape]
    nd, ns = live_sizes(a, b)
    return np.where((nd > WAVE_MAX) | (ns > WAVE_MAX), (nd + ns + T - 1) // T, 0)


def host_tiles(a, b, shape):
    return int(doc_tiles(a, b, shape).sum())


def _with_oracle(a, b):
    rc1, ab = oracle.join(a, b)
    rc2, ba = oracle.join(b, a)
    assert rc1 == 0 and rc2 == 0
    return a, b, ab, ba


# ---------------------------------------------------------------- tile edges

def boundary_sizes(T):
    """(nd, ns) live sizes whose sum sits on T k - 1, T k and T k + 1 for every k
    of BOUNDARY_KS, split evenly and lopsidedly (one side barely above the wave
    kernel's 64), and the pairs around 64 itself."""
    sizes = []
    for k in BOUNDARY_KS:
        for total in (T * k - 1, T * k, T * k + 1):
            sizes.append((total // 2, total - total // 2))
        sizes.append((T * k - 70, 70))
        sizes.append((65, T * k - 65))
    sizes += [(64, 65), (65, 64), (0, T), (64, 64)]  # (64, 64): the wave path, no tile
    return sizes


@functools.lru_cache(maxsize=None)
def boundary_case(T):
    """R = 3, one document pair per size of boundary_sizes(T) over interleaved key
    ranges (test_gpu_tiles.interleaved: shares 0.3, 0.9 and 1.0 of dst's keys also
    in src), dst tight and src with two spare slots a document (so `counts`)."""
    rng = random.Random(0xB0DE + T)
    docs_d, docs_s = [], []
    for i, (nd, ns) in enumerate(boundary_sizes(T)):
        n = int(max(nd, ns) * 1.06) + 48  # (src of interleaved comes out a little short of n)
        (de, dvv), (se, svv) = interleaved(rng, n, BOUNDARY_R, (0.3, 0.9, 1.0)[i % 3])
        assert len(de) >= nd and len(se) >= ns
        docs_d.append(([de[j] for j in sorted(rng.sample(range(len(de)), nd))], dvv))
        docs_s.append(([se[j] for j in sorted(rng.sample(range(len(se)), ns))], svv))
    a, b = batch_of(BOUNDARY_R, docs_d), batch_of(BOUNDARY_R, docs_s, slack=2)
    assert a.counts is None and b.counts is not None
    return _with_oracle(a, b)


# ---------------------------------------------------------------- passes, fallback, grids

MIXED_SIZES = (0, 5, 64, 65, 511, 513, 1023, 1025, 2049, 7000)


@functools.lru_cache(maxsize=None)
def mixed_case():
    """R = 3, 60 pairs of wave-sized, block-sized and multi-tile documents in one
    batch, spare slots (and `counts`) on both inputs."""
    rng = random.Random(0x313ED)
    sz = lambda: rng.choice(MIXED_SIZES)  # noqa: E731
    dsts = [random_state(rng, MIXED_R, sz(), 40000, 20) for _ in range(60)]
    srcs = [random_state(rng, MIXED_R, sz(), 40000, 20) for _ in range(60)]
    return _with_oracle(batch_of(MIXED_R, dsts, slack=5), batch_of(MIXED_R, srcs, slack=2))


# ---------------------------------------------------------------- worklist runs

@functools.lru_cache(maxsize=None)
def many_large_case(n_large):
    """2 n_large pairs, every even one 65 entries against 3 (one tile each, the
    smallest document the worklist takes), every odd one at most 64 a side: a
    worklist of exactly n_large slots."""
    dsts, srcs = _docs(2 * n_large, {2 * i: (65, 3) for i in range(n_large)})
    return _with_oracle(batch_of(SLAB_R, dsts), batch_of(SLAB_R, srcs, slack=1))


# ---------------------------------------------------------------- slab order

def slab_map(C, G):
    """crdt_device.hpp, slab_map: (G, S, C)."""
    if G == 0 or C <= G:
        return 0, 0, C
    return G, (C + G - 1) // G, C


def slab_grid(m):
    G, S, C = m
    return G * S if G else C


PAD = 0xFFFFFFFF


def slab_chunk(m, c):
    G, S, C = m
    if G == 0:
        return c
    ch = (c % G) * S + c // G
    return ch if ch < C else PAD


def slab_geometry(K, v, n_cu, extra_blocks):
    """(n_docs, C, G) of slab_case: C workgroups of 4 K documents, the last one
    document short, against a slab front of G = v n_cu."""
    G = v * n_cu
    n_docs = WAVES * K * (G + extra_blocks) - 1
    per = WAVES * K
    return n_docs, (n_docs + per - 1) // per, G


LARGE_SIZES = ((65, 70), (130, 3), (700, 66), (64, 65), (90, 200))


def slab_large_at(K, v, n_cu, extra_blocks):
    """Five documents above 64 entries: the first and the last document, one in
    the last chunk of the first slab, one in the first chunk of the last slab that
    holds a document, and one in the middle of the batch."""
    n_docs, C, G = slab_geometry(K, v, n_cu, extra_blocks)
    S = max(1, slab_map(C, G)[1])
    per = WAVES * K
    at = [0, n_docs - 1, (S - 1) * per + 2, (C - 1) // S * S * per + 1, n_docs // 2]
    assert len(set(at)) == 5 and max(at) == n_docs - 1
    return dict(zip(at, LARGE_SIZES))


POOL = 1021  # documents the slab batches repeat (a prime: no two workgroups of a slab front alike)


@functools.lru_cache(maxsize=None)
def _pool():
    dsts, srcs = _docs(POOL)
    return batch_of(SLAB_R, dsts), batch_of(SLAB_R, srcs, slack=3)


def _concat(R, parts):
    counted = any(p.counts is not None for p in parts)
    sizes = np.concatenate([np.diff(np.asarray(p.offsets).astype(np.int64)) for p in parts])
    offsets = np.zeros(len(sizes) + 1, dtype=np.uint32)
    np.cumsum(sizes, out=offsets[1:])
    cat = lambda f: np.concatenate([getattr(p, f) for p in parts])  # noqa: E731
    return AWSetBatch(R, offsets, cat("keys"), cat("actors"), cat("counters"), cat("vv"),
                      cat("counts") if counted else None)


def _repeat(pool, n_docs, singles, R):
    """n_docs documents: document i is pool document i mod POOL, or singles[i]."""
    cuts = sorted(singles)
    parts, i = [], 0
    while i < n_docs:
        if i in singles:
            parts.append(singles[i])
            i += 1
            continue
        j = min([n_docs, (i // POOL + 1) * POOL] + [c for c in cuts if c > i])
        parts.append(_sub(pool, i % POOL, i % POOL + (j - i), R))
        i = j
    return _concat(R, parts)


def slab_batches(K, v, n_cu, extra_blocks, large=False):
    n_docs = slab_geometry(K, v, n_cu, extra_blocks)[0]
    pa, pb = _pool()
    sa, sb = {}, {}
    if large:
        at = slab_large_at(K, v, n_cu, extra_blocks)
        dsts, srcs = _docs(len(at), dict(enumerate(at.values())))
        for i, d in enumerate(at):
            sa[d], sb[d] = batch_of(SLAB_R, [dsts[i]]), batch_of(SLAB_R, [srcs[i]], slack=3)
    return _repeat(pa, n_docs, sa, SLAB_R), _repeat(pb, n_docs, sb, SLAB_R)


@functools.lru_cache(maxsize=2)
def slab_case(K, v, n_cu, extra_blocks, large=False):
    """R = 2, documents of 0..64 entries (test_gpu_join_meta._docs, repeated with
    period POOL), one fewer than fill v n_cu + extra_blocks workgroups of the wave
    kernel at K documents a wave; large: five of them above 64 (slab_large_at)."""
    return _with_oracle(*slab_batches(K, v, n_cu, extra_blocks, large))
