"""The conditions that keep tests/test_gpu_join_options.py from passing
vacuously, checked on the CPU: every tile shape's case has a document on each
edge of that shape's tile size, the passes cases have more tiles than two
passes hold, the worklist cases are exactly as long as they say, and the slab
cases give the wave kernel more workgroups than one slab front -- with a
restatement of the slab map itself (crdt_device.hpp: slab_map, slab_grid,
slab_chunk) checked to be a permutation plus padding.  CPU only."""

import re
from pathlib import Path

import numpy as np
import pytest

import join_option_cases as jc
from join_option_cases import PAD, T_OF_SHAPE, slab_chunk, slab_grid, slab_map

CSRC = Path(__file__).resolve().parent.parent / "go-crdt-playground_amd" / "csrc"


def test_tile_table_matches_the_dispatch():
    """T_OF_SHAPE restates tile.hip's tile_positions: every `case s: return a * b`
    line of it, its default (shape 0), and no shape beyond what the option accepts."""
    src = (CSRC / "tile.hip").read_text()
    body = src[src.index("uint32_t tile_positions(uint32_t shape)"):]
    body = body[:body.index("\n}\n")]
    got = {int(s): int(a) * int(b) for s, a, b in re.findall(r"case (\d+): return (\d+) \* (\d+);", body)}
    a, b = re.search(r"default: return (\d+) \* (\d+);", body).groups()
    got[0] = int(a) * int(b)
    assert got == T_OF_SHAPE
    api = (CSRC / "api.cpp").read_text()
    opt = api[api.index('strcmp(name, "join_tile_shape")'):]
    assert "value < 0 || value > %d" % max(T_OF_SHAPE) in opt[:opt.index("return CRDT_OK")]


@pytest.mark.parametrize("shape", sorted(T_OF_SHAPE))
def test_boundary_case_sits_on_every_tile_edge(shape):
    T = T_OF_SHAPE[shape]
    a, b, _, _ = jc.boundary_case(T)
    nd, ns = jc.live_sizes(a, b)
    big = jc.large_docs(a, b)
    tot = nd + ns
    for k in jc.BOUNDARY_KS:
        for edge in (T * k - 1, T * k, T * k + 1):
            hit = big & (tot == edge)
            assert hit.any(), (T, k, edge)
            assert (tot[hit] % T == edge % T).all() and edge % T in (T - 1, 0, 1)
        assert ((nd == T * k - 70) & (ns == 70)).any() and ((nd == 65) & (ns == T * k - 65)).any(), (T, k)
        assert (big & (tot == T * k) & (abs(nd - ns) <= 1)).any(), (T, k)  # and the even split
    assert ((nd == 64) & (ns == 65)).any()
    wave = (nd == 64) & (ns == 64)
    assert wave.any() and not big[wave].any()
    tiles = jc.doc_tiles(a, b, shape)
    assert (tiles[wave] == 0).all() and (tiles[big] >= 1).all()
    assert b.counts is not None and (np.diff(b.offsets.astype(np.int64)) == ns + 2).all()
    assert a.n_docs <= 26


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("shape", sorted(T_OF_SHAPE))
def test_mixed_case_straddles_passes(shape, cap):
    a, b, _, _ = jc.mixed_case()
    assert jc.host_tiles(a, b, shape) >= 2 * cap + 1
    # a document of three tiles or more: at one tile a pass, it straddles two pass boundaries
    assert jc.doc_tiles(a, b, shape).max() >= 3
    nd, ns = jc.live_sizes(a, b)
    big = jc.large_docs(a, b)
    assert (~big).any() and big.any() and a.counts is not None and b.counts is not None
    assert ((nd > 64) & (nd <= 1025)).any() and (nd > 2048).any()


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_many_large_case_worklist_length(n):
    a, b, _, _ = jc.many_large_case(n)
    big = jc.large_docs(a, b)
    assert int(big.sum()) == n and a.n_docs == 2 * n
    assert big[0::2].all() and not big[1::2].any()
    for shape in T_OF_SHAPE:
        assert jc.host_tiles(a, b, shape) == n  # one tile each: pass edges and run edges coincide at cap K_RUN
    assert jc.K_RUN == 1024


def test_k_run_matches_the_kernel():
    assert re.search(r"constexpr uint32_t kRun = (\d+);", (CSRC / "tile.hip").read_text()).group(1) == str(jc.K_RUN)


@pytest.mark.parametrize("G", [0, 1, 2, 256, 1792])
def test_slab_map_is_a_permutation_plus_padding(G):
    for C in sorted({1, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1, 7 * G + 3}):
        if C < 1:
            continue
        m = slab_map(C, G)
        grid = slab_grid(m)
        chunks = [slab_chunk(m, c) for c in range(grid)]
        real = [ch for ch in chunks if ch != PAD]
        assert sorted(real) == list(range(C)), (C, G)  # each chunk once
        assert len(chunks) - len(real) == grid - C
        if G == 0 or C <= G:
            assert chunks == list(range(C)), (C, G)  # identity
        else:
            S = m[1]
            assert S == -(-C // G) and grid == G * S and grid - C < G
            # one dispatch front starts S chunks apart (past C: padding), and each slab goes on in order
            assert [slab_chunk(m, c) for c in range(G)] == [g * S if g * S < C else PAD for g in range(G)]
            for c in range(G, grid):
                prev, ch = slab_chunk(m, c - G), slab_chunk(m, c)
                assert ch == PAD if prev == PAD or prev + 1 >= C else ch == prev + 1


def test_slab_map_restates_the_header():
    """The three functions above, line for line against crdt_device.hpp."""
    src = (CSRC / "crdt_device.hpp").read_text()
    for line in ("if (G == 0 || C <= G) return SlabMap{0u, 0u, C};",
                 "return SlabMap{G, (C + G - 1) / G, C};",
                 "return m.G ? m.G * m.S : m.C;",
                 "if (m.G == 0) return c;",
                 "const uint32_t ch = (c % m.G) * m.S + c / m.G;",
                 "return ch < m.C ? ch : 0xFFFFFFFFu;"):
        assert line in src, line


@pytest.mark.parametrize("v", [1, 2])
@pytest.mark.parametrize("K", [1, 2, 4, 8, 16])
def test_slab_case_engages_and_pads(K, v):
    n_cu = 256
    for extra, S_want in ((0, 0), (1, 2), (v * n_cu + 1, 3)):
        n_docs, C, G = jc.slab_geometry(K, v, n_cu, extra)
        assert G == v * n_cu and C == G + extra and n_docs % (jc.WAVES * K) == jc.WAVES * K - 1
        m = slab_map(C, G)
        if extra == 0:
            assert C == G and m == (0, 0, C)  # the C == G edge: in order
        else:
            assert C > G and m[1] == S_want and slab_grid(m) > C  # engaged, with padding blocks
        at = jc.slab_large_at(K, v, n_cu, extra)
        assert len(at) == 5 and 0 in at and n_docs - 1 in at
        if extra:
            S, per = m[1], jc.WAVES * K
            slabs = {d // per // S for d in at}
            assert 0 in slabs and (C - 1) // S in slabs


def test_slab_batches_are_what_the_geometry_says():
    """The smallest slab case built for real: the size, the promise kept or broken
    at exactly the five places, and the period of the repeated pool."""
    K, v, n_cu, extra = 1, 1, 256, 1
    n_docs = jc.slab_geometry(K, v, n_cu, extra)[0]
    a, b = jc.slab_batches(K, v, n_cu, extra)
    assert a.n_docs == b.n_docs == n_docs == 1027
    assert not jc.large_docs(a, b).any()
    assert a.doc(3) == a.doc(3 + jc.POOL) and b.doc(5) == b.doc(5 + jc.POOL)
    a, b = jc.slab_batches(K, v, n_cu, extra, large=True)
    assert a.n_docs == n_docs
    assert sorted(np.nonzero(jc.large_docs(a, b))[0].tolist()) == sorted(jc.slab_large_at(K, v, n_cu, extra))
    nd, ns = jc.live_sizes(a, b)
    for d, (x, y) in jc.slab_large_at(K, v, n_cu, extra).items():
        assert (nd[d], ns[d]) == (x, y)
