"""CPU: the digest tree's definition (include/crdtgpu.h, "digest trees") restated
in numpy, independently of csrc/digest_hash.hpp, and held to crdt_digest_tree_host.

  - the layout and every node on n_docs = 0, 1, 2, 15, 16, 17, 255, 256, 257,
    4,096, 4,097, 65,537 and 2^20 + 1;
  - two literal roots, so the ABI cannot drift;
  - two swapped children change their node;
  - a descent from the root, restated with the leaf / non-leaf rules of
    crdt_digest_tree_diff_async, returns exactly the flat rule's worklist and
    flags (crdt_digest_diff_async) for masks 1, 2 and 3;
  - the bytes a descent fetches are a function of n and the differing set alone;
    the converged case is 256 B, and the table against the flat 16 * n_docs is
    printed.

The GPU tests (tests/test_gpu_digest_tree.py) use tree_ref, flat_ref and
descend_ref as their reference.
"""

import numpy as np
import pytest

import crdtgpu

U32, U64 = np.uint32, np.uint64
FANOUT = 16
K_P = U64(0x2545F4914F6CDD1D)
K_N = U64(0x85EBCA77C2B2AE63)
LAYOUTS = (0, 1, 2, 15, 16, 17, 255, 256, 257, 4096, 4097, 65537, (1 << 20) + 1)
ELEMENTS, STATE = 1, 2


def fmix(x):
    """splitmix64's finaliser on a u64 array (mod 2^64: numpy wraps)."""
    x = np.asarray(x, U64).copy()
    x ^= x >> U64(30)
    x *= U64(0xBF58476D1CE4E5B9)
    x ^= x >> U64(27)
    x *= U64(0x94D049BB133111EB)
    x ^= x >> U64(31)
    return x


def layout_ref(n_docs):
    """(L, nodes, off): nodes[l] for l = 0 .. L, off[l] the node offset of level l >= 1."""
    nodes, off = [n_docs], [0]
    if n_docs == 0:
        return 0, nodes, off
    o = 0
    while True:
        nodes.append(-(-nodes[-1] // FANOUT))
        off.append(o)
        o += nodes[-1]
        if nodes[-1] == 1:
            return len(nodes) - 1, nodes, off


def level_up(child):
    """Level l from level l - 1 ([n, 2] u64 each)."""
    n = len(child)
    m = -(-n // FANOUT)
    with np.errstate(over="ignore"):
        slot = (np.arange(n, dtype=U64) % U64(FANOUT) + U64(1)) * K_P
        term = np.zeros((m * FANOUT, 2), U64)
        term[:n] = fmix(child + slot[:, None])
        cnt = np.minimum(FANOUT, n - FANOUT * np.arange(m)).astype(U64)
        return fmix(term.reshape(m, FANOUT, 2).sum(axis=1, dtype=U64) + (K_N * cnt)[:, None])


def tree_ref(digest):
    """The tree of a digest array [n, 2]: levels 1 .. L concatenated, [n_nodes, 2] u64."""
    digest = np.asarray(digest, U64).reshape(-1, 2)
    levels, cur = [], digest
    while len(cur) and not (levels and len(cur) == 1):
        cur = level_up(cur)
        levels.append(cur)
    return np.concatenate(levels) if levels else np.zeros((0, 2), U64)


def levels_of(digest, tree):
    """[level 0, level 1, .. level L] as arrays."""
    L, nodes, off = layout_ref(len(digest))
    return [np.asarray(digest, U64).reshape(-1, 2)] + [tree[off[l]: off[l] + nodes[l]] for l in range(1, L + 1)]


def random_digest(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 64, size=(n, 2), dtype=U64)


def flat_ref(mine, theirs, mask):
    """crdt_digest_diff_async's rule: (worklist, its flags)."""
    e = mine[:, 0] != theirs[:, 0]
    s = mine[:, 1] != theirs[:, 1]
    flags = np.where(e, ELEMENTS, np.where(s, STATE, 0)).astype(np.uint8)
    work = np.nonzero(flags & mask)[0].astype(U32)
    return work, flags[work]


def children_ref(level, parents):
    """What crdt_digest_tree_children_async packs: [16 * len(parents), 2], zeros past the level."""
    out = np.zeros((FANOUT * len(parents), 2), U64)
    for j, p in enumerate(parents):
        c = level[FANOUT * int(p): FANOUT * int(p) + FANOUT]
        out[FANOUT * j: FANOUT * j + len(c)] = c
    return out


def diff_ref(mine_level, theirs_packed, parents, leaf, mask):
    """crdt_digest_tree_diff_async: (idx_out, flags_out, summary)."""
    idx, flags, n_e, n_s = [], [], 0, 0
    for j, p in enumerate(parents):
        for c in range(FANOUT):
            ch = FANOUT * int(p) + c
            if ch >= len(mine_level):
                break
            e = mine_level[ch, 0] != theirs_packed[FANOUT * j + c, 0]
            s = mine_level[ch, 1] != theirs_packed[FANOUT * j + c, 1]
            f = (ELEMENTS if e else STATE if s else 0) if leaf else int(e) | int(s) << 1
            n_e += int(e)
            n_s += int(s and not e) if leaf else int(s)
            if f & mask:
                idx.append(ch)
                flags.append(f)
    return np.array(idx, U32), np.array(flags, np.uint8), [n_e, n_s, 0, 0, len(idx)]


def descend_ref(mine_levels, their_levels, mask, start_level=None):
    """A whole descent: (worklist, flags, bytes fetched, parents asked per level)."""
    L = len(mine_levels) - 1
    if L == 0:
        return np.zeros(0, U32), np.zeros(0, np.uint8), 0, []
    lvl = L if start_level is None else start_level
    parents = np.arange(len(mine_levels[lvl]), dtype=U32)
    flags, fetched, asked = np.zeros(0, np.uint8), 0, []
    while lvl >= 1 and len(parents):
        packed = children_ref(their_levels[lvl - 1], parents)  # the peer's side
        fetched += 256 * len(parents)
        asked.append(len(parents))
        parents, flags, _ = diff_ref(mine_levels[lvl - 1], packed, parents, lvl == 1, mask)
        lvl -= 1
    if lvl >= 1:  # (nothing left to ask about)
        return np.zeros(0, U32), np.zeros(0, np.uint8), fetched, asked
    return parents, flags, fetched, asked


def differing(n, docs, seed, kind="both"):
    """(mine, theirs): two digest arrays that differ in `docs`; kind: which word, or per doc at random."""
    mine = random_digest(n, seed)
    theirs = mine.copy()
    rng = np.random.default_rng(seed + 1)
    for d in docs:
        k = kind if kind != "both" else ("e", "s", "es")[int(rng.integers(3))]
        if "e" in k:
            theirs[d, 0] ^= U64(1)
        if "s" in k:
            theirs[d, 1] ^= U64(1 << 63)
    return mine, theirs


def descend_of(mine, theirs, mask, start_level=None):
    return descend_ref(levels_of(mine, tree_ref(mine)), levels_of(theirs, tree_ref(theirs)), mask, start_level)


# ---------------------------------------------------------------------- tests

@pytest.mark.parametrize("n", LAYOUTS)
def test_layout_and_every_node_match_the_host_entry_point(n):
    L, nodes, off = crdtgpu.digest_tree_layout(n)
    rL, rnodes, roff = layout_ref(n)
    assert (L, nodes[: L + 1], off[: L + 1]) == (rL, rnodes, roff)
    assert nodes[L + 1:] == [0] * (8 - L) and off[L + 1:] == [0] * (8 - L) and L <= 8
    assert (n == 0) == (L == 0) and (L == 0 or nodes[L] == 1)
    digest = random_digest(n, 7 + n)
    got = crdtgpu.digest_tree_host(digest)
    want = tree_ref(digest)
    assert got.shape == want.shape == ((off[L] + 1 if L else 0), 2)
    assert (got == want).all()


def test_layout_of_the_largest_array_has_eight_levels():
    L, nodes, off = crdtgpu.digest_tree_layout(0xFFFFFFFF)
    assert L == 8 and nodes[1] == 1 << 28 and nodes[8] == 1 and off[8] == sum(nodes[1:8])


def test_pinned_roots():
    """Hand-stated arrays; the literals were taken once the numpy restatement and
    crdt_digest_tree_host agreed."""
    one = np.array([[1, 2]], U64)
    seventeen = np.array([[d + 1, 100 + d] for d in range(17)], U64)
    for digest, root in ((one, PIN_1), (seventeen, PIN_17)):
        host = crdtgpu.digest_tree_host(digest)
        ref = tree_ref(digest)
        assert (host == ref).all()
        assert [int(x) for x in host[-1]] == root, [hex(int(x)) for x in host[-1]]
    # n = 1 by hand: fmix(fmix(w + K_P) + K_N)
    with np.errstate(over="ignore"):
        assert [int(fmix(fmix(U64(w) + K_P) + K_N)) for w in (1, 2)] == PIN_1


PIN_1 = [0xC61A51FA0309C76E, 0xBAF0985337ECB79A]    # digest [[1, 2]]
PIN_17 = [0x41F823E31F5DC62B, 0xA469BEF27B93BE00]   # digest [[d + 1, 100 + d] for d < 17]


def test_swapping_two_children_changes_their_node():
    digest = random_digest(40, 3)
    base = crdtgpu.digest_tree_host(digest)
    sw = digest.copy()
    sw[[17, 30]] = sw[[30, 17]]  # both under level-1 node 1
    got = crdtgpu.digest_tree_host(sw)
    assert (got == tree_ref(sw)).all()
    assert (got[1] != base[1]).all() and (got[0] == base[0]).all() and (got[2] == base[2]).all()
    assert (got[3] != base[3]).all()  # the root


def test_words_stay_separate():
    digest = random_digest(300, 4)
    base = crdtgpu.digest_tree_host(digest)
    d = digest.copy()
    d[123, 1] ^= U64(5)
    got = crdtgpu.digest_tree_host(d)
    assert (got[:, 0] == base[:, 0]).all() and (got[:, 1] != base[:, 1]).sum() == 3  # one node a level


SINGLE = [(4097, d) for d in (0, 4096, 15, 16, 4095, 2048)] + [(17, 16), (1, 0), (16, 15), (257, 256)]


@pytest.mark.parametrize("mask", (1, 2, 3))
def test_descent_equals_the_flat_rule(mask):
    cases = [(n, [], "both") for n in (1, 17, 4097)]
    cases += [(n, [d], k) for n, d in SINGLE for k in ("e", "s", "es")]
    rng = np.random.default_rng(11)
    for n in (2, 255, 257, 4097, 65537):
        for share in (0.001, 0.05, 0.5):
            k = max(1, int(n * share))
            cases.append((n, sorted(rng.choice(n, size=min(k, n), replace=False).tolist()), "both"))
    for i, (n, docs, kind) in enumerate(cases):
        mine, theirs = differing(n, docs, 100 + i, kind)
        work, flags, fetched, asked = descend_of(mine, theirs, mask)
        fw, ff = flat_ref(mine, theirs, mask)
        assert (work == fw).all() and len(work) == len(fw), (n, docs[:8], kind)
        assert (flags == ff).all(), (n, docs[:8], kind)
        assert fetched == 256 * sum(asked) and asked[0] == 1


def test_word_1_only_difference_beside_a_word_0_difference_under_one_node():
    """The case the non-exclusive inner flags exist for: docs 32 and 33 share level-1
    node 2; 32 differs in word 0 only, 33 in word 1 only.  With mask 2 (STATE) the node
    must still be listed, though its word 0 differs."""
    n = 4097
    mine = random_digest(n, 21)
    theirs = mine.copy()
    theirs[32, 0] ^= U64(1)
    theirs[33, 1] ^= U64(1)
    for mask, want in ((1, [32]), (2, [33]), (3, [32, 33])):
        work, flags, _, _ = descend_of(mine, theirs, mask)
        assert work.tolist() == want
        assert flags.tolist() == [ELEMENTS if d == 32 else STATE for d in want]
    # an exclusive inner flag (ELEMENTS hides STATE, as at the leaves) would lose doc 33
    ml, tl = levels_of(mine, tree_ref(mine)), levels_of(theirs, tree_ref(theirs))
    e = ml[1][2, 0] != tl[1][2, 0]
    s = ml[1][2, 1] != tl[1][2, 1]
    assert e and s


def test_descent_may_start_at_any_level():
    mine, theirs = differing(4097, [5, 4000, 4096], 31)
    want = flat_ref(mine, theirs, 3)
    for start in (1, 2, 3, 4):
        work, flags, fetched, asked = descend_of(mine, theirs, 3, start)
        assert (work == want[0]).all() and (flags == want[1]).all()
        assert asked[0] == layout_ref(4097)[1][start]


def byte_cases(n, seed=5):
    rng = np.random.default_rng(seed)
    out = [("0", [])]
    for name, share in (("0.01 %", 1e-4), ("0.1 %", 1e-3), ("1 %", 1e-2), ("5 %", 5e-2)):
        k = max(1, int(round(n * share)))
        out.append((name + " random", sorted(rng.choice(n, size=k, replace=False).tolist())))
        start = int(rng.integers(0, n - k))
        out.append((name + " clustered", list(range(start, start + k))))
    return out


def test_bytes_fetched_are_a_function_of_n_and_the_differing_set():
    n = 1 << 16
    rows = []
    for name, docs in byte_cases(n):
        a = descend_of(*differing(n, docs, 1), 3)
        b = descend_of(*differing(n, docs, 2), 3)  # other digests, the same set
        assert a[2] == b[2] and a[3] == b[3] and (a[0] == b[0]).all()
        # level by level: the distinct ancestors of the differing docs
        want, cur = [], np.array(docs, np.int64)
        L = layout_ref(n)[0]
        for lvl in range(1, L + 1):
            cur = np.unique(cur // FANOUT)
            want.append(len(cur))
        if docs:
            assert a[3] == want[::-1], name
        else:
            assert a[3] == [1] and a[2] == 256  # converged: the root's children, nothing more
        rows.append((name, len(docs), a[2], 16 * n))
    print("\ndescent bytes at n_docs = %d (flat: %d B)" % (n, 16 * n))
    for name, k, got, flat in rows:
        print("  %-18s %6d docs  %9d B  %6.3fx flat%s" % (name, k, got, got / flat, "  LOSES" if got > flat else ""))


def test_converged_costs_256_bytes_at_every_layout():
    for n in LAYOUTS[1:-1]:
        mine = random_digest(n, n)
        work, flags, fetched, asked = descend_of(mine, mine.copy(), 3)
        assert len(work) == 0 and fetched == 256 and asked == [1]
