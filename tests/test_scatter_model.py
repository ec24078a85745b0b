"""CPU: the scatter (crdt_awset_scatter_async) restated over the packed layout.

scatter_ref is the expectation of the GPU call (tests/test_gpu_scatter.py): a
numpy restatement of the contract in include/crdtgpu.h, built on _live and
select_ref of tests/test_compare_model.py.  It is pinned here by what makes it
select's inverse -- putting a selection back changes nothing -- and by the
round it closes: scattering the exchange of only the differing documents gives
the exchange of the whole batches (oracle/awset_ref.py), because a document
that compares equal is a fixed point of the merge.
"""

import os
import random
import re

import numpy as np

import crdtgpu
from crdtgpu import abi
from crdtgpu.batch import AWSetBatch
from helpers import PKG, batch_of, pad, ref_entries, ref_state
from test_compare_model import _live, compare_ref, golden_pairs, select_ref

U32, U64 = np.uint32, np.uint64
NONE = 0xFFFFFFFF


def inverse_map(n_docs, idx, n_idx):
    """inv[d] = the lowest j < n_idx with idx[j] == d, NONE when no j names d;
    an idx[j] that is no document is ignored."""
    inv = [NONE] * n_docs
    for j in range(n_idx):
        d = int(idx[j])
        if d < n_docs and j < inv[d]:
            inv[d] = j
    return inv


def scatter_ref(state, sub, idx, n_idx=None):
    """The packed batch scatter writes: doc d = sub doc j when idx[j] == d for
    some j < n_idx (the lowest such j), else state doc d; live entries only."""
    assert state.R == sub.R
    R = state.R
    n_idx = sub.n_docs if n_idx is None else min(int(n_idx), sub.n_docs)
    inv = inverse_map(state.n_docs, idx, n_idx)
    docs = []
    for d, j in enumerate(inv):
        src, s = (state, d) if j == NONE else (sub, j)
        k, a, c = _live(src, s)
        docs.append((list(zip(k, a, c)), [int(x) for x in src.vv[s * R:(s + 1) * R]]))
    return select_ref(batch_of(R, docs))


def one_entry_case(seed, n, m):
    """(state, sub, idx, expected) for n documents of 0 or 1 entries of which m are
    replaced, the first and the last among them; the expectation is computed with
    numpy alone, so n can be large (tests/test_gpu_scatter.py)."""
    rng = np.random.default_rng(seed)

    def make(n_docs, lo):
        cnt = rng.integers(0, 2, n_docs).astype(U32)
        off = np.zeros(n_docs + 1, U32)
        np.cumsum(cnt, out=off[1:])
        tot = int(off[-1])
        return AWSetBatch(1, off, np.arange(tot, dtype=U64) * U64(2) + U64(lo), np.zeros(tot, U32),
                          np.arange(tot, dtype=U64) + U64(1), np.arange(n_docs, dtype=U64) * U64(2) + U64(lo),
                          counts=cnt)

    state, sub = make(n, 0), make(m, 1)
    idx = np.concatenate([[n - 1, 0], rng.choice(np.arange(1, n - 1), m - 2, replace=False)]).astype(U32)
    rng.shuffle(idx)
    inv = np.full(n, -1, np.int64)
    inv[idx] = np.arange(m)
    rep = inv >= 0
    j = np.where(rep, inv, 0)
    cnt = np.where(rep, sub.counts[j], state.counts).astype(U32)
    off = np.zeros(n + 1, U32)
    np.cumsum(cnt, out=off[1:])
    live = cnt == 1
    src = np.where(rep, sub.offsets[:-1][j], state.offsets[:-1])[live]  # entry index of a one-entry document
    from_sub = rep[live]

    def pick(f):
        a, b = getattr(sub, f), getattr(state, f)
        return np.where(from_sub, a[np.minimum(src, len(a) - 1)], b[np.minimum(src, len(b) - 1)])

    want = AWSetBatch(1, off, pick("keys"), pick("actors"), pick("counters"), np.where(rep, sub.vv[j], state.vv),
                      counts=cnt)
    return state, sub, idx, want


def test_one_entry_case_is_scatter_ref():
    state, sub, idx, want = one_entry_case(8203, 3000, 500)
    assert {0, 2999} <= set(idx.tolist()) and len(set(idx.tolist())) == 500
    assert same_batch(scatter_ref(state, sub, idx), want)


def same_batch(x, y):
    """Two packed batches (select_ref / scatter_ref results) are bit-identical."""
    return (x.R == y.R and x.n_docs == y.n_docs and (x.offsets == y.offsets).all() and (x.counts == y.counts).all()
            and (x.keys == y.keys).all() and (x.actors == y.actors).all() and (x.counters == y.counters).all()
            and (x.vv == y.vv).all())


def _random_batch(rng, n, R, slack=0):
    docs = []
    for _ in range(n):
        k = sorted(rng.sample(range(40), rng.randint(0, 12)))
        docs.append(([(x, rng.randrange(R), rng.randint(1, 9)) for x in k], [rng.randint(0, 9) for _ in range(R)]))
    return batch_of(R, docs, slack=slack)


def _golden_batches():
    """Every state kat_scenarios.json records, one batch per scenario (with slack)."""
    return [batch_of(R, docs, slack=1) for R, docs, _ in golden_pairs()]


def _subset(rng, n):
    return np.array(rng.sample(range(n), rng.randint(0, n)), U32)


def test_scatter_of_a_selection_is_the_identity():
    rng = random.Random(8200)
    batches = [_random_batch(rng, 200, 3), _random_batch(rng, 200, 2, slack=2)] + _golden_batches()
    assert len(batches) > 2
    for S in batches:
        want = select_ref(S)
        for _ in range(3):
            idx = _subset(rng, S.n_docs)
            sub = select_ref(S, idx, n_out=len(idx))
            assert same_batch(scatter_ref(S, sub, idx), want)
        # the whole batch, reversed
        idx = np.arange(S.n_docs - 1, -1, -1, dtype=U32)
        assert same_batch(scatter_ref(S, select_ref(S, idx, n_out=len(idx)), idx), want)


def test_no_index_is_the_identity_select():
    rng = random.Random(8201)
    for S in [_random_batch(rng, 150, 3, slack=1)] + _golden_batches():
        other = _random_batch(rng, 20, S.R)
        idx = np.arange(20, dtype=U32) % max(S.n_docs, 1)
        assert same_batch(scatter_ref(S, other, idx, n_idx=0), select_ref(S))
        part = scatter_ref(S, other, idx, n_idx=1)  # and one index replaces exactly one document
        assert part.doc(int(idx[0])) == other.doc(0)
        for d in range(S.n_docs):
            if d != int(idx[0]):
                assert part.doc(d) == S.doc(d)


def test_replacements_move_every_later_offset():
    S = batch_of(2, [([(1, 0, 1), (2, 0, 2)], [2, 0]), ([], [0, 0]), ([(5, 1, 1)], [0, 1]), ([(7, 0, 3)], [3, 0])],
                 slack=1)
    sub = batch_of(2, [([(9, 1, 9)], [0, 9]), ([], [4, 4]), ([(1, 0, 1), (3, 1, 1), (4, 1, 2)], [1, 2]),
                       ([(8, 0, 8)], [8, 8])])
    idx = np.array([1, 0, 2, 1, 77], U32)  # empty -> longer, longer -> empty, a duplicate, no document
    out = scatter_ref(S, sub, idx)
    assert out.offsets.tolist() == [0, 0, 1, 4, 5] and out.counts.tolist() == [0, 1, 3, 1]
    assert out.doc(0) == ([], [4, 4]) and out.doc(1) == ([(9, 1, 9)], [0, 9])  # the lowest j wins
    assert out.doc(2) == sub.doc(2) and out.doc(3) == S.doc(3)
    assert out.doc(1) != sub.doc(3)
    # a count above its slots is clamped on either side
    S.counts[3] = 9
    assert scatter_ref(S, sub, idx).counts.tolist() == [0, 1, 3, 2]


def _exchange(a, b):
    """(a <- b, b <- a) per document by the map restatement of the reference's Merge."""
    R = a.R
    ab, ba = [], []
    for d in range(a.n_docs):
        x, y = ref_state(*a.doc(d)), ref_state(*b.doc(d))
        p, q = x.Clone(), y.Clone()
        p.Merge(y)
        q.Merge(x)
        ab.append((ref_entries(p), pad(p.VersionVector, R)))
        ba.append((ref_entries(q), pad(q.VersionVector, R)))
    return batch_of(R, ab), batch_of(R, ba)


def _check_sparse_round(a, b):
    flags, _, work = compare_ref(a, b)
    full_ab, full_ba = _exchange(a, b)
    sub_ab, sub_ba = _exchange(select_ref(a, work, n_out=len(work)), select_ref(b, work, n_out=len(work)))
    assert same_batch(scatter_ref(a, sub_ab, work), select_ref(full_ab))
    assert same_batch(scatter_ref(b, sub_ba, work), select_ref(full_ba))
    return len(work)


def test_scattering_the_exchange_of_the_differing_documents_is_the_full_exchange():
    rng = random.Random(8202)
    R, n = 3, 250
    a = _random_batch(rng, n, R, slack=1)
    docs = [a.doc(d) for d in range(n)]
    other = _random_batch(rng, n, R)
    for d in range(0, n, 4):  # a quarter of the documents differ
        docs[d] = other.doc(d)
    b = batch_of(R, docs, slack=2)
    n_work = _check_sparse_round(a, b)
    assert 40 < n_work < 70
    # every pair of states a golden scenario records
    n_pairs = n_diff = 0
    for R, docs, snaps in golden_pairs():
        pairs = [(i, j) for i in range(len(snaps)) for j in range(len(snaps))]
        ga = batch_of(R, [docs[i] for i, _ in pairs])
        gb = batch_of(R, [docs[j] for _, j in pairs], slack=1)
        n_diff += _check_sparse_round(ga, gb)
        n_pairs += len(pairs)
    assert n_pairs >= 23 * 23 and 0 < n_diff < n_pairs


def test_header_library_and_binding_have_the_entry_point():
    name = "crdt_awset_scatter_async"
    assert name in crdtgpu.header_functions()
    assert getattr(abi.lib(), name) is not None  # exported by libcrdtgpu.so
    text = re.sub(r"/\*.*?\*/", "", open(abi.HEADER_PATH).read(), flags=re.S)
    args = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    assert len(args.split(",")) == 8
    restype, argtypes = abi.signatures()[name]
    assert len(argtypes) == 8 and getattr(abi.lib(), name).argtypes is not None
    assert hasattr(crdtgpu.Engine, "scatter_async")


def test_kernel_chunk_constants_are_the_ones_the_gpu_tests_mirror():
    src = open(os.path.join(PKG, "csrc", "scatter.hip")).read()

    def const(name):
        expr = re.search(r"constexpr \w+ %s = ([^;]+);" % name, src).group(1)
        for _ in range(4):  # constants defined through earlier ones
            expr = re.sub(r"k\w+", lambda m: "(%s)" % re.search(r"constexpr \w+ %s = ([^;]+);" % m.group(0),
                                                                 src).group(1), expr)
        return eval(expr, {"__builtins__": {}})

    assert const("kSctScanChunk") == 1024 and const("kSctPartStep") == 1024
    assert const("kSctGatherChunk") == 2048 and const("kSctRun") == 1024
