"""CPU: the worklist digest (crdt_awset_digest_idx_async; include/crdtgpu.h,
"worklist digests") restated in numpy, and the census of its case table.

digest_idx_ref is what the call writes into a digest array: for every listed
entry the two words of that document (GATHER: document idx[j] of the replica;
PLACE: document j of the sub-batch) at position idx[j], every other word as it
was.  Its hashes are a numpy restatement of the definition of their own, pinned
here to crdt_awset_digest_host of the full replica on the listed positions, in
both modes, over every case of tests/digest_idx_cases.py.  The census asserts
that every boundary the kernels have (csrc/digest_idx.hip) is reached by a named
case; the bounds are read from the kernel file, so a retuned bound moves the
cases with it.
"""

import numpy as np
import pytest

import crdtgpu
from digest_idx_cases import (BLOCK_ODD, K_GRID, K_GRID_WAVES, K_NT, K_PASS, K_STEP, K_WAVE, LADDER, MAIN_NAMES, MIXED_BIG,
                              N_MANY, N_MIXED, N_TURN, block_per, case, cases, listed, main_replica, place_sub)
from test_digest_model import K_A, K_E, K_N, K_T, K_V, known_batches

U32, U64 = np.uint32, np.uint64
M64 = 2 ** 64 - 1
GATHER, PLACE = 0, 1


# ------------------------------------------------------------------ the restatement

def _fmix(x):
    x = x.astype(U64).copy()
    x ^= x >> U64(30)
    x *= U64(0xBF58476D1CE4E5B9)
    x ^= x >> U64(27)
    x *= U64(0x94D049BB133111EB)
    x ^= x >> U64(31)
    return x


def _span(b, d):
    o, e = int(b.offsets[d]), int(b.offsets[d + 1])
    slots = max(e - o, 0)
    live = slots if b.counts is None else int(b.counts[d])
    return o, min(live, slots), live > slots


def doc_words(state, tombs, d):
    """((word 0, word 1), a count was clamped) of document d, all arithmetic mod 2^64."""
    with np.errstate(over="ignore"):
        o, n, over = _span(state, d)
        hk = _fmix(state.keys[o:o + n] + U64(K_E))
        dot = state.counters[o:o + n] + U64(K_A) * (state.actors[o:o + n].astype(U64) + U64(1))
        w0 = int(hk.sum(dtype=U64))
        w1 = int(_fmix(hk ^ dot).sum(dtype=U64))
        m = 0
        if tombs is not None:
            o, m, over_t = _span(tombs, d)
            over = over or over_t
            dot = tombs.counters[o:o + m] + U64(K_A) * (tombs.actors[o:o + m].astype(U64) + U64(1))
            w1 += int(_fmix(_fmix(tombs.keys[o:o + m] + U64(K_T)) ^ dot).sum(dtype=U64))
        R = state.R
        vv = np.asarray(state.vv[d * R:(d + 1) * R], U64)
        hv = _fmix(vv + U64(K_V) * (np.arange(R, dtype=U64) + U64(1)))
        w1 += int(hv[vv != 0].sum(dtype=U64))
        fin = _fmix(np.array([(w0 + K_N * n) & M64, (w1 + K_N * (n + m)) & M64], U64))
    return (int(fin[0]), int(fin[1])), over


class DigestIdxRef:
    """digest: the array after the call; capacity / invalid: what crdt_ctx_sync reports."""

    def __init__(self, digest, capacity, invalid):
        self.digest, self.capacity, self.invalid = digest, capacity, invalid


def digest_idx_ref(state, tombs, idx, n_idx, n_max, digest, mode):
    """state: the replica (GATHER) or the sub-batch (PLACE); digest: numpy u64 [n_digest_docs, 2]."""
    out = np.array(digest, U64).reshape(-1, 2).copy()
    n_digest = len(out)
    n = n_max if n_idx is None else min(int(n_idx), n_max)
    capacity = n_idx is not None and int(n_idx) > n_max
    invalid = False
    seen = {}  # (a list may name a document many times)
    for j in range(n):
        d = int(idx[j])
        if d >= n_digest or (mode == GATHER and d >= state.n_docs):
            invalid = True
            continue
        sd = j if mode == PLACE else d
        if sd not in seen:
            seen[sd] = doc_words(state, tombs, sd)
        words, over = seen[sd]
        capacity = capacity or over
        out[d] = words
    return DigestIdxRef(out, capacity, invalid)


def sentinel(n_docs):
    """A digest array whose every word is its own, recognisable value."""
    return (np.arange(2 * n_docs, dtype=U64) | U64(0xA5C3 << 48)).reshape(n_docs, 2)


_full = {}


def full_digest(c):
    """crdt_awset_digest_host of the case's whole replica (host code, independent of the kernels)."""
    if c.name not in _full:
        _full[c.name] = crdtgpu.digest_host(c.state, c.tombs)
    return _full[c.name]


def expected(c):
    """The array every run of the case must leave: digest_host on the listed documents, the sentinel elsewhere."""
    want = sentinel(c.state.n_docs)
    rows = listed(c).astype(np.int64)
    want[rows] = full_digest(c)[rows]
    return want


# ------------------------------------------------------------------ the restatement against digest_host

def test_restated_hashes_give_the_known_answers():
    for b, t, want in known_batches():
        assert doc_words(b, t, 0)[0] == (int(want[0, 0]), int(want[0, 1]))


@pytest.mark.parametrize("name", [c.name for c in cases()])
def test_gather_agrees_with_digest_host_on_the_listed_positions(name):
    c = case(name)
    ref = digest_idx_ref(c.state, c.tombs, c.idx, c.n_idx, c.n_max, sentinel(c.state.n_docs), GATHER)
    assert not ref.capacity and not ref.invalid
    assert (ref.digest == expected(c)).all()
    rows = np.zeros(c.state.n_docs, bool)
    rows[listed(c)] = True
    assert (ref.digest[~rows] == sentinel(c.state.n_docs)[~rows]).all()  # the untouched words
    if len(listed(c)) > 2:  # no listed word kept its sentinel by accident
        assert (ref.digest[rows] != sentinel(c.state.n_docs)[rows]).all()


@pytest.mark.parametrize("name", [c.name for c in cases() if not c.gather_only])
def test_place_over_the_reference_select_equals_gather(name):
    c = case(name)
    sub, sub_t = place_sub(c)
    assert sub.n_docs == c.n_max
    ref = digest_idx_ref(sub, sub_t, c.idx, c.n_idx, c.n_max, sentinel(c.state.n_docs), PLACE)
    assert not ref.capacity and not ref.invalid
    assert (ref.digest == expected(c)).all()
    # and the sub-batch digested whole is the listed rows of the replica's digest
    n = len(listed(c))
    assert (crdtgpu.digest_host(sub, sub_t)[:n] == full_digest(c)[listed(c).astype(np.int64)]).all()


def test_tombs_null_and_all_empty_digest_alike_and_layouts_agree():
    base = full_digest(case("list_ascending"))
    assert (full_digest(case("tombs_null")) == full_digest(case("tombs_all_empty"))).all()
    assert (full_digest(case("tombs_null"))[:, 0] == base[:, 0]).all()
    assert (full_digest(case("tombs_null"))[:, 1] != base[:, 1]).any()
    for name in ("layout_counts", "layout_slack_zeros", "layout_slack_cont", "layout_shifted_slack"):
        assert (full_digest(case(name)) == base).all(), name


def test_errors_of_the_restatement():
    c = case("list_ascending")
    n = c.state.n_docs
    r = digest_idx_ref(c.state, c.tombs, c.idx, n + 5, n, sentinel(n), GATHER)  # *n_idx above n_max: clamped
    assert r.capacity and not r.invalid and (r.digest == full_digest(c)).all()
    r = digest_idx_ref(c.state, c.tombs, np.array([2, n, 4], U32), 3, 3, sentinel(n), GATHER)
    assert r.invalid and not r.capacity
    want = sentinel(n)
    want[[2, 4]] = full_digest(c)[[2, 4]]
    assert (r.digest == want).all()


# ------------------------------------------------------------------ the census

def _doc(name):
    st, tb = main_replica()
    d = MAIN_NAMES.index(name)
    return d, int(st.offsets[d + 1] - st.offsets[d]), int(tb.offsets[d + 1] - tb.offsets[d])


def test_census_every_boundary_is_a_named_case():
    names = [c.name for c in cases()]
    assert len(set(names)) == len(names)
    st, tb = main_replica()
    ents = np.diff(st.offsets.astype(np.int64))
    tmbs = np.diff(tb.offsets.astype(np.int64))
    # live entry counts and tombstone counts: the ladder around one and two wave steps
    assert K_STEP == 128 and set(LADDER) == {0, 1, 2, 63, 64, 65, 127, 128, 129}
    assert set(LADDER) <= set(ents.tolist()) and set(LADDER) <= set(tmbs.tolist())
    # the wave bound from both sides, by entries alone and by the sum
    assert {K_WAVE - 1, K_WAVE, K_WAVE + 1} <= set(ents.tolist())
    assert sum(_doc("wave_with_tombs")[1:]) == K_WAVE
    d, e, t = _doc("under_but_sum_over")
    assert e < K_WAVE < e + t
    d, e, t = _doc("tombs_over")
    assert e <= K_WAVE < t
    # one block-path document: no multiple of the workgroup, at least three of its passes
    d, e, t = _doc("block_odd")
    assert e == BLOCK_ODD and e % K_NT and e > 2 * K_PASS and e > K_WAVE
    assert _doc("empty_zero_clock")[1:] == (0, 0)
    assert (full_digest(case("list_ascending"))[_doc("empty_zero_clock")[0]] == 0).all()
    # even and odd first slots of documents of two entries or more, entries and tombstones
    for b, sizes in ((st, ents), (tb, tmbs)):
        starts = b.offsets[:-1][sizes >= 2]
        assert (starts % 2 == 0).any() and (starts % 2 == 1).any()
    s3, _ = main_replica("slack_zeros")
    assert ((s3.offsets[:-1] % 2) != (st.offsets[:-1] % 2)).any()  # the slack moves documents to the other parity
    # layouts
    assert case("list_ascending").state.counts is None and case("layout_counts").state.counts is not None
    for name, what in (("layout_slack_zeros", "zeros"), ("layout_slack_cont", "cont")):
        s, t = case(name).state, case(name).tombs
        for b in (s, t):
            d = MAIN_NAMES.index("ladder65")
            o, n = int(b.offsets[d]), int(b.counts[d])
            assert int(b.offsets[d + 1]) - o > n
            assert (b.keys[o + n] == 0) == (what == "zeros")
            # read as live, the slack would change the digest (zeros too: hk(0) != 0 and the count)
        over = AWSetBatchWithCounts(s, +1)
        assert (crdtgpu.digest_host(over, t)[:9] != full_digest(case(name))[:9]).any()
    assert case("layout_shifted").shift and case("layout_shifted_slack").shift
    # tombstone combinations
    assert case("tombs_null").tombs is None
    assert int(case("tombs_all_empty").tombs.counts.sum()) == 0
    # clocks
    for R in (1, 2, 3, 5, 64):
        s = case("clock_R%d" % R).state
        assert s.R == R and not s.vv[:R].any() and s.vv[R:2 * R][0] and s.vv[R:2 * R][R - 1]
        assert R < 3 or not s.vv[R + 1:2 * R - 1].any()
    # values
    v, vt = case("values").state, case("values").tombs
    assert {0, 2 ** 63, M64} <= set(v.keys.tolist()) and {0, M64} <= set(vt.keys.tolist())
    assert {2 ** 32 - 1, 2 ** 32, 2 ** 63, M64} <= set(v.counters.tolist())
    assert {0, v.R - 1} == set(v.actors.tolist())
    # lists
    assert case("list_empty").n_idx == 0 and len(listed(case("list_empty"))) == 0
    n = st.n_docs
    assert listed(case("list_first")).tolist() == [0] and listed(case("list_last")).tolist() == [n - 1]
    assert listed(case("list_ascending")).tolist() == list(range(n))
    assert listed(case("list_descending")).tolist() == list(range(n))[::-1]
    assert listed(case("list_every_other")).tolist() == list(range(0, n, 2))
    rep = case("list_repeat")
    assert rep.gather_only and len(set(rep.idx.tolist())) < len(rep.idx)
    assert [c.name for c in cases() if c.gather_only] == ["list_repeat", "block_second_turn"]
    assert case("list_n_idx_null").n_idx is None
    assert case("list_prefix").n_idx < case("list_prefix").n_max
    many = case("many")
    assert len(listed(many)) == N_MANY > 2 * K_GRID_WAVES  # the grid-stride loop turns more than once
    assert (np.diff(many.state.offsets.astype(np.int64)) == 1).all()


def _big_docs(c):
    """Documents of the case's replica above the wave bound (the block kernel's)."""
    e = np.diff(c.state.offsets.astype(np.int64))
    t = np.diff(c.tombs.offsets.astype(np.int64)) if c.tombs is not None else 0
    return set(np.nonzero(e + t > K_WAVE)[0].tolist())


def _big_per_step(c):
    """{workgroup step: large documents listed in it}, by the launch's own formula (256 CUs)."""
    per = block_per(c.n_max)
    big = _big_docs(c)
    steps = {}
    for j, d in enumerate(listed(c).tolist()):
        if d in big:
            steps.setdefault(j // per, []).append(d)
    return per, steps


def test_census_of_the_block_kernels_steps():
    """The block kernel takes block_per(n_max) list entries per workgroup step, so what a
    workgroup sees depends on the list's length: one large document per step at most in
    the short lists, several in one step in block_shared_step, and a second step of the
    same workgroup with large documents in both in block_second_turn."""
    assert block_per(1) == 1 and block_per(K_GRID) == 1 and block_per(K_GRID + 1) == 2
    assert block_per(K_GRID * K_NT) == K_NT == block_per(2 ** 32 - 1)
    # the short lists: a workgroup of its own for every large document
    per, steps = _big_per_step(case("list_ascending"))
    assert per == 1 and len(steps) == 4 and all(len(v) == 1 for v in steps.values())
    per, steps = _big_per_step(case("many"))
    assert per > 1 and not steps  # no large document at all: every thread of the scan finds nothing
    # several large documents in one step: the LDS staging holds more than one entry and the
    # workgroup walks them one after the other over the same partial sums
    c = case("block_shared_step")
    assert _big_docs(c) == {d for d, _, _ in MIXED_BIG} and c.state.n_docs == N_MIXED
    per, steps = _big_per_step(c)
    assert 2 <= per < K_NT and sorted(len(v) for v in steps.values()) == [2, 3]
    assert -(-c.n_max // per) <= K_GRID  # (one step per workgroup here)
    # wave-bound documents of every kind among them: entries alone, the sum, tombstones alone
    kinds = {(e > K_WAVE, t > K_WAVE) for _, e, t in MIXED_BIG}
    assert kinds == {(True, False), (False, False), (False, True)}
    # a second step of the same workgroup, large documents in both, the staging reused
    c = case("block_second_turn")
    per, steps = _big_per_step(c)
    assert c.n_max == N_TURN and per == K_NT and -(-c.n_max // per) == K_GRID + 2
    assert len(steps[0]) >= 2 and len(steps[K_GRID]) >= 2  # steps 0 and K_GRID are both workgroup 0's (step % K_GRID)
    assert steps[0] != steps[K_GRID]
    assert N_TURN > K_GRID_WAVES  # (and the wave kernel's loop turns many times)


def AWSetBatchWithCounts(s, delta):
    """s with every live count moved by delta (the slack read as live)."""
    from crdtgpu.batch import AWSetBatch

    return AWSetBatch(s.R, s.offsets, s.keys, s.actors, s.counters, s.vv, counts=(s.counts + U32(delta)).astype(U32))
