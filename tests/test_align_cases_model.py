"""CPU: the case table of the alignment-selected kernel arms (tests/align_cases.py)
pinned without a GPU.

The conditions here are conditions on the inputs: the layouts hold what the
table says they hold, the pair census of every layout reaches the 16 B path and
the element path of the vector arm, every placed change of the compare side
occurs in both, the shift sets reach every selector value of every call, and
the pinned references (compare_ref, select_ref, scatter_ref, digest_ref,
digest_idx_ref) give what the table expects.  A table that drifts fails here,
not on the GPU.
"""

import collections
import itertools

import numpy as np
import pytest

import crdtgpu
from align_cases import (AT_WAVE, BIG, BITS, COLUMNS, COMPARE_LAYOUTS, DIGEST_NULL_TOMBS, DOTS, FILLER, GUARD, K_CHUNK,
                         KEYS, KINDS, LAYOUTS, M64, N_DOCS, OVER_WAVE, P32, P64, PLACES, SHIFTS, SIZES, SUB_DOCS, R,
                         cols, compare_case, compare_spans, digest_list, digest_spans, doc_sizes, gather_spans,
                         pair_census, scatter_idx, select_idx, selector, shift_id, state_batch, sub_batch, tomb_batch)
from crdtgpu.batch import AWSetBatch
from digest_idx_cases import K_WAVE
from test_compare_model import compare_ref, select_ref
from test_digest_idx_model import GATHER, PLACE, digest_idx_ref, sentinel
from test_digest_model import digest_ref
from test_replica_model import replica_select_ref
from test_scatter_model import scatter_ref

U32, U64 = np.uint32, np.uint64


def _live_of(b, d):
    o = int(b.offsets[d])
    n = int(b.offsets[d + 1]) - o if b.counts is None else int(b.counts[d])
    return b.keys[o:o + n], b.actors[o:o + n], b.counters[o:o + n]


# ------------------------------------------------------------------ the layouts

@pytest.mark.parametrize("slack", LAYOUTS)
def test_the_state_holds_what_the_table_says(slack):
    st = state_batch(slack)
    sizes = doc_sizes(slack)
    assert st.n_docs == N_DOCS == len(sizes) and st.R == R == 3 and GUARD == 64
    assert (st.counts is None) == (slack == 0)
    assert set(SIZES) <= set(sizes) and SIZES == (0, 1, 2, 3, 63, 64, 65)
    # the 2,050-entry document starts on the last slot of a chunk and spans three
    o = int(st.offsets[BIG])
    assert sizes[BIG] == K_CHUNK + 2 and o % K_CHUNK == K_CHUNK - 1
    assert (o + sizes[BIG] - 1) // K_CHUNK - o // K_CHUNK == 2
    assert 3000 < int(st.offsets[-1]) < 9000  # a few thousand entries
    starts = st.offsets[:-1].astype(np.int64)
    for n in SIZES:  # every size starts at an odd and at an even slot
        par = {int(starts[d]) % 2 for d in range(N_DOCS) if sizes[d] == n}
        assert par == {0, 1}, (n, par)
    assert (st.keys == 0).any() and (st.keys == M64).any()
    seen_high = seen_low = 0
    for d in range(N_DOCS):
        k, a, c = _live_of(st, d)
        assert len(k) == sizes[d]
        assert (np.diff(k.astype(object)) > 0).all()  # strictly ascending
        assert (a[1:] != a[:-1]).all() and (a < R).all()  # the two elements of any pair differ
        x = c[0:len(c) - len(c) % 2:2] ^ c[1::2]
        assert set(x.tolist()) <= {1, 1 << 32}
        seen_high += int((x == 1 << 32).sum())
        seen_low += int((x == 1).sum())
    assert seen_high > 100 and seen_low > 100
    assert (st.counters >= 1 << 63).sum() > 100 and (st.vv >= 1 << 63).sum() >= N_DOCS
    vv = st.vv.reshape(N_DOCS, R)
    assert ((vv[1:, 1] ^ vv[:-1, 1]) < 1 << 32).sum() == 0  # neighbouring documents: the high half only
    assert ((vv[:, 1] ^ vv[:, 2])[vv[:, 2] != 0] < 1 << 32).all() and (vv[:, 2] == 0).any()
    for arr in (st.keys, st.counters, st.vv):
        assert not (arr == P64).any()
    assert not (st.actors == P32).any()
    if slack:  # the stale entries differ between the sides
        other = state_batch(slack, 1)
        stale = np.ones(len(st.keys), bool)
        for d in range(N_DOCS):
            stale[int(st.offsets[d]):int(st.offsets[d]) + sizes[d]] = False
        assert stale.sum() == N_DOCS * slack
        assert (st.keys[stale] != other.keys[stale]).all() and (st.counters[stale] != other.counters[stale]).all()
        assert (st.actors[stale] != other.actors[stale]).all()
        assert (st.keys[~stale] == other.keys[~stale]).all()


@pytest.mark.parametrize("slack", LAYOUTS)
def test_tombstones_put_documents_on_both_sides_of_the_wave_bound(slack):
    st, tb = state_batch(slack), tomb_batch(slack)
    n = lambda d: int(st.offsets[d + 1] - st.offsets[d]) - slack  # noqa: E731
    m = lambda d: int(tb.offsets[d + 1] - tb.offsets[d]) - slack  # noqa: E731
    assert n(AT_WAVE) + m(AT_WAVE) == K_WAVE and n(OVER_WAVE) + m(OVER_WAVE) == K_WAVE + 1
    assert n(AT_WAVE) < K_WAVE and n(OVER_WAVE) < K_WAVE and n(BIG) > K_WAVE and m(BIG) > 0
    assert {AT_WAVE, OVER_WAVE, BIG} <= set(digest_list().tolist())
    assert len(set(range(N_DOCS)) - set(digest_list().tolist())) > 5  # documents whose words must stay
    assert not (tb.keys == P64).any() and not (tb.counters == P64).any() and not (tb.actors == P32).any()
    starts = {int(x) % 2 for x in tb.offsets[:-1]}
    assert starts == {0, 1}


# ------------------------------------------------------------------ the census

def test_compare_census_reaches_both_paths_in_every_layout():
    where = {(k, p): set() for k in KINDS for p in PLACES}
    for sa, sb in COMPARE_LAYOUTS:
        a, b, changes, _ = compare_case(sa, sb)
        spans, total = compare_spans(a, b)
        n_vec, n_elem, kind = pair_census(spans, total)
        assert n_vec > 0 and n_elem > 0, (sa, sb, n_vec, n_elem)
        combos = collections.Counter((c.kind, c.place, int(a.offsets[c.doc]) % 2) for c in changes if c.doc != BIG)
        for k, p in itertools.product(KINDS, PLACES):  # each change in an even-start and in an odd-start document
            assert combos[(k, p, 0)] >= 1 and combos[(k, p, 1)] >= 1, (sa, sb, k, p)
        for c in changes:
            pos = int(a.offsets[c.doc]) + c.entry
            assert kind[pos] in (1, 2)
            where[(c.kind, c.place)].add(int(kind[pos]))
            if c.place in ("pair_first", "pair_second"):  # an inner entry whose pair is its document's
                assert pos % 2 == (c.place == "pair_second") and 0 < c.entry < doc_sizes(sa)[c.doc] - 1
        assert len({c.doc for c in changes}) == len(changes)  # one change per changed document
        assert 0.4 < 1 - len(changes) / N_DOCS < 0.6  # about half are left identical
    for key, kinds in where.items():  # every placed change on the 16 B path and element by element
        assert kinds == {1, 2}, (key, kinds)


def _select_case(slack, which):
    st = state_batch(slack)
    idx = select_idx(which)
    n_out = N_DOCS if idx is None else len(idx)
    return st, idx, select_ref(st, idx, n_out=n_out)


@pytest.mark.parametrize("slack", LAYOUTS)
def test_gather_and_digest_census_reach_both_paths(slack):
    st = state_batch(slack)
    for which in ("identity", "permuted"):
        _, idx, want = _select_case(slack, which)
        src = [int(st.offsets[j if idx is None else int(idx[j])]) for j in range(want.n_docs)]
        n_vec, n_elem, _ = pair_census(*gather_spans(want, src))
        assert n_vec > 0 and n_elem > 0, (which, n_vec, n_elem)
        oo = {int(want.offsets[j]) % 2 for j in range(want.n_docs) if int(want.counts[j]) > 1}
        assert oo == {0, 1}  # documents land at odd and at even output offsets
    sub, idx = sub_batch(slack), scatter_idx()
    want = scatter_ref(st, sub, idx)
    where = {int(d): int(sub.offsets[j]) for j, d in enumerate(idx)}
    src = [where.get(d, int(st.offsets[d])) for d in range(N_DOCS)]
    n_vec, n_elem, _ = pair_census(*gather_spans(want, src))
    assert n_vec > 0 and n_elem > 0
    for b in (st, tomb_batch(slack)):
        spans, total = digest_spans(b)
        n_vec, n_elem, _ = pair_census(spans, total)
        assert n_vec > 0 and n_elem > 0


# ------------------------------------------------------------------ the selectors

@pytest.mark.parametrize("call", sorted(SHIFTS))
def test_every_selector_value_is_enumerated(call):
    reached = {selector(call, s) for s in SHIFTS[call]}
    assert reached == set(itertools.product((0, 1), repeat=BITS[call])), (call, reached)
    assert SHIFTS[call][0] == frozenset() and selector(call, frozenset()) == (1,) * BITS[call]
    assert len(set(SHIFTS[call])) == len(SHIFTS[call]) == len({shift_id(s) for s in SHIFTS[call]})


def test_compare_single_columns_and_the_sides_that_switch_vin():
    singles = [s for s in SHIFTS["compare"] if len(s) == 1]
    assert {next(iter(s)) for s in singles} == {"%s.%s" % (b, c) for b in "ab" for c in COLUMNS}
    assert all(selector("compare", s) == (0,) for s in singles)  # a conjunction of six
    for s in (cols("a"), cols("b"), cols("a", "b")):
        assert s in SHIFTS["compare"]
    # scatter: vin turned off once through the state and once through the sub-batch
    off = [s for s in SHIFTS["scatter"] if selector("scatter", s) == (0, 1)]
    assert cols("state") in off and cols("sub") in off
    assert selector("digest", DIGEST_NULL_TOMBS) == (0, 1) and DIGEST_NULL_TOMBS == cols("state")
    for which in ("identity", "permuted"):
        assert (select_idx(which) is None) == (which == "identity")
    idx = select_idx("permuted")
    assert set(idx.tolist()) == set(range(N_DOCS)) and len(idx) > N_DOCS  # a permutation, then repeats


# ------------------------------------------------------------------ the references

@pytest.mark.parametrize("sa,sb", COMPARE_LAYOUTS)
def test_compare_ref_gives_the_flag_written_beside_each_change(sa, sb):
    a, b, changes, flags = compare_case(sa, sb)
    got, summary, work = compare_ref(a, b)
    for c in changes:
        assert int(got[c.doc]) == c.flag == (KEYS if c.kind == "key" else DOTS), c
    assert (got == flags).all()
    assert work.tolist() == sorted(c.doc for c in changes)
    assert summary.tolist() == [sum(c.flag == KEYS for c in changes), sum(c.flag == DOTS for c in changes), 0, 0,
                                len(changes)]
    assert not compare_ref(a, state_batch(sb, 1, doc_sizes(sa)))[0].any()  # the stale slack alone: equal


@pytest.mark.parametrize("slack", LAYOUTS)
def test_select_and_scatter_refs_copy_the_documents_the_table_names(slack):
    st = state_batch(slack)
    for which in ("identity", "permuted"):
        _, idx, want = _select_case(slack, which)
        assert int(want.offsets[-1]) == int(want.counts.sum())
        for j in range(want.n_docs):
            assert want.doc(j) == st.doc(j if idx is None else int(idx[j])), (which, j)
    sub, idx = sub_batch(slack), scatter_idx()
    assert sorted(idx.tolist()) == sorted(SUB_DOCS) and BIG in SUB_DOCS and sub.n_docs == len(SUB_DOCS)
    want = scatter_ref(st, sub, idx)
    by = {int(d): j for j, d in enumerate(idx)}
    longer = shorter = 0
    for d in range(N_DOCS):
        assert want.doc(d) == (sub.doc(by[d]) if d in by else st.doc(d)), d
        if d in by:
            longer += len(sub.doc(by[d])[0]) > len(st.doc(d)[0])
            shorter += len(sub.doc(by[d])[0]) < len(st.doc(d)[0])
    assert longer > 2 and shorter > 2
    o = int(want.offsets[BIG])
    assert (o + int(want.counts[BIG]) - 1) // K_CHUNK > o // K_CHUNK  # still over a gather chunk boundary
    assert not (sub.keys == P64).any() and not (sub.counters == P64).any() and not (sub.vv == P64).any()


def test_digest_refs_agree_with_the_host_digest_and_across_layouts():
    per_layout = []
    for slack in LAYOUTS:
        st, tb = state_batch(slack), tomb_batch(slack)
        want = digest_ref(st, tb)
        assert (want == crdtgpu.digest_host(st, tb)).all()
        assert (digest_ref(st) == crdtgpu.digest_host(st)).all()
        assert not (want == P64).any() and len({tuple(r) for r in want.tolist()}) > N_DOCS - len(SIZES)
        idx = digest_list()
        got = digest_idx_ref(st, tb, idx, len(idx), len(idx), sentinel(N_DOCS), GATHER)
        rows = idx.astype(np.int64)
        rest = np.setdiff1d(np.arange(N_DOCS), rows)
        assert (got.digest[rows] == want[rows]).all() and (got.digest[rest] == sentinel(N_DOCS)[rest]).all()
        assert not got.capacity and not got.invalid
        sub = replica_select_ref(crdtgpu.batch.Replica(st, tb, 0, None), idx, n_idx=len(idx), n_out=len(idx)).rep
        placed = digest_idx_ref(sub.state, sub.tombs, idx, len(idx), len(idx), sentinel(N_DOCS), PLACE)
        assert (placed.digest == got.digest).all()
        per_layout.append(want)
    same = np.array([d != FILLER for d in range(N_DOCS)])  # (the filler's size is the layout's)
    assert (per_layout[0][same] == per_layout[1][same]).all()
    assert isinstance(state_batch(0), AWSetBatch)
