"""CPU: delta_log_ref (tests/delta_log_cases.py), the expectation
tests/test_gpu_delta_log.py compares the device against, pinned from several sides:
applying a direction's log to dst gives the oracle's output; the lists are
ascending, disjoint and fit the slots their layout gives them; flags agree with
compare_ref; NONE means an empty log, FULL the logged join's; the records are what
oracle/awset_ref.py's merge / deltaMerge remove, add and update on reachable
replicas; and the case sets hold every (path, direction, kind) and every feature.
"""

import random

import numpy as np
import pytest

from crdtgpu import CRDT_DELTA_DELTA, CRDT_DELTA_FULL, CRDT_DELTA_NONE
from delta_log_cases import (ALL_FEATURES, PAD, case_sets, census, delta_log_ref, feature_list, log_features)
from delta_pair_cases import KINDS, WAVE_MAX, _doc_lists, on_wave_path, replica_of_ref
from helpers import intern, out_doc, random_history
from join_log_cases import doc_lists, join_log_ref
from sources_cases import make_replica
from test_compare_model import A_AHEAD, B_AHEAD, DOTS, KEYS, _live, compare_ref
from test_diff_model import ADDED, CLOCK, REMOVED, UPDATED


@pytest.fixture(scope="module")
def sets():
    return {name: (a, b, delta_log_ref(a, b)) for name, (a, b) in case_sets().items()}


SET_NAMES = ("edges", "features", "random1", "random2", "random5", "random64")


def applied(dst, log, d):
    """dst[d]'s live entries with `removed` deleted and `upserted` assigned."""
    k, a, c = _live(dst, d)
    m = {kk: (aa, cc) for kk, aa, cc in zip(k, a, c)}
    rem, ups = doc_lists(log, d)
    for kk, aa, cc in rem:
        assert m.pop(kk) == (aa, cc)  # removed with the dot it had in dst
    for kk, aa, cc, kind in ups:
        assert kind in (ADDED, UPDATED) and (kk in m) == (kind == UPDATED)
        m[kk] = (aa, cc)
    return sorted((kk, aa, cc) for kk, (aa, cc) in m.items())


def directions(a, b, ref):
    return (("ab", a, b, ref.ab, ref.pair.kind_ab), ("ba", b, a, ref.ba, ref.pair.kind_ba))


def test_the_case_sets_are_the_named_ones(sets):
    assert set(sets) == set(SET_NAMES)


@pytest.mark.parametrize("name", SET_NAMES)
def test_round_trip_lists_layout_and_flags(sets, name):
    a, b, ref = sets[name]
    n, R = a.n_docs, a.state.R
    for what, dst, src, lr, kinds in directions(a, b, ref):
        assert lr.rc == 0
        after = lr.out.as_batch()
        log = lr.log
        assert (log["rem_offsets"] == np.asarray(dst.state.offsets, np.uint32)).all()
        assert (log["ups_offsets"] == np.asarray(src.state.offsets, np.uint32)).all()
        cf, _, _ = compare_ref(dst.state, after)
        n_upd = 0
        for d in range(n):
            assert applied(dst.state, log, d) == out_doc(lr.out, d, R)[0], (what, d)
            rem, ups = doc_lists(log, d)
            rk, uk = [x[0] for x in rem], [x[0] for x in ups]
            assert all(x < y for x, y in zip(rk, rk[1:])) and all(x < y for x, y in zip(uk, uk[1:])), (what, d)
            assert not set(rk) & set(uk), (what, d)
            assert len(rem) <= len(_live(dst.state, d)[0]) and len(ups) <= len(_live(src.state, d)[0]), (what, d)
            f = int(log["flags"][d])
            assert bool(f & 7) == bool(int(cf[d]) & (KEYS | DOTS)), (what, d)
            assert bool(f & CLOCK) == bool(int(cf[d]) & (A_AHEAD | B_AHEAD)), (what, d)
            assert not int(cf[d]) & A_AHEAD, (what, d)  # a merge never takes the clock back
            assert bool(f & REMOVED) == bool(rem), (what, d)
            assert bool(f & ADDED) == any(x[3] == ADDED for x in ups), (what, d)
            assert bool(f & UPDATED) == any(x[3] == UPDATED for x in ups), (what, d)
            n_upd += sum(x[3] == UPDATED for x in ups)
            if int(kinds[d]) == CRDT_DELTA_NONE:
                assert f == 0 and not rem and not ups, (what, d)
        fl = log["flags"]
        assert log["summary"].tolist() == [int(log["rem_counts"].sum()), int(log["ups_counts"].sum()), n_upd,
                                           int(((fl & 7) != 0).sum()), int((fl != 0).sum())]


@pytest.mark.parametrize("name", SET_NAMES)
def test_full_documents_carry_the_logged_joins_log(sets, name):
    a, b, ref = sets[name]
    seen = 0
    for what, dst, src, lr, kinds in directions(a, b, ref):
        jr = join_log_ref(dst.state, src.state)
        for d in np.nonzero(kinds == CRDT_DELTA_FULL)[0].tolist():
            assert doc_lists(lr.log, d) == doc_lists(jr.log, d), (what, d)
            assert int(lr.log["flags"][d]) == int(jr.log["flags"][d]), (what, d)
            seen += 1
    assert seen > 0 or name == "features"


def test_census_of_the_case_sets(sets):
    """Every (path, direction, kind) and every (path, feature) is in the sets the GPU file
    runs; the edges set alone holds them all."""
    want_kinds = {(p, x, k) for p in ("wave", "block") for x in ("ab", "ba") for k in KINDS}
    want_feats = {(p, f) for p in ("wave", "block") for f in ALL_FEATURES}
    kinds, feats = set(), set()
    for name in SET_NAMES:
        a, b, _ = sets[name]
        k, f = census(a, b)
        kinds |= k
        feats |= f
        if name == "edges":
            assert k == want_kinds and f >= want_feats, (want_kinds - k, want_feats - f)
        if name == "features":
            assert f >= want_feats, want_feats - f
    assert kinds == want_kinds and feats >= want_feats


def test_each_feature_document_shows_its_feature():
    R = 2
    for name, size, x, y in feature_list(R):
        a, b = make_replica(R, [x], actor=0), make_replica(R, [y], actor=1)
        assert on_wave_path(a, b, 0) == (size == "wave") and (size == "wave" or len(x[0]) > WAVE_MAX >= len(x[0]) - PAD)
        kind, f = log_features(x[0], x[2], y[2], R, 1, y[0], y[1])
        ref = delta_log_ref(a, b)
        rem, ups = doc_lists(ref.ab.log, 0)
        flags = int(ref.ab.log["flags"][0])
        if name == "phase2":
            assert {"p1_add_p2_remove", "tomb_readded", "tomb_absent_key"} <= f
            assert 40 not in [r[0] for r in rem] + [u[0] for u in ups]  # added, then removed: no record
            continue
        assert name in f, (name, size, f)
        if name == "p1_update_p2_remove":
            assert kind == CRDT_DELTA_DELTA and rem == [(40, 1, 2)] and ups == []  # dst's dot, no upsert
            assert flags == REMOVED | CLOCK
        elif name == "tomb_removes_dst_only":
            assert kind == CRDT_DELTA_DELTA and rem == [(50, 0, 1)] and ups == []
        elif name == "delta_keeps_covered_dst_only":
            assert kind == CRDT_DELTA_DELTA and rem == [] and ups == [(70, 1, 6, ADDED)]
            jr = join_log_ref(a.state, b.state)  # the full-state merge would remove it
            assert (60, 0, 3) in doc_lists(jr.log, 0)[0]
        elif name == "none_src_ahead":
            assert kind == CRDT_DELTA_NONE and flags == 0 and not rem and not ups
            assert out_doc(ref.pair.ab, 0, R)[1] == x[2] and any(s > v for s, v in zip(y[2], x[2]))
        elif name == "tomb_absent_key":
            assert kind == CRDT_DELTA_DELTA and not rem and not ups and flags == CLOCK


def test_reachable_histories_equal_the_python_reference():
    """Random histories of three AWSetDelta replicas (Add, AWSetDelta.Del, Merge); document
    d is history d.  The removed / added / updated records of each direction are what the
    reference's own Merge (merge or deltaMerge) removes, adds and updates on a clone."""
    rng = random.Random(8100)
    R = 3
    hist = [random_history(rng, R, rng.randint(4, 40), 12, delta=True) for _ in range(200)]
    seen, n_rem, n_add, n_upd = set(), 0, 0, 0
    for x, y in ((0, 1), (2, 0)):
        ids = intern([s for h in hist for s in h])
        a = replica_of_ref([h[x] for h in hist], ids, R, actor=x)
        b = replica_of_ref([h[y] for h in hist], ids, R, actor=y)
        ref = delta_log_ref(a, b)
        dot = lambda e: (e.actor, e.counter)  # noqa: E731
        for d, h in enumerate(hist):
            for lr, kinds, dst, src in ((ref.ab, ref.pair.kind_ab, h[x], h[y]), (ref.ba, ref.pair.kind_ba, h[y], h[x])):
                p = dst.Clone()
                p.Merge(src)
                rem = sorted((ids[k],) + dot(e) for k, e in dst.Entries.items() if k not in p.Entries)
                add = sorted((ids[k],) + dot(e) for k, e in p.Entries.items() if k not in dst.Entries)
                upd = sorted((ids[k],) + dot(e) for k, e in p.Entries.items()
                             if k in dst.Entries and dot(dst.Entries[k]) != dot(e))
                got_rem, got_ups = doc_lists(lr.log, d)
                assert got_rem == rem, d
                assert [u[:3] for u in got_ups if u[3] == ADDED] == add, d
                assert [u[:3] for u in got_ups if u[3] == UPDATED] == upd, d
                assert bool(int(lr.log["flags"][d]) & CLOCK) == (list(p.VersionVector) != list(dst.VersionVector)), d
                seen.add(int(kinds[d]))
                if int(kinds[d]) == CRDT_DELTA_DELTA:
                    n_rem, n_add, n_upd = n_rem + len(rem), n_add + len(add), n_upd + len(upd)
    assert seen == set(KINDS) and n_rem > 10 and n_add > 10, (seen, n_rem, n_add, n_upd)
