"""CPU: fold_log_ref (tests/fold_log_cases.py), the expectation the GPU test holds
crdt_awset_fold_log_async to, against an independent replay: every case document
goes through oracle/awset_ref.py's (*AWSet).Merge / (*AWSetDelta).Merge step by
step on maps, and the maps before and after are compared key by key.  Also here:
the upserted list's capacity bound (a document's upserts never outnumber its
sources' entries), and the census -- every named edge is reached by a named case,
and every case document lands on the path it is built for.
"""

import numpy as np
import pytest

import fold_edge_cases as fe
from fold_log_cases import (ADDED, AWSET, CLOCK, DELTA, NAMED_EDGES, REMOVED, UPDATED, all_cases, batches, doc_of,
                            fold_log_ref, path_of, replay)
from join_log_cases import doc_lists

CASES = sorted(all_cases())


def map_diff(before, vv0, after, vv1):
    """(removed, upserted, flags) from two (key, actor, counter) lists: the definition itself."""
    b = {k: (a, c) for k, a, c in before}
    f = {k: (a, c) for k, a, c in after}
    rem = [(k,) + b[k] for k in sorted(b) if k not in f]
    ups = [(k,) + f[k] + (UPDATED if k in b else ADDED,) for k in sorted(f) if k not in b or b[k] != f[k]]
    flags = (REMOVED if rem else 0) | (ADDED if any(u[3] == ADDED for u in ups) else 0)
    flags |= (UPDATED if any(u[3] == UPDATED for u in ups) else 0) | (CLOCK if list(vv0) != list(vv1) else 0)
    return rem, ups, flags


def check_batch(mode, dst, srcs, what):
    want = fold_log_ref(mode, dst, srcs)
    assert want.rc == 0, what
    n_upd = n_changed = n_any = 0
    for d in range(dst.n_docs):
        e, vv, chain = doc_of(dst, srcs, d)
        after, vv1, _ = replay(mode, e, vv, chain)
        rem, ups, flags = map_diff(e, vv, after, vv1)
        assert doc_lists(want.log, d) == (rem, ups), (what, d)
        assert int(want.log["flags"][d]) == flags, (what, d)
        # every upserted key takes its final dot from a source entry of the document
        assert len(ups) <= sum(len(s[2]) for s in chain), (what, d)
        held = {(k, a, c) for s in chain for k, a, c in s[2]}
        assert all(u[:3] in held for u in ups), (what, d)
        assert int(want.log["ups_offsets"][d]) == int(srcs.entry_off[int(srcs.doc_srcs[d])])
        n_upd += sum(u[3] == UPDATED for u in ups)
        n_changed += bool(flags & 7)
        n_any += bool(flags)
    lg = want.log
    assert lg["summary"].tolist() == [int(lg["rem_counts"].sum()), int(lg["ups_counts"].sum()), n_upd, n_changed, n_any]
    assert int(lg["ups_offsets"][-1]) == int(np.asarray(srcs.entry_off)[-1])
    return want


@pytest.mark.parametrize("name", CASES)
def test_reference_equals_the_step_by_step_replay(name):
    c = all_cases()[name]
    dst, srcs = batches(c)
    check_batch(c.mode, dst, srcs, name)
    for d, path in c.paths.items():
        assert path_of(c.mode, *c.docs[d]) == path, (name, d)


@pytest.mark.parametrize("name", sorted(fe.all_cases()))
def test_capacity_bound_on_the_fold_edge_cases(name):
    """fold_log_ref asserts both lists' bounds while it lays them out."""
    c = fe.all_cases()[name]
    for dst, srcs in c.batches[:1]:
        assert fold_log_ref(c.mode, dst, srcs).rc == 0


def test_census():
    cases = all_cases()
    reached = {e for c in cases.values() for e in c.edges}
    assert reached == set(NAMED_EDGES), sorted(set(NAMED_EDGES) ^ reached)
    paths = {(c.mode, p if isinstance(p, str) else "bail") for c in cases.values() for p in c.paths.values()}
    assert paths == {(m, p) for m in (AWSET, DELTA) for p in ("wave", "bail", "block")}
    steps = {p[1] for c in cases.values() for p in c.paths.values() if not isinstance(p, str)}
    assert {0, 1, 2} <= steps  # given up at the first, a middle and the last step
    # the width cases mix the paths without naming them: both are there at every R
    for name, c in cases.items():
        if name.startswith("width_"):
            got = {path_of(c.mode, *doc) for doc in c.docs}
            assert "wave" in got and "block" in got, name


def test_the_four_net_effects():
    cases = all_cases()

    def lists(name):
        c = cases[name]
        lg = fold_log_ref(c.mode, *batches(c)).log
        return doc_lists(lg, 0), int(lg["flags"][0])

    assert lists("readd_same_dot_delta") == (([], []), CLOCK)
    for m in ("awset", "delta"):
        assert lists("readd_other_dot_" + m) == (([], [(10, 1, 9, UPDATED)]), UPDATED | CLOCK)
        assert lists("add_then_remove_" + m) == (([], []), CLOCK)
        assert lists("update_then_remove_" + m) == (([(10, 0, 3)], []), REMOVED | CLOCK)
        assert lists("two_updates_" + m) == (([], [(10, 1, 8, UPDATED)]), UPDATED | CLOCK)
    assert lists("update_returns_awset") == (([], []), CLOCK)
    assert lists("tomb_removes_added_delta") == (([], []), CLOCK)
    assert lists("none_step_delta") == (([], []), 0)
    assert lists("first_contact_clock_only_delta") == (([], []), CLOCK)
    assert lists("first_contact_clock_clear_delta") == (([], []), 0)
