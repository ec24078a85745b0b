"""CPU: the reference of the logged local ops (crdt_awset_apply_log_async), pinned.

The expectation of tests/test_gpu_apply_log.py is ref_log: the C oracle's apply (as
oracle_docs of tests/test_gpu_apply_edges.py uses it), then diff_doc of
tests/test_diff_model.py per document; a refused document's log is empty.  Here, on every
case of tests/apply_edge_cases.py and tests/apply_log_cases.py:
  1. round trip: state - removed + upserted = the oracle's output;
  2. the lists are strictly ascending, disjoint and within their capacities (removed: the
     state's live entries; upserted: the document's ADD ops);
  3. the flags agree with compare_ref of tests/test_compare_model.py, and CLOCK is set iff
     the document has a bumping op;
  4. the records are what the map-based replay of the reference (Add / Del /
     AWSetDelta.Del on oracle/awset_ref.py) removes, adds and re-dots;
  5. the hand-stated lists of tests/apply_log_cases.py are the reference's;
and a census recomputes, from the document alone, every edge a case of the new table
claims, and asserts that each edge the issue names is claimed by some case.
"""

import numpy as np

import crdtgpu
from apply_edge_cases import ADD, CASES, DDEL, DDK, DEL, batches, expected_doc
from apply_log_cases import ADDED, CLOCK, EDGES, H, LOG_CASES, REMOVED, TOP, UPDATED
from oracle import oracle
from test_compare_model import A_AHEAD, B_AHEAD, DOTS, KEYS, compare_ref
from test_diff_model import diff_doc

ALL_CASES = list(CASES) + list(LOG_CASES)

# the reference of a call the library lacks pins nothing
assert "crdt_awset_apply_log_async" in crdtgpu.header_functions() and hasattr(crdtgpu.Engine, "apply_log_async")


def ref_log(st, tb, op, refused=(), with_tombs=True):
    """Per document (removed [(key, actor, counter)], upserted [(key, actor, counter, kind)],
    flags) of the call; `refused` documents (their op lists must be empty in `op`): empty."""
    rc, wo, _ = oracle.apply(st, op, tb, with_tombs=with_tombs)
    assert rc == 0
    after = wo.as_batch()
    out, R = [], st.R
    for d in range(st.n_docs):
        if d in refused:
            out.append(([], [], 0))
            continue
        (rk, ra, rc_), (uk, ua, uc), kind = diff_doc(st, after, d)
        rem = list(zip(rk.tolist(), ra.tolist(), rc_.tolist()))
        ups = list(zip(uk.tolist(), ua.tolist(), uc.tolist(), kind.tolist()))
        f = (REMOVED if rem else 0) | (ADDED if any(u[3] == ADDED for u in ups) else 0) | \
            (UPDATED if any(u[3] == UPDATED for u in ups) else 0)
        if (np.asarray(st.vv[d * R:(d + 1) * R]) != np.asarray(after.vv[d * R:(d + 1) * R])).any():
            f |= CLOCK
        out.append((rem, ups, f))
    return out, after


def summary_of(logs):
    """The five words of crdt_merge_log.summary for per-document (removed, upserted, flags)."""
    return [sum(len(r) for r, _, _ in logs), sum(len(u) for _, u, _ in logs),
            sum(1 for _, u, _ in logs for x in u if x[3] == UPDATED), sum(1 for _, _, f in logs if f & 7),
            sum(1 for _, _, f in logs if f)]


def test_round_trip_order_capacity_and_flags_on_both_tables():
    n = seen = 0
    for case in ALL_CASES:
        st, tb, op = batches(case)
        logs, after = ref_log(st, tb, op)
        cmp_flags = compare_ref(st, after)[0]
        for d, (x, (rem, ups, f)) in enumerate(zip(case.docs, logs)):
            m = {k: (a, c) for k, a, c in x.ents}
            for k, a, c in rem:
                assert m.pop(k) == (a, c), (case.name, d)  # removed with the dot the state held
            for k, a, c, kind in ups:
                assert (k in m) == (kind == UPDATED) and m.get(k) != (a, c), (case.name, d)
                m[k] = (a, c)
            assert sorted((k, a, c) for k, (a, c) in m.items()) == expected_doc(x)[0], (case.name, d)  # 1.
            rk, uk = [r[0] for r in rem], [u[0] for u in ups]
            assert all(p < q for p, q in zip(rk, rk[1:])) and all(p < q for p, q in zip(uk, uk[1:]))  # 2.
            assert not set(rk) & set(uk)
            assert len(rem) <= len(x.ents) and len(ups) <= sum(1 for kind, _ in x.ops if kind == ADD), (case.name, d)
            c = int(cmp_flags[d])  # 3.
            assert bool(c & KEYS) == bool(f & (REMOVED | ADDED)), (case.name, d)
            assert bool(c & DOTS) == (not f & (REMOVED | ADDED) and bool(f & UPDATED)), (case.name, d)
            assert bool(c & (A_AHEAD | B_AHEAD)) == bool(f & CLOCK), (case.name, d)
            assert bool(f & CLOCK) == any(kind in (ADD, DDEL) for kind, _ in x.ops), (case.name, d)
            seen |= f
            n += 1
    assert n > 200 and seen == 15


def test_records_are_what_the_map_replay_removes_adds_and_redots():
    for case in ALL_CASES:
        st, tb, op = batches(case)
        logs, _ = ref_log(st, tb, op)
        for d, (x, (rem, ups, _)) in enumerate(zip(case.docs, logs)):
            before = {k: (a, c) for k, a, c in x.ents}
            after = {k: (a, c) for k, a, c in expected_doc(x)[0]}
            assert rem == [(k, *before[k]) for k in sorted(before) if k not in after], (case.name, d)
            assert [u for u in ups if u[3] == ADDED] == [(k, *after[k], ADDED) for k in sorted(after) if k not in before]
            assert [u for u in ups if u[3] == UPDATED] == \
                [(k, *after[k], UPDATED) for k in sorted(after) if k in before and before[k] != after[k]], (case.name, d)


def test_hand_stated_lists_are_the_reference():
    for case in LOG_CASES:
        st, tb, op = batches(case)
        logs, _ = ref_log(st, tb, op)
        rem, ups, flags = case.want
        assert logs[0] == (list(rem), list(ups), flags), case.name


# ------------------------------------------------------------------ the census

def edges_of(x, slack=0):
    """The edges of tests/apply_log_cases.py (EDGES) document x sits on, from the document
    and the map replay alone."""
    before = {k: (a, c) for k, a, c in x.ents}
    ents, tombs, _ = expected_doc(x)
    after = {k: (a, c) for k, a, c in ents}
    names = set()
    live, history, calls = set(before), {}, []
    for kind, k in x.ops:
        if kind == DDEL:
            calls.append(0)
            continue
        past = history.setdefault(k, [])
        if kind == ADD:
            if k in before:
                names.add("add_of_live_key")
                if DEL in past:
                    names.add("del_then_add_of_live_key")
            live.add(k)
        else:
            hit = k in live
            if kind == DDK:
                names.add("effective_ddk" if hit else "ineffective_ddk")
                calls[-1] += hit
                if not hit and k not in before:
                    names.add("ineffective_ddk_of_absent_key")
            elif not hit and k not in before:
                names.add("del_of_absent_key")
            live.discard(k)
        past.append(kind)
    for k, past in history.items():
        if past[-1] != ADD and ADD in past and k not in after:
            names.add("add_then_del_of_live_key" if k in before else "add_then_del_of_absent_key")
        if past[-1] == ADD and before.get(k) == after[k]:
            names.add("add_mints_same_dot")
    if 0 in calls:
        names.add("ddel_call_no_live_key")
    if sorted(tombs) != sorted(x.tombs):
        names.add("tombstone_change_not_logged")
    if not x.ops:
        names.add("no_ops")
    elif all(kind == DEL and k not in before for kind, k in x.ops):
        names.add("only_dels_of_absent_keys")
    rem = [k for k in sorted(before) if k not in after]
    ups = [k for k in sorted(after) if before.get(k) != after[k]]
    if len(ups) == 256:
        names.add("ups_256")
    if len(rem) == 256 == len(before):
        names.add("rem_256_of_256")
    keys = sorted(before)
    for i in (0, 63, 64, 65, 128):
        if i < len(keys) and keys[i] in rem:
            names.add("rem_at_%d" % i)
    if keys and keys[-1] in rem:
        names.add("rem_at_last")
    if len(keys) in (65, 129):
        names.add("state_%d" % len(keys))
    if ups and ups[0] == min(after):
        names.add("ups_first")
    if ups and ups[-1] == max(after):
        names.add("ups_last")
    if len(after) == 1 and ups:
        names.add("ups_only")
    for k, name in ((0, "key_0"), (H, "key_2_63"), (TOP, "key_top")):
        if k in rem or k in ups:
            names.add(name)
    for k in ups:
        if k in before:
            (a0, c0), (a1, c1) = before[k], after[k]
            if a0 != a1 and c0 == c1:
                names.add("updated_actor_only")
            if a0 == a1 and c0 != c1:
                names.add("updated_counter_only")
    if slack:
        names.add("slack")
    return names


def test_census_every_named_edge_is_reached_by_a_named_case():
    claimed = set()
    for case in LOG_CASES:
        have = edges_of(case.docs[0], case.slack)
        assert set(case.edges) <= have, (case.name, sorted(set(case.edges) - have))
        claimed |= set(case.edges)
    assert claimed == set(EDGES), sorted(set(EDGES) ^ claimed)
    # the issue's own list, by the names above
    for name in ("add_of_live_key", "add_mints_same_dot", "add_then_del_of_absent_key", "tombstone_change_not_logged",
                 "del_then_add_of_live_key", "add_then_del_of_live_key", "effective_ddk", "ineffective_ddk",
                 "ddel_call_no_live_key", "no_ops", "only_dels_of_absent_keys", "ups_256", "rem_256_of_256", "rem_at_0",
                 "rem_at_63", "rem_at_64", "rem_at_65", "rem_at_128", "rem_at_last", "state_65", "state_129", "ups_first",
                 "ups_last", "ups_only", "key_0", "key_2_63", "key_top", "updated_actor_only", "updated_counter_only",
                 "slack"):
        assert name in claimed, name
