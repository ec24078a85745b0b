"""CPU: the case table of tests/apply_edge_cases.py is what it claims to be, and the C
oracle's batched local ops agree with the map-based replay on every case.

The census restates the quantities apply_kernel (csrc/apply.hip) computes for one
document -- nops, n_keyed, the runs of the keyed ops sorted by (key, op index), the
resolved keys m, removed / inserted entries, effective DELTA_DEL_KEYs, new and
overwritten tombstones -- with the kernel's own neighbour rules, not with the maps of
`replay`; the two are then checked against each other through the sizes of the result.
Each case's `claims` are asserted on its first document, and the table as a whole must
hit every value the kernel's layouts make an edge of.
"""

from itertools import groupby

import pytest

from apply_cases import doc_of
from apply_edge_cases import (ADD, BY_NAME, CASES, DDEL, DDK, DEL, DOC_COUNTS, LENGTHS, MAX_OPS, OP_COUNTS, R, TOP, batches,
                              expected, expected_doc)
from oracle import oracle


def census(d):
    ops = d.ops
    keyed = sorted((k, j) for j, (kind, k) in enumerate(ops) if kind != DDEL)
    state, tombs = [e[0] for e in d.ents], {t[0] for t in d.tombs}
    c = dict(nops=len(ops), n_keyed=len(keyed), ns=len(state), nt=len(tombs),
             bumps=sum(kind in (ADD, DDEL) for kind, _ in ops), m=0, max_run=0, removed=0, inserted=0, effective=0,
             ineffective=0, new_tombs=0, tomb_inserts=0, already_tombstoned=0, touches_first=False, touches_last=False)
    resolved = []
    for key, run in groupby(keyed, key=lambda x: x[0]):
        idx = [j for _, j in run]
        in_state = key in state
        eff = 0
        for pos, j in enumerate(idx):
            if ops[j][0] != DDK:
                continue
            # effective iff the key is present just before: its previous op is an ADD, or it is
            # the key's first op and the key is in the state
            present = in_state if pos == 0 else ops[idx[pos - 1]][0] == ADD
            eff += present
            c["ineffective"] += not present
        present_after = ops[idx[-1]][0] == ADD
        c["m"] += 1
        c["max_run"] = max(c["max_run"], len(idx))
        c["removed"] += in_state and not present_after
        c["inserted"] += present_after and not in_state
        c["effective"] += eff
        c["new_tombs"] += eff > 0
        c["tomb_inserts"] += eff > 0 and key not in tombs
        c["already_tombstoned"] += eff > 0 and key in tombs
        c["touches_first"] |= bool(state) and key == state[0]
        c["touches_last"] |= bool(state) and key == state[-1]
        resolved.append((key, in_state, present_after, eff > 0))
    ins = [k for k, s, p, _ in resolved if p and not s]
    if ins and state:
        c["where"] = ("below" if max(ins) < state[0] else "above" if min(ins) > state[-1] else
                      "between" if all(state[0] < k < state[-1] for k in ins) else "mixed")
    tk = sorted(tombs)
    tins = [k for k, _, _, t in resolved if t and k not in tombs]
    if len(tins) == 1 and tk:
        c["tomb_where"] = "before" if tins[0] < tk[0] else "after" if tins[0] > tk[-1] else "between"
    if ops and ops[0][0] == DDEL and (len(ops) == 1 or ops[1][0] != DDK):
        c["ddel_empty"] = "start"
    if ops and ops[-1][0] == DDEL and "ddel_empty" not in c:
        c["ddel_empty"] = "end"
    keys = [k for k, _ in keyed] + state + sorted(tombs)
    if keys:
        c["key_min"], c["key_max"] = min(keys), max(keys)
        c["spans_2_63"] = min(keys) < (1 << 63) <= max(keys)
        hi, lo = {k >> 32 for k in keys}, {k & 0xFFFFFFFF for k in keys}
        if min(keys) >= (1 << 32):
            c["differ"] = "high" if len(lo) == 1 and len(hi) > 1 else "low" if len(hi) == 1 and len(lo) > 1 else "both"
    return c


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_is_what_it_claims(case):
    want = expected(case)
    for d, w in zip(case.docs, want):
        c = census(d)
        assert c["nops"] <= MAX_OPS and d.actor < R
        assert [e[0] for e in d.ents] == sorted({e[0] for e in d.ents})
        assert [t[0] for t in d.tombs] == sorted({t[0] for t in d.tombs})
        # a well-formed list: every DELTA_DEL_KEY follows its call
        assert all(kind != DDK or (j and d.ops[j - 1][0] in (DDEL, DDK)) for j, (kind, _) in enumerate(d.ops))
        # the census and the replay agree on the sizes and on the clock
        assert len(w[0]) == c["ns"] - c["removed"] + c["inserted"]
        assert len(w[1]) == c["nt"] + c["tomb_inserts"]
        assert w[2][d.actor] == d.vv[d.actor] + c["bumps"]
    c = census(case.docs[0])
    c["n_docs"] = len(case.docs)
    for q, v in case.claims.items():
        assert c.get(q) == v, (case.name, q, c.get(q), v)
    if case.want is not None:
        assert want[0] == tuple(case.want[:2]) + (list(case.want[2]),), case.name
    if case.null_tombs:
        assert all(not d.tombs for d in case.docs)


def test_the_table_hits_every_edge():
    cs = [(case, census(d)) for case in CASES for d in case.docs]
    firsts = {case.name: census(case.docs[0]) for case in CASES}
    for n in OP_COUNTS:
        assert firsts["adds_%d" % n]["nops"] == n and firsts["adds_%d" % n]["m"] == n
        mixed = BY_NAME["mixed_%d" % n].docs[0]
        assert len(mixed.ops) == n
        if n >= 5:
            assert len({kind for kind, _ in mixed.ops}) == 4
    assert {c["n_keyed"] for _, c in cs} >= {0, 1, 255, 256}
    assert any(c["n_keyed"] == 256 and c["nops"] == 256 and c["bumps"] < 256 for _, c in cs)
    assert any(c["n_keyed"] == 0 and c["nops"] == 256 for _, c in cs)
    assert {c["m"] for _, c in cs} >= {0, 1, 255, 256}
    assert sum(c["max_run"] == 256 for _, c in cs) == 4
    for q in ("removed", "inserted"):
        assert any(c["m"] == 256 and c[q] == 256 for _, c in cs), q
    assert any(c["m"] == 256 and c["removed"] == 128 and c["inserted"] == 128 for _, c in cs)
    assert {c.get("where") for _, c in cs} >= {"below", "above", "between"}
    assert {c.get("tomb_where") for _, c in cs} >= {"before", "between", "after"}
    assert {c.get("ddel_empty") for _, c in cs} >= {"start", "end"}
    assert any(c["touches_first"] for _, c in cs) and any(c["touches_last"] for _, c in cs)
    for n in LENGTHS:
        assert any(c["ns"] == n and c["nops"] == 3 for _, c in cs), n
        assert any(c["nt"] == n and c["nops"] == 3 and c["tomb_inserts"] == 1 for _, c in cs), n
    assert any(c["already_tombstoned"] for _, c in cs)
    assert any(case.null_tombs and c["new_tombs"] for case, c in cs)
    assert any(c["effective"] >= 3 and c["bumps"] == 1 for _, c in cs)  # several keys of one call
    assert any(c["ineffective"] and c["effective"] for _, c in cs)
    assert any(c.get("key_min") == 0 and c.get("key_max") == TOP for _, c in cs)
    assert any(c.get("key_max") == TOP and c["max_run"] > 1 and c["n_keyed"] < 256 for _, c in cs)
    assert any(c.get("spans_2_63") for _, c in cs)
    assert {c.get("differ") for _, c in cs} >= {"high", "low"}
    assert any(case.slack == 3 and census(case.docs[0])["ns"] == 0 and census(case.docs[-1])["ns"] == 0 and
               len(case.docs) > 2 for case in CASES)
    assert {len(case.docs) for case in CASES} >= set(DOC_COUNTS)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_oracle_agrees_with_replay(case):
    st, tb, op = batches(case)
    rc, out, tout = oracle.apply(st, op, tb)
    assert rc == 0
    want = expected(case)
    nops = [len(d.ops) for d in case.docs]
    for d, w in enumerate(want):
        assert doc_of(out, tout, d, R) == w, (case.name, d)
        assert int(out.offsets[d]) == int(st.offsets[d]) + sum(nops[:d])
        assert int(tout.offsets[d]) == (int(tb.offsets[d]) if tb is not None else 0) + sum(nops[:d])
    assert int(out.offsets[-1]) == int(st.offsets[-1]) + sum(nops)


def test_expected_doc_is_the_replay_of_the_calls():
    """One case by hand, op by op, so that calls_of and replay cannot both be wrong the same way."""
    d = BY_NAME["add_ddk_add_ddk"].docs[0]
    e, t, vv = expected_doc(d)
    k = d.ops[0][1]
    assert [x for x in e if x[0] == k] == [] and t == [(k, 0, 11)] and vv == [11, 8, 9]
