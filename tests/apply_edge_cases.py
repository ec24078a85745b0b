"""Deterministic apply cases that sit on every edge of apply_kernel (csrc/apply.hip).

The kernel indexes a document's ops in two lane layouts (lane + q * 64 for the loads,
lane * 4 + q for the scans), sorts the keyed ops in registers, resolves each key's run
with neighbour tests and two segmented scans, keeps three prefix tables with their
total in slot [m] and a sort sentinel in slot [n_keyed], and streams state and
tombstones 64 at a time.  Each Case below is a handful of documents built by hand to
put one of those quantities on a boundary; `claims` states the property in the terms
of the census of tests/test_apply_edges_model.py, which fails when a case drifts.

A document is (actor, entries, tombstones, clock, ops); ops are the (kind, key) pairs
the kernel sees.  Expected results come from `replay` of tests/apply_cases.py (the
map-based restatement of the reference) through `expected`; `want` is the result of
the first document stated by hand where the case is about one outcome.
"""

from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from apply_cases import STALE_KEY, replay, tomb_batch
from crdtgpu import CRDT_OP_ADD, CRDT_OP_DEL, CRDT_OP_DELTA_DEL, CRDT_OP_DELTA_DEL_KEY
from crdtgpu.batch import AWSetBatch, OpBatch

ADD, DEL, DDEL, DDK = CRDT_OP_ADD, CRDT_OP_DEL, CRDT_OP_DELTA_DEL, CRDT_OP_DELTA_DEL_KEY
U32, U64 = np.uint32, np.uint64
TOP = (1 << 64) - 1
MAX_OPS = 256
R = 3

OP_COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256)
LENGTHS = (0, 1, 63, 64, 65, 129)
DOC_COUNTS = (1, 2, 3)


class Doc(NamedTuple):
    actor: int
    ents: List[Tuple[int, int, int]]
    tombs: List[Tuple[int, int, int]]
    vv: List[int]
    ops: List[Tuple[int, int]]


class Case(NamedTuple):
    name: str
    docs: List[Doc]
    claims: Dict[str, object]          # census quantities of docs[0]
    want: Optional[tuple] = None       # (entries, tombstones, vv) of docs[0], stated by hand
    slack: int = 0                     # input slack of state and tombstones (with counts)
    null_tombs: bool = False           # the call passes tombs == NULL


def K(i):
    return 10 * (i + 1)


def scramble(n, mod=257, mul=37):
    """n distinct indices below mod, in no order."""
    return [(i * mul) % mod for i in range(n)]


def ents_of(keys, actor=1, c0=1):
    return [(k, (actor + i) % R, c0 + i % 5) for i, k in enumerate(sorted(keys))]


def doc(ops, ents=(), tombs=(), actor=0, vv=(7, 8, 9)):
    return Doc(actor, list(ents), list(tombs), list(vv), list(ops))


def calls_of(ops):
    """The call script of an op list, as replay takes it."""
    calls = []
    for kind, k in ops:
        if kind == ADD:
            calls.append(("add", [k]))
        elif kind == DEL:
            calls.append(("del", [k]))
        elif kind == DDEL:
            calls.append(("ddel", []))
        else:
            calls[-1][1].append(k)
    return calls


def mixed_ops(n, shift=0):
    """n ops in the fixed pattern ADD, DDEL, DDK, DDK, DEL, ADD, DEL over about n / 3 keys,
    so that most keys get several ops; any prefix of the pattern is a well-formed list."""
    kinds = (ADD, DDEL, DDK, DDK, DEL, ADD, DEL)
    u = n // 3 + 2
    return [(kinds[i % 7], 0 if kinds[i % 7] == DDEL else K((i * 5 + shift) % u)) for i in range(n)]


def mixed_doc(n, actor=0, shift=0):
    u = n // 3 + 2
    return doc(mixed_ops(n, shift), ents_of([K(i) for i in range(0, u, 2)]),
               ents_of([K(i) for i in range(1, u, 3)], actor=2, c0=2), actor=actor)


SMALL = doc([(ADD, 15), (DEL, 20), (DDEL, 0), (DDK, 30)], ents_of([20, 30, 40]), ents_of([5]), actor=1)


def op_count_cases():
    out = []
    for n in OP_COUNTS:
        keys = [3 * i + 1 for i in scramble(n)]
        state = ents_of([3 * i + 1 for i in range(0, 40, 4)] + [3 * i + 2 for i in range(5)])
        out.append(Case("adds_%d" % n, [doc([(ADD, k) for k in keys], state, ents_of([2]), actor=2), SMALL],
                        dict(nops=n, n_keyed=n, m=n, max_run=min(n, 1))))
        out.append(Case("mixed_%d" % n, [mixed_doc(n, actor=1), SMALL], dict(nops=n)))
    return out


def keyed_cases():
    ops = [((ADD, DEL)[(i // 100) % 2 ^ (i % 2)], K(i % 100)) for i in range(256)]
    return [
        Case("keyed_256_no_ddel", [doc(ops, ents_of([K(i) for i in range(0, 100, 3)])), SMALL],
             dict(nops=256, n_keyed=256, m=100)),
        Case("keyed_0_of_256", [doc([(DDEL, 0)] * 256, ents_of([K(1), K(2)]), ents_of([K(0)]), actor=1), SMALL],
             dict(nops=256, n_keyed=0, m=0, bumps=256),
             want=(ents_of([K(1), K(2)]), ents_of([K(0)]), [7, 8 + 256, 9])),
        Case("keyed_1", [doc([(DDEL, 0)] * 10 + [(ADD, K(3))] + [(DDEL, 0)] * 5, ents_of([K(1)])), SMALL],
             dict(nops=16, n_keyed=1, m=1, bumps=16, inserted=1),
             want=(sorted(ents_of([K(1)]) + [(K(3), 0, 7 + 11)]), [], [7 + 16, 8, 9])),
    ]


def one_run_cases():
    k = K(4)
    alt_add = [((DEL, ADD)[i % 2], k) for i in range(256)]  # ends in ADD
    alt_del = [((ADD, DEL)[i % 2], k) for i in range(256)]  # ends in DEL
    here = [(K(2), 1, 1), (k, 2, 2), (K(9), 0, 3)]
    away = [here[0], here[2]]
    return [
        Case("run256_ends_add_in_state", [doc(alt_add, here), SMALL], dict(n_keyed=256, m=1, max_run=256, removed=0, inserted=0),
             want=([(K(2), 1, 1), (k, 0, 7 + 128), (K(9), 0, 3)], [], [7 + 128, 8, 9])),
        Case("run256_ends_add_absent", [doc(alt_add, away), SMALL], dict(m=1, max_run=256, inserted=1)),
        Case("run256_ends_del_in_state", [doc(alt_del, here), SMALL], dict(m=1, max_run=256, removed=1),
             want=(away, [], [7 + 128, 8, 9])),
        Case("run256_ends_del_absent", [doc(alt_del, away), SMALL], dict(m=1, max_run=256, removed=0, inserted=0)),
        Case("ddk_twice_in_one_call", [doc([(ADD, k), (DDEL, 0), (DDK, k), (DDK, k)], away), SMALL],
             dict(m=1, max_run=3, effective=1, ineffective=1, new_tombs=1),
             want=(away, [(k, 0, 9)], [9, 8, 9])),
        Case("add_ddk_add_ddk", [doc([(ADD, k), (DDEL, 0), (DDK, k), (ADD, k), (DDEL, 0), (DDK, k)], away), SMALL],
             dict(m=1, max_run=4, effective=2, new_tombs=1),
             want=(away, [(k, 0, 11)], [11, 8, 9])),  # the later call's dot wins
        Case("ddk_effective_then_ineffective", [doc([(DDEL, 0), (DDK, k), (DDEL, 0), (DDK, k)], here), SMALL],
             dict(m=1, max_run=2, effective=1, ineffective=1, new_tombs=1, removed=1),
             want=(away, [(k, 0, 8)], [9, 8, 9])),  # the first call's dot stays
        Case("add_after_effective_ddk", [doc([(DDEL, 0), (DDK, k), (ADD, k)], here), SMALL],
             dict(m=1, max_run=2, effective=1, new_tombs=1, removed=0, inserted=0),
             want=([(K(2), 1, 1), (k, 0, 9), (K(9), 0, 3)], [(k, 0, 8)], [9, 8, 9])),  # present and newly tombstoned
    ]


def resolved_256_cases():
    idx = scramble(256, mod=256)  # a permutation of 0 .. 255
    state256 = ents_of([K(i) for i in range(256)])
    even, odd = [K(2 * i) for i in range(128)], [K(2 * i + 1) for i in range(128)]
    inter = [((DEL, even[i // 2]) if i % 2 == 0 else (ADD, odd[i // 2])) for i in range(256)]
    ten = ents_of([K(10 * (i + 1)) for i in range(10)])
    lo, hi = ten[0][0], ten[-1][0]
    return [
        Case("m256_inserts_into_empty", [doc([(ADD, K(i)) for i in idx], [], actor=1), SMALL],
             dict(n_keyed=256, m=256, inserted=256, removed=0, ns=0)),
        Case("m256_removals_of_256", [doc([(DEL, K(i)) for i in idx], state256), SMALL],
             dict(m=256, removed=256, inserted=0, ns=256), want=([], [], [7, 8, 9])),
        Case("m256_removals_interleaved_with_inserts", [doc(inter, ents_of(even)), SMALL],
             dict(m=256, removed=128, inserted=128, ns=128)),
        Case("m256_delta_removals_of_256", [doc([(DDEL, 0)] + [(DDK, K(i)) for i in idx[:255]], state256, actor=2), SMALL],
             dict(nops=256, n_keyed=255, m=255, removed=255, new_tombs=255, tomb_inserts=255)),
        Case("inserts_below_the_state", [doc([(ADD, k) for k in (3, 1, 7, 5, 9)], ten), SMALL], dict(inserted=5, where="below")),
        Case("inserts_above_the_state", [doc([(ADD, hi + k) for k in (3, 1, 7, 5, 9)], ten), SMALL],
             dict(inserted=5, where="above")),
        Case("inserts_between_the_state", [doc([(ADD, e[0] + 5) for e in reversed(ten[:-1])], ten), SMALL],
             dict(inserted=9, where="between")),
        Case("ops_on_first_and_last_state_key", [doc([(ADD, lo), (DEL, hi)], ten), doc([(DEL, lo), (ADD, hi)], ten), SMALL],
             dict(m=2, touches_first=True, touches_last=True, removed=1, inserted=0)),
    ]


def length_cases():
    out = []
    for n in LENGTHS:
        keys = [K(i) for i in range(n)]
        last = keys[-1] if n else K(0)
        script = [(ADD, K(n // 2) + 5), (DDEL, 0), (DDK, last)]
        out.append(Case("state_len_%d" % n, [doc(script, ents_of(keys), ents_of([K(0) + 1, K(1) + 1]), actor=1), SMALL],
                        dict(nops=3, ns=n, nt=2, inserted=1, new_tombs=min(n, 1))))
        four = ents_of([K(n // 2) + 5, K(n) + 105, K(n) + 115, K(n) + 125])
        script = [(ADD, 3), (DDEL, 0), (DDK, K(n // 2) + 5)]
        out.append(Case("tomb_len_%d" % n, [doc(script, four, ents_of(keys, actor=2), actor=2), SMALL],
                        dict(nops=3, ns=4, nt=n, new_tombs=1, tomb_inserts=1)))
    tombs = [(100, 1, 2), (200, 2, 3), (300, 0, 1)]
    state = ents_of([50, 150, 200, 350])
    ddk = lambda *ks: [(DDEL, 0)] + [(DDK, k) for k in ks]  # noqa: E731
    out += [
        Case("tomb_new_before", [doc(ddk(50), state, tombs), SMALL], dict(tomb_inserts=1, tomb_where="before")),
        Case("tomb_new_between", [doc(ddk(150), state, tombs), SMALL], dict(tomb_inserts=1, tomb_where="between")),
        Case("tomb_new_after", [doc(ddk(350), state, tombs), SMALL], dict(tomb_inserts=1, tomb_where="after")),
        Case("tomb_new_all_three", [doc(ddk(350, 50, 150), state, tombs), SMALL], dict(tomb_inserts=3, new_tombs=3)),
        Case("tomb_overwritten_in_place", [doc(ddk(200), state, tombs, actor=1), SMALL],
             dict(new_tombs=1, tomb_inserts=0, already_tombstoned=1),
             want=(ents_of([50, 150, 350])[:2] + [(350, 1, 4)], [(100, 1, 2), (200, 1, 9), (300, 0, 1)], [7, 9, 9])),
        Case("null_tombs_effective_ddk", [doc(ddk(150), state, []), doc(ddk(50, 350), state, [], actor=2)],
             dict(new_tombs=1, tomb_inserts=1, nt=0), null_tombs=True),
        Case("ddks_of_one_call_share_one_dot", [doc(ddk(350, 50, 999, 150), state, [], actor=2), SMALL],
             dict(effective=3, ineffective=1, new_tombs=3),
             want=([(200, 0, 3)], [(50, 2, 10), (150, 2, 10), (350, 2, 10)], [7, 8, 10])),
        Case("empty_ddel_at_the_start", [doc([(DDEL, 0), (ADD, 60)], state), SMALL], dict(nops=2, n_keyed=1, bumps=2, ddel_empty="start")),
        Case("empty_ddel_at_the_end", [doc([(ADD, 60), (DDEL, 0)], state), SMALL], dict(nops=2, n_keyed=1, bumps=2, ddel_empty="end")),
    ]
    return out


def key_width_cases():
    h = 1 << 63
    top_run = [(ADD, TOP), (DEL, TOP), (ADD, TOP), (DDEL, 0), (DDK, TOP), (ADD, TOP)]
    w = lambda hi, lo: (hi << 32) | lo  # noqa: E731
    return [
        Case("keys_0_and_top_in_state", [doc([(ADD, 0), (DEL, TOP), (ADD, 5)], ents_of([0, 9, TOP]), ents_of([0, TOP])),
                                         doc([(DDEL, 0), (DDK, TOP), (DDK, 0)], ents_of([0, 9, TOP]), ents_of([0, TOP]))],
             dict(m=3, removed=1, inserted=1, key_min=0, key_max=TOP)),
        Case("keys_0_and_top_inserted", [doc([(ADD, TOP), (ADD, 0)], ents_of([9])), SMALL],
             dict(m=2, inserted=2, key_min=0, key_max=TOP)),
        Case("run_on_top_absent", [doc(top_run, ents_of([9])), SMALL],
             dict(n_keyed=5, max_run=5, m=1, inserted=1, new_tombs=1, key_max=TOP),
             want=([(9, 1, 1), (TOP, 0, 11)], [(TOP, 0, 10)], [11, 8, 9])),
        Case("run_on_top_in_state", [doc(top_run[1:], ents_of([9, TOP]), [(TOP, 1, 1)]), SMALL],
             dict(n_keyed=4, max_run=4, m=1, new_tombs=1, already_tombstoned=1, key_max=TOP)),
        Case("keys_around_2_63", [doc([(ADD, h - 2), (ADD, h + 1), (DEL, h - 1), (DDEL, 0), (DDK, h)], ents_of([h - 1, h]),
                                      [(h - 1, 1, 1), (h + 5, 1, 1)]), SMALL],
             dict(m=4, removed=2, inserted=2, new_tombs=1, spans_2_63=True)),
        Case("keys_differing_in_the_high_word", [doc([(ADD, w(2, 5)), (DEL, w(1, 5)), (DDEL, 0), (DDK, w(3, 5))],
                                                     ents_of([w(1, 5), w(3, 5), w(4, 5)]), [(w(2, 5), 1, 1), (w(4, 5), 1, 1)]), SMALL],
             dict(differ="high", m=3)),
        Case("keys_differing_in_the_low_word", [doc([(ADD, w(7, 2)), (DEL, w(7, 1)), (DDEL, 0), (DDK, w(7, 3))],
                                                    ents_of([w(7, 1), w(7, 3), w(7, 4)]), [(w(7, 2), 1, 1), (w(7, 4), 1, 1)]), SMALL],
             dict(differ="low", m=3)),
    ]


def layout_cases():
    empty = doc([], [], [])
    body = [mixed_doc(20, actor=1), SMALL, mixed_doc(9, actor=2, shift=3)]
    out = [Case("slack_3_first_and_last_empty", [empty] + body + [empty], dict(nops=0, ns=0, nt=0), slack=3),
           Case("slack_3_every_boundary", [mixed_doc(n) for n in (63, 64, 65, 256)], dict(nops=63), slack=3)]
    for n in DOC_COUNTS:
        docs = [mixed_doc(20 + 7 * i, actor=i % R, shift=i) for i in range(n)]
        out.append(Case("n_docs_%d" % n, docs, dict(nops=20, n_docs=n)))
    return out


def all_cases() -> List[Case]:
    cases = (op_count_cases() + keyed_cases() + one_run_cases() + resolved_256_cases() + length_cases() +
             key_width_cases() + layout_cases())
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = all_cases()
BY_NAME = {c.name: c for c in CASES}


# ------------------------------------------------------------------ batches

def state_batch(docs, slack=0):
    st = AWSetBatch.from_docs(R, [(d.ents, d.vv) for d in docs], slack=slack)
    if slack:
        for d in range(st.n_docs):
            lo, hi = int(st.offsets[d]) + int(st.counts[d]), int(st.offsets[d + 1])
            st.keys[lo:hi], st.actors[lo:hi], st.counters[lo:hi] = STALE_KEY, 2, 99
    return st


def op_batch(docs):
    return OpBatch.from_lists([d.ops for d in docs], [d.actor for d in docs])


def batches(case: Case):
    """(state, tombstones or None, ops) of a case."""
    tb = None if case.null_tombs else tomb_batch([d.tombs for d in case.docs], case.slack)
    return state_batch(case.docs, case.slack), tb, op_batch(case.docs)


def expected_doc(d: Doc):
    return replay(d.actor, R, d.ents, d.tombs, d.vv, calls_of(d.ops))


def expected(case: Case):
    """Per document (entries, tombstones, vv) after its ops, from replay."""
    return [expected_doc(d) for d in case.docs]
