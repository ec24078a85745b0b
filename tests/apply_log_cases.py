"""Deterministic cases for the log of crdt_awset_apply_log_async (csrc/apply_wave.hpp,
LOG = true): documents built by hand, no RNG, each on one edge of the log, with the
expected lists of the first document stated by hand.

A document is a Doc of tests/apply_edge_cases.py (actor, entries, tombstones, clock, ops);
the default clock is (7, 8, 9) and the default actor 0, so the k-th bumping op of a
document mints the dot (0, 7 + k).  `want` is (removed, upserted, flags) of docs[0]:
removed as (key, actor, counter) with the dot the state held, upserted as (key, actor,
counter, kind) with the new dot, both in key order.  `edges` names what the case is there
for; the census of tests/test_apply_log_model.py recomputes each name from the document
and fails when a case drifts off its edge.
"""

from __future__ import annotations

from typing import List, NamedTuple, Tuple

from apply_edge_cases import ADD, DDEL, DDK, DEL, SMALL, TOP, Doc, K, doc, ents_of

REMOVED, ADDED, UPDATED, CLOCK = 1, 2, 4, 8
H = 1 << 63


class LogCase(NamedTuple):
    name: str
    docs: List[Doc]
    want: Tuple[list, list, int]   # (removed, upserted, flags) of docs[0]
    edges: Tuple[str, ...]
    slack: int = 0                 # input slack of state and tombstones (with counts)
    null_tombs: bool = False       # (the field batches() of apply_edge_cases reads)


EDGES = (
    "add_of_live_key", "del_then_add_of_live_key", "add_mints_same_dot", "add_then_del_of_absent_key",
    "del_of_absent_key", "ineffective_ddk_of_absent_key", "tombstone_change_not_logged", "add_then_del_of_live_key",
    "effective_ddk", "ineffective_ddk", "ddel_call_no_live_key", "no_ops", "only_dels_of_absent_keys", "ups_256",
    "rem_256_of_256", "rem_at_0", "rem_at_63", "rem_at_64", "rem_at_65", "rem_at_128", "rem_at_last", "state_65",
    "state_129", "ups_first", "ups_last", "ups_only", "key_0", "key_2_63", "key_top", "updated_actor_only",
    "updated_counter_only", "slack",
)

S = ents_of([20, 30, 40])  # [(20, 1, 1), (30, 2, 2), (40, 0, 3)]


def _positions_case(n, at):
    """A state of n entries; DELs of the entries at positions `at`, in no order."""
    state = ents_of([K(i) for i in range(n)])
    ops = [(DEL, state[i][0]) for i in reversed(at)]
    return doc(ops, state), ([state[i] for i in at], [], REMOVED)


def all_cases() -> List[LogCase]:
    out = [
        # ---- the four rules
        LogCase("add_of_live_key", [doc([(ADD, 30)], S), SMALL], ([], [(30, 0, 8, UPDATED)], UPDATED | CLOCK),
                ("add_of_live_key",)),
        LogCase("del_then_add_of_live_key", [doc([(DEL, 30), (ADD, 30)], S), SMALL],
                ([], [(30, 0, 8, UPDATED)], UPDATED | CLOCK), ("del_then_add_of_live_key", "add_of_live_key")),
        LogCase("add_mints_same_dot_first_bump", [doc([(ADD, 30)], [(20, 1, 1), (30, 0, 8), (40, 0, 3)]), SMALL],
                ([], [], CLOCK), ("add_mints_same_dot",)),
        LogCase("add_mints_same_dot_third_bump",
                [doc([(ADD, 50), (DDEL, 0), (ADD, 30)], [(20, 1, 1), (30, 0, 10), (40, 0, 3)]), SMALL],
                ([], [(50, 0, 8, ADDED)], ADDED | CLOCK), ("add_mints_same_dot",)),
        LogCase("add_then_del_of_absent_key", [doc([(ADD, 50), (DEL, 50)], S), SMALL], ([], [], CLOCK),
                ("add_then_del_of_absent_key",)),
        LogCase("add_then_ddk_of_absent_key", [doc([(ADD, 50), (DDEL, 0), (DDK, 50)], S), SMALL], ([], [], CLOCK),
                ("add_then_del_of_absent_key", "effective_ddk", "tombstone_change_not_logged")),
        LogCase("del_and_ddk_of_absent_keys", [doc([(DEL, 50), (DDEL, 0), (DDK, 60)], S), SMALL], ([], [], CLOCK),
                ("del_of_absent_key", "ineffective_ddk_of_absent_key", "ineffective_ddk", "ddel_call_no_live_key")),
        LogCase("tombstone_change_not_logged", [doc([(DDEL, 0), (DDK, 30)], S, [(30, 1, 1)]), SMALL],
                ([(30, 2, 2)], [], REMOVED | CLOCK), ("tombstone_change_not_logged", "effective_ddk")),
        # ---- order of DEL and ADD on a live key
        LogCase("add_then_del_of_live_key", [doc([(ADD, 30), (DEL, 30)], S), SMALL], ([(30, 2, 2)], [], REMOVED | CLOCK),
                ("add_then_del_of_live_key",)),
        LogCase("add_then_ddk_of_live_key", [doc([(ADD, 30), (DDEL, 0), (DDK, 30)], S), SMALL],
                ([(30, 2, 2)], [], REMOVED | CLOCK), ("add_then_del_of_live_key", "effective_ddk")),
        # ---- DELTA_DEL calls
        LogCase("ddk_effective_and_ineffective", [doc([(DDEL, 0), (DDK, 30), (DDK, 55), (DDK, 30)], S), SMALL],
                ([(30, 2, 2)], [], REMOVED | CLOCK), ("effective_ddk", "ineffective_ddk")),
        LogCase("ddel_call_no_live_key", [doc([(DDEL, 0), (DDK, 25), (DDK, 35)], S), SMALL], ([], [], CLOCK),
                ("ddel_call_no_live_key", "ineffective_ddk_of_absent_key")),
        LogCase("empty_ddel_call", [doc([(DDEL, 0)], S), SMALL], ([], [], CLOCK), ("ddel_call_no_live_key",)),
        # ---- nothing changes
        LogCase("no_ops", [doc([], S), SMALL], ([], [], 0), ("no_ops",)),
        LogCase("only_dels_of_absent_keys", [doc([(DEL, 25), (DEL, 50), (DEL, 5), (DEL, 25)], S), SMALL], ([], [], 0),
                ("only_dels_of_absent_keys", "del_of_absent_key")),
    ]
    # ---- 256 records of either kind
    new = [K(i) + 5 for i in range(256)]
    order = [(i * 37) % 256 for i in range(256)]
    ctr = {new[i]: 8 + j for j, i in enumerate(order)}  # the j-th op mints (0, 7 + j + 1)
    out.append(LogCase("ups_256", [doc([(ADD, new[i]) for i in order], S), SMALL],
                       ([], [(k, 0, ctr[k], ADDED) for k in new], ADDED | CLOCK), ("ups_256",)))
    st256 = ents_of([K(i) for i in range(256)])
    out.append(LogCase("rem_256_of_256", [doc([(DEL, K(i)) for i in order], st256), SMALL], (list(st256), [], REMOVED),
                       ("rem_256_of_256", "rem_at_0", "rem_at_63", "rem_at_64", "rem_at_65", "rem_at_128", "rem_at_last")))
    # ---- the 64-wide stream loop
    d65, w65 = _positions_case(65, [0, 63, 64])
    out.append(LogCase("rem_positions_of_65", [d65, SMALL], w65, ("state_65", "rem_at_0", "rem_at_63", "rem_at_64",
                                                                   "rem_at_last")))
    d129, w129 = _positions_case(129, [0, 63, 64, 65, 128])
    out.append(LogCase("rem_positions_of_129", [d129, SMALL], w129, ("state_129", "rem_at_0", "rem_at_63", "rem_at_64",
                                                                      "rem_at_65", "rem_at_128", "rem_at_last")))
    out += [
        # ---- where the upserted key lands
        LogCase("ups_first", [doc([(ADD, 5)], S), SMALL], ([], [(5, 0, 8, ADDED)], ADDED | CLOCK), ("ups_first",)),
        LogCase("ups_last", [doc([(ADD, 45)], S), SMALL], ([], [(45, 0, 8, ADDED)], ADDED | CLOCK), ("ups_last",)),
        LogCase("ups_only", [doc([(ADD, 45)], []), SMALL], ([], [(45, 0, 8, ADDED)], ADDED | CLOCK),
                ("ups_only", "ups_first", "ups_last")),
        # ---- key width
        LogCase("keys_0_2_63_top_in_state",
                [doc([(ADD, 0), (DEL, H), (ADD, TOP)], [(0, 1, 1), (H, 2, 2), (TOP, 0, 3)], actor=1), SMALL],
                ([(H, 2, 2)], [(0, 1, 9, UPDATED), (TOP, 1, 10, UPDATED)], REMOVED | UPDATED | CLOCK),
                ("key_0", "key_2_63", "key_top", "add_of_live_key")),
        LogCase("keys_0_2_63_top_absent", [doc([(ADD, TOP), (ADD, H), (ADD, 0), (DEL, H - 1)], [(H - 1, 1, 1)], actor=2), SMALL],
                ([(H - 1, 1, 1)], [(0, 2, 12, ADDED), (H, 2, 11, ADDED), (TOP, 2, 10, ADDED)], REMOVED | ADDED | CLOCK),
                ("key_0", "key_2_63", "key_top", "ups_first", "ups_last")),
        # ---- UPDATED by one half of the dot
        LogCase("updated_actor_only", [doc([(ADD, 30)], [(20, 1, 1), (30, 1, 8), (40, 0, 3)]), SMALL],
                ([], [(30, 0, 8, UPDATED)], UPDATED | CLOCK), ("updated_actor_only", "add_of_live_key")),
        LogCase("updated_counter_only", [doc([(ADD, 30)], [(20, 1, 1), (30, 0, 3), (40, 0, 3)]), SMALL],
                ([], [(30, 0, 8, UPDATED)], UPDATED | CLOCK), ("updated_counter_only", "add_of_live_key")),
        # ---- slack behind state and tombstones
        LogCase("slack_3", [doc([(ADD, 30), (DEL, 20), (ADD, 25), (DDEL, 0), (DDK, 40)], S, ents_of([5])),
                            doc([], []), SMALL, doc([(DEL, 30)], S)],
                ([(20, 1, 1), (40, 0, 3)], [(25, 0, 9, ADDED), (30, 0, 8, UPDATED)], REMOVED | ADDED | UPDATED | CLOCK),
                ("slack", "effective_ddk"), slack=3),
    ]
    assert len({c.name for c in out}) == len(out)
    return out


LOG_CASES = all_cases()
LOG_BY_NAME = {c.name: c for c in LOG_CASES}
