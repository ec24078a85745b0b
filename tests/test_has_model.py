"""CPU: (*AWSet).Has (awset.go:87) restated over the packed layout.

has_ref is the expectation of the GPU membership reads (tests/test_gpu_has.py,
crdt_awset_has_* / crdt_tomb_has_async): per document a dict of its LIVE slots
only -- the first counts[d] of them -- so whatever lies in the slack past the
live count can never be found.  Here it is pinned against the map-based
restatement of the reference (oracle/awset_ref.py: Has and Entries) on states
reached by random Add / Del / Merge histories and on every state recorded in
tests/golden/kat_scenarios.json.
"""

import json
import random

import numpy as np

from crdtgpu.batch import AWSetBatch
from helpers import GOLDEN, batch_of, ents, intern, pad, random_history, snap_entries

U8, U32, U64 = np.uint8, np.uint32, np.uint64


def has_ref(batch, per_doc_keys):
    """(found u8, actors u32, counters u64), one per query in query order, of a
    host batch with offsets / counts / keys / actors / counters (an AWSetBatch
    or a TombBatch): the entry's dot where the key is live, zeros elsewhere."""
    nq = sum(len(q) for q in per_doc_keys)
    found, actors, counters = np.zeros(nq, U8), np.zeros(nq, U32), np.zeros(nq, U64)
    off = np.asarray(batch.offsets).astype(np.int64)
    assert len(per_doc_keys) == len(off) - 1
    i = 0
    for d, qs in enumerate(per_doc_keys):
        if len(qs) == 0:
            continue
        o = int(off[d])
        n = int(batch.counts[d]) if batch.counts is not None else int(off[d + 1]) - o
        live = {int(k): j for j, k in enumerate(np.asarray(batch.keys[o:o + n]).tolist())}
        for k in qs:
            j = live.get(int(k))
            if j is not None:
                found[i], actors[i], counters[i] = 1, batch.actors[o + j], batch.counters[o + j]
            i += 1
    return found, actors, counters


def check_against_sets(states, universe_ids, slack, absent):
    """has_ref over the packed `states` equals Has / Entries of each map state."""
    R = max(len(s.VersionVector) for s in states)
    b = batch_of(R, [(ents(s.Entries, universe_ids), pad(s.VersionVector, R)) for s in states], slack=slack)
    if slack:  # stale keys past the live count: every id of the universe, so a wrong read would hit
        for d in range(b.n_docs):
            o, n = int(b.offsets[d]) + int(b.counts[d]), slack
            b.keys[o:o + n] = sorted(universe_ids.values())[:n] + [0] * max(0, n - len(universe_ids))
            b.actors[o:o + n] = 7
            b.counters[o:o + n] = 99
    names = sorted(universe_ids)
    queries = [[universe_ids[k] for k in names] + [absent] for _ in states]
    found, actors, counters = has_ref(b, queries)
    i = 0
    for s in states:
        for k in names:
            assert bool(found[i]) == s.Has(k), (k, s.Entries)
            if s.Has(k):
                assert (int(actors[i]), int(counters[i])) == (s.Entries[k].actor, s.Entries[k].counter)
            else:
                assert int(actors[i]) == 0 and int(counters[i]) == 0
            i += 1
        assert found[i] == 0 and actors[i] == 0 and counters[i] == 0  # the absent key
        i += 1
    assert i == len(found)
    return i


def test_has_ref_matches_reference_on_random_histories():
    n = 0
    for seed in range(40):
        rng = random.Random(1000 + seed)
        R = rng.choice([2, 3, 5])
        reps = random_history(rng, R, rng.randint(5, 80), rng.randint(3, 30), delta=bool(seed & 1))
        ids = intern(reps)
        ids.update({k: len(ids) + j for j, k in enumerate(["zz-never-added-1", "zz-never-added-2"])})
        n += check_against_sets(reps, ids, slack=seed % 3, absent=10 ** 12 + seed)
    assert n > 1000


def test_has_ref_on_every_golden_state():
    g = json.load(open(GOLDEN))
    n_states = 0
    for sc in g["scenarios"]:
        snaps = list(sc["final"].values())
        for m in sc["merges"]:
            snaps += [m["dst"], m["src"], m["out"]]
        universe = sorted({e[0] for s in snaps for e in s["entries"] + s.get("deleted", [])})
        ids = {k: i for i, k in enumerate(universe)}
        absent = len(ids) + 5
        for s in snaps:
            R = len(s["vv"])
            b = batch_of(R, [(snap_entries(s, ids), s["vv"])])
            found, actors, counters = has_ref(b, [[ids[k] for k in universe] + [absent]])
            live = {k: (a, c) for k, a, c in s["entries"]}
            for i, k in enumerate(universe):
                assert bool(found[i]) == (k in live), (sc["name"], k)
                assert (int(actors[i]), int(counters[i])) == live.get(k, (0, 0))
            assert found[-1] == 0 and actors[-1] == 0 and counters[-1] == 0
            n_states += 1
    assert n_states >= 23 * 3


def test_has_ref_never_reads_slack_and_keeps_query_order():
    b = AWSetBatch(2, np.array([0, 4, 4, 7], U32), np.array([5, 9, 0, 5, 0, 1, 2], U64),
                   np.array([1, 0, 3, 3, 1, 1, 1], U32), np.array([7, 8, 9, 9, 4, 5, 6], U64),
                   np.zeros(6, U64), counts=np.array([2, 0, 1], U32))
    # doc 0: live {5, 9}, slack holds 0 and a stale 5; doc 1: empty; doc 2: live {0}, slack 1, 2
    found, actors, counters = has_ref(b, [[9, 0, 5, 5, 2 ** 64 - 1], [], [1, 0, 2]])
    assert found.tolist() == [1, 0, 1, 1, 0, 0, 1, 0]
    assert actors.tolist() == [0, 0, 1, 1, 0, 0, 1, 0]
    assert counters.tolist() == [8, 0, 7, 7, 0, 0, 4, 0]
