"""CPU: delta extraction (crdt_awset_delta_extract_*), the send side of
anti-entropy -- its ABI surface, and a Python restatement of its rule over the
map oracle (oracle/awset_ref.py) that tests/test_gpu_delta_extract.py checks
the kernel against.

The rule (include/crdtgpu.h): per AWSetDelta source state and the clock P the
peer is known to have reached,
  tombstones out = Deleted minus the keys added again   awset-delta_test.go:93-102
  FULL   P.Counter(src.Actor) == 0: every entry                          :53
  DELTA  otherwise: entries whose dot P has not seen                  :84-92
  NONE   a DELTA with nothing to send                                    :60
The property that makes the message usable: for any P <= the receiver's clock
(elementwise), folding the messages into the receiver gives exactly what
folding the full states gives.
"""

import ctypes
import os
import random
import re

import crdtgpu
from crdtgpu import abi
from helpers import ref, ref_entries, ref_state

NONE, DELTA, FULL = 0, 1, 2


# ---------------------------------------------------------------- restatement

def extract_ref(src, P):
    """src = (actor, vv, entries [(k, a, c)] by key, tombstones [(k, a, c)] by key
    or None); P = the peer clock (list).  Returns (kind, entries out, tombstones
    out); raises ref.GoPanic where the reference would panic."""
    actor, _vv, ents, tombs = src
    Pv = ref.VersionVector(P)
    emap = {k: (a, c) for k, a, c in ents}
    tout = [(k, a, c) for k, a, c in (tombs or [])
            if not (k in emap and (emap[k][0] != a or emap[k][1] > c))]
    if Pv.Counter(actor) == 0:  # first contact: entry dots are not tested
        return FULL, list(ents), tout
    eout = [(k, a, c) for k, a, c in ents if not Pv.HasDot(ref.Dot(a, c))]
    return (DELTA if eout or tout else NONE), eout, tout


def extract_doc_ref(sources, P):
    """The message of one doc: its sources with the same actor and clock."""
    kinds, msg = [], []
    for s in sources:
        k, e, t = extract_ref(s, P)
        kinds.append(k)
        msg.append((s[0], s[1], e, t))
    return kinds, msg


def fold_ref(dst_entries, dst_vv, sources):
    """dst <- sources in order, each one (*AWSetDelta).Merge."""
    d = ref_state(dst_entries, dst_vv, cls=ref.AWSetDelta)
    for a, vv, e, t in sources:
        d.Merge(ref_state(e, vv, actor=a, cls=ref.AWSetDelta, deleted=t))
    return ref_entries(d), list(d.VersionVector)


# ---------------------------------------------------------------- generators

def pick_actor(rng, R, hi=None):
    """An actor in [0, hi] (default R + 1) that is not R (the reference's panic)."""
    hi = R + 1 if hi is None else hi
    while True:
        a = rng.randint(0, hi)
        if a != R:
            return a


def random_source(rng, R, ne, nt, universe, max_c, actor_hi=None):
    """An arbitrary AWSetDelta state.  Tombstone keys are drawn half from the
    entry keys, so that every re-add case occurs: same actor with a lower, an
    equal and a higher entry counter, a different actor, and an absent key."""
    keys = sorted(rng.sample(range(universe), ne))
    ents = [(k, pick_actor(rng, R, actor_hi), rng.randint(1, max_c)) for k in keys]
    n_in = min(ne, nt // 2 if nt > 1 else rng.randint(0, min(nt, 1)))
    tk = set(rng.sample(keys, n_in))
    free = [k for k in range(universe) if k not in tk]
    tk.update(rng.sample(free, min(nt - n_in, len(free))))
    emap = {k: (a, c) for k, a, c in ents}
    tombs = []
    for k in sorted(tk):
        if k in emap:
            a, c = emap[k]
            how = rng.randrange(4)
            if how == 0:
                tombs.append((k, a, c + rng.randint(1, 3)))  # same actor, the entry's counter lower: kept
            elif how == 1:
                tombs.append((k, a, max(1, c - rng.randint(1, 3))))  # higher (or equal at c == 1)
            elif how == 2:
                tombs.append((k, a, c))  # equal: kept
            else:
                b = pick_actor(rng, R, actor_hi)
                tombs.append((k, b, rng.randint(1, max_c)))  # (mostly) a different actor: dropped
        else:
            tombs.append((k, pick_actor(rng, R, actor_hi), rng.randint(1, max_c)))
    vv = [rng.randint(0, max_c) for _ in range(R)]
    return (pick_actor(rng, R, actor_hi), vv, ents, tombs)


def stale_clock(rng, vv):
    return [rng.randint(0, x) for x in vv]


# ---------------------------------------------------------------- tests

def _header_params():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "crdtgpu.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return {m.group(1): m.group(2).count(",") + 1
            for m in re.finditer(r"\b(crdt_\w+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)}


def test_abi_binds_delta_extract():
    sigs = abi.signatures()
    params = _header_params()
    lib = ctypes.CDLL(crdtgpu.LIB_PATH)
    for name, n in (("crdt_awset_delta_extract_async", 5), ("crdt_awset_delta_extract_batch", 4)):
        assert name in sigs, name
        assert len(sigs[name][1]) == n
        assert params.get(name) == n, (name, params.get(name))
        assert hasattr(lib, name), name
        assert name in crdtgpu.header_functions()
    assert ctypes.sizeof(abi.CDeltaOut) == 12 * 8
    assert (crdtgpu.CRDT_DELTA_NONE, crdtgpu.CRDT_DELTA_DELTA, crdtgpu.CRDT_DELTA_FULL) == (NONE, DELTA, FULL)
    assert crdtgpu.lib().crdt_abi_version() == 1  # an addition only
    assert hasattr(crdtgpu.Engine, "delta_extract_async") and hasattr(crdtgpu.Engine, "delta_extract")


def test_restatement_kinds():
    R = 2
    ents = [(1, 0, 1), (4, 1, 2), (9, 0, 5)]
    tombs = [(2, 0, 3), (4, 1, 1), (9, 0, 7)]  # absent key: kept; re-added (higher counter): dropped; older add: kept
    src = (0, [5, 2], ents, tombs)
    kept = [(2, 0, 3), (9, 0, 7)]
    assert extract_ref(src, [0, 9]) == (FULL, ents, kept)  # first contact: everything, the clock untested
    assert extract_ref(src, [3, 2]) == (DELTA, [(9, 0, 5)], kept)
    assert extract_ref(src, [5, 2]) == (DELTA, [], kept)  # tombstones alone make it a DELTA
    assert extract_ref((0, [5, 2], ents, None), [5, 2]) == (NONE, [], [])
    assert extract_ref((0, [5, 2], [], None), [0, 0]) == (FULL, [], [])  # FULL stays FULL when empty
    assert extract_ref((3, [5, 2], ents, None), [9, 9])[0] == FULL  # actor > R: never seen


def test_restatement_panics_where_the_reference_does():
    import pytest

    R = 2
    with pytest.raises(ref.GoPanic):
        extract_ref((R, [1, 1], [], None), [1, 1])  # Counter(src_actor == R)
    with pytest.raises(ref.GoPanic):
        extract_ref((0, [1, 1], [(3, R, 1)], None), [1, 1])  # HasDot on the DELTA path
    assert extract_ref((0, [1, 1], [(3, R, 1)], None), [0, 1])[0] == FULL  # FULL tests no entry dot
    assert extract_ref((0, [1, 1], [], [(3, R, 1)]), [1, 1]) == (DELTA, [], [(3, R, 1)])  # tombstone dots never are


def test_round_trip_equals_full_state_fold():
    """fold(dst, extract(srcs, P)) == fold(dst, srcs) for P == dst.vv and for
    stale P <= dst.vv, over arbitrary (unreachable) states."""
    rng = random.Random(20261019)
    n = 0
    seen = set()
    for R in (1, 2, 3, 5):
        for _ in range(800):
            universe = rng.choice([4, 8, 16])
            dst_e = [(k, pick_actor(rng, R), rng.randint(1, 6)) for k in sorted(
                rng.sample(range(universe), rng.randint(0, universe)))]
            dst_vv = [rng.choice([0, 0, rng.randint(1, 6)]) for _ in range(R)]
            sources = [random_source(rng, R, rng.randint(0, min(4, universe)), rng.randint(0, 3), universe, 6)
                       for _ in range(rng.randint(0, 4))]
            want = fold_ref(dst_e, dst_vv, sources)
            for P in (list(dst_vv), stale_clock(rng, dst_vv)):
                kinds, msg = extract_doc_ref(sources, P)
                seen.update(kinds)
                assert fold_ref(dst_e, dst_vv, msg) == want, (R, dst_e, dst_vv, sources, P)
                n += 1
    assert n == 6400 and seen == {NONE, DELTA, FULL}
