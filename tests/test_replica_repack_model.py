"""CPU: the replica repack with headroom (crdt_replica_repack_async) restated over
the capacity layout.

replica_repack_ref is the expectation of the GPU call
(tests/test_gpu_replica_repack.py): the packed result of replica_select_ref /
replica_scatter_ref (tests/test_replica_model.py) laid out at the prefix of the
capacities.  It is pinned here by those calls -- compacting it gives them back, and
with both policies NULL it IS them -- by the library's own crdt_headroom_capacity,
and by the rounds the layout exists for: replicas that spill when packed place
every document once repacked with the rounds' policy, against the C oracle.
"""

import ctypes
import os
import re

import numpy as np

import crdtgpu
from crdtgpu import abi
from crdtgpu.batch import AWSetBatch, Headroom, InplaceTarget, Replica, TombBatch, repack_slots
from delta_pair_cases import delta_pair_ref
from helpers import PKG
from oracle import oracle
from replica_repack_cases import (K_GATHER, K_PART, K_RUN, K_SCAN, ONES32, POLICIES, POLICY_SIZES, POLICY_TSIZES,
                                  ROUND_ROOM, big_case, cap_py, caps_py, cases)
from test_replica_inplace_model import replica_scatter_inplace_ref, same_packed
from test_replica_model import (apply_round_case, delta_round_case, out_replica, replica_scatter_ref,
                                replica_select_ref)

U32, U64 = np.uint32, np.uint64


# ------------------------------------------------------------------ reference

class RepackRef:
    """packed: the ReplicaRef of the same select / scatter with no slot limit; per kind
    ("e", "t") off[kind]: the u32 offsets (prefix of the capacities modulo 2^32), cnt[kind]
    the live counts, total[kind] the exact capacity total, limit[kind] the number of
    leading output positions the call may write; capacity / invalid: what
    crdt_ctx_sync reports."""

    def __init__(self, packed, off, cnt, total, limit, capacity, invalid):
        self.packed, self.off, self.cnt, self.total, self.limit = packed, off, cnt, total, limit
        self.capacity, self.invalid = capacity, invalid
        self.vv, self.doc_actor = packed.rep.state.vv, packed.rep.doc_actor

    def _cols(self, kind):
        return self.packed.rep.state if kind == "e" else self.packed.rep.tombs

    def moves(self, kind):
        """(dst, src): output positions written and the packed positions they copy."""
        cnt = self.cnt[kind].astype(np.int64)
        n_live = int(cnt.sum())
        ramp = np.arange(n_live, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        dst = np.repeat(self.off[kind][:-1].astype(np.int64), cnt) + ramp
        src = np.repeat(self._cols(kind).offsets[:-1].astype(np.int64), cnt) + ramp
        ok = dst < self.limit[kind]
        return dst[ok], src[ok]

    def columns(self, kind, length, fill=0):
        """(keys, actors, counters) of `length` slots: `fill` wherever the call does not write."""
        c = self._cols(kind)
        dst, src = self.moves(kind)
        out = []
        for f, dt in (("keys", U64), ("actors", U32), ("counters", U64)):
            a = np.full(max(length, 1), fill & (2 ** (8 * np.dtype(dt).itemsize) - 1), dt)
            a[dst] = np.asarray(getattr(c, f), dt)[src]
            out.append(a)
        return out

    @property
    def rep(self):
        """The capacity layout as a host Replica (zeros in the slack)."""
        te, tt = self.total["e"], self.total["t"]
        assert max(te, tt) <= ONES32 and self.limit["e"] == te and self.limit["t"] == tt
        k, a, n = self.columns("e", te)
        tk, ta, tn = self.columns("t", tt)
        R = self.packed.rep.state.R
        return Replica(AWSetBatch(R, self.off["e"], k, a, n, self.vv, counts=self.cnt["e"]),
                       TombBatch(self.off["t"], tk, ta, tn, counts=self.cnt["t"]), 0, self.doc_actor)


def replica_repack_ref(rep, sub=None, idx=None, n_idx=None, n_out=None, er=None, tr=None, entry_slots=None,
                       tomb_slots=None):
    """What crdt_replica_repack_async writes for host Replicas."""
    if sub is None:
        packed = replica_select_ref(rep, idx, n_idx, n_out)
    else:
        assert n_out is None or n_out == rep.n_docs
        packed = replica_scatter_ref(rep, sub, idx, n_idx)
    capacity = packed.capacity
    off, cnt, total, limit = {}, {}, {}, {}
    for kind, cols, room, slots in (("e", packed.rep.state, er, entry_slots), ("t", packed.rep.tombs, tr, tomb_slots)):
        c = np.asarray(cols.counts, U32)
        caps = caps_py(room, c)
        if room is not None and len(c):
            ms, num, shift, align = room
            capacity |= any(-(-(int(v) + max(ms, (int(v) * num) >> shift)) // align) * align > ONES32 for v in np.unique(c))
        o = [0]
        for x in caps.tolist():
            o.append(o[-1] + x)
        total[kind] = o[-1]
        off[kind] = np.array([x % 2 ** 32 for x in o], U64).astype(U32)
        cnt[kind] = c
        slots = total[kind] if slots is None else int(slots)
        capacity |= total[kind] > slots
        limit[kind] = min(int(off[kind][-1]), slots)
    return RepackRef(packed, off, cnt, total, limit, capacity, packed.invalid)


def ref_of(c):
    return replica_repack_ref(c.rep, c.sub, c.idx, c.n_idx, c.n_out, c.er, c.tr, c.entry_slots, c.tomb_slots)


_refs = {}


def case_ref(name):
    """The reference of a named case, computed once (shared with the GPU file)."""
    if name not in _refs:
        _refs[name] = ref_of(big_case() if name == "big" else cases()[name])
    return _refs[name]


def room_of(t):
    return None if t is None else Headroom(*t)


# ---------------------------------------------------------------------- tests

def test_library_capacity_is_the_restated_expression():
    lib = abi.lib()
    rooms = {r for c in cases().values() for r in (c.er, c.tr)} | {(0, ONES32, 0, 64), (ONES32, 0, 0, 1), (5, 7, 31, 4)}
    ns = [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 2 ** 20 + 1, 2 ** 31, ONES32 - 1, ONES32]
    for room in rooms:
        for n in ns:
            want = cap_py(room, n)
            if room is None:
                assert lib.crdt_headroom_capacity(None, n) == want == n
            else:
                h = abi.CHeadroom(*room)
                assert lib.crdt_headroom_capacity(ctypes.byref(h), n) == want, (room, n)
                assert Headroom(*room).capacity(n) == want
    assert cap_py((0, ONES32, 0, 1), 3) == ONES32 and cap_py((0, 1, 0, 1), 2 ** 20 + 1) == 2 ** 21 + 2
    assert Headroom().capacity(77) == 77
    assert repack_slots([1, 2, 2, 0], [0, 0, 1, 3], Headroom(1, 1, 0, 2), Headroom(1, 0, 0, 1)) == (2 + 4 + 4 + 2, 1 + 1 + 2 + 4)


def test_every_case_is_the_packed_result_at_the_capacity_offsets():
    for name in list(cases()) + ["big"]:
        c = big_case() if name == "big" else cases()[name]
        ref = case_ref(name)
        for kind, room in (("e", c.er), ("t", c.tr)):
            caps = caps_py(room, ref.cnt[kind])
            pre = np.zeros(len(caps) + 1, object)
            pre[1:] = np.cumsum(caps) if len(caps) else []
            assert (ref.off[kind].astype(object) == pre % 2 ** 32).all(), (name, kind)  # the prefix of the capacities
            assert ref.total[kind] == int(pre[-1])
            if c.entry_slots is None and name != "pol-saturate":
                o = ref.off[kind].astype(np.int64)
                assert (np.diff(o) >= ref.cnt[kind]).all() and (o[:-1] % (room[3] if room else 1) == 0).all(), name
        if name == "pol-saturate" or c.entry_slots is not None:
            continue
        packed = ref.packed
        again = replica_select_ref(ref.rep).rep
        assert same_packed(again, packed.rep) is None, name  # compacting it gives select / scatter back
        if c.er is None and c.tr is None:  # both NULL: the packed result word for word
            got = ref.rep
            for a, b in ((got.state, packed.rep.state), (got.tombs, packed.rep.tombs)):
                for f in ("offsets", "counts", "keys", "actors", "counters"):
                    x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
                    assert (x[: len(y)] == y).all() and len(x) == max(len(y), 1), (name, f)
            assert (got.state.vv == packed.rep.state.vv).all() and (got.doc_actor == packed.rep.doc_actor).all()
        assert (ref.capacity, ref.invalid) == (packed.capacity, packed.invalid), name


def test_reported_conditions():
    want = {"map-n_idx-above": (True, False), "map-bad-index": (False, True), "map-duplicate": (False, True),
            "map-empty-beyond": (False, False), "pol-saturate": (True, False), "cap-entries-short": (True, False),
            "cap-tombs-short": (True, False), "pol-big-doc": (False, False)}
    for name, (cap, inv) in want.items():
        ref = case_ref(name)
        assert (ref.capacity, ref.invalid) == (cap, inv), name
    for name, kind, other in (("cap-entries-short", "e", "t"), ("cap-tombs-short", "t", "e")):
        ref = case_ref(name)
        assert ref.limit[kind] == ref.total[kind] - 1 and ref.limit[other] == ref.total[other]
        dst, _ = ref.moves(kind)
        assert (dst < ref.limit[kind]).all()
    sat = case_ref("pol-saturate")
    assert sat.total["e"] == 4 * ONES32 and sat.off["e"].tolist() == [0, ONES32, ONES32 - 1, ONES32 - 2, ONES32 - 3]
    assert sat.moves("e")[0].tolist() == [0, 1, 2]  # document 0 alone lies below the slots


def test_census_every_edge_is_reached_by_a_named_case():
    cs = cases()
    # policy
    assert {0, 1, 63, 64, 65} <= set(POLICY_SIZES)
    rooms = [r for p in POLICIES.values() for r in p if r is not None]
    assert {0, 1, 7} <= {r[0] for r in rooms} and {1, 2, 8, 16, 64} <= {r[3] for r in rooms}
    assert any(r[1] == 0 for r in rooms) and {(1, 1), (3, 2)} <= {(r[1], r[2]) for r in rooms}
    for name in ("align8", "align16"):
        (ms, num, shift, align), _ = POLICIES[name]
        raw = [n + max(ms, (n * num) >> shift) for n in POLICY_SIZES]
        assert any(v % align == 0 for v in raw) and any(v % align == 1 for v in raw), name
    ms, num, shift, _ = POLICIES["min-above-and-below"][0]
    prop = [(n * num) >> shift for n in POLICY_SIZES]
    assert any(p < ms for p in prop) and any(p > ms for p in prop)
    assert all(e != t for e, t in list(POLICIES.values())[1:-1]) and POLICIES["both-null"] == (None, None)
    assert POLICIES["entry-null"][0] is None and POLICIES["tomb-null"][1] is None
    assert POLICY_TSIZES != POLICY_SIZES
    big = cs["pol-big-doc"]
    assert int(big.rep.state.counts.max()) == 2 ** 20 + 1 and big.er == (0, 1, 0, 1)
    assert cs["pol-saturate"].er == (0, ONES32, 0, 1) and set(cs["pol-saturate"].rep.state.counts.tolist()) == {3}
    # mapping: the forms of test_replica_model.py
    for R in (1, 3, 64):
        both, rn, sn, none = (cs["sct-R%d-tombs-%s" % (R, k)] for k in ("both", "rep-none", "sub-none", "none"))
        assert both.rep.state.R == R and both.rep.tombs is not None and both.sub.tombs is not None
        assert rn.rep.tombs is None and rn.sub.tombs is not None and sn.rep.tombs is not None and sn.sub.tombs is None
        assert none.rep.tombs is None and none.sub.tombs is None
        lay = [cs["sel-R%d-layout%d" % (R, p)] for p in range(4)]
        assert lay[0].rep.state.counts is None and lay[1].rep.tombs is None  # counts NULL; tombs NULL
        assert lay[1].rep.doc_actor is not None and lay[0].rep.doc_actor is None  # per document and uniform
        o, c = lay[3].rep.state.offsets.astype(np.int64), lay[3].rep.state.counts.astype(np.int64)
        d = int(np.nonzero(o[1:] - o[:-1] > c)[0][0])
        assert lay[3].rep.state.keys[o[d] + c[d]] != 0  # stale slack
        assert lay[2].n_idx == 0 and lay[1].n_idx < lay[1].n_out  # empty documents beyond *n_idx
    assert {c.er for c in cs.values() if c.sub is not None} >= {None, (2, 1, 0, 1)}
    c = cs["map-empty-beyond"]
    assert c.n_idx < c.n_out and cap_py(c.er, 0) > 0
    assert cs["map-n_idx-above"].n_idx > cs["map-n_idx-above"].n_out
    assert int(cs["map-bad-index"].idx[1]) >= cs["map-bad-index"].rep.n_docs
    assert cs["map-duplicate"].idx.tolist()[:2] == [7, 7]
    # scan
    assert {cs["sel-compact-%d" % n].n_out for n in (K_SCAN - 1, K_SCAN, K_SCAN + 1)} == {1023, 1024, 1025}
    assert {cs["sct-scan-%d" % n].n_out for n in (K_SCAN - 1, K_SCAN, K_SCAN + 1)} == {1023, 1024, 1025}
    assert cs["scan-2049"].n_out == 2049
    b = big_case()
    assert b.n_out == 2 ** 20 + 1 and (b.n_out + K_SCAN - 1) // K_SCAN == K_PART + 1
    assert int(np.asarray(b.rep.state.counts).max()) == 1 and cap_py(b.er, 0) == 0 and b.er[0] == 0
    # gather, from the case's capacity offsets
    ref = case_ref("gather-doubling")
    o, n = ref.off["e"].astype(np.int64), ref.cnt["e"].astype(np.int64)
    live_end = o[:-1] + n

    def where(p):  # (document, in its live prefix)
        d = int(np.searchsorted(o[1:], p, side="right"))
        return d, p < live_end[d]

    assert where(K_GATHER) == (0, False) and where(2 * K_GATHER) == (1, True)  # a boundary in slack; in a live prefix
    assert int(o[3]) == 3 * K_GATHER and int(o[4]) == 7 * K_GATHER  # boundaries exactly at document starts
    for chunk in (5, 6):  # chunks that lie wholly inside document 3's slack
        assert where(chunk * K_GATHER)[0] == 3 == where((chunk + 1) * K_GATHER - 1)[0] and chunk * K_GATHER >= live_end[3]
    assert np.bincount(np.minimum(o[:-1] // K_GATHER, o[-1] // K_GATHER)).max() > K_RUN  # the global search
    odd = case_ref("gather-odd-starts")
    oo, on = odd.off["e"].astype(np.int64)[:-1], odd.cnt["e"]
    assert cases()["gather-odd-starts"].er[3] == 1 and (oo[on >= 2] % 2 == 1).any() and (oo[on >= 2] % 2 == 0).any()
    for name, c in cs.items():  # align >= 2: every document starts on an even position
        for kind, room in (("e", c.er), ("t", c.tr)):
            if room is not None and room[3] >= 2 and name != "pol-saturate":
                assert (case_ref(name).off[kind][:-1] % room[3] == 0).all(), name
    # capacity
    assert cs["cap-entries-short"].entry_slots == case_ref("cap-entries-short").total["e"] - 1
    assert cs["cap-tombs-short"].tomb_slots == case_ref("cap-tombs-short").total["t"] - 1


def test_kernel_chunk_constants_are_the_ones_the_cases_mirror():
    src = open(os.path.join(PKG, "csrc", "replica_repack.hip")).read()

    def const(name):
        expr = re.search(r"constexpr \w+ %s = ([^;]+);" % name, src).group(1)
        for _ in range(4):  # constants defined through earlier ones
            expr = re.sub(r"k\w+", lambda m: "(%s)" % re.search(r"constexpr \w+ %s = ([^;]+);" % m.group(0),
                                                                 src).group(1), expr)
        return eval(expr, {"__builtins__": {}})

    assert const("kRpkScanChunk") == K_SCAN and const("kRpkPartStep") == K_PART
    assert const("kRpkGatherChunk") == K_GATHER and const("kRpkRun") == K_RUN
    # one definition of the capacity: the kernels and the host function read headroom.hpp
    api = open(os.path.join(PKG, "csrc", "api.cpp")).read()
    hdr = open(os.path.join(PKG, "csrc", "headroom.hpp")).read()
    assert "__host__ __device__ inline uint64_t headroom_cap64" in hdr
    assert "headroom_cap(" in src and "headroom_cap(" in api and ">> h.shift" not in src + api


# --- the rounds -----------------------------------------------------------------

_round = {}


def _packed_input(r):
    """A packed ReplicaRef.rep as the resident replica it is (uniform actor kept in doc_actor)."""
    return Replica(r.state, r.tombs, 0, r.doc_actor)


def delta_round_model():
    """delta_round_case's replicas PACKED (the state a fallback leaves), then repacked
    with ROUND_ROOM.  -> dict shared with the GPU file."""
    if "delta" not in _round:
        a0, b0, work, _, _ = delta_round_case()
        full = delta_pair_ref(a0, b0)
        assert full.rc_ab == 0 and full.rc_ba == 0
        want = tuple(replica_select_ref(out_replica(o, r, r)).rep for o, r in ((full.ab, a0), (full.ba, b0)))
        packed = tuple(_packed_input(replica_select_ref(r).rep) for r in (a0, b0))
        sa, sb = (replica_select_ref(r, work, n_out=len(work)).rep for r in packed)
        part = delta_pair_ref(sa, sb)
        assert part.rc_ab == 0 and part.rc_ba == 0
        subs = (out_replica(part.ab, packed[0], sa), out_replica(part.ba, packed[1], sb))
        roomy = tuple(replica_repack_ref(r, er=ROUND_ROOM, tr=ROUND_ROOM).rep for r in packed)
        _round["delta"] = dict(work=work, packed=packed, subs=subs, roomy=roomy, want=want,
                               on_packed=tuple(replica_scatter_inplace_ref(r, s, work) for r, s in zip(packed, subs)),
                               on_roomy=tuple(replica_scatter_inplace_ref(r, s, work) for r, s in zip(roomy, subs)))
    return _round["delta"]


def test_delta_round_spills_when_packed_and_fits_after_the_repack():
    m = delta_round_model()
    # (a) packed replicas: some work document spills on each side taken together
    assert sum(len(r.spill_j) for r in m["on_packed"]) >= 1 and len(m["on_packed"][0].spill_j) >= 1
    for ref, rep, w in zip(m["on_roomy"], m["roomy"], m["want"]):
        assert len(ref.spill_j) == 0 and len(ref.placed_j) == len(m["work"])  # (b)
        assert not ref.capacity and not ref.invalid
        assert same_packed(replica_select_ref(ref.rep).rep, w) is None  # (d) the full exchange, compacted
        InplaceTarget.of(rep)  # the repacked replica is a target as it stands
    # the repack moved nothing but the slots: compacted it is the packed replica
    for rep, p in zip(m["roomy"], m["packed"]):
        assert same_packed(replica_select_ref(rep).rep, replica_select_ref(p).rep) is None


def apply_round_model():
    """apply_round_case's replica packed; round 1 spills and falls back through the
    repack's scatter mapping with ROUND_ROOM; round 2 runs the same ops on the same
    documents again and places everything."""
    if "apply" not in _round:
        rep0, idx, part, full = apply_round_case()
        packed = _packed_input(replica_select_ref(rep0).rep)

        def apply(rep, ops):
            rc, out, tout = oracle.apply(rep.state, ops, rep.tombs)
            assert rc == 0
            return Replica(out.as_batch(), tout, 0, rep.doc_actor)

        def sparse(rep):
            sel = replica_select_ref(rep, idx, n_out=len(idx)).rep
            return _packed_input(sel), apply(_packed_input(sel), part)

        want1 = replica_select_ref(apply(packed, full)).rep
        _, sub1 = sparse(packed)
        ref1 = replica_scatter_inplace_ref(packed, sub1, idx)
        sp = replica_select_ref(sub1, ref1.spill_j, n_out=len(ref1.spill_j)).rep
        back = replica_repack_ref(ref1.rep, _packed_input(sp), ref1.spill_doc, er=ROUND_ROOM, tr=ROUND_ROOM)
        rep2 = back.rep
        want2 = replica_select_ref(apply(_packed_input(want1), full)).rep
        _, sub2 = sparse(rep2)
        ref2 = replica_scatter_inplace_ref(rep2, sub2, idx)
        _round["apply"] = dict(idx=idx, part=part, packed=packed, sub1=sub1, ref1=ref1, back=back, rep2=rep2, sub2=sub2,
                               ref2=ref2, want1=want1, want2=want2)
    return _round["apply"]


def test_apply_round_spill_then_repack_fallback_then_everything_fits():
    m = apply_round_model()
    assert len(m["ref1"].spill_j) >= 1  # (a) the packed replica spills
    assert not m["back"].capacity and not m["back"].invalid
    assert same_packed(replica_select_ref(m["rep2"]).rep, m["want1"]) is None  # (d) round 1 with the fallback
    assert len(m["ref2"].spill_j) == 0 and len(m["ref2"].placed_j) == len(m["idx"])  # (c) round 2 in place
    assert same_packed(replica_select_ref(m["ref2"].rep).rep, m["want2"]) is None  # (d) round 2
    assert same_packed(m["want1"], m["want2"]) is not None  # the second round changed something


# --- the ABI in every layer -----------------------------------------------------

def test_header_library_and_bindings_have_the_entry_points():
    raw = open(abi.HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    go = open(os.path.join(os.path.dirname(PKG), "go", "crdtgpu", "crdtgpu.go")).read()
    lib = ctypes.CDLL(crdtgpu.LIB_PATH)
    for name, n_args in (("crdt_replica_repack_async", 12), ("crdt_headroom_capacity", 2)):
        assert hasattr(lib, name) and getattr(abi.lib(), name).argtypes is not None
        args = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(args.split(",")) == n_args
        assert len(abi.signatures()[name][1]) == n_args
        assert "C.%s(" % name in go
    assert "crdt_replica_repack_async" in crdtgpu.header_functions()
    assert re.search(r"^uint32_t\s+crdt_headroom_capacity\s*\(", text, flags=re.M)
    for method in ("replica_repack_async", "replica_repack"):
        assert hasattr(crdtgpu.Engine, method)
    assert hasattr(crdtgpu, "Headroom") and hasattr(crdtgpu, "repack_slots")
    fields = ["min_spare", "num", "shift", "align"]
    body = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*crdt_headroom\s*;", text).group(1)
    assert re.findall(r"(\w+)\s*;", body) == fields
    assert [f for f, _ in abi.CHeadroom._fields_] == fields
    assert [f.name for f in Headroom.__dataclass_fields__.values()] == fields
    lit = re.search(r"C\.crdt_headroom\{(\w.*?)\}", go, flags=re.S).group(1)
    assert re.findall(r"(\w+):", lit) == fields and "func (e *Engine) ReplicaRepack(" in go
    call = re.search(r"C\.crdt_replica_repack_async\((.*?)\);", go, flags=re.S).group(1)
    depth, n = 0, 1
    for ch in call:
        depth += ch in "([{"
        depth -= ch in ")]}"
        n += ch == "," and depth == 0
    assert n == 12
    doc = re.search(r"/\* ---- replica repack with headroom.*?\*/", raw, flags=re.S).group(0)
    assert "round_up(n + max(min_spare, (n * num) >> shift), align)" in doc and "saturates" in doc
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert all("replica_repack.hip" in re.search(r"^%s := (.*)$" % v, mk, flags=re.M).group(1) for v in ("SRC", "RU_SRC"))
