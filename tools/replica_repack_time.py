#!/usr/bin/env python3
"""Time crdt_replica_repack_async, the in-place scatter onto the layouts it writes,
and the sparse delta round in which every document fits, each beside its baselines
on the same inputs in the same run.  Protocol of tools/replica_time.py: every
comparison runs in three interleaved rounds (A B .. A B .. A B); a round is 5
warm-up calls and 25 timed ones, each between its own pair of device events; per
call the three round medians and their median.

  shape     tools/replica_time.py's: 1,048,576 documents x 64 entries, R = 2, five
            local ops per document (so two tombstones each), 5 % worklist
  policy    the rounds' policy of tests/replica_repack_cases.py (twice the live
            count plus 6 spare slots), at align 1 and at align 16
  repack    the whole replica repacked with the policy | crdt_replica_select_async
            compaction of the same replica | a device copy of the live bytes
  scatter   crdt_replica_scatter_inplace_async of the worklist's documents onto the
            align 1 layout | onto the align 16 layout (the partial sectors at a
            placed document's ends)
  round     b' = a with three more local ops (two Add, one Del) on the worklist's
            documents, written in place into a copy of the repacked a.  digest x 2,
            digest_diff, replica_select x 2, delta_exchange of the selection,
            in-place scatter x 2, n_spill x 2 read back | the full
            crdt_awset_delta_exchange_async of the same replicas; also without the
            digests.  The repack is paid once per many rounds and is timed above.

Prints one JSON line (and writes it to the file named by the first argument).
GPU box only.

    python tools/replica_repack_time.py [out.json]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "go-crdt-playground_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import crdtgpu  # noqa: E402
from bench import box_identity  # noqa: E402
from crdtgpu import CRDT_OP_ADD, CRDT_OP_DEL, CRDT_OP_DELTA_DEL, CRDT_OP_DELTA_DEL_KEY  # noqa: E402
from crdtgpu.batch import (AWSetBatch, CompareBuffers, Headroom, InplaceTarget, OpBatch, OutBuffers, Replica,  # noqa: E402
                           ReplicaBuffers, SpillBuffers, TombBatch, TombBuffers)

WARMUP, STEPS, ROUNDS = 5, 25, 3
N, R, E = 1 << 20, 2, 64
OPS, MORE = 5, 3
SPARE = 6
dev = torch.device("cuda:0")
eng = crdtgpu.Engine(0)
s = torch.cuda.current_stream()


def timed(call):
    for _ in range(WARMUP):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(STEPS)]
    for e0, e1 in ev:
        e0.record(s)
        call()
        e1.record(s)
    ev[-1][1].synchronize()
    eng.sync(s)
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev)


def interleaved(calls):
    got = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, c in calls.items():
            got[k].append(round(timed(c), 4))
    return {k: {"rounds_ms": v, "ms": statistics.median(v)} for k, v in got.items()}


def ratio(res, a, b):
    return round(res[a]["ms"] / res[b]["ms"], 3)


def clone(rep):
    st, t = rep.state, rep.tombs
    return Replica(AWSetBatch(st.R, st.offsets, st.keys.clone(), st.actors.clone(), st.counters.clone(), st.vv.clone(),
                              counts=st.counts.clone()),
                   TombBatch(t.offsets, t.keys.clone(), t.actors.clone(), t.counters.clone(), counts=t.counts.clone()),
                   rep.actor, rep.doc_actor.clone())


def total(x):
    return int(x.to(torch.int64).sum())


# ---- the resident replica (tools/replica_time.py's side a)
A, B = OutBuffers(N, R, N * E, device=dev), OutBuffers(N, R, N * E, device=dev)
eng.gen_pair_async(0xC0FFEE, N, A, B, stream=s)
eng.sync(s)
g = torch.Generator(device=dev)
g.manual_seed(0xDE17A)
off = A.offsets.to(torch.int64)[:N]
cnt = A.counts.to(torch.int64)
i1 = torch.randint(0, 1 << 30, (N,), device=dev, generator=g) % cnt
i2 = (i1 + 1 + torch.randint(0, 1 << 30, (N,), device=dev, generator=g) % (cnt - 1)) % cnt
k1, k2 = A.keys[off + i1], A.keys[off + i2]
knew = torch.randint(0, 1 << 62, (N,), device=dev, dtype=torch.int64, generator=g)
kind = torch.tensor([CRDT_OP_DELTA_DEL, CRDT_OP_DELTA_DEL_KEY, CRDT_OP_DELTA_DEL_KEY, CRDT_OP_ADD, CRDT_OP_ADD],
                    dtype=torch.uint8, device=dev).repeat(N)
keys = torch.stack([torch.zeros_like(k1), k1, k2, k1, knew], dim=1).reshape(-1).contiguous()
ops = OpBatch((torch.arange(N + 1, device=dev, dtype=torch.int64) * OPS).to(torch.int32), kind, keys,
              torch.zeros(N, dtype=torch.int32, device=dev))
none = TombBatch(torch.zeros(N + 1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                 torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
out = OutBuffers(N, R, N * (E + OPS), device=dev)
tout = TombBuffers(N, N * OPS, device=dev)
eng.apply_async(A.as_batch(), ops, out, none, tout, stream=s)
eng.sync(s)
ra = Replica(out.as_batch(), tout, 0, torch.zeros(N, dtype=torch.int32, device=dev))
del A, B, ops, none
eng.reserve(N)
g.manual_seed(0x5E1EC7)
work = torch.nonzero(torch.rand(N, device=dev, generator=g) < 0.05).reshape(-1).to(torch.int32)
M = int(work.numel())
n_work = torch.tensor([M], dtype=torch.int32, device=dev)
live_e, live_t = total(ra.state.counts), total(ra.tombs.counts)
live_bytes = (live_e + live_t) * 20 + N * (R * 8 + 12)

# ---- 1. repack of the whole replica, beside the compaction and a copy of the live bytes
rooms = {a: Headroom(SPARE, 1, 0, a) for a in (1, 16)}
caps = {a: (r.total(ra.state.counts.cpu().numpy()), r.total(ra.tombs.counts.cpu().numpy())) for a, r in rooms.items()}
roomy = {a: ReplicaBuffers(N, R, caps[a][0], caps[a][1], device=dev) for a in rooms}
packed = ReplicaBuffers(N, R, live_e, live_t, device=dev)
cra, cpk = ra.c(), packed.c()
cro = {a: roomy[a].c() for a in rooms}
src = torch.empty(live_bytes, dtype=torch.uint8, device=dev)
dst = torch.empty(live_bytes, dtype=torch.uint8, device=dev)
rp = interleaved({
    "repack_align1": lambda: eng.replica_repack_async(cra, cro[1], None, None, None, N, rooms[1], rooms[1],
                                                      caps[1][0], caps[1][1], stream=s),
    "repack_align16": lambda: eng.replica_repack_async(cra, cro[16], None, None, None, N, rooms[16], rooms[16],
                                                       caps[16][0], caps[16][1], stream=s),
    "replica_select_compaction": lambda: eng.replica_select_async(cra, cpk, None, None, N, live_e, live_t, stream=s),
    "device_copy_of_live_bytes": lambda: dst.copy_(src),
})
eng.sync(s)
del src, dst, packed

# ---- b': three more local ops on the worklist's documents of the repacked a
wl = work.long()
base = roomy[1].as_replica(0)
sel = ReplicaBuffers(M, R, total(base.state.counts[wl]), total(base.tombs.counts[wl]), device=dev)
eng.replica_select_async(base, sel, work, n_work, M, stream=s)
eng.sync(s)
first = sel.state.keys[sel.state.offsets.to(torch.int64)[:M]]
g.manual_seed(0xB0B)
new = torch.randint(0, 1 << 62, (M, 2), device=dev, dtype=torch.int64, generator=g)
mkind = torch.tensor([CRDT_OP_ADD, CRDT_OP_ADD, CRDT_OP_DEL], dtype=torch.uint8, device=dev).repeat(M)
mkeys = torch.stack([new[:, 0], new[:, 1], first], dim=1).reshape(-1).contiguous()
mops = OpBatch((torch.arange(M + 1, device=dev, dtype=torch.int64) * MORE).to(torch.int32), mkind, mkeys,
               torch.ones(M, dtype=torch.int32, device=dev))
mo = OutBuffers(M, R, sel.entry_slots + M * MORE, device=dev)
mt = TombBuffers(M, sel.tomb_slots + M * MORE, device=dev)
eng.apply_async(sel.state.as_batch(), mops, mo, sel.tombs, mt, stream=s)
eng.sync(s)
changed = Replica(mo.as_batch(), mt, 1, torch.ones(M, dtype=torch.int32, device=dev))
cchanged = changed.c()


def pair(align):
    """(a, b') on the layout of `align`, b' = a with the changed documents in place; documents that did not fit."""
    a = roomy[align].as_replica(0)
    bp = clone(a)
    sp = SpillBuffers(M, device=dev)
    eng.replica_scatter_inplace_async(bp, changed, work, sp, n_work, stream=s)
    eng.sync(s)
    return a, bp, int(sp.n_spill[0])


# ---- 2. the in-place scatter onto an align 1 and an align 16 target
tg = {}
for a in rooms:
    _, bp, miss = pair(a)
    tg[a] = (InplaceTarget.of(bp).c(), SpillBuffers(M, device=dev), miss, bp)
sc = interleaved({
    "inplace_onto_align%d" % a: (lambda a=a: eng.replica_scatter_inplace_async(tg[a][0], cchanged, work, tg[a][1].c(),
                                                                                n_work, stream=s)) for a in rooms})
placed_bytes = (total(changed.state.counts) + total(changed.tombs.counts)) * 20 + M * (R * 8 + 12)


# ---- 3. the sparse delta round where every document fits
def round_at(align):
    a, bp, miss = pair(align)
    ca, cb = a.c(), bp.c()
    t_a, t_b = clone(a), clone(bp)
    ct_a, ct_b = InplaceTarget.of(t_a).c(), InplaceTarget.of(t_b).c()
    dig_a = torch.empty(2 * N, dtype=torch.int64, device=dev)
    dig_b = torch.empty(2 * N, dtype=torch.int64, device=dev)
    cmpb = CompareBuffers(N, device=dev)
    ccmp = cmpb.c()
    csa, csa_t, csb, csb_t = a.state.c(), a.tombs.c(), bp.state.c(), bp.tombs.c()
    la, ta = total(a.state.counts[wl]), total(a.tombs.counts[wl])
    lb, tb = total(bp.state.counts[wl]), total(bp.tombs.counts[wl])
    s_a, s_b = ReplicaBuffers(M, R, la, ta, device=dev), ReplicaBuffers(M, R, lb, tb, device=dev)
    cs_a, cs_b = s_a.c(), s_b.c()
    cr_a, cr_b = s_a.as_replica().c(), s_b.as_replica().c()
    y_ab, y_ba = OutBuffers(M, R, la + lb, device=dev), OutBuffers(M, R, la + lb, device=dev)
    cy1, cy2 = y_ab.c(), y_ba.c()
    cu_a = Replica(y_ab.as_batch(), s_a.tombs, 0, s_a.doc_actor).c()
    cu_b = Replica(y_ba.as_batch(), s_b.tombs, 0, s_b.doc_actor).c()
    sp_a, sp_b = SpillBuffers(M, device=dev), SpillBuffers(M, device=dev)
    csp_a, csp_b = sp_a.c(), sp_b.c()
    x_slots = int(a.state.offsets[-1]) + int(bp.state.offsets[-1])
    x_ab, x_ba = OutBuffers(N, R, x_slots, device=dev), OutBuffers(N, R, x_slots, device=dev)
    cx1, cx2 = x_ab.c(), x_ba.c()
    back = torch.empty(2, dtype=torch.int32).pin_memory()

    def digests():
        eng.digest_async(csa, dig_a, csa_t, stream=s)
        eng.digest_async(csb, dig_b, csb_t, stream=s)
        eng.digest_diff_async(dig_a, dig_b, N, ccmp, stream=s)

    def body():
        eng.replica_select_async(ca, cs_a, cmpb.worklist, cmpb.n_work, M, la, ta, stream=s)
        eng.replica_select_async(cb, cs_b, cmpb.worklist, cmpb.n_work, M, lb, tb, stream=s)
        eng.delta_exchange_async(cr_a, cr_b, cy1, cy2, stream=s)
        eng.replica_scatter_inplace_async(ct_a, cu_a, cmpb.worklist, csp_a, cmpb.n_work, stream=s)
        eng.replica_scatter_inplace_async(ct_b, cu_b, cmpb.worklist, csp_b, cmpb.n_work, stream=s)
        back[0:1].copy_(sp_a.n_spill, non_blocking=True)  # the 8 bytes a caller reads to skip the fallback
        back[1:2].copy_(sp_b.n_spill, non_blocking=True)
        s.synchronize()

    digests()
    body()
    eng.sync(s)
    found, spilled = int(cmpb.n_work[0]), [int(back[0]), int(back[1])]
    res = interleaved({
        "sparse_round": lambda: (digests(), body()) and None,
        "sparse_round_without_digests": body,
        "full_delta_exchange": lambda: eng.delta_exchange_async(ca, cb, cx1, cx2, stream=s),
    })
    return {"align": align, "documents_differing": found, "spilled": spilled, "changed_documents_that_did_not_fit_b": miss,
            "times": res, "sparse_round_over_full": ratio(res, "sparse_round", "full_delta_exchange"),
            "sparse_round_without_digests_over_full": ratio(res, "sparse_round_without_digests", "full_delta_exchange")}


del tg
torch.cuda.empty_cache()
rounds = [round_at(1), round_at(16)]

line = {
    "what": "crdt_replica_repack_async of a whole replica beside crdt_replica_select_async compaction of the same replica "
            "and a device copy of the live bytes; crdt_replica_scatter_inplace_async onto the align 1 and the align 16 "
            "layout; the sparse delta round in which every document fits (n_spill read back) beside the full "
            "crdt_awset_delta_exchange_async of the same replicas; same run, three interleaved rounds per comparison; "
            "measured once, on one box",
    "warmup": WARMUP, "steps": STEPS, "rounds": ROUNDS,
    "statistic": "median over the rounds of the per-round median of device-event times", "box": box_identity(dev),
    "n_docs": N, "R": R, "worklist": M, "policy": {"min_spare": SPARE, "num": 1, "shift": 0, "align": [1, 16]},
    "live_entries": live_e, "live_tombstones": live_t, "live_bytes": live_bytes,
    "capacity": {str(a): {"entry_slots": caps[a][0], "tomb_slots": caps[a][1],
                          "capacity_over_live": round((caps[a][0] + caps[a][1]) / (live_e + live_t), 3)} for a in rooms},
    "repack": rp,
    "repack_align1_over_select_compaction": ratio(rp, "repack_align1", "replica_select_compaction"),
    "repack_align16_over_select_compaction": ratio(rp, "repack_align16", "replica_select_compaction"),
    "repack_align1_over_copy": ratio(rp, "repack_align1", "device_copy_of_live_bytes"),
    "repack_align16_over_copy": ratio(rp, "repack_align16", "device_copy_of_live_bytes"),
    "scatter_inplace": sc, "scatter_inplace_placed_bytes": placed_bytes,
    "scatter_inplace_align16_over_align1": ratio(sc, "inplace_onto_align16", "inplace_onto_align1"),
    "delta_round": rounds,
}
text = json.dumps(line)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
eng.close()
