#!/usr/bin/env python3
"""Time crdt_replica_scatter_inplace_async beside crdt_replica_scatter_async, and the
sparse rounds with in-place scatters beside the rounds with packed scatters and the
full exchanges, on the same inputs in the same run.  Protocol of
tools/replica_time.py: every comparison runs in three interleaved rounds
(A B .. A B .. A B); a round is 5 warm-up calls and 25 timed ones, each between its
own pair of device events; per call the three round medians and their median.

  shapes    slack:   tools/replica_time.py's own (1,048,576 documents x 64 entries,
                     R = 2, five local ops per document and side, 5 % worklist); the
                     replicas carry the slack apply left (5 entry and 5 tombstone
                     slots per document, part of them used)
            compact: the same replicas compacted first (replica_select of all): no
                     slack, so every document the merge grows spills
  targets   the in-place calls write into a clone of each replica (same layout), so
            that the round's inputs stay what they were for every timed call; the
            verdicts depend on the layout alone
  scatter   the in-place call, crdt_replica_scatter_async of the same inputs, and a
            device copy of the bytes the placed documents hold
  round     b' = a with 5 % of its documents replaced by b's (in place, so b' keeps
            a's layout).  digest x 2, digest_diff, replica_select x 2, delta_exchange
            of the selection, then: in-place scatter x 2 | in-place x 2 and the
            fallback (select the spilled, packed scatter) x 2 | packed scatter x 2;
            beside the full crdt_awset_delta_exchange_async; each also without the
            digests
  state     the full-state round: compare, select x 2, exchange of the selection,
            state-only in-place scatter x 2 | packed scatter x 2, beside the full
            crdt_awset_exchange_async

Prints one JSON line (and writes it to the file named by the first argument).
GPU box only.

    python tools/replica_inplace_time.py [out.json]
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
from crdtgpu import CRDT_OP_ADD, CRDT_OP_DELTA_DEL, CRDT_OP_DELTA_DEL_KEY  # noqa: E402
from crdtgpu.batch import (AWSetBatch, CompareBuffers, InplaceTarget, OpBatch, OutBuffers, Replica, ReplicaBuffers,  # noqa: E402
                           SpillBuffers, TombBatch, TombBuffers)

WARMUP, STEPS, ROUNDS = 5, 25, 3
N, R, E = 1 << 20, 2, 64
OPS = 5
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
                   rep.actor, torch.full((N,), rep.actor, dtype=torch.int32, device=dev))


def copy_of(nbytes):
    src = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    dst = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    return lambda: dst.copy_(src)


# ---- the two resident replicas (tools/replica_time.py's)
A, B = OutBuffers(N, R, N * E, device=dev), OutBuffers(N, R, N * E, device=dev)
eng.gen_pair_async(0xC0FFEE, N, A, B, stream=s)
eng.sync(s)
g = torch.Generator(device=dev)
reps = []
for p, gen in enumerate((A, B)):
    g.manual_seed(0xDE17A + p)
    off = gen.offsets.to(torch.int64)[:N]
    cnt = gen.counts.to(torch.int64)
    i1 = torch.randint(0, 1 << 30, (N,), device=dev, generator=g) % cnt
    i2 = (i1 + 1 + torch.randint(0, 1 << 30, (N,), device=dev, generator=g) % (cnt - 1)) % cnt
    k1, k2 = gen.keys[off + i1], gen.keys[off + i2]
    knew = torch.randint(0, 1 << 62, (N,), device=dev, dtype=torch.int64, generator=g)
    kind = torch.tensor([CRDT_OP_DELTA_DEL, CRDT_OP_DELTA_DEL_KEY, CRDT_OP_DELTA_DEL_KEY, CRDT_OP_ADD, CRDT_OP_ADD],
                        dtype=torch.uint8, device=dev).repeat(N)
    keys = torch.stack([torch.zeros_like(k1), k1, k2, k1, knew], dim=1).reshape(-1).contiguous()
    ops = OpBatch((torch.arange(N + 1, device=dev, dtype=torch.int64) * OPS).to(torch.int32), kind, keys,
                  torch.full((N,), p, dtype=torch.int32, device=dev))
    none = TombBatch(torch.zeros(N + 1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                     torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
    out = OutBuffers(N, R, N * (E + OPS), device=dev)
    tout = TombBuffers(N, N * OPS, device=dev)
    eng.apply_async(gen.as_batch(), ops, out, none, tout, stream=s)
    eng.sync(s)
    reps.append(Replica(out.as_batch(), tout, actor=p))
del A, B, gen, out, tout
eng.reserve(N)
g.manual_seed(0x5E1EC7)
work = torch.nonzero(torch.rand(N, device=dev, generator=g) < 0.05).reshape(-1).to(torch.int32)
M = int(work.numel())
n_work = torch.tensor([M], dtype=torch.int32, device=dev)


def measure(ra, bp, label):
    """Every comparison at one layout of the pair (ra, bp)."""
    live = int(ra.state.counts.to(torch.int64).sum())
    tomb = int(ra.tombs.counts.to(torch.int64).sum())
    e_slots, t_slots = int(ra.state.offsets[-1]), int(ra.tombs.offsets[-1])
    wl = work.long()
    lb = int(bp.state.counts.to(torch.int64)[wl].sum())
    tb = int(bp.tombs.counts.to(torch.int64)[wl].sum())
    la = int(ra.state.counts.to(torch.int64)[wl].sum())
    ta = int(ra.tombs.counts.to(torch.int64)[wl].sum())
    ca, cbp = ra.c(), bp.c()
    t_a, t_b = clone(ra), clone(bp)  # the targets the in-place calls write
    ct_a, ct_b = InplaceTarget.of(t_a).c(), InplaceTarget.of(t_b).c()
    crt_a, crt_b = t_a.c(), t_b.c()
    dig_a = torch.empty(2 * N, dtype=torch.int64, device=dev)
    dig_b = torch.empty(2 * N, dtype=torch.int64, device=dev)
    cmpb = CompareBuffers(N, device=dev)
    ccmp = cmpb.c()
    csa, csa_t, cbp_s, cbp_t = ra.state.c(), ra.tombs.c(), bp.state.c(), bp.tombs.c()
    s_a = ReplicaBuffers(M, R, la, ta, device=dev)
    s_b = ReplicaBuffers(M, R, max(la, lb), max(ta, tb), device=dev)
    cs_a, cs_b = s_a.c(), s_b.c()
    cr_a, cr_b = s_a.as_replica().c(), s_b.as_replica().c()
    y_slots = la + max(la, lb)
    y_ab, y_ba = OutBuffers(M, R, y_slots, device=dev), OutBuffers(M, R, y_slots, device=dev)
    cy1, cy2 = y_ab.c(), y_ba.c()
    u_a = Replica(y_ab.as_batch(), s_a.tombs, 0, s_a.doc_actor)
    u_b = Replica(y_ba.as_batch(), s_b.tombs, 0, s_b.doc_actor)
    cu_a, cu_b = u_a.c(), u_b.c()
    sp_a, sp_b = SpillBuffers(M, device=dev), SpillBuffers(M, device=dev)
    csp_a, csp_b = sp_a.c(), sp_b.c()
    o_a = ReplicaBuffers(N, R, live + y_slots, tomb + max(ta, tb), device=dev)
    o_b = ReplicaBuffers(N, R, live + lb + y_slots, tomb + 2 * max(ta, tb), device=dev)
    co_a, co_b = o_a.c(), o_b.c()
    f_a = ReplicaBuffers(M, R, y_slots, max(ta, tb), device=dev)  # the fallback's selection of the spilled
    f_b = ReplicaBuffers(M, R, y_slots, max(ta, tb), device=dev)
    cf_a, cf_b = f_a.c(), f_b.c()
    cfr_a, cfr_b = f_a.as_replica().c(), f_b.as_replica().c()
    x_slots = e_slots + int(bp.state.offsets[-1])
    x_ab, x_ba = OutBuffers(N, R, x_slots, device=dev), OutBuffers(N, R, x_slots, device=dev)
    cx1, cx2 = x_ab.c(), x_ba.c()

    def digests():
        eng.digest_async(csa, dig_a, csa_t, stream=s)
        eng.digest_async(cbp_s, dig_b, cbp_t, stream=s)
        eng.digest_diff_async(dig_a, dig_b, N, ccmp, stream=s)

    def head():
        eng.replica_select_async(ca, cs_a, cmpb.worklist, cmpb.n_work, M, s_a.entry_slots, s_a.tomb_slots, stream=s)
        eng.replica_select_async(cbp, cs_b, cmpb.worklist, cmpb.n_work, M, s_b.entry_slots, s_b.tomb_slots, stream=s)
        eng.delta_exchange_async(cr_a, cr_b, cy1, cy2, stream=s)

    def inplace():
        eng.replica_scatter_inplace_async(ct_a, cu_a, cmpb.worklist, csp_a, cmpb.n_work, stream=s)
        eng.replica_scatter_inplace_async(ct_b, cu_b, cmpb.worklist, csp_b, cmpb.n_work, stream=s)

    def packed():
        eng.replica_scatter_async(ca, cu_a, cmpb.worklist, co_a, cmpb.n_work, o_a.entry_slots, o_a.tomb_slots, stream=s)
        eng.replica_scatter_async(cbp, cu_b, cmpb.worklist, co_b, cmpb.n_work, o_b.entry_slots, o_b.tomb_slots, stream=s)

    def fallback():
        eng.replica_select_async(cu_a, cf_a, sp_a.spill_j, sp_a.n_spill, M, f_a.entry_slots, f_a.tomb_slots, stream=s)
        eng.replica_scatter_async(crt_a, cfr_a, sp_a.spill_doc, co_a, sp_a.n_spill, o_a.entry_slots, o_a.tomb_slots, stream=s)
        eng.replica_select_async(cu_b, cf_b, sp_b.spill_j, sp_b.n_spill, M, f_b.entry_slots, f_b.tomb_slots, stream=s)
        eng.replica_scatter_async(crt_b, cfr_b, sp_b.spill_doc, co_b, sp_b.n_spill, o_b.entry_slots, o_b.tomb_slots, stream=s)

    def seq(*fs):
        return lambda: [f() for f in fs] and None

    digests()
    head()
    inplace()
    eng.sync(s)
    n_found = int(cmpb.n_work[0])
    spilled = [int(sp_a.n_spill[0]), int(sp_b.n_spill[0])]
    # the bytes the placed documents of side a hold: entries, tombstones, clock, counts x 2, actor
    mask = torch.arange(M, device=dev) < n_found
    mask[sp_a.spill_j[: spilled[0]].long()] = False
    placed_bytes = int((y_ab.counts.to(torch.int64)[mask].sum() + s_a.tombs.counts.to(torch.int64)[mask].sum()) * 20
                       + int(mask.sum()) * (R * 8 + 12))
    sc = interleaved({
        "inplace": lambda: eng.replica_scatter_inplace_async(ct_a, cu_a, cmpb.worklist, csp_a, cmpb.n_work, stream=s),
        "replica_scatter": lambda: eng.replica_scatter_async(ca, cu_a, cmpb.worklist, co_a, cmpb.n_work, o_a.entry_slots,
                                                             o_a.tomb_slots, stream=s),
        "device_copy_of_placed_bytes": copy_of(placed_bytes),
    })
    rnd = interleaved({
        "sparse_inplace": seq(digests, head, inplace),
        "sparse_inplace_with_fallback": seq(digests, head, inplace, fallback),
        "sparse_packed": seq(digests, head, packed),
        "full_delta_exchange": lambda: eng.delta_exchange_async(ca, cbp, cx1, cx2, stream=s),
        "sparse_inplace_without_digests": seq(head, inplace),
        "sparse_inplace_with_fallback_without_digests": seq(head, inplace, fallback),
        "sparse_packed_without_digests": seq(head, packed),
    })
    # ---- the full-state round
    cbs = bp.state.c()
    zcmp = CompareBuffers(N, device=dev)
    czc = zcmp.c()
    z_a, z_b = OutBuffers(M, R, la, device=dev), OutBuffers(M, R, max(la, lb), device=dev)
    cz_a, cz_b = z_a.c(), z_b.c()
    cza, czb = z_a.as_batch().c(), z_b.as_batch().c()
    w_ab = OutBuffers(M, R, y_slots, device=dev)
    w_ba = OutBuffers(M, R, y_slots, shared_keys=w_ab, device=dev)
    cw1, cw2 = w_ab.c(), w_ba.c()
    cwa, cwb = Replica(w_ab.as_batch()).c(), Replica(w_ba.as_batch()).c()
    cwa_s, cwb_s = w_ab.as_batch().c(), w_ba.as_batch().c()
    zt_a, zt_b = InplaceTarget(t_a.state).c(), InplaceTarget(t_b.state).c()
    p_a, p_b = OutBuffers(N, R, live + y_slots, device=dev), OutBuffers(N, R, live + lb + y_slots, device=dev)
    cp_a, cp_b = p_a.c(), p_b.c()
    fx_slots = e_slots + int(bp.state.offsets[-1])
    fx_ab = OutBuffers(N, R, fx_slots, device=dev)
    fx_ba = OutBuffers(N, R, fx_slots, shared_keys=fx_ab, device=dev)
    cfx1, cfx2 = fx_ab.c(), fx_ba.c()

    def shead():
        eng.compare_async(csa, cbs, czc, stream=s)
        eng.select_async(csa, cz_a, zcmp.worklist, zcmp.n_work, M, la, stream=s)
        eng.select_async(cbs, cz_b, zcmp.worklist, zcmp.n_work, M, max(la, lb), stream=s)
        eng.exchange_async(cza, czb, cw1, cw2, stream=s)

    def sinplace():
        eng.replica_scatter_inplace_async(zt_a, cwa, zcmp.worklist, csp_a, zcmp.n_work, stream=s)
        eng.replica_scatter_inplace_async(zt_b, cwb, zcmp.worklist, csp_b, zcmp.n_work, stream=s)

    def spacked():
        eng.scatter_async(csa, cwa_s, zcmp.worklist, cp_a, zcmp.n_work, p_a.slots, stream=s)
        eng.scatter_async(cbs, cwb_s, zcmp.worklist, cp_b, zcmp.n_work, p_b.slots, stream=s)

    shead()
    sinplace()
    eng.sync(s)
    s_found, s_spilled = int(zcmp.n_work[0]), [int(sp_a.n_spill[0]), int(sp_b.n_spill[0])]
    st = interleaved({
        "sparse_inplace": seq(shead, sinplace),
        "sparse_packed": seq(shead, spacked),
        "full_exchange": lambda: eng.exchange_async(csa, cbs, cfx1, cfx2, stream=s),
    })
    return {
        "layout": label, "live_entries": live, "live_tombstones": tomb, "entry_slots": e_slots, "tomb_slots": t_slots,
        "worklist": M,
        "delta_round_documents_differing": n_found, "delta_round_spilled": spilled,
        "delta_round_spilled_share": [round(x / max(n_found, 1), 4) for x in spilled],
        "placed_bytes_side_a": placed_bytes,
        "scatter": sc, "scatter_inplace_over_replica_scatter": ratio(sc, "inplace", "replica_scatter"),
        "scatter_inplace_over_copy": ratio(sc, "inplace", "device_copy_of_placed_bytes"),
        "delta_round": rnd,
        "delta_round_inplace_over_full": ratio(rnd, "sparse_inplace", "full_delta_exchange"),
        "delta_round_inplace_with_fallback_over_full": ratio(rnd, "sparse_inplace_with_fallback", "full_delta_exchange"),
        "delta_round_packed_over_full": ratio(rnd, "sparse_packed", "full_delta_exchange"),
        "delta_round_inplace_without_digests_over_full": ratio(rnd, "sparse_inplace_without_digests", "full_delta_exchange"),
        "delta_round_inplace_with_fallback_without_digests_over_full":
            ratio(rnd, "sparse_inplace_with_fallback_without_digests", "full_delta_exchange"),
        "delta_round_packed_without_digests_over_full": ratio(rnd, "sparse_packed_without_digests", "full_delta_exchange"),
        "state_round": st, "state_round_documents_differing": s_found, "state_round_spilled": s_spilled,
        "state_round_spilled_share": [round(x / max(s_found, 1), 4) for x in s_spilled],
        "state_round_inplace_over_full": ratio(st, "sparse_inplace", "full_exchange"),
        "state_round_packed_over_full": ratio(st, "sparse_packed", "full_exchange"),
    }


ra, rb = reps
# b' = a with the worklist's documents taken from b, written in place: a's layout
wl0 = work.long()
selb = ReplicaBuffers(M, R, int(rb.state.counts.to(torch.int64)[wl0].sum()), int(rb.tombs.counts.to(torch.int64)[wl0].sum()),
                      device=dev)
eng.replica_select_async(rb, selb, work, n_work, M, stream=s)
bp0 = clone(ra)
sp0 = SpillBuffers(M, device=dev)
eng.replica_scatter_inplace_async(bp0, selb.as_replica(), work, sp0, n_work, stream=s)
eng.sync(s)
not_replaced = int(sp0.n_spill[0])  # (documents of b that did not fit a's slots stay a's: equal, so off the worklist)
del rb, selb
shapes = [measure(ra, bp0, "slack: as apply left the replicas")]
reps = [ra, bp0]
packed_reps = []
for r in reps:
    o = ReplicaBuffers(N, R, int(r.state.counts.to(torch.int64).sum()), int(r.tombs.counts.to(torch.int64).sum()), device=dev)
    eng.replica_select_async(r, o, None, None, N, stream=s)
    eng.sync(s)
    packed_reps.append(o.as_replica(r.actor))
del reps, ra, bp0
torch.cuda.empty_cache()
shapes.append(measure(packed_reps[0], packed_reps[1], "compact: no slack"))

line = {
    "what": "crdt_replica_scatter_inplace_async beside crdt_replica_scatter_async of the same inputs and a device copy of "
            "the placed bytes; the sparse delta round with in-place scatters (with and without the fallback for the "
            "spilled) beside the round with packed scatters and the full crdt_awset_delta_exchange_async; the full-state "
            "round beside crdt_awset_exchange_async; the in-place calls write clones of the replicas so that every timed "
            "call sees the same inputs; same run, three interleaved rounds per comparison; measured once, on one box",
    "warmup": WARMUP, "steps": STEPS, "rounds": ROUNDS,
    "statistic": "median over the rounds of the per-round median of device-event times", "box": box_identity(dev),
    "n_docs": N, "R": R, "ops_per_doc_and_side": OPS, "worklist_documents_of_b_that_did_not_fit_a": not_replaced,
    "shapes": shapes,
}
text = json.dumps(line)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
eng.close()
