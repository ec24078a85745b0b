#!/usr/bin/env python3
"""Time crdt_awset_digest_idx_async beside crdt_awset_digest_async of the same
replica, the sparse delta round whose digest arrays it keeps current, and the
Zipf shape where one workgroup walks a very large listed document.  Protocol of
tools/replica_repack_time.py: every comparison runs in three interleaved rounds
(A B .. A B .. A B); a round is 5 warm-up calls and 25 timed ones, each between
its own pair of device events; per call the three round medians and their median.

  uniform   tools/replica_time.py's shape: 1,048,576 documents x 64 entries, R = 2,
            five local ops per document (so two tombstones each).  digest_idx
            (GATHER) of ascending 1 %, 5 %, 25 % and 100 % worklists | the full
            crdt_awset_digest_async | a device copy of the listed live bytes
  round     tools/replica_repack_time.py's sparse delta round on the align 1
            layout: digest_diff, replica_select x 2, delta_exchange of the
            selection, in-place scatter x 2, n_spill x 2 read back, then both
            digest arrays brought up to date by two digest_idx calls on the
            worklist | the same round with two full digests in front (what the
            parent paid) | the round with no digest work at all | the full
            crdt_awset_delta_exchange_async of the same replicas
  zipf      crdt_gen_zipf_async, 2,048 documents (the config-4 generator, the largest
            about 994 k entries): a worklist of the largest document alone | a 5 %
            worklist | the full digest

Prints one JSON line (and writes it to the file named by the first argument).
GPU box only.

    python tools/digest_idx_time.py [out.json]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "go-crdt-playground_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import crdtgpu  # noqa: E402
from bench import box_identity  # noqa: E402
from crdtgpu import CRDT_OP_ADD, CRDT_OP_DEL, CRDT_OP_DELTA_DEL, CRDT_OP_DELTA_DEL_KEY  # noqa: E402
from crdtgpu.batch import (AWSetBatch, CompareBuffers, Headroom, InplaceTarget, OpBatch, OutBuffers, Replica,  # noqa: E402
                           ReplicaBuffers, SpillBuffers, TombBatch, TombBuffers)
from crdtgpu.engine import zipf_sizes  # noqa: E402

WARMUP, STEPS, ROUNDS = 5, 25, 3
N, R, E = 1 << 20, 2, 64
OPS, MORE = 5, 3
SPARE = 6
ZIPF_SEED, ZIPF_N = 0x5EED, 2048
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


def same(a, b):
    return bool(torch.equal(a, b))


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
live_e, live_t = total(ra.state.counts), total(ra.tombs.counts)

# ---- 1. digest_idx of ascending worklists beside the full digest and a copy of the listed bytes
cst, ctb = ra.state.c(), ra.tombs.c()
full = torch.empty(2 * N, dtype=torch.int64, device=dev)
eng.digest_async(cst, full, ctb, stream=s)
eng.sync(s)
uniform = []
for pct in (1, 5, 25, 100):
    g.manual_seed(0x5E1EC7 + pct)
    if pct == 100:
        wk = torch.arange(N, device=dev, dtype=torch.int32)
    else:
        wk = torch.nonzero(torch.rand(N, device=dev, generator=g) < pct / 100.0).reshape(-1).to(torch.int32)
    m = int(wk.numel())
    nw = torch.tensor([m], dtype=torch.int32, device=dev)
    wl = wk.long()
    listed_bytes = (total(ra.state.counts[wl]) + total(ra.tombs.counts[wl])) * 20 + m * (R * 8 + 16)
    src = torch.empty(listed_bytes, dtype=torch.uint8, device=dev)
    dst = torch.empty(listed_bytes, dtype=torch.uint8, device=dev)
    dig = torch.zeros(2 * N, dtype=torch.int64, device=dev)
    res = interleaved({
        "digest_idx": lambda: eng.digest_idx_async(cst, wk, dig, tombs=ctb, n_idx=nw, n_max=m, stream=s),
        "full_digest": lambda: eng.digest_async(cst, full, ctb, stream=s),
        "device_copy_of_listed_bytes": lambda: dst.copy_(src),
    })
    eng.sync(s)
    d2, f2 = dig.view(N, 2), full.view(N, 2)
    exact = same(d2[wl], f2[wl]) and int((d2 != 0).any(dim=1).sum()) == int((f2[wl] != 0).any(dim=1).sum())
    uniform.append({"percent": pct, "listed": m, "listed_bytes": listed_bytes, "exact": exact, "times": res,
                    "digest_idx_over_full": ratio(res, "digest_idx", "full_digest"),
                    "digest_idx_over_copy": ratio(res, "digest_idx", "device_copy_of_listed_bytes"),
                    "digest_idx_read_gbs": round(listed_bytes / res["digest_idx"]["ms"] / 1e6, 1)})
    del src, dst, dig
torch.cuda.empty_cache()

# ---- 2. the sparse delta round of tools/replica_repack_time.py, align 1
g.manual_seed(0x5E1EC7)
work = torch.nonzero(torch.rand(N, device=dev, generator=g) < 0.05).reshape(-1).to(torch.int32)
M = int(work.numel())
n_work = torch.tensor([M], dtype=torch.int32, device=dev)
room = Headroom(SPARE, 1, 0, 1)
cap_e, cap_t = room.total(ra.state.counts.cpu().numpy()), room.total(ra.tombs.counts.cpu().numpy())
roomy = ReplicaBuffers(N, R, cap_e, cap_t, device=dev)
eng.replica_repack_async(ra.c(), roomy.c(), None, None, None, N, room, room, cap_e, cap_t, stream=s)
eng.sync(s)
del ra, out, tout, full
torch.cuda.empty_cache()
wl = work.long()
a = roomy.as_replica(0)
sel = ReplicaBuffers(M, R, total(a.state.counts[wl]), total(a.tombs.counts[wl]), device=dev)
eng.replica_select_async(a, sel, work, n_work, M, stream=s)
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
bp = clone(a)
sp0 = SpillBuffers(M, device=dev)
eng.replica_scatter_inplace_async(bp, changed, work, sp0, n_work, stream=s)
eng.sync(s)
miss = int(sp0.n_spill[0])


def delta_round():
    ca, cb = a.c(), bp.c()
    t_a, t_b = clone(a), clone(bp)
    ct_a, ct_b = InplaceTarget.of(t_a).c(), InplaceTarget.of(t_b).c()
    cta_s, cta_t, ctb_s, ctb_t = t_a.state.c(), t_a.tombs.c(), t_b.state.c(), t_b.tombs.c()
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
    # the digest arrays a caller keeps beside each replica, current before the round
    eng.digest_async(csa, dig_a, csa_t, stream=s)
    eng.digest_async(csb, dig_b, csb_t, stream=s)
    new_a, new_b = dig_a.clone(), dig_b.clone()  # after the round (the inputs stay: every timed round is the same round)

    def full_digests():
        eng.digest_async(csa, dig_a, csa_t, stream=s)
        eng.digest_async(csb, dig_b, csb_t, stream=s)

    def diff():
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

    def redigest():
        eng.digest_idx_async(cta_s, cmpb.worklist, new_a, tombs=cta_t, n_idx=cmpb.n_work, n_max=M, stream=s)
        eng.digest_idx_async(ctb_s, cmpb.worklist, new_b, tombs=ctb_t, n_idx=cmpb.n_work, n_max=M, stream=s)

    diff()
    body()
    redigest()
    eng.sync(s)
    found, spilled = int(cmpb.n_work[0]), [int(back[0]), int(back[1])]
    # the arrays kept current by the worklist are the full digests of the new replicas
    chk = torch.empty(2 * N, dtype=torch.int64, device=dev)
    current = []
    for st, tbs, got in ((cta_s, cta_t, new_a), (ctb_s, ctb_t, new_b)):
        eng.digest_async(st, chk, tbs, stream=s)
        eng.sync(s)
        current.append(same(chk, got))
    del chk
    res = interleaved({
        "round_digests_kept_current": lambda: (diff(), body(), redigest()) and None,
        "round_with_full_digests": lambda: (full_digests(), diff(), body()) and None,
        "round_without_digest_work": body,
        "two_digest_idx_calls": redigest,
        "two_full_digests": full_digests,
        "full_delta_exchange": lambda: eng.delta_exchange_async(ca, cb, cx1, cx2, stream=s),
    })
    return {"align": 1, "documents_differing": found, "spilled": spilled, "changed_documents_that_did_not_fit_b": miss,
            "digest_arrays_equal_full_digests_after_the_round": current, "times": res,
            "kept_current_over_full_exchange": ratio(res, "round_digests_kept_current", "full_delta_exchange"),
            "with_full_digests_over_full_exchange": ratio(res, "round_with_full_digests", "full_delta_exchange"),
            "without_digest_work_over_full_exchange": ratio(res, "round_without_digest_work", "full_delta_exchange"),
            "two_digest_idx_over_two_full_digests": ratio(res, "two_digest_idx_calls", "two_full_digests")}


rnd = delta_round()
del roomy, a, bp, sel, mo, mt, changed
torch.cuda.empty_cache()

# ---- 3. the Zipf shape: one workgroup per very large listed document
sizes = zipf_sizes(ZIPF_SEED, ZIPF_N)
offs = np.zeros(ZIPF_N + 1, dtype=np.uint32)
np.cumsum(sizes, out=offs[1:])
ZA = OutBuffers(ZIPF_N, 2, int(offs[-1]), device=dev)
ZB = OutBuffers(ZIPF_N, 2, int(offs[-1]), device=dev)
eng.gen_zipf_async(ZIPF_SEED, ZIPF_N, torch.from_numpy(offs.view(np.int32).copy()).to(dev), ZA, ZB, stream=s)
eng.sync(s)
del ZB
zst = ZA.as_batch().c()
zfull = torch.empty(2 * ZIPF_N, dtype=torch.int64, device=dev)
eng.digest_async(zst, zfull, None, stream=s)
eng.sync(s)
big = int(np.argmax(sizes))
rs = np.random.RandomState(0x21BF)
five = np.sort(rs.choice(ZIPF_N, ZIPF_N // 20, replace=False)).astype(np.int32)
lists = {"largest_alone": np.array([big], np.int32), "five_percent": five}
zipf = {"n_docs": ZIPF_N, "entries": int(offs[-1]), "largest": int(sizes.max()), "lists": {}}
for name, lst in lists.items():
    wk = torch.from_numpy(lst).to(dev)
    zd = torch.zeros(2 * ZIPF_N, dtype=torch.int64, device=dev)
    res = interleaved({
        "digest_idx": lambda: eng.digest_idx_async(zst, wk, zd, n_max=len(lst), stream=s),
        "full_digest": lambda: eng.digest_async(zst, zfull, None, stream=s),
    })
    eng.sync(s)
    wl = wk.long()
    listed = int(sizes[lst].sum())
    zipf["lists"][name] = {"listed": len(lst), "listed_entries": listed, "largest_listed": int(sizes[lst].max()),
                           "exact": same(zd.view(-1, 2)[wl], zfull.view(-1, 2)[wl]), "times": res,
                           "digest_idx_over_full": ratio(res, "digest_idx", "full_digest"),
                           "digest_idx_read_gbs": round(listed * 20 / res["digest_idx"]["ms"] / 1e6, 1)}

line = {
    "what": "crdt_awset_digest_idx_async (GATHER) of ascending worklists beside crdt_awset_digest_async of the same "
            "replica and a device copy of the listed live bytes; the sparse delta round with both digest arrays kept "
            "current by two digest_idx calls beside the round with two full digests, the round with no digest work and "
            "the full crdt_awset_delta_exchange_async; the Zipf shape, where one workgroup walks a large listed "
            "document; same run, three interleaved rounds per comparison; measured once, on one box",
    "warmup": WARMUP, "steps": STEPS, "rounds": ROUNDS,
    "statistic": "median over the rounds of the per-round median of device-event times", "box": box_identity(dev),
    "n_docs": N, "R": R, "live_entries": live_e, "live_tombstones": live_t,
    "uniform": uniform, "delta_round": rnd, "zipf": zipf,
}
text = json.dumps(line)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
eng.close()
