#!/usr/bin/env python3
"""Time crdt_replica_select_async / crdt_replica_scatter_async and the sparse delta
round they make possible, beside the existing calls, on the same inputs in the
same run.  Every comparison runs in three interleaved rounds (A B .. A B .. A B);
a round is 5 warm-up calls and 25 timed ones, each between its own pair of device
events; per call the three round medians and their median are reported.

  shape     the delta exchange's measured shape (tools/delta_exchange_time.py): the
            config-2 pair (1,048,576 documents x 2 replicas, 64 entries per
            replica, R = 2), then five local ops per document and side, two of
            them tombstones, so both replicas hold tombstones, slack and counts
  compact   replica_select of all documents, beside crdt_awset_select_async of the
            same state alone and a device copy of the live bytes moved
  select5   the same for a 5 % worklist (ascending, every 20th document on average)
  scatter   replica_scatter of that 5 % back, beside crdt_awset_scatter_async of the
            state part
  offsets   the calls with 0 entry and tombstone slots: the offset scan, the clocks
            and gathers with no position to copy (CRDT_E_CAPACITY is the expected
            report); the closest the ABI gets to the scan alone
  round     b' = a with 5 % of its documents replaced by b's.  Sparse: digest x 2,
            digest_diff, replica_select x 2, delta_exchange of the selection,
            replica_scatter x 2 (compacted outputs).  Full: delta_exchange of
            (a, b') (join layout, not compacted).  Whether the two agree document
            by document is recorded, not assumed.

Prints one JSON line (and writes it to the file named by the first argument).
GPU box only.

    python tools/replica_time.py [out.json]
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
from crdtgpu.batch import CompareBuffers, OpBatch, OutBuffers, Replica, ReplicaBuffers, TombBatch, TombBuffers  # noqa: E402

WARMUP, STEPS, ROUNDS = 5, 25, 3
N, R, E = 1 << 20, 2, 64
OPS = 5
dev = torch.device("cuda:0")
eng = crdtgpu.Engine(0)
s = torch.cuda.current_stream()


def sync():
    try:
        eng.sync(s)
    except crdtgpu.CrdtError as e:  # the 0-slot calls report their totals as above the slots
        assert e.code == crdtgpu.CRDT_E_CAPACITY
    return None


def timed(call):
    for _ in range(WARMUP):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(STEPS)]
    for e0, e1 in ev:
        e0.record(s)
        call()
        e1.record(s)
    ev[-1][1].synchronize()
    sync()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev)


def interleaved(calls):
    """{name: {"rounds_ms": [3 medians], "ms": their median}} of calls timed A B .. A B .. A B."""
    got = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, c in calls.items():
            got[k].append(round(timed(c), 4))
    return {k: {"rounds_ms": v, "ms": statistics.median(v)} for k, v in got.items()}


def ratio(res, a, b):
    return round(res[a]["ms"] / res[b]["ms"], 3)


# ---- the two resident replicas (tools/delta_exchange_time.py's)
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
del A, B
ra, rb = reps
eng.reserve(N)
live = [int(r.state.counts.to(torch.int64).sum()) for r in reps]
tomb = [int(r.tombs.counts.to(torch.int64).sum()) for r in reps]
slots = [int(r.state.offsets[-1]) for r in reps]
tslots = [int(r.tombs.offsets[-1]) for r in reps]

# ---- the 5 % worklist
g.manual_seed(0x5E1EC7)
work = torch.nonzero(torch.rand(N, device=dev, generator=g) < 0.05).reshape(-1).to(torch.int32)
M = int(work.numel())
n_work = torch.tensor([M], dtype=torch.int32, device=dev)
cnt_a = ra.state.counts.to(torch.int64)
tcnt_a = ra.tombs.counts.to(torch.int64)
live5, tomb5 = int(cnt_a[work.long()].sum()), int(tcnt_a[work.long()].sum())

full_r = ReplicaBuffers(N, R, live[0], tomb[0], device=dev)
full_s = OutBuffers(N, R, live[0], device=dev)
sel_r = ReplicaBuffers(M, R, live5, tomb5, device=dev)
sel_s = OutBuffers(M, R, live5, device=dev)
sct_r = ReplicaBuffers(N, R, live[0], tomb[0], device=dev)
sct_s = OutBuffers(N, R, live[0], device=dev)
ca, cb, csa = ra.c(), rb.c(), ra.state.c()
c_full_r, c_full_s, c_sel_r, c_sel_s, c_sct_r, c_sct_s = (x.c() for x in (full_r, full_s, sel_r, sel_s, sct_r, sct_s))


def copy_of(nbytes):
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return lambda: dst.copy_(src)


bytes_full = (live[0] + tomb[0]) * 20 + N * R * 8 + N * 20  # entries, tombstones, clocks, offsets x 2, counts x 2, actors
bytes_5 = (live5 + tomb5) * 20 + M * R * 8 + M * 20
compact = interleaved({
    "replica_select": lambda: eng.replica_select_async(ca, c_full_r, None, None, N, live[0], tomb[0], stream=s),
    "awset_select": lambda: eng.select_async(csa, c_full_s, None, None, N, live[0], stream=s),
    "device_copy": copy_of(bytes_full),
})
select5 = interleaved({
    "replica_select": lambda: eng.replica_select_async(ca, c_sel_r, work, n_work, M, live5, tomb5, stream=s),
    "awset_select": lambda: eng.select_async(csa, c_sel_s, work, n_work, M, live5, stream=s),
    "device_copy": copy_of(bytes_5),
})
sub = sel_r.as_replica()
csub, csub_s = sub.c(), sub.state.c()
scatter = interleaved({
    "replica_scatter": lambda: eng.replica_scatter_async(ca, csub, work, c_sct_r, n_work, live[0], tomb[0], stream=s),
    "awset_scatter": lambda: eng.scatter_async(csa, csub_s, work, c_sct_s, n_work, live[0], stream=s),
})
offsets = interleaved({
    "replica_select_0_slots": lambda: eng.replica_select_async(ca, c_full_r, None, None, N, 0, 0, stream=s),
    "awset_select_0_slots": lambda: eng.select_async(csa, c_full_s, None, None, N, 0, stream=s),
    "replica_scatter_0_slots": lambda: eng.replica_scatter_async(ca, csub, work, c_sct_r, n_work, 0, 0, stream=s),
    "awset_scatter_0_slots": lambda: eng.scatter_async(csa, csub_s, work, c_sct_s, n_work, 0, stream=s),
})

# the state part is the existing calls' output
eng.replica_select_async(ca, c_full_r, None, None, N, live[0], tomb[0], stream=s)
eng.select_async(csa, c_full_s, None, None, N, live[0], stream=s)
eng.replica_scatter_async(ca, csub, work, c_sct_r, n_work, live[0], tomb[0], stream=s)
eng.scatter_async(csa, csub_s, work, c_sct_s, n_work, live[0], stream=s)
eng.sync(s)
for x, y in ((full_r.state, full_s), (sct_r.state, sct_s)):
    for f in ("offsets", "counts", "keys", "actors", "counters", "vv"):
        assert torch.equal(getattr(x, f), getattr(y, f)), f

# ---- the sparse delta round: b' = a with the worklist's documents taken from b
selb = ReplicaBuffers(M, R, int(rb.state.counts.to(torch.int64)[work.long()].sum()),
                      int(rb.tombs.counts.to(torch.int64)[work.long()].sum()), device=dev)
eng.replica_select_async(rb, selb, work, n_work, M, stream=s)
bp_buf = ReplicaBuffers(N, R, live[0] + selb.entry_slots, tomb[0] + selb.tomb_slots, device=dev)
eng.replica_scatter_async(ra, selb.as_replica(), work, bp_buf, n_work, stream=s)
eng.sync(s)
bp = bp_buf.as_replica()
cbp = bp.c()
x_slots = slots[0] + int(bp.state.offsets[-1])
x_ab, x_ba = OutBuffers(N, R, x_slots, device=dev), OutBuffers(N, R, x_slots, device=dev)
cx1, cx2 = x_ab.c(), x_ba.c()
dig_a = torch.empty(2 * N, dtype=torch.int64, device=dev)
dig_b = torch.empty(2 * N, dtype=torch.int64, device=dev)
cmpb = CompareBuffers(N, device=dev)
ccmp = cmpb.c()
csa_t, cbp_s, cbp_t = ra.tombs.c(), bp.state.c(), bp.tombs.c()
s_a = ReplicaBuffers(M, R, live5, tomb5, device=dev)
s_b = ReplicaBuffers(M, R, selb.entry_slots, selb.tomb_slots, device=dev)
cs_a, cs_b = s_a.c(), s_b.c()
r_a, r_b = s_a.as_replica(), s_b.as_replica()
cr_a, cr_b = r_a.c(), r_b.c()
y_slots = live5 + selb.entry_slots
y_ab, y_ba = OutBuffers(M, R, y_slots, device=dev), OutBuffers(M, R, y_slots, device=dev)
cy1, cy2 = y_ab.c(), y_ba.c()
o_a = ReplicaBuffers(N, R, live[0] + y_slots, tomb[0], device=dev)
o_b = ReplicaBuffers(N, R, live[0] + selb.entry_slots + y_slots, tomb[0] + selb.tomb_slots, device=dev)
co_a, co_b = o_a.c(), o_b.c()
cu_a = Replica(y_ab.as_batch(), s_a.tombs, 0, s_a.doc_actor).c()
cu_b = Replica(y_ba.as_batch(), s_b.tombs, 0, s_b.doc_actor).c()


def full_round():
    eng.delta_exchange_async(ca, cbp, cx1, cx2, stream=s)


def sparse_round():
    eng.digest_async(csa, dig_a, csa_t, stream=s)
    eng.digest_async(cbp_s, dig_b, cbp_t, stream=s)
    eng.digest_diff_async(dig_a, dig_b, N, ccmp, stream=s)
    eng.replica_select_async(ca, cs_a, cmpb.worklist, cmpb.n_work, M, s_a.entry_slots, s_a.tomb_slots, stream=s)
    eng.replica_select_async(cbp, cs_b, cmpb.worklist, cmpb.n_work, M, s_b.entry_slots, s_b.tomb_slots, stream=s)
    eng.delta_exchange_async(cr_a, cr_b, cy1, cy2, stream=s)
    eng.replica_scatter_async(ca, cu_a, cmpb.worklist, co_a, cmpb.n_work, o_a.entry_slots, o_a.tomb_slots, stream=s)
    eng.replica_scatter_async(cbp, cu_b, cmpb.worklist, co_b, cmpb.n_work, o_b.entry_slots, o_b.tomb_slots, stream=s)


def sparse_without_digests():
    eng.replica_select_async(ca, cs_a, cmpb.worklist, cmpb.n_work, M, s_a.entry_slots, s_a.tomb_slots, stream=s)
    eng.replica_select_async(cbp, cs_b, cmpb.worklist, cmpb.n_work, M, s_b.entry_slots, s_b.tomb_slots, stream=s)
    eng.delta_exchange_async(cr_a, cr_b, cy1, cy2, stream=s)
    eng.replica_scatter_async(ca, cu_a, cmpb.worklist, co_a, cmpb.n_work, o_a.entry_slots, o_a.tomb_slots, stream=s)
    eng.replica_scatter_async(cbp, cu_b, cmpb.worklist, co_b, cmpb.n_work, o_b.entry_slots, o_b.tomb_slots, stream=s)


def packed(o):
    """(counts, live keys, actors, counters document after document, clocks) of an output."""
    cnt = o.counts.to(torch.int64)
    start = torch.repeat_interleave(o.offsets.to(torch.int64)[:N] & 0xFFFFFFFF, cnt)
    first = torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
    idx = start + (torch.arange(int(cnt.sum()), device=dev) - first)
    return cnt, o.keys[idx], o.actors[idx], o.counters[idx], o.vv[: N * R]


full_round()
sparse_round()
eng.sync(s)
n_found = int(cmpb.n_work[0])
agree = all(torch.equal(u, v) for x, y in ((x_ab, o_a.state), (x_ba, o_b.state)) for u, v in zip(packed(x), packed(y)))
rnd = interleaved({"sparse_round": sparse_round, "full_delta_exchange": full_round,
                   "sparse_round_without_digests": sparse_without_digests})

line = {
    "what": "crdt_replica_select_async / crdt_replica_scatter_async beside crdt_awset_select_async / "
            "crdt_awset_scatter_async of the state part and a device copy of the live bytes, and the sparse delta "
            "round beside the full crdt_awset_delta_exchange_async; same inputs, same run, three interleaved rounds "
            "per comparison; measured once, on one box",
    "warmup": WARMUP, "steps": STEPS, "rounds": ROUNDS,
    "statistic": "median over the rounds of the per-round median of device-event times", "box": box_identity(dev),
    "shape": {"n_docs": N, "R": R, "live_entries": live, "live_tombstones": tomb, "entry_slots": slots,
              "tomb_slots": tslots, "ops_per_doc_and_side": OPS, "worklist": M, "worklist_live_entries": live5,
              "worklist_live_tombstones": tomb5, "bytes_moved_compaction": bytes_full, "bytes_moved_select5": bytes_5},
    "compaction": compact, "compaction_replica_over_awset_select": ratio(compact, "replica_select", "awset_select"),
    "compaction_replica_over_copy": ratio(compact, "replica_select", "device_copy"),
    "select5": select5, "select5_replica_over_awset_select": ratio(select5, "replica_select", "awset_select"),
    "select5_replica_over_copy": ratio(select5, "replica_select", "device_copy"),
    "scatter": scatter, "scatter_replica_over_awset_scatter": ratio(scatter, "replica_scatter", "awset_scatter"),
    "offsets_and_clocks": offsets,
    "state_part_equals_existing_calls": True,
    "delta_round": rnd, "delta_round_documents_differing": n_found, "delta_round_sparse_equals_full": agree,
    "delta_round_sparse_over_full": ratio(rnd, "sparse_round", "full_delta_exchange"),
    "delta_round_sparse_without_digests_over_full": ratio(rnd, "sparse_round_without_digests", "full_delta_exchange"),
}
text = json.dumps(line)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
eng.close()
