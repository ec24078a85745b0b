#!/usr/bin/env python3
"""Time crdt_awset_delta_exchange_async beside the composed path it replaces, on
the same inputs in the same run: 5 warm-up rounds, then 25 timed ones, each
between its own pair of device events; the median is reported (and the minimum).

  shape     the config-2 pair (crdt_gen_pair_async: 1,048,576 documents x 2
            replicas, 64 entries per replica, R = 2), then five local ops per
            document and side through crdt_awset_apply_async -- one
            AWSetDelta.Del of two live keys, one of them added again, and one
            new key -- so both replicas hold tombstones (one re-added, one not),
            slack and counts, as resident replicas do
  fused     crdt_awset_delta_exchange_async
  composed  crdt_awset_sources_async x 2 + crdt_awset_fold_async(CRDT_FOLD_DELTA)
            x 2 through the existing entry points: the baseline

Both paths' documents are compared bit for bit (counts, live entries, clocks)
before anything is timed.  Records the share of each kind, the algorithmic bytes
of the fused call and the fraction of the 8 TB/s HBM peak they reach.  Prints one
JSON line (and writes it to the file named by the first argument).  GPU box only.

    python tools/delta_exchange_time.py [out.json]
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
from crdtgpu import CRDT_FOLD_DELTA, CRDT_OP_ADD, CRDT_OP_DELTA_DEL, CRDT_OP_DELTA_DEL_KEY  # noqa: E402
from crdtgpu.batch import OpBatch, OutBuffers, Replica, SrcBuffers, TombBatch, TombBuffers  # noqa: E402

WARMUP, STEPS = 5, 25
N, R, E = 1 << 20, 2, 64
OPS = 5
PEAK_GBS = 8000.0
dev = torch.device("cuda:0")
eng = crdtgpu.Engine(0)
s = torch.cuda.current_stream()


def timed(call):
    """(median, min) ms of STEPS rounds, each between two device events."""
    for _ in range(WARMUP):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(STEPS)]
    for e0, e1 in ev:
        e0.record(s)
        call()
        e1.record(s)
    ev[-1][1].synchronize()
    eng.sync(s)
    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
    return round(statistics.median(ms), 4), round(min(ms), 4)


# ---- the two resident replicas
A, B = OutBuffers(N, R, N * E, device=dev), OutBuffers(N, R, N * E, device=dev)
eng.gen_pair_async(0xC0FFEE, N, A, B, stream=s)
eng.sync(s)
g = torch.Generator(device=dev)
reps = []
for p, gen in enumerate((A, B)):
    g.manual_seed(0xDE17A + p)
    off = gen.offsets.to(torch.int64)[:N]
    cnt = gen.counts.to(torch.int64)
    assert int(cnt.min()) >= 2
    i1 = torch.randint(0, 1 << 30, (N,), device=dev, generator=g) % cnt
    i2 = (i1 + 1 + torch.randint(0, 1 << 30, (N,), device=dev, generator=g) % (cnt - 1)) % cnt  # another live slot
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
live = [int(r.state.counts.to(torch.int64).sum()) for r in reps]
tomb = [int(r.tombs.counts.to(torch.int64).sum()) for r in reps]
slots = [int(r.state.offsets[-1]) for r in reps]
assert all(int(r.state.counts.max()) <= 64 and int(r.tombs.counts.max()) <= 64 for r in reps)  # the wave path

# ---- fused
o_ab, o_ba = OutBuffers(N, R, slots[0] + slots[1], device=dev), OutBuffers(N, R, slots[0] + slots[1], device=dev)
k_ab = torch.zeros(N, dtype=torch.uint8, device=dev)
k_ba = torch.zeros(N, dtype=torch.uint8, device=dev)
ca, cb, c1, c2 = ra.c(), rb.c(), o_ab.c(), o_ba.c()  # prebuilt descriptors


def fused():
    eng.delta_exchange_async(ca, cb, c1, c2, k_ab, k_ba, stream=s)


# ---- composed: sources x 2 + fold(DELTA) x 2
src_a = SrcBuffers(R, N, N, live[0], tomb[0], device=dev)
src_b = SrcBuffers(R, N, N, live[1], tomb[1], device=dev)
f_ab = OutBuffers(N, R, slots[0] + live[1], device=dev)
f_ba = OutBuffers(N, R, slots[1] + live[0], device=dev)
eng.reserve(N, max(f_ab.slots, f_ba.slots))
sa, sb = ra.state.c(), rb.state.c()
csa, csb, cf1, cf2 = src_a.c(), src_b.c(), f_ab.c(), f_ba.c()


def composed():
    eng.sources_async([ca], src_a, entry_slots=live[0], tomb_slots=tomb[0], stream=s)
    eng.sources_async([cb], src_b, entry_slots=live[1], tomb_slots=tomb[1], stream=s)
    eng.fold_async(CRDT_FOLD_DELTA, sa, csb, cf1, stream=s)
    eng.fold_async(CRDT_FOLD_DELTA, sb, csa, cf2, stream=s)


def sources_only():
    eng.sources_async([ca], src_a, entry_slots=live[0], tomb_slots=tomb[0], stream=s)
    eng.sources_async([cb], src_b, entry_slots=live[1], tomb_slots=tomb[1], stream=s)


def folds_only():
    eng.fold_async(CRDT_FOLD_DELTA, sa, csb, cf1, stream=s)
    eng.fold_async(CRDT_FOLD_DELTA, sb, csa, cf2, stream=s)


def packed(o):
    """(counts, live keys, actors, counters document after document, clocks) of an output."""
    cnt = o.counts.to(torch.int64)
    start = torch.repeat_interleave(o.offsets.to(torch.int64)[:N] & 0xFFFFFFFF, cnt)
    first = torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
    idx = start + (torch.arange(int(cnt.sum()), device=dev) - first)
    return cnt, o.keys[idx], o.actors[idx], o.counters[idx], o.vv[: N * R]


fused()
composed()
eng.sync(s)
for x, y, what in ((o_ab, f_ab, "a <- b"), (o_ba, f_ba, "b <- a")):
    for u, v in zip(packed(x), packed(y)):
        assert torch.equal(u, v), what + ": the two paths differ"
out_live = [int(o.counts.to(torch.int64).sum()) for o in (o_ab, o_ba)]
share = {}
for name, k in (("ab", k_ab), ("ba", k_ba)):
    c = torch.bincount(k.to(torch.int64), minlength=3).tolist()
    share[name] = {"none": round(c[0] / N, 4), "delta": round(c[1] / N, 4), "full": round(c[2] / N, 4)}

fused_ms = timed(fused)
composed_ms = timed(composed)
sources_ms = timed(sources_only)
folds_ms = timed(folds_only)

read_b = (sum(live) + sum(tomb)) * 20 + 2 * N * R * 8 + 2 * N * 16  # entries, tombstones, clocks, offsets and counts
written_b = sum(out_live) * 20 + 2 * N * R * 8 + 2 * N * 8 + 2 * N  # entries, clocks, offsets and counts, kinds
gbs = (read_b + written_b) / (fused_ms[0] * 1e-3) / 1e9
line = {
    "what": "crdt_awset_delta_exchange_async beside sources x 2 + fold(DELTA) x 2 on the same resident replicas; "
            "same inputs, same run; both paths' documents bit-equal; measured once, on one box",
    "warmup": WARMUP, "steps": STEPS, "statistic": "median of per-round device-event times", "box": box_identity(dev),
    "shape": {"n_docs": N, "R": R, "live_entries": live, "live_tombstones": tomb, "entry_slots": slots,
              "ops_per_doc_and_side": OPS, "out_live_entries": out_live},
    "kind_share": share,
    "fused_ms_median": fused_ms[0], "fused_ms_min": fused_ms[1],
    "composed_ms_median": composed_ms[0], "composed_ms_min": composed_ms[1],
    "composed_sources_x2_ms_median": sources_ms[0], "composed_folds_x2_ms_median": folds_ms[0],
    "composed_over_fused": round(composed_ms[0] / fused_ms[0], 3),
    "fused_bytes_read": read_b, "fused_bytes_written": written_b, "fused_gbs": round(gbs, 1),
    "fraction_of_8tbs_peak": round(gbs / PEAK_GBS, 4),
}
text = json.dumps(line)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
eng.close()
