#!/usr/bin/env python3
"""Time the batched membership read (crdt_awset_has_async) on two shapes: 10
warm-up launches, then 50 timed ones between two device events, as
tools/extract_time.py does.

  (a) the config-2 shape: 1,048,576 docs x 64 entries from crdt_gen_pair_async,
      8 queries per doc, half drawn on the device from the doc's own keys and
      half random u64
  (b) the config-4 shape: 16,384 docs from crdt_gen_zipf_*, 2^23 queries spread
      uniformly over the documents (half own keys, half random, the same way)

Per shape: ms per call, queries per second, the bytes every implementation must
stream (8 B of key in and 13 B out per query, 12 B of per-document words) and
the hit share observed.  For context only: the time the same run's
crdt_bw_probe READ rate implies for one read of the state's key column (what a
document-cooperative path would pay) and the PCIe time of downloading the state
at the boundary's measured link rate (what a caller pays today).
Prints one JSON line (and writes it to the file named by the first argument).
GPU box only.

    python tools/has_time.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "go-crdt-playground_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import crdtgpu  # noqa: E402
from crdtgpu import abi  # noqa: E402
from crdtgpu.batch import OutBuffers, QueryBatch, QueryBuffers  # noqa: E402
from crdtgpu.engine import zipf_sizes  # noqa: E402

WARMUP, STEPS = 10, 50
SEED = 0x5EED
PCIE_GBS = 57.0  # the boundary's measured H2D/D2H DMA rate (profiles/r05i_boundary_timeline.txt)
dev = torch.device("cuda:0")
eng = crdtgpu.Engine(0)
s = torch.cuda.current_stream()
gen = torch.Generator(device=dev)
gen.manual_seed(SEED)


def timed(call):
    for _ in range(WARMUP):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(STEPS):
        call()
    e1.record(s)
    e1.synchronize()
    eng.sync(s)
    return e0.elapsed_time(e1) / STEPS


def rand_u64(n):
    hi = torch.randint(0, 2 ** 32, (n,), dtype=torch.int64, device=dev, generator=gen)
    lo = torch.randint(0, 2 ** 32, (n,), dtype=torch.int64, device=dev, generator=gen)
    return (hi << 32) | lo  # (the bits of a u64; torch has no unsigned 64-bit type)


def queries(state, q_doc):
    """Keys for queries whose documents are q_doc (sorted, int64 on the device):
    every other query one of its document's own live keys, the rest random u64."""
    nq = q_doc.numel()
    off = state.offsets.to(torch.int64)
    live = state.counts.to(torch.int64)[q_doc]
    pick = (torch.rand(nq, device=dev, generator=gen) * live.to(torch.float64)).to(torch.int64)
    pick = torch.minimum(pick, torch.clamp(live - 1, min=0))
    own = state.keys[torch.clamp(off[q_doc] + pick, max=state.keys.numel() - 1)]
    keys = torch.where((torch.arange(nq, device=dev) % 2 == 0) & (live > 0), own, rand_u64(nq))
    q_off = torch.zeros(state.n_docs + 1, dtype=torch.int64, device=dev)
    q_off[1:] = torch.cumsum(torch.bincount(q_doc, minlength=state.n_docs), 0)
    return QueryBatch(q_off.to(torch.int32), keys.contiguous(), nq)


def shape(name, state, q, read_gbs):
    out = QueryBuffers(q.n_queries, device=dev)
    cs, cq, co = state.c(), q.c(), out.c()  # prebuilt: per-launch host work is the ctypes call
    ms = timed(lambda: eng.has_async(cs, cq, co, stream=s))
    found = out.found.to(torch.int64)
    assert int(found.max()) <= 1
    hits = int(found.sum())
    n, nq = state.n_docs, q.n_queries
    live = int(state.counts.to(torch.int64).sum())
    stream_b = nq * (8 + 13) + n * 12
    return {
        "shape": name, "n_docs": n, "live_entries": live, "n_queries": nq,
        "ms_per_call": round(ms, 4), "queries_per_s": round(nq / (ms * 1e-3), 1),
        "stream_bytes": stream_b, "stream_ms_at_probe_read_rate": round(stream_b / (read_gbs * 1e9) * 1e3, 4),
        "hit_share": round(hits / nq, 4),
        "context_key_column_read_ms": round(live * 8 / (read_gbs * 1e9) * 1e3, 4),
        "context_state_download_ms_at_%g_GBps" % PCIE_GBS: round(live * 20 / (PCIE_GBS * 1e9) * 1e3, 2),
    }


# the box's own streaming read rate, in this run (2 GiB: 8x the Infinity Cache)
a = torch.empty(2 << 30, dtype=torch.uint8, device=dev)
b = torch.empty(64, dtype=torch.uint8, device=dev)
a.fill_(0x5A)
torch.cuda.synchronize()
read_gbs = eng.bw_probe(abi.CRDT_PROBE_READ, a, b, a.numel(), 10)
del a
torch.cuda.empty_cache()

res = []
# (a) config-2 shape
n = 1 << 20
A = OutBuffers(n, 2, n * 64, device=dev)
B = OutBuffers(n, 2, n * 64, device=dev)
eng.gen_pair_async(SEED, n, A, B, stream=s)
eng.sync(s)
res.append(shape("config 2: 1,048,576 docs x 64 entries, 8 queries per doc", A.as_batch(),
                 queries(A.as_batch(), torch.arange(n, device=dev).repeat_interleave(8)), read_gbs))
del A, B
torch.cuda.empty_cache()
# (b) config-4 shape
n = 16384
sizes = zipf_sizes(SEED, n)
offs = np.zeros(n + 1, dtype=np.uint32)
np.cumsum(sizes, out=offs[1:])
total = int(offs[-1])
d_offs = torch.from_numpy(offs.view(np.int32).copy()).to(dev)
A = OutBuffers(n, 2, total, device=dev)
B = OutBuffers(n, 2, total, device=dev)
eng.gen_zipf_async(SEED, n, d_offs, A, B, stream=s)
eng.sync(s)
q_doc = torch.sort(torch.randint(0, n, (1 << 23,), dtype=torch.int64, device=dev, generator=gen)).values
res.append(shape("config 4: 16,384 Zipf docs, 2^23 queries uniform over docs", A.as_batch(),
                 queries(A.as_batch(), q_doc), read_gbs))

line = {"what": "crdt_awset_has_async, dots written; measured once, on one box",
        "warmup": WARMUP, "steps": STEPS, "probe_read_gbs": round(read_gbs, 1), "pcie_gbs": PCIE_GBS, "shapes": res}
text = json.dumps(line)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
eng.close()
