#!/usr/bin/env python3
"""Time crdt_awset_sources_async beside what it is measured against and what it
replaces, on the same inputs in the same run: 5 warm-up launches, then 25 timed
ones, each between its own pair of device events; the median is reported (and
the minimum).

  shape   the config-3 delta fold's sources as resident replicas: P = 10 replicas
          of 1,048,576 documents, 8 live entries in 16 slots and 2 live
          tombstones in 4 slots each (capacity offsets, counts, slack), R = 16
  (a)     the call
  (b)     hipMemcpyAsync, device to device, of the same live bytes: one copy per
          output column (entries, tombstones, clocks)
  (c)     the host route the call replaces, one round: download every replica,
          pack the live prefixes source-major with numpy (what
          SrcBatch.from_lists builds, vectorised), upload the source batch

Records the box (PCI function, clocks as the driver shows them, measured shader
clock) and its probed streaming copy rate.  Prints one JSON line (and writes it
to the file named by the first argument).  GPU box only.

    python tools/sources_time.py [out.json]
    python tools/sources_time.py --kernels

--kernels: only 30 calls, untimed, for a kernel trace of its own (per-kernel times).
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "go-crdt-playground_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import crdtgpu  # noqa: E402
from bench import box_identity  # noqa: E402
from crdtgpu import abi  # noqa: E402
from crdtgpu.batch import AWSetBatch, Replica, SrcBuffers, TombBatch  # noqa: E402

WARMUP, STEPS = 5, 25
KERNELS_ONLY = len(sys.argv) > 1 and sys.argv[1] == "--kernels"
P, N, R = 10, 1 << 20, 16
E_LIVE, E_SLOTS, T_LIVE, T_SLOTS = 8, 16, 2, 4
dev = torch.device("cuda:0")
eng = crdtgpu.Engine(0)
s = torch.cuda.current_stream()


def timed(call):
    """(median, min) ms of STEPS launches, each between two device events."""
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


copy_gbs = sclk = box = None
if not KERNELS_ONLY:  # the box: identity and the streaming copy rate in this run (2 GiB: 8x the Infinity Cache)
    x = torch.empty(2 << 30, dtype=torch.uint8, device=dev)
    y = torch.empty(2 << 30, dtype=torch.uint8, device=dev)
    x.fill_(0x5A)
    torch.cuda.synchronize()
    copy_gbs = eng.bw_probe(abi.CRDT_PROBE_COPY, x, y, x.numel(), 10)
    sclk = eng.clock_probe()
    box = box_identity(dev)
    del x, y
    torch.cuda.empty_cache()


def columns(p, slots, live):
    """Offsets, counts and the three columns of N documents of `slots` slots, `live` of them live."""
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED + p)
    tot = N * slots
    off = (torch.arange(N + 1, device=dev, dtype=torch.int64) * slots).to(torch.int32)
    cnt = torch.full((N,), live, dtype=torch.int32, device=dev)
    keys = torch.arange(tot, device=dev, dtype=torch.int64) * 16 + p  # ascending in every document
    actors = torch.randint(0, R, (tot,), device=dev, dtype=torch.int32, generator=g)
    counters = torch.randint(1, 1 << 40, (tot,), device=dev, dtype=torch.int64, generator=g)
    return off, cnt, keys, actors, counters


reps = []
for p in range(P):
    o, c, k, a, n_ = columns(p, E_SLOTS, E_LIVE)
    vv = torch.randint(0, 1 << 40, (N * R,), device=dev, dtype=torch.int64)
    to, tc, tk, ta, tn = columns(p + 100, T_SLOTS, T_LIVE)
    reps.append(Replica(AWSetBatch(R, o, k, a, n_, vv, counts=c), TombBatch(to, tk, ta, tn, counts=tc), actor=p))
n_srcs, te, tt = N * P, N * P * E_LIVE, N * P * T_LIVE
out = SrcBuffers(R, N, n_srcs, te, tt, device=dev)
eng.reserve(N)
creps = [r.c() for r in reps]  # prebuilt descriptors: per-launch host work is a few ctypes calls


def call():
    eng.sources_async(creps, out, entry_slots=te, tomb_slots=tt, stream=s)


call()
eng.sync(s)
assert int(out.entry_off[-1]) == te and int(out.tomb_off[-1]) == tt

if KERNELS_ONLY:
    for _ in range(WARMUP + STEPS):
        call()
    eng.sync(s)
    eng.close()
    print("kernels-only run done: %d calls (P %d, n_docs %d, n_srcs %d)" % (WARMUP + STEPS + 1, P, N, n_srcs))
    sys.exit(0)

call_ms = timed(call)

# (b) device copies of the same live bytes, column by column
cp = SrcBuffers(R, N, n_srcs, te, tt, device=dev)
pairs = [(getattr(cp, f), getattr(out, f)) for f in ("keys", "actors", "counters", "tkeys", "tactors", "tcounters", "vv")]


def d2d():
    for d_, s_ in pairs:
        d_.copy_(s_, non_blocking=True)  # hipMemcpyAsync device to device


cpy_ms = timed(d2d)
live_bytes = te * 20 + tt * 20 + n_srcs * R * 8
meta_bytes = n_srcs * 12 + (N + 1) * 4  # src_actor, entry_off, tomb_off, doc_srcs written
moved = 2 * live_bytes
del cp, pairs
torch.cuda.empty_cache()

# (c) the host route, one round
torch.cuda.synchronize()
t0 = time.perf_counter()
host = [r.numpy() for r in reps]
t1 = time.perf_counter()


def pack(cols, live):
    """Live prefixes of every replica's documents, source-major (document, then replica)."""
    outs = []
    for f in ("keys", "actors", "counters"):
        per = [getattr(c, f).reshape(N, -1)[:, :live] for c in cols]  # (the layout of this shape: fixed slots)
        outs.append(np.ascontiguousarray(np.stack(per, axis=1)).reshape(-1))
    return outs


hk, ha, hc = pack([h.state for h in host], E_LIVE)
htk, hta, htc = pack([h.tombs for h in host], T_LIVE)
hvv = np.ascontiguousarray(np.stack([h.state.vv.reshape(N, R) for h in host], axis=1)).reshape(-1)
h_eoff = (np.arange(n_srcs + 1, dtype=np.int64) * E_LIVE).astype(np.uint32)
h_toff = (np.arange(n_srcs + 1, dtype=np.int64) * T_LIVE).astype(np.uint32)
h_actor = np.tile(np.arange(P, dtype=np.uint32), N)
h_docs = (np.arange(N + 1, dtype=np.int64) * P).astype(np.uint32)
t2 = time.perf_counter()
up = [torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).to(dev)
      for a in (h_docs, h_actor, hvv, h_eoff, hk, ha, hc, h_toff, htk, hta, htc)]
torch.cuda.synchronize()
t3 = time.perf_counter()
assert torch.equal(up[4], out.keys) and torch.equal(up[6], out.counters) and torch.equal(up[8], out.tkeys)
assert torch.equal(up[2], out.vv) and torch.equal(up[1], out.src_actor)
down_bytes = sum(int(t.numel()) * t.element_size() for r in reps for t in
                 (r.state.offsets, r.state.counts, r.state.keys, r.state.actors, r.state.counters, r.state.vv,
                  r.tombs.offsets, r.tombs.counts, r.tombs.keys, r.tombs.actors, r.tombs.counters))

line = {
    "what": "crdt_awset_sources_async beside a device copy of the same live bytes and the host route it replaces "
            "(download, pack, upload); same inputs, same run; measured once, on one box",
    "warmup": WARMUP, "steps": STEPS, "statistic": "median of per-launch device-event times",
    "probe_copy_gbs": round(copy_gbs, 1), "sclk_mhz": round(sclk, 1), "box": box,
    "shape": {"replicas": P, "n_docs": N, "R": R, "n_srcs": n_srcs, "live_entries_per_doc": E_LIVE,
              "entry_slots_per_doc": E_SLOTS, "live_tombstones_per_doc": T_LIVE, "tomb_slots_per_doc": T_SLOTS,
              "entries": te, "tombstones": tt},
    "sources_ms_median": call_ms[0], "sources_ms_min": call_ms[1],
    "live_bytes": live_bytes, "offset_and_actor_bytes_written": meta_bytes,
    "bytes_read_plus_written": moved, "sources_gbs": round(moved / (call_ms[0] * 1e-3) / 1e9, 1),
    "d2d_copy_same_live_bytes_ms_median": cpy_ms[0], "d2d_copy_ms_min": cpy_ms[1],
    "d2d_copy_gbs": round(moved / (cpy_ms[0] * 1e-3) / 1e9, 1),
    "sources_over_d2d_copy": round(call_ms[0] / cpy_ms[0], 4),
    "ms_at_probe_copy_rate": round(moved / (copy_gbs * 1e9) * 1e3, 4),
    "host_route_one_round": {
        "download_ms": round((t1 - t0) * 1e3, 1), "download_bytes": down_bytes,
        "pack_ms": round((t2 - t1) * 1e3, 1), "upload_ms": round((t3 - t2) * 1e3, 1),
        "upload_bytes": live_bytes + meta_bytes, "total_ms": round((t3 - t0) * 1e3, 1),
        "host_route_over_sources": round((t3 - t0) * 1e3 / call_ms[0], 1),
        "note": "pageable host arrays; the pack is a numpy restatement of SrcBatch.from_lists for this fixed-slot "
                "layout (the generic builder loops in Python and is slower)",
    },
}
text = json.dumps(line)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
eng.close()
