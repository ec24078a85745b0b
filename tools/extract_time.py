#!/usr/bin/env python3
"""Time the delta extraction at the config-3 shape (1,048,576 docs x 10
AWSetDelta sources of 8 entries + 2 tombstones, R = 16, from
crdt_gen_delta_async) with peer = dst.vv, and beside it the CRDT_FOLD_DELTA
fold of the same inputs in the same run: 10 warm-up launches, then 50 timed
ones between two device events, as the bench legs do.  Prints one JSON line
(and writes it to the file named by the first argument): launch times, the
extraction's algorithmic bytes (count pass + emit pass, from the shapes and the
kept counts) and their time at 8 TB/s, and the shipped share.  GPU box only.

    python tools/extract_time.py [out.json] [n_docs]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "go-crdt-playground_amd"))
import torch  # noqa: E402

import crdtgpu  # noqa: E402
from crdtgpu.batch import OutBuffers, SrcBuffers  # noqa: E402

WARMUP, STEPS = 10, 50
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 20
R, M, E, T = 16, 10, 8, 2
dev = torch.device("cuda:0")
eng = crdtgpu.Engine(0)
D = OutBuffers(n, R, n * 64, device=dev)
S = SrcBuffers(R, n, n * M, n * M * E, n * M * T, device=dev)
eng.gen_delta_async(0x5EED, n, R, M, D, S)
fout = OutBuffers(n, R, n * 64 + n * M * E, device=dev)
msg = SrcBuffers(R, n, n * M, n * M * E, n * M * T, device=dev)
kind = torch.zeros(n * M, dtype=torch.uint8, device=dev)
eng.reserve(n, fout.slots)
s = torch.cuda.current_stream()
dst, peer = D.as_batch(), D.vv


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


t_extract = timed(lambda: eng.delta_extract_async(S, peer, msg, kind=kind, stream=s))
t_fold = timed(lambda: eng.fold_async(crdtgpu.CRDT_FOLD_DELTA, dst, S, fout, stream=s))
t_extract2 = timed(lambda: eng.delta_extract_async(S, peer, msg, kind=kind, stream=s))

ns = n * M
ne_in, nt_in = int(S.entry_off[ns]), int(S.tomb_off[ns])
ne_out, nt_out = int(msg.entry_off[ns]), int(msg.tomb_off[ns])
groups = (n + 64 // R - 1) // (64 // R)
per_src_in = 12  # entry_off, tomb_off, src_actor
common = ns * per_src_in + (n + 1) * 4 + n * R * 8  # + doc_srcs, peer clocks
# count pass: entry actors + counters, whole tombstones, the entry keys their search probes, group counts out
count_b = common + ne_in * 12 + nt_in * 20 + ne_in * 8 + groups * 8
# scan: the group counts in and out
scan_b = groups * 16
# emit pass: whole entries and tombstones in (the search's keys are among them), clocks in and out,
# survivors out, per-source words out
emit_b = (common + groups * 8 + ne_in * 20 + nt_in * 20 + 2 * ns * R * 8 + (ne_out + nt_out) * 20
          + ns * (4 + 4 + 4 + 1) + (n + 1) * 4)
alg = count_b + scan_b + emit_b
kinds = torch.bincount(kind.to(torch.int64), minlength=3).tolist()
line = {
    "what": "delta_extract at the config-3 shape, peer = dst.vv; measured once on one box",
    "n_docs": n, "R": R, "srcs_per_doc": M, "entries_per_src": E, "tombs_per_src": T,
    "warmup": WARMUP, "steps": STEPS,
    "extract_launch_ms": round(t_extract, 4), "extract_launch_ms_again": round(t_extract2, 4),
    "fold_delta_launch_ms": round(t_fold, 4),
    "extract_algorithmic_bytes": alg, "extract_ms_at_8TBps": round(alg / 8e12 * 1e3, 4),
    "extract_bytes_by_pass": {"count": count_b, "scan": scan_b, "emit": emit_b},
    "entries_in": ne_in, "entries_shipped": ne_out, "entry_share": round(ne_out / max(ne_in, 1), 4),
    "tombs_in": nt_in, "tombs_shipped": nt_out, "tomb_share": round(nt_out / max(nt_in, 1), 4),
    "kinds_none_delta_full": kinds,
}
text = json.dumps(line)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
eng.close()
