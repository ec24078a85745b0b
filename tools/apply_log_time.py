#!/usr/bin/env python3
"""Time crdt_awset_apply_log_async beside the plain apply and beside the composition it
replaces (the apply, then crdt_awset_diff_async(state, out)), on the same inputs in the
same run: three interleaved rounds, each call 3 warm-up launches and then 15 timed ones
between their own pairs of device events; the median of each round is recorded, and the
median and minimum over the rounds.

The shape is the one tools/delta_exchange_time.py builds its replicas with: 1,048,576
documents of 64 entries (crdt_gen_pair_async's first replica, R = 2) and five local ops
per document -- one DELTA_DEL call with two keys of the state, an ADD of the first of
them and an ADD of a new key -- with no tombstones yet (tombs' counts are zero).

The three ways are compared bit for bit before anything is timed: offsets, counts, clocks,
live entries and tombstones of the logged and the plain apply, and the log's lists against
the diff's.  Prints one JSON line and writes it to the file named by the first argument
(default profiles/apply_log_time.json).  GPU box only.

    python tools/apply_log_time.py [out.json]
"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "go-crdt-playground_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bench import box_identity  # noqa: E402
from crdtgpu import CRDT_OP_ADD, CRDT_OP_DELTA_DEL, CRDT_OP_DELTA_DEL_KEY  # noqa: E402
from crdtgpu.batch import DiffBuffers, MergeLogBuffers, OpBatch, OutBuffers, TombBatch, TombBuffers  # noqa: E402
from join_log_time import ROUNDS, STEPS, WARMUP, dev, eng, live_mask, s, same_log, same_state, timed  # noqa: E402

OPS = 5


def main():
    N, R, E = 1 << 20, 2, 64
    A, B = OutBuffers(N, R, N * E, device=dev), OutBuffers(N, R, N * E, device=dev)
    eng.gen_pair_async(0xC0FFEE, N, A, B, stream=s)
    eng.sync(s)
    del B
    g = torch.Generator(device=dev)
    g.manual_seed(0xDE17A)
    off = A.offsets.to(torch.int64)[:N]
    cnt = A.counts.to(torch.int64)
    assert int(cnt.min()) >= 2
    i1 = torch.randint(0, 1 << 30, (N,), device=dev, generator=g) % cnt
    i2 = (i1 + 1 + torch.randint(0, 1 << 30, (N,), device=dev, generator=g) % (cnt - 1)) % cnt  # another live slot
    k1, k2 = A.keys[off + i1], A.keys[off + i2]
    knew = torch.randint(0, 1 << 62, (N,), device=dev, dtype=torch.int64, generator=g)
    kind = torch.tensor([CRDT_OP_DELTA_DEL, CRDT_OP_DELTA_DEL_KEY, CRDT_OP_DELTA_DEL_KEY, CRDT_OP_ADD, CRDT_OP_ADD],
                        dtype=torch.uint8, device=dev).repeat(N)
    keys = torch.stack([torch.zeros_like(k1), k1, k2, k1, knew], dim=1).reshape(-1).contiguous()
    ops = OpBatch((torch.arange(N + 1, device=dev, dtype=torch.int64) * OPS).to(torch.int32), kind, keys,
                  torch.zeros(N, dtype=torch.int32, device=dev))
    none = TombBatch(torch.zeros(N + 1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                     torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
    state = A.as_batch()
    ss = A.slots
    lo, po = OutBuffers(N, R, ss + N * OPS, device=dev), OutBuffers(N, R, ss + N * OPS, device=dev)
    lt, pt = TombBuffers(N, N * OPS, device=dev), TombBuffers(N, N * OPS, device=dev)
    log = MergeLogBuffers(N, ss, N * OPS, device=dev)
    diff = DiffBuffers(N, ss, N * OPS, device=dev)
    eng.reserve(N)

    def logged():
        eng.apply_log_async(state, ops, lo, log, none, lt, stream=s)

    def plain():
        eng.apply_async(state, ops, po, none, pt, stream=s)

    def composed():
        eng.apply_async(state, ops, po, none, pt, stream=s)
        eng.diff_async(state, po.as_batch(), diff, stream=s)

    logged()
    composed()
    eng.sync(s)
    same_state(lo, po, N, R)
    assert torch.equal(lt.offsets[: N + 1], pt.offsets[: N + 1]) and torch.equal(lt.counts[:N], pt.counts[:N])
    m = live_mask(lt.offsets[: N + 1], lt.counts[:N], N * OPS)
    for f in ("keys", "actors", "counters"):
        assert torch.equal(getattr(lt, f)[: N * OPS][m], getattr(pt, f)[: N * OPS][m]), f
    same_log(log, diff, N)
    rounds = {"apply_log": [], "apply": [], "apply_plus_diff": []}
    for _ in range(ROUNDS):
        for key, call in (("apply_log", logged), ("apply", plain), ("apply_plus_diff", composed)):
            rounds[key].append(round(timed(call), 4))
    med = {k: round(statistics.median(v), 4) for k, v in rounds.items()}
    res = {"tool": "apply_log_time", "box": box_identity(dev), "rounds": ROUNDS, "warmup": WARMUP, "steps": STEPS,
           "note": "measured once on one box", "n_docs": N, "R": R, "state_slots": ss,
           "live_entries": int(cnt.sum()), "ops_per_doc": OPS, "delta_del_keys_per_doc": 2,
           "summary": [int(x) for x in log.summary.cpu().numpy().view(np.uint32)],
           "new_tombstones": int(lt.counts.to(torch.int64).sum()), "agree_bit_for_bit": True,
           "rounds_ms": rounds, "median_ms": med, "min_ms": {k: min(v) for k, v in rounds.items()},
           "log_over_apply_plus_diff": round(med["apply_log"] / med["apply_plus_diff"], 4),
           "log_over_apply": round(med["apply_log"] / med["apply"], 4)}
    text = json.dumps(res)
    print(text)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "apply_log_time.json")
    with open(path, "w") as f:
        f.write(text + "\n")
    eng.close()


if __name__ == "__main__":
    main()
