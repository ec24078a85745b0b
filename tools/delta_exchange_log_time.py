#!/usr/bin/env python3
"""Time crdt_awset_delta_exchange_log_async beside the plain delta exchange and beside
the composition it replaces (the delta exchange, then crdt_awset_diff_async of each
input against its output), on the same inputs in the same run: three interleaved
rounds, each call 3 warm-up launches and then 15 timed ones between their own pairs of
device events; the median of each round is recorded, and the median and minimum over
the rounds.

  config2   the shape of tools/delta_exchange_time.py: the config-2 pair
            (crdt_gen_pair_async: 1,048,576 documents x 2 replicas, 64 entries per
            replica, R = 2), then five local ops per document and side through
            crdt_awset_apply_async, so both replicas hold tombstones, slack and counts:
            every document on the wave path
  zipf      crdt_gen_zipf_async, 2,048 documents of Zipf sizes (the config-4
            generator), each clock made to have met the other side's actor so that no
            document is FULL: nearly every document above 64 entries, i.e. the worklist
            and the block path

The three ways are compared bit for bit before anything is timed: the merged states and
kinds of the logged and the plain exchange, and the log's lists against the two diffs'.
Prints one JSON line and writes it to the file named by the first argument (default
profiles/delta_exchange_log_time.json).  GPU box only.

    python tools/delta_exchange_log_time.py [out.json]
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
from crdtgpu.batch import DiffBuffers, MergeLogBuffers, OpBatch, OutBuffers, Replica, TombBatch, TombBuffers  # noqa: E402
from crdtgpu.engine import zipf_sizes  # noqa: E402
from join_log_time import ROUNDS, STEPS, WARMUP, dev, eng, live_mask, s, same_log, timed  # noqa: E402

OPS = 5


def same_state(x, y, n, R):
    """Offsets, counts, clocks and live entries of two outputs."""
    assert torch.equal(x.offsets[: n + 1], y.offsets[: n + 1]) and torch.equal(x.counts[:n], y.counts[:n])
    assert torch.equal(x.vv[: n * R], y.vv[: n * R])
    m = live_mask(x.offsets[: n + 1], x.counts[:n], x.slots)
    for f in ("keys", "actors", "counters"):
        assert torch.equal(getattr(x, f)[: x.slots][m], getattr(y, f)[: y.slots][m]), f


def shape(name, n, R, ra, rb):
    sa, sb = int(ra.state.offsets[-1]), int(rb.state.offsets[-1])
    lo = [OutBuffers(n, R, sa + sb, device=dev) for _ in range(2)]
    po = [OutBuffers(n, R, sa + sb, device=dev) for _ in range(2)]
    lk = [torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2)]
    pk = [torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2)]
    logs = [MergeLogBuffers(n, sa, sb, device=dev), MergeLogBuffers(n, sb, sa, device=dev)]
    diffs = [DiffBuffers(n, sa, sb, device=dev), DiffBuffers(n, sb, sa, device=dev)]
    eng.reserve(n)
    ca, cb = ra.c(), rb.c()  # prebuilt descriptors

    def logged():
        eng.delta_exchange_log_async(ca, cb, lo[0], lo[1], logs[0], logs[1], lk[0], lk[1], stream=s)

    def plain():
        eng.delta_exchange_async(ca, cb, po[0], po[1], pk[0], pk[1], stream=s)

    def composed():
        eng.delta_exchange_async(ca, cb, po[0], po[1], pk[0], pk[1], stream=s)
        eng.diff_async(ra.state, po[0].as_batch(), diffs[0], stream=s)
        eng.diff_async(rb.state, po[1].as_batch(), diffs[1], stream=s)

    logged()
    composed()
    eng.sync(s)
    for i in range(2):
        same_state(lo[i], po[i], n, R)
        assert torch.equal(lk[i], pk[i])
        same_log(logs[i], diffs[i], n)
    rounds = {"delta_exchange_log": [], "delta_exchange": [], "delta_exchange_plus_2_diff": []}
    for _ in range(ROUNDS):
        for key, call in (("delta_exchange_log", logged), ("delta_exchange", plain),
                          ("delta_exchange_plus_2_diff", composed)):
            rounds[key].append(round(timed(call), 4))
    med = {k: round(statistics.median(v), 4) for k, v in rounds.items()}
    share = {}
    for key, k in (("ab", lk[0]), ("ba", lk[1])):
        c = torch.bincount(k.to(torch.int64), minlength=3).tolist()
        share[key] = {"none": round(c[0] / n, 4), "delta": round(c[1] / n, 4), "full": round(c[2] / n, 4)}
    summ = [[int(x) for x in lg.summary.cpu().numpy().view(np.uint32)] for lg in logs]
    return {"shape": name, "n_docs": n, "R": R, "slots_a": sa, "slots_b": sb,
            "live_entries": [int(r.state.counts.to(torch.int64).sum()) if r.state.counts is not None
                             else int(r.state.offsets[-1]) for r in (ra, rb)],
            "live_tombstones": [int(r.tombs.counts.to(torch.int64).sum()) if r.tombs is not None else 0 for r in (ra, rb)],
            "kind_share": share, "summary_ab": summ[0], "summary_ba": summ[1], "agree_bit_for_bit": True,
            "rounds_ms": rounds, "median_ms": med, "min_ms": {k: min(v) for k, v in rounds.items()},
            "log_over_plus_2_diff": round(med["delta_exchange_log"] / med["delta_exchange_plus_2_diff"], 4),
            "log_over_plain": round(med["delta_exchange_log"] / med["delta_exchange"], 4)}


def config2_replicas(N, R, E):
    """tools/delta_exchange_time.py's two resident replicas."""
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
    assert all(int(r.state.counts.max()) <= 64 and int(r.tombs.counts.max()) <= 64 for r in reps)  # the wave path
    return reps


def main():
    res = {"tool": "delta_exchange_log_time", "box": box_identity(dev), "rounds": ROUNDS, "warmup": WARMUP,
           "steps": STEPS, "note": "measured once on one box", "shapes": []}
    n, R, E = 1 << 20, 2, 64
    ra, rb = config2_replicas(n, R, E)
    r = shape("config2", n, R, ra, rb)
    r["ops_per_doc_and_side"] = OPS
    res["shapes"].append(r)
    del ra, rb
    torch.cuda.empty_cache()
    nz = 2048
    sizes = zipf_sizes(0x5EED, nz)
    offs = np.zeros(nz + 1, dtype=np.uint32)
    np.cumsum(sizes, out=offs[1:])
    total = int(offs[-1])
    ZA, ZB = OutBuffers(nz, 2, total, device=dev), OutBuffers(nz, 2, total, device=dev)
    eng.gen_zipf_async(0x5EED, nz, torch.from_numpy(offs.view(np.int32).copy()).to(dev), ZA, ZB, stream=s)
    eng.sync(s)
    # the replicas have met: each clock has seen the other side's actor (no document is FULL)
    ZA.vv[: nz * 2].view(nz, 2)[:, 1].clamp_(min=1)
    ZB.vv[: nz * 2].view(nz, 2)[:, 0].clamp_(min=1)
    r = shape("zipf", nz, 2, Replica(ZA.as_batch(), None, actor=0), Replica(ZB.as_batch(), None, actor=1))
    r["docs_above_64"] = int((sizes > 64).sum())
    r["max_doc_entries"] = int(sizes.max())
    res["shapes"].append(r)
    text = json.dumps(res)
    print(text)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "delta_exchange_log_time.json")
    with open(path, "w") as f:
        f.write(text + "\n")
    eng.close()


if __name__ == "__main__":
    main()
