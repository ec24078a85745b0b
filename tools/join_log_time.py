#!/usr/bin/env python3
"""Time crdt_awset_exchange_log_async beside the plain exchange and beside the
composition it replaces (the exchange, then crdt_awset_diff_async of each input against
its output), on the same inputs in the same run: three interleaved rounds, each call
3 warm-up launches and then 15 timed ones between their own pairs of device events;
the median of each round is recorded, and the median and minimum over the rounds.

  config2   the config-2 pair (crdt_gen_pair_async: 1,048,576 documents x 2 replicas,
            64 entries per replica, R = 2): every document on the wave path
  zipf      crdt_gen_zipf_async, 2,048 documents of Zipf sizes (the config-4 generator):
            nearly every document above 64 entries, i.e. the worklist and the block path

The three ways are compared bit for bit before anything is timed: the merged states'
counts, clocks and live entries, the flags and the summary, and the diff's packed lists
against the log's lists read document by document.  The plain exchange runs with two
separate key columns, as the logged one must.  Prints one JSON line (and writes it to
the file named by the first argument).  GPU box only.

    python tools/join_log_time.py [out.json]
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
from crdtgpu.batch import DiffBuffers, MergeLogBuffers, OutBuffers  # noqa: E402
from crdtgpu.engine import zipf_sizes  # noqa: E402

ROUNDS, WARMUP, STEPS = 3, 3, 15
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


def live_mask(offsets, counts, slots):
    """bool [slots]: the slot lies in some document's live prefix."""
    off = offsets.to(torch.int64)
    idx = torch.arange(slots, device=dev, dtype=torch.int64)
    doc = torch.searchsorted(off[1:].contiguous(), idx, right=True).clamp_(max=off.numel() - 2)
    return (idx >= off[doc]) & (idx - off[doc] < counts.to(torch.int64)[doc])


def same_state(x, y, n, R):
    assert torch.equal(x.offsets[: n + 1], y.offsets[: n + 1]) and torch.equal(x.counts[:n], y.counts[:n])
    assert torch.equal(x.vv[: n * R], y.vv[: n * R])
    m = live_mask(x.offsets[: n + 1], x.counts[:n], x.slots)
    for f in ("keys", "actors", "counters"):
        assert torch.equal(getattr(x, f)[: x.slots][m], getattr(y, f)[: y.slots][m]), f


def same_log(log, diff, n):
    assert torch.equal(log.flags[:n], diff.flags[:n]) and torch.equal(log.summary, diff.summary)
    for side, slots in (("rem", log.rem_slots), ("ups", log.ups_slots)):
        cnt = getattr(log, side + "_counts")[:n]
        doff = getattr(diff, side + "_off")[: n + 1]
        assert torch.equal(cnt, doff[1:] - doff[:-1]), side
        total = int(doff[n])
        m = live_mask(getattr(log, side + "_offsets")[: n + 1], cnt, slots)
        for col in ("keys", "actors", "counters") + (("kind",) if side == "ups" else ()):
            g = getattr(log, "%s_%s" % (side, col))[:slots][m]
            assert torch.equal(g, getattr(diff, "%s_%s" % (side, col))[:total]), (side, col)


def shape(name, n, R, A, B):
    sa, sb = A.slots, B.slots
    a, b = A.as_batch(), B.as_batch()
    lo = [OutBuffers(n, R, sa + sb, device=dev) for _ in range(2)]
    po = [OutBuffers(n, R, sa + sb, device=dev) for _ in range(2)]
    logs = [MergeLogBuffers(n, sa, sb, device=dev), MergeLogBuffers(n, sb, sa, device=dev)]
    diffs = [DiffBuffers(n, sa, sb, device=dev), DiffBuffers(n, sb, sa, device=dev)]
    eng.reserve(n)

    def logged():
        eng.exchange_log_async(a, b, lo[0], lo[1], logs[0], logs[1], stream=s)

    def plain():
        eng.exchange_async(a, b, po[0], po[1], stream=s)

    def composed():
        eng.exchange_async(a, b, po[0], po[1], stream=s)
        eng.diff_async(a, po[0].as_batch(), diffs[0], stream=s)
        eng.diff_async(b, po[1].as_batch(), diffs[1], stream=s)

    logged()
    composed()
    eng.sync(s)
    for i in range(2):
        same_state(lo[i], po[i], n, R)
        same_log(logs[i], diffs[i], n)
    rounds = {"exchange_log": [], "exchange": [], "exchange_plus_2_diff": []}
    for _ in range(ROUNDS):
        for key, call in (("exchange_log", logged), ("exchange", plain), ("exchange_plus_2_diff", composed)):
            rounds[key].append(round(timed(call), 4))
    med = {k: round(statistics.median(v), 4) for k, v in rounds.items()}
    summ = [int(x) for x in logs[0].summary.cpu().numpy().view(np.uint32)]
    live = int(a.counts.to(torch.int64).sum()) if a.counts is not None else sa
    return {"shape": name, "n_docs": n, "R": R, "live_entries_a": live, "slots_a": sa, "slots_b": sb,
            "summary_ab": summ, "agree_bit_for_bit": True, "rounds_ms": rounds, "median_ms": med,
            "min_ms": {k: min(v) for k, v in rounds.items()},
            "exchange_log_over_exchange_plus_2_diff": round(med["exchange_log"] / med["exchange_plus_2_diff"], 4),
            "exchange_log_over_exchange": round(med["exchange_log"] / med["exchange"], 4)}


def main():
    res = {"tool": "join_log_time", "box": box_identity(dev), "rounds": ROUNDS, "warmup": WARMUP, "steps": STEPS,
           "note": "measured once on one box", "shapes": []}
    n, R, E = 1 << 20, 2, 64
    A, B = OutBuffers(n, R, n * E, device=dev), OutBuffers(n, R, n * E, device=dev)
    eng.gen_pair_async(0x5EED, n, A, B, stream=s)
    eng.sync(s)
    res["shapes"].append(shape("config2", n, R, A, B))
    del A, B
    torch.cuda.empty_cache()
    nz = 2048
    sizes = zipf_sizes(0x5EED, nz)
    offs = np.zeros(nz + 1, dtype=np.uint32)
    np.cumsum(sizes, out=offs[1:])
    total = int(offs[-1])
    ZA, ZB = OutBuffers(nz, 2, total, device=dev), OutBuffers(nz, 2, total, device=dev)
    eng.gen_zipf_async(0x5EED, nz, torch.from_numpy(offs.view(np.int32).copy()).to(dev), ZA, ZB, stream=s)
    eng.sync(s)
    r = shape("zipf", nz, 2, ZA, ZB)
    r["docs_above_64"] = int((sizes > 64).sum())
    r["max_doc_entries"] = int(sizes.max())
    res["shapes"].append(r)
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
