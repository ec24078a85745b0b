#!/usr/bin/env python3
"""Time crdt_awset_fold_log_async beside the plain fold and beside the composition it
replaces (the fold, then crdt_awset_diff_async of dst against the output), on the same
inputs in the same run: three interleaved rounds, each call 3 warm-up launches and then
15 timed ones between their own pairs of device events; the median of each round is
recorded, and the median and minimum over the rounds.

  config3   the config-3 documents (crdt_gen_delta_async: R = 16, 10 ordered AWSetDelta
            sources of 8 entries + 2 tombstones into up to 64 entries), CRDT_FOLD_DELTA
  config5   the config-5 documents (crdt_gen_replicas_async: 8 replicas x 16 entries,
            R = 8, r0 <- r1 <- .. <- r7), CRDT_FOLD_AWSET

each at 1,048,576 documents (the benchmark's config 5 runs 12.5 M of them; the document
shape is what the comparison is about).  The three ways are compared bit for bit before
anything is timed: the merged states' counts, clocks and live entries, the flags and the
summary, and the diff's packed lists against the log's lists read document by document.
Prints one JSON line (and writes it to the file named by the first argument).  GPU box
only.

    python tools/fold_log_time.py [out.json]
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
from crdtgpu.batch import DiffBuffers, MergeLogBuffers, OutBuffers, SrcBuffers  # noqa: E402

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


def shape(name, mode, n, R, D, S, es):
    ds = D.slots
    d = D.as_batch()
    lo, po = OutBuffers(n, R, ds + es, device=dev), OutBuffers(n, R, ds + es, device=dev)
    log = MergeLogBuffers(n, ds, es, device=dev)
    diff = DiffBuffers(n, ds, es, device=dev)
    eng.reserve(n, ds + es)

    def logged():
        eng.fold_log_async(mode, d, S, lo, log, stream=s)

    def plain():
        eng.fold_async(mode, d, S, po, stream=s)

    def composed():
        eng.fold_async(mode, d, S, po, stream=s)
        eng.diff_async(d, po.as_batch(), diff, stream=s)

    logged()
    composed()
    eng.sync(s)
    same_state(lo, po, n, R)
    same_log(log, diff, n)
    rounds = {"fold_log": [], "fold": [], "fold_plus_diff": []}
    for _ in range(ROUNDS):
        for key, call in (("fold_log", logged), ("fold", plain), ("fold_plus_diff", composed)):
            rounds[key].append(round(timed(call), 4))
    med = {k: round(statistics.median(v), 4) for k, v in rounds.items()}
    summ = [int(x) for x in log.summary.cpu().numpy().view(np.uint32)]
    return {"shape": name, "mode": mode, "n_docs": n, "R": R, "dst_slots": ds, "source_entry_slots": es,
            "summary": summ, "agree_bit_for_bit": True, "rounds_ms": rounds, "median_ms": med,
            "min_ms": {k: min(v) for k, v in rounds.items()},
            "fold_log_over_fold_plus_diff": round(med["fold_log"] / med["fold_plus_diff"], 4),
            "fold_log_over_fold": round(med["fold_log"] / med["fold"], 4)}


def main():
    res = {"tool": "fold_log_time", "box": box_identity(dev), "rounds": ROUNDS, "warmup": WARMUP, "steps": STEPS,
           "note": "measured once on one box", "shapes": []}
    n = 1 << 20
    R, M = 16, 10
    D = OutBuffers(n, R, n * 64, device=dev)
    S = SrcBuffers(R, n, n * M, n * M * 8, n * M * 2, device=dev)
    eng.gen_delta_async(0x5EED, n, R, M, D, S, stream=s)
    eng.sync(s)
    res["shapes"].append(shape("config3", crdtgpu.CRDT_FOLD_DELTA, n, R, D, S, n * M * 8))
    del D, S
    torch.cuda.empty_cache()
    P, E, R = 8, 16, 8
    D = OutBuffers(n, R, n * E, device=dev)
    S = SrcBuffers(R, n, n * (P - 1), n * (P - 1) * E, 0, device=dev)
    eng.gen_replicas_async(0x5EED, n, P, E, D, S, stream=s)
    eng.sync(s)
    res["shapes"].append(shape("config5", crdtgpu.CRDT_FOLD_AWSET, n, R, D, S, n * (P - 1) * E))
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
