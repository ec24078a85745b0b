#!/usr/bin/env python3
"""Time the per-document state digest (crdt_awset_digest_async) beside the
convergence check of the same batch against a copy (crdt_awset_compare_async),
on the same inputs in the same run: 5 warm-up launches, then 25 timed ones, each
between its own pair of device events; the median is reported (and the minimum).

  (a) config-2 shape: 1,048,576 docs x 64 entries (crdt_gen_pair_async, side A)
  (b) config-4 shape: 16,384 Zipf docs (crdt_gen_zipf_*, side A)

The digest reads 20 B per live entry plus the clocks, offsets and counts, and
writes 16 B per document; its read rate is given against the crdt_bw_probe READ
rate of the box, taken in this run.  The compare reads both copies (twice the
bytes).  Records the box (PCI function, clocks as the driver shows them, measured
shader clock).  Prints one JSON line (and writes it to the file named by the
first argument).  GPU box only.

    python tools/digest_time.py [out.json]
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
from crdtgpu import abi  # noqa: E402
from crdtgpu.batch import AWSetBatch, CompareBuffers, OutBuffers  # noqa: E402
from crdtgpu.engine import zipf_sizes  # noqa: E402

WARMUP, STEPS = 5, 25
SEED = 0x5EED
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


def digest_vs_compare(name, A, read_gbs):
    """digest(A) and compare(A, copy of A) on the same batch."""
    n, R = A.n_docs, A.R
    a = A.as_batch()
    copy = AWSetBatch(R, *(t.clone() for t in (a.offsets, a.keys, a.actors, a.counters, a.vv)), counts=a.counts.clone())
    eng.reserve(n)
    dig = torch.empty(2 * n, dtype=torch.int64, device=dev)
    res = CompareBuffers(n, device=dev)
    ca, cc, cr = a.c(), copy.c(), res.c()  # prebuilt: per-launch host work is the ctypes call
    dig_ms = timed(lambda: eng.digest_async(ca, dig, stream=s))
    cmp_ms = timed(lambda: eng.compare_async(ca, cc, cr, stream=s))
    flags, summary, work = res.numpy()
    assert not summary.any()
    live = int(a.counts.to(torch.int64).sum())
    read_b = live * 20 + n * R * 8 + 2 * n * 4  # entries, clocks, offsets and counts
    gbs = read_b / (dig_ms[0] * 1e-3) / 1e9
    return {
        "shape": name, "n_docs": n, "live_entries": live,
        "digest_ms_median": dig_ms[0], "digest_ms_min": dig_ms[1],
        "compare_with_copy_ms_median": cmp_ms[0], "compare_with_copy_ms_min": cmp_ms[1],
        "digest_over_compare": round(dig_ms[0] / cmp_ms[0], 4),
        "digest_read_bytes": read_b, "digest_written_bytes": 16 * n,
        "digest_read_gbs": round(gbs, 1), "share_of_probe_read_rate": round(gbs / read_gbs, 4),
        "ms_at_probe_read_rate": round(read_b / (read_gbs * 1e9) * 1e3, 4),
        "compare_read_gbs": round(2 * read_b / (cmp_ms[0] * 1e-3) / 1e9, 1),
    }


# the box: identity and streaming read rate in this run (2 GiB: 8x the Infinity Cache)
x = torch.empty(2 << 30, dtype=torch.uint8, device=dev)
y = torch.empty(64, dtype=torch.uint8, device=dev)
x.fill_(0x5A)
torch.cuda.synchronize()
read_gbs = eng.bw_probe(abi.CRDT_PROBE_READ, x, y, x.numel(), 10)
sclk = eng.clock_probe()
box = box_identity(dev)
del x, y
torch.cuda.empty_cache()

# (b) config-4 shape first (its buffers are freed before the config-2 case)
n = 16384
sizes = zipf_sizes(SEED, n)
offs = np.zeros(n + 1, dtype=np.uint32)
np.cumsum(sizes, out=offs[1:])
total = int(offs[-1])
A = OutBuffers(n, 2, total, device=dev)
B = OutBuffers(n, 2, total, device=dev)
eng.gen_zipf_async(SEED, n, torch.from_numpy(offs.view(np.int32).copy()).to(dev), A, B, stream=s)
eng.sync(s)
del B
torch.cuda.empty_cache()
row4 = digest_vs_compare("config 4: 16,384 Zipf docs (largest %d entries)" % int(sizes.max()), A, read_gbs)
del A
torch.cuda.empty_cache()

# (a) config-2 shape
n = 1 << 20
A = OutBuffers(n, 2, n * 64, device=dev)
B = OutBuffers(n, 2, n * 64, device=dev)
eng.gen_pair_async(SEED, n, A, B, stream=s)
eng.sync(s)
del B
torch.cuda.empty_cache()
row2 = digest_vs_compare("config 2: 1,048,576 docs x 64 entries", A, read_gbs)

line = {"what": "crdt_awset_digest_async beside crdt_awset_compare_async of the same batch against a copy, same "
                "run; measured once, on one box",
        "warmup": WARMUP, "steps": STEPS, "statistic": "median of per-launch device-event times",
        "probe_read_gbs": round(read_gbs, 1), "sclk_mhz": round(sclk, 1), "box": box, "shapes": [row2, row4]}
text = json.dumps(line)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
eng.close()
