#!/usr/bin/env python3
"""Time the convergence check (crdt_awset_compare_async) and the sub-batch
selection (crdt_awset_select_async) beside the calls a caller would otherwise
make, on the same inputs in the same run: 5 warm-up launches, then 25 timed
ones, each between its own pair of device events; the median is reported (and
the minimum).

  (a) config-2 shape: 1,048,576 docs x 64 entries per side (crdt_gen_pair_async):
      compare(A, B) against exchange(A, B)
  (b) config-4 shape: 16,384 Zipf docs (crdt_gen_zipf_*): the same two calls
  (c) mostly converged: compare of the config-2 exchange's two outputs (same
      keys, only common keys' dots differ), then select of the resulting worklist
  (d) identity select (compaction) of a config-2 exchange output, against a
      device-to-device copy of the same live bytes (three hipMemcpyAsync, one per
      column) and the COPY probe's rate

Compare reads at most what the exchange reads (2 x 20 B per live entry plus the
clocks) and writes about 1 B per document; its read rate is given against the
crdt_bw_probe READ rate of the box, taken in this run.  Records the box (PCI
function, clocks as the driver shows them, measured shader clock).  Prints one
JSON line (and writes it to the file named by the first argument).  GPU box only.

    python tools/compare_time.py [out.json]
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
from crdtgpu.batch import CompareBuffers, OutBuffers  # noqa: E402
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


def live_entries(batch):
    return int(batch.counts.to(torch.int64).sum())


def compare_vs_exchange(name, A, B, read_gbs, max_doc_entries=None):
    """compare(A, B) and exchange(A, B) on the same inputs; returns the row and the exchange's outputs.
    max_doc_entries: the size promise bench.py gives the exchange at this shape (none: no promise)."""
    n, R = A.n_docs, A.R
    if max_doc_entries:
        eng.set_max_doc_entries(max_doc_entries)
    else:
        eng.set_max_doc_entries()
    a, b = A.as_batch(), B.as_batch()
    eng.reserve(n)
    res = CompareBuffers(n, device=dev)
    o1 = OutBuffers(n, R, A.slots + B.slots, device=dev)
    o2 = OutBuffers(n, R, A.slots + B.slots, device=dev, shared_keys=o1)
    ca, cb, cr, c1, c2 = a.c(), b.c(), res.c(), o1.c(), o2.c()  # prebuilt: per-launch host work is the ctypes call
    cmp_ms = timed(lambda: eng.compare_async(ca, cb, cr, stream=s))
    xch_ms = timed(lambda: eng.exchange_async(ca, cb, c1, c2, stream=s))
    flags, summary, work = res.numpy()
    la, lb = live_entries(a), live_entries(b)
    read_b = (la + lb) * 20 + 2 * n * R * 8 + 2 * n * 8  # entries, clocks, offsets and counts
    row = {
        "shape": name, "n_docs": n, "live_entries_a": la, "live_entries_b": lb,
        "compare_ms_median": cmp_ms[0], "compare_ms_min": cmp_ms[1],
        "exchange_ms_median": xch_ms[0], "exchange_ms_min": xch_ms[1],
        "compare_over_exchange": round(cmp_ms[0] / xch_ms[0], 4),
        "compare_read_bytes_upper_bound": read_b,
        "compare_read_gbs_upper_bound": round(read_b / (cmp_ms[0] * 1e-3) / 1e9, 1),
        "share_of_probe_read_rate_upper_bound": round(read_b / (cmp_ms[0] * 1e-3) / 1e9 / read_gbs, 4),
        "summary_keys_dots_aahead_bahead_selected": summary.tolist(), "n_work": int(len(work)),
        "note": "upper bound: a document whose live counts differ has no entry read, and dots are read only "
                "where the keys matched",
    }
    return row, o1, o2


# the box: identity, streaming read and copy rates in this run (2 GiB: 8x the Infinity Cache)
x = torch.empty(2 << 30, dtype=torch.uint8, device=dev)
y = torch.empty(2 << 30, dtype=torch.uint8, device=dev)
x.fill_(0x5A)
torch.cuda.synchronize()
read_gbs = eng.bw_probe(abi.CRDT_PROBE_READ, x, y, x.numel(), 10)
copy_gbs = eng.bw_probe(abi.CRDT_PROBE_COPY, x, y, x.numel(), 10)
sclk = eng.clock_probe()
box = box_identity(dev)
del x, y
torch.cuda.empty_cache()

rows = []
# (b) config-4 shape first (its buffers are freed before the config-2 cases)
n = 16384
sizes = zipf_sizes(SEED, n)
offs = np.zeros(n + 1, dtype=np.uint32)
np.cumsum(sizes, out=offs[1:])
total = int(offs[-1])
A = OutBuffers(n, 2, total, device=dev)
B = OutBuffers(n, 2, total, device=dev)
eng.gen_zipf_async(SEED, n, torch.from_numpy(offs.view(np.int32).copy()).to(dev), A, B, stream=s)
eng.sync(s)
row4, o1, o2 = compare_vs_exchange("config 4: 16,384 Zipf docs (largest %d entries)" % int(sizes.max()), A, B, read_gbs)
del A, B, o1, o2
torch.cuda.empty_cache()

# (a) config-2 shape
n = 1 << 20
A = OutBuffers(n, 2, n * 64, device=dev)
B = OutBuffers(n, 2, n * 64, device=dev)
eng.gen_pair_async(SEED, n, A, B, stream=s)
eng.sync(s)
row2, o1, o2 = compare_vs_exchange("config 2: 1,048,576 docs x 64 entries per side", A, B, read_gbs, max_doc_entries=64)
rows += [row2, row4]

# (c) mostly converged: the exchange's two outputs (capacity offsets, same keys), then select of the worklist
eng.exchange_async(A.as_batch(), B.as_batch(), o1, o2, stream=s)
eng.sync(s)
del A, B
torch.cuda.empty_cache()
res = CompareBuffers(n, device=dev)
b1, b2 = o1.as_batch(), o2.as_batch()
c1, c2, cr = b1.c(), b2.c(), res.c()
cmp_ms = timed(lambda: eng.compare_async(c1, c2, cr, stream=s))
flags, summary, work = res.numpy()
live1 = live_entries(b1)
read_b = 2 * live1 * 20 + 2 * n * 2 * 8 + 2 * n * 8
n_work = int(len(work))
sel_live = int(o1.counts.to(torch.int64)[torch.from_numpy(work.astype(np.int64)).to(dev)].sum()) if n_work else 0
sel = OutBuffers(max(n_work, 1), 2, max(sel_live, 1), device=dev)
cs = sel.c()
sel_ms = timed(lambda: eng.select_async(c1, cs, idx=res.worklist, n_idx=res.n_work, n_out=n_work,
                                        out_slots=sel_live, stream=s))
rows.append({
    "shape": "mostly converged: compare(out_ab, out_ba) of the config-2 exchange, then select of the worklist",
    "n_docs": n, "live_entries_per_side": live1,
    "compare_ms_median": cmp_ms[0], "compare_ms_min": cmp_ms[1],
    "compare_read_bytes": read_b, "compare_read_gbs": round(read_b / (cmp_ms[0] * 1e-3) / 1e9, 1),
    "share_of_probe_read_rate": round(read_b / (cmp_ms[0] * 1e-3) / 1e9 / read_gbs, 4),
    "summary_keys_dots_aahead_bahead_selected": summary.tolist(), "n_work": n_work,
    "select_worklist_ms_median": sel_ms[0], "select_worklist_ms_min": sel_ms[1],
    "select_live_entries": sel_live, "select_bytes_read_plus_written": 2 * sel_live * 20,
})
del sel
torch.cuda.empty_cache()

# (d) identity select (compaction) of out_ab, against a device copy of the same live bytes
packed = OutBuffers(n, 2, live1, device=dev)
cp = packed.c()
idn_ms = timed(lambda: eng.select_async(c1, cp, n_out=n, out_slots=live1, stream=s))
src = [o1.keys[:live1], o1.actors[:live1], o1.counters[:live1]]
dst = [packed.keys[:live1], packed.actors[:live1], packed.counters[:live1]]


def d2d():
    for d_, s_ in zip(dst, src):
        d_.copy_(s_, non_blocking=True)  # hipMemcpyAsync device to device


cpy_ms = timed(d2d)
moved = 2 * live1 * 20
rows.append({
    "shape": "identity select (compaction) of the config-2 exchange output out_ab",
    "n_docs": n, "live_entries": live1, "capacity_slots": o1.slots,
    "select_ms_median": idn_ms[0], "select_ms_min": idn_ms[1],
    "bytes_read_plus_written": moved, "select_gbs": round(moved / (idn_ms[0] * 1e-3) / 1e9, 1),
    "d2d_copy_same_live_bytes_ms_median": cpy_ms[0], "d2d_copy_ms_min": cpy_ms[1],
    "d2d_copy_gbs": round(moved / (cpy_ms[0] * 1e-3) / 1e9, 1),
    "select_over_d2d_copy": round(idn_ms[0] / cpy_ms[0], 4),
    "ms_at_probe_copy_rate": round(moved / (copy_gbs * 1e9) * 1e3, 4),
})

line = {"what": "crdt_awset_compare_async / crdt_awset_select_async beside crdt_awset_exchange_async and a device "
                "copy, same inputs, same run; measured once, on one box",
        "warmup": WARMUP, "steps": STEPS, "statistic": "median of per-launch device-event times",
        "probe_read_gbs": round(read_gbs, 1), "probe_copy_gbs": round(copy_gbs, 1), "sclk_mhz": round(sclk, 1),
        "box": box, "shapes": rows}
text = json.dumps(line)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
eng.close()
