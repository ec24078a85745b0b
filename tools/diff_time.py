#!/usr/bin/env python3
"""Time the merge diff (crdt_awset_diff_async) beside the convergence check of
the same batches (crdt_awset_compare_async) and a device copy of the bytes it
reads, in the same process, in interleaved rounds: ROUNDS rounds, in each the
calls take turns with STEPS launches each, every launch between its own pair of
device events; the median over all rounds is reported (and the minimum).

  (a) config-2 shape: 1,048,576 docs x 64 entries per side (crdt_gen_pair_async):
      diff(A, out_ab) of the exchange(A, B), out_ab as the exchange left it
  (b) config-4 shape: 16,384 Zipf docs (crdt_gen_zipf_*): the same
  (c) fully converged: diff of the config-2 batch A against an identical copy --
      every first probe hits, so the diff should cost what the compare costs
  (d) boundary shape: 65,536 document pairs x 64 entries: bytes and time of
      downloading the two lists, their offsets and the flags, against
      downloading the merged output (offsets, counts, three columns, clocks),
      which the host path does today

Records the box (PCI function, clocks as the driver shows them, measured shader
clock) and its streaming read and copy rates in this run.  Prints one JSON line
(and writes it to the file named by the first argument).  GPU box only.

    python tools/diff_time.py [out.json]
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
from crdtgpu.batch import AWSetBatch, CompareBuffers, DiffBuffers, OutBuffers  # noqa: E402
from crdtgpu.engine import zipf_sizes  # noqa: E402

WARMUP, STEPS, ROUNDS = 3, 8, 3
SEED = 0x5EED
dev = torch.device("cuda:0")
eng = crdtgpu.Engine(0)
s = torch.cuda.current_stream()


def interleaved(calls):
    """{name: (median, min) ms}: ROUNDS rounds, the calls taking turns, STEPS launches each."""
    ms = {k: [] for k in calls}
    for k, call in calls.items():
        for _ in range(WARMUP):
            call()
    for _ in range(ROUNDS):
        for k, call in calls.items():
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(STEPS)]
            for e0, e1 in ev:
                e0.record(s)
                call()
                e1.record(s)
            ev[-1][1].synchronize()
            ms[k] += [e0.elapsed_time(e1) for e0, e1 in ev]
    try:
        eng.sync(s)
    except crdtgpu.CrdtError as e:  # (a list sized too small would show here: CRDT_E_CAPACITY)
        raise SystemExit("diff_time: %s" % e)
    return {k: (round(statistics.median(v), 4), round(min(v), 4)) for k, v in ms.items()}


def live_entries(batch):
    if batch.counts is None:
        return int(batch.offsets[-1])
    return int(batch.counts.to(torch.int64).sum())


def diff_row(name, before, after, read_gbs):
    """diff, compare and a device copy of the bytes read, on the same two batches."""
    n, R = before.n_docs, before.R
    eng.reserve(n)
    lb, la = live_entries(before), live_entries(after)
    out = DiffBuffers(n, lb, la, device=dev)  # worst case: every entry removed, every entry upserted
    res = CompareBuffers(n, device=dev)
    cb, ca, co, cr = before.c(), after.c(), out.c(), res.c()
    read_b = (lb + la) * 20 + 2 * n * R * 8 + 2 * n * 8  # entries, clocks, offsets and counts: an upper bound
    words = (read_b + 7) // 8
    src = torch.empty(words, dtype=torch.int64, device=dev)
    dst = torch.empty(words, dtype=torch.int64, device=dev)
    t = interleaved({
        "diff": lambda: eng.diff_async(cb, ca, co, rem_slots=lb, ups_slots=la, stream=s),
        "compare": lambda: eng.compare_async(cb, ca, cr, stream=s),
        "copy": lambda: dst.copy_(src, non_blocking=True),
    })
    h = out.numpy()
    return {
        "shape": name, "n_docs": n, "live_entries_before": lb, "live_entries_after": la,
        "diff_ms_median": t["diff"][0], "diff_ms_min": t["diff"][1],
        "compare_ms_median": t["compare"][0], "compare_ms_min": t["compare"][1],
        "d2d_copy_of_the_bytes_read_ms_median": t["copy"][0], "d2d_copy_ms_min": t["copy"][1],
        "diff_over_compare": round(t["diff"][0] / t["compare"][0], 4),
        "diff_over_d2d_copy": round(t["diff"][0] / t["copy"][0], 4),
        "read_bytes_upper_bound": read_b,
        "diff_read_gbs_upper_bound": round(read_b / (t["diff"][0] * 1e-3) / 1e9, 1),
        "share_of_probe_read_rate_upper_bound": round(read_b / (t["diff"][0] * 1e-3) / 1e9 / read_gbs, 4),
        "summary_removed_upserts_updated_docs_changed_docs_flagged": h["summary"].tolist(),
        "note": "upper bound on the bytes: the diff runs its search in the count and in the emit pass, so entries "
                "are read up to twice; dots are read only where keys matched",
    }


def download_ms(tensors):
    """(bytes, median ms, min ms) of copying the tensors to the host, one after the other."""
    ms = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for x in tensors:
            x.cpu()
        ms.append((time.perf_counter() - t0) * 1e3)
    return sum(x.numel() * x.element_size() for x in tensors), round(statistics.median(ms), 4), round(min(ms), 4)


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


def exchanged(A, B, max_doc_entries=None):
    n, R = A.n_docs, A.R
    if max_doc_entries:
        eng.set_max_doc_entries(max_doc_entries)
    else:
        eng.set_max_doc_entries()
    o1 = OutBuffers(n, R, A.slots + B.slots, device=dev)
    o2 = OutBuffers(n, R, A.slots + B.slots, device=dev)
    eng.exchange_async(A.as_batch(), B.as_batch(), o1, o2, stream=s)
    eng.sync(s)
    eng.set_max_doc_entries()
    return o1


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
o1 = exchanged(A, B)
row4 = diff_row("config 4: 16,384 Zipf docs (largest %d entries), a against out_ab" % int(sizes.max()),
                A.as_batch(), o1.as_batch(), read_gbs)
del A, B, o1
torch.cuda.empty_cache()

# (a) config-2 shape
n = 1 << 20
A = OutBuffers(n, 2, n * 64, device=dev)
B = OutBuffers(n, 2, n * 64, device=dev)
eng.gen_pair_async(SEED, n, A, B, stream=s)
eng.sync(s)
o1 = exchanged(A, B, 64)
rows.append(diff_row("config 2: 1,048,576 docs x 64 entries per side, a against out_ab", A.as_batch(), o1.as_batch(),
                     read_gbs))
rows.append(row4)
del B, o1
torch.cuda.empty_cache()

# (c) fully converged: A against an identical copy
a = A.as_batch()
twin = AWSetBatch(a.R, a.offsets.clone(), a.keys.clone(), a.actors.clone(), a.counters.clone(), a.vv.clone(),
                  counts=a.counts.clone())
rows.append(diff_row("fully converged: the config-2 batch a against an identical copy", a, twin, read_gbs))
del A, a, twin
torch.cuda.empty_cache()

# (d) boundary shape: what crosses PCIe after the merge, lists against merged state
n = 65536
A = OutBuffers(n, 2, n * 64, device=dev)
B = OutBuffers(n, 2, n * 64, device=dev)
eng.gen_pair_async(SEED, n, A, B, stream=s)
eng.sync(s)
o1 = exchanged(A, B, 64)
before, after = A.as_batch(), o1.as_batch()
out = DiffBuffers(n, live_entries(before), live_entries(after), device=dev)
eng.diff_async(before, after, out, stream=s)
eng.sync(s)
h = out.numpy()
nr, nu = int(h["rem_off"][-1]), int(h["ups_off"][-1])
lists = [out.flags[:n], out.rem_off, out.ups_off, out.rem_keys[:nr], out.rem_actors[:nr], out.rem_counters[:nr],
         out.ups_keys[:nu], out.ups_actors[:nu], out.ups_counters[:nu], out.ups_kind[:nu]]
lists = [t_.contiguous() for t_ in lists if t_.numel()]
merged = [o1.offsets, o1.counts, o1.keys, o1.actors, o1.counters, o1.vv]
lb_, lm, lmin = download_ms(lists)
mb_, mm, mmin = download_ms(merged)
boundary = {
    "shape": "boundary: 65,536 document pairs x 64 entries per side, a against out_ab",
    "n_docs": n, "removed": nr, "upserts": nu, "live_entries_merged": live_entries(after),
    "lists_bytes": lb_, "lists_download_ms_median": lm, "lists_download_ms_min": lmin,
    "merged_output_bytes": mb_, "merged_output_download_ms_median": mm, "merged_output_download_ms_min": mmin,
    "lists_over_merged_bytes": round(lb_ / mb_, 4), "lists_over_merged_ms": round(lm / mm, 4),
    "note": "pageable host memory on both sides, one copy call per array; the merged output at its capacity offsets, "
            "as the host path downloads it without pack_batch_outputs",
}

line = {"what": "crdt_awset_diff_async beside crdt_awset_compare_async and a device copy of the bytes read, same "
                "batches, same process, interleaved rounds; then list against merged-state download at the boundary "
                "shape; measured once, on one box",
        "warmup": WARMUP, "steps_per_round": STEPS, "rounds": ROUNDS,
        "statistic": "median of per-launch device-event times over all rounds",
        "probe_read_gbs": round(read_gbs, 1), "probe_copy_gbs": round(copy_gbs, 1), "sclk_mhz": round(sclk, 1),
        "box": box, "shapes": rows, "boundary": boundary}
text = json.dumps(line)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
eng.close()
