#!/usr/bin/env python3
"""Time the scatter (crdt_awset_scatter_async) and the sparse anti-entropy round
it closes, beside the calls a caller would otherwise make, on the same inputs in
the same run: 5 warm-up launches, then 25 timed ones, each between its own pair
of device events; the median is reported (and the minimum).

  (a) scatter at the "mostly converged" shape: state = the config-2 exchange's
      out_ab (1,048,576 docs at capacity offsets), sub = the documents of the
      worklist of compare(out_ab, out_ba), selected from out_ab, put back;
      against the identity select (compaction) of the same batch and three
      hipMemcpyAsync (one per column) of the same live bytes
  (b) the sparse round at that shape: compare, select x2, exchange of the
      sub-batches, scatter x2 -- against the full exchange of the same inputs
  (c) the same two at a 5 %-differing shape: config-2 A against a copy of A in
      which every 20th document is B's

The sizes of the sub-batches (n_work and their live entries) are read back once
while setting up; the timed round itself runs with the worklist and n_work on
the device.  Records the box (PCI function, clocks as the driver shows them,
measured shader clock).  Prints one JSON line (and writes it to the file named
by the first argument).  GPU box only.

    python tools/scatter_time.py [out.json]
    python tools/scatter_time.py --kernels

--kernels: only 30 identity selects and 30 scatters of shape (a), untimed, for a
kernel trace of its own (per-kernel times of the two offset scans).
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "go-crdt-playground_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import crdtgpu  # noqa: E402
from bench import box_identity  # noqa: E402
from crdtgpu import abi  # noqa: E402
from crdtgpu.batch import CompareBuffers, OutBuffers  # noqa: E402

WARMUP, STEPS = 5, 25
SEED = 0x5EED
KERNELS_ONLY = len(sys.argv) > 1 and sys.argv[1] == "--kernels"
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


def live_entries(batch, docs=None):
    c = batch.counts.to(torch.int64) if batch.counts is not None else \
        (batch.offsets[1:] - batch.offsets[:-1]).to(torch.int64)
    return int((c if docs is None else c[docs]).sum())


class Round:
    """Buffers and prebuilt ctypes structs of one sparse round over batches a, b."""

    def __init__(self, a, b, max_doc_entries=None):
        self.n, self.R = a.n_docs, a.R
        self.promise = max_doc_entries
        n, R = self.n, self.R
        eng.reserve(n)
        self.res = CompareBuffers(n, device=dev)
        self.ca, self.cb, self.cr = a.c(), b.c(), self.res.c()
        eng.compare_async(self.ca, self.cb, self.cr, stream=s)
        eng.sync(s)
        self.flags, self.summary, work = self.res.numpy()
        self.n_work = int(len(work))
        docs = torch.from_numpy(work.astype("int64")).to(dev)
        self.la, self.lb = live_entries(a), live_entries(b)
        self.sla, self.slb = live_entries(a, docs), live_entries(b, docs)
        m = max(self.n_work, 1)
        self.sa = OutBuffers(m, R, max(self.sla, 1), device=dev)
        self.sb = OutBuffers(m, R, max(self.slb, 1), device=dev)
        self.xa = OutBuffers(m, R, self.sa.slots + self.sb.slots, device=dev)
        self.xb = OutBuffers(m, R, self.sa.slots + self.sb.slots, device=dev, shared_keys=self.xa)
        # a merged document holds at most both sides' entries
        self.na = OutBuffers(n, R, self.la + self.slb, device=dev)
        self.nb = OutBuffers(n, R, self.lb + self.sla, device=dev)
        self.csa, self.csb, self.cxa, self.cxb = self.sa.c(), self.sb.c(), self.xa.c(), self.xb.c()
        self.bsa, self.bsb = self.sa.as_batch().c(), self.sb.as_batch().c()
        self.bxa, self.bxb = self.xa.as_batch().c(), self.xb.as_batch().c()
        self.cna, self.cnb = self.na.c(), self.nb.c()

    def set_promise(self):
        if self.promise:
            eng.set_max_doc_entries(self.promise)
        else:
            eng.set_max_doc_entries()

    def compare(self):
        eng.compare_async(self.ca, self.cb, self.cr, stream=s)

    def selects(self):
        w, nw = self.res.worklist, self.res.n_work
        eng.select_async(self.ca, self.csa, idx=w, n_idx=nw, n_out=self.n_work, out_slots=self.sa.slots, stream=s)
        eng.select_async(self.cb, self.csb, idx=w, n_idx=nw, n_out=self.n_work, out_slots=self.sb.slots, stream=s)

    def sub_exchange(self):
        eng.exchange_async(self.bsa, self.bsb, self.cxa, self.cxb, stream=s)

    def scatters(self):
        w, nw = self.res.worklist, self.res.n_work
        eng.scatter_async(self.ca, self.bxa, w, self.cna, n_idx=nw, out_slots=self.na.slots, stream=s)
        eng.scatter_async(self.cb, self.bxb, w, self.cnb, n_idx=nw, out_slots=self.nb.slots, stream=s)

    def whole(self):
        self.compare()
        self.selects()
        self.sub_exchange()
        self.scatters()

    def row(self, name, full_exchange_ms):
        self.set_promise()
        t_cmp, t_sel = timed(self.compare), timed(self.selects)
        t_xch, t_sct = timed(self.sub_exchange), timed(self.scatters)
        t_all = timed(self.whole)
        return {
            "shape": name, "n_docs": self.n, "n_work": self.n_work,
            "share_of_documents_differing": round(self.n_work / self.n, 4),
            "live_entries_a": self.la, "live_entries_b": self.lb,
            "sub_live_entries_a": self.sla, "sub_live_entries_b": self.slb,
            "summary_keys_dots_aahead_bahead_selected": self.summary.tolist(),
            "compare_ms_median": t_cmp[0], "select_x2_ms_median": t_sel[0], "sub_exchange_ms_median": t_xch[0],
            "scatter_x2_ms_median": t_sct[0],
            "sparse_round_ms_median": t_all[0], "sparse_round_ms_min": t_all[1],
            "full_exchange_ms_median": full_exchange_ms[0], "full_exchange_ms_min": full_exchange_ms[1],
            "sparse_round_over_full_exchange": round(t_all[0] / full_exchange_ms[0], 4),
            "winner": "sparse round" if t_all[0] < full_exchange_ms[0] else "full exchange",
        }


def full_exchange(a, b, slots, max_doc_entries=None):
    """Median / min ms of exchange(a, b) into fresh outputs (one shared key column, as bench.py times it)."""
    if max_doc_entries:
        eng.set_max_doc_entries(max_doc_entries)
    else:
        eng.set_max_doc_entries()
    o1 = OutBuffers(a.n_docs, a.R, slots, device=dev)
    o2 = OutBuffers(a.n_docs, a.R, slots, device=dev, shared_keys=o1)
    ca, cb, c1, c2 = a.c(), b.c(), o1.c(), o2.c()
    return timed(lambda: eng.exchange_async(ca, cb, c1, c2, stream=s))


# the box: identity and the streaming copy rate in this run (2 GiB: 8x the Infinity Cache)
copy_gbs = sclk = None
box = None
if not KERNELS_ONLY:
    x = torch.empty(2 << 30, dtype=torch.uint8, device=dev)
    y = torch.empty(2 << 30, dtype=torch.uint8, device=dev)
    x.fill_(0x5A)
    torch.cuda.synchronize()
    copy_gbs = eng.bw_probe(abi.CRDT_PROBE_COPY, x, y, x.numel(), 10)
    sclk = eng.clock_probe()
    box = box_identity(dev)
    del x, y
    torch.cuda.empty_cache()

# config-2 pair and its exchange
n = 1 << 20
A = OutBuffers(n, 2, n * 64, device=dev)
B = OutBuffers(n, 2, n * 64, device=dev)
eng.gen_pair_async(SEED, n, A, B, stream=s)
eng.sync(s)
o1 = OutBuffers(n, 2, 2 * n * 64, device=dev)
o2 = OutBuffers(n, 2, 2 * n * 64, device=dev)
eng.set_max_doc_entries(64)
eng.exchange_async(A.as_batch(), B.as_batch(), o1, o2, stream=s)
eng.sync(s)
eng.set_max_doc_entries()
b1, b2 = o1.as_batch(), o2.as_batch()

# (a) scatter at the mostly converged shape
rnd = Round(b1, b2)
rnd.selects()
eng.sync(s)
live1 = rnd.la
put = OutBuffers(n, 2, live1, device=dev)  # a document put back unchanged: the total stays
cput = put.c()
w, nw = rnd.res.worklist, rnd.res.n_work


def scatter_a():
    eng.scatter_async(rnd.ca, rnd.bsa, w, cput, n_idx=nw, out_slots=live1, stream=s)


def identity_select():
    eng.select_async(rnd.ca, cput, n_out=n, out_slots=live1, stream=s)


if KERNELS_ONLY:
    for _ in range(WARMUP + STEPS):
        identity_select()
    for _ in range(WARMUP + STEPS):
        scatter_a()
    eng.sync(s)
    eng.close()
    print("kernels-only run done: %d identity selects, %d scatters (n_docs %d, n_work %d)"
          % (WARMUP + STEPS, WARMUP + STEPS, n, rnd.n_work))
    sys.exit(0)

sct_ms = timed(scatter_a)
idn_ms = timed(identity_select)
src = [o1.keys[:live1], o1.actors[:live1], o1.counters[:live1]]
dst = [put.keys[:live1], put.actors[:live1], put.counters[:live1]]


def d2d():
    for d_, s_ in zip(dst, src):
        d_.copy_(s_, non_blocking=True)  # hipMemcpyAsync device to device


cpy_ms = timed(d2d)
moved = 2 * live1 * 20
rows = [{
    "shape": "scatter at the mostly converged shape: the config-2 exchange's out_ab with the sub-batch of the "
             "worklist of compare(out_ab, out_ba) put back",
    "n_docs": n, "n_work": rnd.n_work, "live_entries": live1, "sub_live_entries": rnd.sla,
    "capacity_slots": o1.slots,
    "scatter_ms_median": sct_ms[0], "scatter_ms_min": sct_ms[1],
    "bytes_read_plus_written": moved, "scatter_gbs": round(moved / (sct_ms[0] * 1e-3) / 1e9, 1),
    "identity_select_ms_median": idn_ms[0], "identity_select_ms_min": idn_ms[1],
    "scatter_over_identity_select": round(sct_ms[0] / idn_ms[0], 4),
    "d2d_copy_same_live_bytes_ms_median": cpy_ms[0], "d2d_copy_ms_min": cpy_ms[1],
    "d2d_copy_gbs": round(moved / (cpy_ms[0] * 1e-3) / 1e9, 1),
    "scatter_over_d2d_copy": round(sct_ms[0] / cpy_ms[0], 4),
    "ms_at_probe_copy_rate": round(moved / (copy_gbs * 1e9) * 1e3, 4),
}]
del put, src, dst
torch.cuda.empty_cache()

# (b) the sparse round at that shape against the full exchange of out_ab and out_ba
full_ms = full_exchange(b1, b2, 2 * o1.slots)
torch.cuda.empty_cache()
rows.append(rnd.row("sparse round, mostly converged: out_ab against out_ba of the config-2 exchange", full_ms))
del rnd, o1, o2, b1, b2
torch.cuda.empty_cache()

# (c) 5 % differing: A against a copy of A in which every 20th document is B's
Q = OutBuffers(n, 2, n * 64, device=dev)
every = torch.arange(0, n, 20, device=dev)
for f, per in (("keys", 64), ("actors", 64), ("counters", 64), ("vv", 2)):
    q = getattr(Q, f)
    q.copy_(getattr(A, f))
    q.view(n, per)[every] = getattr(B, f).view(n, per)[every]
Q.offsets.copy_(A.offsets)
Q.counts.copy_(A.counts)
Q.counts[every] = B.counts[every]
torch.cuda.synchronize()
del B
torch.cuda.empty_cache()
pa = A.as_batch()
pq = Q.as_batch()
full_ms = full_exchange(pa, pq, 2 * n * 64, max_doc_entries=64)
torch.cuda.empty_cache()
rows.append(Round(pa, pq, max_doc_entries=64).row(
    "sparse round, 5 % differing: config-2 A against A with every 20th document replaced by B's", full_ms))

line = {"what": "crdt_awset_scatter_async beside the identity select and a device copy, and the sparse round "
                "(compare, select x2, sub-exchange, scatter x2) beside the full exchange; same inputs, same run; "
                "measured once, on one box",
        "warmup": WARMUP, "steps": STEPS, "statistic": "median of per-launch device-event times",
        "probe_copy_gbs": round(copy_gbs, 1), "sclk_mhz": round(sclk, 1), "box": box, "shapes": rows}
text = json.dumps(line)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
eng.close()
