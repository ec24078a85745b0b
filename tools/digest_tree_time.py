#!/usr/bin/env python3
"""Time the digest tree beside what it stands in for, at 1,048,576 documents x 64
entries (tools/digest_idx_time.py's protocol: every comparison runs in three
interleaved rounds, A B .. A B .. A B; a round is 5 warm-up calls and 25 timed
ones, each between its own pair of device events; per call the three round medians
and their median).

  build     crdt_digest_tree_async, upper levels fused (the default) | one launch
            per level (crdt_ctx_set_option "digest_tree_fuse" 0, a second context)
            | crdt_awset_digest_async of the replica the array digests | a device
            copy of the 16 MB array
  descent   for 0 / 0.01 % / 0.1 % / 1 % / 5 % differing documents, random and
            clustered: the whole descent chained on the device (children + diff per
            level, each level's idx_out / n_out the next one's list, no download;
            the lists' room is the case's largest level) | the Engine's driver, which
            reads the 4-byte n_out per level (host wall clock around it) |
            crdt_digest_diff_async of the same two arrays; the bytes a peer ships
            (256 B per parent asked) beside the flat 16 B per document

Prints one JSON line (and writes it to the file named by the first argument).
GPU box only.

    python tools/digest_tree_time.py [out.json]
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
from crdtgpu.batch import CompareBuffers, DigestTreeBuffers, OutBuffers  # noqa: E402

WARMUP, STEPS, ROUNDS = 5, 25, 3
N, R, E = 1 << 20, 2, 64
dev = torch.device("cuda:0")
eng = crdtgpu.Engine(0)
unfused = crdtgpu.Engine(0)
unfused.set_option("digest_tree_fuse", 0)
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


def wall(call):
    for _ in range(WARMUP):
        call()
    got = []
    for _ in range(STEPS):
        s.synchronize()
        t0 = time.perf_counter()
        call()
        s.synchronize()
        got.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(got)


def interleaved(calls, clock=timed):
    got = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, c in calls.items():
            got[k].append(round(clock(c), 4))
    return {k: {"rounds_ms": v, "ms": statistics.median(v)} for k, v in got.items()}


def ratio(res, a, b):
    return round(res[a]["ms"] / res[b]["ms"], 3)


# ---- the replica and its digest array
A, B = OutBuffers(N, R, N * E, device=dev), OutBuffers(N, R, N * E, device=dev)
eng.gen_pair_async(0xC0FFEE, N, A, B, stream=s)
eng.sync(s)
del B
cst = A.as_batch().c()
mine = torch.empty(2 * N, dtype=torch.int64, device=dev)
eng.digest_async(cst, mine, stream=s)
eng.sync(s)
eng.reserve(N)
unfused.reserve(N)
tm = DigestTreeBuffers(N, dev)
copy_dst = torch.empty_like(mine)

# ---- 1. the build
build = interleaved({
    "tree_fused": lambda: eng.digest_tree_async(mine, N, tm.tree, stream=s),
    "tree_one_launch_per_level": lambda: unfused.digest_tree_async(mine, N, tm.tree, stream=s),
    "full_digest": lambda: eng.digest_async(cst, mine, stream=s),
    "device_copy_16MB": lambda: copy_dst.copy_(mine),
})
eng.sync(s)
unfused.sync(s)
host_tree = crdtgpu.digest_tree_host(mine.cpu().numpy().view(np.uint64))
tree_exact = bool((tm.tree.cpu().numpy().view(np.uint64).reshape(-1, 2) == host_tree).all())
unfused.digest_tree_async(mine, N, tm.tree, stream=s)
unfused.sync(s)
tree_exact = tree_exact and bool((tm.tree.cpu().numpy().view(np.uint64).reshape(-1, 2) == host_tree).all())
eng.digest_tree_async(mine, N, tm.tree, stream=s)
eng.sync(s)
del A, copy_dst
torch.cuda.empty_cache()


# ---- 2. descents
def cases():
    rng = np.random.default_rng(0x7EE5)
    out = [("0", np.zeros(0, np.int64))]
    for name, share in (("0.01 %", 1e-4), ("0.1 %", 1e-3), ("1 %", 1e-2), ("5 %", 5e-2)):
        k = int(round(N * share))
        out.append((name + " random", np.sort(rng.choice(N, size=k, replace=False))))
        start = int(rng.integers(0, N - k))
        out.append((name + " clustered", np.arange(start, start + k)))
    return out


theirs = mine.clone()
tt = DigestTreeBuffers(N, dev)
flat = CompareBuffers(N, device=dev)
cflat = flat.c()
descents = []
for name, docs in cases():
    theirs.copy_(mine)
    if len(docs):
        d = torch.from_numpy(docs).to(dev)
        theirs[2 * d[d % 2 == 0]] ^= 1  # ELEMENTS
        theirs[2 * d[d % 2 == 1] + 1] ^= 1  # STATE
    eng.digest_tree_async(theirs, N, tt.tree, stream=s)
    asked = [len(np.unique(docs // 16 ** l)) for l in range(tm.L, 0, -1)] if len(docs) else [1]
    cap = max(max(asked), len(docs), 16)
    bufs = DigestTreeBuffers(N, dev, cap=cap)
    bufs.tree = tm.tree
    peer_packed = torch.empty(32 * cap, dtype=torch.int64, device=dev)

    def chained():
        lvl = tm.L
        parents, n_parents, n_max, k = None, None, 1, 0
        while lvl >= 1:
            peer, n_level = tt.level(lvl - 1, theirs)
            eng.digest_tree_children_async(peer, n_level, bufs.packed, parents=parents, n_parents=n_parents,
                                           n_max=n_max, stream=s)
            own, _ = bufs.level(lvl - 1, mine)
            eng.digest_tree_diff_async(own, n_level, bufs.packed, bufs.idx[k], bufs.n_out[k], parents=parents,
                                       n_parents=n_parents, n_max=n_max, leaf=lvl == 1, flags_out=bufs.flags,
                                       out_max=cap, summary=bufs.summary, stream=s)
            parents, n_parents, n_max, k, lvl = bufs.idx[k], bufs.n_out[k], min(cap, tm.nodes[lvl - 1]), k ^ 1, lvl - 1
        return parents, n_parents

    def fetch(level, parents, k):
        peer, n_level = tt.level(level - 1, theirs)
        eng.digest_tree_children_async(peer, n_level, peer_packed, parents=parents, n_max=k, stream=s)
        return peer_packed

    got = {}

    def driver():
        got["r"] = eng.digest_tree_descend(mine, bufs, fetch, stream=s)

    def flat_diff():
        eng.digest_diff_async(mine, theirs, N, cflat, stream=s)

    work, n_work = chained()
    flat_diff()
    eng.sync(s)
    k = int(n_work[0])
    nw = int(flat.n_work[0])
    exact = k == nw == len(docs) and bool(torch.equal(work[:k], flat.worklist[:nw]))
    exact = exact and bool(torch.equal(bufs.flags[:k], flat.flags[flat.worklist[:nw].long()]))
    driver()
    w, f, kd, fetched = got["r"]
    exact = exact and kd == len(docs) and bool(torch.equal(w[:kd], flat.worklist[:nw])) and fetched == 256 * sum(asked)
    res = interleaved({"descent_chained_on_device": chained, "flat_digest_diff": flat_diff})
    res.update(interleaved({"descent_driver_wall": driver, "flat_digest_diff_wall": flat_diff}, clock=wall))
    descents.append({"case": name, "differing": int(len(docs)), "parents_asked_per_level": asked, "exact": exact,
                     "bytes_fetched": fetched, "flat_bytes": 16 * N, "bytes_over_flat": round(fetched / (16 * N), 5),
                     "times": res,
                     "chained_over_flat": ratio(res, "descent_chained_on_device", "flat_digest_diff"),
                     "driver_wall_over_flat_wall": ratio(res, "descent_driver_wall", "flat_digest_diff_wall")})
    del bufs, peer_packed
    torch.cuda.empty_cache()

line = {
    "what": "crdt_digest_tree_async (upper levels fused, and one launch per level) beside crdt_awset_digest_async of the "
            "replica and a device copy of the 16 MB digest array; whole descents (children + diff per level) chained on "
            "the device and through Engine.digest_tree_descend, which reads 4 bytes per level, beside "
            "crdt_digest_diff_async of the same arrays; bytes a peer ships per descent beside 16 B per document; same "
            "run, three interleaved rounds per comparison; measured once, on one box",
    "warmup": WARMUP, "steps": STEPS, "rounds": ROUNDS,
    "statistic": "median over the rounds of the per-round median of device-event times (wall: host clock)",
    "box": box_identity(dev), "n_docs": N, "R": R, "entries_per_doc": E, "levels": tm.L, "level_nodes": tm.nodes,
    "tree_bytes": 16 * tm.n_nodes, "tree_equals_host": tree_exact,
    "build": {"times": build, "fused_over_unfused": ratio(build, "tree_fused", "tree_one_launch_per_level"),
              "tree_over_full_digest": ratio(build, "tree_fused", "full_digest"),
              "tree_over_copy": ratio(build, "tree_fused", "device_copy_16MB")},
    "descents": descents,
}
text = json.dumps(line)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
eng.close()
unfused.close()
