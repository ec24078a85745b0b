"""Shared by tests/test_replica_repack_model.py (CPU) and
tests/test_gpu_replica_repack.py: the deterministic case table of
crdt_replica_repack_async (include/crdtgpu.h).  No RNG decides an edge: every size
and every policy below is written out, and random generators only fill documents
whose sizes do not matter (the select and scatter forms of
tests/test_replica_model.py, taken over as they are).

A case is a Case: host Replicas (sub None: the select mapping), idx / n_idx /
n_out as the select or scatter form takes them, the two policies as (min_spare,
num, shift, align) or None, and the slot limits (None: exactly the capacity
totals).  The kernels work in these units (csrc/replica_repack.hip), and the cases
are sized around them:
  kRpkScanChunk   = 1,024 output documents per workgroup of the offset scan,
  kRpkPartStep    = 1,024 partial sums per step of the one-workgroup partials scan,
  kRpkGatherChunk = 2,048 output positions per gather step,
  kRpkRun         = 1,024 documents of a gather chunk staged in LDS at most.
"""

import collections

import numpy as np

from sources_cases import make_replica
from test_replica_model import big_replica, scatter_cases, select_cases, seq_list, tiny_replicas

U32, U64 = np.uint32, np.uint64
ONES32 = 2 ** 32 - 1
K_SCAN, K_PART, K_GATHER, K_RUN = 1024, 1024, 2048, 1024

Case = collections.namedtuple("Case", "rep sub idx n_idx n_out er tr entry_slots tomb_slots")

# the rounds' policy (tests/test_replica_repack_model.py asserts that it is enough): twice the
# live count plus a constant
ROUND_SPARE = 6
ROUND_ROOM = (ROUND_SPARE, 1, 0, 1)

_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def cap_py(room, n):
    """The header's expression restated: round_up(n + max(min_spare, (n * num) >> shift),
    align), saturated at 2^32 - 1.  (The product asks the library: Headroom.capacity.)"""
    if room is None:
        return int(n)
    ms, num, shift, align = room
    v = int(n) + max(ms, (int(n) * num) >> shift)
    return min(-(-v // align) * align, ONES32)


def caps_py(room, counts):
    """cap_py over a count vector, as Python ints (no saturation lost, none added)."""
    c = np.asarray(counts, U32)
    vals, inv = np.unique(c, return_inverse=True)
    return np.array([cap_py(room, int(v)) for v in vals], object)[inv] if len(c) else np.zeros(0, object)


def _sel(rep, er, tr, idx=None, n_idx=None, n_out=None, entry_slots=None, tomb_slots=None):
    return Case(rep, None, idx, n_idx, rep.n_docs if n_out is None else n_out, er, tr, entry_slots, tomb_slots)


def _sct(rep, sub, idx, er, tr, n_idx=None):
    return Case(rep, sub, idx, n_idx, rep.n_docs, er, tr, None, None)


def sized_replica(sizes, tsizes, R=3, **kw):
    """Documents of exactly sizes[d] entries and tsizes[d] tombstones."""
    docs = [(seq_list(100000 * d, ne, R), seq_list(100000 * d + 1, nt, R), [d + 1] * R)
            for d, (ne, nt) in enumerate(zip(sizes, tsizes))]
    return make_replica(R, docs, **kw)


POLICY_SIZES = [0, 1, 63, 64, 65, 3, 7, 8, 9, 15, 16, 17, 2]
POLICY_TSIZES = [1, 0, 7, 8, 9, 2, 3, 1, 0, 4, 5, 6, 63]

# name -> (entry policy, tombstone policy) over POLICY_SIZES
POLICIES = {
    "min0": ((0, 0, 0, 1), (0, 0, 0, 1)),
    "min1": ((1, 0, 0, 1), (7, 0, 0, 1)),
    "min7": ((7, 0, 0, 1), (1, 0, 0, 1)),
    "half": ((0, 1, 1, 1), (0, 3, 2, 1)),
    "three-quarters": ((0, 3, 2, 1), (0, 1, 1, 1)),
    "min-above-and-below": ((7, 1, 1, 1), (2, 1, 1, 1)),  # 7 > n/2 for n <= 9, below it for n >= 63
    "align2": ((1, 1, 1, 2), (1, 0, 0, 2)),
    "align8": ((1, 0, 0, 8), (0, 1, 1, 8)),    # n = 7: 7 + 1 on a multiple of 8; n = 8: one above
    "align16": ((1, 0, 0, 16), (0, 1, 1, 16)),  # n = 15 on the multiple, n = 16 one above
    "align64": ((1, 1, 0, 64), (1, 0, 0, 64)),  # n = 63: 63 + 63 -> 128; n = 64 -> 128; n = 65 -> 192
    "entry-null": (None, (1, 1, 0, 2)),
    "tomb-null": ((1, 1, 0, 2), None),
    "both-null": (None, None),
}

# policies handed round-robin to the select and scatter forms of test_replica_model.py
ROTATION = [((2, 1, 0, 1), (1, 1, 0, 1)), ((1, 1, 1, 2), (1, 0, 0, 2)), (None, (3, 0, 0, 1)), ((0, 3, 2, 16), None),
            ((1, 0, 0, 1), (0, 0, 0, 1)), (None, None), ((0, 1, 0, 8), (2, 0, 0, 64))]


def gather_sizes():
    """Entry sizes under the doubling policy (0, 1, 0, 1): cap = 2n.
      doc 0: 1,500 live in [0, 3,000): the chunk boundary 2,048 lies in its slack;
      doc 1: 1,500 live from 3,000: the boundary 4,096 lies in its live prefix;
      doc 2: 72 live, 144 slots from 6,000: document 3 starts exactly on 6,144;
      doc 3: 4,096 live, 8,192 slots from 6,144: the chunks [10,240, 12,288) and
             [12,288, 14,336) lie wholly in its slack, and document 4 starts on 14,336;
      then 3,000 documents of 0 or 1 entries (0 or 2 slots): about 2,048 documents in
      one chunk, more than the LDS run holds; then a 5-entry tail."""
    return [1500, 1500, 72, 4096] + [d % 2 for d in range(3000)] + [5]


def cases():
    """name -> Case of every small case."""
    def make():
        out = {}
        # --- policy edges: compaction of one replica under every policy
        pol = sized_replica(POLICY_SIZES, POLICY_TSIZES, slack=2, with_counts=True,
                            garbage=np.random.default_rng(31), doc_actor=[d % 3 for d in range(len(POLICY_SIZES))])
        for name, (er, tr) in POLICIES.items():
            out["pol-" + name] = _sel(pol, er, tr)
        out["pol-big-doc"] = _sel(sized_replica([3, 2 ** 20 + 1, 2], [1, 0, 2], R=1, with_counts=True), (0, 1, 0, 1),
                                  (1, 0, 0, 1))
        out["pol-saturate"] = _sel(sized_replica([3, 3, 3, 3], [1, 1, 1, 1], with_counts=True), (0, ONES32, 0, 1),
                                   (1, 0, 0, 1), entry_slots=64)
        # --- mapping: every select and scatter form of test_replica_model.py
        k = 0
        for name, (rep, idx, n_idx, n_out) in select_cases().items():
            er, tr = ROTATION[k % len(ROTATION)]
            out["sel-" + name] = _sel(rep, er, tr, idx, n_idx, n_out)
            k += 1
        for name, (rep, sub, idx, n_idx) in scatter_cases().items():
            er, tr = ROTATION[k % len(ROTATION)]
            out["sct-" + name] = _sct(rep, sub, idx, er, tr, n_idx)
            k += 1
        r3 = select_cases()["R3-layout0"][0]
        s3 = scatter_cases()["R3-tombs-both"][1]
        out["map-empty-beyond"] = _sel(r3, (2, 0, 0, 1), (1, 0, 0, 2), np.arange(8, dtype=U32) * U32(5), 3, 8)
        out["map-n_idx-above"] = _sel(r3, (2, 0, 0, 1), (1, 0, 0, 2), np.arange(8, dtype=U32) * U32(5), 12, 8)
        out["map-bad-index"] = _sel(r3, (1, 1, 0, 2), None, np.array([1, 300, 2], U32), None, 3)
        out["map-duplicate"] = _sct(r3, s3, np.array([7, 7, 299], U32), (1, 1, 0, 2), (1, 0, 0, 1), 3)
        # --- scan
        out["scan-2049"] = _sel(tiny_replicas(9100 + 2049, 2 * K_SCAN + 1, 1, R=2)[0], (1, 1, 0, 1), (0, 0, 0, 2))
        # --- gather
        gs = gather_sizes()
        out["gather-doubling"] = _sel(sized_replica(gs, [n % 3 for n in gs], R=2, with_counts=True), (0, 1, 0, 1),
                                      (1, 0, 0, 1))
        # align 1 and one spare slot: 2- to 5-entry documents start at both parities
        odd = [2, 3, 4, 5, 2, 2, 3, 3, 4] * 40
        out["gather-odd-starts"] = _sel(sized_replica(odd, [n - 2 for n in odd], R=2, slack=1, lead=1), (1, 0, 0, 1),
                                        (1, 0, 0, 1))
        # --- capacity: one kind one slot short, the other fitting exactly
        er, tr = (1, 1, 0, 2), (1, 0, 0, 2)
        te = sum(cap_py(er, n) for n in POLICY_SIZES)
        tt = sum(cap_py(tr, n) for n in POLICY_TSIZES)
        out["cap-entries-short"] = _sel(pol, er, tr, entry_slots=te - 1, tomb_slots=tt)
        out["cap-tombs-short"] = _sel(pol, er, tr, entry_slots=te, tomb_slots=tt - 1)
        return out
    return _once("cases", make)


def big_case(n=K_PART * K_SCAN + 1):
    """n documents of 0 or 1 entries and tombstones (big_replica), compacted with the
    doubling policy and min_spare = 0, so an empty document owns nothing: at the
    default n, 2^20 + 1 documents and 1,025 partial sums -- one past a partials step."""
    return _sel(big_replica(n), (0, 1, 0, 1), (0, 0, 0, 2))
