"""The case table of the worklist digest (crdt_awset_digest_idx_async), shared by
tests/test_digest_idx_model.py (CPU) and tests/test_gpu_digest_idx.py (GPU).

Deterministic and hand-built: no RNG, every boundary is a named case.  The
kernels (csrc/digest_idx.hip) work in these units, read from that file so that a
retuned bound moves the cases with it:
  K_WAVE   kDigIdxWave: live entries + tombstones one wavefront takes at most; a
           document above it is walked by one 256-thread workgroup,
  K_STEP   128 positions per step of the wave kernel (a lane takes a pair),
  K_PASS   2 * kDigIdxJ * kDigIdxNT positions per step of the workgroup,
  K_GRID   workgroups of the largest grid (256 CUs x 8); K_GRID_WAVES = 4 x that
           wavefronts: a longer list takes the wave kernel's grid-stride loop a
           second time,
  block_per(n_max)  list entries per workgroup step of the block kernel, the launch's
           own formula: n_max spread over K_GRID workgroups, 1 ... kDigIdxNT.  A list
           of at most K_GRID entries gives every large document a workgroup of its
           own; the "mixed" cases put several of them into one step, and into the
           second step of one workgroup.
A case is a resident replica (state, tombs or None), a list and its length word;
both modes run every case (PLACE from the reference select of the same list),
except the ones marked gather_only.
"""

import collections
import os
import re

import numpy as np

from crdtgpu.batch import AWSetBatch, Replica, TombBatch
from helpers import PKG, batch_of
from test_replica_model import replica_select_ref

U32, U64 = np.uint32, np.uint64
M64 = 2 ** 64 - 1


def _kernel_constant(name):
    src = open(os.path.join(PKG, "csrc", "digest_idx.hip")).read()
    return int(re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, src).group(1))


K_WAVE = _kernel_constant("kDigIdxWave")
K_NT = _kernel_constant("kDigIdxNT")
K_J = _kernel_constant("kDigIdxJ")
K_STEP = 128
K_PASS = 2 * K_J * K_NT
K_GRID = 256 * 8
K_GRID_WAVES = K_GRID * 4
LADDER = [0, 1, 2, 63, 64, 65, 127, 128, 129]
BLOCK_ODD = 2 * K_PASS + 333  # three passes of the workgroup, no multiple of 256
N_MANY = 20000
N_MIXED = 5000
# the large documents of the "mixed" replica: (document, live entries, live tombstones)
MIXED_BIG = [(99, K_WAVE + 1, 0), (100, K_WAVE - 50, 77), (101, 2 * K_WAVE + 5, 3), (2001, K_WAVE + 9, 0),
             (2002, 7, K_WAVE + 1)]
N_TURN = K_GRID * K_NT + 2 * K_NT  # a list of two more steps than the grid has workgroups at the largest step


def block_per(n_max):
    """List entries per workgroup step of digest_idx_block_kernel (launch_digest_idx, 256 CUs)."""
    return min((n_max + K_GRID - 1) // K_GRID, K_NT)


Case = collections.namedtuple("Case", "name state tombs idx n_idx n_max shift gather_only")

_made = {}


def _once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


# ------------------------------------------------------------------ builders

def _column(sizes, slack, fill, R, salt):
    """(offsets, counts, keys, actors, counters): document d holds sizes[d] generated
    entries and `slack` more slots, zeros or the entries that would continue it."""
    sizes = np.asarray(sizes, np.int64)
    caps = sizes + slack
    offsets = np.zeros(len(sizes) + 1, U32)
    np.cumsum(caps, out=offsets[1:])
    total = int(offsets[-1])
    keys, actors, counters = np.zeros(total, U64), np.zeros(total, U32), np.zeros(total, U64)
    for d, n in enumerate(sizes.tolist()):
        m = n + slack if fill == "cont" else n
        i = np.arange(m, dtype=U64)
        o = int(offsets[d])
        keys[o:o + m] = (i + U64((d + 1) << 32) + U64(salt)) * U64(0x9E3779B97F4A7C15)  # odd multiplier: distinct
        actors[o:o + m] = (i % U64(R)).astype(U32)
        counters[o:o + m] = i * U64(0x100000001B3) + U64(d + 1)
    return offsets, sizes.astype(U32), keys, actors, counters


def make_replica(R, ent_sizes, tomb_sizes, vvs, slack=0, fill="zeros", counts=False):
    """(AWSetBatch, TombBatch) of generated documents; slack > 0 implies counts."""
    o, c, k, a, x = _column(ent_sizes, slack, fill, R, 0)
    vv = np.array(vvs, U64).reshape(-1)
    st = AWSetBatch(R, o, k, a, x, vv, counts=c if (counts or slack) else None)
    o, c, k, a, x = _column(tomb_sizes, slack, fill, R, 0x5151)
    tb = TombBatch(o, k, a, x, c if (counts or slack) else None)
    return st, tb


# ------------------------------------------------------------------ the main replica

MAIN_R = 3
# (name, live entries, live tombstones): the ladder of entry counts with the ladder of tomb
# counts rotated against it, the wave bound from both sides, and the block path
MAIN_DOCS = ([("ladder%d" % n, n, LADDER[(i + 4) % len(LADDER)]) for i, n in enumerate(LADDER)]
             + [("wave-1", K_WAVE - 1, 0), ("wave", K_WAVE, 0), ("wave+1", K_WAVE + 1, 0),
                ("wave_with_tombs", K_WAVE - 1, 1),       # entries + tombstones == the bound: still the wave's
                ("under_but_sum_over", K_WAVE - 100, 129),  # entries under the bound, the sum above it
                ("block_odd", BLOCK_ODD, 65),
                ("tombs_over", 1, K_WAVE + 5),            # the tombstones alone above the bound
                ("empty_zero_clock", 0, 0)])
MAIN_NAMES = [n for n, _, _ in MAIN_DOCS]


def _main_vvs():
    vvs = []
    for d, (name, _, _) in enumerate(MAIN_DOCS):
        vvs.append([0, 0, 0] if name == "empty_zero_clock" else [d + 1, 0, (d << 40) + 7])  # a zero word between
    return vvs


def main_replica(layout="packed"):
    """The same live state in the layouts: packed (counts NULL), counts (== the slots),
    slack_zeros (3 zero slots behind every document: odd and even starts change
    places), slack_cont (2 slots holding the entries that would continue it)."""
    def make():
        kw = dict(packed={}, counts=dict(counts=True), slack_zeros=dict(slack=3, fill="zeros"),
                  slack_cont=dict(slack=2, fill="cont"))[layout]
        return make_replica(MAIN_R, [e for _, e, _ in MAIN_DOCS], [t for _, _, t in MAIN_DOCS], _main_vvs(), **kw)
    return _once(("main", layout), make)


def empty_tombs(n_docs):
    return TombBatch(np.zeros(n_docs + 1, U32), np.zeros(1, U64), np.zeros(1, U32), np.zeros(1, U64),
                     np.zeros(n_docs, U32))


def clock_replica(R):
    """Four documents: an all-zero clock over two entries; zero words between non-zero
    ones; every word set; an empty document with only the last word set."""
    def make():
        between = [0] * R
        between[0], between[R - 1] = 5, 2 ** 63
        full = [(r + 1) * 0x0101010101010101 & M64 for r in range(R)]
        last = [0] * R
        last[R - 1] = M64
        return make_replica(R, [2, 3, 1, 0], [0, 1, 0, 0], [[0] * R, between, full, last])
    return _once(("clock", R), make)


def values_replica():
    """Keys 0, 2^63, 2^64 - 1; counters 2^32 - 1, 2^32, 2^63, 2^64 - 1; actors 0 and R - 1."""
    def make():
        R = 5
        docs = [([(0, 0, 2 ** 32 - 1), (7, R - 1, 2 ** 32), (2 ** 63, R - 1, 2 ** 63), (M64, 0, M64)],
                 [M64, 0, 2 ** 32, 0, 2 ** 63]),
                ([(M64, R - 1, 2 ** 32 - 1)], [0, 0, 0, 0, 1]),
                ([(0, 0, M64)], [2 ** 32 - 1, 0, 0, 0, 0])]
        tombs = [[(0, R - 1, M64), (M64, 0, 2 ** 32)], [], [(2 ** 63, 0, 2 ** 63)]]
        return batch_of(R, docs), TombBatch.from_lists(tombs)
    return _once("values", make)


def many_replica():
    """N_MANY one-entry documents, every third with one tombstone."""
    def make():
        n = N_MANY
        return make_replica(2, [1] * n, [1 if d % 3 == 0 else 0 for d in range(n)],
                            [[d + 1, 0] for d in range(n)])
    return _once("many", make)


def mixed_replica():
    """N_MIXED documents of 0 ... 3 entries (every fifth with a tombstone) with MIXED_BIG among them."""
    def make():
        ents = [d % 4 for d in range(N_MIXED)]
        tmbs = [1 if d % 5 == 0 else 0 for d in range(N_MIXED)]
        for d, e, t in MIXED_BIG:
            ents[d], tmbs[d] = e, t
        return make_replica(2, ents, tmbs, [[d + 1, d % 3] for d in range(N_MIXED)])
    return _once("mixed", make)


def turn_list():
    """N_TURN entries cycling over the mixed replica (GATHER: repeats), with two large
    documents put into the first entries of step K_GRID, the second step of workgroup 0."""
    idx = (np.arange(N_TURN) % N_MIXED).astype(U32)
    idx[K_GRID * K_NT + 5], idx[K_GRID * K_NT + 6] = 2001, 99
    return idx


# ------------------------------------------------------------------ the table

def _u32(x):
    return np.asarray(x, U32).reshape(-1)


def cases():
    def make():
        out = []

        def add(name, st, tb, idx, n_idx="len", n_max=None, shift=False, gather_only=False):
            idx = _u32(idx)
            n_max = len(idx) if n_max is None else n_max
            out.append(Case(name, st, tb, idx, len(idx) if n_idx == "len" else n_idx, n_max, shift, gather_only))

        st, tb = main_replica()
        n = st.n_docs
        asc = np.arange(n)
        add("list_empty", st, tb, asc, n_idx=0)  # *n_idx == 0 over a list that names everything
        add("list_first", st, tb, [0])
        add("list_last", st, tb, [n - 1])
        add("list_ascending", st, tb, asc)
        add("list_descending", st, tb, asc[::-1])
        add("list_every_other", st, tb, asc[::2])
        add("list_repeat", st, tb, [5, 14, 5, 5, 14, 3], gather_only=True)
        add("list_n_idx_null", st, tb, asc[::-1], n_idx=None)
        add("list_prefix", st, tb, asc[::-1], n_idx=4)  # *n_idx below n_max: the rest of the list is not read as listed
        add("tombs_null", st, None, asc)
        add("tombs_all_empty", st, empty_tombs(n), asc)
        for layout in ("counts", "slack_zeros", "slack_cont"):
            s2, t2 = main_replica(layout)
            add("layout_" + layout, s2, t2, asc[::-1])
        add("layout_shifted", st, tb, asc, shift=True)  # every array one element past its alignment
        s2, t2 = main_replica("slack_zeros")
        add("layout_shifted_slack", s2, t2, asc[::-1], shift=True)
        for R in (1, 2, 3, 5, 64):
            s2, t2 = clock_replica(R)
            add("clock_R%d" % R, s2, t2, [3, 0, 2, 1])
        s2, t2 = values_replica()
        add("values", s2, t2, [2, 1, 0])
        s2, t2 = many_replica()
        add("many", s2, t2, np.arange(N_MANY))
        s2, t2 = mixed_replica()
        add("block_shared_step", s2, t2, np.arange(N_MIXED))  # several large documents in one workgroup step
        add("block_second_turn", s2, t2, turn_list(), gather_only=True)  # ... and in a workgroup's second step
        return out
    return _once("cases", make)


def case(name):
    return next(c for c in cases() if c.name == name)


def listed(c):
    """The list entries the call takes: idx[0 .. min(*n_idx, n_max))."""
    n = c.n_max if c.n_idx is None else min(c.n_idx, c.n_max)
    return c.idx[:n]


def place_sub(c):
    """(state, tombs or None) of the PLACE form: the reference select of the same list,
    n_max documents (the ones at or past *n_idx empty)."""
    def make():
        rep = Replica(c.state, c.tombs, 0, None)
        sub = replica_select_ref(rep, c.idx, n_idx=c.n_idx, n_out=c.n_max).rep
        return sub.state, (sub.tombs if c.tombs is not None else None)
    return _once(("place", c.name), make)
