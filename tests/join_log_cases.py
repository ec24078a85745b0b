"""Shared by tests/test_join_log_model.py (CPU) and tests/test_gpu_join_log.py:
join_log_ref, the expectation of crdt_awset_join_log_async /
crdt_awset_exchange_log_async (include/crdtgpu.h), and the case sets both files
draw from.

join_log_ref(dst, src) is the C oracle's join (oracle.join) and then diff_doc of
tests/test_diff_model.py on (dst, out), document by document, laid out as the call
lays it out: document d's removed list at dst.offsets[d], its upserted list at
src.offsets[d], the merged state at dst.offsets[d] + src.offsets[d].

A document is (entries [(key, actor, counter)], vv); counters and clock values stay
within 0..MAX_C so that tests/counter_maps.py can push the same cases up to the
64-bit edges.
"""

import random

import numpy as np

from crdtgpu.batch import AWSetBatch
from oracle import oracle
from test_compare_model import _live
from test_diff_model import ADDED, CLOCK, REMOVED, UPDATED, diff_doc

U8, U32, U64 = np.uint8, np.uint32, np.uint64
MAX_C = 9          # counters and clock values of every case here lie in 0..MAX_C
WAVE_MAX = 64      # kLogWaveMax: live entries per side on the wave path
LOG_WAVES = 4      # kLogWaves: wavefronts per workgroup of the wave path
LOG_DOCS = 8       # kLogDocs: documents one wavefront takes in turn
WINDOW = 1024      # kLogBlockNT * kLogBlockIPT: merged positions per step of the block path
LISTS = ("rem_keys", "rem_actors", "rem_counters", "ups_keys", "ups_actors", "ups_counters", "ups_kind")
PER_DOC = ("flags", "rem_offsets", "rem_counts", "ups_offsets", "ups_counts")


# ------------------------------------------------------------------ reference

class LogRef:
    """rc: the oracle's status; out: its join output (host OutBuffers); log: a dict shaped
    as MergeLogBuffers.numpy(), the columns zero outside the lists; rem_idx / ups_idx: the
    slots of the columns that hold a record (every document's live prefix of its list)."""

    def __init__(self, rc, out, log, rem_idx, ups_idx):
        self.rc, self.out, self.log, self.rem_idx, self.ups_idx = rc, out, log, rem_idx, ups_idx


def _slots_idx(offsets, counts):
    cnt = counts.astype(np.int64)
    st = offsets[:-1].astype(np.int64)
    return np.repeat(st, cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))


def log_of(dst, src, after):
    """The log of dst <- src given the merged batch `after`: diff_doc per document."""
    n, R = dst.n_docs, dst.R
    ds, ss = int(dst.offsets[-1]), int(src.offsets[-1])
    log = {"flags": np.zeros(n, U8), "summary": np.zeros(5, U32),
           "rem_offsets": np.asarray(dst.offsets, U32).copy(), "rem_counts": np.zeros(n, U32),
           "rem_keys": np.zeros(ds, U64), "rem_actors": np.zeros(ds, U32), "rem_counters": np.zeros(ds, U64),
           "ups_offsets": np.asarray(src.offsets, U32).copy(), "ups_counts": np.zeros(n, U32),
           "ups_keys": np.zeros(ss, U64), "ups_actors": np.zeros(ss, U32), "ups_counters": np.zeros(ss, U64),
           "ups_kind": np.zeros(ss, U8)}
    n_upd = 0
    for d in range(n):
        r, u, k = diff_doc(dst, after, d)
        f = (REMOVED if len(r[0]) else 0) | (ADDED if (k == ADDED).any() else 0) | (UPDATED if (k == UPDATED).any() else 0)
        if (np.asarray(dst.vv[d * R:(d + 1) * R]) != np.asarray(after.vv[d * R:(d + 1) * R])).any():
            f |= CLOCK
        log["flags"][d] = f
        o, m = int(dst.offsets[d]), len(r[0])
        assert o + m <= int(dst.offsets[d + 1])  # a removed entry was a dst entry
        log["rem_counts"][d] = m
        for col, v in zip(("rem_keys", "rem_actors", "rem_counters"), r):
            log[col][o:o + m] = v
        o, m = int(src.offsets[d]), len(u[0])
        assert o + m <= int(src.offsets[d + 1])  # an upserted entry was a src entry
        log["ups_counts"][d] = m
        for col, v in zip(("ups_keys", "ups_actors", "ups_counters", "ups_kind"), u + (k,)):
            log[col][o:o + m] = v
        n_upd += int((k == UPDATED).sum())
    fl = log["flags"]
    log["summary"][:] = [int(log["rem_counts"].sum()), int(log["ups_counts"].sum()), n_upd,
                         int(((fl & 7) != 0).sum()), int((fl != 0).sum())]
    return log


def join_log_ref(dst, src):
    dst, src = dst.numpy(), src.numpy()
    rc, out = oracle.join(dst, src)
    log = log_of(dst, src, out.as_batch())
    return LogRef(rc, out, log, _slots_idx(log["rem_offsets"], log["rem_counts"]),
                  _slots_idx(log["ups_offsets"], log["ups_counts"]))


def doc_lists(log, d):
    """([(key, actor, counter)] removed, [(key, actor, counter, kind)] upserted) of document d."""
    o, m = int(log["rem_offsets"][d]), int(log["rem_counts"][d])
    rem = list(zip(log["rem_keys"][o:o + m].tolist(), log["rem_actors"][o:o + m].tolist(),
                   log["rem_counters"][o:o + m].tolist()))
    o, m = int(log["ups_offsets"][d]), int(log["ups_counts"][d])
    ups = list(zip(log["ups_keys"][o:o + m].tolist(), log["ups_actors"][o:o + m].tolist(),
                   log["ups_counters"][o:o + m].tolist(), log["ups_kind"][o:o + m].tolist()))
    return rem, ups


def assert_log(got, want, what=""):
    """got: MergeLogBuffers.numpy() of a call; want: a LogRef.  Flags, summary, offsets and
    counts whole; the columns at every slot that holds a record (the rest is unspecified)."""
    for f in PER_DOC + ("summary",):
        if got[f] is None:
            continue
        g, w = got[f], want.log[f]
        assert g.shape == w.shape, (what, f, g.shape, w.shape)
        if not (g == w).all():
            i = int(np.nonzero(g != w)[0][0])
            raise AssertionError("%s %s differs first at %d: gpu %d, expected %d" % (what, f, i, g[i], w[i]))
    for f in LISTS:
        if got[f] is None:
            continue
        idx = want.rem_idx if f.startswith("rem") else want.ups_idx
        g, w = got[f][idx], want.log[f][idx]
        if not (g == w).all():
            i = int(idx[np.nonzero(g != w)[0][0]])
            raise AssertionError("%s %s differs first at slot %d: gpu %d, expected %d"
                                 % (what, f, i, got[f][i], want.log[f][i]))


def assert_state(got, want, n, R, what=""):
    """Two host outputs in the join's layout: slot bounds, counts, clocks and live entries."""
    assert (np.asarray(got.offsets)[: n + 1] == np.asarray(want.offsets)[: n + 1]).all(), what + " offsets"
    assert (np.asarray(got.counts)[:n] == np.asarray(want.counts)[:n]).all(), what + " counts"
    assert (np.asarray(got.vv)[: n * R] == np.asarray(want.vv)[: n * R]).all(), what + " vv"
    idx = _slots_idx(np.asarray(want.offsets)[: n + 1], np.asarray(want.counts)[:n])
    for f in ("keys", "actors", "counters"):
        g, w = np.asarray(getattr(got, f))[idx], np.asarray(getattr(want, f))[idx]
        if not (g == w).all():
            i = int(idx[np.nonzero(g != w)[0][0]])
            raise AssertionError("%s %s differs first at slot %d" % (what, f, i))


# ------------------------------------------------------------------- builders

def pack(R, docs, slack=0, with_counts=False, stale=None):
    """docs: [(entries, vv)] -> host AWSetBatch, built column-wise.  slack: spare slots per
    document; stale: an rng whose values fill them (None: zeros); counts are given when
    there is slack or with_counts."""
    n = len(docs)
    counts = np.array([len(e) for e, _ in docs], U32)
    offsets = np.zeros(n + 1, U32)
    np.cumsum(counts + U32(slack), out=offsets[1:])
    total = max(int(offsets[-1]), 1)
    if stale is not None:
        keys = stale.integers(0, 2 ** 63, total, dtype=np.int64).view(U64).copy()
        actors = stale.integers(0, 2 ** 31, total, dtype=np.int64).astype(U32)
        counters = stale.integers(0, 2 ** 63, total, dtype=np.int64).view(U64).copy()
    else:
        keys, actors, counters = np.zeros(total, U64), np.zeros(total, U32), np.zeros(total, U64)
    vv = np.zeros(max(n * R, 1), U64)
    for d, (e, v) in enumerate(docs):
        o, m = int(offsets[d]), len(e)
        if m:
            cols = np.asarray(e, dtype=object).reshape(m, 3)
            keys[o:o + m] = cols[:, 0].astype(U64)
            actors[o:o + m] = cols[:, 1].astype(U32)
            counters[o:o + m] = cols[:, 2].astype(U64)
        vv[d * R:(d + 1) * R] = v
    return AWSetBatch(R, offsets, keys, actors, counters, vv[: n * R], counts=counts if (slack or with_counts) else None)


def pair_doc(rng, R, nd, ns, mode, kmul=1):
    """One document of both sides: ((entries, vv) of dst, the same of src), nd / ns entries.
    mode 0: the general case -- keys drawn from one universe, a common key under the same
            dot half of the time, clocks at random: removes, adds, updates, a clock change;
    mode 1: converged -- src is dst, entry for entry and clock for clock (flags 0; ns unused);
    mode 2: src's clock covers nothing of dst and dst's everything of src: nothing is
            removed and nothing added, common keys still move to src's dot."""
    hi = MAX_C - 1
    if mode == 1:
        keys = [kmul * (1 + 3 * i) for i in sorted(rng.sample(range(nd + nd // 2 + 2), nd))]
        e = [(k, rng.randrange(R), rng.randint(1, hi)) for k in keys]
        v = [rng.randint(0, MAX_C) for _ in range(R)]
        return (e, v), (list(e), list(v))
    U = max(nd, ns) + (min(nd, ns) + 1) // 2 + 2
    universe = [kmul * (1 + 3 * i) for i in range(U)]
    kd, ks = sorted(rng.sample(universe, nd)), sorted(rng.sample(universe, ns))
    if mode == 0:
        ed = [(k, rng.randrange(R), rng.randint(1, hi)) for k in kd]
        dd = {k: (a, c) for k, a, c in ed}
        es = [(k,) + (dd[k] if k in dd and rng.random() < 0.5 else (rng.randrange(R), rng.randint(1, hi))) for k in ks]
        return (ed, [rng.randint(0, MAX_C) for _ in range(R)]), (es, [rng.randint(0, MAX_C) for _ in range(R)])
    ed = [(k, rng.randrange(R), rng.randint(2, hi)) for k in kd]
    es = [(k, rng.randrange(R), 1) for k in ks]
    return (ed, [1] * R), (es, [1] * R)


def random_pair(seed, n_docs, R, max_e=WAVE_MAX, big_every=25, lay_d=None, lay_s=None):
    """The parity set: n_docs documents of 0..max_e entries a side in the modes of pair_doc
    (d % 4 == 1 converged, d % 4 == 3 mode 2, the rest general), either side or both empty
    now and then, and every big_every-th document with 65..130 entries on one side or both,
    so that both sides of the 64-entry dispatch are met in one batch.  lay_*: pack()'s layout."""
    rng = random.Random(seed)
    dd, sd = [], []
    for d in range(n_docs):
        nd, ns = rng.randint(0, max_e), rng.randint(0, max_e)
        if d % 11 == 2:
            nd = 0
        if d % 11 == 5:
            ns = 0
        if d % 31 == 7:
            nd = ns = 0
        if big_every and d % big_every == big_every - 1:
            nd, ns = rng.choice([(rng.randint(65, 130), ns), (nd, rng.randint(65, 130)), (rng.randint(65, 130),) * 2])
        x, y = pair_doc(rng, R, nd, ns, (0, 1, 0, 2)[d % 4], kmul=(1 if d % 2 else 2 ** 40 + 7))
        dd.append(x)
        sd.append(y)
    return pack(R, dd, **(lay_d or {})), pack(R, sd, **(lay_s or {}))


def seq_batch(R, specs):
    """Documents whose entries are given column-wise: specs[d] = (keys, actors, counters, vv),
    numpy arrays (no per-entry Python work: for the documents of 10^5 entries)."""
    n = len(specs)
    counts = np.array([len(s[0]) for s in specs], U32)
    offsets = np.zeros(n + 1, U32)
    np.cumsum(counts, out=offsets[1:])
    cat = lambda i, dt: np.concatenate([np.asarray(s[i], dt) for s in specs]) if n else np.zeros(0, dt)  # noqa: E731
    vv = np.concatenate([np.asarray(s[3], U64) for s in specs]) if n else np.zeros(0, U64)
    return AWSetBatch(R, offsets, cat(0, U64), cat(1, U32), cat(2, U64), vv)


def straddle_pair(pos, R=2, tail=40):
    """One document whose only common key has its dst entry at merged position pos - 1 and
    its src entry at merged position pos (dst first on equal keys): below it dst-only and
    src-only keys alternate, above it `tail` more of each.  The common key's dot differs
    between the sides (UPDATED); both clocks are zero, so nothing is removed or skipped."""
    below = pos - 1
    nd_b, ns_b = (below + 1) // 2, below // 2
    kd = [10 * (2 * i) + 1 for i in range(nd_b)]       # 1, 21, 41, ...
    ks = [10 * (2 * i + 1) + 1 for i in range(ns_b)]   # 11, 31, ...
    common = 10 * (below + 1) + 5
    top = common + 10
    kd += [common] + [top + 20 * i for i in range(tail)]
    ks += [common] + [top + 10 + 20 * i for i in range(tail)]
    ed = (np.array(kd, U64), np.zeros(len(kd), U32), np.full(len(kd), 2, U64), np.zeros(R, U64))
    es = (np.array(ks, U64), np.ones(len(ks), U32) % R, np.full(len(ks), 3, U64), np.zeros(R, U64))
    return ed, es


def merged_position(dst, src, d, key, side):
    """The merged position (dst first on equal keys) of `key` as `side` ('d' or 's') holds it."""
    kd, ks = np.asarray(_live(dst, d)[0], U64), np.asarray(_live(src, d)[0], U64)
    if side == "d":
        return int(np.searchsorted(kd, key)) + int(np.searchsorted(ks, key, "left"))
    return int(np.searchsorted(kd, key, "right")) + int(np.searchsorted(ks, key))


def on_wave_path(dst, src, d):
    return max(len(_live(dst, d)[0]), len(_live(src, d)[0])) <= WAVE_MAX


def census(dst, src, log):
    """Documents per flag bit, with flags == 0, and on each side of the dispatch."""
    f = log["flags"]
    wave = sum(on_wave_path(dst, src, d) for d in range(dst.n_docs))
    return {"removed": int((f & REMOVED != 0).sum()), "added": int((f & ADDED != 0).sum()),
            "updated": int((f & UPDATED != 0).sum()), "clock": int((f & CLOCK != 0).sum()),
            "unchanged": int((f == 0).sum()), "wave": wave, "block": dst.n_docs - wave}
