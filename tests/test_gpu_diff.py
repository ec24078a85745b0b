"""GPU: the merge diff (crdt_awset_diff_async / _batch) against diff_ref
(tests/test_diff_model.py), bit-exact.

Every output buffer is pre-filled with poison (flags 77, words all-ones), so each
word read back was written by the call, and list words at or past the totals
must still hold it.  The kernels (csrc/diff.hip) work in these units, read from
the source by name, and the edge cases below are sized around them:
  C = kDiffChunk     slot positions of a side per chunk,
  S = kDiffRun       documents of a chunk staged in LDS at most (beyond: lanes
                     search the offsets in global memory),
  P = kDiffPartStep  partial sums per step of the one-workgroup partials scan,
  M = kDiffMaxParts  workgroups (partial sums) per side at most: above M chunks a
                     workgroup takes a group of consecutive chunks.
"""

import ctypes
import random

import numpy as np
import pytest

import crdtgpu
from crdtgpu import abi
from crdtgpu.batch import AWSetBatch, DiffBuffers, OutBuffers, SrcBatch
from helpers import batch_of, random_state
from test_compare_model import _live, compare_ref, select_ref
from test_diff_model import (ADDED, CLOCK, LISTS, REMOVED, UPDATED, apply_lists, diff_ref, kernel_const,
                             one_entry_bits, one_entry_pair)
from test_gpu_compare import _code, _rand_doc, _seq_doc, dev_of, host_out, pack, poisoned_cmp, poisoned_out, xchg_case

pytestmark = pytest.mark.gpu

U8, U32, U64 = np.uint8, np.uint32, np.uint64
MAXK = 2 ** 64 - 1
ONES32 = 2 ** 32 - 1
C = kernel_const("kDiffChunk")
S = kernel_const("kDiffRun")
P = kernel_const("kDiffPartStep")
M = kernel_const("kDiffMaxParts")
POISON = {1: 77, 4: ONES32, 8: MAXK}


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "GPU tests need a HIP device"
    return t


@pytest.fixture(scope="module")
def eng(torch):
    e = crdtgpu.Engine(0)
    yield e
    e.close()


def poisoned_diff(torch, n_docs, rem_slots, ups_slots, **kw):
    out = DiffBuffers(n_docs, rem_slots, ups_slots, device=dev_of(torch), **kw)
    for f in DiffBuffers.FIELDS:
        t = getattr(out, f)
        if t is not None:
            t.fill_(77 if t.dtype == torch.uint8 else -1)
    return out


def raw(out, f):
    """Field f of a device DiffBuffers, whole, as unsigned numpy."""
    a = getattr(out, f).cpu().numpy()
    return a.view({1: U8, 4: U32, 8: U64}[a.dtype.itemsize])


def assert_diff(out, want, rem_cut=None, ups_cut=None):
    """A poisoned device DiffBuffers after the call equals `want` (diff_ref's dict);
    list words at or past the totals -- or past rem_cut / ups_cut, the slots given when
    a list did not fit -- still hold the poison."""
    n = len(want["flags"])
    for f in ("flags", "summary", "rem_off", "ups_off"):
        if getattr(out, f) is None:
            continue
        g, w = raw(out, f)[: len(want[f])], want[f]
        if not (g == w).all():
            i = int(np.nonzero(g != w)[0][0])
            raise AssertionError("%s differs first at %d of %d: gpu %d, expected %d" % (f, i, n, g[i], w[i]))
    for side, cut in (("rem", rem_cut), ("ups", ups_cut)):
        total = int(want[side + "_off"][-1])
        m = total if cut is None else min(cut, total)
        for col in ("keys", "actors", "counters", "kind"):
            f = "%s_%s" % (side, col)
            if f not in want or getattr(out, f) is None:
                continue
            g = raw(out, f)
            if not (g[:m] == want[f][:m]).all():
                i = int(np.nonzero(g[:m] != want[f][:m])[0][0])
                raise AssertionError("%s differs first at %d: gpu %d, expected %d" % (f, i, g[i], want[f][i]))
            assert (g[m:] == POISON[g.dtype.itemsize]).all(), "%s written at or past %d" % (f, m)


def diff_on_device(eng, torch, before, after, want, spare=3, stream=None, **kw):
    out = poisoned_diff(torch, before.n_docs, int(want["rem_off"][-1]) + spare, int(want["ups_off"][-1]) + spare, **kw)
    eng.diff_async(before.to(dev_of(torch)), after.to(dev_of(torch)), out, stream=stream)
    return out


def check(eng, torch, before, after, want=None, **kw):
    want = diff_ref(before, after) if want is None else want
    out = diff_on_device(eng, torch, before, after, want, **kw)
    eng.sync()
    assert_diff(out, want)
    return want


# ------------------------------------------------------- 1. placement of a change

def placed_changes(R=2):
    """One change per document: first / last / only entry, of each kind and of the
    clock; before empty, after empty, both empty; dots that differ in the actor
    alone, and in the low or the high half of a counter at the 2^32, 2^63 and 2^64 - 1
    edges.  Returns (before docs, after docs, the flags expected)."""
    db, da, flags = [], [], []

    def add(b, a, f):
        db.append(b)
        da.append(a)
        flags.append(f)

    for n in (1, 2, 5, 70):
        for where in sorted({0, n - 1}):
            k, a, c, v = _seq_doc(10, n)
            add((k, a, c, v), (k[:where] + k[where + 1:], a[:where] + a[where + 1:], c[:where] + c[where + 1:], v), REMOVED)
            add((k[:where] + k[where + 1:], a[:where] + a[where + 1:], c[:where] + c[where + 1:], v), (k, a, c, v), ADDED)
            a2, c2 = list(a), list(c)
            a2[where] ^= 1
            add((k, a, c, v), (k, a2, c, v), UPDATED)  # the actor alone
            c2[where] += 1
            add((k, a, c, v), (k, a, c2, v), UPDATED)
            k2 = list(k)
            k2[where] += 1  # one key replaced: one removed, one added
            add((k, a, c, v), (k2, a, c, v), REMOVED | ADDED)
            add((k, a, c, v), (k, a, c, [v[0], v[1] + 1]), CLOCK)
            add((k, a, c, v), (k, a, c, v), 0)
    k, a, c, v = _seq_doc(3, 4)
    add(([], [], [], v), (k, a, c, v), ADDED)
    add((k, a, c, v), ([], [], [], v), REMOVED)
    add(([], [], [], v), ([], [], [], v), 0)
    add(([], [], [], [0, 2 ** 64 - 1]), ([], [], [], [0, 2 ** 63]), CLOCK)
    wide = [2 ** 32, 2 ** 32, 2 ** 63, 2 ** 64 - 1, 2 ** 32 + 1]
    add(([1, 2, 3, 4, 5], [0] * 5, wide, v),
        ([1, 2, 3, 4, 5], [0] * 5, [2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1, 2 ** 63, 2 ** 32 + 1], v), UPDATED)
    add(([7], [0], [2 ** 32], v), ([7], [0], [2 ** 32 + 1], v), UPDATED)  # the low half alone
    add(([7], [0], [2 ** 32], v), ([7], [0], [2 ** 63], v), UPDATED)      # the high half alone
    add(([7], [0], [2 ** 64 - 1], v), ([7], [0], [2 ** 64 - 1], v), 0)
    return db, da, np.array(flags, U8)


@pytest.mark.parametrize("slack_b,slack_a", [(0, 0), (2, 0), (0, 1), (1, 3)])
def test_placement_of_a_change(eng, torch, slack_b, slack_a):
    db, da, flags = placed_changes()
    before = pack(2, db, slack_b, 0, np.random.default_rng(21))
    after = pack(2, da, slack_a, 0, np.random.default_rng(22))
    want = check(eng, torch, before, after)
    assert (want["flags"] == flags).all()
    wide = len(flags) - 4
    assert int(want["ups_off"][wide + 1]) - int(want["ups_off"][wide]) == 4  # the fifth dot is equal


# ------------------------------------------------------------------- 2. layouts

LAYOUTS = [(0, 0), (0, 1), (3, 1)]  # (slack, counts given); counts == NULL only at zero slack
_small = {}


def small_docs(n_docs=2000, R=2):
    """Documents of 0 to 40 entries; `after` is `before` with a few keys dropped, a
    few added and a few moved to another dot, about a third unchanged."""
    if R not in _small:
        rng = random.Random(9700 + R)
        db, da = [], []
        for d in range(n_docs):
            k, a, c, v = _rand_doc(rng, R, rng.randint(0, 40))
            db.append((k, a, c, v))
            if d % 3 == 0:
                da.append((k, a, c, v))
                continue
            m = {kk: (aa, cc) for kk, aa, cc in zip(k, a, c)}
            for kk in rng.sample(k, min(len(k), rng.randint(0, 3))):
                del m[kk]
            for _ in range(rng.randint(0, 3)):
                m.setdefault(rng.getrandbits(64), (rng.randrange(R), rng.randint(1, 2 ** 40)))
            for kk in rng.sample(sorted(m), min(len(m), rng.randint(0, 3))):
                aa, cc = m[kk]
                m[kk] = (aa, cc + 2 ** 32) if rng.random() < 0.5 else ((aa + 1) % max(R, 2), cc)
            v2 = list(v)
            if rng.random() < 0.4:
                v2[rng.randrange(R)] += 1
            ks = sorted(m)
            da.append((ks, [m[x][0] for x in ks], [m[x][1] for x in ks], v2))
        _small[R] = (db, da)
    return _small[R]


@pytest.mark.parametrize("a_slack,a_counts", LAYOUTS)
@pytest.mark.parametrize("b_slack,b_counts", LAYOUTS)
def test_random_small(eng, torch, b_slack, b_counts, a_slack, a_counts):
    db, da = small_docs()
    before = pack(2, db, b_slack, b_counts, np.random.default_rng(31))
    after = pack(2, da, a_slack, a_counts, np.random.default_rng(32))
    assert (before.counts is None) == (not b_slack and not b_counts)
    want = check(eng, torch, before, after)
    assert int(np.bitwise_or.reduce(want["flags"])) == 15 and 500 < int((want["flags"] == 0).sum()) < 900
    assert min(int(x) for x in want["summary"][:3]) > 300


def test_stale_slack_that_would_match_and_a_live_key_zero(eng, torch):
    """after's slack still holds the entry that was removed, before's slack already
    holds the entry that is added; zero-padded slack beside a live key 0."""
    R = 2
    b = batch_of(R, [([(3, 0, 1), (5, 1, 2), (9, 0, 4)], [4, 2]), ([(3, 0, 1)], [1, 0]), ([(0, 1, 7)], [0, 7]),
                     ([], [0, 0]), ([(0, 0, 1), (2, 0, 2)], [2, 0])], slack=1)
    a = batch_of(R, [([(3, 0, 1), (5, 1, 2)], [4, 2]), ([(3, 0, 1), (8, 1, 1)], [1, 1]), ([], [0, 7]),
                     ([(0, 1, 3)], [0, 3]), ([(2, 0, 2)], [2, 0])], slack=2)
    ao, bo = a.offsets, b.offsets
    a.keys[ao[0] + 2], a.actors[ao[0] + 2], a.counters[ao[0] + 2] = 9, 0, 4  # the removed entry, stale
    b.keys[bo[1] + 1], b.actors[bo[1] + 1], b.counters[bo[1] + 1] = 8, 1, 1  # the added entry, ahead of its time
    assert not a.keys[ao[2]:ao[3]].any() and not b.keys[bo[3]:bo[4]].any()   # zero padding where key 0 is looked for
    want = check(eng, torch, b, a)
    assert want["flags"].tolist() == [REMOVED, ADDED | CLOCK, REMOVED, ADDED | CLOCK, REMOVED]
    assert want["rem_keys"].tolist() == [9, 0, 0] and want["ups_keys"].tolist() == [8, 0]


def test_exchange_output_against_its_input(eng, torch):
    """out_ab diffed against a as the exchange left it (capacity offsets, padded
    slack); the lists applied on the host to a reproduce out_ab."""
    c = xchg_case()
    dev = dev_of(torch)
    o1 = OutBuffers(c["n"], c["R"], c["slots"], device=dev)
    o2 = OutBuffers(c["n"], c["R"], c["slots"], device=dev)
    ab = c["ab"].as_batch()
    want = diff_ref(c["a"], ab)
    out = poisoned_diff(torch, c["n"], int(want["rem_off"][-1]) + 2, int(want["ups_off"][-1]) + 2)
    ad = c["a"].to(dev)
    eng.exchange_async(ad, c["b"].to(dev), o1, o2)
    eng.diff_async(ad, o1.as_batch(), out)
    eng.sync()
    assert_diff(out, want)
    got = apply_lists(c["a"], out.numpy())
    for d in range(c["n"]):
        assert got[d] == list(zip(*_live(ab, d))), d
    assert min(int(x) for x in want["summary"][:3]) > 50


def test_fold_output_against_its_destination(eng, torch):
    rng = random.Random(9710)
    R, n = 3, 300
    dst = [random_state(rng, R, rng.randint(0, 30), 60, 20) for _ in range(n)]
    per_doc = [[(s % R, *reversed(random_state(rng, R, rng.randint(0, 12), 60, 20)), None) for s in range(rng.randint(0, 3))]
               for _ in range(n)]
    dstb, srcs = batch_of(R, dst, slack=1), SrcBatch.from_lists(R, per_doc)
    dev = dev_of(torch)
    out = OutBuffers(n, R, srcs.out_slots(dstb), device=dev)
    dd = dstb.to(dev)
    eng.reserve(n, out.slots)
    eng.fold_async(crdtgpu.CRDT_FOLD_AWSET, dd, srcs.to(dev), out)
    eng.sync()
    folded = host_out(out).as_batch()
    want = diff_ref(dstb, folded)
    res = poisoned_diff(torch, n, int(want["rem_off"][-1]) + 1, int(want["ups_off"][-1]) + 1)
    eng.diff_async(dd, out.as_batch(), res)
    eng.sync()
    assert_diff(res, want)
    assert int(want["summary"][0]) > 20 and int(want["summary"][1]) > 20


@pytest.mark.parametrize("R", [1, 3, 64])
def test_clock_widths(eng, torch, R):
    db, da = small_docs(400, R)
    want = check(eng, torch, pack(R, db), pack(R, da, slack=1))
    assert (want["flags"] & CLOCK).any() and not (want["flags"] & CLOCK).all()


def test_columns_not_asked_for(eng, torch):
    db, da = small_docs()
    before, after = pack(2, db[:300]), pack(2, da[:300], slack=1)
    want = diff_ref(before, after)
    check(eng, torch, before, after, want, dots=False, kind=False, summary=False)


# ------------------------------------------------------ 3. chunk and stage edges

def _changed(doc, where, how):
    k, a, c, v = (list(x) for x in doc)
    if how == "dot":
        c[where] += 1
    elif how == "gone":
        del k[where], a[where], c[where]
    else:
        k[where] += 1  # (keys are 3 apart)
    return k, a, c, v


def chunk_spans(offsets, total):
    """Per chunk of a side, the documents the kernel stages: d_hi - d_lo + 1."""
    off = np.asarray(offsets, np.int64)[1:-1]
    spans = []
    for base in range(0, total, C):
        m = min(C, total - base)
        spans.append(int(np.searchsorted(off, base + m - 1, "right")) - int(np.searchsorted(off, base, "right")) + 1)
    return spans


def test_documents_ending_at_chunk_edges(eng, torch):
    """Documents that end at C - 1, C and C + 1 positions of a chunk, each changed in
    its first and its last entry."""
    sizes = [C - 1, 1, C + 1, C - 1, C, 7]
    assert sum(sizes[:1]) == C - 1 and sum(sizes[:2]) == C and sum(sizes[:3]) == 2 * C + 1 and sum(sizes[:5]) == 4 * C
    db = [_seq_doc(100000 * i, n) for i, n in enumerate(sizes)]
    for how in ("dot", "gone", "key"):
        da = [_changed(_changed(d, len(d[0]) - 1, how), 0, how) if len(d[0]) > 1 else _changed(d, 0, how) for d in db]
        for sb, sa in ((0, 0), (0, 1)):
            check(eng, torch, pack(2, db, sb), pack(2, da, sa))
            check(eng, torch, pack(2, da, sa), pack(2, db, sb))


def test_one_change_at_each_chunk_seam(eng, torch):
    """Documents of 3 C + 1 entries, each starting on a chunk's first position, whose
    only change is the entry on one side of a chunk seam."""
    seams = [C - 1, C, 2 * C - 1, 2 * C, 3 * C - 1, 3 * C]
    db, da, dr = [], [], []
    for i, s in enumerate(seams):
        big, fill = _seq_doc(10 ** 6 * i, 3 * C + 1), _seq_doc(10 ** 6 * i + 500000, C - 1)
        db += [big, fill]
        da += [_changed(big, s, "dot"), fill]
        dr += [_changed(big, s, "gone"), fill]
    before = pack(2, db)
    assert all(int(before.offsets[2 * i]) % C == 0 for i in range(len(seams)))
    want = check(eng, torch, before, pack(2, da))
    assert want["ups_kind"].tolist() == [UPDATED] * 6 and int(want["summary"][0]) == 0
    assert want["ups_keys"].tolist() == [db[2 * i][0][s] for i, s in enumerate(seams)]
    want = check(eng, torch, before, pack(2, dr))   # after's documents begin one position early each
    assert want["rem_keys"].tolist() == [db[2 * i][0][s] for i, s in enumerate(seams)]
    want = check(eng, torch, pack(2, dr), before)
    assert want["ups_kind"].tolist() == [ADDED] * 6


@pytest.mark.parametrize("span", [S - 1, S, S + 1])
def test_documents_staged_per_chunk(eng, torch, span):
    """span documents inside one chunk -- runs of empty and one-entry documents
    between two fillers: at most S are staged in LDS, S + 1 are searched in global
    memory."""
    rng = random.Random(9720 + span)
    run = span - 1  # (the filler behind the run is the chunk's last document)
    db = [_seq_doc(0, C)]
    for i in range(run):
        one = i == 0 or (i % 5 in (1, 2) and sum(len(d[0]) for d in db[1:]) < C - 8)
        db.append(([10 * i + 1], [i % 2], [i + 1], [5, 5]) if one else ([], [], [], [5, 5]))
    db.append(_seq_doc(9 * 10 ** 6, C))
    before = pack(2, db)
    assert span in chunk_spans(before.offsets, int(before.offsets[-1]))
    da = []
    for d in db:
        r = rng.random()
        if not d[0]:
            da.append(d if r < 0.8 else ([4], [0], [1], d[3]))
        elif len(d[0]) == 1:
            da.append(d if r < 0.5 else (_changed(d, 0, "dot") if r < 0.7 else ([], [], [], d[3]) if r < 0.85 else _changed(d, 0, "key")))
        else:
            da.append(_changed(d, len(d[0]) // 2, "dot"))
    after = pack(2, da)
    want = check(eng, torch, before, after)
    assert int(np.bitwise_or.reduce(want["flags"])) == REMOVED | ADDED | UPDATED
    check(eng, torch, after, before)


def test_a_run_of_empty_documents_at_and_across_a_chunk_edge(eng, torch):
    """More than S empty documents in a row: once beginning exactly on a chunk edge
    (the next chunk owns all their offsets), once in the middle of a chunk (its
    span exceeds the stage); the next non-empty document's offsets follow them."""
    empty = ([], [], [], [5, 5])
    db = [_seq_doc(0, C)] + [empty] * (S + 5) + [_seq_doc(10 ** 6, 5), _seq_doc(2 * 10 ** 6, C - 8)] + \
        [empty] * (S + 7) + [_seq_doc(3 * 10 ** 6, 10)] + [empty] * 3
    da = list(db)
    da[0] = _changed(db[0], C - 1, "gone")
    da[S + 6] = _changed(db[S + 6], 0, "gone")
    da[S + 7] = _changed(db[S + 7], 3, "key")
    da[2 * S + 15] = _changed(db[2 * S + 15], 9, "gone")
    da[5] = ([7], [1], [1], [5, 5])  # an empty document of the first run gains an entry
    before, after = pack(2, db), pack(2, da)
    assert max(chunk_spans(before.offsets, int(before.offsets[-1]))) > S
    want = check(eng, torch, before, after)
    d = S + 6
    assert want["rem_off"][1:d + 1].tolist() == [1] * d and int(want["rem_off"][d + 1]) == 2
    assert int(want["rem_off"][-1]) == 4 and want["rem_off"][-4:].tolist() == [4] * 4
    check(eng, torch, after, before)


# ------------------------------------------------------------------ 4. scan edges

def one_entry_docs_for_chunks(seed, chunks):
    """n such that `before` of one_entry_pair(seed, n) holds (chunks - 1) C + 1 positions."""
    cum = np.cumsum(one_entry_bits(seed, 2 * C * (chunks + 2), 1))
    n = int(np.searchsorted(cum, (chunks - 1) * C + 1)) + 1
    assert int(cum[n - 1]) == (chunks - 1) * C + 1
    return n


@pytest.mark.parametrize("chunks", [P - 1, P, P + 1, M + 1], ids=["P-1", "P", "P+1", "M+1"])
def test_partials_scan_edges(eng, torch, chunks):
    """One-entry documents, the expectation numpy alone.  P + 1 chunks need a second
    step of the partials scan; M + 1 chunks make a workgroup take two chunks."""
    before, after, want = one_entry_pair(9730 + chunks, one_entry_docs_for_chunks(9730 + chunks, chunks))
    assert (int(before.offsets[-1]) + C - 1) // C == chunks
    check(eng, torch, before, after, want)


# ----------------------------------------------------------------------- 5. search

N_BIG = 2 ** 20 + 1


@pytest.mark.parametrize("form", ["one_dot", "shifted", "disjoint"])
def test_one_large_document(eng, torch, form):
    """2^20 + 1 entries a side: identical but for one dot in the middle (the first
    probe always hits); after shifted by one key inserted at the front (every probe
    off by one); disjoint key ranges (the gallop's worst case)."""
    k = np.arange(N_BIG, dtype=U64) * U64(3) + U64(10)
    a = (np.arange(N_BIG) % 2).astype(U32)
    c = np.arange(N_BIG, dtype=U64) + U64(1)
    vv = np.array([5, 5], U64)

    def one(keys, actors, counters):
        return AWSetBatch(2, np.array([0, len(keys)], U32), keys, actors, counters, vv)

    before = one(k, a, c)
    z = lambda dt: np.zeros(0, dt)  # noqa: E731
    want = {"flags": None, "rem_off": np.array([0, 0], U32), "rem_keys": z(U64), "rem_actors": z(U32), "rem_counters": z(U64),
            "ups_off": np.array([0, 1], U32)}
    if form == "one_dot":
        c2 = c.copy()
        c2[N_BIG // 2] += U64(2 ** 32)
        after = one(k, a, c2)
        want.update(ups_keys=k[N_BIG // 2:][:1], ups_actors=a[N_BIG // 2:][:1], ups_counters=c2[N_BIG // 2:][:1],
                    ups_kind=np.array([UPDATED], U8), flags=np.array([UPDATED], U8), summary=np.array([0, 1, 1, 1, 1], U32))
    elif form == "shifted":
        after = one(np.concatenate([[U64(1)], k]), np.concatenate([[U32(1)], a]), np.concatenate([[U64(9)], c]))
        want.update(ups_keys=np.array([1], U64), ups_actors=np.array([1], U32), ups_counters=np.array([9], U64),
                    ups_kind=np.array([ADDED], U8), flags=np.array([ADDED], U8), summary=np.array([0, 1, 0, 1, 1], U32))
    else:
        k2 = k + U64(3 * N_BIG)
        after = one(k2, a, c)
        want.update(rem_off=np.array([0, N_BIG], U32), rem_keys=k, rem_actors=a, rem_counters=c,
                    ups_off=np.array([0, N_BIG], U32), ups_keys=k2, ups_actors=a, ups_counters=c,
                    ups_kind=np.full(N_BIG, ADDED, U8), flags=np.array([REMOVED | ADDED], U8),
                    summary=np.array([N_BIG, N_BIG, 0, 1, 1], U32))
    check(eng, torch, before, after, want)


# ----------------------------------------------------------------------- 6. errors

@pytest.mark.parametrize("short", ["rem", "ups"])
def test_a_list_one_slot_short(eng, torch, short):
    db, da = small_docs()
    before, after = pack(2, db, 3, 1), pack(2, da, 0, 1)
    want = diff_ref(before, after)
    nr, nu = int(want["rem_off"][-1]), int(want["ups_off"][-1])
    out = poisoned_diff(torch, before.n_docs, nr - (short == "rem"), nu - (short == "ups"))
    eng.diff_async(before.to(dev_of(torch)), after.to(dev_of(torch)), out)
    assert _code(eng.sync) == crdtgpu.CRDT_E_CAPACITY
    assert_diff(out, want, rem_cut=out.rem_slots, ups_cut=out.ups_slots)  # offsets, totals, the other list: exact
    eng.sync()  # cleared


@pytest.mark.parametrize("side", ["before", "after"])
def test_count_above_slots_is_clamped(eng, torch, side):
    before = batch_of(2, [([(1, 0, 1)], [1, 0]), ([(3, 0, 1)], [1, 0]), ([(9, 1, 4)], [0, 4])], slack=1)
    after = batch_of(2, [([(1, 0, 1)], [1, 0]), ([(3, 0, 1)], [1, 0]), ([(9, 1, 5)], [0, 5])], slack=1)
    over = before if side == "before" else after
    over.keys[int(over.offsets[1]) + 1] = 77  # the slack slot: live once the count says so
    over.counts[1] = 5
    want = diff_ref(before, after)
    assert want["flags"].tolist() == [0, REMOVED if side == "before" else ADDED, UPDATED | CLOCK]
    out = diff_on_device(eng, torch, before, after, want)
    assert _code(eng.sync) == crdtgpu.CRDT_E_CAPACITY
    assert_diff(out, want)
    eng.sync()


def test_argument_errors(eng, torch):
    """Every one of these is refused on the host: nothing is launched."""
    dev = dev_of(torch)
    b = batch_of(2, [([(1, 0, 1), (4, 1, 2)], [1, 2]), ([(3, 0, 1)], [1, 0])], slack=1).to(dev)
    a = batch_of(2, [([(1, 0, 1)], [1, 2]), ([(3, 0, 1), (5, 0, 2)], [2, 0])], slack=1).to(dev)
    a3 = batch_of(2, [([(1, 0, 1)], [1, 2])] * 3).to(dev)
    aR = batch_of(3, [([(1, 0, 1)], [1, 2, 0]), ([(3, 0, 1)], [1, 0, 0])]).to(dev)
    out = poisoned_diff(torch, 2, 4, 4)
    lib, ctx, ref = abi.lib(), eng._ctx, ctypes.byref

    def call(cb, ca, co, nr=4, nu=4):
        return lib.crdt_awset_diff_async(ctx, ref(cb) if cb else None, ref(ca) if ca else None, nr, nu,
                                         ref(co) if co else None, None)

    assert call(None, a.c(), out.c()) == crdtgpu.CRDT_E_INVALID
    assert call(b.c(), None, out.c()) == crdtgpu.CRDT_E_INVALID
    assert call(b.c(), a.c(), None) == crdtgpu.CRDT_E_INVALID
    assert call(b.c(), a3.c(), out.c()) == crdtgpu.CRDT_E_INVALID  # n_docs
    assert call(b.c(), aR.c(), out.c()) == crdtgpu.CRDT_E_INVALID  # R
    cb = b.c()
    cb.R = 65
    assert call(cb, cb, out.c()) == crdtgpu.CRDT_E_INVALID
    for field in ("flags", "rem_off", "ups_off", "rem_keys", "ups_keys", "rem_actors", "rem_counters", "ups_actors",
                  "ups_counters"):  # required, or one of a pair of dot columns
        co = out.c()
        setattr(co, field, None)
        assert call(b.c(), a.c(), co) == crdtgpu.CRDT_E_INVALID, field
    pairs = {"rem_off": ("offsets", "counts"), "ups_off": ("offsets", "counts"), "rem_keys": ("keys",),
             "ups_keys": ("keys",), "rem_actors": ("actors",), "ups_actors": ("actors",),
             "rem_counters": ("counters",), "ups_counters": ("counters",)}
    for src in (b, a):  # an out array starting where an input array of the same kind starts
        for field, kinds in pairs.items():
            for kind in kinds:
                co = out.c()
                setattr(co, field, getattr(src, kind).data_ptr())
                assert call(b.c(), a.c(), co) == crdtgpu.CRDT_E_INVALID, (field, kind)
    eng.sync()
    for f in DiffBuffers.FIELDS:
        g = raw(out, f)
        assert (g == POISON[g.dtype.itemsize]).all(), f
    co = out.c()  # the sizing call: no lists, no slots
    for f in ("rem_keys", "rem_actors", "rem_counters", "ups_keys", "ups_actors", "ups_counters", "ups_kind"):
        setattr(co, f, None)
    assert call(b.c(), a.c(), co, 0, 0) == 0
    assert _code(eng.sync) == crdtgpu.CRDT_E_CAPACITY
    want = diff_ref(b.numpy(), a.numpy())
    assert (raw(out, "rem_off") == want["rem_off"]).all() and (raw(out, "ups_off") == want["ups_off"]).all()
    assert (raw(out, "rem_keys") == MAXK).all() and (raw(out, "ups_keys") == MAXK).all()
    eng.diff_async(b, a, out)  # and the call still works
    eng.sync()
    assert_diff(out, want)


def test_no_documents(eng, torch):
    dev = dev_of(torch)
    z = lambda dt: torch.zeros(1, dtype=dt, device=dev)  # noqa: E731
    e = AWSetBatch(2, z(torch.int32), z(torch.int64), z(torch.int32), z(torch.int64), z(torch.int64))
    assert e.n_docs == 0
    out = poisoned_diff(torch, 1, 4, 4)
    out.n_docs = 0
    eng.diff_async(e, e, out)
    eng.sync()
    assert raw(out, "rem_off").tolist() == [0, ONES32] and raw(out, "ups_off").tolist() == [0, ONES32]
    assert raw(out, "summary").tolist() == [0] * 5 and raw(out, "flags").tolist() == [77]
    for f in LISTS[1:4] + LISTS[5:]:
        g = raw(out, f)
        assert (g == POISON[g.dtype.itemsize]).all(), f


def test_batch_call(eng):
    """Host arrays: the same dict, each list trimmed to its total; an unsorted side is
    refused on the device with the outputs untouched; a list that does not fit still
    brings the offsets and totals back."""
    db, da = small_docs()
    before, after = pack(2, db[:500], 1, 1, np.random.default_rng(41)), pack(2, da[:500])
    want = diff_ref(before, after)
    got = eng.diff(before, after)
    for f in ("flags", "summary") + LISTS:
        assert got[f].shape == want[f].shape and (got[f] == want[f]).all(), f
    lib, ref = abi.lib(), ctypes.byref
    for side in (0, 1):
        pair = [AWSetBatch(2, x.offsets, x.keys.copy(), x.actors, x.counters, x.vv, counts=x.counts) for x in (before, after)]
        bad = pair[side]
        d = next(d for d in range(bad.n_docs) if bad.live(d) >= 2)
        o = int(bad.offsets[d])
        bad.keys[o], bad.keys[o + 1] = bad.keys[o + 1], bad.keys[o]
        out = DiffBuffers(500, int(want["rem_off"][-1]), int(want["ups_off"][-1]))
        for f in DiffBuffers.FIELDS:
            getattr(out, f).fill(77)
        cb, ca, co = pair[0].c(), pair[1].c(), out.c()
        assert lib.crdt_awset_diff_batch(eng._ctx, ref(cb), ref(ca), out.rem_slots, out.ups_slots, ref(co)) == \
            crdtgpu.CRDT_E_UNSORTED
        for f in DiffBuffers.FIELDS:
            assert (getattr(out, f) == 77).all(), f
    out = DiffBuffers(500, int(want["rem_off"][-1]) - 1, int(want["ups_off"][-1]))
    cb, ca, co = before.c(), after.c(), out.c()
    assert lib.crdt_awset_diff_batch(eng._ctx, ref(cb), ref(ca), out.rem_slots, out.ups_slots, ref(co)) == \
        crdtgpu.CRDT_E_CAPACITY
    assert (out.rem_off == want["rem_off"]).all() and (out.ups_off == want["ups_off"]).all()
    assert (out.rem_keys == want["rem_keys"][:-1]).all() and (out.ups_keys == want["ups_keys"]).all()
    over = batch_of(2, [([(1, 0, 1)], [1, 0])], slack=1)
    over.counts[0] = 5
    with pytest.raises(crdtgpu.CrdtError) as ei:
        eng.diff(over, batch_of(2, [([(1, 0, 1)], [1, 0])]))
    assert ei.value.code == crdtgpu.CRDT_E_CAPACITY
    eng.sync()


# ------------------------------------------------------------- 7. device-side use

def fixed_slots(R, docs, cap):
    """docs: [(keys, actors, counters, vv)] at `cap` slots per document, whatever they hold."""
    m = len(docs)
    b = AWSetBatch(R, np.arange(m + 1, dtype=U32) * U32(cap), np.zeros(m * cap, U64), np.zeros(m * cap, U32),
                   np.zeros(m * cap, U64), np.zeros(m * R, U64), counts=np.zeros(m, U32))
    for d, (k, a, c, v) in enumerate(docs):
        o, n = d * cap, len(k)
        assert n <= cap
        b.keys[o:o + n], b.actors[o:o + n], b.counters[o:o + n] = np.asarray(k, U64), np.asarray(a, U32), np.asarray(c, U64)
        b.vv[d * R:(d + 1) * R] = v
        b.counts[d] = n
    return b


def test_graph_capture(torch):
    """A diff captured on a reserved context and replayed with both inputs changed in
    between equals the eager call; on an unreserved context the capture is refused
    with CRDT_E_WORKSPACE and launches nothing."""
    db, da = small_docs()
    n, R, cap = len(db), 2, 48
    assert n > 1024  # (a fresh context's workspace holds 1,024 documents)
    rng = random.Random(9790)
    cases = []
    for r in range(3):
        pb, pa = list(range(n)), list(range(n))
        rng.shuffle(pb)
        if r:
            rng.shuffle(pa)
        else:
            pa = pb
        before, after = fixed_slots(R, [db[i] for i in pb], cap), fixed_slots(R, [da[i] for i in pa], cap)
        cases.append((before, after, diff_ref(before, after)))
    nr = max(int(w["rem_off"][-1]) for _, _, w in cases) + 3
    nu = max(int(w["ups_off"][-1]) for _, _, w in cases) + 3
    dev = dev_of(torch)
    e = crdtgpu.Engine(0)
    try:
        bd, ad = cases[0][0].to(dev), cases[0][1].to(dev)
        out = poisoned_diff(torch, n, nr, nu)
        g0 = torch.cuda.CUDAGraph()
        with pytest.raises(crdtgpu.CrdtError) as ei:
            with torch.cuda.graph(g0):
                e.diff_async(bd, ad, out, stream=torch.cuda.current_stream())
        assert ei.value.code == crdtgpu.CRDT_E_WORKSPACE
        torch.cuda.synchronize()
        for f in DiffBuffers.FIELDS:
            g = raw(out, f)
            assert (g == POISON[g.dtype.itemsize]).all(), f
        e.reserve(n)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.diff_async(bd, ad, out, stream=torch.cuda.current_stream())
        for before, after, want in cases[1:] + cases[:1]:
            for dst, src in ((bd, before.to(dev)), (ad, after.to(dev))):
                for f in ("offsets", "counts", "keys", "actors", "counters", "vv"):
                    getattr(dst, f).copy_(getattr(src, f))
            for f in DiffBuffers.FIELDS:
                t = getattr(out, f)
                t.fill_(77 if t.dtype == torch.uint8 else -1)
            g.replay()
            e.sync(torch.cuda.current_stream())
            assert_diff(out, want)
    finally:
        e.close()


def test_ordered_after_an_exchange_on_another_stream(eng, torch):
    c = xchg_case()
    dev = dev_of(torch)
    o1 = OutBuffers(c["n"], c["R"], c["slots"], device=dev)
    o2 = OutBuffers(c["n"], c["R"], c["slots"], device=dev)
    for o in (o1, o2):
        for t in (o.offsets, o.counts, o.keys, o.actors, o.counters, o.vv):
            t.zero_()  # a diff that ran before the exchange would see an empty `after`
    want = diff_ref(c["a"], c["ab"].as_batch())
    out = poisoned_diff(torch, c["n"], int(want["rem_off"][-1]) + 2, int(want["ups_off"][-1]) + 2)
    ad, bd = c["a"].to(dev), c["b"].to(dev)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.exchange_async(ad, bd, o1, o2, stream=sa)
    eng.diff_async(ad, o1.as_batch(), out, stream=sb)
    eng.sync(sb)
    assert_diff(out, want)


def test_two_eager_runs_are_bit_identical(eng, torch):
    db, da = small_docs()
    before, after = pack(2, db, 3, 1, np.random.default_rng(51)), pack(2, da, 1, 1, np.random.default_rng(52))
    want = diff_ref(before, after)
    bd, ad = before.to(dev_of(torch)), after.to(dev_of(torch))
    outs = []
    for _ in range(2):
        out = poisoned_diff(torch, before.n_docs, int(want["rem_off"][-1]), int(want["ups_off"][-1]))
        eng.diff_async(bd, ad, out)
        outs.append(out)
    eng.sync()
    for f in DiffBuffers.FIELDS:
        assert (raw(outs[0], f) == raw(outs[1], f)).all(), f
    assert_diff(outs[0], want)


def test_round_compare_select_diff(eng, torch):
    """compare -> worklist -> select of both sides -> diff, the worklist and n_work
    left on the device, equals diff_ref of the selected documents."""
    db, da = small_docs()
    before, after = pack(2, db, 2, 1, np.random.default_rng(61)), pack(2, da, 0, 1)
    n, R = before.n_docs, 2
    dev = dev_of(torch)
    _, _, work = compare_ref(before, after)
    assert 1000 < len(work) < n
    sb_want = select_ref(before, work, n_idx=len(work), n_out=len(work))
    sa_want = select_ref(after, work, n_idx=len(work), n_out=len(work))
    want = diff_ref(sb_want, sa_want)
    assert (want["flags"] != 0).all()
    bd, ad = before.to(dev), after.to(dev)
    res = poisoned_cmp(torch, n)
    sb = poisoned_out(torch, len(work), R, int(sb_want.offsets[-1]))
    sa = poisoned_out(torch, len(work), R, int(sa_want.offsets[-1]))
    out = poisoned_diff(torch, len(work), int(want["rem_off"][-1]) + 1, int(want["ups_off"][-1]) + 1)
    eng.compare_async(bd, ad, res, mask=15)
    eng.select_async(bd, sb, idx=res.worklist, n_idx=res.n_work)
    eng.select_async(ad, sa, idx=res.worklist, n_idx=res.n_work)
    eng.diff_async(sb.as_batch(), sa.as_batch(), out)
    eng.sync()
    assert_diff(out, want)
    full = diff_ref(before, after)
    assert (full["flags"][work] == want["flags"]).all() and (full["summary"][:3] == want["summary"][:3]).all()
