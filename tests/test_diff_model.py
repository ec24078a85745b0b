"""CPU: the merge diff restated over the packed layout.

diff_ref is the expectation of the GPU calls (tests/test_gpu_diff.py,
crdt_awset_diff_async / _batch): a numpy restatement of the contract in
include/crdtgpu.h, built on _live of tests/test_compare_model.py, so only the
live prefix of a document is ever looked at.  It is pinned here, not merely used:
  1. round trip: deleting `removed` from before[d] and assigning `upserted`
     gives exactly after[d]'s live entries (every ordered pair of states in
     tests/golden/kat_scenarios.json, and random pairs with differing slack);
  2. the lists are disjoint and strictly ascending; ADDED keys are absent from
     before, UPDATED keys present in both;
  3. agreement with compare_ref: KEYS iff REMOVED | ADDED; DOTS iff neither and
     UPDATED; A_AHEAD | B_AHEAD iff CLOCK;
  4. against the reference's rule: for after = before.Merge(src) by the map
     restatement of the reference (oracle/awset_ref.py), removed / ADDED /
     UPDATED are awset.go:122-158's `remove` / `add` / `update`.
"""

import itertools
import os
import random
import re

import numpy as np

import crdtgpu
from crdtgpu import abi
from crdtgpu.batch import AWSetBatch
from helpers import PKG, batch_of, ents, intern, pad, random_history
from test_compare_model import A_AHEAD, B_AHEAD, DOTS, KEYS, _live, compare_ref, golden_pairs

U8, U32, U64 = np.uint8, np.uint32, np.uint64
REMOVED, ADDED, UPDATED, CLOCK = 1, 2, 4, 8
LISTS = ("rem_off", "rem_keys", "rem_actors", "rem_counters", "ups_off", "ups_keys", "ups_actors", "ups_counters",
         "ups_kind")


def kernel_const(name):
    """A constexpr of csrc/diff.hip by name (constants defined through earlier ones resolved)."""
    src = open(os.path.join(PKG, "csrc", "diff.hip")).read()

    def text(n):
        return re.search(r"constexpr \w+ %s = ([^;]+);" % n, src).group(1)

    expr = text(name)
    for _ in range(4):
        expr = re.sub(r"k[A-Z]\w+", lambda m: "(%s)" % text(m.group(0)), expr)
    return int(eval(re.sub(r"\(uint32_t\)|(?<=\d)u\b", "", expr), {"__builtins__": {}}))


def diff_doc(before, after, d):
    """(removed, upserted, kinds) of one document: arrays of (keys, actors, counters)."""
    kb, ab, cb = (np.asarray(x, dt) for x, dt in zip(_live(before, d), (U64, U32, U64)))
    ka, aa, ca = (np.asarray(x, dt) for x, dt in zip(_live(after, d), (U64, U32, U64)))
    gone = ~np.isin(kb, ka)
    pos = np.minimum(np.searchsorted(kb, ka), max(len(kb) - 1, 0))
    found = (kb[pos] == ka) if len(kb) else np.zeros(len(ka), bool)
    moved = found.copy()
    if len(kb):
        moved &= (ab[pos] != aa) | (cb[pos] != ca)
    ups = ~found | moved
    kind = np.where(found, UPDATED, ADDED).astype(U8)[ups]
    return (kb[gone], ab[gone], cb[gone]), (ka[ups], aa[ups], ca[ups]), kind


def diff_ref(before, after):
    """The dict crdt_awset_diff_* writes (DiffBuffers.numpy()): flags u8 [n_docs],
    summary u32 [5], the [n_docs + 1] offsets and the packed columns of both lists."""
    assert before.n_docs == after.n_docs and before.R == after.R
    n, R = before.n_docs, before.R
    flags = np.zeros(n, U8)
    rem_off, ups_off = np.zeros(n + 1, U32), np.zeros(n + 1, U32)
    rem, ups, kinds = [], [], []
    for d in range(n):
        r, u, k = diff_doc(before, after, d)
        f = (REMOVED if len(r[0]) else 0) | (ADDED if (k == ADDED).any() else 0) | (UPDATED if (k == UPDATED).any() else 0)
        if (np.asarray(before.vv[d * R:(d + 1) * R]) != np.asarray(after.vv[d * R:(d + 1) * R])).any():
            f |= CLOCK
        flags[d] = f
        rem_off[d + 1] = rem_off[d] + U32(len(r[0]))
        ups_off[d + 1] = ups_off[d] + U32(len(u[0]))
        rem.append(r)
        ups.append(u)
        kinds.append(k)

    def col(parts, i, dt):
        return np.concatenate([p[i] for p in parts]).astype(dt) if parts else np.zeros(0, dt)

    kind = np.concatenate(kinds).astype(U8) if kinds else np.zeros(0, U8)
    summary = np.array([int(rem_off[n]), int(ups_off[n]), int((kind == UPDATED).sum()),
                        int(((flags & 7) != 0).sum()), int((flags != 0).sum())], U32)
    return {"flags": flags, "summary": summary, "rem_off": rem_off, "rem_keys": col(rem, 0, U64),
            "rem_actors": col(rem, 1, U32), "rem_counters": col(rem, 2, U64), "ups_off": ups_off,
            "ups_keys": col(ups, 0, U64), "ups_actors": col(ups, 1, U32), "ups_counters": col(ups, 2, U64),
            "ups_kind": kind}


def doc_lists(res, d):
    """({key: dot} removed, {key: (dot, kind)} upserted) of document d of a diff result."""
    r0, r1, u0, u1 = int(res["rem_off"][d]), int(res["rem_off"][d + 1]), int(res["ups_off"][d]), int(res["ups_off"][d + 1])
    rem = list(zip(res["rem_keys"][r0:r1].tolist(), res["rem_actors"][r0:r1].tolist(),
                   res["rem_counters"][r0:r1].tolist()))
    ups = list(zip(res["ups_keys"][u0:u1].tolist(), res["ups_actors"][u0:u1].tolist(),
                   res["ups_counters"][u0:u1].tolist(), res["ups_kind"][u0:u1].tolist()))
    return rem, ups


def apply_lists(before, res):
    """Per document, before[d]'s live entries with `removed` deleted and `upserted` assigned."""
    out = []
    for d in range(before.n_docs):
        k, a, c = _live(before, d)
        m = {kk: (aa, cc) for kk, aa, cc in zip(k, a, c)}
        rem, ups = doc_lists(res, d)
        for kk, aa, cc in rem:
            assert m.pop(kk) == (aa, cc)  # removed with the dot it had in before
        for kk, aa, cc, _ in ups:
            m[kk] = (aa, cc)
        out.append(sorted((kk, aa, cc) for kk, (aa, cc) in m.items()))
    return out


def check_pinned(before, after, res):
    """Checks 1 to 3 on one pair of batches; returns the number of documents."""
    got = apply_lists(before, res)
    cmp_flags = compare_ref(before, after)[0]
    for d in range(before.n_docs):
        kb, ab, cb = _live(before, d)
        ka, aa, ca = _live(after, d)
        assert got[d] == list(zip(ka, aa, ca)), d  # 1. round trip
        rem, ups = doc_lists(res, d)
        rk, uk = [x[0] for x in rem], [x[0] for x in ups]
        assert not set(rk) & set(uk), d  # 2. disjoint, ascending, kinds
        assert all(x < y for x, y in zip(rk, rk[1:])) and all(x < y for x, y in zip(uk, uk[1:])), d
        for key, _, _, kind in ups:
            assert kind in (ADDED, UPDATED)
            assert (key in kb) == (kind == UPDATED) and key in ka, d
        f, c = int(res["flags"][d]), int(cmp_flags[d])
        assert bool(f & REMOVED) == bool(rem) and bool(f & ADDED) == any(x[3] == ADDED for x in ups)
        assert bool(f & UPDATED) == any(x[3] == UPDATED for x in ups)
        assert bool(c & KEYS) == bool(f & (REMOVED | ADDED)), d  # 3. compare_ref
        assert bool(c & DOTS) == (not f & (REMOVED | ADDED) and bool(f & UPDATED)), d
        assert bool(c & (A_AHEAD | B_AHEAD)) == bool(f & CLOCK), d
        assert (f == 0) == (c == 0)
    s = res["summary"]
    assert int(s[0]) == len(res["rem_keys"]) == int(res["rem_off"][-1])
    assert int(s[1]) == len(res["ups_keys"]) == int(res["ups_off"][-1]) and int(s[2]) == int((res["ups_kind"] == UPDATED).sum())
    assert int(s[3]) == int(((res["flags"] & 7) != 0).sum()) and int(s[4]) == int((res["flags"] != 0).sum())
    return before.n_docs


def test_pinned_on_every_golden_pair():
    n = n_changed = 0
    for R, docs, snaps in golden_pairs():
        pairs = list(itertools.product(range(len(snaps)), repeat=2))
        before = batch_of(R, [docs[i] for i, _ in pairs])
        after = batch_of(R, [docs[j] for _, j in pairs], slack=1)
        res = diff_ref(before, after)
        n += check_pinned(before, after, res)
        n_changed += int(res["summary"][3])
    assert n >= 23 * 23 and 0 < n_changed < n


def random_pair(rng, n, R, slack_b, slack_a):
    """Two batches of n documents: `after` is `before` with a few keys dropped, a few
    added and a few moved to another dot; a third of the documents unchanged."""
    db, da = [], []
    for d in range(n):
        keys = sorted(rng.sample(range(60), rng.randint(0, 14)))
        e = [(k, rng.randrange(R), rng.randint(1, 9)) for k in keys]
        v = [rng.randint(0, 9) for _ in range(R)]
        db.append((e, v))
        if d % 3 == 0:
            da.append((list(e), list(v)))
            continue
        m = {k: (a, c) for k, a, c in e}
        for k in rng.sample(keys, min(len(keys), rng.randint(0, 3))):
            del m[k]
        for k in rng.sample(range(60), rng.randint(0, 3)):
            m.setdefault(k, (rng.randrange(R), rng.randint(1, 9)))
        for k in rng.sample(sorted(m), min(len(m), rng.randint(0, 3))):
            a, c = m[k]
            m[k] = ((a + 1) % R, c) if R > 1 and rng.random() < 0.5 else (a, c + 1)
        v2 = list(v)
        if rng.random() < 0.5:
            v2[rng.randrange(R)] += 1
        da.append((sorted((k, a, c) for k, (a, c) in m.items()), v2))
    return batch_of(R, db, slack=slack_b), batch_of(R, da, slack=slack_a)


def test_pinned_on_random_pairs_with_differing_slack():
    n = 0
    seen = 0
    for seed, (sb, sa) in enumerate([(0, 0), (0, 2), (3, 0), (1, 2), (2, 2), (0, 1)]):
        rng = random.Random(8300 + seed)
        before, after = random_pair(rng, 600, rng.choice([1, 2, 5]), sb, sa)
        for b in (before, after):  # stale slack that would match if it were read
            if b.counts is not None:
                for d in range(b.n_docs):
                    o, c, e = int(b.offsets[d]), int(b.counts[d]), int(b.offsets[d + 1])
                    b.keys[o + c:e] = 61 + np.arange(e - o - c, dtype=U64)
        res = diff_ref(before, after)
        n += check_pinned(before, after, res)
        seen |= int(np.bitwise_or.reduce(res["flags"]))
        assert int((res["flags"] == 0).sum()) >= 100
    assert n >= 3000 and seen == 15


def test_against_the_reference_merge_rule():
    """after = before.Merge(src): removed = keys of before not in src whose dot src's
    clock has; ADDED = keys of src not in before whose dot before's clock lacks;
    UPDATED = the common keys whose dots differ (awset.go:122-158)."""
    n = n_rem = n_add = n_upd = 0
    for seed in range(60):
        rng = random.Random(8400 + seed)
        R = rng.choice([2, 3, 5])
        reps = random_history(rng, R, rng.randint(5, 80), rng.randint(3, 30), delta=False)
        ids = intern(reps)
        bdocs, adocs, want = [], [], []
        for x, y in itertools.permutations(reps, 2):
            p = x.Clone()
            p.Merge(y)
            bdocs.append((ents(x.Entries, ids), pad(x.VersionVector, R)))
            adocs.append((ents(p.Entries, ids), pad(p.VersionVector, R)))
            rem = sorted(ids[k] for k, dot in x.Entries.items() if k not in y.Entries and y.VersionVector.HasDot(dot))
            add = sorted(ids[k] for k, dot in y.Entries.items() if k not in x.Entries and not x.VersionVector.HasDot(dot))
            upd = sorted(ids[k] for k, dot in y.Entries.items() if k in x.Entries and
                         (x.Entries[k].actor, x.Entries[k].counter) != (dot.actor, dot.counter))
            want.append((rem, add, upd))
        before, after = batch_of(R, bdocs, slack=seed % 3), batch_of(R, adocs, slack=(seed + 1) % 2)
        res = diff_ref(before, after)
        for d, (rem, add, upd) in enumerate(want):
            got_rem, got_ups = doc_lists(res, d)
            assert [x[0] for x in got_rem] == rem, (seed, d)
            assert [x[0] for x in got_ups if x[3] == ADDED] == add, (seed, d)
            assert [x[0] for x in got_ups if x[3] == UPDATED] == upd, (seed, d)
            n_rem += len(rem)
            n_add += len(add)
            n_upd += len(upd)
        n += len(want)
    assert n > 300 and n_rem > 20 and n_add > 20 and n_upd > 20, (n, n_rem, n_add, n_upd)


def test_header_library_and_binding_have_the_entry_points():
    names = {"crdt_awset_diff_async": 7, "crdt_awset_diff_batch": 6}
    have = crdtgpu.header_functions()
    text = re.sub(r"/\*.*?\*/", "", open(abi.HEADER_PATH).read(), flags=re.S)
    for name, n_args in names.items():
        assert name in have and getattr(abi.lib(), name) is not None  # exported by libcrdtgpu.so
        args = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(args.split(",")) == n_args == len(abi.signatures()[name][1])
    fields = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*crdt_diff_out\s*;", text).group(1)
    assert re.findall(r"(\w+)\s*;", fields) == [f for f, _ in abi.CDiffOut._fields_]
    assert (crdtgpu.CRDT_DIFF_REMOVED, crdtgpu.CRDT_DIFF_ADDED, crdtgpu.CRDT_DIFF_UPDATED, crdtgpu.CRDT_DIFF_CLOCK) == \
        (REMOVED, ADDED, UPDATED, CLOCK)
    assert hasattr(crdtgpu.Engine, "diff_async") and hasattr(crdtgpu.Engine, "diff")
    assert list(crdtgpu.DiffBuffers.FIELDS) == [f for f, _ in abi.CDiffOut._fields_]


def test_kernel_constants_resolve_by_name():
    c, s, p = kernel_const("kDiffChunk"), kernel_const("kDiffRun"), kernel_const("kDiffPartStep")
    assert c == kernel_const("kDiffNT") * kernel_const("kDiffJ") and s >= 2 and p >= 2
    assert kernel_const("kDiffMaxParts") >= p


def one_entry_bits(seed, n, salt, mod=2):
    """n pseudo-random words below `mod`, a function of (seed, salt, index) alone: a
    longer array extends a shorter one, so a test can pick the n that gives a total."""
    x = (np.arange(n, dtype=U64) + U64(seed)) * U64(0x9E3779B97F4A7C15) + U64(salt * 0xC2B2AE3D27D4EB4F % 2 ** 64)
    x ^= x >> U64(31)
    x *= U64(0xBF58476D1CE4E5B9)
    x ^= x >> U64(29)
    return x % U64(mod)


def one_entry_pair(seed, n):
    """(before, after, expected) for n documents of 0 or 1 entries a side, built as
    one_entry_case of tests/test_scatter_model.py builds them; the expectation is
    numpy alone, so n can be large (tests/test_gpu_diff.py).  A document's key is its
    id; the two sides' dots agree on about half of the common documents.  before's
    live count of document d is one_entry_bits(seed, n, 1)[d], after's (seed, n, 2)."""
    cb, ca = one_entry_bits(seed, n, 1).astype(U32), one_entry_bits(seed, n, 2).astype(U32)
    same = one_entry_bits(seed, n, 3).astype(bool)
    ids = np.arange(n, dtype=U64)

    def make(cnt, ctr, vv):
        off = np.zeros(n + 1, U32)
        np.cumsum(cnt, out=off[1:])
        live = cnt == 1
        return AWSetBatch(1, off, ids[live], np.zeros(int(off[-1]), U32), ctr[live], vv, counts=cnt)

    ctr_b = ids + U64(1)
    ctr_a = np.where(same, ctr_b, ctr_b + U64(2 ** 32))
    vv_b = ids * U64(2)
    vv_a = np.where(one_entry_bits(seed, n, 4, 4) == 0, vv_b + U64(1), vv_b)
    before, after = make(cb, ctr_b, vv_b), make(ca, ctr_a, vv_a)
    rem = (cb == 1) & (ca == 0)
    add = (ca == 1) & (cb == 0)
    upd = (ca == 1) & (cb == 1) & ~same
    ups = add | upd
    flags = (rem * REMOVED + add * ADDED + upd * UPDATED + (vv_a != vv_b) * CLOCK).astype(U8)

    def off(mask):
        o = np.zeros(n + 1, U32)
        np.cumsum(mask.astype(U32), out=o[1:])
        return o

    want = {"flags": flags,
            "summary": np.array([rem.sum(), ups.sum(), upd.sum(), (rem | ups).sum(), (flags != 0).sum()], U32),
            "rem_off": off(rem), "rem_keys": ids[rem], "rem_actors": np.zeros(int(rem.sum()), U32),
            "rem_counters": ctr_b[rem], "ups_off": off(ups), "ups_keys": ids[ups],
            "ups_actors": np.zeros(int(ups.sum()), U32), "ups_counters": ctr_a[ups],
            "ups_kind": np.where(upd, UPDATED, ADDED).astype(U8)[ups]}
    return before, after, want


def test_one_entry_pair_is_diff_ref():
    before, after, want = one_entry_pair(8500, 3000)
    res = diff_ref(before, after)
    for f in ("flags", "summary") + LISTS:
        assert res[f].dtype == want[f].dtype and (res[f] == want[f]).all(), f
    assert want["summary"][:3].min() > 100
