"""CPU: join_log_ref (tests/join_log_cases.py), the expectation of
crdt_awset_join_log_async / crdt_awset_exchange_log_async, pinned rather than merely
used:
  1. round trip: dst[d] minus `removed` plus `upserted` is the oracle's output, on every
     ordered pair of states in tests/golden/kat_scenarios.json and on random reachable
     histories;
  2. the rule restated: the same lists from DESIGN.md section 2 applied per key --
     dst-only and srcVV.HasDot(d): removed; src-only and !dstVV.HasDot(s): ADDED; common
     and s != d: UPDATED;
  3. against the reference's log: removed / ADDED / UPDATED are what `remove` / `add` /
     `update` of merge (oracle/awset_ref.py, awset.go:109-158) do to the maps;
  4. the census of the GPU parity set: every flag bit, flags == 0 and both sides of the
     64-entry dispatch in at least 100 of its 3,000 documents;
  5. the entry points exist in the header, the library and the binding.
"""

import itertools
import random
import re

import numpy as np
import pytest

import crdtgpu
from crdtgpu import abi
from helpers import batch_of, ents, intern, pad, random_history
from join_log_cases import (LOG_DOCS, LOG_WAVES, WAVE_MAX, WINDOW, census, doc_lists, join_log_ref, merged_position,
                            on_wave_path, random_pair, seq_batch, straddle_pair)
from test_compare_model import _live, golden_pairs
from test_diff_model import ADDED, UPDATED


def applied(dst, log, d):
    """dst[d]'s live entries with `removed` deleted and `upserted` assigned."""
    k, a, c = _live(dst, d)
    m = {kk: (aa, cc) for kk, aa, cc in zip(k, a, c)}
    rem, ups = doc_lists(log, d)
    for kk, aa, cc in rem:
        assert m.pop(kk) == (aa, cc)  # removed with the dot it had in dst
    for kk, aa, cc, kind in ups:
        assert (kk in m) == (kind == UPDATED)
        m[kk] = (aa, cc)
    return sorted((kk, aa, cc) for kk, (aa, cc) in m.items())


def check_round_trip(dst, src):
    ref = join_log_ref(dst, src)
    assert ref.rc == 0
    after = ref.out.as_batch()
    for d in range(dst.n_docs):
        assert applied(dst, ref.log, d) == list(zip(*_live(after, d))), d
        rem, ups = doc_lists(ref.log, d)
        rk, uk = [x[0] for x in rem], [x[0] for x in ups]
        assert all(x < y for x, y in zip(rk, rk[1:])) and all(x < y for x, y in zip(uk, uk[1:])) and not set(rk) & set(uk)
    assert (ref.log["rem_offsets"] == dst.offsets).all() and (ref.log["ups_offsets"] == src.offsets).all()
    assert (np.asarray(ref.out.offsets)[: dst.n_docs + 1] ==
            np.asarray(dst.offsets, np.uint32) + np.asarray(src.offsets, np.uint32)).all()
    return ref


def test_round_trip_on_every_golden_pair():
    n = changed = 0
    for R, docs, snaps in golden_pairs():
        pairs = list(itertools.product(range(len(snaps)), repeat=2))
        dst = batch_of(R, [docs[i] for i, _ in pairs], slack=1)
        src = batch_of(R, [docs[j] for _, j in pairs])
        ref = check_round_trip(dst, src)
        n += dst.n_docs
        changed += int(ref.log["summary"][3])
    assert n >= 23 * 23 and 0 < changed < n


def history_pairs(seed):
    rng = random.Random(8600 + seed)
    R = rng.choice([2, 3, 5])
    reps = random_history(rng, R, rng.randint(5, 80), rng.randint(3, 30), delta=False)
    return R, reps, intern(reps)


def test_round_trip_and_the_reference_log_on_random_histories():
    n = n_rem = n_add = n_upd = 0
    for seed in range(60):
        R, reps, ids = history_pairs(seed)
        ddocs, sdocs, want = [], [], []
        for x, y in itertools.permutations(reps, 2):
            p = x.Clone()
            p.Merge(y)
            ddocs.append((ents(x.Entries, ids), pad(x.VersionVector, R)))
            sdocs.append((ents(y.Entries, ids), pad(y.VersionVector, R)))
            dot = lambda e: (e.actor, e.counter)  # noqa: E731
            rem = sorted((ids[k],) + dot(e) for k, e in x.Entries.items() if k not in p.Entries)   # `remove`
            add = sorted((ids[k],) + dot(e) for k, e in p.Entries.items() if k not in x.Entries)   # `add`
            upd = sorted((ids[k],) + dot(e) for k, e in p.Entries.items()
                         if k in x.Entries and dot(x.Entries[k]) != dot(e))                        # `update`
            want.append((rem, add, upd, ents(p.Entries, ids), pad(p.VersionVector, R)))
        dst, src = batch_of(R, ddocs, slack=seed % 3), batch_of(R, sdocs, slack=(seed + 1) % 2)
        ref = check_round_trip(dst, src)
        after = ref.out.as_batch()
        for d, (rem, add, upd, e, vv) in enumerate(want):
            got_rem, got_ups = doc_lists(ref.log, d)
            assert got_rem == rem, (seed, d)
            assert [x[:3] for x in got_ups if x[3] == ADDED] == add, (seed, d)
            assert [x[:3] for x in got_ups if x[3] == UPDATED] == upd, (seed, d)
            assert after.doc(d) == (e, vv), (seed, d)
            n_rem += len(rem)
            n_add += len(add)
            n_upd += len(upd)
        n += len(want)
    assert n > 300 and n_rem > 20 and n_add > 20 and n_upd > 20, (n, n_rem, n_add, n_upd)


def rule_lists(dst, src, d):
    """DESIGN.md section 2 per key: (removed, [(key, actor, counter, kind)] upserted)."""
    R = dst.R
    has = lambda vv, a, c: a < R and int(vv[a]) >= c  # noqa: E731
    dvv, svv = dst.vv[d * R:(d + 1) * R], src.vv[d * R:(d + 1) * R]
    D = {k: (a, c) for k, a, c in zip(*_live(dst, d))}
    S = {k: (a, c) for k, a, c in zip(*_live(src, d))}
    rem = sorted((k,) + D[k] for k in D if k not in S and has(svv, *D[k]))
    ups = sorted((k,) + S[k] + (ADDED,) for k in S if k not in D and not has(dvv, *S[k]))
    ups += [(k,) + S[k] + (UPDATED,) for k in S if k in D and S[k] != D[k]]
    return rem, sorted(ups)


@pytest.fixture(scope="module")
def parity():
    dst, src = random_pair(9000 + 2, 3000, 2)
    return dst, src, join_log_ref(dst, src)


def test_the_rule_restated_per_key(parity):
    dst, src, ref = parity
    for d in range(dst.n_docs):
        assert doc_lists(ref.log, d) == rule_lists(dst, src, d), d
    for seed in range(20):
        R, reps, ids = history_pairs(seed)
        pairs = list(itertools.permutations(reps, 2))
        a = batch_of(R, [(ents(x.Entries, ids), pad(x.VersionVector, R)) for x, _ in pairs])
        b = batch_of(R, [(ents(y.Entries, ids), pad(y.VersionVector, R)) for _, y in pairs], slack=1)
        r = join_log_ref(a, b)
        for d in range(a.n_docs):
            assert doc_lists(r.log, d) == rule_lists(a, b, d), (seed, d)


@pytest.mark.parametrize("R", [1, 2, 5, 64])
def test_census_of_the_gpu_parity_set(R):
    dst, src = random_pair(9000 + R, 3000, R)
    assert dst.n_docs == 3000
    ref = join_log_ref(dst, src)
    assert ref.rc == 0
    c = census(dst, src, ref.log)
    assert min(c.values()) >= 100, c
    live = [(len(_live(dst, d)[0]), len(_live(src, d)[0])) for d in range(3000)]
    assert sum(a == 0 and b > 0 for a, b in live) >= 20 and sum(b == 0 and a > 0 for a, b in live) >= 20
    assert sum(a == 0 and b == 0 for a, b in live) >= 20
    s = ref.log["summary"]
    assert int(s[2]) >= 100 and int(s[0]) >= 100 and int(s[1]) - int(s[2]) >= 100


@pytest.mark.parametrize("pos", [WINDOW - 1, WINDOW, WINDOW + 1, 2 * WINDOW - 1, 2 * WINDOW, 2 * WINDOW + 1])
def test_straddle_pair_puts_the_common_key_where_it_says(pos):
    ed, es = straddle_pair(pos)
    dst, src = seq_batch(2, [ed]), seq_batch(2, [es])
    common = sorted(set(ed[0].tolist()) & set(es[0].tolist()))
    assert len(common) == 1 and not on_wave_path(dst, src, 0)
    assert merged_position(dst, src, 0, common[0], "d") == pos - 1
    assert merged_position(dst, src, 0, common[0], "s") == pos
    ref = join_log_ref(dst, src)
    rem, ups = doc_lists(ref.log, 0)
    assert rem == [] and [x[0] for x in ups if x[3] == UPDATED] == common
    assert len(ups) == len(es[0])  # every other src key is an add


def test_kernel_constants_are_the_ones_the_cases_assume():
    import os

    from helpers import PKG

    src = open(os.path.join(PKG, "csrc", "join_log.hip")).read()
    const = lambda n: int(re.search(r"constexpr \w+ %s = (\d+);" % n, src).group(1))  # noqa: E731
    assert const("kLogWaveMax") == WAVE_MAX and const("kLogWaves") == LOG_WAVES and const("kLogDocs") == LOG_DOCS
    assert const("kLogBlockNT") * const("kLogBlockIPT") == WINDOW


def test_header_library_and_binding_have_the_entry_points():
    names = {"crdt_awset_join_log_async": 6, "crdt_awset_exchange_log_async": 8}
    have = crdtgpu.header_functions()
    text = re.sub(r"/\*.*?\*/", "", open(abi.HEADER_PATH).read(), flags=re.S)
    for name, n_args in names.items():
        assert name in have and getattr(abi.lib(), name) is not None  # exported by libcrdtgpu.so
        args = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(args.split(",")) == n_args == len(abi.signatures()[name][1])
    fields = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*crdt_merge_log\s*;", text).group(1)
    assert re.findall(r"(\w+)\s*;", fields) == [f for f, _ in abi.CMergeLog._fields_]
    assert list(crdtgpu.MergeLogBuffers.FIELDS) == [f for f, _ in abi.CMergeLog._fields_]
    for m in ("join_log_async", "exchange_log_async", "join_log"):
        assert hasattr(crdtgpu.Engine, m)
