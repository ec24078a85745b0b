"""CPU: the case table of tests/join_edge_cases.py sits on the edges it was built for, and its
expectations are the reference's.

Every case, both directions, goes through the C oracle (oracle.join), the expectation of
tests/test_gpu_join_edges.py, and is held to the map-based restatement of the reference's
(*AWSet).Merge (oracle/awset_ref.py) and to the results stated by hand.  The oracle's result
must not depend on what the slack holds.  The census tests recompute every `claims` entry from
the case and the oracle's result; an edit to the table that moves a case off its edge fails
the test that names it.
"""

import os
import re

import numpy as np
import pytest

from crdtgpu.batch import AWSetBatch
from helpers import ref_entries, ref_state
from join_edge_cases import (BY_NAME, CASES, COMMON_KINDS, DECIDE, END_MOD16, FILLS, HANDOFF_SIZES, K_DEFAULT, LAYOUTS, N_OUT,
                             OVER_CASES, POSITIONS, SLACKS, T_DEFAULT, T_SMALL, TABLE, TILE_TS, TOP, WAVE_SIZES, WAVES, R,
                             batches, census, concat, over_count, path_of)
from join_option_cases import T_OF_SHAPE, WAVE_MAX
from oracle import oracle

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-crdt-playground_amd", "csrc")

_joined = {}


def joined(case):
    """(a, b, a <- b, b <- a) by the C oracle, the over-count cases with the count clamped; once per case."""
    if case.name not in _joined:
        a, b = batches(case, clamped=True)
        rc1, ab = oracle.join(a, b)
        rc2, ba = oracle.join(b, a)
        assert rc1 == 0 and rc2 == 0, case.name
        _joined[case.name] = (a, b, ab, ba)
    return _joined[case.name]


def doc_of(out, d):
    o, n = int(out.offsets[d]), int(out.counts[d])
    return (list(zip(out.keys[o:o + n].tolist(), out.actors[o:o + n].tolist(), out.counters[o:o + n].tolist())),
            out.vv[d * R:(d + 1) * R].tolist())


_census = {}


def cen(case):
    if case.name not in _census:
        _census[case.name] = census(case, doc_of(joined(case)[2], case.claims.get("at", 0))[0])
    return _census[case.name]


# ------------------------------------------------------------------ the table itself

def test_constants_are_the_kernels():
    """The restated constants against the text of the kernels (no build is imported)."""
    join = open(os.path.join(CSRC, "join.hip")).read()
    tile = open(os.path.join(CSRC, "tile.hip")).read()
    assert "constexpr int kJoinWaves = %d;" % WAVES in join
    assert "default: launch_wave<%d, AUX, EXCH, STG>" % K_DEFAULT in join
    assert join.count("m.dn <= 64 && m.sn <= 64") + join.count("mn.dn <= 64 && mn.sn <= 64") == 3 and WAVE_MAX == 64
    assert re.search(r"case 10: return 256 \* 2;", tile) and T_SMALL == 512 == T_OF_SHAPE[10]
    assert re.search(r"case 9: return 512 \* 2;", tile) and T_DEFAULT == 1024 == T_OF_SHAPE[9]
    assert "m8 = CRDT_JOIN_PAD_STORES == 2 ? 15u : 7u, m4 = CRDT_JOIN_PAD_STORES == 2 ? 31u : 15u" in join


def test_cases_are_well_formed():
    for c in CASES:
        assert c.R == R and len(c.dst_docs) == len(c.src_docs) >= 1, c.name
        for ents, vv in c.dst_docs + c.src_docs:
            keys = [k for k, _, _ in ents]
            assert keys == sorted(set(keys)) and all(0 <= k <= TOP for k in keys), c.name
            assert len(vv) == R and all(a != R for _, a, _ in ents), c.name  # (actor == R has its own tests)
        assert set(c.claims) <= set(cen(c)) | {"key", "lane", "layout", "place", "T", "straddle_key", "dot_ab", "dot_ba",
                                               "zero_tiles", "one_side_below", "ends_in", "top_ends", "tiles_small",
                                               "n_out_before", "n_out_after"}, c.name


def test_table_stays_small():
    n = sum(len(e) for c in CASES for e, _ in c.dst_docs + c.src_docs)
    assert n < 50000 and len(CASES) < 220 and max(len(c.dst_docs) for c in CASES) <= 40, (n, len(CASES))


# ------------------------------------------------------------------ the expectations

@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_oracle_is_the_reference_merge(case):
    """Both directions, every document: the C oracle against the map-based Merge, and the
    first document against the result stated by hand."""
    a, b, ab, ba = joined(case)
    for d in range(a.n_docs):
        (de, dvv), (se, svv) = a.doc(d), b.doc(d)
        for out, (xe, xvv), (ye, yvv) in ((ab, (de, dvv), (se, svv)), (ba, (se, svv), (de, dvv))):
            x = ref_state(xe, xvv)
            x.Merge(ref_state(ye, yvv))
            assert doc_of(out, d) == (ref_entries(x), list(x.VersionVector)), (case.name, d)
    if case.want is not None:
        assert doc_of(ab, 0)[0] == case.want[0] and doc_of(ba, 0)[0] == case.want[1], case.name
    slots = int(a.offsets[-1]) + int(b.offsets[-1])
    assert int(ab.offsets[a.n_docs]) == slots == int(ba.offsets[a.n_docs])
    assert (ab.offsets[:-1] == a.offsets[:-1] + b.offsets[:-1]).all()


def same_live(x, y, n):
    return all(doc_of(x, d) == doc_of(y, d) for d in range(n))


@pytest.mark.parametrize("extra", SLACKS, ids=lambda s: "slack_%d_%d" % s)
def test_oracle_ignores_the_slack(extra):
    """Every case with 1 and 9 (9 and 1) more slots a document, under all three fills: the live
    result is the tight build's, whatever the slack holds.  (The over-count cases keep their own
    layout: their bad document has no slack, its count is clamped to all of its slots.)"""
    for case in TABLE:
        a, b, ab, ba = joined(case)
        for fill in FILLS:
            pa, pb = batches(case, extra, fill, clamped=True)
            if fill != "zeros":  # the fill is there, and it is not the zero fill
                za, zb = batches(case, extra, "zeros", clamped=True)
                assert (pa.keys != za.keys).any() and (pb.counters != zb.counters).any(), case.name
            rc1, pab = oracle.join(pa, pb)
            rc2, pba = oracle.join(pb, pa)
            assert rc1 == 0 and rc2 == 0
            assert same_live(pab, ab, a.n_docs) and same_live(pba, ba, a.n_docs), (case.name, fill)


def test_continuation_fill_would_change_the_result_if_read():
    """The continuation slack, taken as live, passes for entries: its keys ascend past the last
    live key, include keys the other side holds live, and its dots are unseen by the other
    side's clock -- one more live entry a side changes the oracle's result in most cases."""
    changed = with_other_keys = 0
    for case in TABLE:
        a, b = batches(case, (1, 9), "continuation")
        for d in range(a.n_docs):
            for x, y in ((a, b), (b, a)):
                o, n = int(x.offsets[d]), int(x.counts[d])
                slots = int(x.offsets[d + 1]) - o
                keys = x.keys[o:o + slots].tolist()
                tail = [k for k in keys[max(n - 1, 0):] if k != TOP]  # (at the top of the range the key repeats)
                assert tail == sorted(set(tail)) and keys[max(n - 1, 0):] == sorted(keys[max(n - 1, 0):]), (case.name, d)
                yo, yn = int(y.offsets[d]), int(y.counts[d])
                with_other_keys += bool(set(keys[n:]) & set(y.keys[yo:yo + yn].tolist()))
                yvv = y.vv[d * R:(d + 1) * R].tolist()
                assert all(int(c) > yvv[int(act)] for act, c in zip(x.actors[o + n:o + slots], x.counters[o + n:o + slots]))
        grown = a.counts.copy()
        grown += 1
        a1 =AWSetBatch(R, a.offsets, a.keys, a.actors, a.counters, a.vv, grown)
        if all(a1.doc(d)[0][-1][0] != TOP or len(a1.doc(d)[0]) == 1 or a1.doc(d)[0][-2][0] != TOP for d in range(a.n_docs)):
            changed += not same_live(oracle.join(a1, b)[1], oracle.join(a, b)[1], a.n_docs)
    assert changed > len(TABLE) * 3 // 4 and with_other_keys > len(TABLE)


def test_concatenated_table_is_the_cases():
    """The table as one batch (how the GPU test runs it under every option): each case's
    documents come out as they do alone."""
    a, b, first = concat(TABLE)
    rc, ab = oracle.join(a, b)
    assert rc == 0 and a.n_docs == sum(len(c.dst_docs) for c in TABLE)
    for c, f in zip(TABLE, first):
        alone = joined(c)[2]
        assert all(doc_of(ab, f + d) == doc_of(alone, d) for d in range(len(c.dst_docs))), c.name


# ------------------------------------------------------------------ census: every claim

@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_claims_hold(case):
    """Every claims entry the census computes directly: sizes, path, n_out, where the output
    ends, capacity, the wave's k slot, total."""
    got = cen(case)
    for k, v in case.claims.items():
        if k in got and k != "tiles":
            assert got[k] == v, (case.name, k, got[k], v)
    if "tiles" in case.claims:
        assert got["tiles"][case.claims["T"]]["n_tiles"] == case.claims["tiles"], case.name
    if "tiles_small" in case.claims and case.claims["tiles_small"]:
        assert got["tiles"][T_SMALL]["n_tiles"] == case.claims["tiles_small"], case.name


def test_decide_table_is_complete():
    sides = {k: v[0] for k, v in DECIDE.items()}
    assert sorted(sides.values()).count("dst") == 6 == sorted(sides.values()).count("src") and len(COMMON_KINDS) == 3
    for kind, (side, ddot, sdot, dvv, svv, out_ab, out_ba) in DECIDE.items():
        for pos, (n, p) in POSITIONS.items():
            c = BY_NAME["decide_%s_%s" % (kind, pos)]
            ents_d, ents_s = c.dst_docs[0][0], c.src_docs[0][0]
            key = c.claims["key"]
            own = ents_d if side != "src" else ents_s
            assert [k for k, _, _ in own].index(key) == c.claims["lane"] == p, c.name  # the lane of the deciding entry
            assert (key in [k for k, _, _ in ents_d]) == (side != "src") and (key in [k for k, _, _ in ents_s]) == (side != "dst")
            if pos in ("last", "lane63", "block"):
                assert own[-1][0] == key  # the last live entry
            assert cen(c)["path"] == ("large" if pos == "block" else "wave") and len(own) == n
            for want, out in zip(c.want, (out_ab, out_ba)):
                hit = [e for e in want if e[0] == key]
                assert hit == ([(key,) + out] if out else []), c.name
    # the relation of each one-sided row's counter to the clock word it meets
    rel = {}
    for kind, (side, ddot, sdot, dvv, svv, out_ab, _) in DECIDE.items():
        if side == "both":
            continue
        (a, cnt), clock = (ddot, svv) if side == "dst" else (sdot, dvv)
        rel[kind] = ("above_R" if a > R else cnt - clock[a], a, out_ab is not None)
    for s in ("dst", "src"):
        assert rel[s + "_below_clock"][::2] == (-1, False) and rel[s + "_at_clock"][::2] == (0, False)
        assert rel[s + "_clock_plus_1"][::2] == (1, True) and rel[s + "_zero_at_zero"] == (0, 1, False)
        assert rel[s + "_actor_last"] == (0, R - 1, False) and rel[s + "_actor_above"] == ("above_R", R + 1, True)
        # actor R - 1: the other two clock words would have kept the entry
        clock = DECIDE[s + "_actor_last"][4 if s == "dst" else 3]
        assert clock[0] < 5 and clock[1] < 5
        assert DECIDE[s + "_zero_at_zero"][4 if s == "dst" else 3][1] == 0
    _, dd, sd, dvv, svv, ab, ba = DECIDE["common_same_dot"]
    assert dd == sd == ab == ba
    _, dd, sd, dvv, svv, ab, ba = DECIDE["common_src_wins"]
    assert dd != sd and ab == sd and ba == dd
    _, dd, sd, dvv, svv, ab, ba = DECIDE["common_covered"]
    assert svv[dd[0]] >= dd[1] and dvv[sd[0]] >= sd[1] and ab == sd and ba == dd  # both covered, still kept


def test_wave_shapes_are_complete():
    for dn in WAVE_SIZES:
        for sn in WAVE_SIZES:
            for layout in LAYOUTS:
                c = BY_NAME["wave_%d_%d_%s" % (dn, sn, layout)]
                dk, sk = [k for k, _, _ in c.dst_docs[0][0]], [k for k, _, _ in c.src_docs[0][0]]
                assert (len(dk), len(sk)) == (dn, sn)
                if layout == "common":
                    assert len(set(dk) & set(sk)) == min(dn, sn)
                    continue
                assert not set(dk) & set(sk)
                if dn and sn:
                    if layout == "dst_below":
                        assert dk[-1] < sk[0]
                    elif layout == "src_below":
                        assert sk[-1] < dk[0]
                    else:
                        merged = sorted([(k, 0) for k in dk] + [(k, 1) for k in sk])
                        m = 2 * min(dn, sn)
                        assert all(merged[i][1] != merged[i + 1][1] for i in range(m - 1))
    for n_out in N_OUT:
        assert cen(BY_NAME["n_out_%d" % n_out])["n_out"] == n_out
    assert set(N_OUT) == {0, 1, 63, 64, 65, 127, 128}
    seen = set()
    for res in END_MOD16:
        for exact in (True, False):
            got = cen(BY_NAME["pad_end_%d_%s" % (res, "exact" if exact else "spare")])
            assert got["end_mod16"] == res and got["cap_exact"] == exact and got["path"] == "wave" and got["at"] == 1
            seen.add((got["end_mod8"], got["end_mod16"]))
    assert {m8 for m8, _ in seen} == {0, 1, 7} and {0, 1, 15} <= {m16 for _, m16 in seen}
    c = BY_NAME["no_survivors_between_two_full"]
    ab = joined(c)[2]
    assert [int(x) for x in ab.counts] == [c.claims["n_out_before"], 0, c.claims["n_out_after"]]
    # first document, last document, a batch of one, and more
    assert {len(c.dst_docs) for c in CASES} >= {1, 2, 3, 5}


def test_handoff_places():
    for dn, sn in HANDOFF_SIZES:
        for place in ("first", "last", "last_of_k"):
            c = BY_NAME["handoff_%d_%d_%s" % (dn, sn, place)]
            at, n = c.claims["at"], len(c.dst_docs)
            got = cen(c)
            assert got["path"] == "large" and (got["dn"], got["sn"]) == (dn, sn)
            others = [path_of(len(c.dst_docs[d][0]), len(c.src_docs[d][0])) for d in range(n) if d != at]
            assert set(others) == {"wave"}  # its counts, clock and slot bounds come from another kernel than its neighbours'
            assert {"first": at == 0, "last": at == n - 1, "last_of_k": got["k_slot"] == K_DEFAULT - 1 and at + WAVES < n + WAVES}[place]
    assert max(dn + sn for dn, sn in HANDOFF_SIZES) == 129 and min(max(p) for p in HANDOFF_SIZES) == 65


@pytest.mark.parametrize("T", TILE_TS)
def test_tile_edges(T):
    tag = "T%d" % T
    for total in (T - 1, T, T + 1, 2 * T, 2 * T + 1):
        got = cen(BY_NAME["tile_%s_total_%d" % (tag, total)])
        assert got["total"] == total and got["tiles"][T]["n_tiles"] == -(-total // T) and got["path"] == "large"
    for kind in COMMON_KINDS:
        c = BY_NAME["tile_%s_straddle_%s" % (tag, kind)]
        key = c.claims["straddle_key"]
        for d_side, s_side, out, dot in ((c.dst_docs[0][0], c.src_docs[0][0], joined(c)[2], c.claims["dot_ab"]),
                                         (c.src_docs[0][0], c.dst_docs[0][0], joined(c)[3], c.claims["dot_ba"])):
            res = doc_of(out, 0)[0]
            i0, j0 = census(c._replace(dst_docs=[(d_side, [0] * R)], src_docs=[(s_side, [0] * R)]), res)["tiles"][T]["splits"][1]
            # the dst half is the last position of tile 0, the src half the first of tile 1 (the split of
            # tests/test_tile_split_model.py at diagonal T)
            assert d_side[i0 - 1][0] == key == s_side[j0][0] and i0 + j0 == T, (c.name, i0, j0)
            assert [e for e in res if e[0] == key] == [(key,) + dot], c.name
    for name in ("first_tile_removed", "middle_tile_removed", "all_removed", "all_kept"):
        c = BY_NAME["tile_%s_%s" % (tag, name)]
        t = cen(c)["tiles"][T]
        assert [i for i, n in enumerate(t["survivors"]) if n == 0] == c.claims["zero_tiles"], c.name
        assert cen(c)["n_out"] == c.claims["n_out"]
    t = cen(BY_NAME["tile_%s_middle_tile_removed" % tag])["tiles"][T]
    assert t["n_tiles"] == 3 and t["survivors"][0] == T and t["survivors"][2] == 40  # a look-back over a tile of none
    c = BY_NAME["tile_%s_dst_below_src" % tag]
    assert c.dst_docs[0][0][-1][0] < c.src_docs[0][0][0][0] and cen(c)["tiles"][T]["n_tiles"] == 2
    assert cen(c)["tiles"][T]["splits"][1] == (len(c.dst_docs[0][0]), T - len(c.dst_docs[0][0]))


def test_key_range():
    for path in ("wave", "large", "tile"):
        for where in ("dst", "src", "both"):
            c = BY_NAME["keys_0_top_%s_%s" % (where, path)]
            dk, sk = [k for k, _, _ in c.dst_docs[0][0]], [k for k, _, _ in c.src_docs[0][0]]
            assert len(dk) < len(sk)  # dst is the shorter run
            assert ((dk[0], dk[-1]) == (0, TOP)) == (where != "src") and ((sk[0], sk[-1]) == (0, TOP)) == (where != "dst")
            res = [k for k, _, _ in doc_of(joined(c)[2], 0)[0]]
            assert res[0] == 0 and res[-1] == TOP and cen(c)["path"] == ("wave" if path == "wave" else "large")
            if path == "tile":
                assert cen(c)["tiles"][T_SMALL]["n_tiles"] == 2 and c.shape == 10


def test_over_count_cases_stay_inside_the_arrays():
    """The bad count is above the slots, offset + unclamped count stays within the input's
    arrays, an unclamped kernel's survivors stay within the output's, the bad document is never
    the last, and the clamped sizes select the claimed path."""
    names = {c.name for c in OVER_CASES}
    assert {"over_%s_%s" % (s, p) for s in ("dst", "src") for p in ("wave", "block", "tile")} <= names
    for c in OVER_CASES:
        for extra in ((0, 0),):
            side, d, cnt = over_count(c, extra)
            a, b = batches(c, extra)
            x, y = (a, b) if side == "dst" else (b, a)
            slots = int(x.offsets[d + 1]) - int(x.offsets[d])
            assert int(x.counts[d]) == cnt > slots and d < x.n_docs - 1, c.name
            assert int(x.offsets[d]) + cnt <= len(x.keys) == int(x.offsets[-1]), c.name
            obase = int(a.offsets[d]) + int(b.offsets[d])
            assert obase + cnt + int(y.counts[d]) <= int(a.offsets[-1]) + int(b.offsets[-1]), c.name
            # the documents after it own at least that many slots more than they need
            spare = sum(int(x.offsets[e + 1]) - int(x.offsets[e]) - int(x.counts[e]) for e in range(d + 1, x.n_docs))
            assert spare >= c.over[2] >= 9
            ca, cb = batches(c, extra, clamped=True)
            assert int((ca if side == "dst" else cb).counts[d]) == slots
        got = cen(c)
        assert got["path"] == c.claims["path"] and got["unclamped_path"] == c.claims["unclamped_path"], c.name
    assert cen(BY_NAME["over_dst_60_claims_70"])["dn"] == 60 and over_count(BY_NAME["over_dst_60_claims_70"])[2] == 70
    assert cen(BY_NAME["over_dst_60_claims_70_against_80"])["sn"] == 80
    for s in ("dst", "src"):
        assert cen(BY_NAME["over_%s_tile" % s])["total"] == T_SMALL + 1 and BY_NAME["over_%s_tile" % s].shape == 10
        assert (cen(BY_NAME["over_%s_block" % s])["dn"], cen(BY_NAME["over_%s_block" % s])["sn"]) == (80, 80)


def test_sentinel_is_no_value_of_the_table():
    """0x5A5A... (tests/test_gpu_join_edges.py prefills the outputs with it) is no key, actor,
    counter or clock word of any case."""
    for c in CASES:
        a, b = batches(c)
        for x in (a, b):
            assert not (x.keys == 0x5A5A5A5A5A5A5A5A).any() and not (x.counters == 0x5A5A5A5A5A5A5A5A).any()
            assert not (x.actors == 0x5A5A5A5A).any() and not (x.vv == 0x5A5A5A5A5A5A5A5A).any()
    assert np.uint64(0x5A5A5A5A5A5A5A5A) < np.uint64(1 << 63)
