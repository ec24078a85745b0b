"""CPU: the case table of tests/sort_edge_cases.py sits on the edges it was built for.

Every `claims` entry is recomputed by the census from the case alone (a plain-Python model of
the width selection of wave_sort_pairs, of the sort's paths and of the order check's lanes); the
table as a whole is held to the list of edges it has to cover; the order cases' hand-stated
verdicts are the host validators'; the over-count cases stay inside their arrays even for a
kernel that does not clamp.  An edit that moves a case off its edge fails the test that names it.
"""

import os
import re

import numpy as np
import pytest

import crdtgpu
from crdtgpu import CRDT_E_CAPACITY, CRDT_E_DUP_KEY, CRDT_E_UNSORTED
from crdtgpu.engine import validate_tombs
from sort_edge_cases import (BLOCK_SIZES, BY_NAME, CASES, CLEAN, DUP_CASES, DUP_SIZES, FILLS, ITEMS, ORDER_BY_NAME, ORDER_CASES,
                             ORDER_LANES, ORDER_SIZES, OVER_CASES, PATTERNS, THRESHOLDS, TOP, WAVE_MAX, WAVE_SIZES, batch_of,
                             census, clean_of, concat, dup_positions, epl_of, order_batch, order_census, order_other,
                             order_positions, order_srcs, reference, width_of)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-crdt-playground_amd", "csrc")

_census = {}


def cen(c):
    if c.name not in _census:
        _census[c.name] = census(c)
    return _census[c.name]


# ------------------------------------------------------------------ the table itself

def test_constants_are_the_kernels():
    """The restated constants against the text of the kernels (no build is imported)."""
    sort = open(os.path.join(CSRC, "sort.hip")).read()
    wave = open(os.path.join(CSRC, "wave_sort.hpp")).read()
    pack = open(os.path.join(CSRC, "pack.hip")).read()
    assert "constexpr uint32_t kSortWaveMax = %d;" % WAVE_MAX in sort
    assert "constexpr uint32_t kSortItems = %d;" % ITEMS in sort
    assert re.search(r"if \(n <= 64\)\s+err \|= sort_doc_wave<1>", sort) and re.search(r"else if \(n <= 128\)\s+err \|= sort_doc_wave<2>", sort)
    assert "wrap || d + 0x8000ull >= 0x10000ull" in wave and "wrap || d + (1ull << 47) >= (1ull << 48)" in wave
    assert "for (uint32_t i = 1 + lane; i < m; i += %d)" % ORDER_LANES in pack


def test_width_model_bands():
    """The model of the selection at the band edges, stated by hand."""
    b = 1 << 60
    for off, w in ((-0x8000, 32), (-0x8001, 64), (0x7FFF, 32), (0x8000, 64), (-(1 << 47), 64), (-(1 << 47) - 1, 80),
                   ((1 << 47) - 1, 64), (1 << 47, 80), (0, 32)):
        assert width_of([b, b + off]) == w, off
    assert width_of([2, TOP - 1]) == 80 == width_of([TOP - 1, 2]) and width_of([3, 0]) == 32 == width_of([TOP - 2, TOP])
    assert {t: v for t, v in THRESHOLDS.values()} == {-0x8000: 32, -0x8001: 64, 0x7FFF: 32, 0x8000: 64, -(1 << 47): 64,
                                                      -(1 << 47) - 1: 80, (1 << 47) - 1: 64, 1 << 47: 80}


def test_cases_are_well_formed():
    for c in CASES:
        assert len(c.docs) == len(c.slack) >= 1, c.name
        for ents, vv in c.docs:
            assert len(vv) == c.R and all(0 <= k <= TOP and a < c.R and 0 < cnt <= TOP for k, a, cnt in ents), c.name
            if c.want != CRDT_E_DUP_KEY:
                assert len({k for k, _, _ in ents}) == len(ents), c.name
            assert len({(k, cnt) for k, _, cnt in ents}) == len(ents), c.name  # the copies of a repeated key differ
        assert set(c.claims) <= set(cen(c)) | {"threshold", "place", "run", "order", "pattern", "odd_run_alone", "pads",
                                               "pair", "triple"}, c.name
        assert (c.want == CRDT_E_CAPACITY) == (c.over is not None), c.name


def test_table_stays_small():
    n = sum(len(e) for c in CASES for e, _ in c.docs)
    assert n < 160000 and len(CASES) < 520 and max(len(e) for c in CASES for e, _ in c.docs) <= 2049, (n, len(CASES))
    assert len(ORDER_CASES) < 130


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_claims_hold(c):
    got = cen(c)
    for k, v in c.claims.items():
        if k in got:
            assert got[k] == v, (c.name, k, got[k], v)
    if "pair" in c.claims:
        assert [d[:2] for d in got["dups"]] == [c.claims["pair"]], c.name
    if "pads" in c.claims:
        assert got["epl"] * 64 - got["n"] == c.claims["pads"] and got["path"] == "wave", c.name
    if "triple" in c.claims:
        i = c.claims["triple"]
        assert [d[:2] for d in got["dups"]] == [(i - 1, i), (i, i + 1)], c.name


# ------------------------------------------------------------------ coverage of the listed edges

def test_every_width_on_every_path():
    seen = set()
    for c in CLEAN:
        g = cen(c)
        for w in g["widths"]:
            seen.add((g["path"], g["epl"] if g["path"] == "wave" else 4, w))
    assert seen >= {(p, e, w) for p, e in (("wave", 1), ("wave", 2), ("wave", 4), ("block", 4)) for w in (32, 64, 80)}


def test_thresholds_both_sides_everywhere():
    """Each of the eight thresholds, at every EPL and in either run of the block path, at element
    1, at the last live element and in the last lane's last slot: the key sits exactly there, it
    alone decides the width (without it the run is in the 32-bit band), and the pair of cases
    either side of each threshold differ in width."""
    for tname, (off, w) in THRESHOLDS.items():
        for n, epl in ((40, 1), (100, 2), (200, 4)):
            for place in ("elem1", "last_live", "last_slot"):
                c = BY_NAME["width_%s_n%d_%s" % (tname, n, place)]
                keys = [k for k, _, _ in c.docs[0][0]]
                m = len(keys)
                p = {"elem1": 1, "last_live": m - 1, "last_slot": epl * 64 - 1}[place]
                assert keys[p] == keys[0] + off and m == (epl * 64 if place == "last_slot" else n), c.name
                assert p // epl == 63 and p % epl == epl - 1 if place == "last_slot" else True
                assert all(abs(k - keys[0]) <= 100 or m > 200 for i, k in enumerate(keys) if i != p), c.name
                assert all(abs(k - keys[0]) <= 128 for i, k in enumerate(keys) if i != p), c.name
                assert cen(c)["widths"] == [w] and cen(c)["epl"] == epl and width_of(keys[:p] + keys[p + 1:]) == 32, c.name
        for place, n, r, p in (("run0_elem1", 300, 0, 1), ("run0_last_slot", 300, 0, 255), ("run1_elem1", 300, 1, 1),
                               ("run1_last_live", 300, 1, 43), ("run1_last_slot", 512, 1, 255)):
            c = BY_NAME["width_%s_n%d_%s" % (tname, n, place)]
            keys = [k for k, _, _ in c.docs[0][0]]
            run = keys[256 * r:256 * (r + 1)]
            assert len(keys) == n and run[p] == run[0] + off and cen(c)["path"] == "block", c.name
            assert (p == len(run) - 1) == (place != "run0_elem1" and place != "run1_elem1"), c.name
            assert cen(c)["widths"][r] == w and cen(c)["widths"][1 - r] == 32 and width_of(run[:p] + run[p + 1:]) == 32, c.name
    sides = {(abs(off) >> 40 > 0, off < 0): set() for off, _ in THRESHOLDS.values()}
    for off, w in THRESHOLDS.values():
        sides[(abs(off) >> 40 > 0, off < 0)].add(w)
    assert sides == {(False, True): {32, 64}, (False, False): {32, 64}, (True, True): {64, 80}, (True, False): {64, 80}}


def test_range_ends():
    for w in (32, 64):
        for n in (8, 100, 200):
            c = BY_NAME["low_end_w%d_n%d" % (w, n)]
            keys = [k for k, _, _ in c.docs[0][0]]
            assert keys[0] == 3 and min(keys) == 0 and cen(c)["widths"] == [w], c.name
            assert keys[0] - (0x8000 if w == 32 else 1 << 47) < 0  # the rebuild's base is below zero
        for epl in (1, 2, 4):
            for n in (epl * 64 - 1, epl * 64):
                c = BY_NAME["top_end_w%d_n%d" % (w, n)]
                keys = [k for k, _, _ in c.docs[0][0]]
                assert keys[0] == TOP - 2 and max(keys) == TOP and cen(c)["widths"] == [w] and cen(c)["epl"] == epl, c.name
    for name in ("wrap_b2_top", "wrap_btop_2", "wrap_b2_far", "wrap_bfar_2", "wrap_b0_top", "wrap_btop_0"):
        c = BY_NAME[name]
        keys = [k for k, _, _ in c.docs[0][0]]
        assert cen(c)["widths"] == [80], name
        # without the wrap test the offsets alone would pack
        b = keys[0]
        assert all((k - b + (1 << 47)) % (1 << 64) < 1 << 48 for k in keys), name
    assert [k for k, _, _ in BY_NAME["top_alone"].docs[0][0]] == [TOP]
    assert BY_NAME["empty_alone"].docs[0][0] == [] and [k for k, _, _ in BY_NAME["zero_alone"].docs[0][0]] == [0]


def test_sizes_and_block_shapes():
    for n in WAVE_SIZES:
        for order in ("sorted", "reversed", "permuted"):
            c = BY_NAME["size_%d_%s" % (n, order)]
            keys = [k for k, _, _ in c.docs[0][0]]
            assert len(keys) == n and cen(c)["path"] == "wave" and cen(c)["epl"] == epl_of(n)
            if order == "sorted":
                assert keys == sorted(keys)
            elif order == "reversed":
                assert keys == sorted(keys, reverse=True)
            elif n > 2:
                assert keys != sorted(keys) and keys != sorted(keys, reverse=True)
    assert set(WAVE_SIZES) == {0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256}
    c = BY_NAME["empty_between_two_full"]
    assert [len(e) for e, _ in c.docs] == [64, 0, 64]
    assert set(BLOCK_SIZES) == {257, 263, 511, 512, 513, 768, 769, 1024, 1025, 2048, 2049}
    passes = set()
    for n in BLOCK_SIZES:
        for pattern in PATTERNS:
            c = BY_NAME["block_%d_%s" % (n, pattern)]
            g = cen(c)
            keys = [k for k, _, _ in c.docs[0][0]]
            runs = [keys[i:i + WAVE_MAX] for i in range(0, n, WAVE_MAX)]
            assert g["path"] == "block" and g["n"] == n and g["runs"] == len(runs)
            if pattern == "sorted":
                assert keys == sorted(keys)
            elif pattern == "reversed":
                assert keys == sorted(keys, reverse=True)
            elif pattern == "runs_descend":
                assert all(min(runs[r]) > max(runs[r + 1]) for r in range(len(runs) - 1))
            elif pattern == "runs_ascend":
                assert all(max(runs[r]) < min(runs[r + 1]) for r in range(len(runs) - 1)) and keys != sorted(keys)
            elif pattern == "interleaved":
                rank = {k: i for i, k in enumerate(sorted(keys))}
                lead = min(len(r) for r in runs) * len(runs)  # while every run has room, the ranks go round the runs
                assert all(rank[k] % len(runs) == r for r, run in enumerate(runs) for k in run if rank[k] < lead)
            else:
                assert min(keys) == 0 and max(keys) == TOP and 80 in g["widths"]
                passes.add(g["passes"])
    assert passes == {1, 2, 3, 4}
    assert {cen(BY_NAME["block_%d_sorted" % n])["runs"] % 2 for n in BLOCK_SIZES} == {0, 1}  # a run left alone in a pass


def test_dup_positions_in_every_width():
    want = {61: {(0, 1), (59, 60), (15, 16), (31, 32), (47, 48)},
            125: {(0, 1), (123, 124), (1, 2), (31, 32), (63, 64), (95, 96)},
            253: {(0, 1), (251, 252), (3, 4), (63, 64), (127, 128), (191, 192)},
            600: {(0, 1), (598, 599), (255, 256), (7, 8), (511, 512)}}
    assert set(DUP_SIZES) == set(want)
    for n in DUP_SIZES:
        assert {(i - 1, i) for i in dup_positions(n).values()} == want[n]
        for w in (32, 64, 80):
            for pname, i in dup_positions(n).items():
                c = BY_NAME["dup_w%d_n%d_%s" % (w, n, pname)]
                g = cen(c)
                assert g["dups"][0][:2] == (i - 1, i) and len(g["dups"]) == 1 and set(g["widths"]) == {w}, c.name
                if n <= WAVE_MAX:
                    lane, slot = g["dups"][0][2:]
                    assert (lane, slot) == (i // epl_of(n), i % epl_of(n))
                    if pname.startswith("row"):
                        assert slot == 0 and lane in (16, 32, 48)  # the predecessor comes over a DPP row edge
                    if pname == "lane0_1":
                        assert (lane, slot) == (1, 0)
    # at EPL 2 and 4 a pair inside one lane too, and across runs on the block path (what the merge orders)
    assert cen(BY_NAME["dup_w32_n125_first"])["dups"][0][2:] == (0, 1) and cen(BY_NAME["dup_w32_n253_first"])["dups"][0][2:] == (0, 1)
    assert any(len(r) > 1 for c in DUP_CASES if cen(c)["path"] == "block" for runs in cen(c)["dup_runs"] for r in [set(runs)])
    for n in (61, 253, 600):
        assert cen(BY_NAME["dup_zero_n%d" % n])["dup_key"] == 0 and cen(BY_NAME["dup_pad_key_n%d" % n])["dup_key"] == TOP
        assert len(cen(BY_NAME["dup_triple_n%d" % n])["dups"]) == 2
    for w in (32, 64, 80):
        g = cen(BY_NAME["dup_is_b_w%d" % w])
        assert g["first"] == g["dup_key"] and g["widths"] == [w]
    for n in (63, 127, 255):
        c = BY_NAME["top_then_pads_n%d" % n]
        assert max(k for k, _, _ in c.docs[0][0]) == TOP and c.want is None and cen(c)["widths"] == [32]


def test_every_dup_case_has_its_clean_twin():
    assert len(DUP_CASES) >= 66
    for c in DUP_CASES:
        t = BY_NAME[c.twin]
        assert t.want is None and t in CLEAN and t.R == c.R and t.slack == c.slack
        a, b = c.docs[0][0], t.docs[0][0]
        assert len(a) == len(b)
        diff = [i for i in range(len(a)) if a[i] != b[i]]
        seen = set()
        later = []  # input positions holding a second or third copy
        for i, (k, _, _) in enumerate(a):
            if k in seen:
                later.append(i)
            seen.add(k)
        assert set(diff) <= set(later) | {i for i in range(len(a)) if a[i][0] == cen(c)["dup_key"]}, c.name
        assert 1 <= len(later) <= 2 and {k for k, _, _ in b} - {k for k, _, _ in a}, c.name  # replaced by unused keys
        assert not cen(t)["dups"]


def test_reference_is_strictly_ascending():
    for c in CLEAN:
        for want, vv in reference(c):
            keys = [k for k, _, _ in want]
            assert all(keys[i] < keys[i + 1] for i in range(len(keys) - 1)), c.name
    for c in DUP_CASES:  # not strictly: the copies side by side, in input order
        (want, _), = reference(c)
        keys = [k for k, _, _ in want]
        assert all(keys[i] <= keys[i + 1] for i in range(len(keys) - 1)) and sorted(want) == sorted(c.docs[0][0])
        ents = c.docs[0][0]
        for i in range(len(keys) - 1):
            if keys[i] == keys[i + 1]:
                assert ents.index(want[i]) < ents.index(want[i + 1])


def test_concatenated_table_is_the_cases():
    for R in (1, 3, 64):
        cases = clean_of(R)
        assert cases
        b, first = concat(cases, extra=2, fill="continuation")
        for c, f in zip(cases, first):
            for d, (ents, vv) in enumerate(c.docs):
                assert b.doc(f + d) == (ents, vv), c.name
    assert {c.R for c in CLEAN} == {1, 3, 64}


def test_layout_cases():
    for R in (1, 3, 64):
        c = BY_NAME["layout_R%d" % R]
        sizes = [len(e) for e, _ in c.docs]
        assert sizes[0] > WAVE_MAX and sizes[-1] > WAVE_MAX and 0 in sizes and set(c.slack) == {0, 1, 9}
        assert c.slack[sizes.index(0)] == 9  # count == 0 over slots that hold something under the ones / continuation fill
        for fill in FILLS[1:]:
            b = batch_of(c, fill=fill)
            o = int(b.offsets[sizes.index(0)])
            assert (b.keys[o:o + 9] != 0).all()


def test_over_count_cases_stay_inside_the_arrays():
    assert {c.name for c in OVER_CASES} == {"over_wave", "over_block", "over_250_claims_259"}
    for c in OVER_CASES:
        d, above = c.over
        b = batch_of(c)
        slots = int(b.offsets[d + 1]) - int(b.offsets[d])
        cnt = int(b.counts[d])
        assert cnt == slots + above > slots and d < b.n_docs - 1 and above >= 9, c.name
        assert int(b.offsets[d]) + cnt <= int(b.offsets[-1]) == len(b.keys), c.name  # reads and writes: the same slots
        spare = int(b.offsets[d + 2]) - int(b.offsets[d + 1]) - int(b.counts[d + 1])
        assert spare >= above, c.name
        g = cen(c)
        assert g["path"] == c.claims["path"] and g["unclamped_path"] == c.claims["unclamped_path"] and g["n"] == slots, c.name
    assert cen(BY_NAME["over_block"])["path"] == "block" and cen(BY_NAME["over_wave"])["path"] == "wave"


def test_sentinel_is_no_value_of_the_table():
    """0x5A5A... (tests/test_gpu_sort_edges.py prefills the outputs with it) is no key, actor,
    counter or clock word of any case, under any fill."""
    for R in (1, 3, 64):
        for fill in FILLS:
            b, _ = concat(clean_of(R), extra=2, fill=fill)
            assert not (b.keys == 0x5A5A5A5A5A5A5A5A).any() and not (b.counters == 0x5A5A5A5A5A5A5A5A).any()
            assert not (b.actors == 0x5A5A5A5A).any() and not (b.vv == 0x5A5A5A5A5A5A5A5A).any()
    for c in DUP_CASES + OVER_CASES:
        b = batch_of(c)
        assert not (b.keys == 0x5A5A5A5A5A5A5A5A).any() and not (b.counters == 0x5A5A5A5A5A5A5A5A).any()


# ------------------------------------------------------------------ the order cases

def validate(b):
    return crdtgpu.validate(b)


def order_verdict(c):
    rc = validate(order_batch(c))
    if rc == 0 and c.srcs is not None:
        rc = crdtgpu.validate_src(order_srcs(c))
    return rc


@pytest.mark.parametrize("c", ORDER_CASES, ids=lambda c: c.name)
def test_order_case(c):
    """The hand-stated verdict is the host validators'; the claims are the census; the violation
    is the only one, in document 1, and the other side of the join is clean."""
    assert order_verdict(c) == c.want in (0, CRDT_E_UNSORTED), c.name
    got = order_census(c)
    for k, v in c.claims.items():
        if k in got:
            assert got[k] == v, (c.name, k, got[k], v)
    assert got["n_bad"] == (1 if c.want and c.srcs is None else 0)
    assert validate(order_other(c)) == 0 and order_other(c).n_docs == len(c.docs)
    assert c.counted or not any(c.slack_rows)
    for d in (0, 2):
        keys = [k for k, _, _ in c.docs[d][0]]
        assert keys == sorted(set(keys))
    if c.srcs is not None:
        assert validate(order_batch(c)) == 0
        s = order_srcs(c)
        tombs = crdtgpu.TombBatch(s.tomb_off, s.tkeys, s.tactors, s.tcounters)
        assert validate_tombs(tombs, s.n_srcs) == (CRDT_E_UNSORTED if "bad_tombs" in c.name else 0)


def test_order_positions_with_and_without_counts():
    assert set(ORDER_SIZES) == {0, 1, 2, 64, 65, 66, 130}
    seen = set()
    for m in ORDER_SIZES:
        for pname, i in order_positions(m).items():
            for kind in ("inversion", "equal"):
                for tag, counted in (("counts", True), ("no_counts", False)):
                    c = ORDER_BY_NAME["order_%s_m%d_%s_%s" % (kind, m, pname, tag)]
                    g = order_census(c)
                    assert g["pair"] == (i - 1, i) and c.counted == counted and order_batch(c).counts is not None or not counted
                    assert (order_batch(c).counts is None) == (not counted)
                    keys = [k for k, _, _ in c.docs[1][0]]
                    assert (keys[i] == keys[i - 1]) == (kind == "equal")
                    seen.add((g["pair"], g["lane"], g["step"]))
    assert {((0, 1), 0, 0), ((63, 64), 63, 0), ((64, 65), 0, 1), ((128, 129), 0, 2), ((62, 63), 62, 0), ((65, 64)[::-1], 0, 1)} <= seen
    # the descents that are no violation are really there
    c = ORDER_BY_NAME["order_descent_inside_slack"]
    rows = [k for k, _, _ in c.slack_rows[1]]
    assert any(rows[i] <= rows[i - 1] for i in range(1, len(rows))) and rows[0] > c.docs[1][0][-1][0]
    c = ORDER_BY_NAME["order_descent_live_to_slack"]
    assert all(c.slack_rows[d][0][0] < c.docs[d][0][-1][0] for d in range(3))
    c = ORDER_BY_NAME["order_descent_doc_to_doc"]
    assert c.docs[0][0][-1][0] > c.docs[1][0][0][0] and c.docs[1][0][-1][0] > c.docs[2][0][0][0] and not c.counted
    for m in (0, 1):
        c = ORDER_BY_NAME["order_m%d_over_garbage" % m]
        rows = [k for k, _, _ in c.slack_rows[1]]
        assert len(c.docs[1][0]) == m and len(rows) > ORDER_LANES and any(rows[i] <= rows[i - 1] for i in range(1, len(rows)))
    c = ORDER_BY_NAME["order_top_then_zero_counts"]
    assert [k for k, _, _ in c.docs[1][0]][-2:] == [TOP, 0]
    s = order_srcs(ORDER_BY_NAME["order_fold_no_sources_then_bad_tombs"])
    assert list(s.doc_srcs) == [0, 0, 0, 1] and list(s.entry_off) == [0, 0] and list(s.tomb_off) == [0, 2]
    assert np.asarray(order_batch(ORDER_BY_NAME["order_fold_clean"]).counts).tolist() == [3, 66, 3]
