"""CPU: the case table of tests/extract_edge_cases.py reaches every edge it was built for, and
the restatement it is checked against on the GPU is held to the reference's merge.

Every census test below asserts, from `census` alone (the layout of a case: groups, staged
runs, source starts, empty sources, kept lanes per 64-position chunk), that at least one
named case reaches one edge of extract_kernel (csrc/extract.hip); an edit to the table that
drops an edge fails the test that names it.  The fold property -- folding the extracted
message into a receiver whose clock is the peer clock gives what folding the full states
gives, with the map-based reference's own (*AWSetDelta).Merge -- is checked on every document
of every case.
"""

import pytest

import test_delta_extract_model as model
from extract_edge_cases import (BIG_ACTOR, BY_NAME, CASES, CHUNK, GEOMETRY_R, HALF, KIND_DOCS, RUN, RUN_SIZES, TOP, TOTALS,
                                WAVE, census, expected, group_size, receiver)
from helpers import ref
from test_delta_extract_model import DELTA, FULL, NONE

CENSUS = {c.name: census(c) for c in CASES}
ALL = (1 << 64) - 1
ALT = (0x5555555555555555, 0xAAAAAAAAAAAAAAAA)


def runs():
    """(case, group census, run index, run census) of every staged run of the table."""
    for c in CASES:
        for g in CENSUS[c.name]["groups"]:
            for r, run in enumerate(g["runs"]):
                yield c, g, r, run


def some(pred, what):
    hits = [c.name for c, g, r, run in runs() if pred(c, g, r, run)]
    assert hits, "no case reaches: " + what
    return hits


def sources(case):
    return [(d, s) for d, doc in enumerate(case.per_doc) for s in doc]


# ------------------------------------------------------------------ the table itself

def test_constants_are_the_kernels():
    """The restated constants against the text of the kernel (no build is imported)."""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-crdt-playground_amd", "csrc",
                            "extract.hip")).read()
    assert int(re.search(r"constexpr uint32_t kExSrcs = (\d+);", src).group(1)) == RUN
    assert "const uint32_t G = 64u / sv.R;" in src and WAVE == 64
    assert src.count("base += 64") == 2 and CHUNK == 64


def test_cases_are_well_formed():
    for c in CASES:
        assert len(c.per_doc) == len(c.peers) and all(len(P) == c.R for P in c.peers), c.name
        for d, s in sources(c):
            a, vv, ents, tombs = s
            assert len(vv) == c.R and a != c.R, c.name
            for rows in (ents, tombs or []):
                keys = [k for k, _, _ in rows]
                assert keys == sorted(set(keys)) and all(0 <= k <= TOP for k in keys), (c.name, d)
        if c.tombs != "given":
            assert all(s[3] is None for _, s in sources(c)), c.name
        expected(c)  # no case panics


def test_table_stays_small():
    n = sum(len(s[2]) + len(s[3] or []) for c in CASES for _, s in sources(c))
    assert n < 40000 and len(CASES) < 120, (n, len(CASES))


# ------------------------------------------------------------------ R and groups

def test_every_R_and_group_count():
    for R in GEOMETRY_R:
        G = group_size(R)
        shapes = {(len(cen["groups"]), cen["groups"][-1]["nd"]) for c in CASES if c.R == R and c.name.startswith("geo_")
                  for cen in [CENSUS[c.name]]}
        if G > 1:  # one document, one partial group, one full group, full + one document, two full groups
            want = {(1, 1), (1, G - 1), (1, G), (2, 1), (2, G)}
        else:
            want = {(1, 1), (2, 1), (3, 1)}
        assert want <= shapes, (R, want - shapes)
    assert group_size(1) == 64 and [group_size(R) * R for R in (5, 21, 22, 31, 33, 63)] == [60, 63, 44, 62, 33, 63]


def test_a_group_of_no_sources_and_a_document_of_none():
    some(lambda c, g, r, run: 0 in g["doc_srcs"] and g["n_srcs"] > 0, "a document without sources inside a group")
    assert any(g["n_srcs"] == 0 for c in CASES for g in CENSUS[c.name]["groups"]), "a group without sources"


def test_neighbouring_documents_would_change_every_answer():
    """Geometry cases: under the clock of either neighbouring document every source changes
    its kind, and at least one entry of every source that has some is kept instead of
    withheld or withheld instead of kept."""
    for c in CASES:
        if not c.name.startswith("geo_"):
            continue
        n = len(c.per_doc)
        for d, s in sources(c):
            for o in (d - 1, d + 1):
                if not 0 <= o < n or o // group_size(c.R) != d // group_size(c.R):
                    continue
                assert c.peers[o] != c.peers[d]
                mine, theirs = model.extract_ref(s, c.peers[d]), model.extract_ref(s, c.peers[o])
                assert (mine[0] == FULL) != (theirs[0] == FULL), (c.name, d, o)
                assert mine[1] != theirs[1], (c.name, d, o)
        # the first document's clock (lane 0) answers differently for some later document of a group
        G = group_size(c.R)
        for d, s in sources(c):
            if d % G and model.extract_ref(s, c.peers[d - d % G]) != model.extract_ref(s, c.peers[d]):
                break
        else:
            assert n == 1 or G == 1 or all(not doc for doc in c.per_doc[1:]), c.name


def test_last_lanes_hold_a_clock_word_that_matters():
    """Some source's actor, and some entry's, is R - 1 in the last document of a full group."""
    for R in GEOMETRY_R:
        c = BY_NAME["geo_R%d_docs%d" % (R, group_size(R) if group_size(R) > 1 else 1)]
        G = group_size(R)
        tail = [s for d, s in sources(c) if d >= G - 2]  # (the last or the one before: one of them sees R - 1)
        assert any(s[0] == R - 1 for s in tail) and any(a == R - 1 for s in tail for _, a, _ in s[2]), R


# ------------------------------------------------------------------ staging runs

@pytest.mark.parametrize("n", RUN_SIZES)
def test_group_of_exactly_n_sources(n):
    hits = some(lambda c, g, r, run: g["n_srcs"] == n, "a group of %d sources" % n)
    assert "run_%d" % n in hits
    g = [g for g in CENSUS["run_%d" % n]["groups"] if g["n_srcs"] == n][0]
    assert [run["n"] for run in g["runs"]] == [RUN] * (n // RUN) + ([n % RUN] if n % RUN else [])
    assert len(g["doc_srcs"]) == 32 and max(g["doc_srcs"]) > 64 and 0 in g["doc_srcs"]


def seam(name):
    """(last source of run 0, first of run 1) of the named case's heavy group: True where empty."""
    g = [g for g in CENSUS[name]["groups"] if g["n_srcs"] > RUN][0]
    r0, r1 = g["runs"][0], g["runs"][1]
    assert r0["n"] == RUN
    empty = lambda run, i: i in run["e_empty"] and i in run["t_empty"]  # noqa: E731
    return empty(r0, RUN - 1), empty(r1, 0), r0, r1


def test_seam_at_128():
    assert seam("seam_nonempty_both_sides")[:2] == (False, False)
    assert seam("seam_empty_last_of_run0")[:2] == (True, False)
    assert seam("seam_empty_first_of_run1")[:2] == (False, True)
    last, first, r0, r1 = seam("seam_empty_on_both_sides")
    assert (last, first) == (True, True)
    # both are flanked by sources that hold entries and tombstones
    assert r0["e_sizes"][RUN - 2] and r0["t_sizes"][RUN - 2] and r1["e_sizes"][1] and r1["t_sizes"][1]


def test_run_of_128_empty_sources_between_two_that_are_not():
    g = [g for g in CENSUS["run_of_128_empties"]["groups"] if g["n_srcs"] > RUN][0]
    r0, r1, r2 = g["runs"]
    assert r1["n"] == RUN and r1["e_empty"] == list(range(RUN)) and r1["t_empty"] == list(range(RUN))
    assert r1["kinds"] == [NONE] * RUN
    for r in (r0, r2):
        assert r["e_kept"] and r["t_kept"]
    assert r0["e_sizes"][-1] and r2["e_sizes"][0]


def test_run_that_keeps_nothing_before_one_that_does():
    g = [g for g in CENSUS["run_keeps_nothing"]["groups"] if g["n_srcs"] > RUN][0]
    r0, r1 = g["runs"]
    assert r0["kinds"] == [NONE] * RUN and r0["e_total"] == 3 * RUN and r0["e_kept"] == 0 and r0["t_total"] == 0
    assert not r0["e_empty"] and all(m == 0 for m, _ in r0["e_masks"])
    assert r1["e_kept"] and r1["t_kept"]


def test_one_document_of_130_sources_at_G_1():
    cen = CENSUS["one_doc_130_sources_R64"]
    assert cen["G"] == 1 and [g["n_srcs"] for g in cen["groups"]] == [1, 130, 1]
    assert [r["n"] for r in cen["groups"][1]["runs"]] == [128, 2]


# ------------------------------------------------------------------ empty sources inside a run

def stretches(empty, n):
    """Maximal stretches of consecutive indices of `empty`, as (first, length, where): before the
    run's first non-empty source, between two, or at the end."""
    out, full = [], [i for i in range(n) if i not in empty]
    i = 0
    while i < n:
        if i in empty:
            j = i
            while j + 1 < n and j + 1 in empty:
                j += 1
            where = "first" if not full or j < full[0] else "last" if i > full[-1] else "between"
            out.append((i, j - i + 1, where))
            i = j + 1
        else:
            i += 1
    return out


@pytest.mark.parametrize("which", ["both", "e", "t"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_consecutive_empty_sources(which, n):
    """n consecutive empty sources first, between and last in a run -- empty of entries,
    of tombstones, or of both -- in the case named for it."""
    run = CENSUS["empties_%s_%d" % (which, n)]["groups"][1]["runs"][0]
    for col in {"both": ("e_empty", "t_empty"), "e": ("e_empty",), "t": ("t_empty",)}[which]:
        got = [(length, where) for _, length, where in stretches(set(run[col]), run["n"])]
        assert got == [(n, "first"), (n, "between"), (n, "last")], (col, got)
    if which == "e":
        assert not run["t_empty"]
    if which == "t":
        assert not run["e_empty"]


def test_empty_stretches_first_and_last_in_a_run():
    for col in ("e_empty", "t_empty"):
        for n in (1, 2, 3):
            for where in ("first", "last"):
                some(lambda c, g, r, run: (n, where) in {(ln, w) for _, ln, w in stretches(set(run[col]), run["n"])},
                     "%d %s at the %s of a run" % (n, col, where))


def test_all_dropped_source_next_to_an_empty_one():
    run = CENSUS["all_dropped_next_to_empty"]["groups"][0]["runs"][0]
    dropped = [i for i in range(run["n"]) if run["e_sizes"][i] and run["kinds"][i] == NONE]
    assert any(i + 1 in run["e_empty"] for i in dropped) and any(i - 1 in run["e_empty"] for i in dropped)
    assert dropped[-1] == run["n"] - 2 and run["n"] - 1 in run["e_empty"]  # and the pair ends a run


# ------------------------------------------------------------------ chunks

@pytest.mark.parametrize("col", ["e", "t"])
@pytest.mark.parametrize("n", TOTALS)
def test_run_total(col, n):
    hits = some(lambda c, g, r, run: run[col + "_total"] == n and run["n"] > 0, "a run of %d %s" % (n, col))
    assert "%s_total_%d" % (col, n) in hits
    first = CENSUS["%s_total_%d" % (col, n)]["groups"][0]["runs"][0]
    assert first[col + "_total"] % 64 != 0  # the run under test does not start at a multiple of 64


@pytest.mark.parametrize("col", ["e", "t"])
@pytest.mark.parametrize("pos", [0, 63, 64, 65])
def test_source_start_at_run_position(col, pos):
    some(lambda c, g, r, run: any(s == pos and run[col + "_sizes"][i] for i, s in enumerate(run[col + "_starts"])),
         "a non-empty source starting at %s position %d" % (col, pos))
    run = CENSUS["%s_total_129" % col]["groups"][1]["runs"][0]
    assert run[col + "_starts"] == [0, 63, 64, 65]


@pytest.mark.parametrize("col", ["e", "t"])
def test_chunk_masks(col):
    masks = CENSUS[col + "_masks"]["groups"][1]["runs"][0][col + "_masks"]
    assert [v for _, v in masks] == [64] * 6
    m = [x for x, _ in masks]
    assert m[0] == ALL and m[1] == 0 and m[2] == 1 and m[3] == 1 << 63 and m[4] in ALT and m[5] == ALL
    assert m[0] and not m[1] and m[2]  # a middle chunk that keeps nothing between two that do
    # and a partial last chunk somewhere: every lane, and lane 0 alone
    key = col + "_masks"
    some(lambda c, g, r, run: any(0 < v < 64 and x == (1 << v) - 1 for x, v in run[key]), "a full partial chunk")
    some(lambda c, g, r, run: any(x and v == 1 for x, v in run[key]), "a chunk of one position, kept")


# ------------------------------------------------------------------ the re-add filter

def tomb_facts(case):
    """Per tombstone of the case: (relation of its key to the source's entry keys, what the entry
    under that key is to it, kept)."""
    out = []
    for d, s in sources(case):
        _, _, ents, tombs = s
        kept = {t[0] for t in model.extract_ref(s, case.peers[d])[2]}
        keys = [k for k, _, _ in ents]
        emap = {k: (a, c) for k, a, c in ents}
        for k, a, c in tombs or []:
            where = ("none" if not keys else "below" if k < keys[0] else "above" if k > keys[-1] else
                     "first" if k == keys[0] else "last" if k == keys[-1] else "inside")
            if k in emap:
                ea, ec = emap[k]
                what = "other" if ea != a else "lower" if ec < c else "equal" if ec == c else "higher"
            else:
                what = "absent"
            out.append(dict(where=where, what=what, kept=k in kept, key=k, actor=a, R=case.R, ne=len(ents), nt=len(tombs)))
    return out


def test_readd_filter_positions_and_dots():
    facts = tomb_facts(BY_NAME["readd_positions"])
    seen = {(f["where"], f["what"], f["kept"]) for f in facts}
    for want in (("none", "absent", True), ("below", "absent", True), ("above", "absent", True),
                 ("first", "higher", False), ("last", "higher", False), ("first", "equal", True), ("last", "lower", True),
                 ("first", "other", False), ("last", "other", False)):
        assert want in seen, want
    keys = {(f["key"], f["what"] != "absent") for f in facts}
    assert {(0, True), (0, False), (HALF, True), (HALF, False), (TOP, True), (TOP, False)} <= keys
    beyond = [f for f in facts if f["actor"] >= f["R"]]
    assert {f["actor"] for f in beyond} >= {3, 4, BIG_ACTOR}
    assert {(f["what"], f["kept"]) for f in beyond} >= {("absent", True), ("other", False), ("equal", True)}


@pytest.mark.parametrize("nt", [64, 65])
@pytest.mark.parametrize("ne", [1, 130])
def test_readd_filter_sizes(nt, ne):
    facts = [f for f in tomb_facts(BY_NAME["readd_%d_tombs_%d_entries" % (nt, ne)]) if f["nt"] == nt]
    assert len(facts) == nt and {f["ne"] for f in facts} == {ne}
    assert {f["kept"] for f in facts} == {True, False} or ne == 1
    if ne > 1:
        assert {f["what"] for f in facts} == {"absent", "other", "equal", "higher", "lower"}
        assert {f["where"] for f in facts} >= {"first", "inside"}
    else:
        assert {f["where"] for f in facts} == {"below", "first", "above"}  # (one entry: first is last)


def test_tombstones_of_a_source_without_entries():
    some(lambda c, g, r, run: any(i in run["e_empty"] and run["t_sizes"][i] for i in range(run["n"])),
         "tombstones of a source with no entries")


# ------------------------------------------------------------------ kinds and coverage

def test_kinds_and_coverage():
    c = BY_NAME["kinds"]
    R = c.R
    doc = lambda name: KIND_DOCS.index(name)  # noqa: E731
    out = lambda name: [model.extract_ref(s, c.peers[doc(name)]) for s in c.per_doc[doc(name)]]  # noqa: E731
    assert out("full_empty_state") == [(FULL, [], [])]
    d = doc("full_actor_above_R")
    assert all(s[0] > R for s in c.per_doc[d]) and 0 not in c.peers[d] and [o[0] for o in out("full_actor_above_R")] == [FULL] * 2
    assert {s[0] for s in c.per_doc[d]} == {R + 1, BIG_ACTOR}
    (kind, ents, _), = out("full_entries_at_actor_R")
    assert kind == FULL and [a for _, a, _ in ents].count(R) == 2
    (kind, ents, _), = out("delta_equal_below_top")
    P = c.peers[doc("delta_equal_below_top")]
    assert kind == DELTA and ents == [(2, 0, 6), (5, 2, TOP)] and TOP in P
    src = c.per_doc[doc("delta_equal_below_top")][0]
    rel = {(c_ - P[a]) for _, a, c_ in src[2]}
    assert {0, 1, -1} <= rel  # covered at equal, kept at one above the peer, covered below
    (kind, ents, _), = out("delta_entry_above_R")
    assert kind == DELTA and [a for _, a, _ in ents] == [R + 1, BIG_ACTOR]
    assert [(k, len(e), len(t)) for k, e, t in out("delta_one_tombstone_no_entry")] == [(DELTA, 0, 1), (DELTA, 0, 1)]
    assert out("none") == [(NONE, [], [])] * 3
    assert [len(s[2]) + len(s[3] or []) for s in c.per_doc[doc("none")]] == [2, 0, 2]
    side = out("full_and_delta_side_by_side")
    assert [k for k, _, _ in side] == [DELTA, FULL, DELTA, DELTA]
    assert [len(e) for _, e, _ in side] == [2, 3, 2, 1]
    # every kind occurs in one group, and the case is one group
    assert len(CENSUS["kinds"]["groups"]) == 1
    assert set(CENSUS["kinds"]["groups"][0]["runs"][0]["kinds"]) == {NONE, DELTA, FULL}


def test_optional_arrays():
    assert BY_NAME["kind_null"].kind_null and BY_NAME["kind_null"].tombs == "given"
    assert {c.tombs for c in CASES} == {"given", "out_null", "out_given"}
    for name in ("no_tombs_out_arrays_null", "no_tombs_out_tomb_off_given"):
        kinds, _ = expected(BY_NAME[name])
        assert set(kinds) == {DELTA, FULL} and len(CENSUS[name]["groups"]) == 2


# ------------------------------------------------------------------ the property

@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_message_folds_like_the_full_states(case):
    """fold(receiver, extract(sources, P)) == fold(receiver, sources) per document, with the
    receiver's clock == P; where the reference panics on the full states (an entry dot at
    actor R reaches HasDot on the receiving side) it panics on the message as well."""
    shipped = withheld = 0
    for d, srcs in enumerate(case.per_doc):
        if not srcs:
            continue
        ents, vv = receiver(case, d)
        _, msg = model.extract_doc_ref(srcs, case.peers[d])
        shipped += sum(len(m[2]) for m in msg)
        withheld += sum(len(s[2]) - len(m[2]) for s, m in zip(srcs, msg))
        try:
            want = model.fold_ref(ents, vv, srcs)
        except ref.GoPanic:
            with pytest.raises(ref.GoPanic):
                model.fold_ref(ents, vv, msg)
            continue
        assert model.fold_ref(ents, vv, msg) == want, (case.name, d)
    assert shipped or withheld
