"""CPU: the fold edge cases (tests/fold_edge_cases.py) are valid, land on the
dispatch edges of csrc/fold.hip they are built for (tests/fold_paths.py's
census), and fold to something: most outputs non-empty, with surviving dst
entries, surviving source entries, replaced dots and removed dst entries in
every case.  The floors are conditions on the cases, not measurements: a case
that misses one is fixed, the floor stays."""

from collections import Counter

import pytest

import fold_edge_cases as fe
import fold_paths as fp
from fold_edge_cases import AWSET, DELTA
from oracle import oracle

FLOOR = 8
_memo = {}


def oracle_of(name):
    """[(rc, want)] per batch of a case, computed once and shared."""
    if name not in _memo:
        c = fe.all_cases()[name]
        _memo[name] = [oracle.fold(c.mode, dst, srcs) for dst, srcs in c.batches]
    return _memo[name]


def records(name, lean):
    key = (name, "rec", lean)
    if key not in _memo:
        c = fe.all_cases()[name]
        _memo[key] = [r for dst, srcs in c.batches for r in fp.classify(c.mode, lean, dst, srcs)]
    return _memo[key]


CASES = sorted(fe.all_cases())


@pytest.mark.parametrize("name", CASES)
def test_oracle_accepts_the_case(name):
    for rc, _ in oracle_of(name):
        assert rc == 0


@pytest.mark.parametrize("name", CASES)
def test_case_hits_the_classes_it_is_named_for(name):
    c = fe.all_cases()[name]
    assert c.classes
    for label, lean, pred in c.classes:
        got = sum(1 for r in records(name, lean) if pred(r))
        assert got >= FLOOR, "%s: %d documents in class %r (floor %d)" % (name, got, label, FLOOR)


def phenomena(dst, srcs, want, mode):
    """Counter of what the oracle's output shows against the input, over a batch."""
    c = Counter()
    dst, srcs = dst.numpy(), srcs.numpy()
    for d in range(dst.n_docs):
        ents, _, chain = fp.doc_lists(dst, srcs, d)
        o, n = int(want.offsets[d]), int(want.counts[d])
        out = list(zip(want.keys[o:o + n].tolist(), want.actors[o:o + n].tolist(), want.counters[o:o + n].tolist()))
        c["docs"] += 1
        c["non-empty"] += bool(out)
        dmap = {k: (a, cc) for k, a, cc in ents}
        src_dots = {(k, a, cc) for _, _, e, _ in chain for k, a, cc in e}
        okeys = {k for k, _, _ in out}
        for k, a, cc in out:
            if k in dmap:
                c["surviving dst entry" if dmap[k] == (a, cc) else "replaced dot"] += 1
            elif (k, a, cc) in src_dots:
                c["surviving source entry"] += 1
        c["removed dst entry"] += sum(1 for k in dmap if k not in okeys)
    return c


@pytest.mark.parametrize("name", CASES)
def test_case_is_not_trivial(name):
    c = fe.all_cases()[name]
    tot = Counter()
    for (dst, srcs), (rc, want) in zip(c.batches, oracle_of(name)):
        tot += phenomena(dst, srcs, want, c.mode)
    assert 2 * tot["non-empty"] >= tot["docs"], (name, dict(tot))
    for what in ("surviving dst entry", "surviving source entry", "replaced dot", "removed dst entry"):
        assert tot[what] > 0, (name, what, dict(tot))


def whole_census():
    key = "census"
    if key not in _memo:
        tot = Counter()
        for name in CASES:
            for lean in (1, 0):
                tot += fp.census(records(name, lean))
        _memo[key] = tot
    return _memo[key]


REACHABLE = ([("lean", b) for b in ("0", "1..15")] +
             [(p, b) for p in ("general-direct", "general-deferred") for b in ("0", "1..15", "16..32", "33..63", "64")] +
             [("block", b) for b in fp.MS_BANDS])


def test_census_floor_over_the_module(capsys):
    tot = whole_census()
    with capsys.disabled():
        print("\nfold path census (documents per class, both lean settings, all cases):")
        for k in sorted(tot):
            print("  %-44s %6d" % (k, tot[k]))
    need = ["pass=%s ms=%s" % pb for pb in REACHABLE]
    need += ["tomb_search=binary", "tomb_search=table", "tomb_search=binary readd=True", "tomb_search=binary readd=False",
             "noop_replay ms>15", "resolve=slot-walk", "resolve=sort", "seq_walk"]
    need += ["sort kc_tier=%s" % t for t in fp.KC_TIERS]
    need += ["why=%s" % w for w in fp.WHYS]
    short = {k: tot[k] for k in need if tot[k] < FLOOR}
    assert not short, short
    # nothing outside the reachable table either: a new combination means the restatement is off
    seen = {k for k in tot if k.startswith("pass=") and " ms=" in k}
    assert seen <= set(need), seen - set(need)


def test_run_and_grid_edges_are_placed():
    """The document-count ladder meets: a one-document batch, a last run of one and of
    K documents, a grid that is and is not a multiple of the 8 XCDs, and -- in the
    deferred list of a delta fold -- fewer deferred documents than waves (kr < K)."""
    for mode in (AWSET, DELTA):
        k = fp.T("K_DELTA") if mode == DELTA else fp.T("K_AWSET")
        geo = [fp.run_edges(mode, 1, n) for n in fe.DOC_COUNTS[mode]]
        assert {1, k} <= {last for _, last, _ in geo}
        assert {g % fp.T("XCDS") == 0 for g, _, _ in geo} == {True, False}
        assert any(g == 1 for g, _, _ in geo) and any(g > fp.T("XCDS") for g, _, _ in geo)
    c = fe.all_cases()["doc_count_ladder_delta"]
    n_def = [sum(r["pass"] != "lean" for r in fp.classify(DELTA, 1, dst, srcs)) for dst, srcs in c.batches]
    waves = [fp.run_edges(DELTA, 1, dst.n_docs)[0] * fp.T("WAVES_DELTA") for dst, _ in c.batches]
    assert any(0 < n <= w for n, w in zip(n_def, waves)) and any(n > w for n, w in zip(n_def, waves))


def test_special_documents_sit_at_run_edges():
    for mode in (AWSET, DELTA):
        k = fp.T("K_DELTA") if mode == DELTA else fp.T("K_AWSET")
        n = max(fe.DOC_COUNTS[mode])
        got = []
        for v in (0, 1):
            dst, srcs = fe.doc_count_batch(mode, n, v)
            rec = fp.classify(mode, 1, dst, srcs)
            got.append([rec[p]["pass"] for p in (0, k - 1, k, n - 1)])
        assert got[0] == ["general-deferred", "block", "general-deferred", "block"], got
        assert got[1] == ["block", "general-deferred", "block", "general-deferred"], got


def test_slack_holds_what_would_matter():
    for mode in (AWSET, DELTA):
        case, compact = fe.slack_case(mode)
        dst, srcs = case.batches[0]
        slack = (dst.offsets[1:] - dst.offsets[:-1]) - dst.counts
        assert set(slack.tolist()) == set(range(6))
        R, hits = dst.R, Counter()
        for d in range(dst.n_docs):
            o, n = int(dst.offsets[d]), int(dst.counts[d])
            live = dst.keys[o:o + n].tolist()
            for s in range(o + n, int(dst.offsets[d + 1])):
                hits["dup"] += int(dst.keys[s]) in live
                hits["inside"] += bool(live) and min(live) <= int(dst.keys[s]) <= max(live)
                hits["actor==R"] += int(dst.actors[s]) == R
        assert all(hits[k] >= FLOOR for k in ("dup", "inside", "actor==R")), hits
        # the compact twin holds the same live documents
        for d in range(dst.n_docs):
            assert dst.doc(d) == compact.doc(d)
        rc1, w1 = oracle.fold(mode, dst, srcs)
        rc2, w2 = oracle.fold(mode, compact, srcs)
        assert rc1 == 0 and rc2 == 0 and fp.arrays_equal_live(w1, w2, dst.n_docs, R) is None


def test_no_tombstone_twin_is_the_same_fold():
    case, twin = fe.no_tomb_case()
    dst, bare = case.batches[0]
    assert bare.tomb_off is None and twin.tomb_off is not None and int(twin.tomb_off[-1]) == 0
    rc1, w1 = oracle.fold(DELTA, dst, bare)
    rc2, w2 = oracle.fold(DELTA, dst, twin)
    assert rc1 == 0 and rc2 == 0 and fp.arrays_equal_live(w1, w2, dst.n_docs, dst.R) is None


def test_thresholds_table_names_its_lines():
    for name, (value, lines, what) in fp.THRESHOLDS.items():
        assert isinstance(value, int) and lines and what, name
