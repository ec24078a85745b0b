"""GPU: the scalar arms of the alignment-selected kernels, on columns that start
one element past a 16 B (actors: 8 B) boundary.

compare, select, scatter, digest and the worklist digest pick between a vector
and a scalar arm from the alignment of the caller's column pointers
(launch_compare, launch_select, launch_scatter, launch_digest,
launch_digest_idx); whole allocations are always aligned, so only a shifted
view reaches the scalar arm.  Every shift set of tests/align_cases.py -- every
selector value of every call -- runs on the table's device-resident inputs:

  the results are bit-exact against the CPU reference and bit-identical to the
  same call on the unshifted columns; crdt_ctx_sync reports nothing;
  every output array is poisoned before the call: entry slots at or past the
  packed total, worklist words at or past n_work and digest words of unlisted
  documents keep their bits, and around a shifted output column the element
  before the view and the GUARD elements after it still hold the pattern;
  the inputs, and the guard elements around shifted input views, are
  bit-identical after the call.

All views lie inside their allocations; nothing here relies on a fault.
"""

import numpy as np
import pytest

import crdtgpu
from align_cases import (COLUMNS, COMPARE_LAYOUTS, DIGEST_NULL_TOMBS, LAYOUTS, N_DOCS, SHIFTS, R, compare_case,
                         digest_list, guards_intact, scatter_idx, select_idx, selector, shift_id, shifted, state_batch,
                         sub_batch, tomb_batch)
from crdtgpu import CRDT_DIGEST_GATHER as GATHER
from crdtgpu import CRDT_DIGEST_PLACE as PLACE
from crdtgpu.batch import _np
from digest_idx_cases import Case, place_sub
from test_compare_model import compare_ref, select_ref
from test_digest_idx_model import expected, sentinel
from test_digest_model import digest_ref
from test_gpu_compare import assert_cmp, assert_packed, dev_of, poisoned_cmp, poisoned_out, read_cmp
from test_gpu_digest import assert_digest, host_digest, poisoned_digest
from test_gpu_scatter import dev_words
from test_scatter_model import scatter_ref

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64
FIELDS = ("offsets", "counts", "keys", "actors", "counters", "vv")
ALIGNED = frozenset()


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


def ids(v):
    return shift_id(v) if isinstance(v, frozenset) else None


# ------------------------------------------------------------------- helpers

def on_device(torch, host, name, shift):
    """(the host batch uploaded, {column: Shifted}): the columns `name`.* of the shift set
    are views one element past their alignment inside pattern-filled allocations."""
    d = host.to(dev_of(torch))
    rec = {}
    for c in COLUMNS:
        if "%s.%s" % (name, c) in shift:
            rec[c] = shifted(torch, getattr(d, c))
            setattr(d, c, rec[c].view)
    return d, rec


def assert_unchanged(dev, host, rec, what):
    """An input after the call: every array bit-identical to what was uploaded, the guard
    elements around its shifted columns still the pattern."""
    for f in FIELDS:
        h = getattr(host, f, None)
        if h is not None:
            assert (_np(getattr(dev, f), h.dtype)[:len(h)] == h).all(), "%s.%s changed" % (what, f)
    for c, s in rec.items():
        assert guards_intact(s), "%s.%s: a guard element was written" % (what, c)


def out_buffers(torch, n_docs, slots, shift):
    """Poisoned output buffers; the columns out.* of the shift set shifted, poison and all."""
    out = poisoned_out(torch, n_docs, R, slots)
    rec = {}
    for c in COLUMNS:
        if "out.%s" % c in shift:
            rec[c] = shifted(torch, getattr(out, c))
            setattr(out, c, rec[c].view)
    return out, rec


def assert_same_out(h, base):
    for f in FIELDS:
        assert (getattr(h, f) == getattr(base, f)).all(), "%s differs from the unshifted call's" % f


_ref, _base = {}, {}


def once(store, key, make):
    if key not in store:
        store[key] = make()
    return store[key]


# ------------------------------------------------------------------- 1. compare

def run_compare(eng, torch, layout, shift):
    a, b, _, _ = compare_case(*layout)
    da, ra = on_device(torch, a, "a", shift)
    db, rb = on_device(torch, b, "b", shift)
    out = poisoned_cmp(torch, a.n_docs)
    eng.compare_async(da, db, out)
    eng.sync()  # (raises on any status bit)
    got = read_cmp(out)  # (the worklist's tail still poison)
    assert_unchanged(da, a, ra, "a")
    assert_unchanged(db, b, rb, "b")
    return got


@pytest.mark.parametrize("shift", SHIFTS["compare"], ids=ids)
@pytest.mark.parametrize("layout", COMPARE_LAYOUTS, ids=lambda v: "a%d_b%d" % v)
def test_compare(eng, torch, layout, shift):
    a, b, changes, flags = compare_case(*layout)
    want = once(_ref, ("compare", layout), lambda: compare_ref(a, b))
    assert (want[0] == flags).all() and len(want[2]) == len(changes) == int(want[1][4])
    assert selector("compare", shift) == (int(not shift),)
    got = run_compare(eng, torch, layout, shift)
    assert_cmp(got, want)  # flags, summary, worklist (its length is n_work)
    assert_cmp(got, once(_base, ("compare", layout), lambda: run_compare(eng, torch, layout, ALIGNED)))


# ------------------------------------------------------------------- 2. select

def run_select(eng, torch, slack, which, shift):
    st, idx = state_batch(slack), select_idx(which)
    want = once(_ref, ("select", slack, which),
                lambda: select_ref(st, idx, n_out=N_DOCS if idx is None else len(idx)))
    ds, rs = on_device(torch, st, "state", shift)
    out, ro = out_buffers(torch, want.n_docs, int(want.offsets[-1]) + 3, shift)
    eng.select_async(ds, out, idx=None if idx is None else dev_words(torch, idx))
    eng.sync()
    h = assert_packed(out, want)  # all six arrays and the slot bounds; slots past the total still poison
    for c, s in ro.items():
        assert guards_intact(s), "out.%s: written outside the column" % c
    assert_unchanged(ds, st, rs, "state")
    return h


@pytest.mark.parametrize("shift", SHIFTS["select"], ids=ids)
@pytest.mark.parametrize("which", ["identity", "permuted"])
@pytest.mark.parametrize("slack", LAYOUTS)
def test_select(eng, torch, slack, which, shift):
    h = run_select(eng, torch, slack, which, shift)
    assert_same_out(h, once(_base, ("select", slack, which), lambda: run_select(eng, torch, slack, which, ALIGNED)))


# ------------------------------------------------------------------- 3. scatter

def run_scatter(eng, torch, slack, shift):
    st, sub, idx = state_batch(slack), sub_batch(slack), scatter_idx()
    want = once(_ref, ("scatter", slack), lambda: scatter_ref(st, sub, idx))
    ds, rs = on_device(torch, st, "state", shift)
    db, rb = on_device(torch, sub, "sub", shift)
    out, ro = out_buffers(torch, N_DOCS, int(want.offsets[-1]) + 3, shift)
    eng.scatter_async(ds, db, dev_words(torch, idx), out)
    eng.sync()
    h = assert_packed(out, want)
    for c, s in ro.items():
        assert guards_intact(s), "out.%s: written outside the column" % c
    assert_unchanged(ds, st, rs, "state")
    assert_unchanged(db, sub, rb, "sub")
    return h


@pytest.mark.parametrize("shift", SHIFTS["scatter"], ids=ids)
@pytest.mark.parametrize("slack", LAYOUTS)
def test_scatter(eng, torch, slack, shift):
    h = run_scatter(eng, torch, slack, shift)
    assert_same_out(h, once(_base, ("scatter", slack), lambda: run_scatter(eng, torch, slack, ALIGNED)))


# ------------------------------------------------------------------- 4. digest

def run_digest(eng, torch, slack, shift, tombs):
    st, tb = state_batch(slack), tomb_batch(slack) if tombs else None
    ds, rs = on_device(torch, st, "state", shift)
    dt, rt = on_device(torch, tb, "tombs", shift) if tombs else (None, {})
    out = poisoned_digest(torch, N_DOCS)
    eng.digest_async(ds, out, dt)
    eng.sync()
    assert_unchanged(ds, st, rs, "state")
    if tombs:
        assert_unchanged(dt, tb, rt, "tombs")
    return host_digest(out, N_DOCS)


@pytest.mark.parametrize("shift,tombs", [(s, True) for s in SHIFTS["digest"]] + [(DIGEST_NULL_TOMBS, False)],
                         ids=lambda v: shift_id(v) if isinstance(v, frozenset) else ("tombs_null", "tombs")[v])
@pytest.mark.parametrize("slack", LAYOUTS)
def test_digest(eng, torch, slack, shift, tombs):
    want = once(_ref, ("digest", slack, tombs),
                lambda: digest_ref(state_batch(slack), tomb_batch(slack) if tombs else None))
    got = run_digest(eng, torch, slack, shift, tombs)
    assert_digest(got, want)
    assert_digest(got, once(_base, ("digest", slack, tombs), lambda: run_digest(eng, torch, slack, ALIGNED, tombs)))


# ------------------------------------------------------------------- 5. worklist digest

def idx_case(slack):
    idx = digest_list()
    return Case("align_slack%d" % slack, state_batch(slack), tomb_batch(slack), idx, len(idx), len(idx), False, False)


def run_digest_idx(eng, torch, slack, mode, shift):
    c = idx_case(slack)
    st, tb = (c.state, c.tombs) if mode == GATHER else place_sub(c)
    ds, rs = on_device(torch, st, "state", shift)
    dt, rt = on_device(torch, tb, "tombs", shift)
    dig = torch.from_numpy(sentinel(N_DOCS).reshape(-1).view(np.int64).copy()).to(dev_of(torch))
    rd = shifted(torch, dig) if "digest" in shift else None  # 8 B off 16 B: the two-store form
    if rd is not None:
        dig = rd.view
    eng.digest_idx_async(ds, dev_words(torch, c.idx), dig, tombs=dt, n_idx=dev_words(torch, [c.n_idx]),
                         n_max=c.n_max, mode=mode)
    eng.sync()
    assert rd is None or guards_intact(rd), "digest: written outside the array"
    assert_unchanged(ds, st, rs, "state")
    assert_unchanged(dt, tb, rt, "tombs")
    return _np(dig, U64).reshape(N_DOCS, 2)


@pytest.mark.parametrize("shift", SHIFTS["digest_idx"], ids=ids)
@pytest.mark.parametrize("mode", [GATHER, PLACE], ids=["gather", "place"])
@pytest.mark.parametrize("slack", LAYOUTS)
def test_digest_idx(eng, torch, slack, mode, shift):
    c = idx_case(slack)
    want = expected(c)  # the listed documents' words, the sentinel everywhere else
    rows = np.unique(c.idx.astype(np.int64))
    ref = once(_ref, ("digest", slack, True), lambda: digest_ref(c.state, c.tombs))
    assert (want[rows] == ref[rows]).all() and len(rows) < N_DOCS
    got = run_digest_idx(eng, torch, slack, mode, shift)
    assert_digest(got, want)
    assert_digest(got, once(_base, ("digest_idx", slack, mode),
                            lambda: run_digest_idx(eng, torch, slack, mode, ALIGNED)))
