"""GPU: the ingest sort (crdt_awset_sort_async / _batch, csrc/sort.hip, csrc/wave_sort.hpp) and
the device order check (check_order_kernel, csrc/pack.hip) on every case of
tests/sort_edge_cases.py (pinned by tests/test_sort_edges_model.py).

The reference of the sort is Python's `sorted` on int tuples, per document.  The clean cases of
one R run as one batch, through the host path and on device buffers; a failure names the case.
The outputs of the device runs are prefilled with a pattern no case holds, so a store outside a
document's live span shows.  The repeated-key and over-count cases are error-code cases on
inputs that stay inside their arrays (tests/test_sort_edges_model.py); no test provokes a fault.
The order cases go through the calls that run the check: the host-path join (two range lists)
and fold (three), their verdicts held to the host validators'.
"""

import numpy as np
import pytest

import crdtgpu
from crdtgpu import CRDT_E_UNSORTED, CRDT_FOLD_AWSET, CRDT_FOLD_DELTA
from crdtgpu.batch import AWSetBatch, OutBuffers
from helpers import out_doc
from oracle import oracle
from sort_edge_cases import (BY_NAME, DUP_CASES, FILLS, ORDER_BY_NAME, ORDER_CASES, OVER_CASES, affine, batch_of, clean_of,
                             concat, order_batch, order_other, order_srcs, pack, permuted, reference)
from test_gpu_compare import _code, dev_of
from test_gpu_parity import assert_same, assert_same_all, host_out

pytestmark = pytest.mark.gpu

S32, S64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A  # no key, actor, counter or clock word of the table
RS = (1, 3, 64)


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


@pytest.fixture(scope="module")
def n_cu(torch):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ------------------------------------------------------------------- helpers

_tables = {}


def table(R, extra=0, fill="zeros"):
    """The clean cases of one R as one batch, the first document of each, and each document's
    reference; built once, never modified."""
    key = (R, extra, fill)
    if key not in _tables:
        cases = clean_of(R)
        b, first = concat(cases, extra, fill)
        _tables[key] = (b, first, cases, ref_of(R))
    return _tables[key]


def ref_of(R):
    key = ("ref", R)
    if key not in _tables:
        _tables[key] = [reference(c) for c in clean_of(R)]
    return _tables[key]


def poisoned(torch, n, R, slots):
    o = OutBuffers(n, R, slots, device=dev_of(torch))
    o.offsets.fill_(S32)
    o.counts.fill_(S32)
    o.actors.fill_(S32)
    for t in (o.keys, o.counters, o.vv):
        t.fill_(S64)
    return o


def sort_device(eng, torch, b, sync=True):
    """crdt_awset_sort_async of host batch b on device buffers, into poisoned outputs; the host copy."""
    slots = int(b.offsets[-1])
    out = poisoned(torch, b.n_docs, b.R, slots)
    eng.sort_async(b.to(dev_of(torch)), slots, out)
    if sync:
        eng.sync()
    return out


def check_docs(got, b, f, want, what):
    """Documents f .. of the output against `want` [(entries, clock)]: bounds, count, entries, clock."""
    R = b.R
    for d, (ents, vv) in enumerate(want):
        assert int(got.offsets[f + d]) == int(b.offsets[f + d]), "%s: offsets[%d]" % (what, f + d)
        assert int(got.counts[f + d]) == len(ents), "%s: counts[%d] = %d, reference %d" % (what, f + d, int(got.counts[f + d]), len(ents))
        e, v = out_doc(got, f + d, R)
        if e != ents:
            i = next(i for i in range(len(ents)) if e[i] != ents[i])
            raise AssertionError("%s: document %d differs first at %d: %r, reference %r" % (what, d, i, e[i], ents[i]))
        assert v == vv, "%s: clock of document %d" % (what, d)


def check_table(got, b, first, cases, refs, what):
    failed = []
    for c, f, want in zip(cases, first, refs):
        try:
            check_docs(got, b, f, want, "%s %s" % (what, c.name))
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "%d cases failed:\n%s" % (len(failed), "\n".join(failed[:40]))
    assert int(got.offsets[b.n_docs]) == int(b.offsets[b.n_docs]), "%s: offsets[n_docs]" % what


def check_dead_slots(got, b, what):
    """Every output slot outside a document's live span still holds the pattern, in all three columns."""
    slots = int(b.offsets[-1])
    cnt = np.asarray(got.counts[: b.n_docs]).astype(np.int64)
    start = np.asarray(b.offsets[: b.n_docs]).astype(np.int64)
    idx = np.repeat(start, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    dead = np.ones(slots, dtype=bool)
    dead[idx] = False
    assert dead.sum() == slots - cnt.sum()
    for f, s in (("keys", S64), ("actors", S32), ("counters", S64)):
        col = np.asarray(getattr(got, f))[:slots]
        bad = np.flatnonzero(dead & (col != s))
        if bad.size:
            d = int(np.searchsorted(np.asarray(b.offsets).astype(np.int64), bad[0], side="right")) - 1
            raise AssertionError("%s: %s[%d] = %#x was written outside the live span of document %d" % (what, f, bad[0], int(col[bad[0]]), d))


# ------------------------------------------------------------- 1. the clean table

@pytest.mark.parametrize("R", RS)
def test_clean_table_host_path(eng, R):
    b, first, cases, refs = table(R)
    check_table(eng.sort(b), b, first, cases, refs, "sort_batch")


@pytest.mark.parametrize("R", RS)
def test_clean_table_device_buffers(eng, torch, R):
    b, first, cases, refs = table(R)
    got = host_out(sort_device(eng, torch, b), torch)
    check_table(got, b, first, cases, refs, "sort_async")
    check_dead_slots(got, b, "sort_async")


@pytest.mark.parametrize("case", clean_of(3)[:: max(1, len(clean_of(3)) // 24)], ids=lambda c: c.name)
def test_case_alone(eng, torch, case):
    """A spread of the cases as their own batch: the first document is also the last, the one
    that writes offsets[n_docs]."""
    b = batch_of(case)
    check_docs(host_out(sort_device(eng, torch, b), torch), b, 0, reference(case), case.name)
    check_docs(eng.sort(b), b, 0, reference(case), case.name)


# ------------------------------------------------------------- 2. the slack is neither read nor written

@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("R", RS)
def test_slack_untouched(eng, torch, R, fill):
    """Two more slots a document, holding zeros, all-ones, or entries that continue the document:
    the live spans are the reference's and every other output slot still holds the pattern."""
    b, first, cases, refs = table(R, 2, fill)
    got = host_out(sort_device(eng, torch, b), torch)
    check_table(got, b, first, cases, refs, "slack %s" % fill)
    check_dead_slots(got, b, "slack %s" % fill)


# ------------------------------------------------------------- 3. repeated keys, counts above the slots

@pytest.mark.parametrize("case", DUP_CASES, ids=lambda c: c.name)
def test_repeated_key_is_reported(eng, torch, case):
    """CRDT_E_DUP_KEY on device buffers and through the host path, a second sync clean; the copies
    of the repeated key come out side by side in input order (every compare of the sort is on
    (key, input index) and the merge takes the earlier run first: the sort is stable), everything
    else as the reference; then the same engine sorts the clean twin exactly."""
    b = batch_of(case)
    out = sort_device(eng, torch, b, sync=False)
    assert _code(eng.sync) == case.want
    eng.sync()
    got = host_out(out, torch)
    check_docs(got, b, 0, reference(case), case.name)
    check_dead_slots(got, b, case.name)
    assert _code(lambda: eng.sort(b)) == case.want
    twin = BY_NAME[case.twin]
    tb = batch_of(twin)
    check_docs(eng.sort(tb), tb, 0, reference(twin), twin.name)


@pytest.mark.parametrize("case", OVER_CASES, ids=lambda c: c.name)
def test_count_above_slots_is_clamped(eng, torch, case):
    """CRDT_E_CAPACITY; the bad document is the sort of its slots, its count clamped; the document
    after it (whose slots an unclamped kernel would read and write) and all others are the
    reference's; nothing outside the live spans is written; then the same batch with the count
    clamped sorts clean."""
    b = batch_of(case)
    out = sort_device(eng, torch, b, sync=False)
    assert _code(eng.sync) == case.want
    eng.sync()
    got = host_out(out, torch)
    check_docs(got, b, 0, reference(case), case.name)
    check_dead_slots(got, b, case.name)
    assert _code(lambda: eng.sort(b)) == case.want
    cb = pack(case.docs, case.R, case.slack)
    check_docs(eng.sort(cb), cb, 0, reference(case), case.name + " clamped")


# ------------------------------------------------------------- 4. launch shape

def closed_form_batch(sizes, R=2):
    """Documents of the given sizes, keys 3 i + d under an affine permutation, dots a function of the key."""
    docs = []
    for d, m in enumerate(sizes):
        keys = permuted([3 * i + d for i in range(m)], affine(m, c=d % max(m, 1)))
        docs.append(([(k, k % R, 2 * k + 1) for k in keys], [d & 0xFFFF, d >> 16]))
    return docs


def check_all(got, docs, R=2):
    for d, (ents, vv) in enumerate(docs):
        assert out_doc(got, d, R) == (sorted(ents), vv), "document %d of %d entries" % (d, len(ents))


def test_wave_kernel_strides_over_documents(eng, torch, n_cu):
    """64 n_cu + 5 documents: more than the wave kernel's 16 n_cu blocks of 4 take in one
    iteration; the last document goes to the block path from the second iteration."""
    docs = closed_form_batch([d % 4 for d in range(64 * n_cu + 4)] + [257])
    b = AWSetBatch.from_docs(2, docs)
    assert b.n_docs > 64 * n_cu and int(b.offsets[-1]) < 1000000
    got = host_out(sort_device(eng, torch, b), torch)
    check_all(got, docs)
    assert (np.asarray(got.offsets) == b.offsets).all()


def test_block_kernel_takes_more_documents_than_workgroups(eng, torch, n_cu):
    """4 n_cu + 3 documents of 257 entries: more queued documents than sort_block_kernel has workgroups."""
    docs = closed_form_batch([257] * (4 * n_cu + 3))
    b = AWSetBatch.from_docs(2, docs)
    assert int(b.offsets[-1]) < 1000000
    got = host_out(sort_device(eng, torch, b), torch)
    check_all(got, docs)
    assert (np.asarray(got.offsets) == b.offsets).all()


# ------------------------------------------------------------- 5. the order check

def verdict(c):
    rc = crdtgpu.validate(order_batch(c))
    if rc == 0 and c.srcs is not None:
        rc = crdtgpu.validate_src(order_srcs(c))
    return rc


def joined_exact(eng, dst, src, what):
    rc, want = oracle.join(dst, src)
    assert rc == 0
    try:
        assert_same(eng.join(dst, src), want, dst.n_docs, dst.R)
    except crdtgpu.CrdtError as e:
        raise AssertionError("%s: a clean call returned %d" % (what, e.code))


@pytest.mark.parametrize("case", [c for c in ORDER_CASES if c.srcs is None], ids=lambda c: c.name)
def test_order_check_in_join(eng, case):
    """The case as dst and then as src of the host-path join (the check's first and second range
    list): the return code is the host validator's verdict; a clean case is the oracle's join
    bit-exactly; after CRDT_E_UNSORTED the same engine joins clean input exactly."""
    a, o = order_batch(case), order_other(case)
    want = verdict(case)
    assert want == case.want
    for dst, src, side in ((a, o, "dst"), (o, a, "src")):
        if want == 0:
            joined_exact(eng, dst, src, "%s as %s" % (case.name, side))
        else:
            try:
                eng.join(dst, src)
                code = 0
            except crdtgpu.CrdtError as e:
                code = e.code
            assert code == want == CRDT_E_UNSORTED, "%s as %s: returned %d" % (case.name, side, code)
            joined_exact(eng, o, o, "%s as %s, the clean call after it" % (case.name, side))


@pytest.mark.parametrize("mode", [CRDT_FOLD_AWSET, CRDT_FOLD_DELTA], ids=["awset", "delta"])
@pytest.mark.parametrize("case", [c for c in ORDER_CASES if c.srcs is not None], ids=lambda c: c.name)
def test_order_check_in_fold(eng, case, mode):
    """Three range lists: the documents, the sources' entries, the sources' tombstones."""
    dst, srcs = order_batch(case), order_srcs(case)
    want = verdict(case)
    assert want == case.want
    clean = ORDER_BY_NAME["order_fold_clean"]
    if want != 0:
        assert _code(lambda: eng.fold(mode, dst, srcs)) == want == CRDT_E_UNSORTED
        dst, srcs = order_batch(clean), order_srcs(clean)
    rc, ref = oracle.fold(mode, dst, srcs)
    assert rc == 0
    assert_same(eng.fold(mode, dst, srcs), ref, dst.n_docs, dst.R)


def test_order_check_strides_over_ranges(eng, n_cu):
    """More than 64 n_cu ranges in the two lists together: the kernel's 16 n_cu blocks of 4 take
    a second iteration; the only violation is in the last range of the second list."""
    n = 32 * n_cu + 3
    R = 2
    off = (2 * np.arange(n + 1)).astype(np.uint32)
    vv = np.ones(n * R, np.uint64)

    def batch(k0):
        keys = (np.repeat(np.arange(n), 2) * 4 + np.tile([k0, k0 + 2], n)).astype(np.uint64)
        return AWSetBatch(R, off, keys, (keys % R).astype(np.uint32), keys + np.uint64(1), vv)

    a, b = batch(0), batch(1)
    assert 2 * n > 64 * n_cu
    rc, want = oracle.join(a, b)
    assert rc == 0
    assert_same_all(eng.join(a, b), want, n, R)
    bad = batch(1)
    bad.keys[-1], bad.keys[-2] = bad.keys[-2], bad.keys[-1]
    assert crdtgpu.validate(bad) == CRDT_E_UNSORTED and crdtgpu.validate(a) == 0
    assert _code(lambda: eng.join(a, bad)) == CRDT_E_UNSORTED
    assert_same_all(eng.join(a, b), want, n, R)


# ------------------------------------------------------------- 6. sort -> validate -> join

@pytest.mark.parametrize("R", RS)
def test_sorted_table_validates_and_joins_with_itself(eng, R):
    """Every clean case sorted on the device is what the merge kernels ask for: the host
    validator passes it, and its join with itself is itself."""
    b, first, cases, refs = table(R)
    got = eng.sort(b)
    s = AWSetBatch(R, got.offsets, got.keys, got.actors, got.counters, got.vv, got.counts)
    assert crdtgpu.validate(s) == 0
    j = eng.join(s, s)
    for c, f in zip(cases, first):
        for d in range(len(c.docs)):
            assert out_doc(j, f + d, R) == out_doc(got, f + d, R), c.name
