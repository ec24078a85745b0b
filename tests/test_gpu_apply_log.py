"""GPU: crdt_awset_apply_log_async (csrc/apply_wave.hpp with LOG = true, csrc/apply_log.hip)
against the C oracle's apply followed by diff_doc of tests/test_diff_model.py per document
(ref_log of tests/test_apply_log_model.py); a refused document's log is empty.

Every written array is over-allocated and pre-filled with a pattern no case holds; the
whole arrays are then compared with an image built from the expected documents and lists:
offsets, counts, flags and clocks, the live prefix of every document and list, and the
pattern in every other word.  The state part is also compared word for word with what
crdt_awset_apply_async writes into equally poisoned buffers.  No test provokes a fault: the
error cases are the reported ones of the contract (include/crdtgpu.h).
"""

import ctypes

import numpy as np
import pytest

import counter_maps as cm
import crdtgpu
from apply_cases import doc_of, tomb_batch
from apply_edge_cases import ADD, CASES, DDEL, DDK, DEL, Case, Doc, batches, doc, ents_of, mixed_doc, op_batch
from apply_log_cases import ADDED, LOG_BY_NAME, LOG_CASES, UPDATED
from crdtgpu import CRDT_E_ACTOR_RANGE, CRDT_E_CAPACITY, CRDT_E_INVALID, abi
from crdtgpu.batch import (AWSetBatch, DiffBuffers, MergeLogBuffers, OpBatch, OutBuffers, QueryBatch, QueryBuffers, Replica,
                           TombBuffers)
from oracle import oracle
from test_apply_log_model import ref_log, summary_of
from test_gpu_apply_edges import REFUSALS, long_doc, stride_batch
from test_gpu_compare import _code, dev_of
from test_gpu_replica import apply_round_case, poisoned as poisoned_replica, words

pytestmark = pytest.mark.gpu

U8, U32, U64 = np.uint8, np.uint32, np.uint64
P8, P32, P64 = 0x5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A  # no case holds these as a key, a dot, a count, a flag or a clock
PAD = 40  # words every written array is over-allocated by
OUT_F = ("offsets", "counts", "keys", "actors", "counters", "vv")
TOMB_F = ("offsets", "counts", "keys", "actors", "counters")
LOG_F = MergeLogBuffers.FIELDS
ALL_CASES = list(CASES) + list(LOG_CASES)



def _has_ddk(x):
    return any(k == DDK for k, _ in x.ops)


# the cases whose first document has no DELTA_DEL_KEY, without their documents that have one (tomb_out == NULL)
NO_DDK = [c._replace(docs=[x for x in c.docs if not _has_ddk(x)]) for c in ALL_CASES if not _has_ddk(c.docs[0])]


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


# ------------------------------------------------------------------- helpers

def slots_of(x):
    return int(np.asarray(x.offsets)[-1]) if x is not None else 0


def poison(torch, buf, fields):
    for f in fields:
        t = getattr(buf, f)
        if t is not None:
            t.fill_(P8 if t.dtype == torch.uint8 else P32 if t.dtype == torch.int32 else P64)
    return buf


def buffers(torch, st, tb, op, tombs_out=True, pad=PAD, **kw):
    """Poisoned (OutBuffers, TombBuffers or None, MergeLogBuffers), each array `pad` words
    longer than the call needs (the per-document arrays too)."""
    dev, n, nops = dev_of(torch), st.n_docs + pad, slots_of_ops(op)
    out = poison(torch, OutBuffers(n, st.R, slots_of(st) + nops + pad, device=dev), OUT_F)
    tout = poison(torch, TombBuffers(n, slots_of(tb) + nops + pad, device=dev), TOMB_F) if tombs_out else None
    log = poison(torch, MergeLogBuffers(n, slots_of(st) + pad, nops + pad, device=dev, **kw), LOG_F)
    return out, tout, log


def slots_of_ops(op):
    return int(np.asarray(op.op_off)[-1])


def download(buf, fields):
    got = {}
    for f in fields:
        t = getattr(buf, f)
        if t is None:
            got[f] = None
            continue
        a = t.cpu().numpy()
        got[f] = a.view(U32 if a.dtype == np.int32 else U64 if a.dtype == np.int64 else U8)
    return got


def reference(st, tb, op, refused=(), with_tombs=True):
    """(per document (entries, tombstones, clock), per document (removed, upserted, flags)); the
    op lists of `refused` documents must be empty in `op`."""
    logs, _ = ref_log(st, tb, op, refused, with_tombs)
    rc, wo, wt = oracle.apply(st, op, tb, with_tombs=with_tombs)
    assert rc == 0
    return [doc_of(wo, wt, d, st.R) for d in range(st.n_docs)], logs


def put(img, lo, rows, cols):
    for j, f in enumerate(cols):
        if rows:
            img[f][lo:lo + len(rows)] = np.array([r[j] for r in rows], img[f].dtype)


class Image:
    """The arrays a call must leave behind.  parts: (image, care) of the entries, of the
    tombstones (or None) and of the log; care is False over a refused document's slots and
    clock, which are undefined."""

    def __init__(self, st, tb, op, docs, logs, refused=(), tombs_out=True, pad=PAD, kind=True, summary=True):
        n, R, nops = st.n_docs, st.R, slots_of_ops(op)
        op_off = np.asarray(op.op_off).astype(np.int64)
        s_off = np.asarray(st.offsets).astype(np.int64)
        t_off = np.asarray(tb.offsets).astype(np.int64) if tb is not None else np.zeros(n + 1, np.int64)
        self.parts = []
        for off, slots, which, with_vv in ((s_off + op_off, slots_of(st) + nops, 0, True),
                                           (t_off + op_off, slots_of(tb) + nops, 1, False)):
            if which == 1 and not tombs_out:
                self.parts.append(None)
                continue
            img = dict(offsets=np.full(n + pad + 1, P32, U32), counts=np.full(n + pad, P32, U32),
                       keys=np.full(slots + pad, P64, U64), actors=np.full(slots + pad, P32, U32),
                       counters=np.full(slots + pad, P64, U64))
            if with_vv:
                img["vv"] = np.full((n + pad) * R, P64, U64)
            care = {f: np.ones(len(a), bool) for f, a in img.items()}
            img["offsets"][:n + 1] = off
            for d in range(n):
                lo, hi = int(off[d]), int(off[d + 1])
                if d in refused:
                    img["counts"][d] = 0
                    for f in ("keys", "actors", "counters"):
                        care[f][lo:hi] = False
                    if with_vv:
                        care["vv"][d * R:(d + 1) * R] = False
                    continue
                rows = docs[d][which]
                assert lo + len(rows) <= hi
                img["counts"][d] = len(rows)
                put(img, lo, rows, ("keys", "actors", "counters"))
                if with_vv:
                    img["vv"][d * R:(d + 1) * R] = np.array(docs[d][2], U64)
            self.parts.append((img, care))
        ss = slots_of(st)
        lg = dict(flags=np.full(n + pad, P8, U8), summary=np.array(summary_of(logs), U32) if summary else None,
                  rem_offsets=np.full(n + pad + 1, P32, U32), rem_counts=np.full(n + pad, P32, U32),
                  rem_keys=np.full(ss + pad, P64, U64), rem_actors=np.full(ss + pad, P32, U32),
                  rem_counters=np.full(ss + pad, P64, U64), ups_offsets=np.full(n + pad + 1, P32, U32),
                  ups_counts=np.full(n + pad, P32, U32), ups_keys=np.full(nops + pad, P64, U64),
                  ups_actors=np.full(nops + pad, P32, U32), ups_counters=np.full(nops + pad, P64, U64),
                  ups_kind=np.full(nops + pad, P8, U8) if kind else None)
        lg["rem_offsets"][:n + 1], lg["ups_offsets"][:n + 1] = s_off, op_off
        for d, (rem, ups, f) in enumerate(logs):
            assert (d not in refused or (rem, ups, f) == ([], [], 0)) and len(ups) <= int(op_off[d + 1] - op_off[d])
            lg["flags"][d], lg["rem_counts"][d], lg["ups_counts"][d] = f, len(rem), len(ups)
            put(lg, int(s_off[d]), rem, ("rem_keys", "rem_actors", "rem_counters"))
            put(lg, int(op_off[d]), ups, ("ups_keys", "ups_actors", "ups_counters") + (("ups_kind",) if kind else ()))
        self.parts.append((lg, None))

    def check(self, out, tout, log, what="", plain=None):
        """The logged call's arrays against the image; plain: (out, tout) of crdt_awset_apply_async
        into equally poisoned buffers, compared word for word where the result is defined."""
        for part, buf, fields, name in zip(self.parts, (out, tout, log), (OUT_F, TOMB_F, LOG_F),
                                           ("entries", "tombstones", "log")):
            if part is None:
                assert buf is None
                continue
            img, care = part
            got = download(buf, fields)
            for f, a in img.items():
                if a is None:
                    assert got[f] is None
                    continue
                if f == "summary":
                    got[f] = got[f][:5]
                assert len(got[f]) == len(a), (name, f)
                ok = care[f] if care is not None else np.ones(len(a), bool)
                bad = np.flatnonzero((got[f] != a) & ok)
                assert bad.size == 0, "%s %s.%s[%d] = %#x, want %#x" % (what, name, f, bad[0], int(got[f][bad[0]]),
                                                                         int(a[bad[0]]))
            if plain is not None and name != "log":
                pg = download(plain[0] if name == "entries" else plain[1], fields)
                for f in fields:
                    bad = np.flatnonzero((got[f] != pg[f]) & care[f])
                    assert bad.size == 0, "%s %s.%s[%d] differs from the plain apply" % (what, name, f, bad[0])


def run_log(eng, torch, st, tb, op, tombs_out=True, pad=PAD, stream=None, dev=None, **kw):
    """One logged call into poisoned buffers (not synced): (out, tout, log)."""
    out, tout, log = buffers(torch, st, tb, op, tombs_out, pad, **kw)
    dst, dtb, dop = dev or (st.to(dev_of(torch)), tb.to(dev_of(torch)) if tb is not None else None, op.to(dev_of(torch)))
    eng.apply_log_async(dst, dop, out, log, dtb, tout, stream=stream)
    return out, tout, log


def run_plain(eng, torch, st, tb, op, tombs_out=True, pad=PAD):
    out, tout, _ = buffers(torch, st, tb, op, tombs_out, pad)
    dev = dev_of(torch)
    eng.apply_async(st.to(dev), op.to(dev), out, tb.to(dev) if tb is not None else None, tout)
    return out, tout


def check_call(eng, torch, st, tb, op, tombs_out=True, what="", want=None):
    docs, logs = reference(st, tb, op, with_tombs=tombs_out)
    if want is not None:
        assert logs[0] == (list(want[0]), list(want[1]), want[2]), what
    got = run_log(eng, torch, st, tb, op, tombs_out)
    plain = run_plain(eng, torch, st, tb, op, tombs_out)
    eng.sync()
    Image(st, tb, op, docs, logs, tombs_out=tombs_out).check(*got, what=what, plain=plain)
    return logs


# ------------------------------------------------------------- 1. the case tables

@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_case_into_poisoned_buffers(eng, torch, case):
    st, tb, op = batches(case)
    check_call(eng, torch, st, tb, op, what=case.name, want=case.want if case in LOG_CASES else None)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_case_with_null_tombs(eng, torch, case):
    """tombs == NULL: no Deleted yet; the entries and their log do not depend on it."""
    st, _, op = batches(case)
    check_call(eng, torch, st, None, op, what=case.name, want=case.want if case in LOG_CASES else None)


@pytest.mark.parametrize("case", NO_DDK, ids=lambda c: c.name)
def test_case_with_null_tomb_out(eng, torch, case):
    st, tb, op = batches(case)
    check_call(eng, torch, st, tb, op, tombs_out=False, what=case.name, want=getattr(case, "want", None)
               if case.name in LOG_BY_NAME else None)


def test_null_tomb_out_form_has_cases():
    assert len(NO_DDK) >= 25 and sum(c.name in LOG_BY_NAME for c in NO_DDK) >= 15


def concat_docs(R=3):
    """Every document of both tables (R = 3), or those an R allows: for R = 1 the documents of
    actor 0, their entries' and tombstones' actors set to 0 and the clock cut to one word; for
    R = 64 all of them, the clock padded with zeros."""
    docs = [x for c in ALL_CASES for x in c.docs]
    if R == 1:
        docs = [Doc(0, [(k, 0, c) for k, _, c in x.ents], [(k, 0, c) for k, _, c in x.tombs], x.vv[:1], x.ops)
                for x in docs if x.actor == 0]
    elif R != 3:
        docs = [x._replace(vv=list(x.vv) + [0] * (R - 3)) for x in docs]
    st = AWSetBatch.from_docs(R, [(x.ents, x.vv) for x in docs])
    return docs, st, tomb_batch([x.tombs for x in docs]), op_batch(docs)


@pytest.mark.parametrize("R", [3, 1, 64])
def test_both_tables_in_one_batch(eng, torch, R):
    docs, st, tb, op = concat_docs(R)
    assert st.n_docs > (50 if R == 1 else 200)
    logs = check_call(eng, torch, st, tb, op, what="R=%d" % R)
    s = summary_of(logs)
    assert min(s) > 20 and any(f == 8 for _, _, f in logs) and any(f == 0 for _, _, f in logs)


def test_log_equals_the_device_diff_of_state_and_out(eng, torch):
    """flags, counts and summary equal crdt_awset_diff_async(state, out)'s, and its packed lists
    equal the log's lists read document by document."""
    _, st, tb, op = concat_docs()
    n, dev = st.n_docs, dev_of(torch)
    dst = st.to(dev)
    out, tout, log = run_log(eng, torch, st, tb, op, pad=0, dev=(dst, tb.to(dev), op.to(dev)))
    diff = DiffBuffers(n, slots_of(st), slots_of_ops(op), device=dev)
    eng.diff_async(dst, out.as_batch(), diff)
    eng.sync()
    g, df = log.numpy(), diff.numpy()
    assert (g["flags"] == df["flags"]).all() and (g["summary"] == df["summary"]).all()
    assert (g["rem_counts"] == np.diff(df["rem_off"])).all() and (g["ups_counts"] == np.diff(df["ups_off"])).all()
    for side in ("rem", "ups"):
        idx = np.concatenate([np.arange(int(c), dtype=np.int64) + int(o) for o, c in
                              zip(g[side + "_offsets"][:n], g[side + "_counts"])])
        assert len(idx) > 500
        for col in ("keys", "actors", "counters") + (("kind",) if side == "ups" else ()):
            assert (g["%s_%s" % (side, col)][idx] == df["%s_%s" % (side, col)]).all(), (side, col)


# ------------------------------------- 2. a refused document among good ones

@pytest.mark.parametrize("kind", list(REFUSALS))
def test_refused_document_among_good_ones(eng, torch, kind):
    bad, code, tombs_out = REFUSALS[kind]
    for pos in (0, 2, 4):
        docs = [long_doc(i, ddk=tombs_out) for i in range(5)]
        docs[pos] = bad
        st, tb, op = AWSetBatch.from_docs(3, [(x.ents, x.vv) for x in docs]), tomb_batch([x.tombs for x in docs]), \
            op_batch(docs)
        emptied = op_batch([x._replace(ops=[]) if d == pos else x for d, x in enumerate(docs)])
        want, logs = reference(st, tb, emptied, refused={pos}, with_tombs=tombs_out)
        assert all(len(r) + len(u) > 10 for d, (r, u, _) in enumerate(logs) if d != pos)
        got = run_log(eng, torch, st, tb, op, tombs_out)
        assert _code(eng.sync) == code, (kind, pos)
        eng.sync()  # cleared
        # offsets, counts and flags of every document; the refused one's log empty, out of the summary
        Image(st, tb, op, want, logs, refused={pos}, tombs_out=tombs_out).check(*got, what="%s at %d" % (kind, pos))


# ------------------------------------------------ 3. grid stride and stale LDS

def test_grid_stride_and_stale_lds(eng, torch):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * (2 * 16 * cus) + 3  # the grid is 16 workgroups of 2 waves per CU: every wave takes 2 documents, some 3
    st, tb, op, emptied, refused = stride_batch(n)
    assert len(refused) > n // 8
    want, logs = reference(st, tb, emptied, refused=refused)
    got = run_log(eng, torch, st, tb, op)
    assert _code(eng.sync) == CRDT_E_ACTOR_RANGE  # reported before CRDT_E_INVALID (crdt_ctx_sync)
    eng.sync()
    assert min(summary_of(logs)) > n // 16  # (the image's summary is the host sum over the documents not refused)
    Image(st, tb, op, want, logs, refused=refused).check(*got, what="stride")


# ------------------------------------------------------ 4. count above slots

@pytest.mark.parametrize("which", ["state", "tombs"])
def test_count_above_slots_is_clamped(eng, torch, which):
    docs = [mixed_doc(12 + 5 * i, actor=i % 3, shift=i) for i in range(5)]
    docs[2] = docs[2]._replace(ops=docs[2].ops + [(DEL, 10 ** 6), (ADD, 10 ** 6 + 1)])
    st = AWSetBatch.from_docs(3, [(x.ents, x.vv) for x in docs], slack=1)
    tb, op = tomb_batch([x.tombs for x in docs], 1), op_batch(docs)
    x = st if which == "state" else tb
    # the middle document's one slack slot holds a well-formed row above its live keys, which a DEL
    # names: the log is that of the clamped prefix, this row removed with its dot
    last = int(x.offsets[3]) - 1
    x.keys[last], x.actors[last], x.counters[last] = 10 ** 6, 1, 7
    x.counts[2] = int(x.offsets[3]) - int(x.offsets[2])  # the reference on the count the clamp gives
    want, logs = reference(st, tb, op)
    assert ((10 ** 6, 1, 7) in logs[2][0]) == (which == "state")
    x.counts[2] += 9
    got = run_log(eng, torch, st, tb, op)
    assert _code(eng.sync) == CRDT_E_CAPACITY
    eng.sync()  # cleared
    Image(st, tb, op, want, logs).check(*got, what=which)


# ------------------------------------------------------------ 5. wide counters

def test_wide_clocks_and_dots(eng, torch):
    """Log cases with state and tombstone counters through the order-preserving maps of
    tests/counter_maps.py and the acting clock started just below 2^31, 2^32, 2^63 and so that
    it lands on 2^64 - 1; the same-dot case is rebuilt on the moved clock."""
    names = ("add_of_live_key", "add_mints_same_dot_first_bump", "add_then_del_of_live_key", "slack_3",
             "updated_counter_only", "ddk_effective_and_ineffective", "keys_0_2_63_top_in_state")
    starts = [(1 << 31) - 2, (1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 63) - 2, None]
    docs = [LOG_BY_NAME[nm].docs[0] for nm in names for _ in starts]
    tod = cm.mixed(12)
    st = cm.map_batch(AWSetBatch.from_docs(3, [(x.ents, x.vv) for x in docs]), tod)
    tb, op = cm.map_batch(tomb_batch([x.tombs for x in docs]), tod), op_batch(docs)
    n_same = 0
    for d, x in enumerate(docs):
        bumps = sum(1 for k, _ in x.ops if k in (ADD, DDEL))
        s = starts[d % len(starts)]
        clock0 = s if s is not None else (1 << 64) - 1 - bumps
        st.vv[d * 3 + x.actor] = clock0
        if d // len(starts) == 1:  # the entry of key 30 under the dot the first bump mints
            i = int(st.offsets[d]) + 1
            assert int(st.keys[i]) == 30
            st.counters[i] = clock0 + 1
            n_same += 1
    logs = check_call(eng, torch, st, tb, op, what="wide")
    assert n_same == len(starts) and all(logs[len(starts) + j] == ([], [], 8) for j in range(len(starts)))
    top = max(c for _, ups, _ in logs for _, _, c, _ in ups)
    assert top == (1 << 64) - 1 and any(c >= 1 << 63 for r, _, _ in logs for _, _, c in r)


# -------------------------------------------------------------- 6. composition

def test_a_log_list_is_a_tomb_batch(eng, torch):
    """Each list, wrapped as a TombBatch as it stands, answers crdt_tomb_has_async: every
    record's key is found with its dot, a key of another document's list is not."""
    _, st, tb, op = concat_docs()
    n = st.n_docs
    _, logs = reference(st, tb, op)
    out, tout, log = run_log(eng, torch, st, tb, op, pad=0)
    for which, lst in ((0, log.removed()), (1, log.upserted())):
        per_doc = [[r[0] for r in logs[d][which]] + [12345] for d in range(n)]
        want = [w for d in range(n) for w in [(1, r[1], r[2]) for r in logs[d][which]] + [(0, 0, 0)]]
        q = QueryBatch.from_lists(per_doc)
        res = QueryBuffers(q.n_queries, device=dev_of(torch))
        eng.tomb_has_async(lst, q.to(dev_of(torch)), res)
        eng.sync()
        found, actors, counters = res.numpy()
        assert found.tolist() == [w[0] for w in want] and sum(found.tolist()) > 500
        hit = found.astype(bool)
        assert actors[hit].tolist() == [w[1] for w in want if w[0]]
        assert counters[hit].tolist() == [w[2] for w in want if w[0]]


def test_sparse_apply_round_with_the_log(eng, torch):
    """replica_select, apply with log, replica_scatter with nothing downloaded in between:
    the state equals apply over the whole batch (empty op lists elsewhere), and the selected
    documents' logs are the oracle's for those documents."""
    dev = dev_of(torch)
    rep, idx, part, full = apply_round_case()
    n, R, m = rep.n_docs, rep.state.R, len(idx)
    dr, didx = rep.to(dev), words(torch, idx)
    nops = int(full.op_off[-1])
    fo = OutBuffers(n, R, int(rep.state.offsets[-1]) + nops, device=dev)
    ft = TombBuffers(n, int(rep.tombs.offsets[-1]) + nops, device=dev)
    eng.apply_async(dr.state, full.to(dev), fo, dr.tombs, ft)
    want = poisoned_replica(torch, n, R, fo.slots, int(ft.keys.numel()))
    eng.replica_select_async(Replica(fo.as_batch(), ft, 0, dr.doc_actor), want)
    e_sel, t_sel = rep.state.live_slots(), int(rep.tombs.offsets[-1])
    sel = poisoned_replica(torch, m, R, e_sel, t_sel)
    eng.replica_select_async(dr, sel, didx, None, m)
    pops = int(part.op_off[-1])
    so = OutBuffers(m, R, e_sel + pops, device=dev)
    sto = TombBuffers(m, t_sel + pops, device=dev)
    log = poison(torch, MergeLogBuffers(m, e_sel, pops, device=dev), LOG_F)
    dpart = part.to(dev)
    dpart.doc_actor = sel.doc_actor  # the selected actors, as they came out of the select
    eng.apply_log_async(sel.state.as_batch(), dpart, so, log, sel.tombs, sto)
    got = poisoned_replica(torch, n, R, want.entry_slots, want.tomb_slots)
    eng.replica_scatter_async(dr, Replica(so.as_batch(), sto, 0, sel.doc_actor), didx, got)
    eng.sync()
    for a, b in zip(got.poisoned, want.poisoned):
        assert torch.equal(a, b)
    ref, _ = ref_log(rep.state, rep.tombs, full)
    g = log.numpy()
    n_rec = 0
    for j, d in enumerate(np.asarray(idx).tolist()):
        rem, ups, f = ref[d]
        ro, uo = int(g["rem_offsets"][j]), int(g["ups_offsets"][j])
        assert int(g["flags"][j]) == f and int(g["rem_counts"][j]) == len(rem) and int(g["ups_counts"][j]) == len(ups)
        assert list(zip(g["rem_keys"][ro:ro + len(rem)].tolist(), g["rem_actors"][ro:ro + len(rem)].tolist(),
                        g["rem_counters"][ro:ro + len(rem)].tolist())) == rem, d
        assert list(zip(g["ups_keys"][uo:uo + len(ups)].tolist(), g["ups_actors"][uo:uo + len(ups)].tolist(),
                        g["ups_counters"][uo:uo + len(ups)].tolist(), g["ups_kind"][uo:uo + len(ups)].tolist())) == ups, d
        n_rec += len(rem) + len(ups)
    assert n_rec > 0 and g["summary"].tolist() == summary_of([ref[d] for d in np.asarray(idx).tolist()])


# ------------------------------------------------------- 7. call-level checks

def small():
    docs = [LOG_BY_NAME[nm].docs[0] for nm in ("slack_3", "add_of_live_key", "rem_positions_of_65", "ups_256", "no_ops")]
    return AWSetBatch.from_docs(3, [(x.ents, x.vv) for x in docs]), tomb_batch([x.tombs for x in docs]), op_batch(docs)


@pytest.mark.parametrize("kw", [dict(summary=False), dict(kind=False), dict(summary=False, kind=False)],
                         ids=["no_summary", "no_kind", "neither"])
def test_optional_outputs(eng, torch, kw):
    st, tb, op = small()
    docs, logs = reference(st, tb, op)
    got = run_log(eng, torch, st, tb, op, **kw)
    eng.sync()
    Image(st, tb, op, docs, logs, **kw).check(*got, what=str(kw))


def test_no_documents(eng, torch):
    dev = dev_of(torch)
    z = lambda dt: torch.zeros(1, dtype=dt, device=dev)  # noqa: E731
    st = AWSetBatch(3, z(torch.int32), z(torch.int64), z(torch.int32), z(torch.int64), z(torch.int64))
    op = OpBatch(z(torch.int32), z(torch.uint8), z(torch.int64), z(torch.int32))
    assert st.n_docs == 0 and op.n_docs == 0
    host = AWSetBatch.from_docs(3, [])
    out, tout, log = buffers(torch, host, None, OpBatch.from_lists([], []))
    eng.apply_log_async(st, op, out, log, None, tout)
    eng.sync()
    g = download(log, LOG_F)
    assert g["summary"][:5].tolist() == [0] * 5
    for f in LOG_F:
        if f != "summary":
            assert (g[f] == (P8 if g[f].dtype == U8 else P32 if g[f].dtype == U32 else P64)).all(), f
    for buf, fields in ((out, OUT_F), (tout, TOMB_F)):
        for f, a in download(buf, fields).items():
            assert (a == (P32 if a.dtype == U32 else P64)).all(), f


def test_argument_errors(eng, torch):
    """Every one of these is refused on the host: nothing is launched."""
    st, tb, op = small()
    dev = dev_of(torch)
    dst, dtb, dop = st.to(dev), tb.to(dev), op.to(dev)
    out, tout, log = buffers(torch, st, tb, op)
    lib, ctx, ref = abi.lib(), eng._ctx, ctypes.byref

    def call(s=dst, t=dtb, o=dop, ou=out, to=tout, lg=log, edit=None, null=()):
        cs, ct, co, cou, cto, clg = s.c(), t.c(), o.c(), ou.c(), to.c_out(), lg.c()
        named = dict(state=cs, tombs=ct, ops=co, out=cou, tomb_out=cto, log=clg)
        if edit:
            edit(named)
        args = [None if k in null else ref(v) for k, v in named.items()]
        return lib.crdt_awset_apply_log_async(ctx, *args, None)

    for who in ("state", "ops", "out", "log"):
        assert call(null=(who,)) == CRDT_E_INVALID, who
    assert lib.crdt_awset_apply_log_async(None, ref(dst.c()), None, ref(dop.c()), ref(out.c()), None, ref(log.c()),
                                          None) == CRDT_E_INVALID
    for f in [f for f in LOG_F if f not in ("summary", "ups_kind")]:
        assert call(edit=lambda a, f=f: setattr(a["log"], f, None)) == CRDT_E_INVALID, f
    # what crdt_awset_apply_async refuses
    assert call(edit=lambda a: setattr(a["ops"], "n_docs", st.n_docs + 1)) == CRDT_E_INVALID
    assert call(edit=lambda a: setattr(a["ops"], "op_off", None)) == CRDT_E_INVALID
    assert call(edit=lambda a: setattr(a["out"], "keys", None)) == CRDT_E_INVALID
    assert call(edit=lambda a: setattr(a["tomb_out"], "counts", None)) == CRDT_E_INVALID
    assert call(edit=lambda a: setattr(a["tombs"], "keys", None)) == CRDT_E_INVALID
    # two written arrays starting at one address
    for (x, fx), (y, fy) in ((("log", "rem_keys"), ("log", "ups_keys")), (("log", "rem_counts"), ("log", "ups_counts")),
                             (("log", "rem_keys"), ("out", "keys")), (("log", "ups_counters"), ("tomb_out", "counters")),
                             (("log", "rem_offsets"), ("out", "offsets")), (("log", "flags"), ("log", "ups_kind")),
                             (("log", "summary"), ("tomb_out", "counts"))):
        assert call(edit=lambda a: setattr(a[x], fx, getattr(a[y], fy))) == CRDT_E_INVALID, (fx, fy)
    # a written array starting where an input array of the same kind starts
    for (x, fx), (y, fy) in ((("log", "rem_keys"), ("state", "keys")), (("log", "rem_offsets"), ("state", "offsets")),
                             (("log", "ups_offsets"), ("ops", "op_off")), (("log", "ups_keys"), ("ops", "keys")),
                             (("log", "ups_kind"), ("ops", "kind")), (("log", "rem_actors"), ("tombs", "actors")),
                             (("out", "vv"), ("state", "vv")), (("log", "ups_counts"), ("ops", "doc_actor"))):
        assert call(edit=lambda a: setattr(a[x], fx, getattr(a[y], fy))) == CRDT_E_INVALID, (fx, fy)
    eng.sync()
    for buf, fields in ((out, OUT_F), (tout, TOMB_F), (log, LOG_F)):  # the refused calls wrote nothing
        for f, a in download(buf, fields).items():
            assert (a == (P8 if a.dtype == U8 else P32 if a.dtype == U32 else P64)).all(), f
    # the same arguments unedited, and without the optional arrays, are accepted
    docs, logs = reference(st, tb, op)
    for f in (None, "summary", "ups_kind"):
        assert call(edit=(lambda a, f=f: setattr(a["log"], f, None)) if f else None) == 0, f
        eng.sync()
    Image(st, tb, op, docs, logs).check(out, tout, log, what="accepted")


def _bits(got):
    return [download(b, f) for b, f in zip(got, (OUT_F, TOMB_F, LOG_F))]


def test_two_runs_write_the_same_bits(eng, torch):
    _, st, tb, op = concat_docs()
    runs = []
    for _ in range(2):
        got = run_log(eng, torch, st, tb, op)
        eng.sync()
        runs.append(_bits(got))
    for a, b in zip(*runs):
        for f in a:
            assert (a[f] == b[f]).all(), f  # slack and padding included: both runs started from the same poison


def test_graph_capture(torch):
    """Captured on a fresh context (the call's workspace is the context's from its creation),
    replayed once with the op keys changed in place, exact."""
    docs = [c.docs[0] for c in LOG_CASES if not c.slack] + [mixed_doc(256), mixed_doc(255, 1, 1)]
    moved = [x._replace(ops=[(kind, k if kind == DDEL or k > 1 << 62 else k + 10) for kind, k in x.ops]) for x in docs]
    st, tb = AWSetBatch.from_docs(3, [(x.ents, x.vv) for x in docs]), tomb_batch([x.tombs for x in docs])
    op, op2 = op_batch(docs), op_batch(moved)
    assert (op2.kind == op.kind).all() and (op2.keys != op.keys).any()
    dev = dev_of(torch)
    e = crdtgpu.Engine(0)
    try:
        dst, dtb, dop = st.to(dev), tb.to(dev), op.to(dev)
        out, tout, log = buffers(torch, st, tb, op)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.apply_log_async(dst, dop, out, log, dtb, tout, stream=torch.cuda.current_stream())
        dop.keys.copy_(op2.to(dev).keys)
        for buf, fields in ((out, OUT_F), (tout, TOMB_F), (log, LOG_F)):
            poison(torch, buf, fields)
        g.replay()
        e.sync(torch.cuda.current_stream())
        want, logs = reference(st, tb, op2)
        assert logs != reference(st, tb, op)[1]
        Image(st, tb, op2, want, logs).check(out, tout, log, what="replay")
    finally:
        e.close()


def test_ordered_after_a_call_on_another_stream(eng, torch):
    """The logged call reads the output of a plain apply issued on another stream."""
    _, st, tb, op = concat_docs()
    dev = dev_of(torch)
    n, nops = st.n_docs, slots_of_ops(op)
    mid, mid_t = OutBuffers(n, 3, slots_of(st) + nops, device=dev), TombBuffers(n, slots_of(tb) + nops, device=dev)
    for b, fields in ((mid, OUT_F), (mid_t, TOMB_F)):
        for f in fields:
            getattr(b, f).zero_()  # a logged call that ran first would see an empty batch
    rc, wo, wt = oracle.apply(st, op, tb)
    assert rc == 0
    st2, tb2 = wo.as_batch(), wt
    docs, logs = reference(st2, tb2, op)
    out, tout, log = buffers(torch, st2, tb2, op)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    dst, dtb, dop = st.to(dev), tb.to(dev), op.to(dev)
    torch.cuda.synchronize()
    eng.apply_async(dst, dop, mid, dtb, mid_t, stream=sa)
    eng.apply_log_async(mid.as_batch(), dop, out, log, mid_t, tout, stream=sb)
    eng.sync(sb)
    assert sum(len(r) + len(u) for r, u, _ in logs) > 100
    Image(st2, tb2, op, docs, logs).check(out, tout, log, what="second round")


def test_host_form(eng):
    st, tb, op = small()
    docs, logs = reference(st, tb, op)
    go, gt, lg = eng.apply_log(st, op, tb)
    po, pt = eng.apply(st, op, tb)
    for d in range(st.n_docs):
        assert doc_of(go, gt, d, 3) == docs[d] == doc_of(po, pt, d, 3)
        ro, uo = int(lg.rem_offsets[d]), int(lg.ups_offsets[d])
        assert (int(lg.rem_counts[d]), int(lg.ups_counts[d]), int(lg.flags[d])) == (len(logs[d][0]), len(logs[d][1]), logs[d][2])
        assert lg.rem_keys[ro:ro + len(logs[d][0])].tolist() == [r[0] for r in logs[d][0]]
        assert lg.ups_keys[uo:uo + len(logs[d][1])].tolist() == [u[0] for u in logs[d][1]]
    assert lg.summary.tolist() == summary_of(logs)
