"""GPU parity of the wave join's per-wave metadata load (csrc/join.hip,
meta_vec_issue): a wave loads the slot bounds and live counts of its own
cnt <= K documents only (lanes at or past cnt repeat the wave's first
document), so the cases here are the ones where cnt, the last wave and the
last workgroup are partly filled.

Every case is bit-exact against the C oracle (oracle/awset_oracle.c), never
against another GPU run.  Outputs start filled with -1 (bench.py's poison), so
a document that no wave wrote shows in its count, clock and slot bounds.
"""

import functools
import random

import numpy as np
import pytest

from crdtgpu.batch import OutBuffers
from helpers import batch_of, random_state
from oracle import oracle
from test_gpu_parity import assert_same_all, host_out

pytestmark = pytest.mark.gpu

R = 2
WAVES = 4  # waves per workgroup (join.hip, kJoinWaves): wave w of a workgroup takes documents base + w + k * WAVES
N_DOCS = [1, 3, 31, 32, 33, 127, 257, 1025]
KS = [1, 2, 4, 8, 16]
SLACK = 3


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "GPU tests need a HIP device"
    return t


@pytest.fixture(scope="module")
def eng(torch):
    import crdtgpu

    e = crdtgpu.Engine(0)
    yield e
    e.close()


@pytest.fixture(params=KS, ids=lambda k: "K%d" % k)
def k_eng(eng, request):
    eng.set_option("join_docs_per_wave", request.param)
    yield eng, request.param
    eng.set_option("join_docs_per_wave", 8)


def _docs(n, large=()):
    """n document pairs of 0..64 entries a side over a small key universe (common
    keys in most documents, dots above and below the other side's clock);
    large: {document: (dst entries, src entries)} for documents above 64."""
    rng = random.Random(0xA11CE + n)
    large = dict(large)
    sz = lambda: rng.choice([0, 1, 2, 17, 63, 64, rng.randint(0, 64)])  # noqa: E731
    dsts, srcs = [], []
    for d in range(n):
        nd, ns = large.get(d, (sz(), sz()))
        uni = max(300, 3 * max(nd, ns))
        dsts.append(random_state(rng, R, nd, uni, 25))
        srcs.append(random_state(rng, R, ns, uni, 25))
    return dsts, srcs


@functools.lru_cache(maxsize=None)
def case(n, slack):
    """Host batches of n pairs (slack > 0: with `counts` and spare slots) and
    the oracle's join in both directions -- computed once, never modified."""
    dsts, srcs = _docs(n)
    a, b = batch_of(R, dsts, slack=slack), batch_of(R, srcs, slack=slack)
    assert (a.counts is not None) == bool(slack)
    rc1, ab = oracle.join(a, b)
    rc2, ba = oracle.join(b, a)
    assert rc1 == 0 and rc2 == 0
    return a, b, ab, ba


def poisoned(torch, n, slots, shared_keys=None):
    o = OutBuffers(n, R, slots, device=torch.device("cuda:0"), shared_keys=shared_keys)
    for t in (o.offsets, o.counts, o.keys, o.actors, o.counters, o.vv):
        t.fill_(-1)
    return o


@pytest.mark.parametrize("slack", [0, SLACK], ids=["tight", "counts"])
@pytest.mark.parametrize("n", N_DOCS)
def test_join_and_exchange_partial_waves(k_eng, torch, n, slack):
    """n is 1, 3, a workgroup of the default K more or less one document, and
    sizes that leave the last wave fewer than K documents and the last
    workgroup fewer than WAVES waves, for every K; inputs with and without
    `counts`; the join, and the exchange with an own and a shared key column."""
    eng, _ = k_eng
    a, b, ab, ba = case(n, slack)
    dev = torch.device("cuda:0")
    da, db = a.to(dev), b.to(dev)
    slots = int(a.offsets[-1]) + int(b.offsets[-1])
    eng.set_max_doc_entries(64)
    try:
        o = poisoned(torch, n, slots)
        eng.join_async(da, db, o)
        eng.sync()
        assert_same_all(host_out(o, torch), ab, n, R)
        for shared in (False, True):
            o1 = poisoned(torch, n, slots)
            o2 = poisoned(torch, n, slots, shared_keys=o1 if shared else None)
            eng.exchange_async(da, db, o1, o2)
            eng.sync()
            assert_same_all(host_out(o1, torch), ab, n, R)
            assert_same_all(host_out(o2, torch), ba, n, R)
    finally:
        eng.set_max_doc_entries()


@functools.lru_cache(maxsize=None)
def lane_edge_case(K, n=127):
    """n pairs with documents above 64 entries at lane 0 of a wave, at lane
    cnt - 1 of a full and of a partly filled wave of K documents, and the last
    document; with the oracle's join in both directions."""
    per = WAVES * K
    last_block = (n - 1) // per * per
    last_wave = last_block + min(WAVES, n - last_block) - 1  # first document of the last wave that has any
    cnt_last = (n - last_wave + WAVES - 1) // WAVES
    at = {0: (65, 70),  # lane 0 of the first wave
          (K - 1) * WAVES: (130, 3),  # lane cnt - 1 of a full wave (K = 1: document 0 again)
          last_wave: (700, 66),  # lane 0 of the last wave
          last_wave + (cnt_last - 1) * WAVES: (64, 65),  # its lane cnt - 1
          n - 1: (90, 200)}  # the last document
    dsts, srcs = _docs(n, at)
    a, b = batch_of(R, dsts), batch_of(R, srcs)
    rc1, ab = oracle.join(a, b)
    rc2, ba = oracle.join(b, a)
    assert rc1 == 0 and rc2 == 0
    return a, b, ab, ba


def test_large_documents_at_wave_lane_edges(k_eng, torch):
    """Documents above 64 entries at the lane edges of lane_edge_case, with the
    promise of small documents unset: each reaches the worklist of the tile path
    once and comes out equal to the oracle, join and exchange."""
    eng, K = k_eng
    a, b, ab, ba = lane_edge_case(K)
    n = a.n_docs
    dev = torch.device("cuda:0")
    da, db = a.to(dev), b.to(dev)
    slots = int(a.offsets[-1]) + int(b.offsets[-1])
    o = poisoned(torch, n, slots)
    eng.join_async(da, db, o)
    eng.sync()
    assert_same_all(host_out(o, torch), ab, n, R)
    o1, o2 = poisoned(torch, n, slots), poisoned(torch, n, slots)
    eng.exchange_async(da, db, o1, o2)
    eng.sync()
    assert_same_all(host_out(o1, torch), ab, n, R)
    assert_same_all(host_out(o2, torch), ba, n, R)


def test_large_first_document_is_pushed_once(k_eng, torch):
    """Three documents, the first one large: its wave holds one document, and the
    lanes past it repeat that document's metadata.  Were they not masked out of
    the worklist push, the wave would push it 64 times into a worklist of 3
    slots, which the call reports (CRDT_E_WORKSPACE at the sync)."""
    eng, _ = k_eng
    dsts, srcs = _docs(3, {0: (80, 100), 2: (3, 65)})
    a, b = batch_of(R, dsts), batch_of(R, srcs)
    rc, ab = oracle.join(a, b)
    assert rc == 0
    dev = torch.device("cuda:0")
    o = poisoned(torch, 3, int(a.offsets[-1]) + int(b.offsets[-1]))
    eng.join_async(a.to(dev), b.to(dev), o)
    eng.sync()
    assert_same_all(host_out(o, torch), ab, 3, R)
