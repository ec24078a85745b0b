"""CPU: bench.py --dump-outputs writes an exact, repeatable, bounded sample of
what the timed step computed (bench.dump_outputs), and the options a plain run
leaves out need --full."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

CAP = 128  # slots per document, as the config-2 exchange lays its outputs out


class _Out:
    def __init__(self, n, R, rng):
        u64 = lambda k: torch.from_numpy(rng.integers(0, 2 ** 64, k, dtype=np.uint64).view(np.int64))  # noqa: E731
        self.offsets = torch.from_numpy((np.arange(n + 1) * CAP).astype(np.uint32).view(np.int32))
        self.counts = torch.from_numpy(rng.integers(0, CAP + 1, n).astype(np.uint32).view(np.int32))
        self.keys, self.counters, self.vv = u64(n * CAP), u64(n * CAP), u64(n * R)
        self.actors = torch.from_numpy(rng.integers(0, 2 ** 32, n * CAP).astype(np.uint32).view(np.int32))


class _W:
    R = 2

    def __init__(self, n):
        rng = np.random.default_rng(7)
        self.n = n
        self.bufs = {"a_from_b": _Out(n, self.R, rng), "b_from_a": _Out(n, self.R, rng)}

    def results(self):
        return self.bufs


def _u64(a):
    return (a[:, 0].astype(np.uint64) << np.uint64(32)) | a[:, 1].astype(np.uint64)


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    W = _W(3000)
    ctx = torch.tensor([5, -1], dtype=torch.int64)  # -1: the u64 word 2^64 - 1
    d = tmp_path_factory.mktemp("dump")
    info = bench.dump_outputs(W, ctx, str(d / "x"), 0x5EED)
    return W, d, info, {f[:-4]: np.load(str(d / "x" / f)) for f in os.listdir(str(d / "x"))}


def test_dump_is_exact_float64(dumped):
    W, _, info, files = dumped
    assert info["docs"] == W.n and info["files"] == len(files) == 14
    assert all(a.dtype == np.float64 for a in files.values())
    assert files["causal_context"].tolist() == [[0, 5], [2 ** 32 - 1, 2 ** 32 - 1]]
    docs = files["sample_docs"].astype(np.int64)
    assert sorted(docs.tolist()) == list(range(W.n))
    for name, o in W.bufs.items():
        cnt = o.counts.numpy().view(np.uint32).astype(np.int64)[docs]
        assert (files[name + "_counts"] == cnt).all() and (files[name + "_offsets"] == docs * CAP).all()
        idx = np.concatenate([d * CAP + np.arange(c) for d, c in zip(docs, cnt)])
        assert (_u64(files[name + "_keys"]) == o.keys.numpy().view(np.uint64)[idx]).all()
        assert (_u64(files[name + "_counters"]) == o.counters.numpy().view(np.uint64)[idx]).all()
        assert (files[name + "_actors"] == o.actors.numpy().view(np.uint32)[idx]).all()
        vv = o.vv.numpy().view(np.uint64).reshape(W.n, W.R)[docs].reshape(-1)
        assert (_u64(files[name + "_vv"]) == vv).all()


def test_dump_repeats_and_follows_the_seed(dumped):
    W, d, _, files = dumped
    bench.dump_outputs(W, torch.tensor([5, -1], dtype=torch.int64), str(d / "y"), 0x5EED)
    for f, a in files.items():
        assert np.array_equal(a, np.load(str(d / "y" / (f + ".npy")))), f


def test_dump_samples_within_the_budget(dumped, monkeypatch, tmp_path):
    W, _, _, _ = dumped
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 200_000)
    info = bench.dump_outputs(W, torch.zeros(2, dtype=torch.int64), str(tmp_path), 1)
    on_disk = sum(os.path.getsize(str(tmp_path / f)) for f in os.listdir(str(tmp_path)))
    assert 0 < info["docs"] < W.n and info["bytes"] <= 200_000 + 32 and on_disk <= 200_000 + 32 + 128 * 14
    other = bench.dump_outputs(W, torch.zeros(2, dtype=torch.int64), str(tmp_path / "z"), 2)
    assert not np.array_equal(np.load(str(tmp_path / "sample_docs.npy"))[:8],
                              np.load(str(tmp_path / "z" / "sample_docs.npy"))[:8]) and other["docs"] > 0


def test_legs_need_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--legs", "3"], capture_output=True, text=True)
    assert r.returncode == 2 and "--legs needs --full" in r.stderr
