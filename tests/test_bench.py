"""CPU tests of bench.py's command line and of what --dump-outputs writes (the timed path itself needs the GPU)."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def _fake_pipe(torch, w, h, bits, n, seed):
    """an object with the attributes dump_outputs reads from a Pipeline: n output frames of 4:2:0 planes with 256-byte pitches"""
    bps = 2 if bits > 8 else 1
    g = torch.Generator().manual_seed(seed)
    frames = []
    for _ in range(n):
        planes = []
        for p in range(3):
            ph, pw = h >> (1 if p else 0), w >> (1 if p else 0)
            pitch = (pw * bps + 255) // 256 * 256
            planes.append(torch.randint(0, 256, (ph, pitch), generator=g, dtype=torch.int32).to(torch.uint8))
        frames.append(planes)
    return types.SimpleNamespace(w=w, h=h, bits=bits, tr=2, out=frames)


@pytest.mark.parametrize("bits", [8, 16])
def test_dump_outputs_writes_seeded_float_samples(tmp_path, bits):
    import torch
    bench = _bench()
    w, h, n = 96, 40, 5
    pipe = _fake_pipe(torch, w, h, bits, n, seed=7)
    budget = 4 * 2 * w * 30                                      # room for 30 sampled rows per plane
    files = bench.dump_outputs(torch, pipe, str(tmp_path / "a"), budget=budget)
    again = bench.dump_outputs(torch, pipe, str(tmp_path / "b"), budget=budget)
    assert [os.path.basename(f) for f in files] == [os.path.basename(f) for f in again]
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.path.basename(f) for f in files)
    for f, g in zip(files, again):
        a = np.load(f)
        assert a.dtype in (np.float32, np.float64)
        assert np.array_equal(a, np.load(g)), "the same outputs must give the same files"
    bps = 2 if bits > 8 else 1

    def plane(i, p):
        pw = w >> (1 if p else 0)
        raw = pipe.out[i][p][:, :pw * bps].numpy()
        return raw.view(np.uint16) if bps == 2 else raw
    d = str(tmp_path / "a")
    sums = np.load(os.path.join(d, "degrain2_sums.npy"))
    assert sums.shape == (n, 3, 2)
    for i in range(n):
        for p in range(3):
            v = plane(i, p).astype(np.int64)
            wgt = (np.arange(v.size) % 251 + 1).reshape(v.shape)
            assert sums[i, p, 0] == v.sum() and sums[i, p, 1] == (v * wgt).sum()
    total_rows = 0
    for p, name in enumerate("yuv"):
        rows = np.load(os.path.join(d, "degrain2_%s.npy" % name))
        where = np.load(os.path.join(d, "degrain2_%s_rows.npy" % name)).astype(np.int64)
        assert rows.shape == (30, w >> (1 if p else 0)) and where.shape == (30, 2)
        assert len({tuple(x) for x in where}) == 30
        for r, (i, ln) in zip(rows, where):
            assert np.array_equal(r, plane(i, p)[ln].astype(np.float32))
        total_rows += rows.nbytes
    assert total_rows <= budget


def test_bench_options():
    """--full and --dump-outputs exist; --steps sets the number of timed steps and must be positive"""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr
