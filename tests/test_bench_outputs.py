"""CPU: bench.py --dump-outputs (dump_outputs / named_outputs): every value
exact in float32 / float64, the total within the byte budget, and a larger
array cut to the same seeded rows in every run."""
import os

import numpy as np
import torch

import bench


def test_dump_is_exact_and_whole_when_it_fits(tmp_path):
    n = 1000
    g = torch.Generator().manual_seed(7)
    crc = torch.randint(-2**31, 2**31 - 1, (n,), dtype=torch.int32, generator=g)
    crc[0], crc[1] = -1, -2**31  # 0xffffffff and 0x80000000 as uint32
    sig = torch.randint(0, 256, (n, 24), dtype=torch.uint8, generator=g)
    rep = torch.arange(n, dtype=torch.int64) + (1 << 40)
    ref = torch.randint(0, 2**31 - 1, (n,), dtype=torch.int32, generator=g)
    bench.dump_outputs(str(tmp_path), bench.named_outputs(crc, sig, (rep, ref)))
    assert sorted(os.listdir(tmp_path)) == ["crc.npy", "dedup_ref.npy", "dedup_rep.npy", "sig.npy"]
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert got["crc"].dtype == np.float64 and got["sig"].dtype == np.float32
    assert np.array_equal(got["crc"].astype(np.uint32), crc.numpy().view(np.uint32))
    assert got["crc"][0] == 0xFFFFFFFF and got["crc"][1] == 0x80000000
    assert np.array_equal(got["sig"].astype(np.uint8), sig.numpy())
    assert np.array_equal(got["dedup_rep"].astype(np.int64), rep.numpy())
    assert np.array_equal(got["dedup_ref"].astype(np.int32), ref.numpy())


def test_dump_samples_the_same_rows_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 40_000)  # 10,000 bytes per array
    n = 5000
    sig = (torch.arange(n * 24, dtype=torch.int64) % 251).to(torch.uint8).view(n, 24)
    packed = torch.arange(n * 2, dtype=torch.int64).view(n, 2)
    outs = {"crc": torch.arange(n, dtype=torch.int32), "sig": sig, "dedup_packed": packed,
            "x": torch.zeros(3, dtype=torch.int32)}
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), outs)
    bench.dump_outputs(str(b), outs)
    total = 0
    for f in os.listdir(a):
        x, y = np.load(a / f), np.load(b / f)
        assert np.array_equal(x, y), f
        total += x.nbytes
    assert total <= 40_000
    crc = np.load(a / "crc.npy")
    assert crc.shape == (1250,) and np.all(np.diff(crc) > 0)  # sorted distinct rows
    assert np.all(crc < n)
    # each sampled row is a whole row of its source
    s = np.load(a / "sig.npy")
    assert s.shape == (104, 24)
    first = s[:, 0].astype(np.int64)
    assert np.array_equal(s, (first[:, None] + np.arange(24)[None, :]) % 251)
    p = np.load(a / "dedup_packed.npy")
    assert p.shape == (625, 2) and np.array_equal(p[:, 1], p[:, 0] + 1) and np.all(p[:, 0] % 2 == 0)
    assert np.load(a / "x.npy").shape == (3,)  # a small array stays whole


def test_named_outputs_by_path():
    t = torch.zeros(2)
    assert list(bench.named_outputs(t, None, None)) == ["crc"]
    assert list(bench.named_outputs(t, t, (t, t))) == ["crc", "sig", "dedup_rep", "dedup_ref"]
    assert list(bench.named_outputs(None, None, t)) == ["dedup_packed"]
