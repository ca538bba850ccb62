"""CPU check of the writer behind `bench.py --dump-outputs`: float32 .npy files of the loss and of
every store's master weights and AdamW moments, whole when small, else the same seeded sample of
positions on every call (so that two builds' dumps compare element for element)."""
import os
import types

import numpy as np
import torch

import bench


def _state(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    stores = [types.SimpleNamespace(master=torch.randn(n, generator=g)) for n in sizes]
    return types.SimpleNamespace(stores=stores, m=[torch.randn(n, generator=g) for n in sizes],
                                 v=[torch.rand(n, generator=g) for n in sizes])


def test_dump_outputs_sample_is_fixed(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 64)
    opt = _state((1000, 10), seed=0)
    loss = torch.tensor(1.25, dtype=torch.float64)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, loss, opt)
    bench.dump_outputs(b, loss, opt)
    names = sorted(os.listdir(a))
    assert names == sorted(["loss.npy"] + [f"store{i}_{k}.npy" for i in (0, 1)
                                           for k in ("master", "exp_avg", "exp_avg_sq")])
    for f in names:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype == np.float32 and np.array_equal(x, y), f
    assert np.load(os.path.join(a, "loss.npy")).tolist() == [1.25]
    # the small store whole, the large one at 64 positions shared by its three buffers
    assert np.array_equal(np.load(os.path.join(a, "store1_exp_avg.npy")), opt.m[1].numpy())
    big = np.load(os.path.join(a, "store0_master.npy"))
    assert big.shape == (64,)
    where = [int((opt.stores[0].master == v).nonzero()[0, 0]) for v in torch.from_numpy(big)]
    assert np.array_equal(np.load(os.path.join(a, "store0_exp_avg_sq.npy")), opt.v[0][where].numpy())
    # other values at the same positions: the positions do not depend on the data
    other = _state((1000, 10), seed=1)
    bench.dump_outputs(b, loss, other)
    assert np.array_equal(np.load(os.path.join(b, "store0_master.npy")),
                          other.stores[0].master[where].numpy())
