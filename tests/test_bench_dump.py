"""bench.py --dump-outputs on CPU: a train.lua step of small nets through tests/oracle_backend.py, dumped as bench.py dumps
the timed path's last step — float arrays, the same files for the same inputs, large tensors replaced by a fixed sample."""
import json
import os

import numpy as np
import pytest
import torch

import bench
from video_filler_amd import backend as vb

from oracle_backend import OracleBackend


@pytest.fixture()
def cpu_backend():
    old = vb._BACKEND
    b = vb.set_backend(OracleBackend())
    yield b
    vb._BACKEND = old


def _dump(out_dir):
    from video_filler_amd.trainers import CenterTrainer
    tr = CenterTrainer(dict(nBottleneck=32, nef=8, ngf=8, ndf=8, wtl2=0.999, overlapPred=4, batchSize=2), seed=1234)
    tr.set_batch(torch.rand((2, 3, 128, 128), generator=torch.Generator().manual_seed(1234)) * 2 - 1)
    tr.step()
    bench.dump_outputs(tr, tr.losses(), str(out_dir), dict(workload="test"))
    return tr


def test_dump_outputs_deterministic_float_and_sampled(cpu_backend, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 50000)       # netG's parameters (154 k) exceed it, netD's (45 k) do not
    tr = _dump(tmp_path / "a")
    _dump(tmp_path / "b")
    man = json.load(open(tmp_path / "a" / "dump_manifest.json"))
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "a") if f.endswith(".npy"))
    assert names == sorted(man["arrays"]) == ["errD", "errG", "errG_l2", "netG_output", "parametersD", "parametersG"]
    for n in names:
        a, b = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all()
        np.testing.assert_array_equal(a, b)
    assert float(np.load(tmp_path / "a" / "errD.npy")[0]) == tr.losses()["errD"]
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "netG_output.npy"), tr.netG.output.contiguous().numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "parametersD.npy"), tr.netD.reference_flat().numpy())
    pG = tr.netG.reference_flat().numpy()
    assert man["arrays"]["parametersG"]["sampled"] and man["arrays"]["parametersG"]["shape"] == [pG.size]
    idx = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).integers(0, pG.size, 50000))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "parametersG.npy"), pG[idx])
