"""bench.py's command line and its output dump, on the host: what a plain run accepts and what --dump-outputs writes."""
import os

import numpy as np
import pytest
import torch

import bench


def test_plain_run_is_the_default_and_steps_are_checked():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert bench.parse_args(["--full", "--dump-outputs", "d"]).full
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_dump_outputs_is_seeded_and_bounded(tmp_path):
    # two f64 arrays (voltages, currents) of any shape stay within 64 MB of .npy
    assert 2 * 8 * (bench.DUMP_LAST_STEP + bench.DUMP_SAMPLE) + 4 * 4096 <= 64 * 2**20
    g = torch.Generator().manual_seed(3)
    out_v = torch.rand((6, 40001, 5), dtype=torch.float64, generator=g)  # 1.2 M values: sampled
    out_i = torch.rand((6, 11, 9), dtype=torch.float64, generator=g)     # small: kept whole
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"out_v": out_v, "out_i": out_i})
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["out_i_last_step.npy", "out_i_sample.npy", "out_v_last_step.npy", "out_v_sample.npy"]
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype == np.float64 and np.array_equal(x, y)
    assert np.array_equal(np.load(tmp_path / "a" / "out_v_last_step.npy"), out_v[:, -1, :].numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "out_i_sample.npy"), out_i.numpy())
    sample = np.load(tmp_path / "a" / "out_v_sample.npy")
    assert sample.shape == (bench.DUMP_SAMPLE,) and np.isin(sample, out_v.numpy()).all()
