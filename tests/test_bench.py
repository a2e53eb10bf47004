"""bench.py: the options of a plain and a --full run, and what --dump-outputs writes (the sampling without a GPU, the
dumped output of a plain run against fp64 pocketfft on the GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from conftest import REL_L2_TOL_F32, from_complex, rel_l2, to_complex


def test_a_plain_run_is_the_default():
    a = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked(argv):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def test_a_small_output_is_dumped_whole(tmp_path):
    out = torch.randn(3, 16, 8, 2, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path), out)
    got = np.load(tmp_path / "out.npy")
    assert got.dtype == np.float64 and np.array_equal(got, out.numpy())


@pytest.mark.parametrize("shape,budget,lead,k", [((40, 12, 32, 2), 16384, 1, 5),    # whole transforms
                                                 ((4, 64, 32, 2), 8192, 2, 32)])    # one transform is too large: rows
def test_a_large_output_is_a_fixed_sample_of_slices(tmp_path, monkeypatch, shape, budget, lead, k):
    monkeypatch.setattr(bench, "DUMP_BYTES", budget)
    n = int(np.prod(shape[:lead]))
    # every slice holds its own index, so the sample shows which slices it took
    out = torch.arange(n, dtype=torch.float32).reshape((n,) + (1,) * (len(shape) - lead))
    out = out.expand((n,) + shape[lead:]).reshape(shape).contiguous()
    got = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out)
        got.append(np.load(tmp_path / d / "out.npy"))
    assert np.array_equal(got[0], got[1]) and got[0].dtype == np.float32
    assert got[0].shape == (k,) + shape[lead:] and got[0].nbytes <= budget
    taken = got[0].reshape(k, -1)[:, 0]
    assert (got[0].reshape(k, -1) == taken[:, None]).all() and (np.diff(taken) > 0).all()
    assert bench.dump_sample(shape, 4)[0] == lead and np.array_equal(bench.dump_sample(shape, 4)[1], taken)


@pytest.mark.parametrize("esz", [4, 8])
def test_every_workload_dumps_at_most_64_mb(esz):
    for name, (shape, _, _) in bench.WORKLOADS.items():
        full = tuple(shape) + (2,)
        lead, idx = bench.dump_sample(full, esz)
        units = int(np.prod(full[:lead]))
        assert len(idx) >= 1 and len(set(idx.tolist())) == len(idx) and idx.max() < units, name
        assert len(idx) * int(np.prod(full[lead:])) * esz <= 64e6, name


@pytest.mark.gpu
def test_a_plain_run_times_the_headline_and_dumps_what_it_computed(tmp_path):
    r = subprocess.run([sys.executable, bench.__file__, "--gpus", "1", "--steps", "5", "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 5 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "GFLOP/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["config"]["workload"] == bench.DEFAULT_WORKLOAD
    for k in ("configs", "rfft_reference_bench", "strong_config5", "cpu_baseline", "vendor_rocfft"):
        assert k not in d, k
    assert d["roofline"]["copy"] is None and d["roofline"]["launch_ms_hip_events"] is None
    # the same rows of the same seeded input (Bench.make_input), transformed by fp64 pocketfft
    shape = bench.WORKLOADS[bench.DEFAULT_WORKLOAD][0] + (2,)
    lead, idx = bench.dump_sample(shape, 4)
    got = np.load(tmp_path / "out.npy")
    assert got.dtype == np.float32 and got.shape == (len(idx),) + shape[lead:]
    dev = torch.device("cuda", 0)
    x = torch.randn(shape, generator=torch.Generator(device=dev).manual_seed(1234), device=dev, dtype=torch.float32)
    xs = x[torch.as_tensor(idx, device=dev)].cpu().numpy()
    del x
    assert rel_l2(got, from_complex(np.fft.fft(to_complex(xs), axis=1), np.float64)) < REL_L2_TOL_F32
