"""bench.py's host-side pieces, no GPU: the --dump-outputs sampler (dtypes, 64 MB bound, fixed seeded positions) and the option
checks that run before anything touches a device."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_collect_outputs_keeps_small_arrays_whole_in_float32_or_float64():
    named = {"a": torch.arange(12, dtype=torch.float16).reshape(3, 4), "b": torch.ones(5, dtype=torch.float64),
             "idx": torch.tensor([3, 1, 2], dtype=torch.int64), "flag": torch.tensor([True, False]), "note": "not an array"}
    out = bench.collect_outputs(named)
    assert set(out) == {"a", "b", "idx", "flag"}
    assert out["a"].dtype == np.float32 and out["a"].shape == (3, 4) and np.array_equal(out["a"], np.arange(12).reshape(3, 4))
    assert out["b"].dtype == np.float64 and out["idx"].dtype == np.float64 and np.array_equal(out["idx"], [3, 1, 2])
    assert out["flag"].dtype == np.float64 and np.array_equal(out["flag"], [1.0, 0.0])


def test_collect_outputs_samples_what_exceeds_the_budget_at_fixed_positions():
    budget = 4000                                                # bytes: 1000 float32 values over all arrays
    big = torch.arange(100000, dtype=torch.float32)              # value == flat index: the sample shows its positions
    named = {"small": torch.zeros(10), "big": big, "big2": big.reshape(100, 1000).clone()}
    out = bench.collect_outputs(named, budget=budget)
    assert out["small"].shape == (10,)
    assert sum(a.nbytes for a in out.values()) <= budget
    for k in ("big", "big2"):
        a = out[k]
        assert a.ndim == 1 and 400 < a.size < 1000
        assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 100000       # sorted, distinct, in range
    again = bench.collect_outputs(named, budget=budget)
    assert all(np.array_equal(out[k], again[k]) for k in out)                # the same positions every time
    assert not np.array_equal(out["big"], out["big2"])                        # seeded by name


def _bench(*args):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    return subprocess.run([sys.executable, "bench.py"] + list(args), cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=120)


def test_bench_options():
    r = _bench("--help")
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    r = _bench("--workload", "c1", "--breakdown", "x.json")                   # the breakdown is a --full measurement
    assert r.returncode != 0 and "--full" in r.stderr and not os.path.exists(os.path.join(ROOT, "x.json"))
    r = _bench("--workload", "c1", "--steps", "0")
    assert r.returncode != 0 and "--steps" in r.stderr
