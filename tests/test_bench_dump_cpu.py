"""CPU suite: bench.py --dump-outputs -- the writer (dtypes, the 64 MB budget, the fixed sample beyond it) and the command-line
checks that run before anything touches a GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_writes_every_array_whole_under_the_budget(tmp_path):
    flow = torch.arange(2 * 5 * 7, dtype=torch.float32).reshape(2, 5, 7)
    idx = torch.arange(12, dtype=torch.int64) - 3
    half = torch.linspace(-1, 1, 9, dtype=torch.float16)
    bench.dump_outputs(str(tmp_path), {"flow": flow, "argmin": idx, "h": half, "flow_i16": flow.to(torch.int16)})
    got = {n: np.load(tmp_path / (n + ".npy")) for n in ("flow", "argmin", "h", "flow_i16")}
    assert got["flow"].dtype == np.float32 and np.array_equal(got["flow"], flow.numpy())
    assert got["argmin"].dtype == np.float64 and np.array_equal(got["argmin"], idx.numpy())
    assert got["h"].dtype == np.float32 and np.array_equal(got["h"], half.float().numpy())
    assert got["flow_i16"].dtype == np.float64 and np.array_equal(got["flow_i16"], flow.numpy())
    man = json.load(open(tmp_path / "manifest.json"))
    assert man["flow"] == {"shape": [2, 5, 7], "dtype": "float32", "sampled": False}


def test_dump_over_the_budget_is_a_fixed_sample(tmp_path):
    a = torch.arange(40000, dtype=torch.float32)
    b = torch.arange(30000, dtype=torch.float64).reshape(100, 300) * 0.5
    budget = 4096 * 3 + 100000                     # room for 100000 data bytes: well under the 400000 of the two arrays
    for d in ("r1", "r2"):
        bench.dump_outputs(str(tmp_path / d), {"a": a, "b": b}, budget=budget)
    total = sum(os.path.getsize(tmp_path / "r1" / f) for f in os.listdir(tmp_path / "r1"))
    assert total <= budget
    for n, src in (("a", a), ("b", b)):
        x, y = np.load(tmp_path / "r1" / (n + ".npy")), np.load(tmp_path / "r2" / (n + ".npy"))
        assert np.array_equal(x, y) and 0 < x.size < src.numel()                        # the same sample in both runs
        flat = src.numpy().reshape(-1)
        assert np.all(np.diff(x) > 0) and np.isin(x, flat).all()                        # sorted indices into the flattened array
    man = json.load(open(tmp_path / "r1" / "manifest.json"))
    assert man["b"]["sampled"] and man["b"]["shape"] == [100, 300] and man["b"]["sample_size"] == np.load(tmp_path / "r1" / "b.npy").size


def test_steps_below_one_is_refused_before_any_gpu_work():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "--steps" in r.stderr
