"""bench.py's command line: a plain run prints the headline line only, --full the whole
line, and --dump-outputs writes the last timed step's frame -- here config C1 (the
256 x 256 Cornell box), whose frame is pinned bit for bit by tests/golden/c1_cornell_256.npz."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import miro
from conftest import GOLDEN, ROOT
from helpers import bits

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config",
            "scene_setup", "timed_region")
FULL_ONLY = ("roofline", "launch_ms", "frame_latency_ms", "frame_check", "wave_timing_us", "build", "cpu_baseline")


def bench(*argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C1", "--settle-s", "0",
                        *argv], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines   # one JSON result line
    return json.loads(lines[0])


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """Within the budget every array is written whole, as float32 of the given shape; past it
    each file holds the same seeded sample of its array, identical from call to call."""
    import torch
    import bench as B
    shape = (2, 5, 7, 3)
    n = int(np.prod(shape))
    f = torch.arange(n, dtype=torch.float32) / 8
    u = (torch.arange(n) % 256).to(torch.uint8)
    B.dump_outputs(str(tmp_path / "whole"), {"rgb": f, "rgb8": u, "absent": None}, shape)
    assert sorted(os.listdir(tmp_path / "whole")) == ["rgb.npy", "rgb8.npy"]
    a, b = np.load(tmp_path / "whole" / "rgb.npy"), np.load(tmp_path / "whole" / "rgb8.npy")
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == shape
    assert np.array_equal(a.reshape(-1), f.numpy()) and np.array_equal(b.reshape(-1), u.numpy().astype(np.float32))
    # a budget of 2 x (4096 + 4 x 50) bytes: 50 of the 210 elements per file
    monkeypatch.setattr(B, "DUMP_BUDGET", 2 * (4096 + 4 * 50))
    for d in ("s1", "s2"):
        B.dump_outputs(str(tmp_path / d), {"rgb": f, "rgb8": u}, shape)
    s1, s2 = np.load(tmp_path / "s1" / "rgb.npy"), np.load(tmp_path / "s2" / "rgb.npy")
    assert s1.dtype == np.float32 and s1.shape == (50,) and np.array_equal(s1, s2)
    idx = (s1 * 8).astype(np.int64)   # rgb[i] = i / 8: the sampled indices, ascending, the same for both files
    assert (np.diff(idx) >= 0).all() and idx.min() >= 0 and idx.max() < n
    assert np.array_equal(np.load(tmp_path / "s1" / "rgb8.npy"), (idx % 256).astype(np.float32))
    assert sum(os.path.getsize(tmp_path / "s1" / x) for x in os.listdir(tmp_path / "s1")) <= 2 * (4096 + 4 * 50)


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_timed_frame(tmp_path):
    if miro.device_count() < 1:
        pytest.skip("no HIP device")
    out = tmp_path / "dump"
    line = bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(out))
    for k in HEADLINE:
        assert k in line, k
    for k in FULL_ONLY:
        assert k not in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "Mray/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    # value = rays of the timed steps / their time.  The line rounds ms_per_step to 4 decimals
    # (+-0.00005 ms) and value to 2 (+-0.005): value lies between the rates of the two ends of
    # ms_per_step's interval, widened by value's own rounding (and 1e-9 relative for the floats)
    rays, ms, v = line["config"]["rays_per_step"], line["ms_per_step"], line["value"]
    lo = rays / ((ms + 0.00005) * 1e-3) / 1e6 - 0.005
    hi = rays / ((ms - 0.00005) * 1e-3) / 1e6 + 0.005 if ms > 0.00005 else float("inf")
    print("value", v, "between", lo, "and", hi)
    assert lo * (1 - 1e-9) <= v <= hi * (1 + 1e-9)
    g = np.load(os.path.join(GOLDEN, "c1_cornell_256.npz"))
    rgb, rgb8 = np.load(out / "rgb.npy"), np.load(out / "rgb8.npy")
    assert rgb.dtype == rgb8.dtype == np.float32 and rgb.shape == rgb8.shape == (1, 256, 256, 3)
    print("differing float channels:", int((bits(rgb.reshape(-1)) != bits(g["rgb"].reshape(-1))).sum()),
          "8-bit:", int((rgb8.reshape(-1) != g["rgb8"].reshape(-1)).sum()))
    assert np.array_equal(bits(rgb.reshape(-1)), bits(g["rgb"].reshape(-1)))
    assert np.array_equal(rgb8.reshape(-1), g["rgb8"].reshape(-1).astype(np.float32))


@pytest.mark.gpu
def test_full_run_carries_every_other_key():
    if miro.device_count() < 1:
        pytest.skip("no HIP device")
    line = bench("--steps", "2", "--warmup", "1", "--full", "--cpu-seconds", "0.2", "--latency-frames", "1")
    for k in HEADLINE + FULL_ONLY:
        assert k in line, k
    assert line["frame_check"]["equal"] is True and line["build"]["match"] is True
    assert line["cpu_baseline"]["value"] > 0
