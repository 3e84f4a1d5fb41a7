"""bench.py's plain run and --dump-outputs: the line a plain run prints carries the headline
figure and nothing that --full measures, and the dumped frame is the timed loop's last frame
(float32 R, G, B; equal to the oracle's), or a fixed sample of a frame over the size limit."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_decodes_and_samples(tmp_path):
    """dump_outputs on host arrays: packed words decode to R, G, B; an RGB8 frame is taken as
    it is; a frame over DUMP_MAX_BYTES is written as the same DUMP_SAMPLE pixels every time."""
    import bench
    H, W = 5, 7
    words = (np.arange(H * W, dtype=np.uint32) * np.uint32(2654435761) & np.uint32(0xFFFFFF)).reshape(H, W)
    rgb = np.stack([(words >> 16) & 0xFF, (words >> 8) & 0xFF, words & 0xFF], axis=-1).astype(np.uint8)
    bench.dump_outputs(str(tmp_path / "a"), words.view(np.int32))
    bench.dump_outputs(str(tmp_path / "b"), rgb)
    a, b = np.load(tmp_path / "a" / "frame_rgb.npy"), np.load(tmp_path / "b" / "frame_rgb.npy")
    assert a.dtype == np.float32 and a.shape == (H, W, 3)
    assert np.array_equal(a, rgb.astype(np.float32)) and np.array_equal(b, a)

    H, W = 2160, 3840                                   # C5's frame: 99.5 MB as float32 RGB
    big = (np.arange(H * W, dtype=np.uint32) * np.uint32(40503) & np.uint32(0xFFFFFF)).reshape(H, W).view(np.int32)
    bench.dump_outputs(str(tmp_path / "c"), big)
    bench.dump_outputs(str(tmp_path / "d"), big)
    c, d = np.load(tmp_path / "c" / "frame_rgb.npy"), np.load(tmp_path / "d" / "frame_rgb.npy")
    assert c.dtype == np.float32 and c.shape == (bench.DUMP_SAMPLE, 3) and c.nbytes <= 64 * 1000 * 1000
    assert np.array_equal(c, d)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(H * W, bench.DUMP_SAMPLE, replace=False))
    w = big.view(np.uint32).reshape(-1)[idx]
    assert np.array_equal(c[:, 0], (w >> 16) & 0xFF) and np.array_equal(c[:, 2], w & 0xFF)


@pytest.mark.gpu
def test_plain_run_line_and_dumped_frame(tmp_path):
    """A plain one-GPU run (small frame of C2): --steps sets the timed steps, the line has the
    headline fields and none of --full's, and DIR/frame_rgb.npy is the oracle's frame."""
    from tests.test_gpu_multirank import _oracle_rgb8
    W, H = 480, 270
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
           "--resolution", f"{W}x{H}", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, f"bench.py failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 4 and line["warmup"] == 2 and line["n_gpus"] == 1 and line["full"] is False
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0 and "Mrays/sec" in line["metric"]
    assert abs(line["value"] - W * H / (line["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * line["value"]
    for key in ("roofline", "cpu_baseline", "kernel_ms", "kernel_ms_first_render", "value_moving_view",
                "dispatch_phases", "frame_latency_ms"):
        assert key not in line, key
    assert [p.name for p in out.iterdir()] == ["frame_rgb.npy"]
    got = np.load(out / "frame_rgb.npy")
    assert got.dtype == np.float32 and got.shape == (H, W, 3)
    bad = int(np.count_nonzero(np.any(got != _oracle_rgb8("C2", W, H).astype(np.float32), axis=-1)))
    assert bad == 0, f"{bad} of {W * H} pixels of the dumped frame differ from the oracle"
