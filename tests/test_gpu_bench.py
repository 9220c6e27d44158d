"""GPU: a plain bench.py run (no --full) and its --dump-outputs.

A plain run times --steps steps and prints the headline fields alone; what --full adds (self-check, rooflines,
ingest, sustained pass, CPU baseline) is absent. --dump-outputs writes the last timed step's arrays as float32 /
float64 .npy files, below 64 MB in all, zero past every image's keypoint count.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_headline_and_dump(tmp_path):
    out = str(tmp_path / "dump")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "128", "--pipes", "2", "--dump-outputs", out],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["full"] is False
    assert res["unit"] == "frames/s" and res["higher_is_better"] is True and res["dtype"] == "u8"
    assert res["ms_per_step"] > 0 and res["device_errors"] is None
    # value is frames per second of the timed steps: frames per step / ms_per_step
    assert res["value"] == pytest.approx(128 / (res["ms_per_step"] * 1e-3), rel=1e-3)
    for k in ("bit_exact", "roofline", "stage_ms_per_step", "ingest", "sustained", "cpu_baseline"):
        assert k not in res, k

    arrays = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert set(arrays) == {"counts", "nmatch", "frame_sums", "match_sums", "sample_frames", "keypoints", "descriptors",
                           "matches", "xmatch", "xn", "xbow", "xbn"}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    counts, pick = arrays["counts"], arrays["sample_frames"].astype(int)
    assert counts.shape == (128,) and counts.min() > 0
    assert pick[0] == 0 and pick[-1] == 63 and len(set(pick)) == len(pick) == 16
    kps, desc, mat = arrays["keypoints"], arrays["descriptors"], arrays["matches"]
    S = kps.shape[1]
    assert kps.shape == (32, S, 6) and desc.shape == (32, S, 32) and mat.shape == (32, S)
    for g in range(2):  # graph g's sampled frames: rows 16 g .. 16 g + 15, frames 64 g + pick
        for j, b in enumerate(pick):
            n = int(counts[64 * g + b])
            row = 16 * g + j
            assert np.all(kps[row, :n, 2] > 0) and not kps[row, n:].any() and not desc[row, n:].any()
            assert np.all(mat[row, n:] == -1) and mat[row, :n].max() < counts[64 * g + (b - 1) % 64]
            assert arrays["frame_sums"][64 * g + b, 0] == pytest.approx(kps[row, :, 0].astype(np.float64).sum())
            assert arrays["frame_sums"][64 * g + b, 2] == desc[row].astype(np.float64).sum()
            assert arrays["match_sums"][64 * g + b] == mat[row, :n].astype(np.float64).sum()
            assert arrays["nmatch"][64 * g + b] == (mat[row, :n] >= 0).sum()
    assert arrays["xmatch"].shape == (1, S) and arrays["xn"][0] == (arrays["xmatch"][0] >= 0).sum()
