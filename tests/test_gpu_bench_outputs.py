"""bench.py --dump-outputs: what the last timed step computed, as .npy files - the panorama a caller of
horizonator_amd.horizonator.render() gets for the same view, and nothing larger than the budget."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hzutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_dumped_outputs_are_the_render_of_the_benchmarked_view(tmp_path):
    if not hzutil.hip_available():
        pytest.skip("no HIP device")
    out = tmp_path / "dump"
    # a child process of its own (never an exec from a process that has touched the GPU)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "cfg1", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    files = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(files) == {"image", "ranges", "image_row_sums", "image_col_sums", "ranges_row_sums", "ranges_col_sums"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 << 20

    import bench
    import horizonator_amd
    c = bench.CONFIGS["cfg1"]
    R, W, H = c["R"], c["W"], c["H"]
    h = horizonator_amd.horizonator(bench.LAT, bench.LON, W, H, dir_dems=hzutil.dem_dir_for(bench.LAT, bench.LON, R),
                                    render_radius_cells=R)
    try:
        image, ranges = h.render(-180.0, 180.0, znear=bench.ZNEAR, zfar=600000.0)
    finally:
        h.close()
    assert (image[..., 2] > 0).mean() > 0.05                     # terrain is in view
    assert np.array_equal(files["image"], image.astype(np.float32))
    assert np.array_equal(files["ranges"], ranges)
    assert np.array_equal(files["image_row_sums"], image.sum(axis=1, dtype=np.float64))
    assert np.array_equal(files["ranges_col_sums"], ranges.sum(axis=0, dtype=np.float64))
