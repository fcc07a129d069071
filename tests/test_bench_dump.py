"""bench.py --dump-outputs and --steps: the blob of the last timed step as .npy files (float32 / float64, <= 64 MB together,
the same sample positions for the same blob), and exactly --steps timed steps by default."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("blob_bytes", "blob_head", "blob_sample_index", "blob_sample", "blob_sha256")


def _load(d):
    return {name: np.load(os.path.join(d, name + ".npy")) for name in NAMES}


def _check(arrays, raw):
    n = raw.size
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["blob_bytes"].tolist() == [n]
    assert np.array_equal(arrays["blob_head"], raw[:1 << 20].astype(np.float32))
    idx = arrays["blob_sample_index"]
    assert idx.size > 0 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert np.array_equal(arrays["blob_sample"], raw[idx.astype(np.int64)].astype(np.float32))
    assert bytes(arrays["blob_sha256"].astype(np.uint8)) == hashlib.sha256(raw.tobytes()).digest()


def test_dump_outputs_host_tensor(tmp_path):
    """the writer on a host tensor: every file float32 / float64, the sample drawn from a fixed seed"""
    import torch
    import bench
    raw = np.random.default_rng(7).integers(0, 256, size=3 << 20).astype(np.uint8)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch.from_numpy(raw))
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    _check(a, raw)
    assert all(np.array_equal(a[k], b[k]) for k in NAMES)          # same blob, same files


def test_dump_outputs_small_blob(tmp_path):
    import torch
    import bench
    raw = np.arange(1000, dtype=np.uint8)
    bench.dump_outputs(str(tmp_path), torch.from_numpy(raw))
    _check(_load(str(tmp_path)), raw)


@pytest.mark.gpu
def test_bench_dump_outputs_and_exact_steps(tmp_path):
    """a fresh bench.py process: one block of exactly --steps timed steps, and the dumped blob is the one the line verified"""
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--quick", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", out], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["timing"]["blocks"] == 1 and line["timing"]["steps_per_block"] == 3
    assert line["ms_per_step"] > 0
    arrays = _load(out)
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(os.path.getsize(os.path.join(out, k + ".npy")) for k in NAMES) <= 64 << 20
    assert arrays["blob_bytes"].tolist() == [line["config"]["blob_bytes"]]
    assert bytes(arrays["blob_sha256"].astype(np.uint8)).hex() == line["verification"]["blob_sha256"]
    assert line["verified"] is True
