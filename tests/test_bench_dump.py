"""bench.py --dump-outputs and --steps: the blob of the last timed step as .npy files (float32 / float64, <= 64 MB together,
the same sample positions for the same blob), and exactly --steps timed steps by default; a plain run (no --full) prints the
headline alone."""
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
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--full", "--quick", "--steps", "3", "--warmup", "1",
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


# what only --full measures or checks: none of it may run in a plain run
FULL_ONLY = ("verified", "payload_sha256", "verification", "single_call", "serial_layout", "other_operating_points", "cpu_baseline",
             "host_abi", "north_star", "with_gather")
FULL_ONLY_CONFIG = ("default_options", "single_call_latency_ms", "one_call_at_a_time", "secondary")


@pytest.mark.gpu
def test_bench_plain_run_is_the_headline_alone(tmp_path):
    """a fresh plain bench.py process (no --full): the headline line without any leg of --full, and the blob it dumps equals the
    digest the reference pieces give for the bench stack (tests/golden/headline.json), although the run itself checks nothing"""
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", out], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["metric"] == "encode GB/s (input voxels) for bitswap1->lz4 uint16 volume"
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True and line["dtype"] == "u16"
    assert line["steps"] == 3 and line["timing"]["blocks"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert [k for k in FULL_ONLY if k in line] == [] and [k for k in FULL_ONLY_CONFIG if k in line["config"]] == []
    assert "alone_launch_ms" not in line["roofline"] and line["roofline"]["kernel"] != "none"
    golden = [g for g in json.load(open(os.path.join(ROOT, "tests", "golden", "headline.json")))["stacks"]
              if g["shape_zyx"] == [512, 1024, 1024] and g["z_offset"] == 0 and g["z_total"] == 512]
    assert len(golden) == 1
    arrays = _load(out)
    assert arrays["blob_bytes"].tolist() == [golden[0]["blob_bytes"]] == [line["config"]["blob_bytes"]]
    assert line["config"]["payload_bytes"] == golden[0]["payload_bytes"]
    assert bytes(arrays["blob_sha256"].astype(np.uint8)).hex() == golden[0]["blob_sha256"]
