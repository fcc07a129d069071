"""Kernel times of the background-removal head filters on the bench stack (1024 x 1024 x 512 u16, HBM-resident), each stage alone.

  python3 tools/bkrd_stage_times.py [outdir]     runs itself under `rocprofv3 --kernel-trace --stats` (with a time limit) and prints, per
                                                 kernel, the mean time and the share of HBM peak for the bytes the stage has to move;
                                                 the profiler writes to outdir (default: a fresh temporary directory)
  python3 tools/bkrd_stage_times.py --run        the workload alone: every stage encoded 10 times through the device C-ABI

The bytes: the subtract pass and the 5x5x5 filter read the volume once and write it once (2 GiB); the face histograms read a few frames.
Peak: 8 TB/s (MI355X HBM3E spec; about 6.3 TB/s are reachable with a plain copy)."""
import csv
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (512, 1024, 1024)
STAGES = ["rmestbkrd", "rmbkrd_neighbor5x5x5(threshold=120,fraction=0.5)"]
PEAK = 8.0e12


def run(reps=10):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import sqeazy_amd
    from sqeazy_amd import synth
    dev = torch.device("cuda", 0)
    vol = synth.stack_torch(SHAPE, np.uint16, dev)
    for p in STAGES:
        cap = sqeazy_amd.max_compressed_length(p, SHAPE, np.uint16)
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        for _ in range(reps):
            rc, n = sqeazy_amd.encode_device(p, vol.data_ptr(), SHAPE, np.uint16, out.data_ptr(), cap)
            assert rc == 0, p
        torch.cuda.synchronize()
        del out
    print("workload done")


def main(outdir):
    os.makedirs(outdir, exist_ok=True)
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--",
           sys.executable, os.path.abspath(__file__), "--run"]
    r = subprocess.run(cmd, cwd=ROOT)
    if r.returncode:
        sys.exit(r.returncode)
    stats = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    if not stats:
        sys.exit("no kernel_stats.csv under %s" % outdir)
    vox = SHAPE[0] * SHAPE[1] * SHAPE[2]
    moved = {"bkrd_subtract": 2 * 2 * vox, "bkrd_neighbor5": 2 * 2 * vox}
    with open(stats[0]) as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            if "bkrd" not in name:
                continue
            ms = float(row["AverageNs"]) / 1e6
            key = next((k for k in moved if k in name), None)
            share = "  %.1f GB/s, %.0f %% of HBM peak" % (moved[key] / ms / 1e6, 100.0 * moved[key] / (ms / 1e3) / PEAK) if key else ""
            print("%-60s calls %5s  mean %.3f ms%s" % (name[:60], row["Calls"], ms, share))


if __name__ == "__main__":
    if "--run" in sys.argv:
        run()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="bkrd_times_"))
