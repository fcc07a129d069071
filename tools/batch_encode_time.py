"""batch encode against the existing entry points (GPU box):  python3 tools/batch_encode_time.py [k] [config ... | sweep]

Device time per call (hipEvents around the call on its stream), k repetitions (default 5) after a warm-up call, the columns interleaved
repetition by repetition inside one process, u16 volumes from synth.stack_torch:
  loop     -- SQYAMD_PipelineEncode_UI16_DeviceAt per volume, one after the other on one stream
  slabs3   -- SQYAMD_PipelineEncode_Slabs_UI16_Device, inflight 3, over the same voxels (the volumes lie back to back in one allocation)
  batch0   -- SQYAMD_PipelineEncode_Batch_UI16_Device with encode_batch_joint = 0 (every volume on its own inside the call)
  batch    -- .. as it comes
Configurations: a = 64 x 16x512x512 bitswap1->lz4 (the encode mirror of tools/slabs_decode_time.py's d), b = 256 x 16x128x128 bitswap1->lz4,
c = 256 x 16x128x128 lz4, d = 8 x 64x1024x1024 bitswap1->lz4; quantiser->bitswap1->lz4 (columns loop, batch0, batch -- the slabs of slabs3
get other LUTs than the volumes, so their blobs are not comparable): e = 256 x 16x128x128, f = 64 x 16x512x512, g = 4 x 16x128x128.  For
these the baseline is batch0 -- every volume through the single-call path inside the call, what the call did before the joint form --
and the row ends with the per-kernel device times of one profiled batch call (SQYAMD_Profile_*).  `sweep`: bitswap1->lz4 volumes of 128 KiB .. 128 MiB (z x 256 x 256, as many
as make 1 GiB, at most 256), loop against batch with every volume on the joint path -- the largest size at which batch is not slower than
loop in any of the k pairs is the default of "encode_batch_joint_max_bytes".  Every blob is checked against the loop's.  One JSON line per row."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sqeazy_amd  # noqa: E402
from sqeazy_amd import synth  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 5
CONFIGS = {"a": ("bitswap1->lz4", (16, 512, 512), 64), "b": ("bitswap1->lz4", (16, 128, 128), 256), "c": ("lz4", (16, 128, 128), 256),
           "d": ("bitswap1->lz4", (64, 1024, 1024), 8), "e": ("quantiser->bitswap1->lz4", (16, 128, 128), 256),
           "f": ("quantiser->bitswap1->lz4", (16, 512, 512), 64), "g": ("quantiser->bitswap1->lz4", (16, 128, 128), 4)}
WANT = sys.argv[2:] or sorted(CONFIGS)


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    got = fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b), got


def run(name, pipeline, shape, n, columns, dev, stream, joint_max=None):
    Z = shape[0]
    vol = torch.empty((Z * n,) + tuple(shape[1:]), dtype=torch.uint16, device=dev)
    for s in range(n):
        vol[Z * s:Z * (s + 1)] = synth.stack_torch(shape, np.uint16, dev, seed=synth.SEED + s)
    vb = vol[0:Z].numel() * 2
    cap = (sqeazy_amd.max_compressed_length(pipeline, shape, np.uint16) + 255) & ~255
    out = torch.empty(cap * n, dtype=torch.uint8, device=dev)
    srcs = [vol.data_ptr() + i * vb for i in range(n)]
    shapes = [shape] * n
    sp = stream.cuda_stream

    def loop():
        offs, lens = [], []
        for i in range(n):
            rc, at, ln = sqeazy_amd.encode_device_at(pipeline, srcs[i], shape, np.uint16, out.data_ptr() + i * cap, cap, stream=sp)
            assert rc == 0
            offs.append(i * cap + at)
            lens.append(ln)
        return offs, lens

    def slabs3():
        rc, offs, lens = sqeazy_amd.encode_slabs_device(pipeline, vol.data_ptr(), tuple(vol.shape), np.uint16, n, out.data_ptr(), cap, inflight=3)
        assert rc == 0
        return offs, lens

    def batch():
        rc, offs, lens = sqeazy_amd.encode_batch_device(pipeline, srcs, shapes, np.uint16, out.data_ptr(), cap, stream=sp)
        assert rc == 0
        return offs, lens

    def batch0():
        with sqeazy_amd.option("encode_batch_joint", 0):
            return batch()

    fns = {"loop": loop, "slabs3": slabs3, "batch0": batch0, "batch": batch}
    saved = sqeazy_amd.get_option("encode_batch_joint_max_bytes")
    if joint_max is not None:
        sqeazy_amd.set_option("encode_batch_joint_max_bytes", joint_max)
    try:
        ref = None
        for c in columns:                                   # warm-up, and every column's blobs against the loop's
            out.fill_(0)
            offs, lens = fns[c]()
            torch.cuda.synchronize()
            blobs = [out[o:o + ln].clone() for o, ln in zip(offs, lens)]
            if ref is None:
                ref = blobs
            assert all(torch.equal(x, y) for x, y in zip(blobs, ref)), (name, c)
        ms = {c: [] for c in columns}
        for _ in range(K):
            for c in columns:
                ms[c].append(round(timed(fns[c], stream)[0], 3))
    finally:
        sqeazy_amd.set_option("encode_batch_joint_max_bytes", saved)
    row = {"config": name, "pipeline": pipeline, "volumes": n, "shape": list(shape), "volume_bytes": vb, "ms": ms,
           "GB/s": {c: round(n * vb / min(ms[c]) / 1e6, 1) for c in columns}}
    if "batch" in ms:
        base = [min(ms[c][r] for c in columns if c in ("loop", "slabs3")) for r in range(K)]
        row["batch_wins_every_pair"] = all(b < x for b, x in zip(ms["batch"], base))
        row["baseline_over_batch"] = [round(x / b, 2) for b, x in zip(ms["batch"], base)]
        row["loop_spread"] = [min(ms["loop"]), max(ms["loop"])]
    if "batch" in ms and "batch0" in ms:
        row["batch0_over_batch"] = [round(x / b, 2) for b, x in zip(ms["batch"], ms["batch0"])]
        row["batch_faster_than_batch0_every_pair"] = all(b < x for b, x in zip(ms["batch"], ms["batch0"]))
        row["batch_not_slower_than_batch0_any_pair"] = all(b <= x for b, x in zip(ms["batch"], ms["batch0"]))
    if pipeline.startswith("quantiser"):
        sqeazy_amd.profile_reset()
        sqeazy_amd.profile_enable(True)
        try:
            batch()
            torch.cuda.synchronize()
        finally:
            sqeazy_amd.profile_enable(False)
        row["batch_kernel_ms"] = {k: [round(v[0], 3), v[1]] for k, v in sorted(sqeazy_amd.profile_get().items())}
        sqeazy_amd.profile_reset()
    print(json.dumps(row), flush=True)
    del vol, out
    torch.cuda.empty_cache()
    return row


def main():
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    for name in WANT:
        if name == "sweep":
            best = 0
            for z in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024):
                size = z * 256 * 256 * 2
                n = max(1, min(256, (1 << 30) // size))
                row = run("sweep", "bitswap1->lz4", (z, 256, 256), n, ("loop", "batch"), dev, stream, joint_max=(1 << 32) - 1)
                if all(b <= x for b, x in zip(row["ms"]["batch"], row["ms"]["loop"])):
                    best = size
            print(json.dumps({"sweep": "encode_batch_joint_max_bytes", "largest_size_not_slower_in_any_pair": best}), flush=True)
        else:
            pipeline, shape, n = CONFIGS[name]
            run(name, pipeline, shape, n, ("loop", "batch0", "batch") if pipeline.startswith("quantiser") else ("loop", "slabs3", "batch0", "batch"), dev, stream)


if __name__ == "__main__":
    main()
