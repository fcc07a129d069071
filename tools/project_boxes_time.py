"""boxes of ONE large blob projected along an axis in one call, against what a caller can do without the entry point
(GPU box):  python3 tools/project_boxes_time.py [k] [pipeline ...]

Device time per call sequence (hipEvents around it on its stream, so the host's gaps between launches and every call's own synchronisation
count), k interleaved repetitions (default 7) after a warm-up, all in one process; a sample is REPS sequences in a row, divided by REPS.
A 64x1024x1024 u16 synth.stack_torch stack encoded as ONE blob (`bitswap1->lz4` and `quantiser->bitswap1->lz4`).  Rows:
  same / disjoint, K = 4, 16, 64  -- boxes of 16x64x64, axis 0, max; all in the same 16 frames (24 .. 39), or spread over the four
                                     disjoint z-ranges of 16 frames
  one box 16x512x512              -- axes 0, 1 and 2, max; axis 0 once more as sum
  whole stack along z             -- max; the baseline decodes the whole volume into 128 MiB of scratch
Columns:
  base     -- ONE SQYAMD_Decode_Boxes_*_Device call into scratch of the caller's, then the torch reduction over the widened voxels
              (amax / amin / sum(dtype=int64), batched over the K boxes) cast to the same 32-bit images: what a caller runs without the
              entry point
  again    -- the same once more in every repetition: base / again per pair is the spread a ratio has to beat
  project  -- ONE SQYAMD_Project_Boxes_*_Device call (no scratch of the caller's)
  atomics  -- the same call with "project_boxes_walk" = 0: along axis 0 the integer atomics where `project` walks z in registers (the
              other axes: the same kernel as `project`)
Every column's images are held to each other and to the ones torch computes from the full decode's voxels.  Per row: min-max per column,
the per-pair ratios base / project and base / again, whether every pair is faster by more than the spread, the scratch bytes the baseline
holds, and the per-kernel device times of one profiled `project` call and one profiled `base` call (the storing transposer beside the
projecting one: what the atomics cost).  One JSON line per row."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sqeazy_amd  # noqa: E402
from sqeazy_amd import synth  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 7
REPS = 3
SHAPE = (64, 1024, 1024)
EXTENT = (16, 64, 64)
PIPELINES = sys.argv[2:] or ["bitswap1->lz4", "quantiser->bitswap1->lz4"]
PLACEMENTS = {"same": lambda i: 24, "disjoint": lambda i: 16 * (i % 4)}
COLUMNS = ("base", "again", "project", "atomics")


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(REPS):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / REPS


def profiled(fn):
    sqeazy_amd.profile_reset()
    sqeazy_amd.profile_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        sqeazy_amd.profile_enable(False)
    got = {k: [round(v[0], 3), v[1]] for k, v in sorted(sqeazy_amd.profile_get().items())}
    sqeazy_amd.profile_reset()
    return got


def origins_of(placement, count):
    z = PLACEMENTS[placement]
    per = SHAPE[1] // EXTENT[1] - 1
    return [(z(i), (97 * i % per) * EXTENT[1] + 5, (61 * i % per) * EXTENT[2] + 3) for i in range(count)]


def reduced(voxels, axis, op):
    """the projection of a (K, Z, Y, X) int16 tensor that holds 16-bit voxels, as int32 images that hold the 32-bit elements"""
    wide = voxels.to(torch.int32) & 0xffff
    if op == "max":
        return wide.amax(axis + 1)
    if op == "min":
        return wide.amin(axis + 1)
    return wide.sum(axis + 1, dtype=torch.int64).to(torch.int32)


def rows():
    for placement in PLACEMENTS:
        for count in (4, 16, 64):
            yield "%s K=%d" % (placement, count), origins_of(placement, count), EXTENT, 0, "max"
    for axis in range(3):
        yield "one box 16x512x512 axis %d" % axis, [(24, 256, 256)], (16, 512, 512), axis, "max"
    yield "one box 16x512x512 axis 0 sum", [(24, 256, 256)], (16, 512, 512), 0, "sum"
    yield "whole stack along z", [(0, 0, 0)], SHAPE, 0, "max"


def run(pipeline, dev, stream):
    sp = stream.cuda_stream
    vol = synth.stack_torch(SHAPE, np.uint16, dev)
    cap = sqeazy_amd.max_compressed_length(pipeline, SHAPE, np.uint16)
    blob = torch.empty(cap, dtype=torch.uint8, device=dev)
    rc, n = sqeazy_amd.encode_device(pipeline, vol.data_ptr(), SHAPE, np.uint16, blob.data_ptr(), cap, stream=sp)
    assert rc == 0
    del vol
    fb = SHAPE[1] * SHAPE[2] * 2
    full = torch.empty(SHAPE, dtype=torch.int16, device=dev)            # the voxels every column is held to (quantiser: not the stack's)
    rc = sqeazy_amd.decode_frames_device(blob.data_ptr(), n, 0, SHAPE[0], full.data_ptr(), SHAPE[0] * fb, np.uint16, stream=sp)
    assert rc == 0
    torch.cuda.synchronize()
    for name, origins, extent, axis, op in rows():
        count = len(origins)
        extents = [extent] * count
        truth = torch.stack([full[tuple(slice(a, a + e) for a, e in zip(o, extent))] for o in origins])
        want = reduced(truth, axis, op).cpu().numpy()
        del truth
        scratch = torch.empty((count,) + tuple(extent), dtype=torch.int16, device=dev)      # (the baseline's own: the new call needs none)
        images = torch.empty(want.shape, dtype=torch.int32, device=dev)
        sptrs = [scratch[i].data_ptr() for i in range(count)]
        iptrs = [images[i].data_ptr() for i in range(count)]
        got = {}

        def base():
            rc = sqeazy_amd.decode_boxes_device(blob.data_ptr(), n, origins, sptrs, extents, None, np.uint16, stream=sp)
            assert rc == 0
            got["base"] = got["again"] = reduced(scratch, axis, op)

        def project():
            rc = sqeazy_amd.project_boxes_device(blob.data_ptr(), n, origins, extents, axis, op, iptrs, None, np.uint16, stream=sp)
            assert rc == 0
            got["project"] = images

        def atomics():
            sqeazy_amd.set_option("project_boxes_walk", 0)
            try:
                project()
            finally:
                sqeazy_amd.set_option("project_boxes_walk", 1)
            got["atomics"] = images

        fns = {"base": base, "again": base, "project": project, "atomics": atomics}
        for c in COLUMNS:                                       # warm-up, and every column's images against the full decode's
            scratch.fill_(0)
            images.fill_(0x5A5A5A5A)
            fns[c]()
            torch.cuda.synchronize()
            assert np.array_equal(got[c].cpu().numpy(), want), (pipeline, name, c)
        ms = {c: [] for c in COLUMNS}
        for _ in range(K):
            for c in COLUMNS:
                ms[c].append(round(timed(fns[c], stream), 3))
        gain = [round(x / s, 3) for s, x in zip(ms["project"], ms["base"])]
        spread = [round(x / s, 3) for s, x in zip(ms["again"], ms["base"])]
        row = {"pipeline": pipeline, "row": name, "boxes": count, "extent": list(extent), "axis": axis, "op": op, "stack": list(SHAPE), "blob_bytes": n,
               "ms": ms, "min_max": {c: [min(ms[c]), max(ms[c])] for c in COLUMNS}, "base_over_project": gain, "base_over_again": spread,
               "baseline_scratch_bytes": int(scratch.numel()) * 2}
        row["project_faster_every_pair_by_more_than_the_spread"] = bool(min(gain) > max(max(spread), 1 / min(spread)))
        row["base_over_atomics"] = [round(x / s, 3) for s, x in zip(ms["atomics"], ms["base"])]
        row["project_kernel_ms"] = profiled(project)
        row["atomics_kernel_ms"] = profiled(atomics)
        row["base_kernel_ms"] = profiled(base)
        print(json.dumps(row), flush=True)
        got.clear()
        del scratch, images
        torch.cuda.empty_cache()
    del blob, full
    torch.cuda.empty_cache()


def main():
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    for pipeline in PIPELINES:
        run(pipeline, dev, stream)


if __name__ == "__main__":
    main()
