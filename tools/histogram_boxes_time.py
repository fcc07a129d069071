"""the intensity histograms of boxes of ONE large blob in one call, against what a caller can do without the entry point
(GPU box):  python3 tools/histogram_boxes_time.py [k] [pipeline ...]

Device time per call sequence (hipEvents around it on its stream, so the host's gaps between launches and every call's own synchronisation
count), k interleaved repetitions (default 7) after a warm-up, all in one process; a sample is REPS sequences in a row, divided by REPS.
A 64x1024x1024 u16 stack encoded as ONE blob (`bitswap1->lz4` and `quantiser->bitswap1->lz4`).  Rows:
  whole stack, shift 0, 2, 6                            -- synth.stack_torch; 65536, 16384 and 1024 bins; 2048 workgroups flush into ONE histogram
  K = 4, 16, 64 boxes of 16x64x64, shift 2              -- in the same 16 frames, and spread over the four disjoint z-ranges of 16 frames
  constant stack (every voxel 1000), whole, shift 0, 2  -- `bitswap1->lz4` only: 64 lanes on one LDS counter, what the merge is for
  noise stack (uniform over the range), whole, shift 0, 2 -- `bitswap1->lz4` only: no two neighbours equal, at shift 2 every one of the
                                                           16384 bins occupied in every workgroup (the flush's worst case), at shift 0
                                                           three voxels in four outside any window
Columns:
  base     -- ONE SQYAMD_Decode_Boxes_*_Device call into scratch of the caller's, then torch.bincount of the shifted voxels per box (cast
              to 32 bits): the same integers, what a caller runs without the entry point
  again    -- the same once more in every repetition: base / again per pair is the spread a ratio has to beat
  none, runs, pieces -- ONE SQYAMD_Histogram_Boxes_*_Device call (no scratch of the caller's) with "histogram_boxes_merge" = 0 (one LDS
              atomic per voxel), 1 (equal neighbours of a thread's run in one add) and 2 (a piece of sixteen bytes whose bins are all
              equal in one add); `hist` below is the column of the library's default
Every column's histograms are held to each other and to torch.bincount of the full decode's voxels.  Per row: min-max per column, the
per-pair ratios base / hist, base / again and none / runs, none / pieces, whether every pair is faster by more than the spread (and whether every
pair is slower by more than it), the scratch bytes the baseline holds, and the per-kernel device times of one profiled call of each
kind.  One JSON line per row, then the rows once more as a table."""
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
PIPELINES = sys.argv[2:] or ["bitswap1->lz4", "quantiser->bitswap1->lz4"]
FINALS = ("bitswap1_histogram_boxes", "bitswap1_quantiser_histogram_boxes", "boxes_histogram_init", "bitswap1_decode_boxes", "bitswap1_quantiser_decode_boxes",
          "lz4_frames_subset_decode")
MERGES = ("none", "runs", "pieces")                                     # "histogram_boxes_merge" 0, 1, 2
DEFAULT_MERGE = sqeazy_amd.get_option("histogram_boxes_merge")


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


def counted(voxels, shift, nbins):
    """the histograms of a (K, ...) int16 tensor that holds 16-bit voxels, as (K, nbins) int32 that holds the 32-bit counters"""
    return torch.stack([torch.bincount(((v.reshape(-1).to(torch.int32) & 0xffff) >> shift), minlength=nbins).to(torch.int32) for v in voxels])


def stacks(pipeline, dev):
    yield "synth", synth.stack_torch(SHAPE, np.uint16, dev)
    if pipeline == "bitswap1->lz4":
        yield "constant", torch.full(SHAPE, 1000, dtype=torch.int16, device=dev)
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        yield "noise", (torch.randint(0, 65536, SHAPE, dtype=torch.int32, device=dev, generator=g) - 32768).to(torch.int16)


def rows(kind):
    if kind != "synth":
        for shift in (0, 2):
            yield "%s stack whole shift %d" % (kind, shift), [(0, 0, 0)], SHAPE, shift
        return
    for shift in (0, 2, 6):
        yield "whole stack shift %d" % shift, [(0, 0, 0)], SHAPE, shift
    per = SHAPE[1] // 64 - 1
    for k in (4, 16, 64):
        yield "K=%d 16x64x64 same frames" % k, [(24, (97 * i % per) * 64 + 5, (61 * i % per) * 64 + 3) for i in range(k)], (16, 64, 64), 2
        yield "K=%d 16x64x64 disjoint z" % k, [(16 * (i % 4), (97 * i % per) * 64 + 5, (61 * i % per) * 64 + 3) for i in range(k)], (16, 64, 64), 2


def run(pipeline, dev, stream, table):
    sp = stream.cuda_stream
    for kind, vol in stacks(pipeline, dev):
        cap = sqeazy_amd.max_compressed_length(pipeline, SHAPE, np.uint16)
        blob = torch.empty(cap, dtype=torch.uint8, device=dev)
        rc, n = sqeazy_amd.encode_device(pipeline, vol.data_ptr(), SHAPE, np.uint16, blob.data_ptr(), cap, stream=sp)
        assert rc == 0
        del vol
        fb = SHAPE[1] * SHAPE[2] * 2
        full = torch.empty(SHAPE, dtype=torch.int16, device=dev)        # the voxels every column is held to (quantiser: not the stack's)
        rc = sqeazy_amd.decode_frames_device(blob.data_ptr(), n, 0, SHAPE[0], full.data_ptr(), SHAPE[0] * fb, np.uint16, stream=sp)
        assert rc == 0
        torch.cuda.synchronize()
        for name, origins, extent, shift in rows(kind):
            count = len(origins)
            extents = [extent] * count
            nbins = sqeazy_amd.histogram_bins(np.uint16, shift)
            want = counted([full[tuple(slice(a, a + e) for a, e in zip(o, extent))] for o in origins], shift, nbins).cpu().numpy()
            scratch = torch.empty((count,) + tuple(extent), dtype=torch.int16, device=dev)      # (the baseline's own: the new call needs none)
            hists = torch.empty((count, nbins), dtype=torch.int32, device=dev)
            sptrs = [scratch[i].data_ptr() for i in range(count)]
            hptrs = [hists[i].data_ptr() for i in range(count)]
            got = {}

            def base():
                rc = sqeazy_amd.decode_boxes_device(blob.data_ptr(), n, origins, sptrs, extents, None, np.uint16, stream=sp)
                assert rc == 0
                got["base"] = got["again"] = counted(scratch, shift, nbins)

            def hist(merge, key):
                sqeazy_amd.set_option("histogram_boxes_merge", merge)
                try:
                    rc = sqeazy_amd.histogram_boxes_device(blob.data_ptr(), n, origins, extents, shift, hptrs, np.uint16, stream=sp)
                finally:
                    sqeazy_amd.set_option("histogram_boxes_merge", DEFAULT_MERGE)
                assert rc == 0
                got[key] = hists

            fns = {"base": base, "again": base, "none": lambda: hist(0, "none"), "runs": lambda: hist(1, "runs"), "pieces": lambda: hist(2, "pieces")}
            columns = tuple(fns)
            for c in columns:                                       # warm-up, and every column's histograms against the full decode's
                scratch.fill_(0)
                hists.fill_(0x5A5A5A5A)
                fns[c]()
                torch.cuda.synchronize()
                assert np.array_equal(got[c].cpu().numpy(), want), (pipeline, name, c)
            ms = {c: [] for c in columns}
            for _ in range(K):
                for c in columns:
                    ms[c].append(round(timed(fns[c], stream), 3))
            ms["hist"] = ms[MERGES[DEFAULT_MERGE]]
            gain = [round(x / s, 3) for s, x in zip(ms["hist"], ms["base"])]
            spread = [round(x / s, 3) for s, x in zip(ms["again"], ms["base"])]
            runs = [round(x / s, 3) for s, x in zip(ms["runs"], ms["none"])]
            pieces = [round(x / s, 3) for s, x in zip(ms["pieces"], ms["none"])]
            bar = max(max(spread), 1 / min(spread))
            row = {"pipeline": pipeline, "row": name, "boxes": count, "extent": list(extent), "shift": shift, "nbins": nbins, "stack": list(SHAPE), "blob_bytes": n,
                   "ms": ms, "min_max": {c: [min(ms[c]), max(ms[c])] for c in columns}, "base_over_hist": gain, "base_over_again": spread, "none_over_runs": runs, "none_over_pieces": pieces, "default_merge": MERGES[DEFAULT_MERGE],
                   "baseline_scratch_bytes": int(scratch.numel()) * 2}
            row["hist_faster_every_pair_by_more_than_the_spread"] = bool(min(gain) > bar)
            row["hist_slower_every_pair_by_more_than_the_spread"] = bool(max(gain) < 1 / bar)
            for c in MERGES:
                row[c + "_kernel_ms"] = profiled(fns[c])
            row["base_kernel_ms"] = profiled(base)
            print(json.dumps(row), flush=True)
            verdict = "faster" if row["hist_faster_every_pair_by_more_than_the_spread"] else "slower" if row["hist_slower_every_pair_by_more_than_the_spread"] else "level"
            kern = {k: v[0] for k, v in row[MERGES[DEFAULT_MERGE] + "_kernel_ms"].items() if k in FINALS}
            for c in MERGES:
                kern.update({c + ":" + k: v[0] for k, v in row[c + "_kernel_ms"].items() if k in FINALS[:2]})
            kern.update({k: v[0] for k, v in row["base_kernel_ms"].items() if k in FINALS})
            line = "%-25s %-32s" % (pipeline, name) + "".join("  %s %.3f - %.3f" % (c, min(ms[c]), max(ms[c])) for c in columns)
            line += "  base/hist %.3f - %.3f  base/again %.3f - %.3f  none/runs %.3f - %.3f  none/pieces %.3f - %.3f  %s  kernels %s  scratch %d" % (
                min(gain), max(gain), min(spread), max(spread), min(runs), max(runs), min(pieces), max(pieces), verdict,
                " ".join("%s %.3f" % kv for kv in sorted(kern.items())), row["baseline_scratch_bytes"])
            table.append(line)
            got.clear()
            del scratch, hists
            torch.cuda.empty_cache()
        del blob, full
        torch.cuda.empty_cache()


def main():
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    table = []
    for pipeline in PIPELINES:
        run(pipeline, dev, stream, table)
    print()
    for line in table:
        print(line)


if __name__ == "__main__":
    main()
