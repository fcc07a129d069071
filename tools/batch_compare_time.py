"""a box of a tiled store compared with resident voxels, against decode + tensor reductions (GPU box):
    python3 tools/batch_compare_time.py [k] [config[:box,box] ...]      (b:quarter -- the quarter box of grid b alone)

Device time per call sequence (hipEvents around it on its stream, so the host's gaps between launches count), k repetitions (default 5)
after a warm-up, the columns interleaved repetition by repetition inside one process.  `bitswap1->lz4`, u16, the tiles of the regular grid
(sqeazy_amd.tile_views) of a synth.stack_torch parent, written with SQYAMD_PipelineEncode_BatchStrided_*:
  a = 256 tiles of 16x128x128 of a 64x1024x1024 parent, b = 64 tiles of 16x512x512 of a 64x2048x2048 parent
Boxes per grid, half a tile off the grid in every dimension (tools/batch_window_time.py's):
  quarter  -- a quarter of the parent per dimension, from half a tile in
  straddle -- the size of one tile, from one and a half tiles in: it cuts eight tiles
The resident voxels are the parent's box with every 1009th voxel changed, in a dense buffer of the box's shape.
Columns:
  decode+torch -- what a caller does without the compare entry point: SQYAMD_Decode_BatchWindow_* of the same windows into a scratch box,
                  then per tile the torch reductions that give the same eight fields, gathered on the device and read back ONCE
  decode+torch_box -- .. with ONE set of reductions over the whole box: less than the call gives (no per-tile rows), the baseline's floor
  layer1       -- SQYAMD_Compare_BatchWindow_* with batch_compare_fused = 0: every tile decoded dense into the workspace, one compare launch
  compare      -- .. as it comes: the inverse transposer compares the windows' voxels
Every column's statistics are checked against numpy on the parent's box.  Per row: min-max per column, the per-pair ratios decode+torch /
compare, decode+torch_box / compare and layer1 / compare, and the per-kernel device times of one profiled `compare` call.  One JSON line
per row."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sqeazy_amd  # noqa: E402
from sqeazy_amd import synth  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 5
PIPELINE = "bitswap1->lz4"
CONFIGS = {"a": ((64, 1024, 1024), (16, 128, 128)), "b": ((64, 2048, 2048), (16, 512, 512))}
WANT = sys.argv[2:] or sorted(CONFIGS)
COLUMNS = ("decode+torch", "decode+torch_box", "layer1", "compare")


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    got = fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b), got


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


def wide(t):
    """16-bit voxels as int64 (the sums of squares need it)"""
    return t.view(torch.int16).to(torch.int64) & 0xffff


def fields(a, b):
    """the seven device-side fields of a against b, one tensor of int64"""
    d = (a - b).abs()
    return torch.stack([torch.count_nonzero(d), d.sum(), (d * d).sum(), d.max(), b.sum(), b.min(), b.max()])


def fields_numpy(a, b):
    a, b = a.astype(np.int64).reshape(-1), b.astype(np.int64).reshape(-1)
    d = np.abs(a - b)
    return [int(a.size), int(np.count_nonzero(d)), int(d.sum()), int((d * d).sum()), int(d.max()), int(b.sum()), int(b.min()), int(b.max())]


def run(name, shape, tile, dev, stream, boxes_wanted):
    parent = synth.stack_torch(shape, np.uint16, dev)
    ptrs, shapes, strides = sqeazy_amd.tile_views(parent.data_ptr(), shape, tile, 2)
    n = len(ptrs)
    cap = (sqeazy_amd.max_compressed_length(PIPELINE, tile, np.uint16) + 255) & ~255
    store = torch.empty(cap * n, dtype=torch.uint8, device=dev)
    sp = stream.cuda_stream
    rc, offs, lens = sqeazy_amd.encode_batch_strided_device(PIPELINE, ptrs, shapes, strides, np.uint16, store.data_ptr(), cap, stream=sp)
    assert rc == 0
    torch.cuda.synchronize()
    half = tuple(t // 2 for t in tile)
    grid = tuple(-(-d // t) for d, t in zip(shape, tile))
    boxes = {"quarter": (half, tuple(d // 4 for d in shape)), "straddle": (tuple(t + h for t, h in zip(tile, half)), tile)}
    for box_name, (origin, extent) in boxes.items():
        if boxes_wanted and box_name not in boxes_wanted:
            continue
        where = tuple(slice(o, o + e) for o, e in zip(origin, extent))
        decoded = parent[where].cpu().numpy()
        resident = decoded.copy()
        resident.reshape(-1)[::1009] ^= 0x0123
        ref = torch.from_numpy(resident).to(dev)                    # the resident voxels: a dense box
        box = torch.empty(extent, dtype=torch.uint16, device=dev)   # the baseline's scratch
        idx, origins, vptrs, vshapes, vstrides = sqeazy_amd.box_windows(shape, tile, origin, extent, box.data_ptr(), None, 2)
        _, _, rptrs, _, _ = sqeazy_amd.box_windows(shape, tile, origin, extent, ref.data_ptr(), None, 2)
        b_offs, b_lens = [offs[i] for i in idx], [lens[i] for i in idx]
        cells = [np.unravel_index(i, grid) for i in idx]
        at = [tuple(slice(int(c) * t + o - b, int(c) * t + o - b + e) for c, t, o, b, e in zip(cell, tile, org, origin, vs))
              for cell, org, vs in zip(cells, origins, vshapes)]
        want = [fields_numpy(decoded[a], resident[a]) for a in at]
        want_box = fields_numpy(decoded, resident)

        def decode():
            rc, _ = sqeazy_amd.decode_batch_window_device(store.data_ptr(), b_offs, b_lens, origins, vptrs, vshapes, vstrides, np.uint16, stream=sp)
            assert rc == 0

        def decode_torch():
            decode()
            A, B = wide(box), wide(ref)
            got = torch.stack([fields(A[a], B[a]) for a in at]).cpu().numpy()
            return [[int(np.prod(vs))] + [int(x) for x in row] for vs, row in zip(vshapes, got)]

        def decode_torch_box():
            decode()
            got = fields(wide(box), wide(ref)).cpu().numpy()
            return [int(np.prod(extent))] + [int(x) for x in got]

        def compare():
            rc, stats = sqeazy_amd.compare_batch_window_device(store.data_ptr(), b_offs, b_lens, origins, rptrs, vshapes, vstrides, np.uint16, stream=sp)
            assert rc == 0
            return [[int(x) for x in row] for row in stats]

        def layer1():
            with sqeazy_amd.option("batch_compare_fused", 0):
                return compare()

        fns = {"decode+torch": decode_torch, "decode+torch_box": decode_torch_box, "layer1": layer1, "compare": compare}
        for c in COLUMNS:                                   # warm-up, and every column's statistics against numpy's
            got = fns[c]()
            torch.cuda.synchronize()
            assert got == (want_box if c == "decode+torch_box" else want), (name, box_name, c)
        ms = {c: [] for c in COLUMNS}
        for _ in range(K):
            for c in COLUMNS:
                ms[c].append(round(timed(fns[c], stream)[0], 3))
        ratio = lambda c: [round(x / s, 2) for s, x in zip(ms["compare"], ms[c])]
        row = {"config": name, "box": box_name, "origin": list(origin), "extent": list(extent), "pipeline": PIPELINE, "tiles_cut": len(idx), "tile": list(tile),
               "parent": list(shape), "ms": ms, "min_max": {c: [min(ms[c]), max(ms[c])] for c in COLUMNS}, "decode+torch_over_compare": ratio("decode+torch"),
               "decode+torch_box_over_compare": ratio("decode+torch_box"), "layer1_over_compare": ratio("layer1"),
               "workgroups_per_record_max": max(-(-int(np.prod(tile)) // 32768), 1), "box_bytes": int(np.prod(extent)) * 2}
        row["compare_kernel_ms"] = profiled(compare)
        row["layer1_kernel_ms"] = profiled(layer1)
        print(json.dumps(row), flush=True)
        del box, ref
    del parent, store
    torch.cuda.empty_cache()


def main():
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    for want in WANT:
        name, _, boxes = want.partition(":")
        run(name, CONFIGS[name][0], CONFIGS[name][1], dev, stream, boxes.split(",") if boxes else None)


if __name__ == "__main__":
    main()
