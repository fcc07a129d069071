"""a box read out of a tiled store against whole tiles and slice copies (GPU box):  python3 tools/batch_window_time.py [k] [config ...]

Device time per call sequence (hipEvents around it on its stream, so the host's gaps between launches count), k repetitions (default 5)
after a warm-up, the columns interleaved repetition by repetition inside one process.  `bitswap1->lz4`, u16, the tiles of the regular grid
(sqeazy_amd.tile_views) of a synth.stack_torch parent, written with SQYAMD_PipelineEncode_BatchStrided_*:
  a = 256 tiles of 16x128x128 of a 64x1024x1024 parent, b = 64 tiles of 16x512x512 of a 64x2048x2048 parent
Boxes per grid, half a tile off the grid in every dimension:
  quarter  -- a quarter of the parent per dimension, from half a tile in
  straddle -- the size of one tile, from one and a half tiles in: it cuts eight tiles
and `odd`, the quarter box one voxel further in: no row of a window begins on the 16-byte grid of its tile, so on one side or the other
every voxel moves on its own
Columns:
  whole+slice -- what a caller does without the window entry point: SQYAMD_Decode_Batch_* of the intersecting tiles, whole, into scratch,
                 then a slice copy per tile with torch into the box
  layer1      -- SQYAMD_Decode_BatchWindow_* with batch_window_fused = 0: every tile decoded dense into the workspace, one window copy
  window      -- .. as it comes: the inverse transposer stores only the windows' voxels
Every column's box is checked against the parent's.  Per row: min-max per column, the per-pair ratios whole+slice / window and layer1 /
window, the scratch a caller holds (whole tiles) against the box's bytes, and the per-kernel device times of one profiled `window` call.
One JSON line per row."""
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
COLUMNS = ("whole+slice", "layer1", "window")


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


def run(name, shape, tile, dev, stream):
    parent = synth.stack_torch(shape, np.uint16, dev)
    ptrs, shapes, strides = sqeazy_amd.tile_views(parent.data_ptr(), shape, tile, 2)
    n = len(ptrs)
    cap = (sqeazy_amd.max_compressed_length(PIPELINE, tile, np.uint16) + 255) & ~255
    store = torch.empty(cap * n, dtype=torch.uint8, device=dev)
    sp = stream.cuda_stream
    rc, offs, lens = sqeazy_amd.encode_batch_strided_device(PIPELINE, ptrs, shapes, strides, np.uint16, store.data_ptr(), cap, stream=sp)
    assert rc == 0
    torch.cuda.synchronize()
    tile_bytes = int(np.prod(tile)) * 2
    half = tuple(t // 2 for t in tile)
    grid = tuple(-(-d // t) for d, t in zip(shape, tile))
    boxes = {"quarter": (half, tuple(d // 4 for d in shape)), "straddle": (tuple(t + h for t, h in zip(tile, half)), tile),
             "odd": (tuple(h + 1 for h in half), tuple(d // 4 for d in shape))}
    for box_name, (origin, extent) in boxes.items():
        box = torch.empty(extent, dtype=torch.uint16, device=dev)
        idx, origins, vptrs, vshapes, vstrides = sqeazy_amd.box_windows(shape, tile, origin, extent, box.data_ptr(), None, 2)
        b_offs, b_lens = [offs[i] for i in idx], [lens[i] for i in idx]
        # where window i lies in its tile (src) and in the box (at): the tile's cell of the grid, its origin in the parent
        cells = [np.unravel_index(i, grid) for i in idx]
        src = [tuple(slice(o, o + e) for o, e in zip(org, vs)) for org, vs in zip(origins, vshapes)]
        at = [tuple(slice(int(c) * t + o - b, int(c) * t + o - b + e) for c, t, o, b, e in zip(cell, tile, org, origin, vs))
              for cell, org, vs in zip(cells, origins, vshapes)]

        def whole_slice():
            tiles = [torch.empty(tile, dtype=torch.uint16, device=dev) for _ in idx]
            rc, _ = sqeazy_amd.decode_batch_device(store.data_ptr(), b_offs, b_lens, [t.data_ptr() for t in tiles], [tile_bytes] * len(idx), np.uint16, stream=sp)
            assert rc == 0
            for a, s, t in zip(at, src, tiles):
                box[a] = t[s]

        def window():
            rc, _ = sqeazy_amd.decode_batch_window_device(store.data_ptr(), b_offs, b_lens, origins, vptrs, vshapes, vstrides, np.uint16, stream=sp)
            assert rc == 0

        def layer1():
            with sqeazy_amd.option("batch_window_fused", 0):
                window()

        fns = {"whole+slice": whole_slice, "layer1": layer1, "window": window}
        want = parent[tuple(slice(o, o + e) for o, e in zip(origin, extent))]
        for c in COLUMNS:                                   # warm-up, and every column's box against the parent's
            box.fill_(0)
            fns[c]()
            torch.cuda.synchronize()
            assert torch.equal(box, want), (name, box_name, c)
        ms = {c: [] for c in COLUMNS}
        for _ in range(K):
            for c in COLUMNS:
                ms[c].append(round(timed(fns[c], stream)[0], 3))
        row = {"config": name, "box": box_name, "origin": list(origin), "extent": list(extent), "pipeline": PIPELINE, "tiles_cut": len(idx), "tile": list(tile),
               "parent": list(shape), "ms": ms, "min_max": {c: [min(ms[c]), max(ms[c])] for c in COLUMNS},
               "whole+slice_over_window": [round(x / s, 2) for s, x in zip(ms["window"], ms["whole+slice"])],
               "layer1_over_window": [round(x / s, 2) for s, x in zip(ms["window"], ms["layer1"])],
               "scratch_bytes_whole_tiles": len(idx) * tile_bytes, "box_bytes": int(np.prod(extent)) * 2}
        row["window_not_slower_than_whole+slice_any_pair"] = all(s <= x for s, x in zip(ms["window"], ms["whole+slice"]))
        row["window_not_slower_than_layer1_any_pair"] = all(s <= x for s, x in zip(ms["window"], ms["layer1"]))
        row["window_kernel_ms"] = profiled(window)
        print(json.dumps(row), flush=True)
        del box
    del parent, store
    torch.cuda.empty_cache()


def main():
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    for name in WANT:
        run(name, CONFIGS[name][0], CONFIGS[name][1], dev, stream)


if __name__ == "__main__":
    main()
