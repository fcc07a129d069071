"""a box written into a tiled store against decode, slice copies and encode (GPU box):  python3 tools/batch_update_time.py [k] [config ...]

Device time per call sequence (hipEvents around it on its stream, so the host's gaps between launches count), k repetitions (default 7)
after a warm-up, the columns interleaved repetition by repetition inside one process.  `bitswap1->lz4`, u16, the tiles of the regular grid
(sqeazy_amd.tile_views) of a synth.stack_torch parent, written with SQYAMD_PipelineEncode_BatchStrided_*; tools/batch_window_time.py's
geometries:
  a = 256 tiles of 16x128x128 of a 64x1024x1024 parent, b = 64 tiles of 16x512x512 of a 64x2048x2048 parent
Boxes per grid, half a tile off the grid in every dimension:
  quarter  -- a quarter of the parent per dimension, from half a tile in (a: 16x256x256 over 18 tiles, b: 16x512x512 over 8 tiles)
  straddle -- the size of one tile, from one and a half tiles in: it cuts eight tiles (a only)
The box's new voxels are another synthetic stack.  Columns:
  three-step -- what a caller does without the update entry point: SQYAMD_Decode_Batch_* of the intersecting tiles, whole, into scratch,
                a slice copy per tile with torch out of the box, SQYAMD_PipelineEncode_Batch_* of the scratch tiles
  layer1     -- SQYAMD_Update_BatchWindow_* with batch_update_fused = 0: every tile decoded dense into the workspace, one paste, the encode
  update     -- .. as it comes: the LZ4 output straight into the places, the windows patched into the bit planes
Every column's blobs are checked against the three-step column's, byte for byte.  Per row: min-max per column, the per-pair ratios
three-step / update and layer1 / update, the scratch a caller holds (whole tiles), and the per-kernel device times of one profiled
`update` call.  One JSON line per row."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sqeazy_amd  # noqa: E402
from sqeazy_amd import synth  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 7
PIPELINE = "bitswap1->lz4"
CONFIGS = {"a": ((64, 1024, 1024), (16, 128, 128), ("quarter", "straddle")), "b": ((64, 2048, 2048), (16, 512, 512), ("quarter",))}
WANT = sys.argv[2:] or sorted(CONFIGS)
COLUMNS = ("three-step", "layer1", "update")


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


def run(name, shape, tile, box_names, dev, stream):
    parent = synth.stack_torch(shape, np.uint16, dev)
    ptrs, shapes, strides = sqeazy_amd.tile_views(parent.data_ptr(), shape, tile, 2)
    n = len(ptrs)
    cap = (sqeazy_amd.max_compressed_length(PIPELINE, tile, np.uint16) + 255) & ~255
    store = torch.empty(cap * n, dtype=torch.uint8, device=dev)
    sp = stream.cuda_stream
    rc, offs, lens = sqeazy_amd.encode_batch_strided_device(PIPELINE, ptrs, shapes, strides, np.uint16, store.data_ptr(), cap, stream=sp)
    assert rc == 0
    torch.cuda.synchronize()
    del parent
    tile_bytes = int(np.prod(tile)) * 2
    half = tuple(t // 2 for t in tile)
    grid = tuple(-(-d // t) for d, t in zip(shape, tile))
    boxes = {"quarter": (half, tuple(d // 4 for d in shape)), "straddle": (tuple(t + h for t, h in zip(tile, half)), tile)}
    for box_name in box_names:
        origin, extent = boxes[box_name]
        box = synth.stack_torch(extent, np.uint16, dev)
        idx, origins, vptrs, vshapes, vstrides = sqeazy_amd.box_windows(shape, tile, origin, extent, box.data_ptr(), None, 2)
        m = len(idx)
        b_offs, b_lens = [offs[i] for i in idx], [lens[i] for i in idx]
        # where window i lies in its tile (dst) and in the box (at): the tile's cell of the grid, its origin in the parent
        cells = [np.unravel_index(i, grid) for i in idx]
        dst = [tuple(slice(o, o + e) for o, e in zip(org, vs)) for org, vs in zip(origins, vshapes)]
        at = [tuple(slice(int(c) * t + o - b, int(c) * t + o - b + e) for c, t, o, b, e in zip(cell, tile, org, origin, vs))
              for cell, org, vs in zip(cells, origins, vshapes)]
        fresh = {c: torch.zeros(cap * m, dtype=torch.uint8, device=dev) for c in COLUMNS}
        tables = {}

        def three_step():
            tiles = [torch.empty(tile, dtype=torch.uint16, device=dev) for _ in idx]
            rc, _ = sqeazy_amd.decode_batch_device(store.data_ptr(), b_offs, b_lens, [t.data_ptr() for t in tiles], [tile_bytes] * m, np.uint16, stream=sp)
            assert rc == 0
            for a, d, t in zip(at, dst, tiles):
                t[d] = box[a]
            rc, o, l = sqeazy_amd.encode_batch_device(PIPELINE, [t.data_ptr() for t in tiles], [tile] * m, np.uint16, fresh["three-step"].data_ptr(), cap, stream=sp)
            assert rc == 0
            tables["three-step"] = (o, l)

        def update(column="update"):
            rc, o, l = sqeazy_amd.update_batch_window_device(PIPELINE, store.data_ptr(), b_offs, b_lens, origins, vptrs, vshapes, vstrides, np.uint16,
                                                             fresh[column].data_ptr(), cap, stream=sp)
            assert rc == 0
            tables[column] = (o, l)

        def layer1():
            with sqeazy_amd.option("batch_update_fused", 0):
                update("layer1")

        fns = {"three-step": three_step, "layer1": layer1, "update": update}
        for c in COLUMNS:                                   # warm-up, and every column's blobs against the three-step column's
            fns[c]()
            torch.cuda.synchronize()
            assert tables[c] == tables["three-step"], (name, box_name, c)
            for o, l in zip(*tables[c]):
                assert torch.equal(fresh[c][o:o + l], fresh["three-step"][o:o + l]), (name, box_name, c)
        ms = {c: [] for c in COLUMNS}
        for _ in range(K):
            for c in COLUMNS:
                ms[c].append(round(timed(fns[c], stream)[0], 3))
        row = {"config": name, "box": box_name, "origin": list(origin), "extent": list(extent), "pipeline": PIPELINE, "tiles_cut": m, "tile": list(tile),
               "parent": list(shape), "ms": ms, "min_max": {c: [min(ms[c]), max(ms[c])] for c in COLUMNS},
               "three-step_over_update": [round(x / s, 2) for s, x in zip(ms["update"], ms["three-step"])],
               "layer1_over_update": [round(x / s, 2) for s, x in zip(ms["update"], ms["layer1"])],
               "scratch_bytes_whole_tiles": m * tile_bytes, "box_bytes": int(np.prod(extent)) * 2}
        row["update_not_slower_than_three-step_any_pair"] = all(s <= x for s, x in zip(ms["update"], ms["three-step"]))
        row["update_not_slower_than_layer1_any_pair"] = all(s <= x for s, x in zip(ms["update"], ms["layer1"]))
        row["update_kernel_ms"] = profiled(update)
        row["layer1_kernel_ms"] = profiled(layer1)
        print(json.dumps(row), flush=True)
        del box, fresh
    del store
    torch.cuda.empty_cache()


def main():
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    for name in WANT:
        run(name, CONFIGS[name][0], CONFIGS[name][1], CONFIGS[name][2], dev, stream)


if __name__ == "__main__":
    main()
