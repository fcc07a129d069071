"""tiles cut in place against dense copies (GPU box):  python3 tools/batch_strided_time.py [k] [config ...]

Device time per call sequence (hipEvents around it on its stream, so the host's gaps between launches count), k repetitions (default 5)
after a warm-up, the columns interleaved repetition by repetition inside one process.  `bitswap1->lz4`, u16, the tiles of the regular grid
(sqeazy_amd.tile_views) of a synth.stack_torch parent:
  a = 256 tiles of 16x128x128 of a 64x1024x1024 parent, b = 64 tiles of 16x512x512 of a 64x2048x2048 parent
Columns, encode and decode each:
  copy+batch -- what a caller does without the strided entry points: a dense copy per tile with torch, then SQYAMD_PipelineEncode_Batch_*;
                SQYAMD_Decode_Batch_* into dense buffers, then a copy per tile into the parent
  pack       -- SQYAMD_*_BatchStrided_* with batch_strided_fused = 0: one pack / unpack launch per group, the Batch drivers in between
  strided    -- .. as it comes: the transposers gather from and scatter into the parent
Every column's blobs are checked against copy+batch's, every decode against the parent.  Per row: min-max per column, the per-pair ratios
copy+batch / strided and pack / strided, and the per-kernel device times of one profiled `strided` call.  One JSON line per row."""
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
COLUMNS = ("copy+batch", "pack", "strided")


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
    back = torch.empty_like(parent)
    ptrs, shapes, strides = sqeazy_amd.tile_views(parent.data_ptr(), shape, tile, 2)
    back_ptrs, _, _ = sqeazy_amd.tile_views(back.data_ptr(), shape, tile, 2)
    n = len(ptrs)
    origins = [(z, y, x) for z in range(0, shape[0], tile[0]) for y in range(0, shape[1], tile[1]) for x in range(0, shape[2], tile[2])]
    cut = [tuple(slice(o, o + t) for o, t in zip(org, tile)) for org in origins]
    cap = (sqeazy_amd.max_compressed_length(PIPELINE, tile, np.uint16) + 255) & ~255
    out = torch.empty(cap * n, dtype=torch.uint8, device=dev)
    sp = stream.cuda_stream
    tile_bytes = int(np.prod(tile)) * 2

    def enc_copy():
        tiles = [parent[c].contiguous() for c in cut]
        rc, offs, lens = sqeazy_amd.encode_batch_device(PIPELINE, [t.data_ptr() for t in tiles], shapes, np.uint16, out.data_ptr(), cap, stream=sp)
        assert rc == 0
        return offs, lens

    def enc_strided():
        rc, offs, lens = sqeazy_amd.encode_batch_strided_device(PIPELINE, ptrs, shapes, strides, np.uint16, out.data_ptr(), cap, stream=sp)
        assert rc == 0
        return offs, lens

    def enc_pack():
        with sqeazy_amd.option("batch_strided_fused", 0):
            return enc_strided()

    enc = {"copy+batch": enc_copy, "pack": enc_pack, "strided": enc_strided}
    ref = None
    for c in COLUMNS:                                       # warm-up, and every column's blobs against copy+batch's
        out.fill_(0)
        offs, lens = enc[c]()
        torch.cuda.synchronize()
        blobs = [out[o:o + ln].clone() for o, ln in zip(offs, lens)]
        if ref is None:
            ref = blobs
        assert all(torch.equal(x, y) for x, y in zip(blobs, ref)), (name, c)

    def dec_copy():
        tiles = [torch.empty(tile, dtype=torch.uint16, device=dev) for _ in range(n)]
        rc, _ = sqeazy_amd.decode_batch_device(out.data_ptr(), offs, lens, [t.data_ptr() for t in tiles], [tile_bytes] * n, np.uint16, stream=sp)
        assert rc == 0
        for c, t in zip(cut, tiles):
            back[c] = t

    def dec_strided():
        rc, _ = sqeazy_amd.decode_batch_strided_device(out.data_ptr(), offs, lens, back_ptrs, shapes, strides, np.uint16, stream=sp)
        assert rc == 0

    def dec_pack():
        with sqeazy_amd.option("batch_strided_fused", 0):
            dec_strided()

    dec = {"copy+batch": dec_copy, "pack": dec_pack, "strided": dec_strided}
    for c in COLUMNS:
        back.fill_(0)
        dec[c]()
        torch.cuda.synchronize()
        assert torch.equal(back, parent), (name, c)

    for way, fns in (("encode", enc), ("decode", dec)):
        ms = {c: [] for c in COLUMNS}
        for _ in range(K):
            for c in COLUMNS:
                ms[c].append(round(timed(fns[c], stream)[0], 3))
        row = {"config": name, "way": way, "pipeline": PIPELINE, "tiles": n, "tile": list(tile), "parent": list(shape), "ms": ms,
               "min_max": {c: [min(ms[c]), max(ms[c])] for c in COLUMNS},
               "GB/s": {c: round(n * tile_bytes / min(ms[c]) / 1e6, 1) for c in COLUMNS},
               "copy+batch_over_strided": [round(x / s, 2) for s, x in zip(ms["strided"], ms["copy+batch"])],
               "pack_over_strided": [round(x / s, 2) for s, x in zip(ms["strided"], ms["pack"])]}
        row["strided_not_slower_than_copy+batch_any_pair"] = all(s <= x for s, x in zip(ms["strided"], ms["copy+batch"]))
        row["strided_not_slower_than_pack_any_pair"] = all(s <= x for s, x in zip(ms["strided"], ms["pack"]))
        row["strided_kernel_ms"] = profiled(fns["strided"])
        print(json.dumps(row), flush=True)
    del parent, back, out
    torch.cuda.empty_cache()


def main():
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    for name in WANT:
        run(name, CONFIGS[name][0], CONFIGS[name][1], dev, stream)


if __name__ == "__main__":
    main()
