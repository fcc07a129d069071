"""batch decode against the existing entry points (GPU box):  python3 tools/batch_decode_time.py [k] [config ...]

Device time per call (hipEvents around the call on its stream), k repetitions (default 5) after a warm-up call, the columns interleaved
repetition by repetition inside one process, u16 volumes from synth.stack_torch, the blobs made by ONE SQYAMD_PipelineEncode_Batch call
whose offsets and lengths are passed straight through:
  loop     -- SQYAMD_Decode_UI16_Device per blob, one after the other on one stream
  slabs    -- SQYAMD_Decode_Slabs_UI16_Device (the volumes share shape[1..]; the destinations lie back to back in one allocation)
  batch0   -- SQYAMD_Decode_Batch_UI16_Device with decode_batch_joint = 0 (every blob on its own inside the call)
  batch    -- .. as it comes
Configurations (those of tools/batch_encode_time.py): a = 64 x 16x512x512 bitswap1->lz4, b = 256 x 16x128x128 bitswap1->lz4,
c = 256 x 16x128x128 lz4, d = 8 x 64x1024x1024 bitswap1->lz4; the two BASELINE pipelines whose inverses behind the LZ4 decode are joint as
well: e = 256 x 16x128x128 and g = 64 x 16x512x512 diff3x3x1->bitswap1->lz4, f = 256 x 16x128x128 and h = 64 x 16x512x512
quantiser->bitswap1->lz4.  Every column's volumes are checked against the source (the lossy quantiser: against the `loop` column's).  One JSON
line per configuration, then the kernels of one profiled `batch` call (SQYAMD_Profile_Get) on a line of their own."""
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
           "d": ("bitswap1->lz4", (64, 1024, 1024), 8),
           "e": ("diff3x3x1->bitswap1->lz4", (16, 128, 128), 256), "f": ("quantiser->bitswap1->lz4", (16, 128, 128), 256),
           "g": ("diff3x3x1->bitswap1->lz4", (16, 512, 512), 64), "h": ("quantiser->bitswap1->lz4", (16, 512, 512), 64)}
WANT = sys.argv[2:] or sorted(CONFIGS)
COLUMNS = ("loop", "slabs", "batch0", "batch")


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def run(name, pipeline, shape, n, dev, stream):
    Z = shape[0]
    vol = torch.empty((Z * n,) + tuple(shape[1:]), dtype=torch.uint16, device=dev)
    for s in range(n):
        vol[Z * s:Z * (s + 1)] = synth.stack_torch(shape, np.uint16, dev, seed=synth.SEED + s)
    vb = vol[0:Z].numel() * 2
    cap = sqeazy_amd.max_compressed_length(pipeline, shape, np.uint16) + 13          # (no multiple of 16: the blobs are misaligned)
    enc = torch.empty(cap * n, dtype=torch.uint8, device=dev)
    rc, offs, lens = sqeazy_amd.encode_batch_device(pipeline, [vol.data_ptr() + i * vb for i in range(n)], [shape] * n, np.uint16, enc.data_ptr(), cap)
    assert rc == 0
    joined = torch.empty_like(vol)                                   # loop and slabs: one allocation
    apart = [torch.empty(vb // 2, dtype=torch.uint16, device=dev) for _ in range(n)]     # batch: one allocation per destination
    sp = stream.cuda_stream
    L = sqeazy_amd.lib()

    def loop():
        for i in range(n):
            assert L.SQYAMD_Decode_UI16_Device(enc.data_ptr() + offs[i], lens[i], joined.data_ptr() + i * vb, vb, sp) == 0

    def slabs():
        rc, _ = sqeazy_amd.decode_slabs_device(enc.data_ptr(), offs, lens, joined.data_ptr(), n * vb, np.uint16, stream=sp)
        assert rc == 0

    def batch():
        rc, _ = sqeazy_amd.decode_batch_device(enc.data_ptr(), offs, lens, [t.data_ptr() for t in apart], [vb] * n, np.uint16, stream=sp)
        assert rc == 0

    def batch0():
        with sqeazy_amd.option("decode_batch_joint", 0):
            batch()

    fns = {"loop": loop, "slabs": slabs, "batch0": batch0, "batch": batch}
    flat = vol.reshape(n, -1)
    lossy = "quantiser" in pipeline
    for c in COLUMNS:                                                   # warm-up, and every column's volumes against the source
        joined.fill_(0)
        for t in apart:
            t.fill_(0)
        fns[c]()
        torch.cuda.synchronize()
        got = joined.reshape(n, -1) if c in ("loop", "slabs") else torch.stack(apart)
        if lossy and c == "loop":
            flat = got.clone()                                          # (what the single call makes of every blob)
        assert torch.equal(got, flat), (name, c)
    ms = {c: [] for c in COLUMNS}
    for _ in range(K):
        for c in COLUMNS:
            ms[c].append(round(timed(fns[c], stream), 3))
    base = [min(ms["loop"][r], ms["slabs"][r]) for r in range(K)]
    row = {"config": name, "pipeline": pipeline, "blobs": n, "shape": list(shape), "volume_bytes": vb,
           "ms": ms, "min_max": {c: [min(ms[c]), max(ms[c])] for c in COLUMNS},
           "GB/s": {c: round(n * vb / min(ms[c]) / 1e6, 1) for c in COLUMNS},
           "batch_wins_every_pair": all(b < x for b, x in zip(ms["batch"], base)),
           "loop_over_batch": [round(x / b, 2) for b, x in zip(ms["batch"], ms["loop"])],
           "slabs_over_batch": [round(x / b, 2) for b, x in zip(ms["batch"], ms["slabs"])]}
    print(json.dumps(row), flush=True)
    sqeazy_amd.profile_reset()
    sqeazy_amd.profile_enable(True)
    try:
        batch()
    finally:
        sqeazy_amd.profile_enable(False)
    print(json.dumps({"config": name, "batch_kernels_ms_launches": {k: [round(v[0], 3), v[1]] for k, v in sqeazy_amd.profile_get().items()}}), flush=True)
    sqeazy_amd.profile_reset()
    del vol, enc, joined, apart
    torch.cuda.empty_cache()


def main():
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    for name in WANT:
        pipeline, shape, n = CONFIGS[name]
        run(name, pipeline, shape, n, dev, stream)


if __name__ == "__main__":
    main()
