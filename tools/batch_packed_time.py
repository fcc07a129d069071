"""the packed batch encode against what a caller did before it (GPU box):  python3 tools/batch_packed_time.py [k] [--parent-lib PATH] [config ...]

Device time for the whole sequence (hipEvents around it on its stream), k repetitions (default 5) after a warm-up, the columns interleaved
repetition by repetition inside one process (the method of tools/batch_encode_time.py), u16 volumes from synth.stack_torch, bitswap1->lz4:
  A  packed        -- SQYAMD_PipelineEncode_BatchPacked_UI16_Device, align 1
  B  slots+copies  -- SQYAMD_PipelineEncode_Batch_UI16_Device into slots of max_compressed_length, then one device copy per blob into a
                      packed buffer at the same offsets: what a caller does today
  C  parent slots  -- the slot call alone from the library named by --parent-lib (a build of the commit before the packed layout, loaded
                      beside the installed one): what the placement scan and the gather at computed places cost against the code before
Configurations: b = 256 x 16x128x128, a = 64 x 16x512x512 (the README's batch-encode row).  Every column's blobs are checked against A's.
One JSON line per row: the times, A <= B in every pair, A - C per pair beside C's own spread, the destination bytes a caller must hold
(total against nvolumes x max_compressed_length) and the per-kernel device times of one profiled packed call and one profiled slot call."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sqeazy_amd  # noqa: E402
from sqeazy_amd import synth  # noqa: E402

ARGS = sys.argv[1:]
PARENT = None
if "--parent-lib" in ARGS:
    at = ARGS.index("--parent-lib")
    PARENT = ARGS[at + 1]
    del ARGS[at:at + 2]
K = int(ARGS[0]) if ARGS else 5
PIPELINE = "bitswap1->lz4"
CONFIGS = {"a": ((16, 512, 512), 64), "b": ((16, 128, 128), 256)}
WANT = ARGS[1:] or ["b", "a"]


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
    got = {k: [round(v[0], 4), v[1]] for k, v in sorted(sqeazy_amd.profile_get().items())}
    sqeazy_amd.profile_reset()
    return got


def parent_slot_call(path):
    """SQYAMD_PipelineEncode_Batch_UI16_Device of another build of the library"""
    L = ctypes.CDLL(os.path.abspath(path))
    c_long_p = ctypes.POINTER(ctypes.c_long)
    fn = L.SQYAMD_PipelineEncode_Batch_UI16_Device
    fn.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), c_long_p, ctypes.c_uint, ctypes.c_int, ctypes.c_void_p, ctypes.c_long, c_long_p, c_long_p,
                   ctypes.c_int, ctypes.c_void_p]

    def call(srcs, shapes, d_dst, cap, stream):
        n = len(srcs)
        ptrs = (ctypes.c_void_p * n)(*srcs)
        flat = (ctypes.c_long * (n * len(shapes[0])))(*[x for s in shapes for x in s])
        offs, lens = (ctypes.c_long * n)(), (ctypes.c_long * n)()
        rc = fn(PIPELINE.encode(), ptrs, flat, len(shapes[0]), n, ctypes.c_void_p(d_dst), cap, offs, lens, 0, ctypes.c_void_p(stream))
        assert rc == 0
        return list(offs), list(lens)
    return call


def run(name, shape, n, dev, stream, parent):
    Z = shape[0]
    vol = torch.empty((Z * n,) + tuple(shape[1:]), dtype=torch.uint16, device=dev)
    for s in range(n):
        vol[Z * s:Z * (s + 1)] = synth.stack_torch(shape, np.uint16, dev, seed=synth.SEED + s)
    vb = vol[0:Z].numel() * 2
    longest = sqeazy_amd.max_compressed_length(PIPELINE, shape, np.uint16)
    cap = (longest + 255) & ~255
    slots = torch.empty(cap * n, dtype=torch.uint8, device=dev)
    slots_c = torch.empty(cap * n, dtype=torch.uint8, device=dev)
    packed_a = torch.empty(longest * n, dtype=torch.uint8, device=dev)   # (the capacity that needs no retry)
    packed_b = torch.empty(longest * n, dtype=torch.uint8, device=dev)
    srcs = [vol.data_ptr() + i * vb for i in range(n)]
    shapes = [shape] * n
    sp = stream.cuda_stream

    def col_a():
        rc, offs, lens, total = sqeazy_amd.encode_batch_packed_device(PIPELINE, srcs, shapes, None, np.uint16, packed_a.data_ptr(), packed_a.numel(), align=1, stream=sp)
        assert rc == 0
        return offs, lens, total

    def slot_call():
        rc, offs, lens = sqeazy_amd.encode_batch_device(PIPELINE, srcs, shapes, np.uint16, slots.data_ptr(), cap, stream=sp)
        assert rc == 0
        return offs, lens

    def col_b():
        offs, lens = slot_call()
        at = 0
        for o, ln in zip(offs, lens):
            packed_b[at:at + ln].copy_(slots[o:o + ln], non_blocking=True)
            at += ln
        return offs, lens, at

    def col_c():
        return parent(srcs, shapes, slots_c.data_ptr(), cap, sp)

    columns = {"A": col_a, "B": col_b}
    if parent:
        columns["C"] = col_c
    # warm-up, and every column's blobs against A's
    offs, lens, total = col_a()
    torch.cuda.synchronize()
    assert offs[0] == 0 and all(offs[i + 1] == offs[i] + lens[i] for i in range(n - 1)) and total == offs[-1] + lens[-1]
    _, lens_b, total_b = col_b()
    torch.cuda.synchronize()
    assert lens_b == lens and total_b == total and torch.equal(packed_a[:total], packed_b[:total]), name
    if parent:
        offs_c, lens_c = col_c()
        torch.cuda.synchronize()
        assert lens_c == lens and all(torch.equal(slots_c[o:o + ln], packed_a[p:p + ln]) for o, p, ln in zip(offs_c, offs, lens)), name
    ms = {c: [] for c in columns}
    for _ in range(K):
        for c in columns:
            ms[c].append(round(timed(columns[c], stream)[0], 3))
    row = {"config": name, "pipeline": PIPELINE, "volumes": n, "shape": list(shape), "volume_bytes": vb, "ms": ms,
           "A_not_slower_than_B_any_pair": all(x <= y for x, y in zip(ms["A"], ms["B"])),
           "B_minus_A_ms": [round(y - x, 3) for x, y in zip(ms["A"], ms["B"])],
           "destination_bytes": {"packed_total": total, "slots": n * longest, "raw": n * vb}}
    if parent:
        row["A_minus_C_ms"] = [round(x - y, 3) for x, y in zip(ms["A"], ms["C"])]
        row["C_spread_ms"] = round(max(ms["C"]) - min(ms["C"]), 3)
        row["A_slower_than_C_by_more_than_C_spread"] = max(row["A_minus_C_ms"]) > row["C_spread_ms"]
    row["packed_kernel_ms"] = profiled(col_a)
    row["slot_kernel_ms"] = profiled(slot_call)
    print(json.dumps(row), flush=True)
    del vol, slots, slots_c, packed_a, packed_b
    torch.cuda.empty_cache()


def main():
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    parent = parent_slot_call(PARENT) if PARENT else None
    for name in WANT:
        shape, n = CONFIGS[name]
        run(name, shape, n, dev, stream, parent)


if __name__ == "__main__":
    main()
