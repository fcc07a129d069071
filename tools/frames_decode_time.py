"""frame-range decode against the full decode (GPU box):  python3 tools/frames_decode_time.py [reps]

Per-kernel device times (SQYAMD_Profile_*) and the wall time of one call, averaged over `reps` calls after a warm-up call: the full
decode (SQYAMD_Decode_*_Device) and SQYAMD_Decode_Frames_*_Device of 1, 16 and 128 frames of the bench stack (1024x1024x512 u16
bitswap1->lz4), and one frame of the C4 (1024^3 u8 frame_shuffle->lz4) and C5 slab (2048x2048x256 u16 quantiser->bitswap1->lz4) configs.
Every range is checked against the full decode's slice.  One JSON line per row."""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sqeazy_amd  # noqa: E402
from sqeazy_amd import synth  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
CONFIGS = [("bench", "bitswap1->lz4", (512, 1024, 1024), np.uint16, [(256, 1), (248, 16), (192, 128), (0, 1), (511, 1)]),
           ("C4", "frame_shuffle->lz4", (1024, 1024, 1024), np.uint8, [(512, 1)]),
           ("C5_slab", "quantiser->bitswap1->lz4", (256, 2048, 2048), np.uint16, [(128, 1)])]


def timed(fn):
    fn()
    torch.cuda.synchronize()
    sqeazy_amd.profile_reset()
    sqeazy_amd.profile_enable(True)
    t0 = time.perf_counter()
    for _ in range(REPS):
        assert fn() == 0
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / REPS
    sqeazy_amd.profile_enable(False)
    kernels = {k: round(v[0] / REPS, 4) for k, v in sqeazy_amd.profile_get().items()}
    return wall, kernels


def main():
    dev = torch.device("cuda", 0)
    for name, pipeline, shape, dtype, ranges in CONFIGS:
        vol = synth.stack_torch(shape, dtype, dev)
        cap = sqeazy_amd.max_compressed_length(pipeline, shape, dtype)
        enc = torch.empty(cap, dtype=torch.uint8, device=dev)
        rc, n = sqeazy_amd.encode_device(pipeline, vol.data_ptr(), shape, dtype, enc.data_ptr(), cap)
        assert rc == 0
        del vol
        nb = int(np.prod(shape)) * np.dtype(dtype).itemsize
        fb = nb // shape[0]
        full = torch.empty(nb, dtype=torch.uint8, device=dev)
        sfx = "UI16" if dtype == np.uint16 else "UI8"
        dec = getattr(sqeazy_amd.lib(), "SQYAMD_Decode_%s_Device" % sfx)
        wall, kernels = timed(lambda: dec(ctypes.c_void_p(enc.data_ptr()), n, ctypes.c_void_p(full.data_ptr()), nb, None))
        base = sum(kernels.values())
        print(json.dumps({"config": name, "range": "full", "wall_ms": round(wall, 3), "device_ms": round(base, 4), "kernels": kernels}), flush=True)
        for z0, nz in ranges:
            part = torch.empty(nz * fb, dtype=torch.uint8, device=dev)
            for subset in (1, 0):
                with sqeazy_amd.option("decode_frames_subset", subset):
                    wall, kernels = timed(lambda: sqeazy_amd.decode_frames_device(enc.data_ptr(), n, z0, nz, part.data_ptr(), nz * fb, dtype))
                assert torch.equal(part, full[z0 * fb:(z0 + nz) * fb]), (name, z0, nz)
                dms = sum(kernels.values())
                print(json.dumps({"config": name, "range": [z0, nz], "subset": subset, "wall_ms": round(wall, 3), "device_ms": round(dms, 4),
                                  "device_speedup": round(base / dms, 1) if dms else None, "kernels": kernels}), flush=True)
            del part
        del enc, full
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
