"""slab-set decode against a loop of single decodes (GPU box):  python3 tools/slabs_decode_time.py [k] [config ...]

Device time per call (hipEvents around the call on its stream), best of k calls after a warm-up call, for a volume encoded with
SQYAMD_PipelineEncode_Slabs_UI16_Device and decoded
  loop     -- SQYAMD_Decode_UI16_Device over the blobs, one after the other on one stream
  joint0   -- SQYAMD_Decode_Slabs_UI16_Device with decode_slabs_joint = 0 (every blob on its own inside the call)
  joint1   -- SQYAMD_Decode_Slabs_UI16_Device, inflight = 0 (the default grouping), 1, 2, 4, 8
Configurations: a = eight 2048x2048x256 bitswap1->lz4 slabs (north_star's volume, as tools/ns_volume.py makes it), b = four C3 slabs
(diff3x3x1->bitswap1->lz4), c = four C5 slabs (quantiser->bitswap1->lz4), d = 64 slabs of 16x512x512 bitswap1->lz4.  Every output is
checked against the loop's (and, for the lossless pipelines, against the source volume).  One JSON line per row."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sqeazy_amd  # noqa: E402
from sqeazy_amd import synth  # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 5
CONFIGS = {"a": ("bitswap1->lz4", (256, 2048, 2048), 8), "b": ("diff3x3x1->bitswap1->lz4", (256, 2048, 2048), 4),
           "c": ("quantiser->bitswap1->lz4", (256, 2048, 2048), 4), "d": ("bitswap1->lz4", (16, 512, 512), 64)}
WANT = sys.argv[2:] or sorted(CONFIGS)


def best_ms(fn, stream):
    fn()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(K):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        assert fn() == 0
        b.record(stream)
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def main():
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    dec = sqeazy_amd.lib().SQYAMD_Decode_UI16_Device
    for name in WANT:
        pipeline, slab, n = CONFIGS[name]
        Z = slab[0] * n
        shape = (Z,) + slab[1:]
        vol = torch.empty(shape, dtype=torch.uint16, device=dev)
        for s in range(n):
            vol[slab[0] * s:slab[0] * (s + 1)] = synth.stack_torch(slab, np.uint16, dev, z_offset=slab[0] * s, z_total=Z)
        cap = (sqeazy_amd.max_compressed_length(pipeline, slab, np.uint16) + 255) & ~255
        enc = torch.empty(cap * n, dtype=torch.uint8, device=dev)
        rc, offs, lens = sqeazy_amd.encode_slabs_device(pipeline, vol.data_ptr(), shape, np.uint16, n, enc.data_ptr(), cap, inflight=3)
        assert rc == 0
        nb = vol.numel() * 2
        sb = nb // n
        ref = torch.empty(nb, dtype=torch.uint8, device=dev)
        out = torch.empty(nb, dtype=torch.uint8, device=dev)

        def loop():
            rcs = [dec(ctypes.c_void_p(enc.data_ptr() + offs[i]), ctypes.c_long(lens[i]), ctypes.c_void_p(ref.data_ptr() + i * sb), ctypes.c_long(sb), sp)
                   for i in range(n)]
            return max(rcs)

        ms = best_ms(loop, stream)
        if "quantiser" not in pipeline:
            assert torch.equal(ref, vol.view(torch.uint8).reshape(-1)), name
        rows = [{"config": name, "pipeline": pipeline, "slabs": n, "slab": list(slab), "mode": "loop", "device_ms": round(ms, 3),
                 "GB/s": round(nb / ms / 1e6, 1)}]
        print(json.dumps(rows[-1]), flush=True)
        for joint, inflight in ((0, 0), (1, 0), (1, 1), (1, 2), (1, 4), (1, 8)):
            out.fill_(0)
            with sqeazy_amd.option("decode_slabs_joint", joint):
                ms = best_ms(lambda: sqeazy_amd.decode_slabs_device(enc.data_ptr(), offs, lens, out.data_ptr(), nb, np.uint16, inflight=inflight,
                                                                   stream=stream.cuda_stream)[0], stream)
            assert torch.equal(out, ref), (name, joint, inflight)
            rows.append({"config": name, "pipeline": pipeline, "slabs": n, "slab": list(slab), "mode": "joint%d" % joint, "inflight": inflight,
                         "device_ms": round(ms, 3), "GB/s": round(nb / ms / 1e6, 1), "vs_loop": round(rows[0]["device_ms"] / ms, 2)})
            print(json.dumps(rows[-1]), flush=True)
        del vol, enc, ref, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
