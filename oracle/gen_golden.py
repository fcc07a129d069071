#!/usr/bin/env python3
"""Generates tests/golden/: golden vectors that pin the oracle (and through it the HIP path) to the REAL thing.

Run in the build container (needs /root/reference -> oracle/_ref/libsqy_ref.so and the image's liblz4 1.9.3):
    python oracle/gen_golden.py

Sources of truth
  * LZ4 bytes      liblz4.so.1.9.3 driven with sqeazy's call sequence (oracle/ref_driver.cpp cites
                   encoders/lz4.hpp:103-113, lz4_utils.hpp:99-274)
  * bitswap1 u16   the reference's own SSE gather, sqeazy::detail::simd_segment_broadcast
                   (encoders/sse_utils.hpp:1365-1433), compiled in place from the reference tree
  * filter stages  diff3x3x1, rmestbkrd, rmbkrd_neighbor5x5x5, zcurve_reorder, raster_reorder, scalar bitswap1 and the histogram: the
                   reference's own templates compiled in place (oracle/ref_driver.cpp) -> tests/golden/ref_stages.json (--stages)
  * quantiser LUTs the reference's own sqeazy::quantiser<uint16_t, uint8_t> compiled in place (oracle/ref_driver.cpp, with the
                   string_parsers.hpp of oracle/ref_shim/) on the volumes of tests/quantiser_cases.py -> tests/golden/quantiser_luts.json
                   (--quantiser): digests of both tables
  * shuffles       frame_shuffle and tile_shuffle on whole units: the reference's own detail::frame_shuffle / detail::tile_shuffle compiled
                   in place (oracle/ref_driver.cpp, with the Boost.Accumulators stand-in of oracle/boost_standin/, which only their median
                   path names) -> tests/golden/ref_shuffles.json (--shuffles): output digests, decode_maps, decode digests
  * what the reference cannot produce here (needs Boost proper: the sqy header; the remainder / median path of the two shuffles, which
    oracle and product refuse) is NOT in this file's "reference" section; whole pipelines through frame_shuffle carry "oracle" hashes in
    golden.json as regression anchors, and the header is pinned by the reference's own KATs restated in tests/test_oracle_reference_kats.py.

Output
  tests/golden/golden.json     {case: {input: generator spec, stage: {sha256, bytes, source}}}
  tests/golden/*.bin           a few small raw input/expected pairs (data only)
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref, sqy_oracle as o   # noqa: E402
from sqeazy_amd import synth             # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bkrd_restate as R                                            # noqa: E402
import diff_seam_cases as D                                         # noqa: E402
from ref_stage_inputs import stage_input, stage_volume, stage_tile, case_id  # noqa: E402,F401  (the tests import them from here or there)
from ref_stage_inputs import shuffle_volume, shuffle_param, shuffle_whole, shuffle_case_id  # noqa: E402,F401

GOLD = os.path.join(ROOT, "tests", "golden")


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def gen_bytes(kind, n, seed):
    """byte streams; the same function is imported by the tests"""
    rng = np.random.default_rng(seed)
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    if kind == "ff":
        return np.full(n, 255, np.uint8)
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "2level":
        return rng.integers(0, 2, n, dtype=np.uint8)
    if kind == "8level":
        return rng.integers(0, 8, n, dtype=np.uint8)
    if kind == "ramp":
        return (np.arange(n) % 251).astype(np.uint8)
    if kind == "slowramp":
        return ((np.arange(n) // 7) % 256).astype(np.uint8)
    if kind == "sparse":
        s = np.zeros(n, np.uint8)
        k = n // 50
        if k:
            s[rng.integers(0, n, k)] = rng.integers(1, 255, k)
        return s
    if kind == "words":
        words = rng.integers(0, 256, (50, 12), dtype=np.uint8)
        return words[rng.integers(0, 50, n // 12 + 1)].reshape(-1)[:n]
    if kind == "period7":
        return np.tile(np.arange(7, dtype=np.uint8), n // 7 + 1)[:n]
    if kind == "farrep":                                   # repeats just inside the 64 KiB window, across block borders
        c = rng.integers(0, 256, n, dtype=np.uint8)
        for i in range(66000, n - 300, 66000):
            c[i:i + 300] = c[i - 65000:i - 65000 + 300]
        return c
    if kind == "rawmix":                                   # every other 256 KiB incompressible (stored raw), the rest zeros
        d = rng.integers(0, 256, n, dtype=np.uint8)
        for i in range(0, n, 2 * (256 << 10)):
            d[i:i + (256 << 10)] = 0
        return d
    if kind == "periodic":
        b = np.tile(rng.integers(0, 256, 7000, dtype=np.uint8), n // 7000 + 1)[:n].copy()
        b[::1531] ^= 1
        return b
    raise KeyError(kind)


def main():
    assert ref.available(), "oracle/_ref/libsqy_ref.so missing: run `make -C oracle` where /root/reference exists"
    assert ref.lz4_version() == 10903, "golden vectors are pinned to liblz4 1.9.3"
    os.makedirs(GOLD, exist_ok=True)
    G = {"_meta": {"liblz4": "1.9.3 (LZ4_versionNumber 10903)", "reference_pieces": "encoders/sse_utils.hpp simd_segment_broadcast",
                   "generator": "oracle/gen_golden.py"}, "lz4_block": [], "lz4_frames": [], "bitswap1_u16": [], "pipelines": []}

    # ---- LZ4 block level: LZ4_compress_fast_continue(fresh stream, cap n-1) ----
    kinds = ["zeros", "ff", "random", "2level", "8level", "ramp", "slowramp", "sparse", "words", "period7"]
    for kind in kinds:
        for n in (1, 12, 13, 14, 100, 1000, 10000, 65536, 70000, 262144):
            d = gen_bytes(kind, n, 1000 + n)
            r = ref.lz4_block(d)
            mine = o.lz4_block_compress(d)
            assert r == mine, ("oracle differs from liblz4", kind, n)
            G["lz4_block"].append({"kind": kind, "n": n, "seed": 1000 + n, "csize": 0 if r is None else len(r),
                                   "sha256": None if r is None else sha(r), "source": "liblz4-1.9.3"})

    # ---- frames, chunked layout: encode_parallel ----
    for kind in kinds:
        for n in (0, 5, 10000, 262144, 262145, 600000, 2 * 262144 + 10000):
            d = gen_bytes(kind, n, 2000 + n)
            if n == 0:
                continue
            r = ref.lz4_encode_parallel(d, nthreads=2)
            r4 = ref.lz4_encode_parallel(d, nthreads=4)
            assert np.array_equal(r, r4), "chunked layout must not depend on the thread count (>= 2)"
            mine = o.lz4_encode_chunked(d)
            assert np.array_equal(r, mine), ("oracle frames differ from liblz4", kind, n)
            G["lz4_frames"].append({"kind": kind, "n": n, "seed": 2000 + n, "bytes": int(r.size), "sha256": sha(r.tobytes()),
                                    "source": "liblz4-1.9.3 via sqeazy's encode_parallel call sequence"})
    # other block sizes (BD / HC bytes)
    for kb, bid in ((64, 4), (1024, 6)):
        d = gen_bytes("8level", 3 * (kb << 10) + 777, 77)
        r = ref.lz4_encode_parallel(d, chunk=kb << 10, block_id=bid, nthreads=2)
        cfg = o.Lz4Config("blocksize_kb=%d,framestep_kb=%d" % (kb, kb))
        mine = o.lz4_encode_chunked(d, cfg)
        assert np.array_equal(r, mine), kb
        G["lz4_frames"].append({"kind": "8level", "n": int(d.size), "seed": 77, "config": "blocksize_kb=%d,framestep_kb=%d" % (kb, kb), "bytes": int(r.size),
                                "sha256": sha(r.tobytes()), "source": "liblz4-1.9.3"})
    # ---- block-linked frames: encode_serial (nthreads == 1) and chunks of several blocks ----
    G["lz4_linked"] = []
    lkinds = ["zeros", "random", "2level", "8level", "ramp", "sparse", "words", "farrep", "rawmix", "periodic"]
    for kind in lkinds:
        for n in (300000, 2 * (1 << 20) + 12345):
            d = gen_bytes(kind, n, 3000 + n)
            for cfg, step, bid in (("", 256 << 10, 5), ("blocksize_kb=64", 256 << 10, 4), ("framestep_kb=1024", 1 << 20, 5),
                                   ("n_chunks_of_input=3", n // 3, 5), ("blocksize_kb=64,n_chunks_of_input=7", n // 7, 4)):
                c = o.Lz4Config(cfg)
                assert c.bytes_per_chunk(n) == min(step, n) and c.block_id == bid, (cfg, c.bytes_per_chunk(n), step)
                r1 = ref.lz4_encode_serial(d, framestep=c.bytes_per_chunk(n), block_id=bid)
                m1 = o.lz4_encode_serial(d, c)
                assert np.array_equal(r1, m1), ("oracle serial frame differs from liblz4", kind, n, cfg)
                r2 = ref.lz4_encode_parallel(d, chunk=c.bytes_per_chunk(n), block_id=bid, nthreads=2)
                m2 = o.lz4_encode_chunked(d, c)
                assert np.array_equal(r2, m2), ("oracle multi-block chunks differ from liblz4", kind, n, cfg)
                G["lz4_linked"].append({"kind": kind, "n": n, "seed": 3000 + n, "config": cfg,
                                        "serial_bytes": int(r1.size), "serial_sha256": sha(r1.tobytes()),
                                        "chunked_bytes": int(r2.size), "chunked_sha256": sha(r2.tobytes()),
                                        "source": "liblz4-1.9.3 via sqeazy's encode_serial / encode_parallel call sequences"})
    # LZ4F constants the reference's tests pin (tests/test_lz4_sandbox.cpp:387-430)
    G["_meta"]["LZ4F_compressBound_256k"] = int(ref.lz4f_compress_bound(262144))
    G["_meta"]["LZ4F_HEADER_SIZE_MAX"] = int(ref.lib().ref_lz4f_header_size_max())

    # ---- bitswap1 u16 through the reference's SSE kernel ----
    for name, arr in (("ramp128", np.arange(128, dtype=np.uint16)),
                      ("random_64k", np.random.default_rng(5).integers(0, 65536, 1 << 16, dtype=np.uint16)),
                      ("synth_16x64x64", synth.stack((16, 64, 64)).reshape(-1)),
                      ("lowbits_4096", np.random.default_rng(6).integers(0, 16, 4096, dtype=np.uint16))):
        r = ref.bitswap1_encode_u16(arr, nthreads=2)
        assert np.array_equal(r, o.bitswap1_encode(arr)), name
        G["bitswap1_u16"].append({"name": name, "len": int(arr.size), "sha256": sha(r.tobytes()), "source": "reference sse_utils.hpp"})

    # ---- whole pipelines: payload from liblz4 where the stage chain is reference-backed, oracle otherwise ----
    vols = {"synth_u16_32x64x64": synth.stack((32, 64, 64)), "synth_u16_24x100x52": synth.stack((24, 100, 52)),
            "synth_u8_48x64x96": synth.stack((48, 64, 96), np.uint8)}
    for vname, vol in vols.items():
        for pipe in ("bitswap1->lz4", "lz4", "diff3x3x1->bitswap1->lz4", "frame_shuffle->lz4", "quantiser->bitswap1->lz4"):
            if vol.dtype == np.uint8 and pipe.startswith(("quantiser", "diff")):
                continue
            blob = o.pipeline_encode(pipe, vol)
            entry = {"volume": vname, "pipeline": pipe, "bytes": len(blob), "sha256": sha(blob), "source": "oracle"}
            blob1 = o.pipeline_encode(pipe, vol, nthreads=1)
            entry["nthreads1_bytes"], entry["nthreads1_sha256"] = len(blob1), sha(blob1)
            if pipe in ("bitswap1->lz4", "lz4") and vol.dtype == np.uint16 and vol.size % 128 == 0:
                # fully reference-backed payload: reference SSE bitswap + liblz4 frames
                stream = ref.bitswap1_encode_u16(vol, 2).view(np.uint8) if pipe.startswith("bitswap1") else vol.reshape(-1).view(np.uint8)
                payload = ref.lz4_encode_parallel(stream, nthreads=2).tobytes()
                h = o.header_unpack(blob)
                assert blob[h["size"]:] == payload
                entry["payload_sha256"] = sha(payload)
                payload1 = ref.lz4_encode_serial(stream).tobytes()
                assert blob1[o.header_unpack(blob1)["size"]:] == payload1
                entry["nthreads1_payload_sha256"] = sha(payload1)
                entry["source"] = "payload: reference SSE bitswap + liblz4 1.9.3; header: oracle"
            G["pipelines"].append(entry)

    # ---- small raw fixtures (data only) ----
    d = gen_bytes("sparse", 10000, 42)
    d.tofile(os.path.join(GOLD, "sparse_10000.in.bin"))
    ref.lz4_encode_parallel(d, nthreads=2).tofile(os.path.join(GOLD, "sparse_10000.lz4frames.bin"))
    v = synth.stack((4, 16, 32))
    v.tofile(os.path.join(GOLD, "synth_u16_4x16x32.in.bin"))
    ref.bitswap1_encode_u16(v, 1).tofile(os.path.join(GOLD, "synth_u16_4x16x32.bitswap1.bin"))
    ref.lz4_encode_parallel(ref.bitswap1_encode_u16(v, 1).view(np.uint8), nthreads=2).tofile(
        os.path.join(GOLD, "synth_u16_4x16x32.bitswap1_lz4_payload.bin"))

    with open(os.path.join(GOLD, "golden.json"), "w") as f:
        json.dump(G, f, indent=1, sort_keys=True)
    print("wrote", os.path.join(GOLD, "golden.json"), "with", sum(len(v) for k, v in G.items() if k != "_meta"), "vectors")


def headline():
    """tests/golden/headline.json: payload digests of the BASELINE headline stacks (configs[0] 256^3 and configs[1] 1024x1024x512 uint16,
    'bitswap1->lz4') produced by the REFERENCE pieces themselves -- the reference's SSE bit-plane gather (encoders/sse_utils.hpp:1365-1433,
    compiled in place) followed by liblz4 1.9.3 frames through sqeazy's encode_parallel call sequence (encoders/lz4_utils.hpp:193-274) --
    plus the slab 0 of the 2048^3 north_star volume.  The GPU tests and bench.py compare the HIP path's payload with these digests, so
    the headline is pinned to the reference and not only to the restated oracle.  (The sqy header in front of the payload is the oracle's:
    the reference's header code needs Boost.)"""
    assert ref.available() and ref.lz4_version() == 10903
    H = {"_meta": {"generator": "oracle/gen_golden.py --headline", "bitswap1": "reference simd_segment_broadcast (sse_utils.hpp:1365-1433), 16 threads",
                   "lz4": "liblz4 1.9.3 (LZ4_versionNumber 10903) via encode_parallel (lz4_utils.hpp:193-274), 256 KiB chunks",
                   "stack": "sqeazy_amd.synth.stack(shape, uint16[, frames z_offset.. of z_total])"}, "stacks": []}
    cases = (("C1 256x256x256 u16", (256, 256, 256), 0, None), ("C2 1024x1024x512 u16", (512, 1024, 1024), 0, None),
             ("north_star slab 0 of 2048^3 u16 (2048x2048x256)", (256, 2048, 2048), 0, 2048))
    for name, shape, z0, ztot in cases:
        vol = synth.stack(shape, np.uint16) if ztot is None else None
        if vol is None:
            # frames [z0, z0 + Z) of a (ztot, Y, X) volume without building the whole volume
            Z, Y, X = shape
            per = Y * X
            noise = synth._noise(z0 * per, Z * per, synth.SEED).reshape(Z, Y, X)
            sh = synth._shell(z0, Z, ztot, Y, X)
            vol = (100 + (noise >> 2) + sh * 6000).astype(np.uint16)
        planes = ref.bitswap1_encode_u16(vol, 16)
        payload = ref.lz4_encode_parallel(planes.view(np.uint8), nthreads=8)
        mine = o.pipeline_encode("bitswap1->lz4", vol)
        h = o.header_unpack(mine)
        assert mine[h["size"]:] == payload.tobytes(), ("oracle payload differs from the reference pieces", name)
        H["stacks"].append({"name": name, "shape_zyx": list(shape), "z_offset": z0, "z_total": ztot or shape[0], "pipeline": "bitswap1->lz4",
                            "voxels_sha256": sha(vol.tobytes()), "payload_bytes": int(payload.size), "payload_sha256": sha(payload.tobytes()),
                            "blob_bytes": len(mine), "blob_sha256": sha(mine), "header_bytes": h["size"],
                            "source": "payload: reference SSE bitswap + liblz4 1.9.3; header: oracle"})
        print(name, payload.size, H["stacks"][-1]["payload_sha256"][:16], flush=True)
        del vol, planes, payload, mine
    with open(os.path.join(GOLD, "headline.json"), "w") as f:
        json.dump(H, f, indent=1, sort_keys=True)
    print("wrote", os.path.join(GOLD, "headline.json"))


def headline_serial():
    """adds to tests/golden/headline.json the digests of the same stacks in the layout every default caller of the reference gets
    (nthreads = 1: ONE block-linked frame, lz4_utils.hpp:99-173): reference SSE bit-plane gather + liblz4 1.9.3 LZ4F_compressUpdate
    sequence; asserts the oracle's serial payload equals it on the way"""
    assert ref.available() and ref.lz4_version() == 10903
    path = os.path.join(GOLD, "headline.json")
    with open(path) as f:
        H = json.load(f)
    H["_meta"]["lz4_serial"] = "liblz4 1.9.3 via encode_serial (lz4_utils.hpp:99-173): one block-linked frame, one LZ4F_compressUpdate per framestep"
    for st in H["stacks"]:
        shape, z0, ztot = tuple(st["shape_zyx"]), st["z_offset"], st["z_total"]
        if ztot == shape[0]:
            vol = synth.stack(shape, np.uint16)
        else:
            Z, Y, X = shape
            per = Y * X
            noise = synth._noise(z0 * per, Z * per, synth.SEED).reshape(Z, Y, X)
            sh = synth._shell(z0, Z, ztot, Y, X)
            vol = (100 + (noise >> 2) + sh * 6000).astype(np.uint16)
        assert sha(vol.tobytes()) == st["voxels_sha256"]
        planes = ref.bitswap1_encode_u16(vol, 16).view(np.uint8)
        cfg = o.Lz4Config("")
        payload = ref.lz4_encode_serial(planes, framestep=cfg.bytes_per_chunk(planes.size))
        mine = o.pipeline_encode("bitswap1->lz4", vol, nthreads=1)
        h = o.header_unpack(mine)
        assert mine[h["size"]:] == payload.tobytes(), ("oracle serial payload differs from the reference pieces", st["name"])
        st["serial"] = {"payload_bytes": int(payload.size), "payload_sha256": sha(payload.tobytes()), "blob_bytes": len(mine), "blob_sha256": sha(mine),
                        "header_bytes": h["size"]}
        print(st["name"], "serial", payload.size, st["serial"]["payload_sha256"][:16], flush=True)
        del vol, planes, payload, mine
    with open(path, "w") as f:
        json.dump(H, f, indent=1, sort_keys=True)
    print("wrote", path)


def _slab_volume(shape, z0, ztot, frames_per_step=16):
    """frames [z0, z0 + Z) of a (ztot, Y, X) synthetic uint16 volume, built a few frames at a time (1 Gi voxels at once would need ~25 GiB)"""
    Z, Y, X = shape
    per = Y * X
    vol = np.empty(shape, dtype=np.uint16)
    for a in range(0, Z, frames_per_step):
        nz = min(frames_per_step, Z - a)
        noise = synth._noise((z0 + a) * per, nz * per, synth.SEED).reshape(nz, Y, X)
        sh = synth._shell(z0 + a, nz, ztot, Y, X)
        vol[a:a + nz] = (100 + (noise >> 2) + sh * 6000).astype(np.uint16)
    return vol


def headline_slabs():
    """tests/golden/headline_slabs.json (round 6): every z-slab a rank of the sharded BASELINE volumes encodes, at
    FULL plane size -- the shell sweeps through z, slabs 3 and 4 carry data (12-bit shell voxels over whole frames) that slab 0 never sees.
      * north_star 2048^3 u16 'bitswap1->lz4': all eight 2048 x 2048 x 256 slabs; payload = the REFERENCE pieces (SSE bit-plane gather +
        liblz4 1.9.3 through encode_parallel), the oracle's blob asserted equal on the way;
      * configs[2] 2048^3 'diff3x3x1->bitswap1->lz4', slabs 3 and 4, and configs[4] 2048 x 2048 x 1024 'quantiser->bitswap1->lz4', slabs 1
        and 2 of its four (the two around the shell's centre): the ORACLE's blob (those stages of the reference need Boost: unbuildable here).
    One slab at a time; resumes from what the file already holds."""
    assert ref.available() and ref.lz4_version() == 10903
    path = os.path.join(GOLD, "headline_slabs.json")
    H = {"_meta": {"generator": "oracle/gen_golden.py --headline-slabs",
                   "north_star": "payload: reference simd_segment_broadcast (sse_utils.hpp:1365-1433) + liblz4 1.9.3 via encode_parallel (lz4_utils.hpp:193-274); header: oracle",
                   "c3_c5": "blob: oracle (oracle/sqy_oracle.c / sqy_oracle_float.c); the reference's diff / quantiser stages include Boost and cannot be built here",
                   "stack": "frames [z_offset, z_offset + 256) of sqeazy_amd.synth's (z_total, 2048, 2048) uint16 volume"}, "slabs": []}
    if os.path.exists(path):
        with open(path) as f:
            H = json.load(f)
    have = {(e["pipeline"], e["z_total"], e["z_offset"]) for e in H["slabs"]}
    shape = (256, 2048, 2048)
    todo = [("bitswap1->lz4", 2048, s) for s in range(8)] + [("diff3x3x1->bitswap1->lz4", 2048, s) for s in (3, 4)] + \
           [("quantiser->bitswap1->lz4", 1024, s) for s in (1, 2)]
    for pipeline, ztot, slab in todo:
        z0 = 256 * slab
        if (pipeline, ztot, z0) in have:
            continue
        vol = _slab_volume(shape, z0, ztot)
        mine = o.pipeline_encode(pipeline, vol)
        h = o.header_unpack(mine)
        e = {"name": "%s slab %d of %d (2048x2048x256 of %dx2048x2048)" % (pipeline, slab, ztot // 256, ztot), "pipeline": pipeline, "slab": slab,
             "shape_zyx": list(shape), "z_offset": z0, "z_total": ztot, "voxels_sha256": sha(vol.tobytes()), "blob_bytes": len(mine),
             "blob_sha256": sha(mine), "header_bytes": h["size"], "payload_bytes": len(mine) - h["size"], "payload_sha256": sha(mine[h["size"]:])}
        if pipeline == "bitswap1->lz4":
            planes = ref.bitswap1_encode_u16(vol, 8)
            payload = ref.lz4_encode_parallel(planes.view(np.uint8), nthreads=8)
            assert mine[h["size"]:] == payload.tobytes(), ("oracle payload differs from the reference pieces", e["name"])
            e["source"] = "payload: reference SSE bitswap + liblz4 1.9.3 (oracle blob asserted equal); header: oracle"
            del planes, payload
        else:
            e["source"] = "oracle"
        H["slabs"].append(e)
        print(e["name"], e["payload_bytes"], e["payload_sha256"][:16], flush=True)
        with open(path, "w") as f:
            json.dump(H, f, indent=1, sort_keys=True)
        del vol, mine
    print("wrote", path)


def accel():
    """tests/golden/accel.json: liblz4 1.9.3 with an acceleration above 1 -- sqeazy's lz4(accel=-k), a negative LZ4F compression level
    (encoders/lz4.hpp:103-113) -- block level, the chunked layout and the serial block-linked layout; asserts oracle == liblz4 on the way"""
    assert ref.available() and ref.lz4_version() == 10903
    A = {"_meta": {"generator": "oracle/gen_golden.py --accel", "liblz4": "1.9.3 (LZ4_versionNumber 10903)",
                   "mapping": "sqeazy accel = LZ4F compressionLevel; level -k -> LZ4_compress_fast_continue acceleration k + 1 (lz4frame.c), capped at 65537"},
         "cases": []}
    for kind in ["zeros", "random", "2level", "8level", "ramp", "slowramp", "sparse", "words", "period7", "farrep", "rawmix", "periodic"]:
        for n in (10000, 262144, 600000):
            d = gen_bytes(kind, n, 4000 + n)
            for level in (-1, -3, -64, -70000):
                a = o.lz4_acceleration(level)
                rb = ref.lz4_block(d, accel=a)
                assert rb == o.lz4_block_compress(d, acceleration=a), ("block", kind, n, level)
                cfg = o.Lz4Config("accel=%d" % level)
                rc = ref.lz4_encode_parallel(d, accel=level, nthreads=2)
                assert np.array_equal(rc, o.lz4_encode_chunked(d, cfg)), ("chunked", kind, n, level)
                rs = ref.lz4_encode_serial(d, framestep=cfg.bytes_per_chunk(n), accel=level)
                assert np.array_equal(rs, o.lz4_encode_serial(d, cfg)), ("serial", kind, n, level)
                A["cases"].append({"kind": kind, "n": n, "seed": 4000 + n, "accel": level, "acceleration": a,
                                   "block_csize": 0 if rb is None else len(rb), "block_sha256": None if rb is None else sha(rb),
                                   "chunked_bytes": int(rc.size), "chunked_sha256": sha(rc.tobytes()),
                                   "serial_bytes": int(rs.size), "serial_sha256": sha(rs.tobytes()), "source": "liblz4-1.9.3"})
    with open(os.path.join(GOLD, "accel.json"), "w") as f:
        json.dump(A, f, indent=1, sort_keys=True)
    print("wrote", os.path.join(GOLD, "accel.json"), "with", len(A["cases"]), "cases")


def lz4_planted():
    """tests/golden/lz4_planted.json: the planted streams of tests/lz4_planted.py -- per case its length and sha256 and the size and sha256 of the
    oracle's block (no bytes); asserts oracle == liblz4 on the way where the reference driver is built"""
    import lz4_planted as P
    L = {"_meta": {"generator": "oracle/gen_golden.py --lz4-planted", "block": "sqy_oracle.lz4_block_compress(data, cap=lz4_planted.block_cap(n))",
                   "liblz4": "1.9.3 (LZ4_versionNumber 10903)" if ref.available() else "not compared"}, "cases": {}}
    for c in P.cases():
        d = c["data"]
        blk = o.lz4_block_compress(d, cap=P.block_cap(len(d)))
        if ref.available() and len(d) >= 13:
            assert blk == ref.lz4_block(np.frombuffer(d, np.uint8), cap=P.block_cap(len(d))), c["name"]
        L["cases"][c["name"]] = {"n": len(d), "sha256": sha(d), "block_bytes": len(blk), "block_sha256": sha(blk)}
    with open(os.path.join(GOLD, "lz4_planted.json"), "w") as f:
        json.dump(L, f, indent=1, sort_keys=True)
    print("wrote", os.path.join(GOLD, "lz4_planted.json"), "with", len(L["cases"]), "cases")


def lz4_linked_planted():
    """tests/golden/lz4_linked_planted.json: the streams of tests/lz4_linked_planted.py -- per case its length and sha256 and the size and sha256
    of the oracle's frame under the case's configuration (no bytes); asserts oracle == liblz4 on the way where the reference driver is built"""
    import lz4_linked_planted as LP
    L = {"_meta": {"generator": "oracle/gen_golden.py --lz4-linked-planted", "frame": "lz4_linked_planted.oracle_frame(sqy_oracle, case)",
                   "liblz4": "1.9.3 (LZ4_versionNumber 10903)" if ref.available() else "not compared"}, "cases": {}}
    for c in LP.cases():
        fr = LP.oracle_frame(o, c)
        if ref.available():
            assert fr == LP.liblz4_frame(ref, o, c), c["name"]
        L["cases"][c["name"]] = {"n": len(c["data"]), "sha256": sha(c["data"]), "frame_bytes": len(fr), "frame_sha256": sha(fr)}
    with open(os.path.join(GOLD, "lz4_linked_planted.json"), "w") as f:
        json.dump(L, f, indent=1, sort_keys=True)
    print("wrote", os.path.join(GOLD, "lz4_linked_planted.json"), "with", len(L["cases"]), "cases")


# ------------------------------------------------------------------------------------------------------------------------------------
# Filter stages against the reference's own templates (oracle/ref_driver.cpp): ONE table of cases, tests/golden/ref_stages.json
# ------------------------------------------------------------------------------------------------------------------------------------
def _rows(stage, dtypes, shapes, kinds, seed0, params=None, **flags):
    out = []
    for dt in dtypes:
        for shape in shapes:
            for kind in kinds:
                r = {"stage": stage, "dtype": dt, "shape": list(shape), "kind": kind, "seed": seed0 + len(out), "params": dict(params or {})}
                r.update(flags)
                out.append(r)
    return out


# why a row is `undefined` (the reference is not run on it) or `serial_only` (run with one thread only); rows carry the key
REASONS = {
    "race": "scalar_bitplane_reorder_encode (bitplane_reorder_scalar.hpp:46-70) updates an output word shared by 8 * sizeof(T) consecutive inputs "
            "with a read-modify-write from whichever threads hold them: only the one-thread run is defined",
    "sse_fault": "the SSE branch (bitswap_scheme_impl.hpp:106-120) loads with _mm_load_si128 (sse_utils.hpp:1194, :1273): it faults on this address",
    "neighbour_oob": "count_neighbors_if (background_scheme_utils.hpp:248-268) reads neighbours behind the end of the volume",
}
RACE, SSE_FAULT, NB_OOB = "race", "sse_fault", "neighbour_oob"

# zcurve_reorder: the shapes and tiles of tests/test_gpu_new_stages.py::test_zcurve_reorder
ZCURVE = [((8, 8, 8), 2), ((8, 8, 8), 4), ((8, 8, 8), 8), ((8, 16, 8), 2), ((7, 16, 7), 2), ((5, 3, 9), 2), ((64, 128, 256), 16), ((33, 70, 129), 4),
          ((128, 128, 128), 128), ((12, 12, 12), 8)]
# raster_reorder: those of tests/test_gpu_parity.py::test_raster_reorder (tile None: 16 / sizeof(T))
RASTER = [((32, 64, 96), None), ((16, 32, 48), None), ((33, 64, 97), 5), ((7, 13, 21), 5), ((32, 64, 96), 4), ((33, 66, 99), 4)]
# rmbkrd_neighbor5x5x5: extents from {1, 2, 4, 5, 6, 9}
NB_SHAPES = [(9, 9, 5), (9, 6, 5), (9, 5, 6), (6, 6, 5), (9, 9, 6), (6, 9, 5), (9, 6, 6), (9, 9, 9), (6, 6, 6), (5, 6, 9), (4, 9, 9), (2, 6, 6), (6, 5, 9),
             (1, 9, 9), (9, 9, 4), (9, 4, 9), (9, 5, 5), (9, 9, 1), (9, 2, 9), (1, 1, 1), (2, 5, 6), (9, 9, 2)]
# .. and volumes of more than one tile of the product's kernel: the smallest with centres at z = 64..67; x and y tiles with centres on both
# sides of the seam; a third chunk that lies wholly behind z_end = 68; three z chunks, three x tiles, two y tiles, z_end = 132 in the last chunk
NB_SEAM_SHAPES = [(72, 6, 70), (70, 20, 68), (129, 18, 70), (136, 18, 134)]


def neighbor5_reads_in_bounds(shape):
    """True when every neighbour of every voxel flatten_to_neighborhood_scheme::encode visits lies inside the volume
    (offsets of neighborhood_utils.hpp:199-238 for cube_neighborhood<5> on the shape as given, rows of X - 3 voxels)"""
    Z, Y, X = shape
    last = -1
    for z in range(2, X - 2):
        for y in range(2, Y - 2):
            off = z * Y * X + y * X + 2
            if off < Z * Y * X:
                last = max(last, off + X - 4)
    return last < 0 or last + 2 * Y * X + 2 * X + 2 < Z * Y * X


def stage_table():
    T = []
    # ---- diff3x3x1 ----
    dshapes = [(2, 3, 5), (5, 3, 2), (3, 3, 3), (2, 3, 2), (1, 8, 8), (8, 1, 8), (8, 8, 1), (4, 6, 10), (10, 6, 4), (40, 5, 4), (9, 10, 12)]
    T += _rows("diff3x3x1", ["uint16", "uint8", "char"], dshapes, ["random"], 100)
    T += _rows("diff3x3x1", ["uint16"], [(130, 16, 512), (3, 700, 128)], ["random"], 200)
    T += _rows("diff3x3x1", ["uint16", "uint8"], [(4, 6, 10), (9, 10, 12)], ["max", "ramp"], 300)
    T += _rows("diff3x3x1", ["uint8", "char"], [(3, 4, 127), (127, 4, 3), (3, 4, 128), (128, 4, 3), (3, 128, 4)], ["random"], 400)
    T += _rows("diff3x3x1", ["char"], [(4, 6, 10), (9, 10, 12), (10, 6, 4)], ["pm128"], 500)
    # ---- rmestbkrd ----
    T += _rows("rmestbkrd", ["uint16", "uint8"], [(2, 4, 4), (3, 5, 7), (16, 32, 32)], ["zero", "max", "two_level", "gamma", "equal_faces"], 600)
    T += _rows("rmestbkrd", ["uint16", "uint8"], [(1, 4, 4)], ["gamma"], 700)
    # ---- rmbkrd_neighbor5x5x5 ----
    nb = []
    for i, shape in enumerate(NB_SHAPES):
        for dt in ("uint16", "uint8"):
            # values 0..79: a level of 18 (16) puts 28 (25) of the 124 neighbours below it on average, a level of 36 puts 56: most walked
            # voxels stay under the cuts of fraction 0.25 (31) and 0.5 (62), some do not.  Levels 0 and 1 and fraction 1 keep every
            # walked voxel at or above the level, the largest level skips every voxel.  near_wrap: 4 in 13 lie below the wrapped level
            # (38 neighbours, cut 62); a level that saturated instead of wrapping would skip every voxel.
            combos = [(18, 0.25), (1, 1.0), (0, 0.0), (36, 0.5)] if i % 2 == 0 else \
                     [(40, 1.0), (1, 0.25), (65535 if dt == "uint16" else 255, 0.0), (16, 0.25)]
            if not R.neighbor5_defined(shape) or not neighbor5_reads_in_bounds(shape):
                combos = combos[:1]                             # refused by the product, or undefined in the reference: the shape says it all
            for t, f in combos:
                nb += _rows("rmbkrd_neighbor5x5x5", [dt], [shape], ["low80"], 800 + len(nb), {"threshold": t, "fraction": f})
            if len(combos) > 1:
                nb += _rows("rmbkrd_neighbor5x5x5", [dt], [shape], ["near_wrap"], 800 + len(nb), {"threshold": 70000, "fraction": 0.5})
    for r in nb:
        if not neighbor5_reads_in_bounds(r["shape"]):
            r["undefined"] = NB_OOB
    T += nb
    # ---- zcurve_reorder / raster_reorder ----
    for k, (shape, ts) in enumerate(ZCURVE):
        T += _rows("zcurve_reorder", ["uint16", "uint8"], [shape], ["random"], 2000 + 2 * k, {"tile_size": ts})
    for k, (shape, ts) in enumerate(RASTER):
        T += _rows("raster_reorder", ["uint16", "uint8"], [shape], ["random"], 2100 + 2 * k, {"tile_size": ts})
    # ---- bitswap1: (1, 1, len), source `offset_bytes` behind an aligned address ----
    for dt in ("uint16", "uint8"):
        for n in (1, 7, 8, 9, 127, 128, 129, 4096 + 13):
            for off in (0, 2):
                r = _rows("bitswap1", [dt], [(1, 1, n)], ["random"], 2200 + len(T), {"offset_bytes": off})[0]
                sse = dt == "uint16" and n % 128 == 0
                if sse and off % 16:
                    r["undefined"] = SSE_FAULT
                elif not sse:
                    r["serial_only"] = RACE
                T.append(r)
    # ---- histogram statistics (hist_impl.hpp) ----
    T += _rows("histogram", ["uint16", "uint8"], [(1, 1, 5000), (1, 1, 1), (3, 5, 7)], ["gamma", "two_level", "zero", "max", "random"], 2400)
    # ---- rmbkrd_neighbor5x5x5 across the seams of the product's tiles (64 x 16 columns, chunks of 64 frames); appended, so that the rows
    # above keep their ids.  The reference reads in bounds on all four (asserted), so none is `undefined` ----
    seams = []
    for shape in NB_SEAM_SHAPES:
        assert R.neighbor5_defined(shape) and neighbor5_reads_in_bounds(shape), shape
        for dt in ("uint16", "uint8"):
            for t, f in ((36, 0.5), (18, 0.25)):
                seams += _rows("rmbkrd_neighbor5x5x5", [dt], [shape], ["low80"], 5000 + len(seams), {"threshold": t, "fraction": f})
            seams += _rows("rmbkrd_neighbor5x5x5", [dt], [shape], ["planted"], 5000 + len(seams), {"threshold": 100, "fraction": 0.0})
    T += seams
    # ---- rmestbkrd on faces that leave the histogram kernel's window, and a face of more than 32768 voxels ----
    T += _rows("rmestbkrd", ["uint16"], [(4, 40, 520), (3, 130, 260)], ["spread"], 5100)
    # ---- diff3x3x1 at the seams of the product's kernels: the encode cases of tests/diff_seam_cases.py, same seeds ----
    T += _rows("diff3x3x1", ["uint16"], D.ENCODE_SHAPES, ["random"], D.ENCODE_SEED0)
    T += _rows("diff3x3x1", ["uint16"], D.MAX_SHAPES, ["max"], D.MAX_SEED0)
    for i, r in enumerate(T):
        r["id"] = case_id(r, i)
    return T


def oracle_stage(row, vol):
    """the ORACLE's output of a case: (bytes, extra numbers); raises ValueError where the oracle refuses the case"""
    st, p = row["stage"], row["params"]
    if st == "diff3x3x1":
        return o.diff3x3x1_encode(vol, char=row["dtype"] == "char").tobytes(), {}
    if st == "rmestbkrd":
        if vol.shape[0] < 2:
            raise ValueError("rmestbkrd: fewer than two frames")
        sup = [float(R.support(h)) for h in R.face_histograms(vol, 1 << 30)]
        return R.rmestbkrd(vol, 1 << 30).tobytes(), {"supports": sup, "threshold": R.rmestbkrd_threshold(vol, 1 << 30)}
    if st == "rmbkrd_neighbor5x5x5":
        if not R.neighbor5_defined(vol.shape):
            raise ValueError("rmbkrd_neighbor5x5x5: undefined shape")
        t, f = R.neighbor5_params("threshold=%d,fraction=%r" % (p["threshold"], p["fraction"]), vol.dtype)
        return R.neighbor5(vol, t, f).tobytes(), {}
    if st == "zcurve_reorder":
        return o.zcurve_reorder(vol, p["tile_size"]).tobytes(), {}
    if st == "raster_reorder":
        return o.raster_reorder(vol, stage_tile(row)).tobytes(), {}
    if st == "bitswap1":
        return o.bitswap1_encode(vol).tobytes(), {}
    if st == "histogram":
        bins = o.histogram(vol)
        return bins.tobytes(), {"support": float(R.support(bins))}
    raise KeyError(st)


def reference_stage(row, vol, nthreads=1):
    """the REFERENCE's output of a case through oracle/_ref: (bytes, extra numbers); raises ref.Refused"""
    st, p = row["stage"], row["params"]
    if st == "diff3x3x1":
        return ref.diff3x3x1(vol, char=row["dtype"] == "char", nthreads=nthreads).tobytes(), {}
    if st == "rmestbkrd":
        out, sup, thr = ref.rmestbkrd(vol, nthreads)
        return out.tobytes(), {"supports": [float(s) for s in sup], "threshold": thr}
    if st == "rmbkrd_neighbor5x5x5":
        return ref.rmbkrd_neighbor5x5x5(vol, p["threshold"], p["fraction"], nthreads).tobytes(), {}
    if st == "zcurve_reorder":
        return ref.zcurve_reorder(vol, p["tile_size"], nthreads=nthreads).tobytes(), {}
    if st == "raster_reorder":
        return ref.raster_reorder(vol, stage_tile(row), nthreads=nthreads).tobytes(), {}
    if st == "bitswap1":
        return ref.bitswap1(vol, nthreads=nthreads, offset_bytes=p["offset_bytes"]).tobytes(), {}
    if st == "histogram":
        bins, stats = ref.hist_stats(vol)
        return bins.tobytes(), {"support": stats["support"]}          # the oracle restates the bins and the support, nothing else
    raise KeyError(st)


def reference_stage_decode(row, enc):
    """the reference's decode of its own output, one thread (diff3x3x1's decode reads planes other threads still write)"""
    st, p = row["stage"], row["params"]
    if st == "diff3x3x1":
        return ref.diff3x3x1(enc, char=row["dtype"] == "char", decode=True)
    if st == "zcurve_reorder":
        return ref.zcurve_reorder(enc, p["tile_size"], decode=True)
    if st == "raster_reorder":
        return ref.raster_reorder(enc, stage_tile(row), decode=True)
    if st == "bitswap1":
        return ref.bitswap1(enc, decode=True).reshape(enc.shape)
    return None


def stage_refused(row, vol):
    """a case the product refuses: the oracle raises on it (the reference reads out of bounds or throws there; it is not run)"""
    try:
        oracle_stage(row, vol)
        return False
    except ValueError:
        return True


def _lean(c):
    """a case as the golden file holds it: without its id and empty params (ref_stage_inputs.load_cases puts them back)"""
    return {k: v for k, v in c.items() if k != "id" and not (k == "params" and not v)}


def stages():
    """tests/golden/ref_stages.json: for every row of stage_table() the byte count and sha256 of what the REFERENCE's own templates give
    (oracle/ref_driver.cpp), the estimator's supports and threshold as numbers; nthreads 1 and 3 asserted equal unless the row is
    `serial_only`; rows marked `undefined` and refused rows are not run"""
    assert ref.stages_available(), "oracle/_ref/libsqy_ref.so missing or stale: run `make -C oracle` where the reference tree exists"
    rows = stage_table()
    l2 = int(ref.cache_l2_bytes())
    G = {"_meta": {"generator": "oracle/gen_golden.py --stages", "source": "the reference's utility headers compiled in place (oracle/ref_driver.cpp)",
                   "host_l2_bytes": l2, "reasons": REASONS, "inputs": "tests/ref_stage_inputs.py: stage_input(kind, dtype, shape, seed)",
                   "refused": "the PRODUCT's policy (shapes on which the reference reads out of bounds or throws), taken from the oracle, which "
                              "restates that policy; the reference is not run on these rows and says nothing about them",
                   "histogram": "sha256 of the uint32 bins, and calc_support(0.99f); no other statistic is pinned"}, "cases": []}
    for row in rows:
        vol = stage_volume(row)
        e = dict(row)
        e["input_sha256"] = sha(vol.tobytes())[:12]
        if stage_refused(row, vol):
            e["refused"] = True
        elif "undefined" not in row:
            if row["stage"] == "rmestbkrd":
                assert vol.shape[1] * vol.shape[2] <= l2, "the face portion must not depend on this machine's L2"
            out, extra = reference_stage(row, vol, 1)
            if "serial_only" not in row:
                out3, extra3 = reference_stage(row, vol, 3)
                assert out == out3 and extra == extra3, ("the reference disagrees with itself across thread counts", row["id"])
            arr = np.frombuffer(out, vol.dtype)
            back = reference_stage_decode(row, arr.reshape(vol.shape)) if row["stage"] != "histogram" else None
            if back is not None:
                assert np.array_equal(back.reshape(vol.shape), vol), ("the reference's decode does not restore the input", row["id"])
            e.update(extra)
            e["bytes"], e["sha256"] = len(out), sha(out)
        G["cases"].append(e)
    with open(os.path.join(GOLD, "ref_stages.json"), "w") as f:                   # compact, one case per line
        f.write('{"_meta": %s,\n"cases": [\n%s\n]}\n' % (json.dumps(G["_meta"], sort_keys=True),
                                                        ",\n".join(json.dumps(_lean(c), sort_keys=True, separators=(",", ":")) for c in G["cases"])))
    n = len(G["cases"])
    print("wrote ref_stages.json:", n, "cases,", sum("refused" in c for c in G["cases"]), "refused,", sum("undefined" in c for c in G["cases"]), "undefined")


# the volumes of tests/quantiser_cases.py the sanitized driver runs the reference's quantiser on: the Lloyd walk where binary32 rounds, and
# the walk's first case with the top bin occupied
QUANTISER_SAN_CASES = ("uniform_60000", "levels_257_top")


def dump_stage_cases(path):
    """inputs of every case the reference is run on, for tests/sanitize/ref_stages_san.cpp: cases.txt (one line per case:
    id stage dtype z y x p0 p1 offset_bytes serial_only) and <index>.bin, the rows of shuffle_table() behind those of stage_table();
    quantiser.txt (name, voxels) and quantiser_<index>.bin"""
    os.makedirs(path, exist_ok=True)
    lines = []
    for row in stage_table():
        vol = stage_volume(row)
        if "undefined" in row or stage_refused(row, vol):
            continue
        p = row["params"]
        p0 = stage_tile(row) if "reorder" in row["stage"] else p.get("threshold", 0)
        k = len(lines)
        vol.tofile(os.path.join(path, "%d.bin" % k))
        lines.append("%s %s %s %d %d %d %d %r %d %d" % (row["id"], row["stage"], row["dtype"], vol.shape[0], vol.shape[1], vol.shape[2], p0,
                                                       float(p.get("fraction", 0.0)), p.get("offset_bytes", 0), int("serial_only" in row)))
    # the rows of ref_shuffles.json, refused ones included: p0 is frame_chunk_size / tile_size, p1 is 1.0 where the driver has to answer
    # "remainder" without running the reference
    for row in shuffle_table():
        vol = shuffle_volume(row)
        vol.tofile(os.path.join(path, "%d.bin" % len(lines)))
        lines.append("%s %s %s %d %d %d %d %r 0 0" % (row["id"], row["stage"], row["dtype"], vol.shape[0], vol.shape[1], vol.shape[2], shuffle_param(row),
                                                      0.0 if shuffle_whole(row) else 1.0))
    with open(os.path.join(path, "cases.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    import quantiser_cases as Q
    with open(os.path.join(path, "quantiser.txt"), "w") as f:
        for k, name in enumerate(QUANTISER_SAN_CASES):
            Q.volume(name).tofile(os.path.join(path, "quantiser_%d.bin" % k))
            f.write("%s %d\n" % (name, Q.volume(name).size))
    return len(lines)


# the weightings the quantiser goldens hold besides the default: one of each of the reference's two functors
QUANTISER_WEIGHTERS = ("power_of_1_2", "offset_power_of_2_3")


def quantiser_weightings(name):
    """the weightings a case of tests/quantiser_cases.py is recorded and compared with"""
    import quantiser_cases as Q
    return ("none",) + (QUANTISER_WEIGHTERS if Q.FAMILY[name] in (Q.ROUNDING, Q.BOUNDARY) else ())


def quantiser():
    """tests/golden/quantiser_luts.json: for every volume of tests/quantiser_cases.py the sha256 of the encode LUT (65536 bytes) and of the
    decode LUT (256 little-endian uint16) that the REFERENCE's quantiser builds from the voxels, one and three threads asserted equal, the
    oracle asserted equal on the way.  Digests only."""
    import quantiser_cases as Q
    assert ref.quantiser_available(), "oracle/_ref/libsqy_ref.so missing or stale: run `make -C oracle` where the reference tree exists"
    out = {"_meta": {"generator": "oracle/gen_golden.py --quantiser", "cases": "tests/quantiser_cases.py: volume(name)",
                     "source": "sqeazy::quantiser<uint16_t, uint8_t>::setup_com compiled in place (oracle/ref_driver.cpp)",
                     "digests": "[sha256 of lut_encode, uint8[65536]; sha256 of lut_decode, uint16[256] little-endian] per weighting_function"},
           "cases": {}}
    for name in Q.NAMES:
        vol = Q.volume(name)
        e = {"voxels_sha256": sha(vol.tobytes())[:12], "luts": {}}
        for w in quantiser_weightings(name):
            enc, dec = ref.quantiser_luts(vol, w, 1)
            enc3, dec3 = ref.quantiser_luts(vol, w, 3)
            assert np.array_equal(enc, enc3) and np.array_equal(dec, dec3), ("the reference disagrees with itself across thread counts", name, w)
            oenc, odec = o.quantiser_build_luts(o.histogram(vol), w)
            assert np.array_equal(enc, oenc) and np.array_equal(dec, odec), ("the oracle differs from the reference", name, w)
            e["luts"][w] = [sha(enc.tobytes()), sha(dec.astype("<u2").tobytes())]
        out["cases"][name] = e
    with open(os.path.join(GOLD, "quantiser_luts.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote quantiser_luts.json:", len(out["cases"]), "cases")


# ------------------------------------------------------------------------------------------------------------------------------------
# frame_shuffle and tile_shuffle against the reference's own templates (oracle/ref_driver.cpp): tests/golden/ref_shuffles.json
# ------------------------------------------------------------------------------------------------------------------------------------
def shuffle_table():
    """the smallest shapes that still take each branch; every volume at most 64 KiB"""
    T = []

    def add(stage, dtype, shape, kind, p):
        r = {"stage": stage, "dtype": dtype, "shape": list(shape), "kind": kind, "seed": 3000 + len(T)}
        r["frame_chunk_size" if stage == "frame_shuffle" else "tile_size"] = p
        r["id"] = shuffle_case_id(r, len(T))
        T.append(r)

    # ---- frame_shuffle: frames of 1 voxel, of 5 x 37 (no whole 16-byte vectors), of whole vectors; chunks of 1, 2, 3 and Z (one unit) ----
    for dt in ("uint16", "uint8"):
        add("frame_shuffle", dt, (1, 1, 1), "random", 1)
        add("frame_shuffle", dt, (7, 1, 1), "random", 1)
        add("frame_shuffle", dt, (40, 1, 1), "ramp", 1)
        add("frame_shuffle", dt, (40, 1, 1), "descending", 2)
        for chunk in (1, 2):
            add("frame_shuffle", dt, (40, 5, 37), "random", chunk)
        add("frame_shuffle", dt, (39, 5, 37), "random", 3)
        add("frame_shuffle", dt, (12, 5, 37), "random", 12)
        for kind in ("random", "ramp", "descending"):
            add("frame_shuffle", dt, (12, 8, 16), kind, 1)
        for chunk in (2, 3, 12):
            add("frame_shuffle", dt, (12, 8, 16), "descending", chunk)
        add("frame_shuffle", dt, (9, 8, 16), "all_equal", 1)
        add("frame_shuffle", dt, (9, 8, 16), "all_equal", 3)
        add("frame_shuffle", dt, (10, 8, 16), "two_groups", 1)
        add("frame_shuffle", dt, (20, 8, 16), "two_groups", 2)
        add("frame_shuffle", dt, (8, 5, 37), "permuted", 1)
        add("frame_shuffle", dt, (16, 8, 16), "permuted", 2)
        big = (4, 64, 128) if dt == "uint16" else (4, 128, 128)          # 64 KiB: four frames of 4 blocks, or one unit of 16
        add("frame_shuffle", dt, big, "random", 1)
        add("frame_shuffle", dt, big, "descending", 2)
        add("frame_shuffle", dt, big, "random", 4)
    for kind in ("pm128", "neg_means", "extremes", "random", "permuted", "all_equal", "two_groups"):
        add("frame_shuffle", "char", (12, 5, 37), kind, 1)
        add("frame_shuffle", "char", (12, 8, 16), kind, 2)
    add("frame_shuffle", "char", (15, 16, 16), "neg_means", 3)
    add("frame_shuffle", "char", (7, 1, 1), "pm128", 1)
    add("frame_shuffle", "char", (4, 128, 128), "neg_means", 1)
    add("frame_shuffle", "char", (4, 128, 128), "extremes", 1)
    add("frame_shuffle", "char", (4, 128, 128), "pm128", 4)
    # refused: Z is no multiple of the chunk
    for dt in ("uint16", "uint8", "char"):
        add("frame_shuffle", dt, (7, 8, 16), "random", 2)
        add("frame_shuffle", dt, (10, 8, 16), "random", 3)
        add("frame_shuffle", dt, (3, 4, 4), "random", 5)
    # ---- tile_shuffle: tiles of 2, 4, 5, 8 and 16; tile counts that differ per axis; a single tile ----
    for dt in ("uint16", "uint8", "char"):
        for shape, ts in (((4, 6, 8), 2), ((4, 12, 8), 4), ((5, 10, 15), 5), ((8, 16, 24), 8), ((16, 16, 32), 16)):
            add("tile_shuffle", dt, shape, "random", ts)
        for ts in (2, 5, 16):
            add("tile_shuffle", dt, (ts, ts, ts), "random", ts)
        add("tile_shuffle", dt, (8, 16, 24), "ramp", 8)
        add("tile_shuffle", dt, (8, 8, 12), "all_equal", 4)
        add("tile_shuffle", dt, (8, 8, 12), "permuted", 4)
        add("tile_shuffle", dt, (8, 12, 8), "two_groups", 4)
    for dt in ("uint16", "uint8"):
        add("tile_shuffle", dt, (8, 12, 8), "descending", 4)
        for shape, ts in (((4, 6, 8), 2), ((10, 10, 15), 5), ((8, 16, 24), 8), ((16, 32, 32), 16)):
            add("tile_shuffle", dt, shape, "fraction", ts)
    add("tile_shuffle", "uint16", (16, 32, 64), "random", 16)              # 64 KiB: eight tiles of two blocks
    add("tile_shuffle", "uint16", (32, 16, 32), "descending", 16)
    for shape, ts in (((4, 6, 8), 2), ((5, 10, 20), 5), ((8, 16, 24), 8), ((16, 32, 32), 16)):
        add("tile_shuffle", "uint8", shape, "integer_edge", ts)
    for kind in ("pm128", "neg_means", "extremes", "trunc_zero"):
        for shape, ts in (((4, 6, 8), 2), ((5, 10, 20), 5), ((8, 16, 24), 8), ((16, 32, 32), 16)):
            add("tile_shuffle", "char", shape, kind, ts)
    # refused: an axis that is no multiple of the tile, or shorter than it
    for dt in ("uint16", "uint8", "char"):
        add("tile_shuffle", dt, (8, 8, 9), "random", 4)
        add("tile_shuffle", dt, (6, 8, 8), "random", 4)
        add("tile_shuffle", dt, (8, 10, 8), "random", 4)
        add("tile_shuffle", dt, (2, 8, 8), "random", 4)
        add("tile_shuffle", dt, (16, 16, 8), "random", 16)
    return T


def shuffle_fns(row):
    """(oracle encode, oracle decode, reference encode, reference decode) of a row, all on the uint8 / uint16 array the case travels in"""
    char, p = row["dtype"] == "char", shuffle_param(row)
    if row["stage"] == "frame_shuffle":
        return (lambda v: o.frame_shuffle_encode(v, char=char, chunk=p), lambda e, m: o.frame_shuffle_decode(e, m, p),
                lambda v, nt: ref.frame_shuffle_encode(v, p, char, nt), lambda e, m: ref.frame_shuffle_decode(e, m, p, char))
    return (lambda v: o.tile_shuffle_encode(v, p, char=char), lambda e, m: o.tile_shuffle_decode(e, m, p),
            lambda v, nt: ref.tile_shuffle_encode(v, p, char, nt), lambda e, m: ref.tile_shuffle_decode(e, m, p, char))


def oracle_shuffle(row, vol):
    """the ORACLE's (output, decode_map, zero-filled decode of that output from that map); ValueError where the oracle refuses the shape"""
    enc, dec, _, _ = shuffle_fns(row)
    try:
        out, dmap = enc(vol)
    except NotImplementedError as e:                                        # frame_shuffle's word for a remainder
        raise ValueError(str(e))
    return out, dmap, dec(out, dmap)


def reference_shuffle(row, vol, nthreads=1):
    """the REFERENCE's, through oracle/_ref; ref.Remainder, with nothing of the reference run, where the shape has a remainder"""
    _, _, enc, dec = shuffle_fns(row)
    out, dmap = enc(vol, nthreads)
    return out, dmap, dec(out, dmap)


def is_permutation(dmap):
    return sorted(int(m) for m in dmap) == list(range(len(dmap)))


def frame_metric_reference(b, nthreads=1):
    """the live reference on a built case of tests/frame_metric_cases.py: (output, decode_map); the char and chunk forms as the case's kind says"""
    import frame_metric_cases as F
    c = b.case
    if c.kind == F.TILE:
        return ref.tile_shuffle_encode(b.volume, c.tile, nthreads=nthreads)
    return ref.frame_shuffle_encode(b.volume, 2 if c.kind == F.CHUNK else 1, c.kind == F.TAIL, nthreads)


def frame_metric_oracle(b):
    import frame_metric_cases as F
    c = b.case
    if c.kind == F.TILE:
        return o.tile_shuffle_encode(b.volume, c.tile)
    return o.frame_shuffle_encode(b.volume, char=c.kind == F.TAIL, chunk=2 if c.kind == F.CHUNK else 1)


def shuffles():
    """tests/golden/ref_shuffles.json: for every row of shuffle_table() what the REFERENCE's own detail::frame_shuffle / detail::tile_shuffle
    give (oracle/ref_driver.cpp): byte count and sha256 of the output, the decode_map as a list, the sha256 of the zero-filled decode of
    that output from that map; nthreads 1 and 4 asserted equal, the oracle asserted equal on the way.  Rows whose shape has a remainder are
    `refused` and the reference is not run on them.  And, by name, the decode_map the reference gives for every case of
    tests/frame_metric_cases.py, asserted equal to the case's expected_map."""
    import frame_metric_cases as F
    assert ref.shuffles_available(), "oracle/_ref/libsqy_ref.so missing or stale: run `make -C oracle` where the reference tree exists"
    G = {"_meta": {"generator": "oracle/gen_golden.py --shuffles",
                   "source": "sqeazy::detail::frame_shuffle and sqeazy::detail::tile_shuffle compiled in place (oracle/ref_driver.cpp)",
                   "inputs": "tests/ref_stage_inputs.py: shuffle_volume(case); dtype char travels as the uint8 array of the same bytes",
                   "decode_sha256": "the reference's decode of its own output from its own map into a ZERO-FILLED buffer (the driver's choice: the "
                                    "reference leaves slots that no map entry names as they were); the input itself where the map is a permutation",
                   "refused": "shapes with a remainder (Z % frame_chunk_size, an axis % tile_size, an axis shorter than the tile): the reference would "
                              "take its median path; it is not run on these rows and says nothing about them",
                   "frame_metric_cases": "tests/frame_metric_cases.py by name: the decode_map the reference gives for the built volume"},
         "cases": [], "frame_metric_cases": {}}
    for row in shuffle_table():
        vol = shuffle_volume(row)
        assert vol.nbytes <= 64 << 10, row["id"]
        e = dict(row)
        e["input_sha256"] = sha(vol.tobytes())[:12]
        if not shuffle_whole(row):
            for fn in (oracle_shuffle, reference_shuffle):
                try:
                    fn(row, vol)
                    raise AssertionError(("a shape with a remainder was not refused", row["id"], fn.__name__))
                except (ValueError, ref.Remainder):
                    pass
            e["refused"] = True
        else:
            out, dmap, back = reference_shuffle(row, vol, 1)
            out4, dmap4, back4 = reference_shuffle(row, vol, 4)
            assert np.array_equal(out, out4) and np.array_equal(dmap, dmap4) and np.array_equal(back, back4), (
                "the reference disagrees with itself across thread counts", row["id"])
            oout, omap, oback = oracle_shuffle(row, vol)
            assert np.array_equal(out, oout) and np.array_equal(dmap, omap) and np.array_equal(back, oback), ("the oracle differs from the reference", row["id"])
            if is_permutation(dmap):
                assert np.array_equal(back, vol), ("the reference's decode does not restore the input", row["id"])
            e["bytes"], e["sha256"] = out.nbytes, sha(out.tobytes())
            e["map"] = [int(m) for m in dmap]
            e["decode_sha256"] = sha(back.tobytes())
        G["cases"].append(e)
    for name in F.NAMES:
        b = F.built(name)
        out, dmap = frame_metric_reference(b, 1)
        out4, dmap4 = frame_metric_reference(b, 4)
        oout, omap = frame_metric_oracle(b)
        assert np.array_equal(dmap, dmap4) and np.array_equal(out, out4), ("the reference disagrees with itself across thread counts", name)
        assert np.array_equal(dmap, b.expected_map), ("the case's expected_map is not the reference's", name, dmap.tolist(), b.expected_map.tolist())
        assert np.array_equal(dmap, omap) and np.array_equal(out, oout), ("the oracle differs from the reference", name)
        G["frame_metric_cases"][name] = [int(m) for m in dmap]
        del b, out, out4, oout
    with open(os.path.join(GOLD, "ref_shuffles.json"), "w") as f:                 # compact, one case per line
        f.write('{"_meta": %s,\n"cases": [\n%s\n],\n"frame_metric_cases": %s}\n' % (
            json.dumps(G["_meta"], sort_keys=True),
            ",\n".join(json.dumps({k: v for k, v in c.items() if k != "id"}, sort_keys=True, separators=(",", ":")) for c in G["cases"]),
            json.dumps(G["frame_metric_cases"], sort_keys=True, separators=(",", ":"))))
    live = [c for c in G["cases"] if "refused" not in c]
    print("wrote ref_shuffles.json:", len(G["cases"]), "cases,", len(G["cases"]) - len(live), "refused,",
          sum(not is_permutation(c["map"]) for c in live), "with a map that is no permutation;", len(G["frame_metric_cases"]), "maps of frame_metric_cases")
    for stage in ("frame_shuffle", "tile_shuffle"):
        print(" ", stage, {dt: sum(c["stage"] == stage and c["dtype"] == dt for c in G["cases"]) for dt in ("uint16", "uint8", "char")})


if __name__ == "__main__":
    if "--stages" in sys.argv:
        stages()
    elif "--shuffles" in sys.argv:
        shuffles()
    elif "--quantiser" in sys.argv:
        quantiser()
    elif "--accel" in sys.argv:
        accel()
    elif "--lz4-planted" in sys.argv:
        lz4_planted()
    elif "--lz4-linked-planted" in sys.argv:
        lz4_linked_planted()
    elif "--headline-slabs" in sys.argv:
        headline_slabs()
    elif "--headline-serial" in sys.argv:
        headline_serial()
    elif "--headline" in sys.argv:
        lz4_planted()
        headline()
        headline_serial()
    else:
        main()
        stages()
        shuffles()
        quantiser()
        accel()
        lz4_planted()
        lz4_linked_planted()
        headline()
        headline_serial()
