"""bitswap1 at the seams of the transposer kernels it runs through (numpy only, no GPU): a plain definition of the operation, the launchers'
routing restated, and a table of named lengths, each the smallest that reaches one branch, with the route it claims.

THE DEFINITION.  planes(a) / voxels(p) are written from the stage's description alone -- W = 16 or 8 bits per voxel, seg = len // W words per
plane, L = seg * W; plane segment W - 1 - b carries bit b; word w of a segment holds voxels W w .. W w + W - 1, voxel W w + j at bit
W - 1 - j; the voxels [L, len) are copied behind the planes -- as unpackbits / transpose / packbits.  They share no code with the kernels and
none with the C oracle; tests/test_bitswap_seams_host.py holds them to the oracle, tests/test_gpu_bitswap_seams.py holds the kernels to both.

THE ROUTING is RESTATED here, not observed: the functions below repeat the launchers' decisions of csrc/sqy_kernels.hip as plain arithmetic,
each next to the name of what it repeats.  Nothing in the product reports which transposer a call took (the profile tells the fused quantiser
kernels apart, nothing else); a change to a launcher's condition has to be repeated here by hand.  The tile is BSW_TILE_VOX = 8192 voxels,
a constant of sqy_kernels.hip that no header exposes: sqy_pipeline.hpp's kBatchTileVoxels (32768) is the BATCH transposers' tile, another
kernel family's, and not this one.

OUT OF SCOPE, on purpose: the grid-stride loop of the register kernel that is not in place starts beyond 64 * CUs tiles (128 Mi voxels at
256 CUs) -- tests/test_gpu_fullsize.py reaches it; the fused quantiser transposer's grid is capped at 2 * CUs workgroups only beyond
2 * CUs * 4096 plane bytes (16 Mi voxels at 256 CUs), below that its loop makes at most four trips (fused_quantiser_trips)."""
import numpy as np

TILE_VOXELS = 8192                                          # BSW_TILE_VOX: 64 lanes x 128 voxels, 1 KiB of every plane
TILE_WORDS = TILE_VOXELS // 16                              # plane words of a tile


# ---- the plain definition --------------------------------------------------------------------------------------------------------------------
def _width(dtype):
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.uint16), np.dtype(np.uint8)):
        raise TypeError(dtype)
    return dtype.itemsize * 8


def planes(a):
    """the plane stream of the voxels `a` (uint16 or uint8, any shape; flat result of the same type and length)"""
    a = np.ascontiguousarray(a).reshape(-1)
    W = _width(a.dtype)
    L = a.size // W * W
    be = a.dtype.newbyteorder(">")
    bits = np.unpackbits(a[:L].astype(be).view(np.uint8)).reshape(L, W)          # bits[i, k] = bit W - 1 - k of voxel i
    words = np.packbits(np.ascontiguousarray(bits.T), axis=1)                    # row k = segment k; voxel W w + j at bit W - 1 - j of word w
    return np.concatenate([words.reshape(-1).view(be).astype(a.dtype), a[L:]])


def voxels(p):
    """the voxels whose plane stream is `p`: the mirror image of planes()"""
    p = np.ascontiguousarray(p).reshape(-1)
    W = _width(p.dtype)
    L = p.size // W * W
    be = p.dtype.newbyteorder(">")
    bits = np.unpackbits(p[:L].astype(be).view(np.uint8)).reshape(W, L)          # bits[k, i] = bit W - 1 - k of voxel i
    vox = np.packbits(np.ascontiguousarray(bits.T), axis=1)
    return np.concatenate([vox.reshape(-1).view(be).astype(p.dtype), p[L:]])


def first_difference(got, want):
    """None, or where two plane streams of one volume first differ: a dict with the stream index, and either plane segment, word, bit of the
    word and the voxel index and voxel bit that land there, or (behind the planes) the tail voxel"""
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    if got.dtype != want.dtype or got.size != want.size:
        return {"streams": (str(got.dtype), got.size, str(want.dtype), want.size)}
    d = np.flatnonzero(got != want)
    if not len(d):
        return None
    i = int(d[0])
    W = _width(want.dtype)
    seg = want.size // W
    g, w_ = int(got[i]), int(want[i])
    if i >= seg * W:
        return {"index": i, "tail_voxel": i, "got": g, "want": w_, "differing": len(d)}
    segment, word = divmod(i, seg)
    bit = (g ^ w_).bit_length() - 1                                               # the highest differing bit: the first voxel of the word
    return {"index": i, "plane_segment": segment, "word": word, "bit": bit, "voxel": W * word + (W - 1 - bit), "voxel_bit": W - 1 - segment,
            "got": g, "want": w_, "differing": len(d)}


# ---- the launchers' decisions, restated ------------------------------------------------------------------------------------------------------
def _generic(tiles, rest_words, tail, seg):
    if not rest_words and not tail:
        return "none"
    if not tiles and seg:
        return "whole"                                      # every plane word (and the tail, if any) through the generic kernel
    if not rest_words:
        return "tail-only"
    return "both" if tail else "rest"


def encode_route_u16(n, src_aligned=True, lz4_behind=False, in_place=False, tiles_per_wave=1):
    """launch_bitswap1_u16 and bitswap1_piece_hash_words.  src_aligned: source (and, where the planes go to a buffer of the driver's own,
    destination) on a 16-byte boundary; lz4_behind: the stage in front of lz4, which asks for piece hashes; in_place: frames in place
    (the destination takes an offset), possible only with piece hashes.
      tiles: tiles of the register kernel | regs_blocks: its workgroups of two waves | idle_wave: the last workgroup's second wave has no tile
      first_word, rest_words, tail: what the generic kernel takes | generic: none / rest / tail-only / both / whole | generic_blocks
      piece_hashes: 16 x 4 words per tile | in_place: bitswap1_u16_regs<true>"""
    seg = n // 16
    hashes = bool(lz4_behind and n and n % TILE_VOXELS == 0 and src_aligned)
    if in_place and hashes:
        tiles = n // TILE_VOXELS
        return {"tiles": tiles, "regs_blocks": (tiles + 2 * tiles_per_wave - 1) // (2 * tiles_per_wave), "idle_wave": tiles_per_wave == 1 and tiles % 2 == 1,
                "first_word": seg, "rest_words": 0, "tail": 0, "generic": "none", "generic_blocks": 0, "piece_hashes": True, "in_place": True}
    tiles = seg // TILE_WORDS if seg % 8 == 0 and src_aligned else 0
    first_word = TILE_WORDS * tiles
    rest_words, tail = seg - first_word, n - 16 * seg
    launched = bool(rest_words or tail)
    return {"tiles": tiles, "regs_blocks": (tiles + 1) // 2, "idle_wave": tiles % 2 == 1, "first_word": first_word, "rest_words": rest_words, "tail": tail,
            "generic": _generic(tiles, rest_words, tail, seg), "generic_blocks": max((rest_words + 255) // 256, 1) if launched else 0,
            "piece_hashes": hashes, "in_place": False}


def decode_route_u16(n, in_aligned=True):
    """launch_bitswap1_decode, elem_size == 2.  in_aligned: planes and destination on a 16-byte boundary.  The rest kernel
    (bitswap1_decode_kernel) always launches, from word w0, and its block 0 moves the tail"""
    seg = n // 16
    tiles = seg // TILE_WORDS if seg % 8 == 0 and in_aligned else 0
    w0 = TILE_WORDS * tiles
    rest_words, tail = seg - w0, n - 16 * seg
    return {"tiles": tiles, "regs_blocks": min((tiles + 3) // 4, 65536), "w0": w0, "rest_words": rest_words, "tail": tail,
            "generic": _generic(tiles, rest_words, tail, seg), "generic_blocks": max((rest_words + 255) // 256, 1)}


def encode_route_u8(n):
    """launch_bitswap1_u8: bitswap1_u8_generic, one thread per plane byte, workgroups of 128; block 0 moves the tail"""
    seg = n // 8
    return {"seg": seg, "blocks": max((seg + 127) // 128, 1), "last_block_threads": (seg - 1) % 128 + 1 if seg else 0, "tail": n - 8 * seg}


def decode_route_u8(n):
    """launch_bitswap1_decode, the elem_size == 1 branch: bitswap1_decode_kernel<uint8_t>, workgroups of 256"""
    seg = n // 8
    return {"seg": seg, "blocks": max((seg + 255) // 256, 1), "last_block_threads": (seg - 1) % 256 + 1 if seg else 0, "tail": n - 8 * seg}


def lut_decode_possible(n):
    """bitswap1_u8_decode_lut_possible for the driver's own (16-byte aligned) buffers: the fused inverse of quantiser->bitswap1 takes the
    blob; else bitswap1_decode and quantiser_decode one after the other"""
    return n != 0 and n % 128 == 0


def lut_decode_route(n):
    """launch_bitswap1_u8_decode_lut: a lane owns 16 bytes of every plane (128 voxels), a wave 64 of those"""
    nvec = n // 128
    return {"nvec": nvec, "blocks": min((nvec + 255) // 256, 65536), "whole_waves": nvec // 64, "partial_wave_lanes": nvec % 64}


def fused_quantiser_trips(n, cus):
    """launch_quantiser_apply_bitswap1_u8 and the loop of quantiser_apply_bitswap1_u8_kernel: a thread takes plane bytes v0, v0 + step, ..,
    v0 + 3 step per trip (four loads in flight), v0 += 4 step.  slots: the step-wide slots that hold at least one plane byte, over all
    trips; last_slot_threads: the threads of the launch that are live in the last of them"""
    seg = n // 8
    blocks = max(min((seg + 4095) // 4096, 2 * cus), 1)
    step = blocks * 256
    slots = (seg + step - 1) // step
    return {"seg": seg, "blocks": blocks, "step": step, "capped": (seg + 4095) // 4096 > 2 * cus, "trips": (seg + 4 * step - 1) // (4 * step),
            "slots": slots, "last_trip_slots": (slots - 1) % 4 + 1 if slots else 0, "last_slot_threads": seg - (slots - 1) * step if slots else 0,
            "tail": n - 8 * seg}


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
T = TILE_VOXELS
U16_LENGTHS = [
    (T - 1, "no tile: every word and a tail of 15 through the generic kernel"),
    (T, "one tile, no generic launch"),
    (T + 1, "one tile and a tail-only generic launch"),
    (T + 16, "seg = 513, no multiple of 8: the register kernel is dropped for the whole buffer"),
    (T + 128, "one tile and 8 rest words"),
    (T + 128 + 5, "one tile, 8 rest words and a tail"),
    (2 * T, "two tiles: one workgroup, both waves busy"),
    (3 * T + 3 * 128 + 15, "odd tile count: the last workgroup's second wave is idle; rest words and the longest tail"),
    (5 * T + 511 * 16, "the widest rest that is no multiple of 8 words: all generic at five tiles' worth, three generic workgroups"),
    (5 * T + 504 * 16, "the widest rest the register kernel leaves: two generic workgroups, the second partial"),
    (33 * T, "thirty-three tiles"),
]
U8_LENGTHS = [
    (7, "no whole word: tail only"), (8, "one word"), (9, "one word and a tail voxel"),
    (1023, "one 128-thread workgroup short of a word, tail of 7"), (1024, "one 128-thread workgroup, full"), (1025, "the same and a tail voxel"),
    (128 * 63, "a wave of the LUT decode with one lane idle"), (128 * 64, "a whole wave of the LUT decode"), (128 * 65, "a whole wave and a partial one"),
    (128 * 64 + 8, "one word more than whole 16-byte vectors: the LUT decode is refused"),
    (128 * 257, "the LUT decode's second workgroup, of one lane"),
]
KINDS = ("random", "onehot", "top", "ones")
ONEHOT_BITS = (0, 7, 8, 15)
ONEHOT_FIXED = (0, 1, 15, 16, 127, 128, 2047, 2048, 8191, 8192)


def fused_length(cus):
    """the fused quantiser transposer's long case: 5 x (2 cus x 256) + 77 plane bytes and a tail of 5 voxels"""
    return 8 * (5 * (2 * cus * 256) + 77) + 5


def onehot_indices(n, dtype):
    """where the `onehot` kind plants its single-bit voxels: the fixed indices; the last voxel the register kernel owns and the first of the
    rest; the last word's last voxel and the first tail voxel -- each only where the length has it"""
    W = _width(dtype)
    L = n // W * W
    want = list(ONEHOT_FIXED)
    if W == 16:
        owned = encode_route_u16(n)["tiles"] * TILE_VOXELS
        want += [owned - 1, owned]
    want += [L - 1, L]
    return sorted({i for i in want if 0 <= i < n})


def make(kind, dtype, n, seed):
    """the volume of a case: flat, full range, seeded"""
    dtype = np.dtype(dtype)
    W = _width(dtype)
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 1 << W, n, dtype=dtype)
    if kind == "onehot":
        a = np.zeros(n, dtype)
        for k, i in enumerate(onehot_indices(n, dtype)):
            a[i] = 1 << (ONEHOT_BITS[(k + seed) % 4] % W)
        return a
    if kind == "top":
        return ((1 << (W - 1)) | (np.arange(n) & 1)).astype(dtype)
    if kind == "ones":
        return np.full(n, (1 << W) - 1, dtype)
    raise ValueError(kind)


def _case(n, dtype, kind, seed, branch):
    dtype = np.dtype(dtype)
    c = {"name": "%s-%d-%s" % (dtype.name, n, kind), "n": n, "dtype": dtype.name, "kind": kind, "seed": seed, "branch": branch}
    if dtype == np.uint16:
        c["encode"] = encode_route_u16(n)                                           # from the driver's own buffers
        # in front of lz4 through an entry point that takes no offset (SQYAMD_PipelineEncode_*_Device).  The host entry point hands its
        # staging buffer over WITH an offset: for whole tiles lz4_inplace_plan then decides from that buffer's capacity whether the planes
        # are written as frames in place (bitswap1_u16_regs<true>) -- not restated here; the bytes are the oracle's either way
        c["encode_lz4"] = encode_route_u16(n, lz4_behind=True)
        c["encode_off_grid"] = encode_route_u16(n, src_aligned=False, lz4_behind=True)
        c["decode"] = decode_route_u16(n)                                           # behind lz4: the LZ4 stage's output buffer
        c["decode_off_grid"] = decode_route_u16(n, in_aligned=False)                # behind the header, where that is off the grid
    else:
        c["encode"] = c["encode_lz4"] = c["encode_off_grid"] = encode_route_u8(n)
        c["decode"] = c["decode_off_grid"] = decode_route_u8(n)
        c["lut"] = lut_decode_possible(n)
    return c


def _table():
    out = []
    for dtype, lengths in ((np.uint16, U16_LENGTHS), (np.uint8, U8_LENGTHS)):
        for i, (n, branch) in enumerate(lengths):
            for k, kind in enumerate(KINDS):
                out.append(_case(n, dtype, kind, 7100 + 16 * i + k, branch))
    return out


CASES = _table()
BY_NAME = {c["name"]: c for c in CASES}
U16_CASES = [c for c in CASES if c["dtype"] == "uint16"]
U8_CASES = [c for c in CASES if c["dtype"] == "uint8"]
TILE_CASES = [c for c in U16_CASES if c["encode"]["tiles"]]                         # .. also encoded from a source off the 16-byte grid
SHIFTS = {"uint16": (0, 2, 8), "uint8": (0, 1)}                                     # bytes behind a 16-byte boundary; 0: the aligned device source

_volumes = {}


def volume(case):
    """the case's input, shape (1, 1, n), made once"""
    if case["name"] not in _volumes:
        v = make(case["kind"], case["dtype"], case["n"], case["seed"]).reshape(1, 1, -1)
        v.setflags(write=False)
        _volumes[case["name"]] = v
    return _volumes[case["name"]]


def case_id(case):
    return case["name"]


def describe(case, route="encode"):
    return "%s [%s; %s %r]" % (case["name"], case["branch"], route, case[route])


def failure(case, route, what, diff):
    """the message of a failed comparison: the case, its branch and claimed route, the first difference; no blobs"""
    return "%s: %s: first difference %r" % (describe(case, route), what, diff)


# ---- frames in place (bitswap1_u16_regs<true>) -----------------------------------------------------------------------------------------------
def frames_volume(tiles, kind, zero_tiles=()):
    """(tiles, 64, 128) voxels of `kind`, the tiles `zero_tiles` all zero (holes in every plane)"""
    key = ("frames", tiles, kind, tuple(zero_tiles))
    if key not in _volumes:
        v = make(kind, np.uint16, tiles * TILE_VOXELS, 7900 + tiles).reshape(tiles, TILE_VOXELS)
        for t in zero_tiles:
            v[t] = 0
        v = v.reshape(tiles, 64, 128)
        v.setflags(write=False)
        _volumes[key] = v
    return _volumes[key]


# ---- quantiser->bitswap1 ---------------------------------------------------------------------------------------------------------------------
QUANTISER_LENGTHS = [n for n, _ in U8_LENGTHS]


def narrow_band(n, seed):
    """16-bit voxels in a band of 200 values around 1000: every value gets a bucket of its own, so the sink's bytes take 200 values and
    every one of the 8 planes is busy"""
    key = ("narrow", n, seed)
    if key not in _volumes:
        v = (np.random.default_rng(seed).integers(0, 200, n) + 900).astype(np.uint16).reshape(1, 1, -1)
        v.setflags(write=False)
        _volumes[key] = v
    return _volumes[key]
