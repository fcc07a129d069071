"""diff3x3x1 at the seams of the kernels it runs through (numpy only, no GPU): a table of named cases, each the smallest shape that reaches
one branch, with the geometry the launchers derive from the shape, and a numpy model of the decode chain's strip schedule.

The routing is RESTATED here, not observed: the functions below repeat the launchers' decisions of csrc/sqy_kernels.hip and csrc/sqy_capi.cpp
as plain arithmetic, each next to the name of what it repeats.  Nothing in the product reports which kernel a call took; a change to a
launcher's condition has to be repeated here by hand.  What the host-only code does expose -- kDiffStripRows, kDiffChainFrames and
decode_batch_plan's strip and step counts (csrc/sqy_pipeline.hpp) -- tests/test_diff_seams_host.py holds this module to.

Inputs are tests/ref_stage_inputs.py's: kind `random` (full range, so the 3 x 3 sums wrap in 16 bits) and `max`.  The encode cases are also
rows of tests/golden/ref_stages.json (oracle/gen_golden.py takes ENCODE_SHAPES, MAX_SHAPES and their seeds from here), so the reference's own
diff_scheme judges the stage's payload on them."""
import numpy as np

from ref_stage_inputs import stage_input

# ---- constants of the kernels (sqy_kernels.hip: DDK_K, DDK_R, DDK_ROWS, DDK_THREADS, DDK_ITEMS; BSW_TILE_VOX) --------------------------------
CHAIN_FRAMES = 8                                            # DDK_K = kDiffChainFrames: frames per chain launch
STRIP_ROWS = 32                                             # DDK_R = kDiffStripRows: rows a workgroup owns
IMAGE_ROWS = STRIP_ROWS + 2 * CHAIN_FRAMES                  # DDK_ROWS: the strip and the widest halo on both sides
CHAIN_THREADS = 1024                                        # DDK_THREADS
CHAIN_ITEMS = 2                                             # DDK_ITEMS: (row, vector) items of an image a thread owns at most
LDS_BYTES = 64 << 10
TILE_VOXELS = 8192                                          # BSW_TILE_VOX: the transposer's tile, which the side path needs whole


# ---- the launchers' decisions, restated ----------------------------------------------------------------------------------------------------
def halo(shape):
    """(hx, zlim, single): the first lines of launch_diff3x3x1 and launch_diff3x3x1_decode"""
    Z, Y, X = shape
    zlim = min(X, Z)
    single = max(zlim - 1, 0) * max(Y - 2, 0) == 1
    return (0 if single else max(Z - 2, 0)), zlim, single


def rows_geometry(shape):
    """launch_diff3x3x1's condition for diff3x3x1_u16_rows_kernel (16-bit voxels): every row's reach 1 + hx, and x + 1, stay inside the row"""
    Z, Y, X = shape
    hx, _, single = halo(shape)
    return not single and hx + 2 <= X and Y <= 65535 and Z <= 65535 and X <= 0xffffffff


def side_width(shape):
    """diff3x3x1_side_width for 16-bit voxels: the columns of the compact side buffer, 0 = no side path"""
    Z, Y, X = shape
    if X % 128 or (Z * Y * X) % TILE_VOXELS:
        return 0
    if halo(shape)[2] or not rows_geometry(shape):
        return 0
    w = (1 + (Z - 2) + 127) // 128 * 128
    return w if w < X else 0


def rows_per_block(columns):
    """the `rpb` loop of launch_diff3x3x1_side (columns = side_w) and of launch_diff3x3x1_decode (columns = w): a power of two up to 16"""
    rpb = 1
    while rpb < 16 and (columns // 8) * rpb * 2 <= 256:
        rpb *= 2
    return rpb


def encode_route(shape, bitswap1_behind=True, source_aligned=True):
    """which kernel the stage's encode takes, and with what grid.  `side`: SQYAMD's diff3x3x1 stage (sqy_capi.cpp) asks for the side buffer
    when a 16-bit bitswap1 follows and the source lies on a 16-byte boundary; `rows`: launch_diff3x3x1's condition; else `generic`"""
    Z, Y, X = shape
    sw = side_width(shape) if bitswap1_behind and source_aligned else 0
    if sw:
        rpb = rows_per_block(sw)
        tpr = 256 // rpb
        return {"route": "side", "side_w": sw, "rows_per_block": rpb, "threads_per_row": tpr, "lanes_used": sw // 8,
                "bx": (sw // 8 + tpr - 1) // tpr, "by": (Y + rpb - 1) // rpb}
    if rows_geometry(shape):
        return {"route": "rows", "side_w": 0, "rows_per_block": 1, "threads_per_row": 256, "lanes_used": (X + 7) // 8, "bx": (X + 2047) // 2048, "by": Y}
    return {"route": "generic", "side_w": 0, "rows_per_block": 0, "threads_per_row": 0, "lanes_used": 0, "bx": 0, "by": 0}


def chain_columns(shape):
    """diff3x3x1_decode_chain_columns for 16-bit voxels: the leading columns that go through the chain (touched ones and their right-hand
    neighbour, whole 16-byte vectors), 0 = another geometry"""
    Z, Y, X = shape
    if Z * Y * X == 0 or not rows_geometry(shape) or X % 8:
        return 0
    return min((2 + halo(shape)[0] + 7) // 8 * 8, X)


def frames_fit(w):
    """diff3x3x1_decode_frames_fit: two LDS images of IMAGE_ROWS rows of w + 16 voxels, and an image's items within a workgroup's slots"""
    return 2 * IMAGE_ROWS * (w + 16) * 2 <= LDS_BYTES and IMAGE_ROWS * (w // 8 + 1) <= CHAIN_ITEMS * CHAIN_THREADS


def decode_route(shape):
    """what launch_diff3x3x1_decode does with a 16-bit volume whose buffers lie on 16-byte boundaries (the driver's own always do):
    `chain_frames` (diff3x3x1_u16_decode_frames_kernel, CHAIN_FRAMES frames per launch), `chain_per_frame` (the rows kernel, one launch per
    frame, where the images do not fit) or `generic` (diff3x3x1_decode_plane_kernel).  launches / last_frames: the chain's launches and the
    frames of the last one; items: (row, vector) items of an image; item_slots: how many of a thread's CHAIN_ITEMS are in use"""
    w = chain_columns(shape)
    zlim = halo(shape)[1]
    frames = max(zlim - 1, 0)
    if not w:
        return {"route": "generic", "w": 0, "items": 0, "item_slots": 0, "launches": 0, "last_frames": 0, "strips": 0}
    if not frames_fit(w):
        return {"route": "chain_per_frame", "w": w, "items": 0, "item_slots": 0, "launches": frames, "last_frames": min(frames, 1), "strips": 0}
    items = IMAGE_ROWS * (w // 8 + 1)
    launches = (frames + CHAIN_FRAMES - 1) // CHAIN_FRAMES
    return {"route": "chain_frames", "w": w, "items": items, "item_slots": (items + CHAIN_THREADS - 1) // CHAIN_THREADS, "launches": launches,
            "last_frames": frames - CHAIN_FRAMES * (launches - 1) if launches else 0, "strips": (shape[1] + STRIP_ROWS - 1) // STRIP_ROWS}


def batch_joint(shape):
    """batch_stage_form (sqy_capi.cpp) for the two diff forms, destination on a 16-byte boundary: the joint chain takes the blob"""
    w = chain_columns(shape)
    return bool(w) and frames_fit(w)


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
ENCODE_SEED0, MAX_SEED0, DECODE_SEED0 = 5200, 5300, 5400

BOUNDARY = [                                               # encode, rows | generic boundary
    ((10, 5, 10), "Z = X: the last shape of the rows kernel, X % 8 != 0, last rewritten column X - 2"),
    ((11, 5, 10), "Z = X + 1: generic kernel, the reach ends on the row's last voxel"),
    ((12, 5, 10), "Z = X + 2: generic kernel, the first spill into column 0 of the next row"),
    ((9, 4, 24), "hx = 7: the last rewritten voxel is the last of thread 0"),
    ((10, 4, 24), "hx = 8: the last rewritten voxel is the first of thread 1"),
    ((4, 3, 8), "one full 16-byte vector per row"),
    ((4, 3, 9), "a full vector and a partial one of one voxel"),
    ((4, 3, 15), "a full vector and a partial one of seven voxels"),
    ((4, 3, 16), "two full vectors"),
    ((4, 3, 17), "two full vectors and one voxel"),
    ((3, 3, 2048), "bx = 1: one block covers the row"),
    ((3, 3, 2056), "bx = 2: a second block for the last vector"),
]
SIDE = [                                                   # encode, side path (each a whole number of TILE_VOXELS) and its near misses
    ((3, 64, 256), "side path, hx = 1"),
    ((128, 3, 256), "side path, 1 + hx = 127"),
    ((129, 32, 256), "side path, 1 + hx = 128: the side buffer's last column is rewritten"),
    ((130, 16, 256), "1 + hx = 129: side_w = 256 = X, no side buffer"),
    ((130, 16, 512), "side path, side_w = 256 of 512"),
    ((64, 5, 256), "side path, rpb = 16 and Y = 5: a block whose rows run past Y"),
    ((64, 17, 256), "side path, Y = rpb + 1: a second block of one row"),
    ((272, 3, 512), "side path, side_w = 384: rpb = 4, 48 of 64 lanes per row, Y = 3"),
    ((63, 5, 256), "near miss: the length is no multiple of the transposer's tile"),
]
CHAIN = ([((Z, 33, 16), "chain: %d frames in the last launch of %d, a second strip of one row" % ((Z - 2) % 8 + 1, (Z + 5) // 8))
          for Z in (2, 3, 4, 5, 6, 7, 8, 9, 10)] +
         # X = 16 holds no chain of more than 15 frames (hx + 2 <= X means Z <= X): these two take the generic inverse, with rows that spill;
         # the two full launches, and a third of one frame, are the two shapes behind them
         [((17, 33, 16), "Z = X + 1 with two strips' worth of rows: generic inverse, the reach ends on the row's last voxel"),
          ((18, 33, 16), "Z = X + 2 with two strips' worth of rows: generic inverse, rows spill"),
          ((17, 33, 24), "chain: two full launches, a second strip of one row"),
          ((18, 33, 24), "chain: two full launches and one of one frame, a second strip of one row")] +
         [((10, Y, 16), "chain: %d rows, halo clipped at both ends, %d strip(s)" % (Y, (Y + 31) // 32)) for Y in (3, 4, 31, 32, 33, 64, 65)] +
         [((3, 3, 8), "chain: hx = 1, one touched row, w = 8 = X, the narrowest chain"),
          ((14, 5, 16), "chain: w = X, there is no column w"),
          ((14, 5, 24), "chain: w = 16 < X"),
          ((16, 5, 24), "chain: hx + 2 = 16 exactly, w = 16 < X"),
          ((17, 5, 24), "chain: hx + 2 = 17, w = 24 = X"),
          # w = 176: items 1024 .. 1103 are image rows 44 .. 47 = volume rows 36 .. 39 of strip 0 (68 .. 71 of strip 1).  With Y = 3 or 35 the
          # second slot holds only items that must stay off; with Y = 40 it holds live halo rows of strip 0
          ((176, 3, 176), "chain: w = 176, the second item slot holds only rows past Y"),
          ((170, 35, 176), "chain: w = 176, the second item slot holds only rows past Y, two strips"),
          ((170, 40, 176), "chain: w = 176, the second item slot holds the halo rows 36 .. 39 of strip 0"),
          ((320, 3, 320), "chain: w = 320, the widest image that fits; the second item slot holds only rows past Y"),
          ((313, 34, 320), "chain: w = 320, two strips, the second item slot holds rows 17 .. 39 of strip 0"),
          ((321, 3, 328), "w = 328 does not fit: one launch per frame")])

ENCODE_SHAPES = [s for s, _ in BOUNDARY + SIDE]             # rows of ref_stages.json, kind `random`, seeds ENCODE_SEED0 + index
MAX_SHAPES = [(10, 5, 10), (129, 32, 256)]                  # .. and kind `max`, seeds MAX_SEED0 + index


def _case(name, shape, kind, seed, branch, group):
    c = {"name": name, "shape": tuple(shape), "dtype": "uint16", "kind": kind, "seed": seed, "branch": branch, "group": group}
    c["hx"], c["zlim"], c["single"] = halo(shape)
    c["encode"] = encode_route(shape)
    c["decode"] = decode_route(shape)
    return c


def _name(shape, kind="random"):
    return "%dx%dx%d-%s" % (tuple(shape) + (kind,))


def _table():
    T = []
    for i, (shape, branch) in enumerate(BOUNDARY + SIDE):
        T.append(_case(_name(shape), shape, "random", ENCODE_SEED0 + i, branch, "boundary" if i < len(BOUNDARY) else "side"))
    for i, shape in enumerate(MAX_SHAPES):
        branch = dict(BOUNDARY + SIDE)[shape]
        T.append(_case(_name(shape, "max"), shape, "max", MAX_SEED0 + i, branch + " (all voxels 65535)", "boundary" if shape in dict(BOUNDARY) else "side"))
    seen = {c["shape"] for c in T}
    for i, (shape, branch) in enumerate(CHAIN):
        if shape in seen:                                   # (10, 33, 16) stands in both lists: one case, both branches
            prior = [c for c in T if c["shape"] == shape][0]
            prior["branch"] += "; " + branch
            continue
        seen.add(shape)
        T.append(_case(_name(shape), shape, "random", DECODE_SEED0 + i, branch, "chain"))
    return T


CASES = _table()
BY_NAME = {c["name"]: c for c in CASES}
SIDE_CASES = [c for c in CASES if c["group"] == "side"]
MISALIGNED = "64x5x256-random"                              # also encoded from a device source 2 bytes behind a 16-byte boundary
# batch decode: the widest and the narrowest chain in one launch; a blob the planner must keep off the joint path next to one it takes
BATCH_JOINT = ("320x3x320-random", "10x33x16-random", "3x3x8-random")
BATCH_MIXED = ("321x3x328-random", "10x33x16-random")
# the pairs and triples on both sides of a boundary of the reach
REACH_SETS = (("9x4x24-random", "10x4x24-random"), ("128x3x256-random", "129x32x256-random", "130x16x256-random"))

_volumes = {}


def volume(case):
    """the case's input, made once"""
    if case["name"] not in _volumes:
        v = stage_input(case["kind"], np.uint16, case["shape"], case["seed"])
        v.setflags(write=False)
        _volumes[case["name"]] = v
    return _volumes[case["name"]]


def case_id(case):
    return case["name"]


def describe(case):
    return "%s [%s; encode %s, decode %s]" % (case["name"], case["branch"], case["encode"]["route"], case["decode"]["route"])


# ---- which voxels the stage rewrites ---------------------------------------------------------------------------------------------------------
def touched_mask(shape):
    """flat bool mask of the rewritten voxels: the union over 1 <= z < zlim, 1 <= y <= Y - 2 of [s, s + reach), s = z Y X + y X + 1, reach = hx
    (`single`: to the end of the volume) -- the header comment of diff3x3x1_kernel"""
    Z, Y, X = shape
    hx, zlim, single = halo(shape)
    n = Z * Y * X
    m = np.zeros(n + 1, np.int32)
    for z in range(1, zlim):
        for y in range(1, Y - 1):
            s = (z * Y + y) * X + 1
            e = n if single else min(s + hx, n)
            if s < e:
                m[s] += 1
                m[e] -= 1
    return np.cumsum(m[:n]) > 0


def reach_edges(shape):
    """(last, first): flat indices of the last voxel of every rewritten run and of the first voxel behind it"""
    t = touched_mask(shape)
    ends = np.flatnonzero(t[:-1] & ~t[1:])
    return ends, ends + 1


def first_difference(got, want):
    """None, or (z, y, x, got, want) of the first differing voxel"""
    got, want = np.asarray(got), np.asarray(want)
    d = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    if not len(d):
        return None
    z, y, x = np.unravel_index(int(d[0]), want.shape)
    return int(z), int(y), int(x), int(got.reshape(-1)[d[0]]), int(want.reshape(-1)[d[0]])


def failure(case, what, diff):
    """the message of a failed comparison: the case, its branch, the first differing voxel; no blobs"""
    return "%s: %s: first differing voxel (z, y, x, got, want) = %r" % (describe(case), what, diff)


# ---- a numpy model of the chain's strip schedule ---------------------------------------------------------------------------------------------
def _mean9(A, rows, x0, x1):
    """floor(wrapping 16-bit sum of the 3 x 3 neighbours / 9) for image rows `rows`, columns [x0, x1) of image A (column c at A[:, c + 1])"""
    s = np.zeros((len(rows), x1 - x0), np.uint32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            s += A[rows + dy][:, x0 + dx + 1:x1 + dx + 1]
    return (s & 0xffff) // 9


def chain_model(enc, halo_shift=0, items=CHAIN_ITEMS, reach_shift=0, fill=0xA5A5):
    """decode of the 16-bit residual volume `enc` in the chain geometry the way launch_diff3x3x1_decode and
    diff3x3x1_u16_decode_strip schedule it: columns [w, X), frame 0 and the frames z >= zlim are copies; frames 1 .. zlim - 1 go CHAIN_FRAMES
    per launch, every strip of STRIP_ROWS rows on its own -- from the decoded frame z0 - 1 in one image, frame j of the launch is decoded
    for the rows [y0 - h, y0 + STRIP_ROWS + h), h = nframes - 1 - j, into the other image, which keeps what it held everywhere else; only
    the strip's own rows go to the output.  An item is 8 columns of one image row (or the single column w), item t belongs to thread
    t % CHAIN_THREADS, slot t // CHAIN_THREADS.
      halo_shift: added to h (kept within 0 .. CHAIN_FRAMES - 1: a strip always decodes its own rows) | items: item slots a thread has |
      reach_shift: added to the rewritten columns' end 1 + hx
    Voxels nobody writes hold `fill`."""
    enc = np.asarray(enc)
    Z, Y, X = enc.shape
    hx, zlim, single = halo(enc.shape)
    w = chain_columns(enc.shape)
    assert w and enc.dtype == np.uint16
    out = np.full(enc.shape, fill, np.uint16)
    out[:, :, w:] = enc[:, :, w:]
    out[0] = enc[0]
    out[zlim:] = enc[zlim:]
    vpr = w // 8
    t = np.arange(IMAGE_ROWS * (vpr + 1)).reshape(IMAGE_ROWS, vpr + 1)
    owned = t < items * CHAIN_THREADS                                               # (image row, item) -> some thread has it
    col_owned = np.concatenate([np.repeat(owned[:, :vpr], 8, axis=1), owned[:, vpr:]], axis=1)      # per column 0 .. w
    reach = min(1 + hx + reach_shift, w) if hx > 0 else 0
    for z0 in range(1, zlim, CHAIN_FRAMES):
        nframes = min(CHAIN_FRAMES, zlim - z0)
        for y0 in range(0, Y, STRIP_ROWS):
            ys = y0 - CHAIN_FRAMES + np.arange(IMAGE_ROWS)                          # image row i <-> volume row y0 - K + i
            on = (ys >= 0) & (ys < Y)
            img = [np.full((IMAGE_ROWS, w + 2), fill, np.uint32) for _ in range(2)]    # columns -1 .. w

            def load(image, frame, rows_mask):
                sel = np.flatnonzero(rows_mask)
                part = np.zeros((len(sel), w + 1), np.uint32)
                part[:, :w] = frame[ys[sel], :w]
                if w < X:
                    part[:, w] = frame[ys[sel], w]
                keep = col_owned[sel]
                image[sel, 1:] = np.where(keep, part, image[sel, 1:])
            load(img[0], out[z0 - 1], on)
            cur = 0
            for j in range(nframes):
                z = z0 + j
                h = min(max(nframes - 1 - j + halo_shift, 0), CHAIN_FRAMES - 1)
                active = on & (ys >= y0 - h) & (ys < y0 + STRIP_ROWS + h)
                A, B = img[cur], img[cur ^ 1]
                new = B.copy()
                load(new, enc[z], active)
                rows = np.flatnonzero(active & (ys >= 1) & (ys <= Y - 2))
                if len(rows) and reach > 1:
                    dec = (new[rows, 2:reach + 1] + _mean9(A, rows, 1, reach)) & 0xffff
                    new[rows, 2:reach + 1] = np.where(col_owned[rows, 1:reach], dec, B[rows, 2:reach + 1])
                img[cur ^ 1] = new
                own = np.flatnonzero(active & (ys >= y0) & (ys < y0 + STRIP_ROWS))
                keep = col_owned[own, :w]
                out[z, ys[own], :w] = np.where(keep, new[own, 1:w + 1], out[z, ys[own], :w]).astype(np.uint16)
                cur ^= 1
    return out
