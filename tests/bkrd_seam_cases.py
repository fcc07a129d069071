"""Constructed inputs for the seams of the background-removal kernels (bkrd_neighbor5_kernel, bkrd_face_histo_kernel, bkrd_support_kernel),
with their expectations: numpy only, so that tests/test_background_host.py can hold the constructions themselves to what they claim
without a GPU, and tests/test_gpu_background_seams.py runs them.

rmbkrd_neighbor5x5x5: a workgroup owns a 64 (x) by 16 (y) column and walks it in chunks of 64 frames with a ring of five planes, so the
seams lie at x = 64, 128, y = 16 and z = 64, 128.  The expectation is the DIRECT count (bkrd_restate.neighbor5_counts_direct), not the
separated box sum the kernel shares with bkrd_restate.neighbor5_counts.
rmestbkrd: every 256 voxels of a face are counted in a window of 16384 bins around the first of them; a face of more than 32768 voxels
takes a second pass of the 128 workgroups; the support walk gives every thread 256 bins (16-bit) or one (8-bit)."""
import numpy as np

import bkrd_restate as R
from ref_stage_inputs import PLANTED_SEAMS, planted_sites, stage_input

# ---- rmbkrd_neighbor5x5x5: planted voxels ---------------------------------------------------------------------------------------------------
PLANTED_THRESHOLD = 100
# cut = 0: one neighbour below the level zeroes a centre.  cut = 0.0081f * 124.f = 1.0044: one keeps it, two zero it
PLANTED_FRACTIONS = (0.0, 0.0081)
# (shape, seeds): every seam with all its outcomes (test_background_host.py::test_planted_volumes_reach_every_seam)
PLANTED = [((136, 18, 134), tuple(range(8))), ((70, 20, 68), (0, 1, 2, 3, 11, 21))]


def neighbor5_direct(vol, threshold, fraction):
    """(what rmbkrd_neighbor5x5x5 leaves of vol, the counts): bkrd_restate.neighbor5 with the direct count in place of the box sums"""
    n = R.neighbor5_counts_direct(vol, threshold)
    cut = np.float32(fraction) * np.float32(124)
    keep = R.neighbor5_centres(vol.shape) & (vol >= threshold) & ~(n.astype(np.float32) > cut)
    return np.where(keep, vol, 0).astype(vol.dtype), n


def planted_voxels(shape, seed):
    singles, pairs = planted_sites(shape, seed)
    return singles + [s for p in pairs for s in p]


def first_difference(got, want, n):
    """None, or (z, y, x, got, want, n) of the first voxel that differs"""
    at = np.argwhere(got != want)
    if not at.size:
        return None
    z, y, x = (int(c) for c in at[0])
    return z, y, x, int(got[z, y, x]), int(want[z, y, x]), int(n[z, y, x])


def seams_of(shape):
    """{(axis, s): sides} of the kernel's seams inside a volume; sides: "low" (s-2, s-1), "high" (s, s+1) where the band holds centres"""
    centres = R.neighbor5_centres(shape)
    out = {}
    for a, axis in enumerate("zyx"):
        for s in PLANTED_SEAMS[axis]:
            if s >= shape[a]:
                continue
            sides = [side for side, (lo, hi) in (("low", (s - 2, s)), ("high", (s, s + 2))) if np.take(centres, range(lo, min(hi, shape[a])), axis=a).any()]
            if sides:
                out[(axis, s)] = sides
    return out


def seam_outcomes(vol, seed, fraction):
    """the (axis, s, side, outcome) that a planted volume shows, by the direct count.  outcome "kept": a centre of the band that keeps its
    value (above cut 0: with a planted voxel of the other side among its neighbours).  outcome "zeroed": a centre of the band that is
    zeroed and would be kept without the planted voxels on the OTHER side of the seam -- a count that is not carried across the seam
    shows there as a kept voxel."""
    shape = vol.shape
    cut = np.float32(fraction) * np.float32(124)
    want, n = neighbor5_direct(vol, PLANTED_THRESHOLD, fraction)
    centres = R.neighbor5_centres(shape) & (vol >= PLANTED_THRESHOLD)
    planted = planted_voxels(shape, seed)
    seen = set()
    for (axis, s), sides in seams_of(shape).items():
        a = "zyx".index(axis)
        coord = np.arange(shape[a]).reshape([-1 if k == a else 1 for k in range(3)])
        for side in sides:
            band = centres & ((coord >= s - 2) & (coord < s) if side == "low" else (coord >= s) & (coord < s + 2))
            own = vol.copy()                                # without the planted voxels of the other side
            for p in planted:
                if (p[a] >= s) == (side == "low"):
                    own[p] = 200
            n_own = R.neighbor5_counts_direct(own, PLANTED_THRESHOLD)
            # kept: with cut 0 no neighbour at all; above it, kept although a planted voxel of the other side is counted
            if (band & (want != 0) & ((n > n_own) if cut >= 1 else True)).any():
                seen.add((axis, s, side, "kept"))
            if (band & (want == 0) & ~(n_own.astype(np.float32) > cut)).any():
                seen.add((axis, s, side, "zeroed"))
    return seen


def seam_outcomes_wanted(shape):
    return {(axis, s, side, o) for (axis, s), sides in seams_of(shape).items() for side in sides for o in ("kept", "zeroed")}


# ---- rmbkrd_neighbor5x5x5: chunk ends ---------------------------------------------------------------------------------------------------------
# z_end = max(2, min(X - 2, Z)) is Z or X - 2: the chunk that starts at 64 (128) holds 1, 2, 3 or 4 planes of centres whose neighbours
# run past the volume's end (not counted: the product's own rule), then a plane behind z_end; the last two shapes have z_end = 64 (128),
# so that their last chunk holds no centre at all and is zero-filled
CHUNK_END_SHAPES = [(Z, 6, 70) for Z in (65, 66, 67, 68, 69)] + [(Z, 6, 135) for Z in (128, 129, 130, 131)] + [(70, 6, 66), (131, 6, 130)]
CHUNK_END_CONFIGS = ((36, 0.5), (18, 0.25))


def chunk_end_volume(shape, dtype):
    return stage_input("low80", dtype, shape, sum(shape))


# ---- rmestbkrd: the histogram window ----------------------------------------------------------------------------------------------------------
L2_ALL = 1 << 30                                         # host_l2_bytes above every frame here: the z faces are whole frames
WINDOW_SHAPE = (4, 40, 520)                              # a y-face row spans three workgroups; 81.25 segments per z face
STRIDE_SHAPE = (3, 130, 260)                             # 33800 voxels per z face: 128 workgroups of 256 take a second pass
# portion = int(l2 * .75) only where the frame holds MORE voxels than l2 has bytes: 32768 and 32769 need l2 = 43691 and 43692, and so a
# frame of more than 43692 voxels
PORTION_SHAPE = (3, 170, 260)
PORTION_L2 = {32768: 43691, 32769: 43692}
WIN, BINS16 = 16384, 65536


def spread_volume(shape, dtype, seed=5100):
    return stage_input("spread", dtype, shape, seed)


def face_segments(vol, l2):
    """(face, piece, voxels) for every 256-voxel segment a workgroup of bkrd_face_histo_kernel starts on (its first pass); piece: the frame
    or the row the segment is cut from"""
    Z, Y, X = vol.shape
    flat = vol.reshape(-1)
    frame = Y * X
    p = R.face_portion(frame, l2)
    pieces = [(0, flat[:p]), (1, flat[(Z - 1) * frame:(Z - 1) * frame + p])]
    pieces += [(2, vol[z, 0]) for z in (1, Z // 2, Z - 2)] + [(3, vol[z, Y - 1]) for z in (1, Z // 2, Z - 2)]
    return [(face, i, piece[a:a + 256]) for i, (face, piece) in enumerate(pieces) for a in range(0, len(piece), 256)]


def window_base(v0):
    """where the kernel puts the window of a segment that starts with v0 (16-bit)"""
    return min(v0 - WIN // 2, BINS16 - WIN) if v0 > WIN // 2 else 0


# ---- rmestbkrd: the support walk ----------------------------------------------------------------------------------------------------------------
SUPPORT_SHAPE = (5, 10, 100)                             # z faces of 1000 voxels, y faces of 3 rows of 100
SUPPORT_BINS = {np.uint16: (0, 1, 255, 256, 257, 16384, 65535), np.uint8: (0, 1, 128, 255)}


def support_cases(dtype):
    """(lo, hi, k): the faces hold 1000 - k voxels of lo and k of hi.  k = 10: 990 / 1000 is not above (double)0.99f, the walk stops at hi.
    k = 9: 991 / 1000 is, it stops at lo.  For every bin m of SUPPORT_BINS and both gaps (1: bins[m-1] is the other value, and for
    m = 256 another thread's bin; 3: bins[m-1] is empty) the value pairs (m - gap, m) and (m, m + gap), each with both k."""
    top = int(np.iinfo(dtype).max)
    cases = []
    for m in SUPPORT_BINS[dtype]:
        for gap in (1, 3):
            for lo, hi in ((m - gap, m), (m, m + gap)):
                for k in (10, 9):
                    if lo >= 0 and hi <= top and (lo, hi, k) not in cases:
                        cases.append((lo, hi, k))
    return cases


def support_crossing(lo, hi, k):
    """the bin the walk is meant to stop at"""
    return hi if k == 10 else lo


def support_threshold(lo, hi, k):
    """the threshold the volume is meant to produce, from the faces' counts (z faces 1000 - k and k, y faces 297 and 3 or 298 and 2) in
    the reference's arithmetic, float(uint32 numerator) / float(denominator), truncated: k = 9 stops at lo with bins[lo-1] empty, the
    support is lo but for binary32's rounding of bins[lo] * lo; k = 10 stops at hi, the support is hi where bins[hi-1] is empty and
    hi - 0.99 where it holds the other 99 %"""
    m = support_crossing(lo, hi, k)
    if m == 0:
        return 0
    supports = []
    for total, minority in ((1000, k), (300, 3 if k == 10 else 2)):
        here = minority if k == 10 else total - minority
        below = total - minority if k == 10 and lo == hi - 1 else 0
        supports.append(np.float32(np.uint32((here * m + below * (m - 1)) & 0xffffffff)) / np.float32(here + below))
    return int(min(supports))


def support_volume(dtype, lo, hi, k):
    """z faces: 1000 - k voxels of lo and k of hi; y faces (rows y = 0 and Y-1 of frames 1, 2, 3): 99 of lo and one of hi per row for
    k = 10 (297 / 300 = 0.99), the last row all lo for k = 9 (298 / 300).  Interior: threshold - 1 .. threshold + 2 and any value."""
    Z, Y, X = SUPPORT_SHAPE
    top = int(np.iinfo(dtype).max)
    rng = np.random.default_rng(lo * 31 + hi * 7 + k)
    v = np.empty(SUPPORT_SHAPE, np.int64)
    t = support_threshold(lo, hi, k)
    inner = np.stack([np.full(Z * Y * X // 5, t - 1), np.full(Z * Y * X // 5, t), np.full(Z * Y * X // 5, t + 1), np.full(Z * Y * X // 5, t + 2),
                      rng.integers(0, top + 1, Z * Y * X // 5)], axis=1)
    v[:] = np.clip(inner, 0, top).reshape(SUPPORT_SHAPE)
    for z in (0, Z - 1):
        face = np.full(Y * X, lo)
        face[rng.permutation(Y * X)[:k]] = hi
        v[z] = face.reshape(Y, X)
    for i, z in enumerate((1, Z // 2, Z - 2)):
        for y in (0, Y - 1):
            v[z, y] = lo
            if k == 10 or i < 2:
                v[z, y, rng.integers(0, X)] = hi
    return v.astype(dtype)
