"""Inputs of the stage cases of tests/golden/ref_stages.json and of the frame_shuffle / tile_shuffle cases of
tests/golden/ref_shuffles.json, regenerated from their seeds.  numpy only: the GPU tests that hold the product against the reference's
goldens import this and nothing of the oracle."""
import numpy as np


def np_dtype(name):
    """the array type a case's dtype name travels in ("char" is the tail-filter form: the same bytes, read as signed)"""
    return np.uint16 if name == "uint16" else np.uint8


def stage_input(kind, dtype, shape, seed):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    top = int(np.iinfo(dtype).max)
    n = int(np.prod(shape))
    if kind == "random":                                   # full range: the 3x3 sums wrap in the voxel type
        return rng.integers(0, top + 1, shape, dtype=dtype)
    if kind == "max":
        return np.full(shape, top, dtype)
    if kind == "zero":
        return np.zeros(shape, dtype)
    if kind == "ramp":
        return (np.arange(n) % (top + 1)).astype(dtype).reshape(shape)
    if kind == "pm128":                                    # bytes around +-128 when read as `char`
        return rng.integers(120, 137, shape).astype(dtype)
    if kind == "two_level":                                # 10 everywhere, 200 at every 7th voxel behind a first frame that is all 10
        v = np.full(n, 10, dtype)
        v[::7] = 200
        v = v.reshape(shape)
        v[0] = 10
        return v
    if kind == "gamma":
        return np.minimum(rng.gamma(2.0, 30.0, shape), top).astype(dtype)
    if kind == "equal_faces":                              # every face the estimator samples holds one value: four equal supports
        v = rng.integers(37, 200, shape).astype(dtype)
        v[0] = v[-1] = 37
        v[:, 0, :] = v[:, -1, :] = 37
        return v
    if kind == "low80":
        return rng.integers(0, 80, shape).astype(dtype)
    if kind == "near_wrap":                                # around 70000 mod 2^bits (4464 / 112): 4 in 13 below it
        lo = (70000 % (top + 1)) - 40
        return rng.integers(lo, lo + 130, shape).astype(dtype)
    if kind == "planted":                                  # 200 everywhere, single voxels and pairs of 10 next to the tile seams
        v = np.full(n, min(200, top), dtype)
        singles, pairs = planted_sites(shape, seed)
        Z, Y, X = shape
        for z, y, x in singles + [s for p in pairs for s in p]:
            v[(z * Y + y) * X + x] = 10
        return v.reshape(shape)
    if kind == "spread":
        return spread(dtype, shape, rng)
    raise KeyError(kind)


# ---- planted: rmbkrd_neighbor5x5x5 at the seams of its kernel's tiles ---------------------------------------------------------------------
# bkrd_neighbor5_kernel cuts the volume into columns of 64 (x) by 16 (y) voxels and walks them in chunks of 64 frames: a count that is not
# carried from one tile or chunk into the next shows at the centres within two voxels of a seam
PLANTED_SEAMS = {"z": (64, 128), "y": (16,), "x": (64, 128)}


def _near(seams, extent):
    """s - 3 .. s + 2 for every seam s: 61..66 and 125..130, or 13..18 (the voxels that exist); every voxel of an axis too short for a seam"""
    c = [s + d for s in seams for d in range(-3, 3) if s + d < extent]
    return c if c else list(range(extent))


def planted_sites(shape, seed):
    """(singles, pairs) of (z, y, x): voxels whose coordinates all come from _near(), taken in the seed's order as long as the 125 flat
    neighbours of one share no voxel with those of another -- a centre then counts at most one single.  Every second site tries to become
    a pair: a partner one or two voxels away (towards the seams as the seed has it), whose neighbours it shares; a centre near a pair
    counts one or two."""
    Z, Y, X = shape
    YX = Y * X
    rng = np.random.default_rng(seed)
    cand = [(z, y, x) for z in _near(PLANTED_SEAMS["z"], Z) for y in _near(PLANTED_SEAMS["y"], Y) for x in _near(PLANTED_SEAMS["x"], X)]
    inside = set(cand)
    # two voxels share a neighbour exactly when their flat distance is a difference of two of the 125 offsets
    shared = {dz * YX + dy * X + dx for dz in range(-4, 5) for dy in range(-4, 5) for dx in range(-4, 5)}
    flat = lambda s: (s[0] * Y + s[1]) * X + s[2]
    steps = [(1, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 1), (2, 0, 0), (0, 0, 2), (1, 1, 1), (2, 0, 2)]
    taken, singles, pairs = [], [], []
    free = lambda s: all(flat(s) - t not in shared for t in taken)
    for k in rng.permutation(len(cand)):
        s = cand[k]
        if not free(s):
            continue
        mate = None
        if (len(singles) + len(pairs)) % 2 == 1:
            for j in rng.permutation(len(steps)):
                m = tuple(a + b for a, b in zip(s, steps[j]))
                if m in inside and free(m):
                    mate = m
                    break
        if mate is None:
            singles.append(s)
            taken.append(flat(s))
        else:
            pairs.append((s, mate))
            taken += [flat(s), flat(mate)]
    return singles, pairs


# ---- spread: rmestbkrd's face histograms away from one narrow band ------------------------------------------------------------------------
# bkrd_face_histo_kernel counts every 256 voxels of a face into a window of 16384 bins around the first of them: these first values sit at
# the window's switch (8192 / 8193), in the open (40000) and at its clamp (57343 / 57344 / 65535)
SPREAD_STARTS = (8192, 8193, 40000, 57343, 57344, 65535)


def spread(dtype, shape, rng):
    """the interior over the whole range; every face the estimator samples cut into segments of 256 voxels: segment k starts with
    SPREAD_STARTS[k % 6] exactly (8-bit: that value >> 8), holds values within 4000 (15) of it and, where the range has room, two voxels
    more than 8192 below and two more than 8192 above it.  The rows y = Y-1 take the first three starts only, so that their support --
    the smallest of the four -- lies in the middle of the range."""
    Z, Y, X = shape
    top = int(np.iinfo(dtype).max)
    wide = top > 255
    v = rng.integers(0, top + 1, shape).astype(np.int64)
    flat = v.reshape(-1)

    def fill(base, length, starts, k0):
        for k, a in enumerate(range(0, length, 256)):
            L = min(256, length - a)
            s = starts[(k0 + k) % len(starts)] >> (0 if wide else 8)
            seg = s + rng.integers(-4000, 4001, L) // (1 if wide else 256)
            seg = np.where(seg > top, 2 * top - seg, np.abs(seg))                    # folded back into the range, not piled up at its ends
            seg[0] = s
            if wide and L >= 8:
                at = 1 + rng.permutation(L - 1)[:4]
                if s - 8193 >= 0:
                    seg[at[:2]] = rng.integers(0, s - 8192, 2)
                if s + 8193 <= top:
                    seg[at[2:]] = rng.integers(s + 8193, top + 1, 2)
            flat[base + a:base + a + L] = seg

    fill(0, Y * X, SPREAD_STARTS, 0)
    fill((Z - 1) * Y * X, Y * X, SPREAD_STARTS, 3)
    for i, z in enumerate((1, Z // 2, Z - 2)):
        if 0 < z < Z - 1:
            fill(z * Y * X, X, SPREAD_STARTS, 2 * i + 1)
            fill(z * Y * X + (Y - 1) * X, X, SPREAD_STARTS[:3], i)
    return v.astype(dtype)


def stage_volume(case):
    return stage_input(case["kind"], np_dtype(case["dtype"]), tuple(case["shape"]), case["seed"])


def stage_tile(case):
    """tile_size of a reorder case; None in the table means the stage's default, 16 / sizeof(T)"""
    ts = case["params"].get("tile_size")
    return ts if ts else 16 // np.dtype(np_dtype(case["dtype"])).itemsize


# ---- frame_shuffle / tile_shuffle: tests/golden/ref_shuffles.json ---------------------------------------------------------------------
# A volume is built unit by unit -- a unit is what the stage sorts: frame_chunk_size frames, or one tile -- so that a kind can say what
# the units' metrics do.  Values are made as int64 inside the voxel type's range; dtype "char" (the tail-filter form) is signed and travels
# as the uint8 array of the same bytes.
TWO24 = 1 << 24


def tiles_to_volume(tiles, shape, ts):
    """tiles (ntiles, ts^3) in (z, y, x) tile order, row-major inside a tile -> the volume they are cut from"""
    z, y, x = shape
    return np.ascontiguousarray(tiles.reshape(z // ts, y // ts, x // ts, ts, ts, ts).transpose(0, 3, 1, 4, 2, 5).reshape(shape))


def _with_sum(rng, per, total, lo, hi):
    """`per` small values in [lo, hi] that add up to `total` (|total| <= per): zeros, |total| ones of its sign, and a few +2 / -2 pairs"""
    v = np.zeros(per, np.int64)
    at = rng.permutation(per)
    v[at[:abs(total)]] = 1 if total > 0 else -1
    free = at[abs(total):]
    pairs = min(len(free) // 2, 3)
    if lo <= -2 and hi >= 2:
        v[free[:pairs]] = 2
        v[free[pairs:2 * pairs]] = -2
    assert int(v.sum()) == total
    return v


def shuffle_units(kind, dtype, units, per, seed):
    """(units, per) int64 values of a kind; dtype is the case's name for it ("uint16", "uint8", "char")"""
    rng = np.random.default_rng(seed)
    lo, hi = (-128, 127) if dtype == "char" else (0, int(np.iinfo(np_dtype(dtype)).max))
    span = hi - lo + 1
    if kind == "random":                                   # full range
        return rng.integers(lo, hi + 1, (units, per))
    if kind == "ramp":
        return lo + (np.arange(units * per) % span).reshape(units, per)
    if kind == "descending":                               # every unit's values lie below those of the unit in front of it
        w = max(span // units, 1)
        base = np.maximum(hi + 1 - w * (1 + np.arange(units)), lo)
        return base[:, None] + rng.integers(0, w, (units, per))
    if kind == "all_equal":                                # one unit, repeated: every metric ties, the map is all zeros
        return np.tile(rng.integers(lo, hi + 1, per), (units, 1))
    if kind == "two_groups":                               # A B A B ...: B lies below A, so the map is all 1s, then all 0s
        a, b = rng.integers(lo + span // 2, hi + 1, per), rng.integers(lo, lo + span // 2, per)
        return np.stack([a if u % 2 == 0 else b for u in range(units)])
    if kind == "permuted":                                 # even units: the same voxels in another order, sums below 2^24 -- equal in metric
        top = min(hi, max(TWO24 // per - 1, 1))            # whatever the order of the additions, and different in content
        base = rng.integers(max(lo, -top), top + 1, per)
        return np.stack([rng.permutation(base) if u % 2 == 0 else rng.integers(max(lo, -top), top + 1, per) for u in range(units)])
    if kind == "pm128":                                    # bytes around +-128 when read as `char`: 120 .. 127 and -128 .. -120
        return (rng.integers(120, 137, (units, per)) + 128) % 256 - 128
    if kind == "neg_means":                                # signed: every unit's mean is negative, the means differ
        return np.stack([rng.integers(-128, -(u * 5 % 60), per) for u in range(units)])
    if kind == "extremes":                                 # signed: means of exactly -128, 127 and 0, each more than once, and noise
        rows = [np.full(per, -128), np.full(per, 127), np.zeros(per, np.int64), None]
        return np.stack([rows[u % 4] if rows[u % 4] is not None else rng.integers(-128, 128, per) for u in range(units)])
    if kind == "fraction":                                 # tiles: means m + j / per with m one of two integers: they differ in the fraction only,
        out = np.empty((units, per), np.int64)             # truncate to m or m + 1, and every tile takes the first of its group
        for u in range(units):
            out[u] = 100 + (u % 3 == 2)
            out[u, rng.permutation(per)[:(u * 7 + 1) % per]] += 1
        return out
    if kind == "integer_edge":                             # tiles: even units sum to m * per - 1 (truncates to m - 1), odd ones to m * per; m grows
        out = np.empty((units, per), np.int64)             # by one per pair, so an even unit ties with the odd unit in front of it
        for u in range(units):
            m = 50 + u // 2
            out[u] = m
            at = rng.permutation(per)
            pairs = per // 4
            out[u, at[:pairs]] += 1
            out[u, at[pairs:2 * pairs]] -= 1
            if u % 2 == 0:
                out[u, at[-1]] -= 1
        return out
    if kind == "trunc_zero":                               # signed tiles: sums in (-per, 0), 0, in (0, per) -- all truncate toward zero and tie --
        out = np.empty((units, per), np.int64)             # and sums of exactly -per and per, which do not
        for u in range(units):
            k = 1 + (u * 3) % (per - 1)
            out[u] = (_with_sum(rng, per, -k, lo, hi), np.zeros(per, np.int64), _with_sum(rng, per, k, lo, hi), np.full(per, -1), np.full(per, 1))[u % 5]
        return out
    raise KeyError(kind)


def shuffle_param(case):
    return case["frame_chunk_size"] if case["stage"] == "frame_shuffle" else case["tile_size"]


def shuffle_whole(case):
    """True when the shape is a whole number of units: every other shape is refused"""
    z, y, x = case["shape"]
    p = shuffle_param(case)
    return z % p == 0 if case["stage"] == "frame_shuffle" else all(d >= p and d % p == 0 for d in (z, y, x))


def shuffle_volume(case):
    """the volume of a case of ref_shuffles.json.  A shape with a remainder is built frame by frame: it has no units"""
    shape = tuple(case["shape"])
    z, y, x = shape
    p = shuffle_param(case)
    if case["stage"] == "tile_shuffle" and shuffle_whole(case):
        v = tiles_to_volume(shuffle_units(case["kind"], case["dtype"], (z // p) * (y // p) * (x // p), p ** 3, case["seed"]), shape, p)
    else:
        chunk = p if shuffle_whole(case) else 1
        v = shuffle_units(case["kind"], case["dtype"], z // chunk, chunk * y * x, case["seed"]).reshape(shape)
    return v.astype(np.int8).view(np.uint8) if case["dtype"] == "char" else v.astype(np_dtype(case["dtype"]))


def shuffle_case_id(case, index):
    return "%s-%s-%s-%s-p%d-%03d" % (case["stage"], case["dtype"], "x".join(str(d) for d in case["shape"]), case["kind"], shuffle_param(case), index)


def load_shuffle_cases(path):
    """(_meta, cases, expected maps of tests/frame_metric_cases.py by name) of tests/golden/ref_shuffles.json"""
    import json
    with open(path) as f:
        gold = json.load(f)
    for i, c in enumerate(gold["cases"]):
        c["id"] = shuffle_case_id(c, i)
    return gold["_meta"], gold["cases"], gold["frame_metric_cases"]


def case_id(case, index):
    return "%s-%s-%s-%s-%03d" % (case["stage"], case["dtype"], "x".join(str(d) for d in case["shape"]), case["kind"], index)


def load_cases(path):
    """(_meta, cases) of tests/golden/ref_stages.json; the file leaves out what follows from the rest: empty params, and the ids"""
    import json
    with open(path) as f:
        gold = json.load(f)
    for i, c in enumerate(gold["cases"]):
        c.setdefault("params", {})
        c["id"] = case_id(c, i)
    return gold["_meta"], gold["cases"]
