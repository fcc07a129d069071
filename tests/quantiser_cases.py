"""Named, seeded 16-bit volumes for the quantiser's LUTs (default weighting unless a test says otherwise), each with the property it is
here for, and a small numpy restatement of the walk whose float type, rounding rule and total are parameters -- so that the property
is checked (tests/test_oracle_reference_quantiser.py), not claimed.  Plain module, numpy only.

Why these.  The Lloyd walk (the reference's encoders/quantiser_utils.hpp:227-284) is float arithmetic whose result must be byte-exact.
While every `raw_idx * count` and every bucket's weighted sum stays below 2^24 all products and sums are exact integers and only the
divisions round: a walk with a fused multiply-add, a double accumulator, rintf for roundf, a division by reciprocal or a float-summed
total gives the same tables.  The families:
  rounding   bins near the top of the range with hundreds of voxels each: raw_idx * count and the weighted sums pass 2^24, so binary32
             rounds them; a walk in binary64 gives other tables
  ties       pairs of adjacent bins with equal counts: the mean of a bucket of whole pairs lies on .5.  Pairs that start on an even bin
             (from 1000 with 6 voxels, from 40000 with 40) put those means on even + .5, where round-half-away and round-half-even
             part.  Pairs from the odd bin 40001 put every one of them on odd + .5, where the two rules agree: that set holds the walk
             to rounding a half upwards at all (truncation and round-half-down part there), not to the choice between the two rules
  boundary   255 .. 258 occupied bins, packed and at the top of the range: the last cases of the linear mapping, the first of the walk;
             bin 65535 / bin 65534 occupied with at most 256 levels: the decode table's tail
  histogram  tiles of one job in different quarters of the value range, voxels on both sides of 16384 and 49152 (the histogram kernel
             counts a tile's most voted quarter in LDS, the rest in global memory); a job of more than one tile with len % 8 == 7
  big        a bin with 2^24 + 1 voxels (its float count rounds) next to a thin band: a total summed in binary32 gives other tables
"""
import numpy as np

TILE_VOXELS = 32768                # a workgroup of the batch histogram and look-up kernels takes this many voxels of one job
LEVELS = 256


def _shuffled(values, shape, seed):
    v = np.asarray(values, dtype=np.uint16)
    assert v.size == int(np.prod(shape)), (v.size, shape)
    return np.random.default_rng(seed).permutation(v).reshape(shape)


def _from_counts(bins, counts, shape, seed):
    return _shuffled(np.repeat(np.asarray(bins, dtype=np.int64), np.asarray(counts, dtype=np.int64)), shape, seed)


def _uniform(lo, hi, shape, seed):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.uint16)


def _gauss(mean, sigma, shape, seed):
    return np.clip(np.rint(np.random.default_rng(seed).normal(mean, sigma, shape)), 0, 65535).astype(np.uint16)


def _pairs(first, voxels, shape, seed):
    """300 pairs of adjacent bins, a pair every 4 bins from `first`, `voxels` voxels in every bin"""
    bins = np.array([[first + 4 * i, first + 4 * i + 1] for i in range(300)]).reshape(-1)
    return _from_counts(bins, np.full(bins.size, voxels), shape, seed)


def _levels_packed(levels, seed):
    i = np.arange(levels)
    counts = 3 + i % 5
    return _from_counts(1000 + i, counts, (1, 1, int(counts.sum())), seed)


def _levels_top(levels, seed):
    i = np.arange(levels)
    counts = 1 + i % 3
    return _from_counts(65535 - i, counts, (1, 1, int(counts.sum())), seed)


def _top_bin(top, seed):
    """77 levels: 76 bins of 5 voxels from bin 17, every 200, and 9 voxels in `top`"""
    bins = np.append(17 + 200 * np.arange(76), top)
    counts = np.append(np.full(76, 5), 9)
    return _from_counts(bins, counts, (1, 1, int(counts.sum())), seed)


def _quarter_tiles(seed):
    """three tiles of one job: the first mostly in quarter 0 with voxels on 16383 and 16384, the second in quarter 1 with the same two
    and some of quarter 3, the third in quarter 3 with voxels on 49151 and 49152 -- whichever quarter a tile votes for, voxels of the same
    bins are counted through LDS by one tile and through global memory by another"""
    rng = np.random.default_rng(seed)
    n = TILE_VOXELS
    t0 = rng.integers(15800, 16384, n)
    t1 = rng.integers(16384, 17000, n)
    t2 = rng.integers(49152, 49700, n)
    for t, edge in ((t0, (16383, 16384)), (t1, (16383, 16384, 49151, 49152)), (t2, (49151, 49152))):
        at = rng.choice(n, 400 * len(edge), replace=False)
        t[at] = np.tile(edge, 400)
    t1[rng.choice(n, 3000, replace=False)] = rng.integers(60000, 60400, 3000)
    return np.concatenate([t0, t1, t2]).astype(np.uint16).reshape(3, 128, 256)


def _big(seed):
    """exactly 2^24 + 1 voxels of value 500 (an odd count above 2^24: no binary32 holds it) and 70000 voxels of [300, 1500) without 500"""
    rng = np.random.default_rng(seed)
    v = np.full((1 << 24) + 1 + 70000, 500, dtype=np.uint16)
    band = rng.integers(300, 1499, 70000)
    v[rng.choice(v.size, 70000, replace=False)] = band + (band >= 500)
    return v.reshape(27, 4489, 139)


ROUNDING, TIES, BOUNDARY, HISTOGRAM, BIG = "rounding", "ties", "boundary", "histogram", "big"

# name -> (family, builder)
_TABLE = [
    ("uniform_60000", ROUNDING, lambda: _uniform(60000, 60600, (16, 128, 128), 9001)),
    ("uniform_50000", ROUNDING, lambda: _uniform(50000, 50600, (16, 128, 128), 9002)),
    ("gauss_61000", ROUNDING, lambda: _gauss(61000, 150, (16, 128, 128), 9003)),
    ("pairs_1000_x6", TIES, lambda: _pairs(1000, 6, (4, 30, 30), 9004)),
    ("pairs_40001_x40", TIES, lambda: _pairs(40001, 40, (8, 50, 60), 9005)),
    ("pairs_40000_x40", TIES, lambda: _pairs(40000, 40, (8, 50, 60), 9006)),
] + [("levels_%d_packed" % n, BOUNDARY, lambda n=n: _levels_packed(n, 9010 + n)) for n in (255, 256, 257, 258)] + [
    ("levels_%d_top" % n, BOUNDARY, lambda n=n: _levels_top(n, 9020 + n)) for n in (255, 256, 257, 258)] + [
    ("bin_65535_occupied", BOUNDARY, lambda: _top_bin(65535, 9030)),
    ("bin_65534_occupied", BOUNDARY, lambda: _top_bin(65534, 9031)),
    ("quarter_tiles", HISTOGRAM, lambda: _quarter_tiles(9040)),
    ("two_tiles_tail_7", HISTOGRAM, lambda: _uniform(20000, 21000, (3, 13, 841), 9041)),
    ("count_above_2p24", BIG, lambda: _big(9050)),
]
NAMES = [t[0] for t in _TABLE]
FAMILY = {t[0]: t[1] for t in _TABLE}
SMALL = [n for n in NAMES if FAMILY[n] != BIG]          # everything but the big one: at most 2^18 voxels each
_cache = {}


def volume(name):
    """the case's volume (uint16, three axes); built once, read-only"""
    if name not in _cache:
        v = dict((t[0], t[2]) for t in _TABLE)[name]()
        assert v.dtype == np.uint16 and v.ndim == 3 and (FAMILY[name] == BIG or v.size <= 1 << 18), name
        v.setflags(write=False)
        _cache[name] = v
    return _cache[name]


def names(*families):
    return [n for n in NAMES if FAMILY[n] in families]


def histogram(v):
    return np.bincount(np.asarray(v).reshape(-1), minlength=65536).astype(np.uint32)


# the ties whose two roundings differ: the sets whose pairs start on an even bin
TIES_EVEN_START = ("pairs_1000_x6", "pairs_40000_x40")


def _round(x, rule):
    if rule == "even":
        return np.rint(x)
    if rule == "down":                                   # a half goes down, everything else to nearest
        return np.ceil(x - 0.5)
    assert rule == "away"
    t = np.trunc(x)                                      # (x >= 0 here)
    return t + 1 if x - t >= 0.5 else t


def walk(histo, ftype=np.float32, rounding="away", total="double"):
    """(lut_encode uint8[65536], lut_decode uint16[256]) of the default weighting from a 65536-bin histogram: setup_com's choice between
    linear_mapping_quantisation and adaptive_lloyd_com (quantiser_utils.hpp:400-415, :286-306, :227-284) in the reference's statement
    order.  The reference is walk(float32, "away", "double"): importance, sums, products, quotients in binary32, std::round, and the one
    total accumulated in double (std::accumulate with a 0. seed) before it is narrowed.  The other settings are the wrong walks:
      ftype=float64     every value of the walk in binary64
      rounding="even"   rint for round ("down": a half rounds towards zero)
      total="float32"   the total accumulated in binary32, bin by bin
    An empty bin that does not close a bucket leaves the state as it is (it adds 0 and recomputes the same mean): it is skipped."""
    f = ftype
    histo = np.asarray(histo, dtype=np.uint32)
    importance = histo.astype(np.float32).astype(f)       # importance_ is a std::vector<float>; f only widens what is computed from it
    enc = np.zeros(65536, np.uint8)
    dec = np.zeros(LEVELS, np.uint16)
    if total == "float32":
        acc = np.float32(0)
        for x in importance[importance != 0].astype(np.float32):
            acc = np.float32(acc + x)
        importance_sum = f(acc)
    else:
        importance_sum = f(np.float32(importance.astype(np.float64).sum())) if f is np.float32 else f(importance.astype(np.float64).sum())
    if not importance_sum != 0:
        return enc, dec
    occupied = importance != 0
    if int(occupied.sum()) <= LEVELS:
        comp = 0
        for raw in range(65536):
            if comp >= LEVELS:
                break
            enc[raw] = comp
            dec[comp] = raw
            if occupied[raw]:
                comp += 1
        if 0 < comp < LEVELS and dec[comp] == 65535:
            dec[comp:] = dec[comp - 1]
        return enc, dec
    levels_available = LEVELS
    bucket = f(importance_sum / f(levels_available))
    integral = quantile = importance[0]
    weighted = f(0) * importance[0]
    mean = f(0)
    comp = 0
    step = np.zeros(65536, np.int64)                      # 1 where the code goes up
    imp = list(importance)
    occ = occupied.tolist()
    for raw in range(1, 65536):
        closes = quantile >= bucket and comp < LEVELS - 1
        if not closes and not occ[raw]:
            continue
        x = imp[raw]
        if closes:
            dec[comp] = int(mean)
            comp += 1
            levels_available -= 1
            step[raw] = 1
            quantile = x
            weighted = f(f(raw) * x)
            if integral < importance_sum:
                bucket = f(f(importance_sum - integral) / f(levels_available))
        else:
            quantile = f(quantile + x)
            weighted = f(weighted + f(f(raw) * x))
        if quantile != 0:
            mean = f(_round(f(weighted / quantile), rounding))
        integral = f(integral + x)
    dec[comp] = int(mean)
    return np.cumsum(step).astype(np.uint8), dec


def first_difference(a, b):
    """index of the first entry in which two tables differ, or None"""
    d = np.flatnonzero(np.asarray(a) != np.asarray(b))
    return int(d[0]) if d.size else None
