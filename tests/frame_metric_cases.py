"""Named frames for the metric of frame_shuffle / tile_shuffle -- a SEQUENTIAL binary32 sum, so the order of the additions is part of the
result once the sum passes 2^24 -- each with the property it is here for, and a numpy restatement of that sum in which the property is
checked (tests/test_frame_metric_host.py), not claimed.  Plain module, numpy only.  Nothing is taken from the product but the documented
geometry of its block-parallel evaluation: blocks of 4 KiB, 64 bytes per lane, 64 lanes.

How a sum becomes visible.  The metric never leaves the library, the reorder_map in the header does, and the map shows equality: frames
of equal metric all take the first such frame.  So a subject frame with reference sum R, ulp u = 2^k in R's binade, stands in a volume
with three witness frames whose sums are exactly R - u, R and R + u.  Every voxel of a witness is a multiple of 2^k and its sum never
passes 2^(24+k), so every partial sum of a witness is exact in binary32: no rounding logic touches a witness.  The expected map names
the subject and the R witness as one place with the other two on either side; a sum one ulp off in either direction ties with the wrong
witness or leaves the bracket, and the map changes.  That needs the three quotients by Y*X to be distinct: where the division would merge
neighbours (frame sizes that are no power of two) the subject is moved to a nearby sum where it does not -- a wider bracket would keep the
witnesses apart but not show a one-ulp error, so there is none.

Subjects are steered (steer()): the voxels in front of a chosen index are replaced by multiples of u, which add exactly, so that the
float sum in front of that index is a chosen value.  A case's claim is a predicate over the simulation (Sim): np.add.accumulate in float32,
read at block and lane boundaries, next to the integer prefix.

tile_shuffle truncates sum / tile voxels to the voxel type, so there a subject is steered to R = m * per_tile with a witness at R - u
(which truncates to m - 1), and a second one to R = m * per_tile - u with a witness at m * per_tile: a sum one ulp low in the first, one
ulp high in the second changes the truncated metric and the map."""
import numpy as np

BLOCK_BYTES = 4096                 # one block of the block-parallel evaluation
LANE_BYTES = 64                    # one lane's share of a block
PLANNED_MIN_BLOCKS = 16            # frames of at least this many blocks take the planned path (sums, records, chain)
TWO24 = 1 << 24

PLANNED, SCAN, SERIAL, SIGNED = "planned", "scan", "serial", "signed"
FRAME, CHUNK, TAIL, TILE = "frame", "chunk", "tail", "tile"


def geometry(dtype):
    """(voxels per block, voxels per lane and block)"""
    e = np.dtype(dtype).itemsize
    return BLOCK_BYTES // e, LANE_BYTES // e


def fcum(v):
    """the sequential binary32 sum after every voxel, as int64 (every partial sum is an integer below 2^40)"""
    return np.add.accumulate(np.asarray(v).astype(np.float32), dtype=np.float32).astype(np.int64)


def regime(s):
    """k with ulp 2^k at |s|: 0 below 2^24, else floor(log2 |s|) - 23 (elementwise)"""
    _, e = np.frexp(np.abs(np.asarray(s, dtype=np.float64)))          # |s| in [2^(e-1), 2^e)
    return np.maximum(e.astype(np.int64) - 24, 0)


def ulp(s):
    return 1 << int(regime(s))


class Sim:
    """the sequential float sum of one frame (voxel values as int64) next to its integer prefix, read at block and lane boundaries"""

    def __init__(self, values, dtype):
        self.v = np.asarray(values, dtype=np.int64)
        self.n = self.v.size
        self.blk, self.epl = geometry(dtype)
        self.cum = fcum(self.v)
        self.ip = np.cumsum(self.v)
        self.total = int(self.cum[-1])
        self.nb = -(-self.n // self.blk)

    def S(self, i):
        """the float sum in front of voxel i"""
        return int(self.cum[i - 1]) if i else 0

    def P(self, i):
        """the integer sum in front of voxel i"""
        return int(self.ip[i - 1]) if i else 0

    def where(self, i):
        """(block, lane, voxel of the lane) of voxel i"""
        return i // self.blk, (i % self.blk) // self.epl, i % self.epl

    def first_at_least(self, bound):
        """the first voxel after which the float sum is >= bound"""
        at = np.flatnonzero(self.cum >= bound)
        assert at.size, "the sum never reaches %d" % bound
        return int(at[0])

    def block_tot(self, b):
        return self.P(min((b + 1) * self.blk, self.n)) - self.P(b * self.blk)

    def guard_margin(self, b, start=None):
        """2^(e+1) - (S + tot + BLK * u / 2) at the start of block b, S the float sum there (or `start`): the block-parallel evaluation is
        taken while this is positive"""
        s = self.S(b * self.blk) if start is None else start
        assert s >= TWO24
        k = int(regime(s))
        return (1 << (24 + k)) - (s + self.block_tot(b) + self.blk * ((1 << k) >> 1))


# ---- steering ---------------------------------------------------------------------------------------------------------------------
def _limits(signed, dtype, u):
    lo, hi = (-128, 127) if signed else (0, int(np.iinfo(dtype).max))
    return -((-lo) // u) * u, (hi // u) * u


def steer(v, upto, target, dtype, signed=False):
    """replace the fewest voxels in front of index `upto` by multiples of u = ulp(target) so that the float sum in front of `upto` is
    `target`.  The run starts from a sum in target's binade (or both lie below 2^24), so every addition of the run is exact."""
    k = int(regime(target))
    u = 1 << k
    lo, hi = _limits(signed, dtype, u)
    before = np.concatenate([[0], fcum(v[:upto])])                    # before[i] = float sum in front of voxel i
    t = np.arange(1, upto + 1)
    s0 = before[upto - t]
    d = target - s0
    ok = (d >= t * lo) & (d <= t * hi) & (d % u == 0)
    if k:
        ok &= (regime(s0) == k) & (np.sign(s0) == np.sign(target))
    else:
        ok &= np.abs(s0) < TWO24
    at = np.flatnonzero(ok)
    assert at.size, "no run in front of voxel %d reaches %d" % (upto, target)
    n = int(t[at[0]])
    base, rem = divmod(int(d[at[0]]) // u, n)
    run = np.full(n, base, dtype=np.int64)
    run[:rem] += 1
    v[upto - n:upto] = run * u
    assert int(fcum(v[:upto])[-1]) == target
    return n


def quotient(s, per):
    """the metric of frame_shuffle: float sum / size_t voxels, in binary32"""
    return np.float32(s) / np.float32(per)


def _distinct(r, u, per):
    return len({float(quotient(r - u, per)), float(quotient(r, per)), float(quotient(r + u, per))}) == 3


def settle(v, dtype, signed=False):
    """move the frame's sum (by steering its last voxels) to the nearest smaller magnitude whose bracket R - u, R, R + u has three distinct
    quotients; returns R"""
    r = int(fcum(v)[-1])
    k, u = int(regime(r)), ulp(r)
    sign = -1 if r < 0 else 1
    for j in range(4096):
        t = r - sign * j * u
        if int(regime(t)) != k or int(regime(t - u)) > k or int(regime(t + u)) > k:
            break
        if _distinct(t, u, v.size):
            if j:
                steer(v, v.size, t, dtype, signed)
            return t
    raise AssertionError("no sum near %d whose bracket has distinct quotients by %d" % (r, v.size))


def witness(total, n, dtype, k, signed=False):
    """n voxels, multiples of 2^k, that add up to `total`: as even as they go"""
    u = 1 << k
    assert total % u == 0 and abs(total) <= 1 << (24 + k)
    lo, hi = _limits(signed, dtype, u)
    base, rem = divmod(total // u, n)
    w = np.full(n, base, dtype=np.int64)
    w[:rem] += 1
    w *= u
    assert lo <= w.min() and w.max() <= hi, "a witness of %d in %d voxels does not fit the voxel type" % (total, n)
    return w


# ---- the maps, as the reference computes them ---------------------------------------------------------------------------------------
def first_of_sorted(metric):
    """slot i <- the first index whose metric equals the i-th smallest (std::sort, then std::find)"""
    metric = np.asarray(metric)
    return np.array([int(np.flatnonzero(metric == m)[0]) for m in np.sort(metric, kind="stable")], dtype=np.uint64)


def frame_map(sums, per):
    return first_of_sorted(np.asarray(sums, dtype=np.float32) / np.float32(per))


def tile_map(sums, per, dtype):
    """the tile metric is the quotient converted to the voxel type (truncation)"""
    return first_of_sorted((np.asarray(sums, dtype=np.float32) / np.float32(per)).astype(dtype))


def tiles_to_volume(tiles, shape, ts):
    """tiles (ntiles, ts^3) in (z, y, x) tile order, row-major inside a tile -> the volume they are cut from"""
    z, y, x = shape
    return np.ascontiguousarray(tiles.reshape(z // ts, y // ts, x // ts, ts, ts, ts).transpose(0, 3, 1, 4, 2, 5).reshape(shape))


def other_sums(values):
    """what a wrong but plausible kernel computes: name -> sum as binary32"""
    v = np.asarray(values, dtype=np.int64)
    return {"pairwise float32": float(np.sum(v.astype(np.float32), dtype=np.float32)),
            "float64 rounded once": float(np.float32(np.sum(v.astype(np.float64)))),
            "integer converted once": float(np.float32(int(v.sum())))}


# ---- builders: each returns (voxel values of the subject as int64, claim), claim(sim) -> a sentence, or AssertionError ---------------
def _rng(seed):
    return np.random.default_rng(seed)


def _exact(dtype, n, hi, seed):
    v = _rng(seed).integers(0, hi, n)

    def claim(s):
        assert s.cum.max() < TWO24 and np.array_equal(s.cum, s.ip)
        return "exact: the sum %d stays below 2^24, float and integer prefix agree at every voxel" % s.total
    return v, claim


def _random(dtype, n, lo, hi, seed):
    """noise whose sum rounds"""
    v = _rng(seed).integers(lo, hi, n)

    def claim(s):
        assert s.total >= TWO24 and s.total != s.P(s.n)
        return "noise: the sum ends in regime k=%d, %d away from the integer sum" % (int(regime(s.total)), s.total - s.P(s.n))
    return v, claim


def _first_crossing(dtype, n, block, lane, seed):
    blk, epl = geometry(dtype)
    mean = TWO24 / ((block + 0.5) * blk)
    v = _rng(seed).integers(int(mean * 0.5), int(mean * 1.5), n) | 1
    at = block * blk + lane * epl + epl // 2
    v[at] = 1001
    steer(v, at, TWO24 - 3, dtype)

    def claim(s):
        i = s.first_at_least(TWO24)
        assert i == at and s.where(i)[:2] == (block, lane) and s.total != s.P(s.n)
        return "the sum first reaches 2^24 at voxel %d: block %d, lane %d" % (i, block, lane)
    return v, claim


def _regime(dtype, k, seed):
    n = 1 << (max(15, k + 8) if np.dtype(dtype).itemsize == 2 else 16 + k)
    mean = 1.4 * (1 << (23 + k)) / n
    v = _rng(seed).integers(int(0.6 * mean), int(1.4 * mean), n)

    def claim(s):
        ks = regime(s.cum)
        assert int(ks[-1]) == k and int((np.diff(ks) != 0).sum()) == k
        return "the sum ends in regime k=%d (ulp %d) after %d changes of binade" % (k, 1 << k, k)
    return v, claim


TIE, ALTERNATE, DOWN, UP = "tie", "alternate", "down", "up"


def _rounding_run(dtype, n, k, start_block, parity, mode, seed):
    """exact climb into regime k, the float sum at the start of block `start_block` of the given parity, and from there to the end one
    rounding rule: every addition a tie / ties from either parity, an exact addition between two / always just below half an ulp / always just above"""
    blk, _ = geometry(dtype)
    rng = _rng(seed)
    u, lo = 1 << k, 1 << (23 + k)
    start = start_block * blk
    v = np.zeros(n, dtype=np.int64)
    s0 = lo + lo // 16 // (2 * u) * (2 * u) + parity * u
    v[:start] = -(-(lo + lo // 10) // start // 64) * 64
    steer(v, start, s0, dtype)
    m = n - start
    room = int(0.9 * (2 * lo - s0) / m / u)                            # multiples of u per voxel that keep the sum inside the binade
    room = min(max(room, 1), (int(np.iinfo(dtype).max) - u) // u)
    if mode == TIE:
        v[start:] = 2 * rng.integers(0, max(room, 1), m) * u + u // 2       # an even multiple and a half: from an even sum it rounds down
    elif mode == ALTERNATE:
        v[start:] = rng.integers(0, max(room, 1), m) * u + u // 2
        v[start + 1::2] = u * rng.integers(0, max(room, 1), v[start + 1::2].size)     # a multiple: exact, and the next tie starts from either parity
    else:
        assert k >= 2
        v[start:] = rng.integers(0, max(room, 1), m) * u + u // 2 + (-1 if mode == DOWN else 1)

    def claim(s):
        assert (regime(s.cum[start - 1:]) == k).all(), "the run leaves the binade"
        assert (s.S(start) // u) % 2 == parity
        before = np.concatenate([[s.S(start)], s.cum[start:-1]])
        exact = before + s.v[start:]
        rem = exact % u
        if mode == TIE:
            assert (rem == u // 2).all()
        elif mode == ALTERNATE:
            odd = (before[0::2] // u) % 2                                    # the parity each tie starts from
            assert (rem[0::2] == u // 2).all() and (rem[1::2] == 0).all() and min(int(odd.sum()), int((1 - odd).sum())) > m // 8
        elif mode == DOWN:
            assert (rem == u // 2 - 1).all() and (s.cum[start:] < exact).all()
        else:
            assert (rem == u // 2 + 1).all() and (s.cum[start:] > exact).all()
        return "%s: %d additions in regime k=%d from block %d on, parity %d coming in; the float sum ends %d away from the integer sum" % (
            mode, m, k, start_block, parity, s.total - s.P(s.n))
    return v, claim


def _binade_crossing(dtype, n, block, lane, off, seed):
    """2^25 is passed at voxel `off` of `lane` in `block`"""
    blk, epl = geometry(dtype)
    bound = 1 << 25
    mean = bound / ((block + 0.5) * blk)
    v = _rng(seed).integers(int(mean * 0.5), int(mean * 1.5), n) | 1
    at = block * blk + lane * epl + off
    v[at] = 777
    steer(v, at, bound - 2, dtype)

    def claim(s):
        i = s.first_at_least(bound)
        assert i == at and s.where(i) == (block, lane, off) and s.S(i) < bound
        return "the sum passes 2^25 at voxel %d: block %d, lane %d, voxel %d of the lane%s" % (
            i, block, lane, off, " -- the last voxel of the block" if i % blk == blk - 1 else "")
    return v, claim


PASS, FAIL, CROSS = "passes by one u", "fails by one u and does not cross", "fails and crosses"
NEEDED = "fails, S + tot stays below 2^(e+1) and the float sum crosses all the same"


def _guard(dtype, n, block, k, mode, seed):
    """the float sum at the start of `block` set so that the guard S + tot + BLK * u / 2 < 2^(e+1) is met or missed by one u"""
    blk, _ = geometry(dtype)
    u, top = 1 << k, 1 << (24 + k)
    mean = top / ((block + 1.0) * blk)
    v = _rng(seed).integers(int(mean * 0.5), int(mean * 1.5), n) | 1
    if mode == NEEDED:
        # every addition of the block rounds up, by u / 2 - 1, and the voxels are small: the sum crosses well inside the block, and the
        # additions behind the crossing round by the next binade's rule
        assert k >= 2
        v[block * blk:(block + 1) * blk] = v[block * blk:(block + 1) * blk] // u % 2 * u + u // 2 + 1
    tot = int(v[block * blk:(block + 1) * blk].sum())
    s_pass = (top - blk * (u >> 1) - tot - 1) // u * u                     # the largest multiple of u that meets the guard
    start = {PASS: s_pass, FAIL: s_pass + u, CROSS: (top - tot // 2) // u * u, NEEDED: (top - tot - blk * (u // 2 - 1) // 2) // u * u}[mode]
    steer(v, block * blk, start, dtype)

    def claim(s):
        margin = s.guard_margin(block)
        crosses = s.S(min((block + 1) * blk, s.n)) >= top
        assert s.S(block * blk) == start and regime(start) == k
        if mode == PASS:
            assert 0 < margin <= u and not crosses
        elif mode == FAIL:
            assert -u < margin <= 0 and not crosses
        elif mode == CROSS:
            assert margin < 0 and crosses
        else:
            end = (block + 1) * blk
            assert margin <= 0 and start + s.block_tot(block) < top and crosses and s.first_at_least(top) < end - blk // 16
            # (what the block-parallel evaluation would add, had it been taken: every voxel rounded up in the binade below)
            assert s.S(end) != start + int((s.v[block * blk:end] + u // 2 - 1).sum())
        return "guard at block %d in regime k=%d: margin %d (u = %d), %s" % (block, k, margin, u, mode)
    return v, claim


def _record_down(dtype, n, seed):
    """16-bit, 16 blocks.  Values = 1 mod 4 in the binade of ulp 4 always round down: the float sum falls behind the integer prefix.  At the
    start of block 10 the prefix has passed 2^26 and the float sum has not, and the block crosses: a record planned from the prefix is
    valid and names the wrong regime"""
    blk, _ = geometry(dtype)
    b, bound = 10, 1 << 26
    v = np.empty(n, dtype=np.int64)
    v[:4 * blk] = 5312
    v[4 * blk:] = 4 * _rng(seed).integers(380, 580, n - 4 * blk) + 1
    steer(v, b * blk, bound - 400, dtype)
    return v, _record_claim(b, bound, "crosses")


def _record_up(dtype, n, seed):
    """the reverse: 3s and a few 7s in the binade of ulp 4 always round up, the float sum runs ahead.  It reaches 2^26 just in front of
    block 15, whose record was planned (and is valid) for the binade below"""
    blk, _ = geometry(dtype)
    b, bound = 15, 1 << 26
    v = np.empty(n, dtype=np.int64)
    v[:8 * blk] = 4096
    v[8 * blk:] = _rng(seed).choice([3, 7], n - 8 * blk, p=[7 / 8, 1 / 8])
    gain = int(((v[8 * blk:b * blk] + 1)).sum())                          # 3 -> 4 and 7 -> 8 while the ulp is 4
    steer(v, 8 * blk, bound - gain + 16, dtype)
    return v, _record_claim(b, bound, "sum ahead")


def _record_stays(dtype, n, seed):
    """as _record_down, but the block does not cross: 1s (which add nothing while the ulp is 4) and a few 5s (which add 4).  At the start
    of block 15 the prefix has passed 2^26, the float sum stays below it to the end of the frame -- the guard is met in the sum's binade, so
    nothing but the record's regime says that the record is not for this sum"""
    blk, _ = geometry(dtype)
    b, bound = 15, 1 << 26
    v = np.empty(n, dtype=np.int64)
    v[:8 * blk] = 4096
    v[8 * blk:] = _rng(seed).choice([1, 5], n - 8 * blk, p=[7 / 8, 1 / 8])
    gain = int((v[8 * blk:b * blk] - 1).sum())                            # 1 -> 0 and 5 -> 4 while the ulp is 4
    steer(v, 8 * blk, bound - 7400 - gain, dtype)
    return v, _record_claim(b, bound, "stays")


def _record_claim(b, bound, mode):
    def claim(s):
        i = b * s.blk
        S, P = s.S(i), s.P(i)
        kp = int(regime(P))
        valid = P >= TWO24 and s.guard_margin(b, start=P) > 0             # what the planning step sees
        assert valid and int(regime(S)) != kp
        if mode == "crosses":
            assert P >= bound > S and s.S(i + s.blk) >= bound, "the block does not cross"
        elif mode == "stays":
            assert P >= bound > s.S(i + s.blk) and s.guard_margin(b) > 0 and s.S(i + s.blk) > S
        else:
            assert S >= bound > P
        return "block %d: float sum %d, integer prefix %d on the other side of 2^%d -- the record planned from the prefix is valid for k=%d, the sum is in k=%d%s" % (
            b, S, P, bound.bit_length() - 1, kp, int(regime(S)), {"crosses": " and crosses in this block", "stays": " and stays there"}.get(mode, ""))
    return claim


def _geometry(dtype, n, blocks, partial, seed):
    hi = int(np.iinfo(dtype).max) + 1
    v = _rng(seed).integers(hi // 4, hi, n)

    def claim(s):
        assert s.nb == blocks and (s.n % s.blk != 0) == partial and s.n * np.dtype(dtype).itemsize % 16 == 0
        last = (s.nb - 1) * s.blk
        assert s.S(last) >= TWO24 and s.total - s.S(last) != s.P(s.n) - s.P(last), "the last block adds exactly"
        return "%d blocks%s; the last one rounds (regime k=%d)" % (blocks, ", the last of %d voxels" % (s.n - last) if partial else "", int(regime(s.total)))
    return v, claim


def _signed(n, seed):
    """signed bytes: up past 2^24, back down through zero and past -2^24; odd values, so every addition beyond +-2^24 is a tie"""
    rng = _rng(seed)
    up, down = int(n * 0.27), int(n * 0.56)
    v = np.empty(n, dtype=np.int64)
    v[:up] = rng.integers(121, 128, up)
    v[up:up + down] = rng.integers(-128, -120, down)
    v[up + down:] = 2 * rng.integers(-3, 3, n - up - down) + 1

    def claim(s):
        assert s.cum.max() > TWO24 and s.total < -TWO24
        top = int(np.argmax(s.cum))
        zero = top + int(np.flatnonzero(s.cum[top:] < 0)[0])
        ties = int(((np.abs(s.cum) >= TWO24) & (s.v % 2 == 1)).sum())
        assert ties > 1000 and s.total != s.P(s.n)
        return "signed: up to %d at voxel %d, below zero from voxel %d, ends at %d; %d ties on the way" % (int(s.cum.max()), top, zero, s.total, ties)
    return v, claim


def _stall(n):
    v = np.ones(n, dtype=np.int64)

    def claim(s):
        assert s.total == TWO24 and s.P(s.n) == n > TWO24 and s.nb == n // s.blk
        return "stall: %d ones, the float sum stays at 2^24 for the last %d blocks, the integer sum is %d" % (n, (n - TWO24) // s.blk, n)
    return v, claim


# ---- the table ------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, family, dtype, frame, path, build, kind=FRAME, src_shift=0, tile=0, others=False, big=False):
        self.name, self.family, self.dtype, self.frame, self.path = name, family, np.dtype(dtype), tuple(frame), path
        self.build, self.kind, self.src_shift, self.tile, self.others, self.big = build, kind, src_shift, tile, others, big

    @property
    def per_unit(self):
        return self.tile ** 3 if self.kind == TILE else self.frame[0] * self.frame[1]

    @property
    def signed(self):
        return self.kind == TAIL

    def pipelines(self):
        stage = {FRAME: "frame_shuffle", CHUNK: "frame_shuffle(frame_chunk_size=2)", TAIL: "pass_through->frame_shuffle",
                 TILE: "tile_shuffle(tile_size=%d)" % self.tile}[self.kind]
        return [stage, stage + "->lz4"]

    def expected_path(self):
        """the kernel launch_frame_metric documents for these units: signed bytes have their own; 16-byte vectors need a 16-byte aligned
        source and units of whole vectors; of those, units of 16 blocks and more are planned"""
        if self.signed:
            return SIGNED
        nbytes = self.per_unit * self.dtype.itemsize
        if nbytes % 16 or self.src_shift % 16:
            return SERIAL
        return PLANNED if -(-nbytes // BLOCK_BYTES) >= PLANNED_MIN_BLOCKS else SCAN


EXACT, FIRST, BINADES, TIES, CROSSING, GUARD, RECORD, CHAIN, LANE_SERIAL, SIGNED_BYTES, TILES, CHUNKS, STALL = (
    "exact", "first crossing", "every binade", "ties", "binade crossing", "guard", "record", "chain geometry", "lane-serial", "signed bytes",
    "tile_shuffle", "frame_chunk_size", "stall")

U16, U8 = np.uint16, np.uint8
P16 = (128, 256)                    # 64 KiB of uint16: 16 blocks, the smallest planned frame
S16 = (112, 256)                    # 56 KiB: 14 blocks, the scan path
STALL_FRAME = (4101, 4096)          # 2^24 + 5 * 4096 bytes


def _n(frame):
    return frame[0] * frame[1]


def _table():
    t = []

    def add(name, family, dtype, frame, build, **kw):
        path = kw.pop("path", None)
        c = Case(name, family, dtype, frame, path, build, **kw)
        if c.path is None:
            c.path = c.expected_path()
        t.append(c)

    add("exact_u16_scan", EXACT, U16, (100, 200), lambda: _exact(U16, 20000, 400, 7001))
    add("exact_u16_planned", EXACT, U16, P16, lambda: _exact(U16, _n(P16), 500, 7002))
    add("exact_u8_scan", EXACT, U8, (200, 300), lambda: _exact(U8, 60000, 256, 7003))
    add("exact_u8_serial", EXACT, U8, (77, 99), lambda: _exact(U8, 77 * 99, 256, 7004))
    for lane in (0, 29, 63):
        add("first_crossing_lane%d" % lane, FIRST, U16, P16, lambda lane=lane: _first_crossing(U16, _n(P16), 8, lane, 7010 + lane))
    add("first_crossing_scan", FIRST, U16, S16, lambda: _first_crossing(U16, _n(S16), 6, 40, 7015))
    for k in range(1, 11):
        n = 1 << max(15, k + 8)
        add("regime_u16_k%d" % k, BINADES, U16, (n // 256, 256), lambda k=k: _regime(U16, k, 7020 + k))
    for k in range(1, 5):
        n = 1 << (16 + k)
        add("regime_u8_k%d" % k, BINADES, U8, (n // 512, 512), lambda k=k: _regime(U8, k, 7040 + k))
    for frame, tag, blocks in ((P16, "", 5), (S16, "_scan", 4)):
        n = _n(frame)
        add("ties_even" + tag, TIES, U16, frame, lambda n=n, b=blocks: _rounding_run(U16, n, 3, b, 0, TIE, 7050), others=True)
        add("ties_odd" + tag, TIES, U16, frame, lambda n=n, b=blocks: _rounding_run(U16, n, 3, b, 1, TIE, 7051), others=True)
        add("ties_k1" + tag, TIES, U16, frame, lambda n=n, b=blocks: _rounding_run(U16, n, 1, b, 1, TIE, 7052), others=True)
        add("ties_alternate" + tag, TIES, U16, frame, lambda n=n, b=blocks: _rounding_run(U16, n, 2, b, 0, ALTERNATE, 7053))
        add("round_down" + tag, TIES, U16, frame, lambda n=n, b=blocks: _rounding_run(U16, n, 2, b, 0, DOWN, 7054), others=True)
        add("round_up" + tag, TIES, U16, frame, lambda n=n, b=blocks: _rounding_run(U16, n, 3, b, 1, UP, 7055), others=True)
    for tag, lane, off in (("lane0", 0, 0), ("lane37", 37, 11), ("lane63", 63, 5), ("last_voxel", 63, 31)):
        add("binade_crossing_" + tag, CROSSING, U16, P16, lambda lane=lane, off=off: _binade_crossing(U16, _n(P16), 11, lane, off, 7060 + lane + off))
    add("binade_crossing_scan", CROSSING, U16, S16, lambda: _binade_crossing(U16, _n(S16), 9, 63, 31, 7069))
    for frame, tag, block in ((P16, "", 12), (S16, "_scan", 10)):
        for mode, word in ((PASS, "pass"), (FAIL, "fail"), (CROSS, "cross")):
            for k in (1, 3):
                add("guard_%s_k%d%s" % (word, k, tag), GUARD, U16, frame,
                    lambda n=_n(frame), block=block, k=k, mode=mode: _guard(U16, n, block, k, mode, 7070 + k))
        add("guard_needed_k3" + tag, GUARD, U16, frame, lambda n=_n(frame), block=block: _guard(U16, n, block, 3, NEEDED, 7078))
    add("record_prefix_ahead", RECORD, U16, P16, lambda: _record_down(U16, _n(P16), 7080), others=True)
    add("record_prefix_ahead_no_crossing", RECORD, U16, P16, lambda: _record_stays(U16, _n(P16), 7082), others=True)
    add("record_sum_ahead", RECORD, U16, P16, lambda: _record_up(U16, _n(P16), 7081), others=True)
    add("chain_16_blocks", CHAIN, U16, P16, lambda: _geometry(U16, _n(P16), 16, False, 7090))
    add("chain_64_blocks", CHAIN, U16, (256, 512), lambda: _geometry(U16, 256 * 512, 64, False, 7091))
    add("chain_65_blocks", CHAIN, U16, (260, 512), lambda: _geometry(U16, 260 * 512, 65, False, 7092))
    add("chain_130_blocks", CHAIN, U16, (520, 512), lambda: _geometry(U16, 520 * 512, 130, False, 7093))
    add("chain_partial_last_block", CHAIN, U16, (131, 264), lambda: _geometry(U16, 131 * 264, 17, True, 7094))
    add("chain_u8_partial_last_block", CHAIN, U8, (300, 400), lambda: _geometry(U8, 300 * 400, 30, True, 7095))
    add("serial_u16_333x1001", LANE_SERIAL, U16, (333, 1001), lambda: _random(U16, 333 * 1001, 0, 4096, 7100))
    add("serial_u8_999x1001", LANE_SERIAL, U8, (999, 1001), lambda: _random(U8, 999 * 1001, 0, 256, 7101))
    add("serial_short_frames", LANE_SERIAL, U16, (5, 37), lambda: _exact(U16, 5 * 37, 65536, 7102))
    add("serial_shifted_source_ties", LANE_SERIAL, U16, P16, lambda: _rounding_run(U16, _n(P16), 3, 5, 1, TIE, 7103), src_shift=2)
    add("serial_shifted_source_crossing", LANE_SERIAL, U16, P16, lambda: _binade_crossing(U16, _n(P16), 11, 63, 31, 7104), src_shift=2)
    add("signed_aligned", SIGNED_BYTES, U8, (512, 1024), lambda: _signed(512 * 1024, 7110), kind=TAIL, others=True)
    add("signed_odd_frames", SIGNED_BYTES, U8, (515, 1021), lambda: _signed(515 * 1021, 7111), kind=TAIL)
    for ts in (16, 32, 64):
        add("tiles_of_%d" % ts, TILES, U16, (ts, 4 * ts), None, kind=TILE, tile=ts)
    add("chunks_of_two_frames", CHUNKS, U16, P16, lambda: _rounding_run(U16, _n(P16), 3, 5, 0, TIE, 7130), kind=CHUNK)
    add("stall_at_2p24", STALL, U8, STALL_FRAME, lambda: _stall(_n(STALL_FRAME)), others=True, big=True)
    return t


CASES = _table()
NAMES = [c.name for c in CASES]
SMALL = [c.name for c in CASES if not c.big]
BIG = [c.name for c in CASES if c.big]
_by_name = {c.name: c for c in CASES}
assert len(_by_name) == len(CASES)

# where the subject stands among its witnesses (S subject, R the witness of equal sum, L and H the ones an ulp below and above): equal
# metrics name the first index, so the place is part of what is tested
LAYOUTS = ("HSRL", "SRLH", "LRSH", "RLHS", "HLRS", "LSHR")


class Built:
    """a case's volume and what is expected of it.  sums: the reference's float sum of every unit; subjects: [(unit index, R, u, Sim)];
    witnesses[j]: {"L" | "R" | "H": unit index} of subject j (a tile subject has one witness)"""


def case(name):
    return _by_name[name]


_cache = {}


def built(name):
    """built once, read-only"""
    if name not in _cache:
        c = _by_name[name]
        b = _build_tiles(c) if c.kind == TILE else _build_frames(c)
        b.volume.setflags(write=False)
        assert c.big or b.volume.nbytes <= 5 << 20, name
        _cache[name] = b
        if c.big:
            return _cache.pop(name)                              # (not kept: 68 MB)
    return _cache[name]


def _to_dtype(c, values):
    lo, hi = (-128, 127) if c.signed else (0, int(np.iinfo(c.dtype).max))
    assert lo <= values.min() and values.max() <= hi, c.name
    return values.astype(np.int8).view(np.uint8) if c.signed else values.astype(c.dtype)


def _build_frames(c):
    v, claim = c.build()
    v = np.asarray(v, dtype=np.int64)
    n = c.per_unit
    assert v.size == n, (c.name, v.size, n)
    r = settle(v, c.dtype, c.signed)
    k, u = int(regime(r)), ulp(r)
    sim = Sim(v, c.dtype)
    assert sim.total == r
    layout = LAYOUTS[NAMES.index(c.name) % len(LAYOUTS)]
    frames = {"S": v, "L": witness(r - u, n, c.dtype, k, c.signed), "R": witness(r, n, c.dtype, k, c.signed), "H": witness(r + u, n, c.dtype, k, c.signed)}
    b = Built()
    b.case, b.layout, b.claim = c, layout, claim
    vol = np.stack([_to_dtype(c, frames[ch]) for ch in layout]).reshape((4,) + c.frame)
    b.sums = np.array([{"S": r, "L": r - u, "R": r, "H": r + u}[ch] for ch in layout], dtype=np.float32)
    b.subjects = [(layout.index("S"), r, u, sim)]
    b.witnesses = [{ch: layout.index(ch) for ch in "LRH"}]
    b.expected_map = frame_map(b.sums, n)
    if c.kind == CHUNK:                                          # the same units, each cut into two frames
        vol = vol.reshape(8, c.frame[0] // 2, c.frame[1])
    b.volume = vol
    return b


def _build_tiles(c):
    """four tiles along x: [subject 0 at m0 * per, its witness at m0 * per - u, witness of subject 1 at m1 * per, subject 1 at m1 * per - u]"""
    ts, per = c.tile, c.tile ** 3
    tiles, sums, subjects, wit = [None] * 4, [0] * 4, [], []
    for j, (lo, hi, place, wplace) in enumerate(((20000, 60000, 0, 1), (30000, 65000, 3, 2))):
        v = _rng(7120 + ts + j).integers(lo, hi, per)
        nat = int(fcum(v)[-1])
        m, u = nat // per, ulp(nat)
        assert per % u == 0 and int(regime(m * per - u)) == int(regime(nat))
        r = m * per - (u if j else 0)
        steer(v, per, r, c.dtype)
        w = r - u if j == 0 else r + u
        tiles[place], tiles[wplace] = v, witness(w, per, c.dtype, int(regime(nat)))
        sums[place], sums[wplace] = r, w
        subjects.append((place, r, u, Sim(v, c.dtype)))
        wit.append({"L" if j == 0 else "H": wplace})
    b = Built()
    b.case, b.layout = c, "S0 L0 H1 S1"
    b.sums = np.array(sums, dtype=np.float32)
    b.subjects, b.witnesses = subjects, wit
    b.expected_map = tile_map(b.sums, per, c.dtype)

    def claim(_):
        (p0, r0, u0, _s0), (p1, r1, u1, _s1) = subjects
        m0, m1 = r0 // per, (r1 + u1) // per
        assert r0 == m0 * per and r1 == m1 * per - u1 and r0 >= TWO24
        metric = (b.sums / np.float32(per)).astype(c.dtype).tolist()
        assert metric[p0] == m0 and metric[wit[0]["L"]] == m0 - 1 and metric[p1] == m1 - 1 and metric[wit[1]["H"]] == m1 and len(set(metric)) == 4
        return "tiles of %d voxels (%d blocks): tile %d sums to %d * per_tile, one ulp (%d) less truncates to %d; tile %d to %d * per_tile - %d" % (
            per, per * c.dtype.itemsize // BLOCK_BYTES, p0, m0, u0, m0 - 1, p1, m1, u1)
    b.claim = claim
    b.volume = tiles_to_volume(np.stack([_to_dtype(c, t) for t in tiles]), (ts, ts, 4 * ts), ts)
    return b


def units(b):
    """the volume as (units, voxels per unit) in the order the metric reads them; signed cases as int8"""
    c = b.case
    if c.kind == TILE:
        ts = c.tile
        z, y, x = b.volume.shape
        return b.volume.reshape(z // ts, ts, y // ts, ts, x // ts, ts).transpose(0, 2, 4, 1, 3, 5).reshape(-1, ts ** 3)
    flat = b.volume.reshape(4, -1)
    return flat.view(np.int8) if c.signed else flat


def the_map(b, sums):
    """the reorder_map the reference gives for these float sums of the case's units"""
    c = b.case
    return tile_map(sums, c.per_unit, c.dtype) if c.kind == TILE else frame_map(sums, c.per_unit)


def with_subject_sum(b, j, value):
    """the case's sums with subject j's replaced"""
    s = b.sums.copy()
    s[b.subjects[j][0]] = np.float32(value)
    return s


def implied(b, got_map):
    """what a reorder_map that is not the expected one says about the subjects' sums, in words"""
    got = np.asarray(got_map, dtype=np.uint64)
    if np.array_equal(got, b.expected_map):
        return "payload differs, map equal"
    for j, (place, r, u, _) in enumerate(b.subjects):
        for value, words in ((r + u, "ties with the R+u witness"), (r - u, "ties with the R-u witness"), (r + 2 * u, "above R+u"),
                             (r - 2 * u, "below R-u"), (r + u / 2, "between R and R+u"), (r - u / 2, "between R-u and R")):
            if np.array_equal(got, the_map(b, with_subject_sum(b, j, value))):
                return "subject %d (unit %d, R = %d, u = %d): the device's sum %s" % (j, place, r, u, words)
    return "the map %s fits no single sum within two ulps of a subject's (expected %s)" % (got.tolist(), b.expected_map.tolist())
