"""frame_shuffle and tile_shuffle: the oracle, and the expectations of tests/frame_metric_cases.py, against the REFERENCE's own
sqeazy::detail::frame_shuffle and sqeazy::detail::tile_shuffle (oracle/ref_driver.cpp compiles encoders/frame_shuffle_utils.hpp and
encoders/tile_shuffle_utils.hpp in place, with the Boost.Accumulators stand-in of oracle/boost_standin/, which only their median path
names; shapes with a remainder are answered by the driver before the reference is called).  The metric of these stages is a SEQUENTIAL
binary32 sum, divided by a size_t, for tiles truncated to the voxel type, and ties all take the first unit: the order of the additions
and every conversion is part of the result, and this is where it is held to the reference's code and not to our reading of it.
  * everywhere: for every case of tests/golden/ref_shuffles.json (taken from the reference by oracle/gen_golden.py --shuffles) the
    oracle's output hashes to the golden, its decode_map is the golden's list, its zero-filled decode hashes to the golden, and what the
    golden calls refused the oracle refuses; the expected_map of every case of frame_metric_cases.py is the one the golden recorded;
  * where oracle/_ref loads: the live reference gives those expected_maps and the oracle's output byte for byte on the whole case table,
    gives the golden, agrees with the oracle on 300 seeded random draws per stage, and decodes like the oracle from every map met on
    the way and from hand-made maps that name a unit twice and leave one out."""
import hashlib
import os

import numpy as np
import pytest

import frame_metric_cases as F
from ref_stage_inputs import load_shuffle_cases
from oracle import gen_golden as G

HERE = os.path.dirname(os.path.abspath(__file__))
META, CASES, EXPECTED_MAPS = load_shuffle_cases(os.path.join(HERE, "golden", "ref_shuffles.json"))
GROUPS = sorted({(c["stage"], c["dtype"]) for c in CASES})
# One run pins the reference: every unit's metric is computed by one thread from that unit alone, in the same order, and the threads only
# share out the units (frame_shuffle_utils.hpp:121-133, tile_shuffle_utils.hpp:173-186); sort and find see the finished metrics.  So the
# thread count cannot change a map, and the tests below require exactly that of 1 and 4 threads before they rely on either.
THREADS = (1, 4)


def _ref():
    """skips only where the reference library is absent, or is an older one that cannot be rebuilt (no reference tree); a library that
    could be rebuilt here and still lacks the shuffles is an error"""
    from oracle import ref
    if not ref.available():
        pytest.skip("oracle/_ref/libsqy_ref.so not available here")
    if not ref.shuffles_available():
        assert ref.reference_tree() is None, "oracle/_ref/libsqy_ref.so lacks %r although it can be built here" % (ref.SHUFFLE_ENTRY_POINTS,)
        pytest.skip("oracle/_ref/libsqy_ref.so was built from an older driver and cannot be rebuilt here")
    return ref


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _group(stage, dtype):
    return [c for c in CASES if c["stage"] == stage and c["dtype"] == dtype]


# ---- everywhere: table, golden and oracle ----------------------------------------------------------------------------------------------
def test_table_and_golden_are_the_same_cases():
    rows = G.shuffle_table()
    assert [r["id"] for r in rows] == [c["id"] for c in CASES]
    for r, c in zip(rows, CASES):
        for k in r:
            assert r[k] == c[k], (r["id"], k)
        assert ("sha256" in c) + ("refused" in c) == 1, c["id"]
        assert ("refused" in c) == (not G.shuffle_whole(c)), c["id"]
        assert int(np.prod(c["shape"])) * (2 if c["dtype"] == "uint16" else 1) <= 64 << 10, c["id"]
    assert sorted(EXPECTED_MAPS) == sorted(F.NAMES)


def test_the_golden_holds_what_it_is_for():
    """the branches the table is there to take, read off the recorded maps"""
    live = [c for c in CASES if "map" in c]
    for stage, params in (("frame_shuffle", {1, 2, 3}), ("tile_shuffle", {2, 4, 5, 8, 16})):
        for dt in ("uint16", "uint8", "char"):
            mine = [c for c in live if c["stage"] == stage and c["dtype"] == dt]
            assert params <= {G.shuffle_param(c) for c in mine}, (stage, dt)
            assert any(len(c["map"]) == 1 for c in mine), (stage, dt)                             # one unit: the map is [0]
            assert any(len(c["map"]) > 1 and G.is_permutation(c["map"]) for c in mine), (stage, dt)
            assert any(not G.is_permutation(c["map"]) for c in mine), (stage, dt)                 # equal metrics: a unit written twice
            assert any("refused" in c for c in _group(stage, dt)), (stage, dt)
    for c in live:
        n = len(c["map"])
        if c["kind"] == "all_equal":
            assert c["map"] == [0] * n, c["id"]
        if c["kind"] == "two_groups":
            assert c["map"] == [1] * (n // 2) + [0] * (n - n // 2), c["id"]
        if c["kind"] == "descending":
            assert c["map"] == list(range(n))[::-1], c["id"]
        if c["kind"] == "permuted":                          # equal in metric, different in content: the first one stands for all of them
            assert c["map"].count(0) == (n + 1) // 2 and not set(c["map"]) & set(range(2, n, 2)), c["id"]
        if c["kind"] == "integer_edge":                      # m * per - 1 truncates to m - 1 and ties with the unit in front of it
            assert c["map"] == [0] + [u - (u % 2 == 0) for u in range(1, n)], c["id"]
        if c["kind"] == "trunc_zero":                        # (-per, 0), 0 and (0, per) all truncate toward zero; -per and per do not
            assert c["map"] == [3] * len(range(3, n, 5)) + [0] * (n - len(range(3, n, 5)) - len(range(4, n, 5))) + [4] * len(range(4, n, 5)), c["id"]
        if c["kind"] == "fraction":
            assert set(c["map"]) == {0, 2}, c["id"]
    # tile counts that differ per axis: the linear tile order is visible
    assert any(c["stage"] == "tile_shuffle" and len({d // c["tile_size"] for d in c["shape"]}) == 3 for c in live)


@pytest.mark.parametrize("stage,dtype", GROUPS)
def test_oracle_equals_the_golden(oracle, stage, dtype):
    ran = 0
    for c in _group(stage, dtype):
        vol = G.shuffle_volume(c)
        assert _sha(vol)[:12] == c["input_sha256"], c["id"]
        if "refused" in c:
            with pytest.raises(ValueError):
                G.oracle_shuffle(c, vol)
            continue
        out, dmap, back = G.oracle_shuffle(c, vol)
        assert out.nbytes == c["bytes"] and _sha(out) == c["sha256"], c["id"]
        assert dmap.tolist() == c["map"], c["id"]
        assert _sha(back) == c["decode_sha256"], c["id"]
        if G.is_permutation(c["map"]):
            assert c["decode_sha256"] == _sha(vol), c["id"]
        ran += 1
    assert ran


@pytest.mark.parametrize("name", F.NAMES)
def test_expected_map_is_the_one_the_reference_gave(name):
    """the fallback where oracle/_ref is absent: the golden holds what the live reference gave for the case's volume"""
    assert F.built(name).expected_map.tolist() == EXPECTED_MAPS[name], name


# ---- with oracle/_ref: the live reference ------------------------------------------------------------------------------------------------
_maps_met = []                                           # (row, encoded volume, map): every map the live tests produced, for the decode test


def _frame_metric_row(b):
    c = b.case
    if c.kind == F.TILE:
        return {"stage": "tile_shuffle", "dtype": "uint16", "tile_size": c.tile}
    return {"stage": "frame_shuffle", "dtype": "char" if c.kind == F.TAIL else str(c.dtype), "frame_chunk_size": 2 if c.kind == F.CHUNK else 1}


def _decodes_alike(ref, row, enc, dmap):
    _, odec, _, rdec = G.shuffle_fns(row)
    assert np.array_equal(rdec(enc, dmap), odec(enc, dmap)), (row, np.asarray(dmap).tolist())


@pytest.mark.parametrize("name", F.NAMES)
def test_case_table_on_the_live_reference(oracle, name):
    ref = _ref()
    b = F.built(name)
    maps = []
    for nthreads in THREADS:
        out, dmap = G.frame_metric_reference(b, nthreads)
        maps.append(dmap)
    assert np.array_equal(maps[0], maps[1]), (name, "the reference's map depends on the thread count")
    assert np.array_equal(dmap, b.expected_map), "%s: the reference's decode_map is %s, the case expects %s" % (name, dmap.tolist(), b.expected_map.tolist())
    want, omap = G.frame_metric_oracle(b)
    assert np.array_equal(omap, dmap) and out.tobytes() == want.tobytes(), name
    _decodes_alike(ref, _frame_metric_row(b), out, dmap)


@pytest.mark.parametrize("stage,dtype", GROUPS)
def test_live_reference_gives_the_golden(oracle, stage, dtype):
    ref = _ref()
    for c in _group(stage, dtype):
        vol = G.shuffle_volume(c)
        if "refused" in c:
            with pytest.raises(ref.Remainder):               # answered by the driver: the reference is not run
                G.reference_shuffle(c, vol)
            continue
        got = [G.reference_shuffle(c, vol, nthreads) for nthreads in THREADS]
        assert all(np.array_equal(a, b) for a, b in zip(*got)), (c["id"], "the reference depends on the thread count")
        out, dmap, back = got[0]
        assert _sha(out) == c["sha256"] and dmap.tolist() == c["map"] and _sha(back) == c["decode_sha256"], c["id"]
        oout, omap, oback = G.oracle_shuffle(c, vol)
        assert np.array_equal(out, oout) and np.array_equal(dmap, omap) and np.array_equal(back, oback), c["id"]
        _maps_met.append((c, out, dmap))


def _row(stage, dtype, shape, kind, seed, p):
    r = {"stage": stage, "dtype": dtype, "shape": [int(d) for d in shape], "kind": kind, "seed": seed}
    r["frame_chunk_size" if stage == "frame_shuffle" else "tile_size"] = int(p)
    return r


def _narrow(rng, row, vol):
    """the same shape with values from a range of a few: equal frame metrics are common, tile metrics truncate to equal integers"""
    lo = int(rng.integers(0, 250))
    v = rng.integers(lo, lo + int(rng.integers(1, 4)), vol.shape)
    return (v % 256).astype(np.uint8) if row["dtype"] != "uint16" else (v + int(rng.integers(0, 60000))).astype(np.uint16)


def _live(ref, rng, row, narrow):
    vol = G.shuffle_volume(row)
    if narrow:
        vol = _narrow(rng, row, vol)
    assert vol.size <= 4096
    _, _, renc, _ = G.shuffle_fns(row)
    oenc, _, _, _ = G.shuffle_fns(row)
    want, omap = oenc(vol)
    got = [renc(vol, nthreads) for nthreads in THREADS]
    assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][0], got[1][0]), (row, "the reference depends on the thread count")
    out, dmap = got[0]
    assert np.array_equal(dmap, omap), (row, narrow, dmap.tolist(), omap.tolist())
    assert out.tobytes() == want.tobytes(), (row, narrow)
    _decodes_alike(ref, row, out, dmap)
    return int(not G.is_permutation(dmap))


def test_random_draws_frame_shuffle(oracle):
    ref = _ref()
    rng = np.random.default_rng(20261101)
    ties = 0
    for k in range(300):
        chunk = int(rng.integers(1, 5))
        z = chunk * int(rng.integers(1, 13))
        y, x = int(rng.integers(1, 9)), int(rng.integers(1, 11))
        dtype = ("uint16", "uint8", "char")[k % 3]
        kind = "random" if dtype != "char" or k % 2 else "pm128"
        ties += _live(ref, rng, _row("frame_shuffle", dtype, (z, y, x), kind, k, chunk), narrow=k % 2 == 0)
    assert ties > 30, ties


def test_random_draws_tile_shuffle(oracle):
    ref = _ref()
    rng = np.random.default_rng(20261102)
    ties = 0
    for k in range(300):
        ts = int(rng.choice([2, 3, 4, 5, 8]))
        most = {2: 6, 3: 4, 4: 4, 5: 3, 8: 2}[ts]
        while True:
            counts = [int(n) for n in rng.integers(1, most + 1, 3)]
            if int(np.prod(counts)) * ts ** 3 <= 4096:
                break
        dtype = ("uint16", "uint8", "char")[k % 3]
        kind = "random" if dtype != "char" or k % 2 else "pm128"
        ties += _live(ref, rng, _row("tile_shuffle", dtype, [n * ts for n in counts], kind, k, ts), narrow=k % 2 == 0)
    assert ties > 100, ties


def test_decode_from_every_map_and_from_hand_made_ones(oracle):
    """the reference's decode into a zero-filled buffer (the driver's choice: the reference leaves slots no entry names as they were)
    against the oracle's, from every map the golden cases gave and from maps no encode gives: a unit named twice -- the later entry
    wins -- and one left out, which stays zero"""
    ref = _ref()
    if not _maps_met:                                        # (run alone: take the golden's maps)
        for c in CASES:
            if "map" in c:
                _maps_met.append((c, G.shuffle_volume(c), np.array(c["map"], dtype=np.uint64)))
    assert len(_maps_met) >= sum("map" in c for c in CASES)
    for row, enc, dmap in _maps_met:
        _decodes_alike(ref, row, enc, dmap)
    rng = np.random.default_rng(20261103)
    for k in range(60):
        stage = ("frame_shuffle", "tile_shuffle")[k % 2]
        dtype = ("uint16", "uint8", "char")[k % 3]
        if stage == "frame_shuffle":
            p, units = int(rng.integers(1, 4)), int(rng.integers(2, 9))
            row = _row(stage, dtype, (p * units, 3, 5), "random", k, p)
        else:
            p, counts = int(rng.choice([2, 4, 5])), [int(n) for n in rng.integers(1, 4, 3)]
            units = int(np.prod(counts))
            row = _row(stage, dtype, [n * p for n in counts], "random", k, p)
        enc = G.shuffle_volume(row)
        dmap = rng.permutation(units).astype(np.uint64)
        if units > 1:
            twice, out = rng.choice(units, 2, replace=False)
            dmap[dmap == out] = twice                         # `twice` is named by two entries, `out` by none
            assert not G.is_permutation(dmap)
        _, odec, _, rdec = G.shuffle_fns(row)
        want, got = odec(enc, dmap), rdec(enc, dmap)
        assert np.array_equal(got, want), (row, dmap.tolist())
        if units > 1:                                        # the slot nobody names is zero, the slot named twice holds the later unit
            per = enc.size // units
            flat = (lambda v: v.reshape(units, per)) if stage == "frame_shuffle" else (lambda v: oracle._tiles_full(v, p))
            later = max(int(i) for i in np.flatnonzero(dmap == twice))
            assert not flat(got)[int(out)].any() and np.array_equal(flat(got)[int(twice)], enc.reshape(units, per)[later]), (row, dmap.tolist())
    with pytest.raises(ref.Refused):                          # a map that names a unit the shape does not have: not handed to the reference
        ref.frame_shuffle_decode(np.zeros((4, 2, 2), np.uint8), np.array([0, 1, 2, 4], np.uint64))
    with pytest.raises(ref.Refused):
        ref.tile_shuffle_decode(np.zeros((2, 2, 4), np.uint8), np.array([0], np.uint64), 2)
