"""The oracle's quantiser LUTs against the REFERENCE's own sqeazy::quantiser<uint16_t, uint8_t> (oracle/ref_driver.cpp compiles
encoders/quantiser_utils.hpp in place, with the string_parsers.hpp of oracle/ref_shim/), on the volumes of tests/quantiser_cases.py:
  * everywhere: both of the oracle's tables hash to tests/golden/quantiser_luts.json, which holds what the reference gave
    (oracle/gen_golden.py --quantiser), and the properties the case table names are checked with its numpy walk;
  * where oracle/_ref loads: oracle.quantiser_build_luts(oracle.histogram(v)) and oracle.quantiser_encode(v) equal the live reference's,
    entry by entry, the reference run with 1 and 3 threads -- the default weighting on every case, power_of_1_2 and offset_power_of_2_3 on
    the rounding and boundary cases -- and on 200 seeded random volumes of the histogram families of tests/sanitize/quantiser_lut_test.cpp."""
import hashlib
import json
import os

import numpy as np
import pytest

import quantiser_cases as Q
from oracle import gen_golden as G

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "quantiser_luts.json")) as _f:
    GOLDEN = json.load(_f)["cases"]


def _ref():
    """skips only where the reference library is absent, or is an older one that cannot be rebuilt (no reference tree); a library that
    could be rebuilt here and still lacks the quantiser is an error"""
    from oracle import ref
    if not ref.available():
        pytest.skip("oracle/_ref/libsqy_ref.so not available here")
    if not ref.quantiser_available():
        assert ref.reference_tree() is None, "oracle/_ref/libsqy_ref.so lacks %r although it can be built here" % (ref.QUANTISER_ENTRY_POINTS,)
        pytest.skip("oracle/_ref/libsqy_ref.so was built from an older driver and cannot be rebuilt here")
    return ref


def _sha(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


def _same(what, name, got, want):
    at = Q.first_difference(got, want)
    assert at is None, "%s: %s[%d] = %d, the reference has %d" % (name, what, at, got.reshape(-1)[at], want.reshape(-1)[at])


def test_golden_and_table_are_the_same_cases():
    assert list(Q.NAMES) == sorted(GOLDEN, key=Q.NAMES.index) and len(GOLDEN) == len(Q.NAMES)
    for n in Q.NAMES:
        assert sorted(GOLDEN[n]["luts"]) == sorted(G.quantiser_weightings(n)), n
    # the families and their sizes
    assert len(Q.names(Q.ROUNDING)) == 3 and len(Q.names(Q.TIES)) == 3 and len(Q.names(Q.BOUNDARY)) == 10
    assert len(Q.names(Q.HISTOGRAM)) == 2 and Q.names(Q.BIG) == ["count_above_2p24"]


def test_the_cases_are_what_they_are_named():
    for n in Q.SMALL:
        assert Q.volume(n).size <= 1 << 18, n
    for levels in (255, 256, 257, 258):
        for where in ("packed", "top"):
            v = Q.volume("levels_%d_%s" % (levels, where))
            assert len(np.unique(v)) == levels and (where == "packed" or v.max() == 65535)
    assert Q.volume("bin_65535_occupied").max() == 65535 and Q.volume("bin_65534_occupied").max() == 65534
    assert len(np.unique(Q.volume("bin_65535_occupied"))) <= 256
    t = Q.volume("quarter_tiles").reshape(3, Q.TILE_VOXELS)
    quarters = [np.bincount(x >> 14, minlength=4) for x in t]
    assert [int(q.argmax()) for q in quarters] == [0, 1, 3] and all((q > 0).sum() >= 2 for q in quarters)
    for x, edges in zip(t, ((16383, 16384), (16383, 16384, 49151, 49152), (49151, 49152))):
        assert all((x == e).any() for e in edges)
    v = Q.volume("two_tiles_tail_7")
    assert v.shape == (3, 13, 841) and v.size == 32799 and v.size > Q.TILE_VOXELS and v.size % 8 == 7
    h = Q.histogram(Q.volume("count_above_2p24"))
    assert h[500] == (1 << 24) + 1 and int(h.sum()) == (1 << 24) + 1 + 70000 and h[:300].sum() == 0 and h[1500:].sum() == 0


@pytest.mark.parametrize("name", Q.NAMES)
def test_oracle_equals_the_golden(oracle, name):
    vol = Q.volume(name)
    assert _sha(vol)[:12] == GOLDEN[name]["voxels_sha256"], name
    histo = oracle.histogram(vol)
    for w in G.quantiser_weightings(name):
        enc, dec = oracle.quantiser_build_luts(histo, w)
        assert [_sha(enc), _sha(dec.astype("<u2"))] == GOLDEN[name]["luts"][w], (name, w)


@pytest.mark.parametrize("name", Q.NAMES)
def test_oracle_equals_the_live_reference(oracle, name):
    ref = _ref()
    vol = Q.volume(name)
    histo = oracle.histogram(vol)
    for w in G.quantiser_weightings(name):
        enc, dec = oracle.quantiser_build_luts(histo, w)
        codes, dec2 = oracle.quantiser_encode(vol, w)
        for nthreads in (1, 3):
            renc, rdec = ref.quantiser_luts(vol, w, nthreads)
            _same("lut_encode (%s, %d threads)" % (w, nthreads), name, enc, renc)
            _same("lut_decode (%s, %d threads)" % (w, nthreads), name, dec, rdec)
            rcodes, rdec2 = ref.quantiser_encode(vol, w, nthreads)
            _same("codes (%s, %d threads)" % (w, nthreads), name, codes, rcodes)
            _same("encode's lut_decode (%s, %d threads)" % (w, nthreads), name, dec2, rdec2)
        assert [_sha(renc), _sha(rdec.astype("<u2"))] == GOLDEN[name]["luts"][w], (name, w)


@pytest.mark.parametrize("name", Q.NAMES)
def test_the_numpy_walk_is_the_oracle(oracle, name):
    histo = Q.histogram(Q.volume(name))
    assert np.array_equal(histo, oracle.histogram(Q.volume(name)))
    enc, dec = oracle.quantiser_build_luts(histo)
    wenc, wdec = Q.walk(histo, np.float32, "away")
    _same("the walk's lut_encode", name, wenc, enc)
    _same("the walk's lut_decode", name, wdec, dec)


def _differs(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


@pytest.mark.parametrize("name", Q.names(Q.ROUNDING))
def test_rounding_cases_tell_binary32_from_binary64(name):
    histo = Q.histogram(Q.volume(name))
    assert int((np.arange(65536) * histo.astype(np.int64)).max()) > 1 << 24               # raw_idx * count is rounded
    assert _differs(Q.walk(histo, np.float64), Q.walk(histo)), name


@pytest.mark.parametrize("name", Q.names(Q.TIES))
def test_tie_cases_tell_the_rounding_rules_apart(name):
    """pairs that start on an even bin: half-away and half-even part.  Pairs from the odd bin 40001: every tie lies on odd + .5, where the
    two agree (both go up), so that set parts half-up from half-down only"""
    histo = Q.histogram(Q.volume(name))
    away = Q.walk(histo)
    assert _differs(Q.walk(histo, rounding="down"), away), name
    if name in Q.TIES_EVEN_START:
        assert _differs(Q.walk(histo, rounding="even"), away), name
    else:
        first = int(np.flatnonzero(histo)[0])
        assert name == "pairs_40001_x40" and first % 2 == 1 and not _differs(Q.walk(histo, rounding="even"), away)
    assert set(Q.TIES_EVEN_START) < set(Q.names(Q.TIES))


def test_big_count_case_tells_a_float_summed_total():
    histo = Q.histogram(Q.volume("count_above_2p24"))
    assert int(histo.max()) == (1 << 24) + 1 and int(np.float32(histo.max())) == 1 << 24            # the float count itself rounds
    assert _differs(Q.walk(histo, total="float32"), Q.walk(histo))


def _draw(rng, k):
    """a volume of at most 2^18 voxels whose histogram is of the k-th family of tests/sanitize/quantiser_lut_test.cpp; (family, voxels)"""
    budget = 1 << 18

    def spread(lo, hi, levels, max_count):
        levels = min(levels, hi - lo + 1)
        bins = lo + rng.choice(hi - lo + 1, levels, replace=False)
        return bins, rng.integers(1, max_count + 1, levels)
    family = ("narrow band", "wide uniform", "clusters", "near 256 levels", "heavy peak")[k % 5]
    if family == "narrow band":
        lo = int(rng.integers(0, 60000))
        levels = int(rng.integers(100, 1000))
        bins, counts = spread(lo, min(65535, lo + int(rng.integers(300, 5300))), levels, max(1, budget // levels // 2))
    elif family == "wide uniform":
        levels = int(rng.integers(257, 20257))
        bins, counts = spread(0, 65535, levels, max(1, min(50, budget // levels)))
    elif family == "clusters":
        h = np.zeros(65536, np.int64)
        clusters = int(rng.integers(2, 42))
        for c in range(clusters):
            at, n = int(rng.integers(0, 65000)), int(rng.integers(1, 61))
            for i in range(n):
                if at + i < 65536 and rng.integers(0, 3):
                    h[at + i] = int(rng.integers(1, 21 if c % 2 else 1 + budget // (2 * clusters * 60)))
        bins, counts = np.flatnonzero(h), h[np.flatnonzero(h)]
    elif family == "near 256 levels":
        levels = int(rng.integers(240, 280))
        bins, counts = spread(int(rng.integers(0, 1000)), 65535 - int(rng.integers(0, 1000)), levels, int(rng.integers(1, 900)))
    else:
        bins, counts = spread(0, 65535, int(rng.integers(300, 3300)), 3)
        h = np.zeros(65536, np.int64)
        h[bins] = counts
        h[rng.integers(0, 65536, 5)] = rng.integers(20000, 48000, 5)
        bins, counts = np.flatnonzero(h), h[np.flatnonzero(h)]
    if len(bins) == 0:
        bins, counts = np.array([int(rng.integers(0, 65536))]), np.array([7])
    v = rng.permutation(np.repeat(bins, counts).astype(np.uint16))
    assert 0 < v.size <= budget, (family, v.size)
    return family, v.reshape(1, 1, -1)


def test_random_draws(oracle):
    ref = _ref()
    rng = np.random.default_rng(20261024)
    seen = {"lloyd": 0, "linear": 0}
    for k in range(200):
        family, vol = _draw(rng, k)
        w = ("none", "none", "none", "power_of_1_2", "none", "offset_power_of_2_3", "none")[k % 7]
        seen["lloyd" if len(np.unique(vol)) > 256 else "linear"] += 1
        enc, dec = oracle.quantiser_build_luts(oracle.histogram(vol), w)
        codes, dec2 = oracle.quantiser_encode(vol, w)
        nthreads = (1, 3)[k % 2]
        renc, rdec = ref.quantiser_luts(vol, w, nthreads)
        rcodes, rdec2 = ref.quantiser_encode(vol, w, nthreads)
        what = "draw %d (%s, %s, %d voxels)" % (k, family, w, vol.size)
        _same("lut_encode", what, enc, renc)
        _same("lut_decode", what, dec, rdec)
        _same("codes", what, codes, rcodes)
        _same("encode's lut_decode", what, dec2, rdec2)
    assert seen["lloyd"] > 100 and seen["linear"] > 10, seen
