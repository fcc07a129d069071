"""The table of tests/frame_metric_cases.py on the CPU: for every case the oracle's C loop gives the map the module expects (which it does
only if its sequential float sum of the subject is the module's: the subject ties with the witness of that sum), the witnesses are exact,
the bracket's quotients are distinct, a subject sum one ulp off in either direction gives another map -- so tests/test_gpu_frame_metric.py
fails for a one-ulp error in that frame -- and the case's claim holds in the simulation.  For the tie, stall, round-down / round-up and
signed cases three plausible wrong summations (pairwise float32, float64 rounded once, the integer sum converted once) give another map.
No case is skipped: one whose claim cannot be met at its size is fixed in the table."""
import numpy as np
import pytest

import frame_metric_cases as F


@pytest.fixture(scope="module", params=F.NAMES)
def b(request):
    return F.built(request.param)


def _oracle_map(oracle, b):
    c = b.case
    if c.kind == F.TILE:
        return oracle.tile_shuffle_encode(b.volume, c.tile)[1]
    return oracle.frame_shuffle_encode(b.volume, char=c.signed, chunk=2 if c.kind == F.CHUNK else 1)[1]


def test_case(oracle, b):
    c = b.case
    units = F.units(b)
    per = c.per_unit
    assert units.shape == (4, per) and c.path == c.expected_path()
    # the module's sequential sums are the ones its expected map is made of
    sums = [int(F.fcum(u)[-1]) for u in units]
    assert sums == [int(s) for s in b.sums.astype(np.int64)] and [float(np.float32(s)) for s in sums] == b.sums.tolist()
    # ... and the oracle's C loop gives that map
    assert np.array_equal(_oracle_map(oracle, b), b.expected_map), (c.name, b.layout)
    lines = []
    for j, (place, r, u, sim) in enumerate(b.subjects):
        assert sim.total == r == sums[place] and u == F.ulp(r)
        wit = b.witnesses[j]
        # every witness is exact, partial sum by partial sum, and is the intended value
        for ch, at in wit.items():
            w = units[at].astype(np.int64)
            want = r + {"L": -u, "R": 0, "H": u}[ch]
            assert (w % u == 0).all() and np.array_equal(F.fcum(w), np.cumsum(w)) and int(w.sum()) == want == sums[at], (c.name, ch)
        if c.kind == F.TILE:
            # truncated metrics: the subject at m * per is told from one ulp less, the one at m * per - u from one ulp more
            step = -u if "L" in wit else u
            assert not np.array_equal(F.the_map(b, F.with_subject_sum(b, j, r + step)), b.expected_map)
            assert np.array_equal(F.the_map(b, F.with_subject_sum(b, j, r + step)), F.the_map(b, F.with_subject_sum(b, j, np.nextafter(np.float32(r), np.float32(np.inf * step)))))
            lines.append("subject %d: R = %d, u = %d, one ulp %s changes the map" % (j, r, u, "down" if step < 0 else "up"))
            continue
        # frames: the three quotients are distinct, the expected map shows the bracket
        q = [float(F.quotient(r + d, per)) for d in (-u, 0, u)]
        assert q[0] < q[1] < q[2], (c.name, q)
        first = min(place, wit["R"])
        order = [wit["L"], first, first, wit["H"]]
        assert b.expected_map.tolist() == order, (c.name, b.layout)
        # sensitivity: one ulp up, one ulp down
        for to in (np.inf, -np.inf):
            # (below 2^24 a sum of integers is an integer: there the nearest other sum is one away, not an ulp)
            off = np.nextafter(np.float32(r), np.float32(to)) if abs(r) >= F.TWO24 else np.float32(r + (1 if to > 0 else -1))
            assert abs(float(off) - r) in (u, u / 2)
            assert not np.array_equal(F.the_map(b, F.with_subject_sum(b, j, off)), b.expected_map), (c.name, float(off))
        lines.append("subject at %d: R = %d, u = %d, quotients %r" % (place, r, u, q))
        if c.others:
            for what, value in F.other_sums(sim.v).items():
                assert value != r and not np.array_equal(F.the_map(b, F.with_subject_sum(b, j, value)), b.expected_map), (c.name, what, value, r)
                lines.append("%s gives %d" % (what, value))
    said = b.claim(b.subjects[0][3])
    print("\n%s [%s, %s, %s %s, layout %s]: %s\n  %s" % (c.name, c.family, c.path, c.dtype.name, "x".join(map(str, b.volume.shape)), b.layout, said,
                                                          "\n  ".join(lines)))


def test_table_reaches_what_it_lists():
    cs = F.CASES
    fam = {c.family for c in cs}
    assert fam == {F.EXACT, F.FIRST, F.BINADES, F.TIES, F.CROSSING, F.GUARD, F.RECORD, F.CHAIN, F.LANE_SERIAL, F.SIGNED_BYTES, F.TILES, F.CHUNKS, F.STALL}
    assert {c.path for c in cs} == {F.PLANNED, F.SCAN, F.SERIAL, F.SIGNED}
    for family in (F.FIRST, F.TIES, F.CROSSING, F.GUARD):
        assert {c.path for c in cs if c.family == family} >= {F.PLANNED, F.SCAN}, family
    assert all(c.path == F.PLANNED for c in cs if c.family in (F.RECORD, F.STALL))
    assert sorted(c.tile for c in cs if c.kind == F.TILE) == [16, 32, 64]
    assert [c.name for c in cs if c.big] == F.BIG and len(F.BIG) == 1
    # the subject stands first, last and in between
    places = {F.LAYOUTS[i % len(F.LAYOUTS)].index("S") for i in range(len(cs))}
    assert places == {0, 1, 2, 3}


def test_steering_and_witnesses_refuse_what_would_round():
    v = np.full(4096, 60000, dtype=np.int64)
    with pytest.raises(AssertionError):
        F.steer(v, 4096, (1 << 27) + 4, np.uint16)            # 4 is no multiple of the ulp there
    with pytest.raises(AssertionError):
        F.witness((1 << 25) + 2, 100, np.uint16, 1)           # past 2^25 a sum of even voxels is no longer exact
    n = F.steer(v, 4096, 200000000, np.uint16)
    assert int(F.fcum(v)[-1]) == 200000000 and (v[4096 - n:] % 16 == 0).all()
