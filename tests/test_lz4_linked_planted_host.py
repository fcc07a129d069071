"""The streams planted at block borders (tests/lz4_linked_planted.py) on the CPU.  Per case: the oracle's frame under the case's configuration
decodes to the data, its blocks are greedy_trace_linked's block by block (so the per-block catch-up limits the case states are LZ4F's), and
every claimed feature holds.  Sensitivity: every wrong rule of the module's table changes the frame of a case that names it -- in both
block-size classes where the rule has a starred feature -- and no case is there for nothing.  This is the cap on what the GPU test
(test_gpu_lz4_linked_planted.py) may leave out: nothing.  Streams and frames are pinned by digests (tests/golden/lz4_linked_planted.json,
written by oracle/gen_golden.py --lz4-linked-planted); with the reference driver built, the oracle's frames are liblz4 1.9.3's own.

One variant of the issue's table, "low_dict = s_k - 65536 always", is no wrong rule: catch-up keeps ip - match at the accepted offset
(<= 65535) and ip at or above s_k, so no match side ever reaches s_k - 65536 and no lower limit at or below it is ever what stops one
(lz4_linked_planted's docstring, fact (a)).  The test states that instead: the variant changes no case's frame."""
import hashlib
import json
import os

import pytest

import lz4_planted as P
import lz4_linked_planted as L

CASES = L.cases()
NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4_linked_planted.json")

_traces, _frames = {}, {}


def _trace(name, rule=None):
    key = (name, rule)
    if key not in _traces:
        t = L.trace_of(BY_NAME[name], {rule[0]: rule[1]} if rule else None)
        _traces[key] = t if rule is None else [(b["stored"], b["block"]) for b in t]
    return _traces[key]


def _frame(oracle, name):
    if name not in _frames:
        _frames[name] = L.oracle_frame(oracle, BY_NAME[name])
    return _frames[name]


def _blocks(trace):
    return [(b["stored"], b["block"]) for b in trace]


@pytest.mark.parametrize("name", NAMES)
def test_case_is_the_oracles_and_holds_its_features(oracle, name):
    c = BY_NAME[name]
    frame = _frame(oracle, name)
    assert bytes(oracle.lz4_decode_frames(frame, len(c["data"]))) == c["data"]
    want = P.frame_blocks(frame)
    trace = _trace(name)
    assert [(b[0], b[1], b[2]) for b in c["blocks"]] and sum(b[1] for b in c["blocks"]) == len(c["data"])
    assert len(want) == len(trace), (len(want), len(trace))
    for i, (w, t) in enumerate(zip(want, trace)):
        if w != (t["stored"], t["block"]):
            detail = P.first_difference(t["block"], w[1], ("trace", "oracle")) if not (w[0] or t["stored"]) else "trace failed at %s" % (t["failed"],)
            pytest.fail("%s block %d %s: stored %s (oracle) / %s (trace); %s" % (name, i, c["blocks"][i], w[0], t["stored"], detail), pytrace=False)
    assert len(c["blocks"]) >= 3 and c["k"] >= 2, "block-parallel needs three blocks, the border entries from two blocks back"
    ctx = L.Ctx(c, trace)
    assert c["features"]
    missing = [f for f in c["features"] if not L.FEATURES[f](ctx)]
    assert not missing, (name, missing)


def _changed(name, rule):
    return _trace(name, rule) != _blocks(_trace(name))


@pytest.mark.parametrize("rule", L.WRONG, ids=["%s=%s" % r for r in L.WRONG])
def test_every_wrong_rule_changes_a_case_that_names_it(rule):
    named = [c for c in CASES if rule in [tuple(r) for r in c["rules"]]]
    assert named, "no case names this rule"
    caught = [c for c in named if _changed(c["name"], rule)]
    assert len(caught) == len(named), ("named but not changed", [c["name"] for c in named if c not in caught])
    starred = {f for c in named for f in c["features"] if f in L.STAR}
    if starred:
        for cls in L.STAR_CLASSES:
            assert any(c["cls"] == cls for c in caught), (rule, cls)


def test_no_case_is_there_for_nothing():
    """every case but the short last blocks (R9: held by parity with the oracle alone) changes under at least one wrong rule"""
    idle = [c["name"] for c in CASES if not c["rules"] and not c["name"].startswith("last-")]
    assert not idle, idle
    assert all(not c["rules"] for c in CASES if c["name"].startswith("last-"))


@pytest.mark.parametrize("rule", L.EQUIVALENT, ids=["%s=%s" % r for r in L.EQUIVALENT])
def test_the_low_dict_variant_is_no_wrong_rule(rule):
    assert not [c["name"] for c in CASES if _changed(c["name"], rule)]
    for c in CASES:                      # the premise: every non-fresh block's low_dict lies at or below its start - 65536 (or at the stream's start)
        for (s, n, fresh, low_in, low_dict) in c["blocks"]:
            assert fresh or low_dict <= max(s - 65536, 0), (c["name"], s)


def test_every_feature_is_claimed():
    claimed = {f for c in CASES for f in c["features"]}
    assert claimed == set(L.FEATURES), sorted(set(L.FEATURES) ^ claimed)
    star = ["border:off=65535", "border:no-match@65536", "start:found-at-second-byte", "start:first-byte-not-searched", "start:first-byte-is-a-source",
            "prev:last-searched", "prev:not-searched", "prev:cut-at-border", "src:crosses-border", "stored:last-literals", "stored:fails-at-match",
            "catchup:stops-at-block-start", "catchup:dict-start", "parked:tag0"]
    assert set(star) == L.STAR
    want = star + ["border:off=65534", "stored:fails-second-check", "catchup:through-block-start", "catchup:tmp-buffer", "frame:no-history",
                   "parked:boundary", "edge:history-candidate<16", "edge:back_room<4", "dense:history-sources"] \
        + ["catchup:through-block-start=%d" % k for k in (1, 63, 64, 65, 300)] + ["last:n=%d" % n for n in (1, 4, 12, 13, 14, 17, 31)]
    assert not [f for f in want if f not in claimed]
    for cls in L.STAR_CLASSES:
        have = {f for c in CASES if c["cls"] == cls for f in c["features"]}
        assert not [f for f in star if f not in have], (cls, [f for f in star if f not in have])
    assert 50 <= len(CASES) <= 70
    big = [c for c in CASES if len(c["data"]) > 4 * L.CLASS[c["cls"]][1] + 31 or L.CLASS[c["cls"]][1] > 262144]
    assert sorted(c["name"] for c in big) == ["off=65535-ext1024", "off=65535-ext4096", "parked-tag0-ext1024", "parked-tag0-ext4096"]
    assert all(len(c["data"]) <= 12 << 20 for c in CASES)
    for cls, B in (("ext1024", 1 << 20), ("ext4096", 4 << 20)):                       # tsh = 10 and tsh = 8
        assert L.TSH[B] in (10, 8) and {f for c in CASES if c["cls"] == cls for f in c["features"]} >= {"border:off=65535", "parked:tag0"}


def test_pairs_of_cases_share_their_bytes(oracle):
    """one stream under two configurations: the blocks behind the border differ, each frame is its own oracle's (the per-case test)"""
    for a, b in (("stops-at-block-start-ext64", "through-block-start-prefix64"), ("stops-at-block-start-ext256", "through-block-start-prefix256"),
                 ("frame-one-pair64", "frame-no-history-chunked64")):
        assert BY_NAME[a]["data"] == BY_NAME[b]["data"], (a, b)
        k = BY_NAME[a]["k"]
        assert P.frame_blocks(_frame(oracle, a))[k] != P.frame_blocks(_frame(oracle, b))[k], (a, b)


def test_cases_are_deterministic():
    L._cases = None
    again = L.cases()
    assert [(c["name"], c["data"], c["blocks"]) for c in again] == [(c["name"], c["data"], c["blocks"]) for c in CASES]


def test_layouts_on_small_streams():
    K = 65536
    assert L.ext_layout(3 * K + 17, K) == [(0, K, True, 0, 0), (K, K, False, K, 0), (2 * K, K, False, 2 * K, K), (3 * K, 17, False, 2 * K, 2 * K)]
    assert L.prefix_layout(5 * K, K, 4 * K) == [(0, K, True, 0, 0), (K, K, False, 0, 0), (2 * K, K, False, 0, 0), (3 * K, K, False, 0, 0),
                                                (4 * K, K, False, 4 * K, 3 * K)]
    assert L.chunked_layout(3 * K, K, 2 * K) == [(0, K, True, 0, 0), (K, K, False, 0, 0), (2 * K, K, True, 2 * K, 2 * K)]
    assert L.tmp_layout(3 * K + 31, K, K + 10) == [(0, K, True, 0, 0), (K, K, False, 0, 0), (2 * K, K, False, 0, 0), (3 * K, 31, False, 2 * K, 2 * K)]
    assert L.search_positions(10, 145)[:3] == [11, 12, 13] and L.search_positions(10, 145)[64:69] == [75, 76, 78, 80, 82]
    blk = L.emit_block(b"abcdeabcdeaXvwxyz", [(0, 5, 5, 6), (11, 6, 0, 0)])
    assert P.parse_block(blk) == [(0, 5, 5, 6), (11, 6, 0, 0)]


def test_golden_digests(oracle):
    with open(GOLDEN) as f:
        G = json.load(f)["cases"]
    assert sorted(G) == sorted(NAMES)
    for c in CASES:
        fr = _frame(oracle, c["name"])
        got = {"n": len(c["data"]), "sha256": hashlib.sha256(c["data"]).hexdigest(), "frame_bytes": len(fr), "frame_sha256": hashlib.sha256(fr).hexdigest()}
        assert got == G[c["name"]], c["name"]


def test_oracle_is_liblz4_on_every_case(oracle):
    from oracle import ref
    if not ref.available():
        pytest.skip("oracle/_ref/libsqy_ref.so not available here")
    for c in CASES:
        assert _frame(oracle, c["name"]) == L.liblz4_frame(ref, oracle, c), c["name"]
