"""The batch encode's joint path of `quantiser->bitswap1->lz4` on the volumes of tests/quantiser_cases.py: histograms whose Lloyd walk
rounds in binary32 (products and sums above 2^24), ties between the rounding rules, the boundary between the two mappings, tiles that
vote for different quarters of the value range, and a count no binary32 holds.  tests/test_oracle_reference_quantiser.py holds the
oracle to the reference's own quantiser on the same volumes, and shows that a walk in binary64, with rint, or with a float-summed total
gives other tables on them; here the LUT kernel (sqy_quantiser_lut.hpp on the GPU) and the kernels around it must give the oracle's
blob, byte for byte.  A failure names the case, says whether the decode LUT in the header or the payload differs, and gives the first
differing LUT entry."""
import base64
import time

import numpy as np
import pytest

import quantiser_cases as Q
from test_gpu_encode_batch import CANARY, GAP, _batch, _profile, _want
from test_gpu_encode_batch_stages import ONCE, QUANT, SINGLE

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda", 0)


def _key(name):
    return "quantiser_case:" + name


def _header_lut(oracle, blob):
    """(the decode LUT the blob's header carries, the header's size)"""
    h = oracle.header_unpack(blob)
    stage = next(s for s in oracle.build_stages(h["pipename"]) if s.name == "quantiser")
    text = stage.cmap["decode_lut_string"]
    return np.frombuffer(base64.b64decode(text[len("<verbatim>"):-len("</verbatim>")]), dtype="<u2"), h


def _codes(oracle, blob, h, voxels):
    """the quantiser's codes a blob's payload holds, voxel by voxel"""
    body = np.frombuffer(blob, np.uint8)[h["size"]:h["size"] + h["bytes"]]
    return oracle.bitswap1_decode(np.ascontiguousarray(oracle.lz4_decode_frames(body, voxels)).view(np.uint8))


def _explain(oracle, name, vol, got, want):
    """why `got` is not the oracle's blob: the case, header LUT or payload, the first differing LUT entry"""
    try:
        glut, gh = _header_lut(oracle, got)
    except Exception as e:                                       # noqa: BLE001  (a blob that cannot be read is its own finding)
        return "%s: the blob's header cannot be read (%s)" % (name, e)
    wlut, wh = _header_lut(oracle, want)
    at = Q.first_difference(glut, wlut)
    if at is not None:
        return "%s: the decode LUT in the header differs, first at lut_decode[%d] = %d, the oracle has %d (%d entries differ)" % (
            name, at, glut[at], wlut[at], int((glut != wlut).sum()))
    if got[:gh["size"]] != want[:wh["size"]]:
        return "%s: the header differs outside the decode LUT (the LUT's %d entries are equal)" % (name, wlut.size)
    try:
        gc, wc = _codes(oracle, got, gh, vol.size), _codes(oracle, want, wh, vol.size)
        k = Q.first_difference(gc, wc)
    except Exception as e:                                       # noqa: BLE001
        return "%s: the payload differs and does not decode (%s); the decode LUT in the header is the oracle's" % (name, e)
    if k is None:
        return "%s: the payload differs in its LZ4 frames only; codes and the decode LUT are the oracle's" % name
    v = int(vol.reshape(-1)[k])
    return "%s: the payload differs (the decode LUT in the header is the oracle's), first at voxel %d: lut_encode[%d] = %d, the oracle has %d" % (
        name, k, v, gc[k], wc[k])


def _same_blobs(oracle, cases, blobs, wanted):
    """every blob is the oracle's; else one line per failing case (and no dump of the blobs)"""
    bad = [_explain(oracle, name, vol, blob, wanted[name]) for (name, vol), blob in zip(cases, blobs) if blob != wanted[name]]
    if bad:
        pytest.fail("%d of %d blobs are not the oracle's:\n  " % (len(bad), len(blobs)) + "\n  ".join(bad), pytrace=False)


@pytest.fixture(scope="module")
def cases():
    return [(n, Q.volume(n)) for n in Q.SMALL]


@pytest.fixture(scope="module")
def wanted(sqy, oracle, cases):
    """name -> the blob the oracle and the single call both give (test_gpu_encode_batch._want holds them against each other), once"""
    return {n: _want(sqy, oracle, QUANT, v, 0, _dev(), _key(n)) for n, v in cases}


def _joint_call(sqy, oracle, cases, wanted, **kw):
    vols = [v for _, v in cases]
    (rc, blobs), prof = _profile(sqy, lambda: _batch(sqy, QUANT, vols, _dev(), **kw))
    assert rc == 0
    _same_blobs(oracle, cases, blobs, wanted)
    assert {k: prof[k][1] if k in prof else 0 for k in ONCE} == {k: 1 for k in ONCE}, prof
    assert not any(k in prof for k in SINGLE), prof
    return blobs


def test_every_case_in_one_call(sqy, oracle, cases, wanted):
    assert len(cases) == len(Q.NAMES) - 1 and all(v.size <= 1 << 18 for _, v in cases)
    _joint_call(sqy, oracle, cases, wanted)


def test_every_case_from_unaligned_sources(sqy, oracle, cases, wanted):
    """sources 2 bytes behind a 16-byte boundary: the voxel-by-voxel loads of the histogram and of the look-up, across tile boundaries"""
    cap = max(sqy.max_compressed_length(QUANT, v.shape, np.uint16) for _, v in cases) + 7
    assert cap % 16 != 0
    _joint_call(sqy, oracle, cases, wanted, src_shift=2, cap=cap)


def test_every_case_and_back_through_the_batch_decode(sqy, oracle, cases, wanted):
    import torch
    dev = _dev()
    vols = [v for _, v in cases]
    srcs = [torch.from_numpy(v.copy()).to(dev) for v in vols]
    cap = max(sqy.max_compressed_length(QUANT, v.shape, np.uint16) for v in vols) + 13
    buf = torch.full((cap * len(vols),), CANARY, dtype=torch.uint8, device=dev)
    rc, offs, lens = sqy.encode_batch_device(QUANT, [s.data_ptr() for s in srcs], [v.shape for v in vols], np.uint16, buf.data_ptr(), cap)
    assert rc == 0
    outs = [torch.full((GAP + v.nbytes + GAP,), CANARY, dtype=torch.uint8, device=dev) for v in vols]
    rc, decoded = sqy.decode_batch_device(buf.data_ptr(), offs, lens, [o.data_ptr() + GAP for o in outs], [v.nbytes for v in vols], np.uint16)
    torch.cuda.synchronize()
    assert rc == 0 and decoded == [v.nbytes for v in vols]
    for (name, v), o in zip(cases, outs):
        h = o.cpu().numpy()
        assert (h[:GAP] == CANARY).all() and (h[GAP + v.nbytes:] == CANARY).all(), name
        back = h[GAP:GAP + v.nbytes].view(np.uint16)
        ref = oracle.pipeline_decode(wanted[name]).reshape(-1)
        at = Q.first_difference(back, ref)
        if at is not None:
            pytest.fail("%s: voxel %d decodes to %d, the oracle's blob to %d" % (name, at, back[at], ref[at]), pytrace=False)


def test_count_above_2p24(sqy, oracle):
    """2^24 + 1 voxels in one bin: its float count rounds, and a total summed in binary32 gives other tables.  16.8 M voxels, alone in
    its call; the wall time is printed (pytest -s)"""
    t0 = time.perf_counter()
    name = Q.names(Q.BIG)[0]
    vol = Q.volume(name)
    want = _want(sqy, oracle, QUANT, vol, 0, _dev(), _key(name))
    t1 = time.perf_counter()
    (rc, blobs), prof = _profile(sqy, lambda: _batch(sqy, QUANT, [vol], _dev()))
    t2 = time.perf_counter()
    assert rc == 0
    _same_blobs(oracle, [(name, vol)], blobs, {name: want})
    assert {k: prof[k][1] if k in prof else 0 for k in ONCE} == {k: 1 for k in ONCE}, prof
    assert not any(k in prof for k in SINGLE), prof
    print("\ncount_above_2p24: %.2f s in all (volume, oracle and single call %.2f s, batch call %.2f s)" % (time.perf_counter() - t0, t1 - t0, t2 - t1))
