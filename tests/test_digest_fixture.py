"""The noise digest's fixture (digest_planes.py) against liblz4 alone: every planted chunk is a compressed frame, and the same stream
without its plant a stored one.  test_gpu_inplace.py::test_noise_digest compares blobs of this fixture with the oracle's byte for byte,
so a parse that missed a planted match -- the digest giving it a wrong bucket or tag -- stores that chunk raw, and the blob differs."""
import numpy as np
import pytest

import digest_planes as DP


@pytest.mark.parametrize("chunk", DP.DIGEST_CHUNKS, ids=["%dk" % (c >> 10) for c in DP.DIGEST_CHUNKS])
def test_every_plant_decides_its_frame(oracle, chunk):
    pipe = "bitswap1->lz4" + DP.lz4_config(chunk)
    per = DP.chunks_per_plane(chunk)
    for plants in (True, False):
        planes, kinds = DP.plane_streams(chunk, per, plants=plants)
        if plants:                                                      # the blob test_noise_digest compares with
            blob = oracle.pipeline_encode(pipe, oracle.bitswap1_decode(planes.view(np.uint16)).reshape(1, 1, -1), nthreads=2)
            payload = blob[oracle.header_unpack(blob)["size"]:]
        else:                                                           # (its lz4 stage alone: the transposes take seconds here)
            payload = oracle.lz4_encode_chunked(planes, oracle.Lz4Config(DP.lz4_config(chunk)[1:-1])).tobytes()
        stored = DP.frame_kinds(payload)
        assert len(stored) == len(kinds) == 16 * per
        for c, (kind, raw) in enumerate(zip(kinds, stored)):
            if plants:
                assert raw == (kind == 0), (c, kind, "a planted chunk must compress, a chunk of noise must not")
            else:
                assert raw, (c, kind, "without its plant the chunk is noise: stored")
