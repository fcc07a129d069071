"""Plane streams for the noise digest tests (test_gpu_inplace.py::test_noise_digest, test_digest_fixture.py).

The digest (sqy_kernels.hip: bitswap1_u16_regs, lz4_chunks_kernel) stands in for liblz4's search through a chunk of noise from probe 961
on.  A chunk of pure noise is stored raw whatever the parse does, so a plant only tests the digest if the chunk compresses BECAUSE the
planted match is found: L bytes copied from probe position a to probe position b, with L large enough that the block ends below n - 1
bytes (LZ4F_makeBlock's limit) only when the match is taken.  Every chunk of kind != 0 holds exactly one such plant; the chunks are
independent frames, so the stream with no plants at all is "that stream without that one plant" for every chunk at once."""
import numpy as np

KINDS = 8
DIGEST_FROM = 961                                                     # the first probe the digest covers


def probe_positions(chunk):
    """positions liblz4's search probes in a chunk when it starts with the chunk and finds nothing (step schedule of accel 1)"""
    pos, p, st, nb = [], 1, 1, 64
    while True:
        pos.append(p)
        p2 = p + st; st = nb >> 6; nb += 1
        if p2 > chunk - 12 + 1:
            break
        p = p2
    return np.array(pos, dtype=np.int64)                              # pos[u - 1] = probe u


def hash5(y, at):
    """liblz4's LZ4_hash5 (byU32 tables, 12 bits) of the five bytes at positions `at` of y"""
    idx = np.asarray(at)[:, None] + np.arange(8)
    seq = (y[np.minimum(idx, y.size - 1)].astype(np.uint64) << (np.arange(8, dtype=np.uint64) * 8)).sum(axis=1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return ((seq << np.uint64(24)) * np.uint64(889523592379)) >> np.uint64(52)


def match_length(chunk):
    """a match this long is what decides between a compressed and a stored block: the literal-only block is n + n / 255 + 2 bytes"""
    return chunk // 255 + 40


def _found(y, pos, q, src):
    """liblz4 finds src at probe q: src is a probe position (or 0) and no probe between them went to src's bucket"""
    if src != 0 and not np.any(pos == src):
        return False
    between = pos[(pos > src) & (pos < q)]
    h = hash5(y, np.array([src, q] + list(between)))
    return h[0] == h[1] and not np.any(h[2:] == h[0])


def _copy(y, dst, src, L):
    """y[dst:dst + L] = y[src:src + L] as a forward byte copy (LZ4's overlapping match when dst - src < L)"""
    D = dst - src
    for o in range(0, L, D):
        m = min(D, L - o)
        y[dst + o:dst + o + m] = y[src + o:src + o + m]


def _plant(y, pos, b, delta, L, a_choices):
    """copy L bytes from a + delta to b + delta for the first a in a_choices liblz4 would find; returns (a, b) or None.  delta = 0: the
    match starts on probe b; -1: one byte in front of it (found at b, caught up); +1: one byte behind (b finds nothing, the next probe
    b + s finds a + s, which must be a probe too)"""
    if b + delta + L + 16 > y.size:
        return None
    for a in a_choices:
        a = int(a)
        D = b - a
        if D < 8 or D > 65535 or a + delta < 0:
            continue
        q = b
        if delta > 0:
            nxt = pos[pos > b]
            if not nxt.size or not np.any(pos == nxt[0] - D):
                continue
            q = int(nxt[0])
        keep = y[b + delta:b + delta + L].copy()
        _copy(y, b + delta, a + delta, L)
        if _found(y, pos, q, q - D):
            return a, b
        y[b + delta:b + delta + L] = keep
    return None


def plane_streams(chunk, nchunks_per_plane, plants=True):
    """16 bit planes of nchunks_per_plane chunks each; chunk c is of kind c % KINDS (0: pure noise).  Returns (stream, kinds)."""
    rng = np.random.default_rng(chunk + nchunks_per_plane)
    n = 16 * chunk * nchunks_per_plane
    x = rng.integers(0, 256, n, dtype=np.uint8)
    kinds = np.arange(n // chunk) % KINDS
    if not plants:
        return x, kinds
    pos = probe_positions(chunk)
    late = pos[DIGEST_FROM - 1:]
    L = match_length(chunk)
    u961 = int(pos[DIGEST_FROM - 1])

    def sources(b, lo, hi):
        """probes in [lo, hi) in front of b within 64 KiB: those the copy does not overlap first, nearest first; then the overlapping ones"""
        s = pos[(pos >= max(lo, b - 65535)) & (pos < min(hi, b))][::-1]
        return np.concatenate([s[s <= b - L], s[s > b - L]])

    def first_plant(bs, delta=0, lo=0, hi=1 << 62):
        for b in bs:
            got = _plant(y, pos, int(b), delta, L, sources(int(b), lo, hi))
            if got:
                return got
        return None

    for c in range(n // chunk):
        y = x[c * chunk:(c + 1) * chunk]                               # (a view: plants land in x)
        kind = int(kinds[c])
        if kind == 0:
            continue                                                   # pure noise: the whole chunk from the digest, stored
        j = int(rng.integers(0, 1 << 30))
        fits = late[late + L + 16 <= chunk]
        if kind in (1, 2, 3):
            # a match that starts ON a late probe (1), one byte BEHIND it (2: the probe itself finds nothing), one byte IN FRONT of it (3);
            # in every other chunk the source is a probe in front of 961, whose table entry the parse made from the bytes, not the digest
            bs = fits[fits < u961 + 60000] if c % 2 else fits
            got = first_plant(np.roll(bs, -(j % len(bs))), {1: 0, 2: 1, 3: -1}[kind], *((0, u961) if c % 2 else (u961, 1 << 62)))
            if c % 2 and got:
                assert got[0] < u961
        elif kind == 4:                                                # a late probe whose five bytes straddle two 1 KiB pieces
            bs = fits[(fits % 1024) >= 1020]
            got = first_plant(np.roll(bs, -(j % len(bs))))
        elif kind == 5:
            # all-zero 1 KiB pieces in the noise, L bytes and more of them: holes (the transpose writes neither them nor their digest entries,
            # the parse takes this chunk from its bytes); the zeros are what makes the chunk compress
            k = (L + 64 + 1023) // 1024
            pc = 8 + c % 5
            y[pc * 1024:(pc + k) * 1024] = 0
            got = (pc * 1024, (pc + k) * 1024)
        elif kind == 6:                                                # a match in front of probe 961: the digest is never used
            bs = pos[DIGEST_FROM - 300:DIGEST_FROM - 1]
            got = first_plant(np.roll(bs, -(j % len(bs))))
        else:                                                          # kind 7: the chunk's last probes (behind the last whole batch of 64)
            got = first_plant(fits[::-1])
            if got and chunk <= (64 << 10):
                assert got[1] >= late[(len(late) // 64) * 64 - 1]
        assert got, (chunk, c, kind)
    return x, kinds


def chunks_per_plane(chunk):
    return max(1, (512 << 10) // chunk)


def lz4_config(chunk):
    """an lz4 configuration whose chunks are `chunk` bytes, one LZ4F block each, on the plane stream plane_streams(chunk, ..) makes.
    blocksize_kb picks the block ID (the closest of 64 KiB .. 4 MiB) and framestep_kb is a multiple of it: chunks of 128 KiB and
    512 KiB and 2 MiB come from n_chunks_of_input instead"""
    nch = 16 * chunks_per_plane(chunk)
    kb = chunk >> 10
    if kb in (16, 32, 64, 1024, 4096):
        return "(blocksize_kb=%d,framestep_kb=%d)" % (kb, kb)
    if kb == 256:
        return ""
    return "(blocksize_kb=%d,n_chunks_of_input=%d)" % (kb * 2, nch)


DIGEST_CHUNKS = [16 << 10, 32 << 10, 64 << 10, 128 << 10, 256 << 10, 512 << 10, 1 << 20, 2 << 20, 4 << 20]


def frame_kinds(payload):
    """the LZ4 frames of an lz4 payload: for every frame, True when its (single) block is stored raw"""
    out, off = [], 0
    while off < len(payload):
        assert payload[off:off + 4] == bytes([0x04, 0x22, 0x4D, 0x18])
        off += 7
        raw = []
        while True:
            field = int.from_bytes(payload[off:off + 4], "little")
            off += 4
            if field == 0:
                break
            raw.append(bool(field & 0x80000000))
            off += field & 0x7fffffff
        assert len(raw) == 1
        out.append(raw[0])
    return out
