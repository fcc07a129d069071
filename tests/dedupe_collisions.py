"""Plane streams for the duplicate-chunk search's tests (test_dedupe_fixture.py, test_gpu_dedupe_collisions.py): chunks built to SHARE A
KEY with an earlier chunk and differ from it, so that the byte compare behind the key (sqy_kernels.hip: lz4_chunk_dedupe inside the parse
wavefront, lz4_dedupe_verify_kernel everywhere else) has to say "different" -- which honest data never asks of it: a 64-bit key does not
collide by luck.

The key is restated here (piece_hashes: what bitswap1_u16_regs leaves per 1 KiB piece, chunk_keys: what lz4_dedupe_key_kernel folds them
into).  A lane owns the 16 bytes x, y, z, w (little-endian dwords) at piece * 1024 + lane * 16; its term is mix(x C1 + y C2 + z C3 + w C4)
* (2 lane + 1) with mix(a) = a ^ (a >> 15); a row of sixteen lanes stores the sum of its terms with bit 0 forced on, or 0 when all its
bytes are zero; a piece adds the SUM of its four rows to the key, weighted by its number.  Every step is a bijection of 32 bits or a sum,
hence the collision classes:
  0 vanishing  x = C2 t, y = -C1 t: the lane's term is 0 for non-zero bytes.  A piece of such lanes hashes like any other such piece
  1 linear     (x + C2 t, y - C1 t) leaves the lane's term alone: one 16-byte vector differs, at any piece and lane -- the class that
               walks the compare loops' edges (positions())
  2 forced bit one non-zero dword solved for row sum T in one chunk, T ^ 1 in the other: both rows store T | 1
  3 row move   the same term in a lane of row 0 and in a lane of row 2: other row hashes, the same sum
  4 zero sum   a piece whose rows hash to T and -T adds what an all-zero piece adds; the all-zero piece is a HOLE (frames in place: the
               transposer never writes it, the compare goes by its marker) -- in either order
and all-zero chunks (key 1: taken as duplicates without a compare) next to chunks that hold a single set bit -- which collide among
themselves where the bit is bit 31 of x and of w of one lane: 2^31 times any odd constant is 2^31.
Whether the restatement IS the kernels' function is asserted on the GPU (the keys of SQYAMD_Dedupe_Report against chunk_keys)."""
import itertools

import numpy as np

import digest_planes as DP

M = 0xffffffff
C = (0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D, 0x27D4EB2F)
CHUNKS = [16 << 10, 64 << 10, 256 << 10]


def chunks_per_plane(chunk):
    """eight, fewer where a volume would pass 8 MiB"""
    return min(8, (512 << 10) // chunk)


def lz4_config(chunk, accel=None):
    """DP.lz4_config(chunk), with liblz4's acceleration when asked for (accel = -1: acceleration 2, the parse that leaves the search to
    lz4_dedupe_verify_kernel)"""
    cfg = DP.lz4_config(chunk)
    if accel is None:
        return cfg
    return "(accel=%d%s" % (accel, "," + cfg[1:] if cfg else ")")


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def piece_hashes(stream):
    """the four row hashes of every 1 KiB piece of `stream` (uint8, whole pieces): uint32 [pieces, 4]"""
    d = np.ascontiguousarray(stream).view("<u4").reshape(-1, 64, 4).astype(np.uint64)
    with np.errstate(over="ignore"):
        a = (d * np.array(C, dtype=np.uint64)).sum(axis=2) & np.uint64(M)
        a = ((a ^ (a >> np.uint64(15))) * (2 * np.arange(64, dtype=np.uint64) + 1)) & np.uint64(M)
    rows = a.reshape(-1, 4, 16).sum(axis=2) & np.uint64(M)
    nz = d.reshape(-1, 4, 64).any(axis=2)
    return np.where(nz, rows | np.uint64(1), np.uint64(0)).astype(np.uint32)


def chunk_keys(stream, chunk):
    """the key of every full chunk: uint64 [stream.size // chunk]"""
    n = stream.size // chunk
    q = piece_hashes(stream[:n * chunk]).reshape(n, chunk >> 10, 4).astype(np.uint64)
    m = np.uint64(M)
    i = np.arange(chunk >> 10, dtype=np.uint64)
    with np.errstate(over="ignore"):
        s = q.sum(axis=2) & m
        h1 = (s * (((2 * i + 1) * np.uint64(C[0])) & m)).sum(axis=1) & m
        rot = ((s << np.uint64(13)) | (s >> np.uint64(19))) & m
        h2 = (rot * (((2 * i + 3) * np.uint64(C[1])) & m)).sum(axis=1) & m
    return np.where(q.any(axis=(1, 2)), (h2 << np.uint64(32)) | h1 | np.uint64(3), np.uint64(1))


def expected_dup_of(stream, chunk):
    """what the search has to decide: chunk k shares the frame of the FIRST chunk r with its key if their bytes are equal, else its own; a
    ragged last chunk takes no part"""
    keys = chunk_keys(stream, chunk)
    nchunks = (stream.size + chunk - 1) // chunk
    first, out = {}, np.arange(nchunks, dtype=np.uint32)
    for k, key in enumerate(keys.tolist()):
        r = first.setdefault(key, k)
        if r != k and np.array_equal(stream[k * chunk:(k + 1) * chunk], stream[r * chunk:(r + 1) * chunk]):
            out[k] = r
    return out


# ---- solvers ----------------------------------------------------------------------------------------------------------------------------
def _unmix(y):
    """a with a ^ (a >> 15) == y"""
    a = y
    for _ in range(3):
        a = y ^ (a >> 15)
    return a & M


def solve_dword(term, lane, slot=0):
    """the dword that, alone in slot `slot` (0: x .. 3: w) of lane `lane`, gives the lane the term `term`"""
    a = _unmix((term * pow(2 * lane + 1, -1, 1 << 32)) & M)
    return (a * pow(C[slot], -1, 1 << 32)) & M


def _dwords(buf, piece, lane):
    return buf[piece * 1024 + lane * 16:piece * 1024 + lane * 16 + 16].view("<u4")


def linear(buf, piece, lane, t):
    """class 1: the lane's term stays, its bytes do not"""
    d = _dwords(buf, piece, lane)
    d[0] = (int(d[0]) + C[1] * t) & M
    d[1] = (int(d[1]) - C[0] * t) & M


def vanishing_piece(ts):
    """class 0: 64 lanes with term 0 and non-zero bytes (ts: 64 non-zero multipliers)"""
    p = np.zeros(256, dtype="<u4")
    for lane, t in enumerate(ts):
        p[lane * 4], p[lane * 4 + 1] = (C[1] * int(t)) & M, (-C[0] * int(t)) & M
    return p.view(np.uint8)


def single_dword_piece(pairs):
    """a piece that is zero but for one dword (slot x) per (lane, term) of `pairs`"""
    p = np.zeros(256, dtype="<u4")
    for lane, term in pairs:
        p[lane * 4] = solve_dword(term, lane)
    return p.view(np.uint8)


def positions(chunk):
    """(piece, lane) of the 16-byte vectors where the two compares have their edges: the first and the last vector of the chunk; each of
    the four pieces of the fused loop's first and last group (p0 += 4); vectors 0, 255, 256, 1023, 1024 and nvec - 1 of the verify kernel's
    walk (j = i + u * 256, four per thread and round) -- those that exist at this chunk size"""
    n = chunk >> 10
    want = [(0, 0), (1, 17), (2, 40), (3, 63), (4, 0), (15, 63), (16, 0), (n - 4, 5), (n - 3, 30), (n - 2, 50), (n - 1, 20), (n - 1, 63)]
    return [p for i, p in enumerate(want) if p[0] < n and p not in want[:i]]


def hole_pieces(chunk):
    """all-zero pieces next to the positions (never one of them: a zero piece that gains a byte changes its marker, and the key)"""
    n = chunk >> 10
    taken = {p for p, _ in positions(chunk)}
    return sorted({p for p in (5, 14, 17, n - 5) if p < n and p not in taken})


def nearly_zero_spots(chunk):
    """(piece, lane, dword, bit) of the single set bit of a nearly-zero chunk: bit 0 and 31 of x and w in lanes 0 and 15 of each row, in the
    first and the last piece -- all 64 of them where the volume has room, at 256 KiB (32 chunks in all) four that hold every value once"""
    n = chunk >> 10
    lanes = [16 * r + e for r in range(4) for e in (0, 15)]
    if chunks_per_plane(chunk) * 16 >= 128:
        return list(itertools.product((0, n - 1), lanes, (0, 3), (0, 31)))
    return [(0, 0, 0, 0), (0, 63, 3, 31), (n - 1, 31, 3, 0), (n - 1, 32, 0, 31)]


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------
def plane_streams(chunk):
    """(stream, cases): the plane stream of a volume (16 bit planes of chunks_per_plane(chunk) chunks) and what it holds.  A case is a dict:
    name; kind -- "reject" (chunk k has the key of the earlier chunk r, other bytes: its own frame), "accept" (k equals r: r's frame),
    "zero" (all zero, like r) or "alone" (nearly zero with a key of its own); k, r (r == k for "alone"); vectors -- the 16-byte vectors
    (piece * 64 + lane) in which k and r differ, all of them; holes_k, holes_r -- their all-zero pieces"""
    rng = np.random.default_rng(1000 + (chunk >> 10))
    n = chunk >> 10
    total = 16 * chunks_per_plane(chunk)
    roomy = total >= 128
    pos, holes = positions(chunk), hole_pieces(chunk)
    chunks, cases = [], []

    def noise(with_holes=False):
        b = rng.integers(0, 256, chunk, dtype=np.uint8)
        for p in holes if with_holes else ():
            b[p * 1024:(p + 1) * 1024] = 0
        return b

    def soft(with_holes=True):
        """compressible: a period of 488 random bytes, one byte in a hundred random"""
        b = np.resize(rng.integers(0, 256, 488, dtype=np.uint8), chunk).copy()
        at = rng.integers(0, chunk, chunk // 100)
        b[at] = rng.integers(0, 256, at.size, dtype=np.uint8)
        for p in holes if with_holes else ():
            b[p * 1024:(p + 1) * 1024] = 0
        return b

    def add(b):
        chunks.append(b)
        return len(chunks) - 1

    def case(name, kind, k, r, vectors=()):
        zp = [[p for p in range(n) if not chunks[c][p * 1024:(p + 1) * 1024].any()] for c in (k, r)]
        cases.append(dict(name=name, kind=kind, k=k, r=r, vectors=sorted(vectors), holes_k=zp[0], holes_r=zp[1]))

    def with_piece(base, p, piece):
        b = base.copy()
        b[p * 1024:(p + 1) * 1024] = piece
        return b

    def t():
        return int(rng.integers(1, 1 << 32))

    def family(name, base, places, twin_of_first=False):
        """A; one B per place (class 1: that vector alone differs); C == the first B (looked up against A only); A' == A behind them all"""
        a = add(base)
        first = None
        for piece, lane in places:
            b = base.copy()
            linear(b, piece, lane, t())
            k = add(b)
            first = k if first is None else first
            case("%s linear piece %d lane %d" % (name, piece, lane), "reject", k, a, [piece * 64 + lane])
        if twin_of_first:
            piece, lane = places[0]
            case("%s C == B, looked up against A" % name, "reject", add(chunks[first].copy()), a, [piece * 64 + lane])
        case("%s A' == A behind the rejected chunks" % name, "accept", add(base.copy()), a)

    def pair(name, base, p, piece_a, piece_b, lanes):
        a = add(with_piece(base, p, piece_a))
        case(name, "reject", add(with_piece(base, p, piece_b)), a, [p * 64 + lane for lane in lanes])

    zero = np.zeros(chunk, dtype=np.uint8)
    z0 = add(zero)                                                     # the first all-zero chunk: the one every other shares its frame with
    # ---- compressible chunks (frames that are gathered) ----
    if roomy:
        family("soft+holes", soft(), pos)
    # class 0: every lane of a piece vanishes, with other multipliers -- in the piece behind the last hole
    pair("class 0 vanishing piece", soft(), n - 4, vanishing_piece([t() for _ in range(64)]), vanishing_piece([t() for _ in range(64)]), range(64))
    # class 3: the term of lane 5 (row 0) moved to lane 37 (row 2), in the piece behind the first hole
    T = t()
    pair("class 3 row move", soft(), 6, single_dword_piece([(5, T)]), single_dword_piece([(37, T)]), (5, 37))
    # ---- all zero but for one bit, all-zero chunks among them ----
    top = {}
    for i, (p, lane, dw, bit) in enumerate(nearly_zero_spots(chunk)):
        b = zero.copy()
        _dwords(b, p, lane)[dw] = 1 << bit
        k = add(b)
        # (bit 31 times any of the odd constants is bit 31: the same lane's x and w give one term -- a collision nobody had to solve for)
        r = top.setdefault((p, lane), k) if bit == 31 else k
        case("nearly zero: piece %d lane %d dword %d bit %d" % (p, lane, dw, bit), "reject" if r != k else "alone", k, r, [p * 64 + lane] if r != k else [])
        if i in (1, 3):
            case("all zero behind a nearly-zero chunk", "zero", add(zero), z0)
    # ---- honest chunks up to the volume's size: nobody's duplicate, or an honest duplicate two chunks back (holes in both) ----
    tail = 2 + (1 + len(pos) + 2) + 4 + (5 if roomy else 0)            # (the noise chunks below)
    for i in range(total - len(chunks) - tail):
        if i % 3 == 2:
            case("honest duplicate with holes", "accept", add(chunks[-2].copy()), len(chunks) - 3)
        else:
            add(soft() if i % 2 else noise(True))
    # ---- noise (stored frames: the payload's tail, which stays where the transposer put it) ----
    # class 2: lane 21's one dword solved for row sums that differ in bit 0 only, in the first piece
    T = t() & ~1
    pair("class 2 forced bit", noise(), 0, single_dword_piece([(21, T)]), single_dword_piece([(21, T ^ 1)]), (21,))
    if roomy:                                                          # (small chunks compress for their holes alone: these stay stored)
        family("noise", noise(), [pos[0], pos[4], pos[-1]])
    family("noise+holes", noise(True), pos, twin_of_first=True)
    # class 4: rows 0 and 1 hash to T and -T (T odd, so the forced bit changes nothing) against the hole, in both orders
    for order in ("hole first", "zero sum first"):
        T = t() | 1
        zs, base = single_dword_piece([(3, T), (20, -T & M)]), noise(True)
        pieces = (np.zeros(1024, np.uint8), zs) if order == "hole first" else (zs, np.zeros(1024, np.uint8))
        pair("class 4 zero-sum piece against a hole, %s" % order, base, 9, pieces[0], pieces[1], (3, 20))
    assert len(chunks) == total, (len(chunks), total)
    return np.concatenate(chunks), cases


def stale_twin(stream, chunk, cases):
    """the stream with every hole of a rejected pair filled with the partner's bytes at that piece: encoded into the same destination first,
    it leaves under those holes exactly what a compare that read unwritten bytes would need to call the two chunks equal"""
    twin = stream.copy()
    for c in cases:
        if c["kind"] != "reject":
            continue
        for a, b, zp in ((c["k"], c["r"], c["holes_k"]), (c["r"], c["k"], c["holes_r"])):
            for p in zp:
                twin[a * chunk + p * 1024:a * chunk + (p + 1) * 1024] = stream[b * chunk + p * 1024:b * chunk + (p + 1) * 1024]
    return twin


def frames(payload):
    """the byte strings of the LZ4 frames of a chunked lz4 payload (one block each)"""
    out, off = [], 0
    while off < len(payload):
        assert payload[off:off + 4] == bytes([0x04, 0x22, 0x4D, 0x18])
        field = int.from_bytes(payload[off + 7:off + 11], "little")
        end = off + 7 + 4 + (field & 0x7fffffff) + 4
        assert payload[end - 4:end] == bytes(4)
        out.append(bytes(payload[off:end]))
        off = end
    return out
