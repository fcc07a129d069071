"""Streams of several LZ4 blocks built so that liblz4's block-LINKED greedy parse (one frame of linked blocks, the table carried from block to
block) contains a NAMED feature AT A BLOCK BORDER: the inputs of tests/test_lz4_linked_planted_host.py (which shows on the CPU, against the
oracle, that every stream has what it claims and that a wrong rule at the border would change its frame) and of
tests/test_gpu_lz4_linked_planted.py (the LINKED instantiations of lz4_chunks_kernel, the table re-basing, the block-parallel guess, the
verify and the redo runs).  tests/lz4_planted.py does the same for ONE block on a FRESH table; its builder and helpers are reused here.

`greedy_trace_linked` is this file's own statement of liblz4 1.9.3's parse of a sequence of blocks (LZ4_compress_fast_continue, byU32,
acceleration 1, limitedOutput with n - 1 bytes of room as LZ4F_makeBlock gives it), written from liblz4's documented behaviour and the public
hash; nothing is taken from the product or from the oracle.  Per block it is told `(start, n, fresh, low_in, low_dict)`: where the block lies,
whether its table is a new stream's, and the two limits of the backward catch-up on the match side (liblz4: `match > lowLimit`, lowLimit
chosen by where the candidate lies).  Those come from LZ4F's buffer handling and are stated here, per configuration, by the `*_layout`
functions below:

  * blocks taken from the caller's buffer inside ONE LZ4F_compressUpdate follow each other in memory: the first is in external-dictionary
    mode (or a fresh stream's), every later one in prefix mode with a dictionary that grows by a block each time;
  * after an update that took blocks from the caller, LZ4F saves the last 64 KiB into its own buffer; the next block is in
    external-dictionary mode with those 64 KiB (sources inside the block: lowLimit = the block's start, sources in the dictionary:
    lowLimit = the dictionary's start);
  * what an update leaves over (less than a block) is copied behind the saved dictionary and compressed there, in prefix mode with 64 KiB.

Two facts of the format bound what a stream can show, and the features below are stated within them:

  (a) catch-up moves ip and match together, so ip - match stays the offset that was accepted (<= 65535), and ip never falls below the
      block's start s_k.  The match side therefore never falls below s_k - 65535: a `low_dict` at or below s_k - 65536 -- every whole block
      of every layout has one -- can never be what stops a catch-up.  A history source j bytes above low_dict is in reach only from
      ip <= s_k + j - 1, where the ip side has j - 1 bytes of room: the anchor stops the catch-up one byte before low_dict would.
  (b) a match cannot span a block border (it ends at the block's own end - 5), so the "interior of a long match" across s_k - 65536 exists
      only where that line lies inside a block (blocks larger than 64 KiB).
"""
import numpy as np

import lz4_planted as P

MAXD, MFLIMIT, LASTLITERALS = P.MAXD, P.MFLIMIT, P.LASTLITERALS

# ---- the kernel's own geometry, as far as a stream is aimed at it (sqy_kernels.hip: lz4_chunks_kernel<LINKED>) ----------------------------
# A linked block is parsed at positions [LZ4_HIST, LZ4_HIST + n) of its own coordinates, the history below; a table entry is
# position << tsh | tag with tag = (seq32 * 2654435761) >> (32 - tsh) of the four bytes there; between blocks every entry moves down by the
# previous block's length and one that would fall below 0 (older than s_k - 65536) PARKS as entry 0: position 0, tag 0.
LZ4_HIST = 65536
TSH = {65536: 14, 262144: 12, 1 << 20: 10, 4 << 20: 8}
EDGE = 16                     # verdict_word's `edge` rule: a candidate less than 16 bytes above the lowest position of the coordinates


def tag_of(seq32, tsh):
    return ((seq32 * 2654435761) & 0xFFFFFFFF) >> (32 - tsh)


# ---- rules ---------------------------------------------------------------------------------------------------------------------------------
LIBLZ4 = {
    "reach": 65535,           # R1: a candidate is taken iff ip - cand <= 65535, whatever block it lies in
    "start": "entered",       # R2: a non-fresh block enters s_k and searches from s_k + 1     | "not-entered" | "searched"
    "history": "kept",        # R3: entries of earlier blocks stay, a stored block's included  | "reset-after-stored" | "reset-every-block"
    "failure": "stop",        # R4: the parse stops at the first failed output check           | "goes-on" | "nothing-entered"
    "last": 12,               # R5: the last searched position is n - 12                       | 11
    "forward": "own-end",     # R6: a match ends at the block's own end - 5                    | "past-border"
    "source": "runs-on",      # R6: the source may run over s_k into the block's own bytes     | "stops-at-border"
    "catchup": "two-limits",  # R7: low_in for a source inside the block, low_dict otherwise   | "low_dict-for-both" | "low_in=start"
                              #                                                                | "low_dict=start-65536"
    "frames": "fresh",        # R8: the first block of a frame knows nothing in front of it    | "history-kept"
}

# the wrong variants of the table; "low_dict=start-65536" is by fact (a) above NO wrong rule: it cannot change any frame
WRONG = [("reach", 65536), ("reach", 65534), ("start", "not-entered"), ("start", "searched"), ("history", "reset-after-stored"),
         ("history", "reset-every-block"), ("failure", "goes-on"), ("failure", "nothing-entered"), ("last", 11), ("forward", "past-border"),
         ("source", "stops-at-border"), ("catchup", "low_dict-for-both"), ("catchup", "low_in=start"), ("frames", "history-kept"),
         ("reach", 1 << 30)]  # (the last: no limit at all -- what taking a parked entry by its tag would amount to)
EQUIVALENT = [("catchup", "low_dict=start-65536")]


def emit_block(data, seqs):
    """the LZ4 block that holds these sequences (positions absolute in data)"""
    out = bytearray()
    for pos, lit, off, ml in seqs:
        mc = ml - 4 if ml else 0
        out.append((min(lit, 15) << 4) | min(mc, 15))
        if lit >= 15:
            r = lit - 15
            out += b"\xff" * (r // 255) + bytes([r % 255])
        out += data[pos:pos + lit]
        if ml:
            out += bytes([off & 255, (off >> 8) & 255])          # (a wrong rule's offset may not fit: its frame differs anyway)
            if mc >= 15:
                r = mc - 15
                out += b"\xff" * (r // 255) + bytes([r % 255])
    return bytes(out)


def greedy_trace_linked(data, blocks, rules=None):
    """liblz4 1.9.3's greedy parse of the blocks [(start, n, fresh, low_in, low_dict)] of `data`, the table carried over.  Per block a dict:
    seqs [(pos, lit, off, ml)] with absolute positions (the last has off = ml = 0), found [(position the match was found at before catch-up,
    probes since the last match, found by the test right behind a match)], refused {(ip, cand)} (in reach, four bytes differ), toofar
    {(ip, cand)} (refused by distance), failed None | (which check, ip of the found match or anchor), stored, block (bytes as the frame
    holds them)."""
    R = dict(LIBLZ4)
    R.update(rules or {})
    d = bytes(data)
    reach, mfl = R["reach"], R["last"]
    table, origin, out = {}, 0, []
    prev_stored = False

    def h(p):
        return P.hash5(int.from_bytes(d[p:p + 8], "little"))

    for (s, n, fresh, low_in, low_dict) in blocks:
        if (fresh and R["frames"] == "fresh") or s == 0:
            table, origin = {}, s
        elif R["history"] == "reset-every-block" or (R["history"] == "reset-after-stored" and prev_stored):
            table, origin = {}, s
        if R["catchup"] == "low_dict-for-both":
            low_in = low_dict
        elif R["catchup"] == "low_in=start":
            low_in = s
        elif R["catchup"] == "low_dict=start-65536":
            low_dict = max(s - 65536, 0) if not fresh else low_dict
        saved = dict(table) if R["failure"] == "nothing-entered" else None
        end = s + n
        olimit = n - 1
        seqs, found, refused, toofar = [], [], set(), set()
        failed = None
        op = 0
        anchor = s

        def fail(kind, where):
            nonlocal failed
            if failed is None:
                failed = (kind, where)
            return R["failure"] != "goes-on"

        def test(ip, cand):
            if cand + reach < ip:
                toofar.add((ip, cand))
                return False
            if d[cand:cand + 4] == d[ip:ip + 4]:
                return True
            refused.add((ip, cand))
            return False

        if n >= MFLIMIT + 1:
            mfl1, mlimit = end - mfl + 1, end - LASTLITERALS
            flimit = len(d) - LASTLITERALS if R["forward"] == "past-border" else mlimit
            ip = s + 1
            if R["start"] == "searched":
                ip = s
            elif R["start"] == "entered" or fresh:
                table[h(s)] = s
            done = False
            while not done:
                fwd, step, nb, U = ip, 1, 64, 0
                while True:
                    ip = fwd
                    fwd += step
                    step = nb >> 6
                    nb += 1
                    if fwd > mfl1:
                        done = True
                        break
                    hh = h(ip)
                    cand = table.get(hh, origin)
                    table[hh] = ip
                    U += 1
                    if cand < ip and test(ip, cand):
                        break
                if done:
                    break
                f, m, imm = ip, cand, False
                low = low_in if m >= s else low_dict
                while ip > anchor and m > low and d[ip - 1] == d[m - 1]:
                    ip -= 1
                    m -= 1
                stop = False
                while True:
                    lit = ip - anchor
                    if not imm:
                        op += 1                                                        # the token
                        if op + lit + 8 + lit // 255 > olimit and fail("literals", f):
                            stop = True
                            break
                        op += lit + ((lit - 15) // 255 + 1 if lit >= 15 else 0)
                    lim = flimit
                    if R["source"] == "stops-at-border" and m < s:
                        lim = min(lim, ip + (s - m))
                    ml = 4 + P._common(d, ip + 4, m + 4, lim) if ip + 4 <= lim else lim - ip
                    op += 2
                    mc = ml - 4
                    if op + 6 + (mc + 240) // 255 > olimit and fail("match", f):
                        stop = True
                        break
                    op += (mc - 15) // 255 + 1 if mc >= 15 else 0
                    seqs.append((anchor, lit, ip - m, ml))
                    found.append((f, U, imm))
                    ip += ml
                    anchor = ip
                    if ip >= mfl1:
                        done = True
                        break
                    table[h(ip - 2)] = ip - 2
                    hh = h(ip)
                    cand = table.get(hh, origin)
                    table[hh] = ip
                    if cand < ip and test(ip, cand):
                        m, f, imm, U = cand, ip, True, 0
                        op += 1                                                        # the token of a sequence without literals
                        continue
                    ip += 1
                    break
                if stop:
                    break
        last = max(end - anchor, 0)
        if failed is None or R["failure"] == "goes-on":
            if op + last + 1 + (last + 255 - 15) // 255 > olimit:
                fail("last-literals", anchor)
        if failed is None or R["failure"] == "goes-on":
            seqs.append((anchor, max(end - anchor, 0), 0, 0))       # (below 0 only under the wrong rule "past-border")
        stored = failed is not None
        if stored and saved is not None:
            table = saved
        prev_stored = stored
        out.append({"start": s, "n": n, "seqs": seqs, "found": found, "refused": refused, "toofar": toofar, "failed": failed,
                    "stored": stored, "block": d[s:end] if stored else emit_block(d, seqs)})
    return out


# ---- layouts: the per-block limits of a configuration, from LZ4F's buffer handling ---------------------------------------------------------
def ext_layout(total, B):
    """`lz4(blocksize_kb=b,framestep_kb=b)` and plain `lz4` under nthreads = 1: ONE frame, every update is ONE block.  Block 0 is a fresh
    stream.  Each later whole block is taken from the caller after an update that took a block from the caller: LZ4F saved the last 64 KiB,
    so the block is in external-dictionary mode -- a source inside it is limited by its start, one in the dictionary by s - 65536.  A rest
    of less than a block is an update of its own: copied behind the saved dictionary and compressed at the frame's end in prefix mode with
    those 64 KiB -- both limits s - 65536."""
    out = []
    for s in range(0, total, B):
        n = min(B, total - s)
        if s == 0:
            out.append((0, n, True, 0, 0))
        elif n == B:
            out.append((s, n, False, s, s - 65536))
        else:
            out.append((s, n, False, s - 65536, s - 65536))
    return out


def prefix_layout(total, B, step, f0=0, fresh=True):
    """updates of `step` = several blocks (`lz4(blocksize_kb=64)`: 256 KiB, `lz4(framestep_kb=1024)`: 1 MiB; a stream shorter than the step
    is ONE update).  The blocks of an update follow each other in the caller's buffer: the first is a fresh stream (first update) or in
    external-dictionary mode with the 64 KiB saved after the update in front; every later one is in prefix mode, its dictionary everything
    from the update's first block on -- both limits that block's start.  The rest behind the last whole block goes through the tmp buffer
    as in ext_layout."""
    out = []
    for u in range(f0, total, step):
        uend = min(u + step, total)
        for s in range(u, uend, B):
            n = min(B, uend - s)
            if n < B:
                out.append((s, n, False, s - 65536, s - 65536) if s > f0 else (s, n, True, s, s))
            elif s == u:
                out.append((s, n, True, s, s) if (u == f0 and fresh) else (s, n, False, s, s - 65536))
            else:
                out.append((s, n, False, u, u))
    return out


def chunked_layout(total, B, step):
    """nthreads >= 2 with framestep > blocksize: every `step` bytes are a frame of their own, compressed in ONE update: a fresh first
    block, then prefix mode from the frame's start"""
    out = []
    for f0 in range(0, total, step):
        out += prefix_layout(min(f0 + step, total), B, step, f0)
    return out


def tmp_layout(total, B, step):
    """updates of `step` bytes, step no multiple of B (`n_chunks_of_input`).  LZ4F_compressUpdate first completes the block waiting in its
    tmp buffer and compresses it THERE: in prefix mode behind whatever lies in front of it in the buffer (the saved 64 KiB, and the tmp
    blocks compressed since), or as a fresh stream's first block.  Then it takes whole blocks from the caller (the first in
    external-dictionary mode, further ones in prefix mode from that block on), saves 64 KiB if it took any, and copies the rest into the
    tmp buffer.  The buffer holds B + 128 KiB: when the next tmp block would not fit, the last 64 KiB are saved to its start.  The walk
    below is those steps; `hist` is the history that lies in one piece in front of the next tmp block."""
    out = []
    hist, tmp_in, fill, fill_pos = None, 0, 0, 0
    maxbuf = B + (128 << 10)

    def tmp_block(s, n):
        nonlocal hist, tmp_in
        out.append((s, n, True, s, s) if hist is None else (s, n, False, s - hist, s - hist))
        hist = (hist or 0) + n
        tmp_in += n

    for pos in range(0, total, step):
        p, end = pos, min(pos + step, total)
        if fill:
            if B - fill > end - p:
                fill += end - p
                continue
            p += B - fill
            tmp_block(fill_pos, B)
            fill = 0
        u0 = p
        while end - p >= B:
            if hist is None:
                out.append((p, B, True, p, p))
                hist = 0
            else:
                out.append((p, B, False, p, p - hist) if p == u0 else (p, B, False, u0, u0))
            p += B
        if p > u0:
            tmp_in, hist = 65536, 65536
        if tmp_in + B > maxbuf:
            tmp_in, hist = 65536, min(hist, 65536)
        if p < end:
            fill_pos, fill = p, end - p
    if fill:
        tmp_block(fill_pos, fill)
    return out


# ---- configurations ------------------------------------------------------------------------------------------------------------------------
KB = 1024
CLASS = {
    # name: (pipeline parameters, B, nthreads, layout)
    "ext64": ("blocksize_kb=64,framestep_kb=64", 64 * KB, 1, lambda t: ext_layout(t, 64 * KB)),
    "ext256": ("", 256 * KB, 1, lambda t: ext_layout(t, 256 * KB)),
    "ext1024": ("blocksize_kb=1024", 1024 * KB, 1, lambda t: ext_layout(t, 1024 * KB)),
    "ext4096": ("blocksize_kb=4096", 4096 * KB, 1, lambda t: ext_layout(t, 4096 * KB)),
    "prefix64": ("blocksize_kb=64", 64 * KB, 1, lambda t: prefix_layout(t, 64 * KB, 256 * KB)),
    "prefix256": ("framestep_kb=1024", 256 * KB, 1, lambda t: prefix_layout(t, 256 * KB, 1024 * KB)),
    "pair64": ("blocksize_kb=64,framestep_kb=128", 64 * KB, 1, lambda t: prefix_layout(t, 64 * KB, 128 * KB)),
    "chunked64": ("blocksize_kb=64,framestep_kb=128", 64 * KB, 2, lambda t: chunked_layout(t, 64 * KB, 128 * KB)),
    "tmp64": ("blocksize_kb=64,n_chunks_of_input=3", 64 * KB, 1, lambda t: tmp_layout(t, 64 * KB, t // 3)),
}
STAR_CLASSES = ("ext64", "ext256")


def pipe_of(case):
    return "lz4(%s)" % case["config"] if case["config"] else "lz4"


# ---- the builder ---------------------------------------------------------------------------------------------------------------------------
class Plant(P.Plant):
    """lz4_planted's builder with a block size: blocks are ended explicitly, and long copies do not take a Python step per byte"""

    def __init__(self, seed, B):
        super().__init__(seed)
        self.B = B

    def copy(self, off, ml):
        if ml < 256:
            return super().copy(off, ml)
        s = len(self.b) - off
        assert 1 <= off <= len(self.b) and self.b[s] != self.forbid
        left = ml
        while left:
            k = min(left, len(self.b) - s - (ml - left))
            a = s + (ml - left)
            self.b += self.b[a:a + k]
            left -= k
        self.forbid = self.b[s + ml]

    def noise(self, k):
        self.raw(self.rng.integers(0, 256, k, dtype=np.uint8).tobytes() if self.forbid is None else bytes([self._byte()]) +
                 self.rng.integers(0, 256, k - 1, dtype=np.uint8).tobytes())

    def end_block(self, s=None):
        """quiet filler, then 20 literals up to the border s (default: the next one): the block's search ends at s - 12, its last nine
        probes s - 20 .. s - 12 are entered"""
        if s is None:
            s = (len(self.b) // self.B + 1) * self.B
        assert s % self.B == 0 and len(self.b) <= s - 64, (len(self.b), s)
        self.fill_to(s - 20)
        self.lits(20)
        assert len(self.b) == s

    def quiet_blocks(self, upto):
        """whole quiet blocks until the stream is `upto` long"""
        while len(self.b) < upto:
            self.lits(24)
            self.end_block()
        assert len(self.b) == upto

    def to(self, pos):
        """literals, quiet filler and literals again so that the stream is exactly pos long and ends in literals (inside one block)"""
        assert len(self.b) // self.B == (pos - 1) // self.B or len(self.b) % self.B == 0, (len(self.b), pos)
        gap = pos - len(self.b)
        assert gap >= 0, (len(self.b), pos)
        if gap >= 60:
            self.fill_to(pos - 12)
        self.lits(pos - len(self.b))


class Ctx:
    """what a predicate sees: the stream, the layout, greedy_trace_linked's blocks, the builder's marks, the border s = s_k and k"""

    def __init__(self, case, trace):
        self.data, self.blocks, self.t, self.marks = case["data"], case["blocks"], trace, case["marks"]
        self.k = case["k"]
        self.s = case["blocks"][self.k][0]
        self.B = case["blocks"][0][1]
        self.tk = trace[self.k]

    def matches(self, k=None):
        t = self.t[self.k if k is None else k]
        return list(zip([q for q in t["seqs"] if q[3]], t["found"]))

    def first(self, k=None):
        m = self.matches(k)
        return m[0] if m else ((0, 0, 0, 0), (0, 0, False))

    def same(self, a, b, k):
        return self.data[a:a + k] == self.data[b:b + k]

    def dest_free(self, d, k=None):
        """no match of the block starts or is found within four bytes of d"""
        return not any(d - 4 <= q[0] + q[1] <= d + 4 or d - 4 <= f[0] <= d + 4 for q, f in self.matches(k))


FEATURES, STAR = {}, set()


def _feature(name, star=False):
    def deco(fn):
        FEATURES[name] = fn
        if star:
            STAR.add(name)
        return fn
    return deco


def _first_probe_off(off):
    def pred(c):
        (q, f) = c.first()
        return q[0] == c.s and q[1] == 1 and q[2] == off and f[0] == c.s + 1 and f[1] == 1 and not c.t[c.k - 1]["stored"]
    return pred


_feature("border:off=65535", True)(_first_probe_off(65535))
_feature("border:off=65534")(_first_probe_off(65534))


@_feature("border:no-match@65536", True)
def _(c):            # the same string one byte further back: the block's first probe meets it and refuses it by distance
    return (c.same(c.s + 1, c.s - 65535, 8) and (c.s + 1, c.s - 65535) in c.tk["toofar"] and c.dest_free(c.s + 1)
            and all(q[2] <= MAXD for t in c.t for q in t["seqs"]))


@_feature("start:found-at-second-byte", True)
def _(c):
    (q, f) = c.first()
    return f[0] == c.s + 1 and f[1] == 1 and q[1] == 1 and c.s - c.B <= c.s + 1 - q[2] < c.s


@_feature("start:first-byte-not-searched", True)
def _(c):            # the string at s_k stands, entered, at A; liblz4 finds s_k + 1 through C + 1 (the byte in front of C differs): one literal
    A, C = c.marks["A"], c.marks["C"]
    (q, f) = c.first()
    return (c.same(c.s, A, 8) and c.same(c.s + 1, C + 1, 7) and c.data[C] != c.data[c.s] and f[0] == c.s + 1 and q[1] == 1
            and q[2] == c.s - C and q[0] == c.s)


@_feature("start:first-byte-is-a-source", True)
def _(c):            # five bytes of s_k again at t (the sixth differs, so s_k + 1 does not hash like t + 1): found through the entry of s_k
    t = c.marks["t"]
    return any(f[0] == t and q[0] + q[1] == t and q[2] == t - c.s and q[3] == 5 for q, f in c.matches())


@_feature("prev:last-searched", True)
def _(c):
    return any(q[0] + q[1] - q[2] == c.s - 12 and f[0] == q[0] + q[1] for q, f in c.matches())


@_feature("prev:not-searched", True)
def _(c):
    t = c.marks["t"]
    return c.same(t, c.s - 11, 8) and c.data[t - 1] != c.data[c.s - 12] and c.dest_free(t)


@_feature("prev:cut-at-border", True)
def _(c):            # the last match of block k - 1 ends at s_k - 5 though the repeat goes on; block k finds it at its first probe
    q = [x for x in c.t[c.k - 1]["seqs"] if x[3]][-1]
    (q2, f2) = c.first()
    return (q[0] + q[1] + q[3] == c.s - 5 and c.same(c.s - 5, c.s - 5 - q[2], 40) and f2[0] == c.s + 1 and f2[1] == 1 and q2[0] == c.s
            and q2[1] == 0 and q2[2] % q[2] == 0)


@_feature("src:crosses-border", True)
def _(c):
    return any(q[0] + q[1] - q[2] < c.s < q[0] + q[1] - q[2] + q[3] for q, f in c.matches())


@_feature("stored:last-literals", True)
def _(c):            # block k is noise and stored; block k + 1 finds a string at a position that block k's search probed
    src = c.marks["probed"]
    return (c.tk["failed"] is not None and c.tk["failed"][0] == "last-literals" and c.s < src < c.s + c.B
            and any(q[0] + q[1] - q[2] == src for q, f in c.matches(c.k + 1)))


def _fails(kind):
    def pred(c):
        q, x, dq, dx = c.marks["q"], c.marks["X"], c.marks["dq"], c.marks["dX"]
        return (c.tk["failed"] == (kind, q) and q >= c.s + c.B - c.B // 256 and c.same(x, dx, 8) and c.dest_free(dx, c.k + 1) and x > q
                and any(g[0] + g[1] == dq and g[2] == dq - q for g, f in c.matches(c.k + 1)))
    return pred


_feature("stored:fails-at-match", True)(_fails("literals"))
_feature("stored:fails-second-check")(_fails("match"))


@_feature("catchup:stops-at-block-start", True)
def _(c):            # the bytes in front of s_k and in front of the destination are equal; the source is s_k itself, and the catch-up stops there
    t = c.marks["t"]
    return (c.same(t - 4, c.s - 4, 12) and c.blocks[c.k][3] == c.s and any(f[0] == t and g[0] + g[1] == t and g[2] == t - c.s for g, f in c.matches()))


@_feature("catchup:through-block-start")
def _(c):
    t = c.marks["t"]
    return (c.same(t - 4, c.s - 4, 12) and c.blocks[c.k][3] < c.s - 4 and any(f[0] == t and g[0] + g[1] == t - 4 and g[2] == t - c.s for g, f in c.matches()))


for _K in (1, 63, 64, 65, 300):
    @_feature("catchup:through-block-start=%d" % _K)
    def _(c, K=_K):  # prefix mode: found at a source inside block k, the match side walks K bytes back, over s_k into block k - 1
        return any(g[0] + g[1] - g[2] == c.s - K and c.s <= f[0] - g[2] <= c.s + 2 for g, f in c.matches())


@_feature("catchup:dict-start", True)
def _(c):            # a history source 2 bytes above low_dict, in reach only from s_k + 1: by fact (a) the anchor stops the catch-up at low_dict + 1
    (q, f) = c.first()
    low = c.blocks[c.k][4]
    return low == c.s - 65536 and f[0] == c.s + 1 and q[0] + q[1] == c.s and q[2] == 65535 and c.data[c.s - 1] == c.data[low]


@_feature("catchup:tmp-buffer")
def _(c):            # a block compressed in LZ4F's tmp buffer (prefix mode behind the tmp block in front): catch-up over its start
    t = c.marks["t"]
    return c.blocks[c.k][3] < c.s - 4 and any(f[0] == t and g[0] + g[1] == t - 4 for g, f in c.matches())


@_feature("frame:no-history")
def _(c):
    return c.blocks[c.k][2] and c.same(c.s + 1, c.marks["src"], 8) and c.dest_free(c.s + 1) and not c.tk["toofar"]


for _n in (1, 4, 12, 13, 14, 17, 31):
    @_feature("last:n=%d" % _n)
    def _(c, n=_n):
        t = c.t[-1]
        if t["n"] != n:
            return False
        if n < 13:
            return t["stored"] and not t["found"]
        return len(t["found"]) == 1 and t["found"][0][0] == t["start"] + 1 and t["found"][0][1] == 1 and t["start"] + 1 - t["seqs"][0][2] < t["start"]


@_feature("parked:tag0", True)
def _(c):            # four bytes whose tag is 0, entered more than 64 KiB in front of s_k and never overwritten: the probe meets an entry the re-basing parked
    z, t = c.marks["Z"], c.marks["t"]
    seq = int.from_bytes(c.data[t:t + 4], "little")
    return tag_of(seq, TSH[c.B]) == 0 and z < c.s - 65536 and (t, z) in c.tk["toofar"] and c.same(t, z, 8) and c.dest_free(t)


@_feature("parked:boundary")
def _(c):
    return all((t, z) in c.tk["toofar"] and c.same(t, z, 5) and c.dest_free(t) for t, z in c.marks["pairs"]) \
        and sorted(z - (c.s - 65536) for t, z in c.marks["pairs"]) == [-1, 0, 1]


@_feature("edge:history-candidate<16")
def _(c):
    return any(0 < g[0] + g[1] - g[2] - (c.s - 65536) < EDGE for g, f in c.matches())


@_feature("edge:back_room<4")
def _(c):
    lo_in, lo_d = c.blocks[c.k][3], c.blocks[c.k][4]
    m = [f[0] - g[2] for g, f in c.matches()]
    return any(0 <= x - lo_d < 4 for x in m if x < c.s) and any(0 <= x - lo_in < 4 for x in m if x >= c.s)


@_feature("dense:history-sources")
def _(c):
    run = 0
    for g, f in c.matches():
        if not (g[3] < 16 and g[0] + g[1] - g[2] < c.s):
            break
        run += 1
    return run >= 40


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def _case(name, cls, p, feats, k=2, rules=()):
    cfg, B, nthreads, layout = CLASS[cls]
    data = p.bytes()
    return {"name": "%s-%s" % (name, cls), "cls": cls, "config": cfg, "nthreads": nthreads, "data": data, "blocks": layout(len(data)),
            "marks": p.marks, "features": list(feats), "k": k, "rules": list(rules)}


def _head(seed, cls, k=2):
    """k - 1 quiet blocks: the subject border lies between blocks k - 1 and k"""
    p = Plant(seed, CLASS[cls][1])
    p.quiet_blocks((k - 1) * p.B)
    return p


def _reach(cls, seed, off):
    """a string in block k - 1 (searched at step 1) exactly `off` bytes in front of s_k + 1; 65535: byte 2 of block k - 1 in the 64 KiB class"""
    p = _head(seed, cls)
    s = 2 * p.B
    src = s + 1 - off
    p.to(src - min(10, src - p.B))
    p.lits(30)
    p.end_block()
    p.seq(1, off, 8)
    p.lits(20)
    p.end_block()
    if off > MAXD:
        return _case("no-match@%d" % off, cls, p, ["border:no-match@65536"], rules=[("reach", 65536)])
    feats = ["border:off=%d" % off, "start:found-at-second-byte"] if off >= 65534 else ["start:found-at-second-byte"]
    return _case("off=%d" % off, cls, p, feats, rules=[("reach", 65534), ("history", "reset-every-block")] if off == 65535 else [("history", "reset-every-block")])


def _not_searched(cls, seed):
    p = _head(seed, cls)
    s = 2 * p.B
    p.lits(24)
    p.fill_to(s - 3000)
    p.lits(12)
    x = bytes(p._byte() for _ in range(10))
    a = len(p); p.raw(x); p.lits(12)                     # A: the string, every position of it entered
    c = len(p) + 1
    p.seq_from(1, a + 1, 9)                              # C: another first byte, then x[1:]: position C + 1 takes the bucket of x[1:6]
    assert p.b[c - 1] != x[0]
    p.marks.update(A=a, C=c - 1)
    p.end_block()
    assert p.b[-1] != p.b[a - 1]
    p.raw(x)
    p.forbid = p.b[a + 10]
    p.lits(20)
    p.end_block()
    return _case("first-byte-not-searched", cls, p, ["start:first-byte-not-searched"], rules=[("start", "searched")])


def _is_a_source(cls, seed):
    p = _head(seed, cls)
    p.lits(24)
    p.end_block()
    s = len(p)
    p.lits(40)
    t = len(p) + 6
    p.seq_from(6, s, 5)
    p.marks["t"] = t
    p.lits(20)
    p.end_block()
    return _case("first-byte-is-a-source", cls, p, ["start:first-byte-is-a-source"], rules=[("start", "not-entered")])


def _prev_end(cls, seed, back):
    """a copy, in block k, of the bytes `back` in front of s_k: 12 is the last position block k - 1 searched (the copy runs on over s_k
    into block k's own first bytes), 11 was never entered"""
    p = _head(seed, cls)
    p.lits(24)
    p.end_block()
    s = len(p)
    p.lits(30)
    t = len(p) + 6
    p.seq_from(6, s - back, 20 if back == 12 else 8)
    p.marks["t"] = t
    p.lits(20)
    p.end_block()
    if back == 12:
        return _case("prev-last-searched", cls, p, ["prev:last-searched", "src:crosses-border"], rules=[("source", "stops-at-border")])
    return _case("prev-not-searched", cls, p, ["prev:not-searched"], rules=[("last", 11)])


def _cut(cls, seed):
    p = _head(seed, cls)
    s = 2 * p.B
    p.to(s - 3000)
    p.seq(9, 9, 3000 - 9 + 600)                          # a repeat of period 9 from 3000 bytes in front of s_k to 600 behind it
    p.lits(20)
    p.end_block()
    return _case("cut-at-border", cls, p, ["prev:cut-at-border"], rules=[("forward", "past-border")])


def search_positions(anchor, limit):
    """the positions <= limit that liblz4 probes after a match that ended at `anchor` (or from a block's start) while it finds nothing: the
    step in front of probe k + 1 is the one computed at probe k - 1, (64 + k - 1) >> 6 -- 66 probes a byte apart, then 64 two apart, ...
    (lz4_planted.probe_positions changes its step one probe early; its one user reaches its destination by catch-up and does not notice)"""
    out, p, step, nb = [], anchor + 1, 1, 64
    while p <= limit:
        out.append(p)
        p += step
        step = nb >> 6
        nb += 1
    return out


def _noise_probes(B):
    """the positions, relative to its start, that the search of a whole block of noise probes (it finds nothing)"""
    return search_positions(0, B - 12)


def _stored(cls, seed, kind):
    """block 2 is noise.  last-literals: nothing found, the block fails at its end; block 3 copies a probed string of it.
    literals / match: one planted match at a probed position q in the block's last B/256 bytes fails the first / the second output check;
    block 3 copies the string at q (entered: found) and a string X behind it (never entered: stays literal)."""
    p = _head(seed, cls)
    B = p.B
    p.lits(24)
    p.end_block()
    s = len(p)
    probes = [s + q for q in _noise_probes(B)]
    p.noise(B)
    feats, rules = ["stored:last-literals"], [("history", "reset-after-stored")]
    if kind == "last-literals":
        src = probes[-6]
        p.marks["probed"] = src
        p.seq_from(30, src, 8)
    else:
        lit_max = max(l for l in range(B) if 1 + l + 8 + l // 255 <= B - 1)      # the longest literal run that passes the first check
        if kind == "literals":
            q = next(x for x in probes if x - s > lit_max and x >= s + B - B // 256 + 8)
            ml = 8
            start = q
        else:
            # the copy starts at the longest literal run that still passes the first check; the first probe behind that start finds it and
            # the catch-up walks back to it.  Then every match of 19 bytes or more fails the second check.
            start = s + lit_max
            q = next(x for x in probes if x >= start)
            ml = s + B - 5 - start - 24
            assert 1 + (lit_max - 15) // 255 + 1 + lit_max + 2 + 6 + (ml - 4 + 240) // 255 > B - 1 and q >= s + B - B // 256, (q - s, ml)
        qs = max(x for x in probes if x <= start - ml - 64)                      # a probed position not far up: its bucket is still its own
        q0 = qs - (q - start)                                                    # the probe at q meets the entry of qs
        p.b[start:start + ml] = p.b[q0:q0 + ml]
        if p.b[start - 1] == p.b[q0 - 1]:
            p.b[start - 1] ^= 1
        if p.b[start + ml] == p.b[q0 + ml]:
            p.b[start + ml] ^= 1
        x = start + ml + 3
        p.marks.update(q=q, X=x)
        assert x + 8 <= s + B - 5
        p.lits(30)
        p.marks["dq"] = len(p) + 5
        p.seq_from(5, q, 8)
        p.lits(12)
        p.marks["dX"] = len(p) + 5
        p.seq_from(5, x, 8)
        feats = ["stored:fails-at-match" if kind == "literals" else "stored:fails-second-check"]
        rules = [("failure", "goes-on"), ("failure", "nothing-entered")]
    p.lits(20)
    p.end_block()
    return _case("stored-%s" % kind, cls, p, feats, rules=rules)


def _block_start_catchup(cls, seed, name, feats, rules, k=2, tail=0):
    """the four bytes in front of s_k and block k's first eight, again at t - 4 in block k: s_k - 4 .. s_k - 1 were never entered, s_k was"""
    p = _head(seed, cls, k)
    p.lits(24)
    p.end_block()
    s = len(p)
    p.lits(40)
    p.lits(5, last_not=p.b[s - 5])
    t = len(p) + 4
    p.copy(t - s, 12 + 4 - 4)
    p.marks["t"] = t
    p.lits(20)
    p.end_block()
    p.lits(tail)
    return _case(name, cls, p, feats, k=k, rules=rules)


def _through(seed, K):
    """prefix mode (1 MiB updates of 256 KiB blocks).  Block k - 1 ends in ONE long match M (the copy of a string S that lies just in reach of M's
    start and out of reach of everything in block k) and five literals: none of the K bytes in front of s_k was ever entered, s_k is.  Those K bytes and block k's
    first twelve stand again further on in block k behind K + 8 literals: the search meets nothing until it is K bytes (or, at a step of
    two, K + 1) into the copy, where the entry of s_k (s_k + 1) answers; the catch-up walks back over s_k, K bytes into block k - 1"""
    cls = "prefix256"
    p = _head(seed, cls)
    s = 2 * p.B
    p.to(s - 65536 - K - 30)                            # S: in reach of M's start (65531 bytes), out of reach of block k's copy
    s0 = len(p)
    p.lits(K + 30)
    p.fill_to(s - 5 - (K + 30) - 6)
    p.seq_from(6, s0, K + 30)
    p.lits(5)
    assert len(p) == s
    p.lits(60)
    p.seq(8, 8, 40)
    p.lits(K + 8, last_not=p.b[s - K - 1])
    p.copy(len(p) - (s - K), K + 12)
    p.lits(20)
    p.end_block()
    return _case("through-block-start=%d" % K, cls, p, ["catchup:through-block-start=%d" % K], rules=[("catchup", "low_in=start")])


def _dict_start(cls, seed):
    """the bytes at low_dict .. low_dict + 10 (block k - 1's first in the 64 KiB class, a literal run otherwise) again at s_k - 1 .. : the
    block's first probe, s_k + 1, meets low_dict + 2 at offset 65535, and the catch-up takes one byte and stands at the anchor with the
    match side at low_dict + 1 and another equal byte in front of both"""
    p = _head(seed, cls)
    s = 2 * p.B
    low = s - 65536
    if low > p.B:
        p.to(low)
    p.lits(40)
    p.to(s - 1)
    p.b.append(p.b[low])
    p.forbid = None
    assert len(p) == s
    p.raw(bytes(p.b[low + 1:low + 2]))
    p.copy(65535, 9)
    p.lits(20)
    p.end_block()
    return _case("dict-start", cls, p, ["catchup:dict-start", "edge:history-candidate<16"], rules=[("history", "reset-every-block")])


def _frames(cls, seed):
    p = _head(seed, cls)
    p.lits(30)
    src = len(p) - 20
    p.end_block()
    p.seq_from(1, src, 8)
    p.marks["src"] = src
    p.lits(20)
    p.end_block()
    if cls == "chunked64":
        return _case("frame-no-history", cls, p, ["frame:no-history"], rules=[("frames", "history-kept")])
    return _case("frame-one", cls, p, ["start:found-at-second-byte"], rules=[("history", "reset-every-block")])


def _last(seed, r):
    cls = "ext64"
    p = _head(seed, cls, 3)
    p.lits(24)
    p.end_block()
    s = len(p)
    if r >= 13:
        p.seq_from(1, s - 16, 12)                       # (13 bytes: the copy of s_k - 16, probed at step 1, is cut at the block's end - 5)
        p.lits(r - 13)
    else:
        p.lits(r)
    assert len(p) == s + r
    return _case("last-%d" % r, cls, p, ["last:n=%d" % r], k=3)


def _tag0_string(rng, tsh):
    while True:
        v = rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64)
        hit = np.nonzero(((v * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - tsh) == 0)[0]
        for i in hit.tolist():
            b = int(v[i]).to_bytes(4, "little")
            if len(set(b)) == 4:
                return b


def _parked(cls, seed):
    """Z: four bytes of tag 0 and four more, in a literal run of block k - 2 (64 KiB blocks) or early in block k - 1; quiet filler up to
    s_k; in block k the same eight bytes: the bucket still holds Z's entry, which the re-basing parked"""
    B = CLASS[cls][1]
    s = 2 * B
    p = Plant(seed, B) if B == 65536 else _head(seed, cls)
    p.lits(24)
    z = len(p) + 6
    p.lits(6)
    p.raw(_tag0_string(p.rng, TSH[B]))
    p.lits(14)
    if B == 65536:
        p.quiet_blocks(s)
    else:
        p.end_block()
    assert z < s - 65536
    p.lits(30)
    t = len(p) + 5
    p.seq_from(5, z, 8)
    p.marks.update(Z=z, t=t)
    p.lits(20)
    p.end_block()
    return _case("parked-tag0", cls, p, ["parked:tag0"], rules=[("reach", 1 << 30)])


def _parked_boundary(cls, seed):
    p = _head(seed, cls)
    s = 2 * p.B
    p.to(s - 65536 - 20)
    p.lits(40)                                           # (52 literals in a row: every one of them probed)
    p.end_block()
    p.lits(8)                                            # (all three destinations among the block's first 66 probes: a byte apart)
    pairs = []
    for j in (-1, 0, 1):
        t = len(p) + 5
        p.seq_from(5, s - 65536 + j, 5)                  # (five bytes each: the three strings overlap, a sixth byte would let them find each other)
        pairs.append((t, s - 65536 + j))
        p.lits(6)
    p.marks["pairs"] = pairs
    p.end_block()
    return _case("parked-boundary", cls, p, ["parked:boundary"], rules=[("reach", 1 << 30)])


def _back_room(cls, seed):
    """a history candidate at low_dict + 3 (probed from s_k + 2, see _dict_start) and in-block candidates at low_in + 0 .. + 2"""
    p = _head(seed, cls)
    s = 2 * p.B
    low = s - 65536
    p.to(low)
    p.lits(40)
    p.end_block()
    p.lits(2)
    p.copy(65535, 8)
    p.lits(30)
    for j in (0, 1, 2):
        p.seq_from(6, s + j, 7)                          # s_k (entered), s_k + 1 and s_k + 2 (probed): 0 .. 2 bytes above low_in
    p.lits(20)
    p.end_block()
    return _case("back-room", cls, p, ["edge:back_room<4", "edge:history-candidate<16"], rules=[("history", "reset-every-block")])


def _dense(cls, seed):
    p = _head(seed, cls)
    p.lits(24)
    p.fill_to(2 * p.B - 1400)
    starts = []
    for _ in range(60):
        starts.append(len(p))
        p.seq(14, 14, 5)
    p.lits(2 * p.B - len(p))
    for a in starts[:56]:
        p.seq_from(3, a + 3, 7)
    p.lits(20)
    p.end_block()
    return _case("dense-history-sources", cls, p, ["dense:history-sources"], rules=[("history", "reset-every-block")])


_cases = None


def cases():
    """the list of named streams: {"name", "cls", "config", "nthreads", "data", "blocks" (the per-block limits it states), "marks",
    "features", "k" (the subject border lies in front of block k), "rules" (the wrong rules it is there to catch)}"""
    global _cases
    if _cases is not None:
        return _cases
    out, seed = [], 5000

    def S(name):
        nonlocal seed
        seed += 1
        return SEEDS.get(name, seed)
    bs = {"64": S("bs64"), "256": S("bs256")}            # the same bytes under external-dictionary and under prefix mode
    for cls in STAR_CLASSES:
        out.append(_reach(cls, S("reach35" + cls), 65535))
        out.append(_reach(cls, S("reach36" + cls), 65536))
        out.append(_reach(cls, S("second" + cls), 1000))
        out.append(_not_searched(cls, S("notsearched" + cls)))
        out.append(_is_a_source(cls, S("source" + cls)))
        out.append(_prev_end(cls, S("prev12" + cls), 12))
        out.append(_prev_end(cls, S("prev11" + cls), 11))
        out.append(_cut(cls, S("cut" + cls)))
        out.append(_stored(cls, S("stored-ll" + cls), "last-literals"))
        out.append(_stored(cls, S("stored-lit" + cls), "literals"))
        out.append(_block_start_catchup(cls, bs[cls[3:]], "stops-at-block-start", ["catchup:stops-at-block-start"], [("catchup", "low_dict-for-both")]))
        out.append(_dict_start(cls, S("dict" + cls)))
        out.append(_parked(cls, S("parked" + cls)))
    out.append(_reach("ext64", S("reach34"), 65534))
    out.append(_stored("ext64", S("stored-match"), "match"))
    for cls in ("prefix64", "prefix256"):
        out.append(_block_start_catchup(cls, bs[cls[6:]], "through-block-start", ["catchup:through-block-start"], [("catchup", "low_in=start")]))
    for K in (1, 63, 64, 65, 300):
        out.append(_through(S("through%d" % K), K))
    # 3 * 64 KiB + 31 bytes in three updates of 65546: block 0 from the caller, blocks 1 and 2 completed in the tmp buffer (64 and 128 KiB
    # in front of them there), the last 31 bytes behind the 64 KiB saved when the buffer was full
    out.append(_block_start_catchup("tmp64", S("tmp"), "tmp-buffer", ["catchup:tmp-buffer"], [("catchup", "low_in=start")], tail=31))
    sf = S("frames")                                     # the same bytes as one frame and as a frame per two blocks
    out.append(_frames("pair64", sf))
    out.append(_frames("chunked64", sf))
    for r in (1, 4, 12, 13, 14, 17, 31):
        out.append(_last(S("last%d" % r), r))
    out.append(_parked_boundary("ext256", S("pb")))
    out.append(_back_room("ext64", S("br")))
    out.append(_dense("ext64", S("dense64")))
    out.append(_dense("ext256", S("dense256")))
    for cls in ("ext1024", "ext4096"):
        out.append(_reach(cls, S("reach35" + cls), 65535))
        out.append(_parked(cls, S("parked" + cls)))
    assert len({c["name"] for c in out}) == len(out)
    _cases = out
    return out


# seeds at which every planned sequence is liblz4's (see lz4_planted.SEEDS); the host test asserts the features
SEEDS = {}


def trace_of(case, rules=None):
    return greedy_trace_linked(case["data"], case["blocks"], rules)


def oracle_frame(oracle, case):
    d = np.frombuffer(case["data"], np.uint8)
    cfg = oracle.Lz4Config(case["config"])
    return bytes(oracle.lz4_encode_serial(d, cfg) if case["nthreads"] == 1 else oracle.lz4_encode_chunked(d, cfg))


def liblz4_frame(ref, oracle, case):
    """the same frame from liblz4 itself (oracle/ref.py), fed as the reference feeds it"""
    d = np.frombuffer(case["data"], np.uint8)
    cfg = oracle.Lz4Config(case["config"])
    chunk = cfg.bytes_per_chunk(len(d))
    if case["nthreads"] == 1:
        return bytes(ref.lz4_encode_serial(d, framestep=chunk, block_id=cfg.block_id))
    return bytes(ref.lz4_encode_parallel(d, chunk=chunk, block_id=cfg.block_id))
