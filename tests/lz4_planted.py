"""Byte streams built sequence by sequence so that liblz4's greedy parse (acceleration 1) contains a NAMED feature at a NAMED place: the
inputs of tests/test_lz4_planted_host.py (which shows on the CPU, against the oracle, that every stream has what it claims) and of
tests/test_gpu_lz4_planted.py (which sends them through every instantiation of lz4_chunks_kernel).

A stream is written as the decoder would read it -- literals, then a byte-wise copy -- and the greedy encoder has to find what was written.
liblz4 only knows a position that a probe visited, so

  * a match source lies in a literal run that was searched at step 1 (fewer than 64 probes since the last match), or at `end - 2` of a match
    (the one position liblz4 enters after a match), or is the position probed right after a match;
  * the byte in front of the destination differs from the byte in front of the source (unless backward catch-up is the feature), and the
    byte behind the copy differs from the continuation, so the match starts and ends where planned;
  * a match is found through the hash of FIVE bytes, and two strings that differ in the fifth byte alone never hash alike (the multiplier is
    odd), so a match of exactly four bytes is found only through a bucket that nothing has entered yet: it reads as position 0, and the
    four bytes are the chunk's first;
  * between a far source and its destination lies one long match (`fill_to`): it enters three positions into the table, so the source's
    bucket survives.  Random literals would overwrite it (4096 buckets).

`greedy_trace` is this file's own statement of the parse, with what the block itself does not say: where a match was FOUND (before backward
catch-up), after how many probes, which candidates were refused.  The host test holds it to the oracle's block on every case; features that
are about the search (catch-up, buckets, the chunk end) are predicates over it.  Nothing here is taken from the product or from liblz4's
sources; the hash is the public formula."""
import numpy as np

PRIME5 = 889523592379
MAXD = 65535
MFLIMIT = 12
LASTLITERALS = 5


def hash5(seq):
    """liblz4's 5-byte hash of a little-endian read at a position: ((seq << 24) * 889523592379) >> 52 in 64 bits; bytes or an int"""
    if not isinstance(seq, int):
        seq = int.from_bytes(bytes(seq[:8]), "little")
    return (((seq << 24) * PRIME5) & 0xFFFFFFFFFFFFFFFF) >> 52


def _hash5_array(v):
    v = v.astype(np.uint64)
    return ((v << np.uint64(24)) * np.uint64(PRIME5)) >> np.uint64(52)


def parse_block(block):
    """the sequences of one LZ4 block: [(pos, lit, off, ml)], pos the input position of the sequence's first literal; the last has off = ml = 0"""
    block = bytes(block)
    i, pos, out = 0, 0, []
    while i < len(block):
        tok = block[i]; i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = block[i]; i += 1; lit += b
                if b != 255:
                    break
        i += lit
        if i >= len(block):
            out.append((pos, lit, 0, 0))
            break
        off = block[i] | (block[i + 1] << 8); i += 2
        ml = (tok & 15) + 4
        if (tok & 15) == 15:
            while True:
                b = block[i]; i += 1; ml += b
                if b != 255:
                    break
        out.append((pos, lit, off, ml))
        pos += lit + ml
    return out


def first_difference(a, b, names=("got", "want")):
    """the first sequence at which two blocks differ, from both sides: position, literals, offset, length -- for assertion messages"""
    def seqs(x):
        try:
            return parse_block(x), ""
        except IndexError:
            return [], " (block does not parse)"
    (sa, ea), (sb, eb) = seqs(a), seqs(b)

    def show(s, i):
        return "pos %d lit %d off %d ml %d" % s[i] if i < len(s) else "no such sequence"
    for i in range(max(len(sa), len(sb))):
        if i >= len(sa) or i >= len(sb) or sa[i] != sb[i]:
            return "blocks of %d / %d bytes differ at sequence %d: %s%s: %s | %s%s: %s" % (len(a), len(b), i, names[0], ea, show(sa, i), names[1], eb, show(sb, i))
    return "blocks of %d / %d bytes hold the same %d sequences%s%s" % (len(a), len(b), len(sa), ea, eb)


def _common(d, a, b, limit):
    """number of i with d[a + i] == d[b + i] from i = 0 on, a + i < limit"""
    c, w = 0, 32
    while a + c < limit:
        k = min(w, limit - a - c)
        if d[a + c:a + c + k] == d[b + c:b + c + k]:
            c += k
            w = min(w * 2, 1 << 16)
        elif k > 16:
            w = k // 2
        else:
            while d[a + c] == d[b + c]:
                c += 1
            return c
    return c


def probe_positions(anchor, count):
    """the positions liblz4 probes after a match that ended at `anchor` (or from the chunk's start, anchor = 0) while it finds nothing:
    probe k stands at anchor + 1 + sum of the steps, the step after probe k is (64 + k) >> 6"""
    out, p = [], anchor + 1
    for k in range(count):
        out.append(p)
        p += (64 + k) >> 6
    return out


def greedy_trace(data):
    """liblz4 1.9.3's greedy parse of one block on a fresh table (byU32, acceleration 1), restated: returns (seqs, found, refused) --
    seqs as parse_block gives them, found[i] = (position the i-th match was found at before catch-up, probes since the last match,
    found by the test right behind a match), refused = {(position, candidate)} of candidates inside the window whose four bytes differ"""
    d = bytes(data)
    n = len(d)
    seqs, found, refused = [], [], set()
    if n < MFLIMIT + 1:
        return [(0, n, 0, 0)], found, refused
    table = {}

    def h(p):
        return hash5(int.from_bytes(d[p:p + 8], "little"))
    mfl1, mlimit = n - MFLIMIT + 1, n - LASTLITERALS
    anchor, ip = 0, 1
    table[h(0)] = 0
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
            cand = table.get(hh, 0)
            table[hh] = ip
            U += 1
            if cand + MAXD < ip:
                continue
            if d[cand:cand + 4] == d[ip:ip + 4]:
                break
            refused.add((ip, cand))
        if done:
            break
        f, m, imm = ip, cand, False
        while ip > anchor and m > 0 and d[ip - 1] == d[m - 1]:
            ip -= 1
            m -= 1
        while True:
            ml = 4 + _common(d, ip + 4, m + 4, mlimit)
            seqs.append((anchor, ip - anchor, ip - m, ml))
            found.append((f, U, imm))
            ip += ml
            anchor = ip
            if ip >= mfl1:
                done = True
                break
            table[h(ip - 2)] = ip - 2
            hh = h(ip)
            cand = table.get(hh, 0)
            table[hh] = ip
            if cand + MAXD >= ip:
                if d[cand:cand + 4] == d[ip:ip + 4]:
                    m, f, imm, U = cand, ip, True, 0
                    continue
                refused.add((ip, cand))
            ip += 1
            break
    seqs.append((anchor, n - anchor, 0, 0))
    return seqs, found, refused


# ---- the kernel's geometry, as far as a stream is aimed at it (sqy_kernels.hip: Lz4WindowT, LZ4_WIN_LEAN, LZ4_FB, LZ4_AHEAD) -----------
WIN, FB, AHEAD = 8192, 1024, 2048


def ring_lows(ip):
    """The first resident position wlo of the lean ring while the parse stands at ip, in the steady state.  Lz4WindowT::ensure(ip) returns at
    once while ip + AHEAD <= whi; otherwise it fetches whole blocks of FB bytes until whi >= ip + AHEAD, so whi = roundup(ip + AHEAD, FB) for the
    ip that last moved it -- the ip in hand, or one up to FB - 1 bytes in front of it.  It then leaves the block [whi, whi + FB) in flight, and
    issue() gives up that block's slot beforehand: wlo = whi + FB - WIN.  Before that issue (and at the chunk's end, where nothing more is in
    flight) wlo = whi - WIN.  Both are returned; a source at wlo - 1, wlo, wlo + 1 is just outside / just inside the ring."""
    whi = (ip + AHEAD + FB - 1) // FB * FB
    return (whi + FB - WIN, whi - WIN)


class Plant:
    """writes a stream sequence by sequence; `forbid` is the byte that must not come next (it would lengthen the copy just written)"""

    def __init__(self, seed):
        self.b = bytearray()
        self.rng = np.random.default_rng(seed)
        self.forbid = None
        self.pool = []
        self.runs = []                # starts of literal runs written by seq(): sources that were probed at step 1
        self.marks = {}

    def __len__(self):
        return len(self.b)

    def _byte(self, *avoid):
        while True:
            if not self.pool:
                self.pool = self.rng.integers(0, 256, 4096).tolist()
            v = self.pool.pop()
            if v != self.forbid and v not in avoid:
                self.forbid = None
                return v

    def lits(self, k, last_not=None):
        self.runs.append(len(self.b))
        for i in range(k):
            self.b.append(self._byte(last_not) if i == k - 1 and last_not is not None else self._byte())

    def raw(self, bs):
        bs = bytes(bs)
        assert bs and bs[0] != self.forbid, "the copy in front would run on into these bytes"
        self.forbid = None
        self.b += bs

    def copy(self, off, ml):
        assert 1 <= off <= len(self.b)
        s = len(self.b) - off
        assert self.b[s] != self.forbid or ml == 0, "the copy in front would run on into this one"
        for i in range(ml):
            self.b.append(self.b[s + i])
        self.forbid = self.b[s + ml]

    def seq(self, lit, off, ml):
        """one planned sequence: lit literals, then ml bytes from off bytes back; the byte in front of the copy differs from the byte in
        front of its source"""
        s = len(self.b) + lit - off
        assert s >= 0, (lit, off)
        if lit:
            self.lits(lit - 1)
            self.b.append(self._byte(self.b[s - 1]) if s >= 1 else self._byte())
        self.copy(off, ml)

    def recent(self, back=1, skip=1):
        """a source that was probed at step 1: `skip` bytes into the back-th last literal run"""
        return self.runs[-back] + skip

    def seq_from(self, lit, src, ml):
        self.seq(lit, len(self.b) + lit - src, ml)

    def fill_to(self, pos):
        """quiet filler up to position pos: eight literals and one long match at offset 8 (positions entered: the nine it searches, end - 2)"""
        gap = pos - len(self.b)
        assert gap >= 0, (pos, len(self.b))
        if gap < 24:
            self.lits(gap)
        else:
            self.seq(8, 8, gap - 8)

    def far(self, off, lit=5, ml=8, mark=None):
        """a source run of 30 literals, quiet filler, then `lit` literals and a copy of ml bytes from exactly `off` back"""
        r0 = len(self.b)
        self.lits(30)
        self.fill_to(r0 + 10 + off - lit)
        if mark:
            self.marks[mark] = r0 + 10 + off
        self.seq(lit, off, ml)
        assert len(self.b) - ml - off == r0 + 10

    def collide(self, fixed, like=None):
        """two strings of five bytes with the same hash5 that share their first `fixed` bytes and differ in the next one; `like`: the first is given"""
        assert fixed < 4, "strings that differ in the fifth byte alone never hash alike"
        while True:
            a = bytes(like) if like is not None else bytes(self._byte() for _ in range(5))
            self.forbid = None
            free = 5 - fixed if fixed >= 3 else 2
            head = a[:5 - free] if fixed >= 3 else bytes(self._byte(a[0]) for _ in range(3))
            v = np.arange(256 ** free, dtype=np.uint64) << np.uint64(8 * (5 - free))
            v += np.uint64(int.from_bytes(head, "little"))
            hit = np.nonzero(_hash5_array(v) == np.uint64(hash5(a)))[0]
            for x in hit.tolist():
                c = int(v[x]).to_bytes(5, "little")
                if c[fixed] != a[fixed]:
                    assert hash5(c) == hash5(a) and c[:fixed] == a[:fixed]
                    return a, c

    def bytes(self):
        return bytes(self.b)


# ---- features ---------------------------------------------------------------------------------------------------------------------------
class Ctx:
    """what a predicate sees: the stream, the oracle's sequences, greedy_trace's record of the search, the builder's marks, the block's size"""

    def __init__(self, data, seqs, found, refused, marks, csize):
        self.data, self.n, self.seqs, self.found, self.refused, self.marks, self.csize = data, len(data), seqs, found, refused, marks, csize
        self.matches = [s for s in seqs if s[3]]

    def short_runs(self):
        """lengths of the maximal runs of matches shorter than 16 bytes, each with the number of longer matches that follow it"""
        out, run, i = [], 0, 0
        m = self.matches
        while i < len(m):
            if m[i][3] < 16:
                run += 1
                i += 1
                continue
            j = i
            while j < len(m) and m[j][3] >= 16:
                j += 1
            if run:
                out.append((run, j - i))
            run, i = 0, j
        if run:
            out.append((run, 0))
        return out


STAR_LIT = (0, 1, 14, 15, 16, 63, 64, 65)
STAR_ML = (4, 5, 15, 16, 17, 18, 19, 20)
STAR_OFF = (1, 2, 3, 4, 7, 8, 15, 16, 17)
LITS = STAR_LIT + (269, 270, 271, 524, 525, 2047, 2048, 2049, 5000)
MLS = STAR_ML + (273, 274, 275, 1023, 1024, 1025, 1027, 1028, 1029, 8200, 33000)
RING_OFFS = (7167, 7168, 7169, 8175, 8176, 8177, 8191, 8192, 8193, 8207, 8208)      # 8191 - 1024 .. 8192 + 16
OFFS = STAR_OFF + (63, 64, 65, 1023, 1024, 1025) + RING_OFFS + (32767, 32768, 65534, 65535)
CATCHUPS = (1, 2, 3, 4, 5, 20)
SMALL_CHUNKS = (1, 4, 12, 13, 14, 17, 31)
DENSE_TAILS = (111, 112, 113)

FEATURES = {}


def _feature(name, star=False):
    def deco(fn):
        FEATURES[name] = fn
        if star:
            STAR.add(name)
        return fn
    return deco


STAR = set()
for _v in LITS:
    _feature("lit=%d" % _v, _v in STAR_LIT)(lambda c, v=_v: any(s[1] == v for s in c.matches))
for _v in MLS:
    _feature("ml=%d" % _v, _v in STAR_ML)(lambda c, v=_v: any(s[3] == v for s in c.matches))
for _v in OFFS:
    _feature("off=%d" % _v, _v in STAR_OFF)(lambda c, v=_v: any(s[2] == v for s in c.matches))
for _v in (-1, 0, 1):
    _feature("off=wlo%+d" % _v)(lambda c, v=_v: any(s[0] + s[1] - s[2] == w + v for s in c.matches for w in ring_lows(s[0] + s[1])))
    _feature("wrap:start=8192k%+d" % _v)(lambda c, v=_v: any((s[0] + s[1] - v) % WIN == 0 and s[0] + s[1] > 16 and s[3] >= 32 for s in c.matches))
    _feature("wrap:end=8192k%+d" % _v)(lambda c, v=_v: any((s[0] + s[1] + s[3] - v) % WIN == 0 and 32 <= s[3] < WIN for s in c.matches))
for _v in (65536, 65540):
    # a planted copy one and five bytes outside the window: NO sequence has its destination there, and no offset is out of range
    _feature("no-match@%d" % _v)(lambda c, v=_v: c.data[c.marks[v]:c.marks[v] + 8] == c.data[c.marks[v] - v:c.marks[v] - v + 8]
                                 and not any(c.marks[v] - 3 <= s[0] + s[1] <= c.marks[v] + 7 for s in c.matches) and all(s[2] <= MAXD for s in c.matches))
for _v in CATCHUPS:
    _feature("catchup=%d" % _v)(lambda c, v=_v: any(f[0] - (s[0] + s[1]) == v for s, f in zip(c.matches, c.found)))
for _v in SMALL_CHUNKS:
    _feature("n=%d" % _v)(lambda c, v=_v: c.n == v)
for _v in (-2, -1, 0):
    _feature("csize=n%+d" % _v)(lambda c, v=_v: c.csize == c.n + v)
for _v in DENSE_TAILS:
    _feature("dense:tail=%d" % _v)(lambda c, v=_v: max(r for r, _ in c.short_runs()) >= 128 and c.matches[-1][3] < 16
                                   and any(s[0] + s[1] == c.n - 5 - v and s[3] < 16 for s in c.matches)
                                   and all(s[3] < 16 for s in c.matches if s[0] + s[1] >= c.n - 5 - v))


@_feature("lit>=960probes")
def _(c):            # the match is found by a probe of the strided (ring-less) search, its source one that the strided search visited
    return any(f[1] > 960 and s[1] >= 7680 and s[0] + s[1] - s[2] - s[0] > 65 for s, f in zip(c.matches, c.found))


@_feature("ml>whi")
def _(c):            # a match that runs over the resident end: whi <= ip + AHEAD + FB, the block in flight ends FB later
    return any(AHEAD + 2 * FB < s[3] < WIN for s in c.matches)


@_feature("catchup>=300")
def _(c):
    return any(f[0] - (s[0] + s[1]) >= 300 for s, f in zip(c.matches, c.found))


@_feature("catchup:anchor")
def _(c):            # the bytes in front of the anchor are equal too: only the anchor stops the catch-up
    return any(s[1] == 0 and not f[2] and f[0] > s[0] and s[0] - s[2] >= 1 and c.data[s[0] - 1] == c.data[s[0] - s[2] - 1] for s, f in zip(c.matches, c.found))


@_feature("catchup:first-byte")
def _(c):
    return any(s[0] + s[1] == s[2] and f[0] > s[0] + s[1] for s, f in zip(c.matches, c.found))


@_feature("bucket:hazard")
def _(c):            # source and destination are probes of one batch of 64: the source is this literal run's, 5..63 bytes back
    return any(5 <= s[2] <= 63 and s[2] <= s[1] <= 63 for s in c.matches)


@_feature("bucket:collision")
def _(c):            # a at marks, b collides with it and takes the bucket; the copy of a's five bytes at d is not found
    a, b, d = c.marks["collision"]
    return ((b, a) in c.refused and c.data[a:a + 5] == c.data[d:d + 5] and hash5(c.data[a:a + 5]) == hash5(c.data[b:b + 5])
            and not any(d - 4 <= s[0] + s[1] <= d + 4 for s in c.matches) and not any(d - 4 <= f[0] <= d + 4 for f in c.found))


@_feature("bucket:4th-byte")
def _(c):
    a, b = c.marks["4th"]
    return (b, a) in c.refused and c.data[a:a + 3] == c.data[b:b + 3] and c.data[a + 3] != c.data[b + 3] and hash5(c.data[a:a + 5]) == hash5(c.data[b:b + 5])


@_feature("end:n-5", True)
def _(c):            # the last match ends at n - 5 of its own accord
    p, l, o, m = c.matches[-1]
    return p + l + m == c.n - 5 and c.data[c.n - 5] != c.data[c.n - 5 - o]


@_feature("end:cut", True)
def _(c):            # a repeat that runs to n - 1 is cut at n - 5
    p, l, o, m = c.matches[-1]
    return p + l + m == c.n - 5 and c.data[c.n - 5:] == c.data[c.n - 5 - o:c.n - o]


@_feature("end:last-searched", True)
def _(c):            # liblz4 searches n - 12 (mflimitPlusOne = n - 11 is the first position it does not): a match found there
    return any(f[0] == c.n - 12 for f in c.found)


@_feature("end:n-13", True)
def _(c):
    return any(f[0] == c.n - 13 and s[0] + s[1] == c.n - 13 for s, f in zip(c.matches, c.found))


@_feature("end:not-searched", True)
def _(c):            # a copy planted one byte behind the last searched position is not found
    d = c.n - 11
    s = c.marks["unsearched"]
    return c.data[d:d + 6] == c.data[s:s + 6] and c.data[d - 1] != c.data[s - 1] and all(x[0] + x[1] + x[3] <= d - 1 for x in c.matches)


@_feature("dense:whole")
def _(c):
    runs = c.short_runs()
    return runs[0][0] > c.n // 80 and c.matches[0][3] < 16 and sum(g for _, g in runs) <= 2


@_feature("dense:100-then-ordinary")
def _(c):
    runs = c.short_runs()
    return 90 <= runs[0][0] < 128 and max(r for r, _ in runs[1:] + [(0, 0)]) < 16 and c.matches[0][3] < 16


@_feature("dense:leaky")
def _(c):            # blocks of about 120 short matches, each followed by about 40 ordinary ones
    return sum(1 for r, g in c.short_runs() if 100 <= r < 128 and 30 <= g <= 50) >= 8


@_feature("dense:batch-ends")
def _(c):
    return (max(r for r, _ in c.short_runs()) >= 128 and FEATURES["ml=1025"](c) and FEATURES["lit=2049"](c) and FEATURES["catchup>=300"](c)
            and FEATURES["bucket:hazard"](c))


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
SHORT_R = (0, 1, 5, 11, 12, 13, 15)
CLASSES = ["262144", "65536"] + ["%d+%d" % (b, r) for b in (4096, 40000) for r in SHORT_R]
CFG64 = "blocksize_kb=64,framestep_kb=64"


def _class_len(cls):
    return sum(int(x) for x in cls.split("+"))


def _star_body(p):
    """every starred literal run, match length and offset, in some 700 bytes"""
    p.lits(40)
    p.seq_from(9, 0, 4)            # four bytes: only an empty bucket (which reads as position 0) finds a match whose fifth byte differs
    p.seq(16, 16, 15)
    p.seq(15, 15, 16)
    p.seq(14, 7, 17)
    p.seq_from(1, p.recent(1, 2), 18)
    for s in range(p.recent(2), p.recent(2) + 12):                 # no literal: the source's first byte must end the match in front
        if p.b[s] != p.forbid:
            break
    p.seq_from(0, s, 19)
    p.seq(63, 17, 20)
    p.seq(64, 8, 5)
    p.seq(65, 4, 6)
    p.seq(20, 3, 9)
    p.seq(20, 2, 10)
    p.seq(20, 1, 11)
    p.lits(3)


def _tail(p, n, kind):
    feats = []
    if kind == "n-13":                        # found at n - 13, eight bytes, the byte at n - 5 differs
        p.fill_to(n - 13 - 26)
        p.lits(20)
        p.seq_from(6, p.recent(1, 3), 8)
        p.lits(5)
        feats = ["end:n-13", "end:n-5"]
    elif kind == "n-12":
        p.fill_to(n - 12 - 26)
        p.lits(20)
        p.seq_from(6, p.recent(1, 3), 7)
        p.lits(5)
        feats = ["end:last-searched", "end:n-5"]
    elif kind == "cut":
        p.fill_to(n - 60)
        p.seq(9, 9, n - len(p) - 9)
        feats = ["end:cut"]
    elif kind == "n-11":
        p.fill_to(n - 11 - 40)
        p.lits(34)
        s = len(p) - 30
        p.marks["unsearched"] = s
        p.seq_from(6, s, 6)
        p.lits(5)
        feats = ["end:not-searched"]
    assert len(p) == n, (len(p), n)
    return feats


def _star_case(cls, kind, seed):
    n = _class_len(cls)
    p = Plant(seed)
    _star_body(p)
    feats = ["lit=%d" % v for v in STAR_LIT] + ["ml=%d" % v for v in STAR_ML] + ["off=%d" % v for v in STAR_OFF]
    feats += _tail(p, n, kind)
    return {"name": "star-%s-%s" % (cls, kind), "data": p.bytes(), "features": feats, "cls": cls, "marks": p.marks}


def _finish(name, p, feats, n=262144, tail="n-13"):
    feats = list(feats) + _tail(p, n, tail)
    return {"name": name, "data": p.bytes(), "features": feats, "cls": str(n) if n in (262144, 65536) else None, "marks": p.marks}


def _literal_runs(seed):
    p = Plant(seed)
    p.lits(30)
    p.seq(8, 8, 40)
    for L in (269, 270, 271, 524, 525, 2047, 2048, 2049, 5000):
        a = len(p)
        # the source lies at the head of this very run (searched at step 1); the destination is not always probed itself: the next probe
        # inside the copy finds it and catch-up walks back to the planned start
        p.seq(L, L - 2, 40)
        p.fill_to(a + L + 40 + 300)
    return _finish("literal-runs", p, ["lit=%d" % L for L in (269, 270, 271, 524, 525, 2047, 2048, 2049, 5000)])


def _ringless(seed):
    p = Plant(seed)
    p.lits(30)
    p.seq(8, 8, 40)
    a = len(p)
    vis = probe_positions(a, 1100)
    s, d = vis[300], vis[1000]                # the source a position the strided search visited (step 5), the destination its 1001st probe
    assert d - a >= 7680
    p.seq(d - a, d - s, 24)
    return _finish("ringless", p, ["lit>=960probes"])


def _match_lengths(seed, which, name, n=262144):
    p = Plant(seed)
    p.lits(40)
    p.seq(12, 12, 8)
    for ml in which:
        p.seq_from(12, p.recent(1, 2), ml)
    return _finish(name, p, ["ml=%d" % v for v in which], n)


def _wrap(seed):
    p = Plant(seed)
    p.lits(40)
    p.seq(12, 12, 8)
    k = 1
    for v in (-1, 0, 1):
        p.fill_to(WIN * k + v - 100 - 12)      # a match that ends at the wrap
        p.seq(12, 12, 100)
        k += 1
        p.fill_to(WIN * k + v - 12)            # one that starts there
        p.seq(12, 12, 100)
        k += 1
        p.fill_to(WIN * k + v - 50 - 12)       # one that straddles it and is long enough to run over the resident end
        p.seq(12, 12, 3500)
        k += 1
    feats = ["wrap:start=8192k%+d" % v for v in (-1, 0, 1)] + ["wrap:end=8192k%+d" % v for v in (-1, 0, 1)] + ["ml>whi"]
    return _finish("ring-wrap", p, feats)


def _offsets(seed, which, name, n=262144, extra=()):
    p = Plant(seed)
    p.lits(20)
    feats = []
    for off in which:
        if off > MAXD:
            p.far(off, mark=off)
            p.lits(20)
            feats.append("no-match@%d" % off)
        else:
            p.far(off)
            feats.append("off=%d" % off)
    return _finish(name, p, feats + list(extra), n)


def _ring_edge(seed):
    """sources just outside and just inside the lean ring: for a destination at ip the ring starts at ring_lows(ip)"""
    p = Plant(seed)
    p.lits(20)
    p.fill_to(20000)
    for which in (0, 1):
        for v in (-1, 0, 1):
            # the source comes to lie at r0 + 10 = wlo + v, so wlo is chosen first (a multiple of FB), then a destination that has this wlo:
            # whi = wlo + WIN - FB (or wlo + WIN), and ip lies in (whi - AHEAD - FB, whi - AHEAD]
            wlo = (len(p) + 40 + FB) // FB * FB
            p.fill_to(wlo + v - 10)
            whi = wlo + (WIN - FB if which == 0 else WIN)
            d = whi - AHEAD - 500
            p.far(d - (wlo + v))
            assert len(p) - 8 == d and ring_lows(d)[which] == wlo, (d, wlo)
    return _finish("ring-edge", p, ["off=wlo%+d" % v for v in (-1, 0, 1)])


def _catchup(seed, dense=False):
    p = Plant(seed)
    first = bytes(p._byte() for _ in range(5))
    p.raw(first)                                                    # position 0: its bucket is taken over by a colliding string below
    p.lits(12)
    p.raw(p.collide(0, like=first)[1])
    ks = [300] if dense else list(CATCHUPS) + [300, "anchor"]
    src = {}
    for k in ks:                                                    # p0 zone: the strings themselves, more than 65535 bytes in front of their use
        p.seq(8, 8, 24)
        p.lits(2)
        src[k] = len(p)
        p.lits((12 if k == "anchor" else k + 6) + 4)
    p.seq(8, 8, 24)
    p.seq_from(4, 0, 20)                                            # the chunk's first bytes: found at position 1, one byte of catch-up to position 0
    p.lits(3)
    assert len(p) < 900
    p.fill_to(3000)
    mid, head = {}, {}
    for k in ks:                                                    # p1 zone: each string again as ONE match (liblz4 enters its start and end - 2 only)
        m = 12 if k == "anchor" else k + 6
        p.seq_from(6, src[k], m)
        mid[k] = len(p) - m
        p.lits(14)
        if k == "anchor":                                           # and its first 8 bytes on their own, behind it: the bucket of its start is theirs
            p.seq(8, 8, 24)
            p.seq_from(6, src[k], 8)
            head[k] = len(p) - 8
            p.lits(14)
        p.seq(8, 8, 24)
    p.fill_to(66500)
    if dense:
        return p, src, mid
    feats = ["catchup=%d" % k for k in CATCHUPS] + ["catchup>=300", "catchup:anchor", "catchup:first-byte"]
    for k in ks:                                                    # the uses: a copy that starts k bytes in front of end - 2 of the match
        if k == "anchor":
            p.seq_from(3, head[k], 8)                               # the first 8 bytes, found at their start ...
            p.copy(len(p) - (mid[k] + 8), 4 + 10)                   # ... then the rest: found at end - 2, two bytes on; catch-up stops at the anchor
        else:
            e = mid[k] + k + 6
            p.seq_from(3, e - 2 - k, k + 2 + 10)
        p.lits(3)
        p.seq(8, 8, 24)
    return _finish("catch-up", p, feats)


def _buckets(seed):
    p = Plant(seed)
    p.lits(20)
    for period in (5, 31, 63):
        p.seq(period, period, 12)
        p.lits(3)
        p.seq(8, 8, 24)
    p.lits(8)
    a, b = p.collide(0)
    pa = len(p); p.raw(a); p.lits(8)
    pb = len(p); p.raw(b); p.lits(8, last_not=p.b[pa - 1])
    pd = len(p); p.raw(a)
    p.forbid = p.b[pa + 5]
    p.marks["collision"] = (pa, pb, pd)
    p.lits(8)
    a, b = p.collide(3)
    pa = len(p); p.raw(a); p.lits(8)
    pb = len(p); p.raw(b); p.lits(8)
    p.marks["4th"] = (pa, pb)
    return _finish("buckets", p, ["bucket:hazard", "bucket:collision", "bucket:4th-byte"])


def _dense_run(p, count=None, until=None):
    """short matches (5..15 bytes) with 2..6 literals between them, their sources in the literal runs of the last few sequences"""
    k = 0
    while (count is None or k < count) and (until is None or len(p) < until - 40):
        lit = int(p.rng.integers(2, 7))
        ml = int(p.rng.integers(5, 16))
        src = p.recent(int(p.rng.integers(1, min(12, len(p.runs)) + 1)), int(p.rng.integers(0, 2)))
        if src + ml >= len(p) + lit:
            ml = 5
        p.seq_from(lit, src, ml)
        k += 1


def _dense_head(seed):
    p = Plant(seed)
    p.lits(12)
    for _ in range(6):
        p.seq(4, 4, 7)
    return p


def _dense(seed, kind, n=262144):
    p = _dense_head(seed)
    name = "dense-%s-%d" % (kind, n)
    if kind == "whole":
        _dense_run(p, until=n - 30)
        return _finish(name, p, ["dense:whole"], n)
    if kind == "100":
        _dense_run(p, count=94)
        p.lits(20)
        for _ in range(40):
            p.seq_from(12, p.recent(1, 2), 60)
        return _finish(name, p, ["dense:100-then-ordinary"], n)
    if kind == "leaky":
        for _ in range(12):
            _dense_run(p, count=112)
            for _ in range(40):
                p.seq_from(9, p.recent(1, 2), 40)
        return _finish(name, p, ["dense:leaky"], n)
    if kind in DENSE_TAILS:
        _dense_run(p, until=n - 5 - kind - 20)
        lit = n - 5 - kind - len(p)
        p.seq_from(lit, p.recent(2, 0), 7)
        while len(p) < n - 5 - 24:
            _dense_run(p, count=1)
        left = n - 5 - len(p)                                        # the last short match ends at n - 5
        p.seq_from(left - 7, p.recent(1, 0), 7)
        p.lits(5)
        assert len(p) == n
        return {"name": name, "data": p.bytes(), "features": ["dense:tail=%d" % kind], "cls": None, "marks": p.marks}
    raise ValueError(kind)


def _dense_batch_ends(seed):
    """a dense stream with the ends of a dense batch in it: a long match, a long literal run, a long catch-up, two probes in one bucket"""
    p, src, mid = _catchup(seed, dense=True)
    p.lits(6)
    for _ in range(6):
        p.seq(4, 4, 7)
    _dense_run(p, count=30)                                         # (the match it reaches back to must stay inside the window)
    e = mid[300] + 300 + 6
    p.seq_from(3, e - 2 - 300, 300 + 2 + 10)
    _dense_run(p, count=300)
    p.seq(8, 8, 24)
    p.lits(20)
    p.seq_from(4, p.recent(1, 2), 1025)
    _dense_run(p, count=300)
    p.seq(8, 8, 24)
    p.seq(2049, 2049 - 2, 9)
    _dense_run(p, count=300)
    p.seq(8, 8, 24)
    p.seq(31, 31, 9)
    _dense_run(p, until=262144 - 60)
    return _finish("dense-batch-ends", p, ["dense:batch-ends"])


def _small(n):
    data = bytes([7, 7, 7, 9] * 8)[:n]
    return {"name": "small-%d" % n, "data": data, "features": ["n=%d" % n], "cls": None, "marks": {}}


def _capacity(delta, zeros):
    """noise with a run of zeros at its end, as long as it takes for a block of n + delta bytes: the chunk is stored at n - 1 < csize"""
    n = 4096
    rng = np.random.default_rng(4242)
    d = rng.integers(0, 256, n, dtype=np.uint8)
    d[n - zeros:] = 0
    return {"name": "capacity-n%+d" % delta, "data": d.tobytes(), "features": ["csize=n%+d" % delta], "cls": None, "marks": {}}


CAPACITY_ZEROS = {-2: 39, -1: 38, 0: 37}

_cases = None


def cases():
    """the list of named streams: {"name", "data", "features", "cls" (chunk length class or None), "config" (lz4's parameters), "marks"}"""
    global _cases
    if _cases is not None:
        return _cases
    out = []
    seed = 1000
    for cls in CLASSES:
        for kind in ("n-13", "n-12", "cut", "n-11"):
            seed += 1
            out.append(_star_case(cls, kind, SEEDS.get((cls, kind), seed)))
    out.append(_literal_runs(SEEDS.get("literal-runs", 2001)))
    out.append(_ringless(SEEDS.get("ringless", 2002)))
    out.append(_match_lengths(SEEDS.get("ml-a", 2003), (273, 274, 275, 1023, 1024, 1025, 1027, 1028, 1029, 8200), "match-lengths"))
    out.append(_match_lengths(SEEDS.get("ml-b", 2004), (33000,), "match-33000"))
    out.append(_match_lengths(SEEDS.get("ml-c", 2005), (1024, 8200, 33000), "match-lengths-65536", 65536))
    out.append(_wrap(SEEDS.get("wrap", 2006)))
    out.append(_offsets(SEEDS.get("off-a", 2007), (63, 64, 65, 1023, 1024, 1025) + RING_OFFS + (32767, 32768), "offsets-near"))
    out.append(_offsets(SEEDS.get("off-b", 2008), (65534, 65535), "offsets-window"))
    out.append(_offsets(SEEDS.get("off-c", 2009), (65536, 65540), "offsets-outside"))
    out.append(_ring_edge(SEEDS.get("ring-edge", 2010)))
    out.append(_catchup(SEEDS.get("catch-up", 2011)))
    out.append(_buckets(SEEDS.get("buckets", 2012)))
    out.append(_dense(SEEDS.get("dense-whole", 2013), "whole"))
    out.append(_dense(SEEDS.get("dense-whole-64", 2014), "whole", 65536))
    out.append(_dense(SEEDS.get("dense-whole-40013", 2015), "whole", 40013))
    out.append(_dense(SEEDS.get("dense-100", 2016), "100"))
    out.append(_dense(SEEDS.get("dense-leaky", 2017), "leaky"))
    for t in DENSE_TAILS:
        out.append(_dense(SEEDS.get("dense-tail-%d" % t, 2020 + t), t, 40000 + t % 16))
    out.append(_dense_batch_ends(SEEDS.get("dense-batch-ends", 2018)))
    for n in SMALL_CHUNKS:
        out.append(_small(n))
    for delta in (-2, -1, 0):
        out.append(_capacity(delta, CAPACITY_ZEROS[delta]))
    for c in out:
        c["config"] = CFG64 if len(c["data"]) == 65536 else ""
        assert len(c["data"]) <= 262144
    assert len({c["name"] for c in out}) == len(out)
    _cases = out
    return out


# seeds at which every planned sequence is liblz4's (a source's bucket can be taken by one of the random literals behind it: one in 4096
# per literal); tests/test_lz4_planted_host.py asserts the features, so a seed that stops working fails there
SEEDS = {}


# ---- for the tests' messages --------------------------------------------------------------------------------------------------------------
def block_cap(n):
    """room in which every block fits, stored or not: the features are checked on the parse itself"""
    return n + n // 255 + 32


def frame_blocks(payload):
    """the data blocks of a run of LZ4 frames (a blob's payload): [(stored, bytes)]"""
    p, out = bytes(payload), []
    i = 0
    while i + 7 <= len(p) and p[i:i + 4] == b"\x04\x22\x4d\x18":
        flg = p[i + 4]
        i += 6 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0) + 1
        while True:
            size = int.from_bytes(p[i:i + 4], "little")
            i += 4
            if size == 0:
                break
            stored, size = bool(size >> 31), size & 0x7FFFFFFF
            out.append((stored, p[i:i + size]))
            i += size + (4 if flg & 16 else 0)
        i += 4 if flg & 4 else 0
    return out


def explain(got, want, header_size):
    """what differs between two blobs of LZ4 frames, for an assertion message: the first differing block, its first differing sequence"""
    if got is None:
        return "no blob"
    if bytes(got) == bytes(want):
        return "equal"
    try:
        a, b = frame_blocks(bytes(got)[header_size:]), frame_blocks(bytes(want)[header_size:])
    except IndexError:
        return "blobs of %d / %d bytes; the frames do not parse" % (len(got), len(want))
    for i in range(max(len(a), len(b))):
        if i >= len(a) or i >= len(b):
            return "blobs of %d / %d bytes: %d / %d blocks" % (len(got), len(want), len(a), len(b))
        if a[i] != b[i]:
            if a[i][0] or b[i][0]:
                return "block %d: stored %s / %s, %d / %d bytes" % (i, a[i][0], b[i][0], len(a[i][1]), len(b[i][1]))
            return "block %d: %s" % (i, first_difference(a[i][1], b[i][1]))
    return "blobs of %d / %d bytes differ outside the blocks" % (len(got), len(want))
