"""Loader for oracle/_ref/libsqy_ref.so -- the driver around the REAL reference pieces that build in
this image (the reference's filter-stage templates, its SSE bit-plane gather, its quantiser and its frame_shuffle /
tile_shuffle + the image's liblz4 1.9.3).  TEST INFRASTRUCTURE ONLY.

The library is built by oracle/Makefile from /root/reference when that tree is present; on the GPU box
only the prebuilt file (shipped with the snapshot) can be used.  `available()` says whether it loads.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
_TRIED = False

_u8p = ctypes.POINTER(ctypes.c_uint8)
_u16p = ctypes.POINTER(ctypes.c_uint16)


def lib():
    global _LIB, _TRIED
    if not _TRIED:
        _TRIED = True
        path = os.path.join(_HERE, "_ref", "libsqy_ref.so")
        _rebuild_if_stale(path)
        try:
            L = ctypes.CDLL(path)
            for f in ("ref_lz4f_compress_bound", "ref_lz4_encode_serial", "ref_lz4_encode_parallel", "ref_lz4_decode_frames"):
                getattr(L, f).restype = ctypes.c_size_t
            _LIB = L
        except OSError:
            _LIB = None
    return _LIB


def _rebuild_if_stale(path):
    """a library from an older driver (no stage entry points in its symbol table) is rebuilt before it is loaded, where the reference
    tree is there to build it from; where it is not, the old one is kept and serves what it can (sqy_oracle.lib() rebuilds alike)"""
    try:
        with open(path, "rb") as f:
            data = f.read()
    except OSError:
        return
    if all(name.encode() in data for name in STAGE_ENTRY_POINTS + QUANTISER_ENTRY_POINTS + SHUFFLE_ENTRY_POINTS):
        return
    try:
        if reference_tree():
            import subprocess
            subprocess.call(["make", "-s", "-C", _HERE, "ref"], stdout=subprocess.DEVNULL)
    except Exception:                                   # no make, no compiler: keep what is there
        pass


def available():
    return lib() is not None


STAGE_ENTRY_POINTS = ("ref_diff3x3x1", "ref_diff3x3x1_offsets", "ref_rmestbkrd", "ref_cache_l2_bytes", "ref_rmbkrd_neighbor5x5x5",
                      "ref_zcurve_reorder", "ref_raster_reorder", "ref_bitswap1", "ref_hist_stats")


def stages_available():
    """True when the library loads AND holds the filter-stage entry points: a prebuilt oracle/_ref from an older driver, kept where the
    reference tree is absent and nothing can be rebuilt, has only the LZ4 and SSE ones"""
    L = lib()
    return L is not None and all(hasattr(L, f) for f in STAGE_ENTRY_POINTS)


QUANTISER_ENTRY_POINTS = ("ref_quantiser_luts", "ref_quantiser_encode")


def quantiser_available():
    """True when the library also holds the reference's quantiser: a prebuilt oracle/_ref from a driver before those entry points has the
    other stages only"""
    L = lib()
    return L is not None and all(hasattr(L, f) for f in QUANTISER_ENTRY_POINTS)


SHUFFLE_ENTRY_POINTS = ("ref_frame_shuffle_encode", "ref_frame_shuffle_decode", "ref_tile_shuffle_encode", "ref_tile_shuffle_decode")


def shuffles_available():
    """True when the library also holds the reference's frame_shuffle and tile_shuffle (a prebuilt oracle/_ref from a driver before those
    entry points does not)"""
    L = lib()
    return L is not None and all(hasattr(L, f) for f in SHUFFLE_ENTRY_POINTS)


def _make(target):
    import subprocess
    return subprocess.check_output(["make", "-s", "--no-print-directory", "-C", _HERE, target], text=True).strip()


def reference_tree():
    """the reference's source directory oracle/Makefile builds from, or None where it does not exist (then oracle/_ref cannot be rebuilt)"""
    path = _make("ref-tree")
    return path if os.path.isdir(path) else None


def lz4_version():
    return lib().ref_lz4_version()


_DT = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1}
_szp = ctypes.POINTER(ctypes.c_size_t)


class Refused(ValueError):
    """the reference threw, or its own checks returned without doing the work"""


def _aligned(n, dtype, offset_bytes=0):
    """n elements of dtype that start `offset_bytes` behind a 64-byte boundary"""
    dtype = np.dtype(dtype)
    buf = np.zeros(n * dtype.itemsize + 128, dtype=np.uint8)
    at = (-buf.ctypes.data % 64) + offset_bytes
    return buf[at:at + n * dtype.itemsize].view(dtype)


def _io(a, char=False, offset_bytes=0):
    a = np.ascontiguousarray(a)
    src = _aligned(a.size, a.dtype, offset_bytes)
    src[:] = a.reshape(-1)
    dst = _aligned(a.size, a.dtype)
    return a, src, dst, (2 if char else _DT[a.dtype])


def _shape3(shape):
    return (ctypes.c_size_t * 3)(*[int(d) for d in shape])


def _done(rc, what):
    if rc:
        raise Refused("%s: the reference %s" % (what, "threw" if rc == 2 else "did not do the work (%d)" % rc))


def diff3x3x1(a, char=False, decode=False, nthreads=1):
    a, src, dst, dt = _io(a, char)
    _done(lib().ref_diff3x3x1(dt, ctypes.c_void_p(src.ctypes.data), ctypes.c_void_p(dst.ctypes.data), _shape3(a.shape),
                              int(decode), int(nthreads)), "diff3x3x1")
    return dst.reshape(a.shape).copy()


def diff3x3x1_offsets(shape):
    L = lib()
    L.ref_diff3x3x1_offsets.restype = ctypes.c_long
    hx = ctypes.c_size_t(0)
    n = L.ref_diff3x3x1_offsets(_shape3(shape), None, ctypes.c_size_t(0), ctypes.byref(hx))
    if n < 0:
        raise Refused("diff3x3x1 offsets: the reference threw")
    out = np.zeros(max(n, 1), dtype=np.uint64)
    L.ref_diff3x3x1_offsets(_shape3(shape), out.ctypes.data_as(_szp), ctypes.c_size_t(n), ctypes.byref(hx))
    return out[:n], hx.value


def cache_l2_bytes():
    L = lib()
    L.ref_cache_l2_bytes.restype = ctypes.c_uint
    return L.ref_cache_l2_bytes()


def rmestbkrd(a, nthreads=1):
    """(encoded volume, the four face supports as float32, threshold)"""
    a, src, dst, dt = _io(a)
    sup = np.zeros(4, np.float32)
    thr = ctypes.c_double(0)
    _done(lib().ref_rmestbkrd(dt, ctypes.c_void_p(src.ctypes.data), ctypes.c_void_p(dst.ctypes.data), _shape3(a.shape), int(nthreads),
                              sup.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(thr)), "rmestbkrd")
    return dst.reshape(a.shape).copy(), sup, int(thr.value)


def rmbkrd_neighbor5x5x5(a, threshold, fraction, nthreads=1):
    """voxels the reference does not write are 0 here (the output buffer starts zeroed)"""
    a, src, dst, dt = _io(a)
    _done(lib().ref_rmbkrd_neighbor5x5x5(dt, ctypes.c_void_p(src.ctypes.data), ctypes.c_void_p(dst.ctypes.data), _shape3(a.shape),
                                         ctypes.c_long(int(threshold)), ctypes.c_float(float(fraction)), int(nthreads)), "rmbkrd_neighbor5x5x5")
    return dst.reshape(a.shape).copy()


def _reorder(fn, a, tile, decode, nthreads):
    a, src, dst, dt = _io(a)
    _done(fn(dt, ctypes.c_void_p(src.ctypes.data), ctypes.c_void_p(dst.ctypes.data), _shape3(a.shape), ctypes.c_size_t(int(tile)),
             int(decode), int(nthreads)), "reorder")
    return dst.reshape(a.shape).copy()


def zcurve_reorder(a, tile, decode=False, nthreads=1):
    return _reorder(lib().ref_zcurve_reorder, a, tile, decode, nthreads)


def raster_reorder(a, tile, decode=False, nthreads=1):
    return _reorder(lib().ref_raster_reorder, a, tile, decode, nthreads)


def bitswap1(a, decode=False, nthreads=1, offset_bytes=0):
    """bitswap_scheme<T,1> on a flat array of any length whose first element sits `offset_bytes` behind a 64-byte boundary"""
    a, src, dst, dt = _io(np.ascontiguousarray(a).reshape(-1), offset_bytes=offset_bytes)
    if dt == 1 and not decode and a.size % 128 == 0 and offset_bytes % 16:
        raise Refused("the reference's SSE branch loads with _mm_load_si128: it faults on this address")
    _done(lib().ref_bitswap1(dt, ctypes.c_void_p(src.ctypes.data), ctypes.c_void_p(dst.ctypes.data), ctypes.c_size_t(a.size),
                             int(decode), int(nthreads)), "bitswap1")
    return dst.copy()


HIST_STATS = ("smallest_populated_bin", "largest_populated_bin", "integral", "mean", "mean_variation", "median", "median_variation",
              "mode", "entropy", "support")


def hist_stats(a):
    """(bins as uint32, {name: value}) of sqeazy::histogram<T>(begin, end) and calc_support(0.99f)"""
    a = np.ascontiguousarray(a).reshape(-1)
    bins = np.zeros(1 << (8 * a.dtype.itemsize), np.uint32)
    st = np.zeros(len(HIST_STATS), np.float64)
    _done(lib().ref_hist_stats(_DT[a.dtype], ctypes.c_void_p(a.ctypes.data), ctypes.c_size_t(a.size),
                               bins.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), st.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "histogram")
    return bins, dict(zip(HIST_STATS, st.tolist()))


def _weighting(weighting):
    from oracle import sqy_oracle
    return sqy_oracle.quantiser_weighting(weighting)        # the text -> (mode, numerator, denominator), as the scheme reads it


def quantiser_luts(a, weighting="none", nthreads=1):
    """(lut_encode uint8[65536], lut_decode uint16[256]) of sqeazy::quantiser<uint16_t, uint8_t> after setup_com on the voxels"""
    flat = np.ascontiguousarray(a, dtype=np.uint16).reshape(-1)
    enc = np.zeros(65536, np.uint8)
    dec = np.zeros(256, np.uint16)
    mode, num, den = _weighting(weighting)
    _done(lib().ref_quantiser_luts(flat.ctypes.data_as(_u16p), ctypes.c_size_t(flat.size), mode, num, den, int(nthreads),
                                   enc.ctypes.data_as(_u8p), dec.ctypes.data_as(_u16p)), "quantiser")
    return enc, dec


def quantiser_encode(a, weighting="none", nthreads=1):
    """(codes uint8 of a.shape, lut_decode uint16[256]): quantiser_scheme::encode on the voxels"""
    a = np.ascontiguousarray(a, dtype=np.uint16)
    flat = a.reshape(-1)
    codes = np.zeros(flat.size, np.uint8)
    dec = np.zeros(256, np.uint16)
    mode, num, den = _weighting(weighting)
    _done(lib().ref_quantiser_encode(flat.ctypes.data_as(_u16p), ctypes.c_size_t(flat.size), mode, num, den, int(nthreads),
                                     codes.ctypes.data_as(_u8p), dec.ctypes.data_as(_u16p)), "quantiser")
    return codes.reshape(a.shape), dec


class Remainder(Refused):
    """frame_shuffle / tile_shuffle: the shape is no whole number of units.  The reference would take its median path
    (encode_with_remainder), which this build does not have; the driver answers before the reference is called"""


def _shuffle_done(rc, what):
    if rc == 4:
        raise Remainder("%s: the shape has a remainder; the reference's median path is not run" % what)
    if rc == 5:
        raise Refused("%s: the map does not fit the shape" % what)
    _done(rc, what)


def _units(shape, chunk=None, tile=None):
    z, y, x = (int(d) for d in shape)
    return z // chunk if tile is None else (z // tile) * (y // tile) * (x // tile)


def _shuffle_encode(fn, what, a, param, units, char, nthreads):
    a, src, dst, dt = _io(a, char)
    dmap = np.zeros(max(units, 1), dtype=np.uint64)
    _shuffle_done(fn(dt, ctypes.c_void_p(src.ctypes.data), ctypes.c_void_p(dst.ctypes.data), _shape3(a.shape), ctypes.c_size_t(int(param)),
                     int(nthreads), dmap.ctypes.data_as(_szp), ctypes.c_size_t(units)), what)
    return dst.reshape(a.shape).copy(), dmap[:units]


def _shuffle_decode(fn, what, a, dmap, param, char, nthreads):
    a, src, dst, dt = _io(a, char)
    dst[:] = 0xA5 if a.dtype.itemsize == 1 else 0xA5A5     # the driver zero-fills: what is here must not show in the result
    dmap = np.ascontiguousarray(dmap, dtype=np.uint64)
    _shuffle_done(fn(dt, ctypes.c_void_p(src.ctypes.data), ctypes.c_void_p(dst.ctypes.data), _shape3(a.shape), ctypes.c_size_t(int(param)),
                     dmap.ctypes.data_as(_szp), ctypes.c_size_t(dmap.size), int(nthreads)), what)
    return dst.reshape(a.shape).copy()


def frame_shuffle_encode(a, chunk=1, char=False, nthreads=1):
    """(output of a.shape, decode_map as uint64) of sqeazy::detail::frame_shuffle(frame_chunk_size).encode; raises Remainder, without
    running the reference, where Z is no multiple of the chunk"""
    return _shuffle_encode(lib().ref_frame_shuffle_encode, "frame_shuffle", a, chunk, _units(np.shape(a), chunk=max(int(chunk), 1)), char, nthreads)


def frame_shuffle_decode(a, dmap, chunk=1, char=False, nthreads=1):
    """sqeazy::detail::frame_shuffle(frame_chunk_size, map).decode into a ZERO-FILLED output (the driver's choice: the reference leaves
    slots that no map entry names as the buffer had them)"""
    return _shuffle_decode(lib().ref_frame_shuffle_decode, "frame_shuffle", a, dmap, chunk, char, nthreads)


def tile_shuffle_encode(a, tile_size, char=False, nthreads=1):
    """(output of a.shape, decode_map as uint64) of sqeazy::detail::tile_shuffle(tile_size).encode; raises Remainder, without running
    the reference, where an axis is no multiple of the tile"""
    return _shuffle_encode(lib().ref_tile_shuffle_encode, "tile_shuffle", a, tile_size, _units(np.shape(a), tile=max(int(tile_size), 1)), char, nthreads)


def tile_shuffle_decode(a, dmap, tile_size, char=False, nthreads=1):
    """sqeazy::detail::tile_shuffle(tile_size, map).decode into a zero-filled output"""
    return _shuffle_decode(lib().ref_tile_shuffle_decode, "tile_shuffle", a, dmap, tile_size, char, nthreads)


def bitswap1_encode_u16(a, nthreads=1):
    """bitswap_scheme<uint16_t,1>::encode on 16-byte aligned input.  Goes through the entry point every build of the driver has had:
    one built before the stage entry points existed takes only lengths that are a multiple of 128 (the SSE branch)."""
    flat = np.ascontiguousarray(a, dtype=np.uint16).reshape(-1)
    src = _aligned(flat.size, np.uint16)
    src[:] = flat
    out = np.zeros(flat.size, dtype=np.uint16)
    rc = lib().ref_bitswap1_encode_u16(src.ctypes.data_as(_u16p), out.ctypes.data_as(_u16p),
                                       ctypes.c_size_t(flat.size), ctypes.c_int(nthreads))
    if rc:
        raise ValueError("this build of the reference driver does not take its scalar branch")
    return out


def _bytes(a):
    a = a if isinstance(a, np.ndarray) else np.frombuffer(bytes(a), dtype=np.uint8)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def lz4_encode_parallel(data, chunk=256 << 10, accel=1, block_id=5, nthreads=2):
    src = _bytes(data)
    nchunks = max(1, (src.size + chunk - 1) // chunk)
    stride = lib().ref_lz4f_compress_bound(ctypes.c_size_t(chunk), ctypes.c_int(accel), ctypes.c_int(block_id)) + 19
    cap = nchunks * stride + 64
    dst = np.zeros(cap, dtype=np.uint8)
    n = lib().ref_lz4_encode_parallel(src.ctypes.data_as(ctypes.c_char_p), ctypes.c_size_t(src.size),
                                      dst.ctypes.data_as(ctypes.c_char_p), ctypes.c_size_t(cap), ctypes.c_size_t(chunk),
                                      ctypes.c_int(accel), ctypes.c_int(block_id), ctypes.c_int(nthreads))
    if n == 0:
        raise RuntimeError("liblz4 frame compression failed")
    return dst[:n]


def lz4_encode_serial(data, framestep=256 << 10, accel=1, block_id=5):
    src = _bytes(data)
    cap = src.size + (src.size // (64 << 10) + 2) * 16 + 64
    dst = np.zeros(cap, dtype=np.uint8)
    n = lib().ref_lz4_encode_serial(src.ctypes.data_as(ctypes.c_char_p), ctypes.c_size_t(src.size),
                                    dst.ctypes.data_as(ctypes.c_char_p), ctypes.c_size_t(cap), ctypes.c_size_t(framestep),
                                    ctypes.c_int(accel), ctypes.c_int(block_id))
    if n == 0:
        raise RuntimeError("liblz4 frame compression failed")
    return dst[:n]


def lz4_block(data, cap=None, accel=1):
    src = _bytes(data)
    cap = src.size - 1 if cap is None else cap
    dst = np.zeros(max(cap, 1) + 16, dtype=np.uint8)
    r = lib().ref_lz4_block_fast_continue(src.ctypes.data_as(ctypes.c_char_p), ctypes.c_int(src.size),
                                          dst.ctypes.data_as(ctypes.c_char_p), ctypes.c_int(cap), ctypes.c_int(accel))
    return dst[:r].tobytes() if r > 0 else None


def lz4_decode_frames(data, cap):
    src = _bytes(data)
    dst = np.zeros(cap + 8, dtype=np.uint8)
    n = lib().ref_lz4_decode_frames(src.ctypes.data_as(ctypes.c_char_p), ctypes.c_size_t(src.size),
                                    dst.ctypes.data_as(ctypes.c_char_p), ctypes.c_size_t(cap))
    if n == ctypes.c_size_t(-1).value:
        raise ValueError("liblz4 rejected the stream")
    return dst[:n]


def lz4f_compress_bound(n, accel=1, block_id=5):
    return lib().ref_lz4f_compress_bound(ctypes.c_size_t(n), ctypes.c_int(accel), ctypes.c_int(block_id))
