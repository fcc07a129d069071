"""The reference's background-removal head filters restated in numpy, for the tests of rmestbkrd and rmbkrd_neighbor5x5x5.

Paths are relative to the reference's src/cpp/src.  Types follow the reference: histogram bins are uint32, the support walk is
float64 against (double)0.99f, the support itself float32; the neighbour count is compared as float32 with fraction * 124.f.
Deviations of the library from the reference are restated as the library defines them: voxels the reference never
writes are 0, neighbours at or past the volume's end are not counted."""
import numpy as np


# ---- rmbkrd_neighbor5x5x5 configuration (flatten_to_neighborhood_scheme_impl.hpp:44-80) ----------------------------------------------
def neighbor5_params(cfg, dtype):
    """(threshold, fraction) as the constructor leaves them: std::stoi narrowed to the voxel type, std::stof to float32"""
    m = dict(kv.split("=", 1) for kv in cfg.split(",")) if cfg else {}
    t = int(m.get("threshold", "1"))
    f = np.float32(float(m.get("fraction", "0.5")))
    bits = 8 * np.dtype(dtype).itemsize
    return t % (1 << bits), f


def neighbor5_config(threshold, fraction):
    # std::to_string(raw_type) and std::to_string(float) ("%f")
    return "threshold=%d,fraction=%s" % (threshold, "%f" % float(np.float32(fraction)))


def neighbor5_full_name(cfg, dtype):
    return "rmbkrd_neighbor5x5x5(%s)" % neighbor5_config(*neighbor5_params(cfg, dtype))


# ---- rmbkrd_neighbor5x5x5 geometry (neighborhood_utils.hpp:141-240; row_major::x == 2, traits.hpp:92-96) ---------------------------
def neighbor5_z_end(Z, X):
    # halo::compute_offsets_in_x: z runs to non_halo_end(2) = world[2] - 2 = X - 2; offsets >= Z*Y*X are dropped
    return max(2, min(X - 2, Z))


def neighbor5_defined(shape):
    """False where the reference takes its row length from an element its offset list does not have"""
    Z, Y, X = shape
    if X < 5 or Y < 5 or (X == 5 and Y == 5):          # (X-4)(Y-4) <= 1: the single-offset branch, halo_size_x = length - offsets[2]
        return False
    return (neighbor5_z_end(Z, X) - 2) * (Y - 4) != 1  # exactly one offset: offsets.size() != 1 fails the same way


def neighbor5_counts(vol, threshold):
    """for every voxel the number of its 125 FLAT neighbours dz*Y*X + dy*X + dx (d in [-2, 2], rows wrap) below the threshold
    (count_neighbors_if, background_scheme_utils.hpp:232-272); neighbours past the end are not counted.  Meaningful at
    the centres, where no neighbour lies in front of the volume and the centre itself is not below the threshold."""
    vol = np.ascontiguousarray(vol)
    Z, Y, X = vol.shape
    flat = vol.reshape(-1)
    N = flat.size
    YX = Y * X
    off = 2 * YX + 2 * X + 2
    e = np.zeros(N + 2 * off, np.int16)
    e[off:off + N] = flat < threshold

    def box5(a, step):
        out = np.zeros_like(a)
        L = a.size
        s = 2 * step
        out[s:L - s] = a[0:L - 2 * s] + a[step:L - 2 * s + step] + a[2 * step:L - 2 * s + 2 * step] + a[3 * step:L - 2 * s + 3 * step] + a[4 * step:L]
        return out

    return box5(box5(box5(e, 1), X), YX)[off:off + N].reshape(Z, Y, X)


def neighbor5_counts_direct(vol, threshold):
    """the same count by its definition, with no box sum: the 125 flat offsets dz*Y*X + dy*X + dx added one by one (each a shifted
    slice of the whole volume); a neighbour outside [0, N) is not counted.  Independent of neighbor5_counts, which separates the sum the
    way the kernel does."""
    vol = np.ascontiguousarray(vol)
    Z, Y, X = vol.shape
    b = (vol.reshape(-1) < threshold).astype(np.uint8)
    N = b.size
    n = np.zeros(N, np.uint8)                              # at most 125
    for dz in range(-2, 3):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                d = dz * Y * X + dy * X + dx
                lo, hi = max(0, -d), min(N, N - d)         # the voxels c with 0 <= c + d < N
                if lo < hi:
                    n[lo:hi] += b[lo + d:hi + d]
    return n.reshape(Z, Y, X).astype(np.int16)


def neighbor5_centres(shape):
    Z, Y, X = shape
    z, y, x = np.ogrid[:Z, :Y, :X]
    return (z >= 2) & (z < neighbor5_z_end(Z, X)) & (y >= 2) & (y < Y - 2) & (x >= 2) & (x < X - 1)


def neighbor5(vol, threshold, fraction):
    """flatten_to_neighborhood_scheme::encode (flatten_to_neighborhood_scheme_impl.hpp:90-150): a centre (z in [2, z_end), y in [2, Y-2),
    x in [2, X-1)) with in >= threshold keeps its value unless (float)n > fraction * 124.f; every other voxel is 0"""
    cut = np.float32(fraction) * np.float32(124)           # fraction * (size<Neighborhood>() - 1)
    n = neighbor5_counts(vol, threshold)
    keep = neighbor5_centres(vol.shape) & (vol >= threshold) & ~(n.astype(np.float32) > cut)
    return np.where(keep, vol, 0).astype(vol.dtype)


# ---- rmestbkrd (remove_estimated_background_scheme_impl.hpp:71-110) -----------------------------------------------------------------
def face_portion(frame_voxels, l2_bytes):
    # background_scheme_utils.hpp:44-45: voxels compared with bytes, (index_type)(L2 * .75)
    return int(l2_bytes * .75) if frame_voxels > l2_bytes else frame_voxels


def face_histograms(vol, l2_bytes):
    """extract_darkest_face_supports' four histograms (background_scheme_utils.hpp:35-105)"""
    Z, Y, X = vol.shape
    nb = 1 << (8 * vol.dtype.itemsize)
    flat = vol.reshape(-1)
    frame = Y * X
    p = face_portion(frame, l2_bytes)
    h = lambda a: np.bincount(a.astype(np.int64), minlength=nb).astype(np.uint32)
    zs = (1, Z // 2, Z - 2)
    return [h(flat[:p]), h(flat[(Z - 1) * frame:(Z - 1) * frame + p]),
            h(np.concatenate([vol[z, 0] for z in zs])), h(np.concatenate([vol[z, Y - 1] for z in zs]))]


def support(bins):
    """histogram::calc_support(0.99f) (hist_impl.hpp:359-380) on a histogram filled by add_from_image: support_index (:60-90) over all
    bins, total an int sum, running a double sum; result float(uint32 numerator) / float(denominator)"""
    nb = bins.size
    total = np.float64(np.int32(np.uint32(int(bins.sum(dtype=np.uint64)) & 0xffffffff)))
    running = np.cumsum(bins, dtype=np.uint64).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        hit = np.nonzero(running / total > np.float64(np.float32(0.99)))[0]
    m = (int(hit[0]) if hit.size else nb) % nb            # (T)mindex
    if m == 0:
        return np.float32(0)
    num = np.uint32((int(bins[m]) * m + int(bins[m - 1]) * (m - 1)) & 0xffffffff)
    den = np.uint32(int(bins[m - 1]) + int(bins[m]))
    return np.float32(num) / np.float32(den)


def rmestbkrd_threshold(vol, l2_bytes):
    return int(min(support(h) for h in face_histograms(vol, l2_bytes)))       # (raw_type)reduce_by


def rmestbkrd(vol, l2_bytes):
    """remove_background_scheme(reduce_by).encode (remove_background_scheme_impl.hpp:73-95)"""
    t = vol.dtype.type(rmestbkrd_threshold(vol, l2_bytes))
    out = vol - t                                          # (wraps below t; those voxels are zeroed next)
    out[vol <= t] = 0
    return out


# ---- whole blobs -------------------------------------------------------------------------------------------------------------------
def _is_bkrd(name):
    return name in ("rmestbkrd", "rmbkrd_neighbor5x5x5")


def expected_blob(oracle, pipeline, vol, l2_bytes=None):
    """The blob the library writes: runs of other stages through oracle.pipeline_encode, the background stages restated; the header is
    oracle.header_pack(dtype, shape, <full pipename>, len(body))."""
    cur = np.ascontiguousarray(vol)
    names, run = [], []
    body = None

    def flush(final):
        nonlocal cur, body
        if not run:
            return
        blob = oracle.pipeline_encode("->".join(run), cur)
        h = oracle.header_unpack(blob)
        names.append(h["pipename"])
        raw = np.frombuffer(bytes(blob), np.uint8)[h["size"]:h["size"] + h["bytes"]]
        if final:
            body = raw
        else:
            cur = raw.view(vol.dtype).reshape(vol.shape).copy()
        run.clear()

    for name, cfg in oracle.parse_pairs(pipeline):
        if not _is_bkrd(name):
            run.append(name + ("(" + cfg + ")" if cfg else ""))
            continue
        flush(False)
        if name == "rmestbkrd":
            cur = rmestbkrd(cur, l2_bytes)
            names.append("rmestbkrd")
        else:
            t, f = neighbor5_params(cfg, vol.dtype)
            cur = neighbor5(cur, t, f)
            names.append("rmbkrd_neighbor5x5x5(%s)" % neighbor5_config(t, f))
    flush(True)
    if body is None:
        body = cur.reshape(-1).view(np.uint8)
    return oracle.header_pack(vol.dtype, vol.shape, "->".join(names), body.size) + body.tobytes()


def filtered_volume(pipeline, vol, l2_bytes=None):
    """What SQY_Decode returns for a pipeline of background stages in front of lossless ones: the filtered volume"""
    cur = vol
    for name, cfg in _pairs(pipeline):
        if name == "rmestbkrd":
            cur = rmestbkrd(cur, l2_bytes)
        elif name == "rmbkrd_neighbor5x5x5":
            cur = neighbor5(cur, *neighbor5_params(cfg, vol.dtype))
    return cur


def _pairs(pipeline):
    out = []
    for major in pipeline.split("->"):
        d = major.find("(")
        out.append((major, "") if d < 0 else (major[:d], major[d + 1:-1]))
    return out


def full_pipename(oracle, pipeline, dtype):
    """name() of the pipeline as the library's SQY_Pipeline_Max_Compressed_Length / SQYAMD_Header_Build build it (fresh stages)"""
    parts = []
    for name, cfg in oracle.parse_pairs(pipeline):
        if name == "rmestbkrd":
            parts.append("rmestbkrd")
        elif name == "rmbkrd_neighbor5x5x5":
            parts.append(neighbor5_full_name(cfg, dtype))
        else:
            parts.append(oracle.pipeline_name(oracle.build_stages(name + ("(" + cfg + ")" if cfg else ""), dtype)))
    return "->".join(parts)


def max_encoded_size(oracle, pipeline, nbytes, dtype):
    """dynamic_pipeline::max_encoded_size (dynamic_pipeline.hpp:866-890) with the background stages as identity filters"""
    dtype = np.dtype(dtype)
    hdr = oracle.header_pack(dtype, (nbytes,), full_pipename(oracle, pipeline, dtype), nbytes * dtype.itemsize)
    sizes = [nbytes]
    for name, cfg in oracle.parse_pairs(pipeline):
        if name == "lz4":
            sizes.append(oracle.Lz4Config(cfg).max_encoded_size(nbytes, 1))
        elif name == "quantiser":
            sizes.append(nbytes * dtype.itemsize + 256 * dtype.itemsize)
    return 2 * len(hdr) + max(sizes)
