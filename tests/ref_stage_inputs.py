"""Inputs of the stage cases of tests/golden/ref_stages.json, regenerated from their seeds.  numpy only: the GPU test that holds the
product against the reference's goldens imports this and nothing of the oracle."""
import numpy as np


def np_dtype(name):
    """the array type a case's dtype name travels in ("char" is the tail-filter form: the same bytes, read as signed)"""
    return np.uint16 if name == "uint16" else np.uint8


def stage_input(kind, dtype, shape, seed):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    top = int(np.iinfo(dtype).max)
    n = int(np.prod(shape))
    if kind == "random":                                   # full range: the 3x3 sums wrap in the voxel type
        return rng.integers(0, top + 1, shape, dtype=dtype)
    if kind == "max":
        return np.full(shape, top, dtype)
    if kind == "zero":
        return np.zeros(shape, dtype)
    if kind == "ramp":
        return (np.arange(n) % (top + 1)).astype(dtype).reshape(shape)
    if kind == "pm128":                                    # bytes around +-128 when read as `char`
        return rng.integers(120, 137, shape).astype(dtype)
    if kind == "two_level":                                # 10 everywhere, 200 at every 7th voxel behind a first frame that is all 10
        v = np.full(n, 10, dtype)
        v[::7] = 200
        v = v.reshape(shape)
        v[0] = 10
        return v
    if kind == "gamma":
        return np.minimum(rng.gamma(2.0, 30.0, shape), top).astype(dtype)
    if kind == "equal_faces":                              # every face the estimator samples holds one value: four equal supports
        v = rng.integers(37, 200, shape).astype(dtype)
        v[0] = v[-1] = 37
        v[:, 0, :] = v[:, -1, :] = 37
        return v
    if kind == "low80":
        return rng.integers(0, 80, shape).astype(dtype)
    if kind == "near_wrap":                                # around 70000 mod 2^bits (4464 / 112): 4 in 13 below it
        lo = (70000 % (top + 1)) - 40
        return rng.integers(lo, lo + 130, shape).astype(dtype)
    raise KeyError(kind)


def stage_volume(case):
    return stage_input(case["kind"], np_dtype(case["dtype"]), tuple(case["shape"]), case["seed"])


def stage_tile(case):
    """tile_size of a reorder case; None in the table means the stage's default, 16 / sizeof(T)"""
    ts = case["params"].get("tile_size")
    return ts if ts else 16 // np.dtype(np_dtype(case["dtype"])).itemsize


def case_id(case, index):
    return "%s-%s-%s-%s-%03d" % (case["stage"], case["dtype"], "x".join(str(d) for d in case["shape"]), case["kind"], index)


def load_cases(path):
    """(_meta, cases) of tests/golden/ref_stages.json; the file leaves out what follows from the rest: empty params, and the ids"""
    import json
    with open(path) as f:
        gold = json.load(f)
    for i, c in enumerate(gold["cases"]):
        c.setdefault("params", {})
        c["id"] = case_id(c, i)
    return gold["_meta"], gold["cases"]
