"""Shared by the landmark-map edit tests (tests/ only): numpy restatements of the score, of the classes of a prune and of the edits
themselves, the cases the CPU qualification and the GPU tests walk, and the g++-built harness around csrc/sba_landmarks_edit.hpp.

Per landmark X with covariance rows (xx, yy, zz, xy, xz, yz) and `count` accepted observations:

    score = ((xx + yy) + zz) / ((x x + y y) + z z)                      float64, in exactly this order

numpy rounds every one of these operations on its own and never fuses two, so this IS the product's score to the bit.  The classes
of a prune, tested in this order: INVALID (a non-finite entry of X or Sigma, a negative variance), UNCERTAIN (not score <= max_score),
UNOBSERVED (count < min_count), MASKED (mask == 0), KEPT.  The edits are fancy indexing (prune, gather) and concatenation (append)."""
from functools import lru_cache

import numpy as np

import landmark_fusion_reference as lf

INVALID, UNCERTAIN, UNOBSERVED, MASKED, KEPT = range(5)
TILE = 2048                          # kCompactTile
SIZES = (0, 1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4097)
LONG = (6145,)                       # SBA_RESECT_GRID=1: one block takes several steps
COV_SCALE = lf.COV_SCALE
MARGIN = 1e-9
MASKS = ("all", "none", "first", "last", "alternating", "tile", "straddle", "half")


def scores(X, C):
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    with np.errstate(all="ignore"):
        return ((C[:, 0] + C[:, 1]) + C[:, 2]) / ((X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1]) + X[:, 2] * X[:, 2])


def classify(X, C, counts, max_score=np.inf, min_count=0, mask=None):
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    n = len(X)
    with np.errstate(all="ignore"):
        invalid = ~np.isfinite(X).all(axis=1) | ~np.isfinite(C).all(axis=1) | (C[:, :3] < 0).any(axis=1)
        uncertain = ~(scores(X, C) <= max_score)
    unobserved = np.asarray(counts) < min_count
    masked = np.zeros(n, dtype=bool) if mask is None else np.asarray(mask) == 0
    return np.where(invalid, INVALID, np.where(uncertain, UNCERTAIN, np.where(unobserved, UNOBSERVED, np.where(masked, MASKED, KEPT)))).astype(int)


def prune(X, C, counts, max_score=np.inf, min_count=0, mask=None):
    """-> (kept indices ascending, (n_before, n_invalid, n_uncertain, n_unobserved, n_masked, n_kept))."""
    cls = classify(X, C, counts, max_score, min_count, mask)
    return np.flatnonzero(cls == KEPT).astype(np.int64), (len(cls),) + tuple(int((cls == k).sum()) for k in range(5))


def take(state, idx):
    X, C, k = state
    return X[idx], C[idx], k[idx]


def append(state, Xa, Ca, cov_scale):
    X, C, k = state
    Xa, Ca = np.asarray(Xa, dtype=np.float64).reshape(-1, 3), np.asarray(Ca, dtype=np.float64).reshape(-1, 6)
    return np.concatenate([X, Xa]), np.concatenate([C, cov_scale * Ca]), np.concatenate([k, np.zeros(len(Xa), dtype=np.uint32)])


def state_bytes(state):
    X, C, k = state
    return np.ascontiguousarray(X).tobytes() + np.ascontiguousarray(C).tobytes() + np.ascontiguousarray(k, dtype=np.uint32).tobytes()


def median_cut(s):
    """A max_score at the median of the finite scores: the midpoint of the two scores around the middle of their sorted order, so
    that the cut lies between two scores and never on one (a score equal to the cut could not keep the margin the tests demand)."""
    f = np.sort(s[np.isfinite(s)])
    if len(f) == 0:
        return 1.0
    if len(f) == 1:
        return 2.0 * float(f[0])
    k = len(f) // 2
    return 0.5 * (float(f[k - 1]) + float(f[k]))


def margin_ok(s, max_score):
    """No finite score within MARGIN relative of the cut."""
    f = s[np.isfinite(s)]
    return not np.isfinite(max_score) or bool((np.abs(f - max_score) > MARGIN * max_score).all())


def mask(name, n):
    """The mask patterns of the prune tests, (n,) bool; the tile ones fall back on thirds below two tiles."""
    m = np.ones(n, dtype=bool)
    if name == "all":
        return m
    if name == "none":
        return ~m
    if name == "first":
        m[:] = False
        m[:1] = True
    elif name == "last":
        m[:] = False
        m[n - 1:] = True
    elif name == "alternating":
        m[1::2] = False
    elif name == "tile":                    # one whole tile dropped (the second where there are three, else the first)
        lo = TILE if n > 2 * TILE else 0
        m[lo:lo + TILE] = False
    elif name == "straddle":                # one kept run across the first tile boundary (or across the middle)
        mid = TILE if n > TILE else n // 2
        m[:] = False
        m[max(0, mid - 37):mid + 38] = True
    elif name == "half":
        m = np.random.default_rng(7000 + n).random(n) < 0.5
    else:
        raise KeyError(name)
    return m


PLANTED = ("NaN in X", "inf in Sigma", "negative variance", "X = 0")


def planted_rows(n):
    """Rows spread over waves, blocks and tiles, the last row among them: name -> several rows each (n >= 255)."""
    at = lambda frac: min(n - 1, int(frac * n))
    rows = {"NaN in X": (0.03, 0.27, 0.52, 1.0), "inf in Sigma": (0.01, 0.34, 0.61, 0.87), "negative variance": (0.12, 0.49, 0.76),
            "X = 0": (0.2, 0.45, 0.7, 0.93)}
    return {k: sorted({at(f) for f in v}) for k, v in rows.items()}


@lru_cache(maxsize=None)
def edit_map(n, planted=False):
    """A seeded map in the fusion tests' recipe and two frames to fuse into it: (X, cov as given to set, frames), frames a list of
    (bearings, idx or None).  The first frame is dense, the second sees about half the landmarks; both pass a gate, so the counts
    differ per landmark.  planted: rows of every invalid kind and X = 0, which no frame sees (a zero bearing / not in idx)."""
    s = lf.scene(n, "series")
    X, cov, y = s.X.copy(), s.cov.copy(), s.y.copy()
    idx = lf.subset(n)
    if planted:
        rows = planted_rows(n)
        for k, i in enumerate(rows["NaN in X"]):
            X[i, k % 3] = np.nan
        for k, i in enumerate(rows["inf in Sigma"]):
            cov[i, k % 6] = np.inf
        for k, i in enumerate(rows["negative variance"]):
            cov[i, k % 3] = -cov[i, k % 3]
        for i in rows["X = 0"]:
            X[i] = 0.0
            y[i] = 0.0
        idx = np.setdiff1d(idx, rows["X = 0"]).astype(np.int64)
    rng = np.random.default_rng(9100 + n)
    y2 = y + 2e-3 * rng.standard_normal(y.shape) * np.linalg.norm(y, axis=1, keepdims=True)
    for a in (X, cov, y, y2, idx):
        a.setflags(write=False)
    return X, cov, [(y, None), (y2[idx], idx)], (s.rot.copy(), s.tran.copy())


def extra_rows(n_add, seed=0):
    """Rows to append: another seeded map's."""
    s = lf.scene(max(n_add, 3), "closed") if n_add <= 3 else lf.scene(n_add, "closed")
    return s.X[:n_add].copy(), s.cov[:n_add].copy()


# ---- the product's host side through the g++-built harness (tests/harness/landmark_edit_harness.cpp) ----------------------------
_h = None


def harness():
    """csrc/sba_landmarks_edit.hpp compiled for the CPU."""
    global _h
    if _h is None:
        import ctypes as C
        import subprocess
        from pathlib import Path
        root = Path(__file__).resolve().parent.parent
        so = root / "tests" / "harness" / "liblandmark_edit_harness.so"
        src = root / "tests" / "harness" / "landmark_edit_harness.cpp"
        hdrs = [root / "spherical_bundle_adjuster_amd" / "csrc" / f for f in ("sba_landmarks_edit.hpp", "sba_rotation.hpp")]
        if not so.exists() or so.stat().st_mtime < max(f.stat().st_mtime for f in [src] + hdrs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so), str(src)], check=True)
        _h = C.CDLL(str(so))
        dp = C.POINTER(C.c_double)
        _h.landmark_edit_harness_scores.argtypes = [C.c_longlong, dp, dp, dp]
        _h.landmark_edit_harness_classes.argtypes = [C.c_longlong, dp, dp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.c_double, C.c_uint32,
                                                     C.POINTER(C.c_int)]
        _h.landmark_edit_harness_check_max_score.argtypes = [C.c_double]
        _h.landmark_edit_harness_check_gather_index.argtypes = [C.POINTER(C.c_int64), C.c_size_t, C.c_size_t]
        _h.landmark_edit_harness_check_sizes.argtypes = [C.c_size_t, C.c_size_t]
    return _h


def harness_scores(X, C):
    import ctypes as ct
    X, C = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(C, dtype=np.float64)
    out = np.full(len(X), -7.0)
    dp = lambda a: a.ctypes.data_as(ct.POINTER(ct.c_double))
    harness().landmark_edit_harness_scores(len(X), dp(X), dp(C), dp(out))
    return out


def harness_classes(X, C, counts, max_score=np.inf, min_count=0, mask=None):
    import ctypes as ct
    X, C = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(C, dtype=np.float64)
    k = np.ascontiguousarray(counts, dtype=np.uint32)
    mk = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    cls = np.full(len(X), -1, dtype=np.int32)
    dp = lambda a: a.ctypes.data_as(ct.POINTER(ct.c_double))
    harness().landmark_edit_harness_classes(len(X), dp(X), dp(C), k.ctypes.data_as(ct.POINTER(ct.c_uint32)),
                                            None if mk is None else mk.ctypes.data_as(ct.POINTER(ct.c_uint8)), float(max_score), int(min_count),
                                            cls.ctypes.data_as(ct.POINTER(ct.c_int)))
    return cls.astype(int)


@lru_cache(maxsize=None)
def cpu_state(n, planted=False):
    """The map of edit_map(n) after its two frames, fused by csrc/sba_landmarks.hpp on the CPU: (X, Sigma, counts), what the device
    holds up to the rounding of the fusion -- the state the CPU tests classify."""
    X, cov, frames, (rot, tran) = edit_map(n, planted)
    X, C, k = X.copy(), COV_SCALE * cov, np.zeros(n, dtype=np.uint32)
    for y, idx in frames:
        rows = np.arange(n) if idx is None else idx
        if len(rows) == 0:
            continue
        with np.errstate(all="ignore"):
            f = lf.harness_fuse(X[rows], C[rows], y, rot, tran, 1e-3, lf.GATE)
        X[rows], C[rows] = f.X, f.cov
        k[rows] += (f.cls == lf.FUSED).astype(np.uint32)
    return X, C, k
