"""Shared by the robust-resection-guess tests (tests/ only): the Python restatement of the trial sampler, long-double inlier
counts per candidate pose, the count of AMBIGUOUS matches -- those whose |r|^2 lies within 1e-9 tau^2 of tau^2, where float64 on
the device and long double here may fall on different sides -- and the g++-built harness of csrc/sba_resection_consensus.hpp
(tests/harness/resection_consensus_harness.cpp).  Scenes, residuals and the numpy DLT are tests/resection_reference.py's."""
from functools import lru_cache

import numpy as np

import resection_reference as rr

LD = np.longdouble
M64 = (1 << 64) - 1
AMBIGUITY = 1e-9


def splitmix64(s):
    """-> (value, new state), the generator of csrc/sba_epipolar.hpp."""
    s = (s + 0x9E3779B97F4A7C15) & M64
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31), s


def sample_trial(seed, trial, n, sample_size):
    """The matches trial `trial` draws: j = splitmix64 % n until sample_size distinct ones stand, in draw order."""
    s = (seed * 0x2545F4914F6CDD1D + trial * 0xD6E8FEB86659FD93 + 1) & M64
    out = []
    while len(out) < sample_size:
        v, s = splitmix64(s)
        j = v % n
        if j not in out:
            out.append(j)
    return out


def sample(seed, trials, n, sample_size):
    return np.array([sample_trial(seed, t, n, sample_size) for t in range(trials)], dtype=np.int64)


def sq_residuals(X, y, rot, tran):
    """(n,) long double |r_i|^2 at one pose."""
    if len(X) == 0:
        return np.zeros(0, dtype=LD)
    r = rr.per_match(X, y, rot, tran)[2]
    return np.sum(r * r, axis=1)


def counts(X, y, rots, trans, tau):
    """-> (inliers (count,) int64, ambiguous (count,) int64) over the candidate poses, in long double."""
    t2 = LD(tau) * LD(tau)
    inl, amb = [], []
    for rot, tran in zip(np.atleast_2d(rots), np.atleast_2d(trans)):
        s = sq_residuals(X, y, rot, tran)
        inl.append(int(np.sum(s <= t2)))
        amb.append(int(np.sum(np.abs(s - t2) <= LD(AMBIGUITY) * t2)))
    return np.array(inl, dtype=np.int64), np.array(amb, dtype=np.int64)


def noisy_scene(n):
    """The scenes of the consensus tests: bearing noise 1e-3, every third row a wrong match."""
    return rr.make_scene(n, 12, noise=1e-3, outliers=rr.planted(n, 0.3))


def exact_scene(n):
    """Noise-free, every third row a wrong match."""
    return rr.make_scene(n, 12, outliers=rr.planted(n, 0.3))


def inlier_rows(n):
    return np.setdiff1d(np.arange(n), np.array(rr.planted(n, 0.3), dtype=int))


SCORE_TAU = 0.02
SCORE_SIZES = {False: (1, 2, 63, 64, 65, 513), True: (1, 2, 63, 64, 65, 513, 1025)}     # by f32
SCORE_COUNTS = (1, 63, 64, 65, 200)
SCORE_LONG = {False: 1537, True: 3073}       # one block: three grid-stride steps and a ragged tail


def score_scene(n):
    """The scenes of the scoring tests: bearing noise 1e-3, 8 % wrong matches."""
    return rr.make_scene(n, 700 + n, noise=1e-3, outliers=rr.planted(n))


@lru_cache(maxsize=None)
def score_candidates(n, count=200):
    """(rots, trans), each (count, 3): the truth; the truth moved by 1e-3, 1e-1 and 1 along seeded directions; the zero rotation
    (the small-angle branch); a rotation near pi (tests/pose_edges.py); then seeded poses at log-uniform distances 1e-4 .. 1
    from the truth, so that the counts run from nearly all matches to none."""
    import pose_edges
    s = score_scene(n)
    rng = np.random.default_rng(9000 + n)
    unit = lambda: rr._unit(rng.standard_normal(3))
    rots, trans = [s.rot], [s.tran]
    for d in (1e-3, 1e-1, 1.0):
        rots.append(s.rot + d * unit())
        trans.append(s.tran + d * unit())
    rots += [np.zeros(3), pose_edges.POSES["near_pi"]]
    trans += [s.tran, s.tran]
    while len(rots) < count:
        d = 10.0 ** rng.uniform(-4.0, 0.0)
        rots.append(s.rot + d * unit())
        trans.append(s.tran + d * unit())
    rots, trans = np.ascontiguousarray(rots[:count]), np.ascontiguousarray(trans[:count])
    rots.setflags(write=False)
    trans.setflags(write=False)
    return rots, trans


@lru_cache(maxsize=None)
def score_reference(n, f32, count=200, tau=SCORE_TAU):
    """Long-double (inliers, ambiguous) of score_candidates(n, count) on score_scene(n); computed once, shared, left unchanged."""
    X, y = rr.planes(score_scene(n), f32)
    inl, amb = counts(X, y, *score_candidates(n, count), tau)
    inl.setflags(write=False)
    amb.setflags(write=False)
    return inl, amb


# ---- the product's host side through the g++-built harness -------------------------------------------------------------------
_h = None


def harness():
    global _h
    if _h is None:
        import ctypes as C
        import subprocess
        from pathlib import Path
        root = Path(__file__).resolve().parent.parent
        so = root / "tests" / "harness" / "libresection_consensus_harness.so"
        src = root / "tests" / "harness" / "resection_consensus_harness.cpp"
        hdrs = [root / "spherical_bundle_adjuster_amd" / "csrc" / f
                for f in ("sba_resection_consensus.hpp", "sba_resection.hpp", "sba_epipolar.hpp")] + [root / "include" / "sba_hip.h"]
        if not so.exists() or so.stat().st_mtime < max(f.stat().st_mtime for f in [src] + hdrs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so), str(src)], check=True)
        _h = C.CDLL(str(so))
        _h.consensus_harness_sample.argtypes = [C.c_ulonglong, C.c_int, C.c_ulonglong, C.c_int, C.POINTER(C.c_longlong)]
        _h.consensus_harness_sample.restype = None
    return _h


def harness_sample(seed, trials, n, sample_size):
    import ctypes as C
    out = np.full((trials, sample_size), -1, dtype=np.int64)
    h = harness()
    for t in range(trials):
        h.consensus_harness_sample(seed, t, n, sample_size, out[t].ctypes.data_as(C.POINTER(C.c_longlong)))
    return out


def harness_row_moments(rows):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    mom = np.full(61, np.nan)
    harness().consensus_harness_row_moments(rr._dp(rows), len(rows), rr._dp(mom))
    return mom


def harness_trial(rows):
    """-> (status, rot, tran, lambda2 / lambda12) of one trial on rows (m, 6)."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    rot, tran, info = np.zeros(3), np.zeros(3), np.zeros(7)
    rc = harness().consensus_harness_trial(rr._dp(rows), len(rows), rr._dp(rot), rr._dp(tran), rr._dp(info))
    return rc, rot, tran, (info[1] / info[2] if info[2] > 0 else 0.0)


def harness_pick(counts_):
    import ctypes as C
    c = np.ascontiguousarray(counts_, dtype=np.int64)
    return harness().consensus_harness_pick(c.ctypes.data_as(C.POINTER(C.c_longlong)), len(c))


@lru_cache(maxsize=None)
def harness_trials(n, f32, seed=7, trials=128, sample_size=6, noisy=True):
    """Every trial of the consensus call on a test scene through the harness: (status (T,), rot (T, 3), tran (T, 3),
    lambda2 / lambda12 (T,), indices (T, m)).  Computed once, shared, left unchanged."""
    s = noisy_scene(n) if noisy else exact_scene(n)
    X, y = rr.planes(s, f32)
    idx = sample(seed, trials, n, sample_size)
    st, rot, tran, cond = np.zeros(trials, dtype=int), np.zeros((trials, 3)), np.zeros((trials, 3)), np.zeros(trials)
    for t in range(trials):
        st[t], rot[t], tran[t], cond[t] = harness_trial(np.concatenate([X[idx[t]], y[idx[t]]], axis=1))
    for a in (st, rot, tran, cond, idx):
        a.setflags(write=False)
    return st, rot, tran, cond, idx
