"""Shared by tests/test_landmark_associate_cpu.py and tests/test_gpu_landmark_associate.py (import only; numpy, no GPU, no product
code): the rule by which a frame is associated with the landmark map, stated on top of
match_cases.exact_reference, and the case table.

The rule.  The matcher of section 3.10 runs with the frame rows as queries and the map's rows as train rows: frame row j gets
(i0, d0) and (i1, d1) and is ACCEPTED iff i1 >= 0, d0 < ratio * d1 in float32 and d0 <= max_distance in float32.  Landmark i's
claimants are the accepted rows with i0 == i; its winner is the claimant smallest in (bits of d0 as u32, j), compared
lexicographically (d0 >= 0, so the bit order is the value order; among equal distances the lowest frame row wins).  Output k is the
k-th smallest landmark that has a claimant: idx[k] = i, rows[k] its winner, distance[k] the winner's d0.  n_accepted = n_contested +
n_associated.  A frame row or a map row with a non-finite component takes no part.

With integer-valued descriptors inside match_cases.assert_exact_domain every f32 operation of the device path is exact, so the
device must equal this module in every output byte."""
import functools
from typing import NamedTuple

import numpy as np

import match_cases as mc


class Association(NamedTuple):
    n_frame: int
    n_accepted: int
    n_contested: int
    n_associated: int
    idx: np.ndarray        # (n_associated,) int64, strictly increasing
    rows: np.ndarray       # (n_associated,) int32, no repeats
    distance: np.ndarray   # (n_associated,) float32


def accepted(frame, map_rows, ratio, max_distance=np.inf):
    """(j, i0, d0) of the accepted frame rows, j ascending.  Rows with a non-finite component are left out on either side before
    match_cases.exact_reference sees the arrays, and the indices are those of the full arrays."""
    frame, map_rows = np.asarray(frame, dtype=np.float32), np.asarray(map_rows, dtype=np.float32)
    fj = np.flatnonzero(np.isfinite(frame).all(axis=1)) if frame.size else np.arange(len(frame))
    ti = np.flatnonzero(np.isfinite(map_rows).all(axis=1)) if map_rows.size else np.arange(len(map_rows))
    f, t = frame[fj], map_rows[ti]
    mc.assert_exact_domain(f, t)
    ref = mc.exact_reference(f, t, ratio)
    near = ref.distance <= np.float32(max_distance)
    return fj[ref.query_idx[near]].astype(np.int32), ti[ref.train_idx[near]].astype(np.int64), ref.distance[near].astype(np.float32)


def keys(d0, j):
    """(bits of d0 as u32) << 32 | j as uint64."""
    return (np.ascontiguousarray(d0, dtype=np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(j).astype(np.uint64)


def associate(frame, map_rows, ratio=0.3, max_distance=np.inf) -> Association:
    """The rule, vectorised: the accepted rows sorted by (landmark, key); the first of every landmark is its winner."""
    j, i, d = accepted(frame, map_rows, ratio, max_distance)
    order = np.lexsort((keys(d, j), i))
    i_sorted = i[order]
    first = np.ones(len(order), dtype=bool)
    first[1:] = i_sorted[1:] != i_sorted[:-1]
    win = order[first]
    return Association(len(frame), len(j), len(j) - len(win), len(win), i[win].astype(np.int64), j[win].astype(np.int32), d[win].astype(np.float32))


def associate_loop(frame, map_rows, ratio=0.3, max_distance=np.inf) -> Association:
    """The rule as a plain loop over the accepted rows: a dict of the best (bits, row) per landmark."""
    j, i, d = accepted(frame, map_rows, ratio, max_distance)
    best = {}
    for row, lm, dist in zip(j.tolist(), i.tolist(), d):
        cand = (int(np.float32(dist).view(np.uint32)), row)
        if lm not in best or cand < best[lm]:
            best[lm] = cand
    lms = sorted(best)
    dist = np.array([best[lm][0] for lm in lms], dtype=np.uint32).view(np.float32)
    return Association(len(frame), len(j), len(j) - len(lms), len(lms), np.array(lms, dtype=np.int64),
                       np.array([best[lm][1] for lm in lms], dtype=np.int32), dist)


class Case(NamedTuple):
    m: int                 # frame rows
    n: int                 # landmarks
    D: int
    share: float
    counts: dict           # ratio -> (accepted, associated, contested), the reference's own


# match_cases.planted_pair(m, n, D, share), its queries read as the frame and its train rows as the map.  The shapes cross the
# 32-row train tile, the 256-query block, kCompactTile on both sides and dp = 64 / 128, and hold a map of two rows.
CASES = (
    Case(600, 2049, 36, 2 / 3, {0.3: (400, 370, 30), 0.5: (400, 370, 30)}),
    Case(2051, 513, 64, 1.0, {0.3: (2051, 504, 1547), 0.5: (2051, 504, 1547)}),
    Case(257, 33, 5, 1.0, {0.3: (248, 33, 215), 0.5: (257, 33, 224)}),
    Case(1025, 4500, 65, 1 / 2, {0.3: (512, 483, 29), 0.5: (512, 483, 29)}),
    Case(300, 2, 8, 1.0, {0.3: (300, 2, 298), 0.5: (300, 2, 298)}),
)
RATIOS = (0.3, 0.5)


@functools.lru_cache(maxsize=None)
def arrays(k):
    """(frame, map) of CASES[k]: contiguous, read-only, built once."""
    c = CASES[k]
    q, t = mc.planted_pair(c.m, c.n, c.D, c.share)
    q, t = np.ascontiguousarray(q, dtype=np.float32), np.ascontiguousarray(t, dtype=np.float32)
    q.setflags(write=False)
    t.setflags(write=False)
    return q, t


@functools.lru_cache(maxsize=None)
def expected(k, ratio, max_distance=np.inf) -> Association:
    return associate(*arrays(k), ratio, max_distance)


def bearings_for(m, seed=0):
    """(m, 3) float64 unit rows with every bit pattern of interest nearby: random directions, row 0 with a negative zero."""
    rng = np.random.default_rng([77, m, seed])
    y = rng.normal(size=(m, 3))
    y /= np.linalg.norm(y, axis=1, keepdims=True)
    if m:
        y[0] = (-0.0, 0.0, 1.0)
    return y


def map_rows(n, seed=0):
    """(xyz (n, 3), cov (n, 6)) of a plain valid map: points a few units away, small diagonal covariances."""
    rng = np.random.default_rng([78, n, seed])
    xyz = rng.normal(size=(n, 3)) + np.array([0.0, 0.0, 6.0])
    cov = np.zeros((n, 6))
    cov[:, :3] = rng.uniform(1e-4, 1e-3, size=(n, 3))
    return xyz, cov
