"""Shared by tests/test_match_cases_cpu.py and tests/test_gpu_match_exact.py (import only; no GPU, no product code): the
integer-valued descriptor cases of the 2-NN match and their exact reference.

With small-integer descriptors every f32 operation of the device path is exact -- the scaling by -2, the fmaf chain of
|t|^2, the MFMA accumulation started at |t|^2, the rescoring sum (q - t)^2: all partial sums are integers below 2^24 -- so
the device must equal an integer brute force in every output bit and no tie window is needed.  assert_exact_domain states
the condition; every case builder below returns arrays that satisfy it.

split_plan restates the documented split rule.  It only tells which tile ranges a case reaches (the CPU file asserts the
coverage, the GPU file prints it for the device it ran on); no expected result depends on it."""
import functools
import re
from typing import Callable, NamedTuple

import numpy as np

from helpers import ROOT

CSRC = ROOT / "spherical_bundle_adjuster_amd" / "csrc"
TRAIN_TILE = 32                  # train rows per MFMA tile (section 3.10)
RATIOS = (0.3, 0.9, 1.0)         # every random case runs at these
ALL_D = (1, 2, 3, 4, 5, 35, 36, 63, 64, 65, 127, 128, 129, 200, 255, 256)
ALL_NQ = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 513)
ALL_NT = (2, 3, 31, 32, 33, 127, 128, 129, 511, 512, 513, 2049, 8193)


@functools.lru_cache(maxsize=None)
def compact_tile() -> int:
    """kCompactTile, the rows per scan tile of the compaction, read from the sources (not restated)."""
    for f in sorted(CSRC.glob("*.h*")):
        m = re.search(r"constexpr\s+int\s+kCompactTile\s*=\s*(\d+)\s*;", f.read_text())
        if m:
            return int(m.group(1))
    raise AssertionError("kCompactTile not found under csrc/")


# ---------------------------------------------------------------------------------------------------------------------
# the exact reference
# ---------------------------------------------------------------------------------------------------------------------
class Ref(NamedTuple):
    nn_index: np.ndarray      # (nq, 2) int32
    nn_distance: np.ndarray   # (nq, 2) float32
    query_idx: np.ndarray     # (n_matched,) int32, ascending
    train_idx: np.ndarray     # (n_matched,) int32
    distance: np.ndarray      # (n_matched,) float32


class BatchRef(NamedTuple):
    nn_index: np.ndarray
    nn_distance: np.ndarray
    n_matched: np.ndarray     # (B,) int64
    match_offsets: np.ndarray  # (B + 1,) int64
    query_idx: np.ndarray
    train_idx: np.ndarray
    distance: np.ndarray


def assert_exact_domain(q, t):
    """Integer entries with 3 D max|v|^2 < 2^24: |q - t|^2 <= 4 D max^2 would be the crude bound on the rescoring sum, but
    (q_k - t_k)^2 <= 2 (q_k^2 + t_k^2) and the score |t|^2 - 2 q.t has partial sums within |t|^2 + 2 |q||t| <= 3 D max^2."""
    q, t = np.asarray(q), np.asarray(t)
    assert q.ndim == 2 and t.ndim == 2 and q.shape[1] == t.shape[1]
    D = q.shape[1]
    vmax = 0.0
    for a in (q, t):
        if a.size:
            assert np.isfinite(a).all() and np.array_equal(a, np.rint(a)), "entries must be integers"
            vmax = max(vmax, float(np.abs(a).max()))
    assert 3 * D * vmax * vmax < 2.0**24, (D, vmax)


def squared_distances(q, t) -> np.ndarray:
    """(nq, nt) int64 sum_k (q_k - t_k)^2.  Formed as |q|^2 + |t|^2 - 2 q.t in float64, which is exact here: every term and
    every partial sum is an integer far below 2^53 (tests/test_match_cases_cpu.py checks it against a plain int64 loop)."""
    q64, t64 = np.asarray(q, dtype=np.float64), np.asarray(t, dtype=np.float64)
    d2 = (q64 * q64).sum(1)[:, None] + (t64 * t64).sum(1)[None, :] - 2.0 * (q64 @ t64.T)
    return d2.astype(np.int64)


def exact_top2(q, t):
    """Per query the two train rows lowest in (d^2, index): (nn_index (nq, 2) int32, nn_distance (nq, 2) float32 =
    sqrt(float32(d^2)), correctly rounded).  One train row: [0, -1] with (d, +inf); none: [-1, -1] with (+inf, +inf).
    The order is that of a stable sort by d^2; it is taken from the two smallest of the unique keys d^2 * nt + index, which
    is the same thing without sorting whole rows."""
    nq, nt = len(q), len(t)
    idx = np.full((nq, 2), -1, dtype=np.int32)
    dist = np.full((nq, 2), np.inf, dtype=np.float32)
    if nq == 0 or nt == 0:
        return idx, dist
    d2 = squared_distances(q, t)
    key = d2 * nt + np.arange(nt, dtype=np.int64)[None, :]
    k2 = min(2, nt)
    low = np.sort(np.partition(key, k2 - 1, axis=1)[:, :k2], axis=1) if nt > 1 else key
    idx[:, :k2] = low % nt
    dist[:, :k2] = np.sqrt((low // nt).astype(np.float32))
    return idx, dist


def exact_reference(q, t, ratio, top2=None) -> Ref:
    """The match of one pair: top-2 as exact_top2 (pass a precomputed one to share it between ratios), the ratio test
    d0 < float32(ratio) * d1 all in float32, the accepted matches in ascending query order."""
    idx, dist = exact_top2(q, t) if top2 is None else top2
    accept = (idx[:, 1] >= 0) & (dist[:, 0] < np.float32(ratio) * dist[:, 1])
    qi = np.flatnonzero(accept).astype(np.int32)
    return Ref(idx, dist, qi, idx[qi, 0].copy(), dist[qi, 0].copy())


def batch_reference(Q, qo, T, to, ratio) -> BatchRef:
    """exact_reference per pair (rows qo[g] .. qo[g + 1] against to[g] .. to[g + 1]); per-query outputs are indexed by
    query row - qo[0], the matches are concatenated in pair order with pair-local indices."""
    qo, to = np.asarray(qo, dtype=np.int64), np.asarray(to, dtype=np.int64)
    B = qo.size - 1
    refs = [exact_reference(Q[qo[g]:qo[g + 1]], T[to[g]:to[g + 1]], ratio) for g in range(B)]
    n = np.array([r.query_idx.size for r in refs], dtype=np.int64)
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum(n)
    cat = lambda xs, dt, shape: np.concatenate(xs) if xs else np.zeros(shape, dt)
    return BatchRef(cat([r.nn_index for r in refs], np.int32, (0, 2)), cat([r.nn_distance for r in refs], np.float32, (0, 2)),
                    n, off, cat([r.query_idx for r in refs], np.int32, (0,)), cat([r.train_idx for r in refs], np.int32, (0,)),
                    cat([r.distance for r in refs], np.float32, (0,)))


# ---------------------------------------------------------------------------------------------------------------------
# the documented split rule
# ---------------------------------------------------------------------------------------------------------------------
class SplitPlan(NamedTuple):
    dp: int             # padded dimension: 64 / 128 / 256
    query_block: int    # queries per block: 256, or 128 at dp = 256
    qblocks: int        # query blocks of all pairs
    splits: int         # ranges the train tiles of every pair are cut into
    ranges: tuple       # per pair: ((first tile, end tile), ...) of its `splits` ranges


def padded_dim(D: int) -> int:
    return 64 if D <= 64 else 128 if D <= 128 else 256


def query_block(D: int) -> int:
    return 128 if padded_dim(D) == 256 else 256


def split_plan(nqs, nts, D, cus) -> SplitPlan:
    """Section 3.10: about four blocks per CU, at least 4 tiles per range, at most 64 ranges, one count for the batch."""
    dp, qb = padded_dim(D), query_block(D)
    qblocks = sum(-(-int(n) // qb) for n in nqs)
    tiles = [-(-int(n) // TRAIN_TILE) for n in nts]
    max_tiles = max(tiles, default=0)
    splits = -(-4 * max(int(cus), 1) // qblocks) if qblocks else 1
    splits = max(1, min(splits, max(1, max_tiles // 4), 64))
    ranges = tuple(tuple((s * T // splits, (s + 1) * T // splits) for s in range(splits)) for T in tiles)
    return SplitPlan(dp, qb, qblocks, splits, ranges)


def range_of(plan: SplitPlan, pair: int, row) -> np.ndarray:
    """The split range that holds train row `row` (array) of pair `pair`."""
    ends = np.array([e for _, e in plan.ranges[pair]], dtype=np.int64)
    return np.searchsorted(ends, np.asarray(row, dtype=np.int64) // TRAIN_TILE, side="right")


# ---------------------------------------------------------------------------------------------------------------------
# row layouts: contiguous, or a view of a wider array whose padding columns hold NaN / 1e30
# ---------------------------------------------------------------------------------------------------------------------
LAYOUTS = {"contig": (0, 0.0), "pad1_nan": (1, np.nan), "pad7_big": (7, 1e30), "pad7_nan": (7, np.nan), "pad1_big": (1, 1e30)}
LAYOUT_CYCLE = tuple(LAYOUTS)


def strided(a, layout):
    """`a` (n, D) as rows of D + pad floats with the padding columns filled; "contig" returns a contiguous copy."""
    pad, fill = LAYOUTS[layout]
    a = np.ascontiguousarray(a, dtype=np.float32)
    if pad == 0:
        return a.copy()
    wide = np.full((a.shape[0], a.shape[1] + pad), fill, dtype=np.float32)
    wide[:, :a.shape[1]] = a
    return wide[:, :a.shape[1]]


# ---------------------------------------------------------------------------------------------------------------------
# single-pair cases
# ---------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    family: str
    D: int
    nq: int
    nt: int
    ratios: tuple
    layouts: tuple       # keys of LAYOUTS the case runs in
    build: Callable      # () -> (q, t): contiguous f32 (nq, D), (nt, D)


_FAMILY_SEED = {"perm": 1, "ties_small": 2, "ties_pool": 3, "ratio": 4, "planted": 5, "grid": 6, "batch": 7, "stale": 8, "nan": 9,
                "upload": 10}


def _rng(family, *key):
    return np.random.default_rng([_FAMILY_SEED[family], *[int(k) for k in key]])


def _ints(rng, n, D, lo=-8, hi=8):
    return rng.integers(lo, hi + 1, size=(n, D)).astype(np.float32)


def random_pair(family, nq, nt, D):
    rng = _rng(family, nq, nt, D)
    return _ints(rng, nq, D), _ints(rng, nt, D)


def onehot_pair(D):
    """Train rows 2 e_k, k = 0 .. D - 1, then the same in reverse order; queries 2 e_k.  Query k: row k at 0, its copy
    2 D - 1 - k at 0, every other row at 8."""
    eye = 2.0 * np.eye(D, dtype=np.float32)
    return eye.copy(), np.concatenate([eye, eye[::-1]])


def perm_rows(nq, nt):
    """The train rows the queries of a permutation case copy, before shuffling: all of them if nq == nt, else one row per
    32-row tile at a position that walks through all 32 slots (5 i mod 32), the last one moved to the very last row."""
    if nq == nt:
        return np.arange(nt)
    rows = np.array([TRAIN_TILE * i + (5 * i) % TRAIN_TILE for i in range(nq)], dtype=np.int64)
    assert rows[-1] < nt - 1
    rows[-1] = nt - 1
    return rows


def perm_of(nq, nt, D):
    return _rng("perm", nq, nt, D, 1).permutation(perm_rows(nq, nt))


def perm_pair(nq, nt, D):
    """q = t[pi]: every train row pi touches is the nearest row (d^2 = 0) of exactly one query."""
    t = _ints(_rng("perm", nq, nt, D), nt, D)
    return t[perm_of(nq, nt, D)].copy(), t


def ties_small_pair(nq, nt, D):
    """Entries in {-1, 0, 1} (0 with probability 1 / 2): few distinct distances, so ranks 1 / 2 / 3 tie for a large share of
    the queries."""
    rng = _rng("ties_small", nq, nt, D, 1)
    draw = lambda n: rng.choice([-1.0, 0.0, 1.0], size=(n, D), p=[0.25, 0.5, 0.25]).astype(np.float32)
    return draw(nq), draw(nt)


def ties_pool_pair(nq, nt, D):
    """Train rows drawn with replacement from nt / 8 random rows, queries drawn from the same pool: the first two
    neighbours of almost every query are exact copies (d^2 = 0) at arbitrary positions."""
    rng = _rng("ties_pool", nq, nt, D)
    pool = _ints(rng, max(nt // 8, 1), D)
    return pool[rng.integers(0, pool.shape[0], nq)].copy(), pool[rng.integers(0, pool.shape[0], nt)].copy()


def _offset_with_norm2(n, D, first):
    """An integer vector with squared norm n: greedy squares from component `first` on."""
    v = np.zeros(D, dtype=np.float32)
    k = first
    while n > 0:
        a = int(np.floor(np.sqrt(n)))
        v[k % D] = a
        n -= a * a
        k += 1
    return v


class RatioCase(NamedTuple):
    ratio: float
    d0sq: int
    d1sq: int
    accept: bool       # the float32 decision the reference's matcher takes
    accept_f64: bool   # the decision of float64(d0) < float64(float32(ratio)) * float64(d1)


RATIO_CASES = (RatioCase(0.3, 9, 100, False, True), RatioCase(0.3, 36, 400, False, True), RatioCase(0.3, 8, 100, True, True),
               RatioCase(0.5, 25, 100, False, False), RatioCase(0.5, 24, 100, True, True), RatioCase(1.0, 9, 9, False, False),
               RatioCase(1.5, 9, 9, True, True))


def ratio_pair(rc: RatioCase, which: int):
    """Three equal queries c; train rows c + offsets with |offset|^2 = d0sq and d1sq exactly, placed among rows at 900.
    In odd cases the second neighbour comes first in index order."""
    D, nt = 8, 40
    rng = _rng("ratio", which)
    c = _ints(rng, 1, D)[0]
    t = np.repeat(c[None, :], nt, axis=0)
    for r in range(nt):
        t[r, r % D] += 30.0 if (r // D) % 2 == 0 else -30.0
    i0, i1 = (33, 6) if which % 2 else (6, 33)
    t[i0] = c + _offset_with_norm2(rc.d0sq, D, 0)
    t[i1] = c - _offset_with_norm2(rc.d1sq, D, 4)
    return np.repeat(c[None, :], 3, axis=0), t


def planted_pair(nq, nt, D, share):
    """`share` of the queries (the first ones of a shuffled order: positions all over) are a train row with one or two
    entries moved by +-1 (d0^2 in {1, 2} against a second neighbour in the hundreds: accepted at 0.3 and 0.5); the others
    are random rows (never accepted at 0.5 or below)."""
    rng = _rng("planted", nq, nt, D, int(share * 100))
    t = _ints(rng, nt, D)
    q = _ints(rng, nq, D)
    chosen = rng.permutation(nq)[: int(round(share * nq))]
    src = rng.integers(0, nt, chosen.size)
    q[chosen] = t[src]
    for i in chosen:
        cols = rng.choice(D, size=rng.integers(1, 3), replace=False)
        q[i, cols] += rng.choice([-1.0, 1.0], size=cols.size)
    return q, t


def grid_triples():
    """A pairwise-covering list of (D, nq, nt): every D, nq and nt of the issue's lists, and each padded dimension at each
    of nt in {33, 2049, 8193} x nq in {1, block - 1, block, block + 1}."""
    by_dp = {64: [d for d in ALL_D if d <= 64], 128: [d for d in ALL_D if 64 < d <= 128], 256: [d for d in ALL_D if d > 128]}
    out = []
    for dp, ds in by_dp.items():
        qb = query_block(ds[0])
        i = 0
        for nt in (33, 2049, 8193):
            for nq in (1, qb - 1, qb, qb + 1):
                out.append((ds[i % len(ds)], nq, nt))
                i += 1
    nts = (2, 3, 31, 32, 127, 128, 129, 511, 512, 513)
    nqs = (31, 32, 33, 127, 128, 129, 513, 255, 256, 257)
    for i in range(20):
        out.append((ALL_D[(5 * i + 3) % len(ALL_D)], nqs[(3 * i) % len(nqs)], nts[i % len(nts)]))
    return out


def _cases():
    fam = {}

    def add(name, family, D, nq, nt, ratios, build):
        fam.setdefault(family, []).append(Case(name, family, D, nq, nt, tuple(ratios), (), build))

    for D in ALL_D:
        add(f"onehot_D{D}", "onehot", D, D, 2 * D, (0.3, 1.5), functools.partial(onehot_pair, D))
    for nq, nt, D in ((33, 33, 64), (129, 129, 64), (2049, 2049, 64), (256, 8193, 64), (129, 129, 200), (2049, 2049, 100),
                      (256, 8193, 129)):
        add(f"perm_{nq}x{nt}_D{D}", "perm", D, nq, nt, RATIOS, functools.partial(perm_pair, nq, nt, D))
    for nq, nt, D in ((257, 2049, 64), (257, 513, 5)):
        add(f"ties_small_{nq}x{nt}_D{D}", "ties_small", D, nq, nt, RATIOS, functools.partial(ties_small_pair, nq, nt, D))
    for nq, nt, D in ((257, 2049, 64), (129, 8193, 36), (257, 2049, 200)):
        add(f"ties_pool_{nq}x{nt}_D{D}", "ties_pool", D, nq, nt, RATIOS, functools.partial(ties_pool_pair, nq, nt, D))
    for i, rc in enumerate(RATIO_CASES):
        add(f"ratio_{rc.ratio}_{rc.d0sq}_{rc.d1sq}", "ratio", 8, 3, 40, (rc.ratio,), functools.partial(ratio_pair, rc, i))
    tile = compact_tile()
    for nq, nt, D, share in ((tile + 1, 2049, 36, 1 / 3), (tile + 1, 2049, 36, 1.0), (2 * tile + 3, 4500, 65, 1 / 3),
                             (2 * tile + 3, 4500, 65, 1.0)):
        add(f"planted_{nq}x{nt}_D{D}_{'all' if share == 1.0 else 'third'}", "planted", D, nq, nt, (0.3, 0.5),
            functools.partial(planted_pair, nq, nt, D, share))
    for D, nq, nt in grid_triples():
        add(f"grid_D{D}_{nq}x{nt}", "grid", D, nq, nt, RATIOS, functools.partial(random_pair, "grid", nq, nt, D))
    # layouts: the cases of a family walk through LAYOUT_CYCLE; a family with fewer cases than layouts gives its cases several
    out = []
    for k in fam.values():
        for i, c in enumerate(k):
            out.append(c._replace(layouts=LAYOUT_CYCLE[i::len(k)] if len(k) < len(LAYOUT_CYCLE) else
                                  (LAYOUT_CYCLE[i % len(LAYOUT_CYCLE)],)))
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def arrays(name):
    """(q, t) of a case: contiguous, read-only, built once."""
    q, t = CASE_BY_NAME[name].build()
    q, t = np.ascontiguousarray(q, dtype=np.float32), np.ascontiguousarray(t, dtype=np.float32)
    q.setflags(write=False)
    t.setflags(write=False)
    return q, t


@functools.lru_cache(maxsize=None)
def top2(name):
    """exact_top2 of a case, computed once and shared by its ratios."""
    idx, dist = exact_top2(*arrays(name))
    idx.setflags(write=False)
    dist.setflags(write=False)
    return idx, dist


def reference(name, ratio) -> Ref:
    return exact_reference(*arrays(name), ratio, top2=top2(name))


# ---------------------------------------------------------------------------------------------------------------------
# ragged batches
# ---------------------------------------------------------------------------------------------------------------------
class BatchCase(NamedTuple):
    name: str
    D: int
    pairs: tuple         # ((nq, nt), ...)
    ratios: tuple
    layout: str


# empty pairs on either side and both, nt in {0, 1}, nq = 1, and pairs with fewer train tiles than the batch's split count
# (set by the largest pair: 94 / 257 tiles -> 23 / 64 ranges on 256 CUs)
BATCH_CASES = (
    BatchCase("batch_D36", 36, ((300, 1500), (0, 40), (1, 0), (1, 1), (257, 3000), (40, 0), (0, 0), (1, 70), (33, 2), (129, 513)),
              (0.3, 0.9), "contig"),
    BatchCase("batch_D200", 200, ((0, 0), (129, 8193), (1, 33), (0, 5), (128, 1), (7, 0), (127, 160), (1, 1)), (0.3, 1.0),
              "pad7_nan"),
    BatchCase("batch_D65", 65, ((1, 3), (5, 0), (0, 9), (256, 700), (2, 1), (31, 95), (0, 0)), (0.5,), "pad1_big"),
)
BATCH_BY_NAME = {b.name: b for b in BATCH_CASES}
EMBED_Q0, EMBED_T0 = 5, 3     # first offsets of the embedded variant
EMBED_TAIL = 4                # rows after the last pair, NaN like the ones before the first


@functools.lru_cache(maxsize=None)
def batch_arrays(name):
    """(Q, qo, T, to) with offsets from 0: per pair about half the queries are planted (a train row of the pair moved by
    +-1 in one or two entries), the others random."""
    bc = BATCH_BY_NAME[name]
    qs, ts = [], []
    for g, (nq, nt) in enumerate(bc.pairs):
        rng = _rng("batch", bc.D, g, nq, nt)
        t, q = _ints(rng, nt, bc.D), _ints(rng, nq, bc.D)
        if nt > 0:
            for i in np.flatnonzero(rng.random(nq) < 0.5):
                q[i] = t[rng.integers(0, nt)]
                q[i, rng.integers(0, bc.D)] += rng.choice([-1.0, 1.0])
        qs.append(q)
        ts.append(t)
    qo = np.concatenate([[0], np.cumsum([n for n, _ in bc.pairs])]).astype(np.uint64)
    to = np.concatenate([[0], np.cumsum([n for _, n in bc.pairs])]).astype(np.uint64)
    Q, T = np.concatenate(qs), np.concatenate(ts)
    Q.setflags(write=False)
    T.setflags(write=False)
    return Q, qo, T, to


def embedded(a, off, first, tail=EMBED_TAIL, fill=np.nan):
    """`a`'s rows inside a larger array: `first` rows before and `tail` rows after, all `fill`; the offsets moved along."""
    big = np.full((first + a.shape[0] + tail,) + a.shape[1:], fill, dtype=a.dtype)
    big[first:first + a.shape[0]] = a
    return big, (np.asarray(off, dtype=np.uint64) + np.uint64(first))
