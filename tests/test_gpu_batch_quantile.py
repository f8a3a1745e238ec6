"""GPU: every pair's exact order statistics of its squared residual norms (Batch.residual_order_stats / residual_quantiles,
sba_batch_residual_order_stats) and the per-pair inlier cut (Batch.keep_below, sba_batch_keep_below).

A pair's values must be, in all 8 bytes, np.partition of its own rows of Batch.residuals(...).sq_norm, and what the same
pair gives when it is selected alone; keep_below must keep exactly the rows at or below each pair's own threshold and leave
the batch bit-identical to a fresh upload of them."""
import numpy as np
import pytest

from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api, synthetic

pytestmark = pytest.mark.gpu

STORES = (api.STORE_F64, api.STORE_F32)
PROBS = (0.0, 0.25, 0.5, 0.9, 1.0)
RAGGED = [0, 1, 2, 255, 256, 257, 0, 2049, 4097, 1, 30_001, 0]


@pytest.fixture
def pinned_grid(monkeypatch):
    """Same grids for every handle (read at creation / upload): a compacted and a fresh batch reduce in the same order."""
    monkeypatch.setenv("SBA_BLOCKS_PER_CU", "2")


class Pairs:
    def __init__(self, sizes, seed=0):
        self.sizes = list(sizes)
        cs = [synthetic.full_rt(n, seed=synthetic.BASE_SEED + 2500 + 37 * seed + g, outlier_fraction=0.1)
              for g, n in enumerate(self.sizes)]
        B = len(cs)
        self.cs = cs
        self.off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.uint64)
        cat = lambda f, w: np.concatenate([f(c) for c in cs]) if sum(self.sizes) else np.zeros((0, w))
        self.x1, self.x2, self.d12 = cat(lambda c: c.x1, 3), cat(lambda c: c.x2, 3), cat(lambda c: c.d12, 2)
        self.rot = np.stack([c.rot_init for c in cs])
        self.tran = np.stack([c.tran_init for c in cs])
        self.d1 = 1.0 + 0.1 * (np.arange(B) % 5)          # per-pair uniform depths
        self.d2 = 0.7 + 0.05 * (np.arange(B) % 7)
        self.pair = np.repeat(np.arange(B), self.sizes)   # pair of every row

    def kw(self, per_match):
        return dict(depth_mode=api.DEPTH_PER_MATCH) if per_match else dict(d1=self.d1, d2=self.d2, depth_mode=api.DEPTH_UNIFORM)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _want(s, off, probs):
    """np.partition of every pair's own rows at floor(p (n - 1)); NaN for an empty pair."""
    out = np.full((len(off) - 1, len(probs)), np.nan)
    for g in range(len(off) - 1):
        rows = s[int(off[g]):int(off[g + 1])]
        if rows.shape[0]:
            for j, k in enumerate(api.quantile_rank(probs, rows.shape[0])):
                out[g, j] = np.partition(rows, k)[k]
    return out


def _check_exact(b, p, kw, what):
    s = b.residuals(p.rot, p.tran, fields=("sq_norm",), **kw).sq_norm
    got = b.residual_quantiles(p.rot, p.tran, PROBS, **kw)
    want = _want(s, p.off, PROBS)
    assert got.shape == want.shape
    empty = np.diff(p.off.astype(np.int64)) == 0
    assert np.isnan(got[empty]).all()
    assert np.array_equal(_bits(got[~empty]), _bits(want[~empty])), what
    return s, got


@pytest.mark.parametrize("per_match", [False, True], ids=["uniform", "per_match"])
@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
@pytest.mark.parametrize("interleave", ["0", "1"], ids=["contiguous", "interleaved"])
def test_ragged_pairs_equal_partition_and_the_pair_alone(monkeypatch, interleave, store, per_match):
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", interleave)
    p = Pairs(RAGGED, seed=1)
    kw = p.kw(per_match)
    with api.Batch(0) as b:
        b.upload(p.x1, p.x2, p.off, p.d12, store=store)
        s, got = _check_exact(b, p, kw, (interleave, store, per_match))
        again = b.residual_quantiles(p.rot, p.tran, PROBS, **kw)
        assert got.tobytes() == again.tobytes()
    # no dependence on the neighbours: each pair as a batch of its own, and as a single problem
    for g, n in enumerate(p.sizes):
        if n == 0:
            continue
        c = p.cs[g]
        one = dict(kw) if per_match else dict(d1=[p.d1[g]], d2=[p.d2[g]], depth_mode=api.DEPTH_UNIFORM)
        with api.Batch(0) as b1:
            b1.upload(c.x1, c.x2, np.array([0, n], dtype=np.uint64), c.d12, store=store)
            alone = b1.residual_quantiles(c.rot_init[None], c.tran_init[None], PROBS, **one)
        assert np.array_equal(_bits(alone[0]), _bits(got[g])), (g, n)


@pytest.mark.parametrize("shape", ["few_huge_pairs", "bpp3", "many_pairs"])
def test_blocks_per_pair_and_many_pairs(monkeypatch, shape):
    if shape == "few_huge_pairs":                      # several blocks per pair
        sizes = [200_001, 3, 150_000]
    elif shape == "bpp3":                              # forced blocks per pair: blocks loop past one stride step, some get nothing
        monkeypatch.setenv("SBA_BATCH_BPP", "3")
        sizes = [40_001, 0, 9_999, 1, 30_000, 700]
    else:
        sizes = [int(v) for v in np.random.default_rng(5).integers(0, 400, size=1500)]
    p = Pairs(sizes, seed=2)
    for per_match in (True, False):
        with api.Batch(0) as b:
            b.upload(p.x1, p.x2, p.off, p.d12)
            if shape != "many_pairs":
                assert b.blocks_per_pair > 1
            _check_exact(b, p, p.kw(per_match), (shape, per_match))
            # explicit ranks, every pair alike
            if min(sizes) >= 3:
                v = b.residual_order_stats(p.rot, p.tran, [0, 2], **p.kw(per_match))
                assert v.shape == (len(sizes), 2) and np.all(v[:, 0] <= v[:, 1])


def test_full_size_256_pairs_of_50000():
    c = synthetic.full_rt(50_000, outlier_fraction=0.1)
    B, n = 256, 50_000
    rng = np.random.default_rng(9)
    perm = [rng.permutation(n) for _ in range(B)]
    x1 = np.concatenate([c.x1[q] for q in perm])
    x2 = np.concatenate([c.x2[q] for q in perm])
    d12 = np.concatenate([c.d12[q] for q in perm]) * (1.0 + 1e-3 * np.repeat(np.arange(B), n))[:, None]
    off = (np.arange(B + 1) * n).astype(np.uint64)
    rot, tran = np.tile(c.rot_init, (B, 1)), np.tile(c.tran_init, (B, 1))
    kw = dict(depth_mode=api.DEPTH_PER_MATCH)
    with api.Batch(0) as b:
        b.upload(x1, x2, off, d12)
        s = b.residuals(rot, tran, fields=("sq_norm",), **kw).sq_norm
        got = b.residual_quantiles(rot, tran, PROBS, **kw)
        assert np.array_equal(_bits(got), _bits(_want(s, off, PROBS)))
        idx, new_off, thr = b.keep_below(rot, tran, 0.5, 3.0, **kw)
        assert np.array_equal(thr, 3.0 * got[:, 2])
        assert np.array_equal(idx, np.flatnonzero(s <= np.repeat(thr, n)))


def _outcome(fn):
    try:
        return ("ok", fn())
    except api.SbaError as e:
        return ("err", e.code)


def _eq(x, y):
    if isinstance(x, (tuple, list)):
        return len(x) == len(y) and all(_eq(a, c) for a, c in zip(x, y))
    if isinstance(x, api.SolveSummary):
        return (x.num_iterations, x.termination, x.final_cost) == (y.num_iterations, y.termination, y.final_cost)
    if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
        return np.array_equal(x, y)
    return x == y


def _same(b, q, what, fn):
    a, c = _outcome(lambda: fn(b)), _outcome(lambda: fn(q))
    assert a[0] == c[0] and _eq(a[1], c[1]), what


def _same_batch(b, q, p, keep):
    """b (after keep_below) and q (fresh upload of the kept rows): offsets, blocks per pair, packs, moments, an LM solve, a
    d-only stage and the sweep after it, bit for bit."""
    assert np.array_equal(b.offsets, q.offsets) and b.blocks_per_pair == q.blocks_per_pair
    for mode in (api.MODE_ROT, api.MODE_TRAN, api.MODE_RT):
        for dm in (api.DEPTH_UNIFORM, api.DEPTH_PER_MATCH):
            for delta in (1.0, 0.0):
                _same(b, q, ("pack", mode, dm, delta),
                      lambda h: h.eval(mode, p.rot, p.tran, p.d1, p.d2, huber_delta=delta, depth_mode=dm))
    _same(b, q, "epipolar moments", lambda h: h.epipolar_moments())
    _same(b, q, "solve", lambda h: h.solve(api.MODE_RT, p.rot, p.tran, depth_mode=api.DEPTH_PER_MATCH))
    _same(b, q, "solve_depths", lambda h: h.solve_depths(p.rot, p.tran))
    _same(b, q, "pack after solve_depths", lambda h: h.eval(api.MODE_RT, p.rot, p.tran, depth_mode=api.DEPTH_PER_MATCH))


@pytest.mark.parametrize("per_match", [False, True], ids=["uniform", "per_match"])
@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
@pytest.mark.parametrize("interleave", ["0", "1"], ids=["contiguous", "interleaved"])
def test_keep_below_equals_mask_and_fresh_upload(pinned_grid, monkeypatch, interleave, store, per_match):
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", interleave)
    p = Pairs([0, 1, 2, 300, 2049, 0, 9_000, 40_001], seed=3)
    B = len(p.sizes)
    kw = p.kw(per_match)
    prob = np.array([0.5, 0.5, 1.0, 0.25, 0.5, 0.5, 0.9, 0.5])
    scale = np.array([1.0, 1.0, 1.0, 4.0, 9.0, 2.0, 0.5, 6.0])
    with api.Batch(0) as b, api.Batch(0) as q:
        b.upload(p.x1, p.x2, p.off, p.d12, store=store)
        s = b.residuals(p.rot, p.tran, fields=("sq_norm",), **kw).sq_norm
        value = np.array([_want(s, p.off, [prob[g]])[g, 0] for g in range(B)])
        idx, off, thr = b.keep_below(p.rot, p.tran, prob, scale, **kw)
        empty = np.array(p.sizes) == 0
        assert np.isnan(thr[empty]).all() and np.array_equal(thr[~empty], (scale * value)[~empty])
        with np.errstate(invalid="ignore"):
            keep = s <= thr[p.pair]
        assert idx.dtype == np.int64 and np.array_equal(idx, np.flatnonzero(keep))
        n_kept = np.bincount(p.pair[keep], minlength=B)
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(n_kept)]).astype(np.uint64))
        assert np.all(n_kept[~empty] >= 1)                                   # the selected element itself stays when scale >= 1 ...
        q.upload(p.x1[keep], p.x2[keep], off, p.d12[keep], store=store)
        _same_batch(b, q, p, keep)


def test_ties_in_a_batch():
    base = synthetic.full_rt(700, seed=synthetic.BASE_SEED + 2600, outlier_fraction=0.1)
    rep = lambda a: np.repeat(a, 3, axis=0)
    one = lambda a: np.repeat(a[:1], 1001, axis=0)
    x1, x2, d12 = (np.concatenate([rep(a), one(a)]) for a in (base.x1, base.x2, base.d12))
    off = np.array([0, 2100, 3101], dtype=np.uint64)
    rot, tran = np.tile(base.rot_init, (2, 1)), np.tile(base.tran_init, (2, 1))
    kw = dict(depth_mode=api.DEPTH_PER_MATCH)
    with api.Batch(0) as b:
        b.upload(x1, x2, off, d12)
        s = b.residuals(rot, tran, fields=("sq_norm",), **kw).sq_norm
        got = b.residual_quantiles(rot, tran, PROBS, **kw)
        assert np.array_equal(_bits(got), _bits(_want(s, off, PROBS)))
        assert np.unique(s[2100:]).shape[0] == 1 and np.all(got[1] == s[2100])
        idx, new_off, thr = b.keep_below(rot, tran, 0.5, 1.0, **kw)
        keep = s <= np.repeat(thr, [2100, 1001])
        assert np.array_equal(idx, np.flatnonzero(keep)) and new_off[2] - new_off[1] == 1001
        cut = np.flatnonzero(s[:2100] == thr[0])
        assert cut.shape[0] >= 3 and np.all(np.isin(cut, idx))


def test_refusals_and_empty_batches():
    p = Pairs([10, 0, 5], seed=4)
    kw = dict(depth_mode=api.DEPTH_PER_MATCH)
    with api.Batch(0) as b:
        b.upload(p.x1, p.x2, p.off, p.d12)
        ranks = np.array([[9], [123], [4]])                                   # the empty pair's rank is not looked at
        v = b.residual_order_stats(p.rot, p.tran, ranks, **kw)
        assert np.isfinite(v[[0, 2]]).all() and np.isnan(v[1]).all()
        for bad in (np.array([[10], [0], [4]]), np.array([[0], [0], [5]])):
            with pytest.raises(api.SbaError) as ei:
                b.residual_order_stats(p.rot, p.tran, bad, **kw)
            assert ei.value.code == cabi.SBA_ERR_INVALID_ARG and "rank" in ei.value.message
        with pytest.raises(api.SbaError) as ei:
            b.residual_order_stats(p.rot, p.tran, np.zeros((3, 9), dtype=int), **kw)
        assert ei.value.code == cabi.SBA_ERR_INVALID_ARG
        for bad in (-1.0, np.inf, np.nan):
            with pytest.raises(api.SbaError) as ei:
                b.keep_below(p.rot, p.tran, 0.5, [1.0, bad, 1.0], **kw)
            assert ei.value.code == cabi.SBA_ERR_INVALID_ARG
        assert np.array_equal(b.offsets, p.off)
    e = Pairs([0, 0], seed=5)
    with api.Batch(0) as b:
        b.upload(e.x1, e.x2, e.off, e.d12)
        assert np.isnan(b.residual_quantiles(e.rot, e.tran, PROBS, **kw)).all()
        idx, off, thr = b.keep_below(e.rot, e.tran, 0.5, 2.0, **kw)
        assert idx.shape == (0,) and np.array_equal(off, [0, 0, 0]) and np.isnan(thr).all()
