"""GPU: per-match residuals of a batch (Batch.residuals, sba_batch_residuals) and compaction of every pair's matches
(Batch.compact / keep_inliers, sba_batch_compact / sba_batch_keep_inliers).

Residuals are checked pair by pair against an independent long-double restatement and against the batched sweep: every
pair's inlier count is n - n_outlier of its pack, on the one-launch step and on the several-blocks-per-pair chain.  A
compacted batch must be what a fresh upload of the kept rows is: same offsets, blocks per pair and layout, and bit-identical
packs, solves, d-only stages, moments, guesses and pipelines."""
import numpy as np
import pytest

from ref_numpy import rotmat
from spherical_bundle_adjuster_amd import api, synthetic

pytestmark = pytest.mark.gpu

MODES = (api.MODE_ROT, api.MODE_TRAN, api.MODE_RT)
KINDS = (api.KERNEL_FACTORED, api.KERNEL_EXPLICIT)
STORES = (api.STORE_F64, api.STORE_F32)
DELTAS = (1.0, 0.05, 0.0)
NOUT = 23                # SBA_PACK_NOUT
TILE = 2048              # rows per scan tile of the compaction (sba_device.hpp kCompactTile)


@pytest.fixture
def pinned_grid(monkeypatch):
    """Same grids for every handle (read at creation / upload): a compacted and a fresh batch reduce in the same order."""
    monkeypatch.setenv("SBA_BLOCKS_PER_CU", "2")


class Pairs:
    def __init__(self, sizes, seed=0):
        self.sizes = list(sizes)
        cs = [synthetic.full_rt(n, seed=synthetic.BASE_SEED + 1300 + 37 * seed + g, outlier_fraction=0.1)
              for g, n in enumerate(self.sizes)]
        B = len(cs)
        self.off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.uint64)
        cat = lambda f, w: np.concatenate([f(c) for c in cs]) if sum(self.sizes) else np.zeros((0, w))
        self.x1, self.x2, self.d12 = cat(lambda c: c.x1, 3), cat(lambda c: c.x2, 3), cat(lambda c: c.d12, 2)
        self.rot = np.stack([c.rot_init for c in cs]) if B else np.zeros((0, 3))
        self.tran = np.stack([c.tran_init for c in cs]) if B else np.zeros((0, 3))
        self.d1 = 1.0 + 0.1 * (np.arange(B) % 5)          # per-pair uniform depths
        self.d2 = 0.7 + 0.05 * (np.arange(B) % 7)
        self.pair = np.repeat(np.arange(B), self.sizes)   # pair of every row

    def upload(self, b, keep=None, d12=None, store=api.STORE_F64, has_d=True):
        """Upload (the kept rows of) the pairs, offsets from 0."""
        d = self.d12 if d12 is None else d12
        if keep is None:
            b.upload(self.x1, self.x2, self.off, d if has_d else None, store=store)
            return
        n_kept = np.bincount(self.pair[keep], minlength=len(self.sizes))
        off = np.concatenate([[0], np.cumsum(n_kept)]).astype(np.uint64)
        b.upload(self.x1[keep], self.x2[keep], off, d[keep] if has_d else None, store=store)


def _depth_args(p, per_match):
    return (None, None, api.DEPTH_PER_MATCH) if per_match else (p.d1, p.d2, api.DEPTH_UNIFORM)


def _reference(p, store, per_match):
    """e = d2 x2 - (R (d1 x1) - t) per row in long double, from what the planes hold (f32 planes: f32-rounded inputs)."""
    x1, x2 = p.x1, p.x2
    if store == api.STORE_F32:
        x1, x2 = x1.astype(np.float32).astype(np.float64), x2.astype(np.float32).astype(np.float64)
    out = np.zeros((x1.shape[0], 3), dtype=np.longdouble)
    scale = np.ones(x1.shape[0])
    for g in range(len(p.sizes)):
        s = slice(int(p.off[g]), int(p.off[g + 1]))
        d1 = p.d12[s, 0] if per_match else np.full(p.sizes[g], p.d1[g])
        d2 = p.d12[s, 1] if per_match else np.full(p.sizes[g], p.d2[g])
        R = rotmat(p.rot[g]).astype(np.longdouble)
        X1 = x1[s].astype(np.longdouble) * d1.astype(np.longdouble)[:, None]
        X2 = x2[s].astype(np.longdouble) * d2.astype(np.longdouble)[:, None]
        out[s] = X2 - (X1 @ R.T - p.tran[g].astype(np.longdouble))
        scale[s] = np.maximum(1.0, d1 + d2 + np.linalg.norm(p.tran[g]))
    return out, scale


def _check_counts_against_sweep(b, p, r, per_match, delta, kinds=KINDS, modes=MODES):
    d1, d2, dm = _depth_args(p, per_match)
    n = np.asarray(b.offsets[1:] - b.offsets[:-1], dtype=np.int64)
    for kind in kinds:
        b.set_kernel(kind)
        for mode in modes:
            packs = b.eval(mode, p.rot, p.tran, d1, d2, huber_delta=delta, depth_mode=dm)
            assert np.array_equal(n - r.n_inlier, packs[:, NOUT].astype(np.int64)), (kind, mode, delta)
    b.set_kernel(api.KERNEL_FACTORED)


SIZES = [5, 0, 1, 2, 7, 2049, 0, 300, 4099]


@pytest.mark.parametrize("per_match", [False, True], ids=["uniform", "per_match"])
@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
@pytest.mark.parametrize("interleave", ["0", "1"], ids=["contiguous", "interleaved"])
def test_residuals_match_restatement_pair_by_pair(monkeypatch, interleave, store, per_match):
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", interleave)
    p = Pairs(SIZES, seed=1)
    ref, scale = _reference(p, store, per_match)
    d1, d2, dm = _depth_args(p, per_match)
    rows = int(p.off[-1])
    with api.Batch(0) as b:
        p.upload(b, store=store)
        assert np.array_equal(b.offsets, p.off)
        split = False
        for delta in DELTAS:
            r = b.residuals(p.rot, p.tran, d1, d2, huber_delta=delta, depth_mode=dm)
            assert r.e.shape == (rows, 3) and r.sq_norm.shape == (rows,) and r.inlier.dtype == bool
            err = np.abs(r.e.astype(np.longdouble) - ref).max(axis=1) / scale
            assert float(err.max()) <= 1e-12, (delta, float(err.max()))
            s_ref = np.sum(r.e.astype(np.longdouble) ** 2, axis=1)
            assert np.all(np.abs(r.sq_norm - s_ref) <= 1e-15 * s_ref)
            want = np.ones(rows, bool) if delta <= 0.0 else ~(r.sq_norm > delta * delta)
            assert np.array_equal(r.inlier, want)
            assert np.array_equal(r.n_inlier, np.bincount(p.pair[r.inlier], minlength=len(SIZES)))
            split |= 0 < int(r.n_inlier.sum()) < rows
            only = b.residuals(p.rot, p.tran, d1, d2, huber_delta=delta, depth_mode=dm, fields=())
            assert only.e is None and only.inlier is None and np.array_equal(only.n_inlier, r.n_inlier)
            part = b.residuals(p.rot, p.tran, d1, d2, huber_delta=delta, depth_mode=dm, fields=("sq_norm",))
            assert np.array_equal(part.sq_norm, r.sq_norm) and part.e is None
            _check_counts_against_sweep(b, p, r, per_match, delta)
        assert split                                     # both sides of the threshold are exercised


@pytest.mark.parametrize("shape", ["many_pairs", "few_long_pairs", "bpp2", "bpp3", "bpp7"])
@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
def test_inlier_counts_equal_the_sweep_outlier_counts(monkeypatch, shape, store):
    rng = np.random.default_rng(5)
    if shape == "many_pairs":                          # >= one pair per CU: one block per pair, the one-launch step
        sizes = list(rng.integers(0, 3000, size=300))
    elif shape == "few_long_pairs":                    # several blocks per pair, the three-kernel chain
        sizes = [200_001, 3, 150_000]
    else:                                              # forced blocks per pair: each block loops past one grid-stride step
        monkeypatch.setenv("SBA_BATCH_BPP", shape[3:])
        sizes = [40_001, 0, 9_999, 1, 30_000]
    p = Pairs(sizes, seed=2)
    with api.Batch(0) as b:
        p.upload(b, store=store)
        if shape == "many_pairs":
            assert b.blocks_per_pair == 1 and b.step_is_fused
        elif shape == "few_long_pairs":
            assert b.blocks_per_pair > 1 and not b.step_is_fused
        else:
            assert b.blocks_per_pair == int(shape[3:])
        for per_match in (False, True):
            d1, d2, dm = _depth_args(p, per_match)
            for delta in DELTAS:
                r = b.residuals(p.rot, p.tran, d1, d2, huber_delta=delta, depth_mode=dm, fields=("inlier",))
                assert np.array_equal(r.n_inlier, np.bincount(p.pair[r.inlier], minlength=len(sizes)))
                _check_counts_against_sweep(b, p, r, per_match, delta, kinds=(api.KERNEL_FACTORED,),
                                            modes=(api.MODE_RT,))
        if shape == "many_pairs":                      # ... and the three-kernel chain on the same batch
            monkeypatch.setenv("SBA_BATCH_FUSED_STEP", "0")
            assert not b.step_is_fused
            r = b.residuals(p.rot, p.tran, None, None, huber_delta=0.05, depth_mode=api.DEPTH_PER_MATCH, fields=())
            _check_counts_against_sweep(b, p, r, True, 0.05)


# ---- compaction --------------------------------------------------------------------------------------------------------
def _outcome(fn):
    try:
        return ("ok", fn())
    except api.SbaError as e:
        return ("err", e.code)


def _eq(x, y):
    if isinstance(x, dict):
        return x.keys() == y.keys() and all(_eq(x[k], y[k]) for k in x if k != "seconds_inside_the_library")
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


def _assert_equivalent(b, q, p, has_d, deep):
    """b (compacted) and q (fresh upload of the kept rows) give the same bits."""
    assert np.array_equal(b.offsets, q.offsets) and b.num_pairs == q.num_pairs
    assert b.blocks_per_pair == q.blocks_per_pair and b.step_is_fused == q.step_is_fused
    dms = (api.DEPTH_UNIFORM, api.DEPTH_PER_MATCH) if has_d else (api.DEPTH_UNIFORM,)
    for kind in KINDS:
        b.set_kernel(kind)
        q.set_kernel(kind)
        for mode in MODES:
            for dm in dms:
                for delta in (1.0, 0.0):
                    _same(b, q, ("pack", kind, mode, dm, delta),
                          lambda h: h.eval(mode, p.rot, p.tran, p.d1, p.d2, huber_delta=delta, depth_mode=dm))
    b.set_kernel(api.KERNEL_FACTORED)
    q.set_kernel(api.KERNEL_FACTORED)
    r = lambda h: h.residuals(p.rot, p.tran, p.d1, p.d2, huber_delta=0.05)
    _same(b, q, "residuals", r)
    if not deep:
        return
    _same(b, q, "epipolar moments", lambda h: h.epipolar_moments())
    _same(b, q, "initial guess", lambda h: h.initial_guess(check=False))
    for dm in dms:
        _same(b, q, ("solve", dm), lambda h: h.solve(api.MODE_RT, p.rot, p.tran, p.d1 if dm == 0 else None,
                                                     p.d2 if dm == 0 else None, depth_mode=dm))
    if has_d:
        _same(b, q, "solve_depths", lambda h: h.solve_depths(p.rot, p.tran))
        _same(b, q, "pack after solve_depths",
              lambda h: h.eval(api.MODE_RT, p.rot, p.tran, depth_mode=api.DEPTH_PER_MATCH))
        _same(b, q, "solve_problem", lambda h: h.solve_problem(p.rot, p.tran, want_depths=True, check=False))


def _masks(p, seed=0):
    rng = np.random.default_rng(seed)
    rows = int(p.off[-1])
    idx = np.arange(rows)
    local = idx - p.off[p.pair].astype(np.int64)
    m = {"all": np.ones(rows, bool), "none": np.zeros(rows, bool), "rand50": rng.random(rows) < 0.5,
         "pairs_emptied": (p.pair % 3) != 1,
         # rows either side of every compaction tile boundary, and every pair's first and last rows
         "tile_edges": (idx % TILE == 0) | (idx % TILE == TILE - 1) | (idx % TILE == 1),
         "pair_ends": (local == 0) | (local == np.asarray(p.sizes)[p.pair] - 1)}
    return m


@pytest.mark.parametrize("has_d", [False, True], ids=["no_depths", "depths"])
@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
@pytest.mark.parametrize("sizes", [SIZES + [2 * TILE - 1, 2 * TILE, 2 * TILE + 1],
                                   [4000, 4000, 3990, 4001],       # interleaved
                                   [20_000, 20_001, 0, 19_999]],   # few long pairs: several blocks each
                         ids=["ragged", "even", "long"])
def test_compact_equals_fresh_upload(pinned_grid, sizes, store, has_d):
    p = Pairs(sizes, seed=3)
    for name, keep in _masks(p).items():
        with api.Batch(0) as b, api.Batch(0) as q:
            p.upload(b, store=store, has_d=has_d)
            idx, off = b.compact(keep)
            assert idx.dtype == np.int64 and np.array_equal(idx, np.flatnonzero(keep)), name
            n_kept = np.bincount(p.pair[keep], minlength=len(sizes))
            assert np.array_equal(off, np.concatenate([[0], np.cumsum(n_kept)])), name
            p.upload(q, keep, store=store, has_d=has_d)
            _assert_equivalent(b, q, p, has_d, deep=name == "rand50")


def test_compact_changes_layout_and_blocks_per_pair(pinned_grid):
    """Masks that flip the interleave decision and that change the blocks per pair: the handle follows, as an upload."""
    p = Pairs([4000, 4000, 4000, 4000], seed=4)
    shrink = ~((p.pair > 0) & (np.arange(int(p.off[-1])) - p.off[p.pair].astype(np.int64) >= 1000))
    changed = []
    for keep in (shrink, np.random.default_rng(1).random(int(p.off[-1])) < 0.5):
        with api.Batch(0) as b, api.Batch(0) as q:
            p.upload(b)
            bpp0 = b.blocks_per_pair
            b.compact(keep)
            p.upload(q, keep)
            _assert_equivalent(b, q, p, True, deep=False)
            changed.append(b.blocks_per_pair != bpp0)
    assert changed[1]                         # 50 % of each pair: half the vectors, fewer blocks per pair


def test_two_compactions_compose(pinned_grid):
    p = Pairs([30_001, 0, 17, 25_000, 2048], seed=5)
    rng = np.random.default_rng(9)
    k1 = rng.random(int(p.off[-1])) < 0.7
    with api.Batch(0) as b, api.Batch(0) as q:
        p.upload(b)
        i1, _ = b.compact(k1)
        k2 = rng.random(i1.size) < 0.6
        i2, off = b.compact(k2)
        kept = np.zeros(int(p.off[-1]), bool)
        kept[i1[i2]] = True
        assert np.array_equal(i1[i2], np.flatnonzero(k1)[np.flatnonzero(k2)])
        p.upload(q, kept)
        assert np.array_equal(off, q.offsets)
        _assert_equivalent(b, q, p, True, deep=True)


def test_compact_after_solve_depths_carries_the_refined_depths(pinned_grid):
    p = Pairs([20_001, 5, 0, 12_000], seed=6)
    keep = np.random.default_rng(3).random(int(p.off[-1])) < 0.5
    with api.Batch(0) as b, api.Batch(0) as q:
        p.upload(b)
        d_new, _, _ = b.solve_depths(p.rot, p.tran)
        assert not np.array_equal(d_new, p.d12)
        b.compact(keep)
        p.upload(q, keep, d12=d_new)
        _assert_equivalent(b, q, p, True, deep=True)
        d12 = b.solve_depths(p.rot, p.tran)[0]            # d12_out indexed by the new rows
        assert d12.shape == (int(keep.sum()), 2)


@pytest.mark.parametrize("per_match", [False, True], ids=["uniform", "per_match"])
@pytest.mark.parametrize("sizes", [[50_001, 0, 3, 20_000], list(np.random.default_rng(2).integers(0, 2000, size=300))],
                         ids=["few", "many"])
def test_keep_inliers_equals_residuals_then_compact(pinned_grid, sizes, per_match):
    p = Pairs(sizes, seed=7)
    d1, d2, dm = _depth_args(p, per_match)
    for delta in (1.0, 0.05):
        with api.Batch(0) as b, api.Batch(0) as q:
            p.upload(b)
            p.upload(q)
            before = q.residuals(p.rot, p.tran, d1, d2, huber_delta=delta, depth_mode=dm)
            i_q, off_q = q.compact(before.inlier)
            i_b, off_b = b.keep_inliers(p.rot, p.tran, d1, d2, huber_delta=delta, depth_mode=dm)
            assert np.array_equal(i_b, i_q) and np.array_equal(off_b, off_q)
            assert np.array_equal(np.diff(off_b.astype(np.int64)), before.n_inlier)
            assert int(off_b[-1]) < int(p.off[-1])
            after = b.residuals(p.rot, p.tran, d1, d2, huber_delta=delta, depth_mode=dm)
            assert bool(np.all(after.inlier)) and np.array_equal(after.n_inlier, before.n_inlier)
            assert np.array_equal(after.e, before.e[i_b])
            if per_match:
                _assert_equivalent(b, q, p, True, deep=False)


def test_errors_leave_the_handle_usable():
    p = Pairs([600, 0, 401], seed=8)
    rows = int(p.off[-1])
    lib = None
    with api.Batch(0) as b:
        lib = b._lib
        none = np.zeros((0, 3))
        with pytest.raises(api.SbaError) as ei:             # never uploaded
            b.residuals(none, none)
        assert ei.value.code == api.cabi.SBA_ERR_NOT_UPLOADED
        with pytest.raises(api.SbaError):
            b.compact(np.ones(0, bool))
        with pytest.raises(api.SbaError):
            b.keep_inliers(none, none)
        p.upload(b, has_d=False)                            # no depths
        with pytest.raises(api.SbaError):
            b.residuals(p.rot, p.tran, depth_mode=api.DEPTH_PER_MATCH)
        with pytest.raises(api.SbaError):
            b.keep_inliers(p.rot, p.tran, depth_mode=api.DEPTH_PER_MATCH)
        with pytest.raises(ValueError):
            b.compact(np.ones(rows - 1, bool))
        with pytest.raises(ValueError):
            b.residuals(p.rot, p.tran, fields=("e", "bogus"))
        keep = np.ones(rows, np.uint8)
        assert lib.sba_batch_compact(b._h, keep.ctypes.data_as(api.C.c_void_p), None, None) < 0     # NULL n_kept
        assert lib.sba_batch_compact(b._h, None, (api.C.c_size_t * 3)(), None) < 0                 # NULL keep, rows > 0
        assert lib.sba_batch_keep_inliers(b._h, 0, api._dptr(p.rot), api._dptr(p.tran), None, None, 1.0, None, None) < 0
        assert np.array_equal(b.offsets, p.off)            # nothing changed
        r = b.residuals(p.rot, p.tran, p.d1, p.d2)
        assert r.e.shape == (rows, 3)
        keep = np.arange(rows) % 3 != 0
        idx, off = b.compact(keep)
        assert int(off[-1]) == int(keep.sum()) == idx.size
        p.upload(b, has_d=True)                             # a new upload after a compaction
        assert np.array_equal(b.offsets, p.off)
        idx, off = b.compact(np.arange(rows) % 2 == 0)
        with pytest.raises(ValueError):                     # d12 of the old size
            b.set_depths(p.d12)
        b.set_depths(p.d12[idx])
        r = b.residuals(p.rot, p.tran, depth_mode=api.DEPTH_PER_MATCH)
        assert r.e.shape == (idx.size, 3) and int(r.n_inlier.sum()) > 0
        idx, off = b.compact(np.zeros(idx.size, bool))       # every pair empty, still uploaded
        assert idx.size == 0 and np.array_equal(off, np.zeros(4))
        r = b.residuals(p.rot, p.tran, p.d1, p.d2)
        assert r.e.shape == (0, 3) and np.array_equal(r.n_inlier, np.zeros(3))
        assert np.all(b.eval(api.MODE_RT, p.rot, p.tran)[:, NOUT] == 0)
        idx, off = b.keep_inliers(p.rot, p.tran)
        assert idx.size == 0 and np.array_equal(off, np.zeros(4))
    with api.Batch(0) as b:                                 # zero pairs
        b.upload(np.zeros((0, 3)), np.zeros((0, 3)), np.array([0], dtype=np.uint64))
        r = b.residuals(np.zeros((0, 3)), np.zeros((0, 3)))
        assert r.e.shape == (0, 3) and r.n_inlier.shape == (0,)
        idx, off = b.compact(np.zeros(0, bool))
        assert idx.size == 0 and np.array_equal(off, [0])
        idx, off = b.keep_inliers(np.zeros((0, 3)), np.zeros((0, 3)))
        assert idx.size == 0 and np.array_equal(off, [0])
        c = synthetic.rotation_only(100, seed=1)            # offsets not starting at 0; one empty pair
        b.upload(c.x1, c.x2, np.array([10, 10, 60, 100], dtype=np.uint64))
        r = b.residuals(np.zeros((3, 3)), np.zeros((3, 3)), huber_delta=0.0)
        assert r.e.shape == (90, 3) and np.array_equal(r.n_inlier, [0, 50, 40])
        idx, off = b.compact(np.arange(90) < 70)
        assert np.array_equal(idx, np.arange(70)) and np.array_equal(off, [0, 0, 50, 70])
