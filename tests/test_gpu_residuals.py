"""GPU: per-match residuals (Problem.residuals, sba_problem_residuals) and compaction of a problem's matches
(Problem.compact / keep_inliers, sba_problem_compact).

Residuals are checked against an independent long-double restatement and the oracle, and against the sweep itself: the
inlier count is n - n_outlier of the pack and 1/2 sum rho(sq_norm) is its cost.  A compacted handle must be what a fresh
upload of the kept matches is: same size, and bit-identical packs, solves, d-only stages and epipolar moments."""
import numpy as np
import pytest

from ref_numpy import rotmat
from spherical_bundle_adjuster_amd import api, synthetic

pytestmark = pytest.mark.gpu

MODES = (api.MODE_ROT, api.MODE_TRAN, api.MODE_RT)
KINDS = (api.KERNEL_FACTORED, api.KERNEL_EXPLICIT)
STORES = (api.STORE_F64, api.STORE_F32)
DELTAS = (1.0, 0.05, 0.0)
TILE = 2048              # matches per scan tile of the compaction (sba_device.hpp kCompactTile)
BLOCK = 256              # threads per residual block (sba_device.hpp kBlock)


@pytest.fixture
def pinned_grid(monkeypatch):
    """Same blocks per CU for every sweep variant (read at handle creation): a compacted and a fresh handle then reduce in
    the same order and their packs compare bit for bit."""
    monkeypatch.setenv("SBA_BLOCKS_PER_CU", "2")


def _case(n, per_match, seed=0):
    if per_match:
        return synthetic.full_rt(n, seed=synthetic.BASE_SEED + 40 + seed, outlier_fraction=0.1)
    return synthetic.rotation_only(n, seed=synthetic.BASE_SEED + 50 + seed, outlier_fraction=0.1)


def _planes(c, store):
    """What the planes hold: f32 planes are the f32-rounded inputs."""
    if store == api.STORE_F64:
        return c.x1, c.x2
    return c.x1.astype(np.float32).astype(np.float64), c.x2.astype(np.float32).astype(np.float64)


def _reference(x1, x2, rot, tran, d1, d2):
    """e = d2 x2 - (R (d1 x1) - t) in long double; d1, d2 scalars or (n,) arrays."""
    R = rotmat(rot).astype(np.longdouble)
    X1 = x1.astype(np.longdouble) * np.asarray(d1, dtype=np.longdouble).reshape(-1, 1)
    X2 = x2.astype(np.longdouble) * np.asarray(d2, dtype=np.longdouble).reshape(-1, 1)
    return X2 - (X1 @ R.T - np.asarray(tran, dtype=np.longdouble))


def _rho(s, delta):
    if delta <= 0.0:
        return s
    return np.where(s > delta * delta, 2.0 * delta * np.sqrt(s) - delta * delta, s)


def _args(c, per_match):
    """(d1, d2, depth_mode) of the residual / sweep calls and the per-match depths of the reference."""
    if per_match:
        return 1.0, 1.0, api.DEPTH_PER_MATCH, c.d12[:, 0], c.d12[:, 1]
    return 1.3, 0.8, api.DEPTH_UNIFORM, 1.3, 0.8


def _check_against_sweep(p, n, rot, tran, d1, d2, dm, delta, r):
    for kind in KINDS:
        p.set_kernel(kind)
        for mode in MODES:
            pack = p.eval_pack(mode, rot, tran, d1, d2, huber_delta=delta, depth_mode=dm)
            assert r.n_inlier == n - pack[23], (kind, mode, delta, r.n_inlier, n, pack[23])
            cost = 0.5 * float(np.sum(_rho(r.sq_norm.astype(np.longdouble), delta)))
            assert abs(cost - pack[22]) <= 1e-12 * max(abs(cost), 1e-300), (kind, mode, delta, cost, pack[22])
    p.set_kernel(api.KERNEL_FACTORED)


@pytest.mark.parametrize("per_match", [False, True], ids=["uniform", "per_match"])
@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [0, 1, 7, 2049, 1_000_003])
def test_residuals_match_restatement_and_sweep(oracle, n, store, per_match):
    c = _case(n, per_match)
    x1, x2 = _planes(c, store)
    d1, d2, dm, rd1, rd2 = _args(c, per_match)
    rot, tran = c.rot_init, c.tran_init
    ref = _reference(x1, x2, rot, tran, rd1, rd2)
    scale = np.maximum(1.0, np.asarray(rd1) + np.asarray(rd2) + np.linalg.norm(tran))
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12 if per_match else None, store=store)
        for delta in DELTAS:
            r = p.residuals(rot, tran, d1, d2, huber_delta=delta, depth_mode=dm)
            assert r.e.shape == (n, 3) and r.sq_norm.shape == (n,) and r.inlier.shape == (n,) and r.inlier.dtype == bool
            if n == 0:
                assert r.n_inlier == 0
                continue
            err = np.abs((r.e.astype(np.longdouble) - ref)).max(axis=1) / scale
            assert float(err.max()) <= 1e-12, (delta, float(err.max()))
            # sq_norm and inlier as the returned e implies
            s_ref = np.sum(r.e.astype(np.longdouble) ** 2, axis=1)
            assert np.all(np.abs(r.sq_norm - s_ref) <= 1e-15 * s_ref)
            want = np.ones(n, bool) if delta <= 0.0 else ~(r.sq_norm > delta * delta)
            assert np.array_equal(r.inlier, want)
            assert r.n_inlier == int(np.count_nonzero(r.inlier))
            # a sample against the oracle's own residual
            for i in np.unique(np.linspace(0, n - 1, 9).astype(int)):
                e_o, _ = oracle.point(api.MODE_RT, x1[i], x2[i], rot, tran,
                                      float(np.asarray(rd1).reshape(-1)[i if per_match else 0]),
                                      float(np.asarray(rd2).reshape(-1)[i if per_match else 0]))
                assert np.abs(r.e[i] - e_o).max() <= 1e-12 * scale.reshape(-1)[i if per_match else 0], (i, r.e[i], e_o)
            # count-only call and partial outputs agree with the full one
            only = p.residuals(rot, tran, d1, d2, huber_delta=delta, depth_mode=dm, fields=())
            assert only.e is None and only.inlier is None and only.n_inlier == r.n_inlier
            part = p.residuals(rot, tran, d1, d2, huber_delta=delta, depth_mode=dm, fields=("inlier",))
            assert np.array_equal(part.inlier, r.inlier) and part.e is None and part.sq_norm is None
            _check_against_sweep(p, n, rot, tran, d1, d2, dm, delta, r)


@pytest.mark.parametrize("n", [7, 2049, 1_000_003])
def test_residuals_folded_equal_raw(n):
    c = _case(n, True, seed=1)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12)
        folded = [p.residuals(c.rot_init, c.tran_init, huber_delta=d, depth_mode=api.DEPTH_PER_MATCH) for d in DELTAS]
        p.set_folding(False)
        raw = [p.residuals(c.rot_init, c.tran_init, huber_delta=d, depth_mode=api.DEPTH_PER_MATCH) for d in DELTAS]
    for a, b in zip(folded, raw):
        assert np.array_equal(a.e, b.e) and np.array_equal(a.sq_norm, b.sq_norm)
        assert np.array_equal(a.inlier, b.inlier) and a.n_inlier == b.n_inlier


def _device_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
def test_residuals_grid_stride_past_one_step(monkeypatch, store):
    """One block per CU: the residual kernel's lanes run three steps and a bit (plus the ragged vector)."""
    monkeypatch.setenv("SBA_BLOCKS_PER_CU", "1")
    ppt = 2 if store == api.STORE_F64 else 4
    stride = _device_cus() * BLOCK
    n = (3 * stride + 5) * ppt + 1
    c = _case(n, True, seed=2)
    x1, x2 = _planes(c, store)
    ref = _reference(x1, x2, c.rot_init, c.tran_init, c.d12[:, 0], c.d12[:, 1])
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12, store=store)
        for dm in (api.DEPTH_PER_MATCH, api.DEPTH_UNIFORM):
            d1, d2 = (1.0, 1.0) if dm == api.DEPTH_PER_MATCH else (1.3, 0.8)
            r = p.residuals(c.rot_init, c.tran_init, d1, d2, huber_delta=1.0, depth_mode=dm)
            if dm == api.DEPTH_PER_MATCH:
                scale = 1.0 + c.d12.sum(axis=1) + np.linalg.norm(c.tran_init)
                assert float((np.abs(r.e.astype(np.longdouble) - ref).max(axis=1) / scale).max()) <= 1e-12
            _check_against_sweep(p, n, c.rot_init, c.tran_init, d1, d2, dm, 1.0, r)


# ---- compaction -----------------------------------------------------------------------------------------------------
def _masks(n, seed=0):
    rng = np.random.default_rng(seed)
    idx = np.arange(n)
    m = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "first": idx == 0, "last": idx == n - 1,
         "alternating": idx % 2 == 0,
         # runs of 1000 kept / 1000 dropped: run ends fall inside tiles and runs cross tile boundaries
         "runs": (idx // 1000) % 2 == 0,
         # the matches either side of every tile boundary
         "tile_edges": (idx % TILE == 0) | (idx % TILE == TILE - 1)}
    for pct in (5, 50, 95):
        m[f"rand{pct}"] = rng.random(n) < pct / 100.0
    return m


def _outcome(fn):
    try:
        return ("ok", fn())
    except api.SbaError as e:
        return ("err", e.code)


def _same(a, b, what):
    assert a[0] == b[0], (what, a, b)
    if a[0] == "err":
        assert a[1] == b[1], what
        return
    va, vb = a[1], b[1]
    if isinstance(va, tuple):
        for x, y in zip(va, vb):
            if isinstance(x, np.ndarray):
                assert np.array_equal(x, y), what
            elif isinstance(x, api.SolveSummary):
                assert (x.num_iterations, x.termination, x.final_cost) == (y.num_iterations, y.termination, y.final_cost), what
            else:
                assert x == y, what
    else:
        assert np.array_equal(va, vb), what


def _assert_equivalent(p, q, c, has_d, deep):
    """p (compacted) and q (fresh upload of the kept matches) give the same bits."""
    assert p.size == q.size
    dms = (api.DEPTH_UNIFORM, api.DEPTH_PER_MATCH) if has_d else (api.DEPTH_UNIFORM,)
    for kind in KINDS:
        p.set_kernel(kind)
        q.set_kernel(kind)
        for mode in MODES:
            for dm in dms:
                for delta in (1.0, 0.0):
                    f = lambda h: h.eval_pack(mode, c.rot_init, c.tran_init, 1.2, 0.9, huber_delta=delta, depth_mode=dm)
                    _same(_outcome(lambda: f(p)), _outcome(lambda: f(q)), ("pack", kind, mode, dm, delta))
    p.set_kernel(api.KERNEL_FACTORED)
    q.set_kernel(api.KERNEL_FACTORED)
    if p.size > 0:
        _same(_outcome(p.epipolar_moments), _outcome(q.epipolar_moments), "epipolar moments")
    if not deep or p.size < 8:
        return
    for dm in dms:
        f = lambda h: h.solve(api.MODE_RT, c.rot_init, c.tran_init, depth_mode=dm)
        _same(_outcome(lambda: f(p)), _outcome(lambda: f(q)), ("solve", dm))
    if has_d:
        f = lambda h: h.solve_depths(c.rot_init, c.tran_init)
        _same(_outcome(lambda: f(p)), _outcome(lambda: f(q)), "solve_depths")
        # ... and the sweeps after the d-only stage (refolded planes)
        f = lambda h: h.eval_pack(api.MODE_RT, c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH)
        _same(_outcome(lambda: f(p)), _outcome(lambda: f(q)), "pack after solve_depths")


@pytest.mark.parametrize("has_d", [False, True], ids=["no_depths", "depths"])
@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 7, 2049, 1_000_003])
def test_compact_equals_fresh_upload(pinned_grid, n, store, has_d):
    c = _case(n, True, seed=3)
    d = c.d12 if has_d else None
    for name, keep in _masks(n).items():
        with api.Problem(0) as p, api.Problem(0) as q:
            p.upload(c.x1, c.x2, d, store=store)
            idx = p.compact(keep)
            assert idx.dtype == np.int64 and np.array_equal(idx, np.flatnonzero(keep)), name
            q.upload(c.x1[keep], c.x2[keep], None if d is None else d[keep], store=store)
            _assert_equivalent(p, q, c, has_d, deep=name == "rand50")


@pytest.mark.parametrize("n", [2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 1])
def test_compact_at_tile_multiples(pinned_grid, n):
    c = _case(n, True, seed=4)
    for name in ("runs", "tile_edges", "last", "rand50"):
        keep = _masks(n, seed=n)[name]
        with api.Problem(0) as p, api.Problem(0) as q:
            p.upload(c.x1, c.x2, c.d12)
            assert np.array_equal(p.compact(keep), np.flatnonzero(keep)), name
            q.upload(c.x1[keep], c.x2[keep], c.d12[keep])
            _assert_equivalent(p, q, c, True, deep=False)


@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
def test_two_compactions_compose(pinned_grid, store):
    n = 100_003
    c = _case(n, True, seed=5)
    rng = np.random.default_rng(9)
    k1 = rng.random(n) < 0.7
    with api.Problem(0) as p, api.Problem(0) as q:
        p.upload(c.x1, c.x2, c.d12, store=store)
        i1 = p.compact(k1)
        k2 = rng.random(i1.size) < 0.6
        i2 = p.compact(k2)
        kept = i1[i2]
        assert np.array_equal(kept, np.flatnonzero(k1)[np.flatnonzero(k2)])
        q.upload(c.x1[kept], c.x2[kept], c.d12[kept], store=store)
        _assert_equivalent(p, q, c, True, deep=True)


def test_compact_after_solve_depths(pinned_grid):
    """The d-only stage leaves the folded planes stale; compaction carries the refined depths and refolds."""
    n = 50_001
    c = _case(n, True, seed=6)
    keep = np.random.default_rng(3).random(n) < 0.5
    with api.Problem(0) as p, api.Problem(0) as q:
        p.upload(c.x1, c.x2, c.d12)
        d_new, _ = p.solve_depths(c.rot_init, c.tran_init)
        p.compact(keep)
        q.upload(c.x1[keep], c.x2[keep], d_new[keep])
        _assert_equivalent(p, q, c, True, deep=True)


@pytest.mark.parametrize("per_match", [False, True], ids=["uniform", "per_match"])
def test_keep_inliers_round_trip(per_match):
    n = 200_001
    c = _case(n, per_match, seed=7)
    d1, d2, dm, _, _ = _args(c, per_match)
    for delta in (1.0, 0.05):
        with api.Problem(0) as p:
            p.upload(c.x1, c.x2, c.d12 if per_match else None)
            before = p.residuals(c.rot_init, c.tran_init, d1, d2, huber_delta=delta, depth_mode=dm)
            idx = p.keep_inliers(c.rot_init, c.tran_init, d1, d2, huber_delta=delta, depth_mode=dm)
            assert np.array_equal(idx, np.flatnonzero(before.inlier))
            assert p.size == before.n_inlier < n
            after = p.residuals(c.rot_init, c.tran_init, d1, d2, huber_delta=delta, depth_mode=dm)
            assert after.n_inlier == p.size and bool(np.all(after.inlier))
            assert np.array_equal(after.e, before.e[idx])


def test_errors_leave_the_handle_usable():
    c = _case(1001, True, seed=8)
    with api.Problem(0) as p:
        with pytest.raises(api.SbaError) as ei:           # never uploaded
            p.residuals(c.rot_init, c.tran_init)
        assert ei.value.code == api.cabi.SBA_ERR_NOT_UPLOADED
        with pytest.raises(api.SbaError):
            p.compact(np.ones(0, bool))
        p.upload(c.x1, c.x2)                              # no depths
        with pytest.raises(api.SbaError):
            p.residuals(c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH)
        with pytest.raises(ValueError):
            p.compact(np.ones(1000, bool))
        with pytest.raises(ValueError):
            p.residuals(c.rot_init, c.tran_init, fields=("e", "bogus"))
        keep = np.arange(1001) % 3 != 0
        p.compact(keep)
        assert p.size == int(keep.sum())
        with pytest.raises(ValueError):                   # d12 of the old size
            p.set_depths(c.d12)
        p.set_depths(c.d12[keep])
        r = p.residuals(c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH)
        assert r.n_inlier > 0 and r.e.shape == (p.size, 3)
        p.compact(np.zeros(p.size, bool))                 # an empty, still uploaded problem
        assert p.size == 0
        assert p.residuals(c.rot_init, c.tran_init).n_inlier == 0
        assert p.compact(np.zeros(0, bool)).size == 0
