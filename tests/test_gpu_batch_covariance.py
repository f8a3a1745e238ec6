"""GPU: the batched joint covariance (Batch.covariance_joint / sba_batch_covariance_joint; kernel csrc/sba_batch_covariance.hip).

One batch of ten pairs of sizes 0 ... 4097 whose row offsets 0, 0, 1, 4, 9, 72, 136, 201, 458, 971 put the pairs of 3, 63, 257
and 4097 matches on odd rows (the shifted stores) and give every odd-sized pair a ragged last lane, on even and on odd rows;
4097 is eight strides of the block and one match more, and crosses the tiles of the interleaved layout.  References: the DENSE inverse of the whole normal matrix (tests/cov_reference.py)
up to 513 matches, the element-wise long-double Schur form of tests/test_gpu_covariance.py at 4097; then Problem.covariance_joint
on every pair alone, a batch of one, the other pair layout and the lock-step driver (SBA_BATCH_DEVICE_COV=0).

Bounds: those of tests/test_gpu_covariance.py --
    |Sigma_c - ref|_max      <= kappa * TOL * |ref|_max
    |Sigma_dd,i - ref_i|_max <= (2 kappa_i + kappa) * TOL * |ref_i|_max
with TOL = REL_TOL_F64 / REL_TOL_F32 and the scene conditions of cov_reference.kappa_limit asserted from the reference."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import ref_joint_numpy as rj
from cov_reference import check_against, dense_covariance, kappa_limit, sin2_parallax
from helpers import REL_TOL_F32, REL_TOL_F64
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api, synthetic
from test_gpu_covariance import schur_covariances

pytestmark = pytest.mark.gpu

STORES = (api.STORE_F64, api.STORE_F32)
LAYOUTS = ("0", "1")          # SBA_BATCH_INTERLEAVE
TOL = {api.STORE_F64: REL_TOL_F64, api.STORE_F32: REL_TOL_F32}
GAUGES = (api.TRAN_SPHERE, api.TRAN_FREE)
POINTS = ("init", "true")
SIZES = (0, 1, 3, 5, 63, 64, 65, 257, 513, 4097)
OFFSETS = (0, 0, 1, 4, 9, 72, 136, 201, 458, 971, 5068)
DIM = {api.TRAN_SPHERE: 5, api.TRAN_FREE: 6}
PLANTED = {64: (0, 63), 65: (0, 1, 64), 257: (0, 100, 256)}        # pair-local; each set holds 0 and the last match
both = pytest.mark.parametrize("layout", LAYOUTS, ids=["contiguous", "interleaved"])
stores = pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])


@lru_cache(maxsize=None)
def _scene(n):
    return synthetic.full_rt(n, seed=900 + n)


def _scenes():
    return [_scene(n) for n in SIZES]


def _planes(x1, x2, store):
    """What the planes hold: f32 planes are the f32-rounded inputs."""
    if store == api.STORE_F64:
        return x1, x2
    return x1.astype(np.float32).astype(np.float64), x2.astype(np.float32).astype(np.float64)


def _cat(cs, point="init"):
    off = np.concatenate([[0], np.cumsum([len(c.x1) for c in cs])]).astype(np.uint64)
    x1 = np.concatenate([c.x1 for c in cs]).reshape(-1, 3)
    x2 = np.concatenate([c.x2 for c in cs]).reshape(-1, 3)
    d12 = np.concatenate([c.d12 for c in cs]).reshape(-1, 2)
    rot = np.stack([c.rot_init if point == "init" else c.rot_true for c in cs])
    tran = np.stack([c.tran_init if point == "init" else c.tran_true for c in cs])
    return off, x1, x2, d12, rot, tran


def _opt(tran_param):
    return api.default_lm_options(tran_param=tran_param)


def _fails(n, tran_param):
    """Fewer used matches than the gauge's dimension -- and n = 5 with a free translation: 15 residuals, 16 parameters."""
    return n < DIM[tran_param] or (n == 5 and tran_param == api.TRAN_FREE)


@lru_cache(maxsize=None)
def _refs(n, store, point):
    """{tran_param: reference} of the pair of size n, computed once and left unchanged."""
    c = _scene(n)
    x1, x2 = _planes(c.x1, c.x2, store)
    rot, tran = (c.rot_init, c.tran_init) if point == "init" else (c.rot_true, c.tran_true)
    if n > 513:
        return schur_covariances(x1, x2, rot, tran, c.d12)
    return {tp: dense_covariance(x1, x2, rot, tran, c.d12, tp) for tp in GAUGES if not _fails(n, tp)}


def _assert_failed(r, g, n, tran_param, lo, hi):
    assert r.status[g] == cabi.SBA_ERR_NUMERIC, (g, n)
    assert np.isnan(r.cov[g]).all(), (g, n)
    if r.depth_cov is not None:
        assert np.isnan(r.depth_cov[lo:hi]).all(), (g, n)
    assert r.dim[g] == DIM[tran_param] and r.dof[g] == r.n_used[g] - r.dim[g]


def _same(a, b, what=""):
    """Two BatchJointCovariance: every output the same bytes."""
    for k in ("cov", "cost", "sum_w", "n_used", "n_degenerate", "dim", "dof", "status"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), (what, k)
    assert (a.depth_cov is None) == (b.depth_cov is None)
    if a.depth_cov is not None:
        assert a.depth_cov.tobytes() == b.depth_cov.tobytes(), (what, "depth_cov")


def test_the_batch_has_the_offsets_the_store_paths_need():
    """Every store path of the depth phase has a pair: first row even or odd, last lane whole or ragged."""
    off = _cat(_scenes())[0]
    assert tuple(int(v) for v in off) == OFFSETS
    paths = {(o % 2, n % 2) for n, o in zip(SIZES, OFFSETS) if n > 0}
    assert paths >= {(0, 0), (0, 1), (1, 1)}                     # 64 | 5, 65, 513 | 3, 63, 257, 4097 (whose inner lanes are (1, 0))
    assert [n for n, o in zip(SIZES, OFFSETS) if o % 2 == 1 and n > 0] == [3, 63, 257, 4097]
    assert sum(n % 2 for n in SIZES) == 8 and 4097 == 8 * 512 + 1


# ---- 1. the references ------------------------------------------------------------------------------------------------------
@both
@stores
def test_against_the_references(monkeypatch, store, layout):
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    cs = _scenes()
    worst = 0.0
    with api.Batch(0) as b:
        off, x1, x2, d12, _, _ = _cat(cs)
        b.upload(x1, x2, off, d12, store=store)
        for point in POINTS:
            _, _, _, _, rot, tran = _cat(cs, point)
            for tran_param in GAUGES:
                with pytest.raises(api.SbaError) as ei:          # pairs of 0, 1 and 3 matches have no covariance
                    b.covariance_joint(rot, tran, options=_opt(tran_param), depths=False)
                assert ei.value.code == cabi.SBA_ERR_NUMERIC
                r = b.covariance_joint(rot, tran, options=_opt(tran_param), check=False)
                assert r.cov.shape == (len(cs), 6, 6) and r.depth_cov.shape == (int(off[-1]), 3)
                compared = 0
                for g, n in enumerate(SIZES):                    # every pair shown to the GPU is compared or asserted to have failed
                    lo, hi = int(off[g]), int(off[g + 1])
                    assert (r.n_used[g], r.n_degenerate[g]) == (n, 0), (g, n)
                    if _fails(n, tran_param):
                        _assert_failed(r, g, n, tran_param, lo, hi)
                        compared += 1
                        continue
                    ref = _refs(n, store, point)[tran_param]
                    assert ref.kappa <= kappa_limit(n, tran_param), (n, ref.kappa)
                    assert r.status[g] == 0 and (r.dim[g], r.dof[g]) == (ref.m, n - ref.m)
                    rc_, rd_ = check_against(r.cov[g], r.depth_cov[lo:hi], ref, TOL[store],
                                             what=f"batch n={n} store={store} layout={layout} gauge={tran_param} {point}")
                    worst = max(worst, rc_, rd_)
                    assert abs(r.cost[g] - ref.cost) <= TOL[store] * ref.cost and abs(r.sum_w[g] - ref.sum_w) <= TOL[store] * ref.sum_w
                    assert np.array_equal(r.cov[g], r.cov[g].T)
                    pg = r.pair(g)
                    assert pg.cov.tobytes() == r.cov[g].tobytes() and pg.depth_cov.tobytes() == r.depth_cov[lo:hi].tobytes()
                    assert pg.sigma2 == r.sigma2[g] or (np.isnan(pg.sigma2) and np.isnan(r.sigma2[g]))
                    compared += 1
                assert compared == len(SIZES)
        # the default options are the sphere gauge
        d = b.covariance_joint(rot, tran, check=False)
        assert (d.dim == 5).all()
        _same(d, b.covariance_joint(rot, tran, options=_opt(api.TRAN_SPHERE), check=False))
    print(f"largest err / bound store={store} layout={layout}: {worst:.3g}")


# ---- 2. the single problem --------------------------------------------------------------------------------------------------
@both
@stores
def test_against_the_single_problem(monkeypatch, store, layout):
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    cs = _scenes()
    off, x1, x2, d12, rot, tran = _cat(cs)
    with api.Batch(0) as b:
        b.upload(x1, x2, off, d12, store=store)
        got = {tp: b.covariance_joint(rot, tran, options=_opt(tp), check=False) for tp in GAUGES}
    for g, (n, c) in enumerate(zip(SIZES, cs)):
        lo, hi = int(off[g]), int(off[g + 1])
        with api.Problem(0) as p:
            if n > 0:
                p.upload(c.x1, c.x2, c.d12, store=store)
            for tp in GAUGES:
                r = got[tp]
                if _fails(n, tp):
                    assert r.status[g] == cabi.SBA_ERR_NUMERIC
                    if n > 0:
                        with pytest.raises(api.SbaError) as ei:
                            p.covariance_joint(c.rot_init, c.tran_init, options=_opt(tp))
                        assert ei.value.code == cabi.SBA_ERR_NUMERIC
                    continue
                ref = _refs(n, store, "init")[tp]
                one = p.covariance_joint(c.rot_init, c.tran_init, options=_opt(tp))
                assert (r.n_used[g], r.n_degenerate[g], r.dim[g], r.dof[g]) == (one.n_used, one.n_degenerate, one.dim, one.dof)
                assert np.abs(r.cov[g] - one.cov).max() <= ref.kappa * TOL[store] * np.abs(one.cov).max(), (n, tp)
                err = np.abs(r.depth_cov[lo:hi] - one.depth_cov).max(axis=1)
                bound = (2.0 * ref.kappa_i + ref.kappa) * TOL[store] * np.abs(one.depth_cov).max(axis=1)
                print(f"single n={n} store={store} layout={layout} gauge={tp}: camera "
                      f"{np.abs(r.cov[g] - one.cov).max() / (ref.kappa * TOL[store] * np.abs(one.cov).max()):.3g}, depth {(err / bound).max():.3g} of the bound")
                assert (err <= bound).all(), (n, tp, float((err / bound).max()))
                assert abs(r.cost[g] - one.cost) <= TOL[store] * one.cost and abs(r.sum_w[g] - one.sum_w) <= TOL[store] * one.sum_w


# ---- 3. independence --------------------------------------------------------------------------------------------------------
def _raw_call(b, rot, tran, rows, pad, sentinel):
    """The C entry point with a sentinel-filled depth_cov of rows + pad rows."""
    lib = cabi.load_library()
    B = b.num_pairs
    out = (cabi.JointCov * B)()
    dd = np.full((rows + pad, 3), sentinel)
    st = np.full(B, -99, dtype=np.int32)
    r_, t_ = np.ascontiguousarray(rot, dtype=np.float64), np.ascontiguousarray(tran, dtype=np.float64)
    rc = lib.sba_batch_covariance_joint(b._h, r_.ctypes.data_as(cabi._dp), t_.ctypes.data_as(cabi._dp), None, 0.0, out,
                                        dd.ctypes.data_as(cabi._dp), st.ctypes.data_as(C.POINTER(C.c_int)))
    return rc, out, dd, st


@stores
def test_a_pair_does_not_depend_on_its_batch_or_layout(monkeypatch, store):
    cs = _scenes()
    off, x1, x2, d12, rot, tran = _cat(cs)
    total = int(off[-1])
    full = {}
    for layout in LAYOUTS:
        monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
        with api.Batch(0) as b:
            b.upload(x1, x2, off, d12, store=store)
            full[layout] = b.covariance_joint(rot, tran, check=False)
            if layout == "0":
                # every row is written by exactly one pair, nothing past the rows: the sentinel survives only behind them
                rc, out, dd, st = _raw_call(b, rot, tran, total, 7, -7.0)
                assert rc == cabi.SBA_ERR_NUMERIC and list(st) == list(full[layout].status)
                assert (dd[total:] == -7.0).all()
                assert not (dd[:total] == -7.0).any()
                assert dd[:total].tobytes() == full[layout].depth_cov.tobytes()
    _same(full["0"], full["1"], "layouts")
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", "0")
    r = full["0"]
    for g, (n, c) in enumerate(zip(SIZES, cs)):
        lo, hi = int(off[g]), int(off[g + 1])
        with api.Batch(0) as b:
            b.upload(c.x1, c.x2, np.array([0, n], dtype=np.uint64), c.d12, store=store)
            a = b.covariance_joint(c.rot_init[None], c.tran_init[None], check=False)
        assert a.status[0] == r.status[g], n
        assert a.cov[0].tobytes() == r.cov[g].tobytes() and a.depth_cov.tobytes() == r.depth_cov[lo:hi].tobytes(), n
        assert (a.cost[0], a.sum_w[0], a.n_used[0], a.n_degenerate[0], a.dim[0], a.dof[0]) == \
               (r.cost[g], r.sum_w[g], r.n_used[g], r.n_degenerate[g], r.dim[g], r.dof[g]), n
        if r.status[g] == 0:
            assert np.isfinite(r.depth_cov[lo:hi]).all() and (r.depth_cov[lo:hi, :2] > 0).all(), n


# ---- 4. the two drivers -----------------------------------------------------------------------------------------------------
@both
@stores
def test_one_launch_driver_equals_lock_step_driver_bitwise(monkeypatch, store, layout):
    """The lock-step driver runs the host's cov_finish between a reduce launch and a depth launch of the same kernel: equal
    bytes say that the device-compiled cov_finish is the host's."""
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    cs = _scenes()
    off, x1, x2, d12, _, _ = _cat(cs)
    got = {}
    for driver in ("0", "1"):
        monkeypatch.setenv("SBA_BATCH_DEVICE_COV", driver)
        with api.Batch(0) as b:
            b.upload(x1, x2, off, d12, store=store)
            for point in POINTS:
                _, _, _, _, rot, tran = _cat(cs, point)
                for tp in GAUGES:
                    got[driver, point, tp, True] = b.covariance_joint(rot, tran, options=_opt(tp), check=False)
                    got[driver, point, tp, False] = b.covariance_joint(rot, tran, options=_opt(tp), depths=False, check=False)
    for point in POINTS:
        for tp in GAUGES:
            for depths in (True, False):
                _same(got["0", point, tp, depths], got["1", point, tp, depths], (point, tp, depths))
            assert (got["1", point, tp, True].status == 0).sum() == sum(not _fails(n, tp) for n in SIZES)


# ---- 5. degeneracy ----------------------------------------------------------------------------------------------------------
@both
@stores
def test_degenerate_matches_are_left_out(monkeypatch, store, layout):
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    cs = _scenes()
    for point in POINTS:
        off, x1, x2, d12, rot, tran = _cat(cs, point)
        x1, x2 = x1.copy(), x2.copy()
        keep = np.ones(len(x1), dtype=bool)
        for g, n in enumerate(SIZES):
            if n in PLANTED:
                rows = int(off[g]) + np.array(PLANTED[n])
                if store == api.STORE_F32:
                    # parallel in what the planes hold: x1 a multiple of an f32 vector, x2 = R x1 rounded once more stays
                    # within 1e-7 of it -- sin^2 ~ 1e-14, far below the threshold
                    x1[rows] = x1[rows].astype(np.float32)
                x2[rows] = x1[rows] @ rj.rotation(rot[g]).T
                keep[rows] = False
        p1, p2 = _planes(x1, x2, store)
        with api.Batch(0) as b:
            b.upload(x1, x2, off, d12, store=store)
            r = b.covariance_joint(rot, tran, min_sin2_parallax=1e-9, check=False)
            none = b.covariance_joint(rot, tran, min_sin2_parallax=0.0, depths=False, check=False)
        for g, n in enumerate(SIZES):
            lo, hi = int(off[g]), int(off[g + 1])
            if n not in PLANTED:
                assert r.n_degenerate[g] == 0 and r.n_used[g] == n
                assert (r.status[g] != 0) == _fails(n, api.TRAN_SPHERE)
                continue
            planted, kp = np.array(PLANTED[n]), keep[lo:hi]
            sin2 = sin2_parallax(p1[lo:hi], p2[lo:hi], rot[g])
            assert (sin2[planted] < 1e-10).all()
            assert not ((sin2[kp] >= 1e-10) & (sin2[kp] <= 1e-8)).any() and (sin2[kp] > 1e-8).all()
            ref = dense_covariance(p1[lo:hi], p2[lo:hi], rot[g], tran[g], d12[lo:hi], api.TRAN_SPHERE, keep=kp)
            assert ref.kappa <= kappa_limit(n, api.TRAN_SPHERE)
            assert r.status[g] == 0
            assert (r.n_degenerate[g], r.n_used[g], r.dof[g]) == (len(planted), n - len(planted), n - len(planted) - 5)
            assert np.array_equal(r.depth_cov[lo:hi][planted], np.tile([np.inf, np.inf, 0.0], (len(planted), 1)))
            check_against(r.cov[g], r.depth_cov[lo:hi], ref, TOL[store], used=np.flatnonzero(kp),
                          what=f"planted n={n} store={store} layout={layout} {point}")
            assert abs(r.cost[g] - ref.cost) <= TOL[store] * ref.cost and abs(r.sum_w[g] - ref.sum_w) <= TOL[store] * ref.sum_w
            assert none.n_used[g] + none.n_degenerate[g] == n


# ---- 6. state ---------------------------------------------------------------------------------------------------------------
def _counts(s):
    return (s.termination, s.num_iterations, s.num_successful_steps, s.num_evaluations, s.initial_cost, s.final_cost, s.final_radius)


@both
@stores
def test_the_batch_is_left_alone(monkeypatch, store, layout):
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    cs = _scenes()
    off, x1, x2, d12, rot, tran = _cat(cs)
    with api.Batch(0) as b, api.Batch(0) as twin:
        b.upload(x1, x2, off, d12, store=store)
        twin.upload(x1, x2, off, d12, store=store)
        a = b.covariance_joint(rot, tran, check=False)
        _same(a, b.covariance_joint(rot, tran, check=False), "twice")
        nd = b.covariance_joint(rot, tran, depths=False, check=False)
        assert nd.depth_cov is None
        for k in ("cov", "cost", "sum_w", "n_used", "n_degenerate", "dim", "dof", "status"):
            assert getattr(nd, k).tobytes() == getattr(a, k).tobytes(), k
        # solve_joint after a covariance call == solve_joint on a twin without one
        u, v = b.solve_joint(rot, tran, check=False), twin.solve_joint(rot, tran, check=False)
        assert all(p.tobytes() == q.tobytes() for p, q in zip(u[:3], v[:3])) and u[4].tobytes() == v[4].tobytes()
        assert [_counts(s) for s in u[3]] == [_counts(s) for s in v[3]]
        # ... and so is the d-only stage, whose work planes the per-match rows passed through
        b.covariance_joint(u[0], u[1], check=False)
        du, dv = b.solve_depths(u[0], u[1]), twin.solve_depths(v[0], v[1])
        assert du[0].tobytes() == dv[0].tobytes() and du[2].tobytes() == dv[2].tobytes()
    # after keep_below the covariance is that of a fresh upload of the kept rows
    with api.Batch(0) as b, api.Batch(0) as fresh:
        b.upload(x1, x2, off, d12, store=store)
        b.covariance_joint(rot, tran, check=False)
        idx, noff, _ = b.keep_below(rot, tran, 0.9, 1.0, depth_mode=api.DEPTH_PER_MATCH)
        assert 0 < len(idx) < len(x1)
        fresh.upload(x1[idx], x2[idx], noff, d12[idx], store=store)
        _same(b.covariance_joint(rot, tran, check=False), fresh.covariance_joint(rot, tran, check=False), "kept rows")


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    cs = _scenes()
    off, x1, x2, d12, rot, tran = _cat(cs)
    lib = cabi.load_library()
    dp = lambda a: a.ctypes.data_as(cabi._dp)
    with api.Batch(0) as b:
        assert lib.sba_batch_covariance_joint(b._h, dp(rot), dp(tran), None, 0.0, (cabi.JointCov * len(cs))(), None, None) == cabi.SBA_ERR_NOT_UPLOADED
        with pytest.raises(api.SbaError) as ei:
            b.covariance_joint(np.zeros((0, 3)), np.zeros((0, 3)))
        assert ei.value.code == cabi.SBA_ERR_NOT_UPLOADED
        b.upload(x1, x2, off)                             # uniform depths: no per-match planes
        with pytest.raises(api.SbaError) as ei:
            b.covariance_joint(rot, tran)
        assert ei.value.code == cabi.SBA_ERR_UNSUPPORTED
        b.upload(x1, x2, off, d12)
        before = b.covariance_joint(rot, tran, check=False)
        valid = np.array([not _fails(n, api.TRAN_SPHERE) for n in SIZES])
        assert np.array_equal(before.status == 0, valid)
        for bad in (-1.0, float("nan")):
            with pytest.raises(api.SbaError) as ei:
                b.covariance_joint(rot, tran, min_sin2_parallax=bad)
            assert ei.value.code == cabi.SBA_ERR_INVALID_ARG
        assert lib.sba_batch_covariance_joint(b._h, dp(rot), dp(tran), None, 0.0, None, None, None) == cabi.SBA_ERR_INVALID_ARG
        assert lib.sba_batch_covariance_joint(b._h, None, dp(tran), None, 0.0, (cabi.JointCov * len(cs))(), None, None) == cabi.SBA_ERR_INVALID_ARG
        # a pair with a non-finite rot fails alone
        g_bad = SIZES.index(257)
        bad = rot.copy(); bad[g_bad, 1] = np.inf
        r = b.covariance_joint(bad, tran, check=False)
        expect = valid.copy(); expect[g_bad] = False
        assert np.array_equal(r.status == 0, expect) and (r.status[~expect] == cabi.SBA_ERR_NUMERIC).all()
        lo, hi = int(off[g_bad]), int(off[g_bad + 1])
        assert np.isnan(r.cov[g_bad]).all() and np.isnan(r.depth_cov[lo:hi]).all() and r.dim[g_bad] == 5
        for g in np.flatnonzero(expect):
            assert r.cov[g].tobytes() == before.cov[g].tobytes()
            assert r.depth_cov[int(off[g]):int(off[g + 1])].tobytes() == before.depth_cov[int(off[g]):int(off[g + 1])].tobytes()
        # every match degenerate: every pair fails, the call says so, the handle works afterwards
        with pytest.raises(api.SbaError) as ei:
            b.covariance_joint(rot, tran, min_sin2_parallax=2.0)
        assert ei.value.code == cabi.SBA_ERR_NUMERIC
        r = b.covariance_joint(rot, tran, min_sin2_parallax=2.0, check=False)
        assert (r.status == cabi.SBA_ERR_NUMERIC).all() and np.isnan(r.cov).all() and np.isnan(r.depth_cov).all()
        assert (r.n_used == 0).all() and np.array_equal(r.n_degenerate, np.array(SIZES)) and (r.dof == -5).all()
        _same(b.covariance_joint(rot, tran, check=False), before, "after the failures")
    monkeypatch.setenv("SBA_PUBLISH", "0")
    with api.Batch(0) as b:
        b.upload(x1, x2, off, d12)
        with pytest.raises(api.SbaError) as ei:
            b.covariance_joint(rot, tran)
        assert ei.value.code == cabi.SBA_ERR_UNSUPPORTED
