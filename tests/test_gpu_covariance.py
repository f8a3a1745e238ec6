"""GPU: the joint solve's covariance (Problem.covariance_joint / sba_problem_covariance_joint; kernels csrc/sba_covariance.hip).

References: the DENSE inverse of the whole normal matrix (tests/cov_reference.py: no Schur complement, no elimination, no
depth scaling) at small sizes, and an element-wise long-double Schur form (below, with its own long-double m x m inverse) at
the sizes where every lane runs one and three grid-stride steps.

Bounds -- the project's REL_TOL_F64 / REL_TOL_F32 on S, U, W and first-order perturbation of an inverse:
    |Sigma_c - ref|_max      <= kappa * TOL * |ref|_max                  kappa: 2-norm condition of the unit-diagonal projected S
    |Sigma_dd,i - ref_i|_max <= (2 kappa_i + kappa) * TOL * |ref_i|_max   kappa_i: condition of the unit-diagonal U_i
with the scene conditions of cov_reference.kappa_limit asserted from the reference."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

import ref_joint_numpy as rj
from cov_reference import DenseCov, check_against, dense_covariance, kappa_limit, sin2_parallax
from helpers import REL_TOL_F32, REL_TOL_F64
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api, synthetic

pytestmark = pytest.mark.gpu

STORES = (api.STORE_F64, api.STORE_F32)
TOL = {api.STORE_F64: REL_TOL_F64, api.STORE_F32: REL_TOL_F32}
GAUGES = (api.TRAN_SPHERE, api.TRAN_FREE)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@lru_cache(maxsize=None)
def _scene(n):
    return synthetic.full_rt(n, seed=900 + n)


def _planes(c, store):
    """What the planes hold: f32 planes are the f32-rounded inputs."""
    if store == api.STORE_F64:
        return c.x1, c.x2
    return c.x1.astype(np.float32).astype(np.float64), c.x2.astype(np.float32).astype(np.float64)


def _points(c):
    return (("init", c.rot_init, c.tran_init), ("true", c.rot_true, c.tran_true))


def _opt(tran_param):
    return api.default_lm_options(tran_param=tran_param)


@lru_cache(maxsize=None)
def _dense(n, store, point, tran_param):
    c = _scene(n)
    x1, x2 = _planes(c, store)
    rot, tran = (c.rot_init, c.tran_init) if point == "init" else (c.rot_true, c.tran_true)
    return dense_covariance(x1, x2, rot, tran, c.d12, tran_param)


# ---- the long-double Schur form ---------------------------------------------------------------------------------------
def _inverse_longdouble(A):
    """Gauss-Jordan with partial pivoting in the dtype of A (m <= 6)."""
    m = len(A)
    M = np.concatenate([A.copy(), np.eye(m, dtype=A.dtype)], axis=1)
    for k in range(m):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
        M[k] = M[k] / M[k, k]
        for i in range(m):
            if i != k:
                M[i] = M[i] - M[i, k] * M[k]
    return M[:, m:]


def schur_covariances(x1, x2, rot, tran, d, delta=1.0, dt=np.longdouble):
    """Element-wise in `dt`, in the shape of ref_joint_numpy.schur_longdouble at radius = inf: {tran_param: reference}.  The
    per-match blocks are formed once and serve both gauges."""
    n = len(x1)
    P = rj.JointProblem(np.asarray(x1), np.asarray(x2), delta)
    e, w, E, F = P.blocks(rot, tran, np.asarray(d), dt)
    w = w.astype(dt)
    EtE = np.einsum("nri,nrj->nij", E, E) * w[:, None, None]
    EtF = np.einsum("nri,nrj->nij", E, F) * w[:, None, None]
    FtF = np.einsum("nri,nrj->nij", F, F) * w[:, None, None]
    det = EtE[:, 0, 0] * EtE[:, 1, 1] - EtE[:, 0, 1] * EtE[:, 1, 0]
    Ui = np.empty_like(EtE)
    Ui[:, 0, 0], Ui[:, 1, 1], Ui[:, 0, 1], Ui[:, 1, 0] = EtE[:, 1, 1] / det, EtE[:, 0, 0] / det, -EtE[:, 0, 1] / det, -EtE[:, 1, 0] / det
    T = np.einsum("nij,nja->nia", Ui, EtF)                      # unscaled depths: the scaling cancels
    S = (FtF - np.einsum("nia,nib->nab", EtF, T)).sum(0)
    rho, _ = rj.huber(delta, np.sum(e * e, axis=1))
    sin2 = sin2_parallax(x1, x2, rot)
    c = np.sqrt(np.clip(1.0 - sin2, 0.0, 1.0))
    out = {}
    for tran_param in GAUGES:
        Pm = rj.projection(tran_param, tran).astype(dt)
        Sl = Pm.T @ S @ Pm
        cov = Pm @ _inverse_longdouble(Sl) @ Pm.T
        TC = np.einsum("nia,ab->nib", T, cov)
        dd = Ui + np.einsum("nib,njb->nij", TC, T)
        r = DenseCov()
        r.m, r.n_used = Pm.shape[1], n
        r.cov = cov.astype(np.float64)
        r.depth_cov = np.stack([dd[:, 0, 0], dd[:, 1, 1], dd[:, 0, 1]], axis=1).astype(np.float64)
        s = 1.0 / np.sqrt(np.diag(Sl).astype(np.float64))
        r.kappa = float(np.linalg.cond(Sl.astype(np.float64) * s[:, None] * s[None, :]))
        r.sin2 = sin2
        with np.errstate(divide="ignore"):
            r.kappa_i = (1.0 + c) / (1.0 - c)
        r.cost, r.sum_w = float(0.5 * rho.sum()), float(w.sum())
        out[tran_param] = r
    return out


# ---- 1. dense reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [5, 63, 64, 65, 257, 513])
def test_against_the_dense_inverse(n, store):
    c = _scene(n)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12, store=store)
        for tran_param in GAUGES:
            for name, rot, tran in _points(c):
                if n == 5 and tran_param == api.TRAN_FREE:          # 15 residuals, 16 parameters
                    with pytest.raises(api.SbaError) as ei:
                        p.covariance_joint(rot, tran, options=_opt(tran_param))
                    assert ei.value.code == cabi.SBA_ERR_NUMERIC
                    continue
                ref = _dense(n, store, name, tran_param)
                assert ref.kappa <= kappa_limit(n, tran_param), ref.kappa
                got = p.covariance_joint(rot, tran, options=_opt(tran_param))
                assert (got.n_used, got.n_degenerate, got.dim, got.dof) == (n, 0, ref.m, n - ref.m)
                check_against(got.cov, got.depth_cov, ref, TOL[store], what=f"dense n={n} store={store} gauge={tran_param} {name}")
        # the default options are the sphere gauge
        d = p.covariance_joint(c.rot_init, c.tran_init)
        assert d.dim == 5 and np.array_equal(d.cov, p.covariance_joint(c.rot_init, c.tran_init, options=_opt(api.TRAN_SPHERE)).cov)


# ---- 2. long-double Schur form where the loops iterate ---------------------------------------------------------------
def _check_schur(p, c, store, what, own_error=False):
    x1, x2 = _planes(c, store)
    n = len(c.x1)
    for name, rot, tran in _points(c):
        refs = schur_covariances(x1, x2, rot, tran, c.d12)
        f64 = schur_covariances(x1, x2, rot, tran, c.d12, dt=np.float64) if own_error else None
        for tran_param in GAUGES:
            ref = refs[tran_param]
            assert ref.kappa <= kappa_limit(n, tran_param), ref.kappa
            if own_error:       # float64 numpy in the same form against long double: what the reference itself is good for
                check_against(f64[tran_param].cov, f64[tran_param].depth_cov, ref, REL_TOL_F64, what=f"{what} numpy f64 vs long double")
            got = p.covariance_joint(rot, tran, options=_opt(tran_param))
            assert (got.n_used, got.n_degenerate, got.dim) == (n, 0, ref.m)
            check_against(got.cov, got.depth_cov, ref, TOL[store], what=f"{what} gauge={tran_param} {name}")
            assert abs(got.cost - ref.cost) <= TOL[store] * ref.cost and abs(got.sum_w - ref.sum_w) <= TOL[store] * ref.sum_w


@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
def test_against_the_longdouble_schur_form(store):
    c = _scene(4097)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12, store=store)
        _check_schur(p, c, store, f"schur n=4097 store={store}", own_error=True)


@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
def test_over_three_grid_stride_steps(monkeypatch, store):
    """One block per CU: with 2 * 256 * CUs matches per step every lane runs three steps, the last one ragged."""
    monkeypatch.setenv("SBA_JOINT_BLOCKS_PER_CU", "1")
    n = 512 * _cus() * 3 - 515
    c = _scene(n)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12, store=store)
        _check_schur(p, c, store, f"schur steps=3 n={n} store={store}")


# ---- 3. degeneracy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,planted", [(257, (0, 100, 256)), (64, (63,)), (65, (1, 64))])
def test_degenerate_matches_are_left_out(n, planted, store):
    c = _scene(n)
    planted = np.array(planted)
    for name, rot, tran in _points(c):
        x1, x2 = c.x1.copy(), c.x2.copy()
        if store == api.STORE_F32:
            # parallel in what the planes hold: x1 a multiple of an f32 vector, x2 = R x1 rounded once more stays within
            # 1e-7 of it -- sin^2 ~ 1e-14, far below the threshold
            x1[planted] = x1[planted].astype(np.float32)
        x2[planted] = x1[planted] @ rj.rotation(rot).T
        p1, p2 = _planes(type(c)(x1, x2, c.d12, c.rot_true, c.tran_true, c.rot_init, c.tran_init), store)
        keep = np.ones(n, dtype=bool)
        keep[planted] = False
        sin2 = sin2_parallax(p1, p2, rot)
        assert (sin2[planted] < 1e-10).all()
        assert not ((sin2[keep] >= 1e-10) & (sin2[keep] <= 1e-8)).any() and (sin2[keep] > 1e-8).all()
        ref = dense_covariance(p1, p2, rot, tran, c.d12, api.TRAN_SPHERE, keep=keep)
        assert ref.kappa <= kappa_limit(n, api.TRAN_SPHERE)
        with api.Problem(0) as p:
            p.upload(x1, x2, c.d12, store=store)
            got = p.covariance_joint(rot, tran, min_sin2_parallax=1e-9)
            assert (got.n_degenerate, got.n_used, got.dof) == (len(planted), n - len(planted), n - len(planted) - 5)
            assert np.array_equal(got.depth_cov[planted], np.tile([np.inf, np.inf, 0.0], (len(planted), 1)))
            check_against(got.cov, got.depth_cov, ref, TOL[store], used=np.flatnonzero(keep), what=f"planted n={n} store={store} {name}")
            assert abs(got.cost - ref.cost) <= TOL[store] * ref.cost and abs(got.sum_w - ref.sum_w) <= TOL[store] * ref.sum_w
            # ... which is the problem without them
            p.upload(x1[keep], x2[keep], c.d12[keep], store=store)
            less = p.covariance_joint(rot, tran, min_sin2_parallax=1e-9)
            assert less.n_degenerate == 0 and less.n_used == got.n_used
            assert np.abs(less.cov - got.cov).max() <= ref.kappa * TOL[store] * np.abs(ref.cov).max()
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12, store=store)
        assert p.covariance_joint(c.rot_init, c.tran_init, min_sin2_parallax=0.0).n_degenerate == 0


# ---- 4. consistency with what exists -----------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [65, 4097])
def test_consistent_with_eval_joint(n, store):
    c = _scene(n)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12, store=store)
        for name, rot, tran in _points(c):
            eq = p.eval_joint(rot, tran, float("inf"))
            for tran_param in GAUGES:
                got = p.covariance_joint(rot, tran, options=_opt(tran_param))
                assert got.n_degenerate == 0
                assert abs(got.cost - eq.cost) <= TOL[store] * eq.cost and abs(got.sum_w - eq.sum_w) <= TOL[store] * eq.sum_w
                assert np.array_equal(got.cov, got.cov.T)
                # the product's own S, inverted in the tangent space, is the covariance
                Pm = rj.projection(tran_param, tran)
                Sl = Pm.T @ eq.S @ Pm
                s = 1.0 / np.sqrt(np.diag(Sl))
                kappa = np.linalg.cond(Sl * s[:, None] * s[None, :])
                assert kappa <= kappa_limit(n, tran_param)
                own = Pm @ np.linalg.inv(Sl) @ Pm.T
                assert np.abs(got.cov - own).max() <= kappa * TOL[store] * np.abs(own).max()
                if tran_param == api.TRAN_SPHERE:
                    assert np.abs(got.cov[3:, 3:] @ tran).max() <= kappa * TOL[store] * np.abs(got.cov).max()
                    assert np.abs(got.cov[:3, 3:] @ tran).max() <= kappa * TOL[store] * np.abs(got.cov).max()
                assert got.sigma2 == 2.0 * got.cost / got.dof


# ---- 5. state and reproducibility ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [5, 4097])
def test_reproducible_and_leaves_the_handle_alone(n, store):
    c = _scene(n)
    with api.Problem(0) as p, api.Problem(0) as q:
        p.upload(c.x1, c.x2, c.d12, store=store)
        q.upload(c.x1, c.x2, c.d12, store=store)
        a, b = p.covariance_joint(c.rot_init, c.tran_init), p.covariance_joint(c.rot_init, c.tran_init)
        assert a.cov.tobytes() == b.cov.tobytes() and a.depth_cov.tobytes() == b.depth_cov.tobytes()
        assert (a.cost, a.sum_w, a.n_used, a.n_degenerate, a.dim, a.dof) == (b.cost, b.sum_w, b.n_used, b.n_degenerate, b.dim, b.dof)
        nd = p.covariance_joint(c.rot_init, c.tran_init, depths=False)
        assert nd.depth_cov is None and nd.cov.tobytes() == a.cov.tobytes() and nd.cost == a.cost
        assert a.depth_cov.shape == (n, 3) and np.isfinite(a.depth_cov).all() and (a.depth_cov[:, :2] > 0).all()
        # solve_joint after a covariance call == solve_joint without one
        with_cov, without = p.solve_joint(c.rot_init, c.tran_init), q.solve_joint(c.rot_init, c.tran_init)
        for u, v in zip(with_cov[:3], without[:3]):
            assert u.tobytes() == v.tobytes()
        s1, s2 = with_cov[3], without[3]
        assert (s1.termination, s1.num_iterations, s1.num_successful_steps, s1.num_evaluations, s1.initial_cost, s1.final_cost,
                s1.final_gradient_max_norm, s1.final_radius) == \
               (s2.termination, s2.num_iterations, s2.num_successful_steps, s2.num_evaluations, s2.initial_cost, s2.final_cost,
                s2.final_gradient_max_norm, s2.final_radius)
        # ... and at the solution the covariance is that of a fresh handle holding the refined depths
        rot, tran, d, _ = with_cov
        q.upload(c.x1, c.x2, d, store=store)
        assert p.covariance_joint(rot, tran).cov.tobytes() == q.covariance_joint(rot, tran).cov.tobytes()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------
def test_refusals():
    c = _scene(65)
    lib = cabi.load_library()
    with api.Problem(0) as p:
        with pytest.raises(api.SbaError) as ei:
            p.covariance_joint(c.rot_init, c.tran_init)
        assert ei.value.code == cabi.SBA_ERR_NOT_UPLOADED
        p.upload(c.x1, c.x2)                              # uniform depths: no per-match planes
        with pytest.raises(api.SbaError) as ei:
            p.covariance_joint(c.rot_init, c.tran_init)
        assert ei.value.code == cabi.SBA_ERR_UNSUPPORTED
        p.set_depths(c.d12)
        before = p.covariance_joint(c.rot_init, c.tran_init)
        for bad in (-1.0, float("nan")):
            with pytest.raises(api.SbaError) as ei:
                p.covariance_joint(c.rot_init, c.tran_init, min_sin2_parallax=bad)
            assert ei.value.code == cabi.SBA_ERR_INVALID_ARG
        dp = lambda a: a.ctypes.data_as(cabi._dp)
        assert lib.sba_problem_covariance_joint(p._h, dp(c.rot_init), dp(c.tran_init), None, 0.0, None, None) == cabi.SBA_ERR_INVALID_ARG
        bad = c.rot_init.copy(); bad[2] = np.inf
        with pytest.raises(api.SbaError) as ei:
            p.covariance_joint(bad, c.tran_init)
        assert ei.value.code == cabi.SBA_ERR_NUMERIC
        p.set_shard(0, 2)
        with pytest.raises(api.SbaError) as ei:
            p.covariance_joint(c.rot_init, c.tran_init)
        assert ei.value.code == cabi.SBA_ERR_UNSUPPORTED
        p.set_shard(0, 1)
        p.set_allreduce(lambda buf, count, stream: 0)
        with pytest.raises(api.SbaError) as ei:
            p.covariance_joint(c.rot_init, c.tran_init)
        assert ei.value.code == cabi.SBA_ERR_UNSUPPORTED
        p.set_allreduce(None)
        assert p.covariance_joint(c.rot_init, c.tran_init).cov.tobytes() == before.cov.tobytes()
        # every match degenerate: nothing is left to invert
        with pytest.raises(api.SbaError) as ei:
            p.covariance_joint(c.rot_init, c.tran_init, min_sin2_parallax=2.0)
        assert ei.value.code == cabi.SBA_ERR_NUMERIC
    c3 = _scene(3)
    with api.Problem(0) as p:
        p.upload(c3.x1, c3.x2, c3.d12)
        out, dd = cabi.JointCov(), np.full(9, -7.0)
        out.dim = -7
        rc = lib.sba_problem_covariance_joint(p._h, c3.rot_init.ctypes.data_as(cabi._dp), c3.tran_init.ctypes.data_as(cabi._dp), None, 0.0,
                                              C.byref(out), dd.ctypes.data_as(cabi._dp))
        assert rc == cabi.SBA_ERR_NUMERIC and out.dim == -7 and (dd == -7.0).all()       # no outputs written
        # the handle is still usable
        eq = p.eval_joint(c3.rot_init, c3.tran_init)
        assert np.isfinite(eq.cost)
        c65 = _scene(65)
        p.upload(c65.x1, c65.x2, c65.d12)
        assert p.covariance_joint(c65.rot_init, c65.tran_init).n_used == 65


# ---- mirror class / CLI: set_joint_covariance, sba_main --joint --covariance ------------------------------------------
def test_cli_covariance_switch(tmp_path):
    """--covariance adds ONE stdout line after the joint stage -- the 1-sigma of rot (degrees) and tran of
    Problem.covariance_joint at the joint result, scaled by sigma2 -- and changes nothing else: log.txt and log_d.txt are the
    bytes of the --joint run.  Without --joint it is a usage error."""
    import re
    import subprocess

    from test_gpu_joint import SBA_MAIN, _cli_fixture, _run_cli
    c, (kl, kr), deg, args, (W, H, n) = _cli_fixture(tmp_path)
    out_j, log_j, logd_j = _run_cli(tmp_path, ["--joint", *args])
    out_c, log_c, logd_c = _run_cli(tmp_path, ["--joint", *args, "--covariance"])
    assert (log_c, logd_c) == (log_j, logd_j)
    assert "joint covariance" not in out_j
    lines = [ln for ln in out_c.splitlines() if ln.startswith("joint covariance:")]
    assert len(lines) == 1
    mask = lambda t: re.sub(r"[0-9.]+ ms", "ms", t)
    assert mask(out_c).replace(lines[0] + "\n", "") == mask(out_j)
    assert out_c.splitlines()[out_c.splitlines().index(lines[0]) - 1].startswith("joint: iterations")
    # the same library calls from Python
    rot0 = np.array([float(a) for a in args[2:5]]) / 180 * 3.14159265358979323846
    with api.Problem(0) as p:
        p.upload_keypoints(kl, kr, W, H)
        p.set_depths(np.full((n, 2), 6.0))
        d, _ = p.solve_depths(rot0, c.tran_init)
        r1, t1, _ = p.solve(api.MODE_ROT, rot0, c.tran_init, d[0, 0], d[1, 0])
        r2, t2, _ = p.solve(api.MODE_TRAN, r1, t1, d[0, 0], d[1, 0])
        rj_, tj, _, _ = p.solve_joint(r2, t2)
        cov = p.covariance_joint(rj_, tj, depths=False)
    sd = np.sqrt(cov.sigma2 * np.diag(cov.cov))
    want = ("joint covariance: 1-sigma rot (deg) %.6e %.6e %.6e, tran %.6e %.6e %.6e (sigma^2 = 2 cost / dof = %.6e, %d used, %d degenerate)"
            % (*(sd[:3] / 3.14159265358979323846 * 180.0), *sd[3:], cov.sigma2, cov.n_used, cov.n_degenerate))
    assert lines[0] == want
    assert cov.n_used == n and (sd[:3] > 0).all() and np.isfinite(sd).all()
    r = subprocess.run([str(SBA_MAIN), *args, "--covariance"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--covariance needs --joint" in r.stdout and "d-only" not in r.stdout
