"""GPU: triangulated landmarks with their 3 x 3 covariances and the cut driven by them (Problem.structure_joint /
structure_joint_into / structure_order_stats / structure_keep_below; kernel csrc/sba_structure.hip).

References: G Sigma G^T on the DENSE inverse of the whole normal matrix (tests/structure_reference.py: no Schur complement, no
elimination, no depth scaling) at small sizes, and an element-wise long-double Schur form (below) at the sizes where every
lane runs one and three grid-stride steps.

Bounds -- the project's REL_TOL_F64 / REL_TOL_F32:
    |X_i - ref|_max          <= TOL * |X_i|
    |Sigma_X,i - ref_i|_max  <= (2 kappa_i + kappa) * TOL * |ref_i|_max      and the same for q_i
kappa: condition of the unit-diagonal projected S, kappa_i: of the unit-diagonal U_i, with the scene conditions of
cov_reference.kappa_limit asserted from the reference.  This is the bound of the 2 x 2 depth blocks
(tests/test_gpu_covariance.py): Sigma_X,i is a fixed, well-conditioned linear image (|G| <= max(1, d) / 2) of the blocks it covers."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

import ref_joint_numpy as rj
from cov_reference import DenseCov, kappa_limit, sin2_parallax
from helpers import REL_TOL_F32, REL_TOL_F64
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api, synthetic
from structure_reference import DenseStructure, check_structure, dense_structure, landmark_jacobians, landmarks, pack6
from test_gpu_covariance import _inverse_longdouble

pytestmark = pytest.mark.gpu

STORES = (api.STORE_F64, api.STORE_F32)
TOL = {api.STORE_F64: REL_TOL_F64, api.STORE_F32: REL_TOL_F32}
GAUGES = (api.TRAN_SPHERE, api.TRAN_FREE)
INF_ROW = [np.inf, np.inf, np.inf, 0.0, 0.0, 0.0]


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


def _same_pose(a, b):
    """Two JointCovariance records, bit for bit (depth_cov aside)."""
    return a.cov.tobytes() == b.cov.tobytes() and \
        (a.cost, a.sum_w, a.n_used, a.n_degenerate, a.dim, a.dof) == (b.cost, b.sum_w, b.n_used, b.n_degenerate, b.dim, b.dof)


def _planted(c, planted, rot, store):
    """The scene with the rays of `planted` made parallel at `rot` in what the planes hold (tests/test_gpu_covariance.py)."""
    x1, x2 = c.x1.copy(), c.x2.copy()
    if store == api.STORE_F32:
        x1[planted] = x1[planted].astype(np.float32)
    x2[planted] = x1[planted] @ rj.rotation(rot).T
    return type(c)(x1, x2, c.d12, c.rot_true, c.tran_true, c.rot_init, c.tran_init)


# ---- the long-double Schur form ---------------------------------------------------------------------------------------
def schur_structure(x1, x2, rot, tran, d, delta=1.0, dt=np.longdouble):
    """Element-wise in `dt`, the closed form the product evaluates: {tran_param: reference}.
    Sigma_X = G_d U^-1 G_d^T + K Sigma_c K^T, K = G_c - G_d U^-1 W (unscaled depths: the scaling cancels)."""
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
    T = np.einsum("nij,nja->nia", Ui, EtF)
    S = (FtF - np.einsum("nia,nib->nab", EtF, T)).sum(0)
    Gd, Gc = landmark_jacobians(x1, x2, rot, tran, d, dt)
    K = Gc - np.einsum("nri,nia->nra", Gd, T)
    own = np.einsum("nri,nij,nsj->nrs", Gd, Ui, Gd)
    X = landmarks(x1, x2, rot, tran, d, dt)
    rho, _ = rj.huber(delta, np.sum(e * e, axis=1))
    sin2 = sin2_parallax(x1, x2, rot)
    c = np.sqrt(np.clip(1.0 - sin2, 0.0, 1.0))
    out = {}
    for tran_param in GAUGES:
        Pm = rj.projection(tran_param, tran).astype(dt)
        Sl = Pm.T @ S @ Pm
        cov = Pm @ _inverse_longdouble(Sl) @ Pm.T
        SX = own + np.einsum("nrb,nsb->nrs", np.einsum("nra,ab->nrb", K, cov), K)
        r = DenseStructure()
        r.xyz = X.astype(np.float64)
        r.cov = pack6(SX).astype(np.float64)
        r.score = ((SX[:, 0, 0] + SX[:, 1, 1] + SX[:, 2, 2]) / np.sum(X * X, axis=1)).astype(np.float64)
        r.pose = DenseCov()
        r.pose.m, r.pose.n_used = Pm.shape[1], n
        r.pose.cov = cov.astype(np.float64)
        s = 1.0 / np.sqrt(np.diag(Sl).astype(np.float64))
        r.pose.kappa = float(np.linalg.cond(Sl.astype(np.float64) * s[:, None] * s[None, :]))
        r.pose.sin2 = sin2
        with np.errstate(divide="ignore"):
            r.pose.kappa_i = (1.0 + c) / (1.0 - c)
        r.pose.cost, r.pose.sum_w = float(0.5 * rho.sum()), float(w.sum())
        out[tran_param] = r
    return out


@lru_cache(maxsize=None)
def _dense(n, store, point, tran_param):
    c = _scene(n)
    x1, x2 = _planes(c, store)
    rot, tran = (c.rot_init, c.tran_init) if point == "init" else (c.rot_true, c.tran_true)
    return dense_structure(x1, x2, rot, tran, c.d12, tran_param)


# ---- 1. dense reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [5, 63, 64, 65, 257, 513])
def test_against_the_dense_inverse(n, store):
    """Largest err / bound measured on the MI355X (f64 planes): xyz 0.013, covariance 0.167 (n = 257), score 0.16 (n = 64), both
    with free translation at the true pose -- where the 2 x 2 depth blocks of tests/test_gpu_covariance.py measure 0.16 (DESIGN.md
    section 3.15).  No case exceeds 1: the bound stands as stated."""
    c = _scene(n)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12, store=store)
        for tran_param in GAUGES:
            for name, rot, tran in _points(c):
                if n == 5 and tran_param == api.TRAN_FREE:          # 15 residuals, 16 parameters
                    with pytest.raises(api.SbaError) as ei:
                        p.structure_joint(rot, tran, options=_opt(tran_param))
                    assert ei.value.code == cabi.SBA_ERR_NUMERIC
                    continue
                ref = _dense(n, store, name, tran_param)
                assert ref.pose.kappa <= kappa_limit(n, tran_param), ref.pose.kappa
                got = p.structure_joint(rot, tran, options=_opt(tran_param))
                assert (got.n_used, got.n_degenerate, got.dim, got.dof) == (n, 0, ref.pose.m, n - ref.pose.m)
                assert got.xyz.shape == (n, 3) and got.cov.shape == (n, 6) and got.score.shape == (n,)
                check_structure(got.xyz, got.cov, got.score, ref, TOL[store], what=f"dense n={n} store={store} gauge={tran_param} {name}")
        # the default options are the sphere gauge
        d = p.structure_joint(c.rot_init, c.tran_init)
        assert d.dim == 5 and d.cov.tobytes() == p.structure_joint(c.rot_init, c.tran_init, options=_opt(api.TRAN_SPHERE)).cov.tobytes()


# ---- 2. long-double Schur form where the loops iterate ---------------------------------------------------------------
def _check_schur(p, c, store, what, tail=0):
    x1, x2 = _planes(c, store)
    n = len(c.x1)
    for name, rot, tran in _points(c):
        refs = schur_structure(x1, x2, rot, tran, c.d12)
        for tran_param in GAUGES:
            ref = refs[tran_param]
            assert ref.pose.kappa <= kappa_limit(n, tran_param), ref.pose.kappa
            got = p.structure_joint(rot, tran, options=_opt(tran_param))
            assert (got.n_used, got.n_degenerate, got.dim) == (n, 0, ref.pose.m)
            check_structure(got.xyz, got.cov, got.score, ref, TOL[store], what=f"{what} gauge={tran_param} {name}")
            if tail:        # the rows with the largest index, the ragged last vector included, on their own
                rows = np.arange(n - tail, n)
                assert np.isfinite(got.xyz[rows]).all() and np.isfinite(got.cov[rows]).all() and (got.score[rows] > 0).all()
                check_structure(got.xyz[rows], got.cov, got.score, _rows_of(ref, rows), TOL[store], used=rows, what=f"{what} tail")


def _rows_of(ref, rows):
    r = DenseStructure()
    r.xyz, r.cov, r.score, r.pose = ref.xyz[rows], ref.cov, ref.score, ref.pose
    return r


@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
def test_against_the_longdouble_schur_form(store):
    c = _scene(4097)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12, store=store)
        _check_schur(p, c, store, f"schur n=4097 store={store}", tail=3)


@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
def test_over_three_grid_stride_steps(monkeypatch, store):
    """One block per CU: with 2 * 256 * CUs matches per step every lane runs three steps, the last one ragged (n is odd: the
    last vector holds one match and a padding row that must not be stored)."""
    monkeypatch.setenv("SBA_JOINT_BLOCKS_PER_CU", "1")
    n = 512 * _cus() * 3 - 515
    c = _scene(n)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12, store=store)
        _check_schur(p, c, store, f"schur steps=3 n={n} store={store}", tail=515)


# ---- 3. degeneracy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,planted", [(257, (0, 100, 256)), (64, (63,)), (65, (1, 64))])
def test_degenerate_matches_are_left_out(n, planted, store):
    c = _scene(n)
    planted = np.array(planted)
    for name, rot, tran in _points(c):
        cd = _planted(c, planted, rot, store)
        p1, p2 = _planes(cd, store)
        keep = np.ones(n, dtype=bool)
        keep[planted] = False
        sin2 = sin2_parallax(p1, p2, rot)
        assert (sin2[planted] < 1e-10).all()
        assert not ((sin2[keep] >= 1e-10) & (sin2[keep] <= 1e-8)).any() and (sin2[keep] > 1e-8).all()
        ref = dense_structure(p1, p2, rot, tran, c.d12, api.TRAN_SPHERE, keep=keep)
        assert ref.pose.kappa <= kappa_limit(n, api.TRAN_SPHERE)
        with api.Problem(0) as p:
            p.upload(cd.x1, cd.x2, c.d12, store=store)
            got = p.structure_joint(rot, tran, min_sin2_parallax=1e-9)
            assert (got.n_degenerate, got.n_used, got.dof) == (len(planted), n - len(planted), n - len(planted) - 5)
            assert np.array_equal(got.cov[planted], np.tile(INF_ROW, (len(planted), 1)))
            assert np.array_equal(got.score[planted], np.full(len(planted), np.inf))
            assert np.isfinite(got.xyz).all()
            assert np.abs(got.xyz[planted] - ref.xyz[planted]).max() <= TOL[store] * np.abs(ref.xyz[planted]).max()
            check_structure(got.xyz, got.cov, got.score, ref, TOL[store], used=np.flatnonzero(keep), what=f"planted n={n} store={store} {name}")
            assert _same_pose(got.pose, p.covariance_joint(rot, tran, min_sin2_parallax=1e-9, depths=False))


# ---- 4. consistency with what exists -----------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [65, 4097])
def test_consistent_with_covariance_joint(n, store):
    """out is covariance_joint's record bit for bit, and the four-term form G_d Sigma_dd G_d^T + G_d Sigma_dc G_c^T + its
    transpose + G_c Sigma_c G_c^T -- with Sigma_dd from covariance_joint's own depth blocks, Sigma_dc = -U^-1 W Sigma_c in numpy --
    agrees with the product's two-term form within the bound of the dense test."""
    c = _scene(n)
    x1, x2 = _planes(c, store)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12, store=store)
        for name, rot, tran in _points(c):
            _, w, E, F = rj.JointProblem(x1, x2, 1.0).blocks(rot, tran, c.d12)
            EtE = np.einsum("nri,nrj->nij", E, E) * w[:, None, None]
            EtF = np.einsum("nri,nrj->nij", E, F) * w[:, None, None]
            T = np.linalg.solve(EtE, EtF)
            Gd, Gc = landmark_jacobians(x1, x2, rot, tran, c.d12)
            X = landmarks(x1, x2, rot, tran, c.d12)
            for tran_param in GAUGES:
                cj = p.covariance_joint(rot, tran, options=_opt(tran_param))
                got = p.structure_joint(rot, tran, options=_opt(tran_param))
                assert _same_pose(got.pose, cj) and got.sigma2 == cj.sigma2
                dd = np.empty((n, 2, 2))
                dd[:, 0, 0], dd[:, 1, 1], dd[:, 0, 1], dd[:, 1, 0] = cj.depth_cov[:, 0], cj.depth_cov[:, 1], cj.depth_cov[:, 2], cj.depth_cov[:, 2]
                dc = -np.einsum("nia,ab->nib", T, cj.cov)
                cross = np.einsum("nrb,nsb->nrs", np.einsum("nri,nib->nrb", Gd, dc), Gc)
                SX = np.einsum("nri,nij,nsj->nrs", Gd, dd, Gd) + cross + cross.transpose(0, 2, 1) + np.einsum("nrb,nsb->nrs", np.einsum("nra,ab->nrb", Gc, cj.cov), Gc)
                ref = DenseStructure()
                ref.xyz, ref.cov, ref.score = X, pack6(SX), (SX[:, 0, 0] + SX[:, 1, 1] + SX[:, 2, 2]) / np.sum(X * X, axis=1)
                ref.pose = DenseCov()
                Pm = rj.projection(tran_param, tran)
                Sl = np.linalg.inv(Pm.T @ cj.cov @ Pm)
                s = 1.0 / np.sqrt(np.diag(Sl))
                ref.pose.kappa = float(np.linalg.cond(Sl * s[:, None] * s[None, :]))
                assert ref.pose.kappa <= kappa_limit(n, tran_param)
                cs = np.sqrt(np.clip(1.0 - sin2_parallax(x1, x2, rot), 0.0, 1.0))
                ref.pose.kappa_i = (1.0 + cs) / (1.0 - cs)
                check_structure(got.xyz, got.cov, got.score, ref, TOL[store], what=f"four terms n={n} store={store} gauge={tran_param} {name}")


# ---- 5. outputs and the handle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [5, 4097])
def test_outputs_grids_and_the_handle(monkeypatch, n, store):
    c = _scene(n)
    rot, tran = c.rot_init, c.tran_init
    with api.Problem(0) as p, api.Problem(0) as q:
        p.upload(c.x1, c.x2, c.d12, store=store)
        q.upload(c.x1, c.x2, c.d12, store=store)
        a = p.structure_joint(rot, tran)
        assert np.isfinite(a.xyz).all() and np.isfinite(a.cov).all() and (a.cov[:, :3] > 0).all() and (a.score > 0).all()
        # every subset of the outputs gives the bits of the all-outputs call
        for want in range(8):
            kw = dict(xyz=bool(want & 1), cov=bool(want & 2), score=bool(want & 4))
            b = p.structure_joint(rot, tran, **kw)
            assert _same_pose(a.pose, b.pose)
            for name in ("xyz", "cov", "score"):
                assert (getattr(b, name) is None) == (not kw[name])
                if kw[name]:
                    assert getattr(b, name).tobytes() == getattr(a, name).tobytes(), (want, name)
        # ... and so does a grid of one block (the kernel's own grid; the reduce pass keeps its own)
        monkeypatch.setenv("SBA_STRUCTURE_GRID", "1")
        one = p.structure_joint(rot, tran)
        monkeypatch.delenv("SBA_STRUCTURE_GRID")
        again = p.structure_joint(rot, tran)
        for b in (one, again):
            assert _same_pose(a.pose, b.pose)
            assert (a.xyz.tobytes(), a.cov.tobytes(), a.score.tobytes()) == (b.xyz.tobytes(), b.cov.tobytes(), b.score.tobytes())
        # device destinations: torch tensors, bit-equal to the host form; nothing beyond row n is touched
        dev = torch.device("cuda", 0)
        tx = torch.full((n + 2, 3), -7.0, dtype=torch.float64, device=dev)
        tc = torch.full((n + 2, 6), -7.0, dtype=torch.float64, device=dev)
        ts = torch.full((n + 2,), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        pose = p.structure_joint_into(tx.data_ptr(), tc.data_ptr(), ts.data_ptr(), rot, tran)
        assert _same_pose(a.pose, pose)
        hx, hc, hs = tx.cpu().numpy(), tc.cpu().numpy(), ts.cpu().numpy()
        assert (hx[:n].tobytes(), hc[:n].tobytes(), hs[:n].tobytes()) == (a.xyz.tobytes(), a.cov.tobytes(), a.score.tobytes())
        assert (hx[n:] == -7.0).all() and (hc[n:] == -7.0).all() and (hs[n:] == -7.0).all()
        ts2 = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        assert _same_pose(a.pose, p.structure_joint_into(None, None, ts2.data_ptr(), rot, tran))
        assert ts2.cpu().numpy().tobytes() == a.score.tobytes()
        # a destination off by 8 bytes is refused and nothing is written
        for k in range(3):
            ptrs = [tx.data_ptr(), tc.data_ptr(), ts.data_ptr()]
            ptrs[k] += 8
            with pytest.raises(api.SbaError) as ei:
                p.structure_joint_into(*ptrs, rot, tran)
            assert ei.value.code == cabi.SBA_ERR_INVALID_ARG
        assert (tx.cpu().numpy().tobytes(), tc.cpu().numpy().tobytes(), ts.cpu().numpy().tobytes()) == (hx.tobytes(), hc.tobytes(), hs.tobytes())
        # solve_joint after the calls == solve_joint without them
        with_s, without = p.solve_joint(rot, tran), q.solve_joint(rot, tran)
        for u, v in zip(with_s[:3], without[:3]):
            assert u.tobytes() == v.tobytes()
        s1, s2 = with_s[3], without[3]
        assert (s1.termination, s1.num_iterations, s1.num_successful_steps, s1.num_evaluations, s1.initial_cost, s1.final_cost,
                s1.final_gradient_max_norm, s1.final_radius) == \
               (s2.termination, s2.num_iterations, s2.num_successful_steps, s2.num_evaluations, s2.initial_cost, s2.final_cost,
                s2.final_gradient_max_norm, s2.final_radius)


# ---- 6. the cut --------------------------------------------------------------------------------------------------------
@pytest.fixture
def pinned_grid(monkeypatch):
    """Same blocks per CU for every sweep variant (read at handle creation): a compacted and a fresh handle then reduce in
    the same order and their packs compare bit for bit (tests/test_gpu_quantile.py)."""
    monkeypatch.setenv("SBA_BLOCKS_PER_CU", "2")


@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
@pytest.mark.parametrize("n,planted", [(65, (1, 64)), (4097, (0, 100, 4096))])
def test_the_cut(pinned_grid, n, planted, store):
    c = _scene(n)
    planted = np.array(planted)
    rot, tran = c.rot_init, c.tran_init
    cd = _planted(c, planted, rot, store)
    kw = dict(min_sin2_parallax=1e-9)
    with api.Problem(0) as p, api.Problem(0) as q:
        p.upload(cd.x1, cd.x2, c.d12, store=store)
        score = p.structure_joint(rot, tran, **kw).score
        assert np.array_equal(np.flatnonzero(np.isinf(score)), planted) and not np.isnan(score).any()
        # order statistics: elements of the score array, bit for bit
        ranks = np.unique([0, n - 1, n - len(planted) - 1, n - len(planted), *(int(np.floor(pr * np.float64(n - 1))) for pr in (0.25, 0.5, 0.9))])
        for chunk in (ranks[:4], ranks[4:]):
            vals = p.structure_order_stats(rot, tran, chunk, **kw)
            want = np.partition(score, chunk)[chunk]
            assert vals.view(np.uint64).tolist() == want.view(np.uint64).tolist()
        assert p.structure_order_stats(rot, tran, [n - 1], **kw)[0] == np.inf
        # keep_below: exactly score <= scale * q_(k), in order; the planted rows go
        k = int(api.quantile_rank(0.5, n)[0])
        value = np.partition(score, k)[k]
        idx, thr = p.structure_keep_below(rot, tran, 0.5, 4.0, **kw)
        assert thr == np.float64(4.0) * np.float64(value)
        keep = score <= thr
        assert idx.dtype == np.int64 and np.array_equal(idx, np.flatnonzero(keep))
        assert not keep[planted].any() and keep.sum() >= k + 1 and p.size == keep.sum()
        # the handle equals a fresh upload of the kept rows: a sweep's pack, per-match and uniform, and the structure itself
        q.upload(cd.x1[keep], cd.x2[keep], c.d12[keep], store=store)
        for dm in (api.DEPTH_UNIFORM, api.DEPTH_PER_MATCH):
            for mode in (api.MODE_ROT, api.MODE_TRAN, api.MODE_RT):
                f = lambda h: h.eval_pack(mode, rot, tran, 1.2, 0.9, huber_delta=1.0, depth_mode=dm)
                assert f(p).tobytes() == f(q).tobytes(), (dm, mode)
        a, b = p.structure_joint(rot, tran, **kw), q.structure_joint(rot, tran, **kw)
        assert _same_pose(a.pose, b.pose) and a.n_degenerate == 0
        assert (a.xyz.tobytes(), a.cov.tobytes(), a.score.tobytes()) == (b.xyz.tobytes(), b.cov.tobytes(), b.score.tobytes())
    # a rank that lands on a +inf score: the threshold is +inf and every match stays (no score is NaN)
    with api.Problem(0) as p:
        p.upload(cd.x1, cd.x2, c.d12, store=store)
        idx, thr = p.structure_keep_below(rot, tran, 1.0, 4.0, **kw)
        assert thr == np.inf and np.array_equal(idx, np.arange(n)) and p.size == n


# ---- 7. refusals --------------------------------------------------------------------------------------------------------
def _entry_points(p, rot, tran, **kw):
    """The four entry points as thunks (device destinations: none asked for -- the refusals come first)."""
    return {
        "structure_joint": lambda: p.structure_joint(rot, tran, **kw),
        "structure_joint_into": lambda: p.structure_joint_into(None, None, None, rot, tran, **kw),
        "structure_order_stats": lambda: p.structure_order_stats(rot, tran, [0], **kw),
        "structure_keep_below": lambda: p.structure_keep_below(rot, tran, 0.5, 4.0, **kw),
    }


def _refused(p, rot, tran, code, **kw):
    for name, f in _entry_points(p, rot, tran, **kw).items():
        with pytest.raises(api.SbaError) as ei:
            f()
        assert ei.value.code == code, name


def test_refusals():
    c = _scene(65)
    lib = cabi.load_library()
    with api.Problem(0) as p:
        _refused(p, c.rot_init, c.tran_init, cabi.SBA_ERR_NOT_UPLOADED)
        p.upload(c.x1, c.x2)                              # uniform depths: no per-match planes
        _refused(p, c.rot_init, c.tran_init, cabi.SBA_ERR_UNSUPPORTED)
        p.set_depths(c.d12)
        before = p.structure_joint(c.rot_init, c.tran_init)
        for bad in (-1.0, float("nan")):
            _refused(p, c.rot_init, c.tran_init, cabi.SBA_ERR_INVALID_ARG, min_sin2_parallax=bad)
        dp = lambda a: a.ctypes.data_as(cabi._dp)
        for f in (lib.sba_problem_structure_joint, lib.sba_problem_structure_joint_device):
            assert f(p._h, dp(c.rot_init), dp(c.tran_init), None, 0.0, None, None, None, None) == cabi.SBA_ERR_INVALID_ARG
        bad = c.rot_init.copy(); bad[2] = np.inf
        _refused(p, bad, c.tran_init, cabi.SBA_ERR_NUMERIC)
        p.set_shard(0, 2)
        _refused(p, c.rot_init, c.tran_init, cabi.SBA_ERR_UNSUPPORTED)
        p.set_shard(0, 1)
        p.set_allreduce(lambda buf, count, stream: 0)
        _refused(p, c.rot_init, c.tran_init, cabi.SBA_ERR_UNSUPPORTED)
        p.set_allreduce(None)
        # every match degenerate: nothing is left to invert -- and nothing is cut
        _refused(p, c.rot_init, c.tran_init, cabi.SBA_ERR_NUMERIC, min_sin2_parallax=2.0)
        assert p.size == 65
        # the cut's own arguments
        with pytest.raises(api.SbaError) as ei:
            p.structure_order_stats(c.rot_init, c.tran_init, [65])
        assert ei.value.code == cabi.SBA_ERR_INVALID_ARG
        for scale in (-1.0, float("inf"), float("nan")):
            with pytest.raises(api.SbaError) as ei:
                p.structure_keep_below(c.rot_init, c.tran_init, 0.5, scale)
            assert ei.value.code == cabi.SBA_ERR_INVALID_ARG
        after = p.structure_joint(c.rot_init, c.tran_init)
        assert p.size == 65 and _same_pose(before.pose, after.pose) and before.cov.tobytes() == after.cov.tobytes()
    c3 = _scene(3)
    with api.Problem(0) as p:
        p.upload(c3.x1, c3.x2, c3.d12)
        out, xyz, cv, sc = cabi.JointCov(), np.full(9, -7.0), np.full(18, -7.0), np.full(3, -7.0)
        out.dim = -7
        rc = lib.sba_problem_structure_joint(p._h, c3.rot_init.ctypes.data_as(cabi._dp), c3.tran_init.ctypes.data_as(cabi._dp), None, 0.0,
                                             C.byref(out), xyz.ctypes.data_as(cabi._dp), cv.ctypes.data_as(cabi._dp), sc.ctypes.data_as(cabi._dp))
        assert rc == cabi.SBA_ERR_NUMERIC and out.dim == -7 and (xyz == -7.0).all() and (cv == -7.0).all() and (sc == -7.0).all()
        t = torch.full((3, 3), -7.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(api.SbaError) as ei:
            p.structure_joint_into(t.data_ptr(), None, None, c3.rot_init, c3.tran_init)
        assert ei.value.code == cabi.SBA_ERR_NUMERIC and (t.cpu().numpy() == -7.0).all()       # no outputs written
        with pytest.raises(api.SbaError) as ei:
            p.structure_keep_below(c3.rot_init, c3.tran_init, 0.5, 4.0)
        assert ei.value.code == cabi.SBA_ERR_NUMERIC and p.size == 3
        # the handle is still usable
        eq = p.eval_joint(c3.rot_init, c3.tran_init)
        assert np.isfinite(eq.cost)
        c65 = _scene(65)
        p.upload(c65.x1, c65.x2, c65.d12)
        assert p.structure_joint(c65.rot_init, c65.tran_init).n_used == 65


# ---- 8. mirror class / CLI: set_structure_output, sba_main --joint --structure FILE -------------------------------------
def test_cli_structure_switch(tmp_path):
    """--structure FILE adds ONE stdout line after the joint stage and writes the PLY -- x y z of Problem.structure_joint at
    the joint result and q = sigma2 * score, printed with 17 digits -- and changes nothing else: log.txt and log_d.txt are the
    bytes of the --joint run.  Without --joint it is a usage error."""
    import re
    import subprocess

    from test_gpu_joint import SBA_MAIN, _cli_fixture, _run_cli
    c, (kl, kr), deg, args, (W, H, n) = _cli_fixture(tmp_path)
    ply = tmp_path / "structure.ply"
    out_j, log_j, logd_j = _run_cli(tmp_path, ["--joint", *args])
    assert not ply.exists() and "joint structure" not in out_j
    out_s, log_s, logd_s = _run_cli(tmp_path, ["--joint", *args, "--structure", str(ply)])
    assert (log_s, logd_s) == (log_j, logd_j)
    lines = [ln for ln in out_s.splitlines() if ln.startswith("joint structure:")]
    assert len(lines) == 1
    mask = lambda t: re.sub(r"[0-9.]+ ms", "ms", t)
    assert mask(out_s).replace(lines[0] + "\n", "") == mask(out_j)
    assert out_s.splitlines()[out_s.splitlines().index(lines[0]) - 1].startswith("joint: iterations")
    # the same library calls from Python
    rot0 = np.array([float(a) for a in args[2:5]]) / 180 * 3.14159265358979323846
    with api.Problem(0) as p:
        p.upload_keypoints(kl, kr, W, H)
        p.set_depths(np.full((n, 2), 6.0))
        d, _ = p.solve_depths(rot0, c.tran_init)
        r1, t1, _ = p.solve(api.MODE_ROT, rot0, c.tran_init, d[0, 0], d[1, 0])
        r2, t2, _ = p.solve(api.MODE_TRAN, r1, t1, d[0, 0], d[1, 0])
        rj_, tj, _, _ = p.solve_joint(r2, t2)
        st = p.structure_joint(rj_, tj, cov=False)
    text = ply.read_text().splitlines()
    end = text.index("end_header")
    assert text[0] == "ply" and text[1] == "format ascii 1.0" and f"element vertex {n}" in text[:end]
    assert [ln.split()[-1] for ln in text[:end] if ln.startswith("property double")] == ["x", "y", "z", "q"]
    rows = np.array([[float(v) for v in ln.split()] for ln in text[end + 1:]])
    assert rows.shape == (n, 4)
    assert rows[:, :3].tobytes() == st.xyz.tobytes() and rows[:, 3].tobytes() == (st.sigma2 * st.score).tobytes()
    assert lines[0] == "joint structure: %d landmarks to %s (sigma^2 = %.6e, %d degenerate)" % (n, ply, st.sigma2, st.n_degenerate)
    r = subprocess.run([str(SBA_MAIN), *args, "--structure", str(ply)], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--structure needs --joint" in r.stdout and "d-only" not in r.stdout
