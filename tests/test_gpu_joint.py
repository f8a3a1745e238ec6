"""GPU: the joint solve -- depths, rotation and translation free together (Problem.eval_joint / solve_joint,
sba_problem_eval_joint / sba_problem_solve_joint; kernels csrc/sba_joint.hip).

eval_joint is checked against the existing RT sweep and the oracle (unreduced camera block) and against the long-double
element-wise Schur complement of tests/ref_joint_numpy.py (reduced system); solve_joint against the dense restatement and
against the product's own step logic driven by numpy-emulated passes (tests/test_joint_solver_cpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import ref_joint_numpy as rj
from helpers import REL_TOL_F64, ROOT, RT_TOL_F32, RT_TOL_F64
from joint_emulation import EmulatedJoint, drive
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api, synthetic

pytestmark = pytest.mark.gpu

STORES = (api.STORE_F64, api.STORE_F32)
RADII = (float("inf"), 1e4, 1.0, 1e-2)
SIZES = (1, 2, 3, 255, 256, 257, 4097, 100_001)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _planes(c, store):
    """What the planes hold: f32 planes are the f32-rounded inputs."""
    if store == api.STORE_F64:
        return c.x1, c.x2
    return c.x1.astype(np.float32).astype(np.float64), c.x2.astype(np.float32).astype(np.float64)


def _scene(n, seed=0, **kw):
    args = dict(sigma=1e-3, outlier_fraction=0.1, depth_noise=0.05)
    args.update(kw)
    return synthetic.full_rt(n, seed=synthetic.BASE_SEED + 70 + seed, **args)


@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 257, 4097, 100_001])
def test_eval_joint_unreduced_block_is_the_rt_sweep(oracle, n, store):
    c = _scene(n)
    x1, x2 = _planes(c, store)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12, store=store)
        got = p.eval_joint(c.rot_init, c.tran_init)
        for kind in (api.KERNEL_FACTORED, api.KERNEL_EXPLICIT):
            p.set_kernel(kind)
            ne = p.eval(api.MODE_RT, c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH)
            for ref in (ne, oracle.evaluate(api.MODE_RT, x1, x2, c.rot_init, c.tran_init, delta=1.0, d12=c.d12)):
                assert np.abs(got.V - ref.H).max() <= REL_TOL_F64 * np.abs(ref.H).max()
                assert np.abs(got.gc - ref.g).max() <= REL_TOL_F64 * max(np.abs(ref.g).max(), np.abs(ref.H).max())
                assert abs(got.cost - ref.cost) <= REL_TOL_F64 * ref.cost
                assert abs(got.sum_w - ref.sum_w) <= REL_TOL_F64 * ref.sum_w
                assert got.n_outlier == ref.n_outlier
        r = p.residuals(c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH, fields=())
        assert got.n_outlier == n - r.n_inlier


def _check_reduced(p, c, x1, x2, radius, what, schur=rj.schur_longdouble):
    """schur: what forms the reference system; tests/test_gpu_reference_pin.py forms it from the reference's own blocks."""
    got = p.eval_joint(c.rot_init, c.tran_init, radius)
    ref = schur(x1, x2, c.rot_init, c.tran_init, c.d12, radius)
    f64 = schur(x1, x2, c.rot_init, c.tran_init, c.d12, radius, dt=np.float64)
    scale = float(np.abs(ref["V"]).max())
    err_S = float(np.abs(got.S - ref["S"]).max()) / scale
    err_g = float(np.abs(got.gs - ref["gs"]).max()) / max(scale, float(np.abs(ref["gc"]).max()))
    own = float(np.abs(f64["S"] - ref["S"]).max()) / scale      # float64 numpy against long double, same inputs
    print(f"{what} radius={radius:g}: S err {err_S:.3e}, gs err {err_g:.3e} (relative to max |V| = {scale:.3e}); numpy f64 vs long double {own:.3e}")
    assert err_S <= REL_TOL_F64 and err_g <= REL_TOL_F64
    assert abs(got.gd_max - float(ref["gd_max"])) <= REL_TOL_F64 * max(float(ref["gd_max"]), 1.0)
    assert np.array_equal(got.S, got.S.T)


@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_eval_joint_reduced_system(n, store):
    c = _scene(n, seed=1)
    x1, x2 = _planes(c, store)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12, store=store)
        for radius in RADII:
            _check_reduced(p, c, x1, x2, radius, f"n={n} store={store}")


@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
@pytest.mark.parametrize("steps", [1, 3])
def test_eval_joint_reduced_system_over_grid_stride_steps(monkeypatch, steps, store):
    """One block per CU: with 2 * 256 * CUs matches per step every lane runs `steps` steps, the last one ragged."""
    monkeypatch.setenv("SBA_JOINT_BLOCKS_PER_CU", "1")
    n = 512 * _cus() * steps - 515
    c = _scene(n, seed=2)
    x1, x2 = _planes(c, store)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12, store=store)
        for radius in RADII:
            _check_reduced(p, c, x1, x2, radius, f"steps={steps} n={n} store={store}")
        rot, tran, d, s = p.solve_joint(c.rot_init, c.tran_init)
        assert s.final_cost < s.initial_cost and np.isfinite(d).all()


def test_determinism():
    c = _scene(50_001, seed=3)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12)
        a, b = p.eval_joint(c.rot_init, c.tran_init, 10.0), p.eval_joint(c.rot_init, c.tran_init, 10.0)
        for k in ("S", "gs", "V", "gc"):
            assert np.array_equal(getattr(a, k), getattr(b, k))
        assert (a.cost, a.sum_w, a.n_outlier, a.gd_max) == (b.cost, b.sum_w, b.n_outlier, b.gd_max)
        r1 = p.solve_joint(c.rot_init, c.tran_init)
        p.set_depths(c.d12)
        r2 = p.solve_joint(c.rot_init, c.tran_init)
        assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1]) and np.array_equal(r1[2], r2[2])
        assert (r1[3].final_cost, r1[3].num_iterations, r1[3].num_evaluations) == (r2[3].final_cost, r2[3].num_iterations, r2[3].num_evaluations)


@pytest.mark.parametrize("store,tol", [(api.STORE_F64, RT_TOL_F64), (api.STORE_F32, RT_TOL_F32)], ids=["f64", "f32"])
@pytest.mark.parametrize("n,seed,sigma,outliers", [(300, 4, 1e-3, 0.1), (200, 5, 0.0, 0.0), (257, 6, 2e-3, 0.1)])
def test_solve_joint_matches_dense_and_the_driven_solver(n, seed, sigma, outliers, store, tol):
    c = _scene(n, seed=seed, sigma=sigma, outlier_fraction=outliers)
    x1, x2 = _planes(c, store)
    rr, tr, dr, sr = rj.dense_solve(x1, x2, c.rot_init, c.tran_init, c.d12)
    assert sr["margin"] >= 1e-3, sr
    hr, ht, hd, hs, hstatus, _, _ = drive(EmulatedJoint(x1, x2, c.d12), c.rot_init, c.tran_init)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12, store=store)
        rot, tran, d, s = p.solve_joint(c.rot_init, c.tran_init)
        assert (s.termination.replace("CONVERGENCE_", "").lower(), s.num_iterations, s.num_successful_steps, s.num_evaluations) == \
            (sr["termination"], sr["num_iterations"], sr["num_successful_steps"], sr["num_evaluations"])
        assert (s.num_iterations, s.num_successful_steps, s.num_evaluations) == (hs.num_iterations, hs.num_successful_steps, hs.num_evaluations)
        assert cabi.TERMINATION[hs.termination] == s.termination and hstatus == 0
        for ref_r, ref_t, ref_d in ((rr, tr, dr), (hr, ht, hd)):
            assert np.abs(rot - ref_r).max() <= tol and np.abs(tran - ref_t).max() <= tol
            assert np.abs(d - ref_d).max() <= tol * np.abs(ref_d).max()
        # monotone, and the reported final cost is the cost at the returned point
        assert s.final_cost <= s.initial_cost
        r = p.residuals(rot, tran, depth_mode=api.DEPTH_PER_MATCH, fields=("sq_norm",))
        rho = np.where(r.sq_norm > 1.0, 2.0 * np.sqrt(r.sq_norm) - 1.0, r.sq_norm)
        assert abs(0.5 * rho.sum() - s.final_cost) <= REL_TOL_F64 * max(s.final_cost, 1e-300) + 1e-24


def test_joint_refines_the_staged_pipeline():
    n = 4096
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 9, sigma=2e-4, outlier_fraction=0.02)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, np.full((n, 2), 6.0))
        e, t, _ = p.initial_guess(80, 0.25, 0)
        rot0, tran0 = -e, t
        d, _ = p.solve_depths(rot0, tran0)
        r1, t1, _ = p.solve(api.MODE_ROT, rot0, tran0, d[0, 0], d[1, 0])
        r2, t2, _ = p.solve(api.MODE_TRAN, r1, t1, d[0, 0], d[1, 0])
        staged = p.eval_joint(r2, t2)
        rot, tran, dj, s = p.solve_joint(r2, t2)
        assert s.initial_cost == staged.cost
        assert s.final_cost < s.initial_cost and s.num_successful_steps >= 1
        assert abs(np.linalg.norm(tran) - np.linalg.norm(t2)) <= 1e-12 * np.linalg.norm(t2)
        print(f"staged cost {staged.cost:.6e} -> joint {s.final_cost:.6e} ({s.termination}, {s.num_iterations} iterations)")


@pytest.mark.parametrize("folding", [True, False], ids=["folded", "raw"])
def test_state_after_solve_joint(monkeypatch, folding):
    monkeypatch.setenv("SBA_BLOCKS_PER_CU", "2")       # same sweep grid on every handle: packs compare bit for bit
    c = _scene(5001, seed=7)
    with api.Problem(0) as p, api.Problem(0) as q:
        p.set_folding(folding); q.set_folding(folding)
        p.upload(c.x1, c.x2, c.d12)
        rot, tran, d, s = p.solve_joint(c.rot_init, c.tran_init)
        assert s.num_successful_steps >= 1 and not np.array_equal(d, c.d12)
        q.upload(c.x1, c.x2, d)
        a = p.eval_pack(api.MODE_RT, rot, tran, depth_mode=api.DEPTH_PER_MATCH)
        b = q.eval_pack(api.MODE_RT, rot, tran, depth_mode=api.DEPTH_PER_MATCH)
        assert np.array_equal(a, b)
        # keep the inliers, solve again == a fresh upload of the kept rows solved once
        # (with its two depths free a gross outlier keeps a residual along one direction only: after the joint solve hardly
        # any match is left outside Huber's region at delta = 1, so the inlier threshold is taken from the residuals)
        sq = p.residuals(rot, tran, depth_mode=api.DEPTH_PER_MATCH, fields=("sq_norm",)).sq_norm
        delta = float(np.sqrt(np.quantile(sq, 0.8)))
        kept = p.keep_inliers(rot, tran, huber_delta=delta, depth_mode=api.DEPTH_PER_MATCH)
        assert 0 < len(kept) < 5001
        q.upload(c.x1[kept], c.x2[kept], d[kept])
        again, fresh = p.solve_joint(rot, tran), q.solve_joint(rot, tran)
        for u, v in zip(again[:3], fresh[:3]):
            assert np.array_equal(u, v)
        assert again[3].final_cost == fresh[3].final_cost and again[3].num_evaluations == fresh[3].num_evaluations


def test_errors():
    c = _scene(100, seed=8)
    lib = cabi.load_library()
    with api.Problem(0) as p:
        with pytest.raises(api.SbaError) as ei:
            p.solve_joint(c.rot_init, c.tran_init)
        assert ei.value.code == cabi.SBA_ERR_NOT_UPLOADED
        p.upload(c.x1, c.x2)                              # no per-match depths
        for call in (lambda: p.solve_joint(c.rot_init, c.tran_init), lambda: p.eval_joint(c.rot_init, c.tran_init)):
            with pytest.raises(api.SbaError) as ei:
                call()
            assert ei.value.code == cabi.SBA_ERR_UNSUPPORTED
        p.set_depths(c.d12)                               # ... unless set_depths was called
        before = p.eval_joint(c.rot_init, c.tran_init)
        assert np.isfinite(before.cost)
        # NULL outputs
        rot, tran = c.rot_init.copy(), c.tran_init.copy()
        dp = lambda a: a.ctypes.data_as(cabi._dp)
        assert lib.sba_problem_eval_joint(p._h, dp(rot), dp(tran), 1.0, None, None) == cabi.SBA_ERR_INVALID_ARG
        assert lib.sba_problem_solve_joint(p._h, None, dp(tran), None, None, None) == cabi.SBA_ERR_INVALID_ARG
        assert lib.sba_problem_eval_joint(p._h, dp(rot), dp(tran), -1.0, None, C.byref(cabi.JointEq())) == cabi.SBA_ERR_INVALID_ARG
        # non-finite start: SBA_ERR_NUMERIC, the handle stays usable and its depths are unchanged -- observed on the handle
        # itself right after the failed call, with no set_depths in between
        bad = c.rot_init.copy(); bad[1] = np.nan
        with pytest.raises(api.SbaError) as ei:
            p.solve_joint(bad, c.tran_init)
        assert ei.value.code == cabi.SBA_ERR_NUMERIC
        after = p.eval_joint(c.rot_init, c.tran_init)
        for k in ("S", "gs", "V", "gc"):
            assert np.array_equal(getattr(after, k), getattr(before, k))
        assert (after.cost, after.sum_w, after.gd_max) == (before.cost, before.sum_w, before.gd_max)
        nan_d = c.d12.copy(); nan_d[3, 0] = np.nan
        p.set_depths(nan_d)
        e_before = p.residuals(c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH, fields=("e",)).e
        assert np.isnan(e_before[3]).all() and np.isfinite(np.delete(e_before, 3, axis=0)).all()
        with pytest.raises(api.SbaError) as ei:
            p.solve_joint(c.rot_init, c.tran_init)
        assert ei.value.code == cabi.SBA_ERR_NUMERIC
        e_after = p.residuals(c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH, fields=("e",)).e
        assert np.array_equal(e_before, e_after, equal_nan=True)       # every match's depths as uploaded, the NaN one included
        p.set_depths(c.d12)
        after = p.eval_joint(c.rot_init, c.tran_init)
        assert after.cost == before.cost and np.array_equal(after.S, before.S)
        # summary and d12_out may be NULL
        assert lib.sba_problem_solve_joint(p._h, dp(rot), dp(tran), None, None, None) == cabi.SBA_OK
        # sharded / hooked handles
        p.set_depths(c.d12)
        p.set_shard(0, 2)
        with pytest.raises(api.SbaError) as ei:
            p.solve_joint(c.rot_init, c.tran_init)
        assert ei.value.code == cabi.SBA_ERR_UNSUPPORTED
        p.set_shard(0, 1)
        p.set_allreduce(lambda buf, count, stream: 0)
        with pytest.raises(api.SbaError) as ei:
            p.eval_joint(c.rot_init, c.tran_init)
        assert ei.value.code == cabi.SBA_ERR_UNSUPPORTED
        p.set_allreduce(None)
        assert p.eval_joint(c.rot_init, c.tran_init).cost == before.cost


def test_explicit_free_translation_runs_the_functor_as_written():
    c = _scene(2000, seed=9, outlier_fraction=0.0)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12)
        rot, tran, d, s = p.solve_joint(c.rot_init, c.tran_init, options=api.default_lm_options(tran_param=api.TRAN_FREE))
        assert s.final_cost < s.initial_cost and np.linalg.norm(tran) < np.linalg.norm(c.tran_init)
        p.set_depths(c.d12)
        rot, tran, d, s = p.solve_joint(c.rot_init, c.tran_init)      # default: |tran| pinned
        assert abs(np.linalg.norm(tran) - np.linalg.norm(c.tran_init)) <= 1e-12


def test_full_size_properties():
    n = 10_000_000
    c = synthetic.full_rt(n, depth_noise=0.02)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12)
        a = p.eval_joint(c.rot_init, c.tran_init, 1e4)
        b = p.eval_joint(c.rot_init, c.tran_init, 1e4)
        assert np.array_equal(a.S, b.S) and np.array_equal(a.gs, b.gs) and np.array_equal(a.V, b.V) and a.cost == b.cost
        assert np.isfinite(a.S).all() and np.isfinite(a.gs).all() and np.isfinite(a.gd_max)
        ne = p.eval(api.MODE_RT, c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH)
        assert np.abs(a.V - ne.H).max() <= REL_TOL_F64 * np.abs(ne.H).max() and a.n_outlier == ne.n_outlier
        rot, tran, _, s = p.solve_joint(c.rot_init, c.tran_init, return_depths=False)
        assert np.isfinite(rot).all() and np.isfinite(tran).all() and np.isfinite(s.final_cost)
        assert s.final_cost <= s.initial_cost and s.initial_cost == a.cost and s.num_successful_steps >= 1
        print(f"10^7: {s.termination} after {s.num_iterations} iterations / {s.num_evaluations} passes, "
              f"{s.seconds_total * 1e3:.1f} ms, cost {s.initial_cost:.6e} -> {s.final_cost:.6e}")


@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
@pytest.mark.parametrize("rot", [(0.0, 0.0, 0.0), (3e-9, -2e-9, 1e-9)], ids=["zero", "below_eps"])
def test_small_angle_frame(oracle, rot, store):
    """rot.rot <= DBL_EPSILON (the natural start rot = 0) takes the kernels' small-angle frame: a = -d1 x1, J = I."""
    c = _scene(4097, seed=10)
    rot = np.array(rot)
    x1, x2 = _planes(c, store)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12, store=store)
        got = p.eval_joint(rot, c.tran_init, 1e4)
        p.set_kernel(api.KERNEL_EXPLICIT)
        for ref in (p.eval(api.MODE_RT, rot, c.tran_init, depth_mode=api.DEPTH_PER_MATCH),
                    oracle.evaluate(api.MODE_RT, x1, x2, rot, c.tran_init, delta=1.0, d12=c.d12)):
            assert np.abs(got.V - ref.H).max() <= REL_TOL_F64 * np.abs(ref.H).max()
            assert np.abs(got.gc - ref.g).max() <= REL_TOL_F64 * max(np.abs(ref.g).max(), np.abs(ref.H).max())
            assert got.n_outlier == ref.n_outlier
        for radius in RADII:
            c0 = type(c)(c.x1, c.x2, c.d12, c.rot_true, c.tran_true, rot, c.tran_init)
            _check_reduced(p, c0, x1, x2, radius, f"small angle {rot} store={store}")
        r, t, d, s = p.solve_joint(rot, c.tran_init)
        assert s.final_cost < s.initial_cost and s.num_successful_steps >= 1


# ---- mirror class / CLI: set_joint_refinement, sba_main --joint ---------------------------------------------------------
SBA_MAIN = ROOT / "spherical_bundle_adjuster_amd" / "csrc" / "build" / "sba_main"


def _g(v):
    """A double as a C++ ostream prints it by default (%g, six significant digits)."""
    return "%g" % v


def _cli_fixture(tmp_path):
    """The key-point files of tests/test_gpu_pipeline.py's three-stage fixture (config C1) and the CLI arguments after the program."""
    W, H, n = 3840, 1920, 2048
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED, sigma=2e-4, outlier_fraction=0.02)
    kps = []
    for name, x in (("left.kp", c.x1), ("right.kp", c.x2)):
        colat = np.arccos(np.clip(x[:, 2], -1, 1))
        lon = np.mod(np.arctan2(x[:, 1], x[:, 0]), 2 * np.pi)
        kp = np.zeros((n, 7), dtype=np.float32)
        kp[:, 0], kp[:, 1] = lon / (2 * np.pi) * W, colat / np.pi * H
        with open(tmp_path / name, "wb") as f:
            np.array([n, W, H, 0], dtype=np.int32).tofile(f)
            kp.tofile(f)
        kps.append(kp)
    deg = np.rad2deg(c.rot_init)
    args = [str(tmp_path / "left.kp"), str(tmp_path / "right.kp"), *(f"{v:.17g}" for v in deg), *(f"{v:.17g}" for v in c.tran_init), "6"]
    return c, kps, deg, args, (W, H, n)


def _run_cli(tmp_path, args):
    for f in ("log.txt", "log_d.txt"):
        if (tmp_path / f).exists():
            (tmp_path / f).unlink()
    r = subprocess.run([str(SBA_MAIN), *args], cwd=tmp_path, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, SBA_INITIAL_GUESS="0"))
    assert r.returncode == 0, r.stderr + r.stdout
    return r.stdout, (tmp_path / "log.txt").read_text(), (tmp_path / "log_d.txt").read_text()


def _row(deg, rot, tran, n):
    return ",".join([*(_g(v) for v in deg), *(_g(v / np.pi * 180.0) for v in rot), *(_g(v) for v in tran), str(n)]) + "\n"


def test_cli_joint_switch(tmp_path):
    """Without --joint the run is the three stages and nothing else: no joint line, and log.txt / log_d.txt are, byte for
    byte, the staged result of the same library calls.  With --joint (anywhere on the line) the logged pose and depths
    are Problem.solve_joint from that staged result."""
    c, (kl, kr), deg, args, (W, H, n) = _cli_fixture(tmp_path)
    rot0 = np.array([float(a) for a in args[2:5]]) / 180 * 3.14159265358979323846      # as the mirror class converts them
    with api.Problem(0) as p:
        p.upload_keypoints(kl, kr, W, H)
        p.set_depths(np.full((n, 2), 6.0))
        d, _ = p.solve_depths(rot0, c.tran_init)
        r1, t1, _ = p.solve(api.MODE_ROT, rot0, c.tran_init, d[0, 0], d[1, 0])
        r2, t2, _ = p.solve(api.MODE_TRAN, r1, t1, d[0, 0], d[1, 0])
        rj_, tj, dj, sj = p.solve_joint(r2, t2)
    assert sj.num_successful_steps >= 1 and sj.final_cost < sj.initial_cost
    depth_text = lambda dd: "".join(f"{_g(a)},{_g(b)}\n" for a, b in dd)

    out_off, log_off, logd_off = _run_cli(tmp_path, args)
    assert "joint" not in out_off and "tran-only: iterations" in out_off
    assert log_off == _row(deg, r2, t2, n)
    assert logd_off == depth_text(d)

    for where in (0, len(args)):
        a = list(args)
        a.insert(where, "--joint")
        out_on, log_on, logd_on = _run_cli(tmp_path, a)
        assert f"joint: iterations {sj.num_iterations}," in out_on
        assert log_on == _row(deg, rj_, tj, n) and log_on != log_off
        assert logd_on == depth_text(dj)
        assert abs(np.linalg.norm(tj) - np.linalg.norm(t2)) <= 1e-12
    # the lines before the joint stage do not depend on the switch (timings masked)
    import re
    mask = lambda t: re.sub(r"[0-9.]+ ms", "ms", t)
    assert mask(out_on).startswith(mask(out_off).split("expected rotation vector")[0])
