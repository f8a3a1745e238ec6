"""GPU: the resection weighted by landmark covariances (Problem.set_landmark_covariances / freeze_resection_weights /
resection_weights / eval_resection_weighted / solve_resection_weighted / resection_covariance) against the long-double closed form
of tests/resection_weighted_reference.py, on the cases tests/test_resection_weighted_host_cpu.py qualifies (float64 numpy in the
product's formulation meets the same bounds there, and no match sits on the Huber threshold): the vector-per-lane and block
edges of both plane types, several grid-stride steps (SBA_RESECT_GRID=1), with and without the loss, the evaluation pose off the
reference pose, with and without the bearing's noise, the rotations where the frame changes; the stored weights per match; the
zero-weight rules; the isotropic case against the unweighted pass; the solve against the harness-driven LM with the numpy
evaluator; the pose covariance; what drops the covariances and what does not; refusals; the device-pointer path."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import resection_reference as rr
import resection_weighted_reference as wr
from helpers import REL_TOL_F32, REL_TOL_F64, RT_TOL_F32, RT_TOL_F64, assert_normal_eq_close
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api, synthetic

pytestmark = pytest.mark.gpu

STORES = [api.STORE_F64, api.STORE_F32]
IDS = ["f64", "f32"]
TERMINATION = {v: k for k, v in cabi.TERMINATION.items()}
TIGHT = dict(function_tolerance=1e-30, parameter_tolerance=1e-13, gradient_tolerance=1e-13, max_num_iterations=100)
PER_MATCH = dict(depth_mode=api.DEPTH_PER_MATCH)


def _rel(store):
    return REL_TOL_F64 if store == api.STORE_F64 else REL_TOL_F32


def _rt(store):
    return RT_TOL_F64 if store == api.STORE_F64 else RT_TOL_F32


@lru_cache(maxsize=None)
def _row_bound():
    """8 times the worst error of the float64 numpy basis form against long double on the same cases, measured in this run
    (the device orders the operations differently and fuses multiply-adds)."""
    from test_resection_weighted_host_cpu import measured_row_error
    return 8.0 * measured_row_error()


def _bytes(*arrays):
    return b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in arrays)


def _eq_bytes(e):
    return _bytes(e.H, e.g, [e.cost, e.sum_w, e.n_outlier, e.n_behind])


def _check(got, ref, rel, what):
    assert_normal_eq_close(got, ref, rel, what)
    assert (got.n_outlier, got.n_behind) == (ref.n_outlier, ref.n_behind), what
    assert abs(got.sum_w - ref.sum_w) <= rel * max(ref.sum_w, 1e-300), what
    assert np.array_equal(got.H, got.H.T), what
    assert np.isfinite(got.H).all() and np.isfinite(got.g).all() and np.isfinite(got.cost), what


def _load(p, c, store, cov_scale=wr.COV_SCALE):
    """Upload a case, set its covariances and freeze at its reference pose; -> n_zero_weight."""
    p.upload_landmarks(c.scene.X, c.scene.y, store=store)
    p.set_landmark_covariances(c.cov, cov_scale)
    return p.freeze_resection_weights(c.rot_w, c.tran_w, c.bearing_sigma)


def _run_case(p, c, store):
    f32 = store == api.STORE_F32
    assert _load(p, c, store) == 0, c.name
    got = p.eval_resection_weighted(c.rot, c.tran, api.default_lm_options(huber_delta=c.delta))
    ref, M, _ = wr.case_reference(c, f32)
    _check(got, ref, _rel(store), c.name)
    n = len(c.scene.X)
    if c.delta == 0.0 and n > 0:
        assert got.sum_w == n and got.n_outlier == 0, c.name
    if c.delta > 0 and n >= 63:
        assert got.n_outlier >= 1 and got.sum_w < n, c.name
    rows = p.resection_weights()
    assert rows.shape == (n, 6)
    err = wr.row_error(rows, M)
    assert err <= _row_bound(), f"{c.name}: M row error {err:.3e}, bound {_row_bound():.3e}"
    return err


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_eval_and_weights_against_long_double(store):
    worst = 0.0
    with api.Problem(0) as p:
        for c in wr.eval_cases(store == api.STORE_F32):
            if not c.grid_one:
                worst = max(worst, _run_case(p, c, store))
    print(f"worst device M row error {worst:.3e}, bound {_row_bound():.3e}")


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_eval_over_several_grid_stride_steps(monkeypatch, store):
    monkeypatch.setenv("SBA_RESECT_GRID", "1")
    with api.Problem(0) as p:
        for c in wr.eval_cases(store == api.STORE_F32):
            if c.grid_one:
                _run_case(p, c, store)


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_eval_at_the_pose_edges(store):
    with api.Problem(0) as p:
        for c in wr.edge_cases():
            _run_case(p, c, store)


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_two_freezes_return_identical_bytes_for_any_grid(monkeypatch, store):
    c = wr.eval_cases(store == api.STORE_F32)[-1]           # n = 3073
    with api.Problem(0) as p:
        seen = []
        for grid in (None, "1", None):
            if grid is None:
                monkeypatch.delenv("SBA_RESECT_GRID", raising=False)
            else:
                monkeypatch.setenv("SBA_RESECT_GRID", grid)
            assert _load(p, c, store) == 0
            first = p.resection_weights().tobytes()
            assert p.freeze_resection_weights(c.rot_w, c.tran_w, c.bearing_sigma) == 0
            assert p.resection_weights().tobytes() == first
            seen.append(first)
        assert seen[0] == seen[1] == seen[2]                # no reduction in the freeze: the grid does not matter
        e1 = p.eval_resection_weighted(c.rot, c.tran, api.default_lm_options(huber_delta=c.delta))
        e2 = p.eval_resection_weighted(c.rot, c.tran, api.default_lm_options(huber_delta=c.delta))
        assert _eq_bytes(e1) == _eq_bytes(e2)


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_zero_weight(store):
    f32 = store == api.STORE_F32
    n = 67
    s = wr.eval_scene(n, True)
    cov, _ = wr.landmark_cov(s.X, n)
    cov = cov.copy()
    cov[3] = [np.inf, np.inf, np.inf, 0, 0, 0]              # the structure's degenerate row
    cov[10, 4] = np.nan
    cov[20] = 0.0                                           # no weight without bearing noise
    cov[30, :3] = -cov[30, :3]                              # a negative variance
    y = s.y.copy()
    y[40] = 0.0                                             # a zero bearing: d* is not finite
    rw, tw = rr.start_near(s, n + 1000, 0.004, 0.004)
    re, te = rr.start_near(s, n, 0.002, 0.002)
    X32, _ = rr.planes(s, f32)
    y32 = y.astype(np.float32).astype(np.float64) if f32 else y
    opt = api.default_lm_options(huber_delta=wr.DELTA)
    with api.Problem(0) as p:
        p.upload_landmarks(s.X, y, store=store)
        p.set_landmark_covariances(cov, wr.COV_SCALE)
        for bs, dead in ((0.0, [3, 10, 20, 30, 40]), (1e-3, [3, 10, 30, 40])):
            assert p.freeze_resection_weights(rw, tw, bs) == len(dead)
            assert p.freeze_resection_weights(rw, tw, bs) == len(dead)          # an integer: the same on every run
            rows = p.resection_weights()
            assert not rows[dead].any() and np.isfinite(rows).all()
            live = np.setdiff1d(np.arange(n), dead)
            assert (np.abs(rows[live]).max(axis=1) > 0).all()                   # bs > 0: row 20 has weight again
            got = p.eval_resection_weighted(re, te, opt)
            Xk, yk, ck = X32[live], y32[live], cov[live]
            M, zero = wr.info_matrices(Xk, yk, ck, rw, tw, wr.COV_SCALE, bs)
            assert not zero.any()
            ref = wr.sums(Xk, yk, M, zero, re, te, wr.DELTA)
            _check(got, ref, _rel(store), f"zero weight bs={bs}")
            assert wr.row_error(rows[live], M) <= _row_bound()
            cv = p.resection_covariance(re, te, opt)
            assert (cv.n_zero_weight, cv.n_used, cv.dof) == (len(dead), n - len(dead), 2 * (n - len(dead)) - 6)


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_isotropic_covariances_reduce_to_the_unweighted_pass(store):
    sigma2 = 0.05 ** 2
    opt = api.default_lm_options(huber_delta=0.0)
    with api.Problem(0) as p:
        for n in (65, 513):
            s = wr.eval_scene(n, False)                     # unit bearings
            rot, tran = rr.start_near(s, n, 0.002, 0.002)
            p.upload_landmarks(s.X, s.y, store=store)
            plain = p.eval_resection(rot, tran, opt)
            p.set_landmark_covariances(np.tile([sigma2, sigma2, sigma2, 0.0, 0.0, 0.0], (n, 1)), wr.COV_SCALE)
            assert p.freeze_resection_weights(s.rot, s.tran, 0.0) == 0
            got = p.eval_resection_weighted(rot, tran, opt)
            k = 1.0 / (wr.COV_SCALE * sigma2)
            ref = rr.Sums(plain.H * k, plain.g * k, plain.cost * k, plain.sum_w, plain.n_outlier, plain.n_behind)
            _check(got, ref, _rel(store), f"isotropic n={n}")


@pytest.mark.parametrize("store", STORES, ids=IDS)
@pytest.mark.parametrize("rounds", [1, 3])
@pytest.mark.parametrize("n,seed", wr.SOLVE_SCENES)
def test_solve_equals_the_harness_driven_solver_and_the_covariance(n, seed, rounds, store):
    f32 = store == api.STORE_F32
    ns = wr.noisy_scene(n, seed)
    X = ns.X.astype(np.float32).astype(np.float64) if f32 else ns.X
    y = ns.y.astype(np.float32).astype(np.float64) if f32 else ns.y
    r0, t0 = rr.start_near(ns.scene, seed, 0.01, 0.01)
    bs = wr.SOLVE_BEARING_SIGMA
    rh, th, sh, rch = wr.solve_rounds(X, y, ns.cov, r0, t0, wr.COV_SCALE, bs, wr.DELTA, rounds)
    assert rch == 0
    opt = api.default_lm_options(huber_delta=wr.DELTA)
    with api.Problem(0) as p:
        p.upload_landmarks(ns.X, ns.y, store=store)
        p.set_landmark_covariances(ns.cov, wr.COV_SCALE)
        r, t, sm, nb = p.solve_resection_weighted(r0, t0, opt, bearing_sigma=bs, reweight_rounds=rounds)
        assert (TERMINATION[sm.termination], sm.num_iterations, sm.num_successful_steps, sm.num_evaluations) == \
               (sh.termination, sh.num_iterations, sh.num_successful_steps, sh.num_evaluations)
        assert np.abs(r - rh).max() <= _rt(store) and np.abs(t - th).max() <= _rt(store)
        assert abs(sm.final_cost - sh.final_cost) <= 10 * _rel(store) * sh.final_cost
        # store_depths: the handle's d2 plane holds the eliminated depths at the result
        _, dref, _, _, _ = rr.per_match(X, y, r, t)
        d12 = p.solve_joint(r, t, options=api.default_lm_options(max_num_iterations=0, tran_param=api.TRAN_SPHERE))[2]
        assert np.abs(d12[:, 1] - dref.astype(np.float64)).max() <= _rel(store) * np.abs(X).max()
        assert nb == float((dref <= 0).sum())
        # the pose covariance with the weights re-frozen at the result
        assert p.freeze_resection_weights(r, t, bs) == 0
        cv = p.resection_covariance(r, t, opt)
        M, zero = wr.info_matrices(X, y, ns.cov, r, t, wr.COV_SCALE, bs)
        ref = wr.sums(X, y, M, zero, r, t, wr.DELTA)
        want = wr.inverse_ld(ref.H).astype(np.float64)
        cond = float(np.linalg.cond(ref.H))
        for name, blk in (("rot", np.s_[:3, :3]), ("tran", np.s_[3:, 3:]), ("cross", np.s_[:3, 3:])):
            err = np.abs(cv.cov[blk] - want[blk]).max() / np.abs(want[blk]).max()
            assert err <= _rel(store) * cond, f"{name} block: rel err {err:.3e}, cond(H) {cond:.3e}, bound {_rel(store) * cond:.3e}"
        assert np.array_equal(cv.cov, cv.cov.T)
        assert (cv.n_used, cv.n_zero_weight, cv.dof, cv.n_outlier) == (n, 0, 2 * n - 6, ref.n_outlier)
        assert abs(cv.cost - ref.cost) <= _rel(store) * ref.cost and cv.sigma2 == 2 * cv.cost / cv.dof
        assert 0.5 < cv.sigma2 < 2.0                        # honest covariances: near 1 (the Huber loss trims it a little)
        # the weighted pose is the better one
        ru, tu, _, _ = p.solve_resection(r0, t0, api.default_lm_options(huber_delta=0.0), store_depths=False)
        if n >= 513:
            assert np.linalg.norm(r - ns.scene.rot) < np.linalg.norm(ru - ns.scene.rot)


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_solve_returns_the_truth_on_noise_free_scenes(store):
    opt = api.default_lm_options(huber_delta=wr.DELTA, **TIGHT)
    with api.Problem(0) as p:
        for n in (6, 65, 513):
            s = rr.make_scene(n, 100 + n)
            cov, _ = wr.landmark_cov(s.X, n)
            p.upload_landmarks(s.X, s.y, store=store)
            p.set_landmark_covariances(cov, wr.COV_SCALE)
            r0, t0 = rr.start_near(s, n, 0.01, 0.01)
            for rounds in (1, 3):
                r, t, sm, nb = p.solve_resection_weighted(r0, t0, opt, bearing_sigma=1e-3, reweight_rounds=rounds)
                assert np.abs(r - s.rot).max() <= _rt(store) and np.abs(t - s.tran).max() <= _rt(store), (n, rounds, sm)
                assert nb == 0 and sm.final_cost <= sm.initial_cost
            assert np.abs(p.resection_depths(r, t) - s.depth).max() <= 100 * _rt(store)


def _weighted_calls(p, c):
    opt = api.default_lm_options(huber_delta=c.delta)
    return {
        "freeze": lambda: p.freeze_resection_weights(c.rot_w, c.tran_w, c.bearing_sigma),
        "weights": lambda: p.resection_weights(),
        "eval": lambda: p.eval_resection_weighted(c.rot, c.tran, opt),
        "solve": lambda: p.solve_resection_weighted(c.rot, c.tran, opt, bearing_sigma=c.bearing_sigma, store_depths=False),
        "covariance": lambda: p.resection_covariance(c.rot, c.tran, opt),
    }


def _refused(code, calls, which=None):
    for name, call in calls.items():
        if which is None or name in which:
            with pytest.raises(api.SbaError) as ei:
                call()
            assert ei.value.code == code, name


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_what_drops_the_covariances_and_what_does_not(store):
    c = [k for k in wr.eval_cases(store == api.STORE_F32) if k.name == "n=513 delta=2.0 bs=0.001"][0]
    s, n = c.scene, 513
    opt = api.default_lm_options(huber_delta=c.delta)
    with api.Problem(0) as p:
        calls = _weighted_calls(p, c)
        p.upload_landmarks(s.X, s.y, store=store)
        _refused(cabi.SBA_ERR_UNSUPPORTED, calls)                               # nothing set yet
        p.set_landmark_covariances(c.cov, wr.COV_SCALE)
        _refused(cabi.SBA_ERR_UNSUPPORTED, calls, ("weights", "eval", "covariance"))      # set, not frozen
        assert calls["freeze"]() == 0
        before = _eq_bytes(calls["eval"]())
        rows = calls["weights"]().tobytes()
        # depth rewrites leave the frozen weights alone
        d = p.resection_depths(c.rot, c.tran)
        assert _eq_bytes(calls["eval"]()) == before
        p.set_depths(np.stack([np.ones(n), d], axis=1))
        assert _eq_bytes(calls["eval"]()) == before and calls["weights"]().tobytes() == rows
        assert np.isfinite(calls["covariance"]().cov).all()
        # setting covariances again discards the frozen weights
        p.set_landmark_covariances(c.cov, wr.COV_SCALE)
        _refused(cabi.SBA_ERR_UNSUPPORTED, calls, ("weights", "eval", "covariance"))
        # every compaction and every upload drops both
        pair = synthetic.full_rt(65, seed=7)                                    # a two-view scene for the structure's cut
        droppers = {"keep_below": lambda: p.keep_below(c.rot, c.tran, 0.9, 1.0, **PER_MATCH),
                    "compact": lambda: p.compact(np.arange(p.size) % 7 != 0),
                    "keep_inliers": lambda: p.keep_inliers(c.rot, c.tran, huber_delta=0.02, **PER_MATCH),
                    "structure_keep_below": lambda: p.structure_keep_below(pair.rot_init, pair.tran_init, 0.5, 4.0),
                    "upload": lambda: p.upload_landmarks(s.X, s.y, store=store)}
        for name, drop in droppers.items():
            if name == "structure_keep_below":
                p.upload(pair.x1, pair.x2, pair.d12, store=store)
            else:
                p.upload_landmarks(s.X, s.y, store=store)
                p.resection_depths(c.rot, c.tran, return_depths=False)          # the per-match residuals are the resection's
            size = p.size
            p.set_landmark_covariances(np.tile([1.0, 1.0, 1.0, 0.0, 0.0, 0.0], (size, 1)))
            assert p.freeze_resection_weights(c.rot_w, c.tran_w, 0.0) == 0
            assert np.isfinite(calls["eval"]().cost)
            drop()
            assert 0 < p.size <= size and (p.size < size or name in ("upload", "structure_keep_below")), name
            _refused(cabi.SBA_ERR_UNSUPPORTED, calls)
            assert np.isfinite(p.eval_resection(c.rot, c.tran, opt).cost)       # the unweighted resection never needed them
        p.upload_landmarks(s.X, s.y, store=store)
        p.set_landmark_covariances(c.cov, wr.COV_SCALE)
        assert calls["freeze"]() == 0
        assert _eq_bytes(calls["eval"]()) == before and calls["weights"]().tobytes() == rows


def test_refusals_leave_the_handle_usable_and_write_nothing():
    c = [k for k in wr.eval_cases(False) if k.name == "n=65 delta=2.0 bs=0.001"][0]
    s, n = c.scene, 65
    opt = api.default_lm_options(huber_delta=c.delta)
    import torch
    with api.Problem(0) as p:
        calls = _weighted_calls(p, c)
        set_cov = {"set": lambda: p.set_landmark_covariances(c.cov, wr.COV_SCALE)}
        _refused(cabi.SBA_ERR_NOT_UPLOADED, {**calls, "set_dev": lambda: p.set_landmark_covariances_device(16, 1.0)})
        p.upload(s.X, s.y)                                                      # no per-match depths: no landmarks
        _refused(cabi.SBA_ERR_UNSUPPORTED, {**calls, "set_dev": lambda: p.set_landmark_covariances_device(16, 1.0)})
        assert _load(p, c, api.STORE_F64) == 0
        before, rows = _eq_bytes(calls["eval"]()), calls["weights"]().tobytes()
        p.set_shard(0, 2)
        _refused(cabi.SBA_ERR_UNSUPPORTED, {**calls, **set_cov})
        p.set_shard(0, 1)
        p.set_allreduce(lambda buf, count, stream: 0)
        _refused(cabi.SBA_ERR_UNSUPPORTED, {**calls, **set_cov})
        p.set_allreduce(None)
        # bad options: SBA_ERR_INVALID_ARG; the covariances and the frozen weights stay as they were
        for scale in (0.0, -1.0, np.nan, np.inf):
            _refused(cabi.SBA_ERR_INVALID_ARG, {"scale": lambda: p.set_landmark_covariances(c.cov, scale)})
        t = torch.zeros(6 * n + 2, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        _refused(cabi.SBA_ERR_INVALID_ARG, {"misaligned": lambda: p.set_landmark_covariances_device(t.data_ptr() + 8, 1.0),
                                            "null": lambda: p.set_landmark_covariances_device(0, 1.0)})
        for bs in (-1e-3, np.nan, np.inf):
            _refused(cabi.SBA_ERR_INVALID_ARG, {"freeze": lambda: p.freeze_resection_weights(c.rot_w, c.tran_w, bs),
                                                "solve": lambda: p.solve_resection_weighted(c.rot, c.tran, opt, bearing_sigma=bs)})
        for rounds in (0, 9, -1):
            _refused(cabi.SBA_ERR_INVALID_ARG, {"solve": lambda: p.solve_resection_weighted(c.rot, c.tran, opt, reweight_rounds=rounds)})
        bad = np.array([0.1, np.nan, 0.0])
        _refused(cabi.SBA_ERR_NUMERIC, {"freeze": lambda: p.freeze_resection_weights(bad, c.tran_w, 0.0),
                                        "eval": lambda: p.eval_resection_weighted(c.rot, bad, opt),
                                        "solve": lambda: p.solve_resection_weighted(bad, c.tran, opt),
                                        "covariance": lambda: p.resection_covariance(np.array([np.inf, 0, 0]), c.tran, opt)})
        assert _eq_bytes(calls["eval"]()) == before and calls["weights"]().tobytes() == rows
        # nothing is written by a refusal (the C entry points directly)
        z3 = (C.c_double * 3)(*c.rot)
        eq, res = cabi.ResectionEq(), cabi.ResectionCov()
        eq.n_behind, res.dof = -7.0, -7
        r3, t3 = (C.c_double * 3)(0.1, float("nan"), 0.0), (C.c_double * 3)(*c.tran)
        lib, h = p._lib, p._h
        assert lib.sba_problem_eval_resection_weighted(h, r3, t3, None, C.byref(eq)) == cabi.SBA_ERR_NUMERIC and eq.n_behind == -7.0
        assert lib.sba_problem_solve_resection_weighted(h, z3, t3, None, 0.0, 9, None, None, 0) == cabi.SBA_ERR_INVALID_ARG
        assert list(z3) == list(c.rot)
        assert lib.sba_problem_resection_covariance(h, r3, t3, None, C.byref(res)) == cabi.SBA_ERR_NUMERIC and res.dof == -7
        # three matches: dof = 0, the covariance is refused, nothing written, the handle stays usable
        p.upload_landmarks(s.X[:3], s.y[:3])
        p.set_landmark_covariances(c.cov[:3], wr.COV_SCALE)
        assert p.freeze_resection_weights(c.rot_w, c.tran_w, 1e-3) == 0
        assert lib.sba_problem_resection_covariance(h, z3, t3, None, C.byref(res)) == cabi.SBA_ERR_NUMERIC and res.dof == -7
        assert np.isfinite(calls["eval"]().cost)
        assert _load(p, c, api.STORE_F64) == 0
        assert _eq_bytes(calls["eval"]()) == before


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_a_third_frame_against_the_structure_of_a_pair_on_the_device(store):
    """A-B through solve_joint, its structure WITH covariances written to device tensors, the rows seen in C gathered with torch and
    handed over by device pointer, C resected with the weights.  Noise-free, so the pair's sigma^2 is at rounding level (floored at
    1e-12 to stay a legal scale) and the bearing's noise carries the weights; the pose comes back in the pair's gauge as in
    tests/test_gpu_resection.py.  The host-pointer path gives the same bytes."""
    import torch
    f = rr.three_frames(513, 71)
    n = 513
    factor = np.linalg.norm(f.tran_ab)
    opt = api.default_lm_options(tran_param=api.TRAN_SPHERE, **TIGHT)
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    t_start = f.tran_ab / factor + 0.02 * axis
    dev = torch.device("cuda", 0)
    with api.Problem(0) as p, api.Problem(0) as q, api.Problem(0) as q2:
        p.upload(f.x1, f.x2, f.d12 / factor * 1.01, store=store)
        rot, tran, d12, sm = p.solve_joint(f.rot_ab + 0.02 * axis, t_start / np.linalg.norm(t_start), options=opt)
        tx = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        tc = torch.zeros((n, 6), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        pose = p.structure_joint_into(tx.data_ptr(), tc.data_ptr(), None, rot, tran, options=opt)
        scale = max(pose.sigma2, 1e-12)
        seen = torch.arange(0, n, 2, device=dev)                                # the rows matched in frame C
        gx, gc = tx.index_select(0, seen).contiguous(), tc.index_select(0, seen).contiguous()
        gy = torch.from_numpy(np.ascontiguousarray(f.y)).to(dev).index_select(0, seen).contiguous()
        ones = torch.ones((len(seen), 2), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        m = len(seen)
        q.upload_device(gx.data_ptr(), gy.data_ptr(), ones.data_ptr(), m, store=store)
        q.set_landmark_covariances_device(gc.data_ptr(), scale)
        g = q.resection_guess()
        lm = api.default_lm_options(huber_delta=wr.DELTA, **TIGHT)
        r, t, sm, nb = q.solve_resection_weighted(g.rot, g.tran, lm, bearing_sigma=1e-3, reweight_rounds=2)
        assert nb == 0
        assert np.abs(r - f.rot_bc).max() <= 100 * _rt(store) and np.abs(t * factor - f.tran_bc).max() <= 100 * _rt(store), sm
        cv = q.resection_covariance(r, t, lm)
        assert cv.n_zero_weight == 0 and np.isfinite(cv.cov).all() and (np.diag(cv.cov) > 0).all()
        # the host-pointer path, byte for byte
        q2.upload(gx.cpu().numpy(), gy.cpu().numpy(), np.ones((m, 2)), store=store)
        q2.set_landmark_covariances(gc.cpu().numpy(), scale)
        r2, t2, sm2, nb2 = q2.solve_resection_weighted(g.rot, g.tran, lm, bearing_sigma=1e-3, reweight_rounds=2)
        assert _bytes(r, t, [sm.final_cost, sm.num_evaluations, nb]) == _bytes(r2, t2, [sm2.final_cost, sm2.num_evaluations, nb2])
        assert q.resection_weights().tobytes() == q2.resection_weights().tobytes()
        assert _bytes(cv.cov, [cv.cost]) == _bytes(q2.resection_covariance(r, t, lm).cov, [cv.cost])
