"""CPU: the covariance-weighted resection on the reference alone and on the product's host side.

The conditions the GPU tests (tests/test_gpu_resection_weighted.py) rest on, over EVERY case they evaluate: float64 numpy in the
product's basis form and its own summation order meets assert_normal_eq_close at REL_TOL_F64 against the long-double closed form
(so the tolerance is reachable), no match sits within 1e-9 delta^2 of delta^2 (so equal outlier counts may be demanded), and
the worst per-match error of the float64 M rows, which times 8 is the GPU test's bound on resection_weights().  The calibration
of the reference itself over 20 seeds.  The host header (csrc/sba_resection_weighted.hpp) through a g++-built harness against
numpy, and once under AddressSanitizer and UBSan in a program of its own."""
import subprocess

import numpy as np
import pytest

import resection_reference as rr
import resection_weighted_reference as wr
from helpers import REL_TOL_F64, ROOT, assert_normal_eq_close

# Worst error of the float64 basis form's M rows against long double over all cases, relative to the largest entry of the row
# (measured 2.2e-12: the 2 x 2 projected covariance has a condition of up to 1e4 at sigma_r / sigma_t = 100).  The GPU bound
# is 8 times the value measured here, in the run itself.
ROW_ERROR_EXPECTED_BELOW = 5e-12


def _all_cases(f32):
    return wr.eval_cases(f32) + wr.edge_cases()


def _qualify(c, f32):
    X, y = wr.case_planes(c, f32)
    ref, M, zero = wr.case_reference(c, f32)
    W, q, zero64 = wr.basis_factor(X, y, c.cov, c.rot_w, c.tran_w, wr.COV_SCALE, c.bearing_sigma)
    got = wr.basis_sums(X, y, W, zero64, c.rot, c.tran, c.delta)
    assert np.array_equal(zero, zero64) and not zero.any(), c.name
    assert_normal_eq_close(got, ref, REL_TOL_F64, c.name)
    assert (got.n_outlier, got.n_behind) == (ref.n_outlier, ref.n_behind), c.name
    assert abs(got.sum_w - ref.sum_w) <= REL_TOL_F64 * max(ref.sum_w, 1e-300), c.name
    if c.delta > 0 and len(X):
        assert np.abs(ref.s - c.delta ** 2).min() > wr.MARGIN * c.delta ** 2, c.name
        if len(X) >= 63:
            planted = len(rr.planted(len(X)))
            assert ref.n_outlier >= planted and ref.sum_w < len(X), c.name      # both Huber branches populated
    return wr.row_error(wr.basis_rows(W), M)


def measured_row_error():
    """The figure the GPU test multiplies by 8 (tests/test_gpu_resection_weighted.py imports this)."""
    return max(_qualify(c, f32) for f32 in (False, True) for c in _all_cases(f32))


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_float64_basis_form_meets_the_bound_and_the_margin_on_every_gpu_case(f32):
    worst = max(_qualify(c, f32) for c in _all_cases(f32))
    print(f"worst float64 row error against long double: {worst:.3e}")
    assert 0 < worst < ROW_ERROR_EXPECTED_BELOW


def test_the_closed_form_is_the_projected_inverse():
    """The reference itself: M y = 0, M S M = M, and r^T M r is the minimum over d of e^T S^-1 e with e = r + d y."""
    c = wr.eval_cases(False)[-1]
    X, y = wr.case_planes(c, False)
    M, zero = wr.info_matrices(X, y, c.cov, c.rot_w, c.tran_w, wr.COV_SCALE, c.bearing_sigma)
    S, _ = wr.frozen_cov(X, y, c.cov, c.rot_w, c.tran_w, wr.COV_SCALE, c.bearing_sigma)
    yl = np.asarray(y, dtype=wr.LD)
    scale = np.abs(M).max(axis=(1, 2))
    assert (np.abs(np.einsum("iab,ib->ia", M, yl)).max(axis=1) <= 1e-15 * scale).all()
    # the products M S M run up to sigma_r^2 / sigma_t^2 = 1e4 times |M| before they cancel: 1e4 * 2^-63 with room to spare
    assert (np.abs(M @ S @ M - M).max(axis=(1, 2)) <= 1e-11 * scale).all()
    _, _, r, _, _ = rr.per_match(X, y, c.rot, c.tran)
    Si = np.linalg.inv(S.astype(np.float64))
    d = -np.einsum("ia,iab,ib->i", y, Si, r.astype(np.float64)) / np.einsum("ia,iab,ib->i", y, Si, y)
    e = r.astype(np.float64) + d[:, None] * y
    chi = np.einsum("ia,iab,ib->i", e, Si, e)
    s = np.einsum("ia,iab,ib->i", r, M, r).astype(np.float64)
    assert np.abs(chi - s).max() <= 1e-9 * s.max()


def test_zero_weight_rules_of_the_reference():
    s = wr.eval_scene(65, False)
    cov, _ = wr.landmark_cov(s.X, 65)
    cov = cov.copy()
    cov[3] = [np.inf, np.inf, np.inf, 0, 0, 0]
    cov[10, 4] = np.nan
    cov[20] = 0.0
    cov[30, :3] = -cov[30, :3]
    for bs, want in ((0.0, [3, 10, 20, 30]), (1e-3, [3, 10, 30])):
        M, zero = wr.info_matrices(s.X, s.y, cov, s.rot, s.tran, wr.COV_SCALE, bs)
        W, q, zero64 = wr.basis_factor(s.X, s.y, cov, s.rot, s.tran, wr.COV_SCALE, bs)
        assert np.array_equal(np.flatnonzero(zero), want) and np.array_equal(zero, zero64)
        assert not M[zero].any() and not W[zero64].any() and np.isfinite(M.astype(np.float64)).all()


def test_calibration_of_the_reference_over_20_seeds():
    """Landmarks drawn from their covariances, bearing noise 1e-3: the weighted solve beats the unweighted one, H^-1 predicts its
    error and 2 cost / dof is 1."""
    n, bs = 513, 1e-3
    ew, eu, pred, chi = [], [], [], []
    for seed in range(20):
        ns = wr.noisy_scene(n, 4000 + seed)
        s = ns.scene
        ru, tu, _ = wr.gauss_newton(lambda r, t: rr.sums(ns.X, ns.y, r, t, 0.0, np.float64), s.rot, s.tran)
        r, t = ru, tu
        for _ in range(2):                                  # freeze at the current pose, solve, once more
            W, _, zero = wr.basis_factor(ns.X, ns.y, ns.cov, r, t, 1.0, bs)
            r, t, e = wr.gauss_newton(lambda r_, t_: wr.basis_sums(ns.X, ns.y, W, zero, r_, t_, 0.0), r, t)
        C = np.linalg.inv(e.H)
        ew.append((np.sum((r - s.rot) ** 2), np.sum((t - s.tran) ** 2)))
        eu.append((np.sum((ru - s.rot) ** 2), np.sum((tu - s.tran) ** 2)))
        pred.append((np.trace(C[:3, :3]), np.trace(C[3:, 3:])))
        chi.append(2 * e.cost / (2 * n - 6))
    rms_w, rms_u, rms_p = (np.sqrt(np.mean(v, axis=0)) for v in (ew, eu, pred))
    print(f"weighted rms {rms_w}, unweighted {rms_u}, predicted {rms_p}, mean 2 cost / dof {np.mean(chi):.3f}")
    assert rms_w[0] < rms_u[0] and rms_w[1] < rms_u[1]
    assert (rms_w < 2 * rms_p).all() and (rms_p < 2 * rms_w).all()
    assert 0.8 <= np.mean(chi) <= 1.25


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("rounds", [1, 3])
@pytest.mark.parametrize("n,seed", wr.SOLVE_SCENES)
def test_lm_takes_the_same_steps_in_either_precision_on_the_solve_scenes(n, seed, rounds, f32):
    """What lets the GPU test demand equal termination and counts: the product's LM driven by the float64 evaluator and by the
    long-double one takes the same steps, round by round, and ends within RT_TOL_F64 of it."""
    ns = wr.noisy_scene(n, seed)
    X = ns.X.astype(np.float32).astype(np.float64) if f32 else ns.X
    y = ns.y.astype(np.float32).astype(np.float64) if f32 else ns.y
    r0, t0 = rr.start_near(ns.scene, seed, 0.01, 0.01)
    r, t, rl, tl = r0, t0, r0, t0
    for _ in range(rounds):
        ev = wr.weighted_evaluator(X, y, ns.cov, r, t, wr.COV_SCALE, wr.SOLVE_BEARING_SIGMA, wr.DELTA)
        evl = wr.weighted_evaluator(X, y, ns.cov, rl, tl, wr.COV_SCALE, wr.SOLVE_BEARING_SIGMA, wr.DELTA, np.longdouble)
        r, t, sm, rc = rr.harness_solve(r, t, ev)
        rl, tl, sl, rcl = rr.harness_solve(rl, tl, evl)
        assert rc == 0 and rcl == 0 and sm.termination in (1, 2, 3)
        assert (sm.termination, sm.num_iterations, sm.num_successful_steps, sm.num_evaluations) == \
               (sl.termination, sl.num_iterations, sl.num_successful_steps, sl.num_evaluations)
        assert np.abs(r - rl).max() <= 1e-9 and np.abs(t - tl).max() <= 1e-9
    assert sm.final_cost < sm.initial_cost or rounds > 1
    assert 0.5 < 2 * sm.final_cost / (2 * n - 6) < 2.0


# ---- the host header through the harness ------------------------------------------------------------------------------------
def test_basis_equals_the_restatement_also_on_ties():
    import ctypes as C
    h = wr.harness()
    ys = np.array([[0.1, 0.7, -0.7], [0.7, -0.1, 0.7], [0.6, 0.8, 0.0], [1.0, 1.0, 1.0], [0.5, -0.5, 0.7], [0.7, 0.5, 0.5],
                   [0.0, 0.0, 7.5], [-2.0, 2.0, 3.0]])
    b1r, b2r = wr.basis(ys)
    for y, r1, r2 in zip(ys, b1r, b2r):
        b1, b2 = np.zeros(3), np.zeros(3)
        h.resection_weighted_harness_basis(rr._dp(np.ascontiguousarray(y)), rr._dp(b1), rr._dp(b2))
        assert np.array_equal(b1, r1) and np.array_equal(b2, r2), y


def test_factor_and_rows_equal_numpy():
    c = wr.eval_cases(False)[-1]
    X, y = wr.case_planes(c, False)
    S, _ = wr.frozen_cov(X, y, c.cov, c.rot_w, c.tran_w, wr.COV_SCALE, c.bearing_sigma, np.float64)
    W, q, _ = wr.basis_factor(X, y, c.cov, c.rot_w, c.tran_w, wr.COV_SCALE, c.bearing_sigma)
    M, _ = wr.info_matrices(X, y, c.cov, c.rot_w, c.tran_w, wr.COV_SCALE, c.bearing_sigma)
    got = np.array([wr.harness_factor(row, yi)[1] for row, yi in zip(wr.rows_of(S)[:200], y[:200])])
    assert np.abs(got - q[:200]).max() <= 1e-9 * np.abs(q[:200]).max()
    rows = wr.harness_rows(got, y[:200])
    assert wr.row_error(rows, M[:200]) <= 8 * ROW_ERROR_EXPECTED_BELOW
    # the refusals of the factor
    y0 = y[0]
    for S6 in ([0, 0, 0, 0, 0, 0], [-1, -1, -1, 0, 0, 0], [np.inf, np.inf, np.inf, 0, 0, 0], [1, np.nan, 1, 0, 0, 0]):
        ok, qq = wr.harness_factor(S6, y0)
        assert not ok and not qq.any(), S6
    ok, qq = wr.harness_factor([2.0, 2.0, 2.0, 0, 0, 0], y0)        # isotropic: M = P / 2
    Miso = wr.full(wr.harness_rows(qq[None], y0[None]), np.float64)[0]
    assert ok and np.abs(Miso - (np.eye(3) - np.outer(y0, y0) / (y0 @ y0)) / 2).max() <= 1e-15


def test_option_checks():
    h = wr.harness()
    chk = h.resection_weighted_harness_check
    assert [chk(0, v) for v in (1.3, 1e-300, 0.0, -1.0, np.inf, np.nan)] == [1, 1, 0, 0, 0, 0]
    assert [chk(1, v) for v in (0.0, 1e-3, -1e-3, np.inf, np.nan)] == [1, 1, 0, 0, 0]
    assert [chk(2, v) for v in (0, 1, 8, 9, -1)] == [0, 1, 1, 0, 0]


def test_inverse_and_covariance_finish():
    h = wr.harness()
    c = wr.eval_cases(False)[-1]
    ref, _, _ = wr.case_reference(c, False)
    inv = np.full(36, np.nan)
    assert h.resection_weighted_harness_inverse(rr._dp(np.ascontiguousarray(ref.H.reshape(-1))), rr._dp(inv)) == 1
    inv = inv.reshape(6, 6)
    want = np.linalg.inv(ref.H.astype(np.longdouble).astype(np.float64))
    cond = np.linalg.cond(ref.H)
    assert np.array_equal(inv, inv.T)
    for blk in (np.s_[:3, :3], np.s_[3:, 3:], np.s_[:3, 3:]):
        assert np.abs(inv[blk] - want[blk]).max() <= 1e-15 * cond * np.abs(want[blk]).max(), cond
    out = np.full(43, np.nan)
    n = len(c.scene.X)
    assert h.resection_weighted_harness_finish(rr._dp(rr.row_from_sums(ref)), n, 5, rr._dp(out)) == 0
    assert np.array_equal(out[:36].reshape(6, 6), inv)
    assert tuple(out[36:42]) == (ref.cost, ref.sum_w, n - 5, 5, ref.n_outlier, 2 * (n - 5) - 6)
    assert out[42] == 2 * ref.cost / (2 * (n - 5) - 6)
    keep = np.full(43, 7.0)
    assert h.resection_weighted_harness_finish(rr._dp(rr.row_from_sums(ref)), 3, 0, rr._dp(keep)) == -6 and (keep == 7.0).all()
    bad = rr.row_from_sums(ref)
    bad[20] = -1.0                                              # H[5][5] < 0
    assert h.resection_weighted_harness_finish(rr._dp(bad), n, 0, rr._dp(keep)) == -6 and (keep == 7.0).all()
    assert h.resection_weighted_harness_inverse(rr._dp(np.zeros(36)), rr._dp(keep)) == 0 and (keep == 7.0).all()


def test_host_code_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "resection_weighted_sanitize_main"
    src = ROOT / "tests" / "harness" / "resection_weighted_sanitize_main.cpp"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0 and "resection weighted host checks passed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
