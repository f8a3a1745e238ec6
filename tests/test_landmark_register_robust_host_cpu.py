"""CPU: the robust joint registration (Landmarks.eval_register_robust / register_robust) on the reference alone and on the
product's host side.

The reference on its own: its g against central differences of its 1/2 F_rho, and with delta above every sqrt(chi2) the non-robust
reference to the bit.  What the GPU tests (tests/test_gpu_landmark_register_robust.py) rest on: float64 numpy in the product's
formulation counts used, behind and outlier observations as the long-double reference does, no chi2 lies within 1e-9 relative of
delta^2 (so exact counts may be demanded), and float64's own worst errors, which times 8 are the bounds.  The header
csrc/sba_landmarks_register_robust.hpp, the very text the kernel calls, through a g++-built harness against the reference, and once
under AddressSanitizer and UBSan in a program of its own.  The calibration: on section 3.20's scenes with one bearing in ten a
wrong match, the robust solve's pose is closer to the truth than the non-robust one's, in each one's own metric."""
import subprocess

import numpy as np
import pytest

import landmark_register_reference as lr
import landmark_register_robust_reference as rb
import resection_weighted_reference as wr
from helpers import ROOT

LD = rb.LD
HARNESS_SIZES = (3, 65, 513, 1537)


# ---- 1. the reference on its own -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (21, 22, 23))
def test_reference_gradient_is_the_derivative_of_half_the_objective(seed):
    """7 landmarks, 2 of them wrong matches; central differences of 1/2 F_rho in long double with step 1e-6 against g, relative to
    g's largest entry; the bound 1e-7 is that step's truncation error with margin, as in the non-robust Schur test."""
    s = lr.solve_scene(7, 18800 + seed)
    y = rb.displace(s.y, (1, 4), 18900 + seed)
    noise, cls = lr.freeze(s.X, s.cov, y, s.rot0, s.tran0, 1e-3)
    assert (cls == lr.LIVE).all()
    p = np.concatenate([s.rot0, s.tran0]).astype(LD)
    eq = rb.evaluate(s.X, s.cov, y, noise, p[:3], p[3:], rb.DELTA, raw=True)
    assert eq.n_used == 7 and 2 <= eq.n_outlier < 7
    h = LD(1e-6)
    fd = np.array([(rb.half_objective(s.X, s.cov, y, noise, p + h * e, rb.DELTA) - rb.half_objective(s.X, s.cov, y, noise, p - h * e, rb.DELTA))
                   / (2 * h) for e in np.eye(6, dtype=LD)])
    err = float(np.abs(fd - eq.g).max() / np.abs(eq.g).max())
    print(f"seed {seed}: {eq.n_outlier} outliers of 7, gradient against central differences {err:.2e}")
    assert err <= 1e-7


@pytest.mark.parametrize("n", (7, 65))
def test_reference_with_a_large_delta_is_the_plain_reference(n):
    for name in rb.POSE_NAMES:
        s = rb.scene(n, name)
        noise, _ = lr.freeze(s.X, s.cov, s.y, s.rot_ref, s.tran_ref, 1e-3)
        chi2, used = rb.chi2_at(s.X, s.cov, s.y, noise, s.rot, s.tran)
        assert float(np.sqrt(chi2[used].max())) < rb.BIG_DELTA
        a = rb.evaluate(s.X, s.cov, s.y, noise, s.rot, s.tran, rb.BIG_DELTA, raw=True)
        b = lr.evaluate(s.X, s.cov, s.y, noise, s.rot, s.tran, raw=True)
        assert np.array_equal(a.H, b.H) and np.array_equal(a.g, b.g) and a.cost == b.cost
        assert (a.n_used, a.n_behind, a.n_outlier) == (b.n_used, b.n_behind, 0)


# ---- 2. classification and float64's own errors on every GPU case ---------------------------------------------------------------
@pytest.mark.parametrize("n", rb.SIZES + rb.LONG)
def test_float64_counts_alike_and_keeps_the_margins_on_every_evaluation(n):
    worst = np.array(rb.measured_eval_errors((n,)))
    outliers = [rb.eval_reference(n, name, 1e-3, False)[2].n_outlier for name in rb.POSE_NAMES]
    print(f"n = {n}: worst float64 errors of H, g, cost {worst}; outliers {outliers}")
    assert (worst < 1e-10).all()
    if n >= 8:
        assert min(outliers) >= len(rb.planted(n, 8))         # every displaced bearing lands past delta


def test_float64_classifies_alike_on_the_solve_scenes():
    """The posterior cases of the GPU test at the reference's own minimiser: classes alike, no chi2 within 1e-9 of the gate (=
    delta^2), every outlier gated."""
    for n in rb.SOLVE_SIZES + rb.SOLVE_LONG:
        s = rb.solve_scene(n)
        _, _, rot, tran, eq, it = rb.solve_reference(n)
        ref, errs = rb.qualify_posterior(s.X, s.cov, s.y, s.rot0, s.tran0, rot, tran, s.bearing_sigma)
        print(f"n = {n}: {it} iterations, counts {ref.counts()}, {eq.n_outlier} outliers, float64 errors of X+, Sigma+, chi2, Sigma_c {errs}")
        assert ref.counts()[3] == eq.n_outlier >= len(rb.planted(n, 10)) and ref.counts()[4] >= n // 2
        assert all(e < 1e-9 for e in errs)


def test_the_demonstration_scene_separates_the_two_solves():
    """The n = 513 scene of the GPU test's demonstration, on the reference alone: in the metric of the robust reference's H at its
    minimiser, the non-robust minimiser lies at least 10 times as far from the truth (squared distance: 100 times)."""
    s = rb.solve_scene(rb.DEMO_N)
    _, _, rot, tran, eq, _ = rb.solve_reference(rb.DEMO_N)
    _, _, rot_p, tran_p, _, _ = rb.plain_reference(rb.DEMO_N)
    d_rb, d_pl = rb.pose_distance2(rot, tran, s, eq.H), rb.pose_distance2(rot_p, tran_p, s, eq.H)
    print(f"n = {rb.DEMO_N}: squared distance from the truth in the robust H: robust {d_rb:.3f}, non-robust {d_pl:.3f}")
    assert np.sqrt(d_pl) >= 10 * np.sqrt(d_rb)


# ---- 3. the header through the harness -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", HARNESS_SIZES)
def test_header_evaluation_equals_the_reference(n):
    """Bound: 8 times float64 numpy's own worst error against long double over the cases of HARNESS_SIZES, measured here."""
    bound = 8.0 * np.array(rb.measured_eval_errors(HARNESS_SIZES))
    worst = np.zeros(3)
    for s in rb.scenes((n,)):
        for bs, delta in ((0.0, rb.DELTA), (1e-3, rb.DELTA), (1e-3, rb.BIG_DELTA)):
            noise, cls, ref, _, _ = rb.eval_reference(n, s.name.split()[1], bs, False, delta)
            nh, ch = lr.harness_freeze(s.X, s.cov, s.y, s.rot_ref, s.tran_ref, bs)
            assert np.array_equal(ch, cls), s.name
            got = rb.harness_eval(s.X, s.cov, s.y, nh, s.rot, s.tran, delta)
            assert (got.n_used, got.n_behind, got.n_outlier) == (ref.n_used, ref.n_behind, ref.n_outlier), s.name
            assert np.array_equal(got.H, got.H.T)
            if delta == rb.BIG_DELTA:                          # w = 1 exactly: the non-robust header's sums to the bit
                plain = lr.harness_eval(s.X, s.cov, s.y, nh, s.rot, s.tran)
                assert got.H.tobytes() == plain.H.tobytes() and got.g.tobytes() == plain.g.tobytes() and got.cost == plain.cost
            err = np.array(lr.eq_errors(got, ref))
            assert (err <= bound).all(), (s.name, bs, delta, err, bound)
            worst = np.maximum(worst, err)
    print(f"n = {n}: worst header errors {worst}, bounds {bound}")


def test_header_on_planted_rows():
    s = rb.scene(65, "closed")
    X, cov, y = s.X.copy(), s.cov.copy(), s.y.copy()
    cov[3] = [np.inf, np.inf, np.inf, 0, 0, 0]
    X[10, 1] = np.nan
    cov[20, 4] = np.nan
    y[40] = 0.0
    y[50] = -y[50]
    noise, cls = lr.freeze(X, cov, y, s.rot, s.tran, 0.0)
    nh, ch = lr.harness_freeze(X, cov, y, s.rot, s.tran, 0.0)
    assert np.array_equal(ch, cls) and [ch[i] for i in (3, 10, 20, 40, 50)] == [lr.SKIPPED] * 4 + [lr.BEHIND]
    ref = rb.evaluate(X, cov, y, noise, s.rot, s.tran, rb.DELTA)
    got = rb.harness_eval(X, cov, y, nh, s.rot, s.tran, rb.DELTA)
    assert got.n_used == 60 and np.isfinite(got.H).all() and np.isfinite(got.g).all() and np.isfinite(got.cost)
    assert (got.n_used, got.n_behind, got.n_outlier) == (ref.n_used, ref.n_behind, ref.n_outlier)
    assert max(lr.eq_errors(got, ref)) < 1e-10


def test_every_refusal_of_the_check_function():
    chk = rb.harness_check
    inf, nan = float("inf"), float("nan")
    assert [chk(d, 1.0) for d in (2.0, 1.0, 1e-3 ** 0.5 * 40)] == [1, 1, 1]
    assert [chk(d, 1e-300) for d in (0.0, -0.0, -1.0, inf, -inf, nan)] == [0] * 6              # huber_delta finite and > 0
    assert chk(2.0, 4.0) == 1 and chk(2.0, np.nextafter(4.0, 5.0)) == 0                          # the gate against delta^2
    assert [chk(2.0, g) for g in (1.01 * 4.0, inf, nan)] == [0, 0, 0]
    assert chk(3.0, 1.01 * 4.0) == 1


def test_host_code_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "landmark_register_robust_sanitize_main"
    src = ROOT / "tests" / "harness" / "landmark_register_robust_sanitize_main.cpp"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0 and "robust landmark registration host checks passed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- 4. the calibration, on the reference alone in float64 ---------------------------------------------------------------------
def _calibration(n, seeds):
    """-> mean pose Mahalanobis of the robust and of the non-robust solve (each in its own H), landmark rms before and after the
    robust write-back over the fused landmarks, the smallest eigenvalue of a fused Sigma+, mean outliers per scene."""
    rob, plain, before, after, lam_min, nout = [], [], [], [], np.inf, []
    for seed in seeds:
        s = rb.solve_scene(n, seed)
        noise, _ = lr.freeze(s.X, s.cov, s.y, s.rot0, s.tran0, s.bearing_sigma, np.float64)
        rot, tran, eq, _ = rb.solve(s.X, s.cov, s.y, noise, s.rot0, s.tran0, rb.DELTA, np.float64)
        rob.append(rb.pose_distance2(rot, tran, s, eq.H))
        rot_p, tran_p, eq_p, _ = lr.solve(s.X, s.cov, s.y, noise, s.rot0, s.tran0, np.float64)
        plain.append(rb.pose_distance2(rot_p, tran_p, s, eq_p.H))
        post = rb.posterior(s.X, s.cov, s.y, noise, rot, tran, rb.DELTA, rb.GATE, np.float64)
        f = post.cls == rb.FUSED
        assert not f[rb.planted(n, 10)].any()                  # no wrong match is fused
        C = wr.full(post.cov[f], np.float64)
        lam_min = min(lam_min, float(np.linalg.eigvalsh(C).min()))
        e0, e1 = (s.X - s.truth.X)[f], (post.X.astype(np.float64) - s.truth.X)[f]
        before.append(np.sum(e0 * e0, axis=1))
        after.append(np.sum(e1 * e1, axis=1))
        nout.append(eq.n_outlier)
    rms = lambda v: float(np.sqrt(np.concatenate(v).mean()))
    return float(np.mean(rob)), float(np.mean(plain)), rms(before), rms(after), lam_min, float(np.mean(nout))


@pytest.mark.parametrize("n,seeds", ((513, range(27100, 27110)), (64, range(27300, 27340))))
def test_the_robust_solve_is_closer_to_the_truth_on_frames_with_wrong_matches(n, seeds):
    """Section 3.20's scene recipe, one bearing in ten displaced by 0.2 rad.  Nothing is fixed in advance but the ordering that
    gives the feature its meaning, and that every fused Sigma+ is positive definite; the figures go to DESIGN 3.24."""
    rob, plain, rms0, rms1, lam_min, nout = _calibration(n, seeds)
    print(f"{n} x {len(seeds)}: pose Mahalanobis robust {rob:.3f} (6), non-robust {plain:.3f}; fused landmarks rms {rms0:.4f} -> {rms1:.4f}; "
          f"smallest eigenvalue of a fused Sigma+ {lam_min:.3e}; {nout:.1f} outliers per scene")
    assert rob < plain
    assert lam_min > 0
