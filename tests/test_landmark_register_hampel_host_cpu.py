"""CPU: the joint registration under Hampel's redescending loss (Landmarks.eval_register_hampel / register_hampel) on the
reference alone and on the product's host side.

The reference on its own: its g against central differences of its 1/2 F_rho, and with b = c = inf the robust (Huber) reference to
the bit.  What the GPU tests (tests/test_gpu_landmark_register_hampel.py) rest on: float64 numpy in the product's formulation
counts used, behind, outlier and rejected observations as the long-double reference does, every row of the loss holds a used
observation at n >= 63, no chi2 lies within 1e-9 relative of a^2, b^2 or c^2 (so exact counts may be demanded), and float64's own
worst errors, which times 8 are the bounds.  The header csrc/sba_landmarks_register_hampel.hpp, the very text the kernel calls,
through a g++-built harness against the reference, and once under AddressSanitizer and UBSan in a program of its own.  The
calibration: on section 3.24's scenes with one bearing in ten a wrong match, the Hampel solve's pose Mahalanobis distance is below
the Huber solve's, each in its own H."""
import subprocess

import numpy as np
import pytest

import landmark_register_hampel_reference as hp
import landmark_register_reference as lr
import landmark_register_robust_reference as rb
import resection_weighted_reference as wr
from helpers import ROOT

LD = hp.LD
HARNESS_SIZES = (3, 65, 513, 1537)
INF = hp.INF


# ---- 1. the reference on its own -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (21, 22, 23))
def test_reference_gradient_is_the_derivative_of_half_the_objective(seed):
    """9 landmarks, one turned by 0.2 rad (beyond c) and three by 0.015 rad (about 5 sigma: the falling row of the loss);
    central differences of 1/2 F_rho in long double with step 1e-6 against g, relative to g's largest entry; the bound 1e-7 is that
    step's truncation error with margin, as in section 3.24."""
    s = lr.solve_scene(9, 18800 + seed)
    y = rb.displace(s.y, (1,), 18900 + seed)
    y = rb.displace(y, (3, 4, 6), 19000 + seed, 0.015)
    noise, cls = lr.freeze(s.X, s.cov, y, s.rot0, s.tran0, 1e-3)
    assert (cls == lr.LIVE).all()
    p = np.concatenate([s.rot0, s.tran0]).astype(LD)
    eq = hp.evaluate(s.X, s.cov, y, noise, p[:3], p[3:], raw=True)
    chi2, used = rb.chi2_at(s.X, s.cov, y, noise, p[:3], p[3:])
    branches = hp.branch_counts(chi2, used)
    assert eq.n_used == 9 and 2 <= eq.n_outlier < 9 and eq.n_rejected >= 1 and branches[2] >= 1, branches
    h = LD(1e-6)
    fd = np.array([(hp.half_objective(s.X, s.cov, y, noise, p + h * e) - hp.half_objective(s.X, s.cov, y, noise, p - h * e)) / (2 * h)
                   for e in np.eye(6, dtype=LD)])
    err = float(np.abs(fd - eq.g).max() / np.abs(eq.g).max())
    print(f"seed {seed}: rows of the loss {branches}, gradient against central differences {err:.2e}")
    assert err <= 1e-7


@pytest.mark.parametrize("n", (7, 65, 513))
def test_reference_with_infinite_b_and_c_is_the_huber_reference(n):
    for name in hp.POSE_NAMES:
        s = hp.scene(n, name)
        noise, _ = lr.freeze(s.X, s.cov, s.y, s.rot_ref, s.tran_ref, 1e-3)
        a = hp.evaluate(s.X, s.cov, s.y, noise, s.rot, s.tran, hp.A, INF, INF, raw=True)
        b = rb.evaluate(s.X, s.cov, s.y, noise, s.rot, s.tran, hp.A, raw=True)
        assert np.array_equal(a.H, b.H) and np.array_equal(a.g, b.g) and a.cost == b.cost
        assert (a.n_used, a.n_behind, a.n_outlier, a.n_rejected) == (b.n_used, b.n_behind, b.n_outlier, 0)
        assert np.isfinite(a.H.astype(np.float64)).all() and np.isfinite(float(a.cost))


def test_the_loss_is_continuous_with_a_continuous_weight():
    """rho and w at the three thresholds from both sides, and w = d rho / d s inside every row, in long double."""
    a, b, c = LD(hp.A), LD(hp.B), LD(hp.C)
    for t in (a, b, c):
        lo, hi = t * t * (1 - LD(1e-15)), t * t * (1 + LD(1e-15))
        w, rho, *_ = hp.hampel(np.array([lo, hi]), a, b, c)
        assert abs(rho[1] - rho[0]) <= 1e-13 * rho[0] and abs(w[1] - w[0]) <= 1e-13
    for s0 in (1.0, 9.0, 30.0, 100.0):
        e = LD(1e-7)
        _, rho, *_ = hp.hampel(np.array([s0 - e, s0 + e], dtype=LD), a, b, c)
        w = hp.hampel(np.array([s0], dtype=LD), a, b, c)[0][0]
        assert abs((rho[1] - rho[0]) / (2 * e) - w) <= 1e-9


# ---- 2. classification and float64's own errors on every GPU case ---------------------------------------------------------------
@pytest.mark.parametrize("n", hp.SIZES + hp.LONG)
def test_float64_counts_alike_and_keeps_the_margins_on_every_evaluation(n):
    """qualify_eval asserts, on the reference: every row of the loss >= 1 used observation at n >= 63, margin > 1e-9 at a^2, b^2, c^2,
    float64 counts alike."""
    worst = np.array(hp.measured_eval_errors((n,)))
    _, _, ref, chi2, used = hp.eval_reference(n, "closed", 1e-3, False)
    print(f"n = {n}: worst float64 errors of H, g, cost {worst}; rows of the loss (closed, dense) {hp.branch_counts(chi2, used)}")
    assert (worst < 1e-10).all()
    if n >= 8:
        assert ref.n_rejected >= 1 and ref.n_outlier > ref.n_rejected


def test_float64_classifies_alike_on_the_solve_scenes():
    """The posterior cases of the GPU test at the reference's own staged minimiser: classes alike, no chi2 within 1e-9 of the gate or
    of a threshold, every outlier gated, every 0.2-rad wrong match gated; the staged and the direct start reach the same minimum."""
    for n in hp.SOLVE_SIZES + hp.SOLVE_LONG:
        s = hp.solve_scene(n)
        noise, _, rot, tran, eq, it, (rot_h, tran_h, it_h) = hp.solve_reference(n)
        ref, errs = hp.qualify_posterior(s.X, s.cov, s.y, s.rot0, s.tran0, rot, tran, s.bearing_sigma)
        rot_d, tran_d, _, it_d = hp.solve_direct(s.X, s.cov, s.y, noise, s.rot0, s.tran0)
        gap = float(max(np.abs(rot_d - rot).max(), np.abs(tran_d - tran).max()))
        print(f"n = {n}: {it_h} Huber + {it} Hampel iterations ({it_d} direct, poses {gap:.1e} apart), counts {ref.counts()}, {eq.n_outlier} outliers, "
              f"{eq.n_rejected} rejected, float64 errors of X+, Sigma+, chi2, Sigma_c {errs}")
        assert gap < 1e-9
        assert ref.counts()[3] == eq.n_outlier >= eq.n_rejected >= 1 and ref.counts()[4] >= n // 2
        assert (ref.cls[hp.planted(n, 10)] == hp.GATED).all()
        assert all(e < 1e-9 for e in errs)


# ---- 3. the header through the harness -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", HARNESS_SIZES)
def test_header_evaluation_equals_the_reference(n):
    """Bound: 8 times float64 numpy's own worst error against long double over the cases of HARNESS_SIZES, measured here.  With b =
    c = inf the sums are compared with the robust harness's, and whether they are byte-identical is printed."""
    bound = 8.0 * np.array(hp.measured_eval_errors(HARNESS_SIZES))
    worst, identical = np.zeros(3), True
    for s in hp.scenes((n,)):
        for bs, abc in ((0.0, (hp.A, hp.B, hp.C)), (1e-3, (hp.A, hp.B, hp.C)), (1e-3, (hp.A, INF, INF))):
            noise, cls, ref, _, _ = hp.eval_reference(n, s.name.split()[1], bs, False, abc)
            nh, ch = lr.harness_freeze(s.X, s.cov, s.y, s.rot_ref, s.tran_ref, bs)
            assert np.array_equal(ch, cls), s.name
            got = hp.harness_eval(s.X, s.cov, s.y, nh, s.rot, s.tran, *abc)
            assert (got.n_used, got.n_behind, got.n_outlier, got.n_rejected) == (ref.n_used, ref.n_behind, ref.n_outlier, ref.n_rejected), s.name
            assert np.array_equal(got.H, got.H.T)
            err = np.array(lr.eq_errors(got, ref))
            assert (err <= bound).all(), (s.name, bs, abc, err, bound)
            worst = np.maximum(worst, err)
            if abc[1] == INF:
                hub = rb.harness_eval(s.X, s.cov, s.y, nh, s.rot, s.tran, hp.A)
                assert got.n_rejected == 0 and (got.n_used, got.n_behind, got.n_outlier) == (hub.n_used, hub.n_behind, hub.n_outlier)
                assert (np.array(lr.eq_errors(got, hub)) <= bound).all()
                identical &= got.H.tobytes() == hub.H.tobytes() and got.g.tobytes() == hub.g.tobytes() and got.cost == hub.cost
    print(f"n = {n}: worst header errors {worst}, bounds {bound}; the Huber limit is byte-identical to the robust header: {identical}")


def test_header_on_planted_rows():
    s = hp.scene(65, "closed")
    X, cov, y = s.X.copy(), s.cov.copy(), s.y.copy()
    cov[3] = [np.inf, np.inf, np.inf, 0, 0, 0]
    X[10, 1] = np.nan
    cov[20, 4] = np.nan
    y[40] = 0.0
    y[50] = -y[50]
    noise, cls = lr.freeze(X, cov, y, s.rot, s.tran, 0.0)
    nh, ch = lr.harness_freeze(X, cov, y, s.rot, s.tran, 0.0)
    assert np.array_equal(ch, cls) and [ch[i] for i in (3, 10, 20, 40, 50)] == [lr.SKIPPED] * 4 + [lr.BEHIND]
    for abc in ((hp.A, hp.B, hp.C), (hp.A, INF, INF)):
        ref = hp.evaluate(X, cov, y, noise, s.rot, s.tran, *abc)
        got = hp.harness_eval(X, cov, y, nh, s.rot, s.tran, *abc)
        assert got.n_used == 60 and np.isfinite(got.H).all() and np.isfinite(got.g).all() and np.isfinite(got.cost)
        assert (got.n_used, got.n_behind, got.n_outlier, got.n_rejected) == (ref.n_used, ref.n_behind, ref.n_outlier, ref.n_rejected)
        assert max(lr.eq_errors(got, ref)) < 1e-10


def test_every_refusal_of_the_check_function():
    chk = hp.harness_check
    inf, nan = float("inf"), float("nan")
    assert chk(2.0, 4.0, 8.0, 4.0) == 1 and chk(2.0, 4.0, 8.0, 1.0) == 1 and chk(2.0, inf, inf, 4.0) == 1
    assert chk(2.0, np.nextafter(2.0, 3.0), np.nextafter(2.0, 3.0) * 2, 4.0) == 1
    # everything the robust check refuses: a finite and > 0, the gate against a^2
    assert [chk(a, 4.0, 8.0, 1e-300) for a in (0.0, -0.0, -1.0, inf, -inf, nan)] == [0] * 6
    assert [chk(a, inf, inf, 1e-300) for a in (0.0, -1.0, inf, nan)] == [0] * 4
    assert chk(2.0, 4.0, 8.0, np.nextafter(4.0, 5.0)) == 0
    assert [chk(2.0, 4.0, 8.0, g) for g in (1.01 * 4.0, inf, nan)] == [0, 0, 0]
    assert [chk(2.0, inf, inf, g) for g in (1.01 * 4.0, inf, nan)] == [0, 0, 0]
    # b or c NaN
    assert [chk(2.0, b, c, 1.0) for b, c in ((nan, 8.0), (4.0, nan), (nan, nan), (nan, inf), (inf, nan))] == [0] * 5
    # b <= a
    assert [chk(2.0, b, 8.0, 1.0) for b in (2.0, 1.0, 0.0, -4.0)] == [0] * 4
    # c <= b
    assert [chk(2.0, 4.0, c, 1.0) for c in (4.0, 3.0, 0.0, -8.0)] == [0] * 4
    # exactly one of them infinite, and -inf
    assert [chk(2.0, b, c, 1.0) for b, c in ((4.0, inf), (inf, 8.0), (-inf, -inf), (-inf, inf), (inf, -inf), (4.0, -inf))] == [0] * 6


def test_host_code_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "landmark_register_hampel_sanitize_main"
    src = ROOT / "tests" / "harness" / "landmark_register_hampel_sanitize_main.cpp"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0 and "Hampel landmark registration host checks passed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- 4. the calibration, on the reference alone in float64 ---------------------------------------------------------------------
def _calibration(n, seeds):
    """-> mean and largest pose Mahalanobis of the staged Hampel solve and the mean of the Huber solve (each in its own H), the
    smallest eigenvalue of a fused Sigma+, the share of the planted rows beyond c, mean Hampel iterations."""
    ham, hub, lam_min, beyond, its = [], [], np.inf, [], []
    for seed in seeds:
        s = hp.solve_scene(n, seed)
        noise, _ = lr.freeze(s.X, s.cov, s.y, s.rot0, s.tran0, s.bearing_sigma, np.float64)
        rot, tran, eq, it, (rot_h, tran_h, _) = hp.solve(s.X, s.cov, s.y, noise, s.rot0, s.tran0, dtype=np.float64)
        ham.append(hp.pose_distance2(rot, tran, s, eq.H))
        eq_h = rb.evaluate(s.X, s.cov, s.y, noise, rot_h, tran_h, hp.A, np.float64)
        hub.append(hp.pose_distance2(rot_h, tran_h, s, eq_h.H))
        post = hp.posterior(s.X, s.cov, s.y, noise, rot, tran, dtype=np.float64)
        f = post.cls == hp.FUSED
        rows = hp.planted(n, 10)
        assert not f[rows].any()                               # no planted wrong match is fused
        lam_min = min(lam_min, float(np.linalg.eigvalsh(wr.full(post.cov[f], np.float64)).min()))
        beyond.append(float((post.chi2[rows].astype(np.float64) > hp.C * hp.C).mean()))
        its.append(it)
    return float(np.mean(ham)), float(np.max(ham)), float(np.mean(hub)), lam_min, float(np.mean(beyond)), float(np.mean(its))


@pytest.mark.parametrize("n,seeds", ((513, range(27100, 27110)), (64, range(27300, 27340))))
def test_the_hampel_pose_covariance_is_honest_on_frames_with_wrong_matches(n, seeds):
    """Section 3.24's calibration scenes, one bearing in ten displaced by 0.2 rad, thresholds (2, 4, 8).  Asserted: the ordering
    (Hampel's mean pose Mahalanobis distance below Huber's), no planted row fused, every fused Sigma+ positive definite; the figures go
    to DESIGN 3.27."""
    ham, ham_max, hub, lam_min, beyond, its = _calibration(n, seeds)
    print(f"{n} x {len(seeds)}: pose Mahalanobis (6 degrees of freedom) Hampel {ham:.3f} (max {ham_max:.3f}), Huber {hub:.3f}; smallest eigenvalue of "
          f"a fused Sigma+ {lam_min:.3e}; {100 * beyond:.1f} % of the planted rows beyond c; {its:.1f} Hampel iterations after Huber's")
    assert ham < hub
    assert lam_min > 0
