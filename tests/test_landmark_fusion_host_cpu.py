"""CPU: the landmark fusion on the reference alone and on the product's host side.

What the GPU tests (tests/test_gpu_landmark_fusion.py) rest on, over EVERY case they run: float64 numpy in the product's
formulation classifies every observation as the long-double reference does, no chi^2 sits within 1e-9 relative of the gate and no
eliminated depth within 1e-9 of 0 (so exact counts may be demanded), and float64's own worst errors of X+, Sigma+ and chi^2 --
which times 8 are the GPU test's three bounds.  What fusing buys, on the reference alone over 20 seeded scenes.  The header
csrc/sba_landmarks.hpp, the very text the kernels call, through a g++-built harness against the reference on the same cases, and
once under AddressSanitizer and UBSan in a program of its own."""
import subprocess

import numpy as np
import pytest

import landmark_fusion_reference as lf
import pose_edges
import resection_reference as rr
import resection_weighted_reference as wr
from helpers import ROOT

# float64 numpy's worst errors against long double over all cases (measured 6.2e-13 of |X|, 5.9e-13 of the prior row's largest
# entry, 1.3e-12 of max(chi^2, 1): the 2 x 2 projected covariance has a condition of up to 1e4 at sigma_r / sigma_t = 100).  The
# GPU bounds are 8 times the values measured in the run itself.
ERRORS_EXPECTED_BELOW = (2e-12, 2e-12, 4e-12)


@pytest.mark.parametrize("n", lf.SIZES + lf.LONG)
def test_float64_classifies_alike_and_keeps_the_margins_on_every_gpu_case(n):
    worst = np.zeros(3)
    for s in lf.scenes((n,)):
        for bs, pc in lf.variants():
            worst = np.maximum(worst, lf.qualify(s, bs, pc))
            ref = lf.reference(n, s.name.split()[1], bs, pc is not None)
            assert ref.counts()[0] == n and sum(ref.counts()[1:]) == n
            if n >= 511:
                assert ref.counts()[3] >= 1 and ref.counts()[4] >= n // 2, (s.name, ref.counts())      # the gate bites, most are fused
    print(f"n = {n}: worst float64 errors {worst}")
    assert (worst < ERRORS_EXPECTED_BELOW).all()
    if n > 3:
        assert (worst > 0).all()


def test_measured_errors_are_what_the_design_states():
    worst = lf.measured_errors()
    print(f"float64 numpy against long double: X+ {worst[0]:.3e}, Sigma+ {worst[1]:.3e}, chi2 {worst[2]:.3e}")
    assert all(0 < w < b for w, b in zip(worst, ERRORS_EXPECTED_BELOW))


def test_the_update_is_the_information_form_map():
    """The reference itself equals the information-form MAP.  With N = S - R Sigma R^T, the noise of the measurement alone, and M_N
    formed from N as M is from S: Sigma+^-1 = Sigma^-1 + R^T M_N R and (Sigma+^-1)(X+ - X) = R^T M_N r.  float64 inverses against the
    long-double gain form."""
    s = lf.scene(513, "closed")
    ref = lf.fuse(s.X, s.prior_cov, s.y, s.rot, s.tran, 1e-3, np.inf, lf.POSE_COV_FULL)
    Sg, S, R, r, _ = lf._prior_cov_S(np.asarray(s.X, lf.LD), np.asarray(s.prior_cov, lf.LD), np.asarray(s.y, lf.LD), s.rot, s.tran, 1e-3,
                                     lf.POSE_COV_FULL, lf.LD)
    Si, _ = wr._adjugate_inverse(S - R[None] @ Sg @ R.T[None])
    v = np.einsum("iab,ib->ia", Si, np.asarray(s.y, lf.LD))
    M = Si - v[:, :, None] * v[:, None, :] / np.sum(v * s.y, axis=1)[:, None, None]
    info = np.linalg.inv(Sg.astype(np.float64)) + (R.T[None] @ M @ R[None]).astype(np.float64)
    post = np.linalg.inv(info)
    got = wr.full(ref.cov, np.float64)
    scale = np.abs(s.prior_cov).max(axis=1)
    assert (np.abs(post - got).max(axis=(1, 2)) / scale).max() <= 1e-9
    # X+ solves info (X+ - X) = R^T M r
    rhs = np.einsum("ab,ibc,ic->ia", R.T, M, r).astype(np.float64)
    dx = np.linalg.solve(info, rhs[:, :, None])[:, :, 0]
    assert np.abs(dx - (ref.X - s.X).astype(np.float64)).max() <= 1e-9 * np.abs(dx).max()
    assert (ref.cls == lf.FUSED).all()


def test_what_fusing_buys_over_20_seeds():
    """Priors drawn from their covariances, bearing noise 1e-3, the pose drawn once per scene from a diagonal Sigma_pose around the
    truth and passed with it, no gate: chi^2 has 2 degrees of freedom, the landmarks improve by more than half, Sigma+ predicts the
    error that is left, and every Sigma+ stays positive definite."""
    n, bs = 513, 1e-3
    sig = np.sqrt(np.diag(lf.POSE_COV))
    chi, before, after, pred, maha, lam_min = [], [], [], [], [], np.inf
    for seed in range(20):
        ns = wr.noisy_scene(n, 6000 + seed)
        s = ns.scene
        rng = np.random.default_rng(seed + 60000)
        dp = sig * rng.standard_normal(6)
        ref = lf.fuse(ns.X, ns.cov, ns.y, s.rot + dp[:3], s.tran + dp[3:], bs, np.inf, lf.POSE_COV, np.float64)
        assert (ref.cls == lf.FUSED).all()
        e0, e1 = ns.X - s.X, ref.X - s.X
        C = wr.full(ref.cov, np.float64)
        lam_min = min(lam_min, np.linalg.eigvalsh(C).min())
        chi.append(ref.chi2)
        before.append(np.sum(e0 * e0, axis=1))
        after.append(np.sum(e1 * e1, axis=1))
        pred.append(np.trace(C, axis1=1, axis2=2))
        maha.append(np.einsum("ia,ia->i", e1, np.linalg.solve(C, e1[:, :, None])[:, :, 0]))
    chi, before, after, pred, maha = (np.concatenate(v) for v in (chi, before, after, pred, maha))
    rms0, rms1, rmsp = np.sqrt(before.mean()), np.sqrt(after.mean()), np.sqrt(pred.mean())
    print(f"mean chi2 {chi.mean():.3f}, above 9.21: {100 * (chi > 9.21).mean():.2f} %, rms {rms0:.3f} -> {rms1:.3f}, predicted {rmsp:.3f}, "
          f"mean Mahalanobis {maha.mean():.3f}, smallest eigenvalue {lam_min:.3e}")
    assert 0.8 <= chi.mean() / 2 <= 1.25
    assert rms1 <= 0.5 * rms0
    assert rmsp <= 1.25 * rms1 and rms1 <= 1.25 * rmsp
    assert 0.8 <= maha.mean() / 3 <= 1.25
    assert lam_min > 0


# ---- the header through the harness --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (3, 65, 513, 1537))
def test_header_equals_the_reference_on_the_gpu_cases(n):
    bound = 8.0 * np.array(lf.measured_errors())
    worst = np.zeros(3)
    for s in lf.scenes((n,)):
        for bs, pc in lf.variants():
            ref = lf.reference(n, s.name.split()[1], bs, pc is not None)
            got = lf.harness_fuse(s.X, s.prior_cov, s.y, s.rot, s.tran, bs, lf.GATE, pc)
            assert np.array_equal(got.cls, ref.cls), s.name
            keep = ref.cls != lf.FUSED
            assert got.X[keep].tobytes() == s.X[keep].tobytes() and got.cov[keep].tobytes() == s.prior_cov[keep].tobytes()
            err = np.array(lf.errors(got.X, got.cov, got.chi2, ref, s.X, s.prior_cov))
            assert (err <= bound).all(), (s.name, bs, pc is not None, err, bound)
            worst = np.maximum(worst, err)
            C = wr.full(got.cov[~keep], np.float64)
            assert np.array_equal(C, np.swapaxes(C, 1, 2))
    print(f"n = {n}: worst header errors {worst}, bounds {bound}")


def test_header_classes_on_planted_rows():
    s = lf.scene(65, "series")
    X, cov, y = s.X.copy(), s.prior_cov.copy(), s.y.copy()
    cov[3] = [np.inf, np.inf, np.inf, 0, 0, 0]
    X[10, 1] = np.nan
    cov[20, 4] = np.nan
    cov[30] = [-1e-4, -1e-4, -1e-4, 0, 0, 0]
    y[40] = 0.0
    y[50] = -y[50]
    ref = lf.fuse(X, cov, y, s.rot, s.tran, 0.0, lf.GATE)
    got = lf.harness_fuse(X, cov, y, s.rot, s.tran, 0.0, lf.GATE)
    assert np.array_equal(got.cls, ref.cls)
    assert [got.cls[i] for i in (3, 10, 20, 30, 40, 50)] == [lf.SKIPPED] * 5 + [lf.BEHIND]
    assert np.isnan(got.chi2[[3, 10, 20, 30, 40]]).all() and np.isfinite(got.chi2[50])
    keep = got.cls != lf.FUSED
    assert got.X[keep].tobytes() == X[keep].tobytes() and got.cov[keep].tobytes() == cov[keep].tobytes()
    # with bearing noise the negative variance is still indefinite across the bearing only if it outweighs the noise: here it does not
    got2 = lf.harness_fuse(X, cov, y, s.rot, s.tran, 1e-1, lf.GATE)
    ref2 = lf.fuse(X, cov, y, s.rot, s.tran, 1e-1, lf.GATE)
    assert np.array_equal(got2.cls, ref2.cls)


def test_option_and_index_checks():
    import ctypes as C
    h = lf.harness()
    chk = h.landmark_fusion_harness_check
    assert [chk(0, v) for v in (1.3, 1e-300, 0.0, -1.0, np.inf, np.nan)] == [1, 1, 0, 0, 0, 0]
    assert [chk(1, v) for v in (0.0, 1e-3, -1e-3, np.inf, np.nan)] == [1, 1, 0, 0, 0]
    assert [chk(2, v) for v in (9.21, 1e-300, np.inf, 0.0, -1.0, -np.inf, np.nan)] == [1, 1, 1, 0, 0, 0, 0]
    pc = lf.POSE_COV_FULL.copy()
    cp = h.landmark_fusion_harness_check_pose_cov
    assert cp(None) == 1 and cp(rr._dp(pc)) == 1 and cp(rr._dp(np.zeros((6, 6)))) == 1
    for i, j, v in ((0, 1, np.nextafter(pc[0, 1], 1.0)), (5, 5, np.nan), (2, 2, -1e-12), (4, 0, np.inf)):
        bad = pc.copy()
        bad[i, j] = v
        assert cp(rr._dp(bad)) == 0, (i, j, v)

    def ci(idx, m, n):
        a = None if idx is None else np.ascontiguousarray(idx, dtype=np.int64)
        return h.landmark_fusion_harness_check_index(None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64)), m, n)
    assert ci([0, 2, 3, 9], 4, 10) == 1 and ci(np.arange(10), 10, 10) == 1 and ci([], 0, 10) == 1 and ci(None, 10, 10) == 1
    assert ci(None, 0, 0) == 1
    assert ci([0, 2, 2, 9], 4, 10) == 0          # a repeat
    assert ci([0, 3, 2, 9], 4, 10) == 0          # descending
    assert ci([0, 2, 3, 10], 4, 10) == 0         # == n
    assert ci([-1, 2, 3, 9], 4, 10) == 0
    assert ci([0, 1, 2, 3], 4, 3) == 0           # m > n
    assert ci(None, 9, 10) == 0 and ci(None, 11, 10) == 0      # dense with m != n


def test_host_code_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "landmark_fusion_sanitize_main"
    src = ROOT / "tests" / "harness" / "landmark_fusion_sanitize_main.cpp"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0 and "landmark fusion host checks passed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_every_edge_rotation_is_among_the_cases():
    assert {s.name.split()[1] for s in lf.scenes((65,))} == set(pose_edges.NAMES) and len(pose_edges.NAMES) == 9
