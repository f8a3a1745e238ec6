"""CPU: the joint registration (Landmarks.eval_register / register) on the reference alone and on the product's host side.

The reference's reduced six-parameter system against the dense (6 + 3 m)-dimensional Gauss-Newton system it is the Schur complement
of.  What the joint solve buys, on the reference alone in float64 over seeded scenes of section 3.20's recipe.  What the GPU tests
(tests/test_gpu_landmark_register.py) rest on, over EVERY evaluation they run: float64 numpy in the product's formulation classifies
every observation as the long-double reference does and no eliminated depth lies within 1e-9 of 0 (so exact counts may be
demanded), and float64's own worst errors -- which times 8 are the GPU test's bounds.  The header
csrc/sba_landmarks_register.hpp, the very text the kernels call, through a g++-built harness against the reference, and once
under AddressSanitizer and UBSan in a program of its own."""
import subprocess

import numpy as np
import pytest

import landmark_fusion_reference as lf
import landmark_register_reference as lr
import pose_edges
import resection_reference as rr
import resection_weighted_reference as wr
from helpers import ROOT


# ---- 1. the dense identity -----------------------------------------------------------------------------------------------------
def _dense_system(X, cov6, y, noise, p, Xv):
    """The stacked residuals [B_j^T (-R X_j + t) / s_j ; Sigma_j^-1/2 (X_j - Xb_j)] at (p, Xv) in float64, and their Jacobian over
    (w, t, X_1 .. X_m) by CENTRAL DIFFERENCES with step 1e-6."""
    m = len(X)
    B = []
    for yj in y:
        k = np.argmin(np.abs(yj))
        b1 = np.cross(np.eye(3)[k], yj)
        b1 /= np.linalg.norm(b1)
        b2 = np.cross(yj, b1)
        B.append(np.stack([b1, b2 / np.linalg.norm(b2)], axis=1))              # 3 x 2, orthonormal, across the bearing
    roots = []
    for row in wr.full(cov6, np.float64):
        lam, V = np.linalg.eigh(row)
        roots.append(V @ np.diag(lam ** -0.5) @ V.T)

    def residual(z):
        R = rr.rotmat(z[:3], np.float64)
        out = []
        for j in range(m):
            Xj = z[6 + 3 * j:9 + 3 * j]
            out.append(B[j].T @ (-R @ Xj + z[3:6]) / np.sqrt(noise[j]))
            out.append(roots[j] @ (Xj - X[j]))
        return np.concatenate(out)

    z0 = np.concatenate([p, Xv.reshape(-1)])
    h = 1e-6
    J = np.stack([(residual(z0 + h * e) - residual(z0 - h * e)) / (2 * h) for e in np.eye(len(z0))], axis=1)
    return residual(z0), J


@pytest.mark.parametrize("seed", (11, 12, 13))
def test_reduced_system_is_the_schur_complement_of_the_dense_one(seed):
    """Finite differences are used for the dense Jacobian (central, step 1e-6), so the bound is 1e-7: the truncation error of that
    step with margin.  The reduced side is the long-double reference."""
    m, bs = 7, 1e-3
    s = lr.solve_scene(m, 8800 + seed)
    noise, cls = lr.freeze(s.X, s.cov, s.y, s.rot0, s.tran0, bs)
    assert (cls == lr.LIVE).all()
    rot, tran, eq, _ = lr.solve(s.X, s.cov, s.y, noise, s.rot0, s.tran0)
    post = lr.posterior(s.X, s.cov, s.y, noise, rot, tran)
    assert (post.cls == lr.FUSED).all()
    Xh = post.X.astype(np.float64)
    res, J = _dense_system(s.X, s.cov, s.y, noise.astype(np.float64), np.concatenate([rot, tran]), Xh)
    N = J.T @ J
    Ni = np.linalg.inv(N)
    rel = lambda got, ref: float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max())
    errs = {"H": rel(eq.H, np.linalg.inv(Ni[:6, :6])), "Sigma_c": rel(post.pose_cov, Ni[:6, :6]),
            "cost": abs(eq.cost - 0.5 * res @ res) / eq.cost, "gradient": float(np.abs(J.T @ res).max())}
    for j in range(m):
        blk = slice(6 + 3 * j, 9 + 3 * j)
        errs[f"Sigma+ {j}"] = rel(wr.full(post.cov[j:j + 1], np.float64)[0], Ni[blk, blk])
        errs[f"cross {j}"] = rel(post.cross[j], Ni[blk, :6])
    print({k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= 1e-7, (k, v)


# ---- 2. what it buys -----------------------------------------------------------------------------------------------------------
def _joint_route(s, dtype=np.float64):
    noise, cls = lr.freeze(s.X, s.cov, s.y, s.rot0, s.tran0, s.bearing_sigma, dtype)
    rot, tran, eq, _ = lr.solve(s.X, s.cov, s.y, noise, s.rot0, s.tran0, dtype)
    post = lr.posterior(s.X, s.cov, s.y, noise, rot, tran, np.inf, dtype)
    assert (post.cls == lr.FUSED).all()
    return rot, tran, eq, post


def _sequential_route(s):
    """The chain the joint solve replaces: the resection with weights frozen at the start, its covariance, then the fusion with it."""
    M, zero = wr.info_matrices(s.X, s.y, s.cov, s.rot0, s.tran0, 1.0, s.bearing_sigma, np.float64)
    rot, tran, e = wr.gauss_newton(lambda r, t: wr.sums(s.X, s.y, M, zero, r, t, 0.0, np.float64), s.rot0, s.tran0, steps=30)
    return lf.fuse(s.X, s.cov, s.y, rot, tran, s.bearing_sigma, np.inf, np.linalg.inv(e.H), np.float64)


def _maha(e, cov6):
    C = wr.full(cov6, np.float64)
    return np.einsum("ia,ia->i", e, np.linalg.solve(C, e[:, :, None])[:, :, 0]), C


def _calibration(n, seeds):
    pose, land, seq, before, after, pred, lam_min = [], [], [], [], [], [], np.inf
    for seed in seeds:
        s = lr.solve_scene(n, seed)
        rot, tran, eq, post = _joint_route(s)
        dp = np.concatenate([rot - s.truth.rot, tran - s.truth.tran])
        pose.append(dp @ eq.H @ dp)
        e0, e1 = s.X - s.truth.X, post.X.astype(np.float64) - s.truth.X
        mh, C = _maha(e1, post.cov)
        lam_min = min(lam_min, np.linalg.eigvalsh(C).min())
        land.append(mh)
        before.append(np.sum(e0 * e0, axis=1))
        after.append(np.sum(e1 * e1, axis=1))
        pred.append(np.trace(C, axis1=1, axis2=2))
        sq = _sequential_route(s)
        seq.append(_maha(sq.X.astype(np.float64) - s.truth.X, sq.cov)[0])
    cat = lambda v: np.concatenate(v)
    return (float(np.mean(pose)), float(cat(land).mean()), float(cat(seq).mean()), float(np.sqrt(cat(before).mean())),
            float(np.sqrt(cat(after).mean())), float(np.sqrt(cat(pred).mean())), lam_min)


def test_what_the_joint_solve_buys_on_full_frames():
    """20 scenes of 513 landmarks: the pose and the landmarks are calibrated, the landmarks improve by more than half, Sigma+ predicts
    the error that is left and stays positive definite."""
    pose, land, seq, rms0, rms1, rmsp, lam_min = _calibration(513, range(7100, 7120))
    print(f"513 x 20: pose Mahalanobis {pose:.3f} (6), landmark Mahalanobis {land:.3f} (3), sequential route {seq:.3f}, rms {rms0:.3f} -> "
          f"{rms1:.3f}, predicted {rmsp:.3f}, smallest eigenvalue {lam_min:.3e}")
    assert 0.8 <= land / 3 <= 1.25
    assert 0.6 <= pose / 6 <= 1.5
    assert rms1 <= 0.5 * rms0
    assert rmsp <= 1.25 * rms1 and rms1 <= 1.25 * rmsp
    assert lam_min > 0


def test_what_the_joint_solve_buys_on_thin_frames():
    """300 scenes of 8 landmarks, where the sequential route's posterior is optimistic (its landmark Mahalanobis is printed, not
    asserted): the joint route stays calibrated."""
    pose, land, seq, rms0, rms1, rmsp, lam_min = _calibration(8, range(7200, 7500))
    print(f"8 x 300: pose Mahalanobis {pose:.3f} (6), landmark Mahalanobis {land:.3f} (3), sequential route {seq:.3f}, rms {rms0:.3f} -> "
          f"{rms1:.3f}, predicted {rmsp:.3f}, smallest eigenvalue {lam_min:.3e}")
    assert 0.8 <= land / 3 <= 1.25
    assert 0.6 <= pose / 6 <= 1.5
    assert rmsp <= 1.25 * rms1 and rms1 <= 1.25 * rmsp
    assert lam_min > 0


# ---- 5. classification and float64's own errors on every GPU case ---------------------------------------------------------------
@pytest.mark.parametrize("n", lr.SIZES + lr.LONG)
def test_float64_classifies_alike_and_keeps_the_margins_on_every_evaluation(n):
    worst = np.zeros(3)
    for s in lr.scenes((n,)):
        for bs in lr.BEARING_SIGMAS:
            for indexed in (False, True):
                worst = np.maximum(worst, lr.qualify_eval(s, bs, indexed))
    print(f"n = {n}: worst float64 errors of H, g, cost {worst}")
    assert (worst < 1e-10).all()


def test_float64_classifies_alike_on_the_solve_scenes():
    """The posterior cases of the GPU test, here at the reference's own minimiser (the GPU test qualifies again at the device's
    pose): classes alike, no chi2 within 1e-9 of the gate, no depth within 1e-9 of 0."""
    for n in lr.SOLVE_SIZES + lr.SOLVE_LONG:
        s = lr.solve_scene(n)
        _, _, rot, tran, eq, it = lr.solve_reference(n)
        ref, errs = lr.qualify_posterior(s.X, s.cov, s.y, s.rot0, s.tran0, rot, tran, s.bearing_sigma)
        print(f"n = {n}: {it} iterations, counts {ref.counts()}, float64 errors of X+, Sigma+, chi2, Sigma_c {errs}")
        assert ref.counts()[4] >= n // 2 and ref.counts()[1] == 0
        assert all(e < 1e-9 for e in errs)


# ---- 3. the header through the harness -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (3, 65, 513, 1537))
def test_header_evaluation_equals_the_reference(n):
    bound = 8.0 * np.array(lr.measured_eval_errors())
    worst = np.zeros(3)
    for s in lr.scenes((n,)):
        for bs in lr.BEARING_SIGMAS:
            noise, cls, ref = lr.eval_reference(n, s.name.split()[1], bs, False)
            nh, ch = lr.harness_freeze(s.X, s.cov, s.y, s.rot_ref, s.tran_ref, bs)
            assert np.array_equal(ch, cls), s.name
            assert np.abs(nh - noise.astype(np.float64)).max() <= 1e-12 * max(np.abs(nh).max(), 1e-300), s.name
            got = lr.harness_eval(s.X, s.cov, s.y, nh, s.rot, s.tran)
            assert (got.n_used, got.n_behind) == (ref.n_used, ref.n_behind), s.name
            assert np.array_equal(got.H, got.H.T)
            err = np.array(lr.eq_errors(got, ref))
            assert (err <= bound).all(), (s.name, bs, err, bound)
            worst = np.maximum(worst, err)
    print(f"n = {n}: worst header errors {worst}, bounds {bound}")


@pytest.mark.parametrize("n", (3, 65, 513, 1537))
def test_header_write_back_equals_the_reference(n):
    """At the reference's minimiser of a solve scene, with the reference's Sigma_c: classes alike, X+, Sigma+ and chi2 within 8 times
    float64 numpy's own errors on the same case, everything not fused left as it was."""
    s = lr.solve_scene(n)
    noise, cls = lr.freeze(s.X, s.cov, s.y, s.rot0, s.tran0, s.bearing_sigma)
    rot, tran, _, _ = lr.solve(s.X, s.cov, s.y, noise, s.rot0, s.tran0, max_iterations=40)
    ref, errs = lr.qualify_posterior(s.X, s.cov, s.y, s.rot0, s.tran0, rot, tran, s.bearing_sigma)
    nh, ch = lr.harness_freeze(s.X, s.cov, s.y, s.rot0, s.tran0, s.bearing_sigma)
    assert np.array_equal(ch, cls)
    Xo, Co, chi2, c2 = lr.harness_apply(s.X, s.cov, s.y, nh, rot, tran, ref.pose_cov.astype(np.float64), lr.GATE)
    assert np.array_equal(c2, ref.cls)
    keep = ref.cls != lr.FUSED
    assert Xo[keep].tobytes() == s.X[keep].tobytes() and Co[keep].tobytes() == s.cov[keep].tobytes()
    got = np.array(lf.errors(Xo, Co, chi2, ref, s.X, s.cov))
    print(f"n = {n}: header errors {got}, float64 numpy's {errs[:3]}")
    assert (got <= 8.0 * np.array(errs[:3])).all()


def test_header_classes_on_planted_rows():
    s = lr.scene(65, "series")
    X, cov, y = s.X.copy(), s.cov.copy(), s.y.copy()
    cov[3] = [np.inf, np.inf, np.inf, 0, 0, 0]
    X[10, 1] = np.nan
    cov[20, 4] = np.nan
    cov[30] = [-1e-4, -1e-4, -1e-4, 0, 0, 0]
    y[40] = 0.0
    y[50] = -y[50]
    noise, cls = lr.freeze(X, cov, y, s.rot, s.tran, 0.0)
    nh, ch = lr.harness_freeze(X, cov, y, s.rot, s.tran, 0.0)
    assert np.array_equal(ch, cls)
    assert [ch[i] for i in (3, 10, 20, 30, 40, 50)] == [lr.SKIPPED] * 5 + [lr.BEHIND]
    assert np.isnan(nh[[3, 10, 20, 30, 40]]).all() and np.signbit(nh[50])
    ref = lr.posterior(X, cov, y, noise, s.rot, s.tran, lr.GATE)
    got = lr.harness_eval(X, cov, y, nh, s.rot, s.tran)
    assert got.n_used == 59 and np.isfinite(got.H).all()
    Xo, Co, chi2, c2 = lr.harness_apply(X, cov, y, nh, s.rot, s.tran, ref.pose_cov.astype(np.float64), lr.GATE)
    assert np.array_equal(c2, ref.cls)
    assert [c2[i] for i in (3, 10, 20, 30, 40, 50)] == [lr.SKIPPED] * 5 + [lr.BEHIND]
    assert np.isnan(chi2[[3, 10, 20, 30, 40]]).all() and np.isfinite(chi2[50])
    keep = c2 != lr.FUSED
    assert Xo[keep].tobytes() == X[keep].tobytes() and Co[keep].tobytes() == cov[keep].tobytes()


def test_host_code_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "landmark_register_sanitize_main"
    src = ROOT / "tests" / "harness" / "landmark_register_sanitize_main.cpp"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0 and "landmark registration host checks passed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_every_edge_rotation_is_among_the_cases():
    assert {s.name.split()[1] for s in lr.scenes((65,))} == set(pose_edges.NAMES) and len(pose_edges.NAMES) == 9
