"""GPU: the robust joint registration of a frame against the landmark map (api.Landmarks.eval_register_robust / register_robust)
against the long-double reference of tests/landmark_register_robust_reference.py, on the cases
tests/test_landmark_register_robust_host_cpu.py qualifies (float64 numpy counts every observation alike there and no chi2 lies
within 1e-9 relative of delta^2): the vector-per-lane, wave and block edges, several grid-stride steps with a partial last wave
(SBA_RESECT_GRID=1), dense and indexed, with and without the bearing's noise, about one bearing in eight displaced past delta,
three rotations of tests/pose_edges.py (identity: the small-angle branch, one generic, one near pi), the noise frozen 1e-2 rad
off the evaluation pose.  Counts are exact; H, g and the cost, and X+, Sigma+, chi2 and the pose covariance, are held to 8 times
float64 numpy's own error on the same cases, measured in this run.  The solve against the reference's own
minimiser; the posterior at the device's pose; planted rows of every class, at the given pose and solved; the demonstration
against the non-robust register; bytes across handles, forms, histories, grids and host / device bearings, with guard cells around
chi2 on the device; refusals; every entry point on a map that was pruned and appended to.  Every wait inside the library is its
bounded stream wait."""
from functools import lru_cache

import numpy as np
import pytest

import landmark_edit_reference as le
import landmark_fusion_reference as lf
import landmark_register_reference as lr
import landmark_register_robust_reference as rb
import resection_reference as rr
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

pytestmark = pytest.mark.gpu

TIGHT = dict(function_tolerance=1e-30, parameter_tolerance=1e-13, gradient_tolerance=1e-13, max_num_iterations=100)
GRIDS = (None, "1", "2", "3")
D = rb.DELTA
_worst_eval = np.zeros(3)


def _tight():
    return api.default_lm_options(**TIGHT)


def _at_pose():
    return api.default_lm_options(max_num_iterations=0)


@lru_cache(maxsize=None)
def _eval_bounds():
    """8 times float64 numpy's worst errors against long double on the same evaluations, measured in this run."""
    return 8.0 * np.array(rb.measured_eval_errors())


def _state(L):
    X, Cv = L.get()
    return X.tobytes() + Cv.tobytes() + L.counts().tobytes()


def _counts(f):
    return (f.n_obs, f.n_skipped, f.n_behind, f.n_gated, f.n_fused)


def _result_bytes(f, chi2=None):
    chi2 = f.chi2 if chi2 is None else chi2
    return (b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in (f.rot, f.tran, f.cov, chi2))
            + repr(_counts(f) + (f.n_used, f.n_outlier)).encode())


def _eq_bytes(e):
    return e.H.tobytes() + e.g.tobytes() + repr((e.cost, e.n_used, e.n_behind, e.n_outlier)).encode()


# ---- 1. evaluation parity --------------------------------------------------------------------------------------------------------
def _run_eval_size(n):
    global _worst_eval
    identical = []
    with api.Landmarks(0) as L:
        for s in rb.scenes((n,)):
            L.set(s.X, s.cov)
            before = _state(L)
            pose = s.name.split()[1]
            for bs in rb.BEARING_SIGMAS:
                for form, idx in lr.forms(s):
                    _, cls, ref, _, _ = rb.eval_reference(n, pose, bs, idx is not None)
                    y = s.y if idx is None else s.y[idx]
                    got = L.eval_register_robust(y, s.rot, s.tran, D, s.rot_ref, s.tran_ref, bs, idx=idx)
                    what = f"{s.name} bs={bs} {form}"
                    assert (got.n_used, got.n_behind, got.n_outlier) == (ref.n_used, ref.n_behind, ref.n_outlier), what
                    assert got.n_used == int((cls == lr.LIVE).sum()), what
                    assert np.array_equal(got.H, got.H.T), what
                    if ref.n_used:
                        err = np.array(lr.eq_errors(got, ref))
                        print(f"{what}: errors {err}, outliers {got.n_outlier} of {got.n_used}")
                        assert (err <= _eval_bounds()).all(), f"{what}: errors {err}, bounds {_eval_bounds()}"
                        _worst_eval = np.maximum(_worst_eval, err)
                    else:
                        assert not got.H.any() and not got.g.any() and got.cost == 0.0, what
            # a delta above every sqrt(chi2): nothing is an outlier, and the sums are the non-robust pass's
            _, _, ref, _, _ = rb.eval_reference(n, pose, 1e-3, False, rb.BIG_DELTA)
            big = L.eval_register_robust(s.y, s.rot, s.tran, rb.BIG_DELTA, s.rot_ref, s.tran_ref, 1e-3)
            plain = L.eval_register(s.y, s.rot, s.tran, s.rot_ref, s.tran_ref, 1e-3)
            assert (big.n_used, big.n_behind, big.n_outlier) == (plain.n_used, plain.n_behind, 0) == (ref.n_used, ref.n_behind, 0), s.name
            if ref.n_used:
                for got in (big, plain):
                    err = np.array(lr.eq_errors(got, ref))
                    assert (err <= _eval_bounds()).all(), f"{s.name} large delta: errors {err}, bounds {_eval_bounds()}"
            identical.append(big.H.tobytes() == plain.H.tobytes() and big.g.tobytes() == plain.g.tobytes() and big.cost == plain.cost)
            assert _state(L) == before, s.name                                  # an evaluation writes nothing
    print(f"n = {n}: device worst so far H {_worst_eval[0]:.3e}, g {_worst_eval[1]:.3e}, cost {_worst_eval[2]:.3e}; bounds {_eval_bounds()}; "
          f"large delta byte-identical to eval_register: {identical}")


@pytest.mark.parametrize("n", rb.SIZES)
def test_evaluation_against_long_double(n):
    _run_eval_size(n)


@pytest.mark.parametrize("n", rb.LONG)
def test_evaluation_over_several_grid_stride_steps(monkeypatch, n):
    monkeypatch.setenv("SBA_RESECT_GRID", "1")
    _run_eval_size(n)


# ---- 2. the solve and the posterior ----------------------------------------------------------------------------------------------
def _check_posterior(L, X0, C0, cnt0, y, idx, rot0, tran0, bs, f, gate=rb.GATE, form=False):
    """The handle's state after `f` against a reference step from the state before it, AT THE DEVICE'S POSE, with bounds of 8 times
    float64 numpy's own errors on this very case; classes exact; every outlier's landmark untouched, byte for byte."""
    n = len(X0)
    rows = np.arange(n) if idx is None else idx
    ref, errs = rb.qualify_posterior(X0[rows], C0[rows], y, rot0, tran0, f.rot, f.tran, bs, D, gate, form)
    assert _counts(f) == ref.counts(), (_counts(f), ref.counts())
    assert (f.n_used, f.n_outlier) == (ref.eq.n_used, ref.eq.n_outlier)
    X1, C1 = L.get()
    touched = np.zeros(n, dtype=bool)
    touched[rows[ref.cls == rb.FUSED]] = True
    assert np.array_equal(L.counts(), cnt0 + touched.astype(np.uint32))
    assert X1[~touched].tobytes() == X0[~touched].tobytes() and C1[~touched].tobytes() == C0[~touched].tobytes()
    with np.errstate(invalid="ignore"):
        outlier = rows[np.asarray(ref.chi2 > D * D) & (ref.cls != rb.BEHIND)]   # an observation behind the frame is not used at all
    assert len(outlier) == f.n_outlier and not touched[outlier].any()           # all of them gated, none rewritten
    assert np.array_equal(np.isnan(f.chi2), ref.cls == rb.SKIPPED)
    assert np.array_equal(f.cov, f.cov.T)
    err = np.array(lr.post_errors(X1[rows], C1[rows], f.chi2, f.cov, ref, X0[rows], C0[rows]))
    bound = 8.0 * np.array(errs)
    assert (err <= bound).all(), f"errors {err} (X+, Sigma+, chi2, Sigma_c), bounds {bound}"
    return ref, err, bound


def _run_solve(n, indexed):
    s = rb.solve_scene(n)
    idx = lr.subset(n) if indexed else None
    rows = np.arange(n) if idx is None else idx
    if indexed:
        noise, _ = lr.freeze(s.X[rows], s.cov[rows], s.y[rows], s.rot0, s.tran0, s.bearing_sigma)
        rot_r, tran_r, eq_r, _ = rb.solve(s.X[rows], s.cov[rows], s.y[rows], noise, s.rot0, s.tran0, D)
    else:
        _, _, rot_r, tran_r, eq_r, _ = rb.solve_reference(n)
    with api.Landmarks(0) as L:
        L.set(s.X, s.cov)
        X0, C0 = L.get()
        f = L.register_robust(s.y[rows], s.rot0, s.tran0, D, s.bearing_sigma, idx=idx, options=_tight(), return_chi2=True)
        dp = np.concatenate([f.rot - rot_r, f.tran - tran_r])
        maha2 = float(dp @ eq_r.H @ dp)
        print(f"n = {n} {'indexed' if indexed else 'dense'}: {f.summary.termination} after {f.summary.num_iterations} iterations, "
              f"(p - p*)^T H (p - p*) = {maha2:.3e}, {f.n_outlier} outliers")
        assert maha2 <= 1e-6
        ref, err, bound = _check_posterior(L, X0, C0, np.zeros(len(X0), dtype=np.uint32), s.y[rows], idx, s.rot0, s.tran0, s.bearing_sigma, f)
        print(f"    posterior errors {err} (X+, Sigma+, chi2, Sigma_c), bounds {bound}, counts {_counts(f)}")
        planted = np.isin(rows, rb.planted(n, 10))
        assert (ref.cls[planted] == rb.GATED).all() and f.n_fused >= len(rows) // 2


@pytest.mark.parametrize("n", rb.SOLVE_SIZES)
def test_solve_and_posterior_against_long_double(n):
    _run_solve(n, False)
    if n == 513:
        _run_solve(n, True)


@pytest.mark.parametrize("n", rb.SOLVE_LONG)
def test_solve_and_posterior_on_one_block(monkeypatch, n):
    monkeypatch.setenv("SBA_RESECT_GRID", "1")
    _run_solve(n, False)


# ---- 2b. planted rows of every class ---------------------------------------------------------------------------------------------
def _displaced(y, angle):
    """y turned by `angle` about an axis across it."""
    k = np.cross(y, [0.3, -0.5, 0.8])
    k = k / np.linalg.norm(k)
    return y * np.cos(angle) + np.cross(k, y) * np.sin(angle)


def _plant(n):
    """tests/test_gpu_landmark_register.py's 14 planted rows on the robust solve scene, whose every tenth bearing is a wrong match
    already: five skipped kinds, one behind, eight more displaced bearings."""
    s = rb.solve_scene(n)
    X, cov, y = s.X.copy(), s.cov.copy(), s.y.copy()
    at = lambda frac: min(n - 1, int(frac * n))
    skipped = {"inf row": at(0.01), "NaN in X": at(0.26), "NaN in Sigma": at(0.34), "negative variance": at(0.51), "zero bearing": n - 1}
    cov[skipped["inf row"]] = [np.inf, np.inf, np.inf, 0, 0, 0]
    X[skipped["NaN in X"], 2] = np.nan
    cov[skipped["NaN in Sigma"], 5] = np.nan
    cov[skipped["negative variance"]] = [-1e-4, -2e-4, -1e-4, 0, 0, 0]
    y[skipped["zero bearing"]] = 0.0
    behind = at(0.68)
    y[behind] = -y[behind]
    gated = [at(v) for v in (0.02, 0.13, 0.27, 0.40, 0.55, 0.70, 0.85, 0.99)]
    for i in gated:
        y[i] = _displaced(s.y[i], 0.2)
    planted = sorted(set(skipped.values()) | {behind} | set(gated))
    assert len(planted) == 14
    return s, X, cov, y, sorted(skipped.values()), behind, gated, planted


@pytest.mark.parametrize("n,grid", [(513, None), (1537, "1")])
def test_planted_rows_of_every_class(monkeypatch, n, grid):
    """SKIPPED and BEHIND rows among the wrong matches, through the robust accumulate's own selection of the observations it does
    not use: at the given pose the counts are exact, chi2 is NaN exactly on the skipped rows, the planted rows and their counts
    are untouched byte for byte; then the solve against the reference's minimiser over the same rows, and one evaluation."""
    if grid:
        monkeypatch.setenv("SBA_RESECT_GRID", grid)
    s, X, cov, y, skipped, behind, gated, planted = _plant(n)
    bs = s.bearing_sigma
    rot, tran = s.truth.rot, s.truth.tran
    idx = np.array(sorted(set(planted) | set(range(0, n, 4))), dtype=np.int64)
    zeros = np.zeros(n, dtype=np.uint32)
    with np.errstate(all="ignore"):
        noise, cls = lr.freeze(X, cov, y, s.rot0, s.tran0, bs)
        rot_r, tran_r, eq_r, _ = rb.solve(X, cov, y, noise, s.rot0, s.tran0, D)
        noise_i, _ = lr.freeze(X[idx], cov[idx], y[idx], s.rot0, s.tran0, bs)
        eq_i = rb.evaluate(X[idx], cov[idx], y[idx], noise_i, s.rot0, s.tran0, D)
        eq_0 = rb.evaluate(X, cov, y, noise, s.rot0, s.tran0, D)
    assert np.array_equal(np.flatnonzero(cls == lr.SKIPPED), skipped) and np.array_equal(np.flatnonzero(cls == lr.BEHIND), [behind])
    with api.Landmarks(0) as L:
        for form, ii in (("dense", None), ("indexed", idx)):
            rows = np.arange(n) if ii is None else ii
            L.set(X, cov)
            X0, C0 = L.get()
            f = L.register_robust(y[rows], rot, tran, D, bs, idx=ii, options=_at_pose(), return_chi2=True)
            assert f.summary.num_evaluations == 1 and np.array_equal(f.rot, rot) and np.array_equal(f.tran, tran), form
            with np.errstate(all="ignore"):
                ref, err, bound = _check_posterior(L, X0, C0, zeros, y[rows], ii, rot, tran, bs, f)
            print(f"n = {n} {form} at the given pose: counts {_counts(f)}, used {f.n_used}, outliers {f.n_outlier}, errors {err}, bounds {bound}")
            where = {int(r): j for j, r in enumerate(rows)}
            assert all(ref.cls[where[i]] == rb.SKIPPED for i in skipped) and ref.cls[where[behind]] == rb.BEHIND
            assert all(ref.cls[where[i]] == rb.GATED for i in gated)
            assert f.n_skipped == 5 and f.n_behind == 1 and f.n_used == len(rows) - 6 and f.n_gated >= 8
            assert f.n_outlier == ref.eq.n_outlier and f.n_outlier >= 8
            assert np.array_equal(np.flatnonzero(np.isnan(f.chi2)), np.array([where[i] for i in skipped]))
            X1, C1 = L.get()
            for i in planted:
                assert X1[i].tobytes() == X0[i].tobytes() and C1[i].tobytes() == C0[i].tobytes(), (form, i)
            assert not L.counts()[planted].any(), form
        # the solve from the start, dense: the users' case
        L.set(X, cov)
        X0, C0 = L.get()
        f = L.register_robust(y, s.rot0, s.tran0, D, bs, options=_tight(), return_chi2=True)
        dp = np.concatenate([f.rot - rot_r, f.tran - tran_r])
        maha2 = float(dp @ eq_r.H @ dp)
        print(f"n = {n} solved: {f.summary.termination} after {f.summary.num_iterations} iterations, (p - p*)^T H (p - p*) = {maha2:.3e}, "
              f"counts {_counts(f)}, outliers {f.n_outlier}")
        assert maha2 <= 1e-6
        with np.errstate(all="ignore"):
            ref, _, _ = _check_posterior(L, X0, C0, zeros, y, None, s.rot0, s.tran0, bs, f)
        assert f.n_skipped == 5 and f.n_behind == 1 and f.n_used == n - 6
        assert all(ref.cls[i] == rb.GATED for i in gated)
        assert np.array_equal(np.flatnonzero(np.isnan(f.chi2)), np.array(skipped))
        X1, C1 = L.get()
        for i in planted:
            assert X1[i].tobytes() == X0[i].tobytes() and C1[i].tobytes() == C0[i].tobytes(), i
        assert not L.counts()[planted].any()
        # one evaluation at the start, both forms
        L.set(X, cov)
        for ii, want in ((None, eq_0), (idx, eq_i)):
            e = L.eval_register_robust(y if ii is None else y[ii], s.rot0, s.tran0, D, bearing_sigma=bs, idx=ii)
            assert (e.n_used, e.n_behind, e.n_outlier) == (want.n_used, want.n_behind, want.n_outlier)
            assert e.n_used == (n if ii is None else len(ii)) - 6
            assert np.isfinite(e.H).all() and np.isfinite(e.g).all() and np.isfinite(e.cost) and np.array_equal(e.H, e.H.T)
            err = np.array(lr.eq_errors(e, want))
            print(f"n = {n} evaluation at the start: errors {err}, bounds {_eval_bounds()}")
            assert (err <= _eval_bounds()).all(), (err, _eval_bounds())


# ---- 3. the demonstration --------------------------------------------------------------------------------------------------------
def test_the_robust_pose_is_closer_to_the_truth_than_the_plain_register():
    """The n = 513 scene with its wrong matches (tests/test_landmark_register_robust_host_cpu.py shows on the reference alone that
    it separates the two by a factor of 10): distances from the truth in the metric of the robust reference's H."""
    n = rb.DEMO_N
    s = rb.solve_scene(n)
    _, _, _, _, eq_r, _ = rb.solve_reference(n)
    with api.Landmarks(0) as L:
        L.set(s.X, s.cov)
        robust = L.register_robust(s.y, s.rot0, s.tran0, D, s.bearing_sigma, apply=False, options=_tight())
        plain = L.register(s.y, s.rot0, s.tran0, s.bearing_sigma, apply=False, options=api.default_lm_options(huber_delta=0.0, **TIGHT))
    d_rb, d_pl = rb.pose_distance2(robust.rot, robust.tran, s, eq_r.H), rb.pose_distance2(plain.rot, plain.tran, s, eq_r.H)
    print(f"squared distance from the truth in the robust H: register_robust {d_rb:.3f}, register {d_pl:.3f}")
    assert d_pl > d_rb


# ---- 4. bytes --------------------------------------------------------------------------------------------------------------------
def test_dry_run_indexed_form_fresh_handles_and_histories_return_the_same_bytes():
    n = 513
    s = rb.solve_scene(n)
    other = lr.solve_scene(65)
    kw = dict(huber_delta=D, bearing_sigma=s.bearing_sigma, options=_tight(), return_chi2=True)
    with api.Landmarks(0) as A, api.Landmarks(0) as B, api.Landmarks(0) as Dn:
        for H in (A, B, Dn):
            H.set(s.X, s.cov)
        before = _state(A)
        dry = A.register_robust(s.y, s.rot0, s.tran0, apply=False, **kw)
        assert _state(A) == before                                              # the dry run leaves get() and counts() as they were
        wet = B.register_robust(s.y, s.rot0, s.tran0, **kw)                     # a twin handle, a fresh one
        assert _result_bytes(dry) == _result_bytes(wet) and _state(B) != before
        after = _state(B)
        ind = Dn.register_robust(s.y, s.rot0, s.tran0, idx=np.arange(n, dtype=np.int64), **kw)
        assert _result_bytes(ind) == _result_bytes(wet) and _state(Dn) == after  # indexed over arange(n) equals dense
        again = A.register_robust(s.y, s.rot0, s.tran0, **kw)                   # after a dry run on the same handle: run to run
        assert _result_bytes(again) == _result_bytes(wet) and _state(A) == after
        # other passes on the handle in between: another map, register, fuse, prune
        B.set(other.X, other.cov)
        B.register(other.y, other.rot0, other.tran0, other.bearing_sigma, options=api.default_lm_options(huber_delta=0.0))
        B.fuse(other.y, other.truth.rot, other.truth.tran, 1e-3)
        B.prune(max_score=1e-3)
        B.set(s.X, s.cov)
        assert _result_bytes(B.register_robust(s.y, s.rot0, s.tran0, **kw)) == _result_bytes(wet) and _state(B) == after
        # evaluations: run to run, arange(n) against dense
        A.set(s.X, s.cov)
        e1 = A.eval_register_robust(s.y, s.rot0, s.tran0, D, bearing_sigma=1e-3)
        e2 = A.eval_register_robust(s.y, s.rot0, s.tran0, D, bearing_sigma=1e-3)
        e3 = A.eval_register_robust(s.y, s.rot0, s.tran0, D, bearing_sigma=1e-3, idx=np.arange(n, dtype=np.int64))
        assert _eq_bytes(e1) == _eq_bytes(e2) == _eq_bytes(e3)


@pytest.mark.parametrize("n", (512, 513))
def test_device_bearings_return_the_host_bearings_bytes(n):
    """bearings_device, a torch tensor's address, with chi2 on the device: the dense form over an even n reads the caller's rows in
    place, over an odd n or from a pointer that is not 16-byte aligned it copies them device to device first, the indexed form
    always reads in place -- all byte for byte what host bearings give."""
    import torch
    s = rb.solve_scene(513)
    X, cov, y = s.X[:n], s.cov[:n], np.ascontiguousarray(s.y[:n])
    idx = lr.subset(n)
    kw = dict(huber_delta=D, bearing_sigma=s.bearing_sigma, options=_tight())
    dev = torch.device("cuda:0")
    with api.Landmarks(0) as A, api.Landmarks(0) as B:
        for form, ii in (("dense", None), ("indexed", idx)):
            rows = np.array(y if ii is None else y[ii])                         # a writable copy: torch.from_numpy wants one
            m = len(rows)
            buf = torch.empty(3 * m + 1, dtype=torch.float64, device=dev)
            aligned, shifted = buf[:3 * m], buf[1:]                             # the second one starts 8 bytes off a 16-byte boundary
            for name, t in (("aligned", aligned), ("shifted", shifted)):
                t.copy_(torch.from_numpy(rows.reshape(-1)))
                # chi2 between guard cells: 16 bytes in, aligned, two guards on either side; 8 bytes in, off a 16-byte boundary (with
                # aligned bearings chi2 then goes through the scratch and a device-to-device copy), one guard before and three behind
                for off in (2, 1):
                    chi2_dev = torch.full((m + 4,), -7.0, dtype=torch.float64, device=dev)
                    assert chi2_dev.data_ptr() % 16 == 0
                    torch.cuda.synchronize()
                    A.set(X, cov)
                    B.set(X, cov)
                    host = A.register_robust(rows, s.rot0, s.tran0, idx=ii, return_chi2=True, **kw)
                    got = B.register_robust(None, s.rot0, s.tran0, idx=ii, bearings_device=t.data_ptr(), chi2_device=chi2_dev.data_ptr() + 8 * off, **kw)
                    torch.cuda.synchronize()
                    all_chi2 = chi2_dev.cpu().numpy()
                    chi2 = np.ascontiguousarray(all_chi2[off:off + m])
                    assert (all_chi2[:off] == -7.0).all() and (all_chi2[off + m:] == -7.0).all(), (form, name, off, all_chi2[:off], all_chi2[off + m:])
                    assert _result_bytes(got, chi2) == _result_bytes(host), (form, name, off)
                    assert _state(A) == _state(B), (form, name, off)
                assert torch.equal(t.cpu(), torch.from_numpy(rows.reshape(-1))), (form, name)      # the caller's rows are only read
                eh = A.eval_register_robust(rows, s.rot0, s.tran0, D, bearing_sigma=1e-3, idx=ii)
                ed = B.eval_register_robust(None, s.rot0, s.tran0, D, bearing_sigma=1e-3, idx=ii, bearings_device=t.data_ptr())
                assert _eq_bytes(eh) == _eq_bytes(ed), (form, name)
                # without chi2
                B.set(X, cov)
                got = B.register_robust(None, s.rot0, s.tran0, idx=ii, bearings_device=t.data_ptr(), apply=False, **kw)
                assert _result_bytes(got, host.chi2) == _result_bytes(host) and got.chi2 is None, (form, name)


def test_results_across_grids(monkeypatch):
    """At a given pose (max_num_iterations = 0) everything that does not pass through the reduction -- X+, chi2, the classes, the
    counts -- is byte-identical for SBA_RESECT_GRID 1, 2, 3 and unset.  Sigma_c = H^-1 carries the reduction's bits into Sigma+: those
    two, and the whole solved result, agree within the posterior's bounds, and are byte-identical again at a fixed grid."""
    n = 1537
    s = rb.solve_scene(n)
    seen, solved = [], []
    with api.Landmarks(0) as L:
        for grid in GRIDS:
            if grid is None:
                monkeypatch.delenv("SBA_RESECT_GRID", raising=False)
            else:
                monkeypatch.setenv("SBA_RESECT_GRID", grid)
            L.set(s.X, s.cov)
            X0, C0 = L.get()
            f = L.register_robust(s.y, s.truth.rot, s.truth.tran, D, s.bearing_sigma, options=_at_pose(), return_chi2=True)
            assert f.summary.num_evaluations == 1
            _check_posterior(L, X0, C0, np.zeros(n, dtype=np.uint32), s.y, None, s.truth.rot, s.truth.tran, s.bearing_sigma, f)
            X1, C1 = L.get()
            seen.append(X1.tobytes() + f.chi2.tobytes() + L.counts().tobytes() + repr(_counts(f) + (f.n_used, f.n_outlier)).encode())
            L.set(s.X, s.cov)
            g = L.register_robust(s.y, s.truth.rot, s.truth.tran, D, s.bearing_sigma, options=_at_pose(), return_chi2=True)
            assert _result_bytes(g) == _result_bytes(f) and L.get()[1].tobytes() == C1.tobytes()      # a fixed grid: the same bits
            L.set(s.X, s.cov)
            h = L.register_robust(s.y, s.rot0, s.tran0, D, s.bearing_sigma, options=_tight(), return_chi2=True)
            _check_posterior(L, X0, C0, np.zeros(n, dtype=np.uint32), s.y, None, s.rot0, s.tran0, s.bearing_sigma, h)
            solved.append(h)
    assert all(v == seen[0] for v in seen)
    _, _, rot_r, tran_r, eq_r, _ = rb.solve_reference(n)
    for h in solved:
        dp = np.concatenate([h.rot - rot_r, h.tran - tran_r])
        assert float(dp @ eq_r.H @ dp) <= 1e-6
        assert _counts(h) == _counts(solved[0]) and h.n_outlier == solved[0].n_outlier


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_map_as_it_was():
    import torch
    s = rb.solve_scene(65)
    n = 65
    with api.Landmarks(0) as L:
        L.set(s.X, s.cov)
        L.register_robust(s.y, s.rot0, s.tran0, D, s.bearing_sigma, options=_tight())      # counts are no longer zero
        before = _state(L)
        ok = dict(bearings=s.y, rot=s.rot0, tran=s.tran0, huber_delta=D, bearing_sigma=1e-3)
        nan3 = np.array([0.0, np.nan, 0.0])
        inv, num = cabi.SBA_ERR_INVALID_ARG, cabi.SBA_ERR_NUMERIC
        cases = [
            (dict(ok, bearing_sigma=-1e-3), inv),
            (dict(ok, bearing_sigma=np.inf), inv),
            (dict(ok, chi2_gate=0.0), inv),
            (dict(ok, chi2_gate=np.nan), inv),
            (dict(ok, chi2_gate=np.inf), inv),                                                          # above delta^2
            (dict(ok, chi2_gate=1.01 * D * D), inv),
            (dict(ok, huber_delta=0.0, chi2_gate=1.0), inv),
            (dict(ok, huber_delta=-1.0, chi2_gate=1.0), inv),
            (dict(ok, huber_delta=np.inf, chi2_gate=1.0), inv),
            (dict(ok, huber_delta=np.nan, chi2_gate=1.0), inv),
            (dict(ok, bearings=s.y[:-1]), inv),                                                         # dense with m != n
            (dict(ok, bearings=s.y[:3], idx=[0, 1, 1]), inv),
            (dict(ok, bearings=s.y[:3], idx=[2, 1, 0]), inv),
            (dict(ok, bearings=s.y[:3], idx=[0, 1, n]), inv),
            (dict(ok, bearings=s.y[:3], idx=[-1, 1, 2]), inv),
            (dict(ok, rot=nan3), num),
            (dict(ok, tran=np.array([0.0, 0.0, -np.inf])), num),
        ]
        for kw, code in cases:
            with pytest.raises(api.SbaError) as ei:
                L.register_robust(**kw)
            assert ei.value.code == code and ei.value.message, kw
            assert _state(L) == before, kw
        for kw, code in ((dict(bearing_sigma=-1.0), inv), (dict(rot_ref=nan3), num), (dict(idx=np.arange(n)[::-1]), inv),
                         (dict(huber_delta=0.0), inv), (dict(huber_delta=np.nan), inv)):
            args = dict(dict(huber_delta=D), **kw)
            with pytest.raises(api.SbaError) as ei:
                L.eval_register_robust(s.y, s.rot0, s.tran0, **args)
            assert ei.value.code == code, kw
            assert _state(L) == before, kw
        # the device twins: the same refusals, and a device pointer that is not 8-byte aligned
        y_dev = torch.from_numpy(np.array(s.y).reshape(-1)).to("cuda:0")
        torch.cuda.synchronize()
        dev = dict(bearings=None, rot=s.rot0, tran=s.tran0, huber_delta=D, bearing_sigma=1e-3, bearings_device=y_dev.data_ptr())
        for kw, code in ((dict(dev, chi2_gate=np.inf), inv), (dict(dev, chi2_gate=1.01 * D * D), inv), (dict(dev, huber_delta=-2.0, chi2_gate=1.0), inv),
                         (dict(dev, m=n - 1), inv), (dict(dev, bearings_device=y_dev.data_ptr() + 4), inv), (dict(dev, rot=nan3), num)):
            with pytest.raises(api.SbaError) as ei:
                L.register_robust(**kw)
            assert ei.value.code == code and ei.value.message, kw
            assert _state(L) == before, kw
        # after the freeze: fewer than 3 observations take part
        few = np.zeros_like(s.y)
        few[[5, 40]] = s.y[[5, 40]]
        with pytest.raises(api.SbaError) as ei:
            L.register_robust(few, s.rot0, s.tran0, D, 1e-3, options=_tight())
        assert ei.value.code == num and "pose not determined" in ei.value.message and _state(L) == before
        assert L.eval_register_robust(few, s.rot0, s.tran0, D).n_used == 2      # an evaluation is not refused
        # the non-robust register still refuses a loss, and the handle stays usable
        with pytest.raises(api.SbaError) as ei:
            L.register(s.y, s.rot0, s.tran0, 1e-3, options=api.default_lm_options(huber_delta=D))
        assert ei.value.code == cabi.SBA_ERR_UNSUPPORTED and _state(L) == before
        assert L.register_robust(s.y, s.rot0, s.tran0, D, s.bearing_sigma, options=_tight()).n_fused > 0
    # after the solve: three landmarks on one line through the frame's centre leave the rotation about it free
    Xl = np.array([[2.0, 0, 0], [3.0, 0, 0], [5.0, 0, 0]])
    Cl = np.tile([1e-2, 1e-4, 1e-4, 0, 0, 0], (3, 1))
    yl = np.tile([1.0, 0, 0], (3, 1))
    with api.Landmarks(0) as L:
        L.set(Xl, Cl)
        before = _state(L)
        with pytest.raises(api.SbaError) as ei:
            L.register_robust(yl, np.zeros(3), np.zeros(3), D, 1e-3, options=_at_pose())
        assert ei.value.code == num and "positive definite" in ei.value.message and _state(L) == before


def test_empty_map_and_no_observations():
    s = rb.solve_scene(65)
    with api.Landmarks(0) as L:
        f = L.register_robust(np.zeros((0, 3)), s.rot0, s.tran0, D, return_chi2=True)
        assert _counts(f) == (0, 0, 0, 0, 0) and f.n_used == 0 and f.n_outlier == 0 and np.array_equal(f.rot, s.rot0)
        assert f.chi2.shape == (0,) and not f.cov.any()
        L.set(s.X, s.cov)
        before = _state(L)
        e = L.eval_register_robust(np.zeros((0, 3)), s.rot0, s.tran0, D, idx=np.zeros(0, dtype=np.int64))
        assert e.n_used == 0 and e.n_outlier == 0 and not e.H.any() and e.cost == 0.0 and _state(L) == before


# ---- 6. registration on a map that was edited ------------------------------------------------------------------------------------
def _register_like_a_fresh_set(L, y, rot, tran):
    """Every registration entry point on L gives the bytes, and leaves the state, of a fresh handle set from L's rows: prune and
    append swap the planes and change the size under scratch buffers sized for the map before, and nothing of that may show."""
    import torch
    X, Cv = L.get()
    k = L.counts()
    n = len(X)
    y = np.ascontiguousarray(y)
    y_dev = torch.from_numpy(np.array(y).reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    plain = api.default_lm_options(huber_delta=0.0, **TIGHT)
    plain_bytes = lambda f: (b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in (f.rot, f.tran, f.cov, f.chi2))
                             + repr(_counts(f) + (f.n_used,)).encode())
    with api.Landmarks(0) as T:
        T.set(X, Cv, 1.0)
        assert _state(T) == X.tobytes() + Cv.tobytes() + np.zeros(n, dtype=np.uint32).tobytes()

        def alike():
            X1, C1 = L.get()
            X2, C2 = T.get()
            return X1.tobytes() == X2.tobytes() and C1.tobytes() == C2.tobytes() and np.array_equal(L.counts() - k, T.counts())

        a, b = (H.eval_register(y, rot, tran, bearing_sigma=1e-3) for H in (L, T))
        assert a.H.tobytes() + a.g.tobytes() == b.H.tobytes() + b.g.tobytes() and (a.cost, a.n_used, a.n_behind) == (b.cost, b.n_used, b.n_behind)
        assert a.n_used > n // 2
        a, b = (H.eval_register_robust(y, rot, tran, D, bearing_sigma=1e-3) for H in (L, T))
        assert _eq_bytes(a) == _eq_bytes(b)
        a, b = (H.eval_register_robust(None, rot, tran, D, bearing_sigma=1e-3, bearings_device=y_dev.data_ptr()) for H in (L, T))
        assert _eq_bytes(a) == _eq_bytes(b)
        a, b = (H.register(y, rot, tran, 1e-3, lr.GATE, apply=False, options=plain, return_chi2=True) for H in (L, T))
        assert plain_bytes(a) == plain_bytes(b) and alike()
        a, b = (H.register_robust(y, rot, tran, D, 1e-3, apply=False, options=_tight(), return_chi2=True) for H in (L, T))
        assert _result_bytes(a) == _result_bytes(b) and alike()
        a, b = (H.register(y, rot, tran, 1e-3, lr.GATE, options=plain, return_chi2=True) for H in (L, T))
        assert plain_bytes(a) == plain_bytes(b) and alike() and a.n_fused > n // 2
        chi2 = [torch.full((n + 4,), -7.0, dtype=torch.float64, device="cuda:0") for _ in range(2)]
        torch.cuda.synchronize()
        a, b = (H.register_robust(None, rot, tran, D, 1e-3, options=_tight(), bearings_device=y_dev.data_ptr(), chi2_device=c.data_ptr() + 16)
                for H, c in zip((L, T), chi2))
        torch.cuda.synchronize()
        ca, cb = (c.cpu().numpy() for c in chi2)
        assert (ca[:2] == -7.0).all() and (ca[n + 2:] == -7.0).all()
        assert _result_bytes(a, ca[2:n + 2]) == _result_bytes(b, cb[2:n + 2]) and alike() and a.n_fused > 0
        a, b = (H.register_robust(y, rot, tran, D, 1e-3, options=_tight(), return_chi2=True) for H in (L, T))
        assert _result_bytes(a) == _result_bytes(b) and alike()


def test_registration_after_prune_and_append_equals_a_fresh_handle():
    n = 4097
    X, cov, frames, (rot, tran) = le.edit_map(n)
    R = rr.rotmat(rot, np.float64)
    Xa, Ca = le.extra_rows(513)
    ya = Xa @ R.T - tran                                                        # the appended landmarks' exact bearings, any length
    with api.Landmarks(0) as L:
        L.set(X, cov, le.COV_SCALE)
        for y, idx in frames:
            L.fuse(y, rot, tran, 1e-3, lf.GATE, idx=idx)
        y = frames[0][0]
        keep = le.mask("alternating", n)
        assert L.prune(mask=keep).n_kept == 2049                                # the planes have swapped, n is odd
        y = y[keep]
        _register_like_a_fresh_set(L, y, rot, tran)
        L.append(Xa, Ca, le.COV_SCALE)                                          # swapped again, n = 2562 over a scratch sized for 2049
        y = np.concatenate([y, ya])
        assert L.size == len(y) == 2562
        _register_like_a_fresh_set(L, y, rot, tran)
        keep = le.mask("straddle", L.size)                                      # far below everything sized so far, odd again
        assert L.prune(mask=keep).n_kept == 75
        _register_like_a_fresh_set(L, y[keep], rot, tran)
