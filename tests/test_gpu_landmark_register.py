"""GPU: the joint registration of a frame against the landmark map (api.Landmarks.eval_register / register) against the long-double
reference of tests/landmark_register_reference.py, on the cases tests/test_landmark_register_host_cpu.py qualifies (float64 numpy
classifies every observation alike there and no eliminated depth sits on 0): the vector-per-lane, wave and block edges, several
grid-stride steps with a partial last wave (SBA_RESECT_GRID=1), dense and indexed, with and without the bearing's noise, the nine
rotations where the kernels' frame changes, the noise frozen 1e-2 rad off the evaluation pose.  Counts are exact; H, g and the
cost, and X+, Sigma+, chi2 and the pose covariance, are held to 8 times float64 numpy's own error on the same cases, measured in
this run.  The solve against the reference's own minimiser; the posterior at the device's pose; planted
rows of every class; bytes across handles, forms, histories and grids; refusals; two frames in sequence."""
from functools import lru_cache

import numpy as np
import pytest

import landmark_fusion_reference as lf
import landmark_register_reference as lr
import pose_edges
import resection_reference as rr
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

pytestmark = pytest.mark.gpu

TIGHT = dict(function_tolerance=1e-30, parameter_tolerance=1e-13, gradient_tolerance=1e-13, max_num_iterations=100, huber_delta=0.0)
GRIDS = (None, "1", "2", "3", "5")
_worst_eval = np.zeros(3)
_worst_post = np.zeros(4)


def _tight():
    return api.default_lm_options(**TIGHT)


def _at_pose():
    """max_num_iterations = 0: register at the given pose."""
    return api.default_lm_options(huber_delta=0.0, max_num_iterations=0)


@lru_cache(maxsize=None)
def _eval_bounds():
    """8 times float64 numpy's worst errors against long double on the same evaluations, measured in this run: a different order of
    operations and fused multiply-adds are what the factor covers, as in sections 3.19 and 3.20."""
    return 8.0 * np.array(lr.measured_eval_errors())


def _state(L):
    X, Cv = L.get()
    return X.tobytes() + Cv.tobytes() + L.counts().tobytes()


def _counts(f):
    return (f.n_obs, f.n_skipped, f.n_behind, f.n_gated, f.n_fused)


def _result_bytes(f):
    return b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in (f.rot, f.tran, f.cov, f.chi2)) + repr(_counts(f) + (f.n_used,)).encode()


# ---- 1. evaluation parity --------------------------------------------------------------------------------------------------------
def _run_eval_size(n):
    global _worst_eval
    with api.Landmarks(0) as L:
        for s in lr.scenes((n,)):
            L.set(s.X, s.cov)
            before = _state(L)
            for bs in lr.BEARING_SIGMAS:
                for form, idx in lr.forms(s):
                    _, cls, ref = lr.eval_reference(n, s.name.split()[1], bs, idx is not None)
                    got = L.eval_register(s.y if idx is None else s.y[idx], s.rot, s.tran, s.rot_ref, s.tran_ref, bs, idx=idx)
                    what = f"{s.name} bs={bs} {form}"
                    assert (got.n_used, got.n_behind) == (ref.n_used, ref.n_behind), what
                    assert got.n_used == int((cls == lr.LIVE).sum()), what
                    assert np.array_equal(got.H, got.H.T), what
                    if ref.n_used:
                        err = np.array(lr.eq_errors(got, ref))
                        assert (err <= _eval_bounds()).all(), f"{what}: errors {err}, bounds {_eval_bounds()}"
                        _worst_eval = np.maximum(_worst_eval, err)
                    else:
                        assert not got.H.any() and not got.g.any() and got.cost == 0.0, what
            assert _state(L) == before, s.name                                  # an evaluation writes nothing
    print(f"n = {n}: device worst so far H {_worst_eval[0]:.3e}, g {_worst_eval[1]:.3e}, cost {_worst_eval[2]:.3e}; bounds {_eval_bounds()}")


@pytest.mark.parametrize("n", lr.SIZES)
def test_evaluation_against_long_double(n):
    _run_eval_size(n)


@pytest.mark.parametrize("n", lr.LONG)
def test_evaluation_over_several_grid_stride_steps(monkeypatch, n):
    monkeypatch.setenv("SBA_RESECT_GRID", "1")
    _run_eval_size(n)


# ---- 2. the solve and 3. the posterior -------------------------------------------------------------------------------------------
def _check_posterior(L, X0, C0, cnt0, y, idx, rot0, tran0, bs, f, gate=lr.GATE, form=False):
    """The handle's state after `f` against a reference step from the state before it, AT THE DEVICE'S POSE (so the stopping point
    does not enter), with bounds of 8 times float64 numpy's own errors on this very case."""
    global _worst_post
    n = len(X0)
    rows = np.arange(n) if idx is None else idx
    ref, errs = lr.qualify_posterior(X0[rows], C0[rows], y, rot0, tran0, f.rot, f.tran, bs, gate, form)
    assert _counts(f) == ref.counts(), (_counts(f), ref.counts())
    assert f.n_used == ref.eq.n_used
    X1, C1 = L.get()
    touched = np.zeros(n, dtype=bool)
    touched[rows[ref.cls == lr.FUSED]] = True
    assert np.array_equal(L.counts(), cnt0 + touched.astype(np.uint32))
    assert X1[~touched].tobytes() == X0[~touched].tobytes() and C1[~touched].tobytes() == C0[~touched].tobytes()
    assert np.array_equal(np.isnan(f.chi2), ref.cls == lr.SKIPPED)
    assert np.array_equal(f.cov, f.cov.T)
    err = np.array(lr.post_errors(X1[rows], C1[rows], f.chi2, f.cov, ref, X0[rows], C0[rows]))
    bound = 8.0 * np.array(errs)
    assert (err <= bound).all(), f"errors {err} (X+, Sigma+, chi2, Sigma_c), bounds {bound}"
    _worst_post = np.maximum(_worst_post, err / np.maximum(np.array(errs), 1e-300))
    return ref, err, bound


def _run_solve(n, indexed):
    s = lr.solve_scene(n)
    idx = lr.subset(n) if indexed else None
    rows = np.arange(n) if idx is None else idx
    if indexed:
        noise, _ = lr.freeze(s.X[rows], s.cov[rows], s.y[rows], s.rot0, s.tran0, s.bearing_sigma)
        rot_r, tran_r, eq_r, _ = lr.solve(s.X[rows], s.cov[rows], s.y[rows], noise, s.rot0, s.tran0)
    else:
        _, _, rot_r, tran_r, eq_r, _ = lr.solve_reference(n)
    with api.Landmarks(0) as L:
        L.set(s.X, s.cov)
        X0, C0 = L.get()
        f = L.register(s.y[rows], s.rot0, s.tran0, s.bearing_sigma, lr.GATE, idx=idx, options=_tight(), return_chi2=True)
        dp = np.concatenate([f.rot - rot_r, f.tran - tran_r])
        maha2 = float(dp @ eq_r.H @ dp)
        print(f"n = {n} {'indexed' if indexed else 'dense'}: {f.summary.termination} after {f.summary.num_iterations} iterations, "
              f"(p - p*)^T H (p - p*) = {maha2:.3e}")
        assert maha2 <= 1e-6                                                    # a thousandth of a standard deviation
        ref, err, bound = _check_posterior(L, X0, C0, np.zeros(len(X0), dtype=np.uint32), s.y[rows], idx, s.rot0, s.tran0, s.bearing_sigma, f)
        print(f"    posterior errors {err} (X+, Sigma+, chi2, Sigma_c), bounds {bound}, counts {_counts(f)}")
        assert f.n_fused >= len(rows) // 2


@pytest.mark.parametrize("n", lr.SOLVE_SIZES)
def test_solve_and_posterior_against_long_double(n):
    _run_solve(n, False)
    if n == 513:
        _run_solve(n, True)


@pytest.mark.parametrize("n", lr.SOLVE_LONG)
def test_solve_and_posterior_over_several_grid_stride_steps(monkeypatch, n):
    monkeypatch.setenv("SBA_RESECT_GRID", "1")
    _run_solve(n, False)
    _run_solve(n, True)


# ---- 4. max_iterations = 0 with planted rows --------------------------------------------------------------------------------------
def _displaced(y, angle):
    """y turned by `angle` about an axis across it."""
    k = np.cross(y, [0.3, -0.5, 0.8])
    k = k / np.linalg.norm(k)
    return y * np.cos(angle) + np.cross(k, y) * np.sin(angle)


@pytest.mark.parametrize("n,grid", [(513, None), (1537, "1")])
def test_planted_rows_of_every_class_at_the_given_pose(monkeypatch, n, grid):
    """No solve runs here (displaced bearings would drag a pose that has no robust loss): rows spread over waves, blocks and steps
    are untouched byte for byte and counted in their class, chi2 is NaN exactly where skipped."""
    if grid:
        monkeypatch.setenv("SBA_RESECT_GRID", grid)
    s = lr.solve_scene(n)
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
        y[i] = _displaced(y[i], 0.2)
    planted = sorted(set(skipped.values()) | {behind} | set(gated))
    assert len(planted) == 14
    rot, tran = s.truth.rot, s.truth.tran
    with api.Landmarks(0) as L, api.Landmarks(0) as Li:
        for H in (L, Li):
            H.set(X, cov)
        X0, C0 = L.get()
        f = L.register(y, rot, tran, 0.0, lr.GATE, options=_at_pose(), return_chi2=True)
        assert f.summary.num_evaluations == 1 and np.array_equal(f.rot, rot) and np.array_equal(f.tran, tran)
        ref, _, _ = _check_posterior(L, X0, C0, np.zeros(n, dtype=np.uint32), y, None, rot, tran, 0.0, f)
        assert all(ref.cls[i] == lr.SKIPPED for i in skipped.values()) and ref.cls[behind] == lr.BEHIND
        assert all(ref.cls[i] == lr.GATED for i in gated)
        assert f.n_skipped == 5 and f.n_behind == 1 and f.n_gated >= 8 and f.n_used == n - 6
        X1, C1 = L.get()
        for i in planted:
            assert X1[i].tobytes() == X0[i].tobytes() and C1[i].tobytes() == C0[i].tobytes(), i
        assert not L.counts()[planted].any()
        assert np.array_equal(np.flatnonzero(np.isnan(f.chi2)), np.array(sorted(skipped.values())))
        # the indexed form over the planted rows and every fourth other one
        idx = np.array(sorted(set(planted) | set(range(0, n, 4))), dtype=np.int64)
        fi = Li.register(y[idx], rot, tran, 0.0, lr.GATE, idx=idx, options=_at_pose(), return_chi2=True)
        refi, _, _ = _check_posterior(Li, X0, C0, np.zeros(n, dtype=np.uint32), y[idx], idx, rot, tran, 0.0, fi)
        assert fi.n_skipped == 5 and fi.n_behind == 1 and fi.n_gated >= 8


# ---- 5. bytes --------------------------------------------------------------------------------------------------------------------
def test_dry_run_indexed_form_fresh_handles_and_histories_return_the_same_bytes():
    n = 513
    s = lr.solve_scene(n)
    other = lr.solve_scene(65)
    kw = dict(bearing_sigma=s.bearing_sigma, chi2_gate=lr.GATE, options=_tight(), return_chi2=True)
    with api.Landmarks(0) as A, api.Landmarks(0) as B, api.Landmarks(0) as D:
        for H in (A, B, D):
            H.set(s.X, s.cov)
        before = _state(A)
        dry = A.register(s.y, s.rot0, s.tran0, apply=False, **kw)
        assert _state(A) == before                                              # the dry run leaves get() and counts() as they were
        wet = B.register(s.y, s.rot0, s.tran0, **kw)                            # a twin handle, a fresh one
        assert _result_bytes(dry) == _result_bytes(wet) and _state(B) != before
        after = _state(B)
        ind = D.register(s.y, s.rot0, s.tran0, idx=np.arange(n, dtype=np.int64), **kw)
        assert _result_bytes(ind) == _result_bytes(wet) and _state(D) == after  # indexed over arange(n) equals dense
        again = A.register(s.y, s.rot0, s.tran0, **kw)                          # after a dry run on the same handle
        assert _result_bytes(again) == _result_bytes(wet) and _state(A) == after
        # set -> register -> set of the same rows -> register
        A.set(s.X, s.cov)
        assert _result_bytes(A.register(s.y, s.rot0, s.tran0, **kw)) == _result_bytes(wet) and _state(A) == after
        # another map and another pass on the handle in between
        B.set(other.X, other.cov)
        B.register(other.y, other.rot0, other.tran0, other.bearing_sigma, options=_tight())
        B.fuse(other.y, other.truth.rot, other.truth.tran, 1e-3)
        B.set(s.X, s.cov)
        assert _result_bytes(B.register(s.y, s.rot0, s.tran0, **kw)) == _result_bytes(wet) and _state(B) == after


def test_results_across_grids(monkeypatch):
    """At a given pose (max_num_iterations = 0) everything that does not pass through the reduction -- X+, chi2, the classes, the
    counts -- is byte-identical for SBA_RESECT_GRID 1, 2, 3, 5 and unset: the apply pass has no reduction.  Sigma_c = H^-1 carries the
    reduction's bits, which depend on the grid, into Sigma+: those two, and the whole solved result, agree within the posterior's
    bounds, and are byte-identical again at a fixed grid."""
    n = 1537
    s = lr.solve_scene(n)
    seen, solved = [], []
    with api.Landmarks(0) as L:
        for grid in GRIDS:
            if grid is None:
                monkeypatch.delenv("SBA_RESECT_GRID", raising=False)
            else:
                monkeypatch.setenv("SBA_RESECT_GRID", grid)
            L.set(s.X, s.cov)
            X0, C0 = L.get()
            f = L.register(s.y, s.truth.rot, s.truth.tran, s.bearing_sigma, lr.GATE, options=_at_pose(), return_chi2=True)
            _check_posterior(L, X0, C0, np.zeros(n, dtype=np.uint32), s.y, None, s.truth.rot, s.truth.tran, s.bearing_sigma, f)
            X1, C1 = L.get()
            seen.append((X1.tobytes() + f.chi2.tobytes() + L.counts().tobytes() + repr(_counts(f)).encode(), C1, f.cov))
            L.set(s.X, s.cov)
            g = L.register(s.y, s.truth.rot, s.truth.tran, s.bearing_sigma, lr.GATE, options=_at_pose(), return_chi2=True)
            assert _result_bytes(g) == _result_bytes(f) and L.get()[1].tobytes() == C1.tobytes()      # a fixed grid: the same bits
            L.set(s.X, s.cov)
            h = L.register(s.y, s.rot0, s.tran0, s.bearing_sigma, lr.GATE, options=_tight(), return_chi2=True)
            _check_posterior(L, X0, C0, np.zeros(n, dtype=np.uint32), s.y, None, s.rot0, s.tran0, s.bearing_sigma, h)
            solved.append(h)
    assert all(v[0] == seen[0][0] for v in seen)
    _, _, rot_r, tran_r, eq_r, _ = lr.solve_reference(n)
    for h in solved:
        dp = np.concatenate([h.rot - rot_r, h.tran - tran_r])
        assert float(dp @ eq_r.H @ dp) <= 1e-6
        assert _counts(h) == _counts(solved[0])


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_map_as_it_was():
    s = lr.solve_scene(65)
    n = 65
    with api.Landmarks(0) as L:
        L.set(s.X, s.cov)
        L.register(s.y, s.rot0, s.tran0, s.bearing_sigma, options=_tight())      # counts are no longer zero
        before = _state(L)
        ok = dict(bearings=s.y, rot=s.rot0, tran=s.tran0, bearing_sigma=1e-3, chi2_gate=lr.GATE)
        nan3 = np.array([0.0, np.nan, 0.0])
        cases = [
            (dict(ok, bearing_sigma=-1e-3), cabi.SBA_ERR_INVALID_ARG),
            (dict(ok, bearing_sigma=np.inf), cabi.SBA_ERR_INVALID_ARG),
            (dict(ok, chi2_gate=0.0), cabi.SBA_ERR_INVALID_ARG),
            (dict(ok, chi2_gate=np.nan), cabi.SBA_ERR_INVALID_ARG),
            (dict(ok, bearings=s.y[:-1]), cabi.SBA_ERR_INVALID_ARG),                                    # dense with m != n
            (dict(ok, bearings=s.y[:3], idx=[0, 1, 1]), cabi.SBA_ERR_INVALID_ARG),
            (dict(ok, bearings=s.y[:3], idx=[2, 1, 0]), cabi.SBA_ERR_INVALID_ARG),
            (dict(ok, bearings=s.y[:3], idx=[0, 1, n]), cabi.SBA_ERR_INVALID_ARG),
            (dict(ok, bearings=s.y[:3], idx=[-1, 1, 2]), cabi.SBA_ERR_INVALID_ARG),
            (dict(ok, rot=nan3), cabi.SBA_ERR_NUMERIC),
            (dict(ok, tran=np.array([0.0, 0.0, -np.inf])), cabi.SBA_ERR_NUMERIC),
            (dict(ok, options=api.default_lm_options()), cabi.SBA_ERR_UNSUPPORTED),                     # huber_delta = 1: a robust loss
            (dict(ok, options=api.default_lm_options(huber_delta=-1.0)), cabi.SBA_ERR_UNSUPPORTED),
        ]
        for kw, code in cases:
            with pytest.raises(api.SbaError) as ei:
                L.register(**kw)
            assert ei.value.code == code and ei.value.message, kw
            assert _state(L) == before, kw
        for kw, code in ((dict(bearing_sigma=-1.0), cabi.SBA_ERR_INVALID_ARG), (dict(rot_ref=nan3), cabi.SBA_ERR_NUMERIC),
                         (dict(idx=np.arange(n)[::-1]), cabi.SBA_ERR_INVALID_ARG)):
            with pytest.raises(api.SbaError) as ei:
                L.eval_register(s.y, s.rot0, s.tran0, **kw)
            assert ei.value.code == code, kw
            assert _state(L) == before, kw
        # after the freeze: fewer than 3 observations take part
        few = np.zeros_like(s.y)
        few[[5, 40]] = s.y[[5, 40]]
        with pytest.raises(api.SbaError) as ei:
            L.register(few, s.rot0, s.tran0, 1e-3, options=_tight())
        assert ei.value.code == cabi.SBA_ERR_NUMERIC and "pose not determined" in ei.value.message and _state(L) == before
        with pytest.raises(api.SbaError) as ei:
            L.register(s.y[[5, 40]], s.rot0, s.tran0, 1e-3, idx=[5, 40], options=_tight())
        assert ei.value.code == cabi.SBA_ERR_NUMERIC and "pose not determined" in ei.value.message and _state(L) == before
        assert L.eval_register(few, s.rot0, s.tran0).n_used == 2                # an evaluation is not refused
        # the handle stays usable
        assert L.register(s.y, s.rot0, s.tran0, s.bearing_sigma, options=_tight()).n_fused > 0
    # after the solve: three landmarks on one line through the frame's centre leave the rotation about it free -- H[0][0] is an
    # exact zero, so the factorisation fails whatever the rounding
    Xl = np.array([[2.0, 0, 0], [3.0, 0, 0], [5.0, 0, 0]])
    Cl = np.tile([1e-2, 1e-4, 1e-4, 0, 0, 0], (3, 1))
    yl = np.tile([1.0, 0, 0], (3, 1))
    with api.Landmarks(0) as L:
        L.set(Xl, Cl)
        before = _state(L)
        for opt in (_at_pose(), _tight()):
            with pytest.raises(api.SbaError) as ei:
                L.register(yl, np.zeros(3), np.zeros(3), 1e-3, options=opt)
            assert ei.value.code == cabi.SBA_ERR_NUMERIC and "positive definite" in ei.value.message and _state(L) == before
        e = L.eval_register(yl, np.zeros(3), np.zeros(3), bearing_sigma=1e-3)
        assert e.n_used == 3 and e.H[0, 0] == 0.0


def test_empty_map_and_no_observations():
    s = lr.solve_scene(65)
    with api.Landmarks(0) as L:
        f = L.register(np.zeros((0, 3)), s.rot0, s.tran0, return_chi2=True)
        assert _counts(f) == (0, 0, 0, 0, 0) and f.n_used == 0 and np.array_equal(f.rot, s.rot0) and np.array_equal(f.tran, s.tran0)
        assert f.chi2.shape == (0,) and not f.cov.any()
        L.set(s.X, s.cov)
        before = _state(L)
        f = L.register(np.zeros((0, 3)), s.rot0, s.tran0, idx=np.zeros(0, dtype=np.int64))
        assert _counts(f) == (0, 0, 0, 0, 0) and np.array_equal(f.rot, s.rot0) and _state(L) == before
        e = L.eval_register(np.zeros((0, 3)), s.rot0, s.tran0, idx=np.zeros(0, dtype=np.int64))
        assert e.n_used == 0 and not e.H.any() and e.cost == 0.0


# ---- 7. two frames in sequence ---------------------------------------------------------------------------------------------------
def test_two_frames_in_sequence():
    """Every step within the bounds of a reference step from the handle's own state; counts summed exactly; the map improves twice."""
    n = 513
    s = lr.solve_scene(n)
    rng = np.random.default_rng(515)
    rot2, tran2 = s.truth.rot + np.array([0.05, -0.03, 0.02]), s.truth.tran + np.array([0.3, -0.2, 0.1])
    Y = s.truth.X @ rr.rotmat(rot2, np.float64).T - tran2
    y2 = rr._unit(rr._unit(Y) + 1e-3 * rng.standard_normal((n, 3))) * rng.uniform(0.5, 2.0, size=(n, 1))
    start2 = (rot2 + lr.START_ROT * rr._unit(rng.standard_normal(3)), tran2 + lr.START_TRAN * rr._unit(rng.standard_normal(3)))
    frames = ((s.y, s.rot0, s.tran0, None), (y2[lr.subset(n)], start2[0], start2[1], lr.subset(n)))
    rms = [np.sqrt(np.mean(np.sum((s.X - s.truth.X) ** 2, axis=1)))]
    with api.Landmarks(0) as L:
        L.set(s.X, s.cov)
        total = np.zeros(n, dtype=np.uint32)
        for y, r0, t0, idx in frames:
            X0, C0 = L.get()
            f = L.register(y, r0, t0, 1e-3, lr.GATE, idx=idx, options=_tight(), return_chi2=True)
            ref, err, bound = _check_posterior(L, X0, C0, total, y, idx, r0, t0, 1e-3, f)
            rows = np.arange(n) if idx is None else idx
            total[rows[ref.cls == lr.FUSED]] += 1
            assert np.array_equal(L.counts(), total)
            rms.append(np.sqrt(np.mean(np.sum((L.get()[0] - s.truth.X) ** 2, axis=1))))
            print(f"frame: counts {_counts(f)}, errors {err}, bounds {bound}, rms {rms[-1]:.4f}")
        assert total.max() == 2 and rms[2] < rms[1] < rms[0]
    print(f"device worst posterior errors in units of float64 numpy's own (bound 8): {_worst_post}")


def test_every_edge_rotation_is_evaluated():
    assert {s.name.split()[1] for s in lr.scenes((65,))} == set(pose_edges.NAMES) and len(pose_edges.NAMES) == 9
    assert lf.GATE == lr.GATE == 9.21
