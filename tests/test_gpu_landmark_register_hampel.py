"""GPU: the joint registration under Hampel's redescending loss (api.Landmarks.eval_register_hampel / register_hampel) against
the long-double reference of tests/landmark_register_hampel_reference.py, on the cases
tests/test_landmark_register_hampel_host_cpu.py qualifies (float64 numpy counts every observation alike there, every row of the
loss holds a used observation at n >= 63, and no chi2 lies within 1e-9 relative of a^2, b^2 or c^2): the vector-per-lane, wave and
block edges, several grid-stride steps with a partial last wave (SBA_RESECT_GRID=1), dense and indexed, with and without the
bearing's noise, thresholds (2, 4, 8).  The four counts are exact; H, g and the cost, and X+, Sigma+, chi2 and the pose covariance,
are held to 8 times float64 numpy's own error on the same cases, measured in this run.  The Huber limit b =
c = inf against eval_register_robust; the staged solve: its Huber stage byte for byte register_robust's, its minimiser against the
staged reference's, the posterior at the device's pose, every 0.2-rad wrong match gated and untouched; bytes across dry and wet
runs, forms, handles, histories, grids and host / device bearings; refusals, the too-few-weights one included; the demonstration
against register_robust.  Every wait inside the library is its bounded stream wait."""
from functools import lru_cache

import numpy as np
import pytest

import landmark_register_hampel_reference as hp
import landmark_register_reference as lr
import landmark_register_robust_reference as rb
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

pytestmark = pytest.mark.gpu

TIGHT = dict(function_tolerance=1e-30, parameter_tolerance=1e-13, gradient_tolerance=1e-13, max_num_iterations=100)
GRIDS = (None, "1", "2", "3")
A, B, C = hp.A, hp.B, hp.C
ABC = dict(huber_delta=A, b=B, c=C)
INF = hp.INF
_worst_eval = np.zeros(3)


def _tight():
    return api.default_lm_options(**TIGHT)


def _at_pose():
    return api.default_lm_options(max_num_iterations=0)


@lru_cache(maxsize=None)
def _eval_bounds():
    """8 times float64 numpy's worst errors against long double on the same evaluations, measured in this run."""
    return 8.0 * np.array(hp.measured_eval_errors())


def _state(L):
    X, Cv = L.get()
    return X.tobytes() + Cv.tobytes() + L.counts().tobytes()


def _counts(f):
    return (f.n_obs, f.n_skipped, f.n_behind, f.n_gated, f.n_fused)


def _result_bytes(f, chi2=None):
    chi2 = f.chi2 if chi2 is None else chi2
    return (b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in (f.rot, f.tran, f.cov, chi2, f.rot_huber, f.tran_huber))
            + repr(_counts(f) + (f.n_used, f.n_outlier, f.n_rejected, f.huber_iterations, f.summary.num_iterations)).encode())


def _eq_counts(e):
    return (e.n_used, e.n_behind, e.n_outlier, e.n_rejected)


def _eq_bytes(e):
    return e.H.tobytes() + e.g.tobytes() + repr((e.cost,) + _eq_counts(e)).encode()


# ---- 1. evaluation parity --------------------------------------------------------------------------------------------------------
def _run_eval_size(n):
    global _worst_eval
    identical = []
    with api.Landmarks(0) as L:
        for s in hp.scenes((n,)):
            L.set(s.X, s.cov)
            before = _state(L)
            pose = s.name.split()[1]
            for bs in hp.BEARING_SIGMAS:
                for form, idx in lr.forms(s):
                    _, cls, ref, _, _ = hp.eval_reference(n, pose, bs, idx is not None)
                    y = s.y if idx is None else s.y[idx]
                    got = L.eval_register_hampel(y, s.rot, s.tran, A, B, C, s.rot_ref, s.tran_ref, bs, idx=idx)
                    what = f"{s.name} bs={bs} {form}"
                    assert _eq_counts(got) == _eq_counts(ref), what
                    assert got.n_used == int((cls == lr.LIVE).sum()), what
                    assert np.array_equal(got.H, got.H.T), what
                    if ref.n_used:
                        err = np.array(lr.eq_errors(got, ref))
                        print(f"{what}: errors {err}, outliers {got.n_outlier}, rejected {got.n_rejected} of {got.n_used}")
                        assert (err <= _eval_bounds()).all(), f"{what}: errors {err}, bounds {_eval_bounds()}"
                        _worst_eval = np.maximum(_worst_eval, err)
                    else:
                        assert not got.H.any() and not got.g.any() and got.cost == 0.0, what
            # the Huber limit b = c = inf: eval_register_robust's sums, and the reference's
            _, _, ref, _, _ = hp.eval_reference(n, pose, 1e-3, False, (A, INF, INF))
            lim = L.eval_register_hampel(s.y, s.rot, s.tran, A, INF, INF, s.rot_ref, s.tran_ref, 1e-3)
            hub = L.eval_register_robust(s.y, s.rot, s.tran, A, s.rot_ref, s.tran_ref, 1e-3)
            assert _eq_counts(lim) == (hub.n_used, hub.n_behind, hub.n_outlier, 0) == _eq_counts(ref), s.name
            assert np.isfinite(lim.H).all() and np.isfinite(lim.g).all() and np.isfinite(lim.cost)
            if ref.n_used:
                for got, want in ((lim, ref), (hub, ref), (lim, hub)):
                    err = np.array(lr.eq_errors(got, want))
                    assert (err <= _eval_bounds()).all(), f"{s.name} Huber limit: errors {err}, bounds {_eval_bounds()}"
            identical.append(lim.H.tobytes() == hub.H.tobytes() and lim.g.tobytes() == hub.g.tobytes() and lim.cost == hub.cost)
            assert _state(L) == before, s.name                                  # an evaluation writes nothing
    print(f"n = {n}: device worst so far H {_worst_eval[0]:.3e}, g {_worst_eval[1]:.3e}, cost {_worst_eval[2]:.3e}; bounds {_eval_bounds()}; "
          f"Huber limit byte-identical to eval_register_robust: {identical}")


@pytest.mark.parametrize("n", hp.SIZES)
def test_evaluation_against_long_double(n):
    _run_eval_size(n)


@pytest.mark.parametrize("n", hp.LONG)
def test_evaluation_over_several_grid_stride_steps(monkeypatch, n):
    monkeypatch.setenv("SBA_RESECT_GRID", "1")
    _run_eval_size(n)


# ---- 2. the solve and the posterior ----------------------------------------------------------------------------------------------
def _check_posterior(L, X0, C0, cnt0, y, idx, rot0, tran0, bs, f):
    """The handle's state after `f` against a reference step from the state before it, AT THE DEVICE'S POSE, with bounds of 8 times
    float64 numpy's own errors on this very case; classes and counts exact (qualify_posterior asserts that no chi2 lies within 1e-9
    of the gate or a threshold); every downweighted observation's landmark untouched, byte for byte."""
    n = len(X0)
    rows = np.arange(n) if idx is None else idx
    ref, errs = hp.qualify_posterior(X0[rows], C0[rows], y, rot0, tran0, f.rot, f.tran, bs)
    assert _counts(f) == ref.counts(), (_counts(f), ref.counts())
    assert (f.n_used, f.n_outlier, f.n_rejected) == (ref.eq.n_used, ref.eq.n_outlier, ref.eq.n_rejected)
    X1, C1 = L.get()
    touched = np.zeros(n, dtype=bool)
    touched[rows[ref.cls == hp.FUSED]] = True
    assert np.array_equal(L.counts(), cnt0 + touched.astype(np.uint32))
    assert X1[~touched].tobytes() == X0[~touched].tobytes() and C1[~touched].tobytes() == C0[~touched].tobytes()
    with np.errstate(invalid="ignore"):
        outlier = rows[np.asarray(ref.chi2 > A * A) & (ref.cls != hp.BEHIND)]
    assert len(outlier) == f.n_outlier and not touched[outlier].any()           # all of them gated, none rewritten
    assert np.array_equal(np.isnan(f.chi2), ref.cls == hp.SKIPPED)
    assert np.array_equal(f.cov, f.cov.T)
    err = np.array(lr.post_errors(X1[rows], C1[rows], f.chi2, f.cov, ref, X0[rows], C0[rows]))
    bound = 8.0 * np.array(errs)
    assert (err <= bound).all(), f"errors {err} (X+, Sigma+, chi2, Sigma_c), bounds {bound}"
    return ref, err, bound


def _run_solve(n, indexed):
    s = hp.solve_scene(n)
    idx = lr.subset(n) if indexed else None
    rows = np.arange(n) if idx is None else idx
    if indexed:
        noise, _ = lr.freeze(s.X[rows], s.cov[rows], s.y[rows], s.rot0, s.tran0, s.bearing_sigma)
        rot_r, tran_r, eq_r, _, _ = hp.solve(s.X[rows], s.cov[rows], s.y[rows], noise, s.rot0, s.tran0)
    else:
        _, _, rot_r, tran_r, eq_r, _, _ = hp.solve_reference(n)
    with api.Landmarks(0) as L:
        L.set(s.X, s.cov)
        X0, C0 = L.get()
        before = _state(L)
        hub = L.register_robust(s.y[rows], s.rot0, s.tran0, A, s.bearing_sigma, idx=idx, apply=False, options=_tight())
        assert _state(L) == before
        f = L.register_hampel(s.y[rows], s.rot0, s.tran0, A, B, C, bearing_sigma=s.bearing_sigma, idx=idx, options=_tight(), return_chi2=True)
        # the Huber stage is register_robust's solve: the same kernel, noise and options
        assert f.rot_huber.tobytes() == hub.rot.tobytes() and f.tran_huber.tobytes() == hub.tran.tobytes()
        assert f.huber_iterations == hub.summary.num_iterations > 0
        dp = np.concatenate([f.rot - rot_r, f.tran - tran_r])
        maha2 = float(dp @ eq_r.H @ dp)
        print(f"n = {n} {'indexed' if indexed else 'dense'}: Huber stage {f.huber_iterations} iterations, Hampel {f.summary.termination} after "
              f"{f.summary.num_iterations}, (p - p*)^T H (p - p*) = {maha2:.3e}, {f.n_outlier} outliers, {f.n_rejected} rejected")
        assert maha2 <= 1e-6
        ref, err, bound = _check_posterior(L, X0, C0, np.zeros(len(X0), dtype=np.uint32), s.y[rows], idx, s.rot0, s.tran0, s.bearing_sigma, f)
        print(f"    posterior errors {err} (X+, Sigma+, chi2, Sigma_c), bounds {bound}, counts {_counts(f)}")
        planted = np.isin(rows, hp.planted(n, 10))
        assert (ref.cls[planted] == hp.GATED).all() and f.n_fused >= len(rows) // 2
        assert f.n_rejected >= 1 or not planted.any()                           # subset(65) holds none of the planted rows
        X1, C1 = L.get()
        wrong = rows[planted]                                                   # every 0.2-rad wrong match: gated, its landmark untouched
        assert X1[wrong].tobytes() == X0[wrong].tobytes() and C1[wrong].tobytes() == C0[wrong].tobytes() and not L.counts()[wrong].any()
        # without the Huber stage the three fields are the start pose and 0, and the minimum is the same one
        L.set(s.X, s.cov)
        d = L.register_hampel(s.y[rows], s.rot0, s.tran0, A, B, C, huber_first=False, bearing_sigma=s.bearing_sigma, idx=idx, options=_tight())
        assert np.array_equal(d.rot_huber, s.rot0) and np.array_equal(d.tran_huber, s.tran0) and d.huber_iterations == 0
        dp = np.concatenate([d.rot - rot_r, d.tran - tran_r])
        assert float(dp @ eq_r.H @ dp) <= 1e-6
        assert (_counts(d), d.n_used, d.n_outlier, d.n_rejected) == (_counts(f), f.n_used, f.n_outlier, f.n_rejected)


@pytest.mark.parametrize("n", hp.SOLVE_SIZES)
def test_solve_and_posterior_against_long_double(n):
    _run_solve(n, False)
    _run_solve(n, True)


@pytest.mark.parametrize("n", hp.SOLVE_LONG)
def test_solve_and_posterior_on_one_block(monkeypatch, n):
    monkeypatch.setenv("SBA_RESECT_GRID", "1")
    _run_solve(n, False)


# ---- 3. the demonstration --------------------------------------------------------------------------------------------------------
def test_the_hampel_pose_is_not_further_from_the_truth_than_the_huber_one():
    """n = 513 with 51 wrong matches: squared distances from the truth in the metric of the Hampel reference's H."""
    n = hp.DEMO_N
    s = hp.solve_scene(n)
    assert len(hp.planted(n, 10)) == 51
    _, _, _, _, eq_r, _, _ = hp.solve_reference(n)
    with api.Landmarks(0) as L:
        L.set(s.X, s.cov)
        ham = L.register_hampel(s.y, s.rot0, s.tran0, A, B, C, bearing_sigma=s.bearing_sigma, apply=False, options=_tight())
        hub = L.register_robust(s.y, s.rot0, s.tran0, A, s.bearing_sigma, apply=False, options=_tight())
    d_hm, d_hb = hp.pose_distance2(ham.rot, ham.tran, s, eq_r.H), hp.pose_distance2(hub.rot, hub.tran, s, eq_r.H)
    own = lambda f: hp.pose_distance2(f.rot, f.tran, s, np.linalg.inv(f.cov))
    print(f"squared distance from the truth in the Hampel H: register_hampel {d_hm:.3f}, register_robust {d_hb:.3f}; each in its own "
          f"returned covariance: {own(ham):.3f}, {own(hub):.3f}")
    assert d_hm <= d_hb


# ---- 4. bytes --------------------------------------------------------------------------------------------------------------------
def test_dry_run_indexed_form_fresh_handles_and_histories_return_the_same_bytes():
    n = 513
    s = hp.solve_scene(n)
    other = lr.solve_scene(65)
    kw = dict(bearing_sigma=s.bearing_sigma, options=_tight(), return_chi2=True, **ABC)
    with api.Landmarks(0) as Ha, api.Landmarks(0) as Hb, api.Landmarks(0) as Hd:
        for H in (Ha, Hb, Hd):
            H.set(s.X, s.cov)
        before = _state(Ha)
        dry = Ha.register_hampel(s.y, s.rot0, s.tran0, apply=False, **kw)
        assert _state(Ha) == before                                             # the dry run leaves get() and counts() as they were
        wet = Hb.register_hampel(s.y, s.rot0, s.tran0, **kw)                    # a twin handle, a fresh one
        assert _result_bytes(dry) == _result_bytes(wet) and _state(Hb) != before
        after = _state(Hb)
        ind = Hd.register_hampel(s.y, s.rot0, s.tran0, idx=np.arange(n, dtype=np.int64), **kw)
        assert _result_bytes(ind) == _result_bytes(wet) and _state(Hd) == after  # indexed over arange(n) equals dense
        again = Ha.register_hampel(s.y, s.rot0, s.tran0, **kw)                  # after a dry run on the same handle: run to run
        assert _result_bytes(again) == _result_bytes(wet) and _state(Ha) == after
        # other passes on the handle in between: another map, register_robust, fuse, prune
        Hb.set(other.X, other.cov)
        Hb.register_robust(other.y, other.rot0, other.tran0, A, other.bearing_sigma)
        Hb.fuse(other.y, other.truth.rot, other.truth.tran, 1e-3)
        Hb.prune(max_score=1e-3)
        Hb.set(s.X, s.cov)
        assert _result_bytes(Hb.register_hampel(s.y, s.rot0, s.tran0, **kw)) == _result_bytes(wet) and _state(Hb) == after
        # evaluations: run to run, arange(n) against dense
        Ha.set(s.X, s.cov)
        e1 = Ha.eval_register_hampel(s.y, s.rot0, s.tran0, bearing_sigma=1e-3, **ABC)
        e2 = Ha.eval_register_hampel(s.y, s.rot0, s.tran0, bearing_sigma=1e-3, **ABC)
        e3 = Ha.eval_register_hampel(s.y, s.rot0, s.tran0, bearing_sigma=1e-3, idx=np.arange(n, dtype=np.int64), **ABC)
        assert _eq_bytes(e1) == _eq_bytes(e2) == _eq_bytes(e3)
        # the defaults are b = 2 a, c = 4 a, the Huber stage first and the gate a^2
        Ha.set(s.X, s.cov)
        dflt = Ha.register_hampel(s.y, s.rot0, s.tran0, A, bearing_sigma=s.bearing_sigma, options=_tight(), return_chi2=True)
        assert _result_bytes(dflt) == _result_bytes(wet) and _state(Ha) == after


@pytest.mark.parametrize("n", (512, 513))
def test_device_bearings_return_the_host_bearings_bytes(n):
    """bearings_device, a torch tensor's address, with chi2 on the device: the dense form over an even n reads the caller's rows in
    place, over an odd n or from a pointer that is not 16-byte aligned it copies them device to device first, the indexed form
    always reads in place -- all byte for byte what host bearings give."""
    import torch
    s = hp.solve_scene(513)
    X, cov, y = s.X[:n], s.cov[:n], np.ascontiguousarray(s.y[:n])
    idx = lr.subset(n)
    kw = dict(bearing_sigma=s.bearing_sigma, options=_tight(), **ABC)
    dev = torch.device("cuda:0")
    with api.Landmarks(0) as Ha, api.Landmarks(0) as Hb:
        for form, ii in (("dense", None), ("indexed", idx)):
            rows = np.array(y if ii is None else y[ii])                         # a writable copy: torch.from_numpy wants one
            m = len(rows)
            buf = torch.empty(3 * m + 1, dtype=torch.float64, device=dev)
            aligned, shifted = buf[:3 * m], buf[1:]                             # the second one starts 8 bytes off a 16-byte boundary
            for name, t in (("aligned", aligned), ("shifted", shifted)):
                t.copy_(torch.from_numpy(rows.reshape(-1)))
                for off in (2, 1):                                              # chi2 between guard cells, 16 and 8 bytes in
                    chi2_dev = torch.full((m + 4,), -7.0, dtype=torch.float64, device=dev)
                    assert chi2_dev.data_ptr() % 16 == 0
                    torch.cuda.synchronize()
                    Ha.set(X, cov)
                    Hb.set(X, cov)
                    host = Ha.register_hampel(rows, s.rot0, s.tran0, idx=ii, return_chi2=True, **kw)
                    got = Hb.register_hampel(None, s.rot0, s.tran0, idx=ii, bearings_device=t.data_ptr(), chi2_device=chi2_dev.data_ptr() + 8 * off, **kw)
                    torch.cuda.synchronize()
                    all_chi2 = chi2_dev.cpu().numpy()
                    chi2 = np.ascontiguousarray(all_chi2[off:off + m])
                    assert (all_chi2[:off] == -7.0).all() and (all_chi2[off + m:] == -7.0).all(), (form, name, off, all_chi2[:off], all_chi2[off + m:])
                    assert _result_bytes(got, chi2) == _result_bytes(host), (form, name, off)
                    assert _state(Ha) == _state(Hb), (form, name, off)
                assert torch.equal(t.cpu(), torch.from_numpy(rows.reshape(-1))), (form, name)      # the caller's rows are only read
                eh = Ha.eval_register_hampel(rows, s.rot0, s.tran0, bearing_sigma=1e-3, idx=ii, **ABC)
                ed = Hb.eval_register_hampel(None, s.rot0, s.tran0, bearing_sigma=1e-3, idx=ii, bearings_device=t.data_ptr(), **ABC)
                assert _eq_bytes(eh) == _eq_bytes(ed), (form, name)


def test_results_across_grids(monkeypatch):
    """At a given pose (max_num_iterations = 0) everything that does not pass through the reduction -- X+, chi2, the classes, the
    counts -- is byte-identical for SBA_RESECT_GRID 1, 2, 3 and unset.  Sigma_c = H^-1 carries the reduction's bits into Sigma+: those
    two, and the whole solved result, agree within the posterior's bounds, and are byte-identical again at a fixed grid."""
    n = 1537
    s = hp.solve_scene(n)
    zeros = np.zeros(n, dtype=np.uint32)
    seen, solved = [], []
    with api.Landmarks(0) as L:
        for grid in GRIDS:
            if grid is None:
                monkeypatch.delenv("SBA_RESECT_GRID", raising=False)
            else:
                monkeypatch.setenv("SBA_RESECT_GRID", grid)
            L.set(s.X, s.cov)
            X0, C0 = L.get()
            f = L.register_hampel(s.y, s.truth.rot, s.truth.tran, bearing_sigma=s.bearing_sigma, options=_at_pose(), return_chi2=True, **ABC)
            assert f.summary.num_evaluations == 1
            _check_posterior(L, X0, C0, zeros, s.y, None, s.truth.rot, s.truth.tran, s.bearing_sigma, f)
            X1, C1 = L.get()
            seen.append(X1.tobytes() + f.chi2.tobytes() + L.counts().tobytes() + repr(_counts(f) + (f.n_used, f.n_outlier, f.n_rejected)).encode())
            L.set(s.X, s.cov)
            g = L.register_hampel(s.y, s.truth.rot, s.truth.tran, bearing_sigma=s.bearing_sigma, options=_at_pose(), return_chi2=True, **ABC)
            assert _result_bytes(g) == _result_bytes(f) and L.get()[1].tobytes() == C1.tobytes()      # a fixed grid: the same bits
            L.set(s.X, s.cov)
            h = L.register_hampel(s.y, s.rot0, s.tran0, bearing_sigma=s.bearing_sigma, options=_tight(), return_chi2=True, **ABC)
            _check_posterior(L, X0, C0, zeros, s.y, None, s.rot0, s.tran0, s.bearing_sigma, h)
            solved.append(h)
    assert all(v == seen[0] for v in seen)
    _, _, rot_r, tran_r, eq_r, _, _ = hp.solve_reference(n)
    for h in solved:
        dp = np.concatenate([h.rot - rot_r, h.tran - tran_r])
        assert float(dp @ eq_r.H @ dp) <= 1e-6
        assert (_counts(h), h.n_outlier, h.n_rejected) == (_counts(solved[0]), solved[0].n_outlier, solved[0].n_rejected)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_map_as_it_was():
    import torch
    s = hp.solve_scene(65)
    n = 65
    with api.Landmarks(0) as L:
        L.set(s.X, s.cov)
        L.register_hampel(s.y, s.rot0, s.tran0, bearing_sigma=s.bearing_sigma, options=_tight(), **ABC)      # counts are no longer zero
        before = _state(L)
        ok = dict(bearings=s.y, rot=s.rot0, tran=s.tran0, bearing_sigma=1e-3, **ABC)
        nan3 = np.array([0.0, np.nan, 0.0])
        inv, num = cabi.SBA_ERR_INVALID_ARG, cabi.SBA_ERR_NUMERIC
        cases = [
            # everything register_robust refuses, with its codes
            (dict(ok, bearing_sigma=-1e-3), inv),
            (dict(ok, bearing_sigma=np.inf), inv),
            (dict(ok, chi2_gate=0.0), inv),
            (dict(ok, chi2_gate=np.nan), inv),
            (dict(ok, chi2_gate=np.inf), inv),                                                          # above a^2
            (dict(ok, chi2_gate=1.01 * A * A), inv),
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
            # the thresholds
            (dict(ok, b=np.nan), inv),
            (dict(ok, c=np.nan), inv),
            (dict(ok, b=A), inv),
            (dict(ok, b=0.5 * A), inv),
            (dict(ok, c=B), inv),
            (dict(ok, c=0.5 * B), inv),
            (dict(ok, c=np.inf), inv),                                                                  # exactly one infinite
            (dict(ok, b=np.inf), inv),
            (dict(ok, b=-np.inf, c=-np.inf), inv),
        ]
        for kw, code in cases:
            for first in (True, False):
                with pytest.raises(api.SbaError) as ei:
                    L.register_hampel(huber_first=first, **kw)
                assert ei.value.code == code and ei.value.message, kw
                assert _state(L) == before, kw
        for kw, code in ((dict(bearing_sigma=-1.0), inv), (dict(rot_ref=nan3), num), (dict(idx=np.arange(n)[::-1]), inv),
                         (dict(huber_delta=0.0), inv), (dict(huber_delta=np.nan), inv), (dict(b=np.nan), inv), (dict(b=A), inv),
                         (dict(c=B), inv), (dict(c=np.inf), inv), (dict(b=np.inf), inv)):
            args = dict(ABC, **kw)
            with pytest.raises(api.SbaError) as ei:
                L.eval_register_hampel(s.y, s.rot0, s.tran0, **args)
            assert ei.value.code == code, kw
            assert _state(L) == before, kw
        # the device twins: the same refusals, and a device pointer that is not 8-byte aligned
        y_dev = torch.from_numpy(np.array(s.y).reshape(-1)).to("cuda:0")
        torch.cuda.synchronize()
        dev = dict(bearings=None, rot=s.rot0, tran=s.tran0, bearing_sigma=1e-3, bearings_device=y_dev.data_ptr(), **ABC)
        for kw, code in ((dict(dev, chi2_gate=np.inf), inv), (dict(dev, chi2_gate=1.01 * A * A), inv), (dict(dev, huber_delta=-2.0, chi2_gate=1.0), inv),
                         (dict(dev, m=n - 1), inv), (dict(dev, bearings_device=y_dev.data_ptr() + 4), inv), (dict(dev, rot=nan3), num),
                         (dict(dev, b=A), inv), (dict(dev, c=np.inf), inv), (dict(dev, c=np.nan), inv)):
            with pytest.raises(api.SbaError) as ei:
                L.register_hampel(**kw)
            assert ei.value.code == code and ei.value.message, kw
            assert _state(L) == before, kw
        # after the freeze: fewer than 3 observations take part
        few = np.zeros_like(s.y)
        few[[5, 40]] = s.y[[5, 40]]
        with pytest.raises(api.SbaError) as ei:
            L.register_hampel(few, s.rot0, s.tran0, bearing_sigma=1e-3, options=_tight(), **ABC)
        assert ei.value.code == num and "pose not determined" in ei.value.message and _state(L) == before
        assert L.eval_register_hampel(few, s.rot0, s.tran0, **ABC).n_used == 2    # an evaluation is not refused
        # after the solve: fewer than 3 observations keep a weight.  Five observations take part, three of them turned by 0.4 rad:
        # at the true pose (max_num_iterations = 0) those three lie beyond c -- the reference says so -- and two are left.
        lone = np.zeros_like(s.y)
        lone[[6, 20, 40, 50, 60]] = s.y[[6, 20, 40, 50, 60]]
        lone = hp.displace(lone, (20, 50, 60), 4711, 0.4)
        noise, cls = lr.freeze(s.X, s.cov, lone, s.truth.rot, s.truth.tran, 1e-3)
        ref = hp.evaluate(s.X, s.cov, lone, noise, s.truth.rot, s.truth.tran)
        assert int((cls == lr.LIVE).sum()) == 5 and (ref.n_used, ref.n_rejected) == (5, 3)
        for first in (False, True):
            with pytest.raises(api.SbaError) as ei:
                L.register_hampel(lone, s.truth.rot, s.truth.tran, huber_first=first, bearing_sigma=1e-3, options=_at_pose(), **ABC)
            assert ei.value.code == num and "carry no weight" in ei.value.message and _state(L) == before, first
        e = L.eval_register_hampel(lone, s.truth.rot, s.truth.tran, bearing_sigma=1e-3, **ABC)
        assert _eq_counts(e) == _eq_counts(ref)                                 # an evaluation is not refused
        # the handle stays usable
        assert L.register_hampel(s.y, s.rot0, s.tran0, bearing_sigma=s.bearing_sigma, options=_tight(), **ABC).n_fused > 0
    # after the solve: three landmarks on one line through the frame's centre leave the rotation about it free
    Xl = np.array([[2.0, 0, 0], [3.0, 0, 0], [5.0, 0, 0]])
    Cl = np.tile([1e-2, 1e-4, 1e-4, 0, 0, 0], (3, 1))
    yl = np.tile([1.0, 0, 0], (3, 1))
    with api.Landmarks(0) as L:
        L.set(Xl, Cl)
        before = _state(L)
        with pytest.raises(api.SbaError) as ei:
            L.register_hampel(yl, np.zeros(3), np.zeros(3), bearing_sigma=1e-3, options=_at_pose(), **ABC)
        assert ei.value.code == num and "positive definite" in ei.value.message and _state(L) == before


def test_empty_map_and_no_observations():
    s = hp.solve_scene(65)
    with api.Landmarks(0) as L:
        f = L.register_hampel(np.zeros((0, 3)), s.rot0, s.tran0, A, return_chi2=True)
        assert _counts(f) == (0, 0, 0, 0, 0) and (f.n_used, f.n_outlier, f.n_rejected, f.huber_iterations) == (0, 0, 0, 0)
        assert np.array_equal(f.rot, s.rot0) and np.array_equal(f.rot_huber, s.rot0) and np.array_equal(f.tran_huber, s.tran0)
        assert f.chi2.shape == (0,) and not f.cov.any()
        L.set(s.X, s.cov)
        before = _state(L)
        e = L.eval_register_hampel(np.zeros((0, 3)), s.rot0, s.tran0, A, idx=np.zeros(0, dtype=np.int64))
        assert _eq_counts(e) == (0, 0, 0, 0) and not e.H.any() and e.cost == 0.0 and _state(L) == before
