"""GPU: the landmark map (api.Landmarks: set / set_device / get / get_device / counts / fuse) against the long-double reference of
tests/landmark_fusion_reference.py, on the cases tests/test_landmark_fusion_host_cpu.py qualifies (float64 numpy classifies every
observation alike there, and no chi^2 sits on the gate): the vector-per-lane, wave and block edges, several grid-stride steps with
a partial last wave (SBA_RESECT_GRID=1), dense and indexed, with and without the bearing's noise and the pose covariance, a
covariance scale, the nine rotations where the kernels' frame changes.  The five counts are exact; X+, Sigma+ and chi^2 are held to
8 times float64 numpy's own worst error on the same cases, measured in this run.  Planted rows of every class
and every skipped kind; the dry run; indexed against dense; bytes across handles, grids and histories; three frames in sequence;
refusals; the chain from a solved pair's structure through the weighted resection back into the map, on the device."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import landmark_fusion_reference as lf
import pose_edges
import resection_reference as rr
import resection_weighted_reference as wr
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

pytestmark = pytest.mark.gpu

TIGHT = dict(function_tolerance=1e-30, parameter_tolerance=1e-13, gradient_tolerance=1e-13, max_num_iterations=100)
GRIDS = (None, "1", "2", "3", "5")
_worst = np.zeros(3)                 # the device's worst errors over the accuracy tests of this run


@lru_cache(maxsize=None)
def _bounds():
    """8 times float64 numpy's worst errors against long double on the same cases, measured in this run: a different order of
    operations and fused multiply-adds are what the factor covers, as in section 3.19."""
    return 8.0 * np.array(lf.measured_errors())


def _state(L):
    X, Cv = L.get()
    return X.tobytes() + Cv.tobytes() + L.counts().tobytes()


def _counts(f):
    return (f.n_obs, f.n_skipped, f.n_behind, f.n_gated, f.n_fused)


def _check_case(L, s, bs, pc, idx):
    """One case on the handle against its reference; -> the three errors."""
    global _worst
    n = len(s.X)
    ref = lf.reference(n, s.name.split()[1], bs, pc is not None)
    L.set(s.X, s.cov, lf.COV_SCALE)
    assert L.size == n
    X0, C0 = L.get()
    assert X0.tobytes() == s.X.tobytes() and C0.tobytes() == s.prior_cov.tobytes(), s.name       # the pack kernel's product is numpy's
    assert not L.counts().any()
    rows = np.arange(n) if idx is None else idx
    f = L.fuse(s.y if idx is None else s.y[idx], s.rot, s.tran, bs, lf.GATE, pc, idx=idx)
    cls = ref.cls[rows]
    want = (len(rows),) + tuple(int((cls == k).sum()) for k in (lf.SKIPPED, lf.BEHIND, lf.GATED, lf.FUSED))
    assert _counts(f) == want, (s.name, bs, pc is not None, idx is not None, _counts(f), want)
    X1, C1 = L.get()
    cnt = L.counts()
    touched = np.zeros(n, dtype=bool)
    touched[rows[cls == lf.FUSED]] = True
    assert np.array_equal(cnt, touched.astype(np.uint32)), s.name
    assert X1[~touched].tobytes() == X0[~touched].tobytes() and C1[~touched].tobytes() == C0[~touched].tobytes(), s.name
    assert f.chi2.shape == (len(rows),) and np.isfinite(f.chi2).all()
    sub = lf.Fused(ref.X[rows], ref.cov[rows], ref.chi2[rows], cls, ref.dstar[rows])
    err = np.array(lf.errors(X1[rows], C1[rows], f.chi2, sub, X0[rows], C0[rows]))
    assert (err <= _bounds()).all(), f"{s.name} bs={bs} pose_cov={pc is not None} indexed={idx is not None}: errors {err}, bounds {_bounds()}"
    _worst = np.maximum(_worst, err)
    return err


def _run_size(n):
    with api.Landmarks(0) as L:
        for s in lf.scenes((n,)):
            for bs, pc in lf.variants():
                _check_case(L, s, bs, pc, None)
                _check_case(L, s, bs, pc, lf.subset(n))
    print(f"n = {n}: device worst so far X+ {_worst[0]:.3e}, Sigma+ {_worst[1]:.3e}, chi2 {_worst[2]:.3e}; bounds {_bounds()}")


@pytest.mark.parametrize("n", lf.SIZES)
def test_fuse_against_long_double(n):
    _run_size(n)


@pytest.mark.parametrize("n", lf.LONG)
def test_fuse_over_several_grid_stride_steps(monkeypatch, n):
    monkeypatch.setenv("SBA_RESECT_GRID", "1")
    _run_size(n)


def test_empty_map_and_no_observations():
    s = lf.scene(65, "series")
    with api.Landmarks(0) as L:
        assert L.size == 0 and L.get()[0].shape == (0, 3) and L.counts().shape == (0,)
        assert _counts(L.fuse(np.zeros((0, 3)), s.rot, s.tran)) == (0, 0, 0, 0, 0)
        L.set(s.X, s.cov, lf.COV_SCALE)
        before = _state(L)
        f = L.fuse(np.zeros((0, 3)), s.rot, s.tran, idx=np.zeros(0, dtype=np.int64))
        assert _counts(f) == (0, 0, 0, 0, 0) and f.chi2.shape == (0,) and _state(L) == before
        L.set(np.zeros((0, 3)), np.zeros((0, 6)))
        assert L.size == 0


def _displaced(y, angle):
    """y turned by `angle` about an axis across it."""
    k = np.cross(y, [0.3, -0.5, 0.8])
    k = k / np.linalg.norm(k)
    return y * np.cos(angle) + np.cross(k, y) * np.sin(angle)


@pytest.mark.parametrize("n,grid", [(513, None), (1537, "1")])
def test_planted_rows_of_every_class(monkeypatch, n, grid):
    """Rows spread over waves, blocks and steps: untouched byte for byte, counted in their class, chi2 NaN exactly where skipped."""
    if grid:
        monkeypatch.setenv("SBA_RESECT_GRID", grid)
    s = lf.scene(n, "series")
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
    with api.Landmarks(0) as L, api.Landmarks(0) as Li:
        for H in (L, Li):
            H.set(X, cov, lf.COV_SCALE)
        X0, C0 = L.get()
        ref = lf.fuse(X0, C0, y, s.rot, s.tran, 0.0, lf.GATE)
        assert all(ref.cls[i] == lf.SKIPPED for i in skipped.values()) and ref.cls[behind] == lf.BEHIND
        assert all(ref.cls[i] == lf.GATED for i in gated)
        live = ref.cls != lf.SKIPPED
        assert (np.abs(ref.chi2[live] - lf.GATE) > lf.MARGIN * lf.GATE).all() and (np.abs(ref.dstar[live]) > lf.MARGIN).all()
        idx = np.array(sorted(set(planted) | set(lf.subset(n).tolist())), dtype=np.int64)
        for H, rows in ((L, np.arange(n)), (Li, idx)):
            f = H.fuse(y[rows], s.rot, s.tran, 0.0, lf.GATE, idx=None if H is L else rows)
            cls = ref.cls[rows]
            assert _counts(f) == (len(rows),) + tuple(int((cls == k).sum()) for k in range(4))
            assert f.n_skipped >= 5 and f.n_behind >= 1 and f.n_gated >= 8
            assert np.array_equal(np.isnan(f.chi2), cls == lf.SKIPPED)
            X1, C1 = H.get()
            keep = np.ones(n, dtype=bool)
            keep[rows[cls == lf.FUSED]] = False
            assert keep[planted].all()
            assert X1[keep].tobytes() == X0[keep].tobytes() and C1[keep].tobytes() == C0[keep].tobytes()
            assert np.array_equal(H.counts(), (~keep).astype(np.uint32))
            sub = lf.Fused(ref.X[rows], ref.cov[rows], ref.chi2[rows], cls, ref.dstar[rows])
            with np.errstate(invalid="ignore"):
                err = np.array(lf.errors(X1[rows], C1[rows], f.chi2, sub, X0[rows], C0[rows]))
            assert (err <= _bounds()).all(), (err, _bounds())


@pytest.mark.parametrize("indexed", [False, True], ids=["dense", "indexed"])
def test_a_dry_run_reports_the_same_and_stores_nothing(indexed):
    s = lf.scene(513, "closed")
    idx = lf.subset(513) if indexed else None
    y = s.y[idx] if indexed else s.y
    with api.Landmarks(0) as L, api.Landmarks(0) as T:
        for H in (L, T):
            H.set(s.X, s.cov, lf.COV_SCALE)
        before = _state(L)
        dry = L.fuse(y, s.rot, s.tran, 1e-3, lf.GATE, lf.POSE_COV_FULL, idx=idx, apply=False)
        assert _state(L) == before
        wet = T.fuse(y, s.rot, s.tran, 1e-3, lf.GATE, lf.POSE_COV_FULL, idx=idx)
        assert _counts(dry) == _counts(wet) and dry.chi2.tobytes() == wet.chi2.tobytes() and wet.n_fused > 200 and wet.n_gated > 0
        assert _state(T) != before
        assert L.fuse(y, s.rot, s.tran, 1e-3, lf.GATE, lf.POSE_COV_FULL, idx=idx, want_chi2=False).chi2 is None
        assert _state(L) == _state(T)


def test_indexed_over_every_landmark_equals_dense():
    for n in (65, 513):
        s = lf.scene(n, "near_pi")
        with api.Landmarks(0) as L, api.Landmarks(0) as T:
            for H in (L, T):
                H.set(s.X, s.cov, lf.COV_SCALE)
            a = L.fuse(s.y, s.rot, s.tran, 1e-3, lf.GATE, lf.POSE_COV_FULL)
            b = T.fuse(s.y, s.rot, s.tran, 1e-3, lf.GATE, lf.POSE_COV_FULL, idx=np.arange(n))
            assert _counts(a) == _counts(b) and a.chi2.tobytes() == b.chi2.tobytes() and _state(L) == _state(T)


def test_indexed_over_a_subset_equals_dense_with_zero_bearings_elsewhere():
    n = 513
    s = lf.scene(n, "tiny")
    idx = lf.subset(n)
    y0 = np.zeros_like(s.y)
    y0[idx] = s.y[idx]
    with api.Landmarks(0) as L, api.Landmarks(0) as T:
        for H in (L, T):
            H.set(s.X, s.cov, lf.COV_SCALE)
        a = L.fuse(y0, s.rot, s.tran, 0.0, lf.GATE)
        b = T.fuse(s.y[idx], s.rot, s.tran, 0.0, lf.GATE, idx=idx)
        assert _state(L) == _state(T)
        assert (a.n_fused, a.n_gated, a.n_behind) == (b.n_fused, b.n_gated, b.n_behind) and a.n_skipped == b.n_skipped + n - len(idx)
        assert a.chi2[idx].tobytes() == b.chi2.tobytes() and np.isnan(np.delete(a.chi2, idx)).all()


@pytest.mark.parametrize("indexed", [False, True], ids=["dense", "indexed"])
def test_bytes_do_not_depend_on_the_handle_the_grid_or_the_history(monkeypatch, indexed):
    n = 3073                                                   # seven blocks of the dense pass: every capped grid takes several steps
    s = lf.scene(n, "series")
    idx = lf.subset(n) if indexed else None
    y = s.y[idx] if indexed else s.y

    def run(L):
        L.set(s.X, s.cov, lf.COV_SCALE)
        f = L.fuse(y, s.rot, s.tran, 1e-3, lf.GATE, lf.POSE_COV_FULL, idx=idx)
        return _state(L) + f.chi2.tobytes() + np.array(_counts(f)).tobytes()
    seen = []
    for grid in GRIDS:
        if grid is None:
            monkeypatch.delenv("SBA_RESECT_GRID", raising=False)
        else:
            monkeypatch.setenv("SBA_RESECT_GRID", grid)
        with api.Landmarks(0) as L:
            seen.append(run(L))
            if grid in (None, "2"):
                seen.append(run(L))                            # set -> fuse -> set of the same rows -> fuse: a fresh handle's bytes
    monkeypatch.delenv("SBA_RESECT_GRID", raising=False)
    with api.Landmarks(0) as L:
        other = lf.scene(513, "zero")
        L.set(other.X, other.cov, 1.0)                         # another map and another pass first
        L.fuse(other.y, other.rot, other.tran)
        seen.append(run(L))
    assert all(b == seen[0] for b in seen) and len(seen) == len(GRIDS) + 3


def test_three_frames_in_sequence_equal_the_reference_recursion():
    n = 513
    s = lf.scene(n, "closed")
    rng = np.random.default_rng(99)
    frames = []
    for k in range(3):
        yk = s.y + 1e-3 * rng.standard_normal((n, 3)) * np.linalg.norm(s.y, axis=1, keepdims=True)
        frames.append((yk, s.rot + 2e-4 * rng.standard_normal(3), s.tran + 1e-3 * rng.standard_normal(3)))
    Xr, Cr = np.asarray(s.X, lf.LD), np.asarray(s.prior_cov, lf.LD)
    total = np.zeros(n, dtype=np.uint32)
    with api.Landmarks(0) as L:
        L.set(s.X, s.cov, lf.COV_SCALE)
        for k, (yk, rot, tran) in enumerate(frames):
            X0, C0 = L.get()
            step = lf.fuse(X0, C0, yk, rot, tran, 1e-3, lf.GATE, lf.POSE_COV_FULL)        # one reference step from the handle's own state
            assert (np.abs(step.chi2 - lf.GATE) > lf.MARGIN * lf.GATE).all()
            f = L.fuse(yk, rot, tran, 1e-3, lf.GATE, lf.POSE_COV_FULL)
            assert _counts(f) == step.counts()
            X1, C1 = L.get()
            assert (np.array(lf.errors(X1, C1, f.chi2, step, X0, C0)) <= _bounds()).all(), k
            total += (step.cls == lf.FUSED).astype(np.uint32)
            assert np.array_equal(L.counts(), total)
            pure = lf.fuse(Xr, Cr, yk, rot, tran, 1e-3, lf.GATE, lf.POSE_COV_FULL)         # the recursion that never leaves long double
            same = pure.cls == step.cls
            assert same.mean() > 0.99                                                     # a chi2 may straddle the gate between the two
            Xr, Cr = pure.X, pure.cov
        # every step adds at most one bound and the update does not amplify (Sigma+ <= Sigma): three bounds after three frames,
        # on the landmarks both recursions treated alike throughout
        alike = np.ones(n, dtype=bool)
        Xa, Ca = np.asarray(s.X, lf.LD), np.asarray(s.prior_cov, lf.LD)
        Xd, Cd = s.X, s.prior_cov
        for yk, rot, tran in frames:
            a = lf.fuse(Xa, Ca, yk, rot, tran, 1e-3, lf.GATE, lf.POSE_COV_FULL)
            d = lf.fuse(Xd, Cd, yk, rot, tran, 1e-3, lf.GATE, lf.POSE_COV_FULL)
            alike &= a.cls == d.cls
            Xa, Ca, Xd, Cd = a.X, a.cov, d.X.astype(np.float64), d.cov.astype(np.float64)
        X3, C3 = L.get()
        ex = np.abs(X3 - Xr).max(axis=1) / np.linalg.norm(s.X, axis=1)
        ec = np.abs(C3 - Cr).max(axis=1) / np.abs(s.prior_cov).max(axis=1)
        assert alike.sum() > 0.98 * n
        assert ex[alike].max() <= 3 * _bounds()[0] and ec[alike].max() <= 3 * _bounds()[1], (ex[alike].max(), ec[alike].max())
        assert total.max() == 3 and (total > 0).mean() > 0.9


def _refused(code, calls):
    for name, call in calls.items():
        with pytest.raises(api.SbaError) as ei:
            call()
        assert ei.value.code == code and ei.value.message, name


def test_refusals_return_their_code_and_leave_the_map_alone():
    import torch
    n = 65
    s = lf.scene(n, "series")
    idx = lf.subset(n)
    m = len(idx)
    with api.Landmarks(0) as L:
        L.set(s.X, s.cov, lf.COV_SCALE)
        L.fuse(s.y, s.rot, s.tran, 1e-3, lf.GATE)
        before = _state(L)
        rep, desc, top = idx.copy(), idx.copy(), idx.copy()
        rep[3] = rep[2]
        desc[[4, 5]] = desc[[5, 4]]
        top[-1] = n
        asym = lf.POSE_COV_FULL.copy()
        asym[0, 4] = np.nextafter(asym[0, 4], 1.0)
        neg = lf.POSE_COV_FULL.copy()
        neg[2, 2] = -neg[2, 2]
        fz = lambda **kw: L.fuse(**{**dict(bearings=s.y[idx], rot=s.rot, tran=s.tran, bearing_sigma=1e-3, chi2_gate=lf.GATE, idx=idx), **kw})
        _refused(cabi.SBA_ERR_INVALID_ARG, {
            "idx with a repeat": lambda: fz(idx=rep), "idx descending": lambda: fz(idx=desc), "idx == n": lambda: fz(idx=top),
            "idx negative": lambda: fz(idx=np.concatenate([[-1], idx[1:]])),
            "m > n": lambda: L.fuse(np.ones((n + 1, 3)), s.rot, s.tran, idx=np.arange(n + 1)),
            "dense with m != n": lambda: L.fuse(s.y[:-1], s.rot, s.tran),
            "dense with m > n": lambda: L.fuse(np.ones((n + 1, 3)), s.rot, s.tran),
            "NaN gate": lambda: fz(chi2_gate=np.nan), "zero gate": lambda: fz(chi2_gate=0.0), "negative gate": lambda: fz(chi2_gate=-1.0),
            "negative sigma": lambda: fz(bearing_sigma=-1e-3), "NaN sigma": lambda: fz(bearing_sigma=np.nan),
            "infinite sigma": lambda: fz(bearing_sigma=np.inf),
            "asymmetric pose_cov": lambda: fz(pose_cov=asym), "negative pose variance": lambda: fz(pose_cov=neg),
            "NaN pose_cov": lambda: fz(pose_cov=np.full((6, 6), np.nan)),
            "bad cov_scale": lambda: L.set(s.X, s.cov, 0.0), "NaN cov_scale": lambda: L.set(s.X, s.cov, np.nan),
        })
        _refused(cabi.SBA_ERR_NUMERIC, {"NaN rot": lambda: fz(rot=np.array([0.1, np.nan, 0.0])), "infinite tran": lambda: fz(tran=np.array([np.inf, 0, 0]))})
        t = torch.zeros(9 * n + 4, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        _refused(cabi.SBA_ERR_INVALID_ARG, {
            "misaligned set": lambda: L.set_device(t.data_ptr() + 8, t.data_ptr() + 32, n), "null set": lambda: L.set_device(0, t.data_ptr(), n),
            "misaligned get": lambda: L.get_device(t.data_ptr() + 8, 0)})
        # the raw entry point: NULL arguments, nothing written
        lib, h = L._lib, L._h
        z3 = (C.c_double * 3)(*s.rot)
        opt = cabi.LandmarkFuseOptions(0.0, float("inf"), None, 1)
        res = cabi.LandmarkFuseResult(-7, -7, -7, -7, -7)
        yp = np.ascontiguousarray(s.y).ctypes.data_as(cabi._dp)
        for args in ((None, None, n, z3, z3, C.byref(opt), C.byref(res), None), (None, yp, n, None, z3, C.byref(opt), C.byref(res), None),
                     (None, yp, n, z3, z3, None, C.byref(res), None), (None, yp, n, z3, z3, C.byref(opt), None, None)):
            assert lib.sba_landmarks_fuse(h, *args) == cabi.SBA_ERR_INVALID_ARG and cabi.last_error(lib)
        assert res.n_obs == -7 and res.n_fused == -7
        assert _state(L) == before                                                 # every refusal left the map alone
        assert L.fuse(s.y[idx], s.rot, s.tran, 1e-3, lf.GATE, idx=idx).n_obs == m  # and the handle usable


def test_the_device_rows_round_trip():
    """set_device reads exactly n rows and get_device writes exactly n rows, odd n included: the guard doubles around them stay."""
    import torch
    dev = torch.device("cuda", 0)
    for n in (1, 2, 65, 512):
        s = lf.scene(n, "series") if n >= 63 else lf.scene(3, "series")
        X, cov = s.X[:n], s.cov[:n]
        tx = torch.from_numpy(X.copy()).to(dev)
        tc = torch.from_numpy(cov.copy()).to(dev)
        ox = torch.full((3 * n + 2,), -7.0, dtype=torch.float64, device=dev)
        oc = torch.full((6 * n + 2,), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        with api.Landmarks(0) as L, api.Landmarks(0) as T:
            L.set_device(tx.data_ptr(), tc.data_ptr(), n, lf.COV_SCALE)
            T.set(X, cov, lf.COV_SCALE)
            assert _state(L) == _state(T) and L.size == n
            L.get_device(ox.data_ptr(), oc.data_ptr())
            hx, hc = ox.cpu().numpy(), oc.cpu().numpy()
            Xg, Cg = L.get()
            assert hx[:3 * n].tobytes() == Xg.tobytes() and hc[:6 * n].tobytes() == Cg.tobytes()
            assert (hx[3 * n:] == -7.0).all() and (hc[6 * n:] == -7.0).all()
            L.get_device(0, oc.data_ptr())                                          # either output may be skipped
            L.get_device(ox.data_ptr(), None)


def test_the_chain_from_a_solved_pair_back_into_the_map():
    """A-B through solve_joint; its structure with covariances written to device tensors -> Landmarks.set_device -> get_device ->
    Problem.upload_device + set_landmark_covariances_device -> solve_resection_weighted -> resection_covariance -> Landmarks.fuse with
    that pose covariance.  Byte-identical to the same route through host arrays, and within the bounds of the reference run on the
    downloaded inputs."""
    import torch
    n = 513
    f = rr.three_frames(n, 71)
    factor = np.linalg.norm(f.tran_ab)
    opt = api.default_lm_options(tran_param=api.TRAN_SPHERE, **TIGHT)
    lm = api.default_lm_options(huber_delta=wr.DELTA, **TIGHT)
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    t_start = f.tran_ab / factor + 0.02 * axis
    dev = torch.device("cuda", 0)
    with api.Problem(0) as p, api.Problem(0) as q, api.Problem(0) as q2, api.Landmarks(0) as L, api.Landmarks(0) as L2:
        p.upload(f.x1, f.x2, f.d12 / factor * 1.01)
        rot, tran, d12, sm = p.solve_joint(f.rot_ab + 0.02 * axis, t_start / np.linalg.norm(t_start), options=opt)
        tx = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        tc = torch.zeros((n, 6), dtype=torch.float64, device=dev)
        ox, oc = torch.zeros_like(tx), torch.zeros_like(tc)
        gy = torch.from_numpy(np.ascontiguousarray(f.y)).to(dev)
        ones = torch.ones((n, 2), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        pose = p.structure_joint_into(tx.data_ptr(), tc.data_ptr(), None, rot, tran, options=opt)
        scale = max(pose.sigma2, 1e-6)            # noise-free frames: a covariance scale of its own keeps the update from being trivial
        L.set_device(tx.data_ptr(), tc.data_ptr(), n, scale)
        L.get_device(ox.data_ptr(), oc.data_ptr())
        q.upload_device(ox.data_ptr(), gy.data_ptr(), ones.data_ptr(), n)
        q.set_landmark_covariances_device(oc.data_ptr(), 1.0)
        g = q.resection_guess()
        r, t, s1, nb = q.solve_resection_weighted(g.rot, g.tran, lm, bearing_sigma=1e-3, reweight_rounds=2)
        cv = q.resection_covariance(r, t, lm)
        X0, C0 = L.get()
        assert np.isfinite(X0).all() and np.isfinite(C0).all()
        fd = L.fuse(f.y, r, t, 1e-3, lf.GATE, cv.cov)
        assert fd.n_obs == n and fd.n_fused == n and nb == 0
        # the same route through host arrays
        st = p.structure_joint(rot, tran, options=opt)
        L2.set(st.xyz, st.cov, scale)
        Xh, Ch = L2.get()
        assert Xh.tobytes() == X0.tobytes() and Ch.tobytes() == C0.tobytes()
        q2.upload(Xh, f.y, np.ones((n, 2)))
        q2.set_landmark_covariances(Ch, 1.0)
        g2 = q2.resection_guess()
        r2, t2, s2, nb2 = q2.solve_resection_weighted(g2.rot, g2.tran, lm, bearing_sigma=1e-3, reweight_rounds=2)
        cv2 = q2.resection_covariance(r2, t2, lm)
        assert r2.tobytes() == r.tobytes() and t2.tobytes() == t.tobytes() and cv2.cov.tobytes() == cv.cov.tobytes()
        fh = L2.fuse(f.y, r2, t2, 1e-3, lf.GATE, cv2.cov)
        assert _state(L2) == _state(L) and fh.chi2.tobytes() == fd.chi2.tobytes() and _counts(fh) == _counts(fd)
        # the reference on the downloaded inputs
        ref = lf.fuse(X0, C0, f.y, r, t, 1e-3, lf.GATE, cv.cov)
        assert ref.counts() == _counts(fd)
        X1, C1 = L.get()
        err = np.array(lf.errors(X1, C1, fd.chi2, ref, X0, C0))
        assert (err <= _bounds()).all(), (err, _bounds())
        assert (C1[:, :3] <= C0[:, :3]).all() and (C1[:, :3] < C0[:, :3]).any()                # the frame taught the map something
        assert np.abs(r - f.rot_bc).max() <= 1e-6 and np.abs(t * factor - f.tran_bc).max() <= 1e-6
