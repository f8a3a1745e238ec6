"""GPU: the spherical resection (Problem.eval_resection / solve_resection / resection_depths / resection_guess) against the
long-double restatement of tests/resection_reference.py, on the scenes tests/test_resection_host_cpu.py qualifies (float64
numpy in its own order meets the same bounds there), at the vector-per-lane and block edges of both plane types, over
several grid-stride steps (SBA_RESECT_GRID=1), with and without the loss; the d2 column is not read; the existing per-match
machinery sees the same problem once the eliminated depths are stored; the linear start; the solve against the harness-driven
solver with the numpy evaluator; refusals."""
import numpy as np
import pytest

import pose_edges
import resection_reference as rr
from helpers import REL_TOL_F32, REL_TOL_F64, RT_TOL_F32, RT_TOL_F64, assert_normal_eq_close
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api
from test_resection_host_cpu import EDGE_AXIS, GPU_LOSSES, LM_DELTA, LM_SCENES, edge_eval_scene

pytestmark = pytest.mark.gpu

STORES = [api.STORE_F64, api.STORE_F32]
IDS = ["f64", "f32"]
SIZES = {api.STORE_F64: (0, 1, 2, 3, 63, 64, 65, 511, 512, 513), api.STORE_F32: (0, 1, 2, 3, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025)}
LONG = {api.STORE_F64: 1537, api.STORE_F32: 3073}        # SBA_RESECT_GRID=1: three grid-stride steps and a ragged tail
TERMINATION = {v: k for k, v in cabi.TERMINATION.items()}
# The LM stops on the parameter tolerance BEFORE it takes the step that meets it, so the result is about one such step from the
# optimum: the tolerances sit well below RT_TOL.
TIGHT = dict(function_tolerance=1e-30, parameter_tolerance=1e-13, gradient_tolerance=1e-13, max_num_iterations=100)


def _rel(store):
    return REL_TOL_F64 if store == api.STORE_F64 else REL_TOL_F32


def _rt(store):
    return RT_TOL_F64 if store == api.STORE_F64 else RT_TOL_F32


def _eval_scene(n, with_outliers):
    return rr.make_scene(n, 500 + n, noise=1e-3, outliers=rr.planted(n) if with_outliers else ())


def _check(got, ref, rel, what):
    assert_normal_eq_close(got, ref, rel, what)
    assert (got.n_outlier, got.n_behind) == (ref.n_outlier, ref.n_behind), what
    assert abs(got.sum_w - ref.sum_w) <= rel * max(ref.sum_w, 1e-300), what
    assert np.array_equal(got.H, got.H.T), what


def _eval_cases(p, n, store, what):
    for delta, with_outliers in GPU_LOSSES:
        s = _eval_scene(n, with_outliers)
        X, y = rr.planes(s, store == api.STORE_F32)
        rot, tran = rr.start_near(s, n)
        p.upload_landmarks(s.X, s.y, store=store)
        got = p.eval_resection(rot, tran, api.default_lm_options(huber_delta=delta))
        ref = rr.sums(X, y, rot, tran, delta)
        _check(got, ref, _rel(store), f"{what} n={n} delta={delta}")
        if with_outliers and n >= 63:
            assert got.n_outlier >= 1
        if delta == 0.0 and n > 0:
            assert got.sum_w == n and got.n_outlier == 0


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_eval_against_long_double(store):
    with api.Problem(0) as p:
        for n in SIZES[store]:
            _eval_cases(p, n, store, "eval")


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_eval_over_several_grid_stride_steps(monkeypatch, store):
    monkeypatch.setenv("SBA_RESECT_GRID", "1")
    with api.Problem(0) as p:
        _eval_cases(p, LONG[store], store, "one block")
        for n in (513, 1025):
            _eval_cases(p, n, store, "one block")


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_n_behind_counts_landmarks_behind_the_bearing(store):
    s = rr.make_scene(65, 21)
    y = s.y.copy()
    y[[3, 40, 64]] *= -1.0                                 # the landmark lies behind these bearings: d* < 0
    with api.Problem(0) as p:
        p.upload_landmarks(s.X, y, store=store)
        got = p.eval_resection(s.rot, s.tran, api.default_lm_options(huber_delta=0.0))
        assert got.n_behind == 3 and got.sum_w == 65
        d = p.resection_depths(s.rot, s.tran)
        assert np.array_equal(np.flatnonzero(d <= 0), [3, 40, 64])


def _bytes(*arrays):
    return b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in arrays)


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_the_d2_column_is_not_read(store):
    n = 513
    s = rr.make_scene(n, 31, noise=1e-3, outliers=rr.planted(n))
    rot, tran = rr.start_near(s, 31)
    opt = api.default_lm_options(huber_delta=LM_DELTA)
    poison = np.ones((n, 2))
    poison[0::2, 1] = np.nan
    poison[1::2, 1] = 0.0
    seen = []
    with api.Problem(0) as p:
        for d12 in (np.ones((n, 2)), poison):
            p.upload(s.X, s.y, d12, store=store)
            e = p.eval_resection(rot, tran, opt)
            g = p.resection_guess(moments=True)
            r, t, sm, nb = p.solve_resection(rot, tran, opt, store_depths=False)
            seen.append(_bytes(e.H, e.g, [e.cost, e.sum_w, e.n_outlier, e.n_behind], g.rot, g.tran,
                               [g.lambda1, g.lambda2, g.lambda12, g.scale, g.n_behind], g.sv, g.moments, r, t,
                               [sm.num_iterations, sm.num_evaluations, sm.final_cost, nb]))
    assert seen[0] == seen[1]


@pytest.fixture
def pinned_grid(monkeypatch):
    """Same blocks per CU for every sweep variant (read at handle creation): a compacted and a fresh handle then reduce in
    the same order and their packs compare bit for bit (tests/test_gpu_quantile.py)."""
    monkeypatch.setenv("SBA_BLOCKS_PER_CU", "2")


@pytest.mark.parametrize("store", STORES, ids=IDS)
@pytest.mark.parametrize("n", [65, 1025])
def test_the_per_match_machinery_sees_the_same_problem(pinned_grid, n, store):
    s = rr.make_scene(n, 41 + n, noise=1e-3, outliers=rr.planted(n))
    X, y = rr.planes(s, store == api.STORE_F32)
    rot, tran = rr.start_near(s, 41)
    rel, delta = _rel(store), LM_DELTA
    opt = api.default_lm_options(huber_delta=delta)
    kw = dict(depth_mode=api.DEPTH_PER_MATCH)
    with api.Problem(0) as p, api.Problem(0) as q:
        p.upload_landmarks(s.X, s.y, store=store)
        eq = p.eval_resection(rot, tran, opt)
        d = p.resection_depths(rot, tran)
        _, dref, rref, _, _ = rr.per_match(X, y, rot, tran)
        assert np.abs(d - dref.astype(np.float64)).max() <= rel * np.abs(X).max()
        # the plane holds what was returned: a joint solve that may not iterate hands the handle's depths back untouched
        _, _, d12, _ = p.solve_joint(rot, tran, options=api.default_lm_options(max_num_iterations=0, tran_param=api.TRAN_SPHERE))
        assert np.array_equal(d12[:, 1], d) and np.array_equal(d12[:, 0], np.ones(n))
        res = p.residuals(rot, tran, huber_delta=delta, fields=("e", "sq_norm", "inlier"), **kw)
        assert np.abs(res.e - rref.astype(np.float64)).max() <= rel * np.abs(X).max()
        assert n - res.n_inlier == eq.n_outlier and eq.n_outlier >= 1
        ne = p.eval(api.MODE_RT, rot, tran, huber_delta=delta, **kw)
        assert abs(ne.cost - eq.cost) <= rel * eq.cost and ne.n_outlier == eq.n_outlier
        sg = max(np.abs(eq.g).max(), rel * np.abs(eq.H).max())
        assert np.abs(ne.g - eq.g).max() <= 10 * rel * sg
        assert np.abs(ne.H - eq.H).max() > 1e-3 * np.abs(eq.H).max()          # only H differs: by sum w J^T y^ y^^T J
        # the cut, then the resection again: a fresh upload of the kept rows, bit for bit
        idx, thr = p.keep_below(rot, tran, 0.9, 1.0, **kw)
        assert 0 < len(idx) < n and np.array_equal(idx, np.flatnonzero(res.sq_norm <= thr))
        after = p.eval_resection(rot, tran, opt)
        q.upload(s.X[idx], s.y[idx], np.stack([np.ones(len(idx)), d[idx]], axis=1), store=store)
        fresh = q.eval_resection(rot, tran, opt)
        assert _bytes(after.H, after.g, [after.cost, after.sum_w, after.n_outlier, after.n_behind]) == \
               _bytes(fresh.H, fresh.g, [fresh.cost, fresh.sum_w, fresh.n_outlier, fresh.n_behind])
        assert after.n_outlier < eq.n_outlier


def _check_moments(p, s, store, what):
    X, y = rr.planes(s, store == api.STORE_F32)
    p.upload_landmarks(s.X, s.y, store=store)
    g = p.resection_guess(moments=True)
    ref = rr.moments(X, y)
    # f64 arithmetic on both sides of the same (rounded) inputs: the f64 bound for either plane type
    assert np.abs(g.moments - ref.astype(np.float64)).max() <= REL_TOL_F64 * float(np.abs(ref).max()), what
    assert g.n == len(X), what
    return g, rr.dlt(ref.astype(np.float64))


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_moments_and_guess(monkeypatch, store):
    with api.Problem(0) as p:
        for n in [k for k in SIZES[store] if k >= 6] + [6, 7]:
            s = _eval_scene(n, False)
            g, ref = _check_moments(p, s, store, f"moments n={n}")
            if n >= 63:                                        # noisy, well-conditioned: the numpy DLT on the same inputs
                assert ref.lam[1] / ref.lam[11] >= 1e-5
                assert np.abs(g.rot - ref.rot).max() <= _rt(store) and np.abs(g.tran - ref.tran).max() <= _rt(store), n
                assert g.n_behind == 0
        for n in (6, 65, 513):                                 # noise-free: the truth (f32 planes: the numpy DLT of the rounded inputs)
            s = rr.make_scene(n, 100 + n)
            g, ref = _check_moments(p, s, store, f"exact n={n}")
            want = (s.rot, s.tran) if store == api.STORE_F64 else (ref.rot, ref.tran)
            assert np.abs(g.rot - want[0]).max() <= _rt(store) and np.abs(g.tran - want[1]).max() <= _rt(store), n
            assert g.lambda2 > 0 and g.lambda12 > g.lambda2 and g.n_behind == 0
            if store == api.STORE_F64:
                assert g.lambda1 <= 1e-12 * g.lambda12 and np.abs(g.sv - 1.0).max() <= 1e-9
        monkeypatch.setenv("SBA_RESECT_GRID", "1")
        _check_moments(p, _eval_scene(LONG[store], False), store, "one block")


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_guess_refusals_leave_the_handle_usable(store):
    flat, five, ok = rr.make_scene(65, 5, planar=True), rr.make_scene(5, 5), rr.make_scene(65, 6)
    with api.Problem(0) as p:
        for s in (flat, five):
            p.upload_landmarks(s.X, s.y, store=store)
            with pytest.raises(api.SbaError) as ei:
                p.resection_guess()
            assert ei.value.code == cabi.SBA_ERR_NUMERIC
            assert np.isfinite(p.eval_resection(s.rot, s.tran).cost)
        p.upload_landmarks(ok.X, ok.y, store=store)
        assert np.abs(p.resection_guess().rot - ok.rot).max() <= _rt(store)


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_solve_returns_the_truth_on_noise_free_scenes(store):
    opt = api.default_lm_options(**TIGHT)
    with api.Problem(0) as p:
        for n in (6, 65, 513):
            s = rr.make_scene(n, 100 + n)
            p.upload_landmarks(s.X, s.y, store=store)
            r0, t0 = rr.start_near(s, n)
            r, t, sm, nb = p.solve_resection(r0, t0, opt)
            assert np.abs(r - s.rot).max() <= _rt(store) and np.abs(t - s.tran).max() <= _rt(store), (n, sm)
            assert nb == 0 and sm.final_cost <= sm.initial_cost
            # the eliminated depths at the result are the true depths along the bearings
            assert np.abs(p.resection_depths(r, t) - s.depth).max() <= 100 * _rt(store)


@pytest.mark.parametrize("store", STORES, ids=IDS)
@pytest.mark.parametrize("name", pose_edges.NAMES)
def test_solve_at_the_pose_edges(name, store):
    """The rotations where the rotation frame changes, as the truth (start 0.05 off) and as the start (truth 3 degrees off)."""
    w = pose_edges.POSES[name]
    opt = api.default_lm_options(**TIGHT)
    axis = EDGE_AXIS
    with api.Problem(0) as p:
        for truth, start in ((w, w + 0.05 * axis), (w + np.deg2rad(3.0) * axis, w)):
            s = rr.make_scene(129, 61, rot=truth)
            p.upload_landmarks(s.X, s.y, store=store)
            r, t, sm, _ = p.solve_resection(start, s.tran + 0.05 * axis, opt)
            assert np.abs(r - truth).max() <= _rt(store) and np.abs(t - s.tran).max() <= _rt(store), (name, sm)
        # one evaluation AT the rotation against long double
        s = edge_eval_scene(name)
        X, y = rr.planes(s, store == api.STORE_F32)
        p.upload_landmarks(s.X, s.y, store=store)
        _check(p.eval_resection(w, s.tran, api.default_lm_options(huber_delta=LM_DELTA)), rr.sums(X, y, w, s.tran, LM_DELTA), _rel(store), name)


@pytest.mark.parametrize("store", STORES, ids=IDS)
@pytest.mark.parametrize("n,seed", LM_SCENES)
def test_solve_equals_the_harness_driven_solver(n, seed, store):
    s = rr.make_scene(n, seed, noise=1e-3, outliers=rr.planted(n))
    X, y = rr.planes(s, store == api.STORE_F32)
    rc, r0, t0, *_ = rr.harness_dlt(rr.moments(X, y).astype(np.float64), n)
    assert rc == 0
    rh, th, sh, rch = rr.harness_solve(r0, t0, rr.numpy_evaluator(X, y, LM_DELTA))
    assert rch == 0
    with api.Problem(0) as p:
        p.upload_landmarks(s.X, s.y, store=store)
        r, t, sm, nb = p.solve_resection(r0, t0, api.default_lm_options(huber_delta=LM_DELTA))
        assert (TERMINATION[sm.termination], sm.num_iterations, sm.num_successful_steps, sm.num_evaluations) == \
               (sh.termination, sh.num_iterations, sh.num_successful_steps, sh.num_evaluations)
        assert np.abs(r - rh).max() <= _rt(store) and np.abs(t - th).max() <= _rt(store)
        assert abs(sm.final_cost - sh.final_cost) <= _rel(store) * sh.final_cost
        assert nb == rr.sums(X, y, r, t, LM_DELTA).n_behind
        # store_depths: the handle's per-match residuals are the resection's at the result
        res = p.residuals(r, t, huber_delta=LM_DELTA, depth_mode=api.DEPTH_PER_MATCH, fields=("sq_norm",))
        rho = np.where(res.sq_norm > LM_DELTA ** 2, 2 * LM_DELTA * np.sqrt(res.sq_norm) - LM_DELTA ** 2, res.sq_norm)
        assert abs(0.5 * rho.sum() - sm.final_cost) <= 10 * _rel(store) * sm.final_cost


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_solve_limits_gauge_and_reproducibility(store):
    s = rr.make_scene(513, 300, noise=1e-3, outliers=rr.planted(513))
    r0, t0 = rr.start_near(s, 300)
    with api.Problem(0) as p:
        p.upload_landmarks(s.X, s.y, store=store)
        r, t, sm, _ = p.solve_resection(r0, t0, api.default_lm_options(huber_delta=LM_DELTA, max_num_iterations=1))
        assert sm.termination == "NO_CONVERGENCE" and sm.num_iterations == 1 and sm.num_evaluations == 2
        r, t, sm, _ = p.solve_resection(r0, t0, api.default_lm_options(huber_delta=LM_DELTA, tran_param=api.TRAN_SPHERE))
        assert abs(np.linalg.norm(t) - np.linalg.norm(t0)) <= 1e-14 and sm.num_successful_steps >= 1
        # the default: a free translation -- the landmarks fix the scale
        r, t, sm, nb = p.solve_resection(r0, t0, api.default_lm_options(huber_delta=LM_DELTA))
        assert abs(np.linalg.norm(t) - np.linalg.norm(s.tran)) < abs(np.linalg.norm(t0) - np.linalg.norm(s.tran))
        again = p.solve_resection(r0, t0, api.default_lm_options(huber_delta=LM_DELTA))
        assert _bytes(r, t, [sm.final_cost, sm.num_evaluations, nb]) == _bytes(again[0], again[1], [again[2].final_cost, again[2].num_evaluations, again[3]])
        e1, e2 = p.eval_resection(r, t), p.eval_resection(r, t)
        assert _bytes(e1.H, e1.g, [e1.cost]) == _bytes(e2.H, e2.g, [e2.cost])


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_a_third_frame_against_the_structure_of_a_pair(store):
    """A-B through solve_joint and structure_joint, then C resected against those landmarks.  The pair's |tran| is pinned to 1, so
    its structure -- and the B -> C translation the resection returns -- is in units of the true |tran_ab| = 0.7.  Noise-free;
    the pair's pose is good to RT_TOL and a landmark amplifies a pose error by depth / baseline <= 10 / 0.7 < 100."""
    f = rr.three_frames(513, 71)
    factor = np.linalg.norm(f.tran_ab)
    opt = api.default_lm_options(tran_param=api.TRAN_SPHERE, **TIGHT)
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    t_start = f.tran_ab / factor + 0.02 * axis
    with api.Problem(0) as p, api.Problem(0) as q:
        p.upload(f.x1, f.x2, f.d12 / factor * 1.01, store=store)
        rot, tran, d12, sm = p.solve_joint(f.rot_ab + 0.02 * axis, t_start / np.linalg.norm(t_start), options=opt)
        assert np.abs(rot - f.rot_ab).max() <= _rt(store) and np.abs(tran * factor - f.tran_ab).max() <= _rt(store), sm
        xyz = p.structure_joint(rot, tran, options=opt, cov=False, score=False).xyz
        q.upload_landmarks(xyz, f.y, store=store)
        g = q.resection_guess()
        r, t, sm, nb = q.solve_resection(g.rot, g.tran, api.default_lm_options(**TIGHT))
        assert nb == 0
        assert np.abs(r - f.rot_bc).max() <= 100 * _rt(store) and np.abs(t * factor - f.tran_bc).max() <= 100 * _rt(store), sm


def test_refusals():
    s = rr.make_scene(65, 81, noise=1e-3)
    rot, tran = rr.start_near(s, 81)
    with api.Problem(0) as p:
        calls = (lambda: p.eval_resection(rot, tran), lambda: p.solve_resection(rot, tran), lambda: p.resection_depths(rot, tran),
                 lambda: p.resection_guess())

        def refused(code, which=calls):
            for call in which:
                with pytest.raises(api.SbaError) as ei:
                    call()
                assert ei.value.code == code

        refused(cabi.SBA_ERR_NOT_UPLOADED)
        p.upload(s.X, s.y)                                 # no per-match depths: no landmarks
        refused(cabi.SBA_ERR_UNSUPPORTED)
        p.upload_landmarks(s.X, s.y)
        before = p.eval_resection(rot, tran)
        p.set_shard(0, 2)
        refused(cabi.SBA_ERR_UNSUPPORTED)
        p.set_shard(0, 1)
        p.set_allreduce(lambda buf, count, stream: 0)
        refused(cabi.SBA_ERR_UNSUPPORTED)
        p.set_allreduce(None)
        bad = np.array([0.1, np.nan, 0.0])
        refused(cabi.SBA_ERR_NUMERIC, (lambda: p.eval_resection(bad, tran), lambda: p.solve_resection(rot, bad),
                                       lambda: p.resection_depths(np.array([np.inf, 0, 0]), tran)))
        # a zero bearing: non-finite sums, reported, and the handle stays usable
        y = s.y.copy()
        y[7] = 0.0
        p.upload_landmarks(s.X, y)
        refused(cabi.SBA_ERR_NUMERIC, (lambda: p.eval_resection(rot, tran), lambda: p.solve_resection(rot, tran)))
        p.upload_landmarks(s.X, s.y)
        after = p.eval_resection(rot, tran)
        assert _bytes(after.H, after.g, [after.cost]) == _bytes(before.H, before.g, [before.cost])
