"""GPU: the batched joint solve -- every pair's depths, rotation and translation free together (Batch.eval_joint / solve_joint,
sba_batch_eval_joint / sba_batch_solve_joint; kernels csrc/sba_batch_joint.hip, per-match source csrc/sba_joint_core.hpp).

eval_joint is checked pair by pair against Problem.eval_joint on the pair alone and against the long-double element-wise Schur
complement of tests/ref_joint_numpy.py; solve_joint against the dense restatement and Problem.solve_joint; the one-launch
device driver against the host lock-step driver (SBA_BATCH_DEVICE_JOINT=0) bit for bit."""
import ctypes as C
import time

import numpy as np
import pytest

import ref_joint_numpy as rj
from helpers import REL_TOL_F64, RT_TOL_F32, RT_TOL_F64
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api, synthetic

pytestmark = pytest.mark.gpu

STORES = (api.STORE_F64, api.STORE_F32)
LAYOUTS = ("0", "1")          # SBA_BATCH_INTERLEAVE, as tests/test_gpu_batch.py selects the pair layout
RADII = (float("inf"), 1e4, 1.0, 1e-2)
RAGGED = (0, 1, 2, 3, 255, 256, 257, 4097, 50_000)
# (n, seed, scene arguments): ref_joint_numpy.dense_solve reports margin >= 0.036 for every one of them, with the f64 inputs and
# with the f32-rounded ones (checked on the CPU when the seeds were picked; asserted again below).  5 to 8 iterations each.
SOLVE_SCENES = ((300, 0, {}), (200, 1, dict(sigma=0.0, outlier_fraction=0.0)), (257, 2, dict(sigma=2e-3)), (150, 3, {}), (333, 4, {}),
                (180, 5, dict(outlier_fraction=0.0)), (256, 6, {}), (221, 7, dict(sigma=5e-4)), (129, 8, {}), (301, 9, dict(sigma=2e-3)),
                (190, 10, {}), (240, 11, {}))


def _scene(n, seed=0, **kw):
    args = dict(sigma=1e-3, outlier_fraction=0.1, depth_noise=0.05)
    args.update(kw)
    return synthetic.full_rt(n, seed=synthetic.BASE_SEED + 270 + seed, **args)


def _planes(c, store):
    """What the planes hold: f32 planes are the f32-rounded inputs."""
    if store == api.STORE_F64:
        return c.x1, c.x2
    return c.x1.astype(np.float32).astype(np.float64), c.x2.astype(np.float32).astype(np.float64)


def _cat(cs):
    sizes = [len(c.x1) for c in cs]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    x1 = np.concatenate([c.x1 for c in cs]).reshape(-1, 3)
    x2 = np.concatenate([c.x2 for c in cs]).reshape(-1, 3)
    d12 = np.concatenate([c.d12 for c in cs]).reshape(-1, 2)
    rot = np.stack([c.rot_init for c in cs]); tran = np.stack([c.tran_init for c in cs])
    return off, x1, x2, d12, rot, tran


def _solve_scenes():
    return [_scene(n, seed, **kw) for n, seed, kw in SOLVE_SCENES]


def _counts(s):
    return (s.termination, s.num_iterations, s.num_successful_steps, s.num_evaluations)


def _same_solve(a, b):
    """(rot, tran, d12, summaries, status) of two solves: equal bits, equal counts."""
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[4], b[4])
    for u, v in zip(a[3], b[3]):
        assert _counts(u) == _counts(v) and (u.initial_cost, u.final_cost, u.final_radius) == (v.initial_cost, v.final_cost, v.final_radius)


@pytest.mark.parametrize("layout", LAYOUTS, ids=["contiguous", "interleaved"])
@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
def test_eval_joint_matches_the_single_problem_eval(monkeypatch, store, layout):
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    cs = [_scene(n, seed=20 + i) for i, n in enumerate(RAGGED)]
    off, x1, x2, d12, rot, tran = _cat(cs)
    with api.Batch(0) as b:
        b.upload(x1, x2, off, d12, store=store)
        got = {radius: b.eval_joint(rot, tran, radius) for radius in RADII}
        res = b.residuals(rot, tran, depth_mode=api.DEPTH_PER_MATCH, fields=())
    for g, c in enumerate(cs):
        n = len(c.x1)
        if n == 0:
            for radius in RADII:
                e = got[radius][g]
                assert not e.S.any() and not e.gs.any() and not e.V.any() and not e.gc.any()
                assert (e.cost, e.sum_w, e.n_outlier, e.gd_max) == (0.0, 0.0, 0.0, 0.0)
            continue
        a1, a2 = _planes(c, store)
        with api.Problem(0) as p:
            p.upload(c.x1, c.x2, c.d12, store=store)
            for radius in RADII:
                e, ref = got[radius][g], p.eval_joint(c.rot_init, c.tran_init, radius)
                ld = rj.schur_longdouble(a1, a2, c.rot_init, c.tran_init, c.d12, radius)
                scale = float(np.abs(ref.V).max())
                errs = {k: float(np.abs(getattr(e, k) - getattr(ref, k)).max()) / scale for k in ("S", "gs", "V", "gc")}
                err_ld = max(float(np.abs(e.S - ld["S"]).max()), float(np.abs(e.gs - ld["gs"]).max())) / float(np.abs(ld["V"]).max())
                print(f"n={n} store={store} layout={layout} radius={radius:g}: vs single {errs}, S/gs vs long double {err_ld:.3e}")
                assert max(errs.values()) <= REL_TOL_F64, (n, radius, errs)
                assert err_ld <= REL_TOL_F64, (n, radius, err_ld)
                assert abs(e.cost - ref.cost) <= REL_TOL_F64 * ref.cost and abs(e.sum_w - ref.sum_w) <= REL_TOL_F64 * ref.sum_w
                assert e.n_outlier == ref.n_outlier == n - res.n_inlier[g]
                assert abs(e.gd_max - ref.gd_max) <= REL_TOL_F64 * max(ref.gd_max, 1.0)
                assert np.array_equal(e.S, e.S.T)


@pytest.mark.parametrize("layout", LAYOUTS, ids=["contiguous", "interleaved"])
@pytest.mark.parametrize("store,tol", [(api.STORE_F64, RT_TOL_F64), (api.STORE_F32, RT_TOL_F32)], ids=["f64", "f32"])
def test_solve_joint_matches_dense_and_the_single_problem_solve(monkeypatch, store, tol, layout):
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    cs = _solve_scenes()
    off, x1, x2, d12, rot0, tran0 = _cat(cs)
    with api.Batch(0) as b:
        b.upload(x1, x2, off, d12, store=store)
        rot, tran, d, sums, status = b.solve_joint(rot0, tran0)
        at = b.residuals(rot, tran, depth_mode=api.DEPTH_PER_MATCH, fields=("sq_norm",))
    assert not status.any()
    for g, c in enumerate(cs):                    # every pair shown to the GPU is compared
        a1, a2 = _planes(c, store)
        lo, hi = int(off[g]), int(off[g + 1])
        rr, tr, dr, sr = rj.dense_solve(a1, a2, c.rot_init, c.tran_init, c.d12)
        assert sr["margin"] >= 1e-3, (g, sr)
        s = sums[g]
        assert (s.termination.replace("CONVERGENCE_", "").lower(), s.num_iterations, s.num_successful_steps, s.num_evaluations) == \
            (sr["termination"], sr["num_iterations"], sr["num_successful_steps"], sr["num_evaluations"]), g
        with api.Problem(0) as p:
            p.upload(c.x1, c.x2, c.d12, store=store)
            pr, pt, pd, ps = p.solve_joint(c.rot_init, c.tran_init)
        assert _counts(s) == _counts(ps), g
        for ref_r, ref_t, ref_d in ((rr, tr, dr), (pr, pt, pd)):
            assert np.abs(rot[g] - ref_r).max() <= tol and np.abs(tran[g] - ref_t).max() <= tol, g
            assert np.abs(d[lo:hi] - ref_d).max() <= tol * np.abs(ref_d).max(), g
        assert s.final_cost <= s.initial_cost
        sq = at.sq_norm[lo:hi]
        rho = np.where(sq > 1.0, 2.0 * np.sqrt(sq) - 1.0, sq)
        # REL_TOL_F64 of the cost.  The noise-free scenes (sigma = 0) alone get, on top, what f64 can resolve at all: there the
        # final cost (1e-17) is a sum of squared residuals of 1e-10, and a residual component is a sum of four terms of size up
        # to max(|d|, |t|), so it carries an absolute rounding error of up to 4 eps of that, and a squared norm 2 |e| sqrt(3)
        # times as much.  Every scene with noise is held to REL_TOL_F64 alone.
        floor = 0.0
        if SOLVE_SCENES[g][2].get("sigma", 1.0) == 0.0:
            floor = len(sq) * 2.0 * np.sqrt(3.0 * sq.max()) * 4.0 * np.finfo(np.float64).eps * max(np.abs(d[lo:hi]).max(), np.abs(tran[g]).max())
        got_cost = 0.5 * rho.sum()
        print(f"pair {g}: final_cost {s.final_cost:.6e}, from residuals {got_cost:.6e}, difference {abs(got_cost - s.final_cost):.3e}, "
              f"relative bound {REL_TOL_F64 * s.final_cost:.3e}, resolution floor {floor:.3e}")
        assert abs(got_cost - s.final_cost) <= REL_TOL_F64 * s.final_cost + floor, g


@pytest.mark.parametrize("layout", LAYOUTS, ids=["contiguous", "interleaved"])
@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
def test_device_driver_equals_lock_step_driver_bitwise(monkeypatch, store, layout):
    """Both drivers run the same pass code from parameters built on the device and the same solver source: equal bits.  The
    pairs finish after 5 to 8 iterations; an empty pair, 1- and 2-match pairs, a large one and an iteration cap ride along."""
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    cs = _solve_scenes() + [_scene(n, seed=40 + i) for i, n in enumerate((0, 1, 2, 4097, 20_001))]
    off, x1, x2, d12, rot0, tran0 = _cat(cs)
    for opts in (None, api.default_lm_options(max_num_iterations=3, tran_param=api.TRAN_SPHERE), api.default_lm_options(tran_param=api.TRAN_FREE)):
        got = {}
        for driver in ("1", "0"):
            monkeypatch.setenv("SBA_BATCH_DEVICE_JOINT", driver)
            with api.Batch(0) as b:
                b.upload(x1, x2, off, d12, store=store)
                got[driver] = b.solve_joint(rot0, tran0, options=opts, check=False)
        _same_solve(got["1"], got["0"])
        its = sorted({s.num_iterations for s in got["1"][3]})
        print(f"store={store} layout={layout}: iterations per pair {its}")
        if opts is None:
            assert len(its) >= 3 and not got["1"][4].any()


def test_independence_and_determinism(monkeypatch):
    cs = _solve_scenes()[:5] + [_scene(4097, seed=44)]
    off, x1, x2, d12, rot0, tran0 = _cat(cs)
    runs = {}
    for layout in LAYOUTS:
        monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
        with api.Batch(0) as b:
            b.upload(x1, x2, off, d12)
            ev = b.eval_joint(rot0, tran0, 10.0)
            first = b.solve_joint(rot0, tran0)
            b.set_depths(d12)
            _same_solve(first, b.solve_joint(rot0, tran0))            # run twice
            b.set_depths(d12)
            ev2 = b.eval_joint(rot0, tran0, 10.0)
        runs[layout] = (ev, first)
        for u, v in zip(ev, ev2):
            assert all(np.array_equal(getattr(u, k), getattr(v, k)) for k in ("S", "gs", "V", "gc")) and (u.cost, u.gd_max) == (v.cost, v.gd_max)
    _same_solve(runs["0"][1], runs["1"][1])                           # either layout
    for u, v in zip(runs["0"][0], runs["1"][0]):
        assert all(np.array_equal(getattr(u, k), getattr(v, k)) for k in ("S", "gs", "V", "gc")) and u.cost == v.cost
    rot, tran, d, sums, _ = runs["0"][1]
    for g, c in enumerate(cs):                                        # alone in a batch
        with api.Batch(0) as b:
            b.upload(c.x1, c.x2, np.array([0, len(c.x1)], dtype=np.uint64), c.d12)
            e1 = b.eval_joint(c.rot_init[None], c.tran_init[None], 10.0)[0]
            r1, t1, d1, s1, _ = b.solve_joint(c.rot_init[None], c.tran_init[None])
        assert all(np.array_equal(getattr(e1, k), getattr(runs["0"][0][g], k)) for k in ("S", "gs", "V", "gc"))
        assert np.array_equal(r1[0], rot[g]) and np.array_equal(t1[0], tran[g]) and np.array_equal(d1, d[int(off[g]):int(off[g + 1])])
        assert _counts(s1[0]) == _counts(sums[g]) and s1[0].final_cost == sums[g].final_cost


@pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
def test_state_after_solve_joint(store):
    # noisy scenes: their final cost is far above what f64 resolves in a residual, so REL_TOL_F64 of it is a meaningful bound
    cs = [c for k, c in enumerate(_solve_scenes()[:6]) if SOLVE_SCENES[k][2].get("sigma", 1.0) > 0.0] + [_scene(5001, seed=47), _scene(0, seed=48)]
    off, x1, x2, d12, rot0, tran0 = _cat(cs)
    B = len(cs)
    with api.Batch(0) as b, api.Batch(0) as q:
        b.upload(x1, x2, off, d12, store=store)
        rot, tran, d, sums, status = b.solve_joint(rot0, tran0)
        assert not status.any() and not np.array_equal(d, d12)
        # the refined depths are in the batch's planes: the per-match sweep at the returned camera reproduces final_cost
        packs = b.eval(api.MODE_RT, rot, tran, depth_mode=api.DEPTH_PER_MATCH)
        for g in range(B):
            assert abs(packs[g][22] - sums[g].final_cost) <= REL_TOL_F64 * max(sums[g].final_cost, 1e-300), g
        # d12_out is what the planes hold: read them back directly -- a solve with no iteration allowed runs one reduce pass, takes
        # no step and copies the planes out
        back = b.solve_joint(rot, tran, options=api.default_lm_options(max_num_iterations=0, tran_param=api.TRAN_SPHERE))
        assert all(x.num_iterations == 0 and x.num_successful_steps == 0 and x.termination in ("NO_CONVERGENCE", "CONVERGENCE_GRADIENT") for x in back[3])
        assert np.array_equal(back[2], d) and np.array_equal(back[0], rot) and np.array_equal(back[1], tran)
        # ... and a handle uploaded with it gives the same sweep, bit for bit
        q.upload(x1, x2, off, d, store=store)
        assert np.array_equal(packs, q.eval(api.MODE_RT, rot, tran, depth_mode=api.DEPTH_PER_MATCH))
        e_b = b.residuals(rot, tran, depth_mode=api.DEPTH_PER_MATCH, fields=("e",)).e
        assert np.array_equal(e_b, q.residuals(rot, tran, depth_mode=api.DEPTH_PER_MATCH, fields=("e",)).e)
        # set_depths + a second solve reproduces the first
        b.set_depths(d12)
        _same_solve((rot, tran, d, sums, status), b.solve_joint(rot0, tran0))
        # keep the inliers, solve again == a fresh upload of the kept rows solved once (threshold from the residuals: after the
        # joint solve hardly any match is left outside Huber's region at delta = 1)
        sq = b.residuals(rot, tran, depth_mode=api.DEPTH_PER_MATCH, fields=("sq_norm",)).sq_norm
        delta = float(np.sqrt(np.quantile(sq, 0.8)))
        kept, new_off = b.keep_inliers(rot, tran, huber_delta=delta, depth_mode=api.DEPTH_PER_MATCH)
        assert 0 < len(kept) < len(sq)
        q.upload(x1[kept], x2[kept], new_off, d[kept], store=store)
        _same_solve(b.solve_joint(rot, tran), q.solve_joint(rot, tran))


def test_errors(monkeypatch):
    cs = _solve_scenes()[:4]
    off, x1, x2, d12, rot0, tran0 = _cat(cs)
    lib = cabi.load_library()
    dp = lambda a: a.ctypes.data_as(cabi._dp)
    with api.Batch(0) as b:
        r, t = rot0.copy(), tran0.copy()                  # never uploaded
        eqs = (cabi.JointEq * 4)()
        assert lib.sba_batch_eval_joint(b._h, dp(r), dp(t), 1.0, None, eqs) == cabi.SBA_ERR_NOT_UPLOADED
        assert lib.sba_batch_solve_joint(b._h, dp(r), dp(t), None, None, None, None) == cabi.SBA_ERR_NOT_UPLOADED
        b.upload(x1, x2, off)                             # no per-match depths
        for call in (lambda: b.solve_joint(rot0, tran0), lambda: b.eval_joint(rot0, tran0)):
            with pytest.raises(api.SbaError) as ei:
                call()
            assert ei.value.code == cabi.SBA_ERR_UNSUPPORTED
        b.upload(x1, x2, off, d12)
        for radius in (0.0, -1.0, float("nan")):
            with pytest.raises(api.SbaError) as ei:
                b.eval_joint(rot0, tran0, radius)
            assert ei.value.code == cabi.SBA_ERR_INVALID_ARG
        r, t = rot0.copy(), tran0.copy()
        assert lib.sba_batch_solve_joint(b._h, None, dp(t), None, None, None, None) == cabi.SBA_ERR_INVALID_ARG
        assert lib.sba_batch_eval_joint(b._h, dp(r), dp(t), 1.0, None, None) == cabi.SBA_ERR_INVALID_ARG
        assert lib.sba_batch_eval_joint(None, dp(r), dp(t), 1.0, None, None) == cabi.SBA_ERR_INVALID_ARG
        good = b.solve_joint(rot0, tran0)
        # summaries, status and d12_out may be NULL
        b.set_depths(d12)
        assert lib.sba_batch_solve_joint(b._h, dp(r), dp(t), None, None, None, None) == cabi.SBA_OK
        assert np.array_equal(r, good[0]) and np.array_equal(t, good[1])
        # one pair with a NaN start: that pair fails with its depths, rot and tran unchanged, the call says so, the others are served
        for driver_env in (None, "0"):
            b.set_depths(d12)
            bad = rot0.copy(); bad[2, 1] = np.nan
            if driver_env is not None:
                monkeypatch.setenv("SBA_BATCH_DEVICE_JOINT", driver_env)
            with pytest.raises(api.SbaError) as ei:
                b.solve_joint(bad, tran0)
            assert ei.value.code == cabi.SBA_ERR_NUMERIC
            b.set_depths(d12)
            rot, tran, d, sums, status = b.solve_joint(bad, tran0, check=False)
            monkeypatch.delenv("SBA_BATCH_DEVICE_JOINT", raising=False)
            assert list(status) == [0, 0, cabi.SBA_ERR_NUMERIC, 0]
            lo, hi = int(off[2]), int(off[3])
            assert np.array_equal(d[lo:hi], d12[lo:hi]) and np.array_equal(rot[2], bad[2], equal_nan=True) and np.array_equal(tran[2], tran0[2])
            e_after = b.residuals(rot0, tran0, depth_mode=api.DEPTH_PER_MATCH, fields=("e",)).e
            for g in (0, 1, 3):
                l, h = int(off[g]), int(off[g + 1])
                assert np.array_equal(rot[g], good[0][g]) and np.array_equal(tran[g], good[1][g]) and np.array_equal(d[l:h], good[2][l:h])
                assert _counts(sums[g]) == _counts(good[3][g])
        with api.Batch(0) as q:                           # the bad pair's planes hold the uploaded depths
            q.upload(x1, x2, off, d12)
            e_fresh = q.residuals(rot0, tran0, depth_mode=api.DEPTH_PER_MATCH, fields=("e",)).e
        assert np.array_equal(e_after[lo:hi], e_fresh[lo:hi])
        # a NaN depth: the pair's first cost is not finite -- SBA_ERR_NUMERIC for it, depths as uploaded
        nan_d = d12.copy(); nan_d[int(off[1]) + 3, 0] = np.nan
        b.set_depths(nan_d)
        rot, tran, d, sums, status = b.solve_joint(rot0, tran0, check=False)
        assert list(status) == [0, cabi.SBA_ERR_NUMERIC, 0, 0]
        assert np.array_equal(d[int(off[1]):int(off[2])], nan_d[int(off[1]):int(off[2])], equal_nan=True)


def test_publish_off_is_refused(monkeypatch):
    cs = _solve_scenes()[:2]
    off, x1, x2, d12, rot0, tran0 = _cat(cs)
    monkeypatch.setenv("SBA_PUBLISH", "0")
    with api.Batch(0) as b:
        b.upload(x1, x2, off, d12)
        for call in (lambda: b.solve_joint(rot0, tran0), lambda: b.eval_joint(rot0, tran0)):
            with pytest.raises(api.SbaError) as ei:
                call()
            assert ei.value.code == cabi.SBA_ERR_UNSUPPORTED


def test_empty_pairs():
    cs = [_scene(0, seed=50), _scene(300, 0), _scene(0, seed=51)]
    off, x1, x2, d12, rot0, tran0 = _cat(cs)
    with api.Batch(0) as b:
        b.upload(x1, x2, off, d12)
        rot, tran, d, sums, status = b.solve_joint(rot0, tran0)
        assert not status.any()
        for g in (0, 2):
            assert sums[g].termination == "CONVERGENCE_GRADIENT" and sums[g].num_evaluations == 1 and sums[g].num_iterations == 0
            assert np.array_equal(rot[g], rot0[g]) and np.array_equal(tran[g], tran0[g])
        assert sums[1].num_successful_steps >= 1

def test_gauge():
    cs = [_scene(2000, seed=60 + i, outlier_fraction=0.0) for i in range(4)]
    off, x1, x2, d12, rot0, tran0 = _cat(cs)
    with api.Batch(0) as b:
        b.upload(x1, x2, off, d12)
        rot, tran, d, sums, status = b.solve_joint(rot0, tran0)              # default: |tran| pinned per pair
        n0 = np.linalg.norm(tran0, axis=1)
        assert (np.abs(np.linalg.norm(tran, axis=1) - n0) <= 1e-12 * n0).all()
        assert all(s.final_cost < s.initial_cost for s in sums)
        b.set_depths(d12)
        rot, tran, d, sums, status = b.solve_joint(rot0, tran0, options=api.default_lm_options(tran_param=api.TRAN_FREE))
        assert not status.any() and all(s.final_cost < s.initial_cost for s in sums)
        assert (np.linalg.norm(tran, axis=1) < n0).all()                     # the functor as written: (d, t) shrink together


def test_pipeline_keyword():
    sizes = [4096, 3000, 2500, 4097]
    cs = [synthetic.full_rt(n, seed=synthetic.BASE_SEED + 9 + i, sigma=2e-4, outlier_fraction=0.02) for i, n in enumerate(sizes)]
    off, x1, x2, _, _, _ = _cat(cs)
    start = np.full((int(off[-1]), 2), 6.0)
    with api.Batch(0) as b:
        b.upload(x1, x2, off, start)
        plain = b.solve_problem(want_depths=True)
        b.set_depths(start)
        again = b.solve_problem(want_depths=True, joint=False)
        assert set(plain) == set(again) and not any(k.startswith("joint") for k in plain)
        for k in ("rot", "tran", "d_uniform", "guess_candidates", "status", "d12"):
            assert np.array_equal(plain[k], again[k]), k
        staged = b.eval_joint(plain["rot"], plain["tran"])                  # at the staged result, on the refined depths
        manual = b.solve_joint(plain["rot"], plain["tran"])
        b.set_depths(start)
        full = b.solve_problem(want_depths=True, joint=True)
        for k in ("rot", "tran", "d_uniform", "guess_candidates", "status", "d12"):
            assert np.array_equal(plain[k], full[k]), k
        _same_solve(manual, (full["joint_rot"], full["joint_tran"], full["joint_d12"], full["joint_stage"], full["joint_status"]))
        for g, s in enumerate(full["joint_stage"]):
            assert s.initial_cost == staged[g].cost and s.final_cost <= s.initial_cost, g
            print(f"pair {g}: staged cost {staged[g].cost:.6e} -> joint {s.final_cost:.6e} ({s.termination}, {s.num_iterations} iterations)")


def test_full_size():
    """Config C5: 256 pairs x 50 000 matches, per-match f64."""
    B, n = 256, 50_000
    c = synthetic.full_rt(B * n, seed=synthetic.BASE_SEED + 5, depth_noise=0.02)
    off = (np.arange(B + 1) * n).astype(np.uint64)
    rot0 = np.tile(c.rot_init, (B, 1)); tran0 = np.tile(c.tran_init, (B, 1))
    with api.Batch(0) as b:
        b.upload(c.x1, c.x2, off, c.d12)
        b.solve_joint(rot0, tran0, return_depths=False)                     # first call: allocations
        b.set_depths(c.d12)
        t0 = time.perf_counter()
        rot, tran, _, sums, status = b.solve_joint(rot0, tran0, return_depths=False)
        wall = time.perf_counter() - t0
        b.set_depths(c.d12)
        _, _, d, _, _ = b.solve_joint(rot0, tran0)
    assert not status.any()
    assert all(s.final_cost <= s.initial_cost for s in sums)
    assert np.isfinite(d).all() and np.isfinite(rot).all() and np.isfinite(tran).all()
    its = [s.num_iterations for s in sums]
    print(f"C5 joint solve: {wall * 1e3:.2f} ms wall for {B} x {n}; iterations per pair {min(its)}..{max(its)}, "
          f"passes {min(s.num_evaluations for s in sums)}..{max(s.num_evaluations for s in sums)}")
