"""GPU: the two-view kernels on the matches no seeded scene draws (tests/match_edges.py): parallel and nearly parallel rays, zero,
tiny, huge and negative depths, axis bearings, negative zeros, non-unit lengths, and residuals on delta^2 and one ulp from it.

References, measures and bounds are tests/match_edges_reference.py's: long-double numpy, errors of sums relative to the sum of the
absolute per-match terms, per kind 8 times what float64 numpy itself does there (TABLE, reproduced on the CPU by
tests/test_match_edges_cpu.py), and the flat bounds the project states already wherever float64 meets them.  The exact scene is
compared as bytes with integer arithmetic.  Where float64 and long double both divide by an exactly zero determinant (TABLE's
non_finite) the kernels must give non-finite reduced outputs, the solvers an invalid step and a halved radius, and the handle must
afterwards answer as a fresh one."""
from functools import lru_cache

import numpy as np
import pytest

import handle_ops as ops
import match_edges as me
import match_edges_reference as mr
import pose_edges as pe
from helpers import REL_TOL_F64
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

pytestmark = pytest.mark.gpu

STORES = (api.STORE_F64, api.STORE_F32)
LAYOUTS = ("0", "1")                                   # SBA_BATCH_INTERLEAVE
KERNELS = (api.KERNEL_FACTORED, api.KERNEL_EXPLICIT)
DRIVERS = ((513, None), (513, "0"), (4099, None))      # (n, SBA_SMALL_ONE_LAUNCH): one launch, the resident session, the launch path
SMALL = ((513, None), (513, "0"))
SLOTS = {api.MODE_ROT: [0, 1, 2, 3, 4, 5, 16, 17, 18, 22], api.MODE_TRAN: [15, 19, 20, 21, 22], api.MODE_RT: list(range(23))}
KINDS = mr.table_kinds()
stores = pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
kinds = pytest.mark.parametrize("kind", KINDS)
layouts = pytest.mark.parametrize("layout", LAYOUTS, ids=["contiguous", "interleaved"])


def _f32(store):
    return store == api.STORE_F32


def _driver(monkeypatch, one):
    if one is None:
        monkeypatch.delenv("SBA_SMALL_ONE_LAUNCH", raising=False)
    else:
        monkeypatch.setenv("SBA_SMALL_ONE_LAUNCH", one)


def _open(c, store):
    p = api.Problem(0)
    p.upload(c.x1, c.x2, c.d12, store=store)
    return p


def _term(code):
    return cabi.TERMINATION[code]


@lru_cache(maxsize=None)
def _sweep_ref(key, mode, dm, delta):
    """Computed once, shared by the kernel kinds and the drivers, left unchanged."""
    c, _ = mr.qualified(*key)
    s, a = mr.sweep_reference(c, key[4], mode, dm, delta)
    return s["pack"], a["pack"]


@lru_cache(maxsize=None)
def _joint_ref(key, radius, delta=1.0):
    c, _ = mr.qualified(*key)
    return mr.joint_reference(c, key[4], radius, delta)


@lru_cache(maxsize=None)
def _residual_ref(key):
    c, _ = mr.qualified(*key)
    return mr.residual_reference(c, key[4])


@lru_cache(maxsize=None)
def _nout(key):
    c, _ = mr.qualified(*key)
    return float(mr.classes(c, key[4], 1.0, mr.LD)[1].sum())


def _row_bounds(c, kind, pas):
    """Per row: the kind's bound on its edge rows, the ordinary bound elsewhere."""
    b = np.full(len(c.x1), mr.bound("ordinary", pas)[0])
    b[c.rows] = mr.bound(kind, pas)[0]
    return b


def _check_pack(pack, key, mode, dm, delta, kind, what):
    """-> err / bound of one pack in the abs-sum measure; the flat bound where float64 meets it; the outlier count."""
    ref, ab = _sweep_ref(key, mode, dm, delta)
    sl = SLOTS[mode]
    b_abs, b_flat = mr.bound(kind, "sweep")
    err = mr.sum_errors(pack[sl], ref[sl], ab[sl])
    assert err <= b_abs, (what, err, b_abs)
    if b_flat is not None:
        flat = mr.flat_error(pack[sl], ref[sl])
        assert flat <= b_flat, (what, flat, b_flat)
    assert pack[23] == float(ref[23]), (what, pack[23], float(ref[23]))
    return err / b_abs


def _check_joint(got, key, radius, kind, pas, what):
    """One reduce pass against joint_reference by TABLE's entry -> err / bound."""
    c, _ = mr.qualified(*key)
    ref, ab, gd_max, singular = _joint_ref(key, radius)
    cls = mr.TABLE[kind, pas][0]
    b_abs, b_flat = mr.bound(kind, pas)
    out = dict(S=got.S, gs=got.gs, V=got.V, gc=got.gc, cost=got.cost, sum_w=got.sum_w)
    keys = mr.JOINT_KEYS
    if cls == "non_finite":
        assert singular, what
        for k in mr.REDUCED:                      # non-finite wherever the reference is, not finite garbage
            bad = ~np.isfinite(ref[k].astype(np.float64))
            assert bad.any() and not np.isfinite(out[k][bad]).any(), (what, k, out[k])
        keys = ("V", "gc", "cost", "sum_w")
    else:
        assert not singular, what
        assert np.array_equal(got.S, got.S.T), what
    err, flat = mr.joint_errors(out, ref, ab, keys)
    assert err <= b_abs, (what, err, b_abs)
    if b_flat is not None:
        assert flat <= b_flat, (what, flat, b_flat)
    assert got.n_outlier == _nout(key), what
    assert abs(got.gd_max - gd_max) <= max(b_abs, REL_TOL_F64) * max(gd_max, 1.0), (what, got.gd_max, gd_max)
    return err / b_abs


HISTORY_PROBES = ("eval_pack[rt,per-match,factored,huber=1]", "eval_pack[rt,per-match,explicit,huber=1]", "residuals", "eval_joint",
                  "covariance_joint", "structure_joint", "solve[rt]")


def _as_ops_scene(c, store):
    n = len(c.x1)
    rng = np.random.default_rng(n)
    return ops.ProblemScene(n, 0, store, c.x1, c.x2, c.d12, c.rot_init, c.tran_init, c.rot_true, c.tran_true, c.d12, np.ones(n, dtype=bool),
                            rng.integers(0, n, size=(8, 16)).astype(np.int32), np.tile(c.rot_init, (16, 1)), np.tile(c.tran_init, (16, 1)))


def _same_as_fresh(p, c, store, what):
    """The handle answers the probes of tests/handle_ops.py as a fresh handle on the same scene does, byte for byte."""
    s = _as_ops_scene(c, store)
    table = {op.name: op for op in ops.PROBLEM_OPS}
    with ops.open_problem(s) as fresh:
        for name in HISTORY_PROBES:
            assert table[name](p, s) == table[name](fresh, s), (what, name)


# ==== sweeps and residuals ========================================================================================================
@stores
@kinds
def test_sweeps_and_residuals(monkeypatch, kind, store):
    """eval_pack in three modes, both kernel kinds, both depth modes, delta = 1 and 0, and residuals, on every scene of the kind:
    packs within the kind's bound, n_outlier the reference's count, the residual flags summing to the pack's NOUT, rows within the
    per-row bound."""
    worst = 0.0
    for pose in me.POSES:
        for n, one in DRIVERS:
            _driver(monkeypatch, one)
            for rep in range(me.REPEAT):
                key = (kind, pose, n, rep, _f32(store))
                c, _ = mr.qualified(*key)
                what = f"{c.name} store={store} one_launch={one}"
                out_ref = mr.classes(c, key[4], 1.0, mr.LD)[1]
                with _open(c, store) as p:
                    r = p.residuals(c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH)
                    err = mr.residual_errors(r.e, r.sq_norm, c, key[4], _residual_ref(key))
                    bounds = _row_bounds(c, kind, "residuals")
                    assert (err <= bounds).all(), (what, np.flatnonzero(err > bounds), err.max())
                    worst = max(worst, float((err / bounds).max()))
                    assert np.array_equal(r.inlier, ~out_ref) and r.n_inlier == int((~out_ref).sum()), what
                    for kern in KERNELS:
                        p.set_kernel(kern)
                        for mode in mr.MODES:
                            for dm in (api.DEPTH_UNIFORM, api.DEPTH_PER_MATCH):
                                for delta in mr.DELTAS:
                                    pack = p.eval_pack(mode, c.rot_init, c.tran_init, *mr.UNIFORM, huber_delta=delta, depth_mode=dm)
                                    worst = max(worst, _check_pack(pack, key, mode, dm, delta, kind, f"{what} kernel={kern} mode={mode} depth={dm} delta={delta}"))
                                    if dm == api.DEPTH_PER_MATCH and delta == 1.0:
                                        assert n - r.n_inlier == pack[23], what
    print(f"largest err / bound {kind} store={store}: {worst:.3g}")


# ==== the exact scene =============================================================================================================
def _exact_checks(res, pack_of, joint_nout, c, names, delta):
    e, _, out, _ = me.exact_terms(c, delta)
    ref_e = np.array([[float(v) for v in row] for row in e])
    assert np.array_equal(res.e, ref_e), "e differs from integer arithmetic"
    assert np.array_equal(res.inlier, ~out)
    assert res.inlier[names["at_delta"]].all() and res.inlier[names["at_delta_-1ulp"]].all() and res.inlier[names["zero"]].all()
    assert not res.inlier[names["at_delta_+1ulp"]].any()
    assert res.sq_norm[names["at_delta"]].tolist() == [delta * delta] * len(names["at_delta"])
    assert res.sq_norm[names["at_delta_+1ulp"]].tolist() == [float(np.nextafter(delta * delta, 1.0))] * len(names["at_delta_+1ulp"])
    assert res.sq_norm[names["at_delta_-1ulp"]].tolist() == [float(np.nextafter(delta * delta, 0.0))] * len(names["at_delta_-1ulp"])
    assert not res.sq_norm[names["zero"]].any() and not res.e[names["zero"]].any()
    nout = float(out.sum())
    for what, pack in pack_of.items():
        assert pack[23] == nout, (what, pack[23], nout)
    assert joint_nout == nout, (joint_nout, nout)


@stores
@pytest.mark.parametrize("n,one", DRIVERS, ids=["one-launch", "resident", "launch"])
def test_exact_scene(monkeypatch, n, one, store):
    """rot = 0, axis bearings, dyadic depths, t and delta = 0.75.  Every e, every flag and the count of outliers of every path --
    residual_kernel, the factored and the explicit sweep in three modes, joint_block through eval_joint -- equal integer
    arithmetic: s == delta^2 is an inlier, one ulp above it an outlier.  With the loss off, every entry of the three modes' packs
    and of eval_joint's unreduced block is the exact sum, byte for byte, whatever the order of the reduction."""
    _driver(monkeypatch, one)
    delta = me.EXACT_DELTA
    c, names = me.exact_scene(n)
    opt = api.default_lm_options(tran_param=api.TRAN_SPHERE, huber_delta=delta)
    with _open(c, store) as p:
        res = p.residuals(c.rot_init, c.tran_init, huber_delta=delta, depth_mode=api.DEPTH_PER_MATCH)
        packs = {}
        for kern in KERNELS:
            p.set_kernel(kern)
            for mode in mr.MODES:
                packs[kern, mode] = p.eval_pack(mode, c.rot_init, c.tran_init, huber_delta=delta, depth_mode=api.DEPTH_PER_MATCH)
        eq = p.eval_joint(c.rot_init, c.tran_init, 1e4, opt)
    _exact_checks(res, packs, eq.n_outlier, c, names, delta)

    c, _ = me.exact_scene(n, ulp_rows=False)
    _, _, _, exact = me.exact_terms(c, 0.0)
    off = api.default_lm_options(tran_param=api.TRAN_SPHERE, huber_delta=0.0)
    with _open(c, store) as p:
        for kern in KERNELS:
            p.set_kernel(kern)
            for mode in mr.MODES:
                pack = p.eval_pack(mode, c.rot_init, c.tran_init, huber_delta=0.0, depth_mode=api.DEPTH_PER_MATCH)
                want = me.exact_floats(exact[mode])
                sl = SLOTS[mode] + [23]
                assert np.array_equal(pack[sl], want[sl]), (kern, mode, pack[sl] - want[sl])
        eq = p.eval_joint(c.rot_init, c.tran_init, 1e4, off)
        ne = api.expand_pack(api.MODE_RT, me.exact_floats(exact[api.MODE_RT]))
        assert np.array_equal(eq.V, ne.H) and np.array_equal(eq.gc, ne.g) and eq.cost == ne.cost and eq.sum_w == float(n)


@layouts
@stores
def test_exact_scene_batched(monkeypatch, store, layout):
    """The two batched forms (Batch.eval / Batch.residuals, Batch.eval_joint) on exact scenes of 257, 513 and 1025 matches: the
    same flags, counts and, with the loss off, bytes."""
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    delta = me.EXACT_DELTA
    for ulp_rows in (True, False):
        cs = [me.exact_scene(n, ulp_rows) for n in (257, 513, 1025)]
        off, x1, x2, d12, rot, tran = pe.cat([c for c, _ in cs])
        d = delta if ulp_rows else 0.0
        opt = api.default_lm_options(tran_param=api.TRAN_SPHERE, huber_delta=d)
        with api.Batch(0) as b:
            b.upload(x1, x2, off, d12, store=store)
            res = b.residuals(rot, tran, huber_delta=d, depth_mode=api.DEPTH_PER_MATCH)
            packs = {}
            for kern in KERNELS:
                b.set_kernel(kern)
                for mode in mr.MODES:
                    packs[kern, mode] = b.eval(mode, rot, tran, huber_delta=d, depth_mode=api.DEPTH_PER_MATCH)
            eqs = b.eval_joint(rot, tran, 1e4, opt)
        for g, (c, names) in enumerate(cs):
            lo, hi = int(off[g]), int(off[g + 1])
            if ulp_rows:
                one = api.Residuals(res.e[lo:hi], res.sq_norm[lo:hi], res.inlier[lo:hi], int(res.n_inlier[g]))
                _exact_checks(one, {k: v[g] for k, v in packs.items()}, eqs[g].n_outlier, c, names, delta)
            else:
                _, _, _, exact = me.exact_terms(c, 0.0)
                for (kern, mode), pk in packs.items():
                    sl = SLOTS[mode] + [23]
                    assert np.array_equal(pk[g][sl], me.exact_floats(exact[mode])[sl]), (g, kern, mode)
                ne = api.expand_pack(api.MODE_RT, me.exact_floats(exact[api.MODE_RT]))
                assert np.array_equal(eqs[g].V, ne.H) and np.array_equal(eqs[g].gc, ne.g) and eqs[g].cost == ne.cost


# ==== the joint pass ==============================================================================================================
@stores
@kinds
def test_eval_joint(monkeypatch, kind, store):
    """eval_joint at RADII (inf among them) on every scene of the kind by TABLE's entry: the bound, or -- exactly parallel rays
    with no damping -- non-finite S and gs, V, gc, cost and sum_w still within the bound, and a handle that then answers as a
    fresh one."""
    worst = 0.0
    for pas, radii in (("eval_joint", mr.RADII[1:]), ("eval_joint_inf", mr.RADII[:1])):
        for pose in mr.entry_poses(kind, pas):
            for n, one in DRIVERS:
                _driver(monkeypatch, one)
                for rep in range(me.REPEAT):
                    key = (kind, pose, n, rep, _f32(store))
                    c, _ = mr.qualified(*key)
                    with _open(c, store) as p:
                        for radius in radii:
                            what = f"{c.name} store={store} one_launch={one} radius={radius:g}"
                            worst = max(worst, _check_joint(p.eval_joint(c.rot_init, c.tran_init, radius), key, radius, kind, pas, what))
                        if mr.TABLE[kind, pas][0] == "non_finite":
                            _same_as_fresh(p, c, store, what)
    print(f"largest err / bound {kind} store={store}: {worst:.3g}")


# ==== the d-only stage ============================================================================================================
def _depth_opt(iterations, radius=None):
    kw = dict(max_num_iterations=iterations)
    if radius is not None:
        kw.update(initial_trust_region_radius=radius, max_trust_region_radius=max(radius, 1e16))
    return api.default_lm_options(**kw)


def _summary5(s):
    return (s.termination, s.num_iterations, s.num_successful_steps, s.num_evaluations, s.num_line_search_steps)


def _ref5(t):
    return (_term(t[0]),) + tuple(t[1:])


@stores
@kinds
def test_solve_depths(monkeypatch, kind, store):
    """solve_depths with 1 and 3 iterations through both small-problem drivers: the summary of the long-double run of the product's
    own step logic, every row's depths within the kind's bound of it."""
    worst = 0.0
    for pose in me.POSES:
        for n, one in SMALL:
            _driver(monkeypatch, one)
            for rep in range(me.REPEAT):
                key = (kind, pose, n, rep, _f32(store))
                c, dropped = mr.qualified(*key)
                bounds = _row_bounds(c, kind, "depth")
                for it in mr.DEPTH_ITERATIONS:
                    ref_d, ref_s, _, _ = mr.depth_solve(*key, it, True, revert=tuple(sorted(dropped)))
                    with _open(c, store) as p:
                        d, s = p.solve_depths(c.rot_init, c.tran_init, options=_depth_opt(it))
                    what = f"{c.name} store={store} one_launch={one} iterations={it}"
                    assert _summary5(s) == _ref5(ref_s), (what, _summary5(s), ref_s)
                    err = mr.depth_row_errors(d, ref_d)
                    assert (err <= bounds).all(), (what, np.flatnonzero(err > bounds), err.max())
                    worst = max(worst, float((err / bounds).max()))
    print(f"largest err / bound {kind} store={store}: {worst:.3g}")


@stores
@kinds
def test_solve_depths_from_the_singular_radius(monkeypatch, kind, store):
    """One iteration from radius 1e16.  far_parallel (TABLE: non_finite, at rot = 0): the regularisers have underflowed, the damping
    is below half an ulp of the block, the determinant is exactly zero and the step NaN.  That step is invalid: one iteration,
    no successful step, two passes, the radius halved, and the depths returned are the depths given -- none is 0 because
    fmax(NaN, 0) is 0.  Three iterations then move on from the halved radius: the summary and every row's
    depths equal those of the float64 run of the step logic whose passes round every determinant once, within 8 times what float64
    formulations of the step's numerators differ by among themselves there (TABLE's figure: 4.8e-7 of a depth, the size of the
    step along d2 - d1, because at radius 5e15 the numerators are differences of products that agree to an ulp), no edge
    row's depth collapses to 0, and the handle answers afterwards as a fresh one.  Every other kind: the bound."""
    cls = mr.TABLE[kind, "depth_1e16"][0]
    worst = 0.0
    for pose in mr.entry_poses(kind, "depth_1e16"):
        for n, one in SMALL:
            _driver(monkeypatch, one)
            for rep in range(me.REPEAT):
                key = (kind, pose, n, rep, _f32(store))
                c, dropped = mr.qualified(*key)
                rv = tuple(sorted(dropped))
                what = f"{c.name} store={store} one_launch={one}"
                f64 = mr.depth_solve(*key, 1, False, mr.SINGULAR_RADIUS, rv, accurate_det=True)
                with _open(c, store) as p:
                    d, s = p.solve_depths(c.rot_init, c.tran_init, options=_depth_opt(1, mr.SINGULAR_RADIUS))
                    assert _summary5(s) == _ref5(f64[1]), (what, _summary5(s), f64[1])
                    if cls == "non_finite":
                        assert f64[3], what
                        assert d.tobytes() == c.d12.tobytes(), (what, np.flatnonzero((d != c.d12).any(axis=1)))
                        assert s.final_radius == mr.SINGULAR_RADIUS / 2 and s.final_cost == s.initial_cost, what
                        # the next steps, from the halved radius, against the float64 run with exactly rounded determinants
                        ref3 = mr.depth_solve(*key, 3, False, mr.SINGULAR_RADIUS, rv, accurate_det=True)
                        d3, s3 = p.solve_depths(c.rot_init, c.tran_init, options=_depth_opt(3, mr.SINGULAR_RADIUS))
                        assert _summary5(s3) == _ref5(ref3[1]) and ref3[1][2] >= 1, (what, _summary5(s3), ref3[1])
                        err, bounds = mr.depth_row_errors(d3, ref3[0]), _row_bounds(c, kind, "depth_1e16")
                        assert (err <= bounds).all(), (what, "three iterations", np.flatnonzero(err > bounds), err.max())
                        worst = max(worst, float((err / bounds).max()))
                        assert np.isfinite(d3).all() and (d3[c.rows] > 0.5 * c.d12[c.rows]).all(), what
                        assert s3.termination != "FAILURE" and s3.final_cost <= s3.initial_cost, (what, s3)
                        p.set_depths(c.d12)
                        _same_as_fresh(p, c, store, what)
                        # the same without the axis row: every singular block's determinant is a * a - a * a with an inexact a * a
                        plain = me.scene(kind, pose, n, rep, axis_row=False)
                        ref = mr.depth_solve(*key, 1, False, mr.SINGULAR_RADIUS, axis_row=False, accurate_det=True)
                        assert ref[3] and ref[1] == (4, 1, 0, 2, 0), (what, ref[1:])
                        with _open(plain, store) as q:
                            d, s = q.solve_depths(c.rot_init, c.tran_init, options=_depth_opt(1, mr.SINGULAR_RADIUS))
                        assert _summary5(s) == _ref5(ref[1]) and d.tobytes() == plain.d12.tobytes(), (what, "no axis row", _summary5(s))
                    else:
                        assert not f64[3], what
                        ref_d = mr.depth_solve(*key, 1, True, mr.SINGULAR_RADIUS, rv)[0]
                        err, bounds = mr.depth_row_errors(d, ref_d), _row_bounds(c, kind, "depth_1e16")
                        assert (err <= bounds).all(), (what, np.flatnonzero(err > bounds), err.max())
                        worst = max(worst, float((err / bounds).max()))
    print(f"largest err / bound {kind} store={store}: {worst:.3g}")


# ==== the joint solve =============================================================================================================
def _joint_opt(radius=None, iterations=None):
    kw = dict(tran_param=api.TRAN_SPHERE)
    if radius is not None:
        kw.update(initial_trust_region_radius=radius, max_trust_region_radius=max(radius, 1e16))
    if iterations is not None:
        kw.update(max_num_iterations=iterations)
    return api.default_lm_options(**kw)


def _counts(s):
    return (s.termination, s.num_iterations, s.num_successful_steps, s.num_evaluations)


@stores
@kinds
def test_solve_joint(kind, store):
    """solve_joint to termination against rj.dense_solve and the product's step logic over numpy passes, on the scenes that are a
    fair yardstick (match_edges_reference.fair_yardstick: the two agree, no test on its threshold, the run converged): the same
    termination and counts, rot, tran and the depths within the kind's bound of both."""
    worst, fair = 0.0, 0
    b = mr.bound(kind, "solve_joint")[0]
    for key in mr.joint_combos(kind, "solve_joint"):
        if key[4] != _f32(store):
            continue
        c, dropped = mr.qualified(*key)
        emu, dense = mr.joint_solve(*key, revert=tuple(sorted(dropped)))
        if not mr.fair_yardstick(emu, dense):
            continue
        fair += 1
        with _open(c, store) as p:
            rot, tran, d, s = p.solve_joint(c.rot_init, c.tran_init)
        assert _counts(s) == (_term(emu[3][0]),) + emu[3][1:], (c.name, _counts(s), emu[3])
        for ref in (emu, dense):
            err = mr.joint_solve_errors((rot, tran, d), ref)
            worst = max(worst, err / b)
            assert err <= b, (c.name, err, b)
        assert s.final_cost <= s.initial_cost
    assert 2 * fair >= len(mr.joint_combos(kind, "solve_joint")) // 2, (kind, fair)      # at least half of the store's scenes
    print(f"largest err / bound {kind} store={store}: {worst:.3g} over {fair} scenes")


@stores
@kinds
def test_solve_joint_from_the_singular_radius(kind, store):
    """One iteration from radius 1e16.  Exactly parallel rays at rot = 0 (TABLE: non_finite): fma(D, 1 / radius, H) == H, the
    determinant of the depth block is exactly 0, the reduced system is not finite, the Cholesky factorisation fails and the step
    is invalid -- one iteration, no successful step, two passes, the radius halved, rot, tran and the depths unchanged to the byte;
    the handle then answers as a fresh one.  The whole solve from there ends as the step logic over numpy passes ends (FAILURE
    only if that does), with its counts where the dense restatement and the passes with exactly rounded determinants have the
    same: after the invalid step the radius is 5e15, a parallel match's block has a determinant of 1e-16 of its terms, and float64
    formulations differ among themselves in what they accept from there.  Every other kind: counts and the bound."""
    cls = mr.TABLE[kind, "solve_joint_1e16"][0]
    b = mr.bound(kind, "solve_joint_1e16")[0]
    worst, fair = 0.0, 0
    for key in mr.joint_combos(kind, "solve_joint_1e16"):
        if key[4] != _f32(store):
            continue
        c, dropped = mr.qualified(*key)
        rv = tuple(sorted(dropped))
        emu, dense = mr.joint_solve(*key, mr.SINGULAR_RADIUS, 1, rv)
        with _open(c, store) as p:
            eq = p.eval_joint(c.rot_init, c.tran_init, mr.SINGULAR_RADIUS)
            rot, tran, d, s = p.solve_joint(c.rot_init, c.tran_init, _joint_opt(mr.SINGULAR_RADIUS, 1))
            assert _counts(s) == (_term(emu[3][0]),) + emu[3][1:], (c.name, _counts(s), emu[3])
            if cls == "non_finite":
                assert not np.isfinite(eq.S).any() and not np.isfinite(eq.gs).any(), (c.name, eq.S)
                assert np.isfinite(eq.V).all() and np.isfinite(eq.gc).all()
                assert rot.tobytes() == c.rot_init.tobytes() and tran.tobytes() == c.tran_init.tobytes() and d.tobytes() == c.d12.tobytes(), c.name
                assert s.final_radius == mr.SINGULAR_RADIUS / 2 and s.final_cost == s.initial_cost, (c.name, s)
                full_emu, full_dense = mr.joint_solve(*key, mr.SINGULAR_RADIUS, 50, rv)
                _, _, d2, s2 = p.solve_joint(c.rot_init, c.tran_init, _joint_opt(mr.SINGULAR_RADIUS))
                print(f"{c.name} store={store}: {_counts(s2)}, numpy passes {full_emu[3]}, dense {mr.counts_of_dense(full_dense[3])}")
                assert s2.termination == _term(full_emu[3][0]), (c.name, _counts(s2), full_emu[3])
                assert np.isfinite(d2).all() and s2.final_cost <= s2.initial_cost
                if mr.singular_solve_is_fair(key, rv):     # three float64 formulations agree: a fair yardstick
                    fair += 1
                    assert _counts(s2) == (_term(full_emu[3][0]),) + full_emu[3][1:], (c.name, _counts(s2), full_emu[3])
                p.set_depths(c.d12)
                _same_as_fresh(p, c, store, c.name)
            else:
                assert np.isfinite(eq.S).all()
                for ref in (emu, dense):
                    err = mr.joint_solve_errors((rot, tran, d), ref)
                    worst = max(worst, err / b)
                    assert err <= b, (c.name, err, b)
    if cls == "non_finite":
        assert fair >= mr.SINGULAR_FAIR_MIN[kind], (kind, fair)       # the counts were really demanded (asserted on the CPU too)
    print(f"largest err / bound {kind} store={store}: {worst:.3g}")


# ==== covariance and structure ====================================================================================================
@lru_cache(maxsize=None)
def _cov_ref(key):
    c, _ = mr.qualified(*key)
    return mr.cov_structure_reference(c, key[4])


def _check_cov_structure(cov, depth_cov, xyz, scov, score, key, kind, what):
    """The rows min_sin2_parallax leaves out reported as such, the rows kept and the pose block within the kind's bounds of the
    long-double Schur forms -> the largest err / bound."""
    c, _ = mr.qualified(*key)
    keep, cv, st = _cov_ref(key)
    out = ~keep
    assert np.array_equal(depth_cov[out], np.tile([np.inf, np.inf, 0.0], (int(out.sum()), 1))), what
    assert np.isinf(score[out]).all() and np.isinf(scov[out][:, :3]).all() and np.isfinite(xyz).all(), what
    ep, ed = mr.cov_errors(cov, depth_cov[keep], cv)
    es = mr.structure_errors(xyz[keep], scov[keep], score[keep], st)
    edge = np.isin(np.flatnonzero(keep), c.rows)
    worst = ep / mr.pose_bound(kind)
    assert ep <= mr.pose_bound(kind), (what, "pose block", ep, mr.pose_bound(kind))
    for pas, err in (("covariance", ed), ("structure", es)):
        bounds = np.where(edge, mr.bound(kind, pas)[0], mr.bound("ordinary", pas)[0])
        assert (err <= bounds).all(), (what, pas, np.flatnonzero(keep)[err > bounds][:5], float(np.nanmax(err)))
        worst = max(worst, float((err / bounds).max()))
    return worst


@stores
@kinds
def test_covariance_and_structure(monkeypatch, kind, store):
    """covariance_joint and structure_joint with min_sin2_parallax = 1e-9 on every scene of the kind: the rows at or below the cut
    are counted exactly and reported as (inf, inf, 0) / an infinite score, the rows kept (depth blocks; landmark, covariance,
    score) and the pose block are within the kind's bounds of the long-double Schur forms, and structure_joint's pose record is
    covariance_joint's."""
    worst = 0.0
    for pose in me.POSES:
        for n, one in DRIVERS:
            _driver(monkeypatch, one)
            for rep in range(mr.COV_REPEAT):
                key = (kind, pose, n, rep, _f32(store))
                c, _ = mr.qualified(*key)
                out = ~_cov_ref(key)[0]
                with _open(c, store) as p:
                    cv = p.covariance_joint(c.rot_init, c.tran_init, min_sin2_parallax=mr.COV_CUT)
                    st = p.structure_joint(c.rot_init, c.tran_init, min_sin2_parallax=mr.COV_CUT)
                    cv0 = p.covariance_joint(c.rot_init, c.tran_init, min_sin2_parallax=mr.COV_CUT, depths=False)
                assert (cv.n_degenerate, cv.n_used) == (int(out.sum()), n - int(out.sum())), (c.name, cv.n_degenerate, int(out.sum()))
                assert np.array_equal(cv.cov, cv.cov.T), c.name
                assert (st.pose.n_degenerate, st.pose.n_used) == (cv.n_degenerate, cv.n_used) and st.pose.cov.tobytes() == cv0.cov.tobytes(), c.name
                worst = max(worst, _check_cov_structure(cv.cov, cv.depth_cov, st.xyz, st.cov, st.score, key, kind, f"{c.name} store={store} one_launch={one}"))
    print(f"largest err / bound {kind} store={store}: {worst:.3g}")


# ==== the batch ===================================================================================================================
def _batch_scenes(kind, rep, store):
    """me.batch with the edge pairs' dropped rows reverted."""
    return [mr.qualified(c.kind, c.pose, len(c.x1), rep, _f32(store))[0] if g in me.BATCH_EDGE_PAIRS else c for g, c in enumerate(me.batch(kind, rep))]


def _batch(b, kind, rep, store):
    cs = _batch_scenes(kind, rep, store)
    off, x1, x2, d12, rot, tran = pe.cat(cs)
    b.upload(x1, x2, off, d12, store=store)
    return cs, off, rot, tran


def _batch_calls(b, rot, tran):
    """Every batched entry point this file covers, in one order; the mutators last, each from the uploaded depths."""
    out = dict(res=b.residuals(rot, tran, depth_mode=api.DEPTH_PER_MATCH))
    for kern in KERNELS:
        b.set_kernel(kern)
        out["eval", kern] = b.eval(api.MODE_RT, rot, tran, huber_delta=1.0, depth_mode=api.DEPTH_PER_MATCH)
    b.set_kernel(api.KERNEL_FACTORED)
    out["joint"] = {radius: b.eval_joint(rot, tran, radius) for radius in mr.RADII}
    out["cov"] = b.covariance_joint(rot, tran, min_sin2_parallax=1e-9, check=False)
    out["structure"] = b.structure_joint(rot, tran, min_sin2_parallax=1e-9, check=False)
    return out


@layouts
@stores
@kinds
def test_batch(monkeypatch, kind, store, layout):
    """The batch (257, 513, 0, 65, 1025) with the kind's rows in pairs 1 and 3 and ordinary neighbours: residuals, eval and
    eval_joint of pairs 1 and 3 within the single problem's bounds of the same references; covariance_joint and structure_joint
    count the rows below min_sin2_parallax exactly and keep the others within the kind's bounds; and the ordinary pairs give, byte for byte, what they give in the same batch
    with ordinary rows in pairs 1 and 3 -- a pair does not see its neighbour's edge rows."""
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    f32 = _f32(store)
    with api.Batch(0) as b:
        cs, off, rot, tran = _batch(b, kind, 0, store)
        got = _batch_calls(b, rot, tran)
    with api.Batch(0) as b:
        _, _, rot0, tran0 = _batch(b, "ordinary", 0, store)
        plain = _batch_calls(b, rot0, tran0)
    worst = 0.0
    for g, c in enumerate(cs):
        lo, hi = int(off[g]), int(off[g + 1])
        n = hi - lo
        if g not in me.BATCH_EDGE_PAIRS:
            assert got["res"].e[lo:hi].tobytes() == plain["res"].e[lo:hi].tobytes() and got["res"].n_inlier[g] == plain["res"].n_inlier[g], g
            for kern in KERNELS:
                assert got["eval", kern][g].tobytes() == plain["eval", kern][g].tobytes(), (g, kern)
            for radius in mr.RADII:
                u, v = got["joint"][radius][g], plain["joint"][radius][g]
                assert all(getattr(u, k).tobytes() == getattr(v, k).tobytes() for k in ("S", "gs", "V", "gc")), (g, radius)
            for k in ("cov", "depth_cov"):
                sl = slice(lo, hi) if k == "depth_cov" else g
                assert getattr(got["cov"], k)[sl].tobytes() == getattr(plain["cov"], k)[sl].tobytes(), (g, k)
            for k in ("xyz", "cov", "score"):
                assert getattr(got["structure"], k)[lo:hi].tobytes() == getattr(plain["structure"], k)[lo:hi].tobytes(), (g, k)
            continue
        pose = me.BATCH_POSES[g]
        key = (kind, pose, n, 0, f32)
        out_ref = mr.classes(c, f32, 1.0, mr.LD)[1]
        res = got["res"]
        err = mr.residual_errors(res.e[lo:hi], res.sq_norm[lo:hi], c, f32)
        bounds = _row_bounds(c, kind, "residuals")
        assert (err <= bounds).all(), (g, err.max())
        assert np.array_equal(res.inlier[lo:hi], ~out_ref) and res.n_inlier[g] == int((~out_ref).sum()), g
        for kern in KERNELS:
            worst = max(worst, _check_pack(got["eval", kern][g], key, api.MODE_RT, api.DEPTH_PER_MATCH, 1.0, kind, f"pair {g} kernel {kern}"))
        for radius in mr.RADII:
            pas = "eval_joint" if np.isfinite(radius) else "eval_joint_inf"
            if pose in mr.entry_poses(kind, pas):
                worst = max(worst, _check_joint(got["joint"][radius][g], key, radius, kind, pas, f"pair {g} radius {radius:g}"))
        s2 = me.sin2(c, f32)
        assert not ((s2 > 3e-10) & (s2 < 3e-9)).any(), g                 # no row near the cut: the count is the same in any arithmetic
        degenerate = int((s2 <= 1e-9).sum())
        assert got["cov"].status[g] == 0 and got["structure"].status[g] == 0, (g, got["cov"].status[g])
        assert got["cov"].n_degenerate[g] == degenerate and got["cov"].n_used[g] == n - degenerate, (g, got["cov"].n_degenerate[g], degenerate)
        assert got["structure"].pose.n_degenerate[g] == degenerate, g
        worst = max(worst, _check_cov_structure(got["cov"].cov[g], got["cov"].depth_cov[lo:hi], got["structure"].xyz[lo:hi], got["structure"].cov[lo:hi],
                                                got["structure"].score[lo:hi], key, kind, f"pair {g}"))
    print(f"largest err / bound {kind} store={store} layout={layout}: {worst:.3g}")


BATCH_DEPTH_ITERATIONS = 3
BATCH_JOINT_ITERATIONS = 6


def _depth_summary(s):
    return (s.num_iterations, s.num_successful_steps, s.num_line_search_steps, s.termination)


@lru_cache(maxsize=None)
def _single_solves(kind, store):
    """Problem.solve_depths and Problem.solve_joint on pairs 1 and 3 alone, at the options of test_batch_solves: computed once,
    shared by the layouts and the drivers, left unchanged."""
    out = {}
    for g, c in enumerate(_batch_scenes(kind, 0, store)):
        if g in me.BATCH_EDGE_PAIRS:
            with _open(c, store) as p:
                out[g, "depth"] = p.solve_depths(c.rot_init, c.tran_init, options=_depth_opt(BATCH_DEPTH_ITERATIONS))
            with _open(c, store) as p:
                out[g, "joint"] = p.solve_joint(c.rot_init, c.tran_init, _joint_opt(iterations=BATCH_JOINT_ITERATIONS))
    return out


@layouts
@stores
@kinds
def test_batch_solves(monkeypatch, kind, store, layout):
    """Batch.solve_depths (3 iterations) and Batch.solve_joint (6 iterations) on the edge batch, through the one-launch / device
    drivers and the host lock-step drivers (SBA_BATCH_DEVICE_DEPTH, SBA_BATCH_DEVICE_JOINT), and Batch.covariance_joint /
    structure_joint through SBA_BATCH_DEVICE_COV.  Pairs 1 and 3 equal the single-problem solves under the relations of
    tests/test_gpu_batch.py (counts and termination equal, depths to 1e-9 of max(1, |d|)) and tests/test_gpu_batch_joint.py (counts
    equal, rot, tran and depths to RT_TOL); the two joint drivers and the two covariance drivers agree bit for bit; and the
    ordinary pairs give the bytes of the same batch with ordinary rows in pairs 1 and 3, driver by driver."""
    from helpers import RT_TOL_F32, RT_TOL_F64
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    tol = RT_TOL_F32 if _f32(store) else RT_TOL_F64
    single = _single_solves(kind, store)
    got = {}
    for which in (kind, "ordinary"):
        for driver in ("1", "0"):
            for name in ("SBA_BATCH_DEVICE_DEPTH", "SBA_BATCH_DEVICE_JOINT", "SBA_BATCH_DEVICE_COV"):
                monkeypatch.setenv(name, driver)
            with api.Batch(0) as b:
                cs, off, rot, tran = _batch(b, which, 0, store)
                depth = b.solve_depths(rot, tran, options=_depth_opt(BATCH_DEPTH_ITERATIONS))
            with api.Batch(0) as b:
                _batch(b, which, 0, store)
                joint = b.solve_joint(rot, tran, _joint_opt(iterations=BATCH_JOINT_ITERATIONS), check=False)
                b.set_depths(pe.cat(cs)[3])
                cov = b.covariance_joint(rot, tran, min_sin2_parallax=mr.COV_CUT, check=False)
                st = b.structure_joint(rot, tran, min_sin2_parallax=mr.COV_CUT, check=False)
            got[which, driver] = (depth, joint, cov, st)
    cs = _batch_scenes(kind, 0, store)
    off = pe.cat(cs)[0]
    for which in (kind, "ordinary"):                 # the joint and the covariance drivers: the same bytes
        (_, j1, c1, s1), (_, j0, c0, s0) = got[which, "1"], got[which, "0"]
        assert all(np.array_equal(j1[k], j0[k]) for k in (0, 1, 2, 4)) and [_counts(u) for u in j1[3]] == [_counts(v) for v in j0[3]], which
        assert c1.cov.tobytes() == c0.cov.tobytes() and c1.depth_cov.tobytes() == c0.depth_cov.tobytes(), which
        assert all(getattr(s1, k).tobytes() == getattr(s0, k).tobytes() for k in ("xyz", "cov", "score")), which
    for driver in ("1", "0"):
        (d, dsum, dstat), (rot, tran, jd, jsum, jstat), _, _ = got[kind, driver]
        (d0, dsum0, _), (rot0, tran0, jd0, jsum0, _), cov0, st0 = got["ordinary", driver]
        cov, st = got[kind, driver][2], got[kind, driver][3]
        for g in range(len(cs)):
            lo, hi = int(off[g]), int(off[g + 1])
            if g not in me.BATCH_EDGE_PAIRS:             # a pair does not see its neighbour's edge rows
                assert d[lo:hi].tobytes() == d0[lo:hi].tobytes() and _depth_summary(dsum[g]) == _depth_summary(dsum0[g]), (driver, g)
                assert rot[g].tobytes() == rot0[g].tobytes() and tran[g].tobytes() == tran0[g].tobytes() and jd[lo:hi].tobytes() == jd0[lo:hi].tobytes(), (driver, g)
                assert _counts(jsum[g]) == _counts(jsum0[g]) and cov.cov[g].tobytes() == cov0.cov[g].tobytes(), (driver, g)
                assert st.score[lo:hi].tobytes() == st0.score[lo:hi].tobytes(), (driver, g)
                continue
            assert dstat[g] == 0 and jstat[g] == 0, (driver, g, dstat[g], jstat[g])
            d1, s1 = single[g, "depth"]
            assert _depth_summary(dsum[g]) == _depth_summary(s1), (driver, g, _depth_summary(dsum[g]), _depth_summary(s1))
            assert np.abs(d[lo:hi] - d1).max() <= 1e-9 * max(1.0, np.abs(d1).max()), (driver, g, np.abs(d[lo:hi] - d1).max())
            r1, t1, jd1, js1 = single[g, "joint"]
            assert _counts(jsum[g]) == _counts(js1), (driver, g, _counts(jsum[g]), _counts(js1))
            assert np.abs(rot[g] - r1).max() <= tol and np.abs(tran[g] - t1).max() <= tol, (driver, g)
            assert np.abs(jd[lo:hi] - jd1).max() <= tol * np.abs(jd1).max(), (driver, g)
