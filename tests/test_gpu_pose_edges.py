"""GPU: every kernel that picks a rotation frame, at the rotations where the frame changes (tests/pose_edges.py).

The frame is chosen by rot . rot > DBL_EPSILON at eight sites, five of them on the device by one thread per pair; rot = 0 is the
natural start of a solve.  Here the single-problem joint pass, covariance and structure, the batched sweep, residuals, joint pass,
covariance and structure (state and frame built on the device, the small_angle flag read per pair) and the solvers that start in
the small frame and leave it are run at POSES: zero, below and at the threshold, the first rotation above it, the band where
closed forms cancel, either side of the series switch, near pi and beyond it.

Checkers and bounds are the ones the project states already: _check_reduced (tests/test_gpu_joint.py), check_against
(tests/cov_reference.py), check_structure (tests/structure_reference.py), the long-double Schur forms of
tests/test_gpu_covariance.py and tests/test_gpu_structure.py, REL_TOL_* and RT_TOL_* of tests/helpers.py, and the relations of
tests/test_gpu_batch_joint.py, tests/test_gpu_batch_lm_drivers.py and tests/test_gpu_batch.py.  References use what the planes hold
(f32 planes: the f32-rounded inputs).  The scene conditions the bounds rest on are asserted on the CPU in
tests/test_pose_edges_reference_cpu.py and again here from the references."""
import re
from functools import lru_cache

import numpy as np
import pytest

import pose_edges as pe
import ref_joint_numpy as rj
from cov_reference import check_against, kappa_limit, sin2_parallax
from helpers import REL_TOL_F32, REL_TOL_F64, RT_TOL_F32, RT_TOL_F64, pack_from_eval
from joint_emulation import EmulatedJoint, drive
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api
from structure_reference import check_structure, dense_structure
from test_gpu_batch_joint import _counts, _same_solve
from test_gpu_batch_covariance import _same as _same_cov
from test_gpu_batch_structure import _same_rows
from test_gpu_covariance import schur_covariances
from test_gpu_joint import RADII, _check_reduced
from test_gpu_structure import INF_ROW, _planted, _same_pose, schur_structure

pytestmark = pytest.mark.gpu

STORES = (api.STORE_F64, api.STORE_F32)
LAYOUTS = ("0", "1")          # SBA_BATCH_INTERLEAVE
TOL = {api.STORE_F64: REL_TOL_F64, api.STORE_F32: REL_TOL_F32}
RT_TOL = {api.STORE_F64: RT_TOL_F64, api.STORE_F32: RT_TOL_F32}
GAUGES = (api.TRAN_SPHERE, api.TRAN_FREE)
KINDS = (api.KERNEL_FACTORED, api.KERNEL_EXPLICIT)
MODES = (api.MODE_ROT, api.MODE_TRAN, api.MODE_RT)
EVAL_SIZES = (65, 257, 4097)
DENSE_SIZES = (64, 65, 257)
SCHUR_SIZE = 4097             # every lane busy, ragged last vector
EPS = np.finfo(np.float64).eps
EMPTY = pe.BATCH_SIZES.index(0)
stores = pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
layouts = pytest.mark.parametrize("layout", LAYOUTS, ids=["contiguous", "interleaved"])
poses = pytest.mark.parametrize("name", pe.NAMES)


def _opt(tran_param):
    return api.default_lm_options(tran_param=tran_param)


def _f32(store):
    return store == api.STORE_F32


@lru_cache(maxsize=None)
def _structure_refs(name, n, f32, seed=pe.SEED):
    """{tran_param: DenseStructure} of scene_at(name, n), computed once and left unchanged; .pose is the covariance reference.
    The dense inverse up to 513 matches, the long-double Schur forms above."""
    c = pe.scene_at(name, n, seed)
    x1, x2 = pe.planes(c, f32)
    if n > 513:
        refs = schur_structure(x1, x2, c.rot_init, c.tran_init, c.d12)
        full = schur_covariances(x1, x2, c.rot_init, c.tran_init, c.d12)
        for tp in GAUGES:
            refs[tp].pose = full[tp]                     # with the 2 x 2 depth blocks
    else:
        refs = {tp: dense_structure(x1, x2, c.rot_init, c.tran_init, c.d12, tp) for tp in GAUGES}
    for tp in GAUGES:
        assert refs[tp].pose.kappa <= kappa_limit(n, tp), (name, n, tp, refs[tp].pose.kappa)
    return refs


@lru_cache(maxsize=None)
def _schur_ld(name, n, f32, radius, seed=pe.SEED):
    c = pe.scene_at(name, n, seed)
    x1, x2 = pe.planes(c, f32)
    return rj.schur_longdouble(x1, x2, c.rot_init, c.tran_init, c.d12, radius)


def _residual_reference(c, f32):
    """e in long double from the residual definition, and the scale of tests/test_gpu_batch_select.py: max(1, d1 + d2 + |t|)."""
    x1, x2 = pe.planes(c, f32)
    e = rj.JointProblem(x1, x2).residuals(c.rot_init, c.tran_init, c.d12, np.longdouble)
    return e, np.maximum(1.0, c.d12[:, 0] + c.d12[:, 1] + np.linalg.norm(c.tran_init))


# ==== the single problem, every pose ===========================================================================================
@stores
@poses
def test_eval_joint(capsys, name, store):
    """Problem.eval_joint at every pose, n = 65, 257 and 4097: the unreduced block against the RT sweep of both kernel kinds (bound
    REL_TOL_F64), the reduced system at RADII against the long-double Schur complement (_check_reduced, bound REL_TOL_F64).
    Largest err / bound measured on the MI355X: 0.116 (closed, f32 planes, the reduced system); f64 planes 0.054 (series)."""
    worst = 0.0
    for n in EVAL_SIZES:
        c = pe.scene_at(name, n)
        x1, x2 = pe.planes(c, _f32(store))
        with api.Problem(0) as p:
            p.upload(c.x1, c.x2, c.d12, store=store)
            got = p.eval_joint(c.rot_init, c.tran_init)
            for kind in KINDS:
                p.set_kernel(kind)
                ref = p.eval(api.MODE_RT, c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH)
                sH = np.abs(ref.H).max()
                ratios = (np.abs(got.V - ref.H).max() / (REL_TOL_F64 * sH),
                          np.abs(got.gc - ref.g).max() / (REL_TOL_F64 * max(np.abs(ref.g).max(), sH)),
                          abs(got.cost - ref.cost) / (REL_TOL_F64 * ref.cost), abs(got.sum_w - ref.sum_w) / (REL_TOL_F64 * ref.sum_w))
                print(f"{name} n={n} store={store} kind={kind}: unreduced block err / bound {max(ratios):.3g}")
                worst = max(worst, *ratios)
                assert max(ratios) <= 1.0, (name, n, kind, ratios)
                assert got.n_outlier == ref.n_outlier
            p.set_kernel(api.KERNEL_FACTORED)
            for radius in RADII:
                _check_reduced(p, c, x1, x2, radius, f"{name} n={n} store={store}")
    out = capsys.readouterr().out
    print(out, end="")
    reduced = re.findall(r"S err ([0-9.eE+-]+), gs err ([0-9.eE+-]+)", out)
    assert len(reduced) == len(EVAL_SIZES) * len(RADII)          # every _check_reduced line was read back
    worst = max(worst, *(float(v) / REL_TOL_F64 for pair in reduced for v in pair))
    print(f"largest err / bound {name} store={store}: {worst:.3g}")


@stores
@poses
def test_covariance_joint(name, store):
    """Problem.covariance_joint, both gauges: n = 64, 65, 257 against the dense inverse, n = 4097 against the long-double Schur
    form; bounds of check_against.  Largest err / bound measured on the MI355X: 0.0215 (at_eps, f64 planes); f32 planes 1.5e-8."""
    worst = 0.0
    for n in DENSE_SIZES + (SCHUR_SIZE,):
        c = pe.scene_at(name, n)
        with api.Problem(0) as p:
            p.upload(c.x1, c.x2, c.d12, store=store)
            for tp in GAUGES:
                ref = _structure_refs(name, n, _f32(store))[tp].pose
                got = p.covariance_joint(c.rot_init, c.tran_init, options=_opt(tp))
                assert (got.n_used, got.n_degenerate, got.dim, got.dof) == (n, 0, ref.m, n - ref.m)
                worst = max(worst, *check_against(got.cov, got.depth_cov, ref, TOL[store], what=f"{name} n={n} store={store} gauge={tp}"))
                assert abs(got.cost - ref.cost) <= TOL[store] * ref.cost and abs(got.sum_w - ref.sum_w) <= TOL[store] * ref.sum_w
                assert np.array_equal(got.cov, got.cov.T)
    print(f"largest err / bound {name} store={store}: {worst:.3g}")


@stores
@poses
def test_structure_joint(name, store):
    """Problem.structure_joint, both gauges: xyz, cov and score at n = 64, 65, 257 against G Sigma G^T on the dense inverse, at
    n = 4097 against the long-double Schur form; bounds of check_structure.  Largest err / bound measured on the MI355X: 0.0165
    (near_pi, f64 planes); f32 planes 3.4e-9."""
    worst = 0.0
    for n in DENSE_SIZES + (SCHUR_SIZE,):
        c = pe.scene_at(name, n)
        with api.Problem(0) as p:
            p.upload(c.x1, c.x2, c.d12, store=store)
            for tp in GAUGES:
                ref = _structure_refs(name, n, _f32(store))[tp]
                got = p.structure_joint(c.rot_init, c.tran_init, options=_opt(tp))
                assert (got.n_used, got.n_degenerate, got.dim, got.dof) == (n, 0, ref.pose.m, n - ref.pose.m)
                assert got.xyz.shape == (n, 3) and got.cov.shape == (n, 6) and got.score.shape == (n,)
                worst = max(worst, *check_structure(got.xyz, got.cov, got.score, ref, TOL[store], what=f"{name} n={n} store={store} gauge={tp}"))
                assert _same_pose(got.pose, p.covariance_joint(c.rot_init, c.tran_init, options=_opt(tp), depths=False))
    print(f"largest err / bound {name} store={store}: {worst:.3g}")


@stores
@pytest.mark.parametrize("n,planted", [(65, (1, 64)), (257, (0, 100, 256))])
@pytest.mark.parametrize("name", ["zero", "below_eps"])
def test_planted_degenerates_in_the_small_frame(name, n, planted, store):
    """cov_block's cut in the small frame: matches whose rays are parallel at the pose are counted, get (inf, inf, 0) / INF_ROW and
    an infinite score, and the other rows stay within the bounds of check_against / check_structure against the dense reference
    without them.  Largest err / bound measured on the MI355X: 0.0103 (zero, n = 65, f64 planes); f32 planes 5.1e-9."""
    c = pe.scene_at(name, n)
    planted = np.array(planted)
    rot, tran = c.rot_init, c.tran_init
    cd = _planted(c, planted, rot, store)
    p1, p2 = pe.planes(cd, _f32(store))
    keep = np.ones(n, dtype=bool)
    keep[planted] = False
    sin2 = sin2_parallax(p1, p2, rot)
    assert (sin2[planted] < 1e-10).all()
    assert not ((sin2[keep] >= 1e-10) & (sin2[keep] <= 1e-8)).any() and (sin2[keep] > 1e-8).all()
    ref = dense_structure(p1, p2, rot, tran, c.d12, api.TRAN_SPHERE, keep=keep)
    assert ref.pose.kappa <= kappa_limit(n, api.TRAN_SPHERE)
    used = np.flatnonzero(keep)
    with api.Problem(0) as p:
        p.upload(cd.x1, cd.x2, c.d12, store=store)
        cv = p.covariance_joint(rot, tran, min_sin2_parallax=1e-9)
        assert (cv.n_degenerate, cv.n_used, cv.dof) == (len(planted), n - len(planted), n - len(planted) - 5)
        assert np.array_equal(cv.depth_cov[planted], np.tile([np.inf, np.inf, 0.0], (len(planted), 1)))
        worst = max(check_against(cv.cov, cv.depth_cov, ref.pose, TOL[store], used=used, what=f"planted {name} n={n} store={store}"))
        assert abs(cv.cost - ref.pose.cost) <= TOL[store] * ref.pose.cost and abs(cv.sum_w - ref.pose.sum_w) <= TOL[store] * ref.pose.sum_w
        got = p.structure_joint(rot, tran, min_sin2_parallax=1e-9)
        assert (got.n_degenerate, got.n_used, got.dof) == (len(planted), n - len(planted), n - len(planted) - 5)
        assert np.array_equal(got.cov[planted], np.tile(INF_ROW, (len(planted), 1)))
        assert np.array_equal(got.score[planted], np.full(len(planted), np.inf))
        assert np.isfinite(got.xyz).all()
        assert np.abs(got.xyz[planted] - ref.xyz[planted]).max() <= TOL[store] * np.abs(ref.xyz[planted]).max()
        worst = max(worst, *check_structure(got.xyz, got.cov, got.score, ref, TOL[store], used=used, what=f"planted {name} n={n} store={store}"))
        assert _same_pose(got.pose, p.covariance_joint(rot, tran, min_sin2_parallax=1e-9, depths=False))
    print(f"largest err / bound planted {name} n={n} store={store}: {worst:.3g}")


@stores
@poses
def test_residuals(name, store):
    """Problem.residuals with per-match depths against the residual definition in long double: |e - ref| <= REL_TOL * max |e|, the
    squared norms likewise.  Largest err / bound measured on the MI355X: 5.4e-4 (near_pi, f64 planes); f32 planes 7.1e-11."""
    worst = 0.0
    for n in (65, SCHUR_SIZE):
        c = pe.scene_at(name, n)
        ref, _ = _residual_reference(c, _f32(store))
        sq = np.sum(ref * ref, axis=1)
        with api.Problem(0) as p:
            p.upload(c.x1, c.x2, c.d12, store=store)
            r = p.residuals(c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH, fields=("e", "sq_norm"))
        ratios = (float(np.abs(r.e - ref).max() / (TOL[store] * np.abs(ref).max())), float(np.abs(r.sq_norm - sq).max() / (TOL[store] * sq.max())))
        print(f"{name} n={n} store={store}: e err / bound {ratios[0]:.3g}, sq_norm err / bound {ratios[1]:.3g}")
        worst = max(worst, *ratios)
        assert max(ratios) <= 1.0, (name, n, ratios)
        assert r.n_inlier == int((r.sq_norm <= 1.0).sum()) and 0 < r.n_inlier < n
    print(f"largest err / bound {name} store={store}: {worst:.3g}")


# ==== one mixed batch: a pair per pose, an empty pair in the middle ============================================================
_ORACLE_PACKS = {}


def _oracle_pack(oracle, g, f32, mode, dm, d1, d2):
    """The oracle's pack of pair g of the mixed batch: computed once, shared by the kernel kinds and layouts, left unchanged."""
    key = (g, f32, mode, dm, float(d1), float(d2))
    if key not in _ORACLE_PACKS:
        c = pe.batch_scenes()[g]
        a1, a2 = pe.planes(c, f32)
        _ORACLE_PACKS[key] = pack_from_eval(mode, oracle.evaluate(mode, a1, a2, c.rot_init, c.tran_init, d1, d2, 1.0,
                                                                  c.d12 if dm == api.DEPTH_PER_MATCH else None))
    return _ORACLE_PACKS[key]


def _mixed(b, store):
    cs = pe.batch_scenes()
    off, x1, x2, d12, rot, tran = pe.cat(cs)
    b.upload(x1, x2, off, d12, store=store)
    return cs, off, rot, tran


def _expected_status():
    st = np.zeros(len(pe.BATCH_SIZES), dtype=np.int32)
    st[EMPTY] = cabi.SBA_ERR_NUMERIC                     # no match, no covariance
    return st


@layouts
@stores
def test_batch_eval(oracle, monkeypatch, store, layout):
    """Batch.eval on the mixed batch: three modes, both depth modes, both kernel kinds, every pair's pack within REL_TOL_F64 of
    the oracle's -- except at next and tiny, where the oracle's Jacobian carries eps / theta of noise: there MODE_RT per-match is
    held against V, gc and cost of the long-double Schur reference and the other combinations against Problem.eval at the same
    pose.  Largest err / bound measured on the MI355X: 9.1e-4, either store and layout."""
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    B = len(pe.BATCH_SIZES)
    d1, d2 = np.linspace(0.8, 1.7, B), np.linspace(1.3, 0.6, B)
    worst = 0.0
    with api.Batch(0) as b:
        cs, off, rot, tran = _mixed(b, store)
        packs = {}
        for kind in KINDS:
            b.set_kernel(kind)
            for mode in MODES:
                for dm in (api.DEPTH_PER_MATCH, api.DEPTH_UNIFORM):
                    packs[kind, mode, dm] = b.eval(mode, rot, tran, d1, d2, 1.0, dm)
    for g, (name, c) in enumerate(zip(pe.BATCH_POSES, cs)):
        n = len(c.x1)
        single = {}
        if name in pe.NOISY_ORACLE:
            with api.Problem(0) as p:
                p.upload(c.x1, c.x2, c.d12, store=store)
                for kind in KINDS:
                    p.set_kernel(kind)
                    for mode in MODES:
                        for dm in (api.DEPTH_PER_MATCH, api.DEPTH_UNIFORM):
                            single[kind, mode, dm] = p.eval_pack(mode, c.rot_init, c.tran_init, d1[g], d2[g], 1.0, dm)
        for (kind, mode, dm), pk in packs.items():
            if name in pe.NOISY_ORACLE and mode == api.MODE_RT and dm == api.DEPTH_PER_MATCH:
                ld, got = _schur_ld(name, n, _f32(store), float("inf")), api.expand_pack(mode, pk[g])
                sV = float(np.abs(ld["V"]).max())
                ratio = max(float(np.abs(got.H - ld["V"]).max()) / (REL_TOL_F64 * sV),
                            float(np.abs(got.g - ld["gc"]).max()) / (REL_TOL_F64 * max(float(np.abs(ld["gc"]).max()), sV)),
                            abs(got.cost - float(ld["cost"])) / (REL_TOL_F64 * float(ld["cost"])))
            else:
                if name in pe.NOISY_ORACLE:
                    ref = single[kind, mode, dm]
                else:
                    ref = _oracle_pack(oracle, g, _f32(store), mode, dm, d1[g], d2[g])
                ratio = float(np.abs(pk[g] - ref).max()) / (REL_TOL_F64 * max(float(np.abs(ref).max()), 1e-300))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, n, kind, mode, dm, ratio)
    print(f"largest err / bound store={store} layout={layout}: {worst:.3g}")


@layouts
@stores
def test_batch_residuals(monkeypatch, store, layout):
    """Batch.residuals with per-match depths: every pair's rows within 1e-12 * max(1, d1 + d2 + |t|) of the long-double restatement
    (the relation of tests/test_gpu_batch_select.py) and of Problem.residuals on the pair alone; flags and counts equal.  Largest
    err / bound measured on the MI355X: 2.1e-4 (f32 planes), 1.9e-4 (f64 planes)."""
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    with api.Batch(0) as b:
        cs, off, rot, tran = _mixed(b, store)
        r = b.residuals(rot, tran, depth_mode=api.DEPTH_PER_MATCH)
    worst = 0.0
    for g, c in enumerate(cs):
        lo, hi = int(off[g]), int(off[g + 1])
        if lo == hi:
            assert r.n_inlier[g] == 0
            continue
        ref, scale = _residual_reference(c, _f32(store))
        with api.Problem(0) as p:
            p.upload(c.x1, c.x2, c.d12, store=store)
            one = p.residuals(c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH)
        ratios = (float((np.abs(r.e[lo:hi].astype(np.longdouble) - ref).max(axis=1) / scale).max()) / 1e-12,
                  float((np.abs(r.e[lo:hi] - one.e).max(axis=1) / scale).max()) / 1e-12)
        worst = max(worst, *ratios)
        assert max(ratios) <= 1.0, (pe.BATCH_POSES[g], ratios)
        assert np.array_equal(r.inlier[lo:hi], one.inlier) and r.n_inlier[g] == one.n_inlier
        assert np.array_equal(r.inlier[lo:hi], r.sq_norm[lo:hi] <= 1.0)
    print(f"largest err / bound store={store} layout={layout}: {worst:.3g}")


@layouts
@stores
def test_batch_eval_joint(monkeypatch, store, layout):
    """Batch.eval_joint at RADII: every pair against Problem.eval_joint on the pair alone and against the long-double Schur
    complement, as tests/test_gpu_batch_joint.py holds them (REL_TOL_F64 of max |V|).  Largest err / bound measured on the
    MI355X: 0.135 (f32 planes), 0.093 (f64 planes), either layout."""
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    with api.Batch(0) as b:
        cs, off, rot, tran = _mixed(b, store)
        got = {radius: b.eval_joint(rot, tran, radius) for radius in RADII}
        res = b.residuals(rot, tran, depth_mode=api.DEPTH_PER_MATCH, fields=())
    worst = 0.0
    for g, (name, c) in enumerate(zip(pe.BATCH_POSES, cs)):
        n = len(c.x1)
        if n == 0:
            for radius in RADII:
                e = got[radius][g]
                assert not e.S.any() and not e.gs.any() and not e.V.any() and not e.gc.any()
                assert (e.cost, e.sum_w, e.n_outlier, e.gd_max) == (0.0, 0.0, 0.0, 0.0)
            continue
        with api.Problem(0) as p:
            p.upload(c.x1, c.x2, c.d12, store=store)
            for radius in RADII:
                e, ref = got[radius][g], p.eval_joint(c.rot_init, c.tran_init, radius)
                ld = _schur_ld(name, n, _f32(store), radius)
                scale = float(np.abs(ref.V).max())
                errs = {k: float(np.abs(getattr(e, k) - getattr(ref, k)).max()) / scale for k in ("S", "gs", "V", "gc")}
                err_ld = max(float(np.abs(e.S - ld["S"]).max()), float(np.abs(e.gs - ld["gs"]).max()),
                             float(np.abs(e.V - ld["V"]).max())) / float(np.abs(ld["V"]).max())
                print(f"{name} n={n} store={store} layout={layout} radius={radius:g}: vs single {max(errs.values()) / REL_TOL_F64:.3g}, "
                      f"vs long double {err_ld / REL_TOL_F64:.3g} of the bound")
                worst = max(worst, max(errs.values()) / REL_TOL_F64, err_ld / REL_TOL_F64)
                assert max(errs.values()) <= REL_TOL_F64, (name, radius, errs)
                assert err_ld <= REL_TOL_F64, (name, radius, err_ld)
                assert abs(e.cost - ref.cost) <= REL_TOL_F64 * ref.cost and abs(e.sum_w - ref.sum_w) <= REL_TOL_F64 * ref.sum_w
                assert e.n_outlier == ref.n_outlier == n - res.n_inlier[g]
                assert abs(e.gd_max - ref.gd_max) <= REL_TOL_F64 * max(ref.gd_max, 1.0)
                assert np.array_equal(e.S, e.S.T)
    print(f"largest err / bound store={store} layout={layout}: {worst:.3g}")


@layouts
@stores
@poses
def test_batch_covariance_and_structure(monkeypatch, name, store, layout):
    """Batch.covariance_joint and Batch.structure_joint on the mixed batch, both gauges: the pair at `name` against the dense
    references within the bounds of check_against / check_structure (xyz, cov and score); every status 0 but the empty pair's own.
    Largest err / bound measured on the MI355X: 0.0157 (below_eps, f64 planes), 9.7e-9 (near_pi, f32 planes).  With small_angle
    forced to 0 in cov_fill_params the f64 cases at below_eps and at_eps fail, in both layouts, and nothing else in this file:
    zero gives the same numbers in either frame, and at f32 planes the 1e-8 the frame moves A by is inside REL_TOL_F32."""
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    g = pe.BATCH_POSES.index(name)
    worst = 0.0
    with api.Batch(0) as b:
        cs, off, rot, tran = _mixed(b, store)
        c, n, lo, hi = cs[g], len(cs[g].x1), int(off[g]), int(off[g + 1])
        for tp in GAUGES:
            with pytest.raises(api.SbaError) as ei:              # the empty pair has no covariance
                b.covariance_joint(rot, tran, options=_opt(tp), depths=False)
            assert ei.value.code == cabi.SBA_ERR_NUMERIC
            cv = b.covariance_joint(rot, tran, options=_opt(tp), check=False)
            st = b.structure_joint(rot, tran, options=_opt(tp), check=False)
            assert np.array_equal(cv.status, _expected_status()) and np.array_equal(st.status, _expected_status())
            assert np.isnan(cv.cov[EMPTY]).all() and np.isnan(st.pose.cov[EMPTY]).all()
            _same_cov(st.pose, b.covariance_joint(rot, tran, options=_opt(tp), depths=False, check=False), "pose")
            ref = _structure_refs(name, n, _f32(store))[tp]
            assert (cv.n_used[g], cv.n_degenerate[g], cv.dim[g], cv.dof[g]) == (n, 0, ref.pose.m, n - ref.pose.m)
            what = f"batch {name} n={n} store={store} layout={layout} gauge={tp}"
            worst = max(worst, *check_against(cv.cov[g], cv.depth_cov[lo:hi], ref.pose, TOL[store], what=what))
            worst = max(worst, *check_structure(st.xyz[lo:hi], st.cov[lo:hi], st.score[lo:hi], ref, TOL[store], what=what))
            assert abs(cv.cost[g] - ref.pose.cost) <= TOL[store] * ref.pose.cost and abs(cv.sum_w[g] - ref.pose.sum_w) <= TOL[store] * ref.pose.sum_w
            assert np.array_equal(cv.cov[g], cv.cov[g].T)
    print(f"largest err / bound {name} store={store} layout={layout}: {worst:.3g}")


@layouts
@stores
@pytest.mark.parametrize("name", ["below_eps", "at_eps", "next", "near_pi"])
def test_a_pair_does_not_see_its_neighbours_frame(monkeypatch, name, store, layout):
    """Pair g of the mixed batch gives, byte for byte, what a batch holding it alone gives (the relation of
    test_a_pair_does_not_depend_on_its_batch): residuals, the joint pass, the covariance and the structure.  at_eps (small frame)
    and next (general frame) are neighbours in either frame's last and first rotation; below_eps sits between two small-frame
    pairs with B = I and B != I; near_pi between two closed-form pairs.  A flag or a frame taken from the block next door shows
    at the first two, a pair's own state leaking at all four."""
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    g = pe.BATCH_POSES.index(name)
    with api.Batch(0) as b:
        cs, off, rot, tran = _mixed(b, store)
        res = b.residuals(rot, tran, depth_mode=api.DEPTH_PER_MATCH)
        eq = b.eval_joint(rot, tran, 1e4)[g]
        cv = b.covariance_joint(rot, tran, check=False)
        st = b.structure_joint(rot, tran, check=False)
    c, lo, hi = cs[g], int(off[g]), int(off[g + 1])
    with api.Batch(0) as b:
        b.upload(c.x1, c.x2, np.array([0, len(c.x1)], dtype=np.uint64), c.d12, store=store)
        r1, t1 = c.rot_init[None], c.tran_init[None]
        res1 = b.residuals(r1, t1, depth_mode=api.DEPTH_PER_MATCH)
        eq1 = b.eval_joint(r1, t1, 1e4)[0]
        cv1 = b.covariance_joint(r1, t1)
        st1 = b.structure_joint(r1, t1)
    assert res1.e.tobytes() == res.e[lo:hi].tobytes() and res1.sq_norm.tobytes() == res.sq_norm[lo:hi].tobytes()
    assert np.array_equal(res1.inlier, res.inlier[lo:hi]) and res1.n_inlier[0] == res.n_inlier[g]
    assert all(getattr(eq1, k).tobytes() == getattr(eq, k).tobytes() for k in ("S", "gs", "V", "gc"))
    assert (eq1.cost, eq1.sum_w, eq1.n_outlier, eq1.gd_max) == (eq.cost, eq.sum_w, eq.n_outlier, eq.gd_max)
    assert cv1.status[0] == cv.status[g] == 0
    assert cv1.cov[0].tobytes() == cv.cov[g].tobytes() and cv1.depth_cov.tobytes() == cv.depth_cov[lo:hi].tobytes()
    assert (cv1.cost[0], cv1.sum_w[0], cv1.n_used[0], cv1.dim[0]) == (cv.cost[g], cv.sum_w[g], cv.n_used[g], cv.dim[g])
    assert st1.pose.cov[0].tobytes() == st.pose.cov[g].tobytes()
    for k in ("xyz", "cov", "score"):
        assert getattr(st1, k).tobytes() == getattr(st, k)[lo:hi].tobytes(), k


@layouts
@stores
def test_batch_drivers_agree_bitwise(monkeypatch, store, layout):
    """SBA_BATCH_DEVICE_COV=0 and SBA_BATCH_DEVICE_JOINT=0 -- the lock-step drivers, the host's finish and solver between the
    launches -- give the bytes of the default drivers on the mixed batch.  Both drivers of either pair build a pair's pass
    parameters, frame and flag included, on the device from the same code, so this comparison holds the host's solver and finish
    against the device's at these rotations; it does not see a frame that is wrong in both (the references above do)."""
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    got = {}
    for driver in ("1", "0"):
        monkeypatch.setenv("SBA_BATCH_DEVICE_COV", driver)
        monkeypatch.setenv("SBA_BATCH_DEVICE_JOINT", driver)
        with api.Batch(0) as b:
            cs, off, rot, tran = _mixed(b, store)
            got[driver] = ([b.covariance_joint(rot, tran, options=_opt(tp), check=False) for tp in GAUGES],
                           [b.structure_joint(rot, tran, options=_opt(tp), check=False) for tp in GAUGES],
                           [b.solve_joint(rot, tran, options=_opt(tp), check=False) for tp in GAUGES])
    for u, v in zip(got["1"][0], got["0"][0]):
        _same_cov(u, v, "covariance drivers")
    for u, v in zip(got["1"][1], got["0"][1]):
        _same_rows(u, v, "structure drivers")
    for u, v in zip(got["1"][2], got["0"][2]):
        _same_solve(u, v)
        assert not u[4].any()


# ==== solves that start in the small frame and leave it =======================================================================
@stores
@pytest.mark.parametrize("spec", pe.SOLVE_SCENES, ids=[f"{s[0]}-{s[1]}-{s[2]}" for s in pe.SOLVE_SCENES])
def test_solve_joint_leaves_the_small_frame(spec, store):
    """Problem.solve_joint from rot = 0 and from below the threshold, against the dense restatement and the product's step logic
    driven by numpy passes: the assertions of test_solve_joint_matches_dense_and_the_driven_solver, and the later iterations ran
    in the general frame."""
    c = pe.scene_at(*spec)
    tol = RT_TOL[store]
    x1, x2 = pe.planes(c, _f32(store))
    assert float(c.rot_init @ c.rot_init) <= EPS
    rr, tr, dr, sr = rj.dense_solve(x1, x2, c.rot_init, c.tran_init, c.d12)
    assert sr["margin"] >= 1e-3, sr
    hr, ht, hd, hs, hstatus, _, _ = drive(EmulatedJoint(x1, x2, c.d12), c.rot_init, c.tran_init)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12, store=store)
        rot, tran, d, s = p.solve_joint(c.rot_init, c.tran_init)
        assert (s.termination.replace("CONVERGENCE_", "").lower(), s.num_iterations, s.num_successful_steps, s.num_evaluations) == \
            (sr["termination"], sr["num_iterations"], sr["num_successful_steps"], sr["num_evaluations"])
        assert (s.num_iterations, s.num_successful_steps, s.num_evaluations) == (hs.num_iterations, hs.num_successful_steps, hs.num_evaluations)
        assert cabi.TERMINATION[hs.termination] == s.termination and hstatus == 0
        for ref_r, ref_t, ref_d in ((rr, tr, dr), (hr, ht, hd)):
            print(f"{spec} store={store}: rot {np.abs(rot - ref_r).max() / tol:.3g}, tran {np.abs(tran - ref_t).max() / tol:.3g}, "
                  f"depths {np.abs(d - ref_d).max() / (tol * np.abs(ref_d).max()):.3g} of the bound")
            assert np.abs(rot - ref_r).max() <= tol and np.abs(tran - ref_t).max() <= tol
            assert np.abs(d - ref_d).max() <= tol * np.abs(ref_d).max()
        assert s.final_cost <= s.initial_cost
        assert s.num_successful_steps >= 1 and float(rot @ rot) > EPS
        r = p.residuals(rot, tran, depth_mode=api.DEPTH_PER_MATCH, fields=("sq_norm",))
        rho = np.where(r.sq_norm > 1.0, 2.0 * np.sqrt(r.sq_norm) - 1.0, r.sq_norm)
        assert abs(0.5 * rho.sum() - s.final_cost) <= REL_TOL_F64 * max(s.final_cost, 1e-300) + 1e-24


@layouts
@stores
def test_batch_solve_joint_leaves_the_small_frame(monkeypatch, store, layout):
    """Batch.solve_joint on the small-frame starts mixed with two closed-form starts: the device driver equals the lock-step driver
    bit for bit (either builds every pass's frame and flag on the device from the camera the solver asks for), and every pair
    equals dense_solve and Problem.solve_joint by the relation of test_solve_joint_matches_dense_and_the_single_problem_solve:
    a flag that is not rebuilt after the first accepted step moves the later iterations away from the dense restatement."""
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    cs = pe.solve_scenes(with_closed=True)
    off, x1, x2, d12, rot0, tran0 = pe.cat(cs)
    tol = RT_TOL[store]
    got = {}
    for driver in ("1", "0"):
        monkeypatch.setenv("SBA_BATCH_DEVICE_JOINT", driver)
        with api.Batch(0) as b:
            b.upload(x1, x2, off, d12, store=store)
            got[driver] = b.solve_joint(rot0, tran0)
    _same_solve(got["1"], got["0"])
    rot, tran, d, sums, status = got["1"]
    assert not status.any()
    for g, c in enumerate(cs):
        a1, a2 = pe.planes(c, _f32(store))
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
        assert s.final_cost <= s.initial_cost and s.num_successful_steps >= 1 and float(rot[g] @ rot[g]) > EPS


@stores
@pytest.mark.parametrize("kind", KINDS, ids=["factored", "explicit"])
def test_batch_solve_leaves_the_small_frame(kind, store):
    """Batch.solve (state, frame and LM on the device), MODE_ROT and MODE_RT with per-match depths, from the same starts against
    Problem.solve on every pair alone, by the relations tests/test_gpu_batch_lm_drivers.py states: counts equal, final cost to
    1e-9 relative, R|t to 1e-11."""
    cs = pe.solve_scenes(with_closed=True)
    off, x1, x2, d12, rot0, tran0 = pe.cat(cs)
    with api.Batch(0) as b:
        b.set_kernel(kind)
        b.upload(x1, x2, off, d12, store=store)
        for mode, tp in ((api.MODE_ROT, api.TRAN_FREE), (api.MODE_RT, api.TRAN_SPHERE)):
            opt = _opt(tp)
            rot, tran, sums, status = b.solve(mode, rot0, tran0, depth_mode=api.DEPTH_PER_MATCH, options=opt)
            assert (status == 0).all()
            for g, c in enumerate(cs):
                with api.Problem(0) as p:
                    p.set_kernel(kind)
                    p.upload(c.x1, c.x2, c.d12, store=store)
                    r1, t1, s1 = p.solve(mode, c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH, options=opt)
                q = sums[g]
                print(f"mode={mode} kind={kind} store={store} pair {g}: {q.termination} after {q.num_iterations} iterations, "
                      f"R|t difference {max(np.abs(rot[g] - r1).max(), np.abs(tran[g] - t1).max()):.3e}")
                assert (q.num_iterations, q.num_successful_steps, q.num_evaluations, q.termination) == \
                    (s1.num_iterations, s1.num_successful_steps, s1.num_evaluations, s1.termination), (mode, g)
                assert abs(q.final_cost - s1.final_cost) <= 1e-9 * abs(s1.final_cost), (mode, g)
                assert np.abs(rot[g] - r1).max() <= 1e-11 and np.abs(tran[g] - t1).max() <= 1e-11, (mode, g)
                assert q.num_successful_steps >= 1 and float(rot[g] @ rot[g]) > EPS


@stores
def test_batch_pipeline_from_rot_zero(store):
    """Batch.solve_problem(rot = 0, use_initial_guess = False, joint = True): per pair the chain of the single-problem entry points
    from the same start, as test_batch_pipeline_matches_single_problem_pipelines asserts (stage iteration counts equal, depths and
    R|t to 1e-9); the joint stage is Batch.solve_joint from the staged result bit for bit, and Problem.solve_joint's counts and
    results within RT_TOL."""
    cs = pe.solve_scenes(with_closed=True)
    off, x1, x2, _, _, tran0 = pe.cat(cs)
    B = len(cs)
    rot0 = np.zeros((B, 3))
    d0 = np.full((int(off[-1]), 2), 6.0)
    with api.Batch(0) as b:
        b.upload(x1, x2, off, d0, store=store)
        plain = b.solve_problem(rot=rot0, tran=tran0, use_initial_guess=False, want_depths=True)
        manual = b.solve_joint(plain["rot"], plain["tran"])               # at the staged result, on the refined depths
        b.set_depths(d0)
        res = b.solve_problem(rot=rot0, tran=tran0, use_initial_guess=False, want_depths=True, joint=True)
    for k in ("rot", "tran", "d_uniform", "status", "d12"):
        assert np.array_equal(plain[k], res[k]), k
    assert (res["status"] == 0).all() and not res["joint_status"].any()
    _same_solve(manual, (res["joint_rot"], res["joint_tran"], res["joint_d12"], res["joint_stage"], res["joint_status"]))
    for g, c in enumerate(cs):
        lo, hi = int(off[g]), int(off[g + 1])
        with api.Problem(0) as p:
            p.upload(c.x1, c.x2, d0[lo:hi], store=store)
            d, sd = p.solve_depths(rot0[g], tran0[g])
            r1, t1, s1 = p.solve(api.MODE_ROT, rot0[g], tran0[g], d[0, 0], d[1, 0])
            r2, t2, s2 = p.solve(api.MODE_TRAN, r1, t1, d[0, 0], d[1, 0])
            rj_, tj, dj, sj = p.solve_joint(r2, t2)
        got = (res["depth_stage"][g].num_iterations, res["depth_stage"][g].num_line_search_steps, res["rot_stage"][g].num_iterations,
               res["tran_stage"][g].num_iterations)
        assert got == (sd.num_iterations, sd.num_line_search_steps, s1.num_iterations, s2.num_iterations), (g, got)
        assert np.abs(res["d12"][lo:hi] - d).max() <= 1e-9 * max(1.0, np.abs(d).max())
        assert np.abs(res["rot"][g] - r2).max() <= 1e-9 and np.abs(res["tran"][g] - t2).max() <= 1e-9, g
        assert s1.num_successful_steps >= 1 and float(res["rot"][g] @ res["rot"][g]) > EPS
        q = res["joint_stage"][g]
        print(f"pair {g} store={store}: joint {q.termination} after {q.num_iterations} iterations; |rot - single| "
              f"{np.abs(res['joint_rot'][g] - rj_).max():.3e}, |tran - single| {np.abs(res['joint_tran'][g] - tj).max():.3e}")
        assert _counts(q) == _counts(sj), g
        assert q.final_cost <= q.initial_cost
        # the relation of test_solve_joint_matches_dense_and_the_single_problem_solve
        assert np.abs(res["joint_rot"][g] - rj_).max() <= RT_TOL[store] and np.abs(res["joint_tran"][g] - tj).max() <= RT_TOL[store], g
        assert np.abs(res["joint_d12"][lo:hi] - dj).max() <= RT_TOL[store] * np.abs(dj).max(), g
