"""CPU: what tests/test_gpu_pose_edges.py rests on, checked without a GPU -- the reference's rotation derivative at every rotation
of tests/pose_edges.py, and the scene conditions (kappa within cov_reference.kappa_limit, solves away from their thresholds).

Just above the small-angle threshold the closed formula of ref_joint_numpy.rotation_derivatives cancels in float64 (1e-9 relative at
|w| = 3e-8); there it is evaluated at 50 digits and rounded once, and this file pins the result against the 50-digit differentiation
of Rodrigues' formula (ref_numpy.d_rotated_d_w_mp), which shares nothing with it but mpmath."""
import numpy as np
import pytest

import pose_edges as pe
import ref_joint_numpy as rj
import ref_numpy as rn
from cov_reference import check_against, dense_covariance, kappa_limit, sin2_parallax
from helpers import REL_TOL_F64
from structure_reference import check_structure, dense_structure
from test_gpu_covariance import schur_covariances
from test_gpu_joint import RADII
from test_gpu_structure import schur_structure

EPS = np.finfo(np.float64).eps
N_PIN = 64
SINGLE_DENSE = (64, 65, 257)
SINGLE_SCHUR = 4097
GAUGES = (1, 0)                 # TRAN_SPHERE, TRAN_FREE


@pytest.mark.parametrize("name", pe.NAMES)
def test_rotation_columns_of_the_reference(name):
    """Measured: at most 0.36 of the bound (series); 0.11 at next and tiny, where the float64 closed formula is 1e6 times off."""
    c = pe.scene_at(name, N_PIN)
    rot = pe.POSES[name]
    F = rj.JointProblem(c.x1, c.x2).blocks(rot, c.tran_init, c.d12)[3]
    assert np.array_equal(F[:, :, 3:], np.broadcast_to(np.eye(3), (N_PIN, 3, 3)))
    if name in pe.SMALL_FRAME:
        # R = I + [w]x: d(R x1)/dw_j = e_j x x1, so column j of F is -d1 (e_j x x1), bit for bit
        assert float(rot @ rot) <= EPS
        I = np.eye(3)
        want = np.stack([-c.d12[:, 0:1] * np.cross(I[j], c.x1) for j in range(3)], axis=2)
        assert np.array_equal(F[:, :, :3], want)
        return
    assert float(rot @ rot) > EPS
    ref = np.stack([-c.d12[i, 0] * rn.d_rotated_d_w_mp(rot, c.x1[i]) for i in range(N_PIN)])
    err, bound = np.abs(F[:, :, :3] - ref).max(), 8.0 * EPS * np.abs(F).max()
    print(f"{name}: rotation columns err / bound {err / bound:.3g}")
    assert err <= bound, (name, err / bound)


def test_the_threshold_poses_sit_where_they_say():
    th2 = {k: float(w @ w) for k, w in pe.POSES.items()}
    assert th2["at_eps"] == EPS and th2["next"] > EPS and np.nextafter(pe.POSES["at_eps"][0], 1.0) == pe.POSES["next"][0]
    assert pe.SMALL_FRAME == ("zero", "below_eps", "at_eps") and 0.0 < th2["below_eps"] < EPS
    assert EPS < th2["tiny"] < rj.CANCELLATION_BAND < th2["series"] < 0.25 < th2["closed"]
    assert np.sqrt(th2["closed"]) < 3.0 < np.sqrt(th2["near_pi"]) < np.pi < np.sqrt(th2["past_pi"])


def test_outside_the_band_the_reference_is_the_float64_closed_formula():
    """rotation_derivatives returns, outside eps < theta^2 < 1e-4, the bits of the formula as written in numpy."""
    for name in ("series", "closed", "near_pi", "past_pi"):
        w = pe.POSES[name]
        I, R = np.eye(3), rj.rotation(w)
        want = [(w[j] * rj.skew(w) + rj.skew(np.cross(w, (I - R) @ I[j]))) @ R / (w @ w) for j in range(3)]
        assert all(np.array_equal(a, b) for a, b in zip(rj.rotation_derivatives(w), want))
    for name in pe.SMALL_FRAME:
        assert all(np.array_equal(a, rj.skew(np.eye(3)[j])) for j, a in enumerate(rj.rotation_derivatives(pe.POSES[name])))
    ld = rj.rotation_derivatives(pe.POSES["tiny"], np.longdouble)
    assert ld[0].dtype == np.longdouble and np.abs(ld[0].astype(np.float64) - rj.rotation_derivatives(pe.POSES["tiny"])[0]).max() <= EPS


@pytest.mark.parametrize("name", pe.NAMES)
def test_single_problem_scenes_are_well_conditioned(name):
    for n in SINGLE_DENSE:
        c = pe.scene_at(name, n)
        for f32 in (False, True):
            x1, x2 = pe.planes(c, f32)
            for tp in GAUGES:
                ref = dense_covariance(x1, x2, c.rot_init, c.tran_init, c.d12, tp)
                assert ref.kappa <= kappa_limit(n, tp), (name, n, tp, ref.kappa)
                assert 0.5 < ref.sum_w / n < 1.0                     # both Huber branches
    c = pe.scene_at(name, SINGLE_SCHUR)
    refs = schur_covariances(c.x1, c.x2, c.rot_init, c.tran_init, c.d12, dt=np.float64)
    for tp in GAUGES:
        assert refs[tp].kappa <= kappa_limit(SINGLE_SCHUR, tp), (name, tp, refs[tp].kappa)


def _scenes_of(name):
    """Every scene tests/test_gpu_pose_edges.py evaluates at `name`: the single-problem sizes and the pair of the mixed batch."""
    sizes = set(SINGLE_DENSE + (SINGLE_SCHUR,)) | {n for p, n in zip(pe.BATCH_POSES, pe.BATCH_SIZES) if p == name}
    return [pe.scene_at(name, n) for n in sorted(sizes)]


@pytest.mark.parametrize("name", pe.NAMES)
def test_float64_restatements_meet_the_bounds_four_times_over(name):
    """The bounds the GPU tests use -- REL_TOL_F64 of max |V| on the reduced system, check_against, check_structure -- do not scale
    with the worst match's own condition.  They say something about a kernel only on scenes where plain float64 arithmetic in the
    reference's own formulas stays well inside them: here the float64 Schur forms and the dense inverse are held to a quarter of
    each bound against long double, at every radius and for both stores' inputs.  Measured: at most 0.19 of the bound on the reduced
    system (radius = inf), 0.05 on the covariance and structure bounds."""
    for c in _scenes_of(name):
        n = len(c.x1)
        for f32 in (False, True):
            x1, x2 = pe.planes(c, f32)
            assert sin2_parallax(x1, x2, c.rot_init).min() >= 0.99 * pe.MIN_SIN2
            args = (x1, x2, c.rot_init, c.tran_init, c.d12)
            for radius in (RADII if n <= 513 else RADII[:1]):        # damping only improves the blocks' condition: inf is the worst
                ld, f64 = rj.schur_longdouble(*args, radius), rj.schur_longdouble(*args, radius, dt=np.float64)
                scale = float(np.abs(ld["V"]).max())
                own = max(float(np.abs(f64[k] - ld[k]).max()) for k in ("S", "gs", "V")) / scale
                assert own <= 0.25 * REL_TOL_F64, (name, n, f32, radius, own)
            cov_ld, cov_64 = schur_covariances(*args), schur_covariances(*args, dt=np.float64)
            st_ld, st_64 = schur_structure(*args), schur_structure(*args, dt=np.float64)
            for tp in GAUGES:
                assert max(check_against(cov_64[tp].cov, cov_64[tp].depth_cov, cov_ld[tp], REL_TOL_F64, what=f"{name} n={n} Schur f64")) <= 0.25
                assert max(check_structure(st_64[tp].xyz, st_64[tp].cov, st_64[tp].score, st_ld[tp], REL_TOL_F64, what=f"{name} n={n} Schur f64")) <= 0.25
                if n <= 513 and not f32:
                    d = dense_structure(*args, tp)
                    assert max(check_against(d.pose.cov, d.pose.depth_cov, cov_ld[tp], REL_TOL_F64, what=f"{name} n={n} dense")) <= 0.25
                    assert max(check_structure(d.xyz, d.cov, d.score, st_ld[tp], REL_TOL_F64, what=f"{name} n={n} dense")) <= 0.25


def test_without_the_redraw_rule_float64_itself_misses_the_bounds():
    """Why scenes redraw nearly parallel matches: scene_at("near_pi", 64) without the rule holds one match with sin^2 = 2.2e-6, and
    there the references' own float64 forms miss the bounds against long double -- the reduced system 4.3 times over, the dense
    inverse's camera block 2.2 times.  No kernel is involved."""
    c = pe.scene_at("near_pi", 64, min_sin2=0.0)
    args = (c.x1, c.x2, c.rot_init, c.tran_init, c.d12)
    assert 1e-6 < np.sort(sin2_parallax(c.x1, c.x2, c.rot_init))[0] < 1e-5
    ld, f64 = rj.schur_longdouble(*args, float("inf")), rj.schur_longdouble(*args, float("inf"), dt=np.float64)
    assert float(np.abs(f64["S"] - ld["S"]).max()) > 2.0 * REL_TOL_F64 * float(np.abs(ld["V"]).max())
    ref = schur_covariances(*args)[1]
    assert ref.kappa <= kappa_limit(64, 1)
    d = dense_covariance(*args, 1)
    assert np.abs(d.cov - ref.cov).max() > 1.5 * ref.kappa * REL_TOL_F64 * np.abs(ref.cov).max()


def test_batch_scenes_are_well_conditioned():
    assert len(pe.BATCH_SIZES) == len(pe.BATCH_POSES) == len(pe.NAMES) + 1
    assert [p for p in pe.BATCH_POSES if p is not None] == list(pe.NAMES)
    off = pe.cat(pe.batch_scenes())[0]
    assert {int(o) % 2 for o, n in zip(off[:-1], pe.BATCH_SIZES) if n} == {0, 1}      # first rows even and odd
    for name, n, c in zip(pe.BATCH_POSES, pe.BATCH_SIZES, pe.batch_scenes()):
        if n == 0:
            continue
        assert np.array_equal(c.rot_init, pe.POSES[name])
        for tp in GAUGES:
            ref = dense_covariance(c.x1, c.x2, c.rot_init, c.tran_init, c.d12, tp)
            assert ref.kappa <= kappa_limit(n, tp), (name, n, tp, ref.kappa)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_solve_scenes_stay_off_their_thresholds_and_leave_the_small_frame(f32):
    for spec, c in zip(pe.SOLVE_SCENES + pe.SOLVE_CLOSED, pe.solve_scenes(with_closed=True)):
        x1, x2 = pe.planes(c, f32)
        rot, _, _, s = rj.dense_solve(x1, x2, c.rot_init, c.tran_init, c.d12)
        assert s["margin"] >= 1e-3, (spec, s)
        assert s["num_successful_steps"] >= 1 and float(rot @ rot) > EPS, spec
        if spec[0] in pe.SMALL_FRAME:
            assert float(c.rot_init @ c.rot_init) <= EPS
