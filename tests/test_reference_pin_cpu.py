"""CPU: the oracle held against the reference's own compiled code.

oracle/ref_build compiles four of the reference's translation units unchanged (against stand-in OpenCV / Ceres headers) into
oracle/_ref; tests/golden/make_reference_golden.py ran its functions and wrote tests/golden/reference_blocks.npz and
reference_maps.npz.  Where oracle/_ref exists or can be built, the committed fixtures must equal what it produces now, byte for
byte.  Everything else reads the fixtures alone and never skips: the oracle's residual blocks (rot-only, tran-only, joint, d-only)
and its maps equal the reference's byte for byte, and oracle.evaluate equals the long-double sums of the reference's blocks within
REL_TOL_F64 (tests/helpers.py).

What this does not pin: ceres::AngleAxisRotatePoint and the Jet arithmetic are this project's restatements of Ceres' documentation
(oracle/ref_build/include/ceres), so the oracle and the reference share that text's meaning, not its compiled code.  DESIGN.md
section 6 lists the edges.

At the rotations `next` and `tiny` (pose_edges.NOISY_ORACLE) a dual-number Jacobian carries eps / theta of noise in double, so H
and g of oracle.evaluate are held against the sums of the reference's DOUBLE blocks there (the same arithmetic, bit for bit); cost,
sum of weights and the outlier count, which come from the residuals, are held against long double at every rotation."""
import importlib.util

import numpy as np
import pytest

import pose_edges as pe
import reference_pin as rp
from helpers import REL_TOL_F64, ROOT, assert_normal_eq_close

poses = pytest.mark.parametrize("name", pe.NAMES)
MODES = (0, 1, 2)                                         # MODE_ROT, MODE_TRAN, MODE_RT


@pytest.fixture(scope="module")
def blocks():
    return rp.load_blocks()


@pytest.fixture(scope="module")
def maps():
    return rp.load_maps()


def _generator():
    spec = importlib.util.spec_from_file_location("make_reference_golden", ROOT / "tests" / "golden" / "make_reference_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _same_arrays(now, committed, what):
    assert sorted(now) == sorted(committed), (what, sorted(set(now) ^ set(committed)))
    for k, a in now.items():
        b = committed[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), f"{what}: {k} differs from what the reference's code gives now"


# ==== where oracle/_ref can be had: the fixtures are what the reference's code produces ========================================
def _need_ref():
    from oracle import ref_py
    if not ref_py.available():
        pytest.skip(f"neither {ref_py.LIB} nor the reference's sources ({ref_py.reference_dir()}) exist: nothing to re-run")


def test_block_fixture_is_what_the_reference_computes_now(blocks):
    _need_ref()
    _same_arrays(_generator().build_blocks(), blocks, "reference_blocks.npz")


def test_map_fixture_is_what_the_reference_computes_now(maps):
    _need_ref()
    _same_arrays(_generator().build_maps(), maps, "reference_maps.npz")


def test_fixture_scenes_are_the_pose_edge_scenes(blocks):
    """The inputs in the fixture are pose_edges.scene_at(name, 65): the fixture speaks about the scenes the GPU tests run."""
    assert tuple(blocks["poses"]) == pe.NAMES
    for name in pe.NAMES:
        c = pe.scene_at(name, rp.N_BLOCKS)
        for k, a in (("x1", c.x1), ("x2", c.x2), ("d12", c.d12), ("rot", c.rot_init), ("tran", c.tran_init)):
            assert blocks[f"{name}_{k}"].tobytes() == np.ascontiguousarray(a).tobytes(), (name, k)


# ==== what add_residual records ===============================================================================================
@poses
def test_recorded_problems(blocks, name):
    """Loss, parameter blocks, shared pointers and bounds as the reference's add_residual functions set them: the joint problem
    HuberLoss(1.0) on blocks (2, 3, 3) = (the match's own depths, the shared rot, the shared tran) and no bounds; rot-only and
    tran-only HuberLoss(1.0) on the shared rot / tran; d-only no loss, the match's own depths, both lower bounds 0."""
    n = rp.N_BLOCKS
    want = {"joint": ([1, 3, 2, 3, 3, 3, 1, 2], 1.0), "rot": ([1, 1, 3, 0, 0, 1, 0, 0], 1.0), "tran": ([1, 1, 3, 0, 0, 2, 0, 0], 1.0),
            "depth": ([0, 1, 2, 0, 0, 3, 0, 0], 0.0)}
    for key, (meta, delta) in want.items():
        assert np.array_equal(blocks[f"{name}_{key}_meta"], np.tile(np.array(meta, dtype=np.int32), (n, 1))), key
        assert np.array_equal(blocks[f"{name}_{key}_loss_delta"], np.full(n, delta)), key
        lower = blocks[f"{name}_{key}_lower"]
        assert np.array_equal(lower, np.zeros((n, 2))) if key == "depth" else np.isnan(lower).all(), key


# ==== the oracle's blocks, byte for byte =======================================================================================
@poses
def test_oracle_rot_and_tran_blocks(oracle, blocks, name, variant="f64"):
    """oracle.point in MODE_ROT / MODE_TRAN with the depths oracle.stage_depths gives (init_d[0][0], init_d[1][0]) equals the
    reference's rot-only / tran-only blocks byte for byte: residuals and the 3 x 3 Jacobian; the frozen columns are zero."""
    x1, x2, d12, rot, tran = rp.pose_inputs(blocks, name, variant)
    d1, d2 = oracle.stage_depths(d12)
    assert (d1, d2) == rp.quirk_depths(d12)
    for mode, key, cols, frozen in ((0, "rot", slice(0, 3), slice(3, 6)), (1, "tran", slice(3, 6), slice(0, 3))):
        e_ref, J_ref = rp.f64_of(blocks[f"{name}_{variant}_{key}_res"]), rp.f64_of(blocks[f"{name}_{variant}_{key}_jac"])
        for i in range(len(x1)):
            e, J = oracle.point(mode, x1[i], x2[i], rot, tran, d1, d2)
            assert e.tobytes() == e_ref[i].tobytes(), (name, key, i, e, e_ref[i])
            assert np.ascontiguousarray(J[:, cols]).tobytes() == J_ref[i].tobytes(), (name, key, i, J[:, cols], J_ref[i])
            assert not J[:, frozen].any()


@poses
def test_oracle_joint_and_depth_blocks(oracle, blocks, name):
    """oracle.point_joint (3 residuals, 2 + 3 + 3 columns) and oracle.point_depth (5 residuals, the two lambda exp(-c d) among
    them, 2 columns; lambda = c = 1 as .cpp:1057-1058 passes) equal the reference's blocks byte for byte; oracle.point in MODE_RT
    gives the joint block's rot and tran columns."""
    x1, x2, d12, rot, tran = rp.pose_inputs(blocks, name)
    e_j, J_j = rp.f64_of(blocks[f"{name}_f64_joint_res"]), rp.f64_of(blocks[f"{name}_f64_joint_jac"])
    e_d, J_d = rp.f64_of(blocks[f"{name}_f64_depth_res"]), rp.f64_of(blocks[f"{name}_f64_depth_jac"])
    assert J_j.shape == (rp.N_BLOCKS, 3, 8) and e_d.shape == (rp.N_BLOCKS, 5) and J_d.shape == (rp.N_BLOCKS, 5, 2)
    for i in range(len(x1)):
        e, J = oracle.point_joint(x1[i], x2[i], rot, tran, d12[i])
        assert e.tobytes() == e_j[i].tobytes() and J.tobytes() == J_j[i].tobytes(), (name, i, J, J_j[i])
        e6, J6 = oracle.point(2, x1[i], x2[i], rot, tran, d12[i, 0], d12[i, 1])
        assert e6.tobytes() == e_j[i].tobytes() and np.array_equal(J6, J_j[i][:, 2:]), (name, i)
        r, Jd = oracle.point_depth(x1[i], x2[i], rot, tran, d12[i])
        assert r.tobytes() == e_d[i].tobytes() and Jd.tobytes() == J_d[i].tobytes(), (name, i, Jd, J_d[i])
        want = np.exp(-d12[i].astype(np.longdouble))       # residuals 3 and 4 are lambda exp(-c d), to the last bit or the next
        assert (np.abs(r[3:] - want) <= np.finfo(np.float64).eps * want).all(), (name, i, r[3:], want)


@poses
def test_double_blocks_are_within_their_own_long_double(blocks, name):
    """The hi + lo pairs are the long-double evaluation of the same blocks: the reference's double residuals lie within 16 eps of
    them, relative to the largest term d1 + d2 + |t| (a residual is reached through fewer than 16 roundings of terms no larger
    than that), and hi is the pair rounded to double.  Largest measured: 1.9 eps (near_pi)."""
    x1, x2, d12, rot, tran = rp.pose_inputs(blocks, name)
    eps = np.finfo(np.float64).eps
    worst = 0.0
    for key in rp.PROBLEMS:
        res = blocks[f"{name}_f64_{key}_res"]
        s = d12.sum(axis=1) if key in ("joint", "depth") else np.full(len(x1), sum(rp.quirk_depths(d12)))
        s = np.maximum(s + np.linalg.norm(tran), 1.0)
        err = np.abs(rp.f64_of(res).astype(np.longdouble) - rp.ld_of(res)).max(axis=1)
        worst = max(worst, float((err / (eps * s)).max()))
        assert (err <= 16 * eps * s).all(), (name, key, worst)
        for a in (res, blocks[f"{name}_f64_{key}_jac"]):
            assert np.array_equal(rp.ld_of(a).astype(np.float64), a[..., 1])
    print(f"{name}: double against long-double residuals, largest error {worst:.3g} eps of d1 + d2 + |t|")


# ==== oracle.evaluate against the sums of the reference's blocks ==============================================================
@pytest.mark.parametrize("variant", rp.VARIANTS)
@poses
def test_oracle_evaluate_equals_the_sums_of_reference_blocks(oracle, blocks, name, variant):
    """H, g, cost, sum of weights and outlier count of oracle.evaluate against the sums assembled in np.longdouble from the
    reference's blocks with Ceres' Huber corrector (reference_pin.normal_equations): assert_normal_eq_close at REL_TOL_F64, the
    outlier count exact.  MODE_ROT and MODE_TRAN run on the uniform depths of the quirk, MODE_RT on per-match depths."""
    x1, x2, d12, rot, tran = rp.pose_inputs(blocks, name, variant)
    d1, d2 = oracle.stage_depths(d12)
    for mode in MODES:
        got = oracle.evaluate(mode, x1, x2, rot, tran, d1, d2, 1.0, d12 if mode == 2 else None)
        ref = rp.normal_equations(*rp.mode_blocks(blocks, name, variant, mode), 1.0)
        assert got.n_outlier == ref.n_outlier, (name, mode)
        assert mode != 2 or 0 < ref.n_outlier < len(x1)   # per-match depths: both Huber branches are populated
        assert abs(got.cost - ref.cost) <= REL_TOL_F64 * ref.cost and abs(got.sum_w - ref.sum_w) <= REL_TOL_F64 * ref.sum_w, (name, mode)
        if name in pe.NOISY_ORACLE:
            if variant != "f64":
                continue                                   # the f32 variant holds no double blocks
            e, J6 = rp.mode_blocks(blocks, name, variant, mode, part=lambda a: rp.f64_of(a).astype(np.longdouble))
            ref = rp.normal_equations(e, J6, 1.0)
        assert_normal_eq_close(got, ref, REL_TOL_F64, what=f"{name} {variant} mode={mode}")


# ==== the maps, byte for byte ================================================================================================
@pytest.mark.parametrize("h,w,s", rp.CUBE_GEOMETRIES)
def test_oracle_equi2cube_table(oracle, maps, h, w, s):
    """oracle.equi2cube(clamp=True) on the index image equals the reference's get_all table at every pixel whose source lies in
    the image; the pixels where the reference reads beyond it are exactly the pixels the oracle clamps (and counts), and there
    the oracle reads the image's last row."""
    ref = maps[f"equi2cube_{h}_{w}_{s}"]
    im = rp.index_image(h, w)
    out, clamped = oracle.equi2cube(im, s, clamp=True)
    skipped, clamped2 = oracle.equi2cube(im, s, clamp=False)
    got, beyond = rp.decode(out), ref >= h * w
    assert got.shape == ref.shape == (s, 6 * s)
    assert np.array_equal(got[~beyond], ref[~beyond])
    oracle_set = got != rp.decode(skipped)                 # without clamping the oracle leaves those pixels unwritten
    assert np.array_equal(oracle_set, beyond) and clamped == clamped2 == int(beyond.sum())
    assert (got[beyond] // w == h - 1).all()
    if (h, w, s) != (100, 200, 33):
        assert beyond.sum() == 1                           # theta == pi at the centre of the bottom face: row == h
    else:
        assert not beyond.any()


@pytest.mark.parametrize("pitch", rp.CROP_PITCHES)
@pytest.mark.parametrize("h,w", rp.CROP_GEOMETRIES)
def test_oracle_crop_and_rotate(oracle, maps, h, w, pitch):
    """oracle.crop_rotated_image on the index image and oracle.rotate_keypoints on the band's key-points equal the reference's
    crop_rotated_image and rotate_keypoint byte for byte (pitch-only rotations; a pixel the crop skips reads 0 on both sides)."""
    tag = rp.pitch_tag(pitch)
    got = rp.decode(oracle.crop_rotated_image(rp.index_image(h, w), pitch))
    assert got.tobytes() == maps[f"crop_{h}_{w}_{tag}"].tobytes()
    kp = maps[f"band_kp_{h}_{w}"]
    assert kp.tobytes() == rp.band_keypoints(h, w, seed=h).tobytes()
    out = oracle.rotate_keypoints(rp.as_records(kp), pitch, w, h)
    assert np.ascontiguousarray(out[:, :2]).tobytes() == maps[f"rotate_{h}_{w}_{tag}"].tobytes()
    assert not out[:, 2:].any()


@pytest.mark.parametrize("h,w,s", rp.CUBE2EQUI_GEOMETRIES)
def test_oracle_cube2equi(oracle, maps, h, w, s):
    """oracle.cube2equi_keypoints equals the reference's cube2equi_pixel byte for byte, face borders x = k s included."""
    kp = maps[f"cube_kp_{s}"]
    assert kp.tobytes() == rp.cube_keypoints(s, seed=s).tobytes()
    assert all((kp[:, 0] == k * s).sum() >= 20 for k in range(7))
    out = oracle.cube2equi_keypoints(rp.as_records(kp), s, w, h)
    assert np.ascontiguousarray(out[:, :2]).tobytes() == maps[f"cube2equi_{h}_{w}_{s}"].tobytes()
