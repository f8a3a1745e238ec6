"""GPU: the kernels held directly against the reference's own compiled code, through the fixtures tests/golden/reference_blocks.npz
and reference_maps.npz (written by tests/golden/make_reference_golden.py from oracle/_ref; tests/test_reference_pin_cpu.py holds the
oracle against the same files).  Nothing here reads the oracle or the reference's sources.

The sums are assembled in np.longdouble from the reference's long-double residual blocks with Ceres' Huber corrector
(tests/reference_pin.py); bounds are the project's REL_TOL_F64 through helpers.assert_normal_eq_close and test_gpu_joint._check_reduced,
outlier counts are exact, maps are byte for byte.  f32 planes are compared on the blocks of the f32-rounded inputs.  At the rotations
`next` and `tiny` the reference's LONG-DOUBLE Jets carry 1e-19 / theta of noise, five orders below the bound (measured against the
analytic long-double system of tests/ref_joint_numpy.py: 0.006 of the bound at most), so every rotation is treated alike."""
import ctypes as C
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

import pose_edges as pe
import ref_joint_numpy as rj
import reference_pin as rp
from helpers import REL_TOL_F64, assert_normal_eq_close
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api
from test_gpu_joint import RADII, _check_reduced

pytestmark = pytest.mark.gpu

STORES = (api.STORE_F64, api.STORE_F32)
KINDS = (api.KERNEL_FACTORED, api.KERNEL_EXPLICIT)
VARIANT = {api.STORE_F64: "f64", api.STORE_F32: "f32"}
TILED = 4099                  # several blocks and a partial wave
stores = pytest.mark.parametrize("store", STORES, ids=["f64", "f32"])
poses = pytest.mark.parametrize("name", pe.NAMES)


@lru_cache(maxsize=None)
def _blocks():
    return rp.load_blocks()


@lru_cache(maxsize=None)
def _maps():
    return rp.load_maps()


def _row_sets():
    """The fixture's 65 blocks; the same blocks tiled to 4 099 rows in a permuted order; the first block alone."""
    tiled = np.random.default_rng(TILED).permutation(np.arange(TILED) % rp.N_BLOCKS)
    return (np.arange(rp.N_BLOCKS), tiled, np.arange(1))


# ==== sweeps ===================================================================================================================
@stores
@poses
def test_sweeps_equal_the_sums_of_reference_blocks(name, store):
    """Problem.eval in MODE_ROT and MODE_TRAN with the uniform depths the reference's rot-only and tran-only problems use
    (init_d[0][0], init_d[1][0]) and in MODE_RT with per-match depths, both kernels: H, g and cost within REL_TOL_F64 of the
    long-double sums of the reference's blocks, the sum of weights likewise, the outlier count exact; n = 65, 4 099 (tiled,
    permuted) and 1.  Largest H / cost err / bound measured on the MI355X: 0.045 (tiny, either store), 0.017 (near_pi), below
    0.007 elsewhere."""
    z = _blocks()
    x1, x2, d12, rot, tran = rp.pose_inputs(z, name)            # uploaded as given: the f32 store rounds them itself
    d1, d2 = rp.quirk_depths(d12)
    refs = {mode: rp.mode_blocks(z, name, VARIANT[store], mode) for mode in (api.MODE_ROT, api.MODE_TRAN, api.MODE_RT)}
    worst = 0.0
    for rows in _row_sets():
        with api.Problem(0) as p:
            p.upload(x1[rows], x2[rows], d12[rows], store=store)
            for mode, (e, J6) in refs.items():
                ref = rp.normal_equations(e, J6, 1.0, rows=rows)
                for kind in KINDS:
                    p.set_kernel(kind)
                    if mode == api.MODE_RT:
                        got = p.eval(mode, rot, tran, huber_delta=1.0, depth_mode=api.DEPTH_PER_MATCH)
                    else:
                        got = p.eval(mode, rot, tran, d1, d2, 1.0, api.DEPTH_UNIFORM)
                    sH = float(np.abs(ref.H).max())
                    ratio = max(float(np.abs(got.H - ref.H).max()) / (REL_TOL_F64 * sH), float(abs(got.cost - ref.cost) / (REL_TOL_F64 * ref.cost)))
                    print(f"{name} store={store} n={len(rows)} mode={mode} kind={kind}: H, cost err / bound {ratio:.3g}")
                    worst = max(worst, ratio)
                    assert_normal_eq_close(got, ref, REL_TOL_F64, what=f"{name} store={store} n={len(rows)} mode={mode} kind={kind}")
                    if mode != api.MODE_ROT:
                        assert abs(got.sum_w - ref.sum_w) <= REL_TOL_F64 * ref.sum_w
                    assert got.n_outlier == ref.n_outlier, (name, len(rows), mode, kind, got.n_outlier, ref.n_outlier)
    print(f"largest err / bound {name} store={store}: {worst:.3g}")


# ==== the joint pass ===========================================================================================================
@stores
@poses
def test_eval_joint_reduced_system_from_reference_blocks(name, store):
    """Problem.eval_joint at RADII against the Schur complement formed in long double from the reference's joint blocks,
    3 x (2 + 3 + 3) each, by test_gpu_joint._check_reduced; the unreduced block, cost and outlier count against the same blocks."""
    z = _blocks()
    x1, x2, d12, rot, tran = rp.pose_inputs(z, name)
    v = VARIANT[store]
    res, jac = z[f"{name}_{v}_joint_res"], z[f"{name}_{v}_joint_jac"]

    def schur(_x1, _x2, _rot, _tran, _d, radius, dt=np.longdouble):
        part = rp.ld_of if dt == np.longdouble else (lambda a: rp.ld_of(a).astype(dt))
        e, J = part(res), part(jac)
        _, w = rp.huber_ld(1.0, np.sum(e * e, axis=1))
        return rj.schur_of_blocks(e, w, J[:, :, :2], J[:, :, 2:], radius, dt=dt)

    c = SimpleNamespace(rot_init=rot, tran_init=tran, d12=d12)
    ref = rp.normal_equations(*rp.mode_blocks(z, name, v, api.MODE_RT), 1.0)
    with api.Problem(0) as p:
        p.upload(x1, x2, d12, store=store)
        got = p.eval_joint(rot, tran)
        assert_normal_eq_close(SimpleNamespace(H=got.V, g=got.gc, cost=got.cost), ref, REL_TOL_F64, what=f"{name} store={store} unreduced")
        assert got.n_outlier == ref.n_outlier and abs(got.sum_w - ref.sum_w) <= REL_TOL_F64 * ref.sum_w
        for radius in RADII:
            _check_reduced(p, c, x1, x2, radius, f"{name} store={store}", schur=schur)


# ==== the d-only stage ========================================================================================================
@poses
def test_depth_stage_cost_and_bounds(name):
    """Problem.solve_depths: initial_cost is 1/2 sum of the reference's five squared residuals per match (no loss: the recorded
    d-only blocks carry none), and both lower bounds the reference sets (0 on either depth) act -- depths started below 0 end >= 0."""
    z = _blocks()
    x1, x2, d12, rot, tran = rp.pose_inputs(z, name)
    r = rp.ld_of(z[f"{name}_f64_depth_res"])
    assert r.shape == (rp.N_BLOCKS, 5) and not z[f"{name}_depth_meta"][:, 0].any()
    want = 0.5 * np.sum(r * r)
    lower = z[f"{name}_depth_lower"]
    assert np.array_equal(lower, np.zeros((rp.N_BLOCKS, 2)))
    with api.Problem(0) as p:
        p.upload(x1, x2, d12)
        d, s = p.solve_depths(rot, tran)
        print(f"{name}: initial cost err / bound {float(abs(s.initial_cost - want) / (REL_TOL_F64 * want)):.3g}")
        assert abs(s.initial_cost - want) <= REL_TOL_F64 * want
        assert (d >= lower).all() and s.final_cost <= s.initial_cost
        below = d12.copy()
        below[0:8, 0] = -0.5                                   # either bound, and both on one match
        below[4:12, 1] = -0.25
        p.set_depths(below)
        d, s = p.solve_depths(rot, tran)
        assert np.isfinite(d).all() and (d >= lower).all(), (name, d[:12])
        assert s.final_cost <= s.initial_cost


# ==== the remap on index images ===============================================================================================
@pytest.mark.parametrize("tiled", [None, "0"], ids=["default", "untiled"])
@pytest.mark.parametrize("h,w,s", rp.CUBE_GEOMETRIES)
def test_equi2cube_device_equals_the_reference_table(monkeypatch, h, w, s, tiled):
    """sba_equi2cube_device on a batch of 3 frames (the last frame group is short), through the default gather kernel and through
    SBA_GATHER_TILED=0: every pixel whose source the reference reads inside the image holds that source's bytes; the pixels the
    device clamps are exactly those where the reference reads beyond the image, and there it reads the image's last row."""
    torch = pytest.importorskip("torch")
    if tiled is not None:
        monkeypatch.setenv("SBA_GATHER_TILED", tiled)
    lib = cabi.load_library()
    table = _maps()[f"equi2cube_{h}_{w}_{s}"]
    beyond = table >= h * w
    assert int(beyond.sum()) == (0 if (h, w, s) == (100, 200, 33) else 1)
    index = rp.index_image(h, w)
    frames = np.stack([index, index[..., ::-1], 255 - index])           # frame 0 is the index image itself
    src = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    dst = torch.zeros((3, s, 6 * s, 3), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    cabi.check(lib, lib.sba_equi2cube_device(0, C.c_void_p(stream), C.c_void_p(src.data_ptr()), h, w, s, 3, C.c_void_p(dst.data_ptr())))
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    for f in range(3):
        want = frames[f].reshape(-1, 3)[table[~beyond]]
        assert out[f][~beyond].tobytes() == want.tobytes(), (f, tiled)
    got = rp.decode(out[0])
    assert np.array_equal(got != table, beyond)
    assert (got[beyond] // w == h - 1).all()
    single = api.equi2cube(index, s)                                     # the host entry point: one frame
    assert single.tobytes() == out[0].tobytes()


# ==== crop, rotate key-points, cube -> equirectangular ========================================================================
@pytest.mark.parametrize("pitch", rp.CROP_PITCHES)
@pytest.mark.parametrize("h,w", rp.CROP_GEOMETRIES)
def test_crop_and_rotate_kernels_equal_the_reference(h, w, pitch):
    z = _maps()
    tag = rp.pitch_tag(pitch)
    got = rp.decode(api.crop_rotated_image(rp.index_image(h, w), pitch))
    assert got.tobytes() == z[f"crop_{h}_{w}_{tag}"].tobytes()
    out = api.rotate_keypoints(rp.as_records(z[f"band_kp_{h}_{w}"]), pitch, w, h)
    assert np.ascontiguousarray(out[:, :2]).tobytes() == z[f"rotate_{h}_{w}_{tag}"].tobytes()
    assert not out[:, 2:].any()


@pytest.mark.parametrize("h,w,s", rp.CUBE2EQUI_GEOMETRIES)
def test_cube2equi_kernel_equals_the_reference(h, w, s):
    z = _maps()
    out = api.cube2equi_keypoints(rp.as_records(z[f"cube_kp_{s}"]), s, w, h)
    assert np.ascontiguousarray(out[:, :2]).tobytes() == z[f"cube2equi_{h}_{w}_{s}"].tobytes()
    assert not out[:, 2:].any()
