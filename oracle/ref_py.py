"""TEST INFRASTRUCTURE ONLY: ctypes binding of oracle/_ref/libsba_ref.so -- four of the reference's own translation units, compiled
unchanged by oracle/ref_build/Makefile against stand-in OpenCV / Ceres headers.  Used to write and to re-check the fixtures
tests/golden/reference_blocks.npz and reference_maps.npz (tests/golden/make_reference_golden.py); no GPU test and nothing under
spherical_bundle_adjuster_amd/ imports this module.

What runs here is the reference's text: the cube-map and crop tables, the key-point maps, the four cost functors and their
add_residual functions.  What is ours: ceres::AngleAxisRotatePoint and the Jet arithmetic (oracle/ref_build/include/ceres), the
Mat that zero-fills and the 3 x 3 product (oracle/ref_build/include/opencv2/core.hpp)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
BUILD = HERE / "ref_build"
LIB = HERE / "_ref" / "libsba_ref.so"

JOINT, ROT, TRAN, DEPTH = 0, 1, 2, 3
SHAPES = {JOINT: (3, 8), ROT: (3, 3), TRAN: (3, 3), DEPTH: (5, 2)}      # residuals, parameters per block
NAMES = {JOINT: "joint", ROT: "rot", TRAN: "tran", DEPTH: "depth"}
POINTER_ROT, POINTER_TRAN, POINTER_OWN_D = 1, 2, 3

_lib = None


def reference_dir() -> Path:
    """Where the reference's sources are looked for: $SBA_REFERENCE_DIR, else `reference` next to the repository."""
    env = os.environ.get("SBA_REFERENCE_DIR")
    return Path(env) if env else HERE.parent.parent / "reference"


def can_build() -> bool:
    return (reference_dir() / "spherical_bundle_adjuster.cpp").exists()


def available() -> bool:
    """The library exists or can be built."""
    return LIB.exists() or can_build()


def build() -> None:
    r = subprocess.run(["make", "-C", str(BUILD), f"REF={reference_dir()}"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"make -C {BUILD} failed:\n{r.stdout}\n{r.stderr}")


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if can_build():
            build()                  # make: nothing to do when the library is newer than its sources
        # RTLD_LAZY: the matchers, SVDecomp, ceres::Solve ... are linked and never run, and stay undefined
        _lib = C.CDLL(str(LIB), mode=os.RTLD_LAZY)
        _lib.ref_equi2cube_table.restype = C.c_long
        _lib.ref_sba_blocks.restype = C.c_int
    return _lib


def _p(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def equi2cube_table(im_h: int, im_w: int, cube: int):
    """(cube, 6 cube) int32 source indices of the reference's get_all, and how many lie beyond the image (>= im_h * im_w)."""
    t = np.zeros((cube, 6 * cube), dtype=np.int32)
    beyond = lib().ref_equi2cube_table(C.c_int(im_h), C.c_int(im_w), C.c_int(cube), _p(t))
    return t, int(beyond)


def pitch_rotation(pitch_deg: float) -> np.ndarray:
    R = np.zeros(9)
    lib().ref_pitch_rotation(C.c_float(pitch_deg), _p(R))
    return R.reshape(3, 3)


def rotate_pixels(pitch_deg: float, rc: np.ndarray, width: int, height: int) -> np.ndarray:
    rc = np.ascontiguousarray(rc, dtype=np.int32).reshape(-1, 2)
    out = np.zeros_like(rc)
    lib().ref_rotate_pixels(C.c_float(pitch_deg), _p(rc), C.c_size_t(len(rc)), C.c_int(width), C.c_int(height), _p(out))
    return out


def crop_rotated_image(im: np.ndarray, pitch_deg: float) -> np.ndarray:
    im = np.ascontiguousarray(im, dtype=np.uint8)
    out = np.zeros((im.shape[0] // 4, im.shape[1], 3), dtype=np.uint8)
    lib().ref_crop_rotated_image(_p(im), C.c_int(im.shape[0]), C.c_int(im.shape[1]), C.c_float(pitch_deg), _p(out))
    return out


def rotate_keypoints(xy: np.ndarray, pitch_deg: float, width: int, height: int) -> np.ndarray:
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2).copy()
    lib().ref_rotate_keypoints(_p(xy), C.c_size_t(len(xy)), C.c_float(pitch_deg), C.c_int(width), C.c_int(height))
    return xy


def cube2equi_pixels(xy: np.ndarray, cube: int, im_w: int, im_h: int) -> np.ndarray:
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    out = np.zeros_like(xy)
    lib().ref_cube2equi_pixels(_p(xy), C.c_size_t(len(xy)), C.c_int(cube), C.c_int(im_w), C.c_int(im_h), _p(out))
    return out


def sba_blocks(which: int, x1, x2, rot, tran, d12) -> dict:
    """The residual blocks that the reference's add_residual of problem `which` hands Ceres, evaluated where it recorded them.
    res (n, R, 3) and jac (n, R, P, 3): last axis = (double evaluation, long-double hi, long-double lo).  meta, loss_delta, lower:
    see oracle/ref_build/shim_sba.cpp."""
    x1 = np.ascontiguousarray(x1, dtype=np.float64).reshape(-1, 3)
    x2 = np.ascontiguousarray(x2, dtype=np.float64).reshape(-1, 3)
    d12 = np.ascontiguousarray(d12, dtype=np.float64).reshape(-1, 2)
    rot, tran = np.ascontiguousarray(rot, dtype=np.float64), np.ascontiguousarray(tran, dtype=np.float64)
    n = len(x1)
    R, P = SHAPES[which]
    res = [np.zeros((n, R)) for _ in range(3)]
    jac = [np.zeros((n, R, P)) for _ in range(3)]
    meta = np.zeros((n, 8), dtype=np.int32)
    delta, lower = np.zeros(n), np.zeros((n, 2))
    rc = lib().ref_sba_blocks(C.c_int(which), C.c_int(n), _p(x1), _p(x2), _p(rot), _p(tran), _p(d12), _p(res[0]), _p(jac[0]),
                              _p(res[1]), _p(res[2]), _p(jac[1]), _p(jac[2]), _p(meta), _p(delta), _p(lower))
    if rc < 0:
        raise RuntimeError(f"ref_sba_blocks({NAMES[which]}) returned {rc}")
    return {"res": np.stack(res, axis=-1), "jac": np.stack(jac, axis=-1), "meta": meta, "loss_delta": delta, "lower": lower,
            "n_lower": rc}
