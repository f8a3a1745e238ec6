"""Shared by the reference-pin tests and tests/golden/make_reference_golden.py (tests/ only): how the fixtures made from the
reference's own compiled code (oracle/ref_build -> oracle/_ref) are laid out, and the long-double sums assembled from its blocks.

A block array's last axis holds (the reference's double evaluation, long-double hi, long-double lo): the functor ran through
Jet<double> -- what AutoDiffCostFunction hands Ceres -- and through Jet<long double>, stored as two doubles."""
from types import SimpleNamespace

import numpy as np

from helpers import GOLDEN

BLOCKS_NPZ = GOLDEN / "reference_blocks.npz"
MAPS_NPZ = GOLDEN / "reference_maps.npz"
N_BLOCKS = 65
PROBLEMS = ("joint", "rot", "tran", "depth")             # oracle/ref_py.py: JOINT, ROT, TRAN, DEPTH = 0 .. 3
VARIANTS = ("f64", "f32")                                # inputs as given / x1, x2 rounded to float32 (what f32 planes hold)
CUBE_GEOMETRIES = ((64, 128, 16), (90, 182, 22), (100, 200, 33))
CROP_GEOMETRIES = ((96, 192), (100, 200))
CROP_PITCHES = (-45.0, -90.0, 30.0)
CUBE2EQUI_GEOMETRIES = ((96, 192, 24), (100, 200, 33))


def pitch_tag(pitch):
    return f"p{int(pitch)}".replace("-", "m")


def index_image(h, w):
    """(h, w, 3) uint8: pixel i holds i in its three bytes, little endian."""
    idx = np.arange(h * w, dtype=np.uint32)
    return np.stack([idx & 0xff, (idx >> 8) & 0xff, (idx >> 16) & 0xff], axis=-1).astype(np.uint8).reshape(h, w, 3)


def decode(im):
    """(..., 3) uint8 -> int32 indices."""
    im = im.astype(np.int32)
    return im[..., 0] | (im[..., 1] << 8) | (im[..., 2] << 16)


def band_keypoints(h, w, seed):
    """Key-points of the (h / 4) x w band: every integer pixel, then 512 at fractional coordinates.  (n, 2) float32 x, y."""
    rr, cc = np.meshgrid(np.arange(h // 4), np.arange(w), indexing="ij")
    rng = np.random.default_rng(seed)
    frac = np.stack([rng.uniform(0, w, 512), rng.uniform(0, h // 4, 512)], axis=1)
    return np.concatenate([np.stack([cc.ravel(), rr.ravel()], axis=1), frac]).astype(np.float32)


def cube_keypoints(s, seed):
    """Key-points in the 6 s x s strip: 300 per face, then the face borders x = k s (k = 0 .. 6) at 20 heights each, y = 0 and
    y = s among them.  (n, 2) float32 x, y."""
    rng = np.random.default_rng(seed)
    pts = [np.stack([rng.uniform(k * s, (k + 1) * s, 300), rng.uniform(0, s, 300)], axis=1) for k in range(6)]
    ys = np.concatenate([[0.0, float(s)], rng.uniform(0, s, 18)])
    pts += [np.stack([np.full(20, float(k * s)), ys], axis=1) for k in range(7)]
    return np.concatenate(pts).astype(np.float32)


def as_records(xy):
    """(n, 2) float32 -> (n, 7) float32 rows of 28 bytes, the cv::KeyPoint layout the maps take."""
    kp = np.zeros((len(xy), 7), dtype=np.float32)
    kp[:, :2] = xy
    return kp


def load_blocks():
    with np.load(BLOCKS_NPZ) as z:
        return {k: z[k] for k in z.files}


def load_maps():
    with np.load(MAPS_NPZ) as z:
        return {k: z[k] for k in z.files}


def f64_of(a):
    """The reference's double evaluation (f64 variant only)."""
    assert a.shape[-1] == 3
    return np.ascontiguousarray(a[..., 0])


def ld_of(a):
    """The reference's long-double evaluation, hi + lo: the last two entries of the last axis."""
    return a[..., -2].astype(np.longdouble) + a[..., -1].astype(np.longdouble)


def pose_inputs(z, name, variant="f64"):
    """x1, x2 (as the variant's planes hold them), d12, rot, tran of pose `name`."""
    x1, x2 = z[f"{name}_x1"], z[f"{name}_x2"]
    if variant == "f32":
        x1, x2 = x1.astype(np.float32).astype(np.float64), x2.astype(np.float32).astype(np.float64)
    return x1, x2, z[f"{name}_d12"], z[f"{name}_rot"], z[f"{name}_tran"]


def huber_ld(delta, s):
    """rho, rho' of ceres::HuberLoss(delta) at s, element-wise in the type of s."""
    b = delta * delta
    root = np.sqrt(np.where(s > b, s, b))
    return np.where(s > b, 2 * delta * root - b, s), np.where(s > b, delta / root, np.ones_like(s))


def normal_equations(e, J6, delta, rows=None):
    """H (6, 6), g, cost, sum_w, n_outlier over [rot | tran], summed in the type of e, of blocks with residuals e (n, 3) and
    Jacobians J6 (n, 3, 6), with Ceres' Huber corrector: rho'' <= 0 for Huber, so residuals and Jacobian rows are scaled by
    sqrt(rho') -- H = sum rho' J^T J, g = sum rho' J^T e, cost = 1/2 sum rho.  rows: indices into the blocks, repeats allowed."""
    s = np.sum(e * e, axis=1)
    rho, w = huber_ld(delta, s)
    H = np.einsum("nra,nrb->nab", J6, J6) * w[:, None, None]
    g = np.einsum("nra,nr->na", J6, e) * w[:, None]
    out = s > delta * delta
    if rows is not None:
        H, g, rho, w, out = H[rows], g[rows], rho[rows], w[rows], out[rows]
    return SimpleNamespace(H=H.sum(0), g=g.sum(0), cost=0.5 * rho.sum(), sum_w=w.sum(), n_outlier=float(out.sum()))


def mode_blocks(z, name, variant, mode, part=ld_of):
    """e (n, 3) and J (n, 3, 6) over [rot | tran] of the blocks that sweep `mode` sums: MODE_ROT = 0 and MODE_TRAN = 1 the rot-only
    and tran-only problems (uniform depths init_d[0][0], init_d[1][0]), MODE_RT = 2 the joint problem's rot and tran columns
    (per-match depths)."""
    key = {0: "rot", 1: "tran", 2: "joint"}[mode]
    e, J = part(z[f"{name}_{variant}_{key}_res"]), part(z[f"{name}_{variant}_{key}_jac"])
    J6 = np.zeros((len(e), 3, 6), dtype=J.dtype)
    if mode == 0:
        J6[:, :, :3] = J
    elif mode == 1:
        J6[:, :, 3:] = J
    else:
        J6 = J[:, :, 2:]
    return e, J6


def quirk_depths(d12):
    """The uniform depths the rot-only and tran-only functors get: init_d[0][0] and init_d[1][0] (.cpp:941-942, :998-999)."""
    return float(d12[0, 0]), float(d12[1, 0])
