"""Writes tests/golden/reference_blocks.npz and reference_maps.npz from the reference's own compiled code (oracle/_ref, built by
oracle/ref_build from the reference's sources; oracle/ref_py.py).  The files hold data only: inputs, and what the reference's
functions returned for them.  Run where the reference's sources are:  python tests/golden/make_reference_golden.py

tests/test_reference_pin_cpu.py re-runs build_blocks() / build_maps() and compares them with the committed files byte for byte."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from oracle import ref_py as ref  # noqa: E402
import pose_edges as pe  # noqa: E402
import reference_pin as rp  # noqa: E402


def build_blocks():
    """Per rotation of tests/pose_edges.py, n = 65: the scene, and the residual blocks of the reference's four problems evaluated
    at the scene's start -- on the inputs as given (f64) and on x1, x2 rounded to float32 (f32: what f32 planes hold; the d-only
    problem is kept for f64 only).  Arrays <pose>_<variant>_<problem>_{res,jac} hold (double, long-double hi, long-double lo) on
    their last axis, the f32 variant (hi, lo) alone; what add_residual recorded next to each block (loss, parameter blocks, shared pointers, bounds) is kept once
    per problem and pose under <pose>_<problem>_{meta,loss_delta,lower}."""
    out = {"poses": np.array(pe.NAMES)}
    for name in pe.NAMES:
        c = pe.scene_at(name, rp.N_BLOCKS)
        out[f"{name}_x1"], out[f"{name}_x2"], out[f"{name}_d12"] = c.x1, c.x2, c.d12
        out[f"{name}_rot"], out[f"{name}_tran"] = c.rot_init, c.tran_init
        for variant in rp.VARIANTS:
            x1, x2 = pe.planes(c, variant == "f32")
            for which, key in enumerate(rp.PROBLEMS):
                if variant == "f32" and key == "depth":
                    continue
                b = ref.sba_blocks(which, x1, x2, c.rot_init, c.tran_init, c.d12)
                keep = slice(0, 3) if variant == "f64" else slice(1, 3)      # f32: only the long-double pair is used
                out[f"{name}_{variant}_{key}_res"], out[f"{name}_{variant}_{key}_jac"] = b["res"][..., keep], b["jac"][..., keep]
                if variant == "f64":
                    out[f"{name}_{key}_meta"], out[f"{name}_{key}_loss_delta"] = b["meta"], b["loss_delta"]
                    out[f"{name}_{key}_lower"] = b["lower"]
    return out


def build_maps():
    """The reference's maps: get_all's source-index tables (index images: pixel i holds i; an entry >= H W is a read beyond the
    image), crop_rotated_image on index images (a skipped pixel reads 0: the stand-in Mat zero-fills), rotate_keypoint and
    cube2equi_pixel on the key-points of reference_pin.band_keypoints / cube_keypoints (inputs are stored too)."""
    out = {}
    for h, w, s in rp.CUBE_GEOMETRIES:
        out[f"equi2cube_{h}_{w}_{s}"], beyond = ref.equi2cube_table(h, w, s)
        assert beyond == int((out[f"equi2cube_{h}_{w}_{s}"] >= h * w).sum())
    for h, w in rp.CROP_GEOMETRIES:
        kp = rp.band_keypoints(h, w, seed=h)
        out[f"band_kp_{h}_{w}"] = kp
        for pitch in rp.CROP_PITCHES:
            tag = rp.pitch_tag(pitch)
            out[f"crop_{h}_{w}_{tag}"] = rp.decode(ref.crop_rotated_image(rp.index_image(h, w), pitch))
            out[f"rotate_{h}_{w}_{tag}"] = ref.rotate_keypoints(kp, pitch, w, h)
    for h, w, s in rp.CUBE2EQUI_GEOMETRIES:
        kp = rp.cube_keypoints(s, seed=s)
        out[f"cube_kp_{s}"] = kp
        out[f"cube2equi_{h}_{w}_{s}"] = ref.cube2equi_pixels(kp, s, w, h)
    return out


if __name__ == "__main__":
    np.savez_compressed(rp.BLOCKS_NPZ, **build_blocks())
    np.savez_compressed(rp.MAPS_NPZ, **build_maps())
    for p in (rp.BLOCKS_NPZ, rp.MAPS_NPZ):
        print(p.name, p.stat().st_size, "bytes")
