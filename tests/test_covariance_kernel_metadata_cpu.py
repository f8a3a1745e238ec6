"""CPU: the code-object METADATA of the covariance kernels (csrc/sba_covariance.hip compiled for gfx950 with the Makefile's
flags; hipcc cross-compiles): both streaming kernels exist for f64 and f32 planes, none uses scratch memory (a spill would
sit in the hot loop of a streaming kernel), and cov_reduce_kernel's registers allow two 256-thread blocks per CU -- the
point of its 25 accumulators against joint_reduce_kernel's 52.  Only the .amdgpu_metadata records are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spherical_bundle_adjuster_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")

REGISTER_FILE = 512      # unified vector registers per lane of a gfx950 SIMD (vector + accumulation registers)
GRANULE = 8              # allocation granularity


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """kernel name -> {field: int} from the .amdgpu_metadata records."""
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    out = tmp_path_factory.mktemp("cov_meta") / "sba_covariance.s"
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(CSRC, "sba_covariance.hip"), "-o", str(out)],
                   check=True, capture_output=True, cwd=CSRC)
    text = out.read_text()
    meta = text[text.index(".amdgpu_metadata"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for rec in meta.split("  - .agpr_count:")[1:]:
        rec = ".agpr_count:" + rec
        fields = dict(re.findall(r"\.(\w+):\s+(\S+)", rec))
        kernels[fields["name"]] = {k: int(v) for k, v in fields.items() if re.fullmatch(r"\d+", v)}
    return kernels


def _of(kernels, stem):
    return {k: v for k, v in kernels.items() if stem in k}


def test_every_instance_is_compiled(metadata):
    for stem in ("cov_reduce_kernel", "cov_depth_kernel"):
        inst = sorted(_of(metadata, stem))
        assert len(inst) == 2 and any("IdE" in k for k in inst) and any("IfE" in k for k in inst), (stem, list(metadata))
    assert len(_of(metadata, "cov_finalize_kernel")) == 1
    assert len(metadata) == 5, list(metadata)


def test_no_scratch(metadata):
    for k, f in metadata.items():
        assert f["private_segment_fixed_size"] == 0, (k, f)
        assert f["vgpr_spill_count"] == 0, (k, f)


def test_reduce_kernel_fits_two_blocks_per_cu(metadata):
    """A 256-thread block is one wave per SIMD; two resident blocks need two waves' registers in the 512-entry file."""
    for k, f in _of(metadata, "cov_reduce_kernel").items():
        regs = -(-(f["vgpr_count"] + f["agpr_count"]) // GRANULE) * GRANULE
        print(f"{k}: {f['vgpr_count']} vector + {f['agpr_count']} accumulation registers, {f['group_segment_fixed_size']} B LDS")
        assert REGISTER_FILE // regs >= 2, (k, f)
        assert f["max_flat_workgroup_size"] == 256
        assert 2 * f["group_segment_fixed_size"] <= 64 * 1024
    for k, f in _of(metadata, "cov_depth_kernel").items():
        regs = -(-(f["vgpr_count"] + f["agpr_count"]) // GRANULE) * GRANULE
        assert REGISTER_FILE // regs >= 2, (k, f)
