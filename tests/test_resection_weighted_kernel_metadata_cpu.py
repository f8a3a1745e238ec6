"""CPU: the code-object METADATA of the weighted-resection kernels (csrc/sba_resection_weighted.hip compiled for gfx950 with the
Makefile's flags; hipcc cross-compiles): every instantiation exists -- resect_wreduce_kernel for f64 and f32 planes with and
without the loss, resect_weights_kernel and resect_weight_rows_kernel for both plane types -- none uses scratch memory or spills a
vector register, blocks are 256 threads, and the blocks per CU are the ones DESIGN.md section 3.19 states: the reduce pass fits two with
f64 planes and is launched with one with f32 planes (its double buffer is 32 registers larger).  Only the .amdgpu_metadata
records are read."""
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
    out = tmp_path_factory.mktemp("resection_weighted_meta") / "sba_resection_weighted.s"
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(CSRC, "sba_resection_weighted.hip"), "-o", str(out)],
                   check=True, capture_output=True, cwd=CSRC)
    text = out.read_text()
    meta = text[text.index(".amdgpu_metadata"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for rec in meta.split("  - .agpr_count:")[1:]:
        rec = ".agpr_count:" + rec
        fields = dict(re.findall(r"\.(\w+):\s+(\S+)", rec))
        kernels[fields["name"]] = {k: int(v) for k, v in fields.items() if re.fullmatch(r"\d+", v)}
    return kernels


def _blocks_per_cu(f):
    regs = -(-(f["vgpr_count"] + f["agpr_count"]) // GRANULE) * GRANULE
    return REGISTER_FILE // regs


def test_every_instance_is_compiled(metadata):
    assert len(metadata) == 8, list(metadata)
    for st in ("Id", "If"):
        for loss in (0, 1):
            assert any(f"resect_wreduce_kernel{st}Lb{loss}E" in k for k in metadata), (st, loss, list(metadata))
        assert any(f"resect_weights_kernel{st}E" in k for k in metadata), (st, list(metadata))
        assert any(f"resect_weight_rows_kernel{st}E" in k for k in metadata), (st, list(metadata))


def test_no_scratch_no_vector_spills_and_the_blocks_fit(metadata):
    """A 256-thread block is one wave per SIMD: b blocks per CU need b register sets in the 512-entry file."""
    for k, f in sorted(metadata.items()):
        print(f"{k}: {f['vgpr_count']} vector + {f['agpr_count']} accumulation registers, {f['sgpr_count']} scalar "
              f"({f['sgpr_spill_count']} parked in vector lanes), {f['group_segment_fixed_size']} B LDS, "
              f"{f['kernarg_segment_size']} B arguments, {_blocks_per_cu(f)} block(s) per CU")
        assert f["private_segment_fixed_size"] == 0, (k, f)
        assert f["vgpr_spill_count"] == 0, (k, f)
        assert f["max_flat_workgroup_size"] == 256, (k, f)
        if "resect_wreduce_kernelId" in k:
            assert _blocks_per_cu(f) >= 2, (k, f)            # f64 planes: two blocks per CU, as the unweighted pass
        elif "resect_wreduce_kernelIf" in k:
            assert _blocks_per_cu(f) >= 1, (k, f)            # f32 planes: launched with one
        else:
            assert _blocks_per_cu(f) >= 2, (k, f)            # the passes without a reduction
