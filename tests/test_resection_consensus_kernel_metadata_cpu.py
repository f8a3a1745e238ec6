"""CPU: the code-object METADATA of the robust resection guess's kernels (csrc/sba_resection_consensus.hip compiled for gfx950
with the Makefile's flags; hipcc cross-compiles): all six instances exist -- resect_score_kernel, resect_inlier_moments_kernel
and resect_gather_kernel for f64 and f32 planes -- none uses scratch memory or spills (vector or scalar registers: either would
sit in the candidate loop of the compute-bound pass), blocks are 256 threads, the score pass fits at least two blocks per
CU -- by its registers and by its 16 KiB of counters in LDS -- and the inlier-moments pass one.  Only the .amdgpu_metadata
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
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """kernel name -> {field: int} from the .amdgpu_metadata records."""
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    out = tmp_path_factory.mktemp("resection_consensus_meta") / "sba_resection_consensus.s"
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(CSRC, "sba_resection_consensus.hip"), "-o", str(out)],
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
    by_lds = LDS_PER_CU // f["group_segment_fixed_size"] if f["group_segment_fixed_size"] else 1 << 30
    return min(REGISTER_FILE // regs, by_lds)


def test_every_instance_is_compiled(metadata):
    assert len(metadata) == 6, list(metadata)
    for st in ("Id", "If"):
        for kernel in ("resect_score_kernel", "resect_inlier_moments_kernel", "resect_gather_kernel"):
            assert any(f"{kernel}{st}E" in k for k in metadata), (kernel, st, list(metadata))


def test_no_scratch_no_spills_and_the_blocks_fit(metadata):
    """A 256-thread block is one wave per SIMD: b blocks per CU need b register sets in the 512-entry file."""
    for k, f in sorted(metadata.items()):
        print(f"{k}: {f['vgpr_count']} vector + {f['agpr_count']} accumulation registers, {f['sgpr_count']} scalar, "
              f"{f['group_segment_fixed_size']} B LDS, {f['kernarg_segment_size']} B arguments, {_blocks_per_cu(f)} block(s) per CU")
        assert f["private_segment_fixed_size"] == 0, (k, f)
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (k, f)
        assert f["max_flat_workgroup_size"] == 256, (k, f)
        assert _blocks_per_cu(f) >= (2 if "resect_score_kernel" in k else 1), (k, f)
