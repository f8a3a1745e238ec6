"""CPU: the code-object METADATA of the batched structure kernel (csrc/sba_batch_structure.hip compiled for gfx950 with the
Makefile's flags; hipcc cross-compiles): batch_structure_kernel exists for f64 and f32 planes and for the 7 subsets of its
outputs, and nothing else is in the file; no instantiation uses scratch memory or spills a vector register; a 256-thread block
-- one wave per SIMD -- fits a CU's register file and LDS.  Only the .amdgpu_metadata records are read."""
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
    out = tmp_path_factory.mktemp("batch_structure_meta") / "sba_batch_structure.s"
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(CSRC, "sba_batch_structure.hip"), "-o", str(out)],
                   check=True, capture_output=True, cwd=CSRC)
    text = out.read_text()
    meta = text[text.index(".amdgpu_metadata"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for rec in meta.split("  - .agpr_count:")[1:]:
        rec = ".agpr_count:" + rec
        fields = dict(re.findall(r"\.(\w+):\s+(\S+)", rec))
        kernels[fields["name"]] = {k: int(v) for k, v in fields.items() if re.fullmatch(r"\d+", v)}
    return kernels


def test_fourteen_instances_and_nothing_else(metadata):
    inst = sorted(k for k in metadata if "batch_structure_kernel" in k)
    assert len(inst) == 14 and len(metadata) == 14, list(metadata)
    subsets = {(x, c, s) for x in "01" for c in "01" for s in "01"} - {("0", "0", "0")}
    for planes in ("d", "f"):
        got = {m.groups() for m in (re.search(r"batch_structure_kernelI%sLb([01])ELb([01])ELb([01])EE" % planes, k) for k in inst) if m}
        assert got == subsets, (planes, got)


def test_no_scratch_no_spill_and_a_256_thread_block(metadata):
    for k, f in metadata.items():
        assert f["private_segment_fixed_size"] == 0, (k, f)
        assert f["vgpr_spill_count"] == 0, (k, f)
        assert f["max_flat_workgroup_size"] == 256, (k, f)


def test_one_block_per_cu_fits(metadata):
    """A 256-thread block is one wave per SIMD: its vector + accumulation registers, after the 8-register granule, must fit the
    512-entry file, and its LDS the 64 KiB a workgroup may address."""
    for k, f in metadata.items():
        regs = -(-(f["vgpr_count"] + f["agpr_count"]) // GRANULE) * GRANULE
        print(f"{k}: {f['vgpr_count']} vector + {f['agpr_count']} accumulation registers, {f['sgpr_count']} scalar "
              f"({f['sgpr_spill_count']} spilled), {f['group_segment_fixed_size']} B LDS")
        assert regs <= REGISTER_FILE, (k, f)
        assert f["group_segment_fixed_size"] <= 64 * 1024, (k, f)
