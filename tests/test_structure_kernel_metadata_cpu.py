"""CPU: the code-object METADATA of structure_kernel (csrc/sba_structure.hip compiled for gfx950 with the Makefile's flags;
hipcc cross-compiles): every instantiation -- f64 and f32 planes times the seven non-empty subsets of (xyz, cov, score) --
exists, none uses scratch memory (a spill would sit in the hot loop of a streaming kernel), a 256-thread block fits the
register file, and Sigma_c and the pass parameters sit in LDS, not in the kernel arguments.  Only the .amdgpu_metadata
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
    out = tmp_path_factory.mktemp("structure_meta") / "sba_structure.s"
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(CSRC, "sba_structure.hip"), "-o", str(out)],
                   check=True, capture_output=True, cwd=CSRC)
    text = out.read_text()
    meta = text[text.index(".amdgpu_metadata"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for rec in meta.split("  - .agpr_count:")[1:]:
        rec = ".agpr_count:" + rec
        fields = dict(re.findall(r"\.(\w+):\s+(\S+)", rec))
        kernels[fields["name"]] = {k: int(v) for k, v in fields.items() if re.fullmatch(r"\d+", v)}
    return kernels


def test_every_instance_is_compiled(metadata):
    assert all("structure_kernel" in k for k in metadata), list(metadata)
    assert len(metadata) == 14, list(metadata)
    for st in ("IdLb", "IfLb"):
        for x in (0, 1):
            for c in (0, 1):
                for s in (0, 1):
                    tag = f"structure_kernel{st}{x}ELb{c}ELb{s}E"
                    assert any(tag in k for k in metadata) == bool(x or c or s), tag


def test_no_scratch_and_a_block_fits(metadata):
    """A 256-thread block is one wave per SIMD: its vector and accumulation registers must fit the 512-entry file."""
    for k, f in sorted(metadata.items()):
        regs = -(-(f["vgpr_count"] + f["agpr_count"]) // GRANULE) * GRANULE
        print(f"{k}: {f['vgpr_count']} vector + {f['agpr_count']} accumulation registers, {f['sgpr_count']} scalar, "
              f"{f['group_segment_fixed_size']} B LDS, {f['kernarg_segment_size']} B arguments, {REGISTER_FILE // regs} block(s) per CU")
        assert f["private_segment_fixed_size"] == 0, (k, f)
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (k, f)
        assert f["max_flat_workgroup_size"] == 256
        assert REGISTER_FILE // regs >= 1, (k, f)


def test_parameters_are_staged_in_lds(metadata):
    """JointParams + Sigma_c + the threshold are ~1.1 KB: in LDS, while the kernel arguments -- the planes, five pointers and
    the hidden launch arguments -- stay below what the two SweepParams of a JointParams alone would take."""
    params = 36 * 8 + 2 * 43 * 8
    for k, f in metadata.items():
        assert f["group_segment_fixed_size"] >= params, (k, f)
        assert f["kernarg_segment_size"] < 2 * 43 * 8, (k, f)
