"""CPU: the code-object METADATA of the Hampel joint registration's kernel (csrc/sba_landmarks_register_hampel.hip compiled for
gfx950 with the Makefile's flags; hipcc cross-compiles): exactly the two instances of the reduce kernel (dense / indexed) exist,
neither uses scratch memory or spills a vector register, and blocks are 256 threads.  Registers and blocks per CU are printed
beside the robust kernel's (DESIGN.md section 3.27 records them), not mandated.  Only the .amdgpu_metadata records are read."""
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


def _metadata_of(stem, tmp):
    """kernel name -> {field: int} from the .amdgpu_metadata records of csrc/<stem>.hip."""
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    out = tmp / f"{stem}.s"
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(CSRC, f"{stem}.hip"), "-o", str(out)],
                   check=True, capture_output=True, cwd=CSRC)
    text = out.read_text()
    meta = text[text.index(".amdgpu_metadata"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for rec in meta.split("  - .agpr_count:")[1:]:
        rec = ".agpr_count:" + rec
        fields = dict(re.findall(r"\.(\w+):\s+(\S+)", rec))
        kernels[fields["name"]] = {k: int(v) for k, v in fields.items() if re.fullmatch(r"\d+", v)}
    return kernels


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    return _metadata_of("sba_landmarks_register_hampel", tmp_path_factory.mktemp("landmark_register_hampel_meta"))


def _blocks_per_cu(f):
    regs = -(-(f["vgpr_count"] + f["agpr_count"]) // GRANULE) * GRANULE
    return REGISTER_FILE // regs


def test_exactly_the_two_instances_are_compiled(metadata):
    assert len(metadata) == 2, list(metadata)
    for indexed in (0, 1):
        assert any(f"landmarks_register_hampel_reduce_kernelILb{indexed}EE" in k for k in metadata), (indexed, list(metadata))


def test_the_source_file_is_among_the_makefile_sources():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = next(line for line in mk.splitlines() if line.startswith("SRCS_HIP"))
    assert "sba_landmarks_register_hampel.hip" in srcs.split()


def test_no_scratch_and_no_vector_spills(metadata, tmp_path):
    """A 256-thread block is one wave per SIMD: b blocks per CU need b register sets in the 512-entry file.  The robust kernel's
    figures are printed beside for the record."""
    robust = _metadata_of("sba_landmarks_register_robust", tmp_path)
    for k, f in sorted(metadata.items()) + sorted(robust.items()):
        print(f"{k}: {f['vgpr_count']} vector + {f['agpr_count']} accumulation registers, {f['sgpr_count']} scalar "
              f"({f['sgpr_spill_count']} parked in vector lanes), {f['group_segment_fixed_size']} B LDS, "
              f"{f['kernarg_segment_size']} B arguments, {_blocks_per_cu(f)} block(s) per CU")
    for k, f in sorted(metadata.items()):
        assert f["private_segment_fixed_size"] == 0, (k, f)
        assert f["vgpr_spill_count"] == 0, (k, f)
        assert f["max_flat_workgroup_size"] == 256, (k, f)
        assert _blocks_per_cu(f) >= 1, (k, f)
