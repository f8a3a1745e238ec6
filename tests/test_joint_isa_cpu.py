"""CPU: the gfx950 code of the joint-solve kernels (Makefile flags, hipcc cross-compiles): both kernels exist for f64 and f32
coordinate planes and none of them -- nor the finalize kernel -- uses scratch memory (a spill would sit in the hot loop of
a streaming kernel)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spherical_bundle_adjuster_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")


@pytest.fixture(scope="module")
def joint_asm(tmp_path_factory):
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    out = tmp_path_factory.mktemp("isa") / "sba_joint.s"
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(CSRC, "sba_joint.hip"), "-o", str(out)],
                   check=True, capture_output=True, cwd=CSRC)
    return out.read_text()


def _kernels(asm):
    """kernel name -> (body text up to its .Lfunc_end marker, .amdhsa_private_segment_fixed_size)."""
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, flags=re.S | re.M):
        seg = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", m.group(2))
        out[m.group(1)] = (m.group(2), int(seg.group(1)) if seg else None)
    return out


def test_every_instance_is_compiled(joint_asm):
    kernels = _kernels(joint_asm)
    for stem in ("joint_reduce_kernel", "joint_step_kernel"):
        inst = sorted(k for k in kernels if stem in k)
        assert len(inst) == 2 and any("IdE" in k for k in inst) and any("IfE" in k for k in inst), (stem, list(kernels))
    assert sum("joint_finalize_kernel" in k for k in kernels) == 1
    assert len(kernels) == 5, list(kernels)


def test_no_scratch(joint_asm):
    for k, (body, private) in _kernels(joint_asm).items():
        assert private == 0, (k, private)
        assert "scratch_" not in body and "buffer_store" not in body, k


def test_streams_with_16_byte_accesses(joint_asm):
    """f64 planes: the two streaming kernels use 16-byte vector loads and stores (two matches per lane) and no 4- or 8-byte
    global LOADS at all -- every load of theirs is a plane access.  (Narrower stores exist by design: a block's row of
    partial sums is written as single doubles.)"""
    for k, (body, _) in _kernels(joint_asm).items():
        if "IdE" in k:
            assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, k
            assert not re.search(r"global_load_(dword|dwordx2|dwordx3)\b", body), k
