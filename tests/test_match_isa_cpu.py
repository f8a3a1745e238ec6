"""CPU: the gfx950 code of the descriptor-match kernels (Makefile flags, hipcc cross-compiles): the product kernel of
every padded dimension runs on the f32-input MFMA, and no match kernel uses scratch memory (a spill there would sit in
the inner loop of a compute-bound kernel)."""
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
def match_asm(tmp_path_factory):
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    out = tmp_path_factory.mktemp("isa") / "sba_match_kernels.s"
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(CSRC, "sba_match_kernels.hip"), "-o", str(out)],
                   check=True, capture_output=True, cwd=CSRC)
    return out.read_text()


def _kernels(asm):
    """kernel name -> (body text up to its .Lfunc_end marker, .amdhsa_private_segment_fixed_size)."""
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, flags=re.S | re.M):
        seg = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", m.group(2))
        out[m.group(1)] = (m.group(2), int(seg.group(1)) if seg else None)
    return out


def test_product_kernels_use_the_f32_mfma(match_asm):
    kernels = _kernels(match_asm)
    tiles = [k for k in kernels if "match_tiles_kernel" in k]
    assert len(tiles) == 3, list(kernels)
    for k in tiles:
        assert re.search(r"v_mfma_f32_(32x32x2|16x16x4)_f32", kernels[k][0]), k


def test_no_scratch(match_asm):
    kernels = _kernels(match_asm)
    assert len(kernels) == 6, list(kernels)
    for k, (body, private) in kernels.items():
        assert private == 0, (k, private)
        assert "scratch_" not in body and "buffer_store" not in body, k
