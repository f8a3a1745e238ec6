"""CPU: the gfx950 code of the selection kernels (Makefile flags, hipcc cross-compiles): none uses scratch memory, the
kernels that stream the s plane read it with 8-byte or wider loads, and their LDS leaves room for at least two blocks per CU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spherical_bundle_adjuster_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LDS_PER_CU = 160 * 1024      # CDNA4

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")


@pytest.fixture(scope="module")
def quantile_asm(tmp_path_factory):
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    out = tmp_path_factory.mktemp("isa") / "sba_quantile.s"
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(CSRC, "sba_quantile.hip"), "-o", str(out)],
                   check=True, capture_output=True, cwd=CSRC)
    return out.read_text()


def _kernels(asm):
    """kernel name -> (body up to its .Lfunc_end marker, private segment bytes, LDS bytes)."""
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, flags=re.S | re.M):
        seg = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", m.group(2))
        lds = re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", m.group(2))
        out[m.group(1)] = (m.group(2), int(seg.group(1)), int(lds.group(1)))
    return out


def test_every_kernel_is_compiled(quantile_asm):
    kernels = _kernels(quantile_asm)
    for stem in ("select_init_kernel", "select_hist_kernel", "select_narrow_kernel", "keep_below_kernel"):
        assert sum(stem in k for k in kernels) == 1, (stem, list(kernels))
    assert len(kernels) == 4, list(kernels)


def test_no_scratch(quantile_asm):
    for k, (body, private, _) in _kernels(quantile_asm).items():
        assert private == 0, (k, private)
        assert "scratch_" not in body and "buffer_store" not in body and "buffer_load" not in body, k


def test_s_plane_is_read_8_bytes_wide(quantile_asm):
    """The two kernels that stream the plane load it as dwordx2 (or wider) and have no narrower global load at all."""
    for k, (body, _, _) in _kernels(quantile_asm).items():
        if "select_hist_kernel" in k or "keep_below_kernel" in k:
            assert re.search(r"global_load_dwordx[24]\b", body), k
            assert not re.search(r"global_load_(dword|ubyte|ushort|sbyte|sshort)\b", body), k


def test_lds_lets_two_blocks_share_a_cu(quantile_asm):
    for k, (_, _, lds) in _kernels(quantile_asm).items():
        assert 2 * lds <= LDS_PER_CU, (k, lds)
    hist = [v for k, v in _kernels(quantile_asm).items() if "select_hist_kernel" in k][0]
    assert hist[2] == 8 * 256 * 4          # 8 prefixes x 256 bins of 32-bit counts
