"""CPU: the gfx950 code of the batched joint-solve kernels (csrc/sba_batch_joint.hip; Makefile flags, hipcc cross-compiles).
Both kernels exist for f64 and f32 coordinate planes, as one 256-thread block with one wave per SIMD to itself; none uses
scratch memory (a spill would sit in the hot loop of a streaming kernel, a stack frame of the solver in every trip of the
device loop); the f64 instances stream with 16-byte accesses.  And the single-problem file, which now compiles the same
per-match source from sba_joint_core.hpp, still yields exactly its five scratch-free kernels."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spherical_bundle_adjuster_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")

KERNELS = ("batch_joint_pass_kernel", "batch_joint_solve_kernel")


def _asm(tmp_path_factory, name):
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-flags"], check=True, capture_output=True, text=True).stdout.split()
    out = tmp_path_factory.mktemp("isa") / (name + ".s")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", os.path.join(CSRC, name + ".hip"), "-o", str(out)],
                   check=True, capture_output=True, cwd=CSRC)
    return out.read_text()


@pytest.fixture(scope="module")
def batch_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "sba_batch_joint")


@pytest.fixture(scope="module")
def single_asm(tmp_path_factory):
    return _asm(tmp_path_factory, "sba_joint")


def _functions(asm):
    """symbol -> (body text up to its .Lfunc_end marker, its .amdhsa_ kernel descriptor fields or None for a plain function)."""
    desc = {m.group(1): dict(re.findall(r"\.amdhsa_(\w+)\s+(\S+)", m.group(2)))
            for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, flags=re.S | re.M)}
    return {m.group(1): (m.group(2), desc.get(m.group(1)))
            for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, flags=re.S | re.M)}


def test_every_instance_is_compiled_and_nothing_is_called(batch_asm):
    fns = _functions(batch_asm)
    for stem in KERNELS:
        inst = sorted(k for k in fns if stem in k)
        assert len(inst) == 2 and any(stem + "IdE" in k for k in inst) and any(stem + "IfE" in k for k in inst), (stem, list(fns))
    # kernels only: a device function left out of line (the solver's feed() once was) brings a stack frame, i.e. scratch
    assert len(fns) == 4 and all(d is not None for _, d in fns.values()), list(fns)
    for k, (body, _) in fns.items():
        assert "s_swappc" not in body and "s_call" not in body, k


def test_no_scratch(batch_asm):
    for k, (body, d) in _functions(batch_asm).items():
        assert int(d["private_segment_fixed_size"]) == 0, (k, d["private_segment_fixed_size"])
        assert "scratch_" not in body and "buffer_store" not in body and "buffer_load" not in body, k


def test_block_shape_one_wave_per_simd(batch_asm):
    """__launch_bounds__(256, 1): the register budget of joint_reduce_kernel (512 unified registers, more than 256 in use),
    the flat work-group size in the metadata."""
    sizes = {name: int(size) for size, name in re.findall(r"\.max_flat_workgroup_size:\s*(\d+)\s*\n\s*\.name:\s*(\S+)", batch_asm)}
    for k, (_, d) in _functions(batch_asm).items():
        assert sizes.get(k) == 256, (k, sizes)
        total = int(d["next_free_vgpr"])
        assert 256 < total <= 512, (k, total)


def test_f64_instances_stream_with_16_byte_accesses(batch_asm):
    for k, (body, _) in _functions(batch_asm).items():
        if "kernelIdE" in k:
            assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, k


def test_the_device_loop_keeps_its_barriers_at_depth_one(batch_asm):
    """batch_joint_solve_kernel: B0, B1, one barrier inside either fold, one after the loop -- five, none duplicated into a
    private copy of the loop for thread 0."""
    for k, (body, _) in _functions(batch_asm).items():
        if "batch_joint_solve_kernel" in k:
            assert body.count("s_barrier") == 5, (k, body.count("s_barrier"))


def test_single_problem_file_still_yields_its_five_scratch_free_kernels(single_asm):
    fns = _functions(single_asm)
    for stem in ("joint_reduce_kernel", "joint_step_kernel"):
        inst = sorted(k for k in fns if stem in k)
        assert len(inst) == 2 and any("IdE" in k for k in inst) and any("IfE" in k for k in inst), (stem, list(fns))
    assert sum("joint_finalize_kernel" in k for k in fns) == 1
    assert len(fns) == 5, list(fns)
    for k, (body, d) in fns.items():
        assert d is not None and int(d["private_segment_fixed_size"]) == 0, k
        assert "scratch_" not in body and "buffer_store" not in body, k
        if "IdE" in k:
            assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, k
            assert not re.search(r"global_load_(dword|dwordx2|dwordx3)\b", body), k
