"""CPU: the joint solve's per-match source exists once.

csrc/sba_joint_core.hpp holds the per-match block, the plane accesses and the block fold; each of the two per-match loops (reduce,
step) is one include file, csrc/sba_joint_reduce_loop.inc / csrc/sba_joint_step_loop.inc, that the header's stream functions (for
the batched kernels) and the single-problem kernels of csrc/sba_joint.hip both expand.  No file keeps a copy of its own."""
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spherical_bundle_adjuster_amd", "csrc")
LOOPS = ("sba_joint_reduce_loop.inc", "sba_joint_step_loop.inc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_single_problem_kernels_use_the_shared_block_and_fold():
    """The per-match block, the plane accesses and the block fold exist once, in the header; sba_joint.hip has no per-match
    loop and no joint_block() call of its own: it expands the two loop files, once each."""
    single = _read("sba_joint.hip")
    core = _read("sba_joint_core.hpp")
    assert '#include "sba_joint_core.hpp"' in single
    for name in ("struct JointBlock", "void joint_block(", "struct JointRegs", "struct JPair", "void joint_block_fold("):
        assert name in core and name not in single, name
    assert "while (pr < npairs)" not in single and "joint_block(" not in single
    for inc in LOOPS:
        assert single.count(f'#include "{inc}"') == 1 and core.count(f'#include "{inc}"') == 1, inc


def test_each_loop_body_is_defined_in_exactly_one_file():
    """Each loop file holds one loop over a lane's pairs of matches with one joint_block() call, and the statement that marks
    the reduce body (the Schur accumulation) and the one that marks the step body (the candidate's cost) occur once in all the
    library's sources: in their loop file."""
    marks = {"sba_joint_reduce_loop.inc": "acc[JOINT_OUT_S + k] +=", "sba_joint_step_loop.inc": "acc[JOINT_STEP_CAND_COST] ="}
    sources = [p for pat in ("*.hip", "*.hpp", "*.cpp", "*.inc") for p in glob.glob(os.path.join(CSRC, pat))]
    assert len(sources) > 20                                    # the sources were found
    for inc, mark in marks.items():
        text = _read(inc)
        assert text.count("while (pr < npairs)") == 1 and text.count("joint_block(") == 1, inc
        assert [os.path.basename(p) for p in sources if mark in open(p).read()] == [inc], mark
