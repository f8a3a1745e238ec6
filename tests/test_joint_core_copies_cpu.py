"""CPU: the two written-out copies of the joint solve's per-match loops are the same text.

csrc/sba_joint_core.hpp holds the reduce and the step loop as joint_reduce_stream / joint_step_stream (over an address map; the
batched kernels use them).  csrc/sba_joint.hip keeps both loops written out in its kernels, because routed through the functions
they compiled to other last bits and those kernels' results are pinned.  Until that is settled the copies are kept in step by
this test: after the map is taken out of the header's loops (identity: map(x) -> x, the plane index q -> pr) the loop bodies
must be equal token for token."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spherical_bundle_adjuster_amd", "csrc")


def _loop(text, start_marker, end_marker):
    a = text.index(start_marker)
    a = text.index("  while (pr < npairs) {", a)
    b = text.index(end_marker, a)
    return text[a:b]


def _tokens(t):
    t = re.sub(r"//[^\n]*", "", t)
    return re.findall(r"[A-Za-z_]\w*|\d+\.?\d*(?:[eE][-+]?\d+)?|\S", t)


def _identity(t):
    t = t.replace("const size_t pn = pr + stride, q = map(pr);", "const size_t pn = pr + stride;")
    t = t.replace("map(pn)", "pn")
    for plane in ("sc1", "sc2", "c1", "c2"):
        t = t.replace(f"joint_store_pair({plane}, q,", f"joint_store_pair({plane}, pr,")
    assert "map(" not in t
    return t


def test_reduce_and_step_loops_are_the_same_text():
    core = open(os.path.join(CSRC, "sba_joint_core.hpp")).read()
    single = open(os.path.join(CSRC, "sba_joint.hip")).read()
    pairs = (("joint_reduce_stream(", "joint_reduce_kernel("), ("joint_step_stream(", "joint_step_kernel("))
    for in_core, in_single in pairs:
        a = _identity(_loop(core, "void " + in_core, "\n}\n"))
        b = _loop(single, "void " + in_single, "  joint_block_fold<")
        ta, tb = _tokens(a), _tokens(b)
        assert len(ta) > 300, (in_core, len(ta))          # the loops were found, not an empty match
        diff = next((i for i, (x, y) in enumerate(zip(ta, tb)) if x != y), None)
        assert ta == tb, (in_core, diff, ta[diff - 5:diff + 5] if diff is not None else (len(ta), len(tb)),
                          tb[diff - 5:diff + 5] if diff is not None else None)


def test_single_problem_kernels_use_the_shared_block_and_fold():
    """What is NOT copied: the per-match block, the plane accesses and the block fold exist once, in the header."""
    single = open(os.path.join(CSRC, "sba_joint.hip")).read()
    core = open(os.path.join(CSRC, "sba_joint_core.hpp")).read()
    assert '#include "sba_joint_core.hpp"' in single
    for name in ("struct JointBlock", "void joint_block(", "struct JointRegs", "struct JPair", "void joint_block_fold("):
        assert name in core and name not in single, name
