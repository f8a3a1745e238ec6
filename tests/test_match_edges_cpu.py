"""CPU: the qualification of the match-edge suite (tests/match_edges.py, tests/match_edges_reference.py) with the references alone,
the host step logic (csrc/sba_depth_solver.hpp, csrc/sba_joint_solver.hpp, csrc/sba_lm.hpp through their CPU harnesses) on the same
scenes, and the exact scene against integer arithmetic.

The table of measured errors in match_edges_reference.py is recomputed here, kind by kind: float64 numpy may not exceed 1/8 of any
stored bound (the stored figure IS an eighth of the bound), the class of every (kind, pass) must be the stored one, every (kind,
pass) has exactly one entry, and no combination drops more than CAP of its edge rows."""
from fractions import Fraction

import numpy as np
import pytest

import match_edges as me
import match_edges_reference as mr
from helpers import harness_solve


def test_every_kind_and_pass_has_exactly_one_entry():
    want = {(k, p) for k in mr.table_kinds() for p in mr.PASSES}
    assert set(mr.TABLE) == want, (want - set(mr.TABLE), set(mr.TABLE) - want)
    assert set(mr.EXACT_TABLE) == {(k, p) for k in me.RESIDUAL for p in mr.EXACT_PASSES}
    assert {c.name for c in me.CASES} == set(me.KINDS) | set(me.RESIDUAL) and len(me.BY_NAME) == len(me.CASES)
    for (kind, pas), (cls, err, flat) in mr.TABLE.items():
        assert cls in ("bound", "non_finite"), (kind, pas, cls)          # `refused`: no case of this suite is refused
        assert np.isfinite(err) and err >= 0, (kind, pas)
    assert set(mr.EXACT_TABLE.values()) == {"exact"}
    # what must be singular is, and nothing else
    nf = {k for k, v in mr.TABLE.items() if v[0] == "non_finite"}
    assert nf == {(k, "eval_joint_inf") for k in me.PARALLEL_KINDS} | {(k, "solve_joint_1e16") for k in me.PARALLEL_KINDS} | \
        {("far_parallel", "depth_1e16")}, nf


def test_the_scenes_hold_what_they_say():
    for kind in me.KINDS:
        for c in me.scenes(kind):
            s2 = me.sin2(c)[c.rows]
            if kind in me.PARALLEL_KINDS:
                assert (s2 < 1e-30).all(), (c.name, s2.max())
            elif kind in me.WEAK:
                assert np.allclose(s2, me.WEAK[kind], rtol=1e-6 if kind != "weak_1e-14" else 0.2), (c.name, s2)
            if kind == "negative_zero":
                assert np.signbit(c.x1[c.rows]).sum() == 2 * len(c.rows)
            if kind in me.LENGTH:
                assert np.allclose(np.linalg.norm(c.x1[c.rows], axis=1), me.LENGTH[kind])
            base = me.scene("ordinary", c.pose, len(c.x1), c.rep)
            other = np.setdiff1d(np.arange(len(c.x1)), c.rows)
            assert np.array_equal(c.x1[other], base.x1[other]) and np.array_equal(c.d12[other], base.d12[other])
    assert [int(i) for i in me.rows(513)[[0, 1]]] == [0, 1] and {126, 127, 128, 510, 511, 512} <= set(me.rows(513).tolist())
    assert {510, 511, 512, 513, 4098} <= set(me.rows(4099).tolist())
    for g in me.BATCH_EDGE_PAIRS:
        assert me.BATCH_SIZES[g] % 2 == 1                      # the padding partner is an edge row's


@pytest.mark.parametrize("kind", mr.table_kinds())
def test_drop_cap(kind):
    """No combination drops more than CAP of its edge rows (qualified asserts it), a dropped row is named with its reason, and the
    qualified scene has no row left whose class cannot be demanded."""
    total = 0
    for key in mr.combos(kind):
        c, dropped = mr.qualified(*key)
        assert len(dropped) <= mr.CAP * me.N_EDGE
        assert all(i in c.rows and reason for i, reason in dropped.items())
        total += len(dropped)
    print(f"{kind}: {total} rows dropped over {len(mr.combos(kind))} combinations")


@pytest.mark.parametrize("pas", mr.PASSES)
@pytest.mark.parametrize("kind", mr.table_kinds())
def test_the_table_is_reproduced(kind, pas):
    """float64 numpy against long double on the scenes of the kind: the class is TABLE's, and the error does not exceed the stored
    figure, an eighth of the bound the kernels are held to.  The measures themselves assert the conditions the bounds rest on:
    equal outlier counts, equal summaries of the two arithmetics, an invalid first step where the block is singular."""
    cls, err, flat = mr.measure(kind, pas)
    want = mr.TABLE[kind, pas]
    print(f"{kind} {pas}: {cls} {err:.3g} {flat:.3g}; stored {want}")
    assert cls == want[0]
    assert err <= want[1], (kind, pas, err, want[1])
    assert np.isnan(want[2]) or flat <= want[2], (kind, pas, flat, want[2])
    b_abs, b_flat = mr.bound(kind, pas)
    assert b_abs >= 8.0 * mr.TABLE["ordinary", pas][1] and b_abs >= 8.0 * err


def test_exact_scene_against_integer_arithmetic():
    """Every e and s of the exact scene is what float64 numpy computes in any order; the classes at delta^2 and one ulp either side;
    the packs with the loss off are representable and do not depend on the order of the rows."""
    delta = me.EXACT_DELTA
    for n in me.SIZES:
        c, names = me.exact_scene(n)
        e, s, out, _ = me.exact_terms(c, delta)
        e64 = c.d12[:, 1:2] * c.x2 - c.d12[:, 0:1] * c.x1 + c.tran_init
        assert all(Fraction(float(e64[i, k])) == e[i][k] for i in range(n) for k in range(3))
        s64 = e64[:, 0] * e64[:, 0] + e64[:, 1] * e64[:, 1] + e64[:, 2] * e64[:, 2]
        ulp = np.concatenate([names["at_delta_+1ulp"], names["at_delta_-1ulp"]])
        exact_rows = np.setdiff1d(np.arange(n), ulp)
        assert all(Fraction(float(s64[i])) == s[i] for i in exact_rows)
        assert np.array_equal(s64 > delta * delta, out)
        assert (s64[names["at_delta"]] == delta * delta).all() and not out[names["at_delta"]].any()
        assert (s64[names["at_delta_+1ulp"]] == np.nextafter(delta * delta, 1.0)).all() and out[names["at_delta_+1ulp"]].all()
        assert (s64[names["at_delta_-1ulp"]] == np.nextafter(delta * delta, 0.0)).all() and not out[names["at_delta_-1ulp"]].any()
        assert not s64[names["zero"]].any()
        assert 0 < out.sum() < n
        # the same through the references' own blocks, in float64 and long double
        for dt in (np.float64, mr.LD):
            sq, o = mr.classes(c, False, delta, dt)
            assert np.array_equal(o, out)
        c2, _ = me.exact_scene(n, ulp_rows=False)
        _, _, _, packs = me.exact_terms(c2, 0.0)
        perm = np.random.default_rng(n).permutation(n)
        for mode in mr.MODES:
            want = me.exact_floats(packs[mode])
            T = mr.sweep_terms(c2, False, mode, mr.DEPTH_PER_MATCH, 0.0, np.float64)
            assert np.array_equal(T.sum(0)[:23], want[:23]) and np.array_equal(T[perm].sum(0)[:23], want[:23]), mode
            assert np.array_equal(np.cumsum(T, axis=0)[-1][:23], want[:23]), mode


@pytest.mark.parametrize("kind", ["ordinary", "parallel", "far", "far_parallel", "length_1e+3"])
def test_host_lm_on_edge_scenes(kind):
    """csrc/sba_lm.hpp (through tests/harness/lm_harness.cpp) over numpy packs of the kind's scene, MODE_RT with per-match depths:
    the float64 packs and the long-double packs rounded to float64 drive it to the same termination and counts, and to the same
    pose within 1e-9 -- the host solver takes no other path on these scenes than on the ordinary one."""
    c, _ = mr.qualified(kind, "closed", 513, 0, False)

    def evaluator(dt):
        def fn(rot, tran):
            moved = me.Scene(c.x1, c.x2, c.d12, c.rot_true, c.tran_true, rot, tran, c.kind, c.rows, c.name)
            return mr.sweep_terms(moved, False, 2, mr.DEPTH_PER_MATCH, 1.0, dt).sum(0).astype(np.float64)
        return fn
    r64, t64, s64, rc64 = harness_solve(2, c.rot_init, c.tran_init, evaluator(np.float64), tran_param=1)
    rld, tld, sld, rcld = harness_solve(2, c.rot_init, c.tran_init, evaluator(mr.LD), tran_param=1)
    assert rc64 == rcld == 0
    assert (s64.termination, s64.num_iterations, s64.num_successful_steps) == (sld.termination, sld.num_iterations, sld.num_successful_steps)
    assert s64.termination != 6 and s64.final_cost <= s64.initial_cost
    assert np.abs(r64 - rld).max() <= 1e-9 and np.abs(t64 - tld).max() <= 1e-9, (np.abs(r64 - rld).max(), np.abs(t64 - tld).max())


def test_singular_starts_end_as_invalid_steps():
    """The host step logic on the exactly singular block: from radius 1e16 the d-only stage on far_parallel and the joint solve on
    parallel take the first step as invalid (a NaN model, a failed Cholesky factorisation), halve the radius and leave every depth
    as it was -- and go on from there without FAILURE."""
    a = mr.depth_solve("far_parallel", "zero", mr.SOLVE_SIZE, 0, False, 1, False, mr.SINGULAR_RADIUS)
    c = me.scene("far_parallel", "zero", mr.SOLVE_SIZE, 0)
    assert a[3] and a[1] == (4, 1, 0, 2, 0) and a[2] == 0 and np.array_equal(a[0], c.d12)
    for rep in range(me.REPEAT):                 # without the axis row some block is still exactly singular, with either store
        for f32 in (False, True):
            a = mr.depth_solve("far_parallel", "zero", mr.SOLVE_SIZE, rep, f32, 1, False, mr.SINGULAR_RADIUS, axis_row=False)
            assert a[3] and a[1] == (4, 1, 0, 2, 0) and a[2] == 0, (rep, f32, a[1:])
    b = mr.depth_solve("far_parallel", "zero", mr.SOLVE_SIZE, 0, False, 3, False, mr.SINGULAR_RADIUS)
    assert b[1][0] != 6 and b[2] == 0 and np.isfinite(b[0]).all() and (b[0][c.rows] > 0.5 * c.d12[c.rows]).all()
    c = me.scene("parallel", "zero", mr.JOINT_SIZE, 0)
    assert mr.singular_in_float64(c, False, mr.SINGULAR_RADIUS) and not mr.singular_in_float64(c, False, mr.SINGULAR_RADIUS / 2)
    emu, _ = mr.joint_solve("parallel", "zero", mr.JOINT_SIZE, 0, False, mr.SINGULAR_RADIUS, 1)
    assert emu[3] == (4, 1, 0, 2) and emu[4] == 0 and np.array_equal(emu[2], c.d12)
    full, _ = mr.joint_solve("parallel", "zero", mr.JOINT_SIZE, 0, False, mr.SINGULAR_RADIUS, 50)
    assert full[3][0] != 6 and full[4] == 0 and np.isfinite(full[2]).all()


@pytest.mark.parametrize("kind", me.PARALLEL_KINDS)
def test_singular_solves_that_are_a_fair_yardstick(kind):
    """Per store at least SINGULAR_FAIR_MIN whole solves from radius 1e16 end alike in three float64 formulations: on those the
    device is held to the counts."""
    for f32 in (False, True):
        fair = 0
        for key in mr.joint_combos(kind, "solve_joint_1e16"):
            if key[4] == f32:
                _, dropped = mr.qualified(*key)
                fair += mr.singular_solve_is_fair(key, tuple(sorted(dropped)))
        print(f"{kind} f32={f32}: {fair} fair")
        assert fair >= mr.SINGULAR_FAIR_MIN[kind], (kind, f32, fair)
