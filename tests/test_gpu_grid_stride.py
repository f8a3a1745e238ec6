"""GPU: the grid-stride loops of the single-problem kernels against the oracle where their lanes run 1, 2 and more steps.

sweep_kernel, depth_step_kernel (depth_stream, one or two steps of loads in flight), epipolar_moments_kernel (two vectors
ahead) and fold_depths_kernel size their grid to one resident wave of blocks and stride over the rest.  At the problem
sizes of the other files every lane runs one step, so the second and later steps, the prefetch hand-overs and the last
lane's ragged tail never run under a check.  Here the launch geometry is forced small (SBA_BLOCKS_PER_CU,
SBA_DEPTH_BLOCKS_PER_CU, SBA_EPI_BLOCKS_PER_CU: read at handle creation or per call) and the sizes are derived from the
device's CU count with each launcher's own formula, so that the item count lands on k * stride - 1, k * stride and
k * stride + 1 for k = 1, 2, 3.  Tolerances are the suite's (helpers.py)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import REL_TOL_F64, ROOT, assert_normal_eq_close
from spherical_bundle_adjuster_amd import api, synthetic

pytestmark = pytest.mark.gpu

BLOCK = 256              # threads per block of all four kernels (sba_device.hpp kBlock; the depth, epipolar and fold launches)
SWEEP_MAX_PER_CU = 8     # sba_problem_create: max_grid = num_cus * 8; SBA_BLOCKS_PER_CU admits 1 .. 8
FOLD_PER_CU = 8          # ensure_folded (sba_shim.cpp): launch_fold_depths(..., num_cus * 8)
DEPTH_DEFAULT_CAP = 8    # sba_problem_solve_depths: blocks per CU = min(occupancy, 8) unless SBA_DEPTH_BLOCKS_PER_CU
EPI_DEFAULT_PER_CU = 2   # sba_problem_epipolar_moments: two blocks per CU unless SBA_EPI_BLOCKS_PER_CU
STEPS = (1, 2, 3)
OFFSETS = (-1, 0, 1)
# Per-match depths after one accepted step / after two.  The second step solves each match's damped 2 x 2 system at depths
# that already carry the first step's rounding, amplified by that system's condition: two independent f64 restatements
# (the oracle and tests/ref_depth_numpy.py) differ by 4.6e-13 after one step and 1.9e-12 after two at 131 070 matches.
# A wrong Jacobi scale, a stale or missing candidate moves a depth by O(1).
DEPTH_REL = (1e-12, 1e-11)
DEPTH_SOLVE_TOL = 1e-9   # full solves (test_depth_stage_matches_oracle)
TERMINATION = {1: "CONVERGENCE_FUNCTION", 2: "CONVERGENCE_GRADIENT", 3: "CONVERGENCE_PARAMETER", 4: "NO_CONVERGENCE"}


# ---- launch geometry -------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def _counts(kernel, n, ppt):
    """(items the grid is sized for, items the grid-stride loop runs over) of a launch over n matches."""
    if kernel == "sweep":        # grid_for (sba_shim.cpp): whole vectors of ppt matches; the ragged vector is the tail lane's
        return _cdiv(n, ppt), n // ppt
    if kernel in ("depth", "epi"):   # depth_stream / epipolar_moments_kernel: pairs of matches, f64 and f32 planes alike
        return (n + 1) // 2, (n + 1) // 2
    if kernel == "fold":         # launch_fold_depths: the whole allocation, (n rounded up to a vector) + one spare vector
        return _cdiv(n, 2) + 1, _cdiv(n, 2) + 1
    raise ValueError(kernel)


def geometry(kernel, n, cus, per_cu, ppt=2):
    """(grid, stride, steps): the grid its launcher picks for n matches at `per_cu` resident blocks per CU, the stride of
    the loop in items, and the most loop trips a lane makes."""
    sized, looped = _counts(kernel, n, ppt)
    cap = cus * (min(per_cu, SWEEP_MAX_PER_CU) if kernel == "sweep" else per_cu)
    grid = min(_cdiv(sized, BLOCK), cap)
    stride = grid * BLOCK
    return grid, stride, (_cdiv(looped, stride) if grid else 0)


def pick_n(kernel, cus, per_cu, k, off, rem=0, ppt=2):
    """n whose loop count is k * stride + off at the capped grid.  rem: for the sweep the matches of the ragged vector
    (0 .. ppt-1), for the pair kernels 1 = a half-filled last pair.  Asserts the launcher gives the intended step count."""
    stride = cus * per_cu * BLOCK
    items = k * stride + off
    if kernel == "sweep":
        assert 0 <= rem < ppt
        n = items * ppt + rem
    elif kernel in ("depth", "epi"):
        assert rem in (0, 1)
        n = 2 * items - rem
    else:
        assert rem in (0, 1)
        n = 2 * (items - 1) - rem
    grid, got_stride, steps = geometry(kernel, n, cus, per_cu, ppt)
    assert (grid, got_stride, steps) == (cus * per_cu, stride, _cdiv(items, stride)), (kernel, n, grid, steps)
    return n


@functools.lru_cache(maxsize=1)
def device_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=3)
def _case(n, seed):
    return synthetic.full_rt(n, seed=seed, outlier_fraction=0.1)


def _inputs(c, store):
    """What the planes hold: f32 planes are the f32-rounded inputs (the oracle is fed the same)."""
    if store == api.STORE_F64:
        return c.x1, c.x2
    return c.x1.astype(np.float32).astype(np.float64), c.x2.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("cus", [None, 1, 80, 256, 304])
def test_chosen_sizes_give_the_intended_step_counts(cus):
    """The size helper against the launchers' formulas: k * stride +- 1 straddles a step boundary, every kernel reaches
    1, 2, 3 and 4 steps, and the ragged or half-filled tails do not change the step count."""
    cus = cus or device_cus()
    for kernel, per_cus, ppts, rems in (("sweep", (1, 8), (2, 4), None), ("depth", (1, 8), (2,), (0, 1)),
                                        ("epi", (1, 2), (2,), (0, 1)), ("fold", (FOLD_PER_CU,), (2,), (0, 1))):
        for per_cu in per_cus:
            for ppt in ppts:
                seen = set()
                for k in STEPS:
                    for off in OFFSETS:
                        for rem in (rems or range(ppt)):
                            n = pick_n(kernel, cus, per_cu, k, off, rem, ppt)
                            steps = geometry(kernel, n, cus, per_cu, ppt)[2]
                            assert steps == (k + 1 if off > 0 else k)
                            seen.add(steps)
                assert seen == {1, 2, 3, 4}, (kernel, per_cu, ppt)
    # below one capped grid the grid shrinks and every lane runs one step
    assert geometry("sweep", 1001, cus, SWEEP_MAX_PER_CU) == (2, 2 * BLOCK, 1)
    assert geometry("fold", 1, cus, FOLD_PER_CU) == (1, BLOCK, 1)


# ---- sweep -----------------------------------------------------------------------------------------------------------
MODES = (api.MODE_ROT, api.MODE_TRAN, api.MODE_RT)
KINDS = (api.KERNEL_FACTORED, api.KERNEL_EXPLICIT)
D1, D2 = 1.3, 0.9


def _check_sweeps(oracle, p, c, store, delta, forms, what):
    """Every mode, both kernel kinds, in each depth form against oracle.evaluate on the planes' inputs.
    forms: "uniform", "folded" (per-match depths over the folded planes), "raw" (per-match over the 8 raw planes)."""
    x1, x2 = _inputs(c, store)
    for mode in MODES:
        refs = {}
        for form in forms:
            dm = api.DEPTH_UNIFORM if form == "uniform" else api.DEPTH_PER_MATCH
            if dm not in refs:
                refs[dm] = oracle.evaluate(mode, x1, x2, c.rot_init, c.tran_init, D1, D2, delta,
                                           None if dm == api.DEPTH_UNIFORM else c.d12)
            ref = refs[dm]
            p.set_folding(form != "raw")
            for kind in KINDS:
                p.set_kernel(kind)
                got = p.eval(mode, c.rot_init, c.tran_init, D1, D2, delta, dm)
                tag = f"{what} mode={mode} {form} kind={kind} delta={delta}"
                assert_normal_eq_close(got, ref, REL_TOL_F64, tag)
                assert got.n_outlier == ref.n_outlier, tag
                assert mode == api.MODE_ROT or abs(got.sum_w - ref.sum_w) <= REL_TOL_F64 * max(ref.sum_w, 1), tag
    p.set_folding(True)
    p.set_kernel(api.KERNEL_FACTORED)


@pytest.mark.parametrize("store", [api.STORE_F64, api.STORE_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("k", STEPS)
def test_sweep_steps_match_the_oracle(oracle, monkeypatch, k, store):
    """One block per CU: the loop runs k (off <= 0) or k + 1 steps; the ragged vector (n % ppt != 0) goes to the last lane
    of a grid capped below what the problem wants.  Huber on and off alternate over the offsets."""
    monkeypatch.setenv("SBA_BLOCKS_PER_CU", "1")
    cus = device_cus()
    ppt = 2 if store == api.STORE_F64 else 4
    for i, off in enumerate(OFFSETS):
        rem = (k + i) % 2 if store == api.STORE_F64 else (k + i) % 4 or 1
        n = pick_n("sweep", cus, 1, k, off, rem, ppt)
        c = _case(n, 5000 + n)
        delta = 1.0 if (k + i) % 2 else 0.0
        forms = ("uniform", "folded", "raw") if store == api.STORE_F64 else ("uniform", "raw")
        with api.Problem(0) as p:
            p.upload(c.x1, c.x2, c.d12, store=store)
            _check_sweeps(oracle, p, c, store, delta, forms, f"n={n} k={k} off={off}")


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("per_cu", ["1", "8"])
def test_sweep_reductions_over_many_steps(oracle, monkeypatch, fused, per_cu):
    """Both final reductions (finalize kernel / the last block's fold) after a multi-step sweep; at 8 blocks per CU --
    the largest cap; the occupancy may admit fewer, which only adds steps -- the fold runs over the largest grid."""
    monkeypatch.setenv("SBA_BLOCKS_PER_CU", per_cu)
    monkeypatch.setenv("SBA_FUSED", fused)
    cus = device_cus()
    n = pick_n("sweep", cus, int(per_cu), 2, 1, 1)          # >= 3 steps at any admitted occupancy
    c = _case(n, 5100)
    ref = oracle.evaluate(api.MODE_RT, c.x1, c.x2, c.rot_init, c.tran_init, d12=c.d12)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12)
        got = p.eval(api.MODE_RT, c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH)
        assert_normal_eq_close(got, ref, REL_TOL_F64, f"n={n} fused={fused} per_cu={per_cu}")
        assert got.n_outlier == ref.n_outlier
        pack = p.eval_pack(api.MODE_RT, c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH)
        assert np.array_equal(pack, p.eval_pack(api.MODE_RT, c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH))
        if fused == "0":     # the other modes and the uniform form at the largest grid too
            for mode in (api.MODE_ROT, api.MODE_TRAN):
                for dm, d12 in ((api.DEPTH_UNIFORM, None), (api.DEPTH_PER_MATCH, c.d12)):
                    r = oracle.evaluate(mode, c.x1, c.x2, c.rot_init, c.tran_init, D1, D2, 1.0, d12)
                    g = p.eval(mode, c.rot_init, c.tran_init, D1, D2, 1.0, dm)
                    assert_normal_eq_close(g, r, REL_TOL_F64, f"n={n} per_cu={per_cu} mode={mode} dm={dm}")
                    assert g.n_outlier == r.n_outlier


# ---- d-only grid kernel (shared with the AHEAD=2 child process below) ------------------------------------------------
def _depth_n(cus, per_cu, k, off, store):
    """Pair-boundary sizes; f32 planes: n % 4 in {1, 2, 3} (the last 16-byte vector partly filled)."""
    if store == api.STORE_F64:
        rem = (k + off) % 2
    else:
        rem = {-1: 1, 0: 1, 1: 0}[off]         # with an even stride: n % 4 = 1, 3, 2
    n = pick_n("depth", cus, per_cu, k, off, rem)
    assert store == api.STORE_F64 or n % 4 != 0
    assert n > 4096, n        # above one_launch_max_n_depth / resident_max_n_depth: the grid kernel runs
    return n


def check_depth_first_steps(oracle, n, store, setenv=None):
    """max_num_iterations = 1 and 2, one accepted step each: every per-match depth within DEPTH_REL of the oracle's
    (pass 1 writes every lane's candidate and the Jacobi-scale planes; pass 2 reads those back).  With setenv: also with
    non-temporal candidate stores (SBA_DEPTH_NT_STORES, read per call) -- the same bits and summary."""
    c = _case(n, 6000 + n)
    x1, x2 = _inputs(c, store)
    d0 = np.full((n, 2), 3.0)
    for max_it in (1, 2):
        opts = dict(max_num_iterations=max_it)
        dref, sref, rc = oracle.depth_solve(x1, x2, c.rot_init, c.tran_init, d0, options=oracle.default_options(**opts))
        assert rc == 0 and sref.num_successful_steps == max_it, (n, max_it, sref.num_successful_steps)
        runs = []
        for nt in (("0", "1") if setenv else (None,)):
            if nt is not None:
                setenv("SBA_DEPTH_NT_STORES", nt)
            with api.Problem(0) as p:
                p.upload(c.x1, c.x2, d0, store=store)
                runs.append(p.solve_depths(c.rot_init, c.tran_init, options=api.default_lm_options(**opts)))
        d, s = runs[0]
        assert (s.num_iterations, s.num_successful_steps, s.num_line_search_steps) == \
            (sref.num_iterations, sref.num_successful_steps, sref.num_line_search_steps), (n, max_it)
        err = (np.abs(d - dref) / np.maximum(1.0, np.abs(dref))).max()
        assert err <= DEPTH_REL[max_it - 1], f"n={n} store={store} max_it={max_it}: depth rel err {err:.3e}"
        for d_nt, s_nt in runs[1:]:
            assert np.array_equal(d_nt, d), (n, max_it, "non-temporal stores")
            assert (s_nt.num_iterations, s_nt.num_successful_steps, s_nt.num_line_search_steps, s_nt.initial_cost,
                    s_nt.final_cost, s_nt.termination) == \
                (s.num_iterations, s.num_successful_steps, s.num_line_search_steps, s.initial_cost, s.final_cost,
                 s.termination), (n, max_it)


def check_depth_solve(oracle, n, store):
    """A full d-only solve: iteration, accepted-step and line-search counts and termination equal, depths to 1e-9."""
    c = _case(n, 6100 + n)
    x1, x2 = _inputs(c, store)
    d0 = np.full((n, 2), 3.0)
    dref, sref, rc = oracle.depth_solve(x1, x2, c.rot_init, c.tran_init, d0)
    assert rc == 0
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, d0, store=store)
        d, s = p.solve_depths(c.rot_init, c.tran_init)
    assert (s.num_iterations, s.num_successful_steps, s.num_line_search_steps) == \
        (sref.num_iterations, sref.num_successful_steps, sref.num_line_search_steps), n
    assert s.termination == TERMINATION[sref.termination]
    assert np.abs(d - dref).max() <= DEPTH_SOLVE_TOL * max(1.0, np.abs(dref).max()) and (d >= 0).all()
    assert abs(s.final_cost - sref.final_cost) <= 1e-10 * sref.final_cost


@pytest.mark.parametrize("store", [api.STORE_F64, api.STORE_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("k", STEPS)
def test_depth_first_steps_match_the_oracle(oracle, monkeypatch, k, store):
    monkeypatch.setenv("SBA_DEPTH_BLOCKS_PER_CU", "1")
    cus = device_cus()
    for off in OFFSETS:
        check_depth_first_steps(oracle, _depth_n(cus, 1, k, off, store), store, monkeypatch.setenv)


@pytest.mark.parametrize("k,off,store", [(2, 1, api.STORE_F64), (3, -1, api.STORE_F64), (2, 0, api.STORE_F32)],
                         ids=["f64-3steps", "f64-3steps-full", "f32-2steps"])
def test_depth_solves_match_the_oracle(oracle, monkeypatch, k, off, store):
    monkeypatch.setenv("SBA_DEPTH_BLOCKS_PER_CU", "1")
    check_depth_solve(oracle, _depth_n(device_cus(), 1, k, off, store), store)


def test_depth_default_cap(oracle, monkeypatch):
    """The default cap (min(occupancy, 8) blocks per CU): n past two grids even at 8 blocks per CU."""
    monkeypatch.delenv("SBA_DEPTH_BLOCKS_PER_CU", raising=False)
    check_depth_first_steps(oracle, _depth_n(device_cus(), DEPTH_DEFAULT_CAP, 2, 1, api.STORE_F64), api.STORE_F64)


def ahead2_child(cus):
    """Run in a fresh process with SBA_DEPTH_AHEAD=2 (read once per process): the checks above at the boundaries of the
    two-steps-ahead loop.  An assertion ends the process with a non-zero status."""
    from oracle import oracle_py as oracle
    oracle.lib()
    ok = 0
    for store in (api.STORE_F64, api.STORE_F32):
        for k in STEPS:
            for off in OFFSETS:
                if store == api.STORE_F32 and off != 1 and k != 2:
                    continue          # f32: every offset at k = 2, the first-step-past-the-boundary size elsewhere
                n = _depth_n(cus, 1, k, off, store)
                check_depth_first_steps(oracle, n, store, os.environ.__setitem__ if k == 2 else None)
                ok += 1
                print(f"AHEAD=2 first steps ok: n={n} store={store} k={k} off={off}", flush=True)
    n = _depth_n(cus, 1, 2, 1, api.STORE_F64)
    check_depth_solve(oracle, n, api.STORE_F64)
    print(f"AHEAD=2 full solve ok: n={n}; {ok} first-step sizes", flush=True)


def test_depth_two_steps_ahead_in_a_child_process():
    cus = device_cus()
    env = dict(os.environ, SBA_DEPTH_AHEAD="2", SBA_DEPTH_BLOCKS_PER_CU="1")
    env.pop("SBA_DEPTH_NT_STORES", None)
    code = ("import sys; sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']; "
            "import test_gpu_grid_stride as t; t.ahead2_child(int(sys.argv[2]))")
    r = subprocess.run([sys.executable, "-c", code, str(ROOT), str(cus)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, f"child exited {r.returncode}\n{r.stdout}\n{r.stderr}"
    assert r.stdout.count("first steps ok") == 14 and "full solve ok" in r.stdout, r.stdout
    print(r.stdout)


# ---- epipolar moments ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_cu", [1, None], ids=["1-per-cu", "default"])
@pytest.mark.parametrize("k", STEPS)
def test_epipolar_moments_steps(monkeypatch, k, per_cu):
    """Two vectors ahead: q + stride < nvec (nx1) and q + 2 stride < nvec (nx2) flip at these sizes.  numpy reference in
    long double (the 64 group sums run over up to 12 k matches each)."""
    from test_initial_guess_cpu import group_moments
    if per_cu is None:
        monkeypatch.delenv("SBA_EPI_BLOCKS_PER_CU", raising=False)
    else:
        monkeypatch.setenv("SBA_EPI_BLOCKS_PER_CU", str(per_cu))
    cus = device_cus()
    for i, off in enumerate(OFFSETS):
        store = (api.STORE_F64, api.STORE_F32)[(k + i) % 2]
        n = pick_n("epi", cus, per_cu or EPI_DEFAULT_PER_CU, k, off, rem=i % 2)
        c = _case(n, 7000 + n)
        x1, x2 = _inputs(c, store)
        ref, _, _ = group_moments(x1.astype(np.longdouble), x2.astype(np.longdouble))
        with api.Problem(0) as p:
            p.upload(c.x1, c.x2, store=store)
            got = p.epipolar_moments()
            assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (n, store, np.abs(got - ref).max())
            assert np.array_equal(got, p.epipolar_moments())


# ---- fold kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,off,rem", [(2, -1, 0), (2, 0, 1), (2, 1, 0), (3, 1, 1)])
def test_folded_planes_past_one_fold_grid(oracle, k, off, rem):
    """fold_depths_kernel strides over num_cus * 8 blocks: the per-match sweep over its output against the oracle."""
    n = pick_n("fold", device_cus(), FOLD_PER_CU, k, off, rem)
    c = _case(n, 8000 + n)
    ref = oracle.evaluate(api.MODE_RT, c.x1, c.x2, c.rot_init, c.tran_init, d12=c.d12)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12)
        for kind in KINDS:
            p.set_kernel(kind)
            got = p.eval(api.MODE_RT, c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH)
            assert_normal_eq_close(got, ref, REL_TOL_F64, f"n={n} kind={kind}")
            assert got.n_outlier == ref.n_outlier


# ---- plane layout ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stagger", ["0", "1048576"])
def test_plane_stagger_extremes(oracle, monkeypatch, stagger):
    """SBA_PLANE_STAGGER (read at handle creation) moves every plane, folded ones included: a multi-step fold, sweep and
    d-only pass at no stagger and at the largest."""
    monkeypatch.setenv("SBA_PLANE_STAGGER", stagger)
    monkeypatch.setenv("SBA_BLOCKS_PER_CU", "1")
    monkeypatch.setenv("SBA_DEPTH_BLOCKS_PER_CU", "1")
    cus = device_cus()
    n = pick_n("fold", cus, FOLD_PER_CU, 2, 1, 1)
    assert geometry("sweep", n, cus, 1)[2] >= 4
    c = _case(n, 8000 + n)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12)
        _check_sweeps(oracle, p, c, api.STORE_F64, 1.0, ("uniform", "folded"), f"stagger={stagger} n={n}")
    check_depth_first_steps(oracle, _depth_n(cus, 1, 2, 1, api.STORE_F64), api.STORE_F64)
