"""GPU (-m gpu): the drivers of the batched per-pair LM (sba_batch_solve) against one another and against two references.

With one block per pair the default driver is the HYBRID: batch_lm_kernel runs at most SBA_BATCH_LM_FIRST_SWEEPS sweeps of
every pair and hands the pairs that need more -- LmSolver, depths, next sweep state, factored frame -- over to the launches
with dynamic shares (batch_sweep_dyn_kernel -> batch_lm_dyn_feed_kernel -> batch_dyn_compact_kernel).  The baseline of every
comparison here is the one-launch kernel run to the end (SBA_BATCH_DYNAMIC=0, one block per pair); it is held against the
oracle's LM and the independent numpy LM (tests/ref_lm_numpy.py), so that the drivers cannot all agree and all be wrong."""
import numpy as np
import pytest

import ref_lm_numpy as rl
from helpers import RT_TOL_F32, RT_TOL_F64, make_pairs
from spherical_bundle_adjuster_amd import api, synthetic

pytestmark = pytest.mark.gpu

# (name, mode, depth mode, translation parameterisation): the three stages of the pipeline's shape
STAGES = [("rot", api.MODE_ROT, api.DEPTH_UNIFORM, api.TRAN_FREE),
          ("tran", api.MODE_TRAN, api.DEPTH_PER_MATCH, api.TRAN_FREE),
          ("rt", api.MODE_RT, api.DEPTH_PER_MATCH, api.TRAN_SPHERE)]
KINDS = [(api.KERNEL_FACTORED, "factored"), (api.KERNEL_EXPLICIT, "explicit")]
TERM_NUMPY = {"CONVERGENCE_FUNCTION": "function", "CONVERGENCE_GRADIENT": "gradient", "CONVERGENCE_PARAMETER": "parameter",
              "NO_CONVERGENCE": "no_convergence", "MIN_RADIUS": "min_radius"}
EXACT = (0, 9)                 # noise-free pairs started at their exact answer: done at the first evaluation
NEAR = 3                       # a noise-free pair started 1e-12 off its answer: done at the second evaluation
ORACLE_SAMPLE = (4, 6, 11, 14, 20, 29, 38)
NUMPY_PAIR = 4


def _exact_pair(n, seed):
    """A noise-free pair whose residuals vanish at its truth in f64 AND f32 planes: dyadic coordinates (exact in float),
    R = 90 degrees about z (a permutation), t = e_z, unit depths.  Started at the truth, the gradient is at rounding level
    (sin / cos of pi/2), so the solver stops at its first evaluation."""
    rng = np.random.default_rng(seed)
    x1 = rng.integers(-16, 17, (n, 3)) / 8.0
    x1[np.abs(x1).sum(axis=1) == 0] = (0.5, 0.25, 1.0)
    t = np.array([0.0, 0.0, 1.0])
    x2 = np.stack([-x1[:, 1], x1[:, 0], x1[:, 2]], axis=1) - t
    rot = np.array([0.0, 0.0, np.pi / 2])
    return synthetic.Correspondences(x1, x2, np.ones((n, 2)), rot, t, rot.copy(), t.copy())


def _lm_batch(poor="third", seed0=7700):
    """The pair mix of the hand-over tests: 260 pairs, at least one per CU, so one block per pair (config C5's regime).  An
    empty, a 1-match and a 2-match pair, ragged tails (63 / 65 / 1023), two pairs started at their exact answer (EXACT: one
    evaluation), one started 1e-12 off it (NEAR: two), ordinary starts perturbed by 0.5 ... 12 degrees, and poor starts
    that need many more sweeps than any cap, for a third of the pairs (poor="third") or for two only (poor="two", whose
    ordinary starts stay within 5 degrees, so that the two poor ones are the last ones iterating).  Poor starts per stage:
    rot_true + 0.25 (ROT); the translation 3 away along a random axis (TRAN); on the sphere, the translation flipped
    (-tran_true, tilted by 0.3) or the rotation 1.2 off, in turn (RT).  Start values per stage: data["start"][name]."""
    sizes = [300, 0, 1, 257, 700, 64, 1023, 2, 65, 333] + [100 + (37 * g) % 401 for g in range(250)]     # >= 1 pair per CU
    cs, off, x1, x2, d12 = make_pairs(sizes, seed0=seed0)
    for g in EXACT + (NEAR,):
        c = _exact_pair(sizes[g], (seed0, g))
        cs[g] = c
        lo, hi = int(off[g]), int(off[g + 1])
        x1[lo:hi], x2[lo:hi], d12[lo:hi] = c.x1, c.x2, c.d12
    B = len(sizes)
    rot0 = np.stack([c.rot_init for c in cs]); tran0 = np.stack([c.tran_init for c in cs])
    rot0[NEAR] += (1e-12, -2e-12, 1.5e-12)
    tran0[NEAR] += (-1e-12, 1e-12, 0.0)
    degs = (0.5, 2.0, 5.0, 12.0) if poor == "third" else (0.5, 2.0, 5.0)
    for g in range(10, B):                                     # spread the sweeps the ordinary starts need
        axis = np.random.default_rng((seed0, g, 1)).standard_normal(3)
        rot0[g] = cs[g].rot_true + np.deg2rad(degs[g % len(degs)]) * axis / np.linalg.norm(axis)
    poor_idx = [g for g in range(10, B) if g % 3 == 2] if poor == "third" else [14, 41]
    tran0_tran, rot0_rt, tran0_rt = tran0.copy(), rot0.copy(), tran0.copy()
    for k, g in enumerate(poor_idx):
        rot0[g] = cs[g].rot_true + 0.25
        axis = np.random.default_rng((seed0, g, 2)).standard_normal(3)
        axis /= np.linalg.norm(axis)
        tran0_tran[g] = cs[g].tran_true + 3.0 * axis
        if k % 2 == 0:
            rot0_rt[g] = rot0[g]
            tran0_rt[g] = (0.3 * axis - cs[g].tran_true) / np.linalg.norm(0.3 * axis - cs[g].tran_true)
        else:
            rot0_rt[g] = cs[g].rot_true + 1.2
    d1 = np.linspace(0.9, 1.4, B); d2 = np.linspace(1.2, 0.8, B)      # uniform depths: every pair its own
    d1[list(EXACT + (NEAR,))] = 1.0; d2[list(EXACT + (NEAR,))] = 1.0
    return dict(sizes=sizes, cs=cs, off=off, x1=x1, x2=x2, d12=d12, d1=d1, d2=d2,
                start={"rot": (rot0, tran0), "tran": (rot0, tran0_tran), "rt": (rot0_rt, tran0_rt)})


def _solve(b, data, stage, **opts):
    name, mode, dm, tp = stage
    rot0, tran0 = data["start"][name]
    return b.solve(mode, rot0, tran0, data["d1"], data["d2"], depth_mode=dm, options=api.default_lm_options(tran_param=tp, **opts))


def _set_driver(monkeypatch, dynamic=None, first=None, per_cu=None):
    """dynamic None: unset (the hybrid with one block per pair); first / per_cu None: unset (the defaults)."""
    for name, v in (("SBA_BATCH_DYNAMIC", dynamic), ("SBA_BATCH_LM_FIRST_SWEEPS", first), ("SBA_BATCH_DYN_BLOCKS_PER_CU", per_cu)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _key(q):
    return (q.num_iterations, q.num_successful_steps, q.num_evaluations, q.termination)


def _assert_same_solve(base, got, sizes, initial_bitwise, what):
    """Per pair: status, (iterations, successful steps, evaluations, termination), the initial cost (bit for bit when the
    first sweep ran in the same kernel, else to 1e-13), the final cost to 1e-9 and R|t to 1e-11 (a pair swept by several
    shares folds its sums in another order)."""
    r0, t0, s0, st0 = base
    r1, t1, s1, st1 = got
    assert np.array_equal(st0, st1) and (st1 == 0).all(), what
    for g, (a, q) in enumerate(zip(s0, s1)):
        assert _key(a) == _key(q), (what, g, sizes[g], _key(a), _key(q))
        if initial_bitwise:
            assert a.initial_cost == q.initial_cost, (what, g)
        else:
            assert abs(a.initial_cost - q.initial_cost) <= 1e-13 * abs(a.initial_cost), (what, g)
        assert abs(a.final_cost - q.final_cost) <= 1e-9 * abs(a.final_cost), (what, g)
    assert np.abs(r0 - r1).max() <= 1e-11 and np.abs(t0 - t1).max() <= 1e-11, (what, np.abs(r0 - r1).max(), np.abs(t0 - t1).max())


def _assert_handed_over(sums, sizes, cap, what, beyond=2):
    """Pairs went on for more than `beyond` sweeps after the hand-over, and others finished inside the first launch."""
    evals = [q.num_evaluations for q, n in zip(sums, sizes) if n > 0]
    assert max(evals) > cap + beyond and min(evals) <= cap, (what, cap, sorted(evals))


def _planes(c, store):
    if store == api.STORE_F64:
        return c.x1, c.x2
    return c.x1.astype(np.float32).astype(np.float64), c.x2.astype(np.float32).astype(np.float64)


def _check_references(oracle, data, store, stage, base, sample=ORACLE_SAMPLE, numpy_pair=NUMPY_PAIR, **opts):
    """The one-launch baseline against the oracle's LM per sampled pair (equal iteration and accepted-step counts, R|t to
    RT_TOL) and -- TRAN_FREE stages -- against the independent numpy LM on one pair (same termination and counts)."""
    _, mode, dm, tp = stage
    rot, tran, sums, _ = base
    tol = RT_TOL_F64 if store == api.STORE_F64 else RT_TOL_F32
    for g in sample:
        c = data["cs"][g]
        assert data["sizes"][g] >= 50
        a1, a2 = _planes(c, store)
        d12 = c.d12 if dm == api.DEPTH_PER_MATCH else None
        ro, to, so, rc = oracle.lm_solve(mode, a1, a2, *(v[g] for v in data["start"][stage[0]]), data["d1"][g], data["d2"][g], d12=d12,
                                         options=oracle.default_options(tran_param=tp, **opts))
        assert rc == 0
        assert (sums[g].num_iterations, sums[g].num_successful_steps) == (so.num_iterations, so.num_successful_steps), (stage[0], g)
        assert np.abs(rot[g] - ro).max() <= tol and np.abs(tran[g] - to).max() <= tol, (stage[0], g)
    if tp == api.TRAN_FREE and numpy_pair is not None:
        g = numpy_pair
        c = data["cs"][g]
        a1, a2 = _planes(c, store)
        rn, tn, info = rl.solve(mode, a1, a2, *(v[g] for v in data["start"][stage[0]]), data["d1"][g], data["d2"][g],
                                d12=c.d12 if dm == api.DEPTH_PER_MATCH else None, delta=opts.get("huber_delta", 1.0),
                                max_iter=opts.get("max_num_iterations", 50))
        assert (TERM_NUMPY[sums[g].termination], sums[g].num_iterations, sums[g].num_successful_steps) == \
            (info["termination"], info["iterations"], info["successful"]), (stage[0], g)
        assert np.abs(rot[g] - rn).max() <= tol and np.abs(tran[g] - tn).max() <= tol, (stage[0], g)


@pytest.mark.parametrize("store", [api.STORE_F64, api.STORE_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", [k for k, _ in KINDS], ids=[n for _, n in KINDS])
def test_hybrid_hand_over_at_every_point_equals_the_one_launch_solve(oracle, kind, store, monkeypatch):
    """Driver: the HYBRID (default with one block per pair).  Regime: the hand-over after 1, 2, 3 and 6 (the default) sweeps,
    ROT with per-pair uniform depths / TRAN / RT on the sphere, factored and explicit kernels, f64 and f32 planes.  Every pair
    must do exactly what the uncapped one-launch kernel does: same status and counts, the same first sweep (initial cost to
    the bit: it runs in the same kernel), R|t to 1e-11.  A handed-over pair carries its own solver words, depths, next sweep
    state and -- factored, not TRAN -- frame; a wrong pair's state, a stale frame or a lost solver word shows here.  The
    baseline itself is held against the oracle and the numpy LM; the batch holds pairs that end at their first evaluation,
    pairs that end exactly at the cap and one sweep after it, and poor starts that need many more sweeps than any cap."""
    data = _lm_batch()
    sizes = data["sizes"]
    with api.Batch(0) as b:
        b.set_kernel(kind)
        b.upload(data["x1"], data["x2"], data["off"], data["d12"], store=store)
        assert b.blocks_per_pair == 1
        for stage in STAGES:
            _set_driver(monkeypatch, dynamic=0)
            base = _solve(b, data, stage)
            _check_references(oracle, data, store, stage, base)
            if stage[3] == api.TRAN_SPHERE:              # the numpy LM knows no sphere: the same stage on free t against it
                free = (stage[0], stage[1], stage[2], api.TRAN_FREE)
                _check_references(oracle, data, store, free, _solve(b, data, free), sample=(NUMPY_PAIR,))
            evals = sorted(q.num_evaluations for q, n in zip(base[2], sizes) if n > 0)
            print(stage[0], {e: evals.count(e) for e in sorted(set(evals))})
            for cap in (1, 2, 3, 6):
                assert cap in evals and cap + 1 in evals, (stage[0], cap, evals)      # a pair ends AT the cap, one just after
                _set_driver(monkeypatch, first=None if cap == 6 else cap)
                got = _solve(b, data, stage)
                _assert_same_solve(base, got, sizes, True, (stage[0], cap))
                _assert_handed_over(got[2], sizes, cap, (stage[0], cap))


@pytest.mark.parametrize("opts", [dict(max_num_iterations=3), dict(huber_delta=0.0)], ids=["max_iter_3", "no_loss"])
def test_hybrid_hand_over_with_non_default_options(oracle, opts, monkeypatch):
    """Driver: the HYBRID with options off the defaults.  max_num_iterations = 3: a pair handed over after its first sweep
    must still end at the iteration limit (NO_CONVERGENCE, status OK) exactly where the one-launch kernel ends it.
    huber_delta = 0: the LOSS=false instantiations of the capped one-launch kernel and of the dynamic sweep.  Both kernels,
    the three stages, against the one-launch baseline, which is held against the oracle and the numpy LM."""
    data = _lm_batch(seed0=7800)
    sizes = data["sizes"]
    caps = (1,) if "max_num_iterations" in opts else (1, 3)
    for kind, _ in KINDS:
        with api.Batch(0) as b:
            b.set_kernel(kind)
            b.upload(data["x1"], data["x2"], data["off"], data["d12"])
            for stage in STAGES:
                _set_driver(monkeypatch, dynamic=0)
                base = _solve(b, data, stage, **opts)
                if kind == api.KERNEL_FACTORED:
                    _check_references(oracle, data, api.STORE_F64, stage, base, sample=(4, 14, 29), **opts)
                for cap in caps:
                    _set_driver(monkeypatch, first=cap)
                    got = _solve(b, data, stage, **opts)
                    _assert_same_solve(base, got, sizes, True, (stage[0], cap))
                    _assert_handed_over(got[2], sizes, cap, (stage[0], cap),
                                        beyond=2 if "max_num_iterations" in opts else 0)      # least squares: few sweeps
                if "max_num_iterations" in opts:
                    assert any(q.termination == "NO_CONVERGENCE" and q.num_evaluations > 1 for q in got[2]), stage[0]


@pytest.mark.parametrize("store", [api.STORE_F64, api.STORE_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("per_cu", [1, 2, 8])
def test_dynamic_shares_from_the_first_sweep_with_one_block_per_pair(store, per_cu, monkeypatch):
    """Driver: DYNAMIC shares from the first sweep (SBA_BATCH_DYNAMIC=1) although every pair fits one block, with 1, 2 and 8
    sweep blocks per CU.  Regime: S = G / active shares per pair from a few up to thousands (per_cu = 8 with the batch whose
    poor starts are only two: the last passes spread a pair of a few hundred matches over about 1 000 shares, nearly all of
    them empty, which must add exact zeros).  Against the one-launch baseline as in the hybrid test; the first sweep folds in
    another order here, so the initial cost is held to 1e-13."""
    for poor in ("third", "two"):
        data = _lm_batch(poor=poor)
        sizes = data["sizes"]
        for kind, kname in KINDS:
            with api.Batch(0) as b:
                b.set_kernel(kind)
                b.upload(data["x1"], data["x2"], data["off"], data["d12"], store=store)
                assert b.blocks_per_pair == 1
                for stage in STAGES:
                    _set_driver(monkeypatch, dynamic=0)
                    base = _solve(b, data, stage)
                    _set_driver(monkeypatch, dynamic=1, per_cu=per_cu)
                    got = _solve(b, data, stage)
                    _assert_same_solve(base, got, sizes, False, (poor, kname, stage[0]))
                    evals = sorted(q.num_evaluations for q, n in zip(got[2], sizes) if n > 0)
                    if poor == "two":                          # the last passes had one or two pairs left
                        assert evals[-2] > evals[-3], (stage[0], evals)


def _many_pairs(seed0=8100):
    """About 1 500 pairs of 100-400 matches, three in four from poor starts: more than 1 024 pairs are still active after
    the first sweep (and after the d-only stage's first pass)."""
    B = 1500
    sizes = [100 + (53 * g) % 301 for g in range(B)]
    cs, off, x1, x2, d12 = make_pairs(sizes, seed0=seed0)
    rot0 = np.stack([c.rot_init for c in cs]); tran0 = np.stack([c.tran_init for c in cs])
    poor = np.arange(B) % 4 != 0
    rot0[poor] = np.stack([c.rot_true for c in cs])[poor] + 0.25
    return sizes, cs, off, x1, x2, d12, rot0, tran0


def test_more_than_1024_active_pairs(oracle, monkeypatch):
    """Regime: more than 1 024 pairs active in the dynamic launches, so that the feed kernel's grid (min(pairs, 1 024)) loops
    over its slots, the compaction kernel takes several entries per thread (> 256) and every block of the sweep takes several
    pairs in turn (S = 1, active > grid).  Drivers: the HYBRID with a cap of 1 sweep and DYNAMIC shares from the first sweep,
    against the one-launch baseline (itself held against the oracle on sampled pairs), sampled pairs against the
    single-problem solve to 1e-12; and the d-only stage handed over after its first pass against the one-launch stage."""
    sizes, cs, off, x1, x2, d12, rot0, tran0 = _many_pairs()
    opt = api.default_lm_options(tran_param=api.TRAN_SPHERE)
    got = {}
    with api.Batch(0) as b:
        b.upload(x1, x2, off, d12)
        assert b.blocks_per_pair == 1
        for name, dyn, first in (("base", 0, None), ("hybrid_cap1", None, 1), ("dynamic", 1, None)):
            _set_driver(monkeypatch, dynamic=dyn, first=first)
            got[name] = b.solve(api.MODE_RT, rot0, tran0, depth_mode=api.DEPTH_PER_MATCH, options=opt)
        _set_driver(monkeypatch)
        start = np.full_like(d12, 1.5)
        depth = {}
        for cap in ("0", "1"):
            monkeypatch.setenv("SBA_BATCH_DEPTH_FIRST_PASSES", cap)
            b.set_depths(start)
            d, sums, status = b.solve_depths(rot0, tran0)
            packs = b.eval(api.MODE_RT, rot0, tran0, depth_mode=api.DEPTH_PER_MATCH)     # the planes hold the refined depths
            depth[cap] = (d, sums, status, packs)
    base = got["base"]
    assert sum(q.num_evaluations > 1 for q in base[2]) > 1024                    # > 1 024 pairs active after the first sweep
    _assert_same_solve(base, got["hybrid_cap1"], sizes, True, "hybrid_cap1")
    assert max(q.num_evaluations for q in got["hybrid_cap1"][2]) > 3                  # pairs went on long after the hand-over
    _assert_same_solve(base, got["dynamic"], sizes, False, "dynamic")
    for g in (0, 1, 2, 777, 1024, 1499):
        c = cs[g]
        with api.Problem(0) as p:
            p.upload(c.x1, c.x2, c.d12)
            r1, t1, s1 = p.solve(api.MODE_RT, rot0[g], tran0[g], depth_mode=api.DEPTH_PER_MATCH, options=opt)
        for name in ("base", "hybrid_cap1", "dynamic"):
            rot, tran, sums, _ = got[name]
            assert sums[g].num_iterations == s1.num_iterations, (name, g)
            assert np.abs(rot[g] - r1).max() <= 1e-12 and np.abs(tran[g] - t1).max() <= 1e-12, (name, g)
        if g in (1, 1024):
            ro, to, so, rc = oracle.lm_solve(api.MODE_RT, c.x1, c.x2, rot0[g], tran0[g], d12=c.d12,
                                             options=oracle.default_options(tran_param=api.TRAN_SPHERE))
            assert rc == 0 and base[2][g].num_iterations == so.num_iterations
            assert np.abs(base[0][g] - ro).max() <= RT_TOL_F64 and np.abs(base[1][g] - to).max() <= RT_TOL_F64
    d0, s0, st0, p0 = depth["0"]
    d1, s1, st1, p1 = depth["1"]
    assert (st0 == 0).all() and (st1 == 0).all()
    assert [(q.num_iterations, q.num_successful_steps, q.num_line_search_steps, q.num_evaluations, q.termination) for q in s0] == \
           [(q.num_iterations, q.num_successful_steps, q.num_line_search_steps, q.num_evaluations, q.termination) for q in s1]
    assert np.abs(d0 - d1).max() <= 1e-8 * max(1.0, np.abs(d0).max())
    assert np.abs(p0 - p1).max() <= 1e-8 * np.abs(p0).max()
    assert sum(q.num_evaluations > 1 for q in s1) > 1024                       # > 1 024 pairs handed over after the first pass
    assert max(q.num_evaluations for q in s1) > 3


@pytest.mark.parametrize("kind", [k for k, _ in KINDS], ids=[n for _, n in KINDS])
def test_unpublished_launch_equals_the_published_drivers(kind, monkeypatch):
    """Driver: SBA_PUBLISH=0 (read when the handle is created).  One block per pair: the one-launch kernel with a stream
    wait instead of the mapped sequence word -- the same kernel and fold order as the published one-launch baseline, so the
    same bits.  Several blocks per pair (SBA_BATCH_BPP=3): the host lock-step loop, bit for bit the published handle's
    lock-step loop (SBA_BATCH_DYNAMIC=0)."""
    data = _lm_batch(seed0=7900)
    sizes = data["sizes"]

    def run(publish, bpp, **env):
        monkeypatch.setenv("SBA_PUBLISH", publish)
        if bpp > 1:
            monkeypatch.setenv("SBA_BATCH_BPP", str(bpp))
        else:
            monkeypatch.delenv("SBA_BATCH_BPP", raising=False)
        with api.Batch(0) as b:
            monkeypatch.delenv("SBA_PUBLISH")
            b.set_kernel(kind)
            b.upload(data["x1"], data["x2"], data["off"], data["d12"])
            assert b.blocks_per_pair == bpp
            _set_driver(monkeypatch, **env)
            out = [_solve(b, data, stage) for stage in STAGES]
        return out

    for bpp in (1, 3):
        _set_driver(monkeypatch)
        unpublished = run("0", bpp)
        if bpp == 1:
            published = run("1", bpp, dynamic=0)
        else:
            published = run("1", bpp, dynamic=0)
        for stage, u, p in zip(STAGES, unpublished, published):
            assert np.array_equal(u[0], p[0]) and np.array_equal(u[1], p[1]) and np.array_equal(u[3], p[3]), (bpp, stage[0])
            for g, (a, q) in enumerate(zip(u[2], p[2])):
                assert _key(a) + (a.initial_cost, a.final_cost) == _key(q) + (q.initial_cost, q.final_cost), (bpp, stage[0], g, sizes[g])


def _summ(sums):
    return [(q.num_iterations, q.num_successful_steps, q.num_evaluations, q.num_line_search_steps, q.termination, q.initial_cost,
             q.final_cost, q.final_radius) for q in sums]


def test_one_handle_reused_across_drivers_equals_fresh_handles(monkeypatch):
    """Handle reuse: the hybrid LM, the d-only stage, the dynamic LM and the pipeline share the dynamic scratch (solver state,
    active lists, done flags, share rows) and the sequence words of one handle.  On ONE handle, in this order: a hybrid RT
    solve (cap 2), the d-only stage, a hybrid ROT solve (cap 4), dynamic shares at 8 blocks per CU (the scratch grows), a
    hybrid TRAN solve (default cap), the pipeline -- each must equal the same call on a fresh handle bit for bit."""
    data = _lm_batch(seed0=8000)
    x1, x2, off, d12 = data["x1"], data["x2"], data["off"], data["d12"]
    d0 = np.full_like(d12, 1.5)
    rt, rot_stage, tran_stage = STAGES[2], STAGES[0], STAGES[1]
    calls = [(dict(first=2), lambda b: _solve(b, data, rt)),
             (dict(), lambda b: b.solve_depths(*data["start"]["rt"])),
             (dict(first=4), lambda b: _solve(b, data, rot_stage)),
             (dict(dynamic=1, per_cu=8), lambda b: (b.set_depths(d0), _solve(b, data, rt))[1]),     # the d-only stage
             (dict(), lambda b: (b.set_depths(d0), _solve(b, data, tran_stage))[1]),                # moved the depths

             (dict(), lambda b: (b.set_depths(d0), b.solve_problem(seed=3, want_depths=True, check=False))[1])]

    def flat(res):
        if isinstance(res, dict):
            return [res[k] for k in ("rot", "tran", "d_uniform", "guess_candidates", "status", "d12")] + \
                   [_summ(res[k]) for k in ("depth_stage", "rot_stage", "tran_stage")]
        return [_summ(r) if isinstance(r, list) else r for r in res]

    def same(a, b):
        return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(flat(a), flat(b)))

    reused = []
    with api.Batch(0) as b:
        b.upload(x1, x2, off, d0)
        for env, call in calls:
            _set_driver(monkeypatch, **env)
            reused.append(call(b))
    for k, (env, call) in enumerate(calls):
        with api.Batch(0) as b:
            b.upload(x1, x2, off, d0)
            _set_driver(monkeypatch, **env)
            assert same(reused[k], call(b)), k
    assert max(q.num_evaluations for q in reused[0][2]) > 4                  # the first call really handed pairs over
