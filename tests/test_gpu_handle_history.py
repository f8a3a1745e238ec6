"""GPU: what an api.Problem returns does not depend on what ran on the handle before.

Every entry point is bit-identical from run to run, so its bytes after any history must equal its bytes on a fresh handle
holding the same matches.  The handle shares device state between its features by convention -- the d-only scratch the
joint solve, the covariance, the structure and the resection lay out each their own way, the select scratch, the folded
planes behind `folded_valid`, the weighted resection's planes kept across uploads, the sequence words of the sweeps, the
one-launch stages and the resident commands -- and these tests pin the conventions: the operations of handle_ops.py run
after one another on one handle, in both orders, and compare with fresh handles, bytes against bytes, no tolerance."""
import numpy as np
import pytest

import handle_ops as ops
from spherical_bundle_adjuster_amd import api, synthetic

pytestmark = pytest.mark.gpu

SEED = 4100
PROBES = ops.by_kind(ops.PROBLEM_OPS, ops.PROBE)
MUTATORS = ops.by_kind(ops.PROBLEM_OPS, ops.MUTATOR)
REFUSALS = ops.by_kind(ops.PROBLEM_OPS, ops.REFUSAL)

# (n, store, SBA_SMALL_ONE_LAUNCH).  261: odd, n % 4 = 1 (the last vector of f32 planes reaches past the last depth pair),
# below every small-problem threshold -- the stages run as one launch (default) or through the resident sessions and their
# command sequence ("0").  4098: n % 4 = 2, above the resident / one-launch limits: every sweep and d-only pass is a launch.
CONFIGS = [(261, api.STORE_F64, None), (261, api.STORE_F32, None), (261, api.STORE_F64, "0"), (261, api.STORE_F32, "0"),
           (4098, api.STORE_F64, None), (4098, api.STORE_F32, None)]


def _cfg_id(cfg):
    n, store, one = cfg
    return f"n{n}-{'f64' if store == api.STORE_F64 else 'f32'}-{'default' if one is None else 'resident'}"


configs = pytest.mark.parametrize("cfg", CONFIGS, ids=_cfg_id)


def _drivers(monkeypatch, cfg):
    if cfg[2] is None:
        monkeypatch.delenv("SBA_SMALL_ONE_LAUNCH", raising=False)
    else:
        monkeypatch.setenv("SBA_SMALL_ONE_LAUNCH", cfg[2])


def _scene(n, seed, store):
    """The scene with the landmark covariances a fresh handle's structure_joint gives for it."""
    s = ops.problem_scene(n, seed, store)
    with ops.open_problem(s) as p:
        s.landmark_cov = p.structure_joint(s.rot, s.tran).cov
    return s


_REFERENCE = {}


def _reference(cfg):
    """(scene, {probe name: bytes}) of the configuration: every probe on a fresh handle of its own, computed once.  The
    caller has set the configuration's drivers."""
    if cfg not in _REFERENCE:
        s = _scene(cfg[0], SEED, cfg[1])
        ref = {}
        for op in PROBES:
            with ops.open_problem(s) as p:
                ref[op.name] = op(p, s)
        _REFERENCE[cfg] = (s, ref)
    return _REFERENCE[cfg]


def _where(cfg, **kw):
    return ", ".join([f"{k} = {v}" for k, v in kw.items()] + [f"scene {_cfg_id(cfg)} seed {SEED}"])


# ---- (a) the anchor: the probes are deterministic, say something and say something finite -----------------------------------
@configs
def test_probes_are_deterministic_and_not_vacuous(monkeypatch, cfg):
    _drivers(monkeypatch, cfg)
    s, ref = _reference(cfg)
    other = _scene(cfg[0], SEED + 1, cfg[1])
    for op in PROBES:
        assert not ref[op.name].startswith(b"ERR"), _where(cfg, probe=op.name, refused=ref[op.name])
        with ops.open_problem(s) as p:
            raw = op.fn(p, s)
        assert ops.to_bytes(raw) == ref[op.name], _where(cfg, probe=op.name, what="two fresh handles differ")
        if op.name in ops.PROBLEM_FINITE:
            v = ops.float_values(raw)
            assert v.size and np.isfinite(v).all(), _where(cfg, probe=op.name, what="non-finite output")
        if op.name == "structure_joint":
            assert np.isfinite(raw.xyz).all() and np.isfinite(raw.pose.cov).all(), _where(cfg, probe=op.name)
        with ops.open_problem(other) as p:
            assert op(p, other) != ref[op.name], _where(cfg, probe=op.name, what="the same bytes for another scene")
    for op in REFUSALS:
        with ops.open_problem(s) as p:
            got = op(p, s)
        assert got.startswith(b"ERR"), _where(cfg, refusal=op.name, got=got[:40])
    for op in MUTATORS:
        with ops.open_problem(s) as p:
            assert not op(p, s).startswith(b"ERR"), _where(cfg, mutator=op.name)


# ---- (b) every probe after any one probe or refusal, in both orders ---------------------------------------------------------
@configs
@pytest.mark.parametrize("disturber", PROBES + REFUSALS, ids=lambda op: op.name)
def test_probes_after_one_operation(monkeypatch, cfg, disturber):
    _drivers(monkeypatch, cfg)
    s, ref = _reference(cfg)
    for order in ("table", "reverse"):
        with ops.open_problem(s) as p:
            disturber(p, s)
            for op in (PROBES if order == "table" else PROBES[::-1]):
                assert op(p, s) == ref[op.name], _where(cfg, disturber=disturber.name, probe=op.name, order=order)


# ---- (c) the mutators do not see the history either --------------------------------------------------------------------------
@configs
@pytest.mark.parametrize("mutator", MUTATORS, ids=lambda op: op.name)
def test_mutator_after_a_disturber_equals_the_mutator_alone(monkeypatch, cfg, mutator):
    _drivers(monkeypatch, cfg)
    s, _ = _reference(cfg)
    with ops.open_problem(s) as p:
        alone = mutator(p, s)
        after_alone = [op(p, s) for op in PROBES]
    for name in ops.PROBLEM_DISTURBERS:
        with ops.open_problem(s) as p:
            ops.by_name(ops.PROBLEM_OPS, name)(p, s)
            assert mutator(p, s) == alone, _where(cfg, disturber=name, mutator=mutator.name)
            for op, want in zip(PROBES, after_alone):         # a refused probe must be refused with the same code
                assert op(p, s) == want, _where(cfg, disturber=name, mutator=mutator.name, probe=op.name)


# ---- (d) the sequences that reading the code singles out ---------------------------------------------------------------------
def _sweeps(p, s, rot=None, tran=None):
    rot, tran = (s.rot if rot is None else rot), (s.tran if tran is None else tran)
    return b"".join(ops.to_bytes(p.eval_pack(m, rot, tran, depth_mode=api.DEPTH_PER_MATCH))
                    for m in (api.MODE_RT, api.MODE_ROT, api.MODE_TRAN))


WEAK_SIN2 = 1e-8        # the parallax cut of the sequences below: it leaves out exactly the matches _weak_parallax made


def _weak_parallax(s):
    """The scene with two matches of every three nearly without parallax at s.rot (x2 = R x1 up to 1e-5): under the cut
    WEAK_SIN2 their covariance rows are (inf, inf, 0) and their structure rows inf, so whatever layout a per-match pass
    gives the shared scratch, most of what it leaves there is not finite."""
    rng = np.random.default_rng([s.seed, 79])
    weak = np.arange(s.n) % 3 != 0
    x2 = s.x2.copy()
    v = s.x1[weak] @ synthetic.rodrigues(s.rot).T + 1e-5 * rng.standard_normal((int(weak.sum()), 3))
    x2[weak] = v / np.linalg.norm(v, axis=1, keepdims=True)
    s.x2 = x2
    return s, weak


@pytest.mark.parametrize("stage", ["solve_depths", "solve_joint"])
@pytest.mark.parametrize("iterations", [1, 2, 3])
@pytest.mark.parametrize("dirt", ["covariance", "covariance+structure"])
@pytest.mark.parametrize("n,store,one_launch", [(261, api.STORE_F32, None), (261, api.STORE_F32, "0"), (4098, api.STORE_F32, None),
                                                (261, api.STORE_F64, "0"), (4098, api.STORE_F64, None)],
                         ids=["n261-f32-default", "n261-f32-resident", "n4098-f32", "n261-f64-resident", "n4098-f64"])
def test_depth_block_covariance_before_the_depth_stages(monkeypatch, n, store, one_launch, dirt, iterations, stage):
    """The covariance's depth rows and the structure's outputs pass through the scratch whose first four planes the d-only
    stage and the joint solve take their candidate planes from; an accepted step makes a candidate plane the problem's
    depth plane -- where the stage copies whole planes back, padding included -- and a per-match sweep loads that padding
    in its ragged tail.  The scratch is dirtied with rows that are not finite; the stage after it equals the stage on a fresh
    scratch, and the sweep after it is finite."""
    _drivers(monkeypatch, (n, store, one_launch))
    s, weak = _weak_parallax(ops.problem_scene(n, SEED + 2, store))

    def run(p):
        if stage == "solve_depths":
            out = p.solve_depths(s.rot, s.tran, options=api.default_lm_options(max_num_iterations=iterations))
        else:
            out = p.solve_joint(s.rot, s.tran, api.default_lm_options(max_num_iterations=iterations, tran_param=api.TRAN_SPHERE))
        summary = out[1] if stage == "solve_depths" else out[3]
        assert summary.num_successful_steps >= 1, "no step accepted: no candidate plane became a depth plane"
        pack = p.eval_pack(api.MODE_RT, s.rot, s.tran, depth_mode=api.DEPTH_PER_MATCH)
        return ops.to_bytes(out), pack

    with ops.open_problem(s) as p:
        cov = p.covariance_joint(s.rot, s.tran, min_sin2_parallax=WEAK_SIN2, depths=True)
        assert cov.n_degenerate == int(weak.sum()) and np.isinf(cov.depth_cov[weak, :2]).all() and np.isfinite(cov.depth_cov[~weak]).all()
        if dirt == "covariance+structure":
            assert np.isinf(p.structure_joint(s.rot, s.tran, min_sin2_parallax=WEAK_SIN2).score[weak]).all()
        out_a, pack_a = run(p)
        rest_a = _sweeps(p, s)
    with ops.open_problem(s) as p:
        out_b, pack_b = run(p)
        rest_b = _sweeps(p, s)
    assert np.isfinite(pack_a).all() and pack_a[22] > 0.0, pack_a
    assert out_a == out_b, "the stage's own outputs"
    assert pack_a.tobytes() == pack_b.tobytes() and rest_a == rest_b, "the per-match sweeps after the stage"


@pytest.mark.parametrize("store", [api.STORE_F64, api.STORE_F32], ids=["f64", "f32"])
def test_shrinking_scratch(store):
    """After a large problem the handle's scratch is far larger than a small one needs: the d-only stage then frees and
    reallocates it (the others only ever grow it) and the select scratch follows the same rule.  What runs after the shrink
    equals a fresh handle holding the small problem."""
    big = ops.problem_scene(70_001, SEED + 3, store)
    small = 261
    after = [ops.by_name(ops.PROBLEM_OPS, name) for name in ("solve_depths[2]", "eval_joint", "covariance_joint", "structure_joint",
                                                           "eval_resection", "residual_order_stats", "residuals", "structure_order_stats")]
    with ops.open_problem(big) as p:
        p.solve_joint(big.rot, big.tran, api.default_lm_options(max_num_iterations=2, tran_param=api.TRAN_SPHERE))
        p.covariance_joint(big.rot, big.tran)
        p.residuals(big.rot, big.tran, depth_mode=api.DEPTH_PER_MATCH)
        p.structure_order_stats(big.rot, big.tran, [0, 35_000, 70_000])
        p.upload(big.x1[:small], big.x2[:small], big.d12[:small], store=store)
        got = [op(p, big) for op in after]
    with ops.open_problem(big, rows=small) as p:
        want = [op(p, big) for op in after]
    for op, g, w in zip(after, got, want):
        assert not w.startswith(b"ERR"), op.name
        assert g == w, f"{op.name} after the shrink, store {store}"


def _weighted_bytes(p, s, cov):
    p.set_landmark_covariances(cov, 1.0)
    return ops.to_bytes((p.freeze_resection_weights(s.rot, s.tran, 1e-3), p.resection_weights(), p.eval_resection_weighted(s.rot, s.tran),
                         p.resection_covariance(s.rot, s.tran)))


def _unfrozen_code(p, s):
    with pytest.raises(api.SbaError) as ei:
        p.eval_resection_weighted(s.rot, s.tran)
    return ei.value.code


@pytest.mark.parametrize("store", [api.STORE_F64, api.STORE_F32], ids=["f64", "f32"])
def test_resection_weights_across_uploads_and_compaction(store):
    """The weighted resection keeps its covariance copy and weight planes across uploads and compactions, with their sizes;
    only the two flags are cleared.  A handle that had them refuses like one that never did, and after setting and freezing
    again it returns what a fresh handle returns."""
    small, large = _scene(261, SEED + 4, store), _scene(4098, SEED + 5, store)
    with ops.open_problem(large) as p:
        never = _unfrozen_code(p, large)
        fresh = _weighted_bytes(p, large, large.landmark_cov)
    assert not fresh.startswith(b"ERR")
    for first, second in ((small, large), (large, small)):                # growing and shrinking
        with ops.open_problem(second) as p:
            fresh_second = _weighted_bytes(p, second, second.landmark_cov)
        with ops.open_problem(first) as p:
            _weighted_bytes(p, first, first.landmark_cov)
            p.upload(second.x1, second.x2, second.d12, store=store)
            assert _unfrozen_code(p, second) == never
            with pytest.raises(api.SbaError) as ei:
                p.freeze_resection_weights(second.rot, second.tran, 1e-3)            # no covariances either
            assert _weighted_bytes(p, second, second.landmark_cov) == fresh_second, (first.n, second.n)
    assert fresh_second != fresh
    # ... and across a compaction
    kept = np.flatnonzero(large.keep)
    with ops.open_problem(large) as p:
        _weighted_bytes(p, large, large.landmark_cov)
        assert np.array_equal(p.compact(large.keep), kept)
        assert _unfrozen_code(p, large) == never
        got = _weighted_bytes(p, large, large.landmark_cov[kept])
    with api.Problem(0) as p:
        p.upload(large.x1[kept], large.x2[kept], large.d12[kept], store=store)
        assert got == _weighted_bytes(p, large, large.landmark_cov[kept])


def _writers(s):
    """Every writer of the depth planes but the d-only stage's drivers (test_gpu_folded_planes.py has those, and the first
    entry repeats one of them): name -> (call, the depths (n, 2) the handle holds after it, from what the call returned)."""
    lm = api.default_lm_options(max_num_iterations=6)

    def solve_depths(p):
        return p.solve_depths(s.rot, s.tran, options=api.default_lm_options(max_num_iterations=3))[0]

    def solve_joint(p):
        return p.solve_joint(s.rot, s.tran, api.default_lm_options(max_num_iterations=3, tran_param=api.TRAN_SPHERE))[2]

    def d2_at(p, rot, tran):                  # the eliminated depths at the solve's result are what it stored
        return np.column_stack([s.d12[:, 0], p.resection_depths(rot, tran)])

    def solve_resection(p):
        rot, tran, _, _ = p.solve_resection(s.rot, s.tran, lm, store_depths=True)
        return lambda: d2_at(p, rot, tran)

    def solve_resection_weighted(p):
        p.set_landmark_covariances(s.landmark_cov, 1.0)
        rot, tran, _, _ = p.solve_resection_weighted(s.rot, s.tran, lm, bearing_sigma=1e-3, store_depths=True)
        return lambda: d2_at(p, rot, tran)

    def resection_depths(p):
        return np.column_stack([s.d12[:, 0], p.resection_depths(s.rot, s.tran)])

    def set_depths(p):
        p.set_depths(s.d_alt)
        return s.d_alt

    return {f.__name__: f for f in (solve_depths, solve_joint, solve_resection, solve_resection_weighted, resection_depths, set_depths)}


@pytest.mark.parametrize("folding", [True, False], ids=["folded", "raw"])
@pytest.mark.parametrize("writer", ["solve_depths", "solve_joint", "solve_resection", "solve_resection_weighted", "resection_depths",
                                    "set_depths"])
@pytest.mark.parametrize("n", [261, 4098])
def test_every_depth_writer_then_the_folded_sweep(n, writer, folding):
    """The folded planes d1 x1, d2 x2 are a cache every writer of the depth planes has to invalidate.  The handle has swept
    (the cache is formed and valid) before the writer runs; the sweeps after it equal those of a fresh handle uploaded with
    the depths the writer left."""
    s = _scene(n, SEED + 6, api.STORE_F64)
    with ops.open_problem(s) as p:
        p.set_folding(folding)
        before = _sweeps(p, s)
        depths = _writers(s)[writer](p)
        got = _sweeps(p, s)                   # before anything else touches the planes
        if callable(depths):
            depths = depths()
    assert depths.shape == s.d12.shape and not np.array_equal(depths, s.d12)
    with api.Problem(0) as q:
        q.upload(s.x1, s.x2, depths, store=api.STORE_F64)
        q.set_folding(folding)
        want = _sweeps(q, s)
    assert got != before, "the writer changed nothing the sweep sees"
    assert got == want, f"{writer}, n = {n}, folding {folding}"


def test_long_history(monkeypatch):
    """One handle, every probe and every refusal in a seeded random order, three times over -- the sequence words of the
    sweeps, of the one-launch stages and of the resident commands advance by a few hundred -- then every probe in table
    order equals its reference."""
    cfg = (261, api.STORE_F64, "0")
    _drivers(monkeypatch, cfg)
    s, ref = _reference(cfg)
    rng = np.random.default_rng(SEED)
    pool = PROBES + REFUSALS
    with ops.open_problem(s) as p:
        for rnd in range(3):
            for k in rng.permutation(len(pool)):
                got = pool[k](p, s)
                if pool[k].kind == ops.PROBE:
                    assert got == ref[pool[k].name], _where(cfg, round=rnd, probe=pool[k].name)
        for op in PROBES:
            assert op(p, s) == ref[op.name], _where(cfg, probe=op.name, what="after the long history")
