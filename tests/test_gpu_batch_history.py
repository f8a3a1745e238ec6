"""GPU: what an api.Batch returns does not depend on what ran on the handle before.

The batch's stages share `depth_work` -- zeroed once, at first use, on the promise that every pass writes real elements
only and so leaves the padding zero from stage to stage -- and the batched covariance routes its per-match rows through
it and hands it back zeroed; the dynamic-share buffers are allocated by whichever of the LM and the d-only stage runs
first.  As for the single problem (test_gpu_handle_history.py): the operations of handle_ops.py after one another on one
batch, compared with fresh batches, bytes against bytes, no tolerance."""
import numpy as np
import pytest

import handle_ops as ops
from spherical_bundle_adjuster_amd import api

pytestmark = pytest.mark.gpu

SEED = 5200
SIZES = (257, 64, 0, 65, 513, 1026, 7)       # odd and even sizes, an empty pair, one too small for most estimates, several tiles
PROBES = ops.by_kind(ops.BATCH_OPS, ops.PROBE)
MUTATORS = ops.by_kind(ops.BATCH_OPS, ops.MUTATOR)
REFUSALS = ops.by_kind(ops.BATCH_OPS, ops.REFUSAL)

# (store, SBA_BATCH_INTERLEAVE, SBA_BATCH_BPP): both stores in both layouts, and once more with two blocks per pair (the
# step is then not the fused one-launch step)
CONFIGS = [(api.STORE_F64, "0", None), (api.STORE_F64, "1", None), (api.STORE_F32, "0", None), (api.STORE_F32, "1", None),
           (api.STORE_F64, "1", "2"), (api.STORE_F32, "0", "2")]


def _cfg_id(cfg):
    store, inter, bpp = cfg
    return f"{'f64' if store == api.STORE_F64 else 'f32'}-{'interleaved' if inter == '1' else 'contiguous'}" + (f"-bpp{bpp}" if bpp else "")


configs = pytest.mark.parametrize("cfg", CONFIGS, ids=_cfg_id)


def _layout(monkeypatch, cfg):
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", cfg[1])
    if cfg[2] is None:
        monkeypatch.delenv("SBA_BATCH_BPP", raising=False)
    else:
        monkeypatch.setenv("SBA_BATCH_BPP", cfg[2])


_REFERENCE = {}


def _reference(cfg):
    """(scene, {probe name: bytes}): every probe on a fresh batch of its own, once per configuration (whose layout the
    caller has set)."""
    if cfg not in _REFERENCE:
        s = ops.batch_scene(SIZES, SEED, cfg[0])
        ref = {}
        for op in PROBES:
            with ops.open_batch(s) as b:
                ref[op.name] = op(b, s)
        _REFERENCE[cfg] = (s, ref)
    return _REFERENCE[cfg]


def _where(cfg, **kw):
    return ", ".join([f"{k} = {v}" for k, v in kw.items()] + [f"batch {SIZES} {_cfg_id(cfg)} seed {SEED}"])


# ---- (a) the anchor ----------------------------------------------------------------------------------------------------------
@configs
def test_probes_are_deterministic_and_not_vacuous(monkeypatch, cfg):
    _layout(monkeypatch, cfg)
    s, ref = _reference(cfg)
    other = ops.batch_scene(SIZES, SEED + 1, cfg[0])
    checked_finite = set()
    for op in PROBES:
        assert not ref[op.name].startswith(b"ERR"), _where(cfg, probe=op.name, refused=ref[op.name])
        with ops.open_batch(s) as b:
            raw = op.fn(b, s)
        assert ops.to_bytes(raw) == ref[op.name], _where(cfg, probe=op.name, what="two fresh batches differ")
        v = ops.batch_finite_values(op.name, raw, s)
        if v is not None:
            checked_finite.add(op.name)
            assert v.size and np.isfinite(v).all(), _where(cfg, probe=op.name, what="non-finite output")
        with ops.open_batch(other) as b:
            assert op(b, other) != ref[op.name], _where(cfg, probe=op.name, what="the same bytes for another scene")
    assert checked_finite >= {"eval_joint", "covariance_joint[depths]", "covariance_joint[pose]", "structure_joint"}
    for op in REFUSALS:
        with ops.open_batch(s) as b:
            got = op(b, s)
        assert got.startswith(b"ERR"), _where(cfg, refusal=op.name, got=got[:40])
    for op in MUTATORS:
        with ops.open_batch(s) as b:
            assert not op(b, s).startswith(b"ERR"), _where(cfg, mutator=op.name)


# ---- (b) every probe after any one probe or refusal, in both orders ---------------------------------------------------------
@configs
@pytest.mark.parametrize("disturber", PROBES + REFUSALS, ids=lambda op: op.name)
def test_probes_after_one_operation(monkeypatch, cfg, disturber):
    _layout(monkeypatch, cfg)
    s, ref = _reference(cfg)
    for order in ("table", "reverse"):
        with ops.open_batch(s) as b:
            disturber(b, s)
            for op in (PROBES if order == "table" else PROBES[::-1]):
                assert op(b, s) == ref[op.name], _where(cfg, disturber=disturber.name, probe=op.name, order=order)


# ---- (c) the mutators do not see the history either --------------------------------------------------------------------------
@configs
@pytest.mark.parametrize("mutator", MUTATORS, ids=lambda op: op.name)
def test_mutator_after_a_disturber_equals_the_mutator_alone(monkeypatch, cfg, mutator):
    _layout(monkeypatch, cfg)
    s, _ = _reference(cfg)
    with ops.open_batch(s) as b:
        alone = mutator(b, s)
        after_alone = [op(b, s) for op in PROBES]
    for name in ops.BATCH_DISTURBERS:
        with ops.open_batch(s) as b:
            ops.by_name(ops.BATCH_OPS, name)(b, s)
            assert mutator(b, s) == alone, _where(cfg, disturber=name, mutator=mutator.name)
            for op, want in zip(PROBES, after_alone):         # a refused probe must be refused with the same code
                assert op(b, s) == want, _where(cfg, disturber=name, mutator=mutator.name, probe=op.name)


# ---- (d) the sequences that reading the code singles out ---------------------------------------------------------------------
@pytest.mark.parametrize("stage", ["solve_depths", "solve_joint"])
@pytest.mark.parametrize("iterations", [1, 2, 3])
@pytest.mark.parametrize("dirt", ["finite rows", "rows of no usable match"])
@pytest.mark.parametrize("layout", ["0", "1"], ids=["contiguous", "interleaved"])
@pytest.mark.parametrize("store", [api.STORE_F64, api.STORE_F32], ids=["f64", "f32"])
def test_depth_block_covariance_before_the_depth_stages(monkeypatch, store, layout, dirt, iterations, stage):
    """`depth_work`'s padding stays zero: the covariance's per-match rows pass through the planes the d-only stage and the
    joint solve take their candidate planes from, and an accepted step makes a candidate plane a pair's depth plane.  The
    covariance hands the planes back zeroed -- also when its rows were NaN and inf, those of a call that left every match out
    as degenerate.  The stage after the covariance and the structure equals the stage on a batch that ran nothing else, and
    the per-match sweep after it is finite.
    (Today the batched stages write every work-plane element they later read or copy back -- the padding element of an
    odd-sized pair included -- so this holds even without the covariance's final memset; the test is there for the next
    reader of these planes.)"""
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    s = ops.batch_scene(SIZES, SEED + 2, store)

    def run(b):
        if stage == "solve_depths":
            out = b.solve_depths(s.rot, s.tran, options=api.default_lm_options(max_num_iterations=iterations))
        else:
            out = b.solve_joint(s.rot, s.tran, api.default_lm_options(max_num_iterations=iterations, tran_param=api.TRAN_SPHERE),
                                check=False)
        sums = out[1] if stage == "solve_depths" else out[3]
        assert all(sums[g].num_successful_steps >= 1 for g in np.flatnonzero(s.big)), "no step accepted"
        return ops.to_bytes(out), b.eval(api.MODE_RT, s.rot, s.tran, depth_mode=api.DEPTH_PER_MATCH)

    with ops.open_batch(s) as b:
        if dirt == "finite rows":
            b.covariance_joint(s.rot, s.tran, depths=True, check=False)
        else:
            r = b.covariance_joint(s.rot, s.tran, min_sin2_parallax=2.0, depths=True, check=False)
            assert (r.status != 0).all() and not np.isfinite(r.depth_cov[:, :2]).any()
        b.structure_joint(s.rot, s.tran, check=False)
        out_a, packs_a = run(b)
    with ops.open_batch(s) as b:
        out_b, packs_b = run(b)
    assert np.isfinite(packs_a).all() and (packs_a[s.big, 22] > 0.0).all(), packs_a
    assert out_a == out_b, "the stage's own outputs"
    assert packs_a.tobytes() == packs_b.tobytes(), "the per-match sweep after the stage"


def test_long_history(monkeypatch):
    """One batch, every probe and every refusal in a seeded random order, three times over, then every probe in table
    order: all equal their references."""
    cfg = CONFIGS[1]
    _layout(monkeypatch, cfg)
    s, ref = _reference(cfg)
    rng = np.random.default_rng(SEED)
    pool = PROBES + REFUSALS
    with ops.open_batch(s) as b:
        for rnd in range(3):
            for k in rng.permutation(len(pool)):
                got = pool[k](b, s)
                if pool[k].kind == ops.PROBE:
                    assert got == ref[pool[k].name], _where(cfg, round=rnd, probe=pool[k].name)
        for op in PROBES:
            assert op(b, s) == ref[op.name], _where(cfg, probe=op.name, what="after the long history")
