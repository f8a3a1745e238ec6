"""GPU: per-match-depth sweeps over the depth-folded planes (X1 = d1 x1, X2 = d2 x2; sba_problem_set_folding).

The folded planes are a cache of the raw ones: with the grid pinned, a sweep over them gives the same bits as the raw
8-plane sweep, in every mode, kernel kind and loss setting, at ragged sizes too.  Every writer of the coordinate or
depth planes (set_depths, a re-upload, the d-only stage on each of its drivers, the key-point upload) leaves the handle
sweeping what a fresh handle holding the same data sweeps."""
import numpy as np
import pytest

from helpers import REL_TOL_F64, assert_normal_eq_close
from spherical_bundle_adjuster_amd import api, synthetic

pytestmark = pytest.mark.gpu

MODES = (api.MODE_ROT, api.MODE_TRAN, api.MODE_RT)
KINDS = (api.KERNEL_FACTORED, api.KERNEL_EXPLICIT)


@pytest.fixture
def pinned_grid(monkeypatch):
    """Same blocks per CU for every variant (read at handle creation): the folded and the raw sweep then reduce in the
    same order and their packs compare bit for bit."""
    monkeypatch.setenv("SBA_BLOCKS_PER_CU", "2")


def _packs(p, c, rot=None, tran=None):
    rot = c.rot_init if rot is None else rot
    tran = c.tran_init if tran is None else tran
    out = {}
    for kind in KINDS:
        p.set_kernel(kind)
        for mode in MODES:
            for delta in (1.0, 0.0):
                out[(kind, mode, delta)] = p.eval_pack(mode, rot, tran, huber_delta=delta, depth_mode=api.DEPTH_PER_MATCH)
    p.set_kernel(api.KERNEL_FACTORED)
    return out


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (k, np.abs(a[k] - b[k]).max())


@pytest.mark.parametrize("n", [7, 2049, 1_000_003])
def test_folded_equals_raw_planes(pinned_grid, n):
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 11)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12)
        folded = _packs(p, c)
        p.set_folding(False)
        raw = _packs(p, c)
        p.set_folding(True)                                  # folded again lazily, before the next per-match sweep
        again = _packs(p, c)
    _assert_same(folded, raw)
    _assert_same(folded, again)
    assert folded[(api.KERNEL_FACTORED, api.MODE_RT, 1.0)][22] > 0.0


@pytest.mark.parametrize("n", [7, 2049, 20_011])
def test_folded_sweeps_match_the_oracle(oracle, n):
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 12)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12)
        for kind in KINDS:
            p.set_kernel(kind)
            for mode in MODES:
                got = p.eval(mode, c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH)
                ref = oracle.evaluate(mode, c.x1, c.x2, c.rot_init, c.tran_init, d12=c.d12)
                assert_normal_eq_close(got, ref, REL_TOL_F64, f"n={n} kind={kind} mode={mode}")
                assert got.n_outlier == ref.n_outlier


def _fresh_packs(c, x1, x2, d12, rot=None, tran=None):
    """The same sweeps on a new handle holding (x1, x2, d12)."""
    with api.Problem(0) as q:
        q.upload(x1, x2, d12)
        return _packs(q, c, rot, tran)


def test_set_depths_and_reupload_invalidate(pinned_grid):
    c = synthetic.full_rt(30_001, seed=synthetic.BASE_SEED + 13)
    d_new = c.d12 * np.random.default_rng(5).uniform(0.8, 1.25, c.d12.shape)
    small = synthetic.full_rt(4_099, seed=synthetic.BASE_SEED + 14)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12)
        before = _packs(p, c)
        p.set_depths(d_new)
        after_set = _packs(p, c)
        p.upload(small.x1, small.x2, small.d12)              # another size: planes re-laid out, cache re-formed
        after_upload = _packs(p, c)
    _assert_same(after_set, _fresh_packs(c, c.x1, c.x2, d_new))
    assert not np.array_equal(before[(api.KERNEL_FACTORED, api.MODE_RT, 1.0)],
                              after_set[(api.KERNEL_FACTORED, api.MODE_RT, 1.0)])
    _assert_same(after_upload, _fresh_packs(c, small.x1, small.x2, small.d12))


@pytest.mark.parametrize("n,one_launch", [(2_049, "1"), (2_049, "0"), (20_011, "1")],
                         ids=["one-launch", "resident", "launch-per-pass"])
def test_solve_depths_invalidates(pinned_grid, monkeypatch, n, one_launch):
    """The d-only stage rewrites the depth planes on the device (each driver: one launch, the resident evaluator, a
    launch per pass); the next per-match sweep must see the refined depths."""
    monkeypatch.setenv("SBA_SMALL_ONE_LAUNCH", one_launch)
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 15, depth_noise=0.05)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12)
        before = _packs(p, c, c.rot_true, c.tran_true)
        d_out, s = p.solve_depths(c.rot_true, c.tran_true)
        assert s.num_iterations >= 1 and not np.array_equal(d_out, c.d12)
        after = _packs(p, c, c.rot_true, c.tran_true)
    _assert_same(after, _fresh_packs(c, c.x1, c.x2, d_out, c.rot_true, c.tran_true))
    assert not np.array_equal(before[(api.KERNEL_FACTORED, api.MODE_RT, 1.0)], after[(api.KERNEL_FACTORED, api.MODE_RT, 1.0)])


def test_upload_keypoints_with_depths_invalidates(pinned_grid):
    rng = np.random.default_rng(23)
    n, W, H = 5_003, 3840, 1920
    kl = np.zeros((n, 7), dtype=np.float32)
    kl[:, 0] = rng.uniform(0, W, n)
    kl[:, 1] = rng.uniform(0.05 * H, 0.95 * H, n)
    kr = kl.copy()
    kr[:, :2] += rng.normal(0, 3.0, (n, 2)).astype(np.float32)
    d12 = rng.uniform(0.5, 2.0, (n, 2))
    c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 16)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12)                           # something else folded first
        _packs(p, c)
        p.upload_keypoints(kl, kr, W, H, d12=d12)
        got = _packs(p, c)
    _assert_same(got, _fresh_packs(c, api.keypoints_to_sphere(kl, W, H), api.keypoints_to_sphere(kr, W, H), d12))


def test_uniform_depth_sweep_unaffected(pinned_grid):
    """A handle with per-match depths (and folded planes) sweeps uniform depths from the raw coordinate planes."""
    c = synthetic.full_rt(100_003, seed=synthetic.BASE_SEED + 17)
    with api.Problem(0) as p, api.Problem(0) as q:
        p.upload(c.x1, c.x2, c.d12)
        q.upload(c.x1, c.x2)
        for kind in KINDS:
            p.set_kernel(kind)
            q.set_kernel(kind)
            for mode in MODES:
                a = p.eval_pack(mode, c.rot_init, c.tran_init, d1=3.0, d2=5.0, depth_mode=api.DEPTH_UNIFORM)
                b = q.eval_pack(mode, c.rot_init, c.tran_init, d1=3.0, d2=5.0, depth_mode=api.DEPTH_UNIFORM)
                assert np.array_equal(a, b), (kind, mode)


def test_f32_planes_sweep_raw(oracle):
    """f32 planes are never folded (X1, X2 would have to be f64 planes): per-match sweeps still run and agree."""
    from helpers import REL_TOL_F32
    c = synthetic.full_rt(2_049, seed=synthetic.BASE_SEED + 18)
    with api.Problem(0) as p:
        p.upload(c.x1, c.x2, c.d12, store=api.STORE_F32)
        got = p.eval(api.MODE_RT, c.rot_init, c.tran_init, depth_mode=api.DEPTH_PER_MATCH)
    x1, x2 = c.x1.astype(np.float32).astype(np.float64), c.x2.astype(np.float32).astype(np.float64)
    assert_normal_eq_close(got, oracle.evaluate(api.MODE_RT, x1, x2, c.rot_init, c.tran_init, d12=c.d12), REL_TOL_F32)
