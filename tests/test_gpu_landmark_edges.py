"""GPU: the landmark map's passes on the rows no seeded scene draws (tests/landmark_edges.py): singular and ill-conditioned priors,
axis-aligned and tied bearings with their one-ulp neighbours and negative zeros, very short and very long bearings, very near and
very far landmarks, placed where lanes, waves and blocks meet, at the default grid and over several grid-stride steps with a
partial last wave (SBA_RESECT_GRID=1), dense and indexed.  tests/test_landmark_edges_cpu.py qualifies every row in every pass on
the CPU first; a row it drops from a combination gets a zero bearing there.  The reference is the long-double form that needs no
S^-1 (tests/landmark_edges_reference.py).  Classes and counts are exact; values are held, per kind of row, to 8 times float64
numpy's own worst error on the rows of that kind, measured in this run and pooled as tests/landmark_edges_reference.py says
(DESIGN.md section 3.25)."""
import numpy as np
import pytest

import landmark_edges as le
import landmark_edges_reference as er
import landmark_edit_reference as ed
import landmark_fusion_reference as lf
import landmark_register_reference as lr
import landmark_register_robust_reference as rb
from spherical_bundle_adjuster_amd import api
from test_gpu_landmark_register import TIGHT as PLAIN_TIGHT
from test_gpu_landmark_register import _check_posterior as check_register
from test_gpu_landmark_register_robust import TIGHT as ROBUST_TIGHT
from test_gpu_landmark_register_robust import _check_posterior as check_robust

pytestmark = pytest.mark.gpu

D = rb.DELTA
SIZES = pytest.mark.parametrize("n,grid", le.SIZES)


def _counts(f):
    return (f.n_obs, f.n_skipped, f.n_behind, f.n_gated, f.n_fused)


def _grid(monkeypatch, grid):
    if grid:
        monkeypatch.setenv("SBA_RESECT_GRID", grid)
    else:
        monkeypatch.delenv("SBA_RESECT_GRID", raising=False)


def _rows_within(err, bounds, s, rows, what):
    over = (err > bounds).any(axis=1)
    assert not over.any(), (what, [(s.names().get(int(rows[j]), "ordinary"), err[j], bounds[j]) for j in np.flatnonzero(over)])


def _report(what, err, q, bounds):
    held = er.by_kind(bounds, q.kinds)
    for k, v in er.by_kind(err, q.kinds).items():
        print(f"{what} {k:16s}: device {v}, bounds {held[k]}")


def _check_rows(L, X0, C0, chi2, cls_counts, q, pooled, s, rows, what, report, cnt0=0):
    """The handle's state and chi2 after a pass against q.ref: per-row classes (skipped: chi2 is NaN; fused: the landmark's count
    went up from cnt0; behind and gated by their totals), rows not fused untouched byte for byte, values within the per-kind bounds
    out of the pooled float64 errors `pooled`."""
    ref = q.ref
    bounds = er.row_bounds(q.kinds, pooled)
    assert cls_counts == ref.counts(), (what, cls_counts, ref.counts())
    assert np.array_equal(np.isnan(chi2), ref.cls == lf.SKIPPED), (what, np.flatnonzero(np.isnan(chi2) != (ref.cls == lf.SKIPPED)))
    touched = np.zeros(len(X0), dtype=bool)
    touched[rows[ref.cls == lf.FUSED]] = True
    assert np.array_equal(L.counts(), cnt0 + touched.astype(np.uint32)), what
    X1, C1 = L.get()
    assert X1[~touched].tobytes() == X0[~touched].tobytes() and C1[~touched].tobytes() == C0[~touched].tobytes(), what
    err = er.row_errors(X1[rows], C1[rows], chi2, ref, X0[rows], C0[rows])
    if report:
        _report(what, err, q, bounds)
    _rows_within(err, bounds, s, rows, what)
    return err


# ---- 1. the fuse -----------------------------------------------------------------------------------------------------------------
@SIZES
def test_fuse_on_the_edge_rows(monkeypatch, n, grid):
    _grid(monkeypatch, grid)
    s = le.scene(n)
    with api.Landmarks(0) as L:
        for bs in er.BEARING_SIGMAS:
            for pc in (None, lf.POSE_COV_FULL):
                for form, idx in le.forms(s):
                    q = er.fuse(n, bs, pc is not None, idx is not None)
                    what = f"fuse n={n} bs={bs} pose_cov={pc is not None} {form}"
                    rows = np.arange(n) if idx is None else idx
                    L.set(s.X, s.cov)
                    X0, C0 = L.get()
                    assert X0.tobytes() == s.X.tobytes() and C0.tobytes() == s.cov.tobytes()
                    f = L.fuse(q.y, s.rot, s.tran, bs, lf.GATE, pc, idx=idx)
                    _check_rows(L, X0, C0, f.chi2, _counts(f), q, er.fuse_pool(bs, pc is not None), s, rows, what, idx is None)
                    if bs == 0.0 and pc is None:
                        assert np.isnan(f.chi2[rows == s.rows["zero"]][0]), what              # a fixed landmark and an exact bearing


# ---- 2. one evaluation, plain and robust -----------------------------------------------------------------------------------------
@SIZES
def test_evaluations_on_the_edge_rows(monkeypatch, n, grid):
    _grid(monkeypatch, grid)
    worst = {}
    with api.Landmarks(0) as L:
        for pose in rb.POSE_NAMES:
            s = le.scene(n, pose)
            L.set(s.X, s.cov)
            before = L.get()
            for bs in er.BEARING_SIGMAS:
                for form, idx in le.forms(s):
                    rows = np.arange(n) if idx is None else idx
                    for robust in (False, True):
                        q = er.evaluation(s, bs, idx, D if robust else None)
                        what = f"{'robust ' if robust else ''}evaluation n={n} {pose} bs={bs} {form}"
                        if robust:
                            got = L.eval_register_robust(q.y, s.rot, s.tran, D, s.rot_ref, s.tran_ref, bs, idx=idx)
                            assert got.n_outlier == q.ref.n_outlier, what
                        else:
                            got = L.eval_register(q.y, s.rot, s.tran, s.rot_ref, s.tran_ref, bs, idx=idx)
                        assert (got.n_used, got.n_behind) == (q.ref.n_used, q.ref.n_behind), what
                        assert got.n_used == int((q.cls == lr.LIVE).sum()), what
                        assert np.array_equal(got.H, got.H.T), what
                        err = np.array(lr.eq_errors(got, q.ref))
                        bound = er.eval_bounds(bs, robust)
                        key = (bs, robust)
                        worst[key] = np.maximum(worst.get(key, np.zeros(3)), err)
                        assert (err <= bound).all(), (what, err, bound)
                        if not robust:
                            # a delta above every sqrt(chi2): the robust sums are the plain pass's bytes.  rb.BIG_DELTA where it is;
                            # with no bearing noise in the model the `tiny` priors, 0.2 degrees off their pose, have chi2 up to
                            # 3e12, beyond BIG_DELTA^2: there twice the reference's largest sqrt(chi2) of this evaluation
                            with np.errstate(all="ignore"):
                                chi2, used = rb.chi2_at(s.X[rows], s.cov[rows], q.y, q.noise, s.rot, s.tran, basis=lr.PROJECTED)
                            big_delta = max(rb.BIG_DELTA, 2.0 * float(np.sqrt(chi2[used].max())))
                            big = L.eval_register_robust(q.y, s.rot, s.tran, big_delta, s.rot_ref, s.tran_ref, bs, idx=idx)
                            assert (big.n_used, big.n_behind, big.n_outlier) == (got.n_used, got.n_behind, 0), what
                            assert big.H.tobytes() == got.H.tobytes() and big.g.tobytes() == got.g.tobytes() and big.cost == got.cost, what
            after = L.get()
            assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes() and not L.counts().any()
    for (bs, robust), err in worst.items():
        print(f"n={n} bs={bs} {'robust' if robust else 'plain'} evaluation: device worst (H, g, cost) {err}, bounds {er.eval_bounds(bs, robust)}")


# ---- 3. register and register_robust ---------------------------------------------------------------------------------------------
def _register(L, robust, y, rot, tran, bs, idx, options):
    if robust:
        return L.register_robust(y, rot, tran, D, bs, idx=idx, options=api.default_lm_options(**dict(ROBUST_TIGHT, **options)), return_chi2=True)
    return L.register(y, rot, tran, bs, lr.GATE, idx=idx, options=api.default_lm_options(**dict(PLAIN_TIGHT, **options)), return_chi2=True)


@SIZES
def test_registration_at_the_given_pose_on_the_edge_rows(monkeypatch, n, grid):
    """max_num_iterations = 0: the write-back of every edge row at the pose it was placed at, where the ill-conditioned priors are
    fused, not gated."""
    _grid(monkeypatch, grid)
    s = le.scene(n)
    zeros = np.zeros(n, dtype=np.uint32)
    with api.Landmarks(0) as L:
        for robust in (False, True):
            check = check_robust if robust else check_register
            for bs in er.BEARING_SIGMAS:
                for form, idx in le.forms(s):
                    q = er.posterior(s, bs, idx, D if robust else None, rot_ref=s.rot, tran_ref=s.tran)
                    what = f"{'robust ' if robust else ''}register at the pose n={n} bs={bs} {form}"
                    rows = np.arange(n) if idx is None else idx
                    L.set(s.X, s.cov)
                    X0, C0 = L.get()
                    f = _register(L, robust, q.y, s.rot, s.tran, bs, idx, dict(max_num_iterations=0))
                    assert np.array_equal(f.rot, s.rot) and np.array_equal(f.tran, s.tran), what
                    assert f.n_used == q.ref.eq.n_used, what
                    if robust:
                        assert f.n_outlier == q.ref.eq.n_outlier, what
                    _check_rows(L, X0, C0, f.chi2, _counts(f), q, er.posterior_pool(bs, robust, True), s, rows, what, idx is None)
                    with np.errstate(all="ignore"):
                        check(L, X0, C0, zeros, q.y, idx, s.rot, s.tran, bs, f, form=lr.PROJECTED)
                    if bs == 0.0:
                        assert np.isnan(f.chi2[rows == s.rows["zero"]][0]), what


@SIZES
def test_registration_solved_on_the_edge_rows(monkeypatch, n, grid):
    """From the start 2e-3 rad and 1e-2 units off, with the scene's bearing noise in the model: the pose against the long-double
    minimiser, (p - p*)^T H (p - p*) <= 1e-6, and the posterior at the device's pose."""
    _grid(monkeypatch, grid)
    s = le.scene(n)
    bs = s.bearing_sigma
    zeros = np.zeros(n, dtype=np.uint32)
    with api.Landmarks(0) as L:
        for robust in (False, True):
            check = check_robust if robust else check_register
            q = er.posterior(s, bs, None, D if robust else None, rot_ref=s.rot0, tran_ref=s.tran0)
            with np.errstate(all="ignore"):
                noise, _ = lr.freeze(s.X, s.cov, q.y, s.rot0, s.tran0, bs, basis=lr.PROJECTED)
                if robust:
                    rot_r, tran_r, eq_r, _ = rb.solve(s.X, s.cov, q.y, noise, s.rot0, s.tran0, D, basis=lr.PROJECTED)
                else:
                    rot_r, tran_r, eq_r, _ = lr.solve(s.X, s.cov, q.y, noise, s.rot0, s.tran0, basis=lr.PROJECTED)
            L.set(s.X, s.cov)
            X0, C0 = L.get()
            f = _register(L, robust, q.y, s.rot0, s.tran0, bs, None, {})
            dp = np.concatenate([f.rot - rot_r, f.tran - tran_r])
            maha2 = float(dp @ eq_r.H @ dp)
            print(f"n={n} {'robust ' if robust else ''}register solved: {f.summary.termination} after {f.summary.num_iterations} iterations, "
                  f"(p - p*)^T H (p - p*) = {maha2:.3e}, counts {_counts(f)}")
            assert maha2 <= 1e-6
            with np.errstate(all="ignore"):
                ref, err, bound = check(L, X0, C0, zeros, q.y, None, s.rot0, s.tran0, bs, f, form=lr.PROJECTED)
            print(f"    posterior errors {err} (X+, Sigma+, chi2, Sigma_c), bounds {bound}")
            edge = s.edge_rows()
            assert (ref.cls[edge] == lr.FUSED).mean() > 0.5


# ---- 4. six frames in sequence ---------------------------------------------------------------------------------------------------
@SIZES
def test_six_frames_in_sequence_on_the_device(monkeypatch, n, grid):
    """fuse six times on one handle, register_robust six times from starts 2e-3 rad off on another: after every frame classes,
    counts and state against one reference step from the handle's own state; no landmark that was fused before is skipped."""
    _grid(monkeypatch, grid)
    s = le.scene(n)
    bs = er.SEQUENCE_BEARING_SIGMA
    rows = np.arange(n)
    pool_f, pool_r = er.sequence_fuse_pool(), er.sequence_register_pool()
    total_f, total_r = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    XL, CL = np.asarray(s.X, dtype=lf.LD), np.asarray(s.cov, dtype=lf.LD)      # the fuse recursion that never leaves long double
    with api.Landmarks(0) as F, api.Landmarks(0) as R:
        F.set(s.X, s.cov)
        R.set(s.X, s.cov)
        for k, (yk, rot, tran) in enumerate(er.sequence(n)):
            X0, C0 = F.get()
            q = er.fuse_at(X0, C0, yk, rot, tran, bs, None, s, rows)
            assert not q.dropped, (k, q.dropped)                                # every edge row stays in the sequence
            f = F.fuse(q.y, rot, tran, bs, lf.GATE)
            assert not (np.isnan(f.chi2) & (total_f > 0)).any(), k
            _check_rows(F, X0, C0, f.chi2, _counts(f), q, pool_f, s, rows, f"sequence fuse frame {k}", False, total_f)
            with np.errstate(all="ignore"):
                pure = lf.fuse(XL, CL, q.y, rot, tran, bs, lf.GATE, None, projected=True)
            assert np.array_equal(pure.cls, q.ref.cls), (k, np.flatnonzero(pure.cls != q.ref.cls))
            XL, CL = pure.X, pure.cov
            total_f += (q.ref.cls == lf.FUSED).astype(np.uint32)
            X1, C1 = F.get()
            fused = q.ref.cls == lf.FUSED
            low = np.linalg.eigvalsh(er.wr.full(C1, np.float64))[:, 0]
            assert (low[fused] >= -er.row_bounds(q.kinds, pool_f)[fused, 1] * np.abs(C0[fused]).max(axis=1)).all(), k
            # the second handle: the pose is solved for, robustly
            X0, C0 = R.get()
            start = er.sequence_start(n, k, rot)
            g = R.register_robust(q.y, start, tran, D, bs, options=api.default_lm_options(**ROBUST_TIGHT), return_chi2=True)
            p = er.posterior(s, bs, None, D, rot=g.rot, tran=g.tran, rot_ref=start, tran_ref=tran, state=(X0, C0, q.y))
            assert not p.dropped, (k, p.dropped)                                # at the device's pose every row keeps its margins
            assert (g.n_used, g.n_outlier) == (p.ref.eq.n_used, p.ref.eq.n_outlier), k
            assert not (np.isnan(g.chi2) & (total_r > 0)).any(), k
            err = _check_rows(R, X0, C0, g.chi2, _counts(g), p, pool_r, s, rows, f"sequence register_robust frame {k}", False, total_r)
            total_r += (p.ref.cls == rb.FUSED).astype(np.uint32)
            print(f"sequence n={n} frame {k}: fuse {_counts(f)}, register_robust {_counts(g)} outliers {g.n_outlier}, "
                  f"pose off by {np.abs(g.rot - rot).max():.2e} rad, worst posterior errors {err.max(axis=0)}")
        assert total_f.max() == er.SEQUENCE_FRAMES and total_r.max() >= er.SEQUENCE_FRAMES - 1
        # against the recursion that never left long double: every frame adds at most one bound and the update does not amplify
        # (Sigma+ <= Sigma), so six bounds after six frames, relative to the first prior as in the three-frame test of the fusion.
        # Not the `vague` rows: their prior mean lies thousands of units off the ray, the update is far from linear there, and the
        # float64 recursion on the CPU itself drifts from 2e-11 to 4e-8 of |X| over the frames (classes are compared above)
        X6, C6 = F.get()
        bounds = er.SEQUENCE_FRAMES * er.row_bounds(q.kinds, pool_f)
        ex = np.abs(X6 - XL).max(axis=1) / np.linalg.norm(s.X, axis=1)
        ec = np.abs(C6 - CL).max(axis=1) / np.maximum(np.abs(s.cov).max(axis=1), 1e-300)
        over = ((ex > bounds[:, 0]) | (ec > bounds[:, 1])) & (q.kinds != "vague")
        print(f"sequence n={n}: after six frames against the long-double recursion X {float(ex.max()):.3e}, Sigma {float(ec.max()):.3e}")
        assert not over.any(), [(s.names().get(int(i), "ordinary"), float(ex[i]), float(ec[i]), bounds[i]) for i in np.flatnonzero(over)]


# ---- 5. scores and prune ---------------------------------------------------------------------------------------------------------
@SIZES
def test_scores_and_prune_on_the_edge_map(monkeypatch, n, grid):
    _grid(monkeypatch, grid)
    s = le.scene(n)
    with api.Landmarks(0) as L:
        L.set(s.X, s.cov)
        got = L.scores()
        want = ed.scores(s.X, s.cov)
        assert got.tobytes() == want.tobytes()
        assert got[s.rows["zero"]] == 0.0
        cut = ed.median_cut(want)
        assert ed.margin_ok(want, cut)
        kept, record = ed.prune(s.X, s.cov, np.zeros(n, dtype=np.uint32), max_score=cut)
        for apply in (False, True):
            p = L.prune(max_score=cut, apply=apply)
            assert (p.n_before, p.n_invalid, p.n_uncertain, p.n_unobserved, p.n_masked, p.n_kept) == record
            assert np.array_equal(p.kept, kept)
        X1, C1 = L.get()
        assert X1.tobytes() == s.X[kept].tobytes() and C1.tobytes() == s.cov[kept].tobytes()
        assert s.rows["zero"] in kept and 0 < len(kept) < n
