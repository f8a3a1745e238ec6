"""CPU: everything about the landmark map's edge rows (tests/landmark_edges.py) that needs no GPU.

1. The long-double reference that forms no S^-1 (landmark_register_reference.PROJECTED, landmark_fusion_reference.fuse(projected=True))
   against the inverse form the existing tests use, on every existing scene; exact rational arithmetic on the rows where the two
   differ most says which of them the difference belongs to.
2. The qualification: float64 numpy in the product's formulation against the new reference on every edge row in every pass (the
   fuse, the freeze, one evaluation at three poses, the write-back, the robust evaluation), the rows it drops and the cap on them.
3. csrc/sba_landmarks*.hpp compiled for the CPU on the same rows: classes exact, values within 8 times float64 numpy's own error
   on the rows of the same kind.
4. W^T W of the product's factor does not depend on the branch resect_weight_basis takes.
5. Six frames fused in sequence: classes of the float64 and the long-double recursion, and the smallest eigenvalue of every
   stored Sigma+."""
from fractions import Fraction

import numpy as np
import pytest

import landmark_edges as le
import landmark_edges_reference as er
import landmark_fusion_reference as lf
import landmark_register_reference as lr
import landmark_register_robust_reference as rb
import resection_weighted_reference as wr

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
# The spread between the two long-double formulations, pinned at about twice what was measured, so that a regression in either
# shows: M in units of eps cond(S)^2 (measured 0.10), what the references return in units of eps cond(S), cond(S) the scene's worst
# (measured: evaluation 189, posterior 1044, fuse 589, the robust solve scenes 576).
SPREAD_M, SPREAD_EVAL, SPREAD_POST, SPREAD_FUSE, SPREAD_ROBUST = 0.25, 400.0, 2000.0, 1200.0, 1200.0
NS = tuple(n for n, _ in le.SIZES)


# ---- 1. the two reference formulations -------------------------------------------------------------------------------------------
def _cond(S):
    w = np.linalg.eigvalsh(np.asarray(S, dtype=np.float64))
    return w[:, -1] / w[:, 0]


def _fraction(x):
    hi = float(x)
    return Fraction(hi) + Fraction(float(x - LD(hi)))


def _exact_weight(S, y):
    """M = S^-1 - S^-1 y y^T S^-1 / (y^T S^-1 y) of one long-double S and y in rational arithmetic, rounded to float64."""
    S = [[_fraction(S[i, j]) for j in range(3)] for i in range(3)]
    y = [_fraction(v) for v in y]
    a, b, c, d, e, f = S[0][0], S[0][1], S[0][2], S[1][1], S[1][2], S[2][2]
    A = [[d * f - e * e, c * e - b * f, b * e - c * d], [c * e - b * f, a * f - c * c, b * c - a * e], [b * e - c * d, b * c - a * e, a * d - b * b]]
    det = a * A[0][0] + b * A[0][1] + c * A[0][2]
    v = [sum(A[i][j] * y[j] for j in range(3)) / det for i in range(3)]
    vy = sum(v[i] * y[i] for i in range(3))
    return np.array([[float(A[i][j] / det - v[i] * v[j] / vy) for j in range(3)] for i in range(3)])


def test_the_projected_reference_agrees_with_the_inverse_form_on_every_existing_scene():
    """Classes and the frozen noise are identical.  M, relative to its largest entry, agrees within SPREAD_M eps cond(S)^2 per
    row: the inverse form cancels twice, in the cofactors and in the rank-one removal, and each costs a factor of cond(S).  What
    the references return (H, g, cost, X+, Sigma+, chi2, Sigma_c in the normalisations the tests compare them by) agrees within
    SPREAD_* eps cond(S), eps of long double, cond(S) the scene's worst.  That is not a small multiple of eps cond(S); rational
    arithmetic on the worst row shows that the whole of it is the inverse form's error."""
    worst = dict(eq=0.0, post=0.0, fuse=0.0, robust=0.0, M=0.0, M2=0.0, cond=0.0)
    worst_row = None
    for s in lr.scenes():
        for bs in lr.BEARING_SIGMAS:
            n0, c0 = lr.freeze(s.X, s.cov, s.y, s.rot_ref, s.tran_ref, bs)
            n1, c1 = lr.freeze(s.X, s.cov, s.y, s.rot_ref, s.tran_ref, bs, basis=lr.PROJECTED)
            assert np.array_equal(c0, c1) and np.array_equal(n0, n1, equal_nan=True), s.name
            a = lr.point(s.X, s.cov, s.y, n0, s.rot, s.tran)
            b = lr.point(s.X, s.cov, s.y, n0, s.rot, s.tran, basis=lr.PROJECTED)
            S = a.R[None] @ a.Sg @ a.R.T[None] + n0[:, None, None] * np.eye(3, dtype=LD)[None]
            cond = _cond(S)
            sp = (np.abs(a.M - b.M).max(axis=(1, 2)) / np.abs(b.M).max(axis=(1, 2))).astype(np.float64)
            assert (sp <= SPREAD_M * EPS_LD * cond * cond).all(), s.name
            i = int(np.argmax(sp))
            if sp[i] > worst["M"]:
                worst_row = (s.name, bs, S[i], np.asarray(s.y[i], dtype=LD), a.M[i], b.M[i])
            worst["M"], worst["M2"] = max(worst["M"], sp[i]), max(worst["M2"], float((sp / (EPS_LD * cond * cond)).max()))
            worst["cond"] = max(worst["cond"], cond.max())
            unit = EPS_LD * cond.max()
            e0 = lr.evaluate(s.X, s.cov, s.y, n0, s.rot, s.tran)
            e1 = lr.evaluate(s.X, s.cov, s.y, n0, s.rot, s.tran, basis=lr.PROJECTED)
            assert (e0.n_used, e0.n_behind) == (e1.n_used, e1.n_behind)
            eq = max(lr.eq_errors(e0, e1))
            post = 0.0
            if e1.n_used >= 3:                                                  # fewer leave H singular: no Sigma_c
                p0 = lr.posterior(s.X, s.cov, s.y, n0, s.rot, s.tran, lr.GATE)
                p1 = lr.posterior(s.X, s.cov, s.y, n0, s.rot, s.tran, lr.GATE, basis=lr.PROJECTED)
                assert np.array_equal(p0.cls, p1.cls), s.name
                post = max(lr.post_errors(p0.X, p0.cov, p0.chi2, p0.pose_cov, p1, s.X, s.cov))
            assert eq <= SPREAD_EVAL * unit and post <= SPREAD_POST * unit, (s.name, bs, eq / unit, post / unit)
            worst["eq"], worst["post"] = max(worst["eq"], eq / (EPS_LD * cond.max())), max(worst["post"], post / (EPS_LD * cond.max()))
    for s in lf.scenes():
        if not len(s.X):
            continue
        for bs, pc in lf.variants():
            f0 = lf.fuse(s.X, s.prior_cov, s.y, s.rot, s.tran, bs, lf.GATE, pc)
            f1 = lf.fuse(s.X, s.prior_cov, s.y, s.rot, s.tran, bs, lf.GATE, pc, projected=True)
            assert np.array_equal(f0.cls, f1.cls), s.name
            _, S, _, _, _ = lf._prior_cov_S(np.asarray(s.X, dtype=LD), np.asarray(s.prior_cov, dtype=LD), np.asarray(s.y, dtype=LD), s.rot, s.tran, bs, pc, LD)
            c = _cond(S).max()
            e = max(lf.errors(f0.X, f0.cov, f0.chi2, f1, s.X, s.prior_cov))
            assert e <= SPREAD_FUSE * EPS_LD * c, (s.name, bs, e / (EPS_LD * c))
            worst["fuse"], worst["cond"] = max(worst["fuse"], e / (EPS_LD * c)), max(worst["cond"], c)
    solve_scenes = [lr.solve_scene(n) for n in lr.SOLVE_SIZES + lr.SOLVE_LONG] + [rb.solve_scene(n) for n in rb.SOLVE_SIZES + rb.SOLVE_LONG]
    for s in solve_scenes:
        n0, c0 = lr.freeze(s.X, s.cov, s.y, s.rot0, s.tran0, s.bearing_sigma)
        n1, c1 = lr.freeze(s.X, s.cov, s.y, s.rot0, s.tran0, s.bearing_sigma, basis=lr.PROJECTED)
        assert np.array_equal(c0, c1) and np.array_equal(n0, n1, equal_nan=True), s.name
        a = lr.point(s.X, s.cov, s.y, n0, s.rot0, s.tran0)
        c = _cond(a.R[None] @ a.Sg @ a.R.T[None] + n0[:, None, None] * np.eye(3, dtype=LD)[None]).max()
        e0 = rb.evaluate(s.X, s.cov, s.y, n0, s.rot0, s.tran0, rb.DELTA)
        e1 = rb.evaluate(s.X, s.cov, s.y, n0, s.rot0, s.tran0, rb.DELTA, basis=lr.PROJECTED)
        assert (e0.n_used, e0.n_behind, e0.n_outlier) == (e1.n_used, e1.n_behind, e1.n_outlier)
        p0 = rb.posterior(s.X, s.cov, s.y, n0, s.rot0, s.tran0, rb.DELTA)
        p1 = rb.posterior(s.X, s.cov, s.y, n0, s.rot0, s.tran0, rb.DELTA, basis=lr.PROJECTED)
        assert np.array_equal(p0.cls, p1.cls), s.name
        e = max(max(lr.eq_errors(e0, e1)), max(lr.post_errors(p0.X, p0.cov, p0.chi2, p0.pose_cov, p1, s.X, s.cov)))
        assert e <= SPREAD_ROBUST * EPS_LD * c, (s.name, e / (EPS_LD * c))
        worst["robust"] = max(worst["robust"], e / (EPS_LD * c))
    print(f"spread between the two long-double formulations in units of eps cond(S), eps = {EPS_LD:.3e}, worst cond(S) {worst['cond']:.3e}: "
          f"evaluation {worst['eq']:.3f}, posterior {worst['post']:.3f}, fuse {worst['fuse']:.3f}, robust solve scenes {worst['robust']:.3f}; "
          f"M relative to its largest entry {worst['M']:.3e} = {worst['M2']:.3f} eps cond(S)^2")
    # whose error the spread in M is: rational arithmetic on the row where it is largest
    name, bs, S, y, Ma, Mb = worst_row
    Me = _exact_weight(S, y)
    ea = float(np.abs(Ma.astype(np.float64) - Me).max() / np.abs(Me).max())
    eb = float(np.abs(Mb.astype(np.float64) - Me).max() / np.abs(Me).max())
    print(f"{name} bs={bs}: against rational arithmetic the inverse form's M is off by {ea:.3e}, the projected form's by {eb:.3e} (float64 resolution)")
    assert eb <= 4 * np.finfo(np.float64).eps and ea >= eb


def test_the_projected_reference_holds_where_s_is_singular():
    """A prior of rank 2 across the ray with no bearing noise: S is singular, the inverse form divides by a determinant that is
    rounding noise, the projected form returns the weight of the 2 x 2 block."""
    s = le.scene(513)
    i = s.rows["across_only"]
    X, cov, y = s.X[i:i + 1], s.cov[i:i + 1], s.y[i:i + 1]
    f = lf.fuse(X, cov, y, s.rot, s.tran, 0.0, projected=True)
    assert f.cls[0] == lf.FUSED
    b = lf.fuse_basis(X, cov, y, s.rot, s.tran, 0.0)
    assert b.cls[0] == lf.FUSED and max(lf.errors(b.X, b.cov, b.chi2, f, X, cov)) < 1e-9
    # all of the prior's variance lies across the ray, and the bearing has no noise: nothing is left
    assert np.abs(f.cov).max() <= 1e-15 * np.abs(cov).max()
    with np.errstate(all="ignore"):
        old = lf.fuse(X, cov, y, s.rot, s.tran, 0.0)
    e_old = max(lf.errors(old.X, old.cov, old.chi2, f, X, cov)) if old.cls[0] == lf.FUSED else np.inf
    print(f"across_only at bearing_sigma 0: float64 numpy's error against the projected form {max(lf.errors(b.X, b.cov, b.chi2, f, X, cov)):.3e}, "
          f"the inverse form's {e_old:.3e}")


# ---- 2. and 3. the qualification and the host code on the same rows ----------------------------------------------------------
def _print_drops(what, dropped):
    for k, why in dropped.items():
        print(f"{what}: dropped '{k}': {why}")


def _survivors(seen, what):
    """seen: bearing_sigma -> set of dropped kinds.  Every kind survives for at least one bearing_sigma."""
    for kind in le.KINDS:
        assert any(kind not in d for d in seen.values()), f"{what}: kind '{kind}' is dropped for every bearing_sigma"


@pytest.mark.parametrize("n", NS)
def test_fuse_rows_qualify_and_the_header_matches(n):
    s = le.scene(n)
    zero = s.rows["zero"]
    for pc in (None, lf.POSE_COV_FULL):
        seen = {}
        for bs in er.BEARING_SIGMAS:
            for form, idx in le.forms(s):
                q = er.fuse(n, bs, pc is not None, idx is not None)
                what = f"fuse n={n} bs={bs} pose_cov={pc is not None} {form}"
                _print_drops(what, q.dropped)
                er.check_cap(q.dropped, what)
                seen.setdefault(bs, set()).update(er.dropped_kinds(q.dropped))
                rows = np.arange(n) if idx is None else idx
                assert "zero" not in q.dropped
                if bs == 0.0 and pc is None:
                    assert q.ref.cls[rows == zero][0] == lf.SKIPPED and q.got.cls[rows == zero][0] == lf.SKIPPED
                with np.errstate(all="ignore"):
                    h = lf.harness_fuse(s.X[rows], s.cov[rows], q.y, s.rot, s.tran, bs, lf.GATE, pc)
                assert np.array_equal(h.cls, q.ref.cls), (what, np.flatnonzero(h.cls != q.ref.cls))
                keep = q.ref.cls != lf.FUSED
                assert h.X[keep].tobytes() == s.X[rows][keep].tobytes() and h.cov[keep].tobytes() == s.cov[rows][keep].tobytes(), what
                err = er.row_errors(h.X, h.cov, h.chi2, q.ref, s.X[rows], s.cov[rows])
                bounds = er.row_bounds(q.kinds, er.fuse_pool(bs, pc is not None))
                over = err > bounds
                assert not over.any(), (what, [(s.names().get(int(rows[j]), "ordinary"), err[j], bounds[j]) for j in np.flatnonzero(over.any(axis=1))])
                if idx is None:
                    for k, v in er.by_kind(err, q.kinds).items():
                        print(f"{what} {k:16s}: header {v}, float64 numpy {er.by_kind(q.err, q.kinds)[k]}")
        _survivors(seen, f"fuse n={n} pose_cov={pc is not None}")


@pytest.mark.parametrize("n", NS)
def test_freeze_evaluation_and_write_back_qualify_and_the_headers_match(n):
    seen = {p: {} for p in ("evaluation", "robust evaluation", "write-back", "robust write-back")}
    for pose in rb.POSE_NAMES:
        s = le.scene(n, pose)
        zero = s.rows["zero"]
        for bs in er.BEARING_SIGMAS:
            for form, idx in le.forms(s):
                rows = np.arange(n) if idx is None else idx
                X, cov = s.X[rows], s.cov[rows]
                for delta, name in ((None, "evaluation"), (rb.DELTA, "robust evaluation")):
                    q = er.evaluation(s, bs, idx, delta)
                    what = f"{name} n={n} {pose} bs={bs} {form}"
                    _print_drops(what, q.dropped)
                    er.check_cap(q.dropped, what)
                    seen[name].setdefault(bs, set()).update(er.dropped_kinds(q.dropped))
                    assert "zero" not in q.dropped
                    if bs == 0.0:
                        assert q.cls[rows == zero][0] == lr.SKIPPED
                    with np.errstate(all="ignore"):
                        nh, ch = lr.harness_freeze(X, cov, q.y, s.rot_ref, s.tran_ref, bs)
                        assert np.array_equal(ch, q.cls), (what, np.flatnonzero(ch != q.cls))
                        live = lr.live_of(q.noise)
                        ref_n = q.noise.astype(np.float64)
                        own = np.abs(q.noise64[live] - ref_n[live]).max()       # bearing_sigma 0: every s^2 is 0, and the bound too
                        assert np.abs(nh[live] - ref_n[live]).max() <= 8.0 * max(own, np.finfo(np.float64).eps * np.abs(ref_n[live]).max()), what
                        got = lr.harness_eval(X, cov, q.y, nh, s.rot, s.tran) if delta is None else rb.harness_eval(X, cov, q.y, nh, s.rot, s.tran, delta)
                    assert (got.n_used, got.n_behind) == (q.ref.n_used, q.ref.n_behind), what
                    if delta is not None:
                        assert got.n_outlier == q.ref.n_outlier, what
                    assert np.array_equal(got.H, got.H.T), what
                    err = np.array(lr.eq_errors(got, q.ref))
                    bound = er.eval_bounds(bs, delta is not None)
                    print(f"{what}: header (H, g, cost) {err}, float64 numpy {q.err}, bounds {bound}, used {got.n_used} behind {got.n_behind}")
                    assert (err <= bound).all(), (what, err, bound)
                for delta, name in ((None, "write-back"), (rb.DELTA, "robust write-back")):
                    p = er.posterior(s, bs, idx, delta)
                    what = f"{name} n={n} {pose} bs={bs} {form}"
                    er.check_cap(p.dropped, what)
                    seen[name].setdefault(bs, set()).update(er.dropped_kinds(p.dropped))
                    if bs == 0.0:
                        assert p.ref.cls[rows == zero][0] == lr.SKIPPED
                    with np.errstate(all="ignore"):
                        nh, _ = lr.harness_freeze(X, cov, p.y, s.rot_ref, s.tran_ref, bs)
                        Xo, Co, chi2, c2 = lr.harness_apply(X, cov, p.y, nh, s.rot, s.tran, p.ref.pose_cov.astype(np.float64), lr.GATE if delta is None else rb.GATE)
                    assert np.array_equal(c2, p.ref.cls), (what, np.flatnonzero(c2 != p.ref.cls))
                    keep = p.ref.cls != lr.FUSED
                    assert Xo[keep].tobytes() == X[keep].tobytes() and Co[keep].tobytes() == cov[keep].tobytes(), what
                    err = er.row_errors(Xo, Co, chi2, p.ref, X, cov)
                    bounds = er.row_bounds(p.kinds, er.posterior_pool(bs, delta is not None, False))
                    over = err > bounds
                    assert not over.any(), (what, [(s.names().get(int(rows[j]), "ordinary"), err[j], bounds[j]) for j in np.flatnonzero(over.any(axis=1))])
    for name, d in seen.items():
        _survivors(d, f"{name} n={n}")


# ---- 4. the projector does not depend on the branch ----------------------------------------------------------------------------
def _projector(S6, y):
    ok, q = wr.harness_factor(S6, y)
    assert ok
    return wr.harness_rows(q[None], np.asarray(y, dtype=np.float64)[None])[0]


def test_the_projector_does_not_depend_on_the_basis_branch():
    """For every axis and tie bearing and its one-ulp neighbours: W^T W of the product's factor (csrc/sba_resection_weighted.hpp on
    the CPU) against the long-double projected weight of the same S and y, within 8 times float64 numpy's own error on these rows;
    across the neighbours of a tie, whose S and y differ by an ulp, the same bound holds between them.  The branch differs within
    every tie that lies between the two smallest components (or all three); with a zero component the zero is the smallest for
    every neighbour, so there the branch cannot differ, which is asserted too."""
    s = le.scene(513)
    names = [c.name for c in le.CASES if c.kind in ("axis", "negative_zero", "tie", "tie_of_smallest")]
    R = er.rr.rotmat(s.rot, LD)
    got, ref, num = {}, {}, {}
    for k in names:
        i = s.rows[k]
        y = s.y[i]
        S = (R @ wr.full(s.cov[i:i + 1], LD)[0] @ R.T)
        S6 = wr.rows_of(S[None])[0].astype(np.float64)
        M = lr.projected_weight(wr.full(S6[None], LD), np.asarray(y, dtype=LD)[None])
        ref[k] = wr.rows_of(M)[0]
        got[k] = _projector(S6, y)
        W, _, zero = wr.basis_factor(np.zeros((1, 3)), y[None], S6[None], np.zeros(3), np.zeros(3), 1.0, 0.0)
        assert not zero[0]
        num[k] = wr.basis_rows(W)[0]
    scale = lambda k: float(np.abs(ref[k]).max())
    own = max(float(np.abs(num[k] - ref[k]).max()) / scale(k) for k in names)
    bound = 8.0 * own
    worst = max(float(np.abs(got[k] - ref[k]).max()) / scale(k) for k in names)
    print(f"W^T W against the projected weight: the header's worst {worst:.3e}, float64 numpy's {own:.3e}, bound {bound:.3e}")
    assert worst <= bound
    ties = {}
    for c in le.CASES:
        if c.tie is not None:
            ties.setdefault((c.kind, c.tie), {})[c.moved] = c
    for (kind, tie), group in ties.items():
        branches = {m: le.product_branch(group[m].y) for m in (-1, 0, 1)}
        at_smallest = kind == "tie_of_smallest" or 0.0 not in [abs(v) for v in group[0].y]
        assert (len(set(branches.values())) > 1) == at_smallest, (tie, branches)
    # the same S under a bearing and its neighbours: here W^T W must agree across the branches directly
    S6 = wr.rows_of((R @ wr.full(s.cov[s.rows["vague"]:s.rows["vague"] + 1], LD)[0] @ R.T)[None])[0].astype(np.float64)
    direct = 0.0
    for (kind, tie), group in ties.items():
        P = {m: _projector(S6, np.array(group[m].y)) for m in (-1, 0, 1)}
        for m in (-1, 1):
            direct = max(direct, float(np.abs(P[m] - P[0]).max() / np.abs(P[0]).max()))
    print(f"one S under every tie and its one-ulp neighbours: W^T W differs by at most {direct:.3e} (bound {bound:.3e})")
    assert direct <= bound


# ---- 5. six frames in sequence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_six_frames_in_sequence_keep_every_covariance_usable(n):
    """After every frame the float64 recursion (the product's formulation feeding itself) classifies as the long-double recursion
    does, and every stored Sigma+ has its smallest eigenvalue above minus the row's bound (8 times float64's own error there)."""
    s = le.scene(n)
    bs = er.SEQUENCE_BEARING_SIGMA
    pooled = er.sequence_fuse_pool()
    XL, CL = np.asarray(s.X, dtype=LD), np.asarray(s.cov, dtype=LD)
    C64 = np.array(s.cov)
    fused_before = np.zeros(n, dtype=bool)
    for k, ((yk, rot, tran), q) in enumerate(zip(er.sequence(n), er.sequence_fuse(n))):
        assert not q.dropped, (k, q.dropped)                                    # every edge row stays in the sequence
        with np.errstate(all="ignore"):
            pure = lf.fuse(XL, CL, q.y, rot, tran, bs, lf.GATE, None, projected=True)
        assert np.array_equal(pure.cls, q.got.cls), (k, [(s.names().get(int(i), "ordinary"), pure.cls[i], q.got.cls[i]) for i in np.flatnonzero(pure.cls != q.got.cls)])
        lost = fused_before & (q.got.cls == lf.SKIPPED)
        assert not lost.any(), (k, [s.names().get(int(i), "ordinary") for i in np.flatnonzero(lost)])
        scale = np.abs(C64).max(axis=1)                     # the Sigma+ error is relative to the largest entry of the row's prior
        C64 = q.got.cov
        XL, CL = pure.X, pure.cov
        low = np.linalg.eigvalsh(wr.full(C64, np.float64))[:, 0]
        floor = -er.row_bounds(q.kinds, pooled)[:, 1] * scale
        f = q.got.cls == lf.FUSED
        worst = int(np.argmin(np.where(f, low, np.inf)))
        print(f"sequence n={n} frame {k}: counts {q.got.counts()}, smallest eigenvalue of a stored Sigma+ at row {worst} "
              f"({s.names().get(worst, 'ordinary')}): {low[worst]:.3e}, allowed {floor[worst]:.3e}")
        assert (low[f] >= floor[f]).all(), (k, [(s.names().get(int(i), "ordinary"), low[i], floor[i]) for i in np.flatnonzero(f & (low < floor))])
        fused_before |= f
