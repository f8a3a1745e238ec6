"""Shared by the match-edge tests (tests/ only): the references of tests/match_edges.py's scenes, their qualification and the bounds.

Every reference is a long-double form the project has already: ref_joint_numpy.JointProblem.blocks (residuals, weights, Jacobian
blocks), schur_of_blocks' elimination (the reduced system) and ref_depth_numpy's d-only block, written here over a dtype so that the
SAME formulation runs in float64 numpy and in long double.  The rule is landmark_edges_reference.py's: float64 numpy is compared with
long double; its worst error on the scenes of a kind -- pooled over REPEAT seeds, both sizes, both poses, both stores -- is what
float64 can do there, and the host code and the kernels are held to 8 times that, never less than 8 times its worst error on the
ordinary scenes.  Wherever 8 times float64's error ALSO meets the flat bound the project states already (REL_TOL_F64 of the largest
entry, the measure of tests/test_gpu_pose_edges.py), the kernels are held to that flat bound as well: a kind is not let off a bound
that float64 meets.

Errors of a summed output are relative to the long-double sum of the absolute per-match terms of that entry: a `far` row moves a
sum by 1e12, and an error of 1e-4 in it is 1e-16 of what was added up.  Per-row outputs (residuals, depths) are measured per row,
over the edge rows of the kind and, for the floor, over every row of the ordinary scenes.

TABLE holds one entry per (kind, pass), none skipped:

    bound        held to 8 * TABLE's errors (abs-sum measure, flat measure or None where float64 misses the flat bound)
    exact        bytes (the exact scene)
    non_finite   the reference divides by an exactly zero determinant there: float64 numpy AND long double under
                 eval_joint(radius = inf); float64 numpy under the solves started at SINGULAR_RADIUS = 1e16, where D / radius is
                 below half an ulp of the block in float64 (long double still resolves it; what the solvers must DO is float64's:
                 an invalid first step).  The kernels must give non-finite reduced outputs (not finite garbage), leave the
                 unreduced outputs within the bound, take the step as invalid -- one iteration, no successful step, two passes,
                 the radius halved, nothing moved, to the byte -- and the handle must then answer as a fresh one.  Only at pose
                 "zero": at "closed" fl(R0 x1) is parallel to R0 x1 up to rounding, the determinant is rounding noise of either
                 sign, and nothing can be demanded of it.
    refused      with the error code (no case of this suite is refused: negative depths are legal inputs of every entry point)

A row is DROPPED from a combination (it keeps the ordinary match, match_edges.scene(revert=...)) only by name and with the reason:
float64 numpy classifies it differently from long double, or its s lies within MARGIN relative of delta^2.  At most CAP of the edge
rows of a scene.

The measured errors below were produced by `PYTHONPATH=. python tests/match_edges_reference.py` (CPU, numpy float64 against numpy long double)."""
import sys
from functools import lru_cache

import numpy as np

import match_edges as me
import pose_edges as pe
import ref_joint_numpy as rj
from helpers import REL_TOL_F64

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
MARGIN = 1e-9                        # landmark_register_reference.MARGIN
CAP = 1.0 / 8.0
RADII = (float("inf"), 1e4, 1.0, 1e-2)           # tests/test_gpu_joint.py
DELTAS = (1.0, 0.0)
UNIFORM = (3.0, 5.0)                 # d1, d2 of the uniform-depth sweeps
MODES = (0, 1, 2)
DEPTH_UNIFORM, DEPTH_PER_MATCH = 0, 1
SOLVE_SIZE = 513                     # the d-only solves run one block of either small-problem driver
JOINT_SIZE = 257                     # the joint solves have a dense restatement: (2 n + 6)^2 entries an iteration
JOINT_REPEAT = 2
DEPTH_ITERATIONS = (1, 3)
SINGULAR_RADIUS = 1e16               # fma(D, 1 / radius, H) == H from here on for D == H == 0.25


# ---- the per-match terms ---------------------------------------------------------------------------------------------------------
def _blocks(c, f32, delta, dt, d=None):
    x1, x2 = pe.planes(c, f32)
    with np.errstate(all="ignore"):
        return rj.JointProblem(x1, x2, delta).blocks(c.rot_init, c.tran_init, c.d12 if d is None else d, dt)


def classes(c, f32, delta, dt, d=None):
    """s per match and the outlier flags."""
    e = _blocks(c, f32, delta, dt, d)[0]
    s = np.sum(e * e, axis=1)
    return s, (s > dt(delta) * dt(delta)) if delta > 0 else np.zeros(len(s), dtype=bool)


def sweep_terms(c, f32, mode, depth_mode, delta, dt):
    """(n, 24): what every match adds to the explicit pack of include/sba_hip.h (slot 23: the outlier flag)."""
    n = len(c.x1)
    d = c.d12 if depth_mode == DEPTH_PER_MATCH else np.tile(np.array(UNIFORM), (n, 1))
    e, w, _, F = _blocks(c, f32, delta, dt, d)
    A = F[:, :, :3]
    s = np.sum(e * e, axis=1)
    rho, _ = rj.huber(delta, s)
    T = np.zeros((n, 24), dtype=dt)
    if mode in (0, 2):
        k = 0
        for a in range(3):
            for b in range(a, 3):
                T[:, k] = w * np.sum(A[:, :, a] * A[:, :, b], axis=1)
                k += 1
        for a in range(3):
            T[:, 16 + a] = w * np.sum(A[:, :, a] * e, axis=1)
    if mode == 2:
        for a in range(3):
            for cc in range(3):
                T[:, 6 + 3 * a + cc] = w * A[:, cc, a]
    if mode in (1, 2):
        T[:, 15] = w
        T[:, 19:22] = w[:, None] * e
    T[:, 22] = 0.5 * rho
    T[:, 23] = (s > dt(delta) * dt(delta)) if delta > 0 else 0
    return T


def joint_terms(c, f32, radius, delta, dt, jacobi=True, min_diag=1e-6, max_diag=1e32):
    """ref_joint_numpy.schur_of_blocks per match: dict of (n, ...) arrays V, gc, S, gs, cost, sum_w, gd (n, 2), det (n,)."""
    e, w, E, F = _blocks(c, f32, delta, dt)
    with np.errstate(all="ignore"):
        EtE = np.einsum("nri,nrj->nij", E, E) * w[:, None, None]
        EtF = np.einsum("nri,nrj->nij", E, F) * w[:, None, None]
        FtF = np.einsum("nri,nrj->nij", F, F) * w[:, None, None]
        gd = np.einsum("nri,nr->ni", E, e) * w[:, None]
        gc = np.einsum("nri,nr->ni", F, e) * w[:, None]
        dg = np.stack([EtE[:, 0, 0], EtE[:, 1, 1]], axis=1)
        s = 1 / (1 + np.sqrt(dg)) if jacobi else np.ones_like(dg)
        U = EtE * s[:, :, None] * s[:, None, :]
        if np.isfinite(radius):
            D = np.clip(np.stack([U[:, 0, 0], U[:, 1, 1]], axis=1), dt(min_diag), dt(max_diag)) / dt(radius)
            U[:, 0, 0] += D[:, 0]
            U[:, 1, 1] += D[:, 1]
        W, G = EtF * s[:, :, None], gd * s
        det = U[:, 0, 0] * U[:, 1, 1] - U[:, 0, 1] * U[:, 1, 0]
        Ui = np.empty_like(U)
        Ui[:, 0, 0], Ui[:, 1, 1], Ui[:, 0, 1], Ui[:, 1, 0] = U[:, 1, 1] / det, U[:, 0, 0] / det, -U[:, 0, 1] / det, -U[:, 1, 0] / det
        T = np.einsum("nia,nij,njb->nab", W, Ui, W)
        tg = np.einsum("nia,nij,nj->na", W, Ui, G)
        rho, _ = rj.huber(delta, np.sum(e * e, axis=1))
    return dict(V=FtF, gc=gc, S=FtF - T, gs=gc - tg, cost=0.5 * rho, sum_w=w, gd=gd, det=det)


def sums(T):
    """The sum over matches of every entry of a dict of per-match terms, and the sum of their absolute values."""
    with np.errstate(all="ignore"):
        return {k: v.sum(0) for k, v in T.items()}, {k: np.abs(v).sum(0) for k, v in T.items()}


def sum_errors(got, ref_sum, ref_abs):
    """The worst |got - ref| / sum |terms| over the entries of an output (abs-sum measure); 0 where nothing was added up."""
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(got, dtype=LD) - ref_sum)
        r = np.where(ref_abs > 0, d / np.where(ref_abs > 0, ref_abs, 1), np.where(d > 0, np.inf, 0))
    return float(np.max(r, initial=0.0))


def flat_error(got, ref_sum):
    """The project's flat measure: the worst |got - ref| over the largest |ref| of the output."""
    with np.errstate(all="ignore"):
        return float(np.abs(np.asarray(got, dtype=LD) - ref_sum).max() / max(np.abs(ref_sum).max(), LD(1e-300)))


# ---- the d-only stage over a dtype -----------------------------------------------------------------------------------------------
class DepthShard:
    """tests/test_depth_solver_cpu.py's EmulatedShard in `dt`: what depth_step_kernel does per match, on ref_depth_numpy's block."""

    def __init__(self, c, f32, dt, lam=1.0, cc=1.0, min_diag=1e-6, max_diag=1e32, accurate_det=False, fused=False):
        x1, x2 = pe.planes(c, f32)
        self.dt = dt
        self.fused = fused                   # float64 only: the step's numerators as the compiler's fma contraction rounds them
        self.accurate_det = accurate_det     # float64 only: every determinant exact and rounded once, as csrc's depth_block_det
        self.q = x1.astype(dt) @ rj.rotation(c.rot_init, dt).T
        self.u, self.t = x2.astype(dt), c.tran_init.astype(dt)
        self.lam, self.c, self.min_diag, self.max_diag = dt(lam), dt(cc), dt(min_diag), dt(max_diag)
        self.d = c.d12.astype(dt).copy()
        self.cand, self.scale, self.delta = self.d.copy(), None, None

    def _cost_grad(self, d):
        e = d[:, 1:2] * self.u - d[:, 0:1] * self.q + self.t
        reg = self.lam * np.exp(-self.c * d)
        g = np.stack([-np.sum(self.q * e, axis=1) - self.c * reg[:, 0] ** 2, np.sum(self.u * e, axis=1) - self.c * reg[:, 1] ** 2], axis=1)
        return 0.5 * (np.sum(e * e) + np.sum(reg * reg)), g, reg

    def run_pass(self, alpha, keep_diagonal, first, radius):
        dt, d = self.dt, self.d
        with np.errstate(all="ignore"):
            cost, g, reg = self._cost_grad(d)
            h11 = np.sum(self.q * self.q, axis=1) + (self.c * reg[:, 0]) ** 2
            h22 = np.sum(self.u * self.u, axis=1) + (self.c * reg[:, 1]) ** 2
            h12 = -np.sum(self.q * self.u, axis=1)
            if first:
                self.scale = np.stack([1 / (1 + np.sqrt(h11)), 1 / (1 + np.sqrt(h22))], axis=1)
            s = self.scale
            H11, H12, H22 = s[:, 0] ** 2 * h11, s[:, 0] * s[:, 1] * h12, s[:, 1] ** 2 * h22
            G = s * g
            A11 = H11 + np.clip(H11, self.min_diag, self.max_diag) / dt(radius)
            A22 = H22 + np.clip(H22, self.min_diag, self.max_diag) / dt(radius)
            det = A11 * A22 - H12 * H12
            if self.accurate_det:
                det = (A11.astype(LD) * A22 - H12.astype(LD) * H12).astype(dt)
            y = np.stack([(-G[:, 0] * A22 + G[:, 1] * H12) / det, (-G[:, 1] * A11 + G[:, 0] * H12) / det], axis=1)
            if self.fused:              # the numerators as a fused multiply-add forms them: one product exact, the other rounded
                n1 = (G[:, 1].astype(LD) * H12 - (G[:, 0] * A22).astype(LD)).astype(dt)
                n2 = (G[:, 0].astype(LD) * H12 - (G[:, 1] * A11).astype(LD)).astype(dt)
                y = np.stack([n1 / det, n2 / det], axis=1)
            self.det = det
            self.delta = s * y
            self.cand = np.maximum(d + dt(alpha) * self.delta, 0)         # numpy's maximum keeps a NaN: a NaN step stays visible
            cc, cg, _ = self._cost_grad(self.cand)
            out = [cost, -np.sum(G * y) - 0.5 * np.sum(H11 * y[:, 0] ** 2 + 2 * H12 * y[:, 0] * y[:, 1] + H22 * y[:, 1] ** 2),
                   cc, np.sum((self.cand - d) ** 2), np.sum(d * d), np.sum(g * self.delta), np.sum(cg * self.delta)]
            maxima = [np.abs(d - np.maximum(d - g, 0)).max(initial=0), np.abs(self.delta).max(initial=0)]
        return np.array(out, dtype=np.float64), np.array(maxima, dtype=np.float64)

    def take_candidate(self):
        self.d = self.cand.copy()


def summary_tuple(s):
    return (int(s.termination), int(s.num_iterations), int(s.num_successful_steps), int(s.num_evaluations), int(s.num_line_search_steps))


@lru_cache(maxsize=None)
def depth_solve(kind, pose, n, rep, f32, iterations, long_double, radius=1e4, revert=(), axis_row=True, accurate_det=False, fused=False):
    """The product's d-only state machine (csrc/sba_depth_solver.hpp through tests/harness/depth_harness.cpp) over DepthShard's
    passes -> depths (float64), summary tuple, status, whether the first pass held a non-finite step."""
    from test_depth_solver_cpu import drive
    sh = DepthShard(me.scene(kind, pose, n, rep, revert, axis_row), f32, LD if long_double else np.float64, accurate_det=accurate_det, fused=fused)
    seen = []
    run = sh.run_pass

    def spy(*a):
        out = run(*a)
        seen.append(bool(np.isfinite(sh.delta.astype(np.float64)).all()))
        return out
    sh.run_pass = spy
    d, s, status, _ = drive(sh, max_num_iterations=iterations, initial_trust_region_radius=radius,
                            max_trust_region_radius=max(radius, 1e16))
    return np.asarray(d, dtype=np.float64), summary_tuple(s), status, not seen[0]


def depth_row_errors(got, ref):
    """|d - ref| / max(1, |ref|) per row (the worse of the two depths)."""
    with np.errstate(all="ignore"):
        return (np.abs(np.asarray(got, dtype=LD) - ref) / np.maximum(1, np.abs(ref))).max(axis=1).astype(np.float64)


# ---- the joint solve -------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def joint_solve(kind, pose, n, rep, f32, radius=1e4, iterations=50, revert=(), accurate_det=False):
    """The product's joint state machine over numpy-emulated float64 passes (joint_emulation.EmulatedJoint / drive), and the dense
    restatement rj.dense_solve -> ((rot, tran, d, summary tuple, status), (rot, tran, d, summary dict)).  accurate_det: the
    numpy passes form every 2 x 2 determinant exactly and round it once, a third float64 formulation: at radius 5e15 the plain
    a d - b^2 of a parallel match is the difference of two roundings, wrong by its own size."""
    from joint_emulation import EmulatedJoint, drive

    class Adjugate(EmulatedJoint):
        """EmulatedJoint with the 2 x 2 blocks inverted as the kernels do, adjugate over determinant: a singular block gives
        inf and NaN where numpy.linalg.inv raises."""

        def _block(self, rot, tran, radius, first):
            inv = np.linalg.inv

            def adjugate(U):
                if accurate_det:        # the product of float64s is exact in long double: the determinant rounded once
                    det = (U[:, 0, 0].astype(LD) * U[:, 1, 1] - U[:, 0, 1].astype(LD) * U[:, 1, 0]).astype(np.float64)
                else:
                    det = U[:, 0, 0] * U[:, 1, 1] - U[:, 0, 1] * U[:, 1, 0]
                Ui = np.empty_like(U)
                Ui[:, 0, 0], Ui[:, 1, 1], Ui[:, 0, 1], Ui[:, 1, 0] = U[:, 1, 1] / det, U[:, 0, 0] / det, -U[:, 0, 1] / det, -U[:, 1, 0] / det
                return Ui
            np.linalg.inv = adjugate
            try:
                return super()._block(rot, tran, radius, first)
            finally:
                np.linalg.inv = inv
    EmulatedJoint = Adjugate
    c = me.scene(kind, pose, n, rep, revert)
    x1, x2 = pe.planes(c, f32)
    kw = dict(initial_trust_region_radius=radius, max_trust_region_radius=max(radius, 1e16), max_num_iterations=iterations)
    with np.errstate(all="ignore"):
        r, t, d, s, status, _, _ = drive(EmulatedJoint(x1, x2, c.d12), c.rot_init, c.tran_init, **kw)
        dense = rj.dense_solve(x1, x2, c.rot_init, c.tran_init, c.d12, **kw)
    return (r, t, d, (int(s.termination), int(s.num_iterations), int(s.num_successful_steps), int(s.num_evaluations)), status), dense


# ---- qualification ---------------------------------------------------------------------------------------------------------------
def drops(c, f32, delta=1.0):
    """{row: reason} of the edge rows whose class cannot be demanded equal at the scene's own depths and at the uniform ones."""
    out = {}
    n = len(c.x1)
    for d in (None, np.tile(np.array(UNIFORM), (n, 1))):
        s64, o64 = classes(c, f32, delta, np.float64, d)
        sld, old = classes(c, f32, delta, LD, d)
        with np.errstate(all="ignore"):
            near = np.abs(sld - LD(delta) ** 2) <= MARGIN * LD(delta) ** 2
        for i in np.flatnonzero(near | (o64 != old)):
            assert i in c.rows, f"{c.name}: ordinary row {i} sits on delta^2"
            out.setdefault(int(i), "s within 1e-9 of delta^2" if near[i] else "float64 numpy classifies it differently")
    return out


def check_cap(dropped, what):
    assert len(dropped) <= CAP * me.N_EDGE, f"{what}: {len(dropped)} of {me.N_EDGE} edge rows dropped: {dropped}"


@lru_cache(maxsize=None)
def qualified(kind, pose, n, rep, f32):
    """The scene of the combination with its dropped rows reverted, and {row: reason}."""
    c = me.scene(kind, pose, n, rep)
    dropped = drops(c, f32) if kind != "ordinary" else {}
    check_cap(dropped, c.name)
    c2 = me.scene(kind, pose, n, rep, tuple(sorted(dropped)))
    assert kind == "ordinary" or not drops(c2, f32), c2.name
    return c2, dropped


def _pool(acc, key, value):
    acc[key] = np.maximum(acc.get(key, 0.0), value)


def combos(kind, sizes=me.SIZES, poses=me.POSES):
    return [(kind, pose, n, rep, f32) for pose in poses for n in sizes for rep in range(me.REPEAT) for f32 in (False, True)]


def residual_scale(c, f32):
    """max(1, |d1| |x1| + |d2| |x2| + |t|): tests/test_gpu_batch_select.py's scale with the bearings' lengths."""
    x1, x2 = pe.planes(c, f32)
    return np.maximum(1.0, np.abs(c.d12[:, 0]) * np.linalg.norm(x1, axis=1) + np.abs(c.d12[:, 1]) * np.linalg.norm(x2, axis=1) + np.linalg.norm(c.tran_init))


def sweep_reference(c, f32, mode, depth_mode, delta):
    return sums({"pack": sweep_terms(c, f32, mode, depth_mode, delta, LD)})


def measure_sweep(kind):
    """float64 numpy's worst (abs-sum, flat) errors of the packs over the kind's combinations; the outlier counts must be equal."""
    worst = np.zeros(2)
    for key in combos(kind):
        c, _ = qualified(*key)
        for mode in MODES:
            for dm in (DEPTH_UNIFORM, DEPTH_PER_MATCH):
                for delta in DELTAS:
                    ref, ab = sweep_reference(c, key[4], mode, dm, delta)
                    got = sweep_terms(c, key[4], mode, dm, delta, np.float64).sum(0)
                    assert got[23] == ref["pack"][23], (c.name, mode, dm, delta)
                    worst = np.maximum(worst, [sum_errors(got[:23], ref["pack"][:23], ab["pack"][:23]), flat_error(got[:23], ref["pack"][:23])])
    return worst


def residual_reference(c, f32):
    e = _blocks(c, f32, 1.0, LD)[0]
    return e, np.sum(e * e, axis=1)


def residual_errors(e, sq, c, f32, ref=None):
    """Per row: |e - ref| / scale and |sq_norm - ref| / scale^2, the worse of the two."""
    re, rs = residual_reference(c, f32) if ref is None else ref
    sc = residual_scale(c, f32)
    with np.errstate(all="ignore"):
        return np.maximum(np.abs(np.asarray(e, dtype=LD) - re).max(axis=1) / sc, np.abs(np.asarray(sq, dtype=LD) - rs) / (sc * sc)).astype(np.float64)


def _rows_of(c, kind):
    return np.arange(len(c.x1)) if kind == "ordinary" else c.rows


def measure_residuals(kind):
    worst = 0.0
    for key in combos(kind):
        c, _ = qualified(*key)
        e = _blocks(c, key[4], 1.0, np.float64)[0]
        worst = max(worst, float(residual_errors(e, np.sum(e * e, axis=1), c, key[4])[_rows_of(c, kind)].max()))
    return np.array([worst, np.nan])


JOINT_KEYS = ("V", "gc", "S", "gs", "cost", "sum_w")
REDUCED = ("S", "gs")


def joint_reference(c, f32, radius, delta=1.0):
    """-> sums, abs-sums, gd_max (long double) and whether some determinant is exactly zero in long double AND in float64."""
    T = joint_terms(c, f32, radius, delta, LD)
    det64 = joint_terms(c, f32, radius, delta, np.float64)["det"]
    singular = bool(((T["det"] == 0) & (det64 == 0)).any())
    gd = T.pop("gd")
    T.pop("det")
    s, a = sums(T)
    return s, a, float(np.abs(gd).max(initial=0)), singular


def singular_in_float64(c, f32, radius):
    """Some depth block's determinant is exactly zero in float64 numpy (long double still resolves D / radius at 1e16)."""
    return bool((joint_terms(c, f32, radius, 1.0, np.float64)["det"] == 0).any())


def joint_errors(got, ref, ab, keys=JOINT_KEYS):
    """(abs-sum, flat) errors of one reduce pass; flat as tests/test_gpu_joint.py's _check_reduced: S and V relative to max |V|,
    gs and gc to max(max |V|, max |gc|), cost and sum_w to themselves."""
    with np.errstate(all="ignore"):
        sV = np.abs(ref["V"]).max()
        scale = dict(S=sV, V=sV, gs=max(sV, np.abs(ref["gc"]).max()), gc=max(sV, np.abs(ref["gc"]).max()), cost=ref["cost"], sum_w=ref["sum_w"])
        flat = max(float(np.abs(np.asarray(got[k], dtype=LD) - ref[k]).max() / scale[k]) for k in keys)
    return np.array([max(sum_errors(got[k], ref[k], ab[k]) for k in keys), flat])


def _joint64(c, f32, radius):
    T = joint_terms(c, f32, radius, 1.0, np.float64)
    T.pop("gd"), T.pop("det")
    return sums(T)[0]


def measure_eval_joint(kind, radii, poses=me.POSES):
    """-> worst (abs-sum, flat) errors over the finite combinations, and the number of non-finite ones (both arithmetics)."""
    worst, non_finite, finite = np.zeros(2), 0, 0
    for key in combos(kind, poses=poses):
        c, _ = qualified(*key)
        for radius in radii:
            ref, ab, _, singular = joint_reference(c, key[4], radius)
            got = _joint64(c, key[4], radius)
            if singular:
                assert not all(np.isfinite(got[k].astype(np.float64)).all() for k in REDUCED), (c.name, radius)
                assert not all(np.isfinite(ref[k].astype(np.float64)).all() for k in REDUCED), (c.name, radius)
                non_finite += 1
                worst = np.maximum(worst, joint_errors(got, ref, ab, ("V", "gc", "cost", "sum_w")))
            else:
                finite += 1
                worst = np.maximum(worst, joint_errors(got, ref, ab))
    return worst, non_finite, finite


def measure_depth(kind):
    """float64's worst per-row depth error after 1 and 3 iterations of the d-only stage against long double; the summaries of the
    two arithmetics must agree (else the comparison is of two different runs)."""
    worst = 0.0
    for key in combos(kind, sizes=(SOLVE_SIZE,)):
        c, dropped = qualified(*key)
        for it in DEPTH_ITERATIONS:
            a = depth_solve(*key, it, False, revert=tuple(sorted(dropped)))
            b = depth_solve(*key, it, True, revert=tuple(sorted(dropped)))
            assert a[1] == b[1] and a[2] == b[2] == 0, (c.name, it, a[1:], b[1:])
            worst = max(worst, float(depth_row_errors(a[0], b[0])[_rows_of(c, kind)].max()))
    return np.array([worst, np.nan])


def measure_depth_singular(kind):
    """One iteration of the d-only stage from SINGULAR_RADIUS: non_finite where float64 numpy's pass holds a non-finite step (the
    step is invalid, the radius halves, the depths stay), else float64's per-row error against long double.  float64 forms
    every determinant exactly and rounds it once here, which is the product's formulation (csrc/sba_device.hpp depth_block_det):
    with the plain a d - b^2 a nearly parallel row's determinant at this radius is the difference of two roundings and float64's
    own error 57 % of a depth on `antiparallel` -- a bound that would demand nothing."""
    worst, nf, fin = 0.0, 0, 0
    for key in combos(kind, sizes=(SOLVE_SIZE,), poses=entry_poses(kind, "depth_1e16")):
        c, dropped = qualified(*key)
        a = depth_solve(*key, 1, False, SINGULAR_RADIUS, tuple(sorted(dropped)), accurate_det=True)
        if a[3]:
            nf += 1
            assert a[1] == (4, 1, 0, 2, 0) and a[2] == 0 and np.array_equal(a[0], c.d12), (c.name, a[1:])
            # The continuation (3 iterations): at radius 5e15 the damping is one ulp of the block and the step's numerators
            # G2 A12 - G1 A22 are differences of products that agree to that ulp.  Long double takes another path (its first step
            # is valid), so float64's own error is what its formulations differ by: plain products, exactly rounded determinants,
            # and numerators with one product exact as a fused multiply-add leaves it.  Their summaries must agree.
            rv = tuple(sorted(dropped))
            ref3 = depth_solve(*key, 3, False, SINGULAR_RADIUS, rv, accurate_det=True)
            for kw in (dict(), dict(accurate_det=True, fused=True)):
                b = depth_solve(*key, 3, False, SINGULAR_RADIUS, rv, **kw)
                assert b[1] == ref3[1] and b[2] == 0, (c.name, b[1], ref3[1])
                worst = max(worst, float(depth_row_errors(b[0], ref3[0])[_rows_of(c, kind)].max()))
        else:
            fin += 1
            b = depth_solve(*key, 1, True, SINGULAR_RADIUS, tuple(sorted(dropped)))
            assert a[1] == b[1] and a[2] == b[2] == 0, (c.name, a[1:], b[1:])
            worst = max(worst, float(depth_row_errors(a[0], b[0])[_rows_of(c, kind)].max()))
    assert nf == 0 or fin == 0, (kind, nf, fin)
    return ("non_finite" if nf else "bound", worst, np.nan)


def joint_combos(kind, pas):
    return [(kind, pose, JOINT_SIZE, rep, f32) for pose in entry_poses(kind, pas) for rep in range(JOINT_REPEAT) for f32 in (False, True)]


def joint_solve_errors(a, b):
    """(rot, tran) absolute and depths relative to the largest depth: the measures of tests/test_gpu_joint.py."""
    with np.errstate(all="ignore"):
        return max(float(np.abs(a[0] - b[0]).max()), float(np.abs(a[1] - b[1]).max()), float(np.abs(a[2] - b[2]).max() / np.abs(b[2]).max()))


def counts_of_dense(s):
    return ({v: k for k, v in rj.TERM.items()}[s["termination"]], s["num_iterations"], s["num_successful_steps"], s["num_evaluations"])


# Whole solves from SINGULAR_RADIUS whose counts are demanded of the device, at least, per kind and store: measured on the CPU
# (test_match_edges_cpu.py asserts it), `parallel` has rep 1 with f64 planes and both reps with f32 planes on which the numpy
# passes, the dense restatement and the passes with exactly rounded determinants end with the same termination and counts; on
# `antiparallel` and `far_parallel` the three differ among themselves (27 / 11 / 12 iterations on antiparallel rep 0).
SINGULAR_FAIR_MIN = {"parallel": 1, "antiparallel": 0, "far_parallel": 0}


def singular_solve_is_fair(key, revert=()):
    """The whole joint solve of the combination from SINGULAR_RADIUS ends alike in three float64 formulations and converged."""
    emu, dense = joint_solve(*key, SINGULAR_RADIUS, 50, revert)
    third, _ = joint_solve(*key, SINGULAR_RADIUS, 50, revert, True)
    return emu[3] == counts_of_dense(dense[3]) == third[3] and dense[3]["termination"] in ("function", "gradient", "parameter")


def fair_yardstick(emu, dense):
    """A solve whose counts can be demanded of another float64 implementation: the two formulations agree on termination and
    counts, no test of the dense run sat on its threshold (margin >= 1e-3, the rule of tests/test_gpu_joint.py), and the run
    CONVERGED.  A run that is still moving after 50 iterations has no fixed point pulling its iterates together, and roundings
    grow along it: on far pose=closed n=257 rep=1 one ulp on some of the input depths moves the count of successful steps between
    37 and 38 and the final cost in its third digit (measured with the numpy passes, CPU), at a margin of 281."""
    return emu[3] == counts_of_dense(dense[3]) and dense[3]["margin"] >= 1e-3 and dense[3]["termination"] in ("function", "gradient", "parameter")


def measure_solve_joint(kind, pas):
    """The product's joint state machine over float64 numpy passes against the dense float64 restatement -- two formulations in
    one arithmetic, there is no long-double solve: their disagreement is what float64 leaves open.  solve_joint: to termination
    from the default radius, over the combinations that are a fair yardstick (fair_yardstick), at least half of them.  solve_joint_1e16: one iteration from SINGULAR_RADIUS; non_finite where
    the first reduced system is not finite (invalid step, the radius halves, nothing moves)."""
    worst, nf, fin, fair = 0.0, 0, 0, 0
    keys = joint_combos(kind, pas)
    for key in keys:
        c, dropped = qualified(*key)
        rv = tuple(sorted(dropped))
        if pas == "solve_joint":
            emu, dense = joint_solve(*key, revert=rv)
            if fair_yardstick(emu, dense):
                fair += 1
                worst = max(worst, joint_solve_errors(emu, dense))
            continue
        emu, dense = joint_solve(*key, SINGULAR_RADIUS, 1, rv)
        if singular_in_float64(c, key[4], SINGULAR_RADIUS):
            nf += 1
            assert emu[3] == (4, 1, 0, 2) and emu[4] == 0 and np.array_equal(emu[2], c.d12), (c.name, emu[3:])
            assert np.array_equal(emu[0], c.rot_init) and np.array_equal(emu[1], c.tran_init)
        else:
            fin += 1
            assert emu[3] == counts_of_dense(dense[3]), (c.name, emu[3], dense[3])
            worst = max(worst, joint_solve_errors(emu, dense))
    if pas == "solve_joint":
        assert 2 * fair >= len(keys), (kind, fair, len(keys))
        return ("bound", worst, np.nan)
    assert nf == 0 or fin == 0, (kind, nf, fin)
    return ("non_finite" if nf else "bound", worst, np.nan)


COV_REPEAT = 2
COV_CUT = 1e-9                       # min_sin2_parallax of the covariance and structure passes


def cov_keep(c, f32):
    """The rows min_sin2_parallax = COV_CUT keeps; no row may sit within a factor 3 of the cut (the count is then the same in any
    arithmetic)."""
    s2 = me.sin2(c, f32)
    assert not ((s2 > COV_CUT / 3) & (s2 < COV_CUT * 3)).any(), c.name
    return s2 > COV_CUT


def cov_structure_reference(c, f32, dt=LD):
    """tests/test_gpu_covariance.py's schur_covariances and tests/test_gpu_structure.py's schur_structure on the kept rows, sphere
    gauge -> (DenseCov with depth_cov, DenseStructure), rows indexed like keep's True entries."""
    from test_gpu_covariance import schur_covariances
    from test_gpu_structure import schur_structure
    keep = cov_keep(c, f32)
    x1, x2 = pe.planes(c, f32)
    with np.errstate(all="ignore"):
        cv = schur_covariances(x1[keep], x2[keep], c.rot_init, c.tran_init, c.d12[keep], dt=dt)[1]
        st = schur_structure(x1[keep], x2[keep], c.rot_init, c.tran_init, c.d12[keep], dt=dt)[1]
    return keep, cv, st


def _rel_rows(got, ref):
    with np.errstate(all="ignore"):
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        if got.ndim == 1:
            return np.abs(got - ref) / np.abs(ref)
        return np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)


def cov_errors(got_cov, got_dd, ref):
    """-> (pose block error relative to its largest entry, per kept row the depth block's error relative to its largest entry)."""
    return float(np.abs(got_cov - ref.cov).max() / np.abs(ref.cov).max()), _rel_rows(got_dd, ref.depth_cov)


def structure_errors(xyz, cov, score, ref):
    """Per kept row: the worst of xyz relative to |X|, the covariance row relative to its largest entry, the score relative."""
    with np.errstate(all="ignore"):
        ex = np.abs(np.asarray(xyz) - ref.xyz).max(axis=1) / np.linalg.norm(ref.xyz, axis=1)
    return np.maximum(ex, np.maximum(_rel_rows(cov, ref.cov), _rel_rows(score, ref.score)))


def cov_combos(kind):
    return [(kind, pose, n, rep, f32) for pose in me.POSES for n in me.SIZES for rep in range(COV_REPEAT) for f32 in (False, True)]


def kept_rows_of(c, kind, keep):
    """Positions among the kept rows of the kind's edge rows (every kept row of an ordinary scene)."""
    idx = np.flatnonzero(keep)
    return np.arange(len(idx)) if kind == "ordinary" else np.flatnonzero(np.isin(idx, c.rows))


def measure_cov_structure(kind, pas):
    """float64 numpy's Schur forms against long double's on the rows min_sin2_parallax keeps: the worst per-row error of the kind's
    rows (depth blocks; landmark, covariance and score) and, as the flat figure, of the pose block."""
    worst, pose = 0.0, 0.0
    for key in cov_combos(kind):
        c, _ = qualified(*key)
        keep, cv, st = cov_structure_reference(c, key[4])
        _, cv64, st64 = cov_structure_reference(c, key[4], np.float64)
        rows = kept_rows_of(c, kind, keep)
        ep, ed = cov_errors(cv64.cov, cv64.depth_cov, cv)
        pose = max(pose, ep)
        if len(rows):
            e = ed[rows] if pas == "covariance" else structure_errors(st64.xyz, st64.cov, st64.score, st)[rows]
            assert np.isfinite(e).all(), (c.name, pas)
            worst = max(worst, float(e.max()))
    return ("bound", worst, pose)


def pose_bound(kind):
    """The bound of the pose block: 8 times the larger of float64's error on the kind's scenes and on the ordinary ones."""
    return 8.0 * max(TABLE[kind, "covariance"][2], TABLE["ordinary", "covariance"][2])


def entry_poses(kind, pas):
    """The poses a (kind, pass) is measured and tested at: exactly parallel rays are exactly singular at rot = 0 only -- at
    "closed" fl(R0 x1) is parallel to R0 x1 up to rounding and the determinant is rounding noise of either sign."""
    if pas in ("eval_joint_inf", "depth_1e16", "solve_joint_1e16") and kind in me.PARALLEL_KINDS:
        return ("zero",)
    return me.POSES


def measure(kind, pas):
    """-> (class, abs-sum error, flat error)."""
    if pas == "sweep":
        return ("bound",) + tuple(measure_sweep(kind))
    if pas == "residuals":
        return ("bound",) + tuple(measure_residuals(kind))
    if pas == "eval_joint":
        w, nf, _ = measure_eval_joint(kind, RADII[1:])
        assert nf == 0, (kind, nf)
        return ("bound",) + tuple(w)
    if pas == "eval_joint_inf":
        w, nf, fin = measure_eval_joint(kind, RADII[:1], entry_poses(kind, pas))
        assert nf == 0 or fin == 0, (kind, nf, fin)          # a kind is one or the other
        return ("non_finite" if nf else "bound",) + tuple(w)
    if pas == "depth":
        return ("bound",) + tuple(measure_depth(kind))
    if pas == "depth_1e16":
        return measure_depth_singular(kind)
    if pas in ("solve_joint", "solve_joint_1e16"):
        return measure_solve_joint(kind, pas)
    if pas in ("covariance", "structure"):
        return measure_cov_structure(kind, pas)
    raise KeyError(pas)


def _ceil2(v):
    """Up to two significant digits."""
    if not np.isfinite(v) or v == 0:
        return float(v)
    p = 10.0 ** (np.floor(np.log10(v)) - 1)
    return float(np.ceil(v / p) * p)


PASSES = ("sweep", "residuals", "eval_joint", "eval_joint_inf", "depth", "depth_1e16", "solve_joint", "solve_joint_1e16", "covariance",
          "structure")

# (kind, pass) -> (class, float64 numpy's worst abs-sum (or per-row) error, its worst flat error or nan); `python
# tests/match_edges_reference.py` (with PYTHONPATH=.) prints this table (CPU, float64 numpy against long double numpy, rounded up to two digits).
NAN = float("nan")
TABLE = {
    ("ordinary", "sweep"): ("bound", 2.4000000000000002e-14, 8.8e-15),
    ("ordinary", "residuals"): ("bound", 4.5e-16, NAN),
    ("ordinary", "eval_joint"): ("bound", 7.3e-14, 2.0000000000000003e-14),
    ("ordinary", "eval_joint_inf"): ("bound", 1.1e-13, 3.7e-14),
    ("ordinary", "depth"): ("bound", 9.800000000000001e-12, NAN),
    ("ordinary", "depth_1e16"): ("bound", 2.4e-11, NAN),
    ("ordinary", "solve_joint"): ("bound", 5.3e-13, NAN),
    ("ordinary", "solve_joint_1e16"): ("bound", 6.4e-13, NAN),
    ("parallel", "sweep"): ("bound", 2.4000000000000002e-14, 8.6e-15),
    ("parallel", "residuals"): ("bound", 1.4e-16, NAN),
    ("parallel", "eval_joint"): ("bound", 1.2e-13, 2.1000000000000002e-14),
    ("parallel", "eval_joint_inf"): ("non_finite", 3.5e-15, 3.4e-15),
    ("parallel", "depth"): ("bound", 7.6e-13, NAN),
    ("parallel", "depth_1e16"): ("bound", 0.0021000000000000003, NAN),
    ("parallel", "solve_joint"): ("bound", 6.7e-12, NAN),
    ("parallel", "solve_joint_1e16"): ("non_finite", 0.0, NAN),
    ("antiparallel", "sweep"): ("bound", 2.3000000000000003e-14, 8e-15),
    ("antiparallel", "residuals"): ("bound", 4.3000000000000004e-16, NAN),
    ("antiparallel", "eval_joint"): ("bound", 1.4e-13, 2.1000000000000002e-14),
    ("antiparallel", "eval_joint_inf"): ("non_finite", 3.5e-15, 3.4e-15),
    ("antiparallel", "depth"): ("bound", 5.9e-11, NAN),
    ("antiparallel", "depth_1e16"): ("bound", 0.5700000000000001, NAN),
    ("antiparallel", "solve_joint"): ("bound", 4.9e-13, NAN),
    ("antiparallel", "solve_joint_1e16"): ("non_finite", 0.0, NAN),
    ("weak_1e-6", "sweep"): ("bound", 2.4000000000000002e-14, 8.7e-15),
    ("weak_1e-6", "residuals"): ("bound", 1.0000000000000001e-16, NAN),
    ("weak_1e-6", "eval_joint"): ("bound", 8.2e-14, 2.0000000000000003e-14),
    ("weak_1e-6", "eval_joint_inf"): ("bound", 2.1e-11, 4.6e-12),
    ("weak_1e-6", "depth"): ("bound", 7.699999999999999e-11, NAN),
    ("weak_1e-6", "depth_1e16"): ("bound", 7.3e-10, NAN),
    ("weak_1e-6", "solve_joint"): ("bound", 6.000000000000001e-08, NAN),
    ("weak_1e-6", "solve_joint_1e16"): ("bound", 0.0, NAN),
    ("weak_1e-10", "sweep"): ("bound", 2.4000000000000002e-14, 8.6e-15),
    ("weak_1e-10", "residuals"): ("bound", 1.2e-16, NAN),
    ("weak_1e-10", "eval_joint"): ("bound", 8.5e-14, 2.1000000000000002e-14),
    ("weak_1e-10", "eval_joint_inf"): ("bound", 2.2e-07, 3.1e-08),
    ("weak_1e-10", "depth"): ("bound", 7.6e-13, NAN),
    ("weak_1e-10", "depth_1e16"): ("bound", 5.7999999999999995e-06, NAN),
    ("weak_1e-10", "solve_joint"): ("bound", 3.3e-10, NAN),
    ("weak_1e-10", "solve_joint_1e16"): ("bound", 0.0, NAN),
    ("weak_1e-14", "sweep"): ("bound", 2.4000000000000002e-14, 8.5e-15),
    ("weak_1e-14", "residuals"): ("bound", 1.2e-16, NAN),
    ("weak_1e-14", "eval_joint"): ("bound", 1.2e-13, 2.0000000000000003e-14),
    ("weak_1e-14", "eval_joint_inf"): ("bound", 0.0016, 0.00028000000000000003),
    ("weak_1e-14", "depth"): ("bound", 7.2e-13, NAN),
    ("weak_1e-14", "depth_1e16"): ("bound", 0.033, NAN),
    ("weak_1e-14", "solve_joint"): ("bound", 2.4e-11, NAN),
    ("weak_1e-14", "solve_joint_1e16"): ("bound", 0.0, NAN),
    ("d1_zero", "sweep"): ("bound", 2.4000000000000002e-14, 8.7e-15),
    ("d1_zero", "residuals"): ("bound", 3.8e-16, NAN),
    ("d1_zero", "eval_joint"): ("bound", 7.7e-14, 2.1000000000000002e-14),
    ("d1_zero", "eval_joint_inf"): ("bound", 1.2e-13, 4.0000000000000006e-14),
    ("d1_zero", "depth"): ("bound", 2.1000000000000002e-14, NAN),
    ("d1_zero", "depth_1e16"): ("bound", 1.5000000000000002e-14, NAN),
    ("d1_zero", "solve_joint"): ("bound", 3.2e-12, NAN),
    ("d1_zero", "solve_joint_1e16"): ("bound", 1.3e-09, NAN),
    ("d2_zero", "sweep"): ("bound", 2.4000000000000002e-14, 8.6e-15),
    ("d2_zero", "residuals"): ("bound", 4.7e-16, NAN),
    ("d2_zero", "eval_joint"): ("bound", 7.7e-14, 2.1000000000000002e-14),
    ("d2_zero", "eval_joint_inf"): ("bound", 1.4e-13, 4.0000000000000006e-14),
    ("d2_zero", "depth"): ("bound", 2.0000000000000003e-14, NAN),
    ("d2_zero", "depth_1e16"): ("bound", 1.4e-14, NAN),
    ("d2_zero", "solve_joint"): ("bound", 1.2000000000000001e-12, NAN),
    ("d2_zero", "solve_joint_1e16"): ("bound", 5.3000000000000004e-12, NAN),
    ("both_zero", "sweep"): ("bound", 2.7000000000000002e-14, 1.1e-14),
    ("both_zero", "residuals"): ("bound", 1.2e-16, NAN),
    ("both_zero", "eval_joint"): ("bound", 8.400000000000001e-14, 2.1000000000000002e-14),
    ("both_zero", "eval_joint_inf"): ("bound", 6.2e-13, 3.9000000000000004e-14),
    ("both_zero", "depth"): ("bound", 1.3000000000000001e-14, NAN),
    ("both_zero", "depth_1e16"): ("bound", 6.7e-16, NAN),
    ("both_zero", "solve_joint"): ("bound", 1.2000000000000001e-12, NAN),
    ("both_zero", "solve_joint_1e16"): ("bound", 3.3e-12, NAN),
    ("near", "sweep"): ("bound", 2.4000000000000002e-14, 8.6e-15),
    ("near", "residuals"): ("bound", 2.7e-16, NAN),
    ("near", "eval_joint"): ("bound", 7.6e-14, 2.1000000000000002e-14),
    ("near", "eval_joint_inf"): ("bound", 2.6e-13, 4.0000000000000006e-14),
    ("near", "depth"): ("bound", 1.4e-14, NAN),
    ("near", "depth_1e16"): ("bound", 7.800000000000001e-16, NAN),
    ("near", "solve_joint"): ("bound", 4e-13, NAN),
    ("near", "solve_joint_1e16"): ("bound", 6.7e-12, NAN),
    ("far", "sweep"): ("bound", 2.4000000000000002e-14, 8.6e-15),
    ("far", "residuals"): ("bound", 1.3000000000000002e-16, NAN),
    ("far", "eval_joint"): ("bound", 1.4e-12, 9.300000000000001e-14),
    ("far", "eval_joint_inf"): ("bound", 3.4000000000000003e-09, 1.3e-11),
    ("far", "depth"): ("bound", 3e-11, NAN),
    ("far", "depth_1e16"): ("bound", 5.4e-07, NAN),
    ("far", "solve_joint"): ("bound", 9.800000000000001e-12, NAN),
    ("far", "solve_joint_1e16"): ("bound", 5.2e-08, NAN),
    ("far_parallel", "sweep"): ("bound", 5.8e-10, 1.9e-11),
    ("far_parallel", "residuals"): ("bound", 1.4e-16, NAN),
    ("far_parallel", "eval_joint"): ("bound", 5.4e-10, 1.9e-11),
    ("far_parallel", "eval_joint_inf"): ("non_finite", 4.5999999999999996e-11, 8.9e-12),
    ("far_parallel", "depth"): ("bound", 1.2e-16, NAN),
    ("far_parallel", "depth_1e16"): ("non_finite", 4.8e-07, NAN),
    ("far_parallel", "solve_joint"): ("bound", 6e-13, NAN),
    ("far_parallel", "solve_joint_1e16"): ("non_finite", 0.0, NAN),
    ("negative", "sweep"): ("bound", 2.4000000000000002e-14, 8.7e-15),
    ("negative", "residuals"): ("bound", 6.9e-17, NAN),
    ("negative", "eval_joint"): ("bound", 7.4e-14, 2.1000000000000002e-14),
    ("negative", "eval_joint_inf"): ("bound", 1.2e-13, 4.0000000000000006e-14),
    ("negative", "depth"): ("bound", 2.4e-15, NAN),
    ("negative", "depth_1e16"): ("bound", 7.800000000000001e-16, NAN),
    ("negative", "solve_joint"): ("bound", 5.1e-13, NAN),
    ("negative", "solve_joint_1e16"): ("bound", 2e-12, NAN),
    ("axis", "sweep"): ("bound", 2.4000000000000002e-14, 8.6e-15),
    ("axis", "residuals"): ("bound", 8.3e-17, NAN),
    ("axis", "eval_joint"): ("bound", 7.500000000000001e-14, 2.1000000000000002e-14),
    ("axis", "eval_joint_inf"): ("bound", 1.2e-13, 4.7e-14),
    ("axis", "depth"): ("bound", 9.900000000000001e-12, NAN),
    ("axis", "depth_1e16"): ("bound", 4e-11, NAN),
    ("axis", "solve_joint"): ("bound", 1.1e-12, NAN),
    ("axis", "solve_joint_1e16"): ("bound", 3.4e-12, NAN),
    ("negative_zero", "sweep"): ("bound", 2.4000000000000002e-14, 8.8e-15),
    ("negative_zero", "residuals"): ("bound", 1.1000000000000001e-16, NAN),
    ("negative_zero", "eval_joint"): ("bound", 7.6e-14, 2.1000000000000002e-14),
    ("negative_zero", "eval_joint_inf"): ("bound", 2e-13, 9.500000000000001e-14),
    ("negative_zero", "depth"): ("bound", 1.5e-11, NAN),
    ("negative_zero", "depth_1e16"): ("bound", 3.9e-11, NAN),
    ("negative_zero", "solve_joint"): ("bound", 1.2000000000000001e-12, NAN),
    ("negative_zero", "solve_joint_1e16"): ("bound", 2e-12, NAN),
    ("length_1e-3", "sweep"): ("bound", 2.4000000000000002e-14, 8.4e-15),
    ("length_1e-3", "residuals"): ("bound", 1.5000000000000002e-16, NAN),
    ("length_1e-3", "eval_joint"): ("bound", 7.200000000000001e-14, 2.1000000000000002e-14),
    ("length_1e-3", "eval_joint_inf"): ("bound", 1.3e-13, 4.1e-14),
    ("length_1e-3", "depth"): ("bound", 2.8e-11, NAN),
    ("length_1e-3", "depth_1e16"): ("bound", 6.1e-11, NAN),
    ("length_1e-3", "solve_joint"): ("bound", 5.1e-13, NAN),
    ("length_1e-3", "solve_joint_1e16"): ("bound", 5.7e-12, NAN),
    ("length_1e+3", "sweep"): ("bound", 3.7e-13, 5.9e-15),
    ("length_1e+3", "residuals"): ("bound", 1.1000000000000001e-16, NAN),
    ("length_1e+3", "eval_joint"): ("bound", 7.200000000000001e-14, 2.1000000000000002e-14),
    ("length_1e+3", "eval_joint_inf"): ("bound", 9.7e-14, 4.3000000000000006e-14),
    ("length_1e+3", "depth"): ("bound", 1.8e-12, NAN),
    ("length_1e+3", "depth_1e16"): ("bound", 7.5e-12, NAN),
    ("length_1e+3", "solve_joint"): ("bound", 6.8e-13, NAN),
    ("length_1e+3", "solve_joint_1e16"): ("bound", 1.2000000000000001e-12, NAN),
    ("ordinary", "covariance"): ("bound", 4e-12, 6.1e-14),
    ("ordinary", "structure"): ("bound", 4e-12, 6.1e-14),
    ("parallel", "covariance"): ("bound", 0.0, 6.4e-14),
    ("parallel", "structure"): ("bound", 0.0, 6.4e-14),
    ("antiparallel", "covariance"): ("bound", 0.0, 6.4e-14),
    ("antiparallel", "structure"): ("bound", 0.0, 6.4e-14),
    ("weak_1e-6", "covariance"): ("bound", 4.9e-10, 7.7e-12),
    ("weak_1e-6", "structure"): ("bound", 4.9e-10, 7.7e-12),
    ("weak_1e-10", "covariance"): ("bound", 0.0, 6.4e-14),
    ("weak_1e-10", "structure"): ("bound", 0.0, 6.4e-14),
    ("weak_1e-14", "covariance"): ("bound", 0.0, 6.4e-14),
    ("weak_1e-14", "structure"): ("bound", 0.0, 6.4e-14),
    ("d1_zero", "covariance"): ("bound", 2.7000000000000002e-12, 6.4e-14),
    ("d1_zero", "structure"): ("bound", 2.7000000000000002e-12, 6.4e-14),
    ("d2_zero", "covariance"): ("bound", 4.8000000000000005e-12, 6.4e-14),
    ("d2_zero", "structure"): ("bound", 4.8000000000000005e-12, 6.4e-14),
    ("both_zero", "covariance"): ("bound", 3.4e-11, 1.1e-13),
    ("both_zero", "structure"): ("bound", 3.4e-11, 1.1e-13),
    ("near", "covariance"): ("bound", 4.4e-12, 5.8e-14),
    ("near", "structure"): ("bound", 4.4e-12, 5.8e-14),
    ("far", "covariance"): ("bound", 9.5e-11, 3.9000000000000004e-14),
    ("far", "structure"): ("bound", 9.5e-11, 3.9000000000000004e-14),
    ("far_parallel", "covariance"): ("bound", 0.0, 6.4e-14),
    ("far_parallel", "structure"): ("bound", 0.0, 6.4e-14),
    ("negative", "covariance"): ("bound", 1.8e-12, 6.1e-14),
    ("negative", "structure"): ("bound", 1.8e-12, 6.1e-14),
    ("axis", "covariance"): ("bound", 1.7e-11, 5.3e-14),
    ("axis", "structure"): ("bound", 1.7e-11, 5.3e-14),
    ("negative_zero", "covariance"): ("bound", 9.4e-12, 6.600000000000001e-14),
    ("negative_zero", "structure"): ("bound", 9.4e-12, 6.600000000000001e-14),
    ("length_1e-3", "covariance"): ("bound", 4.2e-12, 6.5e-14),
    ("length_1e-3", "structure"): ("bound", 4.2e-12, 6.5e-14),
    ("length_1e+3", "covariance"): ("bound", 3.5e-12, 6.5e-14),
    ("length_1e+3", "structure"): ("bound", 3.5e-12, 6.5e-14),
}


# the `residual` cases live in the exact scene: bytes, on every pass that forms a residual class
EXACT_PASSES = ("sweep", "residuals", "eval_joint")
EXACT_TABLE = {(k, p): "exact" for k in me.RESIDUAL for p in EXACT_PASSES}


def bound(kind, pas):
    """(abs-sum or per-row bound, flat bound or None) of the kind: 8 times the larger of its own and the ordinary scenes' measured
    error; the flat bound is REL_TOL_F64 where 8 times float64's flat error meets it."""
    cls, err, flat = TABLE[kind, pas]
    _, err0, _ = TABLE["ordinary", pas]
    assert cls in ("bound", "non_finite")
    return 8.0 * max(err, err0), (REL_TOL_F64 if np.isfinite(flat) and 8.0 * flat <= REL_TOL_F64 else None)


def table_kinds():
    return ("ordinary",) + me.KINDS


if __name__ == "__main__":
    print("TABLE = {")
    for kind in table_kinds():
        for pas in (sys.argv[1:] or PASSES):
            cls, err, flat = measure(kind, pas)
            flat = "NAN" if np.isnan(flat) else repr(_ceil2(flat))
            print(f'    ("{kind}", "{pas}"): ("{cls}", {_ceil2(err)!r}, {flat}),')
            sys.stdout.flush()
    print("}")
