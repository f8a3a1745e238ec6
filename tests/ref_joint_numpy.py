"""Independent dense restatement of the joint problem (tests/ only): depths, rotation and translation free together.

Per match  e_i = d2_i x2_i - d1_i R(w) x1_i + t,  block-wise Huber(delta).  Everything is built from the residual
definition: the full 3n x (2n + 6) Jacobian, with the rotation columns from the explicit derivative of the exponential map

    dR/dw_j = (w_j [w]x + [w x ((I - R) e_j)]x) R / |w|^2          (|w|^2 <= eps: R = I + [w]x, dR/dw_j = [e_j]x)

-- not from the left Jacobian J_l the product uses --, sqrt(rho') applied to rows, Jacobi scaling of the columns, the LM
damping, the sphere's tangent projection of the translation columns, and the DENSE damped normal equations solved with
numpy.linalg.solve (float64: LAPACK has no long double; the element-wise Schur reference `schur_longdouble` below is
long double where the platform has one).  `dense_solve` runs the same accept / reject schedule as the product.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
CANCELLATION_BAND = 1e-4        # |w|^2 below which rotation_derivatives evaluates its closed formula at 50 digits
TERM = {1: "function", 2: "gradient", 3: "parameter", 4: "no_convergence", 5: "min_radius", 6: "failure"}

DEFAULTS = dict(max_num_iterations=50, initial_trust_region_radius=1e4, max_trust_region_radius=1e16, min_trust_region_radius=1e-32,
                min_relative_decrease=1e-3, min_lm_diagonal=1e-6, max_lm_diagonal=1e32, function_tolerance=1e-6,
                gradient_tolerance=1e-10, parameter_tolerance=1e-8, jacobi_scaling=1, huber_delta=1.0, tran_param=1)


def skew(p, dt=np.float64):
    return np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]], dtype=dt)


def rotation(w, dt=np.float64):
    w = np.asarray(w, dtype=dt)
    th2 = w @ w
    K = skew(w, dt)
    if th2 > EPS:
        th = np.sqrt(th2)
        return np.eye(3, dtype=dt) + np.sin(th) / th * K + (1 - np.cos(th)) / th2 * (K @ K)
    return np.eye(3, dtype=dt) + K


def rotation_derivatives(w, dt=np.float64):
    """[dR/dw_0, dR/dw_1, dR/dw_2]"""
    w = np.asarray(w, dtype=dt)
    th2 = w @ w
    I = np.eye(3, dtype=dt)
    if th2 <= EPS:
        return [skew(I[j], dt) for j in range(3)]
    if th2 < CANCELLATION_BAND:
        return _rotation_derivatives_mp(w, dt)
    R = rotation(w, dt)
    return [(w[j] * skew(w, dt) + skew(np.cross(w, (I - R) @ I[j]), dt)) @ R / th2 for j in range(3)]


def _rotation_derivatives_mp(w, dt, digits=50):
    """The closed formula of rotation_derivatives evaluated at `digits` digits and rounded once to `dt`.  Just above the
    small-angle threshold I - R is of size |w| and loses its leading digits in `dt`: the quotient by |w|^2 then carries eps / |w|
    of noise (1e-9 relative at |w| = 3e-8 in float64), far above what the product's series is held to.  Same formula, no
    series, no left Jacobian -- only the working precision differs."""
    import mpmath as mp
    with mp.workdps(digits):
        def mpf(x):             # exact: a long double is the sum of its float64 head and tail
            hi = float(x)
            return mp.mpf(hi) + mp.mpf(float(x - dt(hi)))

        def to_dt(x):
            return dt(float(x)) if dt == np.float64 else dt(mp.nstr(x, 40))

        def mskew(p):
            return mp.matrix([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
        v = [mpf(x) for x in w]
        th2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
        th = mp.sqrt(th2)
        K = mskew(v)
        Id = mp.eye(3)
        R = Id + (mp.sin(th) / th) * K + ((1 - mp.cos(th)) / th2) * (K * K)
        out = []
        for j in range(3):
            c = (Id - R)[:, j]
            cr = [v[1] * c[2] - v[2] * c[1], v[2] * c[0] - v[0] * c[2], v[0] * c[1] - v[1] * c[0]]
            G = (v[j] * K + mskew(cr)) * R / th2
            out.append(np.array([[to_dt(G[a, b]) for b in range(3)] for a in range(3)], dtype=dt))
        return out


def huber(delta, s):
    """rho, rho' (arrays)"""
    s = np.asarray(s)
    if not delta > 0:
        return s.copy(), np.ones_like(s)
    out = s > delta * delta
    r = np.sqrt(np.where(out, s, 1.0))
    return np.where(out, 2 * delta * r - delta * delta, s), np.where(out, delta / r, 1.0)


def tangent_basis(t):
    """The 3 x 2 basis of the plane perpendicular to t that the product's sphere parameterisation uses (the Jacobi scaling
    of the two tangent columns depends on the basis, so the restatement must pick the same one): the coordinate axis least
    aligned with u = t / |t|, b0 = u x axis normalised, b1 = u x b0."""
    t = np.asarray(t, dtype=np.float64)
    n = np.linalg.norm(t)
    u = t / n if n > 0 else np.array([1.0, 0, 0])
    k = 0
    if abs(u[1]) < abs(u[k]):
        k = 1
    if abs(u[2]) < abs(u[k]):
        k = 2
    a = np.zeros(3)
    a[k] = 1.0
    b0 = np.cross(u, a)
    b0 /= np.linalg.norm(b0)
    return np.stack([b0, np.cross(u, b0)], axis=1)


def projection(tran_param, tran):
    """6 x m: local camera step -> ambient [rot | tran] step."""
    if tran_param == 1:
        P = np.zeros((6, 5))
        P[:3, :3] = np.eye(3)
        P[3:, 3:] = tangent_basis(tran)
        return P
    return np.eye(6)


def plus(tran_param, rot, tran, P, y):
    d6 = P @ y
    r, t = rot + d6[:3], tran + d6[3:]
    if tran_param == 1:
        nn = np.linalg.norm(t)
        if nn > 0:
            t = t * (np.linalg.norm(tran) / nn)
    return r, t


class JointProblem:
    def __init__(self, x1, x2, delta=1.0):
        self.x1 = np.asarray(x1, dtype=np.float64).reshape(-1, 3)
        self.x2 = np.asarray(x2, dtype=np.float64).reshape(-1, 3)
        self.n = len(self.x1)
        self.delta = delta

    def residuals(self, rot, tran, d, dt=np.float64):
        d = np.asarray(d, dtype=dt).reshape(-1, 2)
        R = rotation(rot, dt)
        return d[:, 1:2] * self.x2.astype(dt) - d[:, 0:1] * (self.x1.astype(dt) @ R.T) + np.asarray(tran, dtype=dt)

    def cost(self, rot, tran, d):
        e = self.residuals(rot, tran, d)
        rho, _ = huber(self.delta, np.sum(e * e, axis=1))
        return 0.5 * float(np.sum(rho))

    def blocks(self, rot, tran, d, dt=np.float64):
        """e (n,3), w (n,), E (n,3,2), F (n,3,6) at the point."""
        d = np.asarray(d, dtype=dt).reshape(-1, 2)
        x1, x2 = self.x1.astype(dt), self.x2.astype(dt)
        R = rotation(rot, dt)
        u = x1 @ R.T
        e = d[:, 1:2] * x2 - d[:, 0:1] * u + np.asarray(tran, dtype=dt)
        _, w = huber(self.delta, np.sum(e * e, axis=1))
        E = np.stack([-u, x2], axis=2)
        F = np.zeros((self.n, 3, 6), dtype=dt)
        for j, G in enumerate(rotation_derivatives(rot, dt)):
            F[:, :, j] = -d[:, 0:1] * (x1 @ G.T)
        F[:, :, 3:] = np.eye(3, dtype=dt)
        return e, w, E, F

    def jacobian(self, rot, tran, d):
        """Robustified dense system: sqrt(w) J (3n x (2n + 6)) and sqrt(w) e (3n,)."""
        e, w, E, F = self.blocks(rot, tran, d)
        n = self.n
        J = np.zeros((3 * n, 2 * n + 6))
        sw = np.sqrt(w)
        for i in range(n):
            J[3 * i:3 * i + 3, 2 * i:2 * i + 2] = sw[i] * E[i]
            J[3 * i:3 * i + 3, 2 * n:] = sw[i] * F[i]
        return J, (sw[:, None] * e).reshape(-1)


def schur_longdouble(x1, x2, rot, tran, d, radius, delta=1.0, jacobi_scaling=True, min_diag=1e-6, max_diag=1e32, dt=np.longdouble):
    """The reduced camera system of the product's reduce pass, element-wise in `dt`: V, gc (unreduced), S, gs (reduced, depth
    columns Jacobi-scaled at this point and damped by clamp(diag) / radius), cost, sum_w."""
    P = JointProblem(x1, x2, delta)
    e, w, E, F = P.blocks(rot, tran, d, dt)
    return schur_of_blocks(e, w, E, F, radius, delta, jacobi_scaling, min_diag, max_diag, dt)


def schur_of_blocks(e, w, E, F, radius, delta=1.0, jacobi_scaling=True, min_diag=1e-6, max_diag=1e32, dt=np.longdouble):
    """schur_longdouble from given per-match blocks: residuals e (n, 3), weights w (n,), depth columns E (n, 3, 2) and camera
    columns F (n, 3, 6)."""
    e, E, F = e.astype(dt), E.astype(dt), F.astype(dt)
    w = w.astype(dt)
    EtE = np.einsum("nri,nrj->nij", E, E) * w[:, None, None]
    EtF = np.einsum("nri,nrj->nij", E, F) * w[:, None, None]
    FtF = np.einsum("nri,nrj->nij", F, F) * w[:, None, None]
    gd = np.einsum("nri,nr->ni", E, e) * w[:, None]
    gc = np.einsum("nri,nr->ni", F, e) * w[:, None]
    dg = np.stack([EtE[:, 0, 0], EtE[:, 1, 1]], axis=1)
    s = 1 / (1 + np.sqrt(dg)) if jacobi_scaling else np.ones_like(dg)
    U = EtE * s[:, :, None] * s[:, None, :]
    if np.isfinite(radius):
        D = np.clip(np.stack([U[:, 0, 0], U[:, 1, 1]], axis=1), dt(min_diag), dt(max_diag)) / dt(radius)
        U[:, 0, 0] += D[:, 0]
        U[:, 1, 1] += D[:, 1]
    W = EtF * s[:, :, None]
    G = gd * s
    det = U[:, 0, 0] * U[:, 1, 1] - U[:, 0, 1] * U[:, 1, 0]
    Ui = np.empty_like(U)
    Ui[:, 0, 0], Ui[:, 1, 1], Ui[:, 0, 1], Ui[:, 1, 0] = U[:, 1, 1] / det, U[:, 0, 0] / det, -U[:, 0, 1] / det, -U[:, 1, 0] / det
    T = np.einsum("nia,nij,njb->nab", W, Ui, W)
    tg = np.einsum("nia,nij,nj->na", W, Ui, G)
    rho, _ = huber(delta, np.sum(e * e, axis=1))
    return dict(V=FtF.sum(0), gc=gc.sum(0), S=(FtF - T).sum(0), gs=(gc - tg).sum(0), cost=0.5 * rho.sum(), sum_w=w.sum(),
                gd_max=np.abs(gd).max(initial=0))


def dense_step(P, rot, tran, d, radius, scale, diag, opt):
    """One damped step from the DENSE normal equations.  scale / diag: (2n + m,) Jacobi scaling and LM diagonal, None =
    compute here (first evaluation / after an accepted step).  Returns a dict: delta_d (n,2), y (local camera step),
    delta_c (ambient), model, scale, diag, cond, gmax, cost, valid."""
    n = P.n
    J, f = P.jacobian(rot, tran, d)
    Pm = projection(opt["tran_param"], tran)
    m = Pm.shape[1]
    Jl = np.concatenate([J[:, :2 * n], J[:, 2 * n:] @ Pm], axis=1)
    g = Jl.T @ f
    if scale is None:
        scale = 1.0 / (1.0 + np.sqrt(np.sum(Jl * Jl, axis=0))) if opt["jacobi_scaling"] else np.ones(2 * n + m)
    Js = Jl * scale
    H = Js.T @ Js
    if diag is None:
        diag = np.clip(np.diag(H), opt["min_lm_diagonal"], opt["max_lm_diagonal"])
    A = H + np.diag(diag / radius)
    out = dict(scale=scale, diag=diag, gmax=float(np.abs(g).max(initial=0.0)), m=m, P=Pm)
    try:
        np.linalg.cholesky(A)
        y = np.linalg.solve(A, -(Js.T @ f))
    except np.linalg.LinAlgError:
        out.update(valid=False)
        return out
    delta = scale * y
    Jd = Jl @ delta
    out.update(valid=True, delta_d=delta[:2 * n].reshape(n, 2), y=delta[2 * n:], delta_c=Pm @ delta[2 * n:],
               model=float(-Jd @ (f + 0.5 * Jd)), cond=float(np.linalg.cond(A)))
    return out


def dense_solve(x1, x2, rot0, tran0, d0, **overrides):
    """The product's schedule over the dense system.  Returns rot, tran, d, summary dict (termination, num_iterations,
    num_successful_steps, num_evaluations, initial_cost, final_cost, margin).  margin: the smallest relative distance of any
    evaluated termination / acceptance test from its threshold -- a run is only a fair yardstick for counts when no test sat
    on its threshold."""
    o = dict(DEFAULTS)
    o.update(overrides)
    P = JointProblem(x1, x2, o["huber_delta"])
    rot, tran = np.array(rot0, dtype=np.float64), np.array(tran0, dtype=np.float64)
    d = np.array(d0, dtype=np.float64).reshape(-1, 2).copy()
    radius, nu, reuse, invalid, it, evals, succ = o["initial_trust_region_radius"], 2.0, False, 0, 0, 0, 0
    scale = diag = None
    margin = np.inf
    cost = P.cost(rot, tran, d)
    s = dict(initial_cost=cost)

    def rel(v, thr):
        nonlocal margin
        if thr != 0 and np.isfinite(v):
            margin = min(margin, abs(v - thr) / abs(thr))

    def done(term):
        s.update(termination=term, num_iterations=it, num_successful_steps=succ, num_evaluations=evals, final_cost=cost, margin=margin,
                 final_radius=radius)
        return rot, tran, d, s
    if not np.isfinite(cost):
        evals += 1
        return done("failure")
    while True:
        evals += 1                                       # the Jacobian evaluation at the current point
        st = dense_step(P, rot, tran, d, radius, scale, diag if reuse else None, o)
        scale, diag = st["scale"], st["diag"]
        if it >= o["max_num_iterations"]:
            return done("no_convergence")
        rel(st["gmax"], o["gradient_tolerance"])
        if st["gmax"] <= o["gradient_tolerance"]:
            return done("gradient")
        if radius < o["min_trust_region_radius"]:
            return done("min_radius")
        it += 1
        if st["valid"]:
            evals += 1                                   # the evaluation at the candidate
        if not st["valid"] or not st["model"] > 0:
            invalid += 1
            if invalid >= 5:
                return done("failure")
            radius /= nu; nu *= 2; reuse = True
            continue
        invalid = 0
        rc, tc = plus(o["tran_param"], rot, tran, st["P"], st["y"])
        dc = d + st["delta_d"]
        step = np.sqrt(np.sum(st["delta_d"] ** 2) + np.sum((rc - rot) ** 2) + np.sum((tc - tran) ** 2))
        xn = np.sqrt(np.sum(d * d) + rot @ rot + tran @ tran)
        thr = o["parameter_tolerance"] * (xn + o["parameter_tolerance"])
        rel(step, thr)
        if step <= thr:
            return done("parameter")
        cc = P.cost(rc, tc, dc)
        change = cost - cc
        rel(abs(change), o["function_tolerance"] * cost)
        if np.isfinite(cc) and abs(change) <= o["function_tolerance"] * cost:
            return done("function")
        q = change / st["model"] if np.isfinite(cc) else -1.0
        rel(q, o["min_relative_decrease"])
        if q > o["min_relative_decrease"]:
            rot, tran, d, cost = rc, tc, dc, cc
            succ += 1
            t3 = 2 * q - 1
            radius = min(o["max_trust_region_radius"], radius / max(1.0 / 3.0, 1 - t3 ** 3))
            nu, reuse = 2.0, False
        else:
            radius /= nu; nu *= 2; reuse = True
