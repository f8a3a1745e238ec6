"""Shared by the joint tests (tests/ only): the harness around the product's joint step logic (csrc/sba_joint_solver.hpp,
built with g++ from tests/harness/joint_harness.cpp) and numpy-EMULATED device passes to drive it with.

The emulation (`EmulatedJoint`) does what joint_reduce_kernel / joint_step_kernel do per match -- eliminate the damped,
Jacobi-scaled 2x2 depth block, accumulate the reduced camera system, back-substitute the depth step, evaluate the
candidate.  It takes the per-match blocks (e, w, E, F) from ref_joint_numpy.JointProblem.blocks, the same function the
dense restatement builds its Jacobian from: a comparison of the two is the Schur route against the dense solve on SHARED
blocks, not two derivations of the Jacobian.  The kernels' own Jacobian (J_l form) is checked against the explicit dR/dw on
the GPU, through schur_longdouble and the oracle (tests/test_gpu_joint.py)."""
import ctypes as C
import subprocess

import numpy as np

import ref_joint_numpy as rj
from helpers import ROOT
from spherical_bundle_adjuster_amd import _cabi as cabi

_h = None


def harness():
    global _h
    if _h is None:
        so = ROOT / "tests" / "harness" / "libjoint_harness.so"
        src = ROOT / "tests" / "harness" / "joint_harness.cpp"
        hdrs = [ROOT / "spherical_bundle_adjuster_amd" / "csrc" / f for f in ("sba_joint_solver.hpp", "sba_lm.hpp")]
        if not so.exists() or so.stat().st_mtime < max(f.stat().st_mtime for f in [src] + hdrs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)], check=True)
        _h = C.CDLL(str(so))
        _h.joint_harness_create.restype = C.c_void_p
    return _h


def layout():
    out = (C.c_int * 5)()
    harness().joint_harness_row_layout(out)
    return dict(S=out[0], GS=out[1], GDMAX=out[2], COUNT=out[3], ROW=out[4])


class EmulatedJoint:
    """What the device holds: current depths, candidate depths, depth Jacobi scaling."""

    def __init__(self, x1, x2, d0, delta=1.0, min_diag=1e-6, max_diag=1e32, jacobi=True):
        self.P = rj.JointProblem(x1, x2, delta)
        self.d = np.array(d0, dtype=np.float64).reshape(-1, 2).copy()
        self.cand = self.d.copy()
        self.scale = None
        self.min_diag, self.max_diag, self.jacobi = min_diag, max_diag, jacobi
        self.last_delta_d = None

    def _block(self, rot, tran, radius, first):
        e, w, E, F = self.P.blocks(rot, tran, self.d)
        EtE = np.einsum("nri,nrj->nij", E, E) * w[:, None, None]
        if first:
            dg = np.stack([EtE[:, 0, 0], EtE[:, 1, 1]], axis=1)
            self.scale = 1 / (1 + np.sqrt(dg)) if self.jacobi else np.ones_like(dg)
        s = self.scale
        U = EtE * s[:, :, None] * s[:, None, :]
        D = np.clip(np.stack([U[:, 0, 0], U[:, 1, 1]], axis=1), self.min_diag, self.max_diag) / radius
        U[:, 0, 0] += D[:, 0]
        U[:, 1, 1] += D[:, 1]
        Ui = np.linalg.inv(U) if len(U) else U
        W = np.einsum("nri,nrj->nij", E, F) * w[:, None, None] * s[:, :, None]
        gd = np.einsum("nri,nr->ni", E, e) * w[:, None]
        return e, w, E, F, s, Ui, W, gd

    def reduce(self, rot, tran, radius, first):
        L = layout()
        e, w, E, F, s, Ui, W, gd = self._block(rot, tran, radius, first)
        FtF = np.einsum("nri,nrj->nij", F, F) * w[:, None, None]
        gc = np.einsum("nri,nr->ni", F, e) * w[:, None]
        V, g = FtF.sum(0), gc.sum(0)
        S = (FtF - np.einsum("nia,nij,njb->nab", W, Ui, W)).sum(0)
        gs = (gc - np.einsum("nia,nij,nj->na", W, Ui, gd * s)).sum(0)
        rho, _ = rj.huber(self.P.delta, np.sum(e * e, axis=1))
        row = np.zeros(L["ROW"])
        iu = np.triu_indices(3)
        row[0:6] = V[:3, :3][iu]
        row[6:15] = V[:3, 3:].reshape(-1)
        row[15] = w.sum()
        row[16:22] = g
        row[22] = 0.5 * rho.sum()
        row[23] = float(np.sum(np.sum(e * e, axis=1) > self.P.delta ** 2)) if self.P.delta > 0 else 0.0
        row[L["S"]:L["S"] + 21] = S[np.triu_indices(6)]
        row[L["GS"]:L["GS"] + 6] = gs
        row[L["GDMAX"]] = np.abs(gd).max(initial=0.0)
        return row

    def step(self, rot, tran, radius, delta_c, rot_cand, tran_cand):
        L = layout()
        e, w, E, F, s, Ui, W, gd = self._block(rot, tran, radius, False)
        y = -np.einsum("nij,nj->ni", Ui, gd * s + W @ delta_c)
        dd = s * y
        self.last_delta_d = dd
        self.cand = self.d + dd
        Jd = np.einsum("nri,ni->nr", E, dd) + F @ delta_c
        row = np.zeros(L["ROW"])
        row[0] = self.P.cost(rot_cand, tran_cand, self.cand)
        row[1] = -np.sum(w * np.sum(Jd * (e + 0.5 * Jd), axis=1))
        row[2] = np.sum(dd * dd)
        row[3] = np.sum(self.d * self.d)
        return row

    def take_candidate(self):
        self.d = self.cand.copy()


def make_options(**opt):
    o = cabi.LmOptions()
    harness().joint_harness_default_options(C.byref(o))
    for k, v in opt.items():
        setattr(o, k, v)
    return o


def drive(em, rot0, tran0, max_passes=None, on_step=None, **opt):
    """Run the product's state machine over the emulated passes.  -> rot, tran, d, summary, status, passes, cost trace"""
    h = harness()
    o = make_options(**opt)
    rot0, tran0 = np.array(rot0, dtype=np.float64), np.array(tran0, dtype=np.float64)
    s = C.c_void_p(h.joint_harness_create(rot0.ctypes.data_as(C.c_void_p), tran0.ctypes.data_as(C.c_void_p), C.byref(o)))
    rq = (C.c_double * 21)()
    passes, trace = 0, []
    while not h.joint_harness_done(s) and (max_passes is None or passes < max_passes):
        h.joint_harness_request(s, rq)
        r = np.array(rq[:])
        if int(r[0]) == 0:
            row = em.reduce(r[3:6], r[6:9], r[2], r[1] != 0.0)
            trace.append((row[22], np.linalg.norm(r[6:9])))
        else:
            row = em.step(r[3:6], r[6:9], r[2], r[9:15], r[15:18], r[18:21])
            if on_step is not None:
                on_step(r, em)
        h.joint_harness_feed(s, np.ascontiguousarray(row).ctypes.data_as(C.c_void_p))
        passes += 1
        if h.joint_harness_take_candidate(s):
            em.take_candidate()
        assert passes < 10000
    rot, tran, summ = np.zeros(3), np.zeros(3), cabi.LmSummary()
    h.joint_harness_result(s, rot.ctypes.data_as(C.c_void_p), tran.ctypes.data_as(C.c_void_p), C.byref(summ))
    status = h.joint_harness_status(s)
    h.joint_harness_destroy(s)
    return rot, tran, em.d, summ, status, passes, trace
