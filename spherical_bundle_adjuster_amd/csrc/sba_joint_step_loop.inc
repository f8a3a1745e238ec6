// The step pass's per-match loop: THE definition (no include guard: plain statements, expanded inside a function body).
// Expanded by joint_step_stream (sba_joint_core.hpp, where the batched kernels get it) and by joint_step_kernel
// (sba_joint.hip).  The includer has in scope: ST; pl, d1, d2, c1, c2, sc1, sc2, P; n, npairs; pr (this lane's first pair of
// matches), stride; acc[JOINT_STEP_COUNT], zeroed; map (logical pair-of-matches index -> index into the planes).
  JointRegs<ST> cur, nxt;
  if (pr < npairs) cur.load(pl, d1, d2, sc1, sc2, true, map(pr));
  while (pr < npairs) {
    const size_t pn = pr + stride, q = map(pr);
    if (pn < npairs) nxt.load(pl, d1, d2, sc1, sc2, true, map(pn));
    double NA[2], NB[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bool valid = 2 * pr + h < n;
      const double x = cur.X[h], y = cur.Y[h], z = cur.Z[h], u = cur.U[h], v = cur.V[h], q = cur.W[h];
      const double a = cur.A[h], bd = cur.B[h];
      JointBlock b;
      joint_block(P, x, y, z, u, v, q, a, bd, cur.S1[h], cur.S2[h], valid, b);
      // delta d = -U^-1 (g_d + W delta c), in scaled coordinates, then unscaled
      double t1 = b.G1, t2 = b.G2;
#pragma unroll
      for (int k = 0; k < 6; ++k) { t1 += b.w1[k] * P.delta_c[k]; t2 += b.w2[k] * P.delta_c[k]; }
      const double y1 = (b.U12 * t2 - b.U22 * t1) * b.inv_det, y2 = (b.U12 * t1 - b.U11 * t2) * b.inv_det;
      const double dl1 = b.s1 * y1, dl2 = b.s2 * y2;
      const double na = a + dl1, nb = bd + dl2;
      NA[h] = valid ? na : 0.0; NB[h] = valid ? nb : 0.0;     // the padding stays zero
      // J delta = E delta d + A delta w + delta t
      double jd[3];
#pragma unroll
      for (int r = 0; r < 3; ++r)
        jd[r] = b.nu[r] * dl1 + (r == 0 ? u : (r == 1 ? v : q)) * dl2 + b.A[r][0] * P.delta_c[0] + b.A[r][1] * P.delta_c[1] +
                b.A[r][2] * P.delta_c[2] + P.delta_c[3 + r];
      // the residual at the candidate (w', t', d'), formed as every residual of the library
      double X = x, Y = y, Z = z, Uc = u, Vc = v, Qc = q, r0, r1, r2, f0, f1, f2;
      residual<DEPTH_PER_MATCH>(&P.cand, X, Y, Z, Uc, Vc, Qc, na, nb, r0, r1, r2, f0, f1, f2);
      const double sc = sq_norm(f0, f1, f2);
      double wc = 1.0, rhoc = sc, outc = 0.0;
      if (P.cur.delta > 0.0) huber(sc, P.cur.delta, P.cur.delta2, wc, rhoc, outc);
      if (valid) {
        acc[JOINT_STEP_CAND_COST] = __builtin_fma(0.5, rhoc, acc[JOINT_STEP_CAND_COST]);
        acc[JOINT_STEP_MODEL] -= b.w * (jd[0] * (b.e[0] + 0.5 * jd[0]) + jd[1] * (b.e[1] + 0.5 * jd[1]) + jd[2] * (b.e[2] + 0.5 * jd[2]));
        acc[JOINT_STEP_DSTEP2] += dl1 * dl1 + dl2 * dl2;
        acc[JOINT_STEP_D2] += a * a + bd * bd;
      }
    }
    joint_store_pair(c1, q, NA[0], NA[1]);
    joint_store_pair(c2, q, NB[0], NB[1]);
    cur = nxt;
    pr = pn;
  }
