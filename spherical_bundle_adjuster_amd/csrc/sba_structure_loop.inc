// The structure pass's loop over a lane's pairs of matches: THE definition (no include guard: plain statements, expanded
// inside a function body, as the covariance's two loops are -- DESIGN.md section 3.11).  Expanded by structure_kernel
// (sba_structure.hip, IdentityMap).  The includer has in scope: ST; WANT_XYZ, WANT_COV, WANT_SCORE (compile-time); pl, d1, d2;
// P (a first pass's JointParams, inv_radius = 0), min_sin2, sigma_c (Sigma_c, row-major 6 x 6); n, npairs; pr, stride; map;
// store(pr, both, X, cv, q): where the lane's rows go -- X[h], cv[h], q[h] of match 2 pr + h; both = false: match 2 pr + 1 is the
// padding of an odd-sized problem and must not be stored.
  CovRegs<ST> cur, nxt;
  if (pr < npairs) cur.load(pl, d1, d2, map(pr));
  while (pr < npairs) {
    const size_t pn = pr + stride;
    if (pn < npairs) nxt.load(pl, d1, d2, map(pn));
    double X[2][3], cv[2][6], q[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bool valid = 2 * pr + h < n;
      JointBlock b;
      joint_block(P, cur.X[h], cur.Y[h], cur.Z[h], cur.U[h], cur.V[h], cur.W[h], cur.A[h], cur.B[h], 1.0, 1.0, valid, b);
      double z1[6], z2[6], Ui[3];
      const bool ok = (WANT_COV || WANT_SCORE) && cov_block(b.U11, b.U12, b.U22, b.inv_det, b.w1, b.w2, min_sin2, z1, z2, Ui);
      structure_block(ok, WANT_COV || WANT_SCORE, b.nu, b.A, b.s1, b.s2, z1, z2, Ui, sigma_c, cur.U[h], cur.V[h], cur.W[h],
                      cur.A[h], cur.B[h], P.cur.t, X[h], cv[h], &q[h]);
    }
    store(pr, 2 * pr + 1 < n, X, cv, q);
    cur = nxt;
    pr = pn;
  }
