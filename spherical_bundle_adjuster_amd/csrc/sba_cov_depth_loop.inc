// The covariance's depth loop over a lane's pairs of matches: THE definition (no include guard: plain statements, expanded
// inside a function body).  Expanded by cov_depth_kernel (sba_covariance.hip, IdentityMap) and by batch_cov_kernel
// (sba_batch_covariance.hip, BatchPairMap<ST>) -- in their own bodies, not through a call (DESIGN.md section 3.11).  The includer
// has in scope: ST; pl, d1, d2, P, min_sin2 as for the reduce loop; sigma_c (Sigma_c, row-major 6 x 6); n, npairs; pr, stride;
// map; store(pr, o): where the lane's two rows o[h] = (var d1, var d2, cov) go (o[1] is zeros for the padding match).
  CovRegs<ST> cur, nxt;
  if (pr < npairs) cur.load(pl, d1, d2, map(pr));
  while (pr < npairs) {
    const size_t pn = pr + stride;
    if (pn < npairs) nxt.load(pl, d1, d2, map(pn));
    double o[2][3];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bool valid = 2 * pr + h < n;
      JointBlock b;
      joint_block(P, cur.X[h], cur.Y[h], cur.Z[h], cur.U[h], cur.V[h], cur.W[h], cur.A[h], cur.B[h], 1.0, 1.0, valid, b);
      double z1[6], z2[6], Ui[3];
      const bool ok = cov_block(b.U11, b.U12, b.U22, b.inv_det, b.w1, b.w2, min_sin2, z1, z2, Ui);
      o[h][0] = __builtin_huge_val(); o[h][1] = __builtin_huge_val(); o[h][2] = 0.0;
      if (ok) cov_depth_block(b.s1, b.s2, Ui, z1, z2, sigma_c, o[h]);
      if (!valid) { o[h][0] = 0.0; o[h][1] = 0.0; o[h][2] = 0.0; }
    }
    store(pr, o);
    cur = nxt;
    pr = pn;
  }
