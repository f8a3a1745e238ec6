// The covariance's reduce loop over a lane's pairs of matches: THE definition (no include guard: plain statements, expanded
// inside a function body).  Expanded by cov_reduce_kernel (sba_covariance.hip, IdentityMap) and by batch_cov_kernel
// (sba_batch_covariance.hip, BatchPairMap<ST>) -- in their own bodies, not through a call (DESIGN.md section 3.11).  The includer
// has in scope: ST; pl, d1, d2, P (a first pass's JointParams, inv_radius = 0), min_sin2; n, npairs; pr (this lane's first pair
// of matches), stride; acc[COV_OUT_COUNT], zeroed; map (logical pair-of-matches index -> index into the planes).
  CovRegs<ST> cur, nxt;
  if (pr < npairs) cur.load(pl, d1, d2, map(pr));
  while (pr < npairs) {
    const size_t pn = pr + stride;
    if (pn < npairs) nxt.load(pl, d1, d2, map(pn));
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bool valid = 2 * pr + h < n;
      JointBlock b;
      joint_block(P, cur.X[h], cur.Y[h], cur.Z[h], cur.U[h], cur.V[h], cur.W[h], cur.A[h], cur.B[h], 1.0, 1.0, valid, b);
      double z1[6], z2[6], Ui[3];
      const bool ok = cov_block(b.U11, b.U12, b.U22, b.inv_det, b.w1, b.w2, min_sin2, z1, z2, Ui);
      if (valid && ok) {
        const double w = b.w;
        double wA[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int j = 0; j < 3; ++j) wA[r][j] = w * b.A[r][j];
        double ff[21];      // w F^T F (upper, row by row) of this match
        int k = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
          for (int c = a; c < 3; ++c) ff[k++] = wA[0][a] * b.A[0][c] + wA[1][a] * b.A[1][c] + wA[2][a] * b.A[2][c];
#pragma unroll
          for (int c = 0; c < 3; ++c) ff[k++] = wA[c][a];
        }
        ff[15] = w; ff[16] = 0.0; ff[17] = 0.0; ff[18] = w; ff[19] = 0.0; ff[20] = w;
        k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int c = a; c < 6; ++c) {
            acc[COV_OUT_S + k] += ff[k] - (b.w1[a] * z1[c] + b.w2[a] * z2[c]);
            ++k;
          }
        acc[COV_OUT_COST] = __builtin_fma(0.5, b.rho, acc[COV_OUT_COST]);
        acc[COV_OUT_SW] += w;
        acc[COV_OUT_NUSED] += 1.0;
      } else if (valid) {
        acc[COV_OUT_NDEG] += 1.0;
      }
    }
    cur = nxt;
    pr = pn;
  }
