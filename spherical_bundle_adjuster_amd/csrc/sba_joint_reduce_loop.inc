// The reduce pass's per-match loop: THE definition (no include guard: plain statements, expanded inside a function body).
// Expanded by joint_reduce_stream (sba_joint_core.hpp, where the batched kernels get it) and by joint_reduce_kernel
// (sba_joint.hip).  The includer has in scope: ST; pl, d1, d2, sc1, sc2, P; n, npairs, load_scale; pr (this lane's first pair of
// matches), stride; acc[JOINT_OUT_COUNT], zeroed; map (logical pair-of-matches index -> index into the planes).
  JointRegs<ST> cur, nxt;
  if (pr < npairs) cur.load(pl, d1, d2, sc1, sc2, load_scale, map(pr));
  while (pr < npairs) {
    const size_t pn = pr + stride, q = map(pr);
    if (pn < npairs) nxt.load(pl, d1, d2, sc1, sc2, load_scale, map(pn));
    double NS1[2], NS2[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bool valid = 2 * pr + h < n;
      JointBlock b;
      joint_block(P, cur.X[h], cur.Y[h], cur.Z[h], cur.U[h], cur.V[h], cur.W[h], cur.A[h], cur.B[h], cur.S1[h], cur.S2[h], valid, b);
      NS1[h] = b.s1; NS2[h] = b.s2;
      const double w = b.w;
      // unreduced camera block, SBA_PACK_* layout (as the explicit sweep kernel accumulates it)
      double wA[3][3];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int j = 0; j < 3; ++j) wA[r][j] = w * b.A[r][j];
      double ff[21], fe[6];      // w F^T F (upper, row by row) and w F^T e of this match
      int k = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = a; c < 3; ++c) ff[k++] = wA[0][a] * b.A[0][c] + wA[1][a] * b.A[1][c] + wA[2][a] * b.A[2][c];
#pragma unroll
        for (int c = 0; c < 3; ++c) ff[k++] = wA[c][a];
        fe[a] = wA[0][a] * b.e[0] + wA[1][a] * b.e[1] + wA[2][a] * b.e[2];
      }
      ff[15] = w; ff[16] = 0.0; ff[17] = 0.0; ff[18] = w; ff[19] = 0.0; ff[20] = w;
      fe[3] = w * b.e[0]; fe[4] = w * b.e[1]; fe[5] = w * b.e[2];
      // pack slots: HAA = ff[0..2], ff[6..7], ff[11]; HAT[3 a + c] = ff rows a, columns 3..5
      acc[0] += ff[0]; acc[1] += ff[1]; acc[2] += ff[2]; acc[3] += ff[6]; acc[4] += ff[7]; acc[5] += ff[11];
      acc[6] += ff[3]; acc[7] += ff[4]; acc[8] += ff[5]; acc[9] += ff[8]; acc[10] += ff[9]; acc[11] += ff[10];
      acc[12] += ff[12]; acc[13] += ff[13]; acc[14] += ff[14];
      acc[SBA_PACK_SW] += w;
#pragma unroll
      for (int a = 0; a < 6; ++a) acc[SBA_PACK_GA + a] += fe[a];          // GA[3], GT[3] are consecutive slots
      acc[SBA_PACK_COST] = __builtin_fma(0.5, b.rho, acc[SBA_PACK_COST]);
      acc[SBA_PACK_NOUT] += b.is_out;
      // Schur complement of the depth block: z = U^-1 W (two rows), T = W^T z
      double z1[6], z2[6];
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        z1[a] = (b.U22 * b.w1[a] - b.U12 * b.w2[a]) * b.inv_det;
        z2[a] = (b.U11 * b.w2[a] - b.U12 * b.w1[a]) * b.inv_det;
      }
      k = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int c = a; c < 6; ++c) {
          acc[JOINT_OUT_S + k] += ff[k] - (b.w1[a] * z1[c] + b.w2[a] * z2[c]);
          ++k;
        }
        acc[JOINT_OUT_GS + a] += fe[a] - (z1[a] * b.G1 + z2[a] * b.G2);
      }
      if (valid) acc[JOINT_OUT_GDMAX] = fmax(acc[JOINT_OUT_GDMAX], fmax(fabs(b.gd1), fabs(b.gd2)));
    }
    if (P.first) { joint_store_pair(sc1, q, NS1[0], NS1[1]); joint_store_pair(sc2, q, NS2[0], NS2[1]); }
    cur = nxt;
    pr = pn;
  }
