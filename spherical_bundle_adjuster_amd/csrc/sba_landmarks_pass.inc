// One pass over a frame's observations that updates each observed landmark on its own: THE definition (no include guard: plain
// statements, expanded inside a kernel's body, in the manner of sba_joint_step_loop.inc).  Expanded by landmarks_fuse_kernel
// (sba_landmarks.hip: NOISE = false, landmark_fuse_one) and by landmarks_register_apply_kernel (sba_landmarks_register.hip:
// NOISE = true, landmark_register_one).  The includer has in scope: INDEXED, APPLY, NOISE (compile-time); P (the pass's
// by-value state: P.n landmarks, P.m observations), base, elems, idx, bearings, noise (read when NOISE), chi2 (may be null),
// counters; and the macro SBA_LANDMARK_PASS_ONE(X, Sg, y, noise, Xo, So, &chi2) -> the observation's class, which names the
// per-observation function itself (its noise argument is not evaluated where the function takes none): called through a
// functor the write-back's kernels compiled to another order of operands.
//   dense:   lane p owns landmarks 2 p and 2 p + 1: nine 16-byte plane loads, three 16-byte loads of its 48 bytes of bearing rows
//            (and one of the noise), nine 16-byte stores when one of its two landmarks was fused, one 16-byte store of chi2
//   indexed: lane j owns observation j and gathers landmark idx[j] (sorted: neighbouring lanes, neighbouring lines)
//   APPLY = false: chi2 and counts only.
// Expanded, not called: a function that holds this loop is optimised on its own before it is inlined, with P behind a pointer,
// and the kernels then compile to other register counts and another instruction order (DESIGN 3.23).
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  lm::ClassCounts<LANDMARK_CLASSES> cc;
  cc.init();
  if (INDEXED) {
    const size_t m = P.m;
    for (size_t j = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < m; j += stride) {
      const size_t i = static_cast<size_t>(idx[j]);        // < n: validated on the host
      double X[3], Sg[6], y[3], Xo[3], So[6], s;
      lm::gather(base, elems, i, bearings, j, X, Sg, y);
      const int cls = SBA_LANDMARK_PASS_ONE(X, Sg, y, noise[j], Xo, So, &s);
      cc.add(true, cls);
      if (chi2) chi2[j] = s;
      if (APPLY && cls == LANDMARK_FUSED) {
        lm::scatter(base, elems, i, Xo, So);
        lm::counts(base, elems)[i] += 1u;
      }
    }
  } else {
    const size_t n = P.n, nvec = (n + 1) / 2;
    for (size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < nvec; p += stride) {
      lm::PairRegs<NOISE> cur;
      cur.load(base, elems, bearings, noise, p);
      double s[2];
      bool fused[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const bool valid = 2 * p + h < n;
        double X[3], Sg[6], y[3], Xo[3], So[6];
        cur.get(h, X, Sg, y);
        const int cls = SBA_LANDMARK_PASS_ONE(X, Sg, y, cur.noise(h), Xo, So, &s[h]);
        cc.add(valid, cls);
        fused[h] = valid && cls == LANDMARK_FUSED;
        if (APPLY && fused[h]) cur.set(h, Xo, So);
        __builtin_amdgcn_sched_barrier(0);     // one landmark at a time: the second one's temporaries reuse the first one's registers
      }
      if (chi2) reinterpret_cast<double2*>(chi2)[p] = make_double2(s[0], s[1]);
      if (APPLY && (fused[0] || fused[1])) {
        cur.store(base, elems, p);
        uint2* cp = reinterpret_cast<uint2*>(lm::counts(base, elems)) + p;
        uint2 c = *cp;
        c.x += fused[0] ? 1u : 0u;
        c.y += fused[1] ? 1u : 0u;
        *cp = c;
      }
    }
  }
  cc.flush(counters);
