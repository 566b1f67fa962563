// Fragment of the matrix-core attention bodies, included in place inside the wave-step loop, between
// the QK MFMAs and the PV MFMAs: the online softmax of one 32-token step.
// Reads: S[2] (the step's scores, still scaled by 2^-24 and offset), rv[8], ks[8], vs[8], i0, g,
// qoff, qscale, MT, kWave; in the chunk forms col_lim.
// Updates: m, l, psum, pvc, acc[MT] (rescaled to the new pvc).
// Defines: pb_hi, pb_lo, the PV B operand p * v_scale / pvc as an f16 hi + lo pair (and s, mx, mn, mu,
// alpha, pw, wmax, ca, cinv, beta, phi, plo on the way).
// Islands: [score mask] (ATTN_BODY_CHUNK; ATTN_BODY_WINDOW: also col_lo and col_sink), [window] the
// masked rows' V scales.  A text fragment and not a function: as
// pv_softmax_step<MT> it moved the registers of 15 decode kernels (DESIGN.md).
    float s[8];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#ifdef ATTN_BODY_WINDOW  // [score mask] the windowed kernels: col_lo and col_sink from [window]
      const int ti = i0 + 16 * (j >> 2) + 4 * g + (j & 3);
      const bool seen = ti < col_lim && (ti >= col_lo || ti < col_sink);
      s[j] = rv[j] >= 0 && seen ? (S[j >> 2][j & 3] * kMfmaValScale - qoff) * (qscale * ks[j]) : -INFINITY;
#elif ATTN_BODY_CHUNK  // [score mask] col_lim from [key limit]
      const bool seen = i0 + 16 * (j >> 2) + 4 * g + (j & 3) < col_lim;
      s[j] = rv[j] >= 0 && seen ? (S[j >> 2][j & 3] * kMfmaValScale - qoff) * (qscale * ks[j]) : -INFINITY;
#else
      s[j] = rv[j] >= 0 ? (S[j >> 2][j & 3] * kMfmaValScale - qoff) * (qscale * ks[j]) : -INFINITY;
#endif
      mx = fmaxf(mx, s[j]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, kWave));
    mx = fmaxf(mx, __shfl_xor(mx, 32, kWave));
    const float mn = fmaxf(m, mx);
    const float mu = mn == -INFINITY ? 0.0f : mn;  // no valid token yet: nothing to scale
    const float alpha = attn_exp(m - mu);
    m = mn;
    l *= alpha;
    psum *= alpha;
    float pw[8], wmax = 0.0f;  // p * v_scale
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const float p0 = attn_exp(s[2 * h] - mu), p1 = attn_exp(s[2 * h + 1] - mu);
      l += p0 + p1;
#ifdef ATTN_BODY_WINDOW  // [window] a masked row stands in row 0 of the cache, which may be a released block's: its
      // weight 0 must not meet a V scale that is no number (0 * NaN)
      pw[2 * h] = s[2 * h] == -INFINITY ? 0.0f : p0 * vs[2 * h];
      pw[2 * h + 1] = s[2 * h + 1] == -INFINITY ? 0.0f : p1 * vs[2 * h + 1];
#else
      pw[2 * h] = p0 * vs[2 * h];
      pw[2 * h + 1] = p1 * vs[2 * h + 1];
#endif
      psum += pw[2 * h] + pw[2 * h + 1];
      wmax = fmaxf(wmax, fmaxf(pw[2 * h], pw[2 * h + 1]));
    }
    // [normaliser] pv_norm_pow2 (attention.hip): one power of two per column, uniform over its
    // four lanes as m is; acc holds O / pvc, the operand is pw / pvc < 2 whatever v_scale is
    wmax = fmaxf(wmax, __shfl_xor(wmax, 16, kWave));
    wmax = fmaxf(wmax, __shfl_xor(wmax, 32, kWave));
    const float ca = pvc * alpha;
    pvc = pv_norm_pow2(fmaxf(ca, wmax));
    const float cinv = pv_norm_recip(pvc), beta = ca * cinv;  // alpha, and the old O / pvc in the new pvc (<= 2)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] *= beta;
    uint32_t phi[4], plo[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const float w0 = pw[2 * h] * cinv, w1 = pw[2 * h + 1] * cinv;
      const auto hi = __builtin_amdgcn_cvt_pkrtz(w0, w1);
      const auto lo = __builtin_amdgcn_cvt_pkrtz(w0 - (float)hi[0], w1 - (float)hi[1]);
      phi[h] = __builtin_bit_cast(uint32_t, hi);
      plo[h] = __builtin_bit_cast(uint32_t, lo);
    }
    const f16x8 pb_hi = __builtin_bit_cast(f16x8, u32x4{phi[0], phi[1], phi[2], phi[3]});
    const f16x8 pb_lo = __builtin_bit_cast(f16x8, u32x4{plo[0], plo[1], plo[2], plo[3]});
