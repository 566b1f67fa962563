// Body of paged_attn_h84_mfma_interp_kernel (`a` an InterpArgs): the ragged
// chunk form of attn_h84_mfma_body.inc -- 16 (token, head) columns per
// workgroup, the span ChunkMap, the same operand maps, softmax and merge --
// with Hamming(8,4) double errors interpolated before the words become
// operands (kvecc.h "Interpolated attention").  A sibling of that body, not an
// inclusion of it: the shipped kernels keep their text and their registers.
//
// What differs:
//   * rows[] holds the cache row of every position of the sequence in
//     [t0 - 1, t0 + npad], not of the split's visible tokens only: the one-token
//     halo on each side is bounded by the sequence's length n_b, not by the
//     tile's key limit, and a position past the limit of every column is masked
//     by [score mask] alone.  R(i) is position t0 + i (-1: no block, or outside
//     [0, n_b)).
//   * the first look: h84_double4 of every loaded dword (the syndrome / parity
//     SWAR of the scrubber's h84_dirty4 and four more operations) marks its
//     type-2 bytes.  A lane none of whose words of a K row (of four V rows) holds
//     one goes on as the chunk kernel does.
//   * the slow path, per lane and per operand: the same bytes of rows l - 1 and
//     l + 1 (clamped to [0, n_b - 1]; a -1 block reads as zero codewords) come
//     through the same buffer descriptor, every byte is decoded, doubles become
//     interp_word(q, L, R, type), and the word is re-encoded (h84_interp_fix4) --
//     so the corrected nibbles reach nib_pair_f16 through the same table as every
//     other byte.  The neighbour loads of one K row (of four V rows) are issued
//     together, one round trip; only the words that hold a double are rewritten.
// The counted kernel (paged_attn_h84_mfma_stats_interp_kernel, `a` a StatsInterpArgs) defines
// ATTN_BODY_STATS around its inclusion: the [statistics] islands, which count the words of
// load_step -- every stored byte once -- and never the neighbour words of the slow path; without
// it the preprocessed text is what it was.
// The repairing kernel (paged_attn_h84_mfma_repair_interp_kernel, `a` a RepairInterpArgs) defines
// ATTN_BODY_REPAIR as well: the [repair] islands, which store the corrected codewords of load_step's
// words back before the slow path rewrites any in registers -- a double is never stored, and the
// neighbour words the slow path loads decode to the same nibbles before and after any store.
  constexpr int KK = D / 32;  // QK MFMAs per 16-token tile
  constexpr int MT = D / 16;  // PV M-tiles; V bytes per lane per token
  constexpr int KB = D / 4;   // K bytes per lane per token
  constexpr int KW = KB / 4;  // K dwords per token
  constexpr int VW = MT >= 4 ? MT / 4 : 1;  // V dwords per token
  constexpr uint32_t kVMask = MT >= 4 ? 0xFFFFFFFFu : (1u << (8 * MT)) - 1u;  // the bytes a V load fills
  constexpr int kWaves = kBlock / kWave;
  constexpr int kHalo = 4;  // rows[kHalo + i] is R(i): keeps the 16-byte reads of load_step aligned
  __shared__ __attribute__((aligned(16))) int32_t rows[kHalo + kMaxSplit + kMfmaStep + 4];
  __shared__ int32_t blks[kMaxSplit + 3];
  __shared__ uint8_t lut[256];
  __shared__ float red[kWaves][G][D];
  __shared__ float gml[2][kWaves][G];

  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int n = lane & 15, g = lane >> 4;
  const ChunkMap cm(a, n);  // column n's (token, head); blockIdx.x = tile * nsplit + split
  if (!cm.any) {  // every token of the tile is padding: nothing staged, no table or cache read
    cm.put_empty(a);
    return;
  }
  const int64_t b = cm.b, h0 = cm.h0;
  const int64_t hk = h0 / (a.heads / a.kv_heads);
#ifdef ATTN_BODY_STATS  // [statistics] who counts: as in attn_h84_mfma_body.inc, uniform per workgroup
  const ChunkSpan csp(a, b);
  const bool counts = csp.v1(a) > csp.v0() && cm.tile == (uint32_t)(csp.v1(a) - 1) / (16u >> a.cg_log2) &&
                      h0 % (a.heads / a.kv_heads) == 0;
  // the sequence's n_b rows: the tile's largest key limit unless the span overruns q_max
  const int64_t ctx = counts ? min<int64_t>(a.ctx_lens[b], a.ctx_cap) : cm.ctx;
  uint32_t n_single = 0, n_double = 0;
#ifdef ATTN_BODY_REPAIR  // [repair] bytes rewritten: the statistics buffer's word 2
  uint32_t n_rewritten = 0;
#endif
#else
  const int64_t ctx = cm.ctx;  // the largest key limit of the tile's columns
#endif
  const int64_t t0 = (int64_t)cm.split_idx * a.split;
  const int64_t t1 = min<int64_t>(t0 + a.split, ctx);
  const int ntok = t1 > t0 ? (int)(t1 - t0) : 0;
  const int col_lim = cm.col_limit(t0);  // this column's keys: the split's tokens below it
  // the sequence's length: what neighbours clamp to (shim_read's ctx for this sequence alone)
  const int64_t nb = max<int64_t>(min<int64_t>(a.ctx_lens[b], a.ctx_cap), 0);
  f16x8 qop[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (cm.col_ok) v = *reinterpret_cast<const u32x4 *>(cm.q_row(a) + KB * g + 8 * kk);
    qop[kk] = __builtin_bit_cast(f16x8, v);
  }
  const int npad = (ntok + kMfmaStep - 1) / kMfmaStep * kMfmaStep;
  {  // block-table slice of positions [t0 - 1, t0 + npad] -> cache rows
    const uint32_t bs = (uint32_t)a.bs;
    const int64_t p0 = max<int64_t>(t0 - 1, 0);
    const int64_t p1 = min<int64_t>(t0 + npad, a.max_blocks * a.bs - 1);  // inclusive
    const uint32_t lb0 = (uint32_t)p0 / bs;
    const int nlb = ntok > 0 && p1 >= p0 ? (int)((uint32_t)p1 / bs - lb0 + 1) : 0;
    const int32_t *tab = a.table + b * a.max_blocks + lb0;
    for (int j = threadIdx.x; j < nlb; j += kBlock) blks[j] = tab[j];
    __syncthreads();
    const int32_t head_row0 = (int32_t)((a.layer * a.kv_heads + hk) * a.bs);
    const int32_t blk_rows = (int32_t)(a.layers * a.kv_heads * a.bs);
    if (ntok > 0) {
      for (int idx = threadIdx.x; idx < npad + 2; idx += kBlock) {
        const int64_t p = t0 + idx - 1;
        int32_t row = -1;
        if (p >= 0 && p < nb) {
          const uint32_t pos = (uint32_t)p;
          const uint32_t lb = pos / bs;
          const int32_t blk = blks[lb - lb0];
          if (blk >= 0) row = blk * blk_rows + head_row0 + (int32_t)(pos - lb * bs);
        }
        rows[kHalo - 1 + idx] = row;
      }
    }
  }
  {
    uint32_t dq, dt, n1 = 0, n2 = 0;
    h84_decode4(threadIdx.x, dq, dt, n1, n2);  // kBlock == 256: one table entry per thread
    lut[threadIdx.x] = (uint8_t)(dq & 0xFu);
  }
  float qsum = 0.0f;  // sum of head n's query over all d (the offset fold)
#pragma unroll
  for (int kk = 0; kk < KK; ++kk)
#pragma unroll
    for (int e = 0; e < 8; ++e) qsum += (float)qop[kk][e];
  qsum += __shfl_xor(qsum, 16, kWave);
  qsum += __shfl_xor(qsum, 32, kWave);
  __syncthreads();

  const __amdgpu_buffer_rsrc_t krs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.k_cache), 0, (int)a.cache_bytes, kRsrcWord3);
  const __amdgpu_buffer_rsrc_t vrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.v_cache), 0, (int)a.cache_bytes, kRsrcWord3);
  const __amdgpu_buffer_rsrc_t ksrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.k_scales), 0, (int)a.scale_bytes, kRsrcWord3);
  const __amdgpu_buffer_rsrc_t vsrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.v_scales), 0, (int)a.scale_bytes, kRsrcWord3);
  const float qscale = a.sm_scale * kAttnLogScale;
  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  float m = -INFINITY, l = 0.0f;
  float psum = 0.0f;  // sum of p * v_scale over this lane's tokens (the offset fold)
  float pvc = 0.0f;   // the PV normaliser ([normaliser]); 0: nothing accumulated yet
  const float qoff = kMfmaValOffset * qsum;

  // the cache rows of token i's neighbours, positions max(l - 1, 0) and min(l + 1, n_b - 1)
  auto left_of = [&](int i) { return rows[kHalo + (t0 + i > 0 ? i - 1 : i)]; };
  auto right_of = [&](int i) { return rows[kHalo + (t0 + i + 1 < nb ? i + 1 : i)]; };

  struct Step {
    int32_t rv[8];
    uint32_t kw[2][KW > 0 ? KW : 1];
    uint32_t vw[8][VW];
    float ks[8], vs[8];
  };
  auto load_step = [&](int i0, Step &st) {
    const int4 r0 = *reinterpret_cast<const int4 *>(&rows[kHalo + i0 + 4 * g]);
    const int4 r1 = *reinterpret_cast<const int4 *>(&rows[kHalo + i0 + 16 + 4 * g]);
    st.rv[0] = r0.x; st.rv[1] = r0.y; st.rv[2] = r0.z; st.rv[3] = r0.w;
    st.rv[4] = r1.x; st.rv[5] = r1.y; st.rv[6] = r1.z; st.rv[7] = r1.w;
#pragma unroll
    for (int tau = 0; tau < 2; ++tau) {
      const int32_t r = rows[kHalo + i0 + 16 * tau + n];
      load_chunk<KB>(krs, (uint32_t)max(r, 0) * (uint32_t)D + (uint32_t)(KB * g), st.kw[tau]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t r = (uint32_t)max(st.rv[j], 0);
      load_chunk<MT>(vrs, r * (uint32_t)D + (uint32_t)(MT * n), st.vw[j]);
      st.ks[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ksrs, r * 4u, 0, 0));
      st.vs[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(vsrs, r * 4u, 0, 0));
    }
  };
  constexpr int kStride = kWaves * kMfmaStep;
  for (int i0 = wave * kMfmaStep; i0 < ntok; i0 += kStride) {
    Step cur;
    load_step(i0, cur);
    const int32_t *rv = cur.rv;
    const float *ks = cur.ks, *vs = cur.vs;
    auto &kw = cur.kw;
    auto &vw = cur.vw;
#ifdef ATTN_BODY_REPAIR  // [repair] the [statistics] island below, storing (as in attn_h84_mfma_body.inc):
    // the stored words, before the slow path rewrites any in registers
    if (counts) {
#pragma unroll
      for (int tau = 0; tau < 2; ++tau) {
        const int32_t r = rows[kHalo + i0 + 16 * tau + n];
        uint32_t dirty = 0;
#pragma unroll
        for (int k = 0; k < KW; ++k) dirty |= h_code4(kw[tau][k]);
        if (r >= 0 && dirty) {
          const uint32_t off = (uint32_t)r * (uint32_t)D + (uint32_t)(KB * g);  // load_step's
#pragma unroll
          for (int k = 0; k < KW; ++k) h84_repair_store(krs, off + 4u * k, kw[tau][k], n_single, n_double, n_rewritten);
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        uint32_t dirty = 0;
#pragma unroll
        for (int k = 0; k < VW; ++k) dirty |= h_code4(vw[j][k] & kVMask);
        if (rv[j] >= 0 && dirty) {
          const uint32_t off = (uint32_t)rv[j] * (uint32_t)D + (uint32_t)(MT * n);
          if constexpr (MT < 4) {  // head_dim 32: the lane's two bytes, as a two-byte store
            h84_repair_store<2>(vrs, off, vw[j][0] & kVMask, n_single, n_double, n_rewritten);
          } else {
#pragma unroll
            for (int k = 0; k < VW; ++k) h84_repair_store(vrs, off + 4u * k, vw[j][k], n_single, n_double, n_rewritten);
          }
        }
      }
    }
#elif defined(ATTN_BODY_STATS)  // [statistics] the stored words, before any is rewritten; rows past n_b are -1
    if (counts) {
#pragma unroll
      for (int tau = 0; tau < 2; ++tau) {
        if (rows[kHalo + i0 + 16 * tau + n] >= 0) {
#pragma unroll
          for (int k = 0; k < KW; ++k) h84_count4(kw[tau][k], n_single, n_double);
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (rv[j] >= 0) {
#pragma unroll
          for (int k = 0; k < VW; ++k) h84_count4(vw[j][k] & kVMask, n_single, n_double);
        }
      }
    }
#endif
    // ---- first look, then the slow path in the lanes that hold a double.  One K row, or four V
    // rows, at a time: their neighbour words are what the slow path keeps in registers, and
    // with all ten rows' at once the kernel took 225-256 VGPRs (2 waves per SIMD) for 140
#pragma unroll
    for (int tau = 0; tau < 2; ++tau) {
      uint32_t kd = 0;
#pragma unroll
      for (int k = 0; k < KW; ++k) kd |= h84_double4(kw[tau][k]);
      if (kd) {
        uint32_t wl[KW], wr[KW];
        const int i = i0 + 16 * tau + n;
        const int32_t rl = left_of(i), rr = right_of(i);
        load_chunk<KB>(krs, (uint32_t)max(rl, 0) * (uint32_t)D + (uint32_t)(KB * g), wl);
        load_chunk<KB>(krs, (uint32_t)max(rr, 0) * (uint32_t)D + (uint32_t)(KB * g), wr);
#pragma unroll
        for (int k = 0; k < KW; ++k)
          if (h84_double4(kw[tau][k]))  // the words without a double stay as they are
            kw[tau][k] = h84_interp_fix4(kw[tau][k], rl >= 0 ? wl[k] : 0u, rr >= 0 ? wr[k] : 0u);
      }
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      uint32_t vd = 0;
#pragma unroll
      for (int j = 4 * half; j < 4 * half + 4; ++j)
#pragma unroll
        for (int k = 0; k < VW; ++k) vd |= h84_double4(vw[j][k] & kVMask);
      if (vd) {
        uint32_t wl[4][VW], wr[4][VW];
        int32_t rl[4], rr[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int i = i0 + 16 * half + 4 * g + jj;  // token of row j = 4 half + jj
          rl[jj] = left_of(i);
          rr[jj] = right_of(i);
          load_chunk<MT>(vrs, (uint32_t)max(rl[jj], 0) * (uint32_t)D + (uint32_t)(MT * n), wl[jj]);
          load_chunk<MT>(vrs, (uint32_t)max(rr[jj], 0) * (uint32_t)D + (uint32_t)(MT * n), wr[jj]);
        }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
          for (int k = 0; k < VW; ++k)
            if (h84_double4(vw[4 * half + jj][k] & kVMask))
              vw[4 * half + jj][k] = h84_interp_fix4(vw[4 * half + jj][k], rl[jj] >= 0 ? wl[jj][k] : 0u,
                                                     rr[jj] >= 0 ? wr[jj][k] : 0u);
      }
    }
    // ---- S^T = K . Q^T, two 16-token tiles
    f32x4 S[2];
#pragma unroll
    for (int tau = 0; tau < 2; ++tau) {
      S[tau] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        uint32_t p[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {  // bytes 8kk + 2h, 8kk + 2h + 1
          const uint32_t w = kw[tau][2 * kk + h / 2];
          const int sh = 16 * (h & 1);
          p[h] = nib_pair_f16(lut[(w >> sh) & 0xFFu], lut[(w >> (sh + 8)) & 0xFFu]);
        }
        S[tau] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, u32x4{p[0], p[1], p[2], p[3]}),
                                                        qop[kk], S[tau], 0, 0, 0);
      }
    }
    // ---- online softmax over this lane's 8 tokens of head n
    float s[8];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool seen = i0 + 16 * (j >> 2) + 4 * g + (j & 3) < col_lim;  // [score mask]
      s[j] = rv[j] >= 0 && seen ? (S[j >> 2][j & 3] * kMfmaValScale - qoff) * (qscale * ks[j]) : -INFINITY;
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
      pw[2 * h] = p0 * vs[2 * h];
      pw[2 * h + 1] = p1 * vs[2 * h + 1];
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
    // ---- O^T += V^T . P: M-tile mt takes byte mt of each token's chunk
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      uint32_t p[4];
#pragma unroll
      for (int h = 0; h < 4; ++h) {  // tokens j = 2h, 2h + 1
        const int sh = 8 * (mt & 3);
        p[h] = nib_pair_f16(lut[(vw[2 * h][mt / 4] >> sh) & 0xFFu], lut[(vw[2 * h + 1][mt / 4] >> sh) & 0xFFu]);
      }
      const f16x8 va = __builtin_bit_cast(f16x8, u32x4{p[0], p[1], p[2], p[3]});
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pb_hi, acc[mt], 0, 0, 0);
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pb_lo, acc[mt], 0, 0, 0);
    }
  }

  // ---- merge: the 4 lanes of a head, then the workgroup's waves
  l += __shfl_xor(l, 16, kWave);
  l += __shfl_xor(l, 32, kWave);
  psum += __shfl_xor(psum, 16, kWave);
  psum += __shfl_xor(psum, 32, kWave);
  const float poff = kMfmaValOffset * psum, oscale = pvc * kMfmaValScale;
  if (n < G) {
    if (g == 0) {
      gml[0][wave][n] = m;
      gml[1][wave][n] = l;
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][n][MT * (4 * g + r) + mt] = acc[mt][r] * oscale - poff;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < G * D; idx += kBlock) {
    const int h = idx / D, d = idx % D;
    const int64_t orow = cm.out_row(a, h);  // none: a column past the chunk
    if (orow < 0) continue;
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) M = fmaxf(M, gml[0][w][h]);
    float o = 0.0f, L = 0.0f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const float mw = gml[0][w][h];
      const float wt = mw == -INFINITY ? 0.0f : attn_exp(mw - M);
      o += red[w][h][d] * wt;
      L += gml[1][w][h] * wt;
    }
    float *ws = a.ws + (orow * a.nsplit + cm.split_idx) * (a.d + 2);
    ws_put(ws + 2 + d, o);
    if (d == 0) {
      ws_put(ws, M);
      ws_put(ws + 1, L);
    }
  }
#ifdef ATTN_BODY_STATS  // [statistics] one reduction and at most two atomics per counting workgroup
  if (counts) {
#ifdef ATTN_BODY_REPAIR  // [repair] ... and a third for the bytes rewritten
    const uint32_t cnt[3] = {n_single, n_double, n_rewritten};
    flush_stats_n<3>(a.stats, cnt);
#else
    const uint32_t cnt[2] = {n_single, n_double};
    flush_stats_n<2>(a.stats, cnt);
#endif
  }
#endif
