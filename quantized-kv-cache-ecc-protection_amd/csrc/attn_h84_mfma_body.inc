// Body of paged_attn_h84_mfma_kernel (ATTN_BODY_CHUNK 0, `a` an AttnArgs, G query
// heads in the first G columns) and of paged_attn_h84_mfma_chunk_kernel (ATTN_BODY_CHUNK
// 1, `a` a ChunkArgs, G = 16 (token, head) columns: ChunkMap; the ragged entry's
// paged_attn_h84_mfma_ragged_kernel is the same text over a RaggedArgs and its ChunkMap), included by
// attention.hip inside each kernel: the decode kernel's text is what it always
// was, so its code is too (see ChunkArgs).
// attention.hip defines ATTN_BODY_CHUNK around each inclusion; it is no build switch.
// The counted kernel (paged_attn_h84_mfma_stats_kernel, `a` a StatsArgs, the ragged form) also
// defines ATTN_BODY_STATS: the [statistics] islands; without it the preprocessed text is what it was.
// The repairing kernel (paged_attn_h84_mfma_repair_kernel, `a` a RepairArgs) defines ATTN_BODY_REPAIR
// as well: the [repair] islands, in which the counting workgroup stores the corrected codewords back
// where it counts them (kvecc.h "Repairing attention"); without it the text is the counted kernel's.
  constexpr int KK = D / 32;  // QK MFMAs per 16-token tile
  constexpr int MT = D / 16;  // PV M-tiles; V bytes per lane per token
  constexpr int KB = D / 4;   // K bytes per lane per token
  constexpr int VW = MT >= 4 ? MT / 4 : 1;  // V dwords per token
  constexpr int kWaves = kBlock / kWave;
  __shared__ __attribute__((aligned(16))) int32_t rows[kMaxSplit + kMfmaStep];
  __shared__ int32_t blks[kMaxSplit + 1];
  __shared__ uint8_t lut[256];
  __shared__ float red[kWaves][G][D];
  __shared__ float gml[2][kWaves][G];

  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int n = lane & 15, g = lane >> 4;
#if ATTN_BODY_CHUNK  // [column map] cm is used by every other chunk island of this file
  const ChunkMap cm(a, n);  // column n's (token, head); blockIdx.x = tile * nsplit + split
  if constexpr (ChunkMap::kRagged) {
    if (!cm.any) {  // every token of the tile is padding: nothing staged, no table or cache read
      cm.put_empty(a);
      return;
    }
  }
  const int64_t b = cm.b, h0 = cm.h0;
  const int64_t hk = h0 / (a.heads / a.kv_heads);
#ifdef ATTN_BODY_STATS  // [statistics] who counts (kvecc.h "Counted attention"): uniform per workgroup
  // The tile that holds the sequence's last valid token, in the first column group of
  // its cache head, counts: one workgroup per (sequence, cache head, split).  It walks
  // the sequence's n_b rows -- the tile's largest key limit unless the span overruns
  // q_max; the columns' own limits mask the scores either way ([score mask]).
  const ChunkSpan csp(a, b);
  const bool counts = csp.v1(a) > csp.v0() && cm.tile == (uint32_t)(csp.v1(a) - 1) / (16u >> a.cg_log2) &&
                      h0 % (a.heads / a.kv_heads) == 0;
  const int64_t ctx = counts ? min<int64_t>(a.ctx_lens[b], a.ctx_cap) : cm.ctx;
  uint32_t n_single = 0, n_double = 0;
#ifdef ATTN_BODY_REPAIR  // [repair] bytes rewritten: the statistics buffer's word 2
  uint32_t n_rewritten = 0;
#endif
#else
  const int64_t ctx = cm.ctx;  // the largest key limit of the tile's columns
#endif
  const int64_t t0 = (int64_t)cm.split_idx * a.split;
#else
  const int64_t hgroups = a.heads / G;
  const int64_t b = blockIdx.y / hgroups, h0 = (blockIdx.y % hgroups) * G;
  const int64_t hk = h0 / (a.heads / a.kv_heads);
  const int64_t ctx = min<int64_t>(a.ctx_lens[b], a.ctx_cap);
  const int64_t t0 = (int64_t)blockIdx.x * a.split;
#endif
  const int64_t t1 = min<int64_t>(t0 + a.split, ctx);
  const int ntok = t1 > t0 ? (int)(t1 - t0) : 0;
#if ATTN_BODY_CHUNK  // [key limit] applied at [score mask]
  const int col_lim = cm.col_limit(t0);  // this column's keys: the split's tokens below it
#endif
  // Q^T operand (B): column n = head h0 + n, k-slot 8g + j of MFMA kk = d (D/4)g + 8kk + j.
  // Issued first: it lands during the block-table round trip instead of
  // after it (its first use, the query sum, precedes the first K/V loads)
  f16x8 qop[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) {
    u32x4 v = {0u, 0u, 0u, 0u};
#if ATTN_BODY_CHUNK  // [query load] the column's (token, head) row through the strides
    if (cm.col_ok) v = *reinterpret_cast<const u32x4 *>(cm.q_row(a) + KB * g + 8 * kk);
#else
    if (n < G)
      v = *reinterpret_cast<const u32x4 *>(reinterpret_cast<const __half *>(a.q) +
                                           (b * a.heads + h0 + n) * D + KB * g + 8 * kk);
#endif
    qop[kk] = __builtin_bit_cast(f16x8, v);
  }
  {  // block-table slice -> cache rows (-1: no block / past the split)
    const uint32_t bs = (uint32_t)a.bs;
    const uint32_t lb0 = (uint32_t)(t0 / a.bs);
    // the whole split's slice, bounded by the table rather than the context, so
    // the load does not wait for context_lens (one dependent HBM trip fewer)
    const int64_t tmax = min<int64_t>(t0 + a.split, a.max_blocks * a.bs);
    const int nlb = tmax > t0 ? (int)((uint32_t)(tmax - 1) / bs - lb0 + 1) : 0;
    const int32_t *tab = a.table + b * a.max_blocks + lb0;
    for (int j = threadIdx.x; j < nlb; j += kBlock) blks[j] = tab[j];
    __syncthreads();
    const int32_t head_row0 = (int32_t)((a.layer * a.kv_heads + hk) * a.bs);
    const int32_t blk_rows = (int32_t)(a.layers * a.kv_heads * a.bs);
    const int npad = (ntok + kMfmaStep - 1) / kMfmaStep * kMfmaStep;
    for (int i = threadIdx.x; i < npad; i += kBlock) {
      int32_t row = -1;
      if (i < ntok) {
        const uint32_t pos = (uint32_t)(t0 + i);
        const uint32_t lb = pos / bs;
        const int32_t blk = blks[lb - lb0];
        if (blk >= 0) row = blk * blk_rows + head_row0 + (int32_t)(pos - lb * bs);
      }
      rows[i] = row;
    }
  }
  // kBlock == 256: one table entry per thread (the byte family's kernels: their codec's table)
  lut[threadIdx.x] = (uint8_t)byte_table_nibble(a, threadIdx.x);
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

  // one step's operands in registers: 2 K rows (tokens i0 + n, i0 + 16 + n),
  // 8 V rows and scales (tokens i0 + 16(j >> 2) + 4g + (j & 3)); invalid rows
  // read row 0 and are masked
  struct Step {
    int32_t rv[8];
    uint32_t kw[2][KB / 4 > 0 ? KB / 4 : 1];
    uint32_t vw[8][VW];
    float ks[8], vs[8];
  };
  auto load_step = [&](int i0, Step &st) {
    const int4 r0 = *reinterpret_cast<const int4 *>(&rows[i0 + 4 * g]);
    const int4 r1 = *reinterpret_cast<const int4 *>(&rows[i0 + 16 + 4 * g]);
    st.rv[0] = r0.x; st.rv[1] = r0.y; st.rv[2] = r0.z; st.rv[3] = r0.w;
    st.rv[4] = r1.x; st.rv[5] = r1.y; st.rv[6] = r1.z; st.rv[7] = r1.w;
#pragma unroll
    for (int tau = 0; tau < 2; ++tau) {
      const int32_t r = rows[i0 + 16 * tau + n];
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
#ifdef ATTN_BODY_REPAIR  // [repair] the [statistics] island below, storing: only the counting workgroup,
    // only rows it counts (never a masked lane's row 0), only words with a byte to rewrite.  A
    // row's first look is the OR of its words' h_code4: a clean row counts and stores nothing.
    if (counts) {
#pragma unroll
      for (int tau = 0; tau < 2; ++tau) {
        const int32_t r = rows[i0 + 16 * tau + n];
        uint32_t dirty = 0;
#pragma unroll
        for (int k = 0; k < KB / 4; ++k) dirty |= h_code4(kw[tau][k]);
        if (r >= 0 && dirty) {
          const uint32_t off = (uint32_t)r * (uint32_t)D + (uint32_t)(KB * g);  // load_step's
#pragma unroll
          for (int k = 0; k < KB / 4; ++k) h84_repair_store(krs, off + 4u * k, kw[tau][k], n_single, n_double, n_rewritten);
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        uint32_t dirty = 0;
#pragma unroll
        for (int k = 0; k < VW; ++k) dirty |= h_code4(MT < 4 ? vw[j][k] & 0xFFFFu : vw[j][k]);
        if (rv[j] >= 0 && dirty) {
          const uint32_t off = (uint32_t)rv[j] * (uint32_t)D + (uint32_t)(MT * n);
          if constexpr (MT < 4) {  // head_dim 32: the lane's two bytes, as a two-byte store
            h84_repair_store<2>(vrs, off, vw[j][0] & 0xFFFFu, n_single, n_double, n_rewritten);
          } else {
#pragma unroll
            for (int k = 0; k < VW; ++k) h84_repair_store(vrs, off + 4u * k, vw[j][k], n_single, n_double, n_rewritten);
          }
        }
      }
    }
#elif defined(ATTN_BODY_STATS)  // [statistics] every lane's K and V words are its own: each stored byte once
    if (counts) {
#pragma unroll
      for (int tau = 0; tau < 2; ++tau) {
        if (rows[i0 + 16 * tau + n] >= 0) {  // not a -1 block's / a past row's row 0
#pragma unroll
          for (int k = 0; k < KB / 4; ++k) h84_count4(kw[tau][k], n_single, n_double);
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (rv[j] >= 0) {
#pragma unroll
          for (int k = 0; k < VW; ++k)  // (head_dim 32: two bytes per token, the rest of the dword as clean codewords)
            h84_count4(MT < 4 ? vw[j][k] & ((1u << (8 * (MT & 3))) - 1u) : vw[j][k], n_single, n_double);
        }
      }
    }
#endif
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
#if ATTN_BODY_CHUNK  // [score mask] col_lim from [key limit]
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
#if !ATTN_BODY_CHUNK  // [merge: workspace row] decode: head h0's row, the others at a fixed stride (below)
  const int64_t ws_stride = a.nsplit * (a.d + 2);
  float *ws0 = a.ws + ((b * a.heads + h0) * a.nsplit + blockIdx.x) * (a.d + 2);
#endif
  for (int idx = threadIdx.x; idx < G * D; idx += kBlock) {
    const int h = idx / D, d = idx % D;
#if ATTN_BODY_CHUNK  // [merge: workspace row] chunk: column h's own output row; none: a column past the chunk
    const int64_t orow = cm.out_row(a, h);
    if (orow < 0) continue;
#endif
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
#if ATTN_BODY_CHUNK  // [merge: workspace row] orow from the loop's head / ws0 from before the loop
    float *ws = a.ws + (orow * a.nsplit + cm.split_idx) * (a.d + 2);
#else
    float *ws = ws0 + h * ws_stride;
#endif
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
#if !ATTN_BODY_CHUNK  // the counted combine: decode kernels only (chunk calls always launch the combine)
  if (a.ctr) combine_if_last<__half, G>(a, b * a.heads + h0, reinterpret_cast<float *>(rows));
#endif
