// Body of paged_attn_golay_mfma_kernel (ATTN_BODY_CHUNK 0, `a` an AttnArgs, G query
// heads in the first G columns) and of paged_attn_golay_mfma_chunk_kernel (ATTN_BODY_CHUNK
// 1, `a` a ChunkArgs, G = 16 (token, head) columns: ChunkMap; the ragged entry's
// paged_attn_golay_mfma_ragged_kernel is the same text over a RaggedArgs and its ChunkMap), included by
// attention.hip inside each kernel: the decode kernel's text is what it always
// was, so its code is too (see ChunkArgs).
// attention.hip defines ATTN_BODY_CHUNK around each inclusion; it is no build switch.
// The counted kernel (paged_attn_golay_mfma_stats_kernel, `a` a StatsArgs, the ragged form) also
// defines ATTN_BODY_STATS: the [statistics] islands; without it the preprocessed text is what it was.
  constexpr int D = 128, GC = 43;          // head_dim, codewords per row
  constexpr int KC = PACKED ? 12 : 11;     // K codewords per lane group
  constexpr int KD = 3 * KC, KK = 5;       // its values; QK MFMAs per 16 tokens
  constexpr int VC = 3, MT = 9;            // V codewords per lane; PV M-tiles
  constexpr int KW = PACKED ? 9 : KC;      // K dwords per lane group
  constexpr uint32_t kRowBytes = PACKED ? KVECC_GOLAY_PACKED_ROW(GC) : GC * 4;
  constexpr int kWaves = kBlock / kWave;
  __shared__ __attribute__((aligned(16))) uint32_t gt[8192];  // spread tables (golay_attn_table_dev)
  __shared__ __attribute__((aligned(16))) int32_t rows[kMaxSplit + kMfmaStep];
  __shared__ int32_t blks[kMaxSplit + 1];
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
  // As in attn_h84_mfma_body.inc: the tile that holds the sequence's last valid token, in
  // the first column group of its cache head -- one workgroup per (sequence, cache head,
  // split).  It walks the sequence's n_b rows; the columns' own limits mask the scores.
  const ChunkSpan csp(a, b);
  const bool counts = csp.v1(a) > csp.v0() && cm.tile == (uint32_t)(csp.v1(a) - 1) / (16u >> a.cg_log2) &&
                      h0 % (a.heads / a.kv_heads) == 0;
  const int64_t ctx = counts ? min<int64_t>(a.ctx_lens[b], a.ctx_cap) : cm.ctx;
  uint32_t n_bits = 0, n_unc = 0;  // bits corrected (counts 1..3), uncorrectable words (count 4)
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
  // Q^T operand: k-slot v = 8kk + j of lane group g is d = KD g + v (v < KD, d < 128), else 0;
  // issued before the block-table round trip, as in the H(8,4) kernel
  f16x8 qop[KK];
  {
#if ATTN_BODY_CHUNK  // [query load] the column's (token, head) row through the strides; guard below
    const __half *qh = cm.q_row(a);
#else
    const __half *qh = reinterpret_cast<const __half *>(a.q) + (b * a.heads + h0 + n) * D;
#endif
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int v = 8 * kk + j, d = KD * g + v;
        _Float16 x = 0;
#if ATTN_BODY_CHUNK  // [query load] columns past the chunk load nothing
        if (cm.col_ok && v < KD && d < D) x = __builtin_bit_cast(_Float16, qh[d]);
#else
        if (n < G && v < KD && d < D) x = __builtin_bit_cast(_Float16, qh[d]);
#endif
        qop[kk][j] = x;
      }
    }
  }
  {  // block-table slice -> cache rows, as in the H(8,4) kernel
    const uint32_t bs = (uint32_t)a.bs;
    const uint32_t lb0 = (uint32_t)(t0 / a.bs);
    const int64_t tmax = min<int64_t>(t0 + a.split, a.max_blocks * a.bs);
    const int nlb = tmax > t0 ? (int)((uint32_t)(tmax - 1) / bs - lb0 + 1) : 0;
    const int32_t *tab = a.table + b * a.max_blocks + lb0;
    for (int j = threadIdx.x; j < nlb; j += kBlock) blks[j] = tab[j];
    {
      const u32x4 *src = reinterpret_cast<const u32x4 *>(a.atab);
      for (int i = threadIdx.x; i < 2048; i += kBlock) reinterpret_cast<u32x4 *>(gt)[i] = src[i];
    }
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
  float qsum = 0.0f;
  {
#pragma unroll
    for (int kk = 0; kk < KK; ++kk)
#pragma unroll
      for (int j = 0; j < 8; ++j) qsum += (float)qop[kk][j];
    qsum += __shfl_xor(qsum, 16, kWave);
    qsum += __shfl_xor(qsum, 32, kWave);
  }
  __syncthreads();

  // codeword -> data nibbles one per byte (bytes 0..2), uncorrectable words keep
  // their data.  (The split kernels' table, parity at the codeword's parity
  // bits and the nibbles in bytes 0, 1, 3, measured 1 % slower here:
  // profiles/r04/attn/xtab_ab.log.)
#ifdef ATTN_BODY_STATS  // [statistics] the decoded word keeps the correction entry's byte 3: (bits corrected & 3) |
  // uncorrectable << 6 (runtime.hip, ensure_tables), one v_and_or more per codeword; `pair` reads bytes 0..2 only
  auto sp_of = [&](uint32_t c) -> uint32_t {
    const uint32_t p = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(gt) + ((c << 2) & 0x3FFCu));
    const uint32_t off = ((c >> 10) ^ (p >> 18)) & 0x3FFCu;
    const uint32_t e = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(gt + 4096) + off);
    return (e & 0xFF000000u) | __builtin_amdgcn_bitop3_b32(p, e, 0x000F0F0Fu, 0x28);
  };
  // the count fields of up to 21 codewords summed (3 * 21 < 64), folded into the lane's counters
  auto fold = [&](uint32_t f) {
    n_bits += f & 0x3Fu;
    n_unc += f >> 6;
  };
#else
  auto sp_of = [&](uint32_t c) -> uint32_t {
    const uint32_t p = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(gt) + ((c << 2) & 0x3FFCu));
    const uint32_t off = ((c >> 10) ^ (p >> 18)) & 0x3FFCu;
    const uint32_t e = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(gt + 4096) + off);
    return __builtin_amdgcn_bitop3_b32(p, e, 0x000F0F0Fu, 0x28);  // (p ^ e) & mask
  };
#endif
  // f16 subnormal pair: byte e0 of lo (0x0c: zero), byte e1 of hi, in halves 0 and 1
  auto pair = [](uint32_t hi, uint32_t lo, int e0, int e1) -> uint32_t {
    const uint32_t s0 = e0 < 0 ? 0x0cu : (uint32_t)e0, s1 = e1 < 0 ? 0x0cu : (uint32_t)(4 + e1);
    return __builtin_amdgcn_perm(hi, lo, 0x0c000c00u | s1 << 16 | s0);
  };

  const __amdgpu_buffer_rsrc_t krs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.k_cache), 0, (int)a.cache_bytes, kRsrcWord3);
  const __amdgpu_buffer_rsrc_t vrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.v_cache), 0, (int)a.cache_bytes, kRsrcWord3);
  const __amdgpu_buffer_rsrc_t ksrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.k_scales), 0, (int)a.scale_bytes, kRsrcWord3);
  const __amdgpu_buffer_rsrc_t vsrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.v_scales), 0, (int)a.scale_bytes, kRsrcWord3);
  constexpr float kScale = 16777216.0f, kOff = 8.0f;  // subnormal operands: 2^24, and n - 8
  const float qscale = a.sm_scale * kAttnLogScale;
  const float qoff = kOff * qsum;
  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  float m = -INFINITY, l = 0.0f, psum = 0.0f;
  float pvc = 0.0f;  // the PV normaliser ([normaliser]); 0: nothing accumulated yet

  for (int i0 = wave * kMfmaStep; i0 < ntok; i0 += kWaves * kMfmaStep) {
    int32_t rv[8];
    {
      const int4 r0 = *reinterpret_cast<const int4 *>(&rows[i0 + 4 * g]);
      const int4 r1 = *reinterpret_cast<const int4 *>(&rows[i0 + 16 + 4 * g]);
      rv[0] = r0.x; rv[1] = r0.y; rv[2] = r0.z; rv[3] = r0.w;
      rv[4] = r1.x; rv[5] = r1.y; rv[6] = r1.z; rv[7] = r1.w;
    }
    uint32_t kw[2][KW];
#pragma unroll
    for (int tau = 0; tau < 2; ++tau) {
      const uint32_t off = (uint32_t)max(rows[i0 + 16 * tau + n], 0) * kRowBytes + 4u * KW * g;
      const u32x4 x0 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(krs, off, 0, 0));
      const u32x4 x1 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(krs, off + 16, 0, 0));
      kw[tau][0] = x0.x; kw[tau][1] = x0.y; kw[tau][2] = x0.z; kw[tau][3] = x0.w;
      kw[tau][4] = x1.x; kw[tau][5] = x1.y; kw[tau][6] = x1.z; kw[tau][7] = x1.w;
      if constexpr (PACKED) {
        kw[tau][8] = __builtin_amdgcn_raw_buffer_load_b32(krs, off + 32, 0, 0);
      } else {
        const auto x2 = __builtin_amdgcn_raw_buffer_load_b96(krs, off + 32, 0, 0);
        kw[tau][8] = x2[0]; kw[tau][9] = x2[1]; kw[tau][10] = x2[2];
      }
    }
    // V: this lane's codewords start 12n bytes (int32) or 9n bytes (packed) into the row
    const uint32_t voff = PACKED ? (9u * n) & ~3u : 12u * n;
    const uint32_t vsh = n & 3;  // packed: byte of the first codeword in the loaded dword
    uint32_t vw[8][VC];
    float ks[8], vs[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t r = (uint32_t)max(rv[j], 0);
      const auto x = __builtin_amdgcn_raw_buffer_load_b96(vrs, r * kRowBytes + voff, 0, 0);
      vw[j][0] = x[0]; vw[j][1] = x[1]; vw[j][2] = x[2];
      ks[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ksrs, r * 4u, 0, 0));
      vs[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(vsrs, r * 4u, 0, 0));
    }
    // ---- S^T = K . Q^T
    f32x4 S[2];
#pragma unroll
    for (int tau = 0; tau < 2; ++tau) {
      uint32_t cw[KC];
      if constexpr (PACKED) {  // 4 little-endian 3-byte codewords per 3 dwords
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const uint32_t d0 = kw[tau][3 * t], d1 = kw[tau][3 * t + 1], d2 = kw[tau][3 * t + 2];
          cw[4 * t] = d0;
          cw[4 * t + 1] = __builtin_amdgcn_alignbyte(d1, d0, 3);
          cw[4 * t + 2] = __builtin_amdgcn_alignbyte(d2, d1, 2);
          cw[4 * t + 3] = d2 >> 8;
        }
      } else {
#pragma unroll
        for (int c = 0; c < KC; ++c) cw[c] = kw[tau][c];
      }
      uint32_t sp[KC];
#pragma unroll
      for (int c = 0; c < KC; ++c) sp[c] = sp_of(cw[c]);
#ifdef ATTN_BODY_STATS  // [statistics] K: lane (n, g) holds codewords KC g .. KC g + KC - 1 of token n's row, once
      if (counts && rows[i0 + 16 * tau + n] >= 0) {  // not a -1 block's / a past row's row 0
        uint32_t f = 0;  // <= 12 codewords
#pragma unroll
        for (int c = 0; c < KC; ++c)
          if (c < GC - 3 * KC || g < 3) f += sp[c] >> 24;  // group 3's tail: codewords >= 43 are the next row's
        fold(f);
      }
#endif
      S[tau] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        uint32_t p[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          const int v0 = 8 * kk + 2 * h, v1 = v0 + 1;
          const int c0 = v0 < KD ? v0 / 3 : 0, c1 = v1 < KD ? v1 / 3 : 0;
          p[h] = pair(sp[c1], sp[c0], v0 < KD ? v0 % 3 : -1, v1 < KD ? v1 % 3 : -1);
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
      s[j] = rv[j] >= 0 && seen ? (S[j >> 2][j & 3] * kScale - qoff) * (qscale * ks[j]) : -INFINITY;
#else
      s[j] = rv[j] >= 0 ? (S[j >> 2][j & 3] * kScale - qoff) * (qscale * ks[j]) : -INFINITY;
#endif
      mx = fmaxf(mx, s[j]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, kWave));
    mx = fmaxf(mx, __shfl_xor(mx, 32, kWave));
    const float mn = fmaxf(m, mx);
    const float mu = mn == -INFINITY ? 0.0f : mn;
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
    // ---- O^T += V^T . P: tile mt takes nibble mt % 3 of codeword mt / 3
    uint32_t sv[8][VC];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if constexpr (PACKED) {  // codeword c at byte vsh + 3c of the 12 loaded (alignbyte uses shift & 3)
        const uint32_t d0 = vw[j][0], d1 = vw[j][1], d2 = vw[j][2];
        vw[j][0] = __builtin_amdgcn_alignbyte(d1, d0, vsh);
        vw[j][1] = __builtin_amdgcn_alignbyte(vsh ? d2 : d1, vsh ? d1 : d0, vsh + 3);
        vw[j][2] = __builtin_amdgcn_alignbyte(d2, vsh < 2 ? d1 : d2, vsh + 2);
      }
#pragma unroll
      for (int c = 0; c < VC; ++c) sv[j][c] = sp_of(vw[j][c]);
#ifdef ATTN_BODY_STATS  // [statistics] V: lane n holds codewords 3n .. 3n + 2 of its 8 rows, once (lanes 14-15: >= 43)
      if (counts && rv[j] >= 0) {
        uint32_t f = 0;
#pragma unroll
        for (int c = 0; c < VC; ++c)
          if (VC * n + c < GC) f += sv[j][c] >> 24;
        fold(f);
      }
#endif
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      uint32_t p[4];
#pragma unroll
      for (int h = 0; h < 4; ++h) p[h] = pair(sv[2 * h + 1][mt / 3], sv[2 * h][mt / 3], mt % 3, mt % 3);
      const f16x8 va = __builtin_bit_cast(f16x8, u32x4{p[0], p[1], p[2], p[3]});
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pb_hi, acc[mt], 0, 0, 0);
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pb_lo, acc[mt], 0, 0, 0);
    }
  }

  // ---- merge, as in the H(8,4) kernel
  l += __shfl_xor(l, 16, kWave);
  l += __shfl_xor(l, 32, kWave);
  psum += __shfl_xor(psum, 16, kWave);
  psum += __shfl_xor(psum, 32, kWave);
  const float poff = kOff * psum, oscale = pvc * kScale;
  if (n < G) {
    if (g == 0) {
      gml[0][wave][n] = m;
      gml[1][wave][n] = l;
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int d = MT * (4 * g + r) + mt;
        if (d < D) red[wave][n][d] = acc[mt][r] * oscale - poff;
      }
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
    const uint32_t cnt[2] = {n_bits, n_unc};
    flush_stats_n<2>(a.stats, cnt);
  }
#endif
#if !ATTN_BODY_CHUNK  // the counted combine: decode kernels only (chunk calls always launch the combine)
  if (a.ctr) combine_if_last<__half, G>(a, b * a.heads + h0, reinterpret_cast<float *>(rows));
#endif
