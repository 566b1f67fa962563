// Body of paged_attn_split_kernel (ATTN_BODY_CHUNK 0, `a` an AttnArgs) and of
// paged_attn_split_chunk_kernel (ATTN_BODY_CHUNK 1, `a` a RaggedArgs: ChunkArgs and the
// nullable query spans), included
// by attention.hip inside each kernel: the decode kernel's text is what it
// always was, so its code is too (see ChunkArgs).
// paged_attn_split_interp_kernel includes it at ATTN_BODY_CHUNK 2 (`a` an InterpArgs): the chunk
// form plus the [interpolation] island; at 0 and 1 the preprocessed text is what it was.
// attention.hip defines ATTN_BODY_CHUNK around each inclusion; it is no build switch.
// The counted kernels (paged_attn_split_stats*_kernel, `a` a StatsArgs / StatsInterpArgs) also
// define ATTN_BODY_STATS: the [statistics] islands; without it the preprocessed text is what it was.
// So do the Golay counted kernels (paged_attn_split_golay_stats_kernel, `a` a StatsArgs, ATTN_BODY_CHUNK 1):
// their counters hold bits corrected / uncorrectable words (Chunk::count) under the same names.
// The repairing kernels (paged_attn_split_repair*_kernel, `a` a RepairArgs / RepairInterpArgs, Hamming(8,4))
// define ATTN_BODY_REPAIR besides ATTN_BODY_STATS: the [repair] islands, in which the counting workgroup's
// live lanes store the corrected codewords of the rows they count (kvecc.h "Repairing attention").
// The windowed kernels (paged_attn_split_window_kernel, `a` a WindowArgs, ATTN_BODY_CHUNK 1) define
// ATTN_BODY_WINDOW: the [window] islands -- the row's lower key bound, the empty split's early exit, the
// -1 rows between sinks and window; without it the preprocessed text is what it was.
  constexpr bool SP = (DEC & 1) != 0;  // Chunk::decode's DEC bits (experiment forks only)
  using C = Chunk<CODEC, VEC>;
  constexpr int E = C::E;
  constexpr int TP = kBlock / W;  // token rows per pass (one per lane group)
  // cache row of each token of the split (-1 = no block / past the split),
  // padded so the unrolled loop reads it without bounds checks
  // (UR > 0: another count, for the experiment forks)
  constexpr int U = UR > 0                        ? UR
                    : CODEC == KVECC_CODEC_GOLAY ? kGolayUnroll
                    : CODEC == KVECC_CODEC_H84   ? kH84Unroll
                                                 : kUnroll;
  static_assert(U <= kMaxUnroll, "rows in flight");
  __shared__ int32_t rows[kMaxSplit + (kMaxUnroll - 1) * kBlock];
  // Golay tables copied from the device: the 32 KiB spread tables, or
  // parity[4096] then correct[4096] as uint16 (16 KiB).  With the spread
  // tables the block-table slice (before the copy) and the merge buffer (after
  // the loop) live in the same LDS, which keeps 4 workgroups per CU.
  constexpr bool kSpread = is_golay(CODEC);
  // (DEC 2, the no-lookup probe: no tables, only the aliased block-table slice and merge buffer)
  constexpr int kProbeWords = TP * W * E > kMaxSplit + 1 ? TP * W * E : kMaxSplit + 1;
  constexpr int kTabWords = !is_golay(CODEC) ? 4 : (DEC & 2) ? kProbeWords : SP ? 4096 + 128 : kSpread ? 8192 : 4096;
  static_assert(!kSpread || (TP * W * E <= kTabWords && kMaxSplit + 1 <= kTabWords), "LDS aliasing");
  __shared__ __attribute__((aligned(16))) uint32_t gtab[kTabWords];
  __shared__ float red_own[kSpread ? 1 : TP * W * E];  // per-group acc
  float *red = kSpread ? reinterpret_cast<float *>(gtab) : red_own;
  __shared__ float gml[2][TP];             // per-group running max / sum
  __shared__ h84_lut_t lut[CODEC == KVECC_CODEC_H84 ? 256 : 1];  // H(8,4): codeword byte -> data - 8

  const int64_t hgroups = a.heads / G;
#if ATTN_BODY_CHUNK  // [virtual batch] bt and tq are used by the three islands below
  // b: a row of the virtual batch, token tq of sequence bt (at position context_len - q_len + tq)
  const int64_t b = a.vb0 + blockIdx.y / hgroups, h0 = (blockIdx.y % hgroups) * G;  // query heads h0 .. h0+G-1
  const uint32_t bt = (uint32_t)b / a.q_len, tq = (uint32_t)b - bt * a.q_len;
  const ChunkSpan sp(a, bt);  // the sequence's valid tokens (a uniform call: all q_len)
  const bool row_ok = sp.valid(a, tq);  // a padding row reads no query and sees no key: the empty partial
#else
  const int64_t b = blockIdx.y / hgroups, h0 = (blockIdx.y % hgroups) * G;  // query heads h0 .. h0+G-1
#endif
  const int64_t hk = h0 / (a.heads / a.kv_heads);
  const int grp = threadIdx.x / W, c = threadIdx.x % W;
#if ATTN_BODY_CHUNK  // [virtual batch] the row's key limit
  // the keys at or before the token's own position, max_context_len and the table
  const int64_t ctx = row_ok ? min<int64_t>(sp.lim0(a, bt) + tq, a.ctx_cap) : 0;
#else
  const int64_t ctx = min<int64_t>(a.ctx_lens[b], a.ctx_cap);  // max_context_len and the table
#endif
#ifdef ATTN_BODY_WINDOW  // [window] the row's lower key bound; the split's place follows it (WindowArgs::split_start)
  // The row sits at position p = lim0 + tq - 1 and sees key j < ctx iff j < sinks or j >= lo =
  // max(p - window + 1, 0) (kvecc.h "Windowed attention").
  const int64_t lo = row_ok ? max<int64_t>(sp.lim0(a, bt) + tq - (int64_t)a.window, 0) : 0;
  const int64_t t0 = a.split_start(blockIdx.x, lo);
#else
  const int64_t t0 = (int64_t)blockIdx.x * a.split;
#endif
#ifdef ATTN_BODY_STATS  // [statistics] who counts (kvecc.h "Counted attention"): uniform per workgroup
  // The row of the sequence's last valid token, in the first query-head group of
  // its cache head, counts: one workgroup per (sequence, cache head, split).  It
  // walks the sequence's n_b rows -- its own key limit unless the span overruns
  // q_max, where the rows past the limit are counted and masked (ntok_att).
  const bool counts = row_ok && (int64_t)tq + 1 == sp.v1(a) && h0 % (a.heads / a.kv_heads) == 0;
  const int64_t walk = counts ? min<int64_t>(a.ctx_lens[bt], a.ctx_cap) : ctx;
  const int64_t t1 = min<int64_t>(t0 + a.split, walk);
  const int ntok = t1 > t0 ? (int)(t1 - t0) : 0;
  const int ntok_att = (int)max<int64_t>(min<int64_t>(ctx - t0, ntok), 0);
  uint32_t n_single = 0, n_double = 0;
#ifdef ATTN_BODY_REPAIR  // [repair] bytes rewritten: the statistics buffer's word 2
  uint32_t n_rewritten = 0;
#endif
#else
  const int64_t t1 = min<int64_t>(t0 + a.split, ctx);
  const int ntok = t1 > t0 ? (int)(t1 - t0) : 0;
#endif
  const bool live = c < (a.g + VEC - 1) / VEC;  // lanes past the row idle
  const int cs = live ? c : 0;
  const int64_t ws_stride = a.nsplit * (a.d + 2);  // per query head
  float *ws0 = a.ws + ((b * a.heads + h0) * a.nsplit + blockIdx.x) * (a.d + 2);
#ifdef ATTN_BODY_WINDOW  // [window] the split's share of the row's visible keys
  // In this split the row sees the sink keys [t0, min(t1, sinks)) and the window keys
  // [max(t0, lo), t1).  A split that holds neither -- one past the row's limit included -- reads
  // no block table and no cache: it writes the empty partial (m = -inf, l = 0, zero
  // accumulators), which the combine gives no weight, and leaves.
  const bool sees_sink = min<int64_t>(t1, a.sinks) > t0, sees_win = t1 > max<int64_t>(t0, lo);
  if (!sees_sink && !sees_win) {  // uniform per workgroup
    const int nws = (int)a.d + 2;
    for (int idx = threadIdx.x; idx < G * nws; idx += kBlock) {
      const int j = idx / nws, e = idx - j * nws;
      ws_put(ws0 + j * ws_stride + e, e == 0 ? -INFINITY : 0.0f);
    }
    return;
  }
  // the first pass of the streaming loop that holds a visible key: the passes before it hold -1 rows only
  const int i_first = sees_sink ? 0 : (int)(max<int64_t>(lo - t0, 0) / (TP * U)) * (TP * U);
#endif
  // this lane's query slice, issued before the block-table round trip (first
  // used by the query sums after it)
  float qv[G][E];
  const float qscale = a.sm_scale * kAttnLogScale;
#pragma unroll
  for (int j = 0; j < G; ++j) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int64_t di = (int64_t)c * E + e;
#if ATTN_BODY_CHUNK  // [virtual batch] the row's query through the strides
      qv[j][e] = (live && di < a.d && row_ok)
                     ? to_f32<T>(reinterpret_cast<const T *>(a.q)[bt * a.q_sb + tq * a.q_st + (h0 + j) * a.q_sh + di]) *
                           qscale
#else
      qv[j][e] = (live && di < a.d)
                     ? to_f32<T>(reinterpret_cast<const T *>(a.q)[(b * a.heads + h0 + j) * a.d + di]) * qscale
#endif
                     : 0.0f;
    }
  }

  {  // block-table slice -> LDS (one load per logical block), then one 32-bit
     // division per token; none in the streaming loop
    __shared__ int32_t blks_own[kSpread ? 1 : kMaxSplit + 1];
    int32_t *blks = kSpread ? reinterpret_cast<int32_t *>(gtab) : blks_own;
    const uint32_t bs = (uint32_t)a.bs;
    const uint32_t lb0 = (uint32_t)(t0 / a.bs);
    // the whole split's slice, bounded by the table rather than the context, so
    // the load does not wait for context_lens (one dependent HBM trip fewer)
    const int64_t tmax = min<int64_t>(t0 + a.split, a.max_blocks * a.bs);
    const int nlb = tmax > t0 ? (int)((uint32_t)(tmax - 1) / bs - lb0 + 1) : 0;
#if ATTN_BODY_CHUNK  // [virtual batch] the sequence's block-table row
    const int32_t *tab = a.table + (int64_t)bt * a.max_blocks + lb0;
#else
    const int32_t *tab = a.table + b * a.max_blocks + lb0;
#endif
    for (int j = threadIdx.x; j < nlb; j += kBlock) blks[j] = tab[j];
    __syncthreads();
    const int32_t head_row0 = (int32_t)((a.layer * a.kv_heads + hk) * a.bs);
    const int32_t blk_rows = (int32_t)(a.layers * a.kv_heads * a.bs);
    const int npad = (int)a.split + (U - 1) * kBlock;
    for (int i = threadIdx.x; i < npad; i += kBlock) {
      int32_t row = -1;
#ifdef ATTN_BODY_WINDOW  // [window] a key between the sinks and the window is a -1 row, as a missing block's
      if (i < ntok && (t0 + i >= lo || t0 + i < (int64_t)a.sinks)) {
#else
      if (i < ntok) {
#endif
        const uint32_t pos = (uint32_t)(t0 + i);
        const uint32_t lb = pos / bs;
        const int32_t blk = blks[lb - lb0];
        if (blk >= 0) row = blk * blk_rows + head_row0 + (int32_t)(pos - lb * bs);
      }
      rows[i] = row;
    }
  }
  if (kSpread && (DEC & 2)) {
    __syncthreads();  // blks (aliased) fully read; the probe stages no tables
  } else if (kSpread && SP) {
    __syncthreads();  // blks (aliased) fully read
    // the correction half, then T0[k] = P(k) and T1[k] = P(k << 6)
    const u32x4 *src = reinterpret_cast<const u32x4 *>(a.atab_x + 4096);
    u32x4 *dst = reinterpret_cast<u32x4 *>(gtab);
#pragma unroll
    for (int i = threadIdx.x; i < 1024; i += kBlock) dst[i] = src[i];
    if (threadIdx.x < 128)
      gtab[4096 + threadIdx.x] = a.atab_x[threadIdx.x < 64 ? threadIdx.x : (threadIdx.x - 64) << 6];
  } else if (kSpread) {
    __syncthreads();  // blks (aliased) fully read
    const u32x4 *src = reinterpret_cast<const u32x4 *>(a.atab_x);
    u32x4 *dst = reinterpret_cast<u32x4 *>(gtab);
#pragma unroll
    for (int i = threadIdx.x; i < 2048; i += kBlock) dst[i] = src[i];
  } else if (is_golay(CODEC)) {
    const u32x4 *src0 = reinterpret_cast<const u32x4 *>(a.par);
    const u32x4 *src1 = reinterpret_cast<const u32x4 *>(a.cor);
    u32x4 *dst = reinterpret_cast<u32x4 *>(gtab);
    for (int i = threadIdx.x; i < 512; i += kBlock) {
      dst[i] = src0[i];
      dst[512 + i] = src1[i];
    }
  }
  if (CODEC == KVECC_CODEC_H84 && threadIdx.x < 256)  // (the byte family's kernels: their codec's table)
    lut[threadIdx.x] = (h84_lut_t)((int)byte_table_nibble(a, threadIdx.x) - 8);
  float qsum[G];  // sum of this lane's q (folds the decode's kOffset out of the K sums)
#pragma unroll
  for (int j = 0; j < G; ++j) {
    qsum[j] = 0.0f;
#pragma unroll
    for (int e = 0; e < E; ++e) qsum[j] += qv[j][e];
    if (C::kThird16) {  // decode's 16 n in slots 3k + 2 (after the sum: it folds n - 8)
#pragma unroll
      for (int e = 2; e < E; e += 3) qv[j][e] *= 0.0625f;
    }
  }
  __syncthreads();

  // buffer descriptors (BUF kernels; dead code otherwise)
  const __amdgpu_buffer_rsrc_t krs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.k_cache), 0, (int)a.cache_bytes, kRsrcWord3);
  const __amdgpu_buffer_rsrc_t vrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.v_cache), 0, (int)a.cache_bytes, kRsrcWord3);
  const __amdgpu_buffer_rsrc_t ksrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.k_scales), 0, (int)a.scale_bytes, kRsrcWord3);
  const __amdgpu_buffer_rsrc_t vsrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.v_scales), 0, (int)a.scale_bytes, kRsrcWord3);
  // ---- one pass: U K and V rows in flight per lane, online softmax per group
  // (and per query head j of the workgroup)
  float m[G], l[G], acc[G][E];
  float psum[G];  // sum of p * v_scale, for the kOffset fold of the V sums
#pragma unroll
  for (int j = 0; j < G; ++j) {
    m[j] = -INFINITY;
    l[j] = 0.0f;
    psum[j] = 0.0f;
#pragma unroll
    for (int e = 0; e < E; ++e) acc[j][e] = 0.0f;
  }
  // GQA workgroups (G > 1) do G times the arithmetic per row and have a
  // quarter of MHA's rows: they issue the next iteration's rows before using
  // this one's (MHA measured no gain from that in round 1)
  constexpr bool kPrefetch = G > 1 && CODEC == KVECC_CODEC_H84;
  C pkc[U], pvc[U];
  float pks[U], pvs[U];
  bool pok[U];
  auto load_rows = [&](int i0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {  // branch-free: invalid rows read row 0, masked
      const int32_t r = rows[i0 + u * TP];
      pok[u] = r >= 0;
      const int64_t row = pok[u] ? r : 0;
      if (BUF) {
        pkc[u].load_buf(a, krs, (int32_t)row, cs);
        pvc[u].load_buf(a, vrs, (int32_t)row, cs);
        pks[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ksrs, (uint32_t)row * 4u, 0, 0));
        pvs[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(vsrs, (uint32_t)row * 4u, 0, 0));
      } else {
        pkc[u].load(a, a.k_cache, row, cs);
        pvc[u].load(a, a.v_cache, row, cs);
        pks[u] = a.k_scales[row];
        pvs[u] = a.v_scales[row];
      }
    }
  };
#ifdef ATTN_BODY_WINDOW  // [window] the passes before the first visible key are skipped
  if (kPrefetch && i_first + grp < ntok) load_rows(i_first + grp);
  for (int i0 = i_first + grp; i0 < ntok; i0 += TP * U) {
#else
  if (kPrefetch && grp < ntok) load_rows(grp);
  for (int i0 = grp; i0 < ntok; i0 += TP * U) {
#endif
    if (!kPrefetch) load_rows(i0);
    C kc[U], vc[U];
    float ks[U], vs[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      kc[u] = pkc[u];
      vc[u] = pvc[u];
      ks[u] = pks[u];
      vs[u] = pvs[u];
      ok[u] = pok[u];
#ifdef ATTN_BODY_WINDOW  // [window] a -1 row stands in row 0 of the cache, which may be a released block's:
      // its weight p = 0 must not meet a V scale that is no number (0 * NaN)
      if (!ok[u]) vs[u] = 0.0f;
#endif
    }
    if (kPrefetch && i0 + TP * U < ntok) load_rows(i0 + TP * U);
#ifdef ATTN_BODY_STATS  // [statistics] the stored bytes of the lane's words, before any interpolation
    if (counts) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (live && ok[u]) {  // not the idle lanes' copy of lane 0, nor a -1 block's / a past row's row 0
          if constexpr (is_golay(CODEC)) {
            // the row's own codewords only: a lane's words past g - 1 are the next row's, the pad bytes' or 0
            uint32_t f = 0;  // the count fields of <= 2 VEC codewords (Chunk::count)
#pragma unroll
            for (int k = 0; k < VEC; ++k)
              if (VEC * c + k < a.g) f += kc[u].count(gtab, k) + vc[u].count(gtab, k);
            n_single += f & 0x3Fu;  // bits corrected
            n_double += f >> 6;     // uncorrectable words
          } else {
#ifdef ATTN_BODY_REPAIR  // [repair] count and store: the lane's words are whole words of its row (VEC divides the
            // row's words), at load_buf's offsets.  A lane whose words are all clean codewords does neither.
            uint32_t dirty = 0;
#pragma unroll
            for (int k = 0; k < VEC; ++k) dirty |= h_code4(kc[u].w[k]) | h_code4(vc[u].w[k]);
            if (dirty) {
              const uint32_t off = (uint32_t)rows[i0 + u * TP] * (uint32_t)a.d + 4u * VEC * c;
#pragma unroll
              for (int k = 0; k < VEC; ++k) {
                h84_repair_store(krs, off + 4u * k, kc[u].w[k], n_single, n_double, n_rewritten);
                h84_repair_store(vrs, off + 4u * k, vc[u].w[k], n_single, n_double, n_rewritten);
              }
            }
#else
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
              h84_count4(kc[u].w[k], n_single, n_double);
              h84_count4(vc[u].w[k], n_single, n_double);
            }
#endif
          }
        }
        ok[u] = ok[u] && i0 + u * TP < ntok_att;  // rows past the row's own key limit: counted, not attended
      }
    }
#endif
#if ATTN_BODY_CHUNK == 2  // [interpolation] paged_attn_split_interp_kernel only (kvecc.h "Interpolated attention")
    // First look: h84_double4 of the lane's words.  A lane whose K or V words of
    // a row hold a type-2 byte re-loads the same words of the rows at positions
    // max(l - 1, 0) and min(l + 1, n_b - 1) of its sequence -- through the block
    // table, a -1 block reading as zero codewords -- and replaces its words by
    // the interpolated, re-encoded ones (h84_interp_fix4).
    if (live) {
      const int64_t nb = min<int64_t>(a.ctx_lens[bt], a.ctx_cap);  // the sequence's length: the neighbours' clamp
      const int32_t head_row0 = (int32_t)((a.layer * a.kv_heads + hk) * a.bs);
      const int32_t blk_rows = (int32_t)(a.layers * a.kv_heads * a.bs);
      auto row_at = [&](int64_t p) {
        const uint32_t lb = (uint32_t)p / (uint32_t)a.bs;
        const int32_t blk = a.table[(int64_t)bt * a.max_blocks + lb];
        return blk < 0 ? -1 : blk * blk_rows + head_row0 + (int32_t)((uint32_t)p - lb * (uint32_t)a.bs);
      };
      auto word_at = [&](__amdgpu_buffer_rsrc_t rs, int32_t row, int k) {
        if (row < 0) return 0u;
        return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(
            rs, (uint32_t)row * (uint32_t)a.d + 4u * VEC * cs + 4u * k, 0, 0);
      };
#pragma unroll
      for (int u = 0; u < U; ++u) {
        uint32_t dbl = 0;
#pragma unroll
        for (int k = 0; k < VEC; ++k) dbl |= h84_double4(kc[u].w[k]) | h84_double4(vc[u].w[k]);
        if (dbl && ok[u]) {
          const int64_t pos = t0 + i0 + u * TP;  // < ntok + t0 <= n_b: ok[u]
          const int32_t rl = row_at(max<int64_t>(pos - 1, 0)), rr = row_at(min<int64_t>(pos + 1, nb - 1));
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            if (h84_double4(kc[u].w[k]))
              kc[u].w[k] = h84_interp_fix4(kc[u].w[k], word_at(krs, rl, k), word_at(krs, rr, k));
            if (h84_double4(vc[u].w[k]))
              vc[u].w[k] = h84_interp_fix4(vc[u].w[k], word_at(vrs, rl, k), word_at(vrs, rr, k));
          }
        }
      }
    }
#endif
    float sc[G][U];
    float mn[G];
#pragma unroll
    for (int j = 0; j < G; ++j) mn[j] = m[j];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float part[G];
#pragma unroll
      for (int j = 0; j < G; ++j) part[j] = 0.0f;
      if (live) {
        float kv[E];
        kc[u].template decode<DEC>(lut, gtab, kv);
#pragma unroll
        for (int j = 0; j < G; ++j) {
          part[j] = dot<E>(qv[j], kv);
          if (C::kOffset != 0.0f) part[j] -= C::kOffset * qsum[j];
          part[j] *= ks[u];  // sum q (n - 8) s = s * sum q (n - 8)
        }
      }
#pragma unroll
      for (int j = 0; j < G; ++j) {
        part[j] = group_sum<W>(part[j]);
        sc[j][u] = ok[u] ? part[j] : -INFINITY;
        mn[j] = fmaxf(mn[j], sc[j][u]);
      }
    }
    bool any = false;
#pragma unroll
    for (int j = 0; j < G; ++j) any |= mn[j] != -INFINITY;
    if (!any) continue;  // no valid row yet (uniform per group)
    float ps[G][U];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      if (G > 1 && mn[j] == -INFINITY) {  // this head has no finite score yet: no update
#pragma unroll
        for (int u = 0; u < U; ++u) ps[j][u] = 0.0f;
        continue;
      }
      const float alpha = attn_exp(m[j] - mn[j]);  // m = -inf -> 0
      l[j] *= alpha;
      psum[j] *= alpha;
#pragma unroll
      for (int e = 0; e < E; ++e) acc[j][e] *= alpha;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float p = attn_exp(sc[j][u] - mn[j]);  // invalid rows: exp(-inf) = 0
        l[j] += p;
        ps[j][u] = p * vs[u];
        psum[j] += ps[j][u];
      }
      m[j] = mn[j];
    }
    if (live) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float vv[E];
        vc[u].template decode<DEC>(lut, gtab, vv);
#pragma unroll
        for (int j = 0; j < G; ++j) axpy<E>(acc[j], ps[j][u], vv);
      }
    }
  }

  // ---- merge the TP groups (one query head at a time) ------------------------------
  if (kSpread) __syncthreads();  // the tables (aliased by red) fully read
  __shared__ float gw[TP];  // e^(m_g - M) per group
#pragma unroll
  for (int j = 0; j < G; ++j) {
    if (j > 0) __syncthreads();  // the previous head's merge fully read red / gml / gw
    if (live) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float ae = C::kThird16 && e % 3 == 2 ? acc[j][e] * 0.0625f : acc[j][e];  // 16 n slots
        red[(grp * W + c) * E + e] = C::kOffset != 0.0f ? ae - C::kOffset * psum[j] : ae;
      }
    }
    if (c == 0) {
      gml[0][grp] = m[j];
      gml[1][grp] = l[j];
    }
    __syncthreads();
    float M = -INFINITY;
    for (int gi = 0; gi < TP; ++gi) M = fmaxf(M, gml[0][gi]);
    if (threadIdx.x < TP) {
      const float mg = gml[0][threadIdx.x];
      gw[threadIdx.x] = mg == -INFINITY ? 0.0f : attn_exp(mg - M);
    }
    __syncthreads();
    float *ws = ws0 + j * ws_stride;
    for (int64_t di = threadIdx.x; di < a.d; di += kBlock) {
      float sum = 0.0f;
      for (int gi = 0; gi < TP; ++gi) sum += red[gi * W * E + di] * gw[gi];
      ws_put(ws + 2 + di, sum);
    }
    if (threadIdx.x == 0) {
      float L = 0.0f;
      for (int gi = 0; gi < TP; ++gi) L += gml[1][gi] * gw[gi];
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
  if (a.ctr) combine_if_last<T, G>(a, b * a.heads + h0, reinterpret_cast<float *>(rows));
