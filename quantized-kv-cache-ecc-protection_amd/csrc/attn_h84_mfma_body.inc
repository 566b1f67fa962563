// Body of the Hamming(8,4) matrix-core kernels, included by attention.hip inside each kernel, which
// defines ATTN_BODY_CHUNK (and the island switches below) around the inclusion; they are no build
// switches.  A kernel's code follows from its preprocessed text alone, so a form whose text an edit
// leaves alone keeps its code (see ChunkArgs).
//   ATTN_BODY_CHUNK 0  paged_attn_h84_mfma_kernel: `a` an AttnArgs, G query heads in the first G columns.
//   ATTN_BODY_CHUNK 1  paged_attn_h84_mfma_chunk_kernel: `a` a ChunkArgs, G = 16 (token, head) columns
//     (ChunkMap); the ragged entry's paged_attn_h84_mfma_ragged_kernel is the same text over a
//     RaggedArgs and its ChunkMap.  The byte family's three kernels (paged_attn_byte_mfma_*) are
//     forms 0 and 1 over their argument blocks: only the decode table differs.
//   ATTN_BODY_CHUNK 2  paged_attn_h84_mfma_interp_kernel: `a` an InterpArgs, the ragged form with the
//     [interpolation] islands (kvecc.h "Interpolated attention"), as attn_split_body.inc has them:
//     * rows[] gains a halo: rows[kHalo + i] is R(i), the cache row of position t0 + i of the
//       sequence for i in [-1, npad] (attn_mfma_rows.inc); kHalo is 0 in the other forms.
//     * the first look: h84_double4 of every loaded dword (the syndrome / parity SWAR of the
//       scrubber's h84_dirty4 and four more operations) marks its type-2 bytes.  A lane none of
//       whose words of a K row (of four V rows) holds one goes on as the chunk kernel does.
//     * the slow path, per lane and per operand: the same bytes of rows l - 1 and l + 1 (clamped to
//       [0, n_b - 1]; a -1 block reads as zero codewords) come through the same buffer descriptor,
//       every byte is decoded, doubles become interp_word(q, L, R, type), and the word is
//       re-encoded (h84_interp_fix4) -- so the corrected nibbles reach nib_pair_f16 through the
//       same table as every other byte.  The neighbour loads of one K row (of four V rows) are
//       issued together, one round trip; only the words that hold a double are rewritten.
// ATTN_BODY_STATS (paged_attn_h84_mfma_stats_kernel, `a` a StatsArgs; _stats_interp_kernel, a
// StatsInterpArgs): the [statistics] islands, which count the words of load_step -- every stored
// byte once -- and never the neighbour words of the slow path.
// ATTN_BODY_REPAIR as well (paged_attn_h84_mfma_repair_kernel, a RepairArgs; _repair_interp_kernel, a
// RepairInterpArgs): the [repair] islands, in which the counting workgroup stores the corrected
// codewords back where it counts them (kvecc.h "Repairing attention"), before the slow path
// rewrites any in registers -- a double is never stored, and the neighbour words the slow path
// loads decode to the same nibbles before and after any store.
// ATTN_BODY_WINDOW (paged_attn_h84_mfma_window_kernel, `a` a WindowArgs, the ragged form over a
// WindowMap): the [window] islands of the shared fragments -- the column's lower key bound and sink
// bound at [score mask], the rows no column sees left unstaged, an empty split's early exit -- and
// the loop's first round here.  Its decode table is Hamming(8,4)'s, Hamming(7,4)'s or INT4's (WindowArgs::tab).
// Shared with attn_golay_mfma_body.inc, one copy each: attn_mfma_columns.inc, attn_mfma_rows.inc,
// attn_mfma_descriptors.inc, attn_mfma_softmax.inc, attn_mfma_merge.inc (their headers say what they read
// and define).
  constexpr int KK = D / 32;  // QK MFMAs per 16-token tile
  constexpr int MT = D / 16;  // PV M-tiles; V bytes per lane per token
  constexpr int KB = D / 4;   // K bytes per lane per token
  constexpr int VW = MT >= 4 ? MT / 4 : 1;  // V dwords per token
  constexpr int kWaves = kBlock / kWave;
#if ATTN_BODY_CHUNK == 2  // [interpolation] the halo: 4 keeps the 16-byte reads of load_step aligned
  constexpr int kHalo = 4;
  constexpr uint32_t kVMask = MT >= 4 ? 0xFFFFFFFFu : (1u << (8 * MT)) - 1u;  // the bytes a V load fills
  __shared__ __attribute__((aligned(16))) int32_t rows[kHalo + kMaxSplit + kMfmaStep + 4];
  __shared__ int32_t blks[kMaxSplit + 3];
#else
  constexpr int kHalo = 0;
  __shared__ __attribute__((aligned(16))) int32_t rows[kMaxSplit + kMfmaStep];
  __shared__ int32_t blks[kMaxSplit + 1];
#endif
  __shared__ uint8_t lut[256];
  __shared__ float red[kWaves][G][D];
  __shared__ float gml[2][kWaves][G];

#include "attn_mfma_columns.inc"
#ifdef ATTN_BODY_STATS  // [statistics] this lane's counters
  uint32_t n_single = 0, n_double = 0;
#ifdef ATTN_BODY_REPAIR  // [repair] bytes rewritten: the statistics buffer's word 2
  uint32_t n_rewritten = 0;
#endif
#endif
#if ATTN_BODY_CHUNK == 2  // [interpolation] the sequence's length n_b: what neighbours clamp to
  // (shim_read's ctx for this sequence alone)
  const int64_t nb = max<int64_t>(min<int64_t>(a.ctx_lens[b], a.ctx_cap), 0);
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
#include "attn_mfma_rows.inc"
  // kBlock == 256: one table entry per thread (the byte family's kernels: their codec's table)
  lut[threadIdx.x] = (uint8_t)byte_table_nibble(a, threadIdx.x);
#include "attn_mfma_descriptors.inc"
  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  float m = -INFINITY, l = 0.0f;
  float psum = 0.0f;  // sum of p * v_scale over this lane's tokens (the offset fold)
  float pvc = 0.0f;   // the PV normaliser ([normaliser]); 0: nothing accumulated yet
  const float qoff = kMfmaValOffset * qsum;

#if ATTN_BODY_CHUNK == 2  // [interpolation] the cache rows of token i's neighbours, positions
  // max(l - 1, 0) and min(l + 1, n_b - 1)
  auto left_of = [&](int i) { return rows[kHalo + (t0 + i > 0 ? i - 1 : i)]; };
  auto right_of = [&](int i) { return rows[kHalo + (t0 + i + 1 < nb ? i + 1 : i)]; };
#endif
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
#ifdef ATTN_BODY_WINDOW  // [window] the rounds before the first visible key are skipped (i_first: a multiple of kStride)
  for (int i0 = i_first + wave * kMfmaStep; i0 < ntok; i0 += kStride) {
#else
  for (int i0 = wave * kMfmaStep; i0 < ntok; i0 += kStride) {
#endif
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
        const int32_t r = rows[kHalo + i0 + 16 * tau + n];
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
        if (rows[kHalo + i0 + 16 * tau + n] >= 0) {  // not a -1 block's / a past row's row 0
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
#if ATTN_BODY_CHUNK == 2  // [interpolation] the first look, then the slow path in the lanes that hold a double,
    // after the islands above have seen the stored words.  One K row, or four V rows, at
    // a time: their neighbour words are what the slow path keeps in registers, and
    // with all ten rows' at once the kernel took 225-256 VGPRs (2 waves per SIMD) for 140
#pragma unroll
    for (int tau = 0; tau < 2; ++tau) {
      uint32_t kd = 0;
#pragma unroll
      for (int k = 0; k < KB / 4; ++k) kd |= h84_double4(kw[tau][k]);
      if (kd) {
        uint32_t wl[KB / 4], wr[KB / 4];
        const int i = i0 + 16 * tau + n;
        const int32_t rl = left_of(i), rr = right_of(i);
        load_chunk<KB>(krs, (uint32_t)max(rl, 0) * (uint32_t)D + (uint32_t)(KB * g), wl);
        load_chunk<KB>(krs, (uint32_t)max(rr, 0) * (uint32_t)D + (uint32_t)(KB * g), wr);
#pragma unroll
        for (int k = 0; k < KB / 4; ++k)
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
#include "attn_mfma_softmax.inc"
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
#include "attn_mfma_merge.inc"
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
