// Body of the packed INT4 matrix-core kernels (KVECC_CODEC_INT4_PACKED, kvecc.h: two nibbles per
// byte, rows of D / 2 bytes), included by attention.hip inside each kernel, which defines
// ATTN_BODY_CHUNK around the inclusion; it is no build switch.
//   ATTN_BODY_CHUNK 0  paged_attn_i4p_mfma_kernel: `a` a PackedAttnArgs, G query heads in the first G columns.
//   ATTN_BODY_CHUNK 1  paged_attn_i4p_mfma_chunk_kernel: `a` a PackedUniformArgs, G = 16 (token, head)
//     columns (ChunkMap); paged_attn_i4p_mfma_ragged_kernel is the same text over a PackedChunkArgs
//     and its ChunkMap.
// The operand maps are attn_h84_mfma_body.inc's with half the bytes (D 64 or 128):
//   * K: lane (token n, group g) owns the quarter row d = (D/4)g .. (D/4)g + D/4 - 1 of its token,
//     now D / 8 bytes at byte (D/8)g -- one 16-byte load at D 128 where the byte kernels issue two.
//     Dword kk of it holds the eight values of QK MFMA kk, value j in bits 4j .. 4j + 3, so the
//     Q operand's k -> d map is unchanged.
//   * V: lane n owns D / 16 values of each of its 8 tokens, D / 32 bytes at byte (D/32)n; M-tile mt
//     takes nibble mt of each, so output row m of tile mt is d = (D/16)m + mt as before.
// No decode table: a loaded word w splits into its even nibbles w & 0x0F0F0F0F and its odd nibbles
// (w >> 4) & 0x0F0F0F0F, one per byte, and an operand pair is one v_perm of two such bytes into the
// f16 subnormals n * 2^-24 of the byte kernels (kMfmaValScale; the - 8 folded out by qoff / poff).
// Per K word: 3 VALU + 4 v_perm for 8 values, against 8 LDS lookups + 4 v_perm; no lut[256], no
// staging of it, and nothing in LDS that the loop reads but rows[].
// A masked row (no block, past the split) stands in row 0 of the cache, which the call may not own:
// its weight 0 must not meet a V scale that is no number, so load_step zeroes the scale of such a row.
// Shared with the other bodies, one copy each: attn_mfma_columns.inc, attn_mfma_rows.inc,
// attn_mfma_descriptors.inc, attn_mfma_softmax.inc, attn_mfma_merge.inc.
  static_assert(D == 64 || D == 128, "the packed INT4 matrix-core kernels serve head_dim 64 and 128");
  constexpr int KK = D / 32;  // QK MFMAs per 16-token tile; K dwords per lane per token
  constexpr int MT = D / 16;  // PV M-tiles; V values per lane per token
  constexpr int KB = D / 8;   // K bytes per lane per token
  constexpr int VB = D / 32;  // V bytes per lane per token (2 or 4: one load)
  constexpr uint32_t kRowBytes = D / 2;
  constexpr int kWaves = kBlock / kWave;
  constexpr int kHalo = 0;
  __shared__ __attribute__((aligned(16))) int32_t rows[kMaxSplit + kMfmaStep];
  __shared__ int32_t blks[kMaxSplit + 1];
  __shared__ float red[kWaves][G][D];
  __shared__ float gml[2][kWaves][G];

#include "attn_mfma_columns.inc"
  // Q^T operand (B): column n = head h0 + n, k-slot 8g + j of MFMA kk = d (D/4)g + 8kk + j.
  // Issued first: it lands during the block-table round trip
  f16x8 qop[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) {
    u32x4 v = {0u, 0u, 0u, 0u};
#if ATTN_BODY_CHUNK  // [query load] the column's (token, head) row through the strides
    if (cm.col_ok) v = *reinterpret_cast<const u32x4 *>(cm.q_row(a) + (D / 4) * g + 8 * kk);
#else
    if (n < G)
      v = *reinterpret_cast<const u32x4 *>(reinterpret_cast<const __half *>(a.q) +
                                           (b * a.heads + h0 + n) * D + (D / 4) * g + 8 * kk);
#endif
    qop[kk] = __builtin_bit_cast(f16x8, v);
  }
#include "attn_mfma_rows.inc"
#include "attn_mfma_descriptors.inc"
  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  float m = -INFINITY, l = 0.0f;
  float psum = 0.0f;  // sum of p * v_scale over this lane's tokens (the offset fold)
  float pvc = 0.0f;   // the PV normaliser ([normaliser]); 0: nothing accumulated yet
  const float qoff = kMfmaValOffset * qsum;

  // one step's operands in registers: 2 K rows (tokens i0 + n, i0 + 16 + n), 8 V rows and scales
  // (tokens i0 + 16(j >> 2) + 4g + (j & 3)) -- 2 KK + 8 data dwords where the byte kernels hold
  // 4 KK + 2 MT; invalid rows read row 0 and are masked
  struct Step {
    int32_t rv[8];
    uint32_t kw[2][KK];
    uint32_t vw[8];
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
      load_chunk<KB>(krs, (uint32_t)max(r, 0) * kRowBytes + (uint32_t)(KB * g), st.kw[tau]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t r = (uint32_t)max(st.rv[j], 0);
      load_chunk<VB>(vrs, r * kRowBytes + (uint32_t)(VB * n), &st.vw[j]);
      st.ks[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ksrs, r * 4u, 0, 0));
      const float vsj = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(vsrs, r * 4u, 0, 0));
      st.vs[j] = st.rv[j] >= 0 ? vsj : 0.0f;
    }
  };
  // bytes h of two nibble-per-byte words -> f16 operand pair [0, hi.h, 0, lo.h]
  auto pair_at = [](uint32_t lo, uint32_t hi, int h) {
    return __builtin_amdgcn_perm(hi, lo, 0x0c000c00u | (uint32_t)(4 + h) << 16 | (uint32_t)h);
  };
  constexpr int kStride = kWaves * kMfmaStep;
  for (int i0 = wave * kMfmaStep; i0 < ntok; i0 += kStride) {
    Step cur;
    load_step(i0, cur);
    const int32_t *rv = cur.rv;
    const float *ks = cur.ks, *vs = cur.vs;
    // ---- S^T = K . Q^T, two 16-token tiles
    f32x4 S[2];
#pragma unroll
    for (int tau = 0; tau < 2; ++tau) {
      S[tau] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const uint32_t w = cur.kw[tau][kk];
        const uint32_t ev = w & 0x0F0F0F0Fu, od = (w >> 4) & 0x0F0F0F0Fu;  // values 2h / 2h + 1 in byte h
        const u32x4 p = {pair_at(ev, od, 0), pair_at(ev, od, 1), pair_at(ev, od, 2), pair_at(ev, od, 3)};
        S[tau] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, p), qop[kk], S[tau], 0, 0, 0);
      }
    }
    // ---- online softmax over this lane's 8 tokens of head n
#include "attn_mfma_softmax.inc"
    // ---- O^T += V^T . P: M-tile mt takes nibble mt of each token's chunk -- byte mt / 2 of the
    // token's even (mt even) or odd nibbles
    uint32_t vev[8], vod[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      vev[j] = cur.vw[j] & 0x0F0F0F0Fu;
      vod[j] = (cur.vw[j] >> 4) & 0x0F0F0F0Fu;
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      uint32_t p[4];
#pragma unroll
      for (int h = 0; h < 4; ++h)  // tokens j = 2h, 2h + 1
        p[h] = (mt & 1) ? pair_at(vod[2 * h], vod[2 * h + 1], mt / 2) : pair_at(vev[2 * h], vev[2 * h + 1], mt / 2);
      const f16x8 va = __builtin_bit_cast(f16x8, u32x4{p[0], p[1], p[2], p[3]});
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pb_hi, acc[mt], 0, 0, 0);
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pb_lo, acc[mt], 0, 0, 0);
    }
  }

  // ---- merge: the 4 lanes of a head, then the workgroup's waves
#include "attn_mfma_merge.inc"
#if !ATTN_BODY_CHUNK  // the counted combine: decode kernels only (chunk calls always launch the combine)
  if (a.ctr) combine_if_last<__half, G>(a, b * a.heads + h0, reinterpret_cast<float *>(rows));
#endif
