// Body of the Golay(24,12) matrix-core kernels (head_dim 128), included by attention.hip inside each
// kernel, which defines ATTN_BODY_CHUNK (and ATTN_BODY_STATS) around the inclusion; they are no build
// switches.  A kernel's code follows from its preprocessed text alone (see ChunkArgs).
//   ATTN_BODY_CHUNK 0  paged_attn_golay_mfma_kernel: `a` an AttnArgs, G query heads in the first G columns.
//   ATTN_BODY_CHUNK 1  paged_attn_golay_mfma_chunk_kernel: `a` a ChunkArgs, G = 16 (token, head) columns
//     (ChunkMap); the ragged entry's paged_attn_golay_mfma_ragged_kernel is the same text over a
//     RaggedArgs and its ChunkMap.
// ATTN_BODY_STATS (paged_attn_golay_mfma_stats_kernel, `a` a StatsArgs, the ragged form): the
// [statistics] islands.
// ATTN_BODY_WINDOW (paged_attn_golay_mfma_window_kernel, `a` a WindowArgs, the ragged form over a
// WindowMap): the [window] islands of the shared fragments, and the loop's first round here.
// What is Golay's own stands here: the operand maps, the loads and the decode through the spread
// tables.  Columns, row staging, buffer descriptors, the softmax step and the merge are the
// Hamming(8,4) body's, one copy each: attn_mfma_columns.inc, attn_mfma_rows.inc,
// attn_mfma_descriptors.inc, attn_mfma_softmax.inc, attn_mfma_merge.inc (their headers say what they
// read and define).
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

#include "attn_mfma_columns.inc"
#ifdef ATTN_BODY_STATS  // [statistics] this lane's counters
  uint32_t n_bits = 0, n_unc = 0;  // bits corrected (counts 1..3), uncorrectable words (count 4)
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
#define ATTN_ROWS_SPREAD_TABLES 1  // gt[] is staged under the slice's barrier
#include "attn_mfma_rows.inc"
#undef ATTN_ROWS_SPREAD_TABLES

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

#include "attn_mfma_descriptors.inc"
  const float qoff = kMfmaValOffset * qsum;
  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  float m = -INFINITY, l = 0.0f;
  float psum = 0.0f;  // sum of p * v_scale over this lane's tokens (the offset fold)
  float pvc = 0.0f;   // the PV normaliser ([normaliser]); 0: nothing accumulated yet

#ifdef ATTN_BODY_WINDOW  // [window] the rounds before the first visible key are skipped (i_first: whole rounds)
  for (int i0 = i_first + wave * kMfmaStep; i0 < ntok; i0 += kWaves * kMfmaStep) {
#else
  for (int i0 = wave * kMfmaStep; i0 < ntok; i0 += kWaves * kMfmaStep) {
#endif
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
#include "attn_mfma_softmax.inc"
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

  // ---- merge
#include "attn_mfma_merge.inc"
#ifdef ATTN_BODY_STATS  // [statistics] one reduction and at most two atomics per counting workgroup
  if (counts) {
    const uint32_t cnt[2] = {n_bits, n_unc};
    flush_stats_n<2>(a.stats, cnt);
  }
#endif
#if !ATTN_BODY_CHUNK  // the counted combine: decode kernels only (chunk calls always launch the combine)
  if (a.ctr) combine_if_last<__half, G>(a, b * a.heads + h0, reinterpret_cast<float *>(rows));
#endif
