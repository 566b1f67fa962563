// attention.hip -- paged attention over an ECC-protected INT4 KV cache, decoding
// the codewords inline: kvecc_paged_attention (one query token per sequence,
// the decode step) and kvecc_paged_attention_chunk (q_len tokens per sequence,
// causal: a prefill, a chunk, a verify step's draft tokens; no reference
// counterpart), and kvecc_paged_attention_interp (the chunk form over a
// Hamming(8,4) cache with detected double errors interpolated from the
// neighbouring tokens, in kernels of its own).  Hamming(7,4) and unprotected INT4
// caches (no reference counterpart) run a sibling family of the Hamming(8,4)
// kernels with another decode table (ByteAttnArgs).  The chunked entry runs the same kernel bodies (attn_*_body.inc)
// under kernel names of its own: the matrix-core kernels with 16 (token, head)
// columns per workgroup and a per-column key limit (ChunkMap), the split
// kernels over a virtual batch of batch * q_len rows (ChunkArgs).
//
// Reference: kv_cache/attention_ecc.py:265-427 (paged_attention_ecc_kernel,
// Hamming(8,4) with decode_hamming84_inline :56-149 -- double errors keep their
// uncorrected data -- and dequantize_int4 :152-169) and the wrapper
// paged_attention_ecc :620-780, which the shim calls for seq_len == 1
// (ecc_shim.py:791-800,1091-1136).  Golay(24,12) goes through the Python
// reference_attention_ecc there (:783-909); here it is a native kernel too.
//
// The reference runs one program per (batch, head) walking every context token
// with an online softmax -- B*H programs, a few dozen on a 256-CU part.  This
// is split-context ("flash-decoding"): workgroup (split, b*H + h) owns up to
// 256 tokens (fewer when batch*heads is small, so the grid still fills the
// chip), with the split's slice of the block table staged in LDS.  Lanes are
// grouped W per token row (a lane owns 16 H(8,4) codewords via one 16-byte
// load, or 3 Golay codewords); each group streams its rows in ONE pass --
// kUnroll K and V rows loaded before any is used, the group's partial dot
// products reduced with __shfl_xor, an online softmax per group -- and the
// groups merge through LDS.  The split's (max, sum, acc[D]) go to a workspace
// that a second small launch combines.  Query head h reads cache head
// h / (H / Hkv) (the reference indexes cache head h, which only agrees without
// GQA).  Numerics: fp32 throughout, softmax as exp2 of log2(e)-scaled scores
// (one v_exp_f32 per exponential).  The result differs from the
// reference's sequential online softmax by fp32 summation order and, for Golay,
// by the -8 fold: the kernel sums q*n and p*s*n over the raw nibbles and
// subtracts 8*sum(q) / 8*sum(p*s) once per split (acc - 8*psum), which loses a
// few bits when the values are small against 8*scale (bounded by the
// long-context test in tests/test_attention.py).  A context with no valid
// token (context_len <= 0, or only -1 blocks) gives the reference's values:
// Hamming(8,4) -8.0 in every lane (its kernel scores invalid tokens -1e20, the
// same as its initial max, so each accumulates weight 1 on the masked row
// decode(0) - 8 = -8, attention_ecc.py:342,391-423), Golay 0
// (reference_attention_ecc's torch.zeros, :806-807,885-886).
#include <type_traits>

#include "kvecc_internal.h"

namespace kvecc {

constexpr int kMaxSplit = 1024;   // context tokens per workgroup (upper bound)
constexpr int kMaxSplits = 1024;  // splits per (batch, head)
constexpr int kAttnMaxD = 256;
// Tuned constants (A/B history: DESIGN.md §3 "Paged decode attention";
// tools/exp/run_attn.py and the experiment forks under tools/exp).
// token rows in flight per lane group: packed Golay 4; int32 Golay 2 (72.8 vs
// 80.0 us at 4); Hamming(8,4) 2 (56.9 / 57.1 us vs 60.3 / 60.0 at 4, random /
// encoded caches); every codec loses with 8
constexpr int kUnroll = 4, kGolayUnroll = 2, kH84Unroll = 2;
constexpr int kMaxUnroll = 4;
// codeword words per lane of a token row: H(8,4) 4 (16 codewords, one 16-byte
// load; 8 and 32 per lane measured 57.6 and 65.0 us vs 56.9); Golay 3
// codewords (43 -> 15 of 16 lanes busy; 6 per lane 114.0 vs 104.3 us)
constexpr int kH84Vec = 4, kGolayVec = 3;
// Cache rows go through raw buffer loads with 32-bit offsets when the caches
// and scales are < 4 GiB (the BUF kernels): no 64-bit address arithmetic per
// load, and reads past the row's last codeword need no clamp (inside the
// buffer they read a neighbour row's words, which contribute nothing; past it
// the hardware returns 0).  Golay 105.7 -> 82.1 us at [8,4096,32,128], H84
// unchanged (tools/exp/run_attn.py).  Larger caches take 64-bit addressing.
constexpr uint32_t kRsrcWord3 = 0x00020000u;  // gfx9 raw buffer: 32-bit data format
// Packed Golay caches (KVECC_CODEC_GOLAY_PACKED, 3-byte codewords): a lane owns
// 3 codewords = 9 bytes of its token row, loaded as the 3 aligned dwords that
// hold them and realigned (v_alignbyte): 43 codewords -> 15 of 16 lanes busy.
// 4 codewords per lane (12 bytes, 3 aligned dwords, no realignment) left 5 of
// 16 lanes idle: 68.0 vs 62.8 us per MHA call (profiles/r04/attn/packed_vec_ab.log)
constexpr int kGolayPackedVec = 3;
// Golay decodes through the spread tables (golay_attn_x_table_dev: 32-bit
// entries, nibbles one per byte, parity at the codeword's parity bits): per
// codeword 2 LDS reads + 7 VALU ops (the first table's address, one masked xor
// and a shift for the second's, one masked xor, three v_cvt_f32_ubyteN)
// instead of ~13 through the 16-bit tables.  With the parity at bits 20-31
// (golay_attn_table_dev, the shim's layout) the second address took 3 ops:
// packed MHA main loop 393 -> 357 VALU per 4-row iteration.  Hamming(8,4) decodes through a 256-entry LDS table of data(b) - 8
// as int8 (ds_read_i8 + v_cvt_f32_i32; the 256 bytes are 64 dwords over 32
// banks, so random lookups conflict at most 2-way, where an fp32 table's 256
// dwords conflict ~3.5-way: 60.6 vs 63.5 us per call on random caches).
typedef int8_t h84_lut_t;
// Softmax in base 2: the query is pre-scaled by sm_scale * log2(e), so every
// exponential is one v_exp_f32 (exp2) instead of expf's ~10-instruction range
// reduction (Golay 76.0 -> 72.4 us); the split maxima in the workspace are in
// the same log2 units
__device__ __forceinline__ float attn_exp(float x) { return __builtin_amdgcn_exp2f(x); }  // exp2(-inf) = 0
constexpr float kAttnLogScale = 1.4426950408889634f;  // log2(e)
constexpr bool is_golay(int codec) { return codec == KVECC_CODEC_GOLAY || codec == KVECC_CODEC_GOLAY_PACKED; }

struct AttnArgs {
  const void *q;  // [B, H, D]
  const void *k_cache, *v_cache;
  const int32_t *table;     // [B, max_blocks]
  const int32_t *ctx_lens;  // [B]
  const float *k_scales, *v_scales;
  float *ws;  // [B*H, nsplit, D + 2]: m, l, acc[D]
  void *out;  // [B, H, D]
  int64_t heads, kv_heads, d, g;  // g = codewords per token row
  uint32_t rowb;                  // packed Golay: bytes per token row (KVECC_GOLAY_PACKED_ROW(g))
  int64_t layers, layer, bs, max_blocks, nsplit, split;
  int64_t ctx_cap;  // min(max_context_len, max_blocks * bs): context_lens above it are attended up to it
  uint32_t cache_bytes, scale_bytes;  // buffer-load bounds (BUF kernels)
  float sm_scale;
  float empty_value;          // output when a (b, h) has no valid token
  const uint16_t *par, *cor;  // Golay tables
  const uint32_t *atab;       // Golay spread tables (golay_attn_table_dev): MFMA kernels
  const uint32_t *atab_x;     // the split kernels' layout (golay_attn_x_table_dev)
  uint32_t *ctr;              // per-(batch, head group) split counters (attn_counter_slot), or
                              // null: a separate combine launch
};

// Chunked causal calls (kvecc_paged_attention_chunk) add their fields behind
// AttnArgs and run kernels of their own names over the same bodies: the decode
// kernels keep their argument block byte for byte (a longer one changed their
// register allocation: 122 -> 134 VGPRs for the Hamming(8,4) matrix-core
// kernel at head_dim 128, with no field of it read).  The split kernels see a
// virtual batch of batch * q_len rows: row b' reads block-table row b' / q_len
// and the keys before min(ctx_lens[b' / q_len] - q_len + 1 + b' % q_len, ctx_cap).
struct ChunkArgs : AttnArgs {
  uint32_t q_len;            // query tokens per sequence
  uint32_t vb0;              // first virtual batch row of this launch (grids of > 65535 rows are sliced)
  uint32_t cg_log2;          // matrix-core chunk kernels: log2 of the query heads per column group
  int64_t q_sb, q_st, q_sh;  // query strides in elements: batch, token, head
};
// Ragged calls (kvecc_paged_attention_chunk_ragged) add the spans behind
// ChunkArgs, for the same reason: the uniform matrix-core chunk kernels keep
// ChunkArgs and their code (with the field in ChunkArgs and the span rule in
// their ChunkMap they measured 0.7-1.4 us slower per uniform call at
// [8,4096,*,128], q_len 16, at unchanged registers and LDS:
// profiles/ragged_attention), and the ragged entry runs matrix-core kernels of
// its own names over the same bodies.  The split chunk kernels take RaggedArgs
// for both entries.
struct RaggedArgs : ChunkArgs {
  // [batch, 3] (first, count, row_base) per sequence, q_len the rectangle's
  // q_max; null: the uniform call, first = 0 and count = q_len
  const int32_t *q_spans;
};
// A sequence's span: token t is valid iff first >= 0 and first <= t < min(first
// + count, q_len), and sits at position ctx_lens[b] - count + (t - first).
struct ChunkSpan {
  int64_t first, count;
  __device__ __forceinline__ ChunkSpan(const RaggedArgs &a, int64_t b) {
    first = a.q_spans ? a.q_spans[3 * b] : 0;
    count = a.q_spans ? a.q_spans[3 * b + 1] : a.q_len;
  }
  // [v0, v1): the valid tokens, empty when v1 <= v0
  __device__ __forceinline__ int64_t v0() const { return first; }
  __device__ __forceinline__ int64_t v1(const ChunkArgs &a) const {
    return first < 0 ? first : min<int64_t>(first + count, a.q_len);
  }
  __device__ __forceinline__ bool valid(const ChunkArgs &a, int64_t t) const { return t >= first && t < v1(a); }
  // token 0's key limit; token t's is that + t
  __device__ __forceinline__ int64_t lim0(const ChunkArgs &a, int64_t b) const {
    return (int64_t)a.ctx_lens[b] - count + 1 - first;
  }
};
template <typename A>
constexpr bool is_chunk = std::is_base_of<ChunkArgs, A>::value;

// Interpolating calls (kvecc_paged_attention_interp, Hamming(8,4) only) run
// kernels of their own names over an argument block of their own type: every
// other kernel keeps its text, its arguments and its registers.  The block
// adds nothing to RaggedArgs yet -- the neighbour rule needs only the sequence's
// length, which context_lens and ctx_cap give.
struct InterpArgs : RaggedArgs {};
template <typename A>
constexpr bool is_interp = std::is_same<A, InterpArgs>::value;

// Counted calls (kvecc_paged_attention_stats, Hamming(8,4) only) run kernels of
// their own names over argument blocks of their own: the ragged and the
// interpolating block plus the library's sharded statistics buffer.  Every other
// kernel keeps its block, its text and its registers.  The Golay counted kernels
// (kvecc_paged_attention_golay_stats) are further kernels of their own names over
// StatsArgs: the uncounted Golay kernels never see it.
struct StatsArgs : RaggedArgs {
  // KVECC_STATS_SLOTS x KVECC_STATS_STRIDE: [0] += SINGLE_CORRECTED, [1] += DOUBLE_DETECTED
  // (Golay: [0] += bits corrected, [1] += uncorrectable words)
  uint64_t *stats;
};
struct StatsInterpArgs : InterpArgs {
  uint64_t *stats;
};
template <typename A>
constexpr bool is_stats = std::is_same<A, StatsArgs>::value || std::is_same<A, StatsInterpArgs>::value;

// Repairing calls (kvecc_paged_attention_repair, Hamming(8,4) only) run further
// kernels of their own names: the counted kernels' text plus the [repair]
// islands, in which the counting workgroup stores the corrected codewords back
// through the cache descriptors (kvecc.h "Repairing attention").  Their blocks
// add nothing to the counted ones -- stats word 2 takes the rewritten bytes -- and
// are types of their own so that the counted kernels keep their names, their
// text and their registers.
struct RepairArgs : StatsArgs {};
struct RepairInterpArgs : StatsInterpArgs {};
template <typename A>
constexpr bool is_repair = std::is_same<A, RepairArgs>::value || std::is_same<A, RepairInterpArgs>::value;

// Byte caches without SECDED (KVECC_CODEC_H74, KVECC_CODEC_NONE: Hamming(8,4)'s
// layout, uint8, one value per byte, rows of head_dim bytes) run one sibling
// family of kernels, of their own names, over the Hamming(8,4) bodies: every
// H(8,4) kernel decodes through a 256-entry table that its workgroup fills, so
// the codec is the table.  The family's argument blocks add the table selector
// behind AttnArgs / RaggedArgs -- every other kernel keeps its block, its text
// and its registers -- and the selector is read once per workgroup, where the
// table is staged (byte_table_nibble: a uniform branch outside every loop).
// One family instead of a CODEC template value per codec: one new instantiation
// set, not two, and an instruction stream per shape that is Hamming(8,4)'s.
struct ByteAttnArgs : AttnArgs {
  uint32_t tab;  // KVECC_CODEC_H74 or KVECC_CODEC_NONE
};
struct ByteChunkArgs : RaggedArgs {
  uint32_t tab;
};
// The uniform matrix-core chunk kernels' block: the selector behind ChunkArgs, not
// behind RaggedArgs, for the reason Hamming(8,4)'s uniform kernels keep ChunkArgs
// (see RaggedArgs; profiles/byte_attention has this family's measurement).
struct ByteUniformArgs : ChunkArgs {
  uint32_t tab;
};
template <typename A>
constexpr bool is_byte = std::is_same<A, ByteAttnArgs>::value || std::is_same<A, ByteChunkArgs>::value ||
                         std::is_same<A, ByteUniformArgs>::value;

// Windowed calls (kvecc_paged_attention_window, kvecc.h "Windowed attention") run
// kernels of their own names over an argument block of their own type: every other
// kernel keeps its block, its text and its registers.  A query row at position p
// sees key j < its key limit iff j < sinks or j >= lo = max(p - window + 1, 0).
// One byte family serves Hamming(8,4), Hamming(7,4) and unprotected INT4: `tab`
// selects the decode table as ByteChunkArgs::tab does, KVECC_CODEC_H84 a third value.
//
// The grid follows the window, not the context.  Split index i < sink_splits covers the keys
// [i * split, (i + 1) * split): the sink keys, and whatever else its rows see there.  The
// later indices cover nsplit - sink_splits consecutive splits that START AT THE WORKGROUP'S OWN
// WINDOW: at split max(lo / split, sink_splits), lo the row's (the tile's smallest) lower bound,
// which the workgroup reads from context_lens -- the host promises nothing.  The launcher sizes
// nsplit so that those splits reach past the row's (the tile's last) position (paged_attention_chunk_impl), so
// grid, workspace traffic and combine width scale with sinks + window + q_max.  sink_splits ==
// nsplit is the dense plan: split i at i * split, the whole context.
struct WindowArgs : RaggedArgs {
  uint32_t window, sinks;  // window >= 1; both clamped to INT32_MAX by the entry
  uint32_t tab;            // KVECC_CODEC_H84, KVECC_CODEC_H74 or KVECC_CODEC_NONE (Golay kernels: unused)
  uint32_t sink_splits;    // the leading split indices that sit at their own place
  // first key of split index i of a workgroup whose lower key bound is lo
  __device__ __forceinline__ int64_t split_start(uint32_t i, int64_t lo) const {
    if (i < sink_splits) return (int64_t)i * split;
    return (max<int64_t>(lo / split, sink_splits) + (i - sink_splits)) * split;
  }
};
template <typename A>
constexpr bool is_window = std::is_same<A, WindowArgs>::value;

// Entry b of a workgroup's decode table, as a nibble: data(b) of kvecc.h's
// attention contract.  Hamming(8,4): single errors corrected, doubles keep their
// data.  The byte family: Hamming(7,4) -- bit 7 ignored, doubles miscorrected,
// as h74_decode4 does everywhere -- or the low nibble of an unprotected byte.
template <typename A>
__device__ __forceinline__ uint32_t byte_table_nibble(const A &a, uint32_t b) {
  if constexpr (is_window<A>) {  // the windowed family: all three byte tables
    if (a.tab == KVECC_CODEC_NONE) return b & 0xFu;
    uint32_t q, t, n1 = 0, n2 = 0;
    if (a.tab == KVECC_CODEC_H74)
      h74_decode4(b, q, t, n1);
    else
      h84_decode4(b, q, t, n1, n2);
    return q & 0xFu;
  } else if constexpr (is_byte<A>) {
    if (a.tab == KVECC_CODEC_NONE) return b & 0xFu;
    uint32_t q, f, n = 0;
    h74_decode4(b, q, f, n);
    return q & 0xFu;
  } else {
    uint32_t q, t, n1 = 0, n2 = 0;
    h84_decode4(b, q, t, n1, n2);
    return q & 0xFu;
  }
}

// The first look of the interpolating kernels: bit 3 of each byte that is a
// type-2 codeword (double detected: syndrome != 0, overall parity even) -- the
// scrubber's h84_dirty4 and four more operations.
__device__ __forceinline__ uint32_t h84_double4(uint32_t w) {
  const uint32_t c = h_code4(w);  // syndrome in bits 0..2, parity error in bit 4 of each byte
  return ((c & 0x07070707u) + 0x07070707u) & ~(c >> 1) & 0x08080808u;
}
// The counted kernels' classification of four stored bytes, on the same first
// look: type 1 (single corrected: syndrome != 0, overall parity odd) and type 2
// (double detected); a parity-only byte (type 3) has syndrome 0 and is neither.
__device__ __forceinline__ void h84_count4(uint32_t w, uint32_t &n_single, uint32_t &n_double) {
  const uint32_t c = h_code4(w);
  const uint32_t nz = ((c & 0x07070707u) + 0x07070707u) & 0x08080808u;
  n_single += __builtin_popcount(nz & (c >> 1));
  n_double += __builtin_popcount(nz & ~(c >> 1));
}
// The repairing kernels' store of one counted word: h84_repair4 (codec_math.h:
// h84_scrub4's XOR and counts from the first look's h_code4, without the decode /
// re-encode round trip) counts its four bytes as h84_count4 does, and the bytes it
// rewrites, and gives the XOR to the word the scrubber would leave -- singles and
// parity-only bytes become encode(decoded data), doubles and clean bytes 0 --
// which goes back through the descriptor the word came through, at the offset it
// came from, only if some byte changes.  A plain vector store: what a concurrent
// reader sees, old byte or new, decodes to the same nibble (kvecc.h "Repairing
// attention").
// NB 4: the whole dword; NB 2: its low two bytes (head_dim 32's V chunk).
template <int NB = 4>
__device__ __forceinline__ void h84_repair_store(__amdgpu_buffer_rsrc_t rs, uint32_t off, uint32_t w,
                                                 uint32_t &n_single, uint32_t &n_double, uint32_t &n_rewritten) {
  const uint32_t x = h84_repair4(w, n_single, n_double, n_rewritten);
  if (x) {
    if constexpr (NB == 2)
      __builtin_amdgcn_raw_buffer_store_b16((unsigned short)(w ^ x), rs, off, 0, 0);
    else
      __builtin_amdgcn_raw_buffer_store_b32(w ^ x, rs, off, 0, 0);
  }
}
// ... and their slow path: four codewords decoded, the doubles replaced by
// interp_word of the neighbours' decoded (not interpolated) values wl / wr, and
// re-encoded, so that the corrected nibbles take the operand path of every
// other byte (the decode table); bytes that are no double keep their data
__device__ __forceinline__ uint32_t h84_interp_fix4(uint32_t w, uint32_t wl, uint32_t wr) {
  uint32_t q, ty, ql, qr, tt, n1 = 0, n2 = 0;
  h84_decode4(w, q, ty, n1, n2);
  h84_decode4(wl, ql, tt, n1, n2);
  h84_decode4(wr, qr, tt, n1, n2);
  return h84_encode4(interp_word(q, ql, qr, ty));
}

// Lane chunk c of a token row: VEC 32-bit words = 4*VEC H(8,4) codewords, or
// VEC Golay codewords (3*VEC values; codewords past the row's last are read
// clamped and contribute nothing, their values fall outside [0, d)); E values.
template <int CODEC, int VEC>
struct Chunk {
  static constexpr int E = CODEC == KVECC_CODEC_H84 ? 4 * VEC : 3 * VEC;
  // decode() returns (n - 8) + kOffset: the Golay path skips the subtraction
  // per element and the kernel folds -8 * kOffset into the sums instead
  static constexpr float kOffset = is_golay(CODEC) ? 8.0f : 0.0f;
  // Golay: decode() returns value 3k + 2 of each codeword times 16
  static constexpr bool kThird16 = is_golay(CODEC);
  uint32_t w[VEC];
  __device__ __forceinline__ void load_buf(const AttnArgs &a, __amdgpu_buffer_rsrc_t rs, int32_t row,
                                           int c) {
    if constexpr (CODEC == KVECC_CODEC_H84) {
      const uint32_t off = (uint32_t)row * (uint32_t)a.d + 4u * VEC * c;
      if constexpr (VEC % 4 == 0) {
#pragma unroll
        for (int k = 0; k < VEC; k += 4) {
          const u32x4 v = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off + 4 * k, 0, 0));
          w[k] = v.x;
          w[k + 1] = v.y;
          w[k + 2] = v.z;
          w[k + 3] = v.w;
        }
      } else {  // head_dim % 16 != 0: one dword per word (VEC 1 or 2)
#pragma unroll
        for (int k = 0; k < VEC; ++k) w[k] = __builtin_amdgcn_raw_buffer_load_b32(rs, off + 4 * k, 0, 0);
      }
    } else if constexpr (CODEC == KVECC_CODEC_GOLAY_PACKED) {
      static_assert(CODEC != KVECC_CODEC_GOLAY_PACKED || VEC == 4 || VEC == 3, "packed lanes own 3 or 4 codewords");
      // past the row's end: a neighbour row's bytes (masked by q = 0) or 0
      if constexpr (VEC == 4) {
        const uint32_t off = (uint32_t)row * a.rowb + 12u * c;
        const auto v = __builtin_amdgcn_raw_buffer_load_b96(rs, off, 0, 0);
        unpack3(v[0], v[1], v[2]);
      } else {  // 9 bytes at 9c: the 3 dwords holding them, realigned.  Rows
                // are whole dwords (KVECC_GOLAY_PACKED_ROW), so the alignment
                // is the lane's own constant, not recomputed per row
        const uint32_t off = (uint32_t)row * a.rowb + ((9u * c) & ~3u);
        const auto v = __builtin_amdgcn_raw_buffer_load_b96(rs, off, 0, 0);
        unpack9(v[0], v[1], v[2], (9u * c) & 3u);
      }
    } else {
      const uint32_t off = ((uint32_t)row * (uint32_t)a.g + VEC * c) * 4u;
      // g % 3 != 0: the row's last lane reads past the row, at the cache's last row past the
      // descriptor's range, which is checked per dword (pinned by tests/test_attention_paths.py)
      if constexpr (VEC == 3) {  // one 12-byte load: 71.9 vs 72.6 us per MHA call against
                                 // three dword loads (profiles/r06/attn/golay_no_gather_probe.txt)
        const auto v = __builtin_amdgcn_raw_buffer_load_b96(rs, off, 0, 0);
        w[0] = v[0] << 2;
        w[1] = v[1] << 2;
        w[2] = v[2] << 2;
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) w[k] = __builtin_amdgcn_raw_buffer_load_b32(rs, off + 4 * k, 0, 0) << 2;
      }
    }
  }
  __device__ __forceinline__ void load(const AttnArgs &a, const void *cache, int64_t row, int c) {
    if constexpr (CODEC == KVECC_CODEC_H84) {
      const uint8_t *p = reinterpret_cast<const uint8_t *>(cache) + row * a.d + 4 * VEC * c;
      if constexpr (VEC % 4 == 0) {
#pragma unroll
        for (int k = 0; k < VEC; k += 4) {
          const u32x4 v = reinterpret_cast<const u32x4 *>(p)[k / 4];
          w[k] = v.x;
          w[k + 1] = v.y;
          w[k + 2] = v.z;
          w[k + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) w[k] = reinterpret_cast<const uint32_t *>(p)[k];
      }
    } else if constexpr (CODEC == KVECC_CODEC_GOLAY_PACKED) {
      const uint32_t *p = reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(cache) + row * a.rowb);
      const int last = (int)(a.rowb / 4) - 1;  // clamp inside the row
      if constexpr (VEC == 4) {
        unpack3(p[min(3 * c, last)], p[min(3 * c + 1, last)], p[min(3 * c + 2, last)]);
      } else {
        const int w0 = 9 * c / 4;
        unpack9(p[min(w0, last)], p[min(w0 + 1, last)], p[min(w0 + 2, last)], (uint32_t)(9 * c) & 3u);
      }
    } else {
      const int32_t *p = reinterpret_cast<const int32_t *>(cache) + row * a.g;
#pragma unroll
      for (int k = 0; k < VEC; ++k) w[k] = (uint32_t)p[min<int64_t>(VEC * c + k, a.g - 1)] << 2;
    }
  }
  // Golay words hold codeword << 2 (bits 0-1 and 26-31: neighbouring bytes,
  // ignored by decode): the first table's byte offset is then one mask.
  // 4 little-endian 3-byte codewords from 3 dwords
  __device__ __forceinline__ void unpack3(uint32_t d0, uint32_t d1, uint32_t d2) {
    w[0] = d0 << 2;
    w[1 < VEC ? 1 : 0] = __builtin_amdgcn_alignbit(d1, d0, 22);
    w[2 < VEC ? 2 : 0] = __builtin_amdgcn_alignbit(d2, d1, 14);
    w[3 < VEC ? 3 : 0] = d2 >> 6;
  }
  // 3 little-endian 3-byte codewords starting at byte `sh` (0-3) of 3 dwords
  __device__ __forceinline__ void unpack9(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t sh) {
    const uint32_t x0 = __builtin_amdgcn_alignbyte(d1, d0, sh), x1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
    const uint32_t x2 = d2 >> (8 * sh);
    w[0] = x0 << 2;
    w[1 < VEC ? 1 : 0] = __builtin_amdgcn_alignbit(x1, x0, 22);
    w[2 < VEC ? 2 : 0] = __builtin_amdgcn_alignbit(x2, x1, 14);
  }
  // values before the row scale, (q - 8): H(8,4) through `lut` (LDS, byte ->
  // data(byte) - 8; double errors keep their data, :144-148), Golay through the
  // correction tables (uncorrectable words keep their data, as golay_decode)
  // SP (Golay; instantiated only by tools/exp/attn_exp.hip): the parity half of
  // the spread table as two 64-entry tables, p(lo) = T0[lo & 63] ^ T1[lo >> 6]
  // (the entries are linear in lo), after the 4096-entry correction half: 16.5
  // KiB of LDS instead of 32, conflict-free parity gathers, 2 more VALU per
  // codeword.  Slower at every split and rows-in-flight count tried (MHA
  // int32 75.0 vs 73.2 us, packed 65.2 vs 59.9; profiles/r06/attn/
  // golay_split_parity_ab.txt): the kernel is bound by its VALU work.
  // DEC bits (0: the product; only tools/exp/attn_exp.hip sets any): 1 split
  // parity (SP above), 2 a probe that keeps the decode's VALU but skips its two
  // LDS gathers and the tables' staging and LDS (WRONG values)
  template <int DEC = 0>
  __device__ __forceinline__ void decode(const h84_lut_t *lut, const uint32_t *gtab, float *v) const {
    constexpr bool SP = (DEC & 1) != 0;
    if constexpr (CODEC == KVECC_CODEC_H84) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * k + e] = (float)lut[(w[k] >> (8 * e)) & 0xFFu];
      }
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        // w = codeword << 2.  P = golay_attn_x_table_dev[lo] = nibbles 0, 1
        // in bytes 0, 1, nibble 2 in bits 28-31, parity(lo) << 14 -- where w
        // holds the received parity -- so the syndrome's byte offset into the
        // correction half is ((w ^ P) & 0x3FFC000) >> 12: one v_bitop3
        // (0x28 = (S0 ^ S1) & S2) and a shift
        const char *tb = reinterpret_cast<const char *>(gtab);
        uint32_t p;
        if (DEC & 2)
          p = w[k] & 0x3FFCu;
        else if (SP)
          p = *reinterpret_cast<const uint32_t *>(tb + 16384 + (w[k] & 0xFCu)) ^
              *reinterpret_cast<const uint32_t *>(tb + 16384 + 256 + ((w[k] >> 6) & 0xFCu));
        else
          p = *reinterpret_cast<const uint32_t *>(tb + (w[k] & 0x3FFCu));
        const uint32_t off = __builtin_amdgcn_bitop3_b32(w[k], p, 0x03FFC000u, 0x28) >> 12;
        const uint32_t e = (DEC & 2) ? off : *reinterpret_cast<const uint32_t *>(tb + (SP ? 0 : 16384) + off);
        // corrected nibbles: (p ^ e) & 0xF0000F0F; the conversions are written
        // out because the compiler otherwise re-extracts each nibble with a
        // shift and a mask.  The third value comes out as 16 n (byte 3 = n << 4):
        // the kernel prescales its query slot by 1/16 and rescales its
        // accumulator by 1/16 (kThirdScale; powers of two, so exact)
        const uint32_t sp = __builtin_amdgcn_bitop3_b32(p, e, 0xF0000F0Fu, 0x28);
        asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(v[3 * k]) : "v"(sp));  // n, see kOffset
        asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(v[3 * k + 1]) : "v"(sp));
        asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(v[3 * k + 2]) : "v"(sp));  // 16 n
      }
    }
  }
  // The counted Golay kernels' look at word k (the [statistics] island of
  // attn_split_body.inc): the count field of its correction entry, bits 16-23
  // of golay_attn_x_table_dev's second half -- (bits corrected & 3) |
  // uncorrectable << 6, which decode() masks off -- through decode()'s two
  // lookups.  Bits 0-1 and 26-31 of w (an int32 word's bits 24-31, a packed
  // neighbour's bytes) take no part, as in decode().
  __device__ __forceinline__ uint32_t count(const uint32_t *gtab, int k) const {
    const char *tb = reinterpret_cast<const char *>(gtab);
    const uint32_t p = *reinterpret_cast<const uint32_t *>(tb + (w[k] & 0x3FFCu));
    const uint32_t off = __builtin_amdgcn_bitop3_b32(w[k], p, 0x03FFC000u, 0x28) >> 12;
    return (*reinterpret_cast<const uint32_t *>(tb + 16384 + off) >> 16) & 0xFFu;
  }
};

typedef float f32x2 __attribute__((ext_vector_type(2)));

// sum_e q[e] * v[e] as packed FMAs (v_pk_fma_f32) into two independent lanes
template <int E>
__device__ __forceinline__ float dot(const float *q, const float *v) {
  f32x2 s = {0.0f, 0.0f};
#pragma unroll
  for (int e = 0; e + 1 < E; e += 2) s = __builtin_elementwise_fma(f32x2{q[e], q[e + 1]}, f32x2{v[e], v[e + 1]}, s);
  if (E % 2) s.x = fmaf(q[E - 1], v[E - 1], s.x);
  return s.x + s.y;
}

// acc[e] += p * v[e] as packed FMAs
template <int E>
__device__ __forceinline__ void axpy(float *acc, float p, const float *v) {
#pragma unroll
  for (int e = 0; e + 1 < E; e += 2) {
    const f32x2 r = __builtin_elementwise_fma(f32x2{p, p}, f32x2{v[e], v[e + 1]}, f32x2{acc[e], acc[e + 1]});
    acc[e] = r.x;
    acc[e + 1] = r.y;
  }
  if (E % 2) acc[E - 1] = fmaf(p, v[E - 1], acc[E - 1]);
}

// Workspace entries under the fused combine are read by a workgroup that may
// sit on another XCD (another L2): they are written and read as agent-scope
// relaxed atomics (global_store / global_load sc1, coherent at the memory side)
// -- an agent-scope fence would write back and invalidate the whole L2
// (buffer_wbl2 / buffer_inv sc1), which measured 4x the kernel's time.
__device__ __forceinline__ void ws_put(float *p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool COHERENT>
__device__ __forceinline__ float ws_get(const float *p) {
  if (COHERENT) return __hip_atomic_load(const_cast<float *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return *p;
}

// combine the splits of one (b, h): out = sum_s acc_s e^(m_s - M) / sum_s l_s e^(m_s - M)
// (one workgroup; wt holds kMaxSplits floats, bred kBlock / kWave).  Two
// "one memory round trip" forms measured slower per 32q/8kv call: every thread
// folding all splits online, one thread per output value (29.5 vs 22.7 us), and
// one wave per (b, h) with the weights by v_readlane (31.2 vs 22.5 us) -- fewer,
// longer-lived waves each walking the splits serially.
template <typename T, bool COHERENT = false>
__device__ void combine_bh(const AttnArgs &a, int64_t bh, float *wt, float *bred) {
  const int64_t stride = a.d + 2;
  const float *ws = a.ws + bh * a.nsplit * stride;
  if (a.nsplit <= kBlock) {
    // one memory round trip: thread s < nsplit loads its split's (m, l) while
    // thread d < head_dim loads its first kPre accumulators; the two block
    // reductions then run in LDS
    constexpr int kPre = 16;
    const int t = threadIdx.x, ns = (int)a.nsplit;
    float ov[kPre];
#pragma unroll
    for (int s = 0; s < kPre; ++s) ov[s] = t < a.d && s < ns ? ws_get<COHERENT>(ws + s * stride + 2 + t) : 0.0f;
    const float ms = t < ns ? ws_get<COHERENT>(ws + t * stride) : -INFINITY;
    const float ls = t < ns ? ws_get<COHERENT>(ws + t * stride + 1) : 0.0f;
    float mx = ms;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, kWave));
    if ((t & (kWave - 1)) == 0) bred[t / kWave] = mx;
    __syncthreads();
    mx = bred[0];
#pragma unroll
    for (int w = 1; w < kBlock / kWave; ++w) mx = fmaxf(mx, bred[w]);
    __syncthreads();
    const float w = ms == -INFINITY ? 0.0f : attn_exp(ms - mx);
    if (t < ns) wt[t] = w;
    float L = w * ls;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) L += __shfl_xor(L, off, kWave);
    if ((t & (kWave - 1)) == 0) bred[t / kWave] = L;
    __syncthreads();
    L = 0.0f;
#pragma unroll
    for (int v = 0; v < kBlock / kWave; ++v) L += bred[v];
    if (t < a.d) {
      float acc = 0.0f;
#pragma unroll
      for (int s = 0; s < kPre; ++s) acc += ov[s] * (s < ns ? wt[s] : 0.0f);
      for (int s = kPre; s < ns; ++s) acc += ws_get<COHERENT>(ws + s * stride + 2 + t) * wt[s];
      reinterpret_cast<T *>(a.out)[bh * a.d + t] = from_f32<T>(L > 0.0f ? acc / L : a.empty_value);
    }
    return;
  }
  float mx = -INFINITY;
  for (int64_t s = threadIdx.x; s < a.nsplit; s += kBlock) mx = fmaxf(mx, ws_get<COHERENT>(ws + s * stride));
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, kWave));
  if ((threadIdx.x & (kWave - 1)) == 0) bred[threadIdx.x / kWave] = mx;
  __syncthreads();
  mx = bred[0];
#pragma unroll
  for (int w = 1; w < kBlock / kWave; ++w) mx = fmaxf(mx, bred[w]);
  __syncthreads();
  float L = 0.0f;
  for (int64_t s = threadIdx.x; s < a.nsplit; s += kBlock) {
    const float ms = ws_get<COHERENT>(ws + s * stride);
    const float w = ms == -INFINITY ? 0.0f : attn_exp(ms - mx);
    wt[s] = w;
    L += w * ws_get<COHERENT>(ws + s * stride + 1);
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) L += __shfl_xor(L, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) bred[threadIdx.x / kWave] = L;
  __syncthreads();
  L = 0.0f;
#pragma unroll
  for (int w = 0; w < kBlock / kWave; ++w) L += bred[w];
  T *out = reinterpret_cast<T *>(a.out) + bh * a.d;
  for (int64_t di = threadIdx.x; di < a.d; di += kBlock) {
    float acc = 0.0f;
#pragma unroll 4
    for (int64_t s = 0; s < a.nsplit; ++s) acc += ws_get<COHERENT>(ws + s * stride + 2 + di) * wt[s];
    out[di] = from_f32<T>(L > 0.0f ? acc / L : a.empty_value);  // no valid token: see the header
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void paged_attn_combine_kernel(AttnArgs a) {
  __shared__ float wt[kMaxSplits];
  __shared__ float bred[kBlock / kWave];
  combine_bh<T>(a, blockIdx.x, wt, bred);
}

// The combine for <= kCombineWaveSplits splits and head_dim <= 128: one
// workgroup of two waves per (b, h), thread d owns output d.  Every wave folds
// the splits' (m, l) itself -- lane s holds split s, the maximum and the
// weighted sum by cross-lane reductions, the weights broadcast by readlane --
// so the kernel has no LDS and no barrier between its one memory round trip
// and its store.
constexpr int kCombineWaveSplits = 16;
template <typename T>
__global__ __launch_bounds__(2 * kWave) void paged_attn_combine_wave_kernel(AttnArgs a) {
  const int64_t bh = blockIdx.x, stride = a.d + 2;
  const float *ws = a.ws + bh * a.nsplit * stride;
  const int t = threadIdx.x, lane = t % kWave, ns = (int)a.nsplit;
  float ov[kCombineWaveSplits];
#pragma unroll
  for (int s = 0; s < kCombineWaveSplits; ++s) ov[s] = t < a.d && s < ns ? ws[s * stride + 2 + t] : 0.0f;
  const float ms = lane < ns ? ws[lane * stride] : -INFINITY;
  const float ls = lane < ns ? ws[lane * stride + 1] : 0.0f;
  float mx = ms;
#pragma unroll
  for (int off = kCombineWaveSplits / 2; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, kWave));
  const float w = ms == -INFINITY ? 0.0f : attn_exp(ms - mx);
  float L = w * ls;
#pragma unroll
  for (int off = kCombineWaveSplits / 2; off > 0; off >>= 1) L += __shfl_xor(L, off, kWave);
  L = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, L)));
  if (t < a.d) {
    float acc = 0.0f;
#pragma unroll
    for (int s = 0; s < kCombineWaveSplits; ++s)
      acc += ov[s] * __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, w), s));
    reinterpret_cast<T *>(a.out)[bh * a.d + t] = from_f32<T>(L > 0.0f ? acc / L : a.empty_value);
  }
}

// Fused combine: the workgroup that finishes the last split of its (batch, head
// group) -- counted on a.ctr[blockIdx.y] -- combines the group's G query heads
// and resets the counter, saving the combine launch (the launcher uses it for
// G = 1 only: with G heads the tail after the last split cost more than the
// combine launch, even with all G heads combined in one round trip: 32q/8kv
// 26.7 vs 22.3 us, profiles/r03/attn/attn_gqa19.log).  The workspace stores are
// sc1 (ws_put) and every thread waits for its own before the count; the last
// workgroup reads the entries with sc1 loads.  wt: kMaxSplits floats of LDS the
// caller no longer needs.
//
// Why no release/acquire: on gfx942/gfx950 an sc1 store (ws_put) is performed
// at the memory side (it bypasses the non-coherent per-XCD L2 state for this
// line) once the issuing wave's vmcnt reaches 0, and an sc1 load misses every
// CU/L2 copy, so "store sc1; s_waitcnt vmcnt(0); barrier; atomic add" on the
// writers and "atomic returns the last count; load sc1" on the reader order the
// workspace without the whole-L2 writeback an agent-scope release costs
// (buffer_wbl2: 4x the kernel).  That is a property of these
// targets' cache hierarchy, not of the HIP memory model: any other target must
// not compile this path (the launcher then uses the separate combine kernel).
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__)
#error "combine_if_last relies on gfx942/gfx950 sc1 + vmcnt ordering; use launch_combine on other targets"
#endif
template <typename T, int G>
__device__ void combine_if_last(const AttnArgs &a, int64_t bh0, float *wt) {
  __shared__ float bred[kBlock / kWave];
  __shared__ uint32_t last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's sc1 workspace stores performed
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t prev = __hip_atomic_fetch_add(a.ctr + blockIdx.y, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = prev + 1 == gridDim.x;
    if (last) __hip_atomic_store(a.ctr + blockIdx.y, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!last) return;
  for (int j = 0; j < G; ++j) {
    if (j) __syncthreads();
    combine_bh<T, true>(a, bh0 + j, wt, bred);
  }
}


// GQA (G > 1): workgroup (split, y) serves the G query heads hg*G .. hg*G+G-1
// of batch b = y / (H/G), which share one cache head: each K and V row is
// loaded and decoded once and used G times (a dot product, an online softmax
// state and an accumulator per head), where one workgroup per query head read
// and decoded every cache row H/Hkv times.
template <typename T, int CODEC, int VEC, int W, bool BUF, int G = 1, int UR = 0, int DEC = 0>
__global__ __launch_bounds__(kBlock) void paged_attn_split_kernel(AttnArgs a) {
#define ATTN_BODY_CHUNK 0
#include "attn_split_body.inc"
#undef ATTN_BODY_CHUNK
}
// the general path of a chunked call: the same body over the virtual batch (ChunkArgs)
template <typename T, int CODEC, int VEC, int W, bool BUF, int G = 1>
__global__ __launch_bounds__(kBlock) void paged_attn_split_chunk_kernel(RaggedArgs a) {
  constexpr int UR = 0, DEC = 0;
#define ATTN_BODY_CHUNK 1
#include "attn_split_body.inc"
#undef ATTN_BODY_CHUNK
}
// the general path of an interpolating call (kvecc_paged_attention_interp): the chunk form
// with the [interpolation] island, Hamming(8,4) over buffer-addressed caches only
template <typename T, int VEC, int W, int G = 1>
__global__ __launch_bounds__(kBlock) void paged_attn_split_interp_kernel(InterpArgs a) {
  constexpr int CODEC = KVECC_CODEC_H84, UR = 0, DEC = 0;
  constexpr bool BUF = true;
#define ATTN_BODY_CHUNK 2
#include "attn_split_body.inc"
#undef ATTN_BODY_CHUNK
}
// the counted entry's kernels (kvecc_paged_attention_stats): the chunk form and the interpolating
// form with the [statistics] islands, Hamming(8,4) over buffer-addressed caches only
template <typename T, int VEC, int W, int G = 1>
__global__ __launch_bounds__(kBlock) void paged_attn_split_stats_kernel(StatsArgs a) {
  constexpr int CODEC = KVECC_CODEC_H84, UR = 0, DEC = 0;
  constexpr bool BUF = true;
#define ATTN_BODY_CHUNK 1
#define ATTN_BODY_STATS 1
#include "attn_split_body.inc"
#undef ATTN_BODY_STATS
#undef ATTN_BODY_CHUNK
}
template <typename T, int VEC, int W, int G = 1>
__global__ __launch_bounds__(kBlock) void paged_attn_split_stats_interp_kernel(StatsInterpArgs a) {
  constexpr int CODEC = KVECC_CODEC_H84, UR = 0, DEC = 0;
  constexpr bool BUF = true;
#define ATTN_BODY_CHUNK 2
#define ATTN_BODY_STATS 1
#include "attn_split_body.inc"
#undef ATTN_BODY_STATS
#undef ATTN_BODY_CHUNK
}
// the repairing entry's kernels (kvecc_paged_attention_repair): the counted kernels' two forms with the
// [repair] islands as well
template <typename T, int VEC, int W, int G = 1>
__global__ __launch_bounds__(kBlock) void paged_attn_split_repair_kernel(RepairArgs a) {
  constexpr int CODEC = KVECC_CODEC_H84, UR = 0, DEC = 0;
  constexpr bool BUF = true;
#define ATTN_BODY_CHUNK 1
#define ATTN_BODY_STATS 1
#define ATTN_BODY_REPAIR 1
#include "attn_split_body.inc"
#undef ATTN_BODY_REPAIR
#undef ATTN_BODY_STATS
#undef ATTN_BODY_CHUNK
}
template <typename T, int VEC, int W, int G = 1>
__global__ __launch_bounds__(kBlock) void paged_attn_split_repair_interp_kernel(RepairInterpArgs a) {
  constexpr int CODEC = KVECC_CODEC_H84, UR = 0, DEC = 0;
  constexpr bool BUF = true;
#define ATTN_BODY_CHUNK 2
#define ATTN_BODY_STATS 1
#define ATTN_BODY_REPAIR 1
#include "attn_split_body.inc"
#undef ATTN_BODY_REPAIR
#undef ATTN_BODY_STATS
#undef ATTN_BODY_CHUNK
}
// the Golay counted entry's kernels (kvecc_paged_attention_golay_stats): the chunk form with the
// [statistics] islands, int32 and packed caches, buffer-addressed only
template <typename T, int CODEC, int VEC, int W, int G = 1>
__global__ __launch_bounds__(kBlock) void paged_attn_split_golay_stats_kernel(StatsArgs a) {
  static_assert(is_golay(CODEC), "the Golay counted kernels");
  constexpr int UR = 0, DEC = 0;
  constexpr bool BUF = true;
#define ATTN_BODY_CHUNK 1
#define ATTN_BODY_STATS 1
#include "attn_split_body.inc"
#undef ATTN_BODY_STATS
#undef ATTN_BODY_CHUNK
}
// the byte family's general path (KVECC_CODEC_H74 / KVECC_CODEC_NONE caches): the Hamming(8,4)
// instantiations of the same body, the table by the argument block's selector
template <typename T, int VEC, int W, bool BUF, int G = 1>
__global__ __launch_bounds__(kBlock) void paged_attn_split_byte_kernel(ByteAttnArgs a) {
  constexpr int CODEC = KVECC_CODEC_H84, UR = 0, DEC = 0;
#define ATTN_BODY_CHUNK 0
#include "attn_split_body.inc"
#undef ATTN_BODY_CHUNK
}
template <typename T, int VEC, int W, bool BUF, int G = 1>
__global__ __launch_bounds__(kBlock) void paged_attn_split_byte_chunk_kernel(ByteChunkArgs a) {
  constexpr int CODEC = KVECC_CODEC_H84, UR = 0, DEC = 0;
#define ATTN_BODY_CHUNK 1
#include "attn_split_body.inc"
#undef ATTN_BODY_CHUNK
}
// the windowed entry's kernels (kvecc_paged_attention_window): the chunk form with the [window]
// islands, every codec and query dtype; Hamming(8,4)'s instantiations serve the byte family too
// (WindowArgs::tab)
template <typename T, int CODEC, int VEC, int W, bool BUF, int G = 1>
__global__ __launch_bounds__(kBlock) void paged_attn_split_window_kernel(WindowArgs a) {
  constexpr int UR = 0, DEC = 0;
#define ATTN_BODY_CHUNK 1
#define ATTN_BODY_WINDOW 1
#include "attn_split_body.inc"
#undef ATTN_BODY_WINDOW
#undef ATTN_BODY_CHUNK
}

// ---- GQA on the matrix cores (Hamming(8,4), fp16 queries) -----------------------
//
// With G query heads per cache head the VALU kernel above does G dot products
// and G accumulator updates per decoded value, so its time stays near the MHA
// kernel's while the cache bytes fall by G.  Here both products run on
// v_mfma_f32_16x16x32_f16, and the VALU only decodes:
//   S^T[16 tokens x 16 heads] = K[16 tokens x D] . Q^T[D x 16 heads]   (D/32 MFMAs per 16 tokens)
//   O^T[16 d x 16 heads]     += V^T[16 d x 32 tokens] . P[32 tokens x 16 heads]
// Columns are query heads (G <= 16 used, the rest zero).  Decoded values n - 8
// (integers in [-8, 7]) and the fp16 queries are exact in f16, so the scores
// are the fp32 sums of exact products, as in the VALU kernel; P (fp32) goes
// in as two f16 halves, hi + lo, 22 bits.  The operand maps (A[row l&15][k =
// 8(l>>4)+j], B[k][col l&15], C[row 4(l>>4)+r][col l&15]) are bent so that
// every lane's loads stay contiguous and no value moves between lanes:
//   * K: lane (token t = l&15, group g = l>>4) loads D/4 contiguous bytes of its
//     token row, d = (D/4)g .. ; MFMA kk takes bytes 8kk..8kk+7 (the same k -> d
//     map for the Q operand, which is loaded once);
//   * a wave step is 32 tokens, two S^T tiles; lane (head n, g) then holds
//     the scores of tokens 4g + r and 16 + 4g + r (r = 0..3) for head n -- which
//     are exactly the 8 k-slots of the PV B operand when PV's k maps slot
//     8g + j to token 16(j >> 2) + 4g + (j & 3): P needs no shuffle;
//   * V: the same 8 tokens per lane, D/16 contiguous bytes each at d = (D/16) m
//     (m = l&15); M-tile mt takes byte mt of each, so output row m of tile mt
//     is d = (D/16)(4g + r) + mt.
// Decode: LDS table byte -> data nibble (single errors corrected, doubles keep
// their data, attention_ecc.py:56-149), pairs packed as f16 1024 + n by an OR
// of 0x6400 and shifted by one v_pk_add_f16 of -1032.  The online softmax runs
// per lane on its 8 scores (head maxima across the 4 lanes of a head with two
// xor-shuffles), the workgroup's 4 waves merge through LDS, and the split goes
// to the workspace of the combine kernel above.
// Fused combine: the last split of each (batch, head group) combines it
// (combine_if_last) -- for one query head per workgroup only (see
// kvecc_paged_attention).  Issuing the next step's loads before this step's
// math took the kernel to 191 VGPRs (2 waves per SIMD): 32q/8kv 29.8 us
// against 22.9 without.  4 workgroups per CU for the H(8,4) kernel.
constexpr int kMfmaWgPerCu = 4;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kMfmaStep = 32;  // tokens per wave step

// Decoded values as MFMA operands: the table's nibble n (0..15) goes into an
// f16 half as is -- the subnormal n * 2^-24, exact -- so a pair costs one
// v_perm; the kernel scales the products by 2^24 and folds the -8 out as
// -8 * sum(q) (scores) and -8 * sum(p) (outputs).  (f16 1024 + n by an OR of
// 0x6400 and one v_pk_add_f16 of -1032 per pair measured within noise.)
constexpr float kMfmaValScale = 16777216.0f;  // 2^24
constexpr float kMfmaValOffset = 8.0f;
// The PV operand's normaliser (kvecc.h "Scale range").  The weights w = p * v_scale go
// to the matrix cores as an f16 hi + lo pair, which carries 22 bits only while w is far
// above the f16 subnormal step 2^-24 and below 65504; v_scales are absmax / 7 of the
// activations and bounded by neither.  So each column keeps a power of two c, the
// accumulator holds O / c and the operand is w / c < 2: c is the power of two at or below
// max(c * alpha, the step's largest w), rescaled like l and psum, clamped to 2^+-100 so
// that c, 1 / c and c * 2^24 stay normal floats.  Multiplying by a power of two is exact;
// psum never sees c.
__device__ __forceinline__ float pv_norm_pow2(float x) {
  const float y = fminf(fmaxf(x, 0x1p-100f), 0x1p100f);
  return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, y) & 0x7F800000u);
}
// 1 / c of a normal power of two c in [2^-126, 2^126]
__device__ __forceinline__ float pv_norm_recip(float c) {
  return __builtin_bit_cast(float, 0x7F000000u - __builtin_bit_cast(uint32_t, c));
}
// two table values (data nibbles 0..15) -> f16 operand pair, lo in bits 0..15
__device__ __forceinline__ uint32_t nib_pair_f16(uint32_t lo, uint32_t hi) {
  return __builtin_amdgcn_perm(hi, lo, 0x0c040c00u);  // [0, hi, 0, lo]
}

// NB contiguous bytes (2, 4, 8, 16 or 32) at byte offset off -> dwords w
template <int NB>
__device__ __forceinline__ void load_chunk(__amdgpu_buffer_rsrc_t rs, uint32_t off, uint32_t *w) {
  if constexpr (NB == 2) {
    w[0] = __builtin_amdgcn_raw_buffer_load_b16(rs, off, 0, 0);
  } else if constexpr (NB == 4) {
    w[0] = __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0);
  } else if constexpr (NB == 8) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0);
    w[0] = v[0];
    w[1] = v[1];
  } else {
#pragma unroll
    for (int k = 0; k < NB / 16; ++k) {
      const u32x4 v = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16 * k, 0, 0));
      w[4 * k] = v.x;
      w[4 * k + 1] = v.y;
      w[4 * k + 2] = v.z;
      w[4 * k + 3] = v.w;
    }
  }
}

// What a column of a matrix-core chunk kernel stands for.  The decode kernels'
// column n is query head h0 + n of the workgroup's G (blockIdx.y = (batch, head
// group), blockIdx.x = split), and every column sees the sequence's whole
// context.  The chunk kernels use all 16 columns: with cg = 2^cg_log2 query
// heads sharing the cache head, column n is chunk token tq = (16 / cg) tile +
// n / cg and head h0 + n % cg, blockIdx.x = tile * nsplit + split.  Token tq
// of a span (first, count) -- (0, q_len) in a uniform call -- is a query row when
// the span holds it (ChunkSpan); it sits at position context_len - count + (tq -
// first) and sees the keys at or before it:
// its key limit is that position + 1, clamped to [0, ctx_cap]; the workgroup
// walks the split up to the tile's largest limit (its last valid token's), each
// lane masks the scores at or past its own column's.  A padding column loads no
// query and has limit 0.  A tile without a valid token (`any` false) stages
// nothing: its workgroups write the empty partial (put_empty) and leave.  A masked score is -inf like a
// -1 block's, so it has no weight in l, psum (the -8 fold) or the accumulators,
// and a column with nothing to see in this split leaves m = -inf, l = 0.
template <typename A>
struct ChunkMapT {
  static constexpr bool kRagged = std::is_same<A, RaggedArgs>::value;
  int64_t b, h0, ctx;
  uint32_t split_idx, tile, tq, hq;
  bool col_ok;  // the column holds a query row (a valid token)
  bool any;     // some column of the tile does
  int64_t lim;  // this column's key limit (absolute)
  __device__ __forceinline__ ChunkMapT(const A &a, int n) {
    const uint32_t hgroups = (uint32_t)a.heads >> a.cg_log2;
    b = blockIdx.y / hgroups;
    h0 = (int64_t)(blockIdx.y % hgroups) << a.cg_log2;
    tile = blockIdx.x / (uint32_t)a.nsplit;
    split_idx = blockIdx.x - tile * (uint32_t)a.nsplit;
    const uint32_t tpt = 16u >> a.cg_log2;  // tokens per tile
    tq = tile * tpt + ((uint32_t)n >> a.cg_log2);
    hq = (uint32_t)h0 + ((uint32_t)n & ((1u << a.cg_log2) - 1u));
    if constexpr (kRagged) {
      const ChunkSpan sp(a, b);
      col_ok = sp.valid(a, tq);
      // the tile's valid tokens: [max(v0, tile start), min(v1, tile end))
      const int64_t tv0 = max<int64_t>(sp.v0(), (int64_t)tile * tpt);
      const int64_t tv1 = min<int64_t>(sp.v1(a), (int64_t)tile * tpt + tpt);
      any = tv1 > tv0;
      const int64_t first = any ? sp.lim0(a, b) : 0;  // token 0's key limit (no context_lens read without a token)
      ctx = any ? min<int64_t>(first + tv1 - 1, a.ctx_cap) : 0;
      lim = col_ok ? min<int64_t>(first + tq, a.ctx_cap) : 0;
    } else {  // the uniform call: every token of the chunk is a query row
      any = true;
      col_ok = tq < a.q_len;
      const int64_t first = (int64_t)a.ctx_lens[b] - a.q_len + 1;  // token 0's key limit
      const uint32_t tlast = min(tile * tpt + tpt - 1u, a.q_len - 1u);
      ctx = min<int64_t>(first + tlast, a.ctx_cap);
      lim = col_ok ? min<int64_t>(first + tq, a.ctx_cap) : 0;
    }
  }
  // a tile without a valid token: m = -inf, l = 0 and zero accumulators for
  // every row of the tile in this split, which the combine turns into the empty value
  __device__ __forceinline__ void put_empty(const ChunkArgs &a) const {
    const int64_t stride = a.d + 2;
    for (int64_t idx = threadIdx.x; idx < 16 * stride; idx += kBlock) {
      const int h = (int)(idx / stride), e = (int)(idx - h * stride);
      const int64_t orow = out_row(a, h);
      if (orow >= 0) ws_put(a.ws + (orow * a.nsplit + split_idx) * stride + e, e == 0 ? -INFINITY : 0.0f);
    }
  }
  // the column's limit relative to the split's first token t0, as an int the
  // lanes compare token indices against (clamped: a split has <= kMaxSplit tokens)
  __device__ __forceinline__ int col_limit(int64_t t0) const {
    return (int)max<int64_t>(min<int64_t>(lim - t0, kMaxSplit + kMfmaStep), 0);
  }
  __device__ __forceinline__ const __half *q_row(const ChunkArgs &a) const {
    return reinterpret_cast<const __half *>(a.q) + b * a.q_sb + tq * a.q_st + hq * a.q_sh;
  }
  // output (and workspace) row of column h of the workgroup; -1: no query row there
  __device__ __forceinline__ int64_t out_row(const ChunkArgs &a, int h) const {
    const uint32_t t = tile * (16u >> a.cg_log2) + ((uint32_t)h >> a.cg_log2);
    if (t >= a.q_len) return -1;
    return (b * a.q_len + t) * a.heads + h0 + ((uint32_t)h & ((1u << a.cg_log2) - 1u));
  }
};

// The windowed kernels' map: the ragged map plus the column's lower key bound and the
// tile's smallest (its first valid token's).  Column (tq, hq) at position p = first + tq - 1
// sees key j < lim iff j < sinks or j >= lo = max(p - window + 1, 0); the workgroup stages
// the cache rows some column of the tile can see -- [0, sinks) and [lo_min, ctx) -- and each
// lane masks the scores below its own column's lo ([score mask]).  A type of its own, so
// that ChunkMapT and the kernels over it keep their text.
struct WindowMap : ChunkMapT<RaggedArgs> {
  int64_t lo, lo_min;
  __device__ __forceinline__ WindowMap(const WindowArgs &a, int n) : ChunkMapT<RaggedArgs>(a, n) {
    lo = lo_min = 0;
    if (any) {
      const ChunkSpan sp(a, b);
      const uint32_t tpt = 16u >> a.cg_log2;
      const int64_t first = sp.lim0(a, b), tv0 = max<int64_t>(sp.v0(), (int64_t)tile * tpt);
      lo_min = max<int64_t>(first + tv0 - (int64_t)a.window, 0);
      lo = col_ok ? max<int64_t>(first + tq - (int64_t)a.window, 0) : 0;
    }
  }
  // a bound relative to the split's first token t0, as an int the lanes compare token indices against
  __device__ __forceinline__ static int rel(int64_t x, int64_t t0) {
    return (int)max<int64_t>(min<int64_t>(x - t0, kMaxSplit + kMfmaStep), 0);
  }
};

template <int D, int G>
__global__ __launch_bounds__(kBlock, 2) void paged_attn_h84_mfma_kernel(AttnArgs a) {
#define ATTN_BODY_CHUNK 0
#include "attn_h84_mfma_body.inc"
#undef ATTN_BODY_CHUNK
}
// the chunked causal form: 16 (token, head) columns per workgroup (ChunkMap)
template <int D>
__global__ __launch_bounds__(kBlock, 2) void paged_attn_h84_mfma_chunk_kernel(ChunkArgs a) {
  constexpr int G = 16;
  using ChunkMap = ChunkMapT<ChunkArgs>;
#define ATTN_BODY_CHUNK 1
#include "attn_h84_mfma_body.inc"
#undef ATTN_BODY_CHUNK
}
// the ragged entry's: the same body with the span rule in its ChunkMap
template <int D>
__global__ __launch_bounds__(kBlock, 2) void paged_attn_h84_mfma_ragged_kernel(RaggedArgs a) {
  constexpr int G = 16;
  using ChunkMap = ChunkMapT<RaggedArgs>;
#define ATTN_BODY_CHUNK 1
#include "attn_h84_mfma_body.inc"
#undef ATTN_BODY_CHUNK
}
// the interpolating entry's: the ragged form with double errors interpolated
// from the neighbouring tokens before the operands are built (the body's [interpolation] islands)
template <int D>
__global__ __launch_bounds__(kBlock, 2) void paged_attn_h84_mfma_interp_kernel(InterpArgs a) {
  constexpr int G = 16;
  using ChunkMap = ChunkMapT<RaggedArgs>;
#define ATTN_BODY_CHUNK 2
#include "attn_h84_mfma_body.inc"
#undef ATTN_BODY_CHUNK
}
// the counted entry's (kvecc_paged_attention_stats): the ragged form and the interpolating
// form with the [statistics] islands
template <int D>
__global__ __launch_bounds__(kBlock, 2) void paged_attn_h84_mfma_stats_interp_kernel(StatsInterpArgs a) {
  constexpr int G = 16;
  using ChunkMap = ChunkMapT<RaggedArgs>;
#define ATTN_BODY_CHUNK 2
#define ATTN_BODY_STATS 1
#include "attn_h84_mfma_body.inc"
#undef ATTN_BODY_STATS
#undef ATTN_BODY_CHUNK
}
template <int D>
__global__ __launch_bounds__(kBlock, 2) void paged_attn_h84_mfma_stats_kernel(StatsArgs a) {
  constexpr int G = 16;
  using ChunkMap = ChunkMapT<RaggedArgs>;
#define ATTN_BODY_CHUNK 1
#define ATTN_BODY_STATS 1
#include "attn_h84_mfma_body.inc"
#undef ATTN_BODY_STATS
#undef ATTN_BODY_CHUNK
}
// the repairing entry's (kvecc_paged_attention_repair): the counted kernels' two forms with the [repair]
// islands as well
template <int D>
__global__ __launch_bounds__(kBlock, 2) void paged_attn_h84_mfma_repair_interp_kernel(RepairInterpArgs a) {
  constexpr int G = 16;
  using ChunkMap = ChunkMapT<RaggedArgs>;
#define ATTN_BODY_CHUNK 2
#define ATTN_BODY_STATS 1
#define ATTN_BODY_REPAIR 1
#include "attn_h84_mfma_body.inc"
#undef ATTN_BODY_REPAIR
#undef ATTN_BODY_STATS
#undef ATTN_BODY_CHUNK
}
template <int D>
__global__ __launch_bounds__(kBlock, 2) void paged_attn_h84_mfma_repair_kernel(RepairArgs a) {
  constexpr int G = 16;
  using ChunkMap = ChunkMapT<RaggedArgs>;
#define ATTN_BODY_CHUNK 1
#define ATTN_BODY_STATS 1
#define ATTN_BODY_REPAIR 1
#include "attn_h84_mfma_body.inc"
#undef ATTN_BODY_REPAIR
#undef ATTN_BODY_STATS
#undef ATTN_BODY_CHUNK
}
// the byte family's: the decode, chunk and ragged kernels over the same body
template <int D, int G>
__global__ __launch_bounds__(kBlock, 2) void paged_attn_byte_mfma_kernel(ByteAttnArgs a) {
#define ATTN_BODY_CHUNK 0
#include "attn_h84_mfma_body.inc"
#undef ATTN_BODY_CHUNK
}
template <int D>
__global__ __launch_bounds__(kBlock, 2) void paged_attn_byte_mfma_chunk_kernel(ByteUniformArgs a) {
  constexpr int G = 16;
  using ChunkMap = ChunkMapT<ChunkArgs>;
#define ATTN_BODY_CHUNK 1
#include "attn_h84_mfma_body.inc"
#undef ATTN_BODY_CHUNK
}
template <int D>
__global__ __launch_bounds__(kBlock, 2) void paged_attn_byte_mfma_ragged_kernel(ByteChunkArgs a) {
  constexpr int G = 16;
  using ChunkMap = ChunkMapT<RaggedArgs>;
#define ATTN_BODY_CHUNK 1
#include "attn_h84_mfma_body.inc"
#undef ATTN_BODY_CHUNK
}
// the windowed entry's (kvecc_paged_attention_window): the ragged form with the [window] islands,
// the decode table by WindowArgs::tab (Hamming(8,4), Hamming(7,4) or unprotected INT4)
template <int D>
__global__ __launch_bounds__(kBlock, 2) void paged_attn_h84_mfma_window_kernel(WindowArgs a) {
  constexpr int G = 16;
  using ChunkMap = WindowMap;
#define ATTN_BODY_CHUNK 1
#define ATTN_BODY_WINDOW 1
#include "attn_h84_mfma_body.inc"
#undef ATTN_BODY_WINDOW
#undef ATTN_BODY_CHUNK
}

// ---- GQA on the matrix cores, Golay(24,12) int32 caches, head_dim 128 ---------
//
// The H(8,4) kernel's scheme with codeword-aligned operand maps (a row is 43
// codewords = 129 nibbles, d = 3c + e):
//   * QK: lane group g owns codewords 11g .. 11g+10 of its token's K row (44
//     bytes: two 16-byte loads and a 12-byte one), i.e. d = 33g .. 33g+32, as
//     k-slots 0..32 of 40 (5 MFMAs per 16 tokens; slots past 32, and d >= 128,
//     carry q = 0);
//   * PV: lane m owns codewords 3m .. 3m+2 (a 12-byte load per token), 9
//     M-tiles, output row m of tile mt is d = 9m + mt (d >= 128 discarded).
// Codewords decode through the spread tables (two LDS reads, one v_bitop3) to
// nibbles one per byte; an operand pair is one v_perm of two decoded words
// into f16 subnormals (n * 2^-24), with the 2^24 scale and the -8 folds of the
// H(8,4) kernel.  Tokens, scales, the softmax and the merge are that kernel's.
//
// Packed caches (3-byte codewords, 132-byte rows) keep the maps where the loads
// stay dword-aligned: K lane groups own 12 codewords (36 bytes at 36g, d = 36g
// .. 36g+35, still 5 MFMAs), V lanes own codewords 3m .. 3m+2 (9 bytes at 9m:
// one 12-byte load from the dword below, then v_alignbyte by m & 3).  Bytes past
// the row's 129 belong to d >= 128 (q = 0, outputs discarded).
template <int G, bool PACKED>
__global__ __launch_bounds__(kBlock, 2) void paged_attn_golay_mfma_kernel(AttnArgs a) {
#define ATTN_BODY_CHUNK 0
#include "attn_golay_mfma_body.inc"
#undef ATTN_BODY_CHUNK
}
template <bool PACKED>
__global__ __launch_bounds__(kBlock, 2) void paged_attn_golay_mfma_chunk_kernel(ChunkArgs a) {
  constexpr int G = 16;
  using ChunkMap = ChunkMapT<ChunkArgs>;
#define ATTN_BODY_CHUNK 1
#include "attn_golay_mfma_body.inc"
#undef ATTN_BODY_CHUNK
}
template <bool PACKED>
__global__ __launch_bounds__(kBlock, 2) void paged_attn_golay_mfma_ragged_kernel(RaggedArgs a) {
  constexpr int G = 16;
  using ChunkMap = ChunkMapT<RaggedArgs>;
#define ATTN_BODY_CHUNK 1
#include "attn_golay_mfma_body.inc"
#undef ATTN_BODY_CHUNK
}
// the counted entry's (kvecc_paged_attention_golay_stats): the ragged form with the [statistics]
// islands, at every q_max
template <bool PACKED>
__global__ __launch_bounds__(kBlock, 2) void paged_attn_golay_mfma_stats_kernel(StatsArgs a) {
  constexpr int G = 16;
  using ChunkMap = ChunkMapT<RaggedArgs>;
#define ATTN_BODY_CHUNK 1
#define ATTN_BODY_STATS 1
#include "attn_golay_mfma_body.inc"
#undef ATTN_BODY_STATS
#undef ATTN_BODY_CHUNK
}
// the windowed entry's (kvecc_paged_attention_window): the ragged form with the [window] islands
template <bool PACKED>
__global__ __launch_bounds__(kBlock, 2) void paged_attn_golay_mfma_window_kernel(WindowArgs a) {
  constexpr int G = 16;
  using ChunkMap = WindowMap;
#define ATTN_BODY_CHUNK 1
#define ATTN_BODY_WINDOW 1
#include "attn_golay_mfma_body.inc"
#undef ATTN_BODY_WINDOW
#undef ATTN_BODY_CHUNK
}

// ---- host side: one dispatch path ------------------------------------------------
// Which kernel and which argument block serve a call of a given mode, codec,
// head_dim, dtype and addressing is decided in this section, each decision once:
//   with_q_dtype / with_head_dim / with_codec   run-time value -> template argument
//   split_kernel / tile_kernel / decode_mfma_kernel   (block, codec, ...) -> kernel; a
//     combination without a kernel does not compile, or where it is instantiated
//     returns KVECC_EINVAL: nothing returns KVECC_OK having launched nothing
//   launch_attn / launch_rows / launch_tiles / launch_decode_mfma   grid, launch, combine
//   attn_setup   validation and argument fill of every entry
// and `entry` is the C entry's name without "kvecc_", the prefix of its messages.

template <typename T>
static void launch_combine(const AttnArgs &a, int64_t batch, hipStream_t st) {
  if (a.nsplit <= kCombineWaveSplits && a.d <= 2 * kWave)
    KVECC_LAUNCH(paged_attn_combine_wave_kernel<T>, dim3((unsigned)(batch * a.heads)), dim3(2 * kWave), 0, st, a);
  else
    KVECC_LAUNCH(paged_attn_combine_kernel<T>, dim3((unsigned)(batch * a.heads)), dim3(kBlock), 0, st, a);
}

static int pow2_at_least(int64_t x) {
  int w = 1;
  while (w < x) w <<= 1;
  return w;
}

template <typename T>
struct type_tag {
  using type = T;
};
template <int V>
using int_tag = std::integral_constant<int, V>;

// f(type_tag<T>) for the query's element type T
template <typename F>
static int with_q_dtype(const char *entry, int q_dtype, F &&f) {
  switch (q_dtype) {
    case KVECC_F32: return f(type_tag<float>{});
    case KVECC_F16: return f(type_tag<__half>{});
    case KVECC_BF16: return f(type_tag<__hip_bfloat16>{});
    default: return set_error(KVECC_EINVAL, "%s: bad dtype %d", entry, q_dtype);
  }
}

// f(int_tag<D>) for a matrix-core kernel's head_dim: 32, 64 or 128 (attn_mfma_heads,
// attn_chunk_mfma_heads)
template <typename F>
static int with_head_dim(int64_t d, F &&f) {
  switch (d) {
    case 32: return f(int_tag<32>{});
    case 64: return f(int_tag<64>{});
    default: return f(int_tag<128>{});
  }
}

// The blocks whose kernels decode Golay caches too: every other block's decode
// Hamming(8,4)'s layout only
template <typename A>
constexpr bool takes_golay = std::is_same<A, AttnArgs>::value || std::is_same<A, ChunkArgs>::value ||
                             std::is_same<A, RaggedArgs>::value || std::is_same<A, StatsArgs>::value ||
                             std::is_same<A, WindowArgs>::value;
// The blocks whose kernels address the caches through buffer descriptors only (caches under 4 GiB)
template <typename A>
constexpr bool buf_only = is_interp<A> || is_stats<A> || is_repair<A>;

// f(int_tag<CODEC>) for the codec of block A's kernels (the byte family arrives as Hamming(8,4))
template <typename A, typename F>
static int with_codec(const char *entry, int codec, F &&f) {
  if (codec == KVECC_CODEC_H84) return f(int_tag<KVECC_CODEC_H84>{});
  if constexpr (takes_golay<A>) {
    if (codec == KVECC_CODEC_GOLAY) return f(int_tag<KVECC_CODEC_GOLAY>{});
    if (codec == KVECC_CODEC_GOLAY_PACKED) return f(int_tag<KVECC_CODEC_GOLAY_PACKED>{});
  }
  return set_error(KVECC_EINVAL, "%s: no kernel of this call's mode decodes codec %d", entry, codec);
}

// The split kernel of an argument block: the decode entry's (AttnArgs), the chunked
// call's over its virtual batch (RaggedArgs), or a mode's own
template <typename T, int CODEC, int VEC, int W, bool BUF, int G, typename A>
constexpr auto split_kernel() {
  if constexpr (std::is_same<A, AttnArgs>::value) {
    return &paged_attn_split_kernel<T, CODEC, VEC, W, BUF, G>;
  } else if constexpr (std::is_same<A, RaggedArgs>::value) {
    return &paged_attn_split_chunk_kernel<T, CODEC, VEC, W, BUF, G>;
  } else if constexpr (std::is_same<A, WindowArgs>::value) {
    return &paged_attn_split_window_kernel<T, CODEC, VEC, W, BUF, G>;
  } else if constexpr (std::is_same<A, StatsArgs>::value && is_golay(CODEC)) {
    static_assert(BUF, "the counted kernels are buffer-addressed");
    return &paged_attn_split_golay_stats_kernel<T, CODEC, VEC, W, G>;
  } else {
    static_assert(CODEC == KVECC_CODEC_H84, "this block's kernels decode Hamming(8,4)'s layout only");
    if constexpr (std::is_same<A, ByteAttnArgs>::value) {
      return &paged_attn_split_byte_kernel<T, VEC, W, BUF, G>;
    } else if constexpr (std::is_same<A, ByteChunkArgs>::value) {
      return &paged_attn_split_byte_chunk_kernel<T, VEC, W, BUF, G>;
    } else {
      static_assert(BUF, "the interpolating, counted and repairing kernels are buffer-addressed");
      if constexpr (std::is_same<A, InterpArgs>::value) {
        return &paged_attn_split_interp_kernel<T, VEC, W, G>;
      } else if constexpr (std::is_same<A, StatsArgs>::value) {
        return &paged_attn_split_stats_kernel<T, VEC, W, G>;
      } else if constexpr (std::is_same<A, StatsInterpArgs>::value) {
        return &paged_attn_split_stats_interp_kernel<T, VEC, W, G>;
      } else if constexpr (std::is_same<A, RepairArgs>::value) {
        return &paged_attn_split_repair_kernel<T, VEC, W, G>;
      } else {
        static_assert(std::is_same<A, RepairInterpArgs>::value, "no split kernel takes this block");
        return &paged_attn_split_repair_interp_kernel<T, VEC, W, G>;
      }
    }
  }
}

template <typename T, int CODEC, int VEC, bool BUF, typename A>
static int launch_split_w(const A &a, dim3 grid, hipStream_t st) {
  const int w = pow2_at_least((a.g + VEC - 1) / VEC);
  switch (w) {
#define KVECC_ATTN_CASE(WW)                                                                     \
  case WW:                                                                                      \
    KVECC_LAUNCH((split_kernel<T, CODEC, VEC, WW, BUF, 1, A>()), grid, dim3(kBlock), 0, st, a); \
    return KVECC_OK;
    KVECC_ATTN_CASE(1)
    KVECC_ATTN_CASE(2)
    KVECC_ATTN_CASE(4)
    KVECC_ATTN_CASE(8)
    KVECC_ATTN_CASE(16)
    KVECC_ATTN_CASE(32)
    KVECC_ATTN_CASE(64)
#undef KVECC_ATTN_CASE
    default:
      return set_error(KVECC_EINVAL, "paged_attention: %lld lane chunks per token row > 64",
                       (long long)((a.g + VEC - 1) / VEC));
  }
}

template <typename T, int CODEC, int VEC, typename A>
static int launch_split(const char *entry, const A &a, dim3 grid, hipStream_t st) {
  if (a.cache_bytes) return launch_split_w<T, CODEC, VEC, true>(a, grid, st);
  if constexpr (buf_only<A>)
    return set_error(KVECC_EINVAL, "%s: no kernel of this call's mode reads caches of 4 GiB or more", entry);
  else
    return launch_split_w<T, CODEC, VEC, false>(a, grid, st);
}

// words per lane of a token row: the VEC the codec's kernels use at head_dim d
// (the H(8,4) GQA kernels take 2 words = 8 codewords per lane: with G query
// rows and accumulators per lane, 4 words took 188 VGPRs at G = 4)
constexpr int kH84GqaVec = 2;
static int attn_vec(int codec, int64_t d, bool gqa = false) {
  if (codec == KVECC_CODEC_H84)
    return gqa && d % 8 == 0 ? kH84GqaVec : d % (4 * kH84Vec) == 0 ? kH84Vec : d % 16 == 0 ? 4 : 1;
  return codec == KVECC_CODEC_GOLAY ? kGolayVec : kGolayPackedVec;
}

// query heads per workgroup: the GQA kernels cover buffer-addressed caches with
// lane groups of 8-32 lanes per row (head_dim 64-256) and G in {2, 4} dividing
// H / Hkv (G 8 would hold 8 query rows and accumulators per lane); else 1
static int attn_heads_per_wg(int codec, int64_t d, int64_t g, int64_t heads, int64_t kv_heads, bool buf) {
  const int64_t group = heads / kv_heads;
  const int vec = attn_vec(codec, d, true);
  const int w = pow2_at_least((g + vec - 1) / vec);
  if (!buf || w < 8 || w > 32 || (codec == KVECC_CODEC_H84 && d % 8 != 0)) return 1;
  const int gmax = codec == KVECC_CODEC_GOLAY_PACKED ? 2 : 4;  // packed: G = 2 (the realigned loads' registers)
  return group % 4 == 0 && gmax >= 4 ? 4 : group % 2 == 0 ? 2 : 1;
}

// (gq > 1 only with buffer addressing: attn_heads_per_wg)
template <typename T, int CODEC, int VEC, int G, typename A>
static int launch_split_gqa(const A &a, dim3 grid, hipStream_t st) {
  switch (pow2_at_least((a.g + VEC - 1) / VEC)) {
    case 8: KVECC_LAUNCH((split_kernel<T, CODEC, VEC, 8, true, G, A>()), grid, dim3(kBlock), 0, st, a); break;
    case 16: KVECC_LAUNCH((split_kernel<T, CODEC, VEC, 16, true, G, A>()), grid, dim3(kBlock), 0, st, a); break;
    default: KVECC_LAUNCH((split_kernel<T, CODEC, VEC, 32, true, G, A>()), grid, dim3(kBlock), 0, st, a); break;
  }
  return KVECC_OK;
}

template <typename T, int CODEC, int VEC, typename A>
static int launch_split_g(const char *entry, const A &a, int64_t batch, int gq, hipStream_t st) {
  dim3 grid((unsigned)a.nsplit, (unsigned)(batch * a.heads / gq));
  if (gq == 1) return launch_split<T, CODEC, VEC>(entry, a, grid, st);
  constexpr int GV = CODEC == KVECC_CODEC_H84 ? kH84GqaVec : VEC;
  if constexpr (CODEC != KVECC_CODEC_GOLAY_PACKED)
    if (gq == 4) return launch_split_gqa<T, CODEC, GV, 4>(a, grid, st);
  return launch_split_gqa<T, CODEC, GV, 2>(a, grid, st);
}

// The split kernels over `batch` query rows per head, then the combine unless it is
// fused (a.ctr) or the caller's (combine false: launch_rows' slices)
template <typename T, int CODEC, typename A>
static int launch_attn(const char *entry, const A &a, int64_t batch, int gq, hipStream_t st, bool combine = true) {
  int rc;
  if constexpr (CODEC == KVECC_CODEC_H84) {
    if (a.d % (4 * kH84Vec) == 0)
      rc = launch_split_g<T, CODEC, kH84Vec>(entry, a, batch, gq, st);  // 16-byte loads, 16 codewords per lane
    else if (a.d % 16 == 0)
      rc = launch_split_g<T, CODEC, 4>(entry, a, batch, gq, st);
    else
      rc = launch_split_g<T, CODEC, 1>(entry, a, batch, gq, st);
  } else if constexpr (CODEC == KVECC_CODEC_GOLAY) {
    rc = launch_split_g<T, CODEC, kGolayVec>(entry, a, batch, gq, st);  // 3 codewords per lane: 43 -> 15 of 16 lanes
  } else {
    rc = launch_split_g<T, CODEC, kGolayPackedVec>(entry, a, batch, gq, st);  // 3 codewords per lane: 43 -> 15 of 16
  }
  if (rc != KVECC_OK) return rc;
  if (!a.ctr && combine) launch_combine<T>(a, batch, st);
  return KVECC_OK;
}

// The general path of a chunked call: the split kernels of block A over the virtual
// batch of `rows` = batch * q_len query rows (ChunkArgs::q_len), in slices that fit
// grid.y, then one combine over all rows.
constexpr int64_t kMaxGridY = 65535;
template <typename T, typename A>
static int launch_rows(const char *entry, int codec, A a, int64_t rows, int gq, hipStream_t st) {
  return with_codec<A>(entry, codec, [&](auto c) {
    constexpr int CODEC = decltype(c)::value;
    const int64_t wg_per_row = a.heads / gq;
    if (rows * wg_per_row <= kMaxGridY) return launch_attn<T, CODEC>(entry, a, rows, gq, st);
    const int64_t per = kMaxGridY / wg_per_row;  // >= 1: checked by the caller
    for (int64_t vb = 0; vb < rows; vb += per) {
      a.vb0 = (uint32_t)vb;
      const int rc = launch_attn<T, CODEC>(entry, a, std::min(per, rows - vb), gq, st, false);
      if (rc != KVECC_OK) return rc;
    }
    launch_combine<T>(a, rows, st);
    return (int)KVECC_OK;
  });
}

// The decode entry's matrix-core kernel of (block, codec, head_dim, G query heads per
// workgroup); Golay: head_dim 128 and G >= 2 (attn_mfma_heads)
template <typename A, int CODEC, int D, int G>
constexpr auto decode_mfma_kernel() {
  if constexpr (std::is_same<A, ByteAttnArgs>::value) {
    static_assert(CODEC == KVECC_CODEC_H84, "the byte family decodes Hamming(8,4)'s layout");
    return &paged_attn_byte_mfma_kernel<D, G>;
  } else {
    static_assert(std::is_same<A, AttnArgs>::value, "no decode matrix-core kernel takes this block");
    if constexpr (is_golay(CODEC))
      return &paged_attn_golay_mfma_kernel<G, CODEC == KVECC_CODEC_GOLAY_PACKED>;
    else
      return &paged_attn_h84_mfma_kernel<D, G>;
  }
}

template <typename A>
static int launch_decode_mfma(const char *entry, int codec, const A &a, int64_t batch, int gm, hipStream_t st) {
  const dim3 grid((unsigned)a.nsplit, (unsigned)(batch * a.heads / gm));
  auto launch = [&](auto c, auto d, auto g) {
    constexpr int CODEC = decltype(c)::value, G = decltype(g)::value;
    if constexpr (is_golay(CODEC) && G == 1) {  // Golay MHA stays on the split kernels (attn_mfma_heads)
      return set_error(KVECC_EINVAL, "%s: no Golay matrix-core kernel for one query head per workgroup", entry);
    } else {
      KVECC_LAUNCH((decode_mfma_kernel<A, CODEC, decltype(d)::value, G>()), grid, dim3(kBlock), 0, st, a);
      return (int)KVECC_OK;
    }
  };
  const int rc = with_codec<A>(entry, codec, [&](auto c) {
    return with_head_dim(a.d, [&](auto d) {
      switch (gm) {
        case 1: return launch(c, d, int_tag<1>{});
        case 2: return launch(c, d, int_tag<2>{});
        case 4: return launch(c, d, int_tag<4>{});
        case 8: return launch(c, d, int_tag<8>{});
        default: return launch(c, d, int_tag<16>{});
      }
    });
  });
  if (rc != KVECC_OK) return rc;
  if (!a.ctr) launch_combine<__half>(a, batch, st);
  return KVECC_OK;
}

// query heads per workgroup of the MFMA kernels (0: not applicable): caches under
// 4 GiB, fp16 queries (16-byte aligned); Hamming(8,4) at head_dim 32 / 64 / 128
// for any group, Golay (int32 or packed) at head_dim 128 for groups of >= 2
// workgroups per CU of the Golay kernel's split choice (157 VGPRs, 49-73 KiB of
// LDS): 2 measured 30.6 vs 34.2 us at 4 (32q/8kv; profiles/r03/attn/attn_gqa14.log)
constexpr int kMfmaGolayWgPerCu = 2;
static int attn_mfma_heads(int codec, int q_dtype, const void *query, int64_t d, int64_t heads,
                           int64_t kv_heads, bool buf) {
  const int64_t group = heads / kv_heads;
  const bool h84 = codec == KVECC_CODEC_H84 && (d == 32 || d == 64 || d == 128);
  const bool golay = (codec == KVECC_CODEC_GOLAY || codec == KVECC_CODEC_GOLAY_PACKED) &&
                     d == 128;
  if (!(h84 || golay) || q_dtype != KVECC_F16 || !buf || !aligned(query, 16)) return 0;
  // MHA (one query head per cache head): H(8,4) too, one of the 16 MFMA
  // columns used -- the matrix cores take the dot products and the V update
  // off the VALU, and the table lookups are the only per-value LDS work:
  // [8,4096,32,128] 49.5 us per call against 54.6 for the VALU split kernel.
  // Golay MHA stays on the VALU kernels (packed 76 vs 68 us, int32 86 vs 73:
  // its per-codeword decode, not the arithmetic, is the work).
  // (tools/exp/run_attn_exp.py, profiles/r04/attn/mfma_mha_ab.log)
  if (group == 1) return h84 ? 1 : 0;
  return group % 16 == 0 ? 16 : group % 8 == 0 ? 8 : group % 4 == 0 ? 4 : group % 2 == 0 ? 2 : 0;
}

// heads per column group of the matrix-core chunk kernels (0: the general
// path): attn_mfma_heads' domain with every query row 16-byte aligned, Golay
// MHA included -- a decoded row serves 16 query columns here, so its decode
// cost is shared where the decode-step kernel spends it on one
static int attn_chunk_mfma_heads(int codec, int q_dtype, const void *query, int64_t sb, int64_t st, int64_t sh,
                                 int64_t d, int64_t heads, int64_t kv_heads, bool buf) {
  const int64_t group = heads / kv_heads;
  const bool h84 = codec == KVECC_CODEC_H84 && (d == 32 || d == 64 || d == 128);
  const bool golay = (codec == KVECC_CODEC_GOLAY || codec == KVECC_CODEC_GOLAY_PACKED) && d == 128;
  if (!(h84 || golay) || q_dtype != KVECC_F16 || !buf) return 0;
  if (!aligned(query, 16) || sb % 8 || st % 8 || sh % 8) return 0;
  if (group == 1) return 1;
  return group % 16 == 0 ? 16 : group % 8 == 0 ? 8 : group % 4 == 0 ? 4 : group % 2 == 0 ? 2 : 0;
}

// The matrix-core tile kernel of a chunked call's (block, codec, head_dim); Golay:
// head_dim 128 (attn_chunk_mfma_heads).  The uniform kernels take the narrower
// blocks ChunkArgs / ByteUniformArgs (see RaggedArgs, ByteUniformArgs).
template <typename A, int CODEC, int D>
constexpr auto tile_kernel() {
  if constexpr (is_golay(CODEC)) {
    constexpr bool PACKED = CODEC == KVECC_CODEC_GOLAY_PACKED;
    if constexpr (std::is_same<A, ChunkArgs>::value) {
      return &paged_attn_golay_mfma_chunk_kernel<PACKED>;
    } else if constexpr (std::is_same<A, RaggedArgs>::value) {
      return &paged_attn_golay_mfma_ragged_kernel<PACKED>;
    } else if constexpr (std::is_same<A, WindowArgs>::value) {
      return &paged_attn_golay_mfma_window_kernel<PACKED>;
    } else {
      static_assert(std::is_same<A, StatsArgs>::value, "no Golay tile kernel takes this block");
      return &paged_attn_golay_mfma_stats_kernel<PACKED>;
    }
  } else if constexpr (std::is_same<A, ChunkArgs>::value) {
    return &paged_attn_h84_mfma_chunk_kernel<D>;
  } else if constexpr (std::is_same<A, RaggedArgs>::value) {
    return &paged_attn_h84_mfma_ragged_kernel<D>;
  } else if constexpr (std::is_same<A, WindowArgs>::value) {
    return &paged_attn_h84_mfma_window_kernel<D>;
  } else if constexpr (std::is_same<A, InterpArgs>::value) {
    return &paged_attn_h84_mfma_interp_kernel<D>;
  } else if constexpr (std::is_same<A, StatsArgs>::value) {
    return &paged_attn_h84_mfma_stats_kernel<D>;
  } else if constexpr (std::is_same<A, StatsInterpArgs>::value) {
    return &paged_attn_h84_mfma_stats_interp_kernel<D>;
  } else if constexpr (std::is_same<A, RepairArgs>::value) {
    return &paged_attn_h84_mfma_repair_kernel<D>;
  } else if constexpr (std::is_same<A, RepairInterpArgs>::value) {
    return &paged_attn_h84_mfma_repair_interp_kernel<D>;
  } else if constexpr (std::is_same<A, ByteUniformArgs>::value) {
    return &paged_attn_byte_mfma_chunk_kernel<D>;
  } else {
    static_assert(std::is_same<A, ByteChunkArgs>::value, "no tile kernel takes this block");
    return &paged_attn_byte_mfma_ragged_kernel<D>;
  }
}

// The matrix-core path of a chunked call: block A's tile kernel over `tiles`
// 16-column tiles per (sequence, head group), then the combine.  A uniform call of
// the plain and the byte kernels (no spans) hands over the narrower block.
template <typename A>
static int launch_tiles(const char *entry, int codec, const A &a, int64_t batch, int64_t tiles, hipStream_t st) {
  if constexpr (std::is_same<A, RaggedArgs>::value) {
    if (!a.q_spans) return launch_tiles<ChunkArgs>(entry, codec, a, batch, tiles, st);
  } else if constexpr (std::is_same<A, ByteChunkArgs>::value) {
    if (!a.q_spans) {
      ByteUniformArgs u;
      static_cast<ChunkArgs &>(u) = a;
      u.tab = a.tab;
      return launch_tiles(entry, codec, u, batch, tiles, st);
    }
  }
  const dim3 grid((unsigned)(a.nsplit * tiles), (unsigned)(batch * (a.heads >> a.cg_log2)));
  const int rc = with_codec<A>(entry, codec, [&](auto c) {
    return with_head_dim(a.d, [&](auto d) {
      KVECC_LAUNCH((tile_kernel<A, decltype(c)::value, decltype(d)::value>()), grid, dim3(kBlock), 0, st, a);
      return (int)KVECC_OK;
    });
  });
  if (rc != KVECC_OK) return rc;
  launch_combine<__half>(a, batch * a.q_len, st);
  return KVECC_OK;
}

// tokens per workgroup: the largest power of two <= kMaxSplit that still gives
// >= per_cu workgroups per CU (small batch*heads decode steps split finer); 8
// per CU made every codec 1-15 % slower
static int64_t choose_split(int64_t bh, int64_t max_context_len, int per_cu = 4) {
  // longer splits amortise each workgroup's fixed work (table staging, the
  // group merge); measured best at 1024 for both codecs at [8,4096,32,128]
  const int64_t top = kMaxSplit;
  int64_t split = top;
  const int64_t want = (int64_t)per_cu * cu_count();
  while (split > 32 && bh * cdiv(max_context_len, split) < want) split >>= 1;
  while (cdiv(max_context_len, split) > kMaxSplits && split < top) split <<= 1;
  return split;
}

// The finest split a chunked call can pick: its matrix-core grid has at least
// rows / 16 workgroups per split (16 query rows per tile), the split kernels'
// rows / 4.
static int64_t chunk_finest_split(int64_t rows, int64_t max_context_len) {
  return choose_split(std::max<int64_t>(1, rows / 16), max_context_len);
}

// ---- the entries' shared front half ----------------------------------------------
// (AttnCall, the record of a call, and AttnMode are in kvecc_internal.h: the host twin takes them too)

// What an entry decides between the argument fill and the split count (attn_setup's
// `plan`, which also sets a.split and, in a chunked call, a.cg_log2)
struct AttnPlan {
  int gq = 1, gm = 0;  // query heads per workgroup: the split kernels', the matrix-core kernels' (0: not taken)
  int64_t tiles = 1;   // matrix-core chunk kernels: 16-column tiles per (sequence, head group)
  bool ctr = false;    // the fused combine (AttnArgs::ctr)
};

// Validation and argument fill of every attention entry, in the order the messages
// have always come in.  A: ByteAttnArgs (the decode entry) or ByteChunkArgs -- the
// byte family's blocks, which hold every other codec's (AttnArgs / RaggedArgs) as
// their base.  codec: the call's; on return the kernels' (the byte family runs as
// Hamming(8,4): kvecc.h).  plan(a, fits, max_context_len, p) is the entry's choice
// of kernels and split size, `fits` saying that the caches are buffer-addressable.
template <typename A, typename Plan>
static int attn_setup(const char *entry, const AttnCall &c, int &codec, A &a, AttnPlan &p, Plan &&plan) {
  if (c.kv_heads < 1 || c.heads % c.kv_heads != 0)
    return set_error(KVECC_EINVAL, "%s: %lld heads not a multiple of %lld kv heads", entry, (long long)c.heads,
                     (long long)c.kv_heads);
  if (c.head_dim < 1 || c.head_dim > kAttnMaxD)
    return set_error(KVECC_EINVAL, "%s: head_dim %lld not in [1, %d]", entry, (long long)c.head_dim, kAttnMaxD);
  if (codec != KVECC_CODEC_NONE && codec != KVECC_CODEC_H74 && codec != KVECC_CODEC_H84 &&
      codec != KVECC_CODEC_GOLAY && codec != KVECC_CODEC_GOLAY_PACKED)
    return set_error(KVECC_EINVAL, "%s: codec %d (int4, hamming74, hamming84, golay or golay_packed only)", entry,
                     codec);
  // the byte family (kvecc.h): Hamming(8,4)'s layout, rules and launch geometry, its own kernels
  const int table = codec;
  if (codec == KVECC_CODEC_NONE || codec == KVECC_CODEC_H74) codec = KVECC_CODEC_H84;
  if (codec == KVECC_CODEC_H84 && c.head_dim % 4 != 0)
    return set_error(KVECC_EINVAL, "%s: %s head_dim must be a multiple of 4", entry,
                     table == KVECC_CODEC_NONE ? "int4" : table == KVECC_CODEC_H74 ? "hamming74" : "hamming84");
  if constexpr (is_chunk<A>)  // (the decode entry names a bad dtype last, where it dispatches on it)
    if (c.q_dtype != KVECC_F32 && c.q_dtype != KVECC_F16 && c.q_dtype != KVECC_BF16)
      return set_error(KVECC_EINVAL, "%s: bad dtype %d", entry, c.q_dtype);
  if (c.num_layers < 1 || c.layer < 0 || c.layer >= c.num_layers || c.block_size < 1 || c.max_blocks < 1)
    return set_error(KVECC_EINVAL, "%s: bad cache geometry", entry);
  const int64_t rows_total = c.num_blocks * c.num_layers * c.kv_heads * c.block_size;
  if (c.num_blocks < 1 || rows_total > 0x7FFFFFFFLL)
    return set_error(KVECC_EINVAL, "%s: cache rows must fit int32", entry);
  const int64_t max_context_len = c.max_context_len <= 0 ? c.max_blocks * c.block_size : c.max_context_len;
  if (!c.query || !c.k_cache || !c.v_cache || !c.block_table || !c.context_lens || !c.k_scales || !c.v_scales ||
      !c.out || !c.workspace)
    return set_error(KVECC_EINVAL, "%s: null pointer", entry);
  if constexpr (is_chunk<A>) {
    const int64_t vbatch = c.batch * c.q_len;  // query rows per head: the virtual batch
    if (c.q_len > 0x7FFFFFFFLL || vbatch > 0x7FFFFFFFLL || vbatch * c.heads > 0x7FFFFFFFLL)
      return set_error(KVECC_EINVAL, "%s: %lld x %lld x %lld query rows exceed the grid", entry, (long long)c.batch,
                       (long long)c.q_len, (long long)c.heads);
  }
  // (q_len 1: kvecc_paged_attention_workspace, the decode entry's bound)
  const int64_t need =
      kvecc_paged_attention_chunk_workspace(c.batch, c.q_len, c.heads, c.head_dim, max_context_len);
  if (c.workspace_floats < need)
    return set_error(KVECC_EINVAL, "%s: workspace %lld < %lld floats", entry, (long long)c.workspace_floats,
                     (long long)need);
  a.tab = (uint32_t)table;
  a.q = c.query;
  a.k_cache = c.k_cache;
  a.v_cache = c.v_cache;
  a.table = c.block_table;
  a.ctx_lens = c.context_lens;
  a.k_scales = c.k_scales;
  a.v_scales = c.v_scales;
  a.ws = c.workspace;
  a.out = c.out;
  a.heads = c.heads;
  a.kv_heads = c.kv_heads;
  a.d = c.head_dim;
  a.g = codec == KVECC_CODEC_H84 ? c.head_dim / 4 : (c.head_dim + 2) / 3;
  a.rowb = (uint32_t)KVECC_GOLAY_PACKED_ROW(a.g);
  a.layers = c.num_layers;
  a.layer = c.layer;
  a.bs = c.block_size;
  a.max_blocks = c.max_blocks;
  a.ctx_cap = std::min(max_context_len, c.max_blocks * c.block_size);
  a.sm_scale = c.sm_scale;
  a.empty_value = codec == KVECC_CODEC_H84 ? -8.0f : 0.0f;
  if constexpr (is_chunk<A>) {
    a.q_len = (uint32_t)c.q_len;
    a.vb0 = 0;
    a.q_sb = c.q_sb;
    a.q_st = c.q_st;
    a.q_sh = c.q_sh;
    a.cg_log2 = 0;
    a.q_spans = c.q_spans;
  }
  const int64_t cb = rows_total * (codec == KVECC_CODEC_H84            ? c.head_dim
                                   : codec == KVECC_CODEC_GOLAY_PACKED ? (int64_t)a.rowb
                                                                       : 4 * a.g);
  const bool fits = cb <= 0xFFFFFFFFLL && rows_total * 4 <= 0xFFFFFFFFLL;
  a.cache_bytes = fits ? (uint32_t)cb : 0u;  // 0 selects the 64-bit-addressed kernels
  a.scale_bytes = fits ? (uint32_t)(rows_total * 4) : 0u;
  const int rc = plan(a, fits, max_context_len, p);
  if (rc != KVECC_OK) return rc;
  a.nsplit = cdiv(max_context_len, a.split);
  if (a.nsplit > kMaxSplits)
    return set_error(KVECC_EINVAL, "%s: context %lld too long", entry, (long long)max_context_len);
  if (p.gm && a.nsplit * p.tiles > 0x7FFFFFFFLL)
    return set_error(KVECC_EINVAL, "%s: %lld splits x %lld tiles exceed the grid", entry, (long long)a.nsplit,
                     (long long)p.tiles);
  a.par = a.cor = nullptr;
  a.atab = a.atab_x = nullptr;
  a.ctr = nullptr;
  if (p.ctr) {
    a.ctr = attn_counter_slot(c.stream);
    if (!a.ctr) return KVECC_EHIP;
  }
  if (codec != KVECC_CODEC_H84) {
    a.par = golay_parity_table_dev();
    a.cor = golay_correct_table_dev();
    a.atab = golay_attn_table_dev();
    a.atab_x = golay_attn_x_table_dev();
    if (!a.par || !a.cor || !a.atab || !a.atab_x) return KVECC_EHIP;
  }
  return KVECC_OK;
}

// ---- the decode entry --------------------------------------------------------------
static int paged_attention_decode(const AttnCall &c) {
  const char *entry = "paged_attention";
  if (c.batch < 0 || c.heads < 0 || c.kv_heads < 0 || c.head_dim < 0)
    return set_error(KVECC_EINVAL, "paged_attention: negative size");
  if (c.batch == 0 || c.heads == 0) return KVECC_OK;
  int codec = c.codec;
  ByteAttnArgs a;  // AttnArgs for every other codec's kernels
  AttnPlan p;
  const int rc = attn_setup(entry, c, codec, a, p, [&](ByteAttnArgs &a, bool fits, int64_t max_context_len, AttnPlan &p) {
    p.gq = attn_heads_per_wg(codec, c.head_dim, a.g, c.heads, c.kv_heads, fits);
    p.gm = attn_mfma_heads(codec, c.q_dtype, c.query, c.head_dim, c.heads, c.kv_heads, fits);
    if (p.gm)  // kMfma*WgPerCu workgroups per CU, never finer than the workspace allows
      a.split = std::max(choose_split(c.batch * c.heads / p.gm, max_context_len,
                                      codec != KVECC_CODEC_H84 ? kMfmaGolayWgPerCu : kMfmaWgPerCu),
                         choose_split(std::max<int64_t>(1, c.batch * c.heads / 4), max_context_len));
    else
      a.split = choose_split(c.batch * c.heads / p.gq, max_context_len);
    // fused combine for one query head per workgroup only (MHA 59.7 -> 58.9 us).
    // With G heads the tail after the last split -- the sc1 stores' acknowledgement,
    // the counter's round trip and rounds of sc1 loads, which bypass the L2 -- cost
    // more than the combine launch: 32q/8kv 22.6 -> 32.8 us with the G heads
    // combined serially, 26.9 with one wave per head, 26.7 (against 22.3) with all
    // G heads in one round trip (combine_group; profiles/r03/attn/).
    const int gw = p.gm ? p.gm : p.gq;  // query heads per workgroup
    p.ctr = gw == 1 && c.batch * c.heads <= kAttnCtrPerSlot;
    return (int)KVECC_OK;
  });
  if (rc != KVECC_OK) return rc;
  hipStream_t st = as_stream(c.stream);
  auto run = [&](const auto &b) {  // b: the block of the codec's kernels
    using B = std::decay_t<decltype(b)>;
    if (p.gm) return launch_decode_mfma(entry, codec, b, c.batch, p.gm, st);
    return with_q_dtype(entry, c.q_dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      return with_codec<B>(entry, codec,
                           [&](auto cd) { return launch_attn<T, decltype(cd)::value>(entry, b, c.batch, p.gq, st); });
    });
  };
  const bool bytes = c.codec == KVECC_CODEC_NONE || c.codec == KVECC_CODEC_H74;
  const int lrc = bytes ? run(a) : run(static_cast<const AttnArgs &>(a));
  if (lrc != KVECC_OK) return lrc;
  return check_launch("paged_attention");
}

// ---- chunked causal attention ---------------------------------------------------
static const char *mode_entry(const AttnMode &m) {
  switch (m.kind) {
    case AttnKind::golay_counted: return "paged_attention_golay_stats";
    case AttnKind::repair: return "paged_attention_repair";
    case AttnKind::counted: return "paged_attention_stats";
    case AttnKind::windowed: return "paged_attention_window";
    default: return m.interp ? "paged_attention_interp" : "paged_attention_chunk";
  }
}

static int paged_attention_chunk_impl(const AttnCall &c, const AttnMode &m) {
  const char *entry = "paged_attention_chunk";
  if (c.batch < 0 || c.q_len < 0 || c.heads < 0 || c.kv_heads < 0 || c.head_dim < 0)
    return set_error(KVECC_EINVAL, "paged_attention_chunk: negative size");
  // the mode's legal combinations (the entries have checked their own codec and buffer first)
  const bool windowed = m.kind == AttnKind::windowed;  // (its entry has checked window >= 1 and sinks >= 0)
  const bool counts = m.kind != AttnKind::plain && !windowed;
  if (counts != (m.stats != nullptr) || (m.kind == AttnKind::golay_counted && m.interp) || (windowed && m.interp))
    return set_error(KVECC_EINVAL, "%s: illegal mode (kind %d, interp %d, stats %s)", mode_entry(m), (int)m.kind,
                     (int)m.interp, m.stats ? "set" : "null");
  int codec = c.codec;
  if (counts && m.kind != AttnKind::golay_counted && codec != KVECC_CODEC_H84)
    return set_error(KVECC_EINVAL, "paged_attention_stats: codec %d (the counted kernels need hamming84)", codec);
  if (m.interp && codec != KVECC_CODEC_H84)
    return set_error(KVECC_EINVAL, "paged_attention_interp: codec %d (interpolation needs hamming84)", codec);
  if (c.batch == 0 || c.q_len == 0 || c.heads == 0) return KVECC_OK;
  if (c.q_sb < 0 || c.q_st < 0 || c.q_sh < 0 || (c.heads > 1 && c.q_sh < c.head_dim) ||
      (c.q_len > 1 && c.q_st < c.head_dim))
    return set_error(KVECC_EINVAL, "paged_attention_chunk: query strides (%lld, %lld, %lld) for head_dim %lld",
                     (long long)c.q_sb, (long long)c.q_st, (long long)c.q_sh, (long long)c.head_dim);
  // one token per sequence, [B, H, D] in place: the decode entry, its kernels and its bits
  // (a ragged call stays here: the decode entry knows no spans)
  // (a windowed call stays here too: the decode entry knows no window)
  if (!m.interp && !counts && !windowed && !c.q_spans && c.q_len == 1 && (c.heads == 1 || c.q_sh == c.head_dim) &&
      (c.batch == 1 || c.q_sb == c.heads * c.head_dim))
    return paged_attention_decode(c);
  const int64_t vbatch = c.batch * c.q_len;  // query rows per head: the virtual batch
  ByteChunkArgs a;  // RaggedArgs for every other codec's kernels; a mode's own block is a copy, below
  AttnPlan p;
  const int rc = attn_setup(entry, c, codec, a, p, [&](ByteChunkArgs &a, bool fits, int64_t max_context_len, AttnPlan &p) {
    if (m.interp && !fits)
      return set_error(KVECC_EINVAL, "paged_attention_interp: caches of 4 GiB or more are not supported");
    if (counts && !fits)
      return set_error(KVECC_EINVAL, "%s: caches of 4 GiB or more are not supported", mode_entry(m));
    p.gq = attn_heads_per_wg(codec, c.head_dim, a.g, c.heads, c.kv_heads, fits);
    // q_len 1 reaches here with a strided query only: the split kernels (and the decode entry's workspace bound);
    // an interpolating call takes its matrix-core kernels at q_len 1 too (one tile, the same bound: `finest`)
    // (a counted call takes its matrix-core kernels at every q_len too)
    p.gm = c.q_len > 1 || m.interp || counts
               ? attn_chunk_mfma_heads(codec, c.q_dtype, c.query, c.q_sb, c.q_st, c.q_sh, c.head_dim, c.heads,
                                       c.kv_heads, fits)
               : 0;
    // (a counted Golay decode step without GQA stays on the split kernels, as the decode entry's does: attn_mfma_heads)
    if (m.kind == AttnKind::golay_counted && c.q_len == 1 && c.heads == c.kv_heads) p.gm = 0;
    int64_t wgs = 0;  // workgroups per split
    if (p.gm) {
      for (a.cg_log2 = 0; (1 << a.cg_log2) < p.gm; ++a.cg_log2) {}
      p.tiles = cdiv(c.q_len, 16 / p.gm);
      wgs = c.batch * (c.heads / p.gm) * p.tiles;
      if (c.batch * (c.heads / p.gm) > kMaxGridY) p.gm = 0;  // the split kernels slice their grid
    }
    if (!p.gm) {
      a.cg_log2 = 0;
      wgs = vbatch * c.heads / p.gq;
      if (c.heads / p.gq > kMaxGridY)
        return set_error(KVECC_EINVAL, "paged_attention_chunk: %lld heads exceed the grid", (long long)c.heads);
    }
    const int64_t finest = c.q_len > 1
                               ? chunk_finest_split(vbatch * c.heads, max_context_len)
                               : choose_split(std::max<int64_t>(1, c.batch * c.heads / 4), max_context_len);
    a.split = std::max(choose_split(wgs, max_context_len,
                                    !p.gm                      ? 4
                                    : codec != KVECC_CODEC_H84 ? kMfmaGolayWgPerCu
                                                               : kMfmaWgPerCu),
                       finest);
    // the counted combine as in the decode entry: one query head per workgroup of the split kernels
    // (a windowed call launches the combine: its empty splits leave before the count)
    p.ctr = !p.gm && p.gq == 1 && vbatch * c.heads <= kAttnCtrPerSlot && !windowed;
    return (int)KVECC_OK;
  });
  if (rc != KVECC_OK) return rc;
  // A windowed call plans its grid by the window (WindowArgs): sink_splits splits in place, then
  // enough to span a workgroup's window from wherever it starts -- window + split - 1 keys, and the
  // 15 further positions of a tile's later tokens -- at the split size the launcher would pick for a
  // context of that many keys.  The partials must fit what the contract requires of the workspace --
  // kvecc_paged_attention_chunk_workspace for this call, the dense plan's bound, NOT the capacity the
  // caller happens to pass (a cached, grown buffer would otherwise change the plan, and with it the
  // summation order, from one call to the next): the split doubles until they do.  Where that is no
  // fewer splits than the dense plan, the dense plan (attn_setup's) stands: sink_splits == nsplit.
  uint32_t sink_splits = (uint32_t)a.nsplit;
  if (windowed) {
    const int64_t need = kvecc_paged_attention_chunk_workspace(
        c.batch, c.q_len, c.heads, c.head_dim, c.max_context_len <= 0 ? c.max_blocks * c.block_size : c.max_context_len);
    const int64_t rows = vbatch * c.heads, sinks = std::min<int64_t>(m.sinks, a.ctx_cap);
    const int64_t span = m.window + (p.gm ? 15 : 0);
    const int64_t wgs = p.gm ? c.batch * (c.heads / p.gm) * p.tiles : vbatch * c.heads / p.gq;
    const int per_cu = !p.gm ? 4 : codec != KVECC_CODEC_H84 ? kMfmaGolayWgPerCu : kMfmaWgPerCu;
    for (int64_t split = choose_split(wgs, std::min<int64_t>(a.ctx_cap, sinks + span), per_cu);; split <<= 1) {
      const int64_t ss = cdiv(sinks, split), n = ss + cdiv(span + split - 1, split);
      if (n >= cdiv(a.ctx_cap, split)) break;
      if (n <= kMaxSplits && rows * n * (c.head_dim + 2) <= need) {
        a.split = split;
        a.nsplit = n;
        sink_splits = (uint32_t)ss;
        break;
      }
      if (split >= kMaxSplit) break;
    }
  }
  hipStream_t st = as_stream(c.stream);
  // the block the mode's kernels take, then its matrix-core tiles or the general path
  auto run = [&](auto b) {
    using B = decltype(b);
    if constexpr (!is_byte<B>) static_cast<RaggedArgs &>(b) = a;
    if constexpr (is_stats<B> || is_repair<B>) b.stats = m.stats;
    if constexpr (is_window<B>) {  // one block for every codec: the byte table by its selector
      b.window = (uint32_t)std::min<int64_t>(m.window, 0x7FFFFFFF);
      b.sinks = (uint32_t)std::min<int64_t>(m.sinks, 0x7FFFFFFF);
      b.tab = a.tab;
      b.sink_splits = sink_splits;
    }
    if (p.gm) return launch_tiles(mode_entry(m), codec, b, c.batch, p.tiles, st);
    return with_q_dtype(mode_entry(m), c.q_dtype, [&](auto t) {
      return launch_rows<typename decltype(t)::type>(mode_entry(m), codec, b, vbatch, p.gq, st);
    });
  };
  const bool bytes = c.codec == KVECC_CODEC_NONE || c.codec == KVECC_CODEC_H74;
  int lrc;
  switch (m.kind) {
    case AttnKind::golay_counted: lrc = run(StatsArgs{}); break;
    case AttnKind::repair: lrc = m.interp ? run(RepairInterpArgs{}) : run(RepairArgs{}); break;
    case AttnKind::counted: lrc = m.interp ? run(StatsInterpArgs{}) : run(StatsArgs{}); break;
    case AttnKind::windowed: lrc = run(WindowArgs{}); break;
    default: lrc = m.interp ? run(InterpArgs{}) : bytes ? run(a) : run(RaggedArgs{}); break;
  }
  if (lrc != KVECC_OK) return lrc;
  return check_launch("paged_attention_chunk");
}

}  // namespace kvecc

using namespace kvecc;

extern "C" {

KVECC_API int64_t kvecc_paged_attention_workspace(int64_t batch, int64_t heads, int64_t head_dim,
                                                  int64_t max_context_len) {
  if (batch <= 0 || heads <= 0 || head_dim <= 0 || max_context_len <= 0) return 0;
  // the GQA kernels split finer (their grid has H/G workgroups per split):
  // room for the finest, G = 4 (choose_split is monotone in its first argument)
  const int64_t bh = std::max<int64_t>(1, batch * heads / 4);
  return batch * heads * cdiv(max_context_len, choose_split(bh, max_context_len)) * (head_dim + 2);
}

KVECC_API int kvecc_paged_attention(const void *query, int q_dtype, const void *k_cache,
                                    const void *v_cache, const int32_t *block_table,
                                    const int32_t *context_lens, const float *k_scales,
                                    const float *v_scales, void *out, int64_t batch,
                                    int64_t heads, int64_t kv_heads, int64_t head_dim,
                                    int64_t num_blocks, int64_t num_layers, int64_t layer, int64_t block_size,
                                    int64_t max_blocks, int64_t max_context_len, float sm_scale,
                                    int codec, float *workspace, int64_t workspace_floats,
                                    void *stream) {
  return paged_attention_decode({query, heads * head_dim, heads * head_dim, head_dim, q_dtype, k_cache, v_cache,
                                 block_table, context_lens, nullptr, k_scales, v_scales, out, batch, 1, heads,
                                 kv_heads, head_dim, num_blocks, num_layers, layer, block_size, max_blocks,
                                 max_context_len, sm_scale, codec, workspace, workspace_floats, stream});
}

KVECC_API int64_t kvecc_paged_attention_chunk_workspace(int64_t batch, int64_t q_len, int64_t heads,
                                                        int64_t head_dim, int64_t max_context_len) {
  if (batch < 0 || q_len < 0 || heads < 0 || head_dim < 0) {
    set_error(KVECC_EINVAL, "paged_attention_chunk_workspace: negative size");
    return KVECC_EINVAL;
  }
  if (batch == 0 || q_len == 0 || heads == 0 || head_dim == 0 || max_context_len <= 0) return 0;
  if (q_len == 1) return kvecc_paged_attention_workspace(batch, heads, head_dim, max_context_len);
  const int64_t rows = batch * q_len * heads;
  return rows * cdiv(max_context_len, chunk_finest_split(rows, max_context_len)) * (head_dim + 2);
}

KVECC_API int kvecc_paged_attention_chunk(const void *query, int64_t q_batch_stride,
                                          int64_t q_token_stride, int64_t q_head_stride, int q_dtype,
                                          const void *k_cache, const void *v_cache,
                                          const int32_t *block_table, const int32_t *context_lens,
                                          const float *k_scales, const float *v_scales, void *out,
                                          int64_t batch, int64_t q_len, int64_t heads, int64_t kv_heads,
                                          int64_t head_dim, int64_t num_blocks, int64_t num_layers,
                                          int64_t layer, int64_t block_size, int64_t max_blocks,
                                          int64_t max_context_len, float sm_scale, int codec,
                                          float *workspace, int64_t workspace_floats, void *stream) {
  return paged_attention_chunk_impl({query, q_batch_stride, q_token_stride, q_head_stride, q_dtype, k_cache, v_cache,
                                     block_table, context_lens, nullptr, k_scales, v_scales, out, batch, q_len, heads,
                                     kv_heads, head_dim, num_blocks, num_layers, layer, block_size, max_blocks,
                                     max_context_len, sm_scale, codec, workspace, workspace_floats, stream},
                                    {});
}

KVECC_API int kvecc_paged_attention_chunk_ragged(const void *query, int64_t q_batch_stride,
                                                 int64_t q_token_stride, int64_t q_head_stride, int q_dtype,
                                                 const void *k_cache, const void *v_cache,
                                                 const int32_t *block_table, const int32_t *context_lens,
                                                 const int32_t *q_spans, const float *k_scales,
                                                 const float *v_scales, void *out, int64_t batch,
                                                 int64_t q_max, int64_t heads, int64_t kv_heads,
                                                 int64_t head_dim, int64_t num_blocks, int64_t num_layers,
                                                 int64_t layer, int64_t block_size, int64_t max_blocks,
                                                 int64_t max_context_len, float sm_scale, int codec,
                                                 float *workspace, int64_t workspace_floats, void *stream) {
  if (!q_spans) return set_error(KVECC_EINVAL, "paged_attention_chunk_ragged: null q_spans");
  return paged_attention_chunk_impl({query, q_batch_stride, q_token_stride, q_head_stride, q_dtype, k_cache, v_cache,
                                     block_table, context_lens, q_spans, k_scales, v_scales, out, batch, q_max, heads,
                                     kv_heads, head_dim, num_blocks, num_layers, layer, block_size, max_blocks,
                                     max_context_len, sm_scale, codec, workspace, workspace_floats, stream},
                                    {});
}

KVECC_API int kvecc_paged_attention_window(const void *query, int64_t q_batch_stride, int64_t q_token_stride,
                                           int64_t q_head_stride, int q_dtype, const void *k_cache,
                                           const void *v_cache, const int32_t *block_table,
                                           const int32_t *context_lens, const int32_t *q_spans,
                                           const float *k_scales, const float *v_scales, void *out,
                                           int64_t batch, int64_t q_max, int64_t heads, int64_t kv_heads,
                                           int64_t head_dim, int64_t num_blocks, int64_t num_layers,
                                           int64_t layer, int64_t block_size, int64_t max_blocks,
                                           int64_t max_context_len, float sm_scale, int codec, int64_t window,
                                           int64_t sinks, float *workspace, int64_t workspace_floats,
                                           void *stream) {
  if (window < 0 || sinks < 0)
    return set_error(KVECC_EINVAL, "paged_attention_window: negative window %lld or sinks %lld", (long long)window,
                     (long long)sinks);
  // No window, or one that covers every key a row can see (its key limit is at most ctx_cap =
  // min(max_context_len, max_blocks * block_size)): the plain entry, its kernels and its bits.
  const int64_t table_cap = max_blocks > 0 && block_size > 0 ? max_blocks * block_size : 0;
  const int64_t ctx_cap = max_context_len > 0 ? std::min(max_context_len, table_cap) : table_cap;
  AttnMode m;
  if (window > 0 && window < ctx_cap) {
    m.kind = AttnKind::windowed;
    m.window = window;
    m.sinks = sinks;
  }
  return paged_attention_chunk_impl({query, q_batch_stride, q_token_stride, q_head_stride, q_dtype, k_cache, v_cache,
                                     block_table, context_lens, q_spans, k_scales, v_scales, out, batch, q_max, heads,
                                     kv_heads, head_dim, num_blocks, num_layers, layer, block_size, max_blocks,
                                     max_context_len, sm_scale, codec, workspace, workspace_floats, stream},
                                    m);
}

KVECC_API int kvecc_paged_attention_interp(const void *query, int64_t q_batch_stride, int64_t q_token_stride,
                                           int64_t q_head_stride, int q_dtype, const void *k_cache,
                                           const void *v_cache, const int32_t *block_table,
                                           const int32_t *context_lens, const int32_t *q_spans,
                                           const float *k_scales, const float *v_scales, void *out,
                                           int64_t batch, int64_t q_max, int64_t heads, int64_t kv_heads,
                                           int64_t head_dim, int64_t num_blocks, int64_t num_layers,
                                           int64_t layer, int64_t block_size, int64_t max_blocks,
                                           int64_t max_context_len, float sm_scale, int codec,
                                           float *workspace, int64_t workspace_floats, void *stream) {
  return paged_attention_chunk_impl({query, q_batch_stride, q_token_stride, q_head_stride, q_dtype, k_cache, v_cache,
                                     block_table, context_lens, q_spans, k_scales, v_scales, out, batch, q_max, heads,
                                     kv_heads, head_dim, num_blocks, num_layers, layer, block_size, max_blocks,
                                     max_context_len, sm_scale, codec, workspace, workspace_floats, stream},
                                    {AttnKind::plain, true});
}

KVECC_API int kvecc_paged_attention_stats(const void *query, int64_t q_batch_stride, int64_t q_token_stride,
                                          int64_t q_head_stride, int q_dtype, const void *k_cache,
                                          const void *v_cache, const int32_t *block_table,
                                          const int32_t *context_lens, const int32_t *q_spans,
                                          const float *k_scales, const float *v_scales, void *out,
                                          int64_t batch, int64_t q_max, int64_t heads, int64_t kv_heads,
                                          int64_t head_dim, int64_t num_blocks, int64_t num_layers,
                                          int64_t layer, int64_t block_size, int64_t max_blocks,
                                          int64_t max_context_len, float sm_scale, int codec, int interp,
                                          uint64_t *stats, float *workspace, int64_t workspace_floats,
                                          void *stream) {
  if (!stats) return set_error(KVECC_EINVAL, "paged_attention_stats: null stats");
  if (codec != KVECC_CODEC_H84)
    return set_error(KVECC_EINVAL, "paged_attention_stats: codec %d (the counted kernels need hamming84)", codec);
  return paged_attention_chunk_impl({query, q_batch_stride, q_token_stride, q_head_stride, q_dtype, k_cache, v_cache,
                                     block_table, context_lens, q_spans, k_scales, v_scales, out, batch, q_max, heads,
                                     kv_heads, head_dim, num_blocks, num_layers, layer, block_size, max_blocks,
                                     max_context_len, sm_scale, codec, workspace, workspace_floats, stream},
                                    {AttnKind::counted, interp != 0, stats});
}

KVECC_API int kvecc_paged_attention_repair(const void *query, int64_t q_batch_stride, int64_t q_token_stride,
                                           int64_t q_head_stride, int q_dtype, void *k_cache, void *v_cache,
                                           const int32_t *block_table, const int32_t *context_lens,
                                           const int32_t *q_spans, const float *k_scales,
                                           const float *v_scales, void *out, int64_t batch, int64_t q_max,
                                           int64_t heads, int64_t kv_heads, int64_t head_dim,
                                           int64_t num_blocks, int64_t num_layers, int64_t layer,
                                           int64_t block_size, int64_t max_blocks, int64_t max_context_len,
                                           float sm_scale, int codec, int interp, uint64_t *stats,
                                           float *workspace, int64_t workspace_floats, void *stream) {
  if (!stats) return set_error(KVECC_EINVAL, "paged_attention_repair: null stats");
  if (codec != KVECC_CODEC_H84)
    return set_error(KVECC_EINVAL, "paged_attention_repair: codec %d (the repairing kernels need hamming84)", codec);
  return paged_attention_chunk_impl({query, q_batch_stride, q_token_stride, q_head_stride, q_dtype, k_cache, v_cache,
                                     block_table, context_lens, q_spans, k_scales, v_scales, out, batch, q_max, heads,
                                     kv_heads, head_dim, num_blocks, num_layers, layer, block_size, max_blocks,
                                     max_context_len, sm_scale, codec, workspace, workspace_floats, stream},
                                    {AttnKind::repair, interp != 0, stats});
}

KVECC_API int kvecc_paged_attention_golay_stats(const void *query, int64_t q_batch_stride, int64_t q_token_stride,
                                                int64_t q_head_stride, int q_dtype, const void *k_cache,
                                                const void *v_cache, const int32_t *block_table,
                                                const int32_t *context_lens, const int32_t *q_spans,
                                                const float *k_scales, const float *v_scales, void *out,
                                                int64_t batch, int64_t q_max, int64_t heads, int64_t kv_heads,
                                                int64_t head_dim, int64_t num_blocks, int64_t num_layers,
                                                int64_t layer, int64_t block_size, int64_t max_blocks,
                                                int64_t max_context_len, float sm_scale, int codec,
                                                uint64_t *stats, float *workspace, int64_t workspace_floats,
                                                void *stream) {
  if (!stats) return set_error(KVECC_EINVAL, "paged_attention_golay_stats: null stats");
  if (codec != KVECC_CODEC_GOLAY && codec != KVECC_CODEC_GOLAY_PACKED)
    return set_error(KVECC_EINVAL, "paged_attention_golay_stats: codec %d (these counted kernels need golay or golay_packed)",
                     codec);
  return paged_attention_chunk_impl({query, q_batch_stride, q_token_stride, q_head_stride, q_dtype, k_cache, v_cache,
                                     block_table, context_lens, q_spans, k_scales, v_scales, out, batch, q_max, heads,
                                     kv_heads, head_dim, num_blocks, num_layers, layer, block_size, max_blocks,
                                     max_context_len, sm_scale, codec, workspace, workspace_floats, stream},
                                    {AttnKind::golay_counted, false, stats});
}

}  // extern "C"
