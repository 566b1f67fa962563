/*
 * kvecc.h -- C ABI of the MI355X-native ECC KV-cache codec (libkvecc.so).
 *
 * This is the drop-in boundary for the reference's hot path,
 * ecc_codecs/triton_kernels/ (Hamming(7,4)/(8,4), Golay(24,12), Bernoulli bit
 * flip injection, double-error interpolation, fused quantize/encode and
 * decode/dequantize).  The reference exposes these as Python functions over
 * torch tensors; each entry point below replaces the Triton kernel + wrapper
 * cited next to it (paths relative to the reference repository root).  The
 * Python host package `kvecc` binds them with ctypes.
 *
 * Conventions (all entry points):
 *   - Pointers are DEVICE pointers (hipMalloc / torch CUDA tensors) unless the
 *     name ends in _host.  Buffers must not overlap unless stated.
 *   - `stream` is a hipStream_t (NULL = legacy default stream).  Calls only
 *     enqueue work: no allocation, no host synchronisation (graph-capturable
 *     once kvecc_init_device() has run for the device).
 *   - Statistics accumulate (+=) into a caller-provided, zero-initialised device
 *     buffer of KVECC_STATS_WORDS uint64 words, or are skipped when the pointer
 *     is NULL.  The buffer is sharded: workgroup g adds its partial sums to
 *     slot (g % KVECC_STATS_SLOTS), one 128-byte line per slot, and statistic k
 *     (the "stats[k]" named below) is  sum over s of buf[s*KVECC_STATS_STRIDE + k].
 *     (Thousands of device-scope atomics on ONE address serialise at ~10 ns
 *     each -- longer than the kernels themselves.)
 *   - Return 0 on success, a negative KVECC_E* code on failure; the message is
 *     available from kvecc_last_error() (thread-local).
 *   - n / m / rows == 0 is valid and enqueues nothing.
 */
#ifndef KVECC_H
#define KVECC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KVECC_API __attribute__((visibility("default")))

enum {
  KVECC_OK = 0,
  KVECC_EINVAL = -1, /* bad argument (null pointer, negative size, bad enum) */
  KVECC_EHIP = -2,   /* HIP runtime error (launch / memory)                  */
  KVECC_ENODEV = -3  /* no HIP device                                         */
};

/* statistics buffer geometry (see conventions above) */
#define KVECC_STATS_SLOTS 32
#define KVECC_STATS_STRIDE 16 /* uint64 words per slot = one 128-B line */
#define KVECC_STATS_WORDS (KVECC_STATS_SLOTS * KVECC_STATS_STRIDE)

/* dtype codes for fused kernels */
enum { KVECC_F32 = 0, KVECC_F16 = 1, KVECC_BF16 = 2 };
/* codec codes for fused kernels */
enum { KVECC_CODEC_NONE = 0, KVECC_CODEC_H74 = 1, KVECC_CODEC_H84 = 2, KVECC_CODEC_GOLAY = 3,
       /* shim caches only (kvecc_shim_write / kvecc_shim_read and the cpu twins):
        * Golay(24,12) codewords stored as 3 little-endian bytes, a token row of
        * g = ceil(d/3) codewords padded to KVECC_GOLAY_PACKED_ROW(g) bytes --
        * 132 B instead of the reference's 172 B (int32) at d = 128 */
       KVECC_CODEC_GOLAY_PACKED = 4 };
#define KVECC_GOLAY_PACKED_ROW(g) ((3 * (g) + 3) / 4 * 4)

/* Row scale rule of the INT4 quantizer.  The reference computes
 * `abs_max / 7.0` with a Python-scalar divisor (paged_cache_ecc.py:330); torch
 * evaluates that as IEEE division on CPU tensors but as abs_max * RN(1/7) on
 * GPU tensors (its CPU-scalar-divisor shortcut), and the two differ in ~55% of
 * rows.  DIV7 reproduces the reference run on the CPU (the golden fixtures),
 * MUL_INV7 the reference run on a GPU.  q = x / scale is IEEE under both. */
enum { KVECC_SCALE_DIV7 = 0, KVECC_SCALE_MUL_INV7 = 1 };

/* ---- runtime --------------------------------------------------------------- */
KVECC_API const char *kvecc_version(void);
KVECC_API const char *kvecc_last_error(void);
KVECC_API int kvecc_device_count(void);
/* Kernel timing without marker packets: the NEXT kernel this thread launches
 * through any kvecc_* device entry point records its own start and end into
 * the given hipEvent_t's (either may be NULL) via hipExtLaunchKernel, then the
 * hook disarms.  Entry points that launch a main kernel and a tail kernel time
 * the first one.  The reference has no counterpart (benchmark_harness.py:42-57
 * brackets launches with events); bench.py uses this to time every step. */
KVECC_API int kvecc_time_next_launch(void *start_event, void *stop_event);
/* Upload the Golay tables to `device` (done lazily otherwise; call before graph
 * capture).  Replaces golay_triton.py:304-330 (_build_syndrome_table cache). */
KVECC_API int kvecc_init_device(int device);
/* Work / split counters of the dynamically scheduled kernels (the fused shim
 * reads, the per-head Golay rows, the packed decodes, the paged-attention fused
 * combine).  No reference counterpart: the reference launches one program per
 * row and schedules nothing.  Each kernel needs its counters zero and to itself
 * while it runs, and leaves them zero.  The library gives eager launches one
 * counter slot per stream (per thread for hipStreamPerThread; keyed by the
 * stream's address -- a stream created at a destroyed stream's address inherits
 * its slot, safe because hipStreamDestroy drains the queue first), and
 * launches captured into a graph a slot of their own per (capture, stream), so
 * launches that can overlap never share counters.  Slots (48 KiB each) come
 * from a pool that grows from eager launches only (never inside the launching
 * stream's own capture): every eager launch of such a kernel tops the free list
 * back up to 32 slots, so 32 captures can follow any eager launch;
 * kvecc_reserve_counter_slots(device, n) makes n more available ahead of a
 * longer run of captures.  Growth allocates in relaxed capture mode, so an
 * eager launch beside another stream's global-mode capture (torch.cuda.graph's
 * default) neither fails nor invalidates that capture.  A captured slot is tied to its graph by
 * a HIP user object and returns to the pool when the graph and all its
 * executable instances are destroyed.  A graph keeps its slots for every
 * replay: replay one graph on one stream at a time (two overlapping replays of
 * the same graph would share counters). */
KVECC_API int kvecc_reserve_counter_slots(int device, int n);
/* Diagnostic (synchronises the device): slots handed out, and how many counter
 * words of all slots are non-zero -- 0 whenever no launch is in flight. */
KVECC_API int kvecc_counter_slots_check(int device, int64_t *slots_in_use, int64_t *nonzero_words);
/* Test hook: on != 0 makes the step that ties a captured launch's slot to its
 * graph fail (as hipGraphRetainUserObject might); such a slot then stays with
 * its capture for the life of the process instead of returning to the pool. */
KVECC_API int kvecc_debug_fail_graph_retain(int on);
/* Host copies of the code tables the kernels use (for verification):
 *   syndrome table as the reference builds it, config.py:403-457 -> int32[4096]
 *   H row masks, config.py:354-379 -> uint32[12]                              */
KVECC_API int kvecc_golay_syndrome_table_host(int32_t *out4096);
KVECC_API int kvecc_golay_h_row_masks_host(uint32_t *out12);
/* Integer form of the reference's `tl.rand(..) < ber` test (random.py:126-143):
 * the smallest folded 31-bit value x with fp32(x)*0x2FFFFFFF >= fp32(ber). */
KVECC_API uint32_t kvecc_ber_threshold(float ber);

/* ---- Hamming(7,4) / Hamming(8,4) ------------------------------------------ */
/* hamming74_triton.py:48-91 + :170-201 */
KVECC_API int kvecc_hamming74_encode(const uint8_t *in, uint8_t *out, int64_t n, void *stream);
/* hamming74_triton.py:100-162 + :218-277 ; stats[0] += #syndrome != 0 */
KVECC_API int kvecc_hamming74_decode(const uint8_t *cw, uint8_t *data, uint8_t *flag,
                                     int64_t n, uint64_t *stats, void *stream);
/* hamming84_triton.py:50-108 + :217-254 */
KVECC_API int kvecc_hamming84_encode(const uint8_t *in, uint8_t *out, int64_t n, void *stream);
/* hamming84_triton.py:117-209 + :281-351 ; error_type may be NULL;
 * stats[0] += #SINGLE_CORRECTED, stats[1] += #DOUBLE_DETECTED */
KVECC_API int kvecc_hamming84_decode(const uint8_t *cw, uint8_t *data, uint8_t *error_type,
                                     int64_t n, uint64_t *stats, void *stream);

/* ---- Golay(24,12) ------------------------------------------------------------ */
/* golay_triton.py:99-157 + :382-422 ; triplets uint8[m][3] -> int32[m] */
KVECC_API int kvecc_golay_encode(const uint8_t *triplets, int32_t *codewords, int64_t m,
                                 void *stream);
/* golay_triton.py:213-295 + :425-498 ; counts may be NULL;
 * stats[0] += sum of counts < 4 (bits corrected), stats[1] += #count == 4 */
KVECC_API int kvecc_golay_decode(const int32_t *codewords, uint8_t *triplets, uint8_t *counts,
                                 int64_t m, uint64_t *stats, void *stream);
/* Per-head packing of the shim (ecc_shim.py:623-624,669-682): each row of d
 * nibbles is zero-padded to 3*ceil(d/3) and encoded to ceil(d/3) codewords. */
KVECC_API int kvecc_golay_encode_rows(const uint8_t *nibbles, int32_t *codewords, int64_t rows,
                                      int64_t d, void *stream);
/* Inverse of the above (ecc_shim.py:990-1008): decoded rows of d nibbles. */
KVECC_API int kvecc_golay_decode_rows(const int32_t *codewords, uint8_t *nibbles,
                                      int64_t rows, int64_t d, uint64_t *stats, void *stream);

/* ---- Bernoulli bit-flip injection ------------------------------------------- */
/* fault_injection_triton.py:228-299 (uint8) and :303-334 (int32), wrapper
 * :337-424.  Element i is global element offset0+i of a global_n-element flat
 * tensor (pass global_n = n, offset0 = 0 for the unsharded call), so shards
 * reproduce the single-device flip pattern.  counts (uint8 per element) may be
 * NULL; stats[0] += flips, stats[1] += elements with >=1 flip.  in == out is
 * allowed (in-place). */
KVECC_API int kvecc_inject_u8(const uint8_t *in, uint8_t *out, uint8_t *counts, int64_t n,
                              int n_bits, int64_t seed, float ber, int64_t global_n,
                              int64_t offset0, uint64_t *stats, void *stream);
KVECC_API int kvecc_inject_i32(const int32_t *in, int32_t *out, uint8_t *counts, int64_t n,
                               int n_bits, int64_t seed, float ber, int64_t global_n,
                               int64_t offset0, uint64_t *stats, void *stream);
/* rand4x variants, fault_injection_triton.py:57-133 / :137-224 / :434-496 */
KVECC_API int kvecc_inject_u8_vectorized(const uint8_t *in, uint8_t *out, uint8_t *counts,
                                         int64_t n, int n_bits, int64_t seed, float ber,
                                         uint64_t *stats, void *stream);
KVECC_API int kvecc_inject_i32_vectorized(const int32_t *in, int32_t *out, uint8_t *counts,
                                          int64_t n, int n_bits, int64_t seed, float ber,
                                          uint64_t *stats, void *stream);
/* Per-row scheme of the shim (ecc_shim.py:643-651,684-691,713-721): row r
 * (row_len elements, contiguous, rows back to back) is injected as its own
 * call with N = row_len and seed = seed_base + r.  in == out allowed. */
KVECC_API int kvecc_inject_rows_u8(const uint8_t *in, uint8_t *out, int64_t rows,
                                   int64_t row_len, int n_bits, int64_t seed_base, float ber,
                                   uint64_t *stats, void *stream);
KVECC_API int kvecc_inject_rows_i32(const int32_t *in, int32_t *out, int64_t rows,
                                    int64_t row_len, int n_bits, int64_t seed_base, float ber,
                                    uint64_t *stats, void *stream);

/* ---- Interpolation ----------------------------------------------------------- */
/* interpolation_triton.py:120-159 + :162-265 on a contiguous [outer][len][inner]
 * uint8 array whose sequence axis is the middle one (no permute copies).
 * err == 2 elements become round_half_up((q[l-1]+q[l+1])/2) from clamped
 * neighbours, every element is clamped to [0,15] -- unless `gate` is non-NULL
 * and *gate == 0 (device int32), in which case out = q (the reference's
 * no-double fast path, :199-201, decided on the device). */
KVECC_API int kvecc_interpolate(const uint8_t *q, const uint8_t *err, uint8_t *out,
                                int64_t outer, int64_t len, int64_t inner, const int32_t *gate,
                                void *stream);
/* The reference wrapper in full (interpolation_triton.py:162-265) in one pass:
 * out = the interpolated, clamped result when any err == 2, else out = q (its
 * `q.clone()` fast path, :199-201).  No host sync, no separate scan of err and
 * no zeroing pass: the kernel sets flags[0] = epoch if any err == 2 and
 * flags[1] = epoch if any q > 15 (device int32[2]); a trailing copy kernel
 * restores out = q only when flags[0] != epoch and flags[1] == epoch (without
 * doubles, clamping is visible only where q > 15).  `epoch` must be non-zero
 * and differ from both words of `flags` on entry (e.g. a per-buffer call
 * counter); afterwards "flags[k] == epoch" reads as "condition k was seen". */
KVECC_API int kvecc_interpolate_auto(const uint8_t *q, const uint8_t *err, uint8_t *out,
                                     int64_t outer, int64_t len, int64_t inner, int32_t *flags,
                                     int32_t epoch, void *stream);
/* *flag = (any x[i] == value) ? 1 : 0 (device int32, overwritten). */
KVECC_API int kvecc_any_equal_u8(const uint8_t *x, int64_t n, uint8_t value, int32_t *flag,
                                 void *stream);
/* stats[0] += number of positions i < n with a[i] != b[i] (device buffers;
 * sharded statistics buffer as the codecs use).  The codec-level sweep's
 * residual-error count, `(decoded != truth).sum()` in the reference's Monte
 * Carlo (evaluation/experiments/monte_carlo.py:75-395), as one HBM pass. */
KVECC_API int kvecc_count_ne_u8(const uint8_t *a, const uint8_t *b, int64_t n, uint64_t *stats,
                                void *stream);

/* ---- Monte-Carlo trial (BASELINE config 5) ---------------------------------- */
/* One trial of the codec-level fault-injection sweep in one launch: for every
 * value of the ground-truth INT4 tensor x [outer, len, heads, head_dim] (uint8
 * nibbles, contiguous), encode -> Bernoulli flips (the reference's per-bit
 * Philox stream of fault_injection_triton.py:228-334 over the shard's global
 * indices: global_n elements, this shard starting at offset0) -> decode
 * (-> double-error interpolation along `len`) -> compare with x, keeping only
 * the statistics; the codewords and decoded values never reach HBM.  The
 * counterpart of the reference's encode / inject_bit_errors_triton / decode
 * trial (evaluation/experiments/quantization_ecc_comparison.py:164-203,
 * evaluation/sweep.py:352-626) and exactly the counters of that pipeline run
 * kernel by kernel:
 *   stats[0] flips, stats[1] elements with >= 1 flip,
 *   stats[2] corrected (H74: syndrome != 0; H84: single errors; Golay: bits),
 *   stats[3] detected (H74: 0; H84: double errors; Golay: uncorrectable words),
 *   stats[4] decoded (interpolated) values != x.
 * Hamming codecs draw n_bits 7 / 8 per value (global_n, offset0 in values);
 * Golay packs each head row into ceil(head_dim/3) codewords (the shim's
 * per-head padding, ecc_shim.py:623-682) and draws 24 bits per codeword
 * (global_n, offset0 in codewords).  KVECC_MC_H84_INTERP needs heads*head_dim
 * % 4 == 0. */
enum { KVECC_MC_H74 = 1, KVECC_MC_H84 = 2, KVECC_MC_H84_INTERP = 3, KVECC_MC_GOLAY = 4 };
KVECC_API int kvecc_mc_trial(const uint8_t *x, int64_t outer, int64_t len, int64_t heads,
                             int64_t head_dim, int codec, float ber, int64_t seed, int64_t global_n,
                             int64_t offset0, uint64_t *stats, void *stream);
/* dst[b * dst_stride + w] += stats word w summed over the KVECC_STATS_SLOTS
 * slots of buffer b (buffers KVECC_STATS_WORDS apart), for b < nbuf and
 * w < nwords <= KVECC_STATS_STRIDE; the buffers are zeroed afterwards.  One
 * launch folds every trial's counters into the sweep's table. */
KVECC_API int kvecc_stats_fold(uint64_t *stats, int64_t nbuf, int nwords, int64_t *dst,
                               int64_t dst_stride, void *stream);

/* ---- Fused quantize / encode and decode / dequantize ----------------------- */
/* fused_kernels.py:18-160 (H84), :163-269 (H74), and the shim's torch path
 * ecc_shim.py:572-580: per row of d values (dtype x_dtype), scale = absmax/7
 * under `scale_rule` (KVECC_SCALE_*; 0 -> 1), q = rint(x/scale) clamped [-8,7]
 * + 8, then encoded with `codec` (KVECC_CODEC_NONE stores the raw nibble).
 * scales: fp32 per row. */
KVECC_API int kvecc_quantize_encode_rows(const void *x, int x_dtype, int codec, int scale_rule,
                                         uint8_t *cw, float *scales, int64_t rows, int64_t d,
                                         void *stream);
/* fused_kernels.py:272-437 : H84 decode + (q-8)*scale -> out (out_dtype).
 * zero_doubles = 1 reproduces :344 (double-error data -> 0).
 * stats[0] += #SINGLE_CORRECTED, stats[1] += #DOUBLE_DETECTED. */
KVECC_API int kvecc_decode_dequant_h84_rows(const uint8_t *cw, const float *scales, void *out,
                                            int out_dtype, int64_t rows, int64_t d,
                                            int zero_doubles, uint64_t *stats, void *stream);

/* ---- Packed Golay storage (native layout, not the reference's) -- */
/* values as INT4 nibbles two per byte (value j in byte j/2, low nibble first),
 * codewords as 3 little-endian bytes (data12 | parity12 << 12, as
 * golay_triton.py:130-155), so codeword k covers values 3k..3k+2.
 * nibbles: ceil(3m/2) bytes; codewords: 3m bytes; uncorrectable (may be NULL):
 * ceil(m/8) bytes, bit k%8 of byte k/8 = codeword k uncorrectable (data kept);
 * stats[0] += bits corrected, stats[1] += #uncorrectable.  Decode moves 4.625 B
 * per codeword (reference layout: 8), encode 4.5 B (reference: 7). */
KVECC_API int kvecc_golay_encode_packed(const uint8_t *nibbles, uint8_t *codewords, int64_t m,
                                        void *stream);
KVECC_API int kvecc_golay_decode_packed(const uint8_t *codewords, uint8_t *nibbles,
                                        uint8_t *uncorrectable, int64_t m, uint64_t *stats,
                                        void *stream);

/* Hamming(8,4) with packed values: nibbles two per byte (as above), codewords
 * one byte each (the reference's), error types 2 bits per value (value j at
 * bits 2*(j%4) of byte j/4; may be NULL).  stats as kvecc_hamming84_decode.
 * Encode moves 1.5 B/value (reference layout: 2), decode 1.75 (reference: 3). */
KVECC_API int kvecc_hamming84_encode_packed(const uint8_t *nibbles, uint8_t *codewords, int64_t n,
                                            void *stream);
KVECC_API int kvecc_hamming84_decode_packed(const uint8_t *codewords, uint8_t *nibbles,
                                            uint8_t *error_types, int64_t n, uint64_t *stats,
                                            void *stream);

/* ---- ECC shim: KV-cache write and read -------------------------------------- */
/* ecc_shim.py:557-721 (ECCBackend.write) for codec KVECC_CODEC_NONE (int4),
 * H74, H84, GOLAY in ONE launch: K and V [batch, seq, hkv*d] (x_dtype,
 * contiguous) are quantized per (pos, head) row (absmax/7 under scale_rule,
 * round-half-even),
 * encoded, injected with the row's own seed when `inject` and ber > 0
 * (K: seed0 + r, V: seed0 + r + 1, r = (b*seq + pos)*hkv + h; n_bits per
 * codeword as ecc_shim.py:555-560) and stored into the paged caches -- only the
 * last batch, which is what the reference's same-slot writes leave behind.
 * Caches: [blocks, num_layers, hkv, block_size, P] with P = d (uint8) or
 * ceil(d/3) (int32, Golay per-head padding), or KVECC_GOLAY_PACKED_ROW(ceil(d/3))
 * bytes for KVECC_CODEC_GOLAY_PACKED (not a reference layout); scales fp32 [blocks, num_layers,
 * hkv, block_size]; token pos lives in physical block block_table[pos / block_size]
 * (device int32).  d <= 512. */
KVECC_API int kvecc_shim_write(const void *k, const void *v, int x_dtype, int64_t batch,
                               int64_t seq, int64_t hkv, int64_t d, int codec, int scale_rule,
                               int n_bits,
                               int inject, float ber, int64_t seed0, void *k_cache, void *v_cache,
                               float *k_scales, float *v_scales, const int32_t *block_table,
                               int64_t num_layers, int64_t block_size, int64_t layer,
                               void *stream);
/* kvecc_shim_write on strided K/V: element (b, pos, h, e) of K lives at
 * k[b*k_batch_stride + pos*k_seq_stride + h*k_head_stride + e] (same for V;
 * each head's d values contiguous), so the projections' views are read in
 * place -- a slice of GPT-2's fused c_attn output, or Llama's post-RoPE
 * [b, h, s, d] tensor transposed -- where the reference first copies them
 * with .transpose(1, 2).contiguous() (ecc_shim.py:1290-1291, :1351-1352).
 * Strides are >= 0 and head strides >= d. */
KVECC_API int kvecc_shim_write_strided(const void *k, const void *v, int64_t k_batch_stride,
                                       int64_t k_seq_stride, int64_t k_head_stride,
                                       int64_t v_batch_stride, int64_t v_seq_stride,
                                       int64_t v_head_stride, int x_dtype, int64_t batch,
                                       int64_t seq, int64_t hkv, int64_t d, int codec,
                                       int scale_rule, int n_bits, int inject, float ber,
                                       int64_t seed0, void *k_cache, void *v_cache,
                                       float *k_scales, float *v_scales,
                                       const int32_t *block_table, int64_t num_layers,
                                       int64_t block_size, int64_t layer, void *stream);
/* Append-mode write (no reference counterpart: the reference keeps one cache
 * for the whole batch and never grows it): K and V [batch, q_len, hkv, d] by
 * element strides as kvecc_shim_write_strided, quantized, encoded, injected
 * and scattered in ONE launch for EVERY sequence of the batch.  block_table is
 * [batch, table_stride] int32 (row b = sequence b); start_pos is a DEVICE
 * int32 [batch] the host never reads.  Token t of sequence b goes to logical
 * position p = start_pos[b] + t, physical block
 * block_table[b*table_stride + p / block_size], slot p % block_size; caches and
 * scales as kvecc_shim_write.  A row is skipped -- nothing written, nothing read
 * past the table -- when start_pos[b] < 0 (inactive sequence), when
 * p / block_size >= table_stride, or when the block id is negative.  Injection
 * seeds are kvecc_shim_write's: K seed0 + r, V seed0 + r + 1 with the running
 * row r = (b*q_len + t)*hkv + h, and skipped rows keep their r, so sequence b
 * of an append at start_pos 0 holds the bits kvecc_shim_write stores for a
 * batch of b + 1.  Same dtypes, codecs, scale_rule and n_bits clamps as
 * kvecc_shim_write; d <= 512; table_stride >= 1; batch == 0 or q_len == 0
 * enqueues nothing. */
KVECC_API int kvecc_shim_append(const void *k, const void *v, int64_t k_batch_stride,
                                int64_t k_seq_stride, int64_t k_head_stride,
                                int64_t v_batch_stride, int64_t v_seq_stride,
                                int64_t v_head_stride, int x_dtype, int64_t batch, int64_t q_len,
                                int64_t hkv, int64_t d, int codec, int scale_rule, int n_bits,
                                int inject, float ber, int64_t seed0, void *k_cache,
                                void *v_cache, float *k_scales, float *v_scales,
                                const int32_t *block_table, int64_t table_stride,
                                const int32_t *start_pos, int64_t num_layers,
                                int64_t block_size, int64_t layer, void *stream);
/* Query spans (ragged batches; no reference counterpart).  A ragged call keeps
 * the rectangular [batch, q_max, ...] tensors and adds q_spans, an int32
 * [batch, 3] of (first, count, row_base) per sequence: token t of row b is
 * VALID iff first >= 0 and first <= t < min(first + count, q_max), else
 * PADDING (left padding: first = q_max - count; right padding: first = 0; an
 * inactive sequence: count = 0; a full row: (0, q_max)).  A span that overruns
 * q_max is clamped and never read past; a negative first or a count <= 0 makes
 * the whole row padding.  row_base is the exclusive prefix sum of the valid
 * counts before b; only the append reads it.  On the device entries q_spans is
 * a DEVICE pointer the host never reads, on the kvecc_cpu_ twins a host one;
 * null is KVECC_EINVAL.
 *
 * kvecc_shim_append with spans: the arguments are kvecc_shim_append's with
 * q_len read as q_max.  Valid token t of sequence b goes to logical position
 * start_pos[b] + (t - first); a padding token writes nothing (no cache byte,
 * no scale) and its K/V elements are never loaded.  The injection row is dense
 * over the valid tokens, r = (row_base + t - first)*hkv + h (K seed0 + r, V
 * seed0 + r + 1); kvecc_shim_append's skip rules apply to valid tokens, which
 * keep their r.  All spans (0, q_max, b*q_max) write kvecc_shim_append's bits;
 * sequence b of any call holds what a batch-1 kvecc_shim_append of its valid
 * tokens writes with seed0 + row_base*hkv. */
KVECC_API int kvecc_shim_append_ragged(const void *k, const void *v, int64_t k_batch_stride,
                                       int64_t k_seq_stride, int64_t k_head_stride,
                                       int64_t v_batch_stride, int64_t v_seq_stride,
                                       int64_t v_head_stride, int x_dtype, int64_t batch, int64_t q_max,
                                       int64_t hkv, int64_t d, int codec, int scale_rule, int n_bits,
                                       int inject, float ber, int64_t seed0, void *k_cache,
                                       void *v_cache, float *k_scales, float *v_scales,
                                       const int32_t *block_table, int64_t table_stride,
                                       const int32_t *start_pos, const int32_t *q_spans,
                                       int64_t num_layers, int64_t block_size, int64_t layer,
                                       void *stream);
/* ecc_shim.py:990-1071 (ECCBackend.attend, decode side) in ONE launch: gather
 * the first ctx tokens of layer `layer`, decode (H74: stats[0] += #flagged;
 * H84: stats[0] += #SINGLE_CORRECTED, stats[1] += #DOUBLE_DETECTED; Golay:
 * stats[0] += bits corrected, stats[1] += #uncorrectable; stats may be NULL),
 * interpolate H84 double errors along the context when `interp`, dequantize
 * (q - 8) * scale in fp32 and store k_out / v_out as [hkv, ctx, d] in out_dtype
 * (RNE).  Byte codecs need d % 4 == 0. */
KVECC_API int kvecc_shim_read(const void *k_cache, const void *v_cache, const float *k_scales,
                              const float *v_scales, const int32_t *block_table, int64_t ctx,
                              int64_t hkv, int64_t d, int64_t num_layers, int64_t block_size,
                              int64_t layer, int codec, int interp, void *k_out, void *v_out,
                              int out_dtype, uint64_t *stats, void *stream);
/* kvecc_shim_read over `batch` sequences in one call: sequence b reads its first
 * ctx tokens through block_table row b (block_table[b * table_stride + lb],
 * table_stride >= ceil(ctx / block_size)); k_out / v_out are [batch, hkv, ctx,
 * d].  Golay caches with d % 8 == 0 take the wave-tile kernel (one launch for
 * every sequence and both sides; the fused decode BASELINE's north_star
 * measures); the other codecs launch once per sequence.  Every codec reads a
 * negative block id as zero codewords: its rows output +0 (no statistics), and
 * as an H84 interpolation neighbour its values read as decode(0) = 0.  batch 1
 * is kvecc_shim_read. */
KVECC_API int kvecc_shim_read_batch(const void *k_cache, const void *v_cache, const float *k_scales,
                                    const float *v_scales, const int32_t *block_table,
                                    int64_t table_stride, int64_t batch, int64_t ctx, int64_t hkv,
                                    int64_t d, int64_t num_layers, int64_t block_size, int64_t layer,
                                    int codec, int interp, void *k_out, void *v_out, int out_dtype,
                                    uint64_t *stats, void *stream);

/* ---- Paged decode attention with inline ECC decode ---------------------------- */
/* attention_ecc.py:620-780 (paged_attention_ecc) + :265-427 (kernel): one query
 * token per sequence, query [batch, heads, head_dim] (q_dtype), caches as above
 * (codec H84: uint8, double errors keep their data -- kvecc_paged_attention_interp
 * below interpolates them; GOLAY: int32, uncorrectable
 * data kept; GOLAY_PACKED: 3-byte codewords, rows of KVECC_GOLAY_PACKED_ROW bytes), block_table [batch, max_blocks] int32 (-1 = no block, token
 * skipped), context_lens [batch] int32, max_context_len (<= 0 means
 * max_blocks*block_size; a context_len above it, or above the table's
 * max_blocks*block_size, is attended up to that bound, on the device and the
 * host alike), out [batch, heads, head_dim] in q_dtype.  A sequence
 * with no valid token (context_len <= 0 or only -1 blocks) gets the reference's
 * values: -8.0 in every lane for H84 (its kernel's -1e20 masking,
 * attention_ecc.py:342,391-423), 0 for Golay (reference_attention_ecc).  Query head h reads cache head h / (heads / kv_heads).  `workspace`:
 * kvecc_paged_attention_workspace(...) floats.  head_dim <= 256.
 *
 * Scale range (every attention entry of this header, device and host).  Scales
 * are non-negative finite floats; a scale of exactly 0 (an unwritten slot of a
 * zeroed cache) gives its token the value 0, and a sequence whose V scales are all
 * 0 returns exactly 0.  The accuracy of the output relative to the largest
 * v_scale of a sequence does not depend on that scale's magnitude anywhere
 * between 2^-100 and 2^100: the matrix-core kernels (fp16 queries) carry
 * p * v_scale to the matrix cores divided by a running power of two, kept in the
 * online-softmax state and clamped to [2^-100, 2^100], and every other kernel
 * works in fp32 throughout.  What bounds a call is its output type, not the
 * kernels: an output above the largest finite value of q_dtype is +-inf and one
 * below its smallest subnormal is 0 (fp16: 65504 and 2^-24, so v_scales between
 * about 2^-12 and 2^13 keep fp16 outputs normal and finite).  Weights below 2^-100
 * lose precision gradually, far below anything an output type can hold.
 * k_scales enter the scores only, in fp32.  Negative, infinite and NaN scales are
 * undefined (the writers never produce them).
 *
 * Byte caches without SECDED (no reference counterpart: the reference attends
 * over Hamming(8,4) and Golay only).  kvecc_paged_attention,
 * kvecc_paged_attention_chunk, kvecc_paged_attention_chunk_ragged and their
 * kvecc_cpu_ twins also take KVECC_CODEC_H74 and KVECC_CODEC_NONE caches, which
 * share H84's layout (uint8, one value per byte, rows of head_dim bytes).  A
 * stored byte b is worth (data(b) - 8) * scale:
 *   - H74:  data(b) is h74_decode4's nibble -- bit 7 is ignored and a double
 *           error is miscorrected, as everywhere in the library;
 *   - NONE: data(b) = b & 0xF.
 * Everything else follows H84's rules: head_dim % 4 == 0 and head_dim <= 256,
 * the query dtypes, the GQA map, -1 blocks, the max_context_len clamp, and the
 * empty value, -8.0 in every lane (the kernels share H84's body, and no
 * reference defines another value for these codecs).  The launch geometry is
 * H84's at the same shape, so a clean cache of either codec returns the bits
 * an H84 cache of the same nibbles returns.  The workspace functions are
 * unchanged.  kvecc_paged_attention_interp keeps rejecting everything but H84.
 * A deliberate difference: kvecc_shim_read dequantizes a NONE byte raw (all 8
 * bits, unmasked), the attention kernels read its low nibble.  The two agree on
 * every byte the write, the 4-bit injection and a 4-bit ageing can produce
 * (b < 16) and differ only on bytes nothing in the library stores. */
KVECC_API int64_t kvecc_paged_attention_workspace(int64_t batch, int64_t heads, int64_t head_dim,
                                                  int64_t max_context_len);
KVECC_API int kvecc_paged_attention(const void *query, int q_dtype, const void *k_cache,
                                    const void *v_cache, const int32_t *block_table,
                                    const int32_t *context_lens, const float *k_scales,
                                    const float *v_scales, void *out, int64_t batch,
                                    int64_t heads, int64_t kv_heads, int64_t head_dim,
                                    int64_t num_blocks, int64_t num_layers, int64_t layer, int64_t block_size,
                                    int64_t max_blocks, int64_t max_context_len, float sm_scale,
                                    int codec, float *workspace, int64_t workspace_floats,
                                    void *stream);

/* Chunked causal form: q_len query tokens per sequence (a prefill, a chunk of
 * one, the draft tokens of a verify step) against the same caches, which
 * already hold the chunk's own tokens: context_lens[b] counts them.  Query
 * element (b, t, h, e) is query[b*q_batch_stride + t*q_token_stride +
 * h*q_head_stride + e] (strides in elements, >= 0; head and token strides >=
 * head_dim), so [batch, heads, q_len, d] and [batch, q_len, heads*d] tensors
 * are both read in place; out is contiguous [batch, q_len, heads, head_dim] in
 * q_dtype.  Query t of sequence b sits at position p = context_lens[b] - q_len
 * + t and attends to the keys j with 0 <= j <= p and j < min(max_context_len,
 * max_blocks*block_size); -1 blocks are skipped.  A row without a valid key
 * (p < 0, or only -1 blocks at or before p) gets the decode entry's empty
 * value, per row.  Codecs, dtypes, head_dim domain, GQA mapping and argument
 * checks are kvecc_paged_attention's; q_len 1 with a contiguous query is that
 * entry, bit for bit.  batch, q_len or heads 0 enqueue nothing; a shape beyond
 * the grid limits is KVECC_EINVAL.  `workspace`:
 * kvecc_paged_attention_chunk_workspace(...) floats (0 for an empty call,
 * KVECC_EINVAL with a message for a negative size). */
KVECC_API int64_t kvecc_paged_attention_chunk_workspace(int64_t batch, int64_t q_len, int64_t heads,
                                                        int64_t head_dim, int64_t max_context_len);
KVECC_API int kvecc_paged_attention_chunk(const void *query, int64_t q_batch_stride,
                                          int64_t q_token_stride, int64_t q_head_stride, int q_dtype,
                                          const void *k_cache, const void *v_cache,
                                          const int32_t *block_table, const int32_t *context_lens,
                                          const float *k_scales, const float *v_scales, void *out,
                                          int64_t batch, int64_t q_len, int64_t heads, int64_t kv_heads,
                                          int64_t head_dim, int64_t num_blocks, int64_t num_layers,
                                          int64_t layer, int64_t block_size, int64_t max_blocks,
                                          int64_t max_context_len, float sm_scale, int codec,
                                          float *workspace, int64_t workspace_floats, void *stream);
/* kvecc_paged_attention_chunk over query spans (see "Query spans" above): the
 * arguments are that entry's with q_len read as q_max, plus q_spans after
 * context_lens; the workspace is kvecc_paged_attention_chunk_workspace at
 * q_len = q_max.  context_lens[b] counts sequence b's own valid tokens: valid
 * token t sits at p = context_lens[b] - count + (t - first) and attends as a
 * chunk row at p does.  A padding row gets the empty value (-8.0 for H84, 0
 * for Golay) in every lane, and its query elements are never read, so NaN or
 * Inf there reaches no output.  Launch geometry is chosen from batch, q_max and
 * heads as the uniform entry chooses it: all spans (0, q_max, .) return that
 * entry's bits for q_max > 1.  q_max 1 runs the split kernels (the decode
 * entry knows no spans).  A workgroup whose query rows are all padding reads no
 * table and no cache. */
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
                                                 float *workspace, int64_t workspace_floats, void *stream);

/* Interpolated attention (Hamming(8,4) with temporal interpolation of detected
 * double errors: the reference's config 4, interpolation_triton.py).  The
 * arguments, the workspace (kvecc_paged_attention_chunk_workspace at q_len =
 * q_max), the query strides, the output layout [batch, q_max, heads, head_dim],
 * the empty value -8.0, the GQA map and every other rule are
 * kvecc_paged_attention_chunk_ragged's, except that q_spans may be NULL (the
 * uniform call: first 0, count q_max) and q_max 1 is allowed and is the decode
 * step.  codec must be KVECC_CODEC_H84, and the caches must be under 4 GiB;
 * anything else is KVECC_EINVAL with a message (callers fall back).  No
 * statistics are kept.
 *
 * Interpolation is a property of the stored key / value, not of the query row
 * that looks at it.  With n_b = min(context_lens[b], max_context_len,
 * max_blocks*block_size), the value used for position l < n_b of sequence b is
 * bit for bit what kvecc_shim_read(..., ctx = n_b, interp = 1) gives for that
 * sequence alone: every byte decodes with the SECDED decoder; a byte of type 2
 * (double detected) becomes min(15, (L + R + 1) >> 1), where L and R are the
 * decoded, NOT interpolated, values of the same (head, d) element at positions
 * max(l - 1, 0) and min(l + 1, n_b - 1); a neighbour whose block-table entry is
 * < 0 reads as 0; a row whose own block is < 0 is skipped, as everywhere.
 * Consequences: in a chunk call the last key a query row sees, p_t, is
 * interpolated from key p_t + 1 when p_t + 1 < n_b although the row does not
 * attend to that key -- the neighbour bound is the sequence's length, never the
 * row's, the column's or the tile's key limit -- so row t is NOT the decode
 * call at context_lens = p_t + 1 whenever key p_t holds a double.  A batched
 * rectangular kvecc_shim_read_batch interpolates a shorter sequence's last
 * token against the zero row past its length; this entry clamps per sequence,
 * as the reference kernel does.  Launch geometry comes from batch, q_max and
 * heads only: all-full spans return the uniform call's bits. */
KVECC_API int kvecc_paged_attention_interp(const void *query, int64_t q_batch_stride, int64_t q_token_stride,
                                           int64_t q_head_stride, int q_dtype, const void *k_cache,
                                           const void *v_cache, const int32_t *block_table,
                                           const int32_t *context_lens, const int32_t *q_spans,
                                           const float *k_scales, const float *v_scales, void *out,
                                           int64_t batch, int64_t q_max, int64_t heads, int64_t kv_heads,
                                           int64_t head_dim, int64_t num_blocks, int64_t num_layers,
                                           int64_t layer, int64_t block_size, int64_t max_blocks,
                                           int64_t max_context_len, float sm_scale, int codec,
                                           float *workspace, int64_t workspace_floats, void *stream);

/* ---- Windowed attention ------------------------------------------------------ */
/* Sliding-window paged attention with sink tokens (Mistral-style masking over the
 * stored, post-RoPE keys: positions stay absolute, nothing in the cache is
 * re-indexed; no reference counterpart).  The arguments up to codec, the
 * workspace (kvecc_paged_attention_chunk_workspace at q_len = q_max), the query
 * strides, the output layout [batch, q_max, heads, head_dim], head_dim <= 256,
 * the GQA map, the spans and the max_context_len clamp are
 * kvecc_paged_attention_chunk_ragged's, except that q_spans may be NULL (the
 * uniform call: first 0, count q_max) and q_max 1 is allowed and is the decode
 * step.  codec: KVECC_CODEC_H84, _H74, _NONE, _GOLAY or _GOLAY_PACKED; query
 * dtypes fp32, fp16, bf16.  Plain attention only: no interpolation, no
 * statistics, no repair.
 *
 * window = W >= 0 and sinks = S >= 0; a negative one is KVECC_EINVAL.  For a
 * valid query row at position p (the ragged entry's rule) and ctx_cap =
 * min(max_context_len, max_blocks * block_size), key j is visible iff all of
 *   0 <= j <= p;   j < ctx_cap;   its block-table entry is >= 0;
 *   j < S  or  j > p - W.
 * A key that is both a sink and inside the window counts once.  A row with no
 * visible key gets the entry's empty value (-8.0 for the byte codecs, 0 for
 * Golay), per row; a padding row reads no query, and a workgroup whose rows are
 * all padding reads no table and no cache.  A workgroup whose stretch of the
 * context holds no key that any of its rows can see reads no table and no cache
 * either.  A stored row that no row of a workgroup can see is not fetched for
 * its own sake and takes no part in the arithmetic (a masked lane reads row 0 of
 * the cache instead, as for a -1 block, with weight and V scale forced to 0):
 * what lies in an invisible row -- a released block's bytes, a scale that is no
 * number -- reaches no output.
 *
 * W == 0 means no window: the call is kvecc_paged_attention_chunk_ragged's (or,
 * with NULL spans, kvecc_paged_attention_chunk's) and returns its bits; S is
 * ignored.  So is W >= ctx_cap, a window that covers every key a row below
 * ctx_cap can see -- also for a sequence whose context_lens exceeds ctx_cap
 * (its rows sit past the keys that are attended at all), where this sentence
 * takes precedence over the rule above.  Otherwise the kernels (matrix-core
 * tiles or the general path, heads per workgroup) are chosen as the ragged entry
 * chooses them, and the grid follows the window, not the context: ceil(S /
 * split) splits sit at the start of the context, and each workgroup places the
 * remaining ones at its own window, which it finds from context_lens -- the
 * caller promises nothing about the lengths.  Their number spans W + split - 1
 * keys (and the 15 later positions of a 16-column tile), at the split size the
 * launcher would pick for a context of S + W keys, doubled until the partials
 * fit the size kvecc_paged_attention_chunk_workspace returns for the call (the
 * plan never looks at workspace_floats beyond the check against that size, so a
 * larger buffer changes no bit); so grid, workspace traffic and combine width scale with
 * S + W + q_max.  Where that is no fewer splits than the whole context's, the
 * ragged entry's geometry is used as it is.  Results do not depend on the plan
 * beyond fp32 summation order. */
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
                                           void *stream);

/* ---- Counted attention ------------------------------------------------------- */
/* Paged attention over a Hamming(8,4) cache that keeps the decode statistics of
 * the bytes it reads (no reference counterpart: the reference kernel discards
 * them).  The arguments up to codec, the query strides, the output layout
 * [batch, q_max, heads, head_dim], the empty value -8.0, the GQA map, -1 blocks
 * and the max_context_len clamp are kvecc_paged_attention_interp's; the
 * workspace is kvecc_paged_attention_chunk_workspace at q_len = q_max; q_spans
 * may be NULL (first 0, count q_max) and q_max 1 is the decode step.  codec must
 * be KVECC_CODEC_H84, the caches must be under 4 GiB and stats must be non-NULL;
 * anything else is KVECC_EINVAL with a message and launches nothing (callers
 * fall back).  Golay, packed Golay and Hamming(7,4) caches are out of scope of
 * this entry.
 *
 * Output.  interp == 0: kvecc_paged_attention_chunk_ragged's contract (single
 * errors corrected, doubles keep their data), extended to q_max == 1 and NULL
 * spans.  interp != 0: kvecc_paged_attention_interp's contract, word for word.
 * Neither mode promises the bits of the uncounted kernels (fp32 summation
 * order).
 *
 * Statistics.  Let n_b = min(context_lens[b], max_context_len,
 * max_blocks*block_size).  One call adds to stats[0] / stats[1], for layer
 * `layer`: for each sequence b that has at least one valid query token, each
 * cache head, K and V, each stored byte of each position l < n_b whose
 * block-table entry is >= 0, counted EXACTLY ONCE, its SINGLE_CORRECTED (type
 * 1) / DOUBLE_DETECTED (type 2) classification; parity-only bytes (type 3) are
 * not counted.  That is what kvecc_shim_read(ctx = n_b, stats) adds for that
 * sequence alone.  Exactly once holds however the launch is cut: across the
 * query heads of one cache head, the tokens of a chunk, the context splits, the
 * one-pass-per-query-row form of the kernels, the interpolation's neighbour
 * rows, padded rows and keys beyond a row's causal limit (a span that overruns
 * q_max included: the positions past its last token's limit are counted and not
 * attended).  Not counted: a sequence whose row is all padding (count <= 0 or
 * first < 0 or first >= q_max), which is not read; positions >= n_b; other
 * layers; -1 blocks.  stats is the library's sharded buffer (KVECC_STATS_SLOTS
 * x KVECC_STATS_STRIDE, see the conventions above); totals accumulate across
 * calls.  The launch path reads nothing on the host: the call replays in a
 * captured graph.
 *
 * Kernels.  Counted siblings of the uncounted kernels, under their own names and
 * over an argument block of their own: of the matrix-core kernels (fp16 queries,
 * head_dim 32 / 64 / 128, both modes) and of the split kernels (every other dtype
 * and head_dim <= 256, both modes).  Of each (sequence, cache head, context
 * split) exactly one workgroup counts -- the first query-head group of the cache
 * head, in the token tile (matrix cores) or query row (split kernels) of the
 * sequence's last valid token, which walks the sequence's n_b rows -- on the
 * words its lanes load anyway, in registers, with one reduction and at most two
 * atomics per workgroup; every other workgroup runs the uncounted stream.  The
 * interpolating kernels' neighbour rows are never counted. */
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
                                          void *stream);

/* The same over a Golay(24,12) cache (no reference counterpart).  The arguments
 * are kvecc_paged_attention_stats's without interp (the reference interpolates
 * no Golay word).  codec must be KVECC_CODEC_GOLAY or KVECC_CODEC_GOLAY_PACKED
 * and stats non-NULL; anything else is KVECC_EINVAL with a message (naming golay
 * for a wrong codec, stats for a NULL buffer) and launches nothing.
 * kvecc_paged_attention_stats itself keeps rejecting every codec but
 * Hamming(8,4).  head_dim (<= 256), the query dtypes and the cache layouts are
 * kvecc_paged_attention_chunk_ragged's for Golay, except that the counted
 * kernels address the caches through buffer descriptors only: caches (or scale
 * arrays) of 4 GiB or more are KVECC_EINVAL with a message.
 *
 * Output.  kvecc_paged_attention_chunk_ragged's contract for Golay --
 * uncorrectable words keep their data, the empty value is 0, padding rows are
 * never read, its GQA map, -1 blocks and max_context_len clamp -- extended to
 * q_max == 1 and NULL spans; not the uncounted kernels' bits (fp32 summation
 * order, and the launcher may pick another kernel family for the same shape).
 *
 * Statistics.  With n_b as above, one call adds for layer `layer`, for each
 * sequence with at least one valid query token, each cache head, K and V, each
 * position l < n_b whose block-table entry is >= 0 and each of the row's g =
 * ceil(head_dim / 3) codewords, EXACTLY ONCE: stats[0] += the decoder's count
 * when it is 0..3 (bits corrected, parity bits included), stats[1] += 1 when it
 * is 4 (uncorrectable) -- bit for bit what kvecc_shim_read(ctx = n_b, stats)
 * adds for that sequence alone.  Exactly once holds however the launch is cut,
 * as above.  Never counted: bits 24..31 of an int32 word, the pad bytes of a
 * packed row, the codewords past g - 1 that a lane's wider load brings in (the
 * next row's, or past the buffer), the row that a -1 block's lanes read in its
 * place, positions >= n_b, other layers, all-padding sequences.  The buffer,
 * the accumulation across calls and graph replay are as above.
 *
 * Kernels.  Counted siblings of the ragged Golay kernels, under their own names:
 * two matrix-core kernels (fp16 queries, head_dim 128; int32 and packed), which
 * read the count from byte 3 of the correction entry their decode fetches
 * anyway, and the split kernels (every other dtype, group and head_dim), which
 * read it from bits 16-23 of theirs.  A decode step (q_max 1) without GQA takes
 * the split kernels.  The counting workgroup is chosen as above; the other
 * workgroups of the matrix-core kernels carry the count byte through their
 * decode (one more instruction per codeword) and add nothing. */
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
                                                void *stream);

/* ---- Repairing attention ----------------------------------------------------- */
/* kvecc_paged_attention_stats that also writes the corrected codewords back
 * (read-repair; no reference counterpart): one launch attends, counts and
 * scrubs what it counts.  The arguments are kvecc_paged_attention_stats's,
 * interp and stats included, except that k_cache / v_cache are NOT const: they
 * are the only arguments written besides out, stats and the workspace.
 * Validation is the counted entry's: KVECC_CODEC_H84 only, caches and scale
 * arrays under 4 GiB, stats non-NULL -- anything else is KVECC_EINVAL with a
 * message that names paged_attention_repair, and nothing is launched or
 * written.  The launch path reads nothing on the host: the call replays in a
 * captured graph.
 *
 * With n_b = min(context_lens[b], max_context_len, max_blocks*block_size) as in
 * "Counted attention":
 *
 * Output.  Bit for bit what kvecc_paged_attention_stats writes for the same
 * arguments on the cache as it stood before the call, in both interp modes: the
 * launcher picks the counted entry's geometry and the kernels run its
 * arithmetic stream.  This is derivable, not a tolerance: a rewritten byte
 * decodes to the same nibble as the byte it replaces (type 1: the corrected
 * nibble; type 3: the data bits were never wrong), a double is never rewritten
 * -- so its type, the one thing interpolation looks at besides decoded nibbles,
 * never changes -- and interpolation reads its neighbours' DECODED nibbles.  So
 * whether a concurrently reading workgroup (another query-head group of the
 * cache head, another token tile or query row, an interpolation halo) sees the
 * old or the new byte cannot matter.
 *
 * Statistics.  stats[0] / stats[1] += exactly what the counted entry adds;
 * stats[2] += the number of bytes rewritten.
 *
 * Cache after the call.  What kvecc_cache_scrub leaves of the cache as it stood
 * before the call when run with layer_first = layer, layer_count = 1, the same
 * clamp, and the length of every sequence without a valid query token set to 0:
 * for layer `layer`, each sequence with at least one valid query token, each
 * cache head, K and V, each position l < n_b whose block-table entry is >= 0, a
 * type-1 (single) or type-3 (overall parity) byte becomes encode(decoded data);
 * type-2 and clean bytes stay bit for bit (h84_scrub4 of csrc/codec_math.h).
 * Every other byte of both caches keeps its bits: other layers, positions >=
 * n_b, -1 blocks, blocks no counted row names, all-padding sequences, and the
 * row-0 stand-ins that masked lanes read.  Both scale arrays keep theirs.
 * stats[2] equals that scrub's stats[2].  A call over a clean or already
 * repaired region stores nothing.  Two table rows may name the same block: the
 * bytes come out as the scrub's (every writer stores the same value), but a
 * byte of that block may then be counted in stats[0] / stats[2] by one row
 * before and by the other after it was rewritten, so those two totals are only
 * bounded by the counted entry's / the scrub's.
 *
 * Kernels.  Repairing siblings of the 126 counted Hamming(8,4) kernels, under
 * their own names.  Only the counting workgroup of each (sequence, cache head,
 * context split) stores, where it counts and on the words as loaded -- before the
 * interpolating kernels rewrite any in registers.  There each stored byte of
 * the first n_b positions is held by exactly one lane, once per call; a lane
 * stores a word (head_dim 32's V chunk: its two bytes) only if the XOR of
 * h84_scrub4 is non-zero, with a plain vector buffer store through the
 * descriptor the word was loaded through.  No fence and no atomic touches the
 * cache; kernel completion publishes the stores. */
KVECC_API int kvecc_paged_attention_repair(const void *query, int64_t q_batch_stride, int64_t q_token_stride,
                                           int64_t q_head_stride, int q_dtype, void *k_cache, void *v_cache,
                                           const int32_t *block_table, const int32_t *context_lens,
                                           const int32_t *q_spans, const float *k_scales,
                                           const float *v_scales, void *out, int64_t batch, int64_t q_max,
                                           int64_t heads, int64_t kv_heads, int64_t head_dim,
                                           int64_t num_blocks, int64_t num_layers, int64_t layer,
                                           int64_t block_size, int64_t max_blocks, int64_t max_context_len,
                                           float sm_scale, int codec, int interp, uint64_t *stats,
                                           float *workspace, int64_t workspace_floats, void *stream);

/* ---- Cache scrub --------------------------------------------------------------- */
/* In-place patrol scrub of a resident paged cache (no reference counterpart:
 * the reference's cache lives for one forward, and every reader here corrects
 * into its output or its registers and leaves the codeword in HBM wrong).  ONE
 * launch handles every codeword of every valid token of layers [layer_first,
 * layer_first + layer_count) of every sequence, K and V alike: the word is
 * decoded with the library's decoder and
 *   - a CORRECTABLE word whose stored codeword bits differ from
 *     encode(decoded data) is replaced by that codeword: H74 any non-zero
 *     syndrome (doubles are miscorrected, as the decoder does); H84 a single
 *     (type 1) or an overall-parity error (type 3); Golay 1 to 3 flipped bits,
 *     parity bits with clean data included;
 *   - an UNCORRECTABLE word (H84 double, type 2; Golay count 4) stays bit for
 *     bit as it is -- the readers keep its data too;
 *   - bits outside the codeword are neither examined nor changed: bit 7 of an
 *     H74 byte, bits 24..31 of an int32 Golay word, the pad bytes of a packed
 *     row.  Scales, slots at or beyond a sequence's length, layers outside the
 *     range and blocks no table row names stay untouched;
 *   - a clean word is not stored (a lane may store the whole 16-byte vector or
 *     12-byte packed group it loaded when a word in it is dirty): a pass over a
 *     clean cache writes nothing, and a second pass rewrites nothing.
 * Caches as kvecc_shim_write ([blocks, num_layers, hkv, block_size, P]; codec
 * H74, H84, GOLAY or GOLAY_PACKED -- KVECC_CODEC_NONE is KVECC_EINVAL, there is
 * nothing to scrub), 4-byte aligned; d <= 512, d % 4 == 0 for the byte codecs.
 * block_table is [batch, table_stride] device int32; context_lens is device
 * int32 the host never reads: sequence b of layer l holds
 * context_lens[(l - layer_first) * lens_layer_stride + b] tokens (stride 0: one
 * row serves every layer), clamped to min(max_context_len, table_stride *
 * block_size) as kvecc_paged_attention clamps (max_context_len <= 0: the table
 * bound).  A length <= 0 skips the sequence, a block id < 0 or >= num_blocks
 * the block: nothing is read and nothing written.  Two table rows may name the
 * same block (both writers store the same value).  batch == 0 or layer_count
 * == 0 enqueues nothing.
 * stats (sharded buffer, may be NULL): stats[0] and stats[1] += what
 * kvecc_shim_read adds for the codec (H74: flagged / 0; H84: single corrected /
 * double detected; Golay: bits corrected / uncorrectable words), stats[2] +=
 * words rewritten, stats[3] += words scanned. */
KVECC_API int kvecc_cache_scrub(void *k_cache, void *v_cache, const int32_t *block_table,
                                int64_t table_stride, const int32_t *context_lens,
                                int64_t lens_layer_stride, int64_t batch, int64_t hkv, int64_t d,
                                int64_t num_blocks, int64_t num_layers, int64_t layer_first,
                                int64_t layer_count, int64_t block_size, int64_t max_context_len,
                                int codec, uint64_t *stats, void *stream);

/* ---- Host ("cpu") backend ------------------------------------------------- */
/* The reference has no CPU codec backend (every wrapper asserts x.is_cuda,
 * e.g. hamming74_triton.py:185,246, golay_triton.py:399,456); BASELINE config 1 asks
 * for backend="cpu".  These are the host twins of the entry points above:
 * same arguments minus the stream, HOST pointers, the same codec algebra
 * (csrc/codec_math.h) run by `threads` std::threads (<= 0: all cores).
 * `stats` is a plain host uint64 array (stats[0], stats[1] += ...), not the
 * sharded device buffer. */
KVECC_API int kvecc_cpu_hamming74_encode(const uint8_t *in, uint8_t *out, int64_t n, int threads);
KVECC_API int kvecc_cpu_hamming84_encode(const uint8_t *in, uint8_t *out, int64_t n, int threads);
KVECC_API int kvecc_cpu_hamming74_decode(const uint8_t *cw, uint8_t *data, uint8_t *flag, int64_t n,
                                         uint64_t *stats, int threads);
KVECC_API int kvecc_cpu_hamming84_decode(const uint8_t *cw, uint8_t *data, uint8_t *etype, int64_t n,
                                         uint64_t *stats, int threads);
KVECC_API int kvecc_cpu_golay_encode(const uint8_t *trip, int32_t *cw, int64_t m, int threads);
KVECC_API int kvecc_cpu_golay_decode(const int32_t *cw, uint8_t *trip, uint8_t *counts, int64_t m,
                                     uint64_t *stats, int threads);
KVECC_API int kvecc_cpu_golay_encode_rows(const uint8_t *nibbles, int32_t *codewords, int64_t rows,
                                          int64_t d, int threads);
KVECC_API int kvecc_cpu_golay_decode_rows(const int32_t *codewords, uint8_t *nibbles, int64_t rows,
                                          int64_t d, uint64_t *stats, int threads);
KVECC_API int kvecc_cpu_golay_encode_packed(const uint8_t *nibbles, uint8_t *codewords, int64_t m,
                                            int threads);
KVECC_API int kvecc_cpu_golay_decode_packed(const uint8_t *codewords, uint8_t *nibbles,
                                            uint8_t *uncorrectable, int64_t m, uint64_t *stats,
                                            int threads);
KVECC_API int kvecc_cpu_hamming84_encode_packed(const uint8_t *nibbles, uint8_t *codewords,
                                                int64_t n, int threads);
KVECC_API int kvecc_cpu_hamming84_decode_packed(const uint8_t *codewords, uint8_t *nibbles,
                                                uint8_t *error_types, int64_t n, uint64_t *stats,
                                                int threads);
KVECC_API int kvecc_cpu_inject_u8(const uint8_t *in, uint8_t *out, uint8_t *counts, int64_t n,
                                  int n_bits, int64_t seed, float ber, int64_t global_n,
                                  int64_t offset0, uint64_t *stats, int threads);
KVECC_API int kvecc_cpu_inject_i32(const int32_t *in, int32_t *out, uint8_t *counts, int64_t n,
                                   int n_bits, int64_t seed, float ber, int64_t global_n,
                                   int64_t offset0, uint64_t *stats, int threads);
KVECC_API int kvecc_cpu_inject_u8_vectorized(const uint8_t *in, uint8_t *out, uint8_t *counts,
                                             int64_t n, int n_bits, int64_t seed, float ber,
                                             uint64_t *stats, int threads);
KVECC_API int kvecc_cpu_inject_i32_vectorized(const int32_t *in, int32_t *out, uint8_t *counts,
                                              int64_t n, int n_bits, int64_t seed, float ber,
                                              uint64_t *stats, int threads);
KVECC_API int kvecc_cpu_inject_rows_u8(const uint8_t *in, uint8_t *out, int64_t rows,
                                       int64_t row_len, int n_bits, int64_t seed_base, float ber,
                                       uint64_t *stats, int threads);
KVECC_API int kvecc_cpu_inject_rows_i32(const int32_t *in, int32_t *out, int64_t rows,
                                        int64_t row_len, int n_bits, int64_t seed_base, float ber,
                                        uint64_t *stats, int threads);
KVECC_API int kvecc_cpu_count_ne_u8(const uint8_t *a, const uint8_t *b, int64_t n, uint64_t *stats,
                                    int threads);
KVECC_API int kvecc_cpu_interpolate(const uint8_t *q, const uint8_t *err, uint8_t *out,
                                    int64_t outer, int64_t len, int64_t inner, int threads);
KVECC_API int kvecc_cpu_quantize_encode_rows(const void *x, int x_dtype, int codec,
                                             int scale_rule, uint8_t *cw, float *scales,
                                             int64_t rows, int64_t d, int threads);
KVECC_API int kvecc_cpu_decode_dequant_h84_rows(const uint8_t *cw, const float *scales, void *out,
                                                int out_dtype, int64_t rows, int64_t d,
                                                int zero_doubles, uint64_t *stats, int threads);
KVECC_API int kvecc_cpu_shim_write(const void *k, const void *v, int x_dtype, int64_t batch,
                                   int64_t seq, int64_t hkv, int64_t d, int codec,
                                   int scale_rule, int n_bits,
                                   int inject, float ber, int64_t seed0, void *k_cache,
                                   void *v_cache, float *k_scales, float *v_scales,
                                   const int32_t *block_table, int64_t num_layers,
                                   int64_t block_size, int64_t layer, int threads);
/* kvecc_shim_append on contiguous K/V [batch, q_len, hkv*d]; start_pos is a host int32 [batch] */
KVECC_API int kvecc_cpu_shim_append(const void *k, const void *v, int x_dtype, int64_t batch,
                                    int64_t q_len, int64_t hkv, int64_t d, int codec,
                                    int scale_rule, int n_bits, int inject, float ber,
                                    int64_t seed0, void *k_cache, void *v_cache, float *k_scales,
                                    float *v_scales, const int32_t *block_table,
                                    int64_t table_stride, const int32_t *start_pos,
                                    int64_t num_layers, int64_t block_size, int64_t layer,
                                    int threads);
/* kvecc_shim_append_ragged on contiguous K/V [batch, q_max, hkv*d]; start_pos and q_spans are host int32 */
KVECC_API int kvecc_cpu_shim_append_ragged(const void *k, const void *v, int x_dtype, int64_t batch,
                                           int64_t q_max, int64_t hkv, int64_t d, int codec,
                                           int scale_rule, int n_bits, int inject, float ber,
                                           int64_t seed0, void *k_cache, void *v_cache, float *k_scales,
                                           float *v_scales, const int32_t *block_table,
                                           int64_t table_stride, const int32_t *start_pos,
                                           const int32_t *q_spans, int64_t num_layers,
                                           int64_t block_size, int64_t layer, int threads);
KVECC_API int kvecc_cpu_shim_read(const void *k_cache, const void *v_cache, const float *k_scales,
                                  const float *v_scales, const int32_t *block_table, int64_t ctx,
                                  int64_t hkv, int64_t d, int64_t num_layers, int64_t block_size,
                                  int64_t layer, int codec, int interp, void *k_out, void *v_out,
                                  int out_dtype, uint64_t *stats, int threads);
KVECC_API int kvecc_cpu_shim_read_batch(const void *k_cache, const void *v_cache,
                                        const float *k_scales, const float *v_scales,
                                        const int32_t *block_table, int64_t table_stride,
                                        int64_t batch, int64_t ctx, int64_t hkv, int64_t d,
                                        int64_t num_layers, int64_t block_size, int64_t layer,
                                        int codec, int interp, void *k_out, void *v_out,
                                        int out_dtype, uint64_t *stats, int threads);
/* kvecc_cache_scrub on host pointers; stats[0..3] += into a plain host array */
KVECC_API int kvecc_cpu_cache_scrub(void *k_cache, void *v_cache, const int32_t *block_table,
                                    int64_t table_stride, const int32_t *context_lens,
                                    int64_t lens_layer_stride, int64_t batch, int64_t hkv, int64_t d,
                                    int64_t num_blocks, int64_t num_layers, int64_t layer_first,
                                    int64_t layer_count, int64_t block_size, int64_t max_context_len,
                                    int codec, uint64_t *stats, int threads);
KVECC_API int kvecc_cpu_paged_attention(const void *query, int q_dtype, const void *k_cache,
                                        const void *v_cache, const int32_t *block_table,
                                        const int32_t *context_lens, const float *k_scales,
                                        const float *v_scales, void *out, int64_t batch,
                                        int64_t heads, int64_t kv_heads, int64_t head_dim,
                                        int64_t num_blocks, int64_t num_layers, int64_t layer, int64_t block_size,
                                        int64_t max_blocks, int64_t max_context_len,
                                        float sm_scale, int codec, int threads);
KVECC_API int kvecc_cpu_paged_attention_chunk(const void *query, int64_t q_batch_stride,
                                              int64_t q_token_stride, int64_t q_head_stride, int q_dtype,
                                              const void *k_cache, const void *v_cache,
                                              const int32_t *block_table, const int32_t *context_lens,
                                              const float *k_scales, const float *v_scales, void *out,
                                              int64_t batch, int64_t q_len, int64_t heads, int64_t kv_heads,
                                              int64_t head_dim, int64_t num_blocks, int64_t num_layers,
                                              int64_t layer, int64_t block_size, int64_t max_blocks,
                                              int64_t max_context_len, float sm_scale, int codec, int threads);
KVECC_API int kvecc_cpu_paged_attention_chunk_ragged(const void *query, int64_t q_batch_stride,
                                                     int64_t q_token_stride, int64_t q_head_stride, int q_dtype,
                                                     const void *k_cache, const void *v_cache,
                                                     const int32_t *block_table, const int32_t *context_lens,
                                                     const int32_t *q_spans, const float *k_scales,
                                                     const float *v_scales, void *out, int64_t batch,
                                                     int64_t q_max, int64_t heads, int64_t kv_heads,
                                                     int64_t head_dim, int64_t num_blocks, int64_t num_layers,
                                                     int64_t layer, int64_t block_size, int64_t max_blocks,
                                                     int64_t max_context_len, float sm_scale, int codec,
                                                     int threads);
/* host twin of kvecc_paged_attention_interp (q_spans may be NULL) */
KVECC_API int kvecc_cpu_paged_attention_interp(const void *query, int64_t q_batch_stride,
                                               int64_t q_token_stride, int64_t q_head_stride, int q_dtype,
                                               const void *k_cache, const void *v_cache,
                                               const int32_t *block_table, const int32_t *context_lens,
                                               const int32_t *q_spans, const float *k_scales,
                                               const float *v_scales, void *out, int64_t batch,
                                               int64_t q_max, int64_t heads, int64_t kv_heads,
                                               int64_t head_dim, int64_t num_blocks, int64_t num_layers,
                                               int64_t layer, int64_t block_size, int64_t max_blocks,
                                               int64_t max_context_len, float sm_scale, int codec,
                                               int threads);
/* host twin of kvecc_paged_attention_window (q_spans may be NULL; fp32 throughout; window 0
 * is the ragged / chunk twin's bits) */
KVECC_API int kvecc_cpu_paged_attention_window(const void *query, int64_t q_batch_stride,
                                               int64_t q_token_stride, int64_t q_head_stride, int q_dtype,
                                               const void *k_cache, const void *v_cache,
                                               const int32_t *block_table, const int32_t *context_lens,
                                               const int32_t *q_spans, const float *k_scales,
                                               const float *v_scales, void *out, int64_t batch,
                                               int64_t q_max, int64_t heads, int64_t kv_heads,
                                               int64_t head_dim, int64_t num_blocks, int64_t num_layers,
                                               int64_t layer, int64_t block_size, int64_t max_blocks,
                                               int64_t max_context_len, float sm_scale, int codec,
                                               int64_t window, int64_t sinks, int threads);
/* host twin of kvecc_paged_attention_stats (q_spans may be NULL; stats a host buffer whose
 * words 0 and 1 take the totals) */
KVECC_API int kvecc_cpu_paged_attention_stats(const void *query, int64_t q_batch_stride,
                                              int64_t q_token_stride, int64_t q_head_stride, int q_dtype,
                                              const void *k_cache, const void *v_cache,
                                              const int32_t *block_table, const int32_t *context_lens,
                                              const int32_t *q_spans, const float *k_scales,
                                              const float *v_scales, void *out, int64_t batch,
                                              int64_t q_max, int64_t heads, int64_t kv_heads,
                                              int64_t head_dim, int64_t num_blocks, int64_t num_layers,
                                              int64_t layer, int64_t block_size, int64_t max_blocks,
                                              int64_t max_context_len, float sm_scale, int codec, int interp,
                                              uint64_t *stats, int threads);
/* host twin of kvecc_paged_attention_repair: the host counted twin's output (computed on the cache
 * as it stood) and counts, then h84_scrub4 over the same region of the HOST caches, which it
 * writes; stats a host buffer of >= 3 words, word 2 += bytes rewritten */
KVECC_API int kvecc_cpu_paged_attention_repair(const void *query, int64_t q_batch_stride,
                                               int64_t q_token_stride, int64_t q_head_stride, int q_dtype,
                                               void *k_cache, void *v_cache, const int32_t *block_table,
                                               const int32_t *context_lens, const int32_t *q_spans,
                                               const float *k_scales, const float *v_scales, void *out,
                                               int64_t batch, int64_t q_max, int64_t heads, int64_t kv_heads,
                                               int64_t head_dim, int64_t num_blocks, int64_t num_layers,
                                               int64_t layer, int64_t block_size, int64_t max_blocks,
                                               int64_t max_context_len, float sm_scale, int codec, int interp,
                                               uint64_t *stats, int threads);
/* host twin of kvecc_paged_attention_golay_stats (as above) */
KVECC_API int kvecc_cpu_paged_attention_golay_stats(const void *query, int64_t q_batch_stride,
                                                    int64_t q_token_stride, int64_t q_head_stride, int q_dtype,
                                                    const void *k_cache, const void *v_cache,
                                                    const int32_t *block_table, const int32_t *context_lens,
                                                    const int32_t *q_spans, const float *k_scales,
                                                    const float *v_scales, void *out, int64_t batch,
                                                    int64_t q_max, int64_t heads, int64_t kv_heads,
                                                    int64_t head_dim, int64_t num_blocks, int64_t num_layers,
                                                    int64_t layer, int64_t block_size, int64_t max_blocks,
                                                    int64_t max_context_len, float sm_scale, int codec,
                                                    uint64_t *stats, int threads);

#ifdef __cplusplus
}
#endif
#endif /* KVECC_H */
