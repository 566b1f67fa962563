// scrub.hip -- in-place KV-cache scrub (kvecc_cache_scrub): decode every
// resident codeword of the valid tokens, and store back encode(decoded data)
// where a correctable word differs from it.  No reference counterpart (the
// reference's cache lives for one forward); the semantics are kvecc.h's
// "Cache scrub" section, the bit operations codec_math.h's *_scrub*, shared
// with the host twin in cpu.hip.
//
// One launch covers every sequence, every layer of the range and both sides.
// A segment is one (sequence, layer, logical block, side): inside a physical
// block the layout is [layer][head][slot][P], so a full block's heads are ONE
// contiguous run of hkv * block_size * P elements and a partial block's are hkv
// runs of n_valid * P.  A persistent grid of workgroups strides over the
// segments (Golay stages its 16 KiB of tables once per workgroup, and only if
// it meets a live segment); a segment past its sequence's length, or whose
// table entry names no block, is left before anything of the cache is loaded.
//
// Byte codecs and int32 Golay are independent per dword, so a run is cut into
// an unaligned head (0-3 dwords), 16-byte vectors and a tail (0-3 dwords); one
// lane owns one piece.  Packed Golay rows (3-byte codewords, pad bytes after
// the last) are cut into 12-byte groups of 4 codewords, one lane each; the pad
// bytes travel with the group and go back as they came.  A piece is first only
// looked at (one v_perm syndrome code per Hamming dword, one `par` lookup per
// Golay codeword); the full decode / re-encode runs for pieces that hold a
// non-codeword, and a lane stores its piece only when a word in it changed: a
// pass over a clean cache writes nothing.
#include <algorithm>

#include "kvecc_internal.h"

namespace kvecc {
namespace {

constexpr int kScrubBlock = 256;
// Workgroups per CU = waves per SIMD (a workgroup is one wave on each of a CU's 4
// SIMDs).  The grid is persistent, so it must not exceed what is resident at
// once: a workgroup that waits for another to retire starts its share of the
// segments when the rest of the chip is done (98 VGPRs gave 5 waves per SIMD
// under a grid of 8 per CU: 1.3-1.5x slower).  The launch bounds hold the
// kernels to 8 per SIMD (<= 64 VGPRs; 16 KiB of Golay tables each also fit 8
// per CU); Hamming(8,4) keeps 2 pieces per lane in flight instead of 4 to fit
// (it spills at 64 VGPRs with 4).
constexpr int kScrubPerCu = 8;

struct ScrubArgs {
  void *cache[2];
  const int32_t *table, *lens;
  const uint16_t *par;  // parity[4096] then correct[4096] (runtime.hip keeps them together)
  uint64_t *stats;
  uint32_t tstride, lens_stride, hkv, g, rowb, num_blocks, layers, layer_first, layer_count, bs;
  uint32_t bound;  // min(max_context_len, table_stride * block_size)
  uint32_t nlb;    // logical blocks up to the bound
  uint32_t nseg;   // batch * layer_count * nlb * 2
  uint32_t gpr, gpr_magic;  // packed: 12-byte groups per row, and floor(2^32 / gpr) + 1 (i / gpr by mulhi; gpr > 1)
};

struct __attribute__((packed, aligned(4))) Dw3 {
  uint32_t a, b, c;
};

// the XOR pattern of one dword of a byte codec or of int32 Golay
template <int CODEC>
__device__ __forceinline__ uint32_t scrub_word(uint32_t w, const uint16_t *tab, uint32_t (&cnt)[4]) {
  if constexpr (CODEC == KVECC_CODEC_H84) return h84_scrub4(w, cnt[0], cnt[1], cnt[2]);
  if constexpr (CODEC == KVECC_CODEC_H74) return h74_scrub4(w, cnt[0], cnt[2]);
  return golay_scrub1(w, tab, tab + 4096, cnt[0], cnt[1], cnt[2]);
}

// non-zero iff the dword holds a word that is not a codeword (the pass's cheap first look)
template <int CODEC>
__device__ __forceinline__ uint32_t dirty_word(uint32_t w, const uint16_t *tab) {
  if constexpr (CODEC == KVECC_CODEC_H84) return h84_dirty4(w);
  if constexpr (CODEC == KVECC_CODEC_H74) return h74_dirty4(w);
  return golay_syndrome1(w, tab);
}

template <int CODEC>
__global__ __launch_bounds__(kScrubBlock, kScrubPerCu) void cache_scrub_kernel(ScrubArgs a) {
  constexpr bool kGolay = CODEC == KVECC_CODEC_GOLAY || CODEC == KVECC_CODEC_GOLAY_PACKED;
  __shared__ __attribute__((aligned(16))) uint16_t tab[kGolay ? 8192 : 8];
  constexpr int kScrubUnroll = CODEC == KVECC_CODEC_H84 ? 2 : 4;  // pieces a lane has in flight
  bool staged = !kGolay;
  uint32_t cnt[4] = {0, 0, 0, 0};  // statistics 0 and 1, rewritten, scanned
  const uint32_t tid = threadIdx.x;
  for (uint32_t s = blockIdx.x; s < a.nseg; s += gridDim.x) {
    const uint32_t side = s & 1u, t = s >> 1;
    const uint32_t lb = t % a.nlb, bl = t / a.nlb;
    const uint32_t li = bl % a.layer_count, b = bl / a.layer_count;
    const int32_t len = min(a.lens[(size_t)li * a.lens_stride + b], (int32_t)a.bound);
    if (len <= 0) continue;  // an inactive sequence
    const int32_t nv = min((int32_t)a.bs, len - (int32_t)(lb * a.bs));
    if (nv <= 0) continue;  // past the sequence's length
    const int32_t blk = a.table[(size_t)b * a.tstride + lb];
    if (blk < 0 || (uint32_t)blk >= a.num_blocks) continue;
    if (kGolay && !staged) {  // uniform: every thread of the workgroup gets here together
      const u32x4 *src = reinterpret_cast<const u32x4 *>(a.par);
      u32x4 *dst = reinterpret_cast<u32x4 *>(tab);
      for (uint32_t k = tid; k < 1024; k += kScrubBlock) dst[k] = src[k];
      __syncthreads();
      staged = true;
    }
    char *base = reinterpret_cast<char *>(a.cache[side]) +
                 ((size_t)blk * a.layers + a.layer_first + li) * a.hkv * a.bs * a.rowb;
    // runs: a full block's heads are one contiguous run, a partial block's one run per head
    const bool full = (uint32_t)nv == a.bs;
    const uint32_t nruns = full ? 1u : a.hkv;
    const uint32_t run_rows = full ? a.hkv * a.bs : (uint32_t)nv;
    const uint32_t run_stride = a.bs * a.rowb;  // bytes between two heads' runs
    for (uint32_t r = 0; r < nruns; ++r) {
      char *rb = base + (size_t)r * run_stride;
      if constexpr (CODEC == KVECC_CODEC_GOLAY_PACKED) {
        const uint32_t items = run_rows * a.gpr;  // 12-byte groups of 4 codewords
        for (uint32_t it = 0; it < items; it += kScrubBlock * kScrubUnroll) {
          uint32_t *p[kScrubUnroll];
          uint32_t ncw[kScrubUnroll], w[kScrubUnroll][3];
#pragma unroll
          for (int u = 0; u < kScrubUnroll; ++u) {
            const uint32_t i = it + u * kScrubBlock + tid;
            ncw[u] = 0;
            p[u] = reinterpret_cast<uint32_t *>(rb);
            w[u][0] = w[u][1] = w[u][2] = 0;
            if (i < items) {
              const uint32_t row = a.gpr == 1 ? i : __umulhi(i, a.gpr_magic), q = i - row * a.gpr;  // i / gpr, i % gpr
              p[u] = reinterpret_cast<uint32_t *>(rb + (size_t)row * a.rowb) + 3 * q;
              ncw[u] = min(4u, a.g - 4 * q);
              if (ncw[u] >= 3) {
                const Dw3 v = *reinterpret_cast<const Dw3 *>(p[u]);
                w[u][0] = v.a;
                w[u][1] = v.b;
                w[u][2] = v.c;
              } else {
                w[u][0] = p[u][0];
                if (ncw[u] == 2) w[u][1] = p[u][1];
              }
            }
          }
#pragma unroll
          for (int u = 0; u < kScrubUnroll; ++u) {
            if (ncw[u] == 0) continue;
            cnt[3] += ncw[u];
            // 4 little-endian 3-byte codewords in 3 dwords; past ncw: pad or the next row, left alone
            const uint32_t c[4] = {w[u][0], w[u][0] >> 24 | w[u][1] << 8, w[u][1] >> 16 | w[u][2] << 16,
                                   w[u][2] >> 8};
            uint32_t syn = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if ((uint32_t)k < ncw[u]) syn |= golay_syndrome1(c[k], tab);
            if (syn == 0) continue;  // four codewords: nothing to count, nothing to store
            uint32_t x[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
              x[k] = (uint32_t)k < ncw[u] ? golay_scrub1(c[k], tab, tab + 4096, cnt[0], cnt[1], cnt[2]) : 0u;
            const uint32_t x0 = x[0] | x[1] << 24, x1 = x[1] >> 8 | x[2] << 16, x2 = x[2] >> 16 | x[3] << 8;
            if ((x0 | x1 | x2) == 0) continue;  // uncorrectable only: no store
            if (ncw[u] >= 3) {
              *reinterpret_cast<Dw3 *>(p[u]) = Dw3{w[u][0] ^ x0, w[u][1] ^ x1, w[u][2] ^ x2};
            } else {
              if (x0) p[u][0] = w[u][0] ^ x0;
              if (x1) p[u][1] = w[u][1] ^ x1;
            }
          }
        }
      } else {
        constexpr uint32_t kPerDw = kGolay ? 1u : 4u;  // codewords per dword
        const uint32_t run_dw = run_rows * (a.rowb / 4);
        // pieces of the run: an unaligned head (0-3 dwords), 16-byte vectors, a tail (0-3 dwords)
        const uint32_t hd = min(run_dw, (uint32_t)((0 - reinterpret_cast<uintptr_t>(rb)) & 15u) >> 2);
        const uint32_t nvec = (run_dw - hd) >> 2;
        const uint32_t items = nvec + 2;
        for (uint32_t it = 0; it < items; it += kScrubBlock * kScrubUnroll) {
          uint32_t *p[kScrubUnroll];
          uint32_t n[kScrubUnroll];
          u32x4 v[kScrubUnroll];
#pragma unroll
          for (int u = 0; u < kScrubUnroll; ++u) {
            const uint32_t c = it + u * kScrubBlock + tid;
            uint32_t off = 0;
            n[u] = 0;
            if (c < nvec) {
              off = hd + 4 * c;
              n[u] = 4;
            } else if (c == nvec) {
              n[u] = hd;
            } else if (c == nvec + 1) {
              off = hd + 4 * nvec;
              n[u] = run_dw - off;
            }
            p[u] = reinterpret_cast<uint32_t *>(rb) + off;
            v[u] = u32x4{0, 0, 0, 0};
            if (n[u] == 4) {
              v[u] = *reinterpret_cast<const u32x4 *>(p[u]);
            } else {
              if (n[u] > 0) v[u].x = p[u][0];
              if (n[u] > 1) v[u].y = p[u][1];
              if (n[u] > 2) v[u].z = p[u][2];
            }
          }
#pragma unroll
          for (int u = 0; u < kScrubUnroll; ++u) {
            if (n[u] == 0) continue;
            cnt[3] += kPerDw * n[u];
            // words past n are zero: a clean codeword under every codec, no statistics
            if ((dirty_word<CODEC>(v[u].x, tab) | dirty_word<CODEC>(v[u].y, tab) | dirty_word<CODEC>(v[u].z, tab) |
                 dirty_word<CODEC>(v[u].w, tab)) == 0)
              continue;  // every codeword of the piece is one: nothing to count, nothing to store
            const u32x4 x = {scrub_word<CODEC>(v[u].x, tab, cnt), scrub_word<CODEC>(v[u].y, tab, cnt),
                             scrub_word<CODEC>(v[u].z, tab, cnt), scrub_word<CODEC>(v[u].w, tab, cnt)};
            if ((x.x | x.y | x.z | x.w) == 0) continue;  // uncorrectable only: no store
            if (n[u] == 4) {
              *reinterpret_cast<u32x4 *>(p[u]) = v[u] ^ x;
            } else {
              if (x.x) p[u][0] = v[u].x ^ x.x;
              if (x.y) p[u][1] = v[u].y ^ x.y;
              if (x.z) p[u][2] = v[u].z ^ x.z;
            }
          }
        }
      }
    }
  }
  if (a.stats) flush_stats_n<4, kScrubBlock>(a.stats, cnt);
}

}  // namespace
}  // namespace kvecc

using namespace kvecc;

extern "C" {

KVECC_API int kvecc_cache_scrub(void *k_cache, void *v_cache, const int32_t *block_table,
                                int64_t table_stride, const int32_t *context_lens,
                                int64_t lens_layer_stride, int64_t batch, int64_t hkv, int64_t d,
                                int64_t num_blocks, int64_t num_layers, int64_t layer_first,
                                int64_t layer_count, int64_t block_size, int64_t max_context_len,
                                int codec, uint64_t *stats, void *stream) {
  if (table_stride < 0 || lens_layer_stride < 0 || batch < 0 || hkv < 0 || d < 0 || num_blocks < 0 ||
      num_layers < 0 || layer_first < 0 || layer_count < 0 || block_size < 0)
    return set_error(KVECC_EINVAL, "cache_scrub: negative size");
  if (codec == KVECC_CODEC_NONE) return set_error(KVECC_EINVAL, "cache_scrub: codec none has nothing to scrub");
  if (codec < KVECC_CODEC_NONE || codec > KVECC_CODEC_GOLAY_PACKED)
    return set_error(KVECC_EINVAL, "cache_scrub: bad codec %d", codec);
  if (batch == 0 || layer_count == 0 || hkv == 0) return KVECC_OK;
  const bool golay = codec == KVECC_CODEC_GOLAY || codec == KVECC_CODEC_GOLAY_PACKED;
  if (d < 1 || d > 512) return set_error(KVECC_EINVAL, "cache_scrub: head_dim %lld not in [1, 512]", (long long)d);
  if (!golay && d % 4 != 0)
    return set_error(KVECC_EINVAL, "cache_scrub: head_dim %lld must be a multiple of 4", (long long)d);
  if (num_layers < 1 || block_size < 1 || num_blocks < 1 || layer_first + layer_count > num_layers)
    return set_error(KVECC_EINVAL, "cache_scrub: bad cache geometry (layers [%lld, %lld) of %lld)",
                     (long long)layer_first, (long long)(layer_first + layer_count), (long long)num_layers);
  if (table_stride < 1) return set_error(KVECC_EINVAL, "cache_scrub: table stride %lld < 1", (long long)table_stride);
  if (!k_cache || !v_cache || !block_table || !context_lens)
    return set_error(KVECC_EINVAL, "cache_scrub: null pointer");
  if (!aligned(k_cache, 4) || !aligned(v_cache, 4))
    return set_error(KVECC_EINVAL, "cache_scrub: caches must be 4-byte aligned");
  const int64_t g = golay ? (d + 2) / 3 : d;
  const int64_t rowb = codec == KVECC_CODEC_GOLAY_PACKED ? KVECC_GOLAY_PACKED_ROW(g) : golay ? 4 * g : d;
  // every factor first: the products below then fit 64 bits
  if (batch > 0x7FFFFFFFLL || hkv > 0x7FFFFFFFLL || table_stride > 0x7FFFFFFFLL || block_size > 0x7FFFFFFFLL ||
      num_layers > 0x7FFFFFFFLL || num_blocks > 0x7FFFFFFFLL || lens_layer_stride > 0x7FFFFFFFLL ||
      table_stride * block_size > 0x7FFFFFFFLL || hkv * block_size > 0x7FFFFFFFLL ||
      hkv * block_size * rowb > 0x7FFFFFFFLL)
    return set_error(KVECC_EINVAL, "cache_scrub: sizes exceed 32-bit indexing");
  int64_t bound = table_stride * block_size;
  if (max_context_len > 0 && max_context_len < bound) bound = max_context_len;
  const int64_t nlb = cdiv(bound, block_size);
  if (batch * layer_count > 0x3FFFFFFFLL || batch * layer_count * nlb > 0x3FFFFFFFLL)
    return set_error(KVECC_EINVAL, "cache_scrub: sizes exceed 32-bit indexing");
  ScrubArgs a;
  a.cache[0] = k_cache;
  a.cache[1] = v_cache;
  a.table = block_table;
  a.lens = context_lens;
  a.par = nullptr;
  a.stats = stats;
  a.tstride = (uint32_t)table_stride;
  a.lens_stride = (uint32_t)lens_layer_stride;
  a.hkv = (uint32_t)hkv;
  a.g = (uint32_t)g;
  a.rowb = (uint32_t)rowb;
  a.num_blocks = (uint32_t)num_blocks;
  a.layers = (uint32_t)num_layers;
  a.layer_first = (uint32_t)layer_first;
  a.layer_count = (uint32_t)layer_count;
  a.bs = (uint32_t)block_size;
  a.bound = (uint32_t)bound;
  a.nlb = (uint32_t)nlb;
  a.nseg = (uint32_t)(2 * batch * layer_count * nlb);
  a.gpr = (uint32_t)cdiv(g, 4);
  a.gpr_magic = (uint32_t)((1ULL << 32) / a.gpr + 1);
  // mulhi(i, magic) == i / gpr while i * gpr < 2^32; i < hkv * block_size * gpr
  if (codec == KVECC_CODEC_GOLAY_PACKED && hkv * block_size * (int64_t)a.gpr * a.gpr >= (1LL << 32))
    return set_error(KVECC_EINVAL, "cache_scrub: sizes exceed 32-bit indexing");
  if (golay) {
    a.par = golay_parity_table_dev();
    const uint16_t *cor = golay_correct_table_dev();
    if (!a.par || !cor) return KVECC_EHIP;
    if (cor != a.par + 4096) return set_error(KVECC_EHIP, "cache_scrub: golay tables not contiguous");
  }
  const unsigned grid = (unsigned)std::min<int64_t>(a.nseg, (int64_t)cu_count() * kScrubPerCu);
  hipStream_t st = as_stream(stream);
  switch (codec) {
    case KVECC_CODEC_H74:
      KVECC_LAUNCH(cache_scrub_kernel<KVECC_CODEC_H74>, dim3(grid), dim3(kScrubBlock), 0, st, a);
      break;
    case KVECC_CODEC_H84:
      KVECC_LAUNCH(cache_scrub_kernel<KVECC_CODEC_H84>, dim3(grid), dim3(kScrubBlock), 0, st, a);
      break;
    case KVECC_CODEC_GOLAY:
      KVECC_LAUNCH(cache_scrub_kernel<KVECC_CODEC_GOLAY>, dim3(grid), dim3(kScrubBlock), 0, st, a);
      break;
    default:
      KVECC_LAUNCH(cache_scrub_kernel<KVECC_CODEC_GOLAY_PACKED>, dim3(grid), dim3(kScrubBlock), 0, st, a);
      break;
  }
  return check_launch("cache_scrub");
}

}  // extern "C"
