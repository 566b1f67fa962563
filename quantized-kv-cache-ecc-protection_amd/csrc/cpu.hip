// cpu.hip -- the host ("cpu") codec backend: same algebra as the gfx950
// kernels (codec_math.h), run over host memory with std::thread workers.
//
// This is the explicit `backend="cpu"` of kvecc.backends (BASELINE config 1:
// Hamming(7,4) on the host, no GPU) -- never a fallback of the "hip" backend.
// Statistics are plain host uint64 arrays (+=), not the sharded device buffer.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "kvecc_internal.h"

namespace kvecc {
namespace {

int clamp_threads(int threads, int64_t work, int64_t grain) {
  int hw = (int)std::thread::hardware_concurrency();
  if (threads <= 0) threads = hw > 0 ? hw : 1;
  int64_t useful = std::max<int64_t>(1, work / std::max<int64_t>(1, grain));
  return (int)std::max<int64_t>(1, std::min<int64_t>(threads, useful));
}

// run fn(begin, end, thread_index) over [0, n) in `threads` contiguous chunks
// whose boundaries are multiples of `align`
template <class F>
void parallel_for(int64_t n, int threads, int64_t align, F fn) {
  int t = clamp_threads(threads, n, 1 << 16);
  if (t == 1) {
    fn((int64_t)0, n, 0);
    return;
  }
  int64_t chunk = (n + t - 1) / t;
  chunk = (chunk + align - 1) / align * align;
  std::vector<std::thread> pool;
  for (int i = 0; i < t; ++i) {
    int64_t b = i * chunk, e = std::min<int64_t>(n, b + chunk);
    if (b >= e) break;
    pool.emplace_back(fn, b, e, i);
  }
  for (auto &th : pool) th.join();
}

inline uint32_t load4(const uint8_t *p) {
  uint32_t w;
  std::memcpy(&w, p, 4);
  return w;
}
inline void store4(uint8_t *p, uint32_t w) { std::memcpy(p, &w, 4); }

template <class Op>
void map_bytes(const uint8_t *in, uint8_t *out, int64_t n, int threads, Op op) {
  parallel_for(n, threads, 64, [&](int64_t b, int64_t e, int) {
    int64_t i = b;
    for (; i + 4 <= e; i += 4) store4(out + i, op(load4(in + i)));
    for (; i < e; ++i) out[i] = (uint8_t)op(in[i]);
  });
}

struct Acc2 {
  uint64_t a = 0, b = 0;
  char pad[48];
};

void add_stats(uint64_t *stats, const std::vector<Acc2> &acc, int n) {
  if (!stats) return;
  for (auto &x : acc) {
    stats[0] += x.a;
    if (n > 1) stats[1] += x.b;
  }
}

float load_x(const void *x, int dtype, int64_t i) {
  if (dtype == KVECC_F16) return __half2float(reinterpret_cast<const __half *>(x)[i]);
  if (dtype == KVECC_BF16) return __bfloat162float(reinterpret_cast<const __hip_bfloat16 *>(x)[i]);
  return reinterpret_cast<const float *>(x)[i];
}

void store_y(void *y, int dtype, int64_t i, float v) {
  if (dtype == KVECC_F16)
    reinterpret_cast<__half *>(y)[i] = __float2half_rn(v);
  else if (dtype == KVECC_BF16)
    reinterpret_cast<__hip_bfloat16 *>(y)[i] = __float2bfloat16(v);
  else
    reinterpret_cast<float *>(y)[i] = v;
}

bool bad(int64_t n) { return n < 0; }

// the host Golay tables, built on first use: parity[4096], then correct[4096]
// (kvecc_internal.h); the encoders take the first half only
const uint16_t *host_golay_tables() {
  static const struct Tables {
    uint16_t t[8192];
    Tables() {
      build_golay_parity_table(t);
      build_golay_correct_table(t + 4096);
    }
  } tables;
  return tables.t;
}

// Golay word k of cache row `row` (g words a row): 3 little-endian bytes of a
// packed row, or the int32 word (bits 24-31 as stored: golay_decode1 ignores them)
inline uint32_t golay_word(const void *cache, bool packed, int64_t row, int64_t g, int64_t k) {
  if (!packed) return (uint32_t)reinterpret_cast<const int32_t *>(cache)[row * g + k];
  const uint8_t *c = reinterpret_cast<const uint8_t *>(cache) + row * KVECC_GOLAY_PACKED_ROW(g) + 3 * k;
  return (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16;
}

// sequence b's query span (kvecc.h "Query spans"); no spans: the uniform call's (0, q_len)
struct Span {
  int64_t first, count;
};
inline Span span_of(const int32_t *q_spans, int64_t b, int64_t q_len) {
  return q_spans ? Span{q_spans[3 * b], q_spans[3 * b + 1]} : Span{0, q_len};
}

// row index of position `pos` of cache head h in physical block blk, in a
// [blocks, layers, kv_heads, block_size] cache (rows of codewords, and the scales)
inline int64_t cache_slot(int64_t blk, int64_t layers, int64_t layer, int64_t kv_heads, int64_t h,
                          int64_t block_size, int64_t pos) {
  return ((blk * layers + layer) * kv_heads + h) * block_size + pos % block_size;
}

}  // namespace
}  // namespace kvecc

using namespace kvecc;

extern "C" {

KVECC_API int kvecc_cpu_hamming74_encode(const uint8_t *in, uint8_t *out, int64_t n, int threads) {
  if (bad(n)) return set_error(KVECC_EINVAL, "cpu_hamming74_encode: negative n");
  if (n && (!in || !out)) return set_error(KVECC_EINVAL, "cpu_hamming74_encode: null pointer");
  map_bytes(in, out, n, threads, [](uint32_t w) { return h74_encode4(w); });
  return KVECC_OK;
}

KVECC_API int kvecc_cpu_hamming84_encode(const uint8_t *in, uint8_t *out, int64_t n, int threads) {
  if (bad(n)) return set_error(KVECC_EINVAL, "cpu_hamming84_encode: negative n");
  if (n && (!in || !out)) return set_error(KVECC_EINVAL, "cpu_hamming84_encode: null pointer");
  map_bytes(in, out, n, threads, [](uint32_t w) { return h84_encode4(w); });
  return KVECC_OK;
}

KVECC_API int kvecc_cpu_hamming74_decode(const uint8_t *cw, uint8_t *data, uint8_t *flag, int64_t n,
                                         uint64_t *stats, int threads) {
  if (bad(n)) return set_error(KVECC_EINVAL, "cpu_hamming74_decode: negative n");
  if (n && (!cw || !data)) return set_error(KVECC_EINVAL, "cpu_hamming74_decode: null pointer");
  std::vector<Acc2> acc(std::max(1, clamp_threads(threads, n, 1 << 16)));
  parallel_for(n, threads, 64, [&](int64_t b, int64_t e, int t) {
    uint32_t c = 0;
    int64_t i = b;
    for (; i + 4 <= e; i += 4) {
      uint32_t d, f;
      h74_decode4(load4(cw + i), d, f, c);
      store4(data + i, d);
      if (flag) store4(flag + i, f);
    }
    for (; i < e; ++i) {
      uint32_t d, f;
      h74_decode4(cw[i], d, f, c);
      data[i] = (uint8_t)d;
      if (flag) flag[i] = (uint8_t)f;
    }
    acc[t].a += c;
  });
  add_stats(stats, acc, 1);
  return KVECC_OK;
}

KVECC_API int kvecc_cpu_hamming84_decode(const uint8_t *cw, uint8_t *data, uint8_t *etype, int64_t n,
                                         uint64_t *stats, int threads) {
  if (bad(n)) return set_error(KVECC_EINVAL, "cpu_hamming84_decode: negative n");
  if (n && (!cw || !data)) return set_error(KVECC_EINVAL, "cpu_hamming84_decode: null pointer");
  std::vector<Acc2> acc(std::max(1, clamp_threads(threads, n, 1 << 16)));
  parallel_for(n, threads, 64, [&](int64_t b, int64_t e, int t) {
    uint32_t c1 = 0, c2 = 0;
    int64_t i = b;
    for (; i + 4 <= e; i += 4) {
      uint32_t d, ty;
      h84_decode4(load4(cw + i), d, ty, c1, c2);
      store4(data + i, d);
      if (etype) store4(etype + i, ty);
    }
    for (; i < e; ++i) {
      uint32_t d, ty;
      h84_decode4(cw[i], d, ty, c1, c2);
      data[i] = (uint8_t)d;
      if (etype) etype[i] = (uint8_t)ty;
    }
    acc[t].a += c1;
    acc[t].b += c2;
  });
  add_stats(stats, acc, 2);
  return KVECC_OK;
}

KVECC_API int kvecc_cpu_golay_encode(const uint8_t *trip, int32_t *cw, int64_t m, int threads) {
  if (bad(m)) return set_error(KVECC_EINVAL, "cpu_golay_encode: negative m");
  if (m && (!trip || !cw)) return set_error(KVECC_EINVAL, "cpu_golay_encode: null pointer");
  const uint16_t *par = host_golay_tables();
  parallel_for(m, threads, 64, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; ++i) {
      uint32_t d = golay_pack(trip[3 * i], trip[3 * i + 1], trip[3 * i + 2]);
      cw[i] = (int32_t)(d | (uint32_t)par[d] << 12);
    }
  });
  return KVECC_OK;
}

KVECC_API int kvecc_cpu_golay_decode(const int32_t *cw, uint8_t *trip, uint8_t *counts, int64_t m,
                                     uint64_t *stats, int threads) {
  if (bad(m)) return set_error(KVECC_EINVAL, "cpu_golay_decode: negative m");
  if (m && (!trip || !cw)) return set_error(KVECC_EINVAL, "cpu_golay_decode: null pointer");
  const uint16_t *tab = host_golay_tables();
  std::vector<Acc2> acc(std::max(1, clamp_threads(threads, m, 1 << 16)));
  parallel_for(m, threads, 64, [&](int64_t b, int64_t e, int t) {
    uint64_t bits = 0, unc = 0;
    for (int64_t i = b; i < e; ++i) {
      uint32_t c;
      uint32_t d = golay_decode1((uint32_t)cw[i], tab, tab + 4096, c);
      trip[3 * i] = (uint8_t)(d & 0xF);
      trip[3 * i + 1] = (uint8_t)(d >> 4 & 0xF);
      trip[3 * i + 2] = (uint8_t)(d >> 8);
      if (counts) counts[i] = (uint8_t)c;
      bits += c & 3u;
      unc += c >> 2;
    }
    acc[t].a += bits;
    acc[t].b += unc;
  });
  add_stats(stats, acc, 2);
  return KVECC_OK;
}

KVECC_API int kvecc_cpu_golay_encode_rows(const uint8_t *nibbles, int32_t *cw, int64_t rows,
                                          int64_t d, int threads) {
  if (rows < 0 || d < 0) return set_error(KVECC_EINVAL, "cpu_golay_encode_rows: negative size");
  if (rows && d && (!nibbles || !cw)) return set_error(KVECC_EINVAL, "cpu_golay_encode_rows: null pointer");
  const uint16_t *par = host_golay_tables();
  const int64_t g = (d + 2) / 3;
  parallel_for(rows, threads, 1, [&](int64_t b, int64_t e, int) {
    for (int64_t r = b; r < e; ++r)
      for (int64_t k = 0; k < g; ++k) {
        const uint8_t *x = nibbles + r * d + 3 * k;
        const int64_t left = d - 3 * k;  // zero padding of the last group
        uint32_t dw = golay_pack(x[0], left > 1 ? x[1] : 0, left > 2 ? x[2] : 0);
        cw[r * g + k] = (int32_t)(dw | (uint32_t)par[dw] << 12);
      }
  });
  return KVECC_OK;
}

KVECC_API int kvecc_cpu_golay_decode_rows(const int32_t *cw, uint8_t *nibbles, int64_t rows,
                                          int64_t d, uint64_t *stats, int threads) {
  if (rows < 0 || d < 0) return set_error(KVECC_EINVAL, "cpu_golay_decode_rows: negative size");
  if (rows && d && (!nibbles || !cw)) return set_error(KVECC_EINVAL, "cpu_golay_decode_rows: null pointer");
  const uint16_t *tab = host_golay_tables();
  const int64_t g = (d + 2) / 3;
  std::vector<Acc2> acc(std::max(1, clamp_threads(threads, rows, 1)));
  parallel_for(rows, threads, 1, [&](int64_t b, int64_t e, int t) {
    uint64_t bits = 0, unc = 0;
    for (int64_t r = b; r < e; ++r)
      for (int64_t k = 0; k < g; ++k) {
        uint32_t c;
        const uint32_t dw = golay_decode1((uint32_t)cw[r * g + k], tab, tab + 4096, c);
        bits += c & 3u;
        unc += c >> 2;
        uint8_t *o = nibbles + r * d + 3 * k;
        const int64_t left = d - 3 * k;
        o[0] = (uint8_t)(dw & 0xF);
        if (left > 1) o[1] = (uint8_t)(dw >> 4 & 0xF);
        if (left > 2) o[2] = (uint8_t)(dw >> 8);
      }
    acc[t].a += bits;
    acc[t].b += unc;
  });
  add_stats(stats, acc, 2);
  return KVECC_OK;
}

// packed Golay storage (host twins of packed.hip): one group of 8 codewords
// (12 nibble bytes, 24 codeword bytes, 1 flag byte) per work item
KVECC_API int kvecc_cpu_golay_encode_packed(const uint8_t *nibbles, uint8_t *codewords, int64_t m,
                                            int threads) {
  if (m < 0) return set_error(KVECC_EINVAL, "cpu_golay_encode_packed: negative m");
  if (m && (!nibbles || !codewords)) return set_error(KVECC_EINVAL, "cpu_golay_encode_packed: null pointer");
  const uint16_t *par = host_golay_tables();
  parallel_for((m + 7) / 8, threads, 1, [&](int64_t b, int64_t e, int) {
    for (int64_t g = b; g < e; ++g)
      for (int64_t k = 8 * g; k < m && k < 8 * g + 8; ++k) {
        uint32_t d = 0;
        for (int u = 0; u < 3; ++u) {
          const int64_t j = 3 * k + u;
          d |= (uint32_t)(nibbles[j >> 1] >> (4 * (j & 1)) & 0xF) << (4 * u);
        }
        const uint32_t c = d | (uint32_t)par[d] << 12;
        codewords[3 * k] = (uint8_t)c;
        codewords[3 * k + 1] = (uint8_t)(c >> 8);
        codewords[3 * k + 2] = (uint8_t)(c >> 16);
      }
  });
  return KVECC_OK;
}

KVECC_API int kvecc_cpu_golay_decode_packed(const uint8_t *codewords, uint8_t *nibbles,
                                            uint8_t *uncorrectable, int64_t m, uint64_t *stats,
                                            int threads) {
  if (m < 0) return set_error(KVECC_EINVAL, "cpu_golay_decode_packed: negative m");
  if (m && (!nibbles || !codewords)) return set_error(KVECC_EINVAL, "cpu_golay_decode_packed: null pointer");
  const uint16_t *tab = host_golay_tables();
  const int64_t groups = (m + 7) / 8;
  std::vector<Acc2> acc(std::max(1, clamp_threads(threads, groups, 1 << 10)));
  parallel_for(groups, threads, 1, [&](int64_t b, int64_t e, int t) {
    uint64_t bits = 0, unc = 0;
    for (int64_t g = b; g < e; ++g) {
      uint32_t fl = 0;
      for (int64_t k = 8 * g; k < m && k < 8 * g + 8; ++k) {
        const uint32_t c = codewords[3 * k] | (uint32_t)codewords[3 * k + 1] << 8 |
                           (uint32_t)codewords[3 * k + 2] << 16;
        uint32_t cnt;
        const uint32_t d = golay_decode1(c, tab, tab + 4096, cnt);
        bits += cnt & 3u;
        unc += cnt >> 2;
        fl |= (cnt >> 2) << (k - 8 * g);
        for (int u = 0; u < 3; ++u) {
          const int64_t j = 3 * k + u;
          const uint32_t v = d >> (4 * u) & 0xFu;
          if ((j & 1) == 0)
            nibbles[j >> 1] = (uint8_t)v;  // high nibble: next value, or zero padding
          else
            nibbles[j >> 1] = (uint8_t)((nibbles[j >> 1] & 0x0Fu) | v << 4);
        }
      }
      if (uncorrectable) uncorrectable[g] = (uint8_t)fl;
    }
    acc[t].a += bits;
    acc[t].b += unc;
  });
  add_stats(stats, acc, 2);
  return KVECC_OK;
}

// packed Hamming(8,4) (host twins of packed.hip): groups of 4 values share a
// type byte and two nibble bytes, one group per work item
KVECC_API int kvecc_cpu_hamming84_encode_packed(const uint8_t *nibbles, uint8_t *codewords,
                                                int64_t n, int threads) {
  if (n < 0) return set_error(KVECC_EINVAL, "cpu_hamming84_encode_packed: negative n");
  if (n && (!nibbles || !codewords)) return set_error(KVECC_EINVAL, "cpu_hamming84_encode_packed: null pointer");
  parallel_for(n, threads, 64, [&](int64_t b, int64_t e, int) {
    for (int64_t j = b; j < e; ++j)
      codewords[j] = (uint8_t)(h84_encode4(nibbles[j >> 1] >> (4 * (j & 1)) & 0xFu) & 0xFFu);
  });
  return KVECC_OK;
}

KVECC_API int kvecc_cpu_hamming84_decode_packed(const uint8_t *codewords, uint8_t *nibbles,
                                                uint8_t *error_types, int64_t n, uint64_t *stats,
                                                int threads) {
  if (n < 0) return set_error(KVECC_EINVAL, "cpu_hamming84_decode_packed: negative n");
  if (n && (!nibbles || !codewords)) return set_error(KVECC_EINVAL, "cpu_hamming84_decode_packed: null pointer");
  const int64_t groups = (n + 3) / 4;
  std::vector<Acc2> acc(std::max(1, clamp_threads(threads, groups, 1 << 14)));
  parallel_for(groups, threads, 16, [&](int64_t b, int64_t e, int t) {
    uint32_t n1 = 0, n2 = 0;
    for (int64_t g = b; g < e; ++g) {
      uint32_t tb = 0;
      for (int64_t j = 4 * g; j < n && j < 4 * g + 4; ++j) {
        uint32_t d, ty;
        h84_decode4(codewords[j], d, ty, n1, n2);
        if ((j & 1) == 0)
          nibbles[j >> 1] = (uint8_t)d;  // high nibble: next value, or zero padding
        else
          nibbles[j >> 1] = (uint8_t)((nibbles[j >> 1] & 0x0Fu) | d << 4);
        tb |= ty << (2 * (j & 3));
      }
      if (error_types) error_types[g] = (uint8_t)tb;
    }
    acc[t].a += n1;
    acc[t].b += n2;
  });
  add_stats(stats, acc, 2);
  return KVECC_OK;
}

}  // extern "C"

template <typename T>
static int cpu_inject(const T *in, T *out, uint8_t *counts, int64_t n, int n_bits, int64_t seed,
                      float ber, int64_t global_n, int64_t offset0, uint64_t *stats, int threads,
                      const char *name) {
  if (n < 0 || global_n < 0 || offset0 < 0) return set_error(KVECC_EINVAL, "%s: negative size", name);
  if (n && (!in || !out)) return set_error(KVECC_EINVAL, "%s: null pointer", name);
  if (offset0 + n > global_n) return set_error(KVECC_EINVAL, "%s: shard exceeds global_n", name);
  const uint32_t seedmul = (uint32_t)((uint64_t)seed * (uint64_t)(uint32_t)((uint64_t)global_n * (uint64_t)n_bits));
  const uint32_t thr = kvecc_ber_threshold(ber);
  const int nb = sizeof(T) == 1 ? (n_bits < 1 ? 1 : (n_bits > 8 ? 8 : n_bits))
                                : (n_bits < 0 ? 0 : (n_bits > 24 ? 24 : n_bits));
  std::vector<Acc2> acc(std::max(1, clamp_threads(threads, n, 1 << 12)));
  parallel_for(n, threads, 64, [&](int64_t b, int64_t e, int t) {
    uint64_t flips = 0, hit = 0;
    for (int64_t i = b; i < e; ++i) {
      const uint32_t g = (uint32_t)(offset0 + i);
      const uint32_t m = philox_flip_mask<-1>(seedmul + g * (uint32_t)n_bits, g, thr, nb);
      out[i] = (T)((uint32_t)in[i] ^ m);
      uint32_t c = __builtin_popcount(m);
      if (counts) counts[i] = (uint8_t)c;
      flips += c;
      hit += c != 0;
    }
    acc[t].a += flips;
    acc[t].b += hit;
  });
  add_stats(stats, acc, 2);
  return KVECC_OK;
}

template <typename T>
static int cpu_inject_rows(const T *in, T *out, int64_t rows, int64_t row_len, int n_bits,
                           int64_t seed_base, float ber, uint64_t *stats, int threads,
                           const char *name) {
  if (rows < 0 || row_len < 0) return set_error(KVECC_EINVAL, "%s: negative size", name);
  const int64_t total = rows * row_len;
  if (total && (!in || !out)) return set_error(KVECC_EINVAL, "%s: null pointer", name);
  const uint32_t rowmul = (uint32_t)((uint64_t)row_len * (uint64_t)n_bits);
  const uint32_t sb = (uint32_t)(uint64_t)seed_base;
  const uint32_t thr = kvecc_ber_threshold(ber);
  const int nb = sizeof(T) == 1 ? (n_bits < 1 ? 1 : (n_bits > 8 ? 8 : n_bits))
                                : (n_bits < 0 ? 0 : (n_bits > 24 ? 24 : n_bits));
  std::vector<Acc2> acc(std::max(1, clamp_threads(threads, total, 1 << 12)));
  parallel_for(total, threads, 64, [&](int64_t b, int64_t e, int t) {
    uint64_t flips = 0, hit = 0;
    for (int64_t i = b; i < e; ++i) {
      const int64_t r = i / row_len;
      const uint32_t j = (uint32_t)(i - r * row_len);
      const uint32_t m = philox_flip_mask<-1>((sb + (uint32_t)r) * rowmul + j * (uint32_t)n_bits,
                                              j, thr, nb);
      out[i] = (T)((uint32_t)in[i] ^ m);
      uint32_t c = __builtin_popcount(m);
      flips += c;
      hit += c != 0;
    }
    acc[t].a += flips;
    acc[t].b += hit;
  });
  add_stats(stats, acc, 2);
  return KVECC_OK;
}

template <typename T>
static int cpu_inject_vec(const T *in, T *out, uint8_t *counts, int64_t n, int n_bits,
                          int64_t seed, float ber, uint64_t *stats, int threads, const char *name) {
  if (n < 0) return set_error(KVECC_EINVAL, "%s: negative n", name);
  if (n && (!in || !out)) return set_error(KVECC_EINVAL, "%s: null pointer", name);
  const uint32_t seedn = (uint32_t)((uint64_t)seed * (uint64_t)n);
  const uint32_t thr = kvecc_ber_threshold(ber);
  const int nb = sizeof(T) == 1 ? (n_bits < 1 ? 1 : (n_bits > 8 ? 8 : n_bits))
                                : (n_bits < 0 ? 0 : (n_bits > 24 ? 24 : n_bits));
  std::vector<Acc2> acc(std::max(1, clamp_threads(threads, n, 1 << 12)));
  parallel_for(n, threads, 64, [&](int64_t b, int64_t e, int t) {
    uint64_t flips = 0, hit = 0;
    for (int64_t i = b; i < e; ++i) {
      const uint32_t m = philox_flip_mask_vec(seedn, (uint32_t)n, (uint32_t)i, thr, nb);
      out[i] = (T)((uint32_t)in[i] ^ m);
      uint32_t c = __builtin_popcount(m);
      if (counts) counts[i] = (uint8_t)c;
      flips += c;
      hit += c != 0;
    }
    acc[t].a += flips;
    acc[t].b += hit;
  });
  add_stats(stats, acc, 2);
  return KVECC_OK;
}

extern "C" {

KVECC_API int kvecc_cpu_inject_u8(const uint8_t *in, uint8_t *out, uint8_t *counts, int64_t n,
                                  int n_bits, int64_t seed, float ber, int64_t global_n,
                                  int64_t offset0, uint64_t *stats, int threads) {
  return cpu_inject<uint8_t>(in, out, counts, n, n_bits, seed, ber, global_n, offset0, stats,
                             threads, "cpu_inject_u8");
}

KVECC_API int kvecc_cpu_inject_i32(const int32_t *in, int32_t *out, uint8_t *counts, int64_t n,
                                   int n_bits, int64_t seed, float ber, int64_t global_n,
                                   int64_t offset0, uint64_t *stats, int threads) {
  return cpu_inject<int32_t>(in, out, counts, n, n_bits, seed, ber, global_n, offset0, stats,
                             threads, "cpu_inject_i32");
}

KVECC_API int kvecc_cpu_inject_u8_vectorized(const uint8_t *in, uint8_t *out, uint8_t *counts,
                                             int64_t n, int n_bits, int64_t seed, float ber,
                                             uint64_t *stats, int threads) {
  return cpu_inject_vec<uint8_t>(in, out, counts, n, n_bits, seed, ber, stats, threads,
                                 "cpu_inject_u8_vectorized");
}

KVECC_API int kvecc_cpu_inject_i32_vectorized(const int32_t *in, int32_t *out, uint8_t *counts,
                                              int64_t n, int n_bits, int64_t seed, float ber,
                                              uint64_t *stats, int threads) {
  return cpu_inject_vec<int32_t>(in, out, counts, n, n_bits, seed, ber, stats, threads,
                                 "cpu_inject_i32_vectorized");
}

KVECC_API int kvecc_cpu_inject_rows_u8(const uint8_t *in, uint8_t *out, int64_t rows,
                                       int64_t row_len, int n_bits, int64_t seed_base, float ber,
                                       uint64_t *stats, int threads) {
  return cpu_inject_rows<uint8_t>(in, out, rows, row_len, n_bits, seed_base, ber, stats, threads,
                                  "cpu_inject_rows_u8");
}

KVECC_API int kvecc_cpu_inject_rows_i32(const int32_t *in, int32_t *out, int64_t rows,
                                        int64_t row_len, int n_bits, int64_t seed_base, float ber,
                                        uint64_t *stats, int threads) {
  return cpu_inject_rows<int32_t>(in, out, rows, row_len, n_bits, seed_base, ber, stats, threads,
                                  "cpu_inject_rows_i32");
}

KVECC_API int kvecc_cpu_count_ne_u8(const uint8_t *a, const uint8_t *b, int64_t n, uint64_t *stats,
                                    int threads) {
  if (n < 0) return set_error(KVECC_EINVAL, "cpu_count_ne_u8: negative n");
  if (n == 0) return KVECC_OK;
  if (!a || !b || !stats) return set_error(KVECC_EINVAL, "cpu_count_ne_u8: null pointer");
  std::vector<Acc2> acc(std::max(1, clamp_threads(threads, n, 1 << 16)));
  parallel_for(n, threads, 1 << 16, [&](int64_t lo, int64_t hi, int t) {
    uint64_t c = 0;
    for (int64_t i = lo; i < hi; ++i) c += a[i] != b[i];
    acc[t].a += c;
  });
  add_stats(stats, acc, 1);
  return KVECC_OK;
}

KVECC_API int kvecc_cpu_interpolate(const uint8_t *q, const uint8_t *err, uint8_t *out,
                                    int64_t outer, int64_t len, int64_t inner, int threads) {
  if (outer < 0 || len < 0 || inner < 0) return set_error(KVECC_EINVAL, "cpu_interpolate: negative size");
  const int64_t total = outer * len * inner;
  if (total && (!q || !err || !out)) return set_error(KVECC_EINVAL, "cpu_interpolate: null pointer");
  parallel_for(total, threads, 64, [&](int64_t b, int64_t e, int) {
    for (int64_t i = b; i < e; ++i) {
      const int64_t l = (i / inner) % len;
      const int64_t row = i - l * inner;
      const uint32_t left = q[row + (l > 0 ? l - 1 : 0) * inner];
      const uint32_t right = q[row + (l + 1 < len ? l + 1 : len - 1) * inner];
      out[i] = (uint8_t)interp_word(q[i], left, right, err[i]);
    }
  });
  return KVECC_OK;
}

KVECC_API int kvecc_cpu_quantize_encode_rows(const void *x, int x_dtype, int codec,
                                             int scale_rule, uint8_t *cw, float *scales,
                                             int64_t rows, int64_t d, int threads) {
  if (rows < 0 || d < 0) return set_error(KVECC_EINVAL, "cpu_quantize_encode_rows: negative size");
  if (rows == 0) return KVECC_OK;
  if (d == 0) return set_error(KVECC_EINVAL, "cpu_quantize_encode_rows: empty rows");
  if (!x || !cw || !scales) return set_error(KVECC_EINVAL, "cpu_quantize_encode_rows: null pointer");
  if (x_dtype < KVECC_F32 || x_dtype > KVECC_BF16)
    return set_error(KVECC_EINVAL, "cpu_quantize_encode_rows: bad dtype %d", x_dtype);
  if (codec < KVECC_CODEC_NONE || codec > KVECC_CODEC_H84)
    return set_error(KVECC_EINVAL, "cpu_quantize_encode_rows: bad codec %d", codec);
  if (scale_rule != KVECC_SCALE_DIV7 && scale_rule != KVECC_SCALE_MUL_INV7)
    return set_error(KVECC_EINVAL, "cpu_quantize_encode_rows: bad scale rule %d", scale_rule);
  parallel_for(rows, threads, 1, [&](int64_t b, int64_t e, int) {
    for (int64_t r = b; r < e; ++r) {
      float amax = 0.0f;
      for (int64_t j = 0; j < d; ++j) amax = std::max(amax, std::fabs(load_x(x, x_dtype, r * d + j)));
      const float scale = row_scale(amax, scale_rule);
      scales[r] = scale;
      for (int64_t j = 0; j < d; ++j)
        cw[r * d + j] = (uint8_t)encode_nibble(quantize_nibble(load_x(x, x_dtype, r * d + j), scale), codec);
    }
  });
  return KVECC_OK;
}

KVECC_API int kvecc_cpu_decode_dequant_h84_rows(const uint8_t *cw, const float *scales, void *out,
                                                int out_dtype, int64_t rows, int64_t d,
                                                int zero_doubles, uint64_t *stats, int threads) {
  if (rows < 0 || d < 0) return set_error(KVECC_EINVAL, "cpu_decode_dequant_h84_rows: negative size");
  if (rows == 0 || d == 0) return KVECC_OK;
  if (!cw || !scales || !out) return set_error(KVECC_EINVAL, "cpu_decode_dequant_h84_rows: null pointer");
  if (out_dtype < KVECC_F32 || out_dtype > KVECC_BF16)
    return set_error(KVECC_EINVAL, "cpu_decode_dequant_h84_rows: bad dtype %d", out_dtype);
  std::vector<Acc2> acc(std::max(1, clamp_threads(threads, rows, 1)));
  parallel_for(rows, threads, 1, [&](int64_t b, int64_t e, int t) {
    uint32_t n1 = 0, n2 = 0;
    for (int64_t r = b; r < e; ++r)
      for (int64_t j = 0; j < d; ++j) {
        uint32_t data, type;
        h84_decode4(cw[r * d + j], data, type, n1, n2);
        if (zero_doubles && type == 2) data = 0;
        store_y(out, out_dtype, r * d + j, ((float)data - 8.0f) * scales[r]);
      }
    acc[t].a += n1;
    acc[t].b += n2;
  });
  add_stats(stats, acc, 2);
  return KVECC_OK;
}

// ---- shim write / read (host twins of shim.hip) ------------------------------

// what a shim write needs to store one (side, row): shared by the overwrite
// and the append twin
struct HostShimRows {
  const void *x[2];  // K, V: contiguous [rows, d]
  void *cache[2];
  float *scales[2];
  int x_dtype, codec, scale_rule, n_bits, nb;
  bool inj, golay, packed;
  int64_t d, g;
  uint32_t seed0, rowmul, thr;

  int init(const char *fn, const void *k, const void *v, int x_dtype_, int64_t d_, int codec_, int scale_rule_,
           int n_bits_, int inject, float ber, int64_t seed0_, void *k_cache, void *v_cache, float *k_scales,
           float *v_scales, const int32_t *block_table, int64_t num_layers, int64_t block_size, int64_t layer) {
    if (d_ < 1) return set_error(KVECC_EINVAL, "%s: empty rows", fn);
    if (codec_ < KVECC_CODEC_NONE || codec_ > KVECC_CODEC_GOLAY_PACKED)
      return set_error(KVECC_EINVAL, "%s: bad codec %d", fn, codec_);
    if (scale_rule_ != KVECC_SCALE_DIV7 && scale_rule_ != KVECC_SCALE_MUL_INV7)
      return set_error(KVECC_EINVAL, "%s: bad scale rule %d", fn, scale_rule_);
    if (x_dtype_ < KVECC_F32 || x_dtype_ > KVECC_BF16) return set_error(KVECC_EINVAL, "%s: bad dtype %d", fn, x_dtype_);
    if (num_layers < 1 || block_size < 1 || layer < 0 || layer >= num_layers)
      return set_error(KVECC_EINVAL, "%s: bad cache geometry", fn);
    if (!k || !v || !k_cache || !v_cache || !k_scales || !v_scales || !block_table)
      return set_error(KVECC_EINVAL, "%s: null pointer", fn);
    x[0] = k, x[1] = v;
    cache[0] = k_cache, cache[1] = v_cache;
    scales[0] = k_scales, scales[1] = v_scales;
    x_dtype = x_dtype_, codec = codec_, scale_rule = scale_rule_, n_bits = n_bits_, d = d_;
    packed = codec == KVECC_CODEC_GOLAY_PACKED;
    golay = codec == KVECC_CODEC_GOLAY || packed;
    g = golay ? (d + 2) / 3 : d;
    seed0 = (uint32_t)(uint64_t)seed0_;
    rowmul = (uint32_t)((uint64_t)g * (uint64_t)n_bits);
    thr = kvecc_ber_threshold(ber);
    inj = inject != 0 && ber > 0.0f;
    nb = golay ? (n_bits < 0 ? 0 : (n_bits > 24 ? 24 : n_bits)) : (n_bits < 1 ? 1 : (n_bits > 8 ? 8 : n_bits));
    return KVECC_OK;
  }

  // input row r of side `side` -> cache row `slot`; nib: 3 g + 3 scratch bytes
  void store(int side, int64_t r, int64_t slot, std::vector<uint8_t> &nib) const { store(side, r, r, slot, nib); }
  // the same with the injection row index `ri` apart from the input row r (ragged appends)
  void store(int side, int64_t r, int64_t ri, int64_t slot, std::vector<uint8_t> &nib) const {
    const uint32_t key0 = (seed0 + (uint32_t)ri + (uint32_t)side) * rowmul;
    const void *xs = x[side];
    float amax = 0.0f;
    for (int64_t j = 0; j < d; ++j) amax = std::max(amax, std::fabs(load_x(xs, x_dtype, r * d + j)));
    const float scale = row_scale(amax, scale_rule);
    scales[side][slot] = scale;
    if (!golay) {
      uint8_t *c = reinterpret_cast<uint8_t *>(cache[side]) + slot * g;
      for (int64_t j = 0; j < d; ++j) {
        uint32_t cw = encode_nibble(quantize_nibble(load_x(xs, x_dtype, r * d + j), scale), codec);
        if (inj) cw ^= philox_flip_mask<-1>(key0 + (uint32_t)j * (uint32_t)n_bits, (uint32_t)j, thr, nb);
        c[j] = (uint8_t)cw;
      }
      return;
    }
    std::fill(nib.begin(), nib.end(), 0);
    for (int64_t j = 0; j < d; ++j) nib[j] = (uint8_t)quantize_nibble(load_x(xs, x_dtype, r * d + j), scale);
    for (int64_t q = 0; q < g; ++q) {
      const uint32_t dw = golay_pack(nib[3 * q], nib[3 * q + 1], nib[3 * q + 2]);
      uint32_t cw = dw | golay_parity12(dw) << 12;
      if (inj) cw ^= philox_flip_mask<-1>(key0 + (uint32_t)q * (uint32_t)n_bits, (uint32_t)q, thr, nb);
      if (packed) {
        uint8_t *c = reinterpret_cast<uint8_t *>(cache[side]) + slot * KVECC_GOLAY_PACKED_ROW(g) + 3 * q;
        c[0] = (uint8_t)cw;
        c[1] = (uint8_t)(cw >> 8);
        c[2] = (uint8_t)(cw >> 16);
      } else {
        reinterpret_cast<int32_t *>(cache[side])[slot * g + q] = (int32_t)cw;
      }
    }
  }
};

KVECC_API int kvecc_cpu_shim_write(const void *k, const void *v, int x_dtype, int64_t batch,
                                   int64_t seq, int64_t hkv, int64_t d, int codec,
                                   int scale_rule, int n_bits, int inject, float ber,
                                   int64_t seed0, void *k_cache,
                                   void *v_cache, float *k_scales, float *v_scales,
                                   const int32_t *block_table, int64_t num_layers,
                                   int64_t block_size, int64_t layer, int threads) {
  if (batch < 0 || seq < 0 || hkv < 0 || d < 0) return set_error(KVECC_EINVAL, "cpu_shim_write: negative size");
  if (batch == 0 || seq == 0 || hkv == 0) return KVECC_OK;
  HostShimRows rows;
  const int rc = rows.init("cpu_shim_write", k, v, x_dtype, d, codec, scale_rule, n_bits, inject, ber, seed0, k_cache,
                           v_cache, k_scales, v_scales, block_table, num_layers, block_size, layer);
  if (rc != KVECC_OK) return rc;
  const int64_t per_side = seq * hkv;
  parallel_for(2 * per_side, threads, 1, [&](int64_t b, int64_t e, int) {
    std::vector<uint8_t> nib(3 * rows.g + 3);
    for (int64_t item = b; item < e; ++item) {
      const int side = (int)(item / per_side);
      const int64_t rr = item - side * per_side;
      const int64_t pos = rr / hkv, h = rr - pos * hkv;
      const int64_t r = (batch - 1) * per_side + rr;  // only the last batch is stored
      const int64_t slot = cache_slot(block_table[pos / block_size], num_layers, layer, hkv, h, block_size, pos);
      rows.store(side, r, slot, nib);
    }
  });
  return KVECC_OK;
}

// host twin of kvecc_shim_append: same placement, skip rules and seeds
KVECC_API int kvecc_cpu_shim_append(const void *k, const void *v, int x_dtype, int64_t batch,
                                    int64_t q_len, int64_t hkv, int64_t d, int codec,
                                    int scale_rule, int n_bits, int inject, float ber,
                                    int64_t seed0, void *k_cache, void *v_cache, float *k_scales,
                                    float *v_scales, const int32_t *block_table,
                                    int64_t table_stride, const int32_t *start_pos,
                                    int64_t num_layers, int64_t block_size, int64_t layer,
                                    int threads) {
  if (batch < 0 || q_len < 0 || hkv < 0 || d < 0) return set_error(KVECC_EINVAL, "cpu_shim_append: negative size");
  if (batch == 0 || q_len == 0 || hkv == 0) return KVECC_OK;
  HostShimRows rows;
  const int rc = rows.init("cpu_shim_append", k, v, x_dtype, d, codec, scale_rule, n_bits, inject, ber, seed0, k_cache,
                           v_cache, k_scales, v_scales, block_table, num_layers, block_size, layer);
  if (rc != KVECC_OK) return rc;
  if (table_stride < 1) return set_error(KVECC_EINVAL, "cpu_shim_append: table stride %lld < 1", (long long)table_stride);
  if (!start_pos) return set_error(KVECC_EINVAL, "cpu_shim_append: null pointer");
  const int64_t per_side = batch * q_len * hkv;
  parallel_for(2 * per_side, threads, 1, [&](int64_t b0, int64_t e0, int) {
    std::vector<uint8_t> nib(3 * rows.g + 3);
    for (int64_t item = b0; item < e0; ++item) {
      const int side = (int)(item / per_side);
      const int64_t r = item - side * per_side;  // (b * q_len + t) * hkv + h
      const int64_t bt = r / hkv, h = r - bt * hkv;
      const int64_t b = bt / q_len, t = bt - b * q_len;
      if (start_pos[b] < 0) continue;
      const int64_t p = (int64_t)start_pos[b] + t, lb = p / block_size;
      if (lb >= table_stride) continue;
      const int64_t blk = block_table[b * table_stride + lb];
      if (blk < 0) continue;
      rows.store(side, r, cache_slot(blk, num_layers, layer, hkv, h, block_size, p), nib);
    }
  });
  return KVECC_OK;
}

// host twin of kvecc_shim_append_ragged: the span rule (kvecc.h "Query spans"),
// then kvecc_cpu_shim_append's placement and skip rules on the valid tokens
KVECC_API int kvecc_cpu_shim_append_ragged(const void *k, const void *v, int x_dtype, int64_t batch,
                                           int64_t q_max, int64_t hkv, int64_t d, int codec,
                                           int scale_rule, int n_bits, int inject, float ber,
                                           int64_t seed0, void *k_cache, void *v_cache, float *k_scales,
                                           float *v_scales, const int32_t *block_table,
                                           int64_t table_stride, const int32_t *start_pos,
                                           const int32_t *q_spans, int64_t num_layers,
                                           int64_t block_size, int64_t layer, int threads) {
  if (batch < 0 || q_max < 0 || hkv < 0 || d < 0)
    return set_error(KVECC_EINVAL, "cpu_shim_append_ragged: negative size");
  if (!q_spans) return set_error(KVECC_EINVAL, "cpu_shim_append_ragged: null q_spans");
  if (batch == 0 || q_max == 0 || hkv == 0) return KVECC_OK;
  HostShimRows rows;
  const int rc = rows.init("cpu_shim_append_ragged", k, v, x_dtype, d, codec, scale_rule, n_bits, inject, ber, seed0,
                           k_cache, v_cache, k_scales, v_scales, block_table, num_layers, block_size, layer);
  if (rc != KVECC_OK) return rc;
  if (table_stride < 1)
    return set_error(KVECC_EINVAL, "cpu_shim_append_ragged: table stride %lld < 1", (long long)table_stride);
  if (!start_pos) return set_error(KVECC_EINVAL, "cpu_shim_append_ragged: null pointer");
  const int64_t per_side = batch * q_max * hkv;
  parallel_for(2 * per_side, threads, 1, [&](int64_t b0, int64_t e0, int) {
    std::vector<uint8_t> nib(3 * rows.g + 3);
    for (int64_t item = b0; item < e0; ++item) {
      const int side = (int)(item / per_side);
      const int64_t r = item - side * per_side;  // (b * q_max + t) * hkv + h: the input row
      const int64_t bt = r / hkv, h = r - bt * hkv;
      const int64_t b = bt / q_max, t = bt - b * q_max;
      const auto [first, count] = span_of(q_spans, b, q_max);
      const int64_t base = q_spans[3 * b + 2];
      if (first < 0 || t < first || t >= std::min(first + count, q_max)) continue;  // padding
      const int64_t ri = (base + t - first) * hkv + h;  // dense over the valid tokens
      if (start_pos[b] < 0) continue;
      const int64_t p = (int64_t)start_pos[b] + (t - first), lb = p / block_size;
      if (lb >= table_stride) continue;
      const int64_t blk = block_table[b * table_stride + lb];
      if (blk < 0) continue;
      rows.store(side, r, ri, cache_slot(blk, num_layers, layer, hkv, h, block_size, p), nib);
    }
  });
  return KVECC_OK;
}

KVECC_API int kvecc_cpu_shim_read(const void *k_cache, const void *v_cache, const float *k_scales,
                                  const float *v_scales, const int32_t *block_table, int64_t ctx,
                                  int64_t hkv, int64_t d, int64_t num_layers, int64_t block_size,
                                  int64_t layer, int codec, int interp, void *k_out, void *v_out,
                                  int out_dtype, uint64_t *stats, int threads) {
  if (ctx < 0 || hkv < 0 || d < 0) return set_error(KVECC_EINVAL, "cpu_shim_read: negative size");
  if (ctx == 0 || hkv == 0 || d == 0) return KVECC_OK;
  if (codec < KVECC_CODEC_NONE || codec > KVECC_CODEC_GOLAY_PACKED)
    return set_error(KVECC_EINVAL, "cpu_shim_read: bad codec %d", codec);
  if (interp && codec != KVECC_CODEC_H84)
    return set_error(KVECC_EINVAL, "cpu_shim_read: interpolation needs the hamming84 codec");
  if (out_dtype < KVECC_F32 || out_dtype > KVECC_BF16)
    return set_error(KVECC_EINVAL, "cpu_shim_read: bad dtype %d", out_dtype);
  if (num_layers < 1 || block_size < 1 || layer < 0 || layer >= num_layers)
    return set_error(KVECC_EINVAL, "cpu_shim_read: bad cache geometry");
  if (!k_cache || !v_cache || !k_scales || !v_scales || !block_table || !k_out || !v_out)
    return set_error(KVECC_EINVAL, "cpu_shim_read: null pointer");
  const uint16_t *tab = host_golay_tables();
  const bool packed = codec == KVECC_CODEC_GOLAY_PACKED;
  const bool golay = codec == KVECC_CODEC_GOLAY || packed;
  const int64_t g = golay ? (d + 2) / 3 : d;
  auto slot_of = [&](int64_t l, int64_t h) {
    return cache_slot(block_table[l / block_size], num_layers, layer, hkv, h, block_size, l);
  };
  const int64_t per_side = hkv * ctx;
  const std::vector<uint8_t> zero_row(golay ? 0 : (size_t)d, 0);  // a missing block's codewords
  std::vector<Acc2> acc(std::max(1, clamp_threads(threads, 2 * per_side, 1)));
  parallel_for(2 * per_side, threads, 1, [&](int64_t b, int64_t e, int t) {
    uint32_t n1 = 0, n2 = 0;
    uint64_t bits = 0, unc = 0;
    for (int64_t item = b; item < e; ++item) {
      const int side = (int)(item / per_side);
      const int64_t hl = item - side * per_side;
      const int64_t h = hl / ctx, l = hl % ctx;
      const int64_t slot = slot_of(l, h);
      void *out = side ? v_out : k_out;
      const int64_t o = (h * ctx + l) * d;
      if (block_table[l / block_size] < 0) {  // no physical block: zeros
        for (int64_t j = 0; j < d; ++j) store_y(out, out_dtype, o + j, 0.0f);
        continue;
      }
      const float s = (side ? v_scales : k_scales)[slot];
      if (golay) {
        const void *cache = side ? v_cache : k_cache;
        for (int64_t q = 0; q < g; ++q) {
          uint32_t cnt;
          const uint32_t dw = golay_decode1(golay_word(cache, packed, slot, g, q), tab, tab + 4096, cnt);
          bits += cnt & 3u;
          unc += cnt >> 2;
          for (int64_t u = 0; u < 3 && 3 * q + u < d; ++u)
            store_y(out, out_dtype, o + 3 * q + u, ((float)(dw >> (4 * u) & 0xFu) - 8.0f) * s);
        }
        continue;
      }
      const uint8_t *base = reinterpret_cast<const uint8_t *>(side ? v_cache : k_cache);
      const uint8_t *c = base + slot * d;
      // neighbours in a missing block read as zero codewords (the device kernels do the same)
      const int64_t ll = l > 0 ? l - 1 : 0, lr = l + 1 < ctx ? l + 1 : ctx - 1;
      const uint8_t *cl = block_table[ll / block_size] < 0 ? zero_row.data() : base + slot_of(ll, h) * d;
      const uint8_t *cr = block_table[lr / block_size] < 0 ? zero_row.data() : base + slot_of(lr, h) * d;
      for (int64_t j = 0; j < d; ++j) {
        uint32_t q = c[j], type = 0;
        if (codec == KVECC_CODEC_H84) {
          h84_decode4(c[j], q, type, n1, n2);
          if (interp) {
            uint32_t ql, qr, tt, u1 = 0, u2 = 0;
            h84_decode4(cl[j], ql, tt, u1, u2);
            h84_decode4(cr[j], qr, tt, u1, u2);
            q = interp_word(q, ql, qr, type) & 0xFFu;
          }
        } else if (codec == KVECC_CODEC_H74) {
          h74_decode4(c[j], q, type, n1);
        }
        store_y(out, out_dtype, o + j, ((float)q - 8.0f) * s);
      }
    }
    acc[t].a += golay ? bits : n1;
    acc[t].b += golay ? unc : n2;
  });
  add_stats(stats, acc, 2);
  return KVECC_OK;
}

KVECC_API int kvecc_cpu_shim_read_batch(const void *k_cache, const void *v_cache,
                                        const float *k_scales, const float *v_scales,
                                        const int32_t *block_table, int64_t table_stride,
                                        int64_t batch, int64_t ctx, int64_t hkv, int64_t d,
                                        int64_t num_layers, int64_t block_size, int64_t layer,
                                        int codec, int interp, void *k_out, void *v_out,
                                        int out_dtype, uint64_t *stats, int threads) {
  if (batch < 0) return set_error(KVECC_EINVAL, "cpu_shim_read_batch: negative batch");
  if (batch > 1 && ctx > 0 && table_stride < (ctx + block_size - 1) / std::max<int64_t>(block_size, 1))
    return set_error(KVECC_EINVAL, "cpu_shim_read_batch: table stride too small");
  const int64_t osz = out_dtype == KVECC_F32 ? 4 : 2;
  for (int64_t b = 0; b < batch; ++b) {
    const int64_t off = b * hkv * ctx * d * osz;
    const int rc = kvecc_cpu_shim_read(k_cache, v_cache, k_scales, v_scales, block_table + b * table_stride,
                                       ctx, hkv, d, num_layers, block_size, layer, codec, interp,
                                       reinterpret_cast<char *>(k_out) + off,
                                       reinterpret_cast<char *>(v_out) + off, out_dtype, stats, threads);
    if (rc != KVECC_OK) return rc;
  }
  return KVECC_OK;
}

// host twin of kvecc_cache_scrub (scrub.hip): the same segments, skip rules and
// per-word functions (codec_math.h *_scrub*), one (sequence, layer, block, side)
// at a time; statistics 0..3 into a plain host array
KVECC_API int kvecc_cpu_cache_scrub(void *k_cache, void *v_cache, const int32_t *block_table,
                                    int64_t table_stride, const int32_t *context_lens,
                                    int64_t lens_layer_stride, int64_t batch, int64_t hkv, int64_t d,
                                    int64_t num_blocks, int64_t num_layers, int64_t layer_first,
                                    int64_t layer_count, int64_t block_size, int64_t max_context_len,
                                    int codec, uint64_t *stats, int threads) {
  if (table_stride < 0 || lens_layer_stride < 0 || batch < 0 || hkv < 0 || d < 0 || num_blocks < 0 ||
      num_layers < 0 || layer_first < 0 || layer_count < 0 || block_size < 0)
    return set_error(KVECC_EINVAL, "cpu_cache_scrub: negative size");
  if (codec == KVECC_CODEC_NONE)
    return set_error(KVECC_EINVAL, "cpu_cache_scrub: codec none has nothing to scrub");
  if (codec < KVECC_CODEC_NONE || codec > KVECC_CODEC_GOLAY_PACKED)
    return set_error(KVECC_EINVAL, "cpu_cache_scrub: bad codec %d", codec);
  if (batch == 0 || layer_count == 0 || hkv == 0) return KVECC_OK;
  const bool packed = codec == KVECC_CODEC_GOLAY_PACKED;
  const bool golay = codec == KVECC_CODEC_GOLAY || packed;
  if (d < 1 || d > 512)
    return set_error(KVECC_EINVAL, "cpu_cache_scrub: head_dim %lld not in [1, 512]", (long long)d);
  if (!golay && d % 4 != 0)
    return set_error(KVECC_EINVAL, "cpu_cache_scrub: head_dim %lld must be a multiple of 4", (long long)d);
  if (num_layers < 1 || block_size < 1 || num_blocks < 1 || layer_first + layer_count > num_layers)
    return set_error(KVECC_EINVAL, "cpu_cache_scrub: bad cache geometry (layers [%lld, %lld) of %lld)",
                     (long long)layer_first, (long long)(layer_first + layer_count), (long long)num_layers);
  if (table_stride < 1)
    return set_error(KVECC_EINVAL, "cpu_cache_scrub: table stride %lld < 1", (long long)table_stride);
  if (!k_cache || !v_cache || !block_table || !context_lens)
    return set_error(KVECC_EINVAL, "cpu_cache_scrub: null pointer");
  if (table_stride > 0x7FFFFFFFLL || block_size > 0x7FFFFFFFLL || table_stride * block_size > 0x7FFFFFFFLL ||
      batch > 0x7FFFFFFFLL || layer_count > 0x7FFFFFFFLL)
    return set_error(KVECC_EINVAL, "cpu_cache_scrub: sizes exceed 32-bit indexing");
  const uint16_t *tab = host_golay_tables();
  const int64_t g = golay ? (d + 2) / 3 : d;
  const int64_t rowb = packed ? KVECC_GOLAY_PACKED_ROW(g) : golay ? 4 * g : d;
  int64_t bound = table_stride * block_size;
  if (max_context_len > 0 && max_context_len < bound) bound = max_context_len;
  const int64_t nlb = (bound + block_size - 1) / block_size;
  const int64_t nseg = 2 * batch * layer_count * nlb;
  struct Acc4 {
    uint64_t v[4] = {0, 0, 0, 0};
    char pad[32];
  };
  std::vector<Acc4> acc(std::max(1, clamp_threads(threads, nseg, 1)));
  parallel_for(nseg, threads, 1, [&](int64_t s0, int64_t s1, int t) {
    uint32_t c0 = 0, c1 = 0, rew = 0;  // per run of one head (< 2^31 codewords), summed into acc
    for (int64_t s = s0; s < s1; ++s) {
      const int64_t side = s & 1, q = s >> 1;
      const int64_t lb = q % nlb, bl = q / nlb;
      const int64_t li = bl % layer_count, b = bl / layer_count;
      const int64_t len = std::min<int64_t>(context_lens[li * lens_layer_stride + b], bound);
      const int64_t nv = std::min<int64_t>(block_size, len - lb * block_size);
      if (nv <= 0) continue;
      const int64_t blk = block_table[b * table_stride + lb];
      if (blk < 0 || blk >= num_blocks) continue;
      for (int64_t h = 0; h < hkv; ++h) {
        // the block's rows of this head: row 0 of the run is position 0's slot
        const int64_t row0 = cache_slot(blk, num_layers, layer_first + li, hkv, h, block_size, 0);
        uint8_t *run = reinterpret_cast<uint8_t *>(side ? v_cache : k_cache) + row0 * rowb;
        c0 = c1 = rew = 0;
        if (packed) {
          for (int64_t r = 0; r < nv; ++r)
            for (int64_t k = 0; k < g; ++k) {
              uint8_t *c = run + r * rowb + 3 * k;
              const uint32_t w = golay_word(run, true, r, g, k);
              const uint32_t x = golay_scrub1(w, tab, tab + 4096, c0, c1, rew);
              if (x) {  // whole bytes of the canonical word: a second writer of a shared block stores the same
                c[0] = (uint8_t)(w ^ x);
                c[1] = (uint8_t)((w ^ x) >> 8);
                c[2] = (uint8_t)((w ^ x) >> 16);
              }
            }
          acc[t].v[3] += (uint64_t)(nv * g);
        } else {
          for (int64_t i = 0; i < nv * rowb; i += 4) {
            const uint32_t w = load4(run + i);
            const uint32_t x = codec == KVECC_CODEC_H84   ? h84_scrub4(w, c0, c1, rew)
                               : codec == KVECC_CODEC_H74 ? h74_scrub4(w, c0, rew)
                                                          : golay_scrub1(w, tab, tab + 4096, c0, c1, rew);
            if (x) store4(run + i, w ^ x);
          }
          acc[t].v[3] += (uint64_t)(nv * g);
        }
        acc[t].v[0] += c0;
        acc[t].v[1] += c1;
        acc[t].v[2] += rew;
      }
    }
  });
  if (stats)
    for (auto &x : acc)
      for (int k = 0; k < 4; ++k) stats[k] += x.v[k];
  return KVECC_OK;
}

}  // extern "C"

// ---- paged attention (host twin of attention.hip) ----------------------------
namespace kvecc {
namespace {

// Every (sequence, position, cache head, K|V row) a counting call counts, in
// that order, as fn(cache, row): the first n_b positions -- context_lens[b]
// clamped by max_context_len and by max_blocks * block_size -- of each sequence
// that has a valid query token (an all-padding span is not read), -1 blocks
// skipped; once per cache head, whatever the query rows and heads that look at it.
template <class F>
void for_each_counted_row(const AttnCall &c, F fn) {
  const int64_t mcl = c.max_context_len > 0 ? c.max_context_len : c.max_blocks * c.block_size;
  for (int64_t b = 0; b < c.batch; ++b) {
    const auto [first, count] = span_of(c.q_spans, b, c.q_len);
    if (first < 0 || count <= 0 || first >= c.q_len) continue;
    const int64_t nb = std::min<int64_t>(std::min<int64_t>(c.context_lens[b], mcl), c.max_blocks * c.block_size);
    for (int64_t pos = 0; pos < nb; ++pos) {
      const int32_t blk = c.block_table[b * c.max_blocks + pos / c.block_size];
      if (blk < 0) continue;
      for (int64_t hk = 0; hk < c.kv_heads; ++hk) {
        const int64_t row = cache_slot(blk, c.num_layers, c.layer, c.kv_heads, hk, c.block_size, pos);
        fn(c.k_cache, row);
        fn(c.v_cache, row);
      }
    }
  }
}

// The rows of a validated call, in the reference's order exactly: one (b, t, h) at
// a time, tokens in order, online softmax in fp32 (attention_ecc.py:355-427).  No valid token: Hamming(8,4)
// -8.0 per lane (the reference kernel's -1e20 masking, :342,391-423), Golay 0
// (reference_attention_ecc, :806-807,885-886).  Query row (b, t, h) is at
// b*q_sb + t*q_st + h*q_sh (elements), at position context_lens[b] - q_len + t,
// attending to the keys at or before it; q_len 1 is the decode entry.  q_spans
// (kvecc.h "Query spans"): row b's (first, count) replace (0, q_len).  An
// interpolating call sends every stored byte through h84_decode4 and doubles
// through interp_word of the neighbouring tokens (clamped to the sequence).
// INTERP is a template argument so that the byte loop of a call that does not interpolate
// carries no neighbour test (with the flag read in the loop a plain Hamming(8,4) call
// takes over twice as long); the results are the same bits either way.
// window > 0 (a windowed call, kvecc.h "Windowed attention"): the row at position p skips the
// keys sinks <= j < max(p - window + 1, 0); what it keeps it takes in the same order.
template <bool INTERP>
void attention_rows(const AttnCall &c, int threads, int64_t window = 0, int64_t sinks = 0) {
  // hot fields into locals: the row loop reads no record
  const void *const query = c.query, *const k_cache = c.k_cache, *const v_cache = c.v_cache;
  const int64_t q_sb = c.q_sb, q_st = c.q_st, q_sh = c.q_sh;
  const int q_dtype = c.q_dtype, codec = c.codec;
  const int32_t *const block_table = c.block_table, *const context_lens = c.context_lens, *const q_spans = c.q_spans;
  const float *const k_scales = c.k_scales, *const v_scales = c.v_scales;
  void *const out = c.out;
  const int64_t batch = c.batch, q_len = c.q_len, heads = c.heads, kv_heads = c.kv_heads, head_dim = c.head_dim;
  const int64_t num_layers = c.num_layers, layer = c.layer, block_size = c.block_size, max_blocks = c.max_blocks;
  const float sm_scale = c.sm_scale;
  constexpr bool interp = INTERP;
  const int64_t max_context_len = c.max_context_len > 0 ? c.max_context_len : max_blocks * block_size;
  const uint16_t *tab = host_golay_tables();
  const bool packed = codec == KVECC_CODEC_GOLAY_PACKED;
  const bool golay = codec == KVECC_CODEC_GOLAY || packed;
  const int64_t g = golay ? (head_dim + 2) / 3 : head_dim;
  const int64_t groups = heads / kv_heads;
  parallel_for(batch * q_len * heads, threads, 1, [&](int64_t b0, int64_t e0, int) {
    std::vector<float> q(head_dim), kv(head_dim), acc(head_dim);
    const std::vector<uint8_t> zero_row(golay ? 0 : (size_t)head_dim, 0);  // a missing block's codewords
    // cl / cr (interpolating calls): the codewords of the row's neighbours
    auto decode_row = [&](const void *cache, int64_t srow, float s, const uint8_t *cl = nullptr,
                          const uint8_t *cr = nullptr) {
      if (golay) {
        for (int64_t k = 0; k < g; ++k) {
          uint32_t cnt;
          const uint32_t dw = golay_decode1(golay_word(cache, packed, srow, g, k), tab, tab + 4096, cnt);
          for (int64_t u = 0; u < 3 && 3 * k + u < head_dim; ++u)
            kv[3 * k + u] = ((float)(dw >> (4 * u) & 0xFu) - 8.0f) * s;
        }
      } else {
        const uint8_t *c = reinterpret_cast<const uint8_t *>(cache) + srow * head_dim;
        for (int64_t j = 0; j < head_dim; ++j) {
          uint32_t d, t = 0, n1 = 0, n2 = 0;
          if (codec == KVECC_CODEC_NONE) {  // an unprotected byte's low nibble
            d = c[j] & 0xFu;
          } else if (codec == KVECC_CODEC_H74) {  // bit 7 ignored, doubles miscorrected
            h74_decode4(c[j], d, t, n1);
            d &= 0xFu;
          } else {
            h84_decode4(c[j], d, t, n1, n2);
          }
          if (cl) {  // a double becomes the rounded mean of its neighbours' decoded values
            uint32_t dl, dr, tt;
            h84_decode4(cl[j], dl, tt, n1, n2);
            h84_decode4(cr[j], dr, tt, n1, n2);
            d = interp_word(d, dl, dr, t) & 0xFFu;
          }
          kv[j] = ((float)d - 8.0f) * s;
        }
      }
    };
    for (int64_t bh = b0; bh < e0; ++bh) {
      const int64_t b = bh / (q_len * heads), t = bh / heads % q_len, h = bh % heads, hk = h / groups;
      // the sequence's span (null: the uniform call); a padding row reads no query and sees no key
      const auto [first, count] = span_of(q_spans, b, q_len);
      const bool valid = first >= 0 && t >= first && t < std::min(first + count, q_len);
      if (valid)
        for (int64_t j = 0; j < head_dim; ++j) q[j] = load_x(query, q_dtype, b * q_sb + t * q_st + h * q_sh + j);
      std::fill(acc.begin(), acc.end(), 0.0f);
      float m = -INFINITY, l = 0.0f;
      const int64_t ctx =
          valid ? std::min<int64_t>(std::min<int64_t>((int64_t)context_lens[b] - count + 1 + (t - first), max_context_len),
                                    max_blocks * block_size)
                : 0;
      // the sequence's length, which the neighbours of an interpolating call clamp to (not the row's key limit)
      const int64_t nb = std::min<int64_t>(std::min<int64_t>(context_lens[b], max_context_len), max_blocks * block_size);
      auto slot_of = [&](int64_t pos) {  // -1: no block
        const int32_t blk = block_table[b * max_blocks + pos / block_size];
        return blk < 0 ? (int64_t)-1 : cache_slot(blk, num_layers, layer, kv_heads, hk, block_size, pos);
      };
      auto codewords = [&](const void *cache, int64_t slot) {
        return slot < 0 ? zero_row.data() : reinterpret_cast<const uint8_t *>(cache) + slot * head_dim;
      };
      // the first key of the row's window (its position is the unclamped key limit - 1)
      const int64_t lo =
          valid && window > 0 ? std::max<int64_t>((int64_t)context_lens[b] - count + 1 + (t - first) - window, 0) : 0;
      for (int64_t pos = 0; pos < ctx; ++pos) {
        if (pos >= sinks && pos < lo) {  // between the sinks and the window: unseen, unread
          pos = lo - 1;
          continue;
        }
        const int64_t srow = slot_of(pos);
        if (srow < 0) continue;
        const int64_t sl = interp ? slot_of(pos > 0 ? pos - 1 : 0) : -1;
        const int64_t sr = interp ? slot_of(pos + 1 < nb ? pos + 1 : nb - 1) : -1;
        if (interp)
          decode_row(k_cache, srow, k_scales[srow], codewords(k_cache, sl), codewords(k_cache, sr));
        else
          decode_row(k_cache, srow, k_scales[srow]);
        // the dot product in double: a serial fp32 sum's error grows with |k_scale| and the
        // softmax sees it absolutely (tests/test_attention_scale_range.py, the kk = +6 rungs)
        double dot = 0.0;
        for (int64_t j = 0; j < head_dim; ++j) dot += (double)q[j] * (double)kv[j];
        const float sc = (float)(dot * (double)sm_scale);
        const float mn = std::max(m, sc);
        const float alpha = m == -INFINITY ? 0.0f : std::exp(m - mn);
        const float beta = std::exp(sc - mn);
        if (interp)
          decode_row(v_cache, srow, v_scales[srow], codewords(v_cache, sl), codewords(v_cache, sr));
        else
          decode_row(v_cache, srow, v_scales[srow]);
        for (int64_t j = 0; j < head_dim; ++j) acc[j] = alpha * acc[j] + beta * kv[j];
        l = alpha * l + beta;
        m = mn;
      }
      for (int64_t j = 0; j < head_dim; ++j)
        store_y(out, q_dtype, bh * head_dim + j, l > 0.0f ? acc[j] / l : golay ? 0.0f : -8.0f);
    }
  });
}

// The one path of the seven kvecc_cpu_paged_attention* entries, as attention.hip's
// entries share theirs: the record of the call (workspace and stream unused: null),
// the mode, and the thread count.
//
// Counting modes (m.stats a plain host buffer), after the rows -- so a repairing
// call's output is that of the cache as it stood -- over for_each_counted_row:
//   counted        stats[0] / stats[1] += the SINGLE_CORRECTED / DOUBLE_DETECTED bytes (h84_decode4)
//   repair         the same counts through h84_scrub4, every word with a correctable
//                  non-canonical byte stored back, stats[2] += bytes rewritten
//   golay_counted  stats[0] += the decoder's counts 0..3 (bits corrected), stats[1] += the
//                  words of count 4; bits 24-31 of an int32 word and a packed row's pad
//                  bytes take no part (golay_decode1)
//
// The checks come in the order, and under the names, they have always come in.  What
// is odd about that is kept: the messages of the shared part say cpu_paged_attention
// whichever entry was called (and a codec that cannot interpolate cpu_paged_attention_interp),
// the entries' own say `who`; the decode entry checks no q_len and no strides, only the
// chunk entry calls q_len by that name, only the ragged entry needs its spans; a counting
// call reports null stats, then its codec, before anything else; the interpolating call
// refuses a head_dim that is no multiple of 4 ahead of the negative-size and codec checks
// (a Hamming(8,4) counting call ahead of negative size), the others accept it for hamming84
// (int4 and hamming74 are refused, as the device entries refuse them); `negative size` does
// not look at q_len; a call with no rows returns before the later checks; num_blocks is not checked.
int cpu_attention(const char *who, const AttnCall &c, const AttnMode &m, int threads) {
  const bool decode = !std::strcmp(who, "cpu_paged_attention");
  const bool chunk = !std::strcmp(who, "cpu_paged_attention_chunk");
  const bool ragged = !std::strcmp(who, "cpu_paged_attention_chunk_ragged");
  const bool windowed = m.kind == AttnKind::windowed;  // (its entry has checked window and sinks)
  const bool counts = m.kind != AttnKind::plain && !windowed, golay_counts = m.kind == AttnKind::golay_counted;
  const bool repair = m.kind == AttnKind::repair;
  if (windowed && m.interp) return set_error(KVECC_EINVAL, "%s: a windowed call does not interpolate", who);
  if (counts && !m.stats) return set_error(KVECC_EINVAL, "%s: null stats", who);
  if (golay_counts && c.codec != KVECC_CODEC_GOLAY && c.codec != KVECC_CODEC_GOLAY_PACKED)
    return set_error(KVECC_EINVAL, "%s: codec %d (this counted twin needs golay or golay_packed)", who, c.codec);
  if (counts && !golay_counts && c.codec != KVECC_CODEC_H84)
    return set_error(KVECC_EINVAL, "%s: codec %d (the %s twin needs hamming84)", who, c.codec,
                     repair ? "repairing" : "counted");
  if (!decode) {
    if (c.q_len < 0) return set_error(KVECC_EINVAL, "%s: negative %s", who, chunk ? "q_len" : "q_max");
    if (ragged && !c.q_spans) return set_error(KVECC_EINVAL, "%s: null q_spans", who);
    if (c.q_sb < 0 || c.q_st < 0 || c.q_sh < 0 || (c.heads > 1 && c.q_sh < c.head_dim) ||
        (c.q_len > 1 && c.q_st < c.head_dim))
      return set_error(KVECC_EINVAL, "%s: bad query strides", who);
    if ((m.interp || (counts && !golay_counts)) && c.head_dim % 4 != 0)
      return set_error(KVECC_EINVAL, "%s: hamming84 head_dim must be a multiple of 4", who);
  }
  if (c.batch < 0 || c.heads < 0 || c.kv_heads < 0 || c.head_dim < 0)
    return set_error(KVECC_EINVAL, "cpu_paged_attention: negative size");
  if (m.interp && c.codec != KVECC_CODEC_H84)
    return set_error(KVECC_EINVAL, "cpu_paged_attention_interp: codec %d (interpolation needs hamming84)", c.codec);
  if (c.batch == 0 || c.heads == 0 || c.q_len == 0) return KVECC_OK;
  if (c.kv_heads < 1 || c.heads % c.kv_heads != 0)
    return set_error(KVECC_EINVAL, "cpu_paged_attention: heads not a multiple of kv heads");
  if (c.head_dim < 1) return set_error(KVECC_EINVAL, "cpu_paged_attention: empty head_dim");
  if (c.codec != KVECC_CODEC_NONE && c.codec != KVECC_CODEC_H74 && c.codec != KVECC_CODEC_H84 &&
      c.codec != KVECC_CODEC_GOLAY && c.codec != KVECC_CODEC_GOLAY_PACKED)
    return set_error(KVECC_EINVAL,
                     "cpu_paged_attention: codec %d (int4, hamming74, hamming84, golay or golay_packed only)",
                     c.codec);
  if ((c.codec == KVECC_CODEC_NONE || c.codec == KVECC_CODEC_H74) && c.head_dim % 4 != 0)  // as the device entries
    return set_error(KVECC_EINVAL, "cpu_paged_attention: %s head_dim must be a multiple of 4",
                     c.codec == KVECC_CODEC_NONE ? "int4" : "hamming74");
  if (c.q_dtype < KVECC_F32 || c.q_dtype > KVECC_BF16)
    return set_error(KVECC_EINVAL, "cpu_paged_attention: bad dtype %d", c.q_dtype);
  if (c.num_layers < 1 || c.layer < 0 || c.layer >= c.num_layers || c.block_size < 1 || c.max_blocks < 1)
    return set_error(KVECC_EINVAL, "cpu_paged_attention: bad cache geometry");
  if (!c.query || !c.k_cache || !c.v_cache || !c.block_table || !c.context_lens || !c.k_scales || !c.v_scales || !c.out)
    return set_error(KVECC_EINVAL, "cpu_paged_attention: null pointer");
  if (m.interp)
    attention_rows<true>(c, threads);
  else if (windowed)
    attention_rows<false>(c, threads, m.window, m.sinks);
  else
    attention_rows<false>(c, threads);
  if (!counts) return KVECC_OK;
  uint64_t n[3] = {0, 0, 0};
  if (golay_counts) {
    const uint16_t *tab = host_golay_tables();
    const bool packed = c.codec == KVECC_CODEC_GOLAY_PACKED;
    const int64_t g = (c.head_dim + 2) / 3;
    for_each_counted_row(c, [&](const void *cache, int64_t row) {
      for (int64_t k = 0; k < g; ++k) {
        uint32_t cnt;
        golay_decode1(golay_word(cache, packed, row, g, k), tab, tab + 4096, cnt);
        n[0] += cnt & 3u;
        n[1] += cnt >> 2;
      }
    });
  } else {
    for_each_counted_row(c, [&](const void *cache, int64_t row) {
      // (a repairing entry's caches are its caller's to write: kvecc_cpu_paged_attention_repair)
      uint8_t *p = const_cast<uint8_t *>(reinterpret_cast<const uint8_t *>(cache)) + row * c.head_dim;
      uint32_t n1 = 0, n2 = 0, nr = 0;  // of one row, summed into n
      for (int64_t j = 0; j < c.head_dim; j += 4) {
        const uint32_t w = load4(p + j);
        if (repair) {
          const uint32_t x = h84_scrub4(w, n1, n2, nr);
          if (x) store4(p + j, w ^ x);
        } else {
          uint32_t d, t;
          h84_decode4(w, d, t, n1, n2);
        }
      }
      n[0] += n1;
      n[1] += n2;
      n[2] += nr;
    });
  }
  m.stats[0] += n[0];
  m.stats[1] += n[1];
  if (repair) m.stats[2] += n[2];
  return KVECC_OK;
}

}  // namespace
}  // namespace kvecc

extern "C" {

KVECC_API int kvecc_cpu_paged_attention(const void *query, int q_dtype, const void *k_cache,
                                        const void *v_cache, const int32_t *block_table,
                                        const int32_t *context_lens, const float *k_scales,
                                        const float *v_scales, void *out, int64_t batch,
                                        int64_t heads, int64_t kv_heads, int64_t head_dim,
                                        int64_t num_blocks, int64_t num_layers, int64_t layer, int64_t block_size,
                                        int64_t max_blocks, int64_t max_context_len,
                                        float sm_scale, int codec, int threads) {
  return cpu_attention("cpu_paged_attention",
                       {query, heads * head_dim, 0, head_dim, q_dtype, k_cache, v_cache, block_table, context_lens,
                        nullptr, k_scales, v_scales, out, batch, 1, heads, kv_heads, head_dim, num_blocks, num_layers,
                        layer, block_size, max_blocks, max_context_len, sm_scale, codec, nullptr, 0, nullptr},
                       {}, threads);
}

// Chunked causal twin (kvecc_paged_attention_chunk): out [batch, q_len, heads, head_dim]
KVECC_API int kvecc_cpu_paged_attention_chunk(const void *query, int64_t q_batch_stride,
                                              int64_t q_token_stride, int64_t q_head_stride, int q_dtype,
                                              const void *k_cache, const void *v_cache,
                                              const int32_t *block_table, const int32_t *context_lens,
                                              const float *k_scales, const float *v_scales, void *out,
                                              int64_t batch, int64_t q_len, int64_t heads, int64_t kv_heads,
                                              int64_t head_dim, int64_t num_blocks, int64_t num_layers,
                                              int64_t layer, int64_t block_size, int64_t max_blocks,
                                              int64_t max_context_len, float sm_scale, int codec, int threads) {
  return cpu_attention("cpu_paged_attention_chunk",
                       {query, q_batch_stride, q_token_stride, q_head_stride, q_dtype, k_cache, v_cache, block_table,
                        context_lens, nullptr, k_scales, v_scales, out, batch, q_len, heads, kv_heads, head_dim,
                        num_blocks, num_layers, layer, block_size, max_blocks, max_context_len, sm_scale, codec,
                        nullptr, 0, nullptr},
                       {}, threads);
}

// Ragged twin (kvecc_paged_attention_chunk_ragged): per-sequence query spans, padding rows the empty value
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
                                                     int threads) {
  return cpu_attention("cpu_paged_attention_chunk_ragged",
                       {query, q_batch_stride, q_token_stride, q_head_stride, q_dtype, k_cache, v_cache, block_table,
                        context_lens, q_spans, k_scales, v_scales, out, batch, q_max, heads, kv_heads, head_dim,
                        num_blocks, num_layers, layer, block_size, max_blocks, max_context_len, sm_scale, codec,
                        nullptr, 0, nullptr},
                       {}, threads);
}

// Windowed twin (kvecc_paged_attention_window); q_spans may be null.  window 0 or >= ctx_cap: the
// ragged / chunk twin's bits (the same rows, no key skipped); head_dim is bounded as the device entry's is.
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
                                               int64_t window, int64_t sinks, int threads) {
  if (window < 0 || sinks < 0)
    return set_error(KVECC_EINVAL, "cpu_paged_attention_window: negative window %lld or sinks %lld",
                     (long long)window, (long long)sinks);
  if (head_dim > 256)
    return set_error(KVECC_EINVAL, "cpu_paged_attention_window: head_dim %lld not in [1, 256]", (long long)head_dim);
  // (as the device entry: a window of ctx_cap keys or more is no window)
  const int64_t table_cap = max_blocks > 0 && block_size > 0 ? max_blocks * block_size : 0;
  const int64_t ctx_cap = max_context_len > 0 ? std::min(max_context_len, table_cap) : table_cap;
  AttnMode m;
  if (window > 0 && window < ctx_cap) {
    m.kind = AttnKind::windowed;
    m.window = window;
    m.sinks = sinks;
  }
  return cpu_attention("cpu_paged_attention_window",
                       {query, q_batch_stride, q_token_stride, q_head_stride, q_dtype, k_cache, v_cache, block_table,
                        context_lens, q_spans, k_scales, v_scales, out, batch, q_max, heads, kv_heads, head_dim,
                        num_blocks, num_layers, layer, block_size, max_blocks, max_context_len, sm_scale, codec,
                        nullptr, 0, nullptr},
                       m, threads);
}

// Interpolating twin (kvecc_paged_attention_interp); q_spans may be null
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
                                               int threads) {
  return cpu_attention("cpu_paged_attention_interp",
                       {query, q_batch_stride, q_token_stride, q_head_stride, q_dtype, k_cache, v_cache, block_table,
                        context_lens, q_spans, k_scales, v_scales, out, batch, q_max, heads, kv_heads, head_dim,
                        num_blocks, num_layers, layer, block_size, max_blocks, max_context_len, sm_scale, codec,
                        nullptr, 0, nullptr},
                       {AttnKind::plain, true}, threads);
}

// Counted twin (kvecc_paged_attention_stats): the ragged (interp == 0) or the interpolating
// twin's output and the Hamming(8,4) counts; stats is a host buffer
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
                                              uint64_t *stats, int threads) {
  return cpu_attention("cpu_paged_attention_stats",
                       {query, q_batch_stride, q_token_stride, q_head_stride, q_dtype, k_cache, v_cache, block_table,
                        context_lens, q_spans, k_scales, v_scales, out, batch, q_max, heads, kv_heads, head_dim,
                        num_blocks, num_layers, layer, block_size, max_blocks, max_context_len, sm_scale, codec,
                        nullptr, 0, nullptr},
                       {AttnKind::counted, interp != 0, stats}, threads);
}

// Repairing twin (kvecc_paged_attention_repair): the counted twin's output and counts, the
// counted region of k_cache / v_cache rewritten in place
KVECC_API int kvecc_cpu_paged_attention_repair(const void *query, int64_t q_batch_stride,
                                               int64_t q_token_stride, int64_t q_head_stride, int q_dtype,
                                               void *k_cache, void *v_cache, const int32_t *block_table,
                                               const int32_t *context_lens, const int32_t *q_spans,
                                               const float *k_scales, const float *v_scales, void *out,
                                               int64_t batch, int64_t q_max, int64_t heads, int64_t kv_heads,
                                               int64_t head_dim, int64_t num_blocks, int64_t num_layers,
                                               int64_t layer, int64_t block_size, int64_t max_blocks,
                                               int64_t max_context_len, float sm_scale, int codec, int interp,
                                               uint64_t *stats, int threads) {
  return cpu_attention("cpu_paged_attention_repair",
                       {query, q_batch_stride, q_token_stride, q_head_stride, q_dtype, k_cache, v_cache, block_table,
                        context_lens, q_spans, k_scales, v_scales, out, batch, q_max, heads, kv_heads, head_dim,
                        num_blocks, num_layers, layer, block_size, max_blocks, max_context_len, sm_scale, codec,
                        nullptr, 0, nullptr},
                       {AttnKind::repair, interp != 0, stats}, threads);
}

// Golay counted twin (kvecc_paged_attention_golay_stats): the ragged twin's output (q_spans may
// be null) and the Golay decoder's counts
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
                                                    uint64_t *stats, int threads) {
  return cpu_attention("cpu_paged_attention_golay_stats",
                       {query, q_batch_stride, q_token_stride, q_head_stride, q_dtype, k_cache, v_cache, block_table,
                        context_lens, q_spans, k_scales, v_scales, out, batch, q_max, heads, kv_heads, head_dim,
                        num_blocks, num_layers, layer, block_size, max_blocks, max_context_len, sm_scale, codec,
                        nullptr, 0, nullptr},
                       {AttnKind::golay_counted, false, stats}, threads);
}

}  // extern "C"
