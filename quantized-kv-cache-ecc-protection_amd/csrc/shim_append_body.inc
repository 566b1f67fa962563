// Body of shim_append_kernel (SHIM_APPEND_RAGGED 0) and of shim_append_ragged_kernel
// (SHIM_APPEND_RAGGED 1, with `q_spans`), included by shim.hip inside each kernel: the uniform
// kernel's text is what it always was, so its code is too (a shared __device__ function changed it).
// shim.hip defines SHIM_APPEND_RAGGED around each inclusion; it is no build switch.
// The packed INT4 kernels (shim_append_packed_kernel, shim_append_packed_ragged_kernel,
// KVECC_CODEC_INT4_PACKED) also define SHIM_APPEND_PACKED: the [packed] islands, in which a lane
// owns the 8 adjacent values of one dword of the packed row; without it the preprocessed text is
// what it was.
#ifndef SHIM_APPEND_PACKED
  __shared__ uint8_t nib[kWavesPerBlock][kMaxShimD + 4];
#endif
  const ShimGeom &geo = a.geo;
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const uint32_t per_side = a.batch * a.qlen * geo.hkv;
  const uint32_t item = blockIdx.x * kWavesPerBlock + w;
  const bool in_grid = item < 2 * per_side;
  const int side = in_grid && item >= per_side ? 1 : 0;
  const uint32_t r = in_grid ? item - side * per_side : 0;  // (b * qlen + t) * hkv + h
  const uint32_t bt = r / geo.hkv, h = r - bt * geo.hkv;
#if SHIM_APPEND_RAGGED  // [spans] tq: the token's place in its row; t: its offset from start_pos[b]; ri: its seed row
  const uint32_t b = bt / a.qlen, tq = bt - b * a.qlen;
  uint32_t t = tq, ri = r;
  bool live = in_grid;
  if (live) {
    const int32_t first = q_spans[3 * b], count = q_spans[3 * b + 1], base = q_spans[3 * b + 2];
    live = first >= 0 && (int64_t)tq >= first && (int64_t)tq < min<int64_t>((int64_t)first + count, a.qlen);
    t = tq - (uint32_t)first;
    ri = ((uint32_t)base + t) * geo.hkv + h;
  }
#ifdef SHIM_APPEND_PACKED  // [packed] no injection, so no seed
  (void)ri;
#else
  const uint32_t key0 = (a.seed0 + ri + (uint32_t)side) * a.rowmul;
#endif
#else
  const uint32_t b = bt / a.qlen, t = bt - b * a.qlen;
#ifndef SHIM_APPEND_PACKED
  const uint32_t key0 = (a.seed0 + r + (uint32_t)side) * a.rowmul;
#endif
  bool live = in_grid;
#endif
  int64_t slot = 0;
  if (live) {
    const int32_t sp = a.start_pos[b];
    const uint32_t p = (uint32_t)sp + t;  // sp >= 0, t < 2^31: no wrap
    const uint32_t lb = p / geo.bs;
    live = sp >= 0 && lb < a.tstride;
    if (live) {
      const int64_t blk = geo.table[(int64_t)b * a.tstride + lb];
      live = blk >= 0;
      slot = ((blk * geo.layers + geo.layer) * geo.hkv + h) * geo.bs + (p - lb * geo.bs);
    }
  }

#ifdef SHIM_APPEND_PACKED  // [packed] lane i owns values 8i .. 8i + 7: dword i of the row of d / 2 bytes
  // (d % 8 == 0 and d <= 256: the row's d / 8 dwords sit in the wave's first 32 lanes).  The
  // row maximum, the scale and the quantiser are the byte kernels'; the lane's eight nibbles meet
  // in its own register, nibble j at bits 4j -- byte i of the row holds value 2i low, 2i + 1
  // high -- and leave as one dword store.  An input row that is 16-byte aligned (uniform per
  // wave) is read with 16-byte loads, any other element by element.
  constexpr int kPk = 8;
  float v[kPk];
  float amax = 0.0f;
  const bool own = live && (uint32_t)(kPk * lane) < geo.d;
  if (own) {
#if SHIM_APPEND_RAGGED  // [spans] the input row is the token's place in the rectangle
    const T *x = reinterpret_cast<const T *>(a.x[side]) + (int64_t)b * a.xb[side] + (int64_t)tq * a.xs[side] +
                 (int64_t)h * a.xh[side];
#else
    const T *x = reinterpret_cast<const T *>(a.x[side]) + (int64_t)b * a.xb[side] + (int64_t)t * a.xs[side] +
                 (int64_t)h * a.xh[side];
#endif
    if ((reinterpret_cast<uintptr_t>(x) & 15u) == 0) {
      constexpr int kVecs = kPk * (int)sizeof(T) / 16;  // 16-byte loads per lane: 2 (fp32) or 1
      u32x4 raw[kVecs];
#pragma unroll
      for (int k = 0; k < kVecs; ++k) raw[k] = reinterpret_cast<const u32x4 *>(x + kPk * lane)[k];
      T xe[kPk];
      __builtin_memcpy(xe, raw, sizeof(xe));
#pragma unroll
      for (int j = 0; j < kPk; ++j) v[j] = to_f32<T>(xe[j]);
    } else {
#pragma unroll
      for (int j = 0; j < kPk; ++j) v[j] = to_f32<T>(x[kPk * lane + j]);
    }
#pragma unroll
    for (int j = 0; j < kPk; ++j) amax = fmaxf(amax, fabsf(v[j]));
  }
#else
  constexpr int kPer = kMaxShimD / kWave;
  float v[kPer];
  float amax = 0.0f;
  if (live) {
#if SHIM_APPEND_RAGGED  // [spans] the input row is the token's place in the rectangle
    const T *x = reinterpret_cast<const T *>(a.x[side]) + (int64_t)b * a.xb[side] + (int64_t)tq * a.xs[side] +
                 (int64_t)h * a.xh[side];
#else
    const T *x = reinterpret_cast<const T *>(a.x[side]) + (int64_t)b * a.xb[side] + (int64_t)t * a.xs[side] +
                 (int64_t)h * a.xh[side];
#endif
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const uint32_t e = lane + i * kWave;
      v[i] = e < geo.d ? to_f32<T>(x[e]) : 0.0f;
      amax = fmaxf(amax, fabsf(v[i]));
    }
  }
#endif
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off, kWave));
  const float scale = row_scale(amax, a.scale_rule);
  if (live && lane == 0) a.scales[side][slot] = scale;
  const bool recip = sizeof(T) == 2 && recip_ok(scale);
  const float inv = div_rn(1.0f, scale);
  auto quant = [&](float x) {
    return recip ? nibble_of_quotient(div_recip(x, scale, inv)) : quantize_nibble(x, scale);
  };

#ifdef SHIM_APPEND_PACKED  // [packed] eight nibbles, one dword, one store
  if (!own) return;
  uint32_t word = 0;
#pragma unroll
  for (int j = 0; j < kPk; ++j) word |= quant(v[j]) << (4 * j);
  reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(a.cache[side]) + slot * KVECC_INT4_PACKED_ROW(geo.d))[lane] =
      word;
#else
  constexpr bool kGolay = CODEC == KVECC_CODEC_GOLAY || CODEC == KVECC_CODEC_GOLAY_PACKED;
  if (!kGolay) {
    if (!live) return;
    uint8_t *c = reinterpret_cast<uint8_t *>(a.cache[side]) + slot * geo.g;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const uint32_t e = lane + i * kWave;
      if (e < geo.d) {
        uint32_t cw = encode_nibble(quant(v[i]), CODEC);
        if (a.inject) cw ^= philox_flip_mask<NB>(key0 + e * a.nbits, e, a.thr, a.nb_eff);
        c[e] = (uint8_t)cw;
      }
    }
    return;
  }
  // Golay: nibbles through LDS, one lane per codeword of 3; skipped rows reach the barrier too
  if (live) {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const uint32_t e = lane + i * kWave;
      if (e < geo.d) nib[w][e] = (uint8_t)quant(v[i]);
    }
    if ((uint32_t)lane < 3 * geo.g - geo.d) nib[w][geo.d + lane] = 0;  // per-head zero padding
  }
  __syncthreads();
  if (!live) return;
  for (uint32_t k = lane; k < geo.g; k += kWave) {
    const uint32_t dw = golay_pack(nib[w][3 * k], nib[w][3 * k + 1], nib[w][3 * k + 2]);
    uint32_t cw = dw | golay_parity12(dw) << 12;
    if (a.inject) cw ^= philox_flip_mask<NB>(key0 + k * a.nbits, k, a.thr, a.nb_eff);
    if (CODEC == KVECC_CODEC_GOLAY_PACKED) {
      uint8_t *c = reinterpret_cast<uint8_t *>(a.cache[side]) + slot * KVECC_GOLAY_PACKED_ROW(geo.g) + 3 * k;
      c[0] = (uint8_t)cw;
      c[1] = (uint8_t)(cw >> 8);
      c[2] = (uint8_t)(cw >> 16);
    } else {
      reinterpret_cast<int32_t *>(a.cache[side])[slot * geo.g + k] = (int32_t)cw;
    }
  }
#endif
