// Body of shim_append_kernel (SHIM_APPEND_RAGGED 0) and of shim_append_ragged_kernel
// (SHIM_APPEND_RAGGED 1, with `q_spans`), included by shim.hip inside each kernel: the uniform
// kernel's text is what it always was, so its code is too (a shared __device__ function changed it).
// shim.hip defines SHIM_APPEND_RAGGED around each inclusion; it is no build switch.
  __shared__ uint8_t nib[kWavesPerBlock][kMaxShimD + 4];
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
  const uint32_t key0 = (a.seed0 + ri + (uint32_t)side) * a.rowmul;
#else
  const uint32_t b = bt / a.qlen, t = bt - b * a.qlen;
  const uint32_t key0 = (a.seed0 + r + (uint32_t)side) * a.rowmul;
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
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off, kWave));
  const float scale = row_scale(amax, a.scale_rule);
  if (live && lane == 0) a.scales[side][slot] = scale;
  const bool recip = sizeof(T) == 2 && recip_ok(scale);
  const float inv = div_rn(1.0f, scale);
  auto quant = [&](float x) {
    return recip ? nibble_of_quotient(div_recip(x, scale, inv)) : quantize_nibble(x, scale);
  };

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
