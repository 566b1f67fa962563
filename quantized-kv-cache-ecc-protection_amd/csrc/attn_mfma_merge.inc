// Fragment of the matrix-core attention bodies, included in place after the wave-step loop: the 4
// lanes of a column merge, then the workgroup's waves through LDS, and the split's partial
// (M, L, o[D]) goes to the workspace of the combine kernel.
// Reads: a, m, l, psum, pvc, acc[MT], wave, n, g, G, D, MT, kWaves, kBlock; b, h0 (decode form), cm
// (chunk forms).
// Writes: gml[][][], red[][][] (LDS; one __syncthreads() between their stores and their loads) and
// the workspace rows of this workgroup's columns.  Updates l, psum to their column sums.
// Output row d of M-tile mt is MT (4g + r) + mt: the guard on it is a constant where 16 MT == D
// (Hamming(8,4)) and drops Golay's d >= 128 (9 tiles of 16 rows for 128).
// Islands: [merge: workspace row] (ATTN_BODY_CHUNK against the decode form).  A text fragment and
// not a function: as one it moved the registers of 13 more kernels (DESIGN.md).
  l += __shfl_xor(l, 16, kWave);
  l += __shfl_xor(l, 32, kWave);
  psum += __shfl_xor(psum, 16, kWave);
  psum += __shfl_xor(psum, 32, kWave);
  const float poff = kMfmaValOffset * psum, oscale = pvc * kMfmaValScale;
  if (n < G) {
    if (g == 0) {
      gml[0][wave][n] = m;
      gml[1][wave][n] = l;
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int d = MT * (4 * g + r) + mt;
        if (16 * MT == D || d < D) red[wave][n][d] = acc[mt][r] * oscale - poff;
      }
  }
  __syncthreads();
#if !ATTN_BODY_CHUNK  // [merge: workspace row] decode: head h0's row, the others at a fixed stride (below)
  const int64_t ws_stride = a.nsplit * (a.d + 2);
  float *ws0 = a.ws + ((b * a.heads + h0) * a.nsplit + blockIdx.x) * (a.d + 2);
#endif
  for (int idx = threadIdx.x; idx < G * D; idx += kBlock) {
    const int h = idx / D, d = idx % D;
#if ATTN_BODY_CHUNK  // [merge: workspace row] chunk: column h's own output row; none: a column past the chunk
    const int64_t orow = cm.out_row(a, h);
    if (orow < 0) continue;
#endif
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) M = fmaxf(M, gml[0][w][h]);
    float o = 0.0f, L = 0.0f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const float mw = gml[0][w][h];
      const float wt = mw == -INFINITY ? 0.0f : attn_exp(mw - M);
      o += red[w][h][d] * wt;
      L += gml[1][w][h] * wt;
    }
#if ATTN_BODY_CHUNK  // [merge: workspace row] orow from the loop's head / ws0 from before the loop
    float *ws = a.ws + (orow * a.nsplit + cm.split_idx) * (a.d + 2);
#else
    float *ws = ws0 + h * ws_stride;
#endif
    ws_put(ws + 2 + d, o);
    if (d == 0) {
      ws_put(ws, M);
      ws_put(ws + 1, L);
    }
  }
