// Fragment of the matrix-core attention bodies, included in place: the split's slice of
// the block table becomes cache rows in LDS (-1: no block / past the split).
// Reads: a, b, hk, t0, ntok, kBlock, kMfmaStep; the halo form also nb and kHalo.
// Writes: blks[] (scratch) and rows[]: rows[i] is the row of token t0 + i for i < npad, ntok rounded
// up to whole wave steps.  It holds one __syncthreads(), after the slice's loads: the including
// body's own barrier, after this fragment, is what publishes rows[].
// Islands:
//   [interpolation] (ATTN_BODY_CHUNK == 2) the halo form: rows[kHalo + i] is R(i), the row of
//     position t0 + i of the sequence for i in [-1, npad] -- a token on each side of the split's,
//     bounded by the sequence's length nb, not by the tile's key limit ([score mask] alone masks a
//     position past every column's limit); -1: no block, or outside [0, nb).
//   [window] (ATTN_BODY_WINDOW, the windowed kernels) the positions between the sinks and the tile's
//     smallest lower bound (cm.lo_min) get -1.
//   [spread tables] (ATTN_ROWS_SPREAD_TABLES, which attn_golay_mfma_body.inc defines around its
//     inclusion) Golay's decode tables go to gt[] between the slice's loads and their barrier.
#if ATTN_BODY_CHUNK == 2  // [interpolation] the halo form
  {  // block-table slice of positions [t0 - 1, t0 + npad] -> cache rows
    const int npad = (ntok + kMfmaStep - 1) / kMfmaStep * kMfmaStep;
    const uint32_t bs = (uint32_t)a.bs;
    const int64_t p0 = max<int64_t>(t0 - 1, 0);
    const int64_t p1 = min<int64_t>(t0 + npad, a.max_blocks * a.bs - 1);  // inclusive
    const uint32_t lb0 = (uint32_t)p0 / bs;
    const int nlb = ntok > 0 && p1 >= p0 ? (int)((uint32_t)p1 / bs - lb0 + 1) : 0;
    const int32_t *tab = a.table + b * a.max_blocks + lb0;
    for (int j = threadIdx.x; j < nlb; j += kBlock) blks[j] = tab[j];
    __syncthreads();
    const int32_t head_row0 = (int32_t)((a.layer * a.kv_heads + hk) * a.bs);
    const int32_t blk_rows = (int32_t)(a.layers * a.kv_heads * a.bs);
    if (ntok > 0) {
      for (int idx = threadIdx.x; idx < npad + 2; idx += kBlock) {
        const int64_t p = t0 + idx - 1;
        int32_t row = -1;
        if (p >= 0 && p < nb) {
          const uint32_t pos = (uint32_t)p;
          const uint32_t lb = pos / bs;
          const int32_t blk = blks[lb - lb0];
          if (blk >= 0) row = blk * blk_rows + head_row0 + (int32_t)(pos - lb * bs);
        }
        rows[kHalo - 1 + idx] = row;
      }
    }
  }
#else
  {  // block-table slice -> cache rows (-1: no block / past the split)
    const uint32_t bs = (uint32_t)a.bs;
    const uint32_t lb0 = (uint32_t)(t0 / a.bs);
    // the whole split's slice, bounded by the table rather than the context, so
    // the load does not wait for context_lens (one dependent HBM trip fewer)
    const int64_t tmax = min<int64_t>(t0 + a.split, a.max_blocks * a.bs);
    const int nlb = tmax > t0 ? (int)((uint32_t)(tmax - 1) / bs - lb0 + 1) : 0;
    const int32_t *tab = a.table + b * a.max_blocks + lb0;
    for (int j = threadIdx.x; j < nlb; j += kBlock) blks[j] = tab[j];
#ifdef ATTN_ROWS_SPREAD_TABLES  // [spread tables] 32 KiB from a.atab, under the slice's barrier
    {
      const u32x4 *src = reinterpret_cast<const u32x4 *>(a.atab);
      for (int i = threadIdx.x; i < 2048; i += kBlock) reinterpret_cast<u32x4 *>(gt)[i] = src[i];
    }
#endif
    __syncthreads();
    const int32_t head_row0 = (int32_t)((a.layer * a.kv_heads + hk) * a.bs);
    const int32_t blk_rows = (int32_t)(a.layers * a.kv_heads * a.bs);
    const int npad = (ntok + kMfmaStep - 1) / kMfmaStep * kMfmaStep;
    for (int i = threadIdx.x; i < npad; i += kBlock) {
      int32_t row = -1;
#ifdef ATTN_BODY_WINDOW  // [window] a key that no column of the tile sees is a -1 row, as a missing block's
      if (i < ntok && (t0 + i >= cm.lo_min || t0 + i < (int64_t)a.sinks)) {
#else
      if (i < ntok) {
#endif
        const uint32_t pos = (uint32_t)(t0 + i);
        const uint32_t lb = pos / bs;
        const int32_t blk = blks[lb - lb0];
        if (blk >= 0) row = blk * blk_rows + head_row0 + (int32_t)(pos - lb * bs);
      }
      rows[i] = row;
    }
  }
#endif
