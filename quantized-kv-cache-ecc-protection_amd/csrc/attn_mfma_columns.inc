// Fragment of the matrix-core attention bodies (attn_h84_mfma_body.inc, attn_golay_mfma_body.inc),
// included in place: what this lane, and this workgroup, stand for.
// Reads: a, G (decode form), ChunkMap (chunk forms), kBlock, kWave.
// Defines: wave, lane, n, g; b, h0, hk; ctx, t0, t1, ntok; in the chunk forms cm and col_lim; with
// ATTN_BODY_STATS csp and counts -- the body declares its own counters after the inclusion.
// Leaves the kernel (put_empty) when a ragged tile holds no valid token.
// Islands: [column map], [key limit] (ATTN_BODY_CHUNK), [statistics] who counts (ATTN_BODY_STATS),
// [window] (ATTN_BODY_WINDOW, the windowed kernels: defines col_lo, col_sink, i_first; leaves the kernel
// when the split holds no key the tile can see).
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int n = lane & 15, g = lane >> 4;
#if ATTN_BODY_CHUNK  // [column map] cm is used by every other chunk island of the bodies
  const ChunkMap cm(a, n);  // column n's (token, head); blockIdx.x = tile * nsplit + split
  if constexpr (ChunkMap::kRagged) {
    if (!cm.any) {  // every token of the tile is padding: nothing staged, no table or cache read
      cm.put_empty(a);
      return;
    }
  }
  const int64_t b = cm.b, h0 = cm.h0;
  const int64_t hk = h0 / (a.heads / a.kv_heads);
#ifdef ATTN_BODY_STATS  // [statistics] who counts (kvecc.h "Counted attention"): uniform per workgroup
  // The tile that holds the sequence's last valid token, in the first column group of
  // its cache head, counts: one workgroup per (sequence, cache head, split).  It walks
  // the sequence's n_b rows -- the tile's largest key limit unless the span overruns
  // q_max; the columns' own limits mask the scores either way ([score mask]).
  const ChunkSpan csp(a, b);
  const bool counts = csp.v1(a) > csp.v0() && cm.tile == (uint32_t)(csp.v1(a) - 1) / (16u >> a.cg_log2) &&
                      h0 % (a.heads / a.kv_heads) == 0;
  const int64_t ctx = counts ? min<int64_t>(a.ctx_lens[b], a.ctx_cap) : cm.ctx;
#else
  const int64_t ctx = cm.ctx;  // the largest key limit of the tile's columns
#endif
#ifdef ATTN_BODY_WINDOW  // [window] the split's place follows the tile's smallest lower bound (WindowArgs::split_start)
  const int64_t t0 = a.split_start(cm.split_idx, cm.lo_min);
#else
  const int64_t t0 = (int64_t)cm.split_idx * a.split;
#endif
#else
  const int64_t hgroups = a.heads / G;
  const int64_t b = blockIdx.y / hgroups, h0 = (blockIdx.y % hgroups) * G;
  const int64_t hk = h0 / (a.heads / a.kv_heads);
  const int64_t ctx = min<int64_t>(a.ctx_lens[b], a.ctx_cap);
  const int64_t t0 = (int64_t)blockIdx.x * a.split;
#endif
  const int64_t t1 = min<int64_t>(t0 + a.split, ctx);
  const int ntok = t1 > t0 ? (int)(t1 - t0) : 0;
#if ATTN_BODY_CHUNK  // [key limit] applied at [score mask]
  const int col_lim = cm.col_limit(t0);  // this column's keys: the split's tokens below it
#endif
#ifdef ATTN_BODY_WINDOW  // [window] the split's share of the tile's visible keys (cm a WindowMap)
  // Some column of the tile sees the sink keys [t0, min(t1, sinks)) and the window keys
  // [max(t0, lo_min), t1).  A split that holds neither -- one past the tile's limit included --
  // stages nothing: it writes the empty partial and leaves, as an all-padding tile does.
  const bool sees_sink = min<int64_t>(t1, a.sinks) > t0, sees_win = t1 > max<int64_t>(t0, cm.lo_min);
  if (!sees_sink && !sees_win) {  // uniform per workgroup
    cm.put_empty(a);
    return;
  }
  // this column's window and sink bounds relative to t0, applied at [score mask]
  const int col_lo = WindowMap::rel(cm.lo, t0), col_sink = WindowMap::rel(a.sinks, t0);
  // the first round of wave steps that holds a visible key: the rounds before it hold -1 rows only
  const int i_first = sees_sink ? 0 : (int)(max<int64_t>(cm.lo_min - t0, 0) / (kBlock / kWave * kMfmaStep)) *
                                          (kBlock / kWave * kMfmaStep);
#endif
