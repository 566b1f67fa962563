// Fragment of the matrix-core attention bodies, included in place after the staging
// (attn_mfma_rows.inc, the body's decode table): the query sum, the barrier that publishes what was
// staged, and the buffer descriptors.
// Reads: a, qop[KK], kWave.
// Defines: qsum (head n's query summed over d, for the -8 fold of the scores); krs, vrs, ksrs, vsrs; qscale.
// The softmax state (acc[MT], m, l, psum, pvc) and qoff = kMfmaValOffset * qsum stay in the bodies:
// qoff stands before the accumulators' initialisation in the Golay body and after it in the
// Hamming(8,4) body, and either order in both moves the schedule of the other's kernels (DESIGN.md).
// Islands: none.
  float qsum = 0.0f;  // sum of head n's query over all d (the offset fold)
#pragma unroll
  for (int kk = 0; kk < KK; ++kk)
#pragma unroll
    for (int e = 0; e < 8; ++e) qsum += (float)qop[kk][e];
  qsum += __shfl_xor(qsum, 16, kWave);
  qsum += __shfl_xor(qsum, 32, kWave);
  __syncthreads();

  const __amdgpu_buffer_rsrc_t krs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.k_cache), 0, (int)a.cache_bytes, kRsrcWord3);
  const __amdgpu_buffer_rsrc_t vrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.v_cache), 0, (int)a.cache_bytes, kRsrcWord3);
  const __amdgpu_buffer_rsrc_t ksrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.k_scales), 0, (int)a.scale_bytes, kRsrcWord3);
  const __amdgpu_buffer_rsrc_t vsrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.v_scales), 0, (int)a.scale_bytes, kRsrcWord3);
  const float qscale = a.sm_scale * kAttnLogScale;
