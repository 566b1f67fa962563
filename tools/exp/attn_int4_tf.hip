// attn_int4_tf.hip -- INT4 paged attention without the decode table (NOT shipped).
//
// The product runs unprotected INT4 caches (KVECC_CODEC_NONE) through the byte
// family's kernels: the Hamming(8,4) bodies with a 256-entry LDS table that
// holds b & 15.  This fork builds the same library entries with the byte
// family's matrix-core kernels (decode, chunk, ragged) over a generated copy of
// attn_h84_mfma_body.inc in which the table is the object below: the low
// nibble is masked in registers, no LDS lookup per value, nothing staged.  (The
// Makefile generates the two gen_int4_tf_* files with sed from the product
// sources; the fork's Hamming(7,4) results are wrong, only INT4 is run.)
// tools/exp/run_int4_table_free.py times both through kvecc_paged_attention and
// kvecc_paged_attention_chunk, alternating in one process, and compares bits.
#include <cstdint>

#include <hip/hip_runtime.h>

namespace kvecc {
struct NibbleOf {  // stands where the body's `lut` stands
  __device__ __forceinline__ uint32_t operator[](uint32_t b) const { return b & 0xFu; }
};
}  // namespace kvecc

#include "gen_int4_tf_attention.inc"
