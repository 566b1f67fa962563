"""Every kernel instantiation kvecc_paged_attention can select, at the ragged
and buffer-end edges, against a float64 restatement of the operation.

PATHS lists one (codec, query dtype, head_dim, heads, kv_heads, batch) per
instantiation the launcher (csrc/attention.hip: attn_mfma_heads,
attn_heads_per_wg, launch_split_w, launch_split_gqa, launch_mfma) picks for a
cache under 4 GiB and a 16-byte-aligned query, with the instantiation's name.
`_select` restates those functions; `test_table_is_the_launchers_choice`
checks every entry's name against it and the table against a sweep of every
head_dim, group and dtype, so a changed launcher shows up here as a stale table.
profiles/attention_paths/kernels.txt is a kernel trace of this file (the suite
does not read it).

Not reachable at a small shape, and not listed:
- the 64-bit-addressed kernels (BUF = false): caches of 4 GiB and more only
  (`_select(..., buf=False)` restates their choice; tests/test_paged_cache_large.py runs them);
- Hamming(8,4) VEC 4 at W 32 / 64 and Golay at W 64: compiled, but head_dim
  would exceed 256, which kvecc_paged_attention refuses.
Reachable only at other shapes than the usual ones: with fp16 queries every
even group at head_dim 32 / 64 / 128 (Hamming(8,4)) or 128 (Golay) goes to a
matrix-core kernel, so the fp16 split kernels are listed at a group of 3
(G = 1) and at head_dim 40 / 72 / 100 / 256 (G = 2 / 4).

The edge bundle (one call per entry and max_context_len): batch 4, 2 layers of
which the last is read, block_size 16, context_lens [96, 1, 0, 41], a table two
columns wider than the longest sequence.  Sequence 0's last block is the
cache's last block, so with the last layer and the last cache head its final
token is the buffer's last row; sequence 1's one token is in block 0; sequence
2 is empty; sequence 3 has a -1 block inside its context.  The buffer's last
row holds the largest nibble (15) at the largest scale in K and V, and the
last query head of sequence 0 is non-negative, so that row has weight in that
head and losing its last codeword is visible (test_buffer_end_row_is_visible
asserts by how much).
"""

import functools
import math

import pytest
import torch

from tests.test_attention import _pack_golay

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
# the suite's tolerances (tests/test_attention.py): (atol, rtol) per query dtype
TOL = {F32: (2e-5, 2e-4), F16: (1e-3, 1e-3), BF16: (1e-2, 1e-2)}
EMPTY = {"hamming84": -8.0, "golay": 0.0, "golay_packed": 0.0}

# ---- the launcher, restated ------------------------------------------------------------
K_BLOCK, K_MAX_SPLIT, K_MAX_SPLITS, CUS = 256, 1024, 1024, 256
K_COMBINE_WAVE_SPLITS, K_CTR_PER_SLOT = 16, 4096
_TNAME = {F32: "float", F16: "__half", BF16: "__hip_bfloat16"}
_CODEC = {"hamming84": 2, "golay": 3, "golay_packed": 4}  # KVECC_CODEC_*


def _pow2(x):
    w = 1
    while w < x:
        w <<= 1
    return w


def _cdiv(a, b):
    return -(-a // b)


def _words(codec, d):
    return d // 4 if codec == "hamming84" else (d + 2) // 3


def _mfma_heads(codec, dtype, d, heads, kvh, buf=True):
    group = heads // kvh
    h84 = codec == "hamming84" and d in (32, 64, 128)
    golay = codec != "hamming84" and d == 128
    if not (h84 or golay) or dtype != F16 or not buf:
        return 0
    if group == 1:
        return 1 if h84 else 0
    return next((g for g in (16, 8, 4, 2) if group % g == 0), 0)


def _heads_per_wg(codec, d, heads, kvh, buf=True):
    group = heads // kvh
    vec = (2 if d % 8 == 0 else 1) if codec == "hamming84" else 3
    w = _pow2(_cdiv(_words(codec, d), vec))
    if not buf or w < 8 or w > 32 or (codec == "hamming84" and d % 8 != 0):
        return 1
    gmax = 2 if codec == "golay_packed" else 4
    return 4 if group % 4 == 0 and gmax >= 4 else 2 if group % 2 == 0 else 1


def _select(codec, dtype, d, heads, kvh, buf=True):
    """-> (kernel name, query heads per workgroup, workgroups per CU of its split choice).
    buf: the caches are buffer-addressable (attn_setup's `fits`: under 4 GiB); False restates the
    launcher's choice for a cache of 4 GiB or more -- no matrix cores, one head per workgroup."""
    gm = _mfma_heads(codec, dtype, d, heads, kvh, buf)
    if gm:
        if codec == "hamming84":
            return f"paged_attn_h84_mfma_kernel<{d}, {gm}>", gm, 4
        return f"paged_attn_golay_mfma_kernel<{gm}, {'true' if codec == 'golay_packed' else 'false'}>", gm, 2
    gq = _heads_per_wg(codec, d, heads, kvh, buf)
    if codec == "hamming84":
        vec = 2 if gq > 1 else 4 if d % 16 == 0 else 1
    else:
        vec = 3
    w = _pow2(_cdiv(_words(codec, d), vec))
    b = "true" if buf else "false"
    return f"paged_attn_split_kernel<{_TNAME[dtype]}, {_CODEC[codec]}, {vec}, {w}, {b}, {gq}, 0, 0>", gq, 4


def _choose_split(bh, mcl, per_cu=4):
    split = K_MAX_SPLIT
    while split > 32 and bh * _cdiv(mcl, split) < per_cu * CUS:
        split >>= 1
    while _cdiv(mcl, split) > K_MAX_SPLITS and split < K_MAX_SPLIT:
        split <<= 1
    return split


def _geometry(codec, dtype, d, heads, kvh, batch, mcl):
    """-> (split, nsplit, combine): the combine is 'fused' (the last split's
    workgroup, counted), or the name of the combine kernel launched."""
    name, gw, per_cu = _select(codec, dtype, d, heads, kvh)
    if "mfma" in name:
        split = max(_choose_split(batch * heads // gw, mcl, per_cu), _choose_split(max(1, batch * heads // 4), mcl))
        t = "__half"
    else:
        split = _choose_split(batch * heads // gw, mcl)
        t = _TNAME[dtype]
    nsplit = _cdiv(mcl, split)
    if gw == 1 and batch * heads <= K_CTR_PER_SLOT:
        return split, nsplit, "fused"
    if nsplit <= K_COMBINE_WAVE_SPLITS and d <= 128:
        return split, nsplit, f"paged_attn_combine_wave_kernel<{t}>"
    return split, nsplit, f"paged_attn_combine_kernel<{t}>"


# ---- the path table -----------------------------------------------------------------------
# (codec, query dtype, head_dim, heads, kv_heads, batch, the instantiation selected)
PATHS = [
    ("hamming84", F16, 32, 2, 2, 4, "paged_attn_h84_mfma_kernel<32, 1>"),
    ("hamming84", F16, 64, 2, 2, 4, "paged_attn_h84_mfma_kernel<64, 1>"),
    ("hamming84", F16, 128, 2, 2, 4, "paged_attn_h84_mfma_kernel<128, 1>"),
    ("hamming84", F16, 32, 4, 2, 4, "paged_attn_h84_mfma_kernel<32, 2>"),
    ("hamming84", F16, 32, 8, 2, 4, "paged_attn_h84_mfma_kernel<32, 4>"),
    ("hamming84", F16, 32, 16, 2, 4, "paged_attn_h84_mfma_kernel<32, 8>"),
    ("hamming84", F16, 32, 32, 2, 4, "paged_attn_h84_mfma_kernel<32, 16>"),
    ("hamming84", F16, 64, 4, 2, 4, "paged_attn_h84_mfma_kernel<64, 2>"),
    ("hamming84", F16, 64, 8, 2, 4, "paged_attn_h84_mfma_kernel<64, 4>"),
    ("hamming84", F16, 64, 16, 2, 4, "paged_attn_h84_mfma_kernel<64, 8>"),
    ("hamming84", F16, 64, 32, 2, 4, "paged_attn_h84_mfma_kernel<64, 16>"),
    ("hamming84", F16, 128, 4, 2, 4, "paged_attn_h84_mfma_kernel<128, 2>"),
    ("hamming84", F16, 128, 8, 2, 4, "paged_attn_h84_mfma_kernel<128, 4>"),
    ("hamming84", F16, 128, 16, 2, 4, "paged_attn_h84_mfma_kernel<128, 8>"),
    ("hamming84", F16, 128, 32, 2, 4, "paged_attn_h84_mfma_kernel<128, 16>"),
    ("golay", F16, 128, 4, 2, 4, "paged_attn_golay_mfma_kernel<2, false>"),
    ("golay", F16, 128, 8, 2, 4, "paged_attn_golay_mfma_kernel<4, false>"),
    ("golay", F16, 128, 16, 2, 4, "paged_attn_golay_mfma_kernel<8, false>"),
    ("golay", F16, 128, 32, 2, 4, "paged_attn_golay_mfma_kernel<16, false>"),
    ("golay_packed", F16, 128, 4, 2, 4, "paged_attn_golay_mfma_kernel<2, true>"),
    ("golay_packed", F16, 128, 8, 2, 4, "paged_attn_golay_mfma_kernel<4, true>"),
    ("golay_packed", F16, 128, 16, 2, 4, "paged_attn_golay_mfma_kernel<8, true>"),
    ("golay_packed", F16, 128, 32, 2, 4, "paged_attn_golay_mfma_kernel<16, true>"),
    ("golay", F32, 7, 2, 2, 4, "paged_attn_split_kernel<float, 3, 3, 1, true, 1, 0, 0>"),
    ("golay", F32, 12, 2, 2, 4, "paged_attn_split_kernel<float, 3, 3, 2, true, 1, 0, 0>"),
    ("golay", F32, 20, 2, 2, 4, "paged_attn_split_kernel<float, 3, 3, 4, true, 1, 0, 0>"),
    ("golay", F32, 64, 2, 2, 4, "paged_attn_split_kernel<float, 3, 3, 8, true, 1, 0, 0>"),
    ("golay", F32, 128, 2, 2, 4, "paged_attn_split_kernel<float, 3, 3, 16, true, 1, 0, 0>"),
    ("golay", F32, 256, 2, 2, 4, "paged_attn_split_kernel<float, 3, 3, 32, true, 1, 0, 0>"),
    ("golay", F32, 64, 4, 2, 4, "paged_attn_split_kernel<float, 3, 3, 8, true, 2, 0, 0>"),
    ("golay", F32, 64, 8, 2, 4, "paged_attn_split_kernel<float, 3, 3, 8, true, 4, 0, 0>"),
    ("golay", F32, 128, 4, 2, 4, "paged_attn_split_kernel<float, 3, 3, 16, true, 2, 0, 0>"),
    ("golay", F32, 128, 8, 2, 4, "paged_attn_split_kernel<float, 3, 3, 16, true, 4, 0, 0>"),
    ("golay", F32, 256, 4, 2, 4, "paged_attn_split_kernel<float, 3, 3, 32, true, 2, 0, 0>"),
    ("golay", F32, 256, 8, 2, 4, "paged_attn_split_kernel<float, 3, 3, 32, true, 4, 0, 0>"),
    ("golay", F16, 4, 2, 2, 4, "paged_attn_split_kernel<__half, 3, 3, 1, true, 1, 0, 0>"),
    ("golay", F16, 12, 2, 2, 4, "paged_attn_split_kernel<__half, 3, 3, 2, true, 1, 0, 0>"),
    ("golay", F16, 20, 2, 2, 4, "paged_attn_split_kernel<__half, 3, 3, 4, true, 1, 0, 0>"),
    ("golay", F16, 64, 2, 2, 4, "paged_attn_split_kernel<__half, 3, 3, 8, true, 1, 0, 0>"),
    ("golay", F16, 128, 2, 2, 4, "paged_attn_split_kernel<__half, 3, 3, 16, true, 1, 0, 0>"),
    ("golay", F16, 256, 2, 2, 4, "paged_attn_split_kernel<__half, 3, 3, 32, true, 1, 0, 0>"),
    ("golay", F16, 64, 4, 2, 4, "paged_attn_split_kernel<__half, 3, 3, 8, true, 2, 0, 0>"),
    ("golay", F16, 64, 8, 2, 4, "paged_attn_split_kernel<__half, 3, 3, 8, true, 4, 0, 0>"),
    ("golay", F16, 100, 4, 2, 4, "paged_attn_split_kernel<__half, 3, 3, 16, true, 2, 0, 0>"),
    ("golay", F16, 100, 8, 2, 4, "paged_attn_split_kernel<__half, 3, 3, 16, true, 4, 0, 0>"),
    ("golay", F16, 256, 4, 2, 4, "paged_attn_split_kernel<__half, 3, 3, 32, true, 2, 0, 0>"),
    ("golay", F16, 256, 8, 2, 4, "paged_attn_split_kernel<__half, 3, 3, 32, true, 4, 0, 0>"),
    ("golay", BF16, 5, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 3, 3, 1, true, 1, 0, 0>"),
    ("golay", BF16, 12, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 3, 3, 2, true, 1, 0, 0>"),
    ("golay", BF16, 20, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 3, 3, 4, true, 1, 0, 0>"),
    ("golay", BF16, 64, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 3, 3, 8, true, 1, 0, 0>"),
    ("golay", BF16, 128, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 3, 3, 16, true, 1, 0, 0>"),
    ("golay", BF16, 256, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 3, 3, 32, true, 1, 0, 0>"),
    ("golay", BF16, 64, 4, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 3, 3, 8, true, 2, 0, 0>"),
    ("golay", BF16, 64, 8, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 3, 3, 8, true, 4, 0, 0>"),
    ("golay", BF16, 128, 4, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 3, 3, 16, true, 2, 0, 0>"),
    ("golay", BF16, 128, 8, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 3, 3, 16, true, 4, 0, 0>"),
    ("golay", BF16, 256, 4, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 3, 3, 32, true, 2, 0, 0>"),
    ("golay", BF16, 256, 8, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 3, 3, 32, true, 4, 0, 0>"),
    ("golay_packed", F32, 7, 2, 2, 4, "paged_attn_split_kernel<float, 4, 3, 1, true, 1, 0, 0>"),
    ("golay_packed", F32, 12, 2, 2, 4, "paged_attn_split_kernel<float, 4, 3, 2, true, 1, 0, 0>"),
    ("golay_packed", F32, 20, 2, 2, 4, "paged_attn_split_kernel<float, 4, 3, 4, true, 1, 0, 0>"),
    ("golay_packed", F32, 64, 2, 2, 4, "paged_attn_split_kernel<float, 4, 3, 8, true, 1, 0, 0>"),
    ("golay_packed", F32, 128, 2, 2, 4, "paged_attn_split_kernel<float, 4, 3, 16, true, 1, 0, 0>"),
    ("golay_packed", F32, 256, 2, 2, 4, "paged_attn_split_kernel<float, 4, 3, 32, true, 1, 0, 0>"),
    ("golay_packed", F32, 64, 4, 2, 4, "paged_attn_split_kernel<float, 4, 3, 8, true, 2, 0, 0>"),
    ("golay_packed", F32, 128, 8, 2, 4, "paged_attn_split_kernel<float, 4, 3, 16, true, 2, 0, 0>"),
    ("golay_packed", F32, 256, 4, 2, 4, "paged_attn_split_kernel<float, 4, 3, 32, true, 2, 0, 0>"),
    ("golay_packed", F16, 4, 2, 2, 4, "paged_attn_split_kernel<__half, 4, 3, 1, true, 1, 0, 0>"),
    ("golay_packed", F16, 12, 2, 2, 4, "paged_attn_split_kernel<__half, 4, 3, 2, true, 1, 0, 0>"),
    ("golay_packed", F16, 20, 2, 2, 4, "paged_attn_split_kernel<__half, 4, 3, 4, true, 1, 0, 0>"),
    ("golay_packed", F16, 64, 2, 2, 4, "paged_attn_split_kernel<__half, 4, 3, 8, true, 1, 0, 0>"),
    ("golay_packed", F16, 128, 2, 2, 4, "paged_attn_split_kernel<__half, 4, 3, 16, true, 1, 0, 0>"),
    ("golay_packed", F16, 256, 2, 2, 4, "paged_attn_split_kernel<__half, 4, 3, 32, true, 1, 0, 0>"),
    ("golay_packed", F16, 64, 4, 2, 4, "paged_attn_split_kernel<__half, 4, 3, 8, true, 2, 0, 0>"),
    ("golay_packed", F16, 100, 4, 2, 4, "paged_attn_split_kernel<__half, 4, 3, 16, true, 2, 0, 0>"),
    ("golay_packed", F16, 256, 4, 2, 4, "paged_attn_split_kernel<__half, 4, 3, 32, true, 2, 0, 0>"),
    ("golay_packed", BF16, 5, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 4, 3, 1, true, 1, 0, 0>"),
    ("golay_packed", BF16, 12, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 4, 3, 2, true, 1, 0, 0>"),
    ("golay_packed", BF16, 20, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 4, 3, 4, true, 1, 0, 0>"),
    ("golay_packed", BF16, 64, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 4, 3, 8, true, 1, 0, 0>"),
    ("golay_packed", BF16, 128, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 4, 3, 16, true, 1, 0, 0>"),
    ("golay_packed", BF16, 256, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 4, 3, 32, true, 1, 0, 0>"),
    ("golay_packed", BF16, 64, 4, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 4, 3, 8, true, 2, 0, 0>"),
    ("golay_packed", BF16, 128, 8, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 4, 3, 16, true, 2, 0, 0>"),
    ("golay_packed", BF16, 256, 4, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 4, 3, 32, true, 2, 0, 0>"),
    ("hamming84", F32, 4, 2, 2, 4, "paged_attn_split_kernel<float, 2, 1, 1, true, 1, 0, 0>"),
    ("hamming84", F32, 8, 2, 2, 4, "paged_attn_split_kernel<float, 2, 1, 2, true, 1, 0, 0>"),
    ("hamming84", F32, 12, 2, 2, 4, "paged_attn_split_kernel<float, 2, 1, 4, true, 1, 0, 0>"),
    ("hamming84", F32, 16, 2, 2, 4, "paged_attn_split_kernel<float, 2, 4, 1, true, 1, 0, 0>"),
    ("hamming84", F32, 20, 2, 2, 4, "paged_attn_split_kernel<float, 2, 1, 8, true, 1, 0, 0>"),
    ("hamming84", F32, 32, 2, 2, 4, "paged_attn_split_kernel<float, 2, 4, 2, true, 1, 0, 0>"),
    ("hamming84", F32, 52, 2, 2, 4, "paged_attn_split_kernel<float, 2, 1, 16, true, 1, 0, 0>"),
    ("hamming84", F32, 64, 2, 2, 4, "paged_attn_split_kernel<float, 2, 4, 4, true, 1, 0, 0>"),
    ("hamming84", F32, 100, 2, 2, 4, "paged_attn_split_kernel<float, 2, 1, 32, true, 1, 0, 0>"),
    ("hamming84", F32, 128, 2, 2, 4, "paged_attn_split_kernel<float, 2, 4, 8, true, 1, 0, 0>"),
    ("hamming84", F32, 252, 2, 2, 4, "paged_attn_split_kernel<float, 2, 1, 64, true, 1, 0, 0>"),
    ("hamming84", F32, 256, 2, 2, 4, "paged_attn_split_kernel<float, 2, 4, 16, true, 1, 0, 0>"),
    ("hamming84", F32, 64, 4, 2, 4, "paged_attn_split_kernel<float, 2, 2, 8, true, 2, 0, 0>"),
    ("hamming84", F32, 64, 8, 2, 4, "paged_attn_split_kernel<float, 2, 2, 8, true, 4, 0, 0>"),
    ("hamming84", F32, 128, 4, 2, 4, "paged_attn_split_kernel<float, 2, 2, 16, true, 2, 0, 0>"),
    ("hamming84", F32, 128, 8, 2, 4, "paged_attn_split_kernel<float, 2, 2, 16, true, 4, 0, 0>"),
    ("hamming84", F32, 256, 4, 2, 4, "paged_attn_split_kernel<float, 2, 2, 32, true, 2, 0, 0>"),
    ("hamming84", F32, 256, 8, 2, 4, "paged_attn_split_kernel<float, 2, 2, 32, true, 4, 0, 0>"),
    ("hamming84", F16, 4, 2, 2, 4, "paged_attn_split_kernel<__half, 2, 1, 1, true, 1, 0, 0>"),
    ("hamming84", F16, 8, 2, 2, 4, "paged_attn_split_kernel<__half, 2, 1, 2, true, 1, 0, 0>"),
    ("hamming84", F16, 12, 2, 2, 4, "paged_attn_split_kernel<__half, 2, 1, 4, true, 1, 0, 0>"),
    ("hamming84", F16, 16, 2, 2, 4, "paged_attn_split_kernel<__half, 2, 4, 1, true, 1, 0, 0>"),
    ("hamming84", F16, 20, 2, 2, 4, "paged_attn_split_kernel<__half, 2, 1, 8, true, 1, 0, 0>"),
    ("hamming84", F16, 52, 2, 2, 4, "paged_attn_split_kernel<__half, 2, 1, 16, true, 1, 0, 0>"),
    ("hamming84", F16, 100, 2, 2, 4, "paged_attn_split_kernel<__half, 2, 1, 32, true, 1, 0, 0>"),
    ("hamming84", F16, 252, 2, 2, 4, "paged_attn_split_kernel<__half, 2, 1, 64, true, 1, 0, 0>"),
    ("hamming84", F16, 256, 2, 2, 4, "paged_attn_split_kernel<__half, 2, 4, 16, true, 1, 0, 0>"),
    ("hamming84", F16, 32, 6, 2, 4, "paged_attn_split_kernel<__half, 2, 4, 2, true, 1, 0, 0>"),
    ("hamming84", F16, 40, 4, 2, 4, "paged_attn_split_kernel<__half, 2, 2, 8, true, 2, 0, 0>"),
    ("hamming84", F16, 40, 8, 2, 4, "paged_attn_split_kernel<__half, 2, 2, 8, true, 4, 0, 0>"),
    ("hamming84", F16, 64, 6, 2, 4, "paged_attn_split_kernel<__half, 2, 4, 4, true, 1, 0, 0>"),
    ("hamming84", F16, 72, 4, 2, 4, "paged_attn_split_kernel<__half, 2, 2, 16, true, 2, 0, 0>"),
    ("hamming84", F16, 72, 8, 2, 4, "paged_attn_split_kernel<__half, 2, 2, 16, true, 4, 0, 0>"),
    ("hamming84", F16, 128, 6, 2, 4, "paged_attn_split_kernel<__half, 2, 4, 8, true, 1, 0, 0>"),
    ("hamming84", F16, 256, 4, 2, 4, "paged_attn_split_kernel<__half, 2, 2, 32, true, 2, 0, 0>"),
    ("hamming84", F16, 256, 8, 2, 4, "paged_attn_split_kernel<__half, 2, 2, 32, true, 4, 0, 0>"),
    ("hamming84", BF16, 4, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 2, 1, 1, true, 1, 0, 0>"),
    ("hamming84", BF16, 8, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 2, 1, 2, true, 1, 0, 0>"),
    ("hamming84", BF16, 12, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 2, 1, 4, true, 1, 0, 0>"),
    ("hamming84", BF16, 16, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 2, 4, 1, true, 1, 0, 0>"),
    ("hamming84", BF16, 20, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 2, 1, 8, true, 1, 0, 0>"),
    ("hamming84", BF16, 32, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 2, 4, 2, true, 1, 0, 0>"),
    ("hamming84", BF16, 52, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 2, 1, 16, true, 1, 0, 0>"),
    ("hamming84", BF16, 64, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 2, 4, 4, true, 1, 0, 0>"),
    ("hamming84", BF16, 100, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 2, 1, 32, true, 1, 0, 0>"),
    ("hamming84", BF16, 128, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 2, 4, 8, true, 1, 0, 0>"),
    ("hamming84", BF16, 252, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 2, 1, 64, true, 1, 0, 0>"),
    ("hamming84", BF16, 256, 2, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 2, 4, 16, true, 1, 0, 0>"),
    ("hamming84", BF16, 64, 4, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 2, 2, 8, true, 2, 0, 0>"),
    ("hamming84", BF16, 64, 8, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 2, 2, 8, true, 4, 0, 0>"),
    ("hamming84", BF16, 128, 4, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 2, 2, 16, true, 2, 0, 0>"),
    ("hamming84", BF16, 128, 8, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 2, 2, 16, true, 4, 0, 0>"),
    ("hamming84", BF16, 256, 4, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 2, 2, 32, true, 2, 0, 0>"),
    ("hamming84", BF16, 256, 8, 2, 4, "paged_attn_split_kernel<__hip_bfloat16, 2, 2, 32, true, 4, 0, 0>"),
]


def _sweep():
    """Every instantiation the restated launcher reaches: name -> the first (smallest) shape."""
    found = {}
    for codec in ("hamming84", "golay", "golay_packed"):
        for dtype in (F32, F16, BF16):
            for d in range(1, 257):
                if codec == "hamming84" and d % 4:
                    continue
                for group in (1, 2, 3, 4, 8, 16):
                    name = _select(codec, dtype, d, 2 * group, 2)[0]
                    found.setdefault(name, (codec, dtype, d, 2 * group, 2, 4, name))
    return found


def test_table_is_the_launchers_choice():
    names = [p[6] for p in PATHS]
    assert len(set(names)) == len(names)
    for codec, dtype, d, heads, kvh, batch, name in PATHS:
        assert _select(codec, dtype, d, heads, kvh)[0] == name
        assert batch == 4 and kvh == 2
    assert set(names) == set(_sweep())
    # the combine forms the bundle reaches: the counted one, the one-wave kernel
    # and the block kernel (nsplit <= workgroup size); the > form: test_many_splits
    forms = {_geometry(*p[:6], 128)[2].split("<")[0] for p in PATHS}
    assert forms == {"fused", "paged_attn_combine_wave_kernel", "paged_attn_combine_kernel"}


# ---- data -----------------------------------------------------------------------------------
def _base(codec):
    return "hamming84" if codec == "hamming84" else "golay"


@functools.lru_cache(maxsize=None)
def _caches(base, d, kvh, bs, num_blocks, layers, ber, seed, pin_last_row):
    """Random caches written through the host backend (oracle-pinned) -> kc, vc, ks, vs
    ([blocks, layers, kv_heads, bs * words] / [blocks, layers, kv_heads, bs])."""
    from kvecc import cpu_ops
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, num_blocks, layers, kvh, bs, d, generator=g)
    if pin_last_row:
        x[:, -1, -1, -1, -1, :] = 4.0  # one value for the whole row: every nibble 15
    out = []
    for xi in x:
        q, _ = cpu_ops.quantize_rows(xi)
        if base == "hamming84":
            enc = cpu_ops.hamming84_encode(q)
        else:
            enc = cpu_ops.golay_encode_rows(q)
        if ber > 0:
            enc = cpu_ops.inject_bit_errors_triton(enc, ber, 8 if base == "hamming84" else 24, seed=seed)
        out.append(enc.reshape(num_blocks, layers, kvh, -1).contiguous())
    for _ in range(2):
        s = torch.rand(num_blocks, layers, kvh, bs, generator=g) * 0.3 + 0.05
        if pin_last_row:
            s[-1, -1, -1, -1] = 0.35
        out.append(s)
    return tuple(out)


def _unpack_golay(packed, d):
    """The packed layout back to int32 codewords (inverse of _pack_golay)."""
    g = (d + 2) // 3
    row = (3 * g + 3) // 4 * 4
    b = packed.view(*packed.shape[:-1], -1, row)[..., :3 * g].to(torch.int32)
    w = b[..., 0::3] | b[..., 1::3] << 8 | b[..., 2::3] << 16
    return w.reshape(*packed.shape[:-1], -1).contiguous()


def _for_codec(codec, d, kc, vc):
    return (_pack_golay(kc, d), _pack_golay(vc, d)) if codec == "golay_packed" else (kc, vc)


def _zero_tail(codec, d, kc, vc):
    """The int32 / uint8 caches as the reference reads them after the last 4 bytes of
    each buffer, in the layout the kernel is given, are zeroed: the last codeword
    (int32 Golay) or the last four (Hamming(8,4)).  A packed row ends in 0-3 bytes
    of padding after its last 3-byte codeword, so its last 4 bytes hold padding
    and that codeword's parity bits only, which the decoder corrects back (measured:
    no output moves at all); there the zeroing starts at the last codeword's first
    byte, which covers the last 4 bytes whenever the row is padded."""
    g = (d + 2) // 3
    nz = max(4, 3 + (-3 * g) % 4) if codec == "golay_packed" else 4
    out = []
    for c in _for_codec(codec, d, kc, vc):
        c = c.clone()
        c.view(-1).view(torch.uint8)[-nz:] = 0
        out.append(_unpack_golay(c, d) if codec == "golay_packed" else c)
    return out


def _ref64(q, kc, vc, table, lens, ks, vs, layer, bs, base):
    """float64 paged attention over the int32 / uint8 caches: decode through cpu_ops,
    dequantize, softmax over the valid tokens per (b, h), every head of a batch row at once."""
    from kvecc import cpu_ops
    nb_, nl_, kvh, _ = kc.shape
    b_, h_, d = q.shape
    out = torch.empty(b_, h_, d, dtype=torch.float64)
    for b in range(b_):
        n = min(max(int(lens[b]), 0), table.shape[1] * bs)
        pos = torch.arange(n)
        blk = table[b, pos // bs].long()
        ok = blk >= 0
        if not bool(ok.any()):
            out[b] = EMPTY[base]
            continue
        blk, slot = blk[ok], (pos % bs)[ok]
        f = []
        for cache, sc in ((kc, ks), (vc, vs)):
            rows = cache.view(nb_, nl_, kvh, bs, -1)[blk, layer, :, slot].contiguous()  # [n, Hkv, words]
            dec = cpu_ops.hamming84_decode(rows)[0] if base == "hamming84" else cpu_ops.golay_decode_rows(rows, d)
            f.append((dec.double() - 8.0) * sc[blk, layer, :, slot].double().unsqueeze(-1))
        s = torch.einsum("kgd,nkd->kgn", q[b].double().view(kvh, h_ // kvh, d), f[0]) / math.sqrt(d)
        out[b] = torch.einsum("kgn,nkd->kgd", torch.softmax(s, dim=-1), f[1]).reshape(h_, d)
    return out


def _query(batch, heads, d, dtype, seed=1):
    return torch.randn(batch, heads, d, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _attend(mod, dev, codec, q, kc, vc, table, lens, ks, vs, layer, bs, mcl=0):
    """paged_attention_into of ops (dev: the GPU) or cpu_ops (dev None) -> float64 on the host."""
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    d = q.shape[-1]
    pk, pv = _for_codec(codec, d, kc, vc)
    out = torch.empty(q.shape, dtype=q.dtype, device=dev)
    mod.paged_attention_into(t(q), t(pk), t(pv), t(table), t(lens), t(ks), t(vs), out, layer, bs,
                             1 / math.sqrt(d), codec, max_context_len=mcl)
    return out.cpu().double()


def _close(got, ref, dtype):
    atol, rtol = TOL[dtype]
    return bool(((got - ref).abs() <= atol + rtol * ref.abs()).all())


def _err(got, ref):
    return float((got - ref).abs().max())


# ---- the edge bundle ----------------------------------------------------------------------------
LAYERS, LAYER = 2, 1


@functools.lru_cache(maxsize=None)
def _bundle(codec, dtype, d, heads, kvh, bs):
    """bs 16: the bundle of the module docstring.  bs 4: the same with sequence 0
    holding the cache's last block only (its last row carries about a quarter of
    the softmax weight; the bf16 entries' buffer-end case)."""
    base = _base(codec)
    lens = torch.tensor([96 if bs == 16 else bs, 1, 0, 41], dtype=torch.int32)
    nblk = [_cdiv(int(n), bs) for n in lens]
    num_blocks = nblk[0] + 1 + 1 + nblk[3] + 2
    kc, vc, ks, vs = _caches(base, d, kvh, bs, num_blocks, LAYERS, 0.01, 100 + d, True)
    mid = (1 + torch.randperm(num_blocks - 2, generator=torch.Generator().manual_seed(d))).to(torch.int32).tolist()
    table = torch.full((4, max(nblk) + 2), -1, dtype=torch.int32)
    table[0, :nblk[0]] = torch.tensor([mid.pop() for _ in range(nblk[0] - 1)] + [num_blocks - 1])
    table[1, 0] = 0
    table[2, 0] = mid.pop()  # a block it owns, at length 0
    table[3, :nblk[3]] = torch.tensor([mid.pop() for _ in range(nblk[3])])
    table[3, nblk[3] // 2] = -1  # tokens inside the context are skipped
    q = _query(4, heads, d, dtype)
    # sequence 0's last head looks at the last row (K there is +7 k_scale in every lane)
    q[0, -1] = q[0, -1].abs() * 0.5
    ref = _ref64(q, kc, vc, table, lens, ks, vs, LAYER, bs, base)
    zk, zv = _zero_tail(codec, d, kc, vc)
    moved = _ref64(q[:1], zk, zv, table[:1], lens[:1], ks, vs, LAYER, bs, base)
    return dict(q=q, kc=kc, vc=vc, table=table, lens=lens, ks=ks, vs=vs, ref=ref, moved=moved)


def _check_bundle(mod, dev, path, bs):
    codec, dtype, d, heads, kvh, _, _ = path
    c = _bundle(codec, dtype, d, heads, kvh, bs)
    for mcl in (0, int(c["lens"].max())):  # the default, and what append mode passes
        got = _attend(mod, dev, codec, c["q"], c["kc"], c["vc"], c["table"], c["lens"], c["ks"], c["vs"],
                      LAYER, bs, mcl)
        assert torch.equal(got[2], torch.full((heads, d), EMPTY[codec], dtype=torch.float64)), mcl
        assert _close(got, c["ref"], dtype), (mcl, _err(got, c["ref"]))


def _id(path):
    return f"{path[0]}-{_TNAME[path[1]].strip('_')}-d{path[2]}-{path[3]}q{path[4]}kv"


BF16_PATHS = [p for p in PATHS if p[1] == BF16]


@pytest.mark.parametrize("path", PATHS, ids=_id)
def test_cpu_bundle(path):
    from kvecc import cpu_ops
    _check_bundle(cpu_ops, None, path, 16)


@pytest.mark.parametrize("path", BF16_PATHS, ids=_id)
def test_cpu_bundle_last_block_only(path):
    from kvecc import cpu_ops
    _check_bundle(cpu_ops, None, path, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS, ids=_id)
def test_hip_bundle(gpu, path):
    from kvecc import ops
    _check_bundle(ops, gpu, path, 16)


@pytest.mark.gpu
@pytest.mark.parametrize("path", BF16_PATHS, ids=_id)
def test_hip_bundle_last_block_only(gpu, path):
    from kvecc import ops
    _check_bundle(ops, gpu, path, 4)


@pytest.mark.parametrize("path", PATHS, ids=_id)
def test_buffer_end_row_is_visible(path):
    """With the last 4 bytes of each cache buffer zeroed the reference's last query
    head of sequence 0 moves by at least 10 tolerances, so a kernel whose load
    dropped the row's last codeword fails the bundle.  bf16 entries: in the
    last-block-only bundle."""
    codec, dtype, d, heads, kvh, _, _ = path
    c = _bundle(codec, dtype, d, heads, kvh, 4 if dtype == BF16 else 16)
    ref, moved = c["ref"][0, -1], c["moved"][0, -1]
    atol, rtol = TOL[dtype]
    assert float(((moved - ref).abs() - 10 * (atol + rtol * ref.abs())).max()) >= 0, _err(moved, ref)
    # the heads of the other cache head read nothing of the last row
    assert torch.equal(c["moved"][0, :heads // kvh], c["ref"][0, :heads // kvh])


# ---- the max_context_len contract ------------------------------------------------------------------
# one entry per kernel family: split G = 1, split GQA, Hamming(8,4) matrix-core, Golay matrix-core
FAMILIES = [("golay", F32, 64, 2, 2), ("hamming84", F32, 64, 8, 2), ("hamming84", F16, 128, 8, 2),
            ("golay_packed", F16, 128, 8, 2)]


def test_families_are_what_they_say():
    kinds = [_select(*f)[0] for f in FAMILIES]
    assert kinds == ["paged_attn_split_kernel<float, 3, 3, 8, true, 1, 0, 0>",
                     "paged_attn_split_kernel<float, 2, 2, 8, true, 4, 0, 0>",
                     "paged_attn_h84_mfma_kernel<128, 4>", "paged_attn_golay_mfma_kernel<4, true>"]


@functools.lru_cache(maxsize=None)
def _contract(family, bs=16, nblk=7):
    codec, dtype, d, heads, kvh = family
    kc, vc, ks, vs = _caches(_base(codec), d, kvh, bs, 2 * nblk + 1, 2, 0.01, 7 + d, False)
    table = torch.randperm(2 * nblk + 1, generator=torch.Generator().manual_seed(3))[:2 * nblk]
    return dict(q=_query(2, heads, d, dtype, seed=5), kc=kc, vc=vc, ks=ks, vs=vs,
                table=table.to(torch.int32).view(2, nblk).contiguous())


def _contract_run(mod, dev, family, lens, mcl):
    c = _contract(family)
    return _attend(mod, dev, family[0], c["q"], c["kc"], c["vc"], c["table"],
                   torch.tensor(lens, dtype=torch.int32), c["ks"], c["vs"], 1, 16, mcl)


def _contract_ref(family, lens):
    c = _contract(family)
    return _ref64(c["q"], c["kc"], c["vc"], c["table"], torch.tensor(lens, dtype=torch.int32), c["ks"], c["vs"],
                  1, 16, _base(family[0]))


def _check_contract(mod, dev, family):
    from kvecc import cpu_ops
    dtype = family[1]
    # context_lens above max_context_len are attended up to max_context_len (include/kvecc.h)
    got = _contract_run(mod, dev, family, [100, 93], 50)
    ref = _contract_ref(family, [50, 50])
    print(f"clamp: max |got - ref(lens 50)| = {_err(got, ref):.3e}, "
          f"max |ref(lens 100, 93) - ref(lens 50)| = {_err(_contract_ref(family, [100, 93]), ref):.3e}")
    assert _close(got, ref, dtype), _err(got, ref)
    if dev is not None:  # and the host twin, which clamps
        twin = _contract_run(cpu_ops, None, family, [100, 93], 50)
        assert _close(got, twin, dtype), _err(got, twin)
    # max_context_len past the table: the table (7 blocks of 16) bounds the context
    got = _contract_run(mod, dev, family, [100, 200], 300)
    assert _close(got, _contract_ref(family, [100, 112]), dtype)
    assert _close(got, _contract_run(mod, dev, family, [100, 200], 0), dtype)
    # a negative length is an empty context
    got = _contract_run(mod, dev, family, [-5, 93], 0)
    assert torch.equal(got[0], torch.full(got[0].shape, EMPTY[family[0]], dtype=torch.float64))
    assert _close(got, _contract_ref(family, [0, 93]), dtype)


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f"{f[0]}-{_TNAME[f[1]].strip('_')}-{f[3]}q{f[4]}kv")
def test_cpu_max_context_len_contract(family):
    from kvecc import cpu_ops
    _check_contract(cpu_ops, None, family)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f"{f[0]}-{_TNAME[f[1]].strip('_')}-{f[3]}q{f[4]}kv")
def test_hip_max_context_len_contract(gpu, family):
    from kvecc import ops
    _check_contract(ops, gpu, family)


# ---- coarse splits -----------------------------------------------------------------------------------
# split = kMaxSplit survives choose_split when (batch x heads / G) x splits >= 4 x 256 CUs: two
# splits (context 1025..2048) need batch x heads = 512, the smallest product at any split count
# (three splits: 342 x 2049 tokens).  head_dim 32 keeps G = 1 for both codecs at any group, so 64
# query heads over 8 cache heads give the same grid as MHA over a cache an eighth the size.
COARSE = [("hamming84", F32, 32, 64, 8, 8), ("golay", F32, 32, 64, 8, 8)]
COARSE_LENS = [1030, 1025, 1024, 1023, 513, 1, 0, 777]
# more splits than the combine workgroup has threads (split 32 x 257): the counted combine
# (fp32, one head per workgroup) and the block combine kernel (fp16, matrix-core G = 2)
MANY = [("hamming84", F32, 32, 2, 2, 1), ("hamming84", F16, 32, 2, 1, 1)]
MANY_LEN = 32 * K_BLOCK + 8


def test_split_geometry_of_the_long_cases():
    for c in COARSE:
        mcl = _cdiv(max(COARSE_LENS), 16) * 16
        assert _geometry(*c, mcl)[:2] == (K_MAX_SPLIT, 2)
        assert _geometry(*c[:5], c[5] - 1, mcl)[0] < K_MAX_SPLIT  # one batch row fewer splits finer
    mcl = _cdiv(MANY_LEN, 16) * 16
    assert _geometry(*MANY[0], mcl) == (32, K_BLOCK + 1, "fused")
    assert _geometry(*MANY[1], mcl) == (32, K_BLOCK + 1, "paged_attn_combine_kernel<__half>")


@functools.lru_cache(maxsize=None)
def _long(case, lens):
    codec, dtype, d, heads, kvh, batch = case
    nblk = _cdiv(max(lens), 16)
    kc, vc, ks, vs = _caches(_base(codec), d, kvh, 16, batch * nblk + 1, 1, 0.01, 11, False)
    table = torch.randperm(batch * nblk + 1, generator=torch.Generator().manual_seed(2))[:batch * nblk]
    table = table.to(torch.int32).view(batch, nblk).contiguous()
    table[0, 1] = -1
    lens = torch.tensor(lens, dtype=torch.int32)
    q = _query(batch, heads, d, dtype, seed=9)
    return dict(q=q, kc=kc, vc=vc, ks=ks, vs=vs, table=table, lens=lens,
                ref=_ref64(q, kc, vc, table, lens, ks, vs, 0, 16, _base(codec)))


def _check_long(mod, dev, case, lens):
    c = _long(case, tuple(lens))
    got = _attend(mod, dev, case[0], c["q"], c["kc"], c["vc"], c["table"], c["lens"], c["ks"], c["vs"], 0, 16)
    assert _close(got, c["ref"], case[1]), _err(got, c["ref"])


@pytest.mark.parametrize("case", COARSE, ids=lambda c: c[0])
def test_cpu_coarse_split(case):
    from kvecc import cpu_ops
    _check_long(cpu_ops, None, case, COARSE_LENS)


@pytest.mark.gpu
@pytest.mark.parametrize("case", COARSE, ids=lambda c: c[0])
def test_hip_coarse_split(gpu, case):
    from kvecc import ops
    _check_long(ops, gpu, case, COARSE_LENS)


@pytest.mark.parametrize("case", MANY, ids=lambda c: _TNAME[c[1]].strip("_"))
def test_cpu_many_splits(case):
    from kvecc import cpu_ops
    _check_long(cpu_ops, None, case, [MANY_LEN])


@pytest.mark.gpu
@pytest.mark.parametrize("case", MANY, ids=lambda c: _TNAME[c[1]].strip("_"))
def test_hip_many_splits(gpu, case):
    from kvecc import ops
    _check_long(ops, gpu, case, [MANY_LEN])
