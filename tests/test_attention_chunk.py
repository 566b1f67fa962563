"""kvecc_paged_attention_chunk: q_len query tokens per sequence, causal, against a
float64 restatement and against the decode entry row by row.

Contract (include/kvecc.h): context_lens[b] counts the chunk's own tokens;
query t of sequence b sits at position p = context_lens[b] - q_len + t and
attends to the keys j <= p below min(max_context_len, max_blocks * block_size);
-1 blocks are skipped; a row without a valid key gets the decode entry's empty
value.  Every case runs on the host twin and, marked gpu, on the device.

`_chunk_select` restates the launcher's choice (csrc/attention.hip:
attn_chunk_mfma_heads and kvecc_paged_attention_chunk): fp16 queries with
16-byte aligned rows over Hamming(8,4) at head_dim 32 / 64 / 128 or Golay at
128, for a group of 1 or an even one, go to a matrix-core chunk kernel whose 16
columns are (token, head) pairs; everything else runs the split kernels over
the virtual batch of batch * q_len rows.

The edge bundle (one launch per path, q_len and max_context_len): batch 5,
block_size 16, context_lens [q_len, q_len + 41, 0, q_len - 1, 96 + q_len].
Sequence 4 is the longest; a -1 block sits in its middle and its second block
is the cache's last block, whose last row (the buffer's last row, last layer,
last cache head, nibble 15 at the largest scale) is position 31, which every
one of its query rows sees.  The -1 first block is sequence 0's for q_len <= 16
(all its rows empty; sequence 3's row 1 is then the row that sees one key) and
sequence 3's above (its rows 0..16 are empty, the later ones see block 1 only,
and sequence 0's position 0 sees one key).
"""

import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from tests.test_attention_decode_probe import COLS, _cache, _oracle, _per_head, _rows
from tests.test_attention_decode_probe import LAYER as P_LAYER
from tests.test_attention_decode_probe import LAYERS as P_LAYERS
from tests.test_attention_paths import (BF16, EMPTY, F16, F32, FAMILIES, K_BLOCK, TOL, _TNAME, _attend, _base,
                                        _caches, _cdiv, _choose_split, _close, _contract, _err, _for_codec,
                                        _select)

LAYERS, LAYER, BS = 2, 1, 16


# ---- the launcher, restated ---------------------------------------------------------------------
def _chunk_mfma_heads(codec, dtype, d, heads, kvh, buf=True):
    group = heads // kvh
    h84 = codec == "hamming84" and d in (32, 64, 128)
    golay = codec != "hamming84" and d == 128
    if not (h84 or golay) or dtype != F16 or not buf:
        return 0
    if group == 1:
        return 1
    return next((g for g in (16, 8, 4, 2) if group % g == 0), 0)


def _chunk_select(codec, dtype, d, heads, kvh, buf=True):
    """-> (kernel name, heads per column group or per workgroup, workgroups per CU) at q_len > 1
    for a query with 16-byte aligned rows; buf False: over a cache of 4 GiB or more (_select)."""
    gm = _chunk_mfma_heads(codec, dtype, d, heads, kvh, buf)
    if gm:
        if codec == "hamming84":
            return f"paged_attn_h84_mfma_chunk_kernel<{d}>", gm, 4
        return f"paged_attn_golay_mfma_chunk_kernel<{'true' if codec == 'golay_packed' else 'false'}>", gm, 2
    name, gq, per_cu = _select(codec, dtype, d, heads, kvh, buf)  # the split kernels over the virtual batch
    assert "split_kernel" in name
    return name, gq, per_cu


def _chunk_geometry(codec, dtype, d, heads, kvh, batch, q_len, mcl):
    name, g, per_cu = _chunk_select(codec, dtype, d, heads, kvh)
    if "mfma" in name:
        wgs = batch * (heads // g) * _cdiv(q_len, 16 // g)
    else:
        wgs = batch * q_len * heads // g
    split = max(_choose_split(wgs, mcl, per_cu), _choose_split(max(1, batch * q_len * heads // 16), mcl))
    return split, _cdiv(mcl, split)


# matrix-core paths: every chunk instantiation at MHA, GQA with several heads per column group,
# and one group of 16 (one token per tile)
MFMA_PATHS = [(c, F16, d, h, k) for c, d in (("hamming84", 32), ("hamming84", 64), ("hamming84", 128),
                                             ("golay", 128), ("golay_packed", 128))
              for h, k in ((4, 4), (8, 2), (16, 1))]
GENERAL_PATHS = [("hamming84", F32, 100, 6, 2), ("golay", BF16, 20, 2, 2), ("golay_packed", F32, 7, 2, 2)]
CHUNK_PATHS = MFMA_PATHS + GENERAL_PATHS
Q_LENS = [2, 3, 5, 16, 17, 33]


def _pid(p):
    return f"{p[0]}-{_TNAME[p[1]].strip('_')}-d{p[2]}-{p[3]}q{p[4]}kv"


def test_paths_are_what_they_say():
    kinds = {_chunk_select(*p)[0] for p in MFMA_PATHS}
    assert kinds == {"paged_attn_h84_mfma_chunk_kernel<32>", "paged_attn_h84_mfma_chunk_kernel<64>",
                     "paged_attn_h84_mfma_chunk_kernel<128>", "paged_attn_golay_mfma_chunk_kernel<false>",
                     "paged_attn_golay_mfma_chunk_kernel<true>"}
    assert [_chunk_select(*p)[1] for p in MFMA_PATHS[:3]] == [1, 4, 16]  # 16, 4 and 1 tokens per tile
    assert all("split_kernel" in _chunk_select(*p)[0] for p in GENERAL_PATHS)
    # q_len 17 and 33 cross a tile at 16 tokens per tile, 5 at 4, 3 at 2 (a group of 8)
    assert _cdiv(17, 16) == 2 and _cdiv(33, 16) == 3 and _cdiv(5, 4) == 2 and _cdiv(3, 2) == 2


def test_restated_names_are_in_the_kernel_trace():
    """profiles/chunk_attention/kernels.txt is the kernel trace of this file's gpu tests (every
    kvecc attention kernel they launched, by name): each path's restated choice is a kernel that
    ran, and every chunk kernel that ran is some path's restated choice."""
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "chunk_attention",
                        "kernels.txt")
    traced = {ln.strip() for ln in open(path) if ln.strip()}
    want = set()
    for p in CHUNK_PATHS + MASK_PATHS + [c[0] for c in SPLITS] + PROBE_PATHS:
        name = _chunk_select(*p)[0]
        want.add(f"void kvecc::{name.replace('paged_attn_split_kernel', 'paged_attn_split_chunk_kernel')}"
                 .replace(", 0, 0>", ">") + "(kvecc::ChunkArgs)")
    # test_hip_query_layouts' query 8 bytes off alignment: the split kernel of its shape, fp16
    unaligned = _select("hamming84", F32, 128, 8, 2)[0].replace("<float", "<__half")
    assert unaligned == "paged_attn_split_kernel<__half, 2, 2, 16, true, 4, 0, 0>"
    want.add("void kvecc::paged_attn_split_chunk_kernel<__half, 2, 2, 16, true, 4>(kvecc::ChunkArgs)")
    assert want <= traced, sorted(want - traced)
    assert {t for t in traced if "chunk_kernel" in t} == want


# ---- reference and runners ----------------------------------------------------------------------
def _decode_rows(cache, sc, blk, slot, layer, bs, base, d):
    """-> float64 [n, Hkv, d] dequantized rows.  The decode is cpu_ops', the library's own
    codec_math, which tests/test_cpu_backend.py pins to the oracle and the golden vectors
    (test_hamming_random_vs_oracle, test_golay_golden, test_golay_rows_vs_flat); in this file
    only the V probe takes its expectation from the oracle directly."""
    from kvecc import cpu_ops
    nb_, nl_, kvh, _ = cache.shape
    rows = cache.view(nb_, nl_, kvh, bs, -1)[blk, layer, :, slot].contiguous()
    dec = cpu_ops.hamming84_decode(rows)[0] if base == "hamming84" else cpu_ops.golay_decode_rows(rows, d)
    return (dec.double() - 8.0) * sc[blk, layer, :, slot].double().unsqueeze(-1)


def _ref_chunk(q, kc, vc, table, lens, ks, vs, layer, bs, base, mcl=0):
    """float64 causal paged attention, q [B, T, H, d] -> [B, T, H, d]: row t of sequence b over the
    keys j <= lens[b] - T + t, j < cap, whose block is not -1; no such key: the empty value."""
    b_, t_, h_, d = q.shape
    kvh = kc.shape[2]
    cap = table.shape[1] * bs if mcl <= 0 else min(mcl, table.shape[1] * bs)
    out = torch.full((b_, t_, h_, d), EMPTY[base], dtype=torch.float64)
    for b in range(b_):
        n = min(max(int(lens[b]), 0), cap)
        pos = torch.arange(n)
        blk = table[b, pos // bs].long()
        ok = blk >= 0
        if not bool(ok.any()):
            continue
        pos, blk = pos[ok], blk[ok]
        k = _decode_rows(kc, ks, blk, pos % bs, layer, bs, base, d)
        v = _decode_rows(vc, vs, blk, pos % bs, layer, bs, base, d)
        s = torch.einsum("tkgd,nkd->tkgn", q[b].double().view(t_, kvh, h_ // kvh, d), k) / math.sqrt(d)
        limit = (int(lens[b]) - t_ + 1 + torch.arange(t_)).clamp(max=cap)
        seen = pos[None, :] < limit[:, None]  # [T, n]
        live = seen.any(1)
        s = s.masked_fill(~seen[:, None, None, :], -math.inf)[live]
        out[b, live] = torch.einsum("tkgn,nkd->tkgd", torch.softmax(s, dim=-1), v).reshape(-1, h_, d)
    return out


def _attend_chunk(mod, dev, codec, q, kc, vc, table, lens, ks, vs, layer, bs, mcl=0):
    """paged_attention_chunk_into of ops (dev: the GPU) or cpu_ops (dev None) on q as given (its
    strides are kept) -> (float64 on the host, the raw output on the host)."""
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    d = q.shape[-1]
    pk, pv = _for_codec(codec, d, kc, vc)
    if dev is not None:  # the same strides, and the same offset from a 16-byte boundary
        off = (q.data_ptr() % 16) // q.element_size()
        extent = 1 + sum((n - 1) * st for n, st in zip(q.shape, q.stride()))
        qd = torch.as_strided(torch.empty(off + extent, dtype=q.dtype, device=dev), q.shape, q.stride(), off)
        qd.copy_(q)
        assert qd.data_ptr() % 16 == q.data_ptr() % 16
    else:
        qd = q
    out = torch.empty(q.shape, dtype=q.dtype, device=dev)
    mod.paged_attention_chunk_into(qd, t(pk), t(pv), t(table), t(lens), t(ks), t(vs), out, layer, bs,
                                   1 / math.sqrt(d), codec, max_context_len=mcl)
    raw = out.cpu()
    return raw.double(), raw


def _decode_rowwise(mod, dev, codec, q, kc, vc, table, lens, ks, vs, layer, bs, mcl=0):
    """The yardstick: row t through paged_attention_into with context_lens = p_t + 1, clamped at 0."""
    t_ = q.shape[1]
    outs = []
    for t in range(t_):
        lt = (lens - t_ + 1 + t).clamp(min=0).to(torch.int32)
        outs.append(_attend(mod, dev, codec, q[:, t].contiguous(), kc, vc, table, lt, ks, vs, layer, bs, mcl))
    return torch.stack(outs, 1)


def _check_both(mod, dev, codec, dtype, c, mcls=(0,)):
    """The chunk call meets TOL against the float64 reference, and so does the decode entry row by row."""
    base = _base(codec)
    for mcl in mcls:
        ref = _ref_chunk(c["q"], c["kc"], c["vc"], c["table"], c["lens"], c["ks"], c["vs"], c["layer"], c["bs"],
                         base, mcl)
        got, _ = _attend_chunk(mod, dev, codec, c["q"], c["kc"], c["vc"], c["table"], c["lens"], c["ks"], c["vs"],
                               c["layer"], c["bs"], mcl)
        dec = _decode_rowwise(mod, dev, codec, c["q"], c["kc"], c["vc"], c["table"], c["lens"], c["ks"], c["vs"],
                              c["layer"], c["bs"], mcl)
        print(f"mcl {mcl}: chunk max err {_err(got, ref):.3e}, decode rows max err {_err(dec, ref):.3e}")
        empty = (ref == EMPTY[base]).all(-1).all(-1)  # [B, T]: rows without a visible key, every head
        assert torch.equal(got[empty], ref[empty]), mcl  # the empty value is exact
        assert _close(got, ref, dtype), (mcl, _err(got, ref))
        assert _close(dec, ref, dtype), (mcl, _err(dec, ref))
    return ref


def _mods(gpu):
    from kvecc import cpu_ops, ops
    return (cpu_ops, None) if gpu is None else (ops, gpu)


# ---- 1. q_len 1 is the decode entry -------------------------------------------------------------
ONE = FAMILIES + [("hamming84", F16, 64, 2, 2), ("golay", F16, 128, 4, 2)]


def _check_one(mod, dev, family):
    c = _contract(family)
    lens = torch.tensor([100, 93], dtype=torch.int32)
    q = c["q"]  # [2, H, d]
    for mcl in (0, 100):
        dec = _attend(mod, dev, family[0], q, c["kc"], c["vc"], c["table"], lens, c["ks"], c["vs"], 1, 16, mcl)
        _, raw = _attend_chunk(mod, dev, family[0], q.unsqueeze(1), c["kc"], c["vc"], c["table"], lens, c["ks"],
                               c["vs"], 1, 16, mcl)
        assert torch.equal(raw[:, 0].double(), dec), mcl


def test_one_token_families():
    assert "h84_mfma_kernel<64, 1>" in _select(*ONE[4])[0] and "golay_mfma_kernel<2, false>" in _select(*ONE[5])[0]


@pytest.mark.parametrize("family", ONE, ids=_pid)
def test_cpu_one_token_is_the_decode_entry(family):
    _check_one(*_mods(None), family)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ONE, ids=_pid)
def test_hip_one_token_is_the_decode_entry(gpu, family):
    _check_one(*_mods(gpu), family)


# ---- 2. the edge bundle -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bundle(codec, dtype, d, heads, kvh, q_len):
    base = _base(codec)
    lens = torch.tensor([q_len, q_len + 41, 0, q_len - 1, 96 + q_len], dtype=torch.int32)
    nblk = [_cdiv(int(n), BS) for n in lens]
    num_blocks = sum(nblk) + 3
    kc, vc, ks, vs = _caches(base, d, kvh, BS, num_blocks, LAYERS, 0.01, 200 + d, True)
    mid = (1 + torch.randperm(num_blocks - 2, generator=torch.Generator().manual_seed(d))).to(torch.int32).tolist()
    table = torch.full((5, max(nblk) + 2), -1, dtype=torch.int32)
    for b in (0, 1, 3, 4):
        table[b, :nblk[b]] = torch.tensor([mid.pop() for _ in range(nblk[b])], dtype=torch.int32)
    table[2, 0] = mid.pop()  # a block it owns, at length 0
    table[4, 1] = num_blocks - 1  # positions 16..31: the buffer's last row is position 31
    table[4, nblk[4] // 2] = -1  # tokens inside the context are skipped
    table[0 if q_len <= 16 else 3, 0] = -1  # the early rows of that sequence have nothing to see
    g = torch.Generator().manual_seed(q_len)
    q = torch.randn(5, q_len, heads, d, generator=g).to(dtype)
    q[4, :, -1] = q[4, :, -1].abs() * 0.5  # the last head looks at the last row (K there is +7 k_scale)
    return dict(q=q, kc=kc, vc=vc, ks=ks, vs=vs, table=table, lens=lens, layer=LAYER, bs=BS)


def _check_bundle(mod, dev, path, q_len):
    codec, dtype, d, heads, kvh = path
    c = _bundle(codec, dtype, d, heads, kvh, q_len)
    ref = _check_both(mod, dev, codec, dtype, c, (0, int(c["lens"].max())))
    empty = (ref == EMPTY[_base(codec)]).all(-1).all(-1)  # [5, q_len]
    assert bool(empty[2].all()) and bool(empty[3, 0]) and not bool(empty[1].any()) and not bool(empty[4].any())
    if q_len <= 16:
        assert bool(empty[0].all()) and not bool(empty[3, 1:].any())
    else:
        assert bool(empty[3, :17].all()) and not bool(empty[3, 17:].any()) and not bool(empty[0].any())


@pytest.mark.parametrize("q_len", Q_LENS)
@pytest.mark.parametrize("path", CHUNK_PATHS, ids=_pid)
def test_cpu_bundle(path, q_len):
    _check_bundle(*_mods(None), path, q_len)


@pytest.mark.gpu
@pytest.mark.parametrize("q_len", Q_LENS)
@pytest.mark.parametrize("path", CHUNK_PATHS, ids=_pid)
def test_hip_bundle(gpu, path, q_len):
    _check_bundle(*_mods(gpu), path, q_len)


def _check_query_layouts(mod, dev):
    """The [B, H, q_len, D] tensor viewed as [B, q_len, H, D], and a query 8 bytes off a 16-byte
    boundary (the matrix-core kernels' loads need aligned rows: the split kernels take it)."""
    path = ("hamming84", F16, 128, 8, 2)
    c = dict(_bundle(*path, 5))
    q = c["q"]
    c["q"] = q.transpose(1, 2).contiguous().transpose(1, 2)
    assert not c["q"].is_contiguous() and c["q"].stride(3) == 1
    ref = _check_both(mod, dev, path[0], path[1], c)
    buf = torch.zeros(q.numel() + 4, dtype=q.dtype)
    c["q"] = buf[4:].view(q.shape).copy_(q)
    assert c["q"].data_ptr() % 16 == 8
    assert torch.equal(_check_both(mod, dev, path[0], path[1], c), ref)


def test_cpu_query_layouts():
    _check_query_layouts(*_mods(None))


@pytest.mark.gpu
def test_hip_query_layouts(gpu):
    _check_query_layouts(*_mods(gpu))


# ---- 3. the causal limit across splits ----------------------------------------------------------
# batch 1: the launcher picks its finest split of 32 tokens.  (path, q_len, context_lens, table blocks)
MANY_LEN = 32 * K_BLOCK + 8
SPLITS = [
    (("hamming84", F16, 32, 2, 2), 16, 70 + 16, 6),   # keys 71..86 per row, 3 splits
    (("hamming84", F32, 32, 2, 2), 16, 70 + 16, 6),
    (("golay", F16, 128, 2, 1), 16, 70 + 16, 6),
    (("hamming84", F16, 32, 2, 2), 16, 58 + 16, 6),   # keys 59..74: rows 0..5 see nothing of the last split
    (("golay_packed", F16, 128, 2, 2), 16, 58 + 16, 6),
    (("hamming84", F32, 32, 2, 2), 16, 58 + 16, 6),
    (("hamming84", F16, 32, 2, 1), 16, MANY_LEN, _cdiv(MANY_LEN, 16)),  # 257 splits, the block combine;
    (("hamming84", F32, 32, 2, 2), 2, MANY_LEN, _cdiv(MANY_LEN, 16)),   # keys 8185..8200 straddle 8192
]


def test_split_geometry_of_the_split_cases():
    for path, q_len, n, nblk in SPLITS:
        split, nsplit = _chunk_geometry(*path, 1, q_len, nblk * 16)
        assert split == 32 and nsplit == (3 if nblk == 6 else K_BLOCK + 1), (path, split, nsplit)
    assert (58 + 1) <= 64 < (58 + 16) and (MANY_LEN - 16 + 1) <= 8192 < MANY_LEN  # a boundary inside the chunk


@functools.lru_cache(maxsize=None)
def _split_case(path, q_len, n, nblk):
    codec, dtype, d, heads, kvh = path
    kc, vc, ks, vs = _caches(_base(codec), d, kvh, 16, nblk + 1, 1, 0.01, 13, False)
    table = torch.randperm(nblk + 1, generator=torch.Generator().manual_seed(4))[:nblk].to(torch.int32).view(1, nblk)
    q = torch.randn(1, q_len, heads, d, generator=torch.Generator().manual_seed(6)).to(dtype)
    return dict(q=q, kc=kc, vc=vc, ks=ks, vs=vs, table=table.contiguous(), lens=torch.tensor([n], dtype=torch.int32),
                layer=0, bs=16)


def _sid(c):
    return f"{_pid(c[0])}-q{c[1]}-len{c[2]}"


@pytest.mark.parametrize("case", SPLITS, ids=_sid)
def test_cpu_causal_limit_across_splits(case):
    mod, dev = _mods(None)
    _check_both(mod, dev, case[0][0], case[0][1], _split_case(*case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", SPLITS, ids=_sid)
def test_hip_causal_limit_across_splits(gpu, case):
    mod, dev = _mods(gpu)
    _check_both(mod, dev, case[0][0], case[0][1], _split_case(*case))


# ---- 4. mask sensitivity ------------------------------------------------------------------------
MASK_PATHS = FAMILIES + [("golay", F16, 128, 2, 2), ("hamming84", F16, 32, 16, 1)]
MASK_T = 4


def _const_rows(base, d, kvh, n, x):
    """n token rows of one value x = +-4 in every lane (nibble 15 / 1: +-7 scales) -> codewords [n, kvh, words]."""
    from kvecc import cpu_ops
    q, _ = cpu_ops.quantize_rows(torch.full((n, kvh, d), x))
    assert int(q.min()) == int(q.max()) == (15 if x > 0 else 1)
    return cpu_ops.hamming84_encode(q) if base == "hamming84" else cpu_ops.golay_encode_rows(q)


def _set_rows(c, base, d, positions, v=4.0):
    """K rows at `positions` of the one sequence <- +7 scales, V rows +7 (v = 4) or -7 (v = -4)
    scales, at scale 0.35 (clones)."""
    kvh = c["kc"].shape[2]
    pos = torch.as_tensor(positions)
    blk, slot = c["table"][0, pos // 16].long(), pos % 16
    out = dict(c)
    for name in ("kc", "vc"):
        cache = c[name].clone()
        cache.view(cache.shape[0], 1, kvh, 16, -1)[blk, 0, :, slot] = _const_rows(base, d, kvh, len(pos),
                                                                                 4.0 if name == "kc" else v)
        out[name] = cache
    for name in ("ks", "vs"):
        s = c[name].clone()
        s[blk, 0, :, slot] = 0.35
        out[name] = s
    return out


@functools.lru_cache(maxsize=None)
def _mask_case(family, limit):
    """Row 0 sees exactly `limit` keys.  Its own position holds a strong row (K and V +7 scales, the
    largest scale) and the queries are non-negative, so losing that key is far outside the tolerance."""
    codec, dtype, d, heads, kvh = family
    base, n = _base(codec), limit + MASK_T - 1
    nblk = _cdiv(n, 16) + 1
    kc, vc, ks, vs = _caches(base, d, kvh, 16, nblk, 1, 0.01, 17, False)
    q = torch.randn(1, MASK_T, heads, d, generator=torch.Generator().manual_seed(8)).abs().mul(0.5).to(dtype)
    c = dict(q=q, kc=kc, vc=vc, ks=ks, vs=vs, table=torch.arange(nblk, dtype=torch.int32).view(1, nblk),
             lens=torch.tensor([n], dtype=torch.int32), layer=0, bs=16)
    before = _set_rows(c, base, d, [limit - 1])
    # later keys as strong as row 0's own, with the opposite value
    after = _set_rows(before, base, d, list(range(limit, nblk * 16)), -4.0)
    refs = [_ref_chunk(x["q"], x["kc"], x["vc"], x["table"], x["lens"], x["ks"], x["vs"], 0, 16, base)
            for x in (before, after)]
    without = dict(before, lens=before["lens"] - 1)  # row 0 one key short
    lost = _ref_chunk(q, without["kc"], without["vc"], without["table"], without["lens"], without["ks"],
                      without["vs"], 0, 16, base)
    return before, after, refs, lost


def _moved(a, b, dtype, n=10):
    atol, rtol = TOL[dtype]
    return float(((a - b).abs() - n * (atol + rtol * b.abs())).max()) >= 0


def _check_mask(mod, dev, family, limit):
    codec, dtype = family[:2]
    before, after, refs, lost = _mask_case(family, limit)
    # the construction: the rewritten rows move the last row, row 0's own key moves row 0
    assert torch.equal(refs[0][0, 0], refs[1][0, 0]) and _moved(refs[1][0, -1], refs[0][0, -1], dtype)
    assert _moved(lost[0, 0], refs[0][0, 0], dtype)
    outs = []
    for c, ref in zip((before, after), refs):
        got, raw = _attend_chunk(mod, dev, codec, c["q"], c["kc"], c["vc"], c["table"], c["lens"], c["ks"],
                                 c["vs"], 0, 16)
        assert _close(got, ref, dtype), _err(got, ref)
        outs.append(raw)
    assert torch.equal(outs[0][0, 0], outs[1][0, 0])  # nothing past its position reaches row 0
    assert _moved(outs[1][0, -1].double(), outs[0][0, -1].double(), dtype)


@pytest.mark.parametrize("limit", [16, 32, 64])
@pytest.mark.parametrize("family", MASK_PATHS, ids=_pid)
def test_cpu_mask_sensitivity(family, limit):
    _check_mask(*_mods(None), family, limit)


@pytest.mark.gpu
@pytest.mark.parametrize("limit", [16, 32, 64])
@pytest.mark.parametrize("family", MASK_PATHS, ids=_pid)
def test_hip_mask_sensitivity(gpu, family, limit):
    _check_mask(*_mods(gpu), family, limit)


# ---- 5. decode exactness of the chunk kernels ---------------------------------------------------
PROBE_PATHS = [p for p in MFMA_PATHS if (p[3], p[4]) == (8, 2)] + GENERAL_PATHS


def _check_v_probe(mod, dev, path):
    """The V probe of tests/test_attention_decode_probe.py through the chunk entry: q_len 2,
    block_size 1, 256 table columns of which one, at a position <= p_0 = 254, holds a block; V
    scales 2^-(row % 4).  Both query rows are (nibble - 8) * v_scale of the one visible token."""
    codec, dtype, d, heads, kvh = path
    base, group = _base(codec), heads // kvh
    words, nib, _, _, kinds = _rows(base, d)
    rows = len(words)
    nseq = max(rows, COLS)
    blocks = np.arange(nseq) % rows
    w = np.zeros((rows, kvh, 1, words.shape[1]), words.dtype)
    w[:, :, 0] = _per_head(words, kvh)
    vc = _cache(codec, d, w)
    vs = torch.ones(rows, P_LAYERS, kvh, 1)
    vs[:] = (2.0 ** -(torch.arange(rows) % 4)).view(rows, 1, 1, 1)
    table = np.full((nseq, COLS), -1, np.int32)
    table[np.arange(nseq), np.arange(nseq) % (COLS - 1)] = blocks
    q = torch.randn(nseq, 2, heads, d, generator=torch.Generator().manual_seed(d)).to(dtype)
    lens = torch.full((nseq,), COLS, dtype=torch.int32)
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    out = torch.empty(q.shape, dtype=dtype, device=dev)
    mod.paged_attention_chunk_into(t(q), t(vc), t(vc), t(torch.from_numpy(table)), t(lens), t(torch.ones_like(vs)),
                                   t(vs), out, P_LAYER, 1, 0.25, codec)
    assert len(np.unique(kinds[np.unique(blocks)])) == (4096 if base == "golay" else 256)
    scale = vs[blocks, P_LAYER, 0, 0].double().numpy()[:, None, None]
    exp_nib = np.repeat(_per_head(nib, kvh)[blocks], group, axis=1)  # [seq, heads, d], from the oracle
    exp = torch.from_numpy((exp_nib.astype(np.float64) - 8.0) * scale).to(dtype)
    raw = out.cpu()
    for row in (0, 1):
        bad = np.argwhere((raw[:, row] != exp).numpy())
        assert len(bad) == 0, (row, bad[:8].tolist())


@pytest.mark.parametrize("path", PROBE_PATHS, ids=_pid)
def test_cpu_chunk_v_probe(path):
    _oracle()
    _check_v_probe(*_mods(None), path)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PROBE_PATHS, ids=_pid)
def test_hip_chunk_v_probe(gpu, path):
    _check_v_probe(*_mods(gpu), path)


# ---- 6. the Python layer ------------------------------------------------------------------------
def _small(dev=None):
    c = _split_case(SPLITS[0][0], 16, 86, 6)
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    a = dict(query=t(c["q"]), k_cache=t(c["kc"]), v_cache=t(c["vc"]), block_table=t(c["table"]),
             context_lens=t(c["lens"]), k_scales=t(c["ks"]), v_scales=t(c["vs"]))
    a["out"] = torch.full(c["q"].shape, 77.0, dtype=c["q"].dtype, device=dev)
    return a


def _call(mod, a, **over):
    a = dict(a, **over)
    return mod.paged_attention_chunk_into(a["query"], a["k_cache"], a["v_cache"], a["block_table"],
                                          a["context_lens"], a["k_scales"], a["v_scales"], a["out"], 0, 16,
                                          1 / math.sqrt(32), a.get("codec", "hamming84"))


def _check_validation(mod, dev, other=None):
    a = _small(dev)
    q = a["query"]
    bad = [
        dict(query=q.to(torch.float64)),
        dict(k_cache=a["k_cache"].to(torch.int32)),
        dict(block_table=a["block_table"].to(torch.int64)),
        dict(context_lens=a["context_lens"].to(torch.int64)),
        dict(k_scales=a["k_scales"].half()),
        dict(out=a["out"].float()),
        dict(k_cache=a["k_cache"][..., :-16].contiguous(), v_cache=a["v_cache"][..., :-16].contiguous()),
        dict(codec="golay"),  # uint8 caches, Hamming(8,4) row width
        dict(out=torch.full((1, 16, 2, 64), 77.0, dtype=q.dtype, device=dev)[..., :32]),  # not contiguous
        dict(block_table=a["block_table"].repeat(2, 1)),  # wrong batch
        dict(context_lens=a["context_lens"].repeat(2)),
        dict(query=torch.zeros((1, 16, 2, 64), dtype=q.dtype, device=dev)[..., ::2]),  # innermost stride 2
        dict(query=q[:, :, :, :16].expand(1, 16, 2, 16).repeat(1, 1, 1, 2)[:, :, :1].expand(1, 16, 2, 32)),  # head stride 0
    ]
    if other is not None:
        bad.append(dict(v_scales=a["v_scales"].to(other)))  # a mixed-device argument
        bad.append(dict(out=a["out"].to(other)))
    for over in bad:
        with pytest.raises(ValueError):
            _call(mod, a, **over)
        assert bool((a["out"] == 77.0).all()), list(over)  # nothing was launched
    _call(mod, a)
    assert not bool((a["out"] == 77.0).any())


def test_cpu_validation():
    _check_validation(*_mods(None))


@pytest.mark.gpu
def test_hip_validation(gpu):
    _check_validation(*_mods(gpu), other="cpu")


def test_dispatcher_op_on_the_host_is_cpu_ops():
    import kvecc
    from kvecc import cpu_ops, torch_ops
    assert "paged_attention_chunk" in torch_ops.OPS
    a = _small()
    got = torch.ops.kvecc.paged_attention_chunk(a["query"], a["k_cache"], a["v_cache"], a["block_table"],
                                                a["context_lens"], a["k_scales"], a["v_scales"], 0, 16,
                                                1 / math.sqrt(32), "hamming84")
    _call(cpu_ops, a)
    assert torch.equal(got, a["out"])
    assert torch.equal(kvecc.paged_attention_chunk(a["query"], a["k_cache"], a["v_cache"], a["block_table"],
                                                   a["context_lens"], a["k_scales"], a["v_scales"], 0, 16), got)


@pytest.mark.gpu
def test_hip_dispatcher_op_compiles(gpu):
    import kvecc  # noqa: F401
    a = _small(gpu)

    def f(q):
        return torch.ops.kvecc.paged_attention_chunk(q * 1.0, a["k_cache"], a["v_cache"], a["block_table"],
                                                     a["context_lens"], a["k_scales"], a["v_scales"], 0, 16,
                                                     1 / math.sqrt(32), "hamming84") + 0.0

    eager = f(a["query"])
    assert torch.equal(torch.compile(f, fullgraph=True)(a["query"]), eager)
    from kvecc import ops
    assert torch.equal(eager, _call(ops, a))


def _abi_args(a, ws, ws_floats):
    from kvecc import _lib
    q = a["query"]
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    return [p(q), q.stride(0), q.stride(1), q.stride(2), _lib.F16, p(a["k_cache"]), p(a["v_cache"]),
            p(a["block_table"]), p(a["context_lens"]), p(a["k_scales"]), p(a["v_scales"]), p(a["out"]), 1, 16, 2, 2,
            32, a["k_cache"].shape[0], 1, 0, 16, 6, 96, 1 / math.sqrt(32), _lib.CODEC_H84, p(ws), ws_floats, None]


def test_workspace_bounds_every_split_choice():
    from kvecc import _lib
    lib = _lib.load()
    for batch, q_len, heads, mcl in [(1, 16, 2, 96), (1, 2, 2, 8208), (8, 16, 32, 4096), (3, 5, 6, 1000), (2, 1, 8, 300)]:
        n = lib.kvecc_paged_attention_chunk_workspace(batch, q_len, heads, 32, mcl)
        rows = batch * q_len * heads
        if q_len == 1:
            assert n == lib.kvecc_paged_attention_workspace(batch, heads, 32, mcl)
        else:
            assert n == rows * _cdiv(mcl, _choose_split(max(1, rows // 16), mcl)) * 34
    assert lib.kvecc_paged_attention_chunk_workspace(0, 4, 2, 32, 96) == 0


@pytest.mark.gpu
def test_hip_short_workspace_is_einval(gpu):
    from kvecc import _lib
    lib = _lib.load()
    a = _small(gpu)
    need = lib.kvecc_paged_attention_chunk_workspace(1, 16, 2, 32, 96)
    assert need == 32 * 3 * 34
    ws = torch.empty(need, dtype=torch.float32, device=gpu)
    fn = lib.kvecc_paged_attention_chunk
    assert fn(*_abi_args(a, ws, need - 1)) == -1  # KVECC_EINVAL
    assert "workspace" in lib.kvecc_last_error().decode()
    torch.cuda.synchronize()
    assert bool((a["out"] == 77.0).all())
    assert fn(*_abi_args(a, ws, need)) == 0
    torch.cuda.synchronize()
    assert not bool((a["out"] == 77.0).any())
