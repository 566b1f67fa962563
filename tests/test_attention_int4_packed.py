"""Packed INT4 caches (codec "int4_packed", KVECC_CODEC_INT4_PACKED: int4's nibbles two per byte,
rows of head_dim / 2 bytes) through the append writers and the plain paged-attention entries, on the
host twin and on the GPU.

Append: bit for bit `lo | hi << 4` of what codec "int4" writes from the same input, the same
scales, and poison everywhere else.  Attention: against float64 numpy attention over the nibbles
unpacked from the packed cache, (nib - 8) * scale, causal by absolute position, within the suite's
TOL (tests/test_attention_paths.py) -- the bound the byte INT4 path meets against the same reference.
"""

import math

import numpy as np
import pytest
import torch

from tests.test_attention_paths import BF16, F16, F32, TOL

BS, LAYERS, LAYER, POISON = 16, 2, 1, 0xA5
DEVICES = ["cpu", pytest.param("hip", marks=pytest.mark.gpu)]


@pytest.fixture
def be(request):
    """(backend module, device) of a DEVICES entry."""
    if request.param == "cpu":
        from kvecc import cpu_ops
        return cpu_ops, torch.device("cpu")
    from kvecc import ops
    return ops, request.getfixturevalue("gpu")


# ---- append ----------------------------------------------------------------------------------------
def _pool(codec, d, hkv, blocks, dev):
    row = BS * (d // 2 if codec == "int4_packed" else d)
    return ([torch.full((blocks, LAYERS, hkv, row), POISON, dtype=torch.uint8, device=dev) for _ in range(2)] +
            [torch.full((blocks, LAYERS, hkv, BS), -123.0, device=dev) for _ in range(2)])


@pytest.mark.parametrize("be", DEVICES, indirect=True)
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("dtype", [F32, F16, BF16])
@pytest.mark.parametrize("d", [8, 64, 128, 256])
def test_append_packs_the_byte_caches_nibbles(be, d, dtype, ragged):
    mod, dev = be
    batch, q_len, hkv, blocks = 3, 5, 2, 12
    g = torch.Generator().manual_seed(d + ragged)
    k, v = (torch.randn(batch, q_len, hkv, d, generator=g).to(dtype).to(dev) for _ in range(2))
    table = torch.full((batch, 4), -1, dtype=torch.int32)
    table[:, :3] = (1 + torch.randperm(blocks - 1, generator=g))[:9].view(3, 3).int()  # block 0 unnamed
    table, start = table.to(dev), torch.tensor([0, 13, 30], dtype=torch.int32, device=dev)  # 13 + 5 straddles 16
    pools = {}
    for codec in ("int4", "int4_packed"):
        pools[codec] = p = _pool(codec, d, hkv, blocks, dev)
        args = (k, v, *p, table, start, LAYERS, BS, hkv, d, LAYER, codec, 4, False, 0.0, 7)
        if ragged:  # spans of 0, 1 and 3 tokens, left-padded
            spans = mod.query_spans([0, 1, 3], [0, 4, 2], q_max=q_len, device=dev)
            mod.shim_append_ragged_tensors(*args, spans, scale_rule="div7")
        else:
            mod.shim_append_tensors(*args, scale_rule="div7")
    for side in range(2):
        byte, packed = pools["int4"][side].cpu(), pools["int4_packed"][side].cpu()
        lo, hi = byte[..., 0::2], byte[..., 1::2]
        assert bool(((lo <= 15) == (hi <= 15)).all()) and int((lo <= 15).sum()) > 0
        assert torch.equal(packed, torch.where(lo <= 15, lo | hi << 4, torch.tensor(POISON, dtype=torch.uint8)))
        assert torch.equal(pools["int4"][2 + side].cpu(), pools["int4_packed"][2 + side].cpu())


# ---- attention -------------------------------------------------------------------------------------
# (dtype, head_dim, query heads, cache heads): the matrix-core kernels, then the general path
SHAPES = [(F16, 64, 2, 2), (F16, 64, 8, 2), (F16, 128, 2, 2), (F16, 128, 8, 2),
          (F32, 40, 4, 2), (BF16, 256, 2, 2), (F16, 128, 6, 2)]
LENS = [86, 51]  # one sequence ends mid-block, one split is partial; the third holds the chunk alone


def _case(d, hkv, lens, dev, seed=0):
    """A random packed pool whose tables are a permutation with -1 past each length; block 0 unnamed."""
    g = torch.Generator().manual_seed(seed)
    blocks, max_blocks = 16, 7
    kc, vc = (torch.randint(0, 256, (blocks, LAYERS, hkv, BS * d // 2), generator=g, dtype=torch.uint8)
              for _ in range(2))
    ks, vs = (torch.rand(blocks, LAYERS, hkv, BS, generator=g) * 0.2 + 0.01 for _ in range(2))
    perm = (1 + torch.randperm(blocks - 1, generator=g)).int()
    table = torch.full((len(lens), max_blocks), -1, dtype=torch.int32)
    at = 0
    for b, n in enumerate(lens):
        nb = -(-n // BS)
        table[b, :nb] = perm[at:at + nb]
        at += nb
    return [t.to(dev) for t in (kc, vc, table, torch.tensor(lens, dtype=torch.int32), ks, vs)]


def _reference(q, kc, vc, table, lens, ks, vs, spans):
    """float64 attention over the unpacked nibbles; a row without a key (padding) is the empty value -8."""
    q, kc, vc, table, lens, ks, vs = (t.cpu().double().numpy() if t.is_floating_point() else t.cpu().numpy()
                                      for t in (q, kc, vc, table, lens, ks, vs))
    batch, q_len, heads, d = q.shape
    group = heads // kc.shape[2]
    out = np.full(q.shape, -8.0)
    for b in range(batch):
        first, count = spans[b]
        n = int(lens[b])
        if n == 0 or count == 0:
            continue
        slots = [(int(table[b, j // BS]), j % BS) for j in range(n)]
        for hk in range(kc.shape[2]):
            def rows(c, s):
                raw = np.stack([c[blk, LAYER, hk, i * d // 2:(i + 1) * d // 2] for blk, i in slots])
                nib = np.stack([raw & 15, raw >> 4], axis=-1).reshape(n, d).astype(np.float64)
                return (nib - 8.0) * np.array([s[blk, LAYER, hk, i] for blk, i in slots])[:, None]
            kk, vv = rows(kc, ks), rows(vc, vs)
            for t in range(first, min(first + count, q_len)):
                lim = n - count + (t - first) + 1
                for h in range(hk * group, (hk + 1) * group):
                    s = kk[:lim] @ q[b, t, h] / math.sqrt(d)
                    p = np.exp(s - s.max())
                    out[b, t, h] = p @ vv[:lim] / p.sum()
    return out


def _attend(q, case, spans=None):
    from kvecc import ops  # (host tensors go to the host twin)
    kc, vc, table, lens, ks, vs = case
    sp = None if spans is None else ops.query_spans([c for _, c in spans], [f for f, _ in spans], device=q.device)
    return ops.paged_attention_chunk(q, kc, vc, table, lens, ks, vs, LAYER, BS, codec="int4_packed", q_spans=sp)


def _check(out, ref, dtype):
    atol, rtol = TOL[dtype]
    err = np.abs(out.cpu().double().numpy() - ref)
    print(f"max |out - ref| = {err.max():.3e}")
    assert bool((err <= atol + rtol * np.abs(ref)).all())


@pytest.mark.parametrize("be", DEVICES, indirect=True)
@pytest.mark.parametrize("q_len", [1, 5, 17])
@pytest.mark.parametrize("dtype,d,heads,hkv", SHAPES)
def test_attention_matches_float64_over_the_unpacked_nibbles(be, dtype, d, heads, hkv, q_len):
    dev = be[1]
    case = _case(d, hkv, [q_len] + LENS, dev)
    q = torch.randn(3, q_len, heads, d, generator=torch.Generator().manual_seed(q_len)).to(dtype).to(dev)
    _check(_attend(q, case), _reference(q, *case, [(0, q_len)] * 3), dtype)


@pytest.mark.parametrize("be", DEVICES, indirect=True)
@pytest.mark.parametrize("dtype,d,heads,hkv", [SHAPES[3], SHAPES[4]])
def test_ragged_spans_and_rows_the_call_must_not_read(be, dtype, d, heads, hkv):
    dev = be[1]
    spans, lens = [(0, 0), (2, 3), (0, 5)], [0] + LENS
    case = _case(d, hkv, lens, dev, seed=1)
    q = torch.randn(3, 5, heads, d, generator=torch.Generator().manual_seed(9)).to(dtype).to(dev)
    out = _attend(q, case, spans)
    _check(out, _reference(q, *case, spans), dtype)
    # everything but the named rows of the attended layer: 0xFF bytes and NaN scales, the same bits out
    kc, vc, _, _, ks, vs = case
    keep, table = torch.zeros(ks.shape, dtype=torch.bool), case[2].cpu()
    for b, n in enumerate(lens):
        for j in range(n):
            keep[int(table[b, j // BS]), LAYER, :, j % BS] = True
    keep = keep.to(dev)
    wide = keep.repeat_interleave(d // 2, dim=-1)
    poisoned = [torch.where(wide, kc, torch.full_like(kc, 0xFF)), torch.where(wide, vc, torch.full_like(vc, 0xFF)),
                case[2], case[3], torch.where(keep, ks, torch.full_like(ks, math.nan)),
                torch.where(keep, vs, torch.full_like(vs, math.nan))]
    assert torch.equal(_attend(q, poisoned, spans), out)
    # the uniform decode step over the same pool (no spans, q_len 1)
    assert torch.equal(_attend(q[:, :1].contiguous(), poisoned), _attend(q[:, :1].contiguous(), case))


# ---- validation: an error before any launch, the output untouched ------------------------------------
def _attn_call(d, **kw):
    from kvecc import cpu_ops
    case = _case(max(d // 8 * 8, 8), 2, [5] + LENS, "cpu")
    case[0], case[1] = (torch.zeros(16, LAYERS, 2, BS * d // 2, dtype=torch.uint8) for _ in range(2))
    out = torch.full((3, 1, 2, d), 77.0)
    with pytest.raises(ValueError):
        cpu_ops.paged_attention_chunk_into(torch.zeros(3, 1, 2, d), *case[:6], out, LAYER, BS, 1.0, "int4_packed", **kw)
    assert bool((out == 77.0).all())


@pytest.mark.parametrize("d,kw", [(12, {}), (260, {}), (64, {"window": 4}), (64, {"interp": True}),
                                  (64, {"stats": torch.zeros(4, dtype=torch.int64)}),
                                  (64, {"stats": torch.zeros(4, dtype=torch.int64), "repair": True})])
def test_attention_refuses_what_the_layout_does_not_serve(d, kw):
    _attn_call(d, **kw)


def test_the_other_entries_refuse_the_codec():
    from kvecc import cpu_ops, ops
    d, hkv = 64, 2
    kc, vc, ks, vs = _pool("int4_packed", d, hkv, 4, "cpu")
    table, lens = torch.zeros(1, 2, dtype=torch.int32), torch.ones(1, dtype=torch.int32)
    x = torch.zeros(1, 1, hkv, d)
    with pytest.raises(ValueError, match="inject"):
        cpu_ops.shim_append_tensors(x, x, kc, vc, ks, vs, table, lens, LAYERS, BS, hkv, d, 0, "int4_packed", 4, True,
                                    1e-2, 7)
    with pytest.raises(ValueError):
        ops.cache_scrub(kc, vc, table, lens, head_dim=d, block_size=BS, num_layers=LAYERS, codec="int4_packed")
    with pytest.raises(ValueError):
        cpu_ops.shim_read_batch(kc, vc, ks, vs, table, 1, d, 0, "int4_packed", torch.float32)
    with pytest.raises(ValueError):
        cpu_ops.shim_write_tensors(x, x, kc, vc, ks, vs, table[0], LAYERS, BS, hkv, d, 0, "int4_packed", 4, False,
                                   0.0, 7)
    assert bool((kc == POISON).all()) and bool((ks == -123.0).all())
    with pytest.raises(ValueError, match="int4, hamming74, hamming84, golay or golay_packed"):
        cpu_ops.paged_attention_chunk_into(x, kc, vc, table, lens, ks, vs, x.clone(), 0, BS, 1.0, "int5")


def test_the_c_entries_refuse_the_codec_themselves():
    from kvecc import _lib, ops
    case, q, out = _case(64, 2, [5] + LENS, "cpu"), torch.zeros(3, 1, 2, 64), torch.full((3, 1, 2, 64), 77.0)
    st = torch.zeros(4, dtype=torch.int64)
    for entry, sp, window in (("window", None, (4, 0)), ("window", None, (0, 0)), ("interp", None, None),
                              ("stats", st.data_ptr(), None), ("repair", st.data_ptr(), None)):
        args = ops._chunk_entry_args(entry, q, *case, out, LAYER, BS, 1.0, "int4_packed", 0, None, False, sp, window)
        with pytest.raises(_lib.KveccError):
            _lib.call("kvecc_cpu_paged_attention_" + entry, *args, 1)
    assert bool((out == 77.0).all()) and int(st.sum()) == 0


# ---- the shim ----------------------------------------------------------------------------------------
def _shim_run(model, backend, dev, storage):
    from kvecc.ecc_shim import ECCShimConfig
    from tests.test_shim_chunk import BS as SHIM_BS, _run
    return _run(model, ECCShimConfig(codec="int4", block_size=SHIM_BS, backend=backend, cache_mode="append",
                                     kernel_attention=True, int4_storage=storage), dev)


@pytest.mark.parametrize("be", DEVICES, indirect=True)
@pytest.mark.parametrize("name", ["gpt2", "llama"])
def test_shim_packed_storage_generates_the_byte_storages_logits(be, name):
    from tests.test_shim_chunk import MODELS, _agree
    _, dev = be
    model = MODELS[name]().to(dev)
    backend = "cpu" if dev.type == "cpu" else "hip"
    packed, byte = _shim_run(model, backend, dev, "packed"), _shim_run(model, backend, dev, "byte")
    _agree(packed, byte, caches=False)
    for p, b in zip(packed["caches"][:2], byte["caches"][:2]):
        assert p.dtype == b.dtype == torch.uint8 and 2 * p.numel() == b.numel()  # the pools are half the bytes
        assert torch.equal(p, b[..., 0::2] | b[..., 1::2] << 4)
    for p, b in zip(packed["caches"][2:], byte["caches"][2:]):
        assert torch.equal(p, b)


def test_shim_config_names_the_failed_condition():
    from kvecc.ecc_shim import ECCShimConfig, SimpleBlockManager
    ok = dict(codec="int4", cache_mode="append", kernel_attention=True, int4_storage="packed")
    assert ECCShimConfig(**ok).int4_storage == "packed" and ECCShimConfig().int4_storage == "byte"
    for bad, word in ((dict(codec="hamming74"), "codec"), (dict(cache_mode="overwrite", kernel_attention=False), "append"),
                      (dict(kernel_attention=False), "kernel_attention"), (dict(attention_window=8), "attention_window"),
                      (dict(int4_storage="nibble"), "int4_storage")):
        with pytest.raises(ValueError, match=word):
            ECCShimConfig(**{**ok, **bad})
    with pytest.raises(ValueError, match="head_dim"):
        SimpleBlockManager(4, BS, 1, 1, 12, device="cpu", codec="int4", int4_storage="packed")
    mgr = SimpleBlockManager(4, BS, 1, 1, 64, device="cpu", codec="int4", int4_storage="packed")
    assert mgr.shim_codec == "int4_packed" and mgr.k_cache.shape[-1] == BS * 32
    assert not SimpleBlockManager.fits_buffer_kernels(1 << 20, 1, 8, 16, 128, "int4", int4_storage="packed")
