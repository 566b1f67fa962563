"""Token-by-token generation through a patched model in append mode
(ECCShimConfig(cache_mode="append")): every batch row owns a cache that grows
by what each forward brings.

Model: the random-init LlamaForCausalLM of tests/test_shim_llama.py (2 layers,
4 query / 2 KV heads, head_dim 32, RoPE).  Schedule: batch 2, a 9-token
prefill, then 4 single-token forwards with explicit position_ids; block_size 4,
so the steps cross block boundaries.
"""

import pytest
import torch

from tests.test_shim_llama import LOGIT_ATOL, _llama

PRE, STEPS, BS = 9, 4, 4
TOTAL = PRE + STEPS
HKV, D, LAYERS = 2, 32, 2


def _ids(batch=2):
    return torch.randint(0, 101, (batch, TOTAL), generator=torch.Generator().manual_seed(7))


def _cfg(codec, ber=0.0, backend="cpu", **kw):
    from kvecc.ecc_shim import ECCShimConfig
    storage = "int32"
    if codec == "golay_packed":
        codec, storage = "golay", "packed"
    return ECCShimConfig(codec=codec, ber=ber, inject_errors=ber > 0, seed=42, block_size=BS, backend=backend,
                         golay_storage=storage, **kw)


def _schedule(model, ids, pre=PRE, total=TOTAL):
    """Prefill + single-token steps -> logits [B, total, V], statistics after the prefill."""
    from kvecc.ecc_shim import get_ecc_stats
    b, dev = ids.shape[0], ids.device
    pos = torch.arange(total, device=dev).unsqueeze(0).expand(b, -1)
    outs = [model(ids[:, :pre], position_ids=pos[:, :pre]).logits.float()]
    after_prefill = get_ecc_stats(model)
    for i in range(pre, total):
        outs.append(model(ids[:, i:i + 1], position_ids=pos[:, i:i + 1]).logits.float())
    return torch.cat(outs, dim=1), after_prefill


def _run(model, ids, cfg, num_blocks=16):
    """The schedule on a fresh patched model -> dict of logits, statistics and the manager's state."""
    from kvecc.ecc_shim import get_ecc_stats, patch_model_with_ecc_attention, reset_ecc_cache
    with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=num_blocks):
        reset_ecc_cache(model)
        logits, after_prefill = _schedule(model, ids)
        mgr = model._ecc_block_manager
        b = ids.shape[0]
        return dict(logits=logits, stats=get_ecc_stats(model), after_prefill=after_prefill,
                    lens=[mgr.layer_lens(layer, b) for layer in range(LAYERS)],
                    dev_lens=mgr.ctx_lens[:, :b].cpu().tolist(), overwrite_len=mgr.get_context_len(0),
                    blocks={s: list(bl) for s, bl in mgr.seq_to_blocks.items()},
                    rows=[_layer0_rows(mgr, s) for s in range(b)])


def _layer0_rows(mgr, seq, n=TOTAL):
    """Layer 0's K / V codeword rows and scales of positions [0, n) of a sequence."""
    blocks = mgr.seq_to_blocks.get(seq, [])
    if len(blocks) * mgr.block_size < n:
        return None
    pos = torch.arange(n)
    blk = torch.tensor(blocks)[pos // mgr.block_size].to(mgr.k_cache.device)
    slot = (pos % mgr.block_size).to(mgr.k_cache.device)
    return [mgr.view5(t)[blk, 0, :, slot, :].cpu() for t in (mgr.k_cache, mgr.v_cache, mgr.k_scales, mgr.v_scales)]


@pytest.fixture
def exact_linear(monkeypatch):
    """The model's projections are fp32 GEMMs whose summation order depends on
    the GEMM's row count (a one-row forward takes a GEMV): the K / V of one
    token differ in the last bit between a batch-2 step, a batch-1 step and a
    13-token forward, and so do the row scales absmax / 7 stored from them
    (seen here on the step rows; the codewords agreed).  Where a test compares
    caches of differently shaped forwards bit for bit, the linears run in
    float64 and round to fp32, which takes the GEMM's shape out of a token's
    K / V and leaves the cache write as the only thing compared."""
    linear = torch.nn.functional.linear

    def linear64(x, w, b=None):
        return linear(x.double(), w.double(), None if b is None else b.double()).to(x.dtype)

    monkeypatch.setattr(torch.nn.functional, "linear", linear64)


# ---- 1. construction errors ---------------------------------------------------------
def test_construction_errors():
    from kvecc.ecc_shim import ECCShimConfig
    for bad in (dict(codec="fp16"), dict(codec="fp8"), dict(codec="hamming84", fused=False),
                dict(codec="golay", fused=False)):
        with pytest.raises(ValueError):
            ECCShimConfig(cache_mode="append", **bad)
    with pytest.raises(ValueError):
        ECCShimConfig(cache_mode="ring")
    c = ECCShimConfig(codec="golay", golay_storage="packed", cache_mode="append", decode_stats=True)
    assert c.cache_mode == "append" and c.decode_stats
    d = ECCShimConfig()
    assert d.cache_mode == "overwrite" and d.decode_stats is False


def test_batch_larger_than_the_manager_raises():
    from kvecc.ecc_shim import patch_model_with_ecc_attention
    model, _ = _llama()
    with torch.no_grad(), patch_model_with_ecc_attention(model, _cfg("hamming84", cache_mode="append"), 64):
        many = model._ecc_block_manager.max_seqs + 1
        with pytest.raises(ValueError):
            model(torch.zeros(many, 1, dtype=torch.long))


# ---- 2. growth -------------------------------------------------------------------------
def test_growth_cpu():
    model, _ = _llama()
    r = _run(model, _ids(), _cfg("hamming84", 1e-2, cache_mode="append"))
    assert r["lens"] == [[TOTAL, TOTAL]] * LAYERS and r["dev_lens"] == [[TOTAL, TOTAL]] * LAYERS
    assert len(r["blocks"][0]) == len(r["blocks"][1]) == 4 and not set(r["blocks"][0]) & set(r["blocks"][1])
    assert r["stats"]["injection_count"] == LAYERS * 2 * TOTAL * HKV
    assert r["stats"]["total_values"] == LAYERS * 2 * 2 * TOTAL * HKV * D
    assert r["stats"]["sequences"] == 2 and r["stats"]["allocated_blocks"] == 8
    # the default mode on the same schedule: every forward writes from position 0
    o = _run(model, _ids(), _cfg("hamming84", 1e-2))
    assert o["overwrite_len"] == PRE and list(o["blocks"]) == [0]
    assert o["lens"] == [[0, 0]] * LAYERS
    assert o["stats"]["injection_count"] == r["stats"]["injection_count"]


# ---- 3. per-sequence caches ----------------------------------------------------------------
@pytest.mark.parametrize("codec", ["hamming84", "golay_packed"])
def test_sequences_keep_their_own_caches_cpu(codec, exact_linear):
    model, _ = _llama()
    ids = _ids()
    assert not torch.equal(ids[0], ids[1])
    both = _run(model, ids, _cfg(codec, cache_mode="append"))
    for b in range(2):
        alone = _run(model, ids[b:b + 1], _cfg(codec, cache_mode="append"))
        for got, want in zip(both["rows"][b], alone["rows"][0]):
            assert torch.equal(got, want), b


# ---- 4. append versus one shot -----------------------------------------------------------------
# Measured on the host backend, max |append - one shot| over the 2 x 13 x 101
# logits (largest logit 0.80): 1.0e-7 as run here (float64 linears, see
# exact_linear), 3.0e-7 with the model's own fp32 linears; the same for
# hamming84 and golay, which store the same nibbles at BER 0.  Both are far
# under LOGIT_ATOL / 2, so LOGIT_ATOL is asserted.
@pytest.mark.parametrize("codec", ["hamming84", "golay"])
def test_append_equals_one_shot_cpu(codec, exact_linear):
    from kvecc.ecc_shim import patch_model_with_ecc_attention, reset_ecc_cache
    model, _ = _llama()
    ids = _ids()
    app = _run(model, ids, _cfg(codec, cache_mode="append"))
    for b in range(2):  # the default path keeps one cache: one sequence per forward
        with torch.no_grad(), patch_model_with_ecc_attention(model, _cfg(codec), num_blocks=16):
            reset_ecc_cache(model)
            shot = model(ids[b:b + 1]).logits.float()
            rows = _layer0_rows(model._ecc_block_manager, 0)
        for got, want in zip(app["rows"][b], rows):
            assert torch.equal(got, want), b
        diff = (app["logits"][b] - shot[0]).abs().max().item()
        print(f"append vs one shot, {codec}, sequence {b}: max |diff| = {diff:.3e}")
        assert torch.allclose(app["logits"][b], shot[0], atol=LOGIT_ATOL, rtol=LOGIT_ATOL)


# ---- 5. against the unpatched model ----------------------------------------------------------------
@pytest.mark.parametrize("codec", ["hamming84", "golay", "int4"])
def test_generation_tracks_the_unpatched_model_cpu(codec):
    model, _ = _llama()
    ids = _ids()
    with torch.no_grad():
        ref = model(ids).logits.float()
    out = _run(model, ids, _cfg(codec, cache_mode="append"))["logits"]
    cos = torch.nn.functional.cosine_similarity(out.flatten()[None], ref.flatten()[None]).item()
    assert cos > 0.98, (codec, cos)


# ---- 6. decode statistics --------------------------------------------------------------------------
def test_decode_stats_cpu():
    model, _ = _llama()
    quiet = _run(model, _ids(), _cfg("hamming84", 1e-2, cache_mode="append"))
    assert quiet["after_prefill"]["errors_corrected"] > 0
    for key in ("errors_corrected", "errors_detected"):  # the paged steps keep no statistics
        assert quiet["stats"][key] == quiet["after_prefill"][key]
    counted = _run(model, _ids(), _cfg("hamming84", 1e-2, cache_mode="append", decode_stats=True))
    assert counted["after_prefill"] == quiet["after_prefill"]
    assert counted["stats"]["errors_corrected"] > counted["after_prefill"]["errors_corrected"]


# ---- 7. HIP equals the host backend ------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("codec,kw", [("hamming84", {}), ("hamming84", dict(use_interpolation=True)),
                                      ("golay", {}), ("golay_packed", {}), ("hamming74", {})],
                         ids=["hamming84", "hamming84_interp", "golay", "golay_packed", "hamming74"])
def test_hip_equals_cpu_backend(gpu, codec, kw):
    model, _ = _llama()
    ids = _ids()
    cpu = _run(model, ids, _cfg(codec, 1e-2, "cpu", cache_mode="append", **kw))
    model = model.to(gpu)
    hip = _run(model, ids.to(gpu), _cfg(codec, 1e-2, "hip", cache_mode="append", **kw))
    assert hip["stats"] == cpu["stats"] and hip["lens"] == cpu["lens"] and hip["dev_lens"] == cpu["dev_lens"]
    for t in range(TOTAL):
        assert torch.allclose(hip["logits"][:, t].cpu(), cpu["logits"][:, t], atol=LOGIT_ATOL, rtol=LOGIT_ATOL), t


# ---- 8. free --------------------------------------------------------------------------------------------
def test_free_leaves_the_other_sequence_cpu():
    from kvecc import cpu_ops
    from kvecc.ecc_shim import patch_model_with_ecc_attention, reset_ecc_cache
    model, _ = _llama()
    with torch.no_grad(), patch_model_with_ecc_attention(model, _cfg("hamming84", 1e-2, cache_mode="append"), 16):
        reset_ecc_cache(model)
        _schedule(model, _ids())
        mgr = model._ecc_block_manager

        def read(seq, layer):
            return cpu_ops.shim_read_batch(mgr.k_cache, mgr.v_cache, mgr.k_scales, mgr.v_scales,
                                           mgr.block_table[seq:seq + 1], TOTAL, D, layer, "hamming84",
                                           torch.float32)

        before = [read(1, layer) for layer in range(LAYERS)]
        gone = list(mgr.seq_to_blocks[0])
        mgr.free(0)
        for layer in range(LAYERS):
            for x, y in zip(read(1, layer), before[layer]):
                assert torch.equal(x, y)
        assert 0 not in mgr.seq_to_blocks and set(gone) <= set(mgr.free_blocks) and len(mgr.free_blocks) == 12
        assert mgr.block_table[0].max().item() == -1 and mgr.block_table[1, :4].min().item() >= 0
        assert mgr.ctx_lens[:, 0].tolist() == [0, 0] and mgr.ctx_lens[:, 1].tolist() == [TOTAL, TOTAL]
        assert mgr.layer_lens(0, 2) == [0, TOTAL]
        for t in (mgr.k_cache, mgr.v_cache, mgr.k_scales, mgr.v_scales):
            assert not t[gone].any()
        mgr.reset()
        assert mgr.ctx_lens.sum().item() == 0 and mgr.layer_lens(1, 2) == [0, 0] and len(mgr.free_blocks) == 16


def test_reused_blocks_add_no_stale_statistics_cpu():
    from kvecc.ecc_shim import get_ecc_stats, patch_model_with_ecc_attention, reset_ecc_cache
    model, _ = _llama()
    cfg = _cfg("hamming84", 1e-2, cache_mode="append", decode_stats=True)
    long_ids, short_ids = _ids(1), _ids(2)[1:, :7]

    def short_run():
        model._ecc_backend.reset_stats()
        _schedule(model, short_ids, pre=5, total=7)
        return get_ecc_stats(model), list(model._ecc_block_manager.seq_to_blocks[0])

    with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=16):
        reset_ecc_cache(model)
        _schedule(model, long_ids)
        first = list(model._ecc_block_manager.seq_to_blocks[0])
        model._ecc_block_manager.free(0)
        reused, blocks = short_run()
        assert blocks == first[:2]  # the freed blocks are taken again
    with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=16):
        reset_ecc_cache(model)
        fresh, _ = short_run()
    assert reused == fresh and fresh["errors_corrected"] > 0


# ---- 9. ragged generation ---------------------------------------------------------------------------------
# Batch 2: a 7-token prefill, free(1), a 3-token chunk (masked SDPA, layer lengths 10 / 3), then
# two single-token steps (the paged path, 11 / 4 and 12 / 5).  Row 1 starts a new sequence at
# position 0 in the freed row, with its own tokens and position_ids.
RAG_PRE, RAG_CHUNK, RAG_STEPS = 7, 3, 2
RAG_LENS = [RAG_PRE + RAG_CHUNK + RAG_STEPS, RAG_CHUNK + RAG_STEPS]


def _ragged_ids():
    g = torch.Generator().manual_seed(17)
    return [torch.randint(0, 101, (n,), generator=g) for n in (RAG_LENS[0], RAG_PRE, RAG_LENS[1])]


def _forwards(model, ids, starts, sizes):
    """One forward per size over ids [B, sum(sizes)], row b starting at position starts[b] -> logits."""
    outs, at = [], 0
    for n in sizes:
        pos = torch.stack([s + at + torch.arange(n) for s in starts]).to(ids.device)
        outs.append(model(ids[:, at:at + n], position_ids=pos).logits.float())
        at += n
    return torch.cat(outs, dim=1)


def _state(model, logits, lens):
    from kvecc.ecc_shim import get_ecc_stats
    mgr = model._ecc_block_manager
    b = len(logits)
    return dict(logits=[x.cpu() for x in logits], stats=get_ecc_stats(model),
                lens=[mgr.layer_lens(layer, b) for layer in range(LAYERS)],
                dev_lens=mgr.ctx_lens[:, :b].cpu().tolist(),
                rows=[_layer0_rows(mgr, s, n) for s, n in enumerate(lens)])


def _ragged_run(model, cfg, dev="cpu"):
    from kvecc.ecc_shim import patch_model_with_ecc_attention, reset_ecc_cache
    long, old, new = (t.to(dev) for t in _ragged_ids())
    steps = [RAG_CHUNK] + [1] * RAG_STEPS
    with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=16):
        reset_ecc_cache(model)
        first = _forwards(model, torch.stack([long[:RAG_PRE], old]), [0, 0], [RAG_PRE])
        model._ecc_block_manager.free(1)
        rest = _forwards(model, torch.stack([long[RAG_PRE:], new]), [RAG_PRE, 0], steps)
        return _state(model, [torch.cat([first[0], rest[0]]), rest[1]], RAG_LENS)


def _alone_run(model, cfg, ids, sizes):
    from kvecc.ecc_shim import patch_model_with_ecc_attention, reset_ecc_cache
    with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=16):
        reset_ecc_cache(model)
        return _state(model, [_forwards(model, ids[None], [0], sizes)[0]], [len(ids)])


@pytest.mark.parametrize("codec", ["hamming84", "golay", "hamming74"])
def test_ragged_rows_equal_the_sequences_alone_cpu(codec, exact_linear):
    model, _ = _llama()
    cfg = _cfg(codec, cache_mode="append")
    long, _, new = _ragged_ids()
    steps = [RAG_CHUNK] + [1] * RAG_STEPS
    both = _ragged_run(model, cfg)
    assert both["lens"] == [RAG_LENS] * LAYERS and both["dev_lens"] == [RAG_LENS] * LAYERS
    for b, alone in enumerate((_alone_run(model, cfg, long, [RAG_PRE] + steps), _alone_run(model, cfg, new, steps))):
        assert alone["lens"] == [[RAG_LENS[b]]] * LAYERS
        for got, want in zip(both["rows"][b], alone["rows"][0]):
            assert torch.equal(got, want), b
        diff = (both["logits"][b] - alone["logits"][0]).abs().max().item()
        print(f"ragged vs alone, {codec}, row {b}: max |diff| = {diff:.3e}")
        assert torch.allclose(both["logits"][b], alone["logits"][0], atol=LOGIT_ATOL, rtol=LOGIT_ATOL), b


@pytest.mark.gpu
@pytest.mark.parametrize("codec", ["hamming84", "golay", "golay_packed"])
def test_ragged_hip_equals_cpu_backend(gpu, codec):
    model, _ = _llama()
    cpu = _ragged_run(model, _cfg(codec, 1e-2, "cpu", cache_mode="append"))
    hip = _ragged_run(model.to(gpu), _cfg(codec, 1e-2, "hip", cache_mode="append"), gpu)
    assert hip["stats"] == cpu["stats"] and hip["stats"]["injection_count"] > 0
    assert hip["lens"] == cpu["lens"] == [RAG_LENS] * LAYERS and hip["dev_lens"] == cpu["dev_lens"] == hip["lens"]
    for b in range(2):
        assert torch.allclose(hip["logits"][b], cpu["logits"][b], atol=LOGIT_ATOL, rtol=LOGIT_ATOL), b


# ---- 10. head_dim 64: the decode steps take a GQA kernel (2 query heads per cache head) ---------------------
@pytest.mark.gpu
@pytest.mark.parametrize("codec", ["hamming84", "golay"])
def test_hip_equals_cpu_backend_head_dim_64(gpu, codec):
    model, _ = _llama(hidden_size=256)
    assert model.config.hidden_size // model.config.num_attention_heads == 64
    ids = _ids()
    cpu = _run(model, ids, _cfg(codec, 1e-2, "cpu", cache_mode="append"))
    model = model.to(gpu)
    hip = _run(model, ids.to(gpu), _cfg(codec, 1e-2, "hip", cache_mode="append"))
    assert hip["stats"] == cpu["stats"] and hip["lens"] == cpu["lens"] and hip["dev_lens"] == cpu["dev_lens"]
    for t in range(TOTAL):
        assert torch.allclose(hip["logits"][:, t].cpu(), cpu["logits"][:, t], atol=LOGIT_ATOL, rtol=LOGIT_ATOL), t
