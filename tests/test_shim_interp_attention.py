"""ECCShimConfig(interp_attention=True): an append-mode model with Hamming(8,4) and
interpolation runs every forward on the interpolating paged attention
(kvecc_paged_attention_interp) instead of the batched interpolating read + masked SDPA.

Models: the random-init GPT-2 (2 layers, 4 heads, head_dim 32) and the GQA LLaMA (4 query / 2 KV
heads, RoPE) of tests/test_shim_chunk.py, block_size 4.

Equal lengths (batch 2): an 8-token prefill written with injection at BER 1e-2, the resident
cache aged at BER 2e-2 (age_ecc_cache: a codeword is a double with probability about 28 p^2, 1 %),
then 4 single-token steps.  Flag on and off must agree to LOGIT_ATOL, the append-mode model
tests' tolerance: at equal lengths the batched read is exactly what the kernel interpolates.

Unequal lengths (batch 3, prompts of 9 / 6 / 3 tokens, left-padded spans): a ragged prefill, a
ragged chunk of 3 / 2 / 1 tokens, then 4 single-token steps, the cache aged after the prefill and
after the chunk.  The batched read interpolates a shorter sequence's last token against the zero
row past its length, so each sequence is compared with its own batch-1 run (flag off: one
sequence is the longest of its batch).  The batch-1 run sees the same errors because the aged
blocks of the batch run are copied into its cache after each ageing (_transplant).
"""

import pytest
import torch

from tests.test_shim_chunk import BS, _gpt2
from tests.test_shim_llama import LOGIT_ATOL, _llama

MODELS = {"gpt2": _gpt2, "llama": lambda: _llama()[0]}
STEPS, AGE_BER = 4, 2e-2


def _cfg(interp_attention, backend="cpu", ber=0.0, **kw):
    from kvecc.ecc_shim import ECCShimConfig
    return ECCShimConfig(codec="hamming84", ber=ber, inject_errors=ber > 0, seed=42, block_size=BS, backend=backend,
                         cache_mode="append", use_interpolation=True, interp_attention=interp_attention, **kw)


def test_flag_errors():
    from kvecc.ecc_shim import ECCShimConfig
    ok = dict(codec="hamming84", cache_mode="append", use_interpolation=True, interp_attention=True)
    assert ECCShimConfig(**ok).interp_attention is True
    assert ECCShimConfig().interp_attention is False
    assert ECCShimConfig(codec="hamming84", cache_mode="append", use_interpolation=True).interp_attention is False
    for bad in (dict(cache_mode="overwrite"), dict(codec="golay"), dict(codec="hamming74"), dict(codec="int4"),
                dict(use_interpolation=False)):
        with pytest.raises(ValueError):
            ECCShimConfig(**{**ok, **bad})


# ---- equal lengths: flag on against flag off ---------------------------------------------------
def _equal_run(model, cfg, dev):
    from kvecc.ecc_shim import (age_ecc_cache, get_ecc_stats, patch_model_with_ecc_attention, reset_ecc_cache,
                                scrub_ecc_cache)
    g = torch.Generator().manual_seed(17)
    ids = torch.randint(1, 101, (2, 8 + STEPS), generator=g).to(dev)
    logits, stats = [], []
    with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=32):
        reset_ecc_cache(model)
        pos = torch.arange(8).expand(2, 8).to(dev)
        logits.append(model(ids[:, :8], position_ids=pos).logits.float().cpu())
        stats.append(get_ecc_stats(model))
        age_ecc_cache(model, AGE_BER, 99)
        for s in range(STEPS):
            pos = torch.full((2, 1), 8 + s).to(dev)
            logits.append(model(ids[:, 8 + s:9 + s], position_ids=pos).logits.float().cpu())
            stats.append(get_ecc_stats(model))
        scrub = scrub_ecc_cache(model)
    return torch.cat(logits, dim=1), stats, scrub


def _check_equal(name, backend, dev):
    model = MODELS[name]().to(dev)
    on, st_on, scrub = _equal_run(model, _cfg(True, backend, 1e-2), dev)
    off, st_off, _ = _equal_run(model, _cfg(False, backend, 1e-2), dev)
    assert scrub["detected"] > 0 and scrub["corrected"] > 0  # the aged cache held doubles
    err = float((on - off).abs().max())
    print(f"interp attention on vs off: max |logit diff| = {err:.3e}")
    assert torch.allclose(on, off, atol=LOGIT_ATOL, rtol=LOGIT_ATOL), err
    # the fast path keeps no decode statistics; the counting path does; injection is counted alike
    for st in st_on:
        assert st["errors_corrected"] == 0 and st["errors_detected"] == 0
    assert st_off[0]["errors_corrected"] > 0 and st_off[-1]["errors_detected"] > 0
    assert [s["injection_count"] for s in st_on] == [s["injection_count"] for s in st_off]
    return on


@pytest.mark.parametrize("name", list(MODELS))
def test_equal_lengths_cpu(name):
    _check_equal(name, "cpu", "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_equal_lengths_hip(gpu, name):
    on = _check_equal(name, "hip", gpu)
    twin, _, _ = _equal_run(MODELS[name](), _cfg(True, "cpu", 1e-2), "cpu")
    # the host twin's projections are other GEMMs: the K / V it stores may differ in a last bit
    assert torch.allclose(on, twin, atol=LOGIT_ATOL, rtol=LOGIT_ATOL), float((on - twin).abs().max())


def test_dense_read_is_never_called(monkeypatch):
    """With the flag set no forward materialises dense K / V; without it every forward does."""
    from kvecc import cpu_ops
    calls = []
    real = cpu_ops.shim_read_batch
    monkeypatch.setattr(cpu_ops, "shim_read_batch", lambda *a, **k: calls.append(1) or real(*a, **k))
    model = _gpt2()
    _equal_run(model, _cfg(True), "cpu")
    assert calls == []
    _equal_run(model, _cfg(False), "cpu")
    assert len(calls) == 2 * (1 + STEPS)  # layers x forwards
    calls.clear()
    _equal_run(model, _cfg(True, decode_stats=True), "cpu")  # decode_stats keeps the counting path
    assert len(calls) == 2 * (1 + STEPS)


# ---- unequal lengths: each sequence against its own batch-1 run -----------------------------------
LENS, CHUNK = [9, 6, 3], [3, 2, 1]


def _tokens():
    g = torch.Generator().manual_seed(31)
    return [torch.randint(1, 101, (n + c + STEPS,), generator=g) for n, c in zip(LENS, CHUNK)]


def _left_padded(rows, q_max):
    ids = torch.zeros(len(rows), q_max, dtype=torch.long)
    firsts = [q_max - len(r) for r in rows]
    for b, r in enumerate(rows):
        ids[b, firsts[b]:] = r
    return ids, firsts


def _snapshot(mgr, batch):
    return dict(k=mgr.k_cache.clone(), v=mgr.v_cache.clone(),
                blocks=[list(mgr.seq_to_blocks.get(b, [])) for b in range(batch)])


def _transplant(snap, b, mgr):
    """Sequence b's blocks of the batch run, as aged, into the batch-1 run's cache."""
    mine = list(mgr.seq_to_blocks[0])
    assert len(mine) == len(snap["blocks"][b])
    for dst, src in zip(mine, snap["blocks"][b]):
        mgr.k_cache[dst] = snap["k"][src]
        mgr.v_cache[dst] = snap["v"][src]


def _ragged_run(model, cfg, dev):
    """-> per sequence [chunk + steps, V] logits of the tokens after the prefill, the snapshots, scrub counts."""
    from kvecc.ecc_shim import (age_ecc_cache, get_ecc_stats, patch_model_with_ecc_attention, reset_ecc_cache,
                                scrub_ecc_cache, set_ecc_query_spans)
    toks = _tokens()
    snaps, outs = [], [[] for _ in LENS]
    with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=32):
        reset_ecc_cache(model)
        mgr = model._ecc_block_manager
        lens = [0, 0, 0]
        for counts in (LENS, CHUNK):
            rows = [t[at:at + n] for t, at, n in zip(toks, lens, counts)]
            ids, firsts = _left_padded(rows, max(counts))
            pos = torch.stack([(at + torch.arange(max(counts)) - f).clamp(min=0) for at, f in zip(lens, firsts)])
            set_ecc_query_spans(model, counts, firsts)
            out = model(ids.to(dev), position_ids=pos.to(dev)).logits.float().cpu()
            assert bool(out.isfinite().all())
            if counts is CHUNK:
                for b, f in enumerate(firsts):
                    outs[b].append(out[b, f:])
            lens = [at + n for at, n in zip(lens, counts)]
            age_ecc_cache(model, AGE_BER, 7 + len(snaps))
            snaps.append(_snapshot(mgr, 3))
        set_ecc_query_spans(model, [1, 1, 1])
        for s in range(STEPS):
            tok = torch.stack([t[at:at + 1] for t, at in zip(toks, lens)])
            out = model(tok.to(dev), position_ids=torch.tensor(lens).view(3, 1).to(dev)).logits.float().cpu()
            for b in range(3):
                outs[b].append(out[b])
            lens = [at + 1 for at in lens]
        stats = get_ecc_stats(model)
        scrub = scrub_ecc_cache(model)
    return [torch.cat(o) for o in outs], snaps, stats, scrub


def _solo_run(model, cfg, dev, b, snaps):
    from kvecc.ecc_shim import patch_model_with_ecc_attention, reset_ecc_cache
    t = _tokens()[b]
    outs, at = [], 0
    with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=32):
        reset_ecc_cache(model)
        mgr = model._ecc_block_manager
        for i, n in enumerate((LENS[b], CHUNK[b])):
            pos = (at + torch.arange(n)).unsqueeze(0).to(dev)
            out = model(t[at:at + n].unsqueeze(0).to(dev), position_ids=pos).logits.float().cpu()
            if i == 1:
                outs.append(out[0])
            at += n
            _transplant(snaps[i], b, mgr)
        for s in range(STEPS):
            outs.append(model(t[at:at + 1].unsqueeze(0).to(dev),
                              position_ids=torch.tensor([[at]]).to(dev)).logits.float().cpu()[0])
            at += 1
    return torch.cat(outs)


def _check_ragged(name, backend, dev):
    model = MODELS[name]().to(dev)
    got, snaps, stats, scrub = _ragged_run(model, _cfg(True, backend), dev)
    assert scrub["detected"] > 0  # the aged cache held doubles
    assert stats["errors_corrected"] == 0 and stats["errors_detected"] == 0
    for b in range(3):
        want = _solo_run(model, _cfg(False, backend), dev, b, snaps)
        err = float((got[b] - want).abs().max())
        print(f"sequence {b}: max |logit diff| against its batch-1 run = {err:.3e}")
        assert got[b].shape == want.shape == (CHUNK[b] + STEPS, want.shape[-1])
        assert torch.allclose(got[b], want, atol=LOGIT_ATOL, rtol=LOGIT_ATOL), (b, err)


@pytest.mark.parametrize("name", list(MODELS))
def test_unequal_lengths_cpu(name):
    _check_ragged(name, "cpu", "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_unequal_lengths_hip(gpu, name):
    _check_ragged(name, "hip", gpu)


# ---- torch.compile ------------------------------------------------------------------------------
def _compiled_forward(device, q_len):
    """One attention forward, compiled against eager: the dispatcher operator is traced."""
    from kvecc.ecc_shim import age_ecc_cache, patch_model_with_ecc_attention, reset_ecc_cache
    model = _gpt2().to(device)
    cfg = _cfg(True, "hip" if device.type == "cuda" else "cpu")
    h = torch.randn(2, 12 + q_len, 128, generator=torch.Generator().manual_seed(1)).to(device)
    outs = []
    for compiled in (False, True):
        with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=32):
            reset_ecc_cache(model)
            attn = model.transformer.h[0].attn
            attn.forward(h[:, :12].contiguous())
            age_ecc_cache(model, AGE_BER, 5)
            fwd = attn.forward
            if compiled:
                torch._dynamo.reset()
                fwd = torch.compile(attn.forward, fullgraph=True, backend="aot_eager")
            out = fwd(h[:, 12:].contiguous())[0]
            outs.append((out.clone(), model._ecc_backend._stats.clone()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert not bool(outs[1][1].any())  # no decode statistics


@pytest.mark.parametrize("q_len", [1, 5])
def test_compiled_forward_cpu(q_len):
    _compiled_forward(torch.device("cpu"), q_len)


@pytest.mark.gpu
def test_compiled_forward_hip(gpu):
    _compiled_forward(gpu, 5)
