"""ECCShimConfig(stats_attention=True): an append-mode Hamming(8,4) model runs every forward on
the counted paged attention (kvecc_paged_attention_stats) and keeps the decode statistics that
decode_stats=True keeps through the batched counting read + masked SDPA.

Models: the random-init GPT-2 (2 layers, 4 heads, head_dim 32) and the GQA LLaMA (4 query / 2 KV
heads, RoPE) of tests/test_shim_interp_attention.py, block_size 4, injection at BER 1e-2.

Equal lengths (batch 2): an 8-token prefill, 4 single-token steps and a 3-token verify chunk; after
every forward errors_corrected / errors_detected / injection_count of the two configurations are
equal exactly, and the logits agree to LOGIT_ATOL, with and without use_interpolation (equal
lengths, because of the interpolating kernels' documented last-token clamp).

Ragged batches (prompts of 9 / 6 / 3 tokens, left-padded spans): after every forward the counts
grew by what a batch-1 counting read of each ACTIVE sequence's n_b rows adds, per layer -- with
every sequence active that is also decode_stats=True's total; with one sequence held at count 0
the rectangular read counts it too and the counted kernels do not.
"""

import pytest
import torch

from tests.test_shim_chunk import BS
from tests.test_shim_interp_attention import LENS, MODELS, STEPS, _left_padded, _tokens
from tests.test_shim_llama import LOGIT_ATOL

BER = 1e-2
KEYS = ("errors_corrected", "errors_detected", "injection_count")


def _cfg(backend="cpu", interp=False, **kw):
    from kvecc.ecc_shim import ECCShimConfig
    return ECCShimConfig(codec="hamming84", ber=BER, inject_errors=True, seed=42, block_size=BS, backend=backend,
                         cache_mode="append", use_interpolation=interp, **kw)


# ---- 8. construction ---------------------------------------------------------------------------
def test_flag_errors():
    from kvecc.ecc_shim import ECCShimConfig
    ok = dict(codec="hamming84", cache_mode="append", stats_attention=True)
    assert ECCShimConfig(**ok).stats_attention is True
    assert ECCShimConfig(**ok, use_interpolation=True).stats_attention is True
    assert ECCShimConfig().stats_attention is False
    assert ECCShimConfig(codec="hamming84", cache_mode="append").stats_attention is False
    for bad in (dict(cache_mode="overwrite"), dict(codec="golay"), dict(codec="hamming74"), dict(codec="int4")):
        with pytest.raises(ValueError, match="stats_attention"):
            ECCShimConfig(**{**ok, **bad})


# ---- 9. flag on against decode_stats=True ----------------------------------------------------------
def _equal_run(model, cfg, dev):
    from kvecc.ecc_shim import get_ecc_stats, patch_model_with_ecc_attention, reset_ecc_cache
    g = torch.Generator().manual_seed(17)
    ids = torch.randint(1, 101, (2, 8 + STEPS + 3), generator=g).to(dev)
    logits, stats = [], []
    with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=32):
        reset_ecc_cache(model)
        at = 0
        for n in [8] + [1] * STEPS + [3]:  # the prefill, single-token steps, a verify chunk
            pos = (at + torch.arange(n)).expand(2, n).to(dev)
            logits.append(model(ids[:, at:at + n], position_ids=pos).logits.float().cpu())
            stats.append({k: get_ecc_stats(model)[k] for k in KEYS})
            at += n
    return torch.cat(logits, dim=1), stats


def _check_equal(name, backend, dev, interp):
    model = MODELS[name]().to(dev)
    on, st_on = _equal_run(model, _cfg(backend, interp, stats_attention=True), dev)
    off, st_off = _equal_run(model, _cfg(backend, interp, decode_stats=True), dev)
    print(f"statistics per forward: {st_on}")
    assert st_on == st_off
    assert st_on[0]["errors_corrected"] > 0 and st_on[-1]["errors_detected"] > 0
    assert all(b[k] > a[k] for a, b in zip(st_on, st_on[1:]) for k in ("errors_corrected", "injection_count"))
    err = float((on - off).abs().max())
    print(f"stats attention vs decode_stats: max |logit diff| = {err:.3e}")
    assert torch.allclose(on, off, atol=LOGIT_ATOL, rtol=LOGIT_ATOL), err
    return on, st_on


@pytest.mark.parametrize("interp", [False, True], ids=["plain", "interp"])
@pytest.mark.parametrize("name", list(MODELS))
def test_equal_lengths_cpu(name, interp):
    _check_equal(name, "cpu", "cpu", interp)


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [False, True], ids=["plain", "interp"])
@pytest.mark.parametrize("name", list(MODELS))
def test_equal_lengths_hip(gpu, name, interp):
    _check_equal(name, "hip", gpu, interp)


def test_flag_takes_precedence_and_reads_no_dense_cache(monkeypatch):
    """With the flag set no forward materialises dense K / V, whatever the other flags say."""
    from kvecc import cpu_ops
    calls = []
    real = cpu_ops.shim_read_batch
    monkeypatch.setattr(cpu_ops, "shim_read_batch", lambda *a, **k: calls.append(1) or real(*a, **k))
    model = MODELS["gpt2"]()
    _, st = _equal_run(model, _cfg(stats_attention=True, decode_stats=True, chunk_attention=True), "cpu")
    assert calls == [] and st[-1]["errors_corrected"] > 0
    _, st2 = _equal_run(model, _cfg(interp=True, stats_attention=True, interp_attention=True), "cpu")
    assert calls == [] and st2 == st  # the same cache bytes, counted alike by both kernel families
    _equal_run(model, _cfg(decode_stats=True), "cpu")
    assert len(calls) == 2 * (2 + STEPS)  # layers x forwards


# ---- 10 / 11. ragged batches -------------------------------------------------------------------------
def _solo_counts(model, active):
    """What a batch-1 counting read of each active sequence's n_b rows adds, over all layers."""
    be, mgr = model._ecc_backend, model._ecc_block_manager
    ops = be.codec_backend
    st = ops.new_stats(mgr.k_cache.device)
    for layer in range(mgr.num_layers):
        for b, n in enumerate(mgr.layer_lens(layer, len(active))):
            if active[b] and n > 0:
                ops.shim_read_batch(mgr.k_cache, mgr.v_cache, mgr.k_scales, mgr.v_scales,
                                    mgr.block_table[b:b + 1].contiguous(), n, mgr.head_dim, layer, mgr.shim_codec,
                                    torch.float32, stats=st)
    return ops.read_stats(st)


def _ragged_run(model, cfg, dev, plan, solo=True):
    """plan: per forward, the valid token count of each sequence (left-padded spans).
    -> (per forward get_ecc_stats, per forward the batch-1 sum of the active sequences)."""
    from kvecc.ecc_shim import (get_ecc_stats, patch_model_with_ecc_attention, reset_ecc_cache,
                                set_ecc_query_spans)
    toks = _tokens()
    stats, want = [], []
    with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=32):
        reset_ecc_cache(model)
        lens = [0, 0, 0]
        for counts in plan:
            q_max = max(counts)
            rows = [t[at:at + n] for t, at, n in zip(toks, lens, counts)]
            ids, firsts = _left_padded(rows, q_max)
            firsts = [f if n else 0 for f, n in zip(firsts, counts)]
            pos = torch.stack([(at + torch.arange(q_max) - f).clamp(min=0) for at, f in zip(lens, firsts)])
            set_ecc_query_spans(model, counts, firsts)
            out = model(ids.to(dev), position_ids=pos.to(dev)).logits.float().cpu()
            assert bool(out.isfinite().all())
            lens = [at + n for at, n in zip(lens, counts)]
            stats.append({k: get_ecc_stats(model)[k] for k in KEYS})
            if solo:
                want.append(_solo_counts(model, [n > 0 for n in counts]))
    return stats, want


def _increments(stats):
    prev = dict.fromkeys(KEYS, 0)
    out = []
    for s in stats:
        out.append([s["errors_corrected"] - prev["errors_corrected"], s["errors_detected"] - prev["errors_detected"]])
        prev = s
    return out


ALL_ACTIVE = [LENS, [3, 2, 1], [1, 1, 1], [1, 1, 1]]
ONE_IDLE = [LENS, [3, 0, 1], [1, 0, 1], [1, 2, 1]]  # sequence 1 is held for two forwards, then resumes


def _check_ragged(name, backend, dev, interp, plan):
    model = MODELS[name]().to(dev)
    stats, want = _ragged_run(model, _cfg(backend, interp, stats_attention=True), dev, plan)
    got = _increments(stats)
    print(f"increments {got} batch-1 sums {want}")
    assert got == want
    assert stats[-1]["errors_corrected"] > 0 and stats[-1]["errors_detected"] > 0
    ref, _ = _ragged_run(model, _cfg(backend, interp, decode_stats=True), dev, plan, solo=False)
    assert [s["injection_count"] for s in ref] == [s["injection_count"] for s in stats]
    if all(all(c) for c in plan):
        assert ref == stats  # every sequence active: the rectangular counting read's totals
    else:  # the rectangular read also counts the held sequence, the counted kernels do not read it
        assert ref[-1]["errors_corrected"] > stats[-1]["errors_corrected"]


@pytest.mark.parametrize("interp", [False, True], ids=["plain", "interp"])
@pytest.mark.parametrize("name", list(MODELS))
def test_ragged_all_active_cpu(name, interp):
    _check_ragged(name, "cpu", "cpu", interp, ALL_ACTIVE)


@pytest.mark.parametrize("name", list(MODELS))
def test_ragged_one_inactive_cpu(name):
    _check_ragged(name, "cpu", "cpu", False, ONE_IDLE)


@pytest.mark.gpu
@pytest.mark.parametrize("plan", [ALL_ACTIVE, ONE_IDLE], ids=["all_active", "one_inactive"])
@pytest.mark.parametrize("name", list(MODELS))
def test_ragged_hip(gpu, name, plan):
    _check_ragged(name, "hip", gpu, plan is ALL_ACTIVE, plan)


# ---- 12. reset, and the scrub's own counters ----------------------------------------------------------
def _check_reset(backend, dev):
    from kvecc.ecc_shim import (get_ecc_stats, patch_model_with_ecc_attention, reset_ecc_cache, scrub_ecc_cache)
    model = MODELS["gpt2"]().to(dev)
    ids = torch.randint(1, 101, (2, 8), generator=torch.Generator().manual_seed(3)).to(dev)
    with torch.no_grad(), patch_model_with_ecc_attention(model, _cfg(backend, stats_attention=True), num_blocks=32):
        reset_ecc_cache(model)
        model(ids)
        first = {k: get_ecc_stats(model)[k] for k in KEYS}
        assert first["errors_corrected"] > 0
        scrub = scrub_ecc_cache(model)
        assert scrub["corrected"] > 0
        assert {k: get_ecc_stats(model)[k] for k in KEYS} == first  # the scrub's counters are its own
        assert int(model._ecc_backend.scrub_totals()[0]) == scrub["corrected"]
        reset_ecc_cache(model)
        st = get_ecc_stats(model)
        assert st["errors_corrected"] == 0 and st["errors_detected"] == 0
        assert not bool(model._ecc_backend.scrub_totals().any())


def test_reset_cpu():
    _check_reset("cpu", "cpu")


@pytest.mark.gpu
def test_reset_hip(gpu):
    _check_reset("hip", gpu)


# ---- torch.compile: the dispatcher operator is traced, the counts are kept ---------------------------
@pytest.mark.parametrize("q_len", [1, 5])
def test_compiled_forward_cpu(q_len):
    from kvecc.ecc_shim import patch_model_with_ecc_attention, reset_ecc_cache
    model = MODELS["gpt2"]()
    cfg = _cfg(stats_attention=True)
    h = torch.randn(2, 12 + q_len, 128, generator=torch.Generator().manual_seed(1))
    outs = []
    for compiled in (False, True):
        with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=32):
            reset_ecc_cache(model)
            attn = model.transformer.h[0].attn
            attn.forward(h[:, :12].contiguous())
            fwd = attn.forward
            if compiled:
                torch._dynamo.reset()
                fwd = torch.compile(attn.forward, fullgraph=True, backend="aot_eager")
            out = fwd(h[:, 12:].contiguous())[0]
            outs.append((out.clone(), model._ecc_backend._stats.clone()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1]) and bool(outs[1][1].any())
