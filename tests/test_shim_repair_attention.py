"""ECCShimConfig(repair_attention=True): an append-mode Hamming(8,4) model runs every forward on
the repairing paged attention (kvecc_paged_attention_repair): stats_attention=True's logits and
counts, and every layer's resident cache repaired in place as part of its attention launch.

Models: the random-init GPT-2 (2 layers, 4 heads, head_dim 32) and the GQA LLaMA (4 query / 2 KV
heads, RoPE) of tests/test_shim_interp_attention.py, block_size 4, written at ber = 0.

Clean model: flag on against stats_attention=True through a prefill, a chunk, single-token steps
and a ragged batch with one sequence held -- equal logits and get_ecc_stats, nothing repaired, the
caches byte-identical.

Accumulation experiment: model A (repair_attention) ages its cache and runs one single-token
forward per round; model B (stats_attention) ages with the same seed, runs the same forward and
then calls scrub_ecc_cache.  After every round the logits are equal, the K / V caches of A and B
are byte-identical, the decode statistics are equal and A's get_ecc_repaired equals B's summed
scrub "rewritten" -- with and without use_interpolation.
"""

import pytest
import torch

from tests.test_generation_append import _forwards
from tests.test_shim_chunk import BS
from tests.test_shim_interp_attention import LENS, MODELS, _left_padded, _tokens

KEYS = ("errors_corrected", "errors_detected", "injection_count", "total_values", "allocated_blocks")
AGE_BER, AGE_SEED, ROUNDS, PREFILL = 1e-2, 7, 4, 9


def _cfg(backend="cpu", interp=False, **kw):
    from kvecc.ecc_shim import ECCShimConfig
    return ECCShimConfig(codec="hamming84", ber=0.0, inject_errors=False, seed=42, block_size=BS, backend=backend,
                         cache_mode="append", use_interpolation=interp, **kw)


@pytest.fixture(params=["cpu", pytest.param("hip", marks=pytest.mark.gpu)])
def be(request):
    """(backend name, device) of the host twin / the HIP kernels."""
    if request.param == "cpu":
        return "cpu", torch.device("cpu")
    return "hip", request.getfixturevalue("gpu")


def _patched(name, cfg, dev):
    from kvecc.ecc_shim import patch_model_with_ecc_attention
    model = MODELS[name]().to(dev)
    return model, patch_model_with_ecc_attention(model, cfg, num_blocks=32)


# ---- construction and reset ------------------------------------------------------------------------
def test_flag_errors():
    from kvecc.ecc_shim import ECCShimConfig
    ok = dict(codec="hamming84", cache_mode="append", repair_attention=True)
    assert ECCShimConfig(**ok).repair_attention is True
    assert ECCShimConfig(**ok, use_interpolation=True).repair_attention is True
    assert ECCShimConfig().repair_attention is False
    assert ECCShimConfig(codec="hamming84", cache_mode="append").repair_attention is False
    for bad in (dict(cache_mode="overwrite"), dict(codec="golay"), dict(codec="hamming74"), dict(codec="int4")):
        with pytest.raises(ValueError, match="repair_attention"):
            ECCShimConfig(**{**ok, **bad})


def test_unpatched_model_raises():
    from kvecc.ecc_shim import get_ecc_repaired
    with pytest.raises(ValueError, match="not patched"):
        get_ecc_repaired(MODELS["gpt2"]())


def test_reset_clears_the_count(be):
    from kvecc.ecc_shim import age_ecc_cache, get_ecc_repaired, get_ecc_stats, reset_ecc_cache
    backend, dev = be
    ids = torch.randint(1, 101, (2, PREFILL + 1), generator=torch.Generator().manual_seed(3)).to(dev)
    model, ctx = _patched("gpt2", _cfg(backend, repair_attention=True), dev)
    with torch.no_grad(), ctx:
        reset_ecc_cache(model)
        keys = set(get_ecc_stats(model))
        _forwards(model, ids[:, :PREFILL], [0, 0], [PREFILL])
        assert get_ecc_repaired(model) == 0
        age_ecc_cache(model, AGE_BER, AGE_SEED)
        _forwards(model, ids[:, PREFILL:], [PREFILL, PREFILL], [1])
        assert get_ecc_repaired(model) > 0 and get_ecc_stats(model)["errors_corrected"] > 0
        assert set(get_ecc_stats(model)) == keys and "repaired" not in keys  # get_ecc_stats keeps its keys
        reset_ecc_cache(model)
        st = get_ecc_stats(model)
        assert get_ecc_repaired(model) == 0 and st["errors_corrected"] == 0 and st["errors_detected"] == 0
    other, ctx = _patched("gpt2", _cfg(backend, stats_attention=True), dev)
    with torch.no_grad(), ctx:
        assert get_ecc_repaired(other) == 0  # without the flag there is nothing to report


# ---- the clean model --------------------------------------------------------------------------------
def _clean_run(name, cfg, dev):
    """Prefill 8, a 3-token chunk, two single-token steps, then a ragged batch-3 generation with
    sequence 1 held for a forward -> (logits, get_ecc_stats after each forward, repaired, caches)."""
    from kvecc.ecc_shim import get_ecc_repaired, get_ecc_stats, reset_ecc_cache, set_ecc_query_spans
    model, ctx = _patched(name, cfg, dev)
    logits, stats = [], []
    with torch.no_grad(), ctx:
        reset_ecc_cache(model)
        ids = torch.randint(1, 101, (2, 13), generator=torch.Generator().manual_seed(17)).to(dev)
        at = 0
        for n in (8, 3, 1, 1):
            logits.append(_forwards(model, ids[:, at:at + n], [at, at], [n]).cpu())
            stats.append({k: get_ecc_stats(model)[k] for k in KEYS})
            at += n
        reset_ecc_cache(model)
        toks, lens = _tokens(), [0, 0, 0]
        for counts in (LENS, [3, 0, 1], [1, 2, 1]):
            q_max = max(counts)
            rows = [t[a:a + n] for t, a, n in zip(toks, lens, counts)]
            tok, firsts = _left_padded(rows, q_max)
            firsts = [f if n else 0 for f, n in zip(firsts, counts)]
            pos = torch.stack([(a + torch.arange(q_max) - f).clamp(min=0) for a, f in zip(lens, firsts)])
            set_ecc_query_spans(model, counts, firsts)
            logits.append(model(tok.to(dev), position_ids=pos.to(dev)).logits.float().cpu())
            stats.append({k: get_ecc_stats(model)[k] for k in KEYS})
            lens = [a + n for a, n in zip(lens, counts)]
        mgr = model._ecc_block_manager
        return logits, stats, get_ecc_repaired(model), (mgr.k_cache.cpu().clone(), mgr.v_cache.cpu().clone())


@pytest.mark.parametrize("interp", [False, True], ids=["plain", "interp"])
@pytest.mark.parametrize("name", list(MODELS))
def test_clean_model_equals_stats_attention(be, name, interp):
    backend, dev = be
    on, st_on, repaired, cache_on = _clean_run(name, _cfg(backend, interp, repair_attention=True), dev)
    off, st_off, none, cache_off = _clean_run(name, _cfg(backend, interp, stats_attention=True), dev)
    assert all(torch.equal(a, b) for a, b in zip(on, off))
    assert st_on == st_off and st_on[-1]["errors_corrected"] == 0 and st_on[-1]["total_values"] == st_off[-1]["total_values"]
    assert repaired == 0 and none == 0
    assert all(torch.equal(a, b) for a, b in zip(cache_on, cache_off))  # a clean cache is not written


# ---- the accumulation experiment ----------------------------------------------------------------------
def _accumulate(name, backend, dev, interp):
    from kvecc.ecc_shim import (age_ecc_cache, get_ecc_repaired, get_ecc_stats, reset_ecc_cache, scrub_ecc_cache)
    ids = torch.randint(1, 101, (2, PREFILL + ROUNDS), generator=torch.Generator().manual_seed(23)).to(dev)
    a, ctx_a = _patched(name, _cfg(backend, interp, repair_attention=True), dev)
    b, ctx_b = _patched(name, _cfg(backend, interp, stats_attention=True), dev)
    with torch.no_grad(), ctx_a, ctx_b:
        for m in (a, b):
            reset_ecc_cache(m)
            _forwards(m, ids[:, :PREFILL], [0, 0], [PREFILL])
        rewritten, detected = 0, 0
        for r in range(ROUNDS):
            at = PREFILL + r
            age_ecc_cache(a, AGE_BER, AGE_SEED + r)
            la = _forwards(a, ids[:, at:at + 1], [at, at], [1]).cpu()
            age_ecc_cache(b, AGE_BER, AGE_SEED + r)
            lb = _forwards(b, ids[:, at:at + 1], [at, at], [1]).cpu()
            got = scrub_ecc_cache(b)
            rewritten += got["rewritten"]
            detected += got["detected"]
            sa, sb = get_ecc_stats(a), get_ecc_stats(b)
            print(f"round {r}: repaired {get_ecc_repaired(a)}, scrub rewritten so far {rewritten}, "
                  f"corrected {sa['errors_corrected']}, detected {sa['errors_detected']}")
            assert torch.equal(la, lb)
            ma, mb = a._ecc_block_manager, b._ecc_block_manager
            assert torch.equal(ma.k_cache, mb.k_cache) and torch.equal(ma.v_cache, mb.v_cache)
            assert torch.equal(ma.k_scales, mb.k_scales) and torch.equal(ma.v_scales, mb.v_scales)
            assert sa["errors_corrected"] == sb["errors_corrected"] and sa["errors_detected"] == sb["errors_detected"]
            assert get_ecc_repaired(a) == rewritten
            assert get_ecc_repaired(b) == 0
        assert rewritten > 0 and sa["errors_corrected"] > 0 and detected > 0  # singles to repair, doubles that stay


@pytest.mark.parametrize("interp", [False, True], ids=["plain", "interp"])
@pytest.mark.parametrize("name", list(MODELS))
def test_accumulation_experiment(be, name, interp):
    backend, dev = be
    _accumulate(name, backend, dev, interp)


# ---- torch.compile: the dispatcher operator is traced, the caches and the counts move as in eager -------
def _check_compiled(backend, dev, q_len):
    from kvecc.ecc_shim import age_ecc_cache, get_ecc_repaired, reset_ecc_cache
    h = torch.randn(2, 12 + q_len, 128, generator=torch.Generator().manual_seed(1)).to(dev)
    outs = []
    for compiled in (False, True):
        model, ctx = _patched("gpt2", _cfg(backend, repair_attention=True), dev)  # (the same seeded weights)
        with torch.no_grad(), ctx:
            reset_ecc_cache(model)
            attn = model.transformer.h[0].attn
            attn.forward(h[:, :12].contiguous())
            age_ecc_cache(model, AGE_BER, AGE_SEED)
            fwd = attn.forward
            if compiled:
                torch._dynamo.reset()
                fwd = torch.compile(attn.forward, fullgraph=True, backend="aot_eager")
            out = fwd(h[:, 12:].contiguous())[0]
            mgr = model._ecc_block_manager
            outs.append((out.clone(), model._ecc_backend._stats.clone(), mgr.k_cache.clone(), mgr.v_cache.clone(),
                         get_ecc_repaired(model)))
    assert all(torch.equal(x, y) for x, y in zip(outs[0][:4], outs[1][:4]))
    assert outs[0][4] == outs[1][4] > 0


@pytest.mark.parametrize("q_len", [1, 5])
def test_compiled_forward_cpu(q_len):
    _check_compiled("cpu", torch.device("cpu"), q_len)


@pytest.mark.gpu
def test_compiled_forward_hip(gpu):
    _check_compiled("hip", gpu, 1)
