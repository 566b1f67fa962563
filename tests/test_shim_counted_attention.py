"""ECCShimConfig(counted_attention=True): an append-mode Golay model (int32 or packed rows) runs every
forward on the counted paged attention (kvecc_paged_attention_golay_stats) and keeps the decode
statistics that decode_stats=True keeps through the batched counting read + masked SDPA; with
codec="hamming84" the flag is stats_attention=True.

Models, tokens and plans: tests/test_shim_stats_attention.py's (random-init GPT-2 and the GQA LLaMA,
block_size 4, injection at BER 1e-2).  Equal lengths (batch 2): an 8-token prefill, a 5-token chunk
and 4 single-token steps; after every forward errors_corrected / errors_detected / injection_count of
the two configurations are equal exactly and the logits agree to LOGIT_ATOL.  Ragged batch (left-padded
spans through set_ecc_query_spans, every sequence active): the same, and each forward's increment is the
batch-1 counting read of every sequence's n_b rows.
"""

import pytest
import torch

from tests.test_shim_chunk import BS
from tests.test_shim_interp_attention import MODELS, STEPS
from tests.test_shim_llama import LOGIT_ATOL
from tests.test_shim_stats_attention import ALL_ACTIVE, BER, KEYS, _increments, _ragged_run

STORAGE = ["int32", "packed"]
assert STEPS == 4


def _cfg(backend="cpu", storage="int32", codec="golay", **kw):
    from kvecc.ecc_shim import ECCShimConfig
    return ECCShimConfig(codec=codec, ber=BER, inject_errors=True, seed=42, block_size=BS, backend=backend,
                         cache_mode="append", golay_storage=storage, **kw)


def test_flag_errors():
    from kvecc.ecc_shim import ECCShimConfig
    for codec in ("golay", "hamming84"):
        assert ECCShimConfig(codec=codec, cache_mode="append", counted_attention=True).counted_attention is True
    assert ECCShimConfig(codec="golay", cache_mode="append", golay_storage="packed",
                         counted_attention=True).counted_attention is True
    assert ECCShimConfig().counted_attention is False
    for bad in (dict(cache_mode="overwrite"), dict(codec="hamming74"), dict(codec="int4")):
        with pytest.raises(ValueError, match="counted_attention"):
            ECCShimConfig(**{**dict(codec="golay", cache_mode="append", counted_attention=True), **bad})
    with pytest.raises(ValueError, match="stats_attention"):  # the Hamming(8,4) flag keeps refusing Golay
        ECCShimConfig(codec="golay", cache_mode="append", stats_attention=True)


def _equal_run(model, cfg, dev):
    from kvecc.ecc_shim import get_ecc_stats, patch_model_with_ecc_attention, reset_ecc_cache
    g = torch.Generator().manual_seed(17)
    ids = torch.randint(1, 101, (2, 8 + 5 + STEPS), generator=g).to(dev)
    logits, stats = [], []
    with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=32):
        reset_ecc_cache(model)
        at = 0
        for n in [8, 5] + [1] * STEPS:  # the prefill, a chunk, single-token steps
            pos = (at + torch.arange(n)).expand(2, n).to(dev)
            logits.append(model(ids[:, at:at + n], position_ids=pos).logits.float().cpu())
            stats.append({k: get_ecc_stats(model)[k] for k in KEYS})
            at += n
    return torch.cat(logits, dim=1), stats


def _check_equal(name, backend, dev, storage):
    model = MODELS[name]().to(dev)
    on, st_on = _equal_run(model, _cfg(backend, storage, counted_attention=True), dev)
    off, st_off = _equal_run(model, _cfg(backend, storage, decode_stats=True), dev)
    print(f"statistics per forward: {st_on}")
    assert st_on == st_off
    assert st_on[0]["errors_corrected"] > 0
    assert all(b[k] > a[k] for a, b in zip(st_on, st_on[1:]) for k in ("errors_corrected", "injection_count"))
    err = float((on - off).abs().max())
    print(f"counted attention vs decode_stats: max |logit diff| = {err:.3e}")
    assert torch.allclose(on, off, atol=LOGIT_ATOL, rtol=LOGIT_ATOL), err


@pytest.mark.parametrize("storage", STORAGE)
@pytest.mark.parametrize("name", list(MODELS))
def test_equal_lengths_cpu(name, storage):
    _check_equal(name, "cpu", "cpu", storage)


@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGE)
@pytest.mark.parametrize("name", list(MODELS))
def test_equal_lengths_hip(gpu, name, storage):
    _check_equal(name, "hip", gpu, storage)


def _check_ragged(name, backend, dev, storage):
    model = MODELS[name]().to(dev)
    stats, want = _ragged_run(model, _cfg(backend, storage, counted_attention=True), dev, ALL_ACTIVE)
    got = _increments(stats)
    print(f"increments {got} batch-1 sums {want}")
    assert got == want and stats[-1]["errors_corrected"] > 0
    ref, _ = _ragged_run(model, _cfg(backend, storage, decode_stats=True), dev, ALL_ACTIVE, solo=False)
    assert ref == stats  # every sequence active: the rectangular counting read's totals


@pytest.mark.parametrize("storage", STORAGE)
@pytest.mark.parametrize("name", list(MODELS))
def test_ragged_cpu(name, storage):
    _check_ragged(name, "cpu", "cpu", storage)


@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGE)
@pytest.mark.parametrize("name", list(MODELS))
def test_ragged_hip(gpu, name, storage):
    _check_ragged(name, "hip", gpu, storage)


def test_flag_reads_no_dense_cache(monkeypatch):
    """With the flag set no forward materialises dense K / V, whatever the other flags say."""
    from kvecc import cpu_ops
    calls = []
    real = cpu_ops.shim_read_batch
    monkeypatch.setattr(cpu_ops, "shim_read_batch", lambda *a, **k: calls.append(1) or real(*a, **k))
    model = MODELS["gpt2"]()
    _, st = _equal_run(model, _cfg(counted_attention=True, decode_stats=True, chunk_attention=True), "cpu")
    assert calls == [] and st[-1]["errors_corrected"] > 0
    _equal_run(model, _cfg(decode_stats=True), "cpu")
    assert len(calls) == 2 * (2 + STEPS)  # layers x forwards


def _check_hamming84(backend, dev):
    """codec='hamming84': counted_attention is stats_attention, interpolation included."""
    from tests.test_shim_stats_attention import _equal_run as h84_run
    model = MODELS["llama"]().to(dev) if "llama" in MODELS else MODELS[list(MODELS)[-1]]().to(dev)
    for interp in (False, True):
        a = h84_run(model, _cfg(backend, codec="hamming84", use_interpolation=interp, counted_attention=True), dev)
        b = h84_run(model, _cfg(backend, codec="hamming84", use_interpolation=interp, stats_attention=True), dev)
        assert torch.equal(a[0], b[0]) and a[1] == b[1] and a[1][-1]["errors_corrected"] > 0


def test_hamming84_is_stats_attention_cpu():
    _check_hamming84("cpu", "cpu")


@pytest.mark.gpu
def test_hamming84_is_stats_attention_hip(gpu):
    _check_hamming84("hip", gpu)


@pytest.mark.parametrize("storage", STORAGE)
@pytest.mark.parametrize("q_len", [1, 5])
def test_compiled_forward_cpu(q_len, storage):
    """torch.compile: the dispatcher operator is traced, the counts are kept."""
    from kvecc.ecc_shim import patch_model_with_ecc_attention, reset_ecc_cache
    model = MODELS["gpt2"]()
    cfg = _cfg(storage=storage, counted_attention=True)
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
