"""ECCShimConfig(chunk_attention=True): the forwards of more than one token of an
append-mode model run on the chunked causal paged attention kernel instead of
the batched read + masked SDPA.

Models: the random-init GPT-2 of tests/test_torch_ops.py (2 layers, 4 heads,
head_dim 32) and the LLaMA of tests/test_shim_llama.py (4 query / 2 KV heads,
RoPE).  Schedule, batch 2, block_size 4: a 7-token forward, free(1), then
forwards of 19, 5, 5, 1, 1, 1 tokens with row 0 continuing at position 7 and
row 1 starting a new sequence at position 0 -- so the 19-token forward is a
prefill for row 1 and a chunk for row 0, and the two rows' contexts differ in
every forward (26 / 19, 31 / 24, 36 / 29, then 37..39 / 30..32).  BER 1e-2 with
injection.

Flag on and off must agree: logits to LOGIT_ATOL (the append-mode model tests'
tolerance), and layer 0's caches bit for bit.  Layer 0's K / V come from the
embeddings alone.  A later layer's come through the attention outputs, which
the two paths sum in different orders, so its caches cannot be bit-identical
in general; they are bounded instead (_later_layers):

- row scales absmax / 7 to 1e-5 relative.  The two attention outputs differ by
  fp32 rounding of sums of a few dozen terms, eps 6e-8 each, and pass through
  one block's fp32 linears and norms: 1e-5 is two orders above that;
- stored nibbles: both runs inject the same bit flips (same seeds, same
  positions) and the codes are linear, so the XOR of the two caches is the
  encoding of (nibble_on ^ nibble_off) with the flips cancelled, and decoding
  it gives that XOR exactly.  A value x / scale in [-7, 7] perturbed by 1e-5
  relative moves by at most 7e-5, so it rounds to another nibble only within
  7e-5 of a half-integer: for a smooth density 1.4e-4 of the values.  At most
  1e-3 of a later layer's written nibbles may differ (the estimate times 7, for
  the small sample of 4.5e3 to 9e3 values per cache and the density's shape), and each
  differing pair must be one quantisation step apart, whose XOR is 1, 3, 7 or 15.
"""

import pytest
import torch

from tests.test_attention_paths import _unpack_golay
from tests.test_generation_append import _forwards
from tests.test_shim_llama import LOGIT_ATOL, _llama

BS, FIRST, SIZES, D = 4, 7, [19, 5, 5, 1, 1, 1], 32  # D: both models' head_dim
LENS = [FIRST + sum(SIZES), sum(SIZES)]
CODECS = ["hamming84", "golay", "golay_packed"]


def _gpt2():
    from transformers import GPT2Config, GPT2LMHeadModel
    torch.manual_seed(0)
    return GPT2LMHeadModel(GPT2Config(n_layer=2, n_head=4, n_embd=128, n_positions=128, vocab_size=101)).eval()


MODELS = {"gpt2": _gpt2, "llama": lambda: _llama()[0]}


def _cfg(codec, chunk, backend="cpu", **kw):
    from kvecc.ecc_shim import ECCShimConfig
    storage = "packed" if codec == "golay_packed" else "int32"
    return ECCShimConfig(codec=codec.replace("_packed", ""), ber=1e-2, inject_errors=True, seed=42, block_size=BS,
                         backend=backend, golay_storage=storage, cache_mode="append", chunk_attention=chunk, **kw)


def _ids():
    g = torch.Generator().manual_seed(23)
    return [torch.randint(0, 101, (n,), generator=g) for n in (LENS[0], FIRST, LENS[1])]


def _run(model, cfg, dev="cpu"):
    """The schedule on a fresh patched model -> logits per row, statistics after every forward, caches."""
    from kvecc.ecc_shim import get_ecc_stats, patch_model_with_ecc_attention, reset_ecc_cache
    long, old, new = (t.to(dev) for t in _ids())
    stats = []
    with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=32):
        reset_ecc_cache(model)
        first = _forwards(model, torch.stack([long[:FIRST], old]), [0, 0], [FIRST])
        stats.append(get_ecc_stats(model))
        mgr = model._ecc_block_manager
        mgr.free(1)
        rest = []
        at = 0
        for n in SIZES:  # one forward at a time, to read the statistics between them
            pos = torch.stack([s + at + torch.arange(n) for s in (FIRST, 0)]).to(dev)
            ids = torch.stack([long[FIRST + at:FIRST + at + n], new[at:at + n]])
            rest.append(model(ids, position_ids=pos).logits.float())
            stats.append(get_ecc_stats(model))
            at += n
        rest = torch.cat(rest, dim=1)
        return dict(logits=[torch.cat([first[0], rest[0]]).cpu(), rest[1].cpu()], stats=stats,
                    lens=[mgr.layer_lens(layer, 2) for layer in range(mgr.num_layers)],
                    caches=[t.cpu().clone() for t in (mgr.k_cache, mgr.v_cache, mgr.k_scales, mgr.v_scales)])


def _nibble_xor(x, y, codec):
    """K or V caches of two runs with the same injected flips -> nibble_x ^ nibble_y per stored value
    (the codes are linear: the XOR of the codewords is the codeword of the XOR, flips cancelled)."""
    from kvecc import cpu_ops
    if codec == "golay_packed":
        x, y = _unpack_golay(x, D), _unpack_golay(y, D)
    w = (x ^ y).contiguous()
    if codec == "hamming84":
        return cpu_ops.hamming84_decode(w.view(-1))[0]
    return cpu_ops.golay_decode_rows(w.view(-1, (D + 2) // 3), D)


def _later_layers(on, off, codec):
    """The bounds of the module docstring on the layers after the first."""
    for x, y in zip(on["caches"][2:], off["caches"][2:]):
        assert torch.allclose(x[:, 1:], y[:, 1:], rtol=1e-5, atol=0)
    written = 2 * sum(LENS) * on["caches"][2].shape[2] * D  # K and V values of one layer
    for x, y in zip(on["caches"][:2], off["caches"][:2]):
        for layer in range(1, x.shape[1]):
            d = _nibble_xor(x[:, layer], y[:, layer], codec)
            n = int((d != 0).sum())
            print(f"layer {layer}: {n} of {written // 2} stored nibbles differ")
            assert n <= 1e-3 * (written // 2), n
            assert bool(torch.isin(d, torch.tensor([0, 1, 3, 7, 15], dtype=d.dtype)).all())


def _agree(on, off, caches=True, codec=None):
    assert on["lens"] == off["lens"] == [LENS] * 2
    for b in range(2):
        diff = (on["logits"][b] - off["logits"][b]).abs().max().item()
        print(f"chunk attention on vs off, row {b}: max |logit diff| = {diff:.3e}")
        assert torch.allclose(on["logits"][b], off["logits"][b], atol=LOGIT_ATOL, rtol=LOGIT_ATOL), b
    if not caches:
        return
    for x, y in zip(on["caches"], off["caches"]):
        assert torch.equal(x[:, 0], y[:, 0])  # layer 0, bit for bit
    _later_layers(on, off, codec)


def _check_stats(on, off):
    """No decode statistics from the chunk forwards (nor from the paged decode steps); injection counted."""
    for st in on["stats"]:
        assert st["errors_corrected"] == 0 and st["errors_detected"] == 0
    assert off["stats"][0]["errors_corrected"] > 0
    assert off["stats"][3]["errors_corrected"] > off["stats"][0]["errors_corrected"]
    counts = [st["injection_count"] for st in on["stats"]]
    assert counts == [st["injection_count"] for st in off["stats"]]
    assert all(b > a for a, b in zip(counts, counts[1:])) and counts[0] > 0


def test_flag_needs_append_mode():
    from kvecc.ecc_shim import ECCShimConfig
    with pytest.raises(ValueError):
        ECCShimConfig(codec="hamming84", chunk_attention=True)
    with pytest.raises(ValueError):
        ECCShimConfig(codec="golay", cache_mode="overwrite", chunk_attention=True)
    assert ECCShimConfig().chunk_attention is False
    assert ECCShimConfig(cache_mode="append").chunk_attention is False
    assert ECCShimConfig(cache_mode="append", chunk_attention=True).chunk_attention is True


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("name", list(MODELS))
def test_chunk_attention_equals_the_default_path_cpu(name, codec):
    model = MODELS[name]()
    on, off = _run(model, _cfg(codec, True)), _run(model, _cfg(codec, False))
    _agree(on, off, codec=codec)
    _check_stats(on, off)


def test_flag_is_ignored_where_the_decode_step_is(monkeypatch):
    """Interpolation and decode_stats keep the counting path, as for single-token steps."""
    from kvecc import cpu_ops
    calls = []
    real = cpu_ops.paged_attention_chunk_into
    monkeypatch.setattr(cpu_ops, "paged_attention_chunk_into", lambda *a, **k: calls.append(1) or real(*a, **k))
    model = _gpt2()
    for kw in (dict(use_interpolation=True), dict(decode_stats=True)):
        r = _run(model, _cfg("hamming84", True, **kw))
        assert r["stats"][1]["errors_corrected"] > 0
    assert calls == []
    _run(model, _cfg("hamming84", True))
    assert len(calls) == 2 * 4  # layers x forwards of more than one token


@pytest.mark.gpu
@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("name", list(MODELS))
def test_chunk_attention_hip(gpu, name, codec):
    model = MODELS[name]()
    cpu_on = _run(model, _cfg(codec, True))
    model = model.to(gpu)
    on, off = _run(model, _cfg(codec, True, "hip"), gpu), _run(model, _cfg(codec, False, "hip"), gpu)
    _agree(on, off, codec=codec)
    _check_stats(on, off)
    # and the host twin (its projections are other GEMMs: the K / V it stores differ in the last bit)
    _agree(on, cpu_on, caches=False)
    assert on["stats"] == cpu_on["stats"]


def _compiled_forward(device, codec):
    """One attention forward of 24 tokens, compiled against eager: the dispatcher op is traced."""
    from kvecc.ecc_shim import patch_model_with_ecc_attention, reset_ecc_cache
    model = _gpt2().to(device)
    cfg = _cfg(codec, True, "hip" if device.type == "cuda" else "cpu")
    h = torch.randn(2, 24, 128, generator=torch.Generator().manual_seed(1)).to(device)
    outs = []
    for compiled in (False, True):
        with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=32):
            reset_ecc_cache(model)
            attn = model.transformer.h[0].attn
            fwd = attn.forward
            if compiled:
                torch._dynamo.reset()
                fwd = torch.compile(attn.forward, fullgraph=True, backend="aot_eager")
            out = fwd(h)[0]
            mgr = model._ecc_block_manager
            outs.append((out.clone(), mgr.k_cache.clone(), mgr.v_cache.clone(), model._ecc_backend._stats.clone()))
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    assert not bool(outs[0][3].any())  # no decode statistics


def test_compiled_forward_cpu():
    _compiled_forward(torch.device("cpu"), "hamming84")


@pytest.mark.gpu
def test_compiled_forward_hip(gpu):
    _compiled_forward(gpu, "golay")
