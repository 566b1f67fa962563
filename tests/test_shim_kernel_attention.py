"""ECCShimConfig(kernel_attention=True): every forward of an append-mode hamming74 or int4 model
runs on the paged attention kernels -- single-token steps on the decode entry, longer forwards
on the chunked causal entry, held spans on the ragged entry -- instead of the batched read +
masked SDPA, and keeps no decode statistics.

Models, schedule and bounds are tests/test_shim_chunk.py's (GPT-2 and the GQA LLaMA; a 7-token
forward, free(1), then 19, 5, 5, 1, 1, 1 tokens; BER 1e-2 with injection): flag on and off
agree on the logits to LOGIT_ATOL, on layer 0's caches bit for bit and on the later layers
within that file's bounds (both codes are linear, so its XOR argument holds: the XOR of two
Hamming(7,4) codewords with the same flips decodes to the XOR of the nibbles, and two raw
nibbles XOR directly).  The ragged batch is tests/test_shim_ragged.py's: prompts of 7 / 4 / 1
tokens against solo runs.

int4 has no code, so its counting path counts nothing either: for it "statistics present with
the flag off" is vacuous, and only the injection counts and the zero counts are compared.
"""

import pytest
import torch

from tests import test_shim_chunk as shim_chunk
from tests.test_shim_chunk import MODELS, _agree, _cfg, _check_stats, _gpt2, _run
from tests.test_shim_ragged import _check_ragged

CODECS = ["hamming74", "int4"]


def _on(codec, backend="cpu", **kw):
    return _cfg(codec, False, backend, kernel_attention=True, **kw)


def _off(codec, backend="cpu", **kw):
    return _cfg(codec, False, backend, **kw)


def _nibble_xor(x, y, codec):
    """tests/test_shim_chunk.py's _nibble_xor for the two byte codecs."""
    from kvecc import cpu_ops
    w = (x ^ y).contiguous()
    return cpu_ops.hamming74_decode(w.view(-1))[0] if codec == "hamming74" else w.view(-1)


def _check_counts(on, off, codec):
    if codec == "hamming74":
        _check_stats(on, off)
        return
    for st in on["stats"] + off["stats"]:  # nothing to count without a code
        assert st["errors_corrected"] == 0 and st["errors_detected"] == 0
    counts = [st["injection_count"] for st in on["stats"]]
    assert counts == [st["injection_count"] for st in off["stats"]]
    assert all(b > a for a, b in zip(counts, counts[1:])) and counts[0] > 0


def test_flag_validation():
    from kvecc.ecc_shim import ECCShimConfig
    for codec in CODECS:
        with pytest.raises(ValueError):
            ECCShimConfig(codec=codec, kernel_attention=True)  # overwrite mode, the default
        with pytest.raises(ValueError):
            ECCShimConfig(codec=codec, cache_mode="overwrite", kernel_attention=True)
        assert ECCShimConfig(codec=codec, cache_mode="append", kernel_attention=True).kernel_attention is True
        assert ECCShimConfig(codec=codec, cache_mode="append").kernel_attention is False
    for codec in ("hamming84", "golay", "fp16", "fp8"):
        with pytest.raises(ValueError):
            ECCShimConfig(codec=codec, cache_mode="append" if codec in ("hamming84", "golay") else "overwrite",
                          kernel_attention=True)
    with pytest.raises(ValueError):
        ECCShimConfig(codec="golay", golay_storage="packed", cache_mode="append", kernel_attention=True)
    assert ECCShimConfig().kernel_attention is False


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("name", list(MODELS))
def test_kernel_attention_equals_the_default_path_cpu(monkeypatch, name, codec):
    monkeypatch.setattr(shim_chunk, "_nibble_xor", _nibble_xor)
    model = MODELS[name]()
    on, off = _run(model, _on(codec)), _run(model, _off(codec))
    _agree(on, off, codec=codec)
    _check_counts(on, off, codec)


def test_the_flag_routes_every_forward_and_decode_stats_keeps_the_counting_path(monkeypatch):
    from kvecc import cpu_ops
    calls = {"decode": 0, "chunk": 0}
    real_d, real_c = cpu_ops.paged_attention_into, cpu_ops.paged_attention_chunk_into

    def decode(*a, **k):
        calls["decode"] += 1
        return real_d(*a, **k)

    def chunked(*a, **k):
        calls["chunk"] += 1
        return real_c(*a, **k)

    monkeypatch.setattr(cpu_ops, "paged_attention_into", decode)
    monkeypatch.setattr(cpu_ops, "paged_attention_chunk_into", chunked)
    model = _gpt2()
    r = _run(model, _on("hamming74", decode_stats=True))
    assert r["stats"][1]["errors_corrected"] > 0 and calls == {"decode": 0, "chunk": 0}
    _run(model, _cfg("hamming74", True))  # chunk_attention alone: read + SDPA, as before
    _run(model, _cfg("int4", True))
    assert calls == {"decode": 0, "chunk": 0}
    _run(model, _on("hamming74"))
    assert calls == {"decode": 2 * 3, "chunk": 2 * 4}  # layers x (single-token steps, longer forwards)


@pytest.mark.gpu
@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("name", list(MODELS))
def test_kernel_attention_hip(gpu, monkeypatch, name, codec):
    monkeypatch.setattr(shim_chunk, "_nibble_xor", _nibble_xor)
    model = MODELS[name]()
    cpu_on = _run(model, _on(codec))
    model = model.to(gpu)
    on, off = _run(model, _on(codec, "hip"), gpu), _run(model, _off(codec, "hip"), gpu)
    _agree(on, off, codec=codec)
    _check_counts(on, off, codec)
    # and the host twin (its projections are other GEMMs: the K / V it stores differ in the last bit)
    _agree(on, cpu_on, caches=False)
    assert on["stats"] == cpu_on["stats"]


# ---- ragged batches: prompts of 7 / 4 / 1 tokens against solo runs --------------------------------
RAGGED = [(n, c, side) for n in MODELS for c in CODECS for side in ("left", "right")]
RAGGED_IDS = [f"{n}-{c}-{side}" for n, c, side in RAGGED]


@pytest.mark.parametrize("name,codec,side", RAGGED, ids=RAGGED_IDS)
def test_ragged_cpu(monkeypatch, name, codec, side):
    from kvecc import cpu_ops
    spans = []
    real = cpu_ops.paged_attention_chunk_into
    monkeypatch.setattr(cpu_ops, "paged_attention_chunk_into",
                        lambda *a, **k: spans.append(k.get("q_spans") is not None) or real(*a, **k))
    _check_ragged(name, codec, False, "cpu", "cpu", side, kernel_attention=True)
    # the solo prefills of 7 and 4 tokens (2 layers each) are uniform calls, the batch's prefill is ragged
    assert spans == [False] * 4 + [True] * 2


@pytest.mark.gpu
@pytest.mark.parametrize("name,codec,side", RAGGED, ids=RAGGED_IDS)
def test_ragged_hip(gpu, name, codec, side):
    _check_ragged(name, codec, False, "hip", gpu, side, kernel_attention=True)


# ---- torch.compile: the dispatcher ops are traced -------------------------------------------------
def _compiled(monkeypatch, device, codec):
    monkeypatch.setattr(shim_chunk, "_cfg", lambda c, chunk, backend="cpu", **kw: _on(c, backend, **kw))
    shim_chunk._compiled_forward(device, codec)


@pytest.mark.parametrize("codec", CODECS)
def test_compiled_forward_cpu(monkeypatch, codec):
    _compiled(monkeypatch, torch.device("cpu"), codec)


@pytest.mark.gpu
def test_compiled_forward_hip(gpu, monkeypatch):
    _compiled(monkeypatch, gpu, "int4")
