"""The shim on a LLaMA-architecture model (RoPE, GQA: 4 query heads over 2 KV
heads), after the reference's TestPatchModelWithECCAttention
(tests/test_ecc_shim.py:310-445), which loads TinyLlama from the hub; here a
random-init LlamaForCausalLM (no network).

tests/golden/shim_llama.npz is the reference shim's own prefill of such a model
(fp32, 2 layers, head_dim 16, 20 tokens over blocks of 16; weights in the
fixture; tools/gen_golden.py:gen_shim_llama) for every codec, with the post-RoPE
K and the V that ECCBackend.write was given and the dequantized K/V handed to
_run_attention.  Against it, for the host and the HIP backend:

  * the patched model: get_ecc_stats equal (the per-row seed order with
    Hkv < H, the error classes), logits within LOGIT_ATOL / LOGIT_RTOL (RoPE
    positions, the repeat_interleave direction), layer 0's post-RoPE write
    inputs within test_attention's ATOL / RTOL;
  * the backend fed the reference's write inputs layer by layer: the K/V read
    back equal the reference's dequantized K/V in every bit, and so do the
    counters.
"""

import numpy as np
import pytest
import torch

LOGIT_ATOL = 2e-3
LOGIT_RTOL = 2e-3
NAME = "shim_llama"
RUNS = [("hamming84", False), ("hamming84", True), ("golay", False), ("hamming74", False), ("int4", False),
        ("fp16", False)]


def _llama(hidden_size=128):
    """head_dim = hidden_size / 4: 32, or 64 at hidden_size 256."""
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=101, hidden_size=hidden_size, intermediate_size=256, num_hidden_layers=2,
                      num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=128)
    return LlamaForCausalLM(cfg).eval(), torch.randint(0, 101, (1, 20),
                                                       generator=torch.Generator().manual_seed(1))


def _run(model, ids, backend, codec, ber, interp=False):
    from kvecc.ecc_shim import (ECCShimConfig, get_ecc_stats, patch_model_with_ecc_attention,
                                reset_ecc_cache)
    cfg = ECCShimConfig(codec=codec, ber=ber, inject_errors=ber > 0, seed=42, backend=backend,
                        use_interpolation=interp)
    with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=16):
        reset_ecc_cache(model)
        logits = model(ids).logits.float()
        return logits, get_ecc_stats(model)


def test_patch_replace_restore_and_rope_cpu():
    from kvecc.ecc_shim import ECCPagedAttentionShim, ECCShimConfig, patch_model_with_ecc_attention
    model, ids = _llama()
    orig_type = type(model.model.layers[0].self_attn)
    with torch.no_grad():
        ref = model(ids).logits
    with patch_model_with_ecc_attention(model, ECCShimConfig(codec="hamming84", backend="cpu"),
                                        num_blocks=16):
        assert isinstance(model.model.layers[0].self_attn, ECCPagedAttentionShim)
    assert type(model.model.layers[0].self_attn) is orig_type
    # fp16 storage: only fp16 rounding of K/V, so RoPE and GQA must match the model exactly-ish
    out, _ = _run(model, ids, "cpu", "fp16", 0.0)
    assert torch.allclose(out, ref, atol=1e-3)
    for codec in ("hamming84", "golay", "int4"):  # INT4 quantization noise only
        out, st = _run(model, ids, "cpu", codec, 0.0, interp=codec == "hamming84")
        cos = torch.nn.functional.cosine_similarity(out.flatten()[None], ref.flatten()[None]).item()
        assert cos > 0.98, (codec, cos)
        assert st["errors_corrected"] == 0 and st["total_values"] == 2 * 2 * 20 * 2 * 32


def test_errors_corrected_cpu():
    model, ids = _llama()
    clean, _ = _run(model, ids, "cpu", "golay", 0.0)
    noisy, st = _run(model, ids, "cpu", "golay", 1e-2)
    assert st["injection_count"] == 2 * 20 * 2 and st["errors_corrected"] > 0
    if st["errors_detected"] == 0:  # everything corrected -> identical logits
        assert torch.equal(noisy, clean)


@pytest.mark.gpu
@pytest.mark.parametrize("codec,interp", [("hamming84", True), ("hamming84", False),
                                          ("golay", False), ("hamming74", False)])
def test_hip_equals_cpu_backend(gpu, codec, interp):
    model, ids = _llama()
    cpu_logits, cpu_st = _run(model, ids, "cpu", codec, 1e-2, interp)
    model = model.to(gpu)
    hip_logits, hip_st = _run(model, ids.to(gpu), "hip", codec, 1e-2, interp)
    assert hip_st == cpu_st
    assert torch.allclose(hip_logits.cpu(), cpu_logits, atol=LOGIT_ATOL, rtol=LOGIT_ATOL)


# ---- against the reference's own run (tests/golden/shim_llama.npz) --------------

def fixture_llama(golden, model_cfg, device, name=NAME, prefix="w_"):
    """The random-init LLaMA whose weights fixture `name` holds as {prefix}*."""
    from transformers import LlamaConfig, LlamaForCausalLM
    model = LlamaForCausalLM(LlamaConfig(**model_cfg)).eval()
    state = {k[len(prefix):].replace("__", "."): torch.from_numpy(v) for k, v in golden(name).items()
             if k.startswith(prefix)}
    model.load_state_dict(state, strict=True)
    return model.to(device)


def ref_cfg(run, backend):
    from kvecc.ecc_shim import ECCShimConfig
    # the fixtures are the reference run on CPU tensors: IEEE scale division
    return ECCShimConfig(codec=run["codec"], ber=run["ber"], inject_errors=run["ber"] > 0, seed=42,
                         block_size=16, use_interpolation=run["use_interpolation"], backend=backend,
                         scale_rule="div7")


def logits_close(got, ref, what):
    """Logits within LOGIT_ATOL / LOGIT_RTOL of the reference's; prints the margin."""
    got = got.float().cpu().numpy()
    err = float(np.abs(got - ref).max())
    print(f"{what}: max |logit - reference| = {err:.3e}")
    assert np.allclose(got, ref, atol=LOGIT_ATOL, rtol=LOGIT_RTOL), (what, err)


def layer0_write_close(writes, g, prefix, what):
    """Layer 0's K/V as the patched model hands them to ECCBackend.write
    (`writes`: test_shim_fp16.capture's records of one forward) against the
    reference's.  They come from the embedding, one norm, the K/V projections
    and, for LLaMA, RoPE at the forward's position_ids: a wrong position turns K
    by a wrong angle, an O(|K|) error, while a correct one leaves the rounding of
    64-term fp32 dot products in another order, at most 64 * 2^-24 * sum|a||b|
    ~ 5e-6 for these weights (std 0.02) -- inside test_attention's ATOL / RTOL."""
    from tests.test_attention import ATOL, RTOL
    (k, v), = [(k, v) for layer, k, v in writes if layer == 0]
    for side, got in (("k", k), ("v", v)):
        ref = g[f"{prefix}_l0_{side}_in"]
        got = got.float().cpu().numpy().reshape(ref.shape)
        err = float(np.abs(got - ref).max())
        print(f"{what}: max |layer-0 {side.upper()} write input - reference| = {err:.3e}")
        assert np.allclose(got, ref, atol=ATOL, rtol=RTOL), (what, side, err)


def replay_read_equals(be, g, prefix, layer, ctx):
    """What the backend reads of `layer` after a replayed write is the K/V the
    reference handed to _run_attention ({prefix}_l{layer}_[kv]_deq, [ctx, Hkv, D]),
    bit for bit: the counting fused read (head-major, in the fp32 SDPA saw) or,
    for the fp16 codec, the cache rows themselves."""
    mgr, codec = be.manager, be.config.codec
    ref = [torch.from_numpy(g[f"{prefix}_l{layer}_{s}_deq"]) for s in ("k", "v")]
    if codec == "fp16":
        blk, slot = mgr.slots(0, ctx)
        got = [be._gather(c, blk, slot, layer) for c in (mgr.k_cache, mgr.v_cache)]
        assert ref[0].dtype == torch.float16
    else:
        interp = be.config.use_interpolation and codec == "hamming84"
        got = be.codec_backend.shim_read(mgr, layer, ctx, mgr.shim_codec, interp, torch.float32, be._stats)
        ref = [r.to(torch.float32).permute(1, 0, 2).contiguous() for r in ref]
    for side, a, b in zip("KV", got, ref):
        assert a.dtype == b.dtype and torch.equal(a.cpu(), b), (prefix, layer, side)


def counters_equal(be, stats, what):
    got = {"injection_count": be._injection_count, "errors_corrected": be._errors_corrected,
           "errors_detected": be._errors_detected, "total_values": be._total_values,
           "allocated_blocks": sum(len(b) for b in be.manager.seq_to_blocks.values())}
    assert got == {k: stats[k] for k in got}, (what, got, stats)


def test_llama_fixture_inventory(manifest, golden):
    p = manifest[NAME]["params"]
    m = p["model"]
    assert (m["num_attention_heads"], m["num_key_value_heads"], m["hidden_size"]) == (4, 2, 64)
    assert p["seq_len"] == 20 and p["dtype"] == "float32"
    assert [(r["codec"], r["use_interpolation"]) for r in p["runs"]] == RUNS
    g = golden(NAME)
    assert g["input_ids"].shape == (1, 20)
    for i, r in enumerate(p["runs"]):
        assert g[f"r{i}_logits"].dtype == np.float32 and g[f"r{i}_logits"].shape == (1, 20, 61)
        assert g[f"r{i}_l1_k_in"].dtype == np.float32 and g[f"r{i}_l1_k_in"].shape == (1, 20, 32)
        assert g[f"r{i}_l1_v_deq"].shape == (20, 2, 16)
        assert g[f"r{i}_l1_v_deq"].dtype == (np.float16 if r["codec"] == "fp16" else np.float32)
        st = r["stats"]
        assert st["total_values"] == 2 * 2 * 20 * 2 * 16 and st["allocated_blocks"] == 2
        assert st["injection_count"] == (0 if r["codec"] == "fp16" else 2 * 20 * 2)
        if r["codec"] == "hamming84":  # doubles: the interpolation has work, the plain decode keeps them
            assert st["errors_detected"] > 0 and st["errors_corrected"] > 0
        if r["codec"] in ("golay", "hamming74"):
            assert st["errors_corrected"] > 0


def _llama_matches_reference(device, backend, golden, manifest):
    from kvecc.ecc_shim import get_ecc_stats, patch_model_with_ecc_attention, reset_ecc_cache
    from tests.test_shim_fp16 import capture
    p = manifest[NAME]["params"]
    g = golden(NAME)
    model = fixture_llama(golden, p["model"], device)
    ids = torch.from_numpy(g["input_ids"]).to(device)
    for i, run in enumerate(p["runs"]):
        with torch.no_grad(), capture() as rec, \
                patch_model_with_ecc_attention(model, ref_cfg(run, backend), num_blocks=16):
            reset_ecc_cache(model)
            out = model(ids)
            st = get_ecc_stats(model)
        assert st == run["stats"], (run["codec"], st, run["stats"])
        what = f"{NAME} {backend} run {i} {run['codec']}"
        layer0_write_close(rec["write"], g, f"r{i}", what)
        logits_close(out.logits, g[f"r{i}_logits"], what)


def test_llama_matches_reference_cpu_backend(golden, manifest):
    _llama_matches_reference(torch.device("cpu"), "cpu", golden, manifest)


@pytest.mark.gpu
def test_llama_matches_reference(gpu, golden, manifest):
    _llama_matches_reference(gpu, "hip", golden, manifest)


def _llama_data_path_matches_reference(dev, backend, golden, manifest):
    from kvecc.ecc_shim import ECCBackend, SimpleBlockManager
    p = manifest[NAME]["params"]
    g = golden(NAME)
    m = p["model"]
    h, hk, nl = m["num_attention_heads"], m["num_key_value_heads"], m["num_hidden_layers"]
    d = m["hidden_size"] // h
    for i, run in enumerate(p["runs"]):
        mgr = SimpleBlockManager(16, 16, nl, hk, d, device=dev, codec=run["codec"])
        be = ECCBackend(mgr, ref_cfg(run, backend), num_heads=h)
        for layer in range(nl):
            be.write(torch.from_numpy(g[f"r{i}_l{layer}_k_in"]).to(dev),
                     torch.from_numpy(g[f"r{i}_l{layer}_v_in"]).to(dev), layer)
            replay_read_equals(be, g, f"r{i}", layer, p["seq_len"])
        counters_equal(be, run["stats"], (i, run["codec"]))


def test_llama_data_path_matches_reference_cpu_backend(golden, manifest):
    _llama_data_path_matches_reference(torch.device("cpu"), "cpu", golden, manifest)


@pytest.mark.gpu
def test_llama_data_path_matches_reference(gpu, golden, manifest):
    _llama_data_path_matches_reference(gpu, "hip", golden, manifest)
