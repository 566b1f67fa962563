"""Single-token forwards after a prefill in the shim's default (overwrite) mode,
against the reference shim's own run.

tests/golden/shim_gpt2_steps.npz and shim_llama_steps.npz hold the reference
shim (kv_cache/ecc_shim.py) run on CPU tensors over a 20-token prefill and then
4 (GPT-2) or 2 (LLaMA) single-token forwards with explicit position_ids
(tools/gen_golden.py:gen_shim_gpt2_steps, gen_shim_llama_steps; the model
weights are those of shim_gpt2.npz / shim_llama.npz, the MHA twin's are m_w_*
here).  What the reference does there, and what these tests pin:

  * every forward writes from position 0: a step's token overwrites slot 0,
    context_len stays 20, allocated_blocks stays 2, and each step re-reads (and
    on the Python path re-counts) all 20 slots;
  * _injection_count runs on across forwards, so a step's rows get seeds
    behind the prefill's;
  * Hamming(8,4) without interpolation takes paged_attention_ecc at seq_len 1,
    which counts nothing; Hamming(8,4) + interpolation and Golay keep to the
    Python path and count.

Per run, for the host backend and (gpu) the HIP backend:

  * model level: get_ecc_stats after every forward equals the fixture's, logits
    within LOGIT_ATOL / LOGIT_RTOL, and layer 0's write inputs (the step's
    position through RoPE, before any drift) within ATOL / RTOL;
  * backend level: the recorded write inputs replayed forward by forward, layer
    by layer; on the Python path the fused read returns the reference's
    dequantized K/V bit for bit, on the kernel path attend(recorded q) is within
    test_attention's ATOL / RTOL of the recorded output; counters equal after
    every forward.

The GQA kernel-path steps (4 query heads over 2 cache heads) are where this
project differs on purpose: ours reads cache head h // groups, the reference
kernel cache head h.  There every head must equal a float64 restatement with
h // groups over the oracle-decoded cache, and some head other than 0 must
differ from the reference's recorded output; model-level logits of those steps
are compared on the MHA twin only.

One more check was planned there and cannot hold: that head 0, "cache head 0
under both mappings", equals the reference's recorded output.  The reference
kernel does not only index head h, it strides the [blocks, layers, Hkv, .]
caches and scales by H (attention_ecc.py:362-383): it reads row (block * layers
+ layer) * H + h of the flattened cache where the layout has (block * layers +
layer) * Hkv + h // groups.  With Hkv = 2, H = 4 these agree for head 0 in block
0 of layer 0 alone; the 20-token context's second block (tokens 16..19) the
reference reads from physical block 2, which is never written (zero codewords,
zero scales).  So its head 0 is not attention over the sequence either: measured
on the replayed cache, |ours - reference| on head 0 is 3.0e-2 .. 1.2e-1 (other
heads 1.5e-1 .. 1.6e-1), far from ATOL, and no kernel can match both it and the
h // groups restatement.  In its place, and for every head instead of one: the
reference's recorded output must equal a float64 restatement of its own stride-H
addressing over the same replayed cache (measured 1e-8 .. 3e-8).  That ties the
recorded outputs to the cache bits our write kernels left (the step's one-token
write included) and states the difference exactly.
"""

import math

import numpy as np
import pytest
import torch

from tests.test_attention import ATOL, RTOL
from tests.test_shim_fp16 import capture
from tests.test_shim_llama import (counters_equal, fixture_llama, layer0_write_close, logits_close, ref_cfg,
                                   replay_read_equals)

FIXTURES = {"shim_gpt2_steps": [("gpt2", "hamming84", False), ("gpt2", "hamming84", True), ("gpt2", "golay", False)],
            "shim_llama_steps": [("gqa", "golay", False), ("gqa", "hamming84", False), ("mha", "hamming84", False)]}


def _dims(name, manifest):
    """which -> (query heads, cache heads, head_dim, layers, model config)."""
    p = manifest[name]["params"]
    if name == "shim_gpt2_steps":
        m = p["model"]
        return {"gpt2": (m["n_head"], m["n_head"], m["n_embd"] // m["n_head"], m["n_layer"], m)}
    return {w: (m["num_attention_heads"], m["num_key_value_heads"], m["hidden_size"] // m["num_attention_heads"],
                m["num_hidden_layers"], m) for w, m in p["models"].items()}


def _models(name, golden, manifest, device):
    p = manifest[name]["params"]
    if name == "shim_gpt2_steps":
        from transformers import GPT2Config, GPT2LMHeadModel
        model = GPT2LMHeadModel(GPT2Config(**p["model"])).eval()
        model.load_state_dict({k[2:].replace("__", "."): torch.from_numpy(v)
                               for k, v in golden(p["weights"]).items() if k.startswith("w_")}, strict=True)
        return {"gpt2": model.to(device)}
    return {"gqa": fixture_llama(golden, p["models"]["gqa"], device, name=p["gqa_weights"]),
            "mha": fixture_llama(golden, p["models"]["mha"], device, name=name, prefix="m_w_")}


def _forwards(g, device):
    ids, steps = torch.from_numpy(g["input_ids"]), torch.from_numpy(g["step_ids"])
    n = ids.shape[1]
    return [(ids.to(device), None)] + [(steps[:, s:s + 1].to(device), torch.tensor([[n + s]], device=device))
                                       for s in range(steps.shape[1])]


@pytest.mark.parametrize("name", list(FIXTURES))
def test_steps_fixture_inventory(name, manifest, golden):
    p = manifest[name]["params"]
    g = golden(name)
    dims = _dims(name, manifest)
    assert [(r["model"], r["codec"], r["use_interpolation"]) for r in p["runs"]] == FIXTURES[name]
    assert p["seq_len"] == 20 and g["input_ids"].shape == (1, 20) and g["step_ids"].shape == (1, p["steps"])
    for i, r in enumerate(p["runs"]):
        h, hk, d, nl, _ = dims[r["model"]]
        st = r["stats"]
        assert len(st) == 1 + p["steps"] and r["ber"] > 0
        assert r["fast_path"] == (r["codec"] == "hamming84" and not r["use_interpolation"])
        assert st[0]["total_values"] == 2 * nl * 20 * hk * d and st[0]["injection_count"] == nl * 20 * hk
        assert st[0]["errors_corrected"] > 0
        if r["codec"] == "hamming84":  # doubles in the prefill: the interpolation is exercised
            assert st[0]["errors_detected"] > 0
        for f in range(1, len(st)):
            # one token's worth per step; the cache keeps its 20 slots in 2 blocks
            assert st[f]["total_values"] - st[f - 1]["total_values"] == 2 * nl * hk * d
            assert st[f]["injection_count"] - st[f - 1]["injection_count"] == nl * hk
            assert (st[f]["allocated_blocks"], st[f]["free_blocks"], st[f]["sequences"]) == (2, 14, 1)
            grew = st[f]["errors_corrected"] - st[f - 1]["errors_corrected"]
            # the kernel path counts nothing; the Python path re-counts all 20 slots
            assert grew == 0 if r["fast_path"] else grew > 0
            if r["fast_path"]:
                assert st[f]["errors_detected"] == st[0]["errors_detected"]
        for f in range(len(st)):
            p_ = f"r{i}_f{f}"
            assert g[f"{p_}_logits"].dtype == np.float32 and g[f"{p_}_logits"].shape[:2] == (1, 20 if f == 0 else 1)
            for layer in range(nl):
                assert g[f"{p_}_l{layer}_k_in"].shape == (1, 20 if f == 0 else 1, hk * d)
                assert g[f"{p_}_l{layer}_k_in"].dtype == np.float32
                if r["fast_path"] and f > 0:
                    assert g[f"{p_}_l{layer}_q"].shape == g[f"{p_}_l{layer}_out"].shape == (1, h, 1, d)
                    assert f"{p_}_l{layer}_k_deq" not in g
                else:
                    assert g[f"{p_}_l{layer}_k_deq"].shape == (20, hk, d)
                    assert g[f"{p_}_l{layer}_k_deq"].dtype == np.float32


# ---- model level --------------------------------------------------------------------

def _steps_match_reference(name, device, backend, golden, manifest):
    from kvecc.ecc_shim import get_ecc_stats, patch_model_with_ecc_attention, reset_ecc_cache
    p, g, dims = manifest[name]["params"], golden(name), _dims(name, manifest)
    models = _models(name, golden, manifest, device)
    forwards = _forwards(g, device)
    for i, run in enumerate(p["runs"]):
        model = models[run["model"]]
        h, hk = dims[run["model"]][:2]
        with torch.no_grad(), capture() as rec, \
                patch_model_with_ecc_attention(model, ref_cfg(run, backend), num_blocks=16):
            reset_ecc_cache(model)
            for f, (ids, pos) in enumerate(forwards):
                rec["write"].clear()
                out = model(ids) if pos is None else model(ids, position_ids=pos)
                st = get_ecc_stats(model)
                assert st == run["stats"][f], (i, f, st, run["stats"][f])
                what = f"{name} {backend} run {i} forward {f}"
                layer0_write_close(rec["write"], g, f"r{i}_f{f}", what)  # the step's position reached RoPE
                if run["fast_path"] and hk != h and f > 0:
                    continue  # cache head h // groups, not the reference's h: pinned at backend level
                logits_close(out.logits, g[f"r{i}_f{f}_logits"], what)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_steps_match_reference_cpu_backend(name, golden, manifest):
    _steps_match_reference(name, torch.device("cpu"), "cpu", golden, manifest)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FIXTURES))
def test_steps_match_reference(name, gpu, golden, manifest):
    _steps_match_reference(name, gpu, "hip", golden, manifest)


# ---- backend level ------------------------------------------------------------------

def _attention_f64(mgr, layer, q, ctx, row):
    """softmax(q . K / sqrt(d)) . V in float64 over the oracle-decoded Hamming(8,4)
    cache, q [H, D] -> [H, D].  row(block, head) names the [block_size, D] row of
    the caches, flattened to [blocks * layers * Hkv, block_size * D], that query
    head `head` reads for the tokens of physical block `block`."""
    from oracle import oracle
    bs, d = mgr.block_size, mgr.head_dim
    table = mgr.block_table[0].cpu().numpy()
    kv = []
    for cache, scales in ((mgr.k_cache, mgr.k_scales), (mgr.v_cache, mgr.v_scales)):
        cw = cache.cpu().contiguous().numpy().reshape(-1, bs, d)
        sc = scales.cpu().contiguous().numpy().reshape(-1, bs)
        data, _, _ = oracle.hamming84_decode(cw)
        kv.append((data.astype(np.float64) - 8.0) * sc.astype(np.float64)[..., None])
    out = np.empty(q.shape, np.float64)
    for head in range(q.shape[0]):
        k, v = (np.stack([x[row(int(table[t // bs]), head), t % bs] for t in range(ctx)]) for x in kv)
        s = k @ q[head].astype(np.float64) / math.sqrt(d)
        w = np.exp(s - s.max())
        out[head] = (w / w.sum()) @ v
    return out


def _close(a, b):
    return np.abs(a - b) <= ATOL + RTOL * np.abs(b)


def _replay_matches_reference(name, dev, backend, golden, manifest):
    from kvecc.ecc_shim import ECCBackend, SimpleBlockManager
    p, g, dims = manifest[name]["params"], golden(name), _dims(name, manifest)
    ctx = p["seq_len"]
    for i, run in enumerate(p["runs"]):
        h, hk, d, nl, _ = dims[run["model"]]
        mgr = SimpleBlockManager(16, 16, nl, hk, d, device=dev, codec=run["codec"])
        be = ECCBackend(mgr, ref_cfg(run, backend), num_heads=h)
        assert (be.num_heads, be.num_kv_heads) == (h, hk)
        differs = False
        for f in range(1 + p["steps"]):
            for layer in range(nl):
                pre = f"r{i}_f{f}"
                be.write(torch.from_numpy(g[f"{pre}_l{layer}_k_in"]).to(dev),
                         torch.from_numpy(g[f"{pre}_l{layer}_v_in"]).to(dev), layer)
                if f"{pre}_l{layer}_q" not in g:  # Python path: the counting read
                    replay_read_equals(be, g, pre, layer, ctx)
                    continue
                q, ref = g[f"{pre}_l{layer}_q"], g[f"{pre}_l{layer}_out"]
                got = be.attend(torch.from_numpy(q).to(dev), layer).cpu().numpy()
                assert got.shape == ref.shape == (1, h, 1, d) and got.dtype == np.float32
                what = f"{name} {backend} run {i} forward {f} layer {layer}"
                if hk == h:
                    print(f"{what}: max |attend - reference| = {float(np.abs(got - ref).max()):.3e}")
                    assert _close(got, ref).all(), what
                    continue
                # GQA: ours reads cache row (block, layer, h // groups) of the
                # [blocks, layers, Hkv, .] caches; the reference kernel strides them
                # by H (attention_ecc.py:362-383), i.e. row (block * layers + layer) * H + h
                want = _attention_f64(mgr, layer, q[0, :, 0], ctx,
                                      lambda blk, hd: (blk * nl + layer) * hk + hd // (h // hk))
                theirs = _attention_f64(mgr, layer, q[0, :, 0], ctx, lambda blk, hd: (blk * nl + layer) * h + hd)
                print(f"{what}: max |attend - float64 h//groups| = {float(np.abs(got[0, :, 0] - want).max()):.3e}, "
                      f"|reference - float64 stride-H| = {float(np.abs(ref[0, :, 0] - theirs).max()):.3e}, "
                      f"head 0 vs reference {float(np.abs(got[0, 0] - ref[0, 0]).max()):.3e}, "
                      f"other heads vs reference {float(np.abs(got[0, 1:] - ref[0, 1:]).max()):.3e}")
                assert _close(got[0, :, 0], want).all(), what
                # the recorded output is the reference's addressing over these cache
                # bits (the step's one-token write included), every head
                assert _close(ref[0, :, 0], theirs).all(), what
                differs = differs or not _close(got[0, 1:], ref[0, 1:]).all()
            counters_equal(be, run["stats"][f], (name, i, f))
        # the fixture exercises the difference: some head h > 0 is not the reference's
        assert differs == (run["fast_path"] and hk != h), (name, i)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_steps_replay_matches_reference_cpu_backend(name, golden, manifest):
    _replay_matches_reference(name, torch.device("cpu"), "cpu", golden, manifest)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FIXTURES))
def test_steps_replay_matches_reference(name, gpu, golden, manifest):
    _replay_matches_reference(name, gpu, "hip", golden, manifest)
