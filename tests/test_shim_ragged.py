"""set_ecc_query_spans: ragged batches through a patched append-mode model.

Models: the 2-layer GPT-2 and the GQA LLaMA of tests/test_shim_chunk.py.  Three prompts of 7, 4
and 1 tokens in one [3, 7] batch, padded on the left or on the right, prefilled in one forward;
then three single-token steps in which sequence 1 is finished after the first (count 0).  With
injection off every valid position's logits must match the same prompt run alone (batch 1, no
spans, a freshly patched model) to LOGIT_ATOL, the append-mode model tests' tolerance; padding
positions must be finite.  Lengths, blocks and counters follow the valid tokens only.
"""

import pytest
import torch

from tests.test_shim_chunk import BS, D, _gpt2
from tests.test_shim_llama import LOGIT_ATOL, _llama

LENS, QMAX, STEPS = [7, 4, 1], 7, 3
STEP_COUNTS = [[1, 1, 1], [1, 0, 1], [1, 0, 1]]
MODELS = {"gpt2": _gpt2, "llama": lambda: _llama()[0]}
CODECS = ["hamming84", "golay", "golay_packed"]
HKV = {"gpt2": 4, "llama": 2}


def _cfg(codec, chunk, backend, ber=0.0, overwrite=False, **kw):
    from kvecc.ecc_shim import ECCShimConfig
    storage = "packed" if codec == "golay_packed" else "int32"
    return ECCShimConfig(codec=codec.replace("_packed", ""), ber=ber, inject_errors=ber > 0, seed=42, block_size=BS,
                         backend=backend, golay_storage=storage, cache_mode="overwrite" if overwrite else "append",
                         chunk_attention=chunk, **kw)


def _tokens():
    g = torch.Generator().manual_seed(31)
    prompts = [torch.randint(1, 101, (n,), generator=g) for n in LENS]
    steps = torch.randint(1, 101, (3, STEPS), generator=g)
    return prompts, steps


def _firsts(side):
    return [QMAX - n if side == "left" else 0 for n in LENS]


def _padded(prompts, firsts):
    ids = torch.zeros(3, QMAX, dtype=torch.long)
    for b, (p, f) in enumerate(zip(prompts, firsts)):
        ids[b, f:f + len(p)] = p
    pos = (torch.arange(QMAX).unsqueeze(0) - torch.tensor(firsts).unsqueeze(1)).clamp(min=0)
    return ids, pos


def _solo(model, cfg, dev):
    """Each prompt alone -> (prefill logits [n_b, V], step logits [steps_b, V]) per sequence."""
    from kvecc.ecc_shim import patch_model_with_ecc_attention, reset_ecc_cache
    prompts, steps = _tokens()
    outs = []
    for b, p in enumerate(prompts):
        with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=32):
            reset_ecc_cache(model)
            n = len(p)
            pre = model(p.unsqueeze(0).to(dev), position_ids=torch.arange(n).unsqueeze(0).to(dev)).logits[0].float()
            gen = []
            for s in range(STEPS):
                if STEP_COUNTS[s][b]:
                    gen.append(model(steps[b, s].view(1, 1).to(dev),
                                     position_ids=torch.tensor([[n + s]]).to(dev)).logits[0, 0].float())
            outs.append((pre.cpu(), torch.stack(gen).cpu()))
    return outs


def _blocks(mgr):
    return [len(mgr.seq_to_blocks.get(b, [])) for b in range(3)]


def _check_lens(mgr, want):
    for layer in range(mgr.num_layers):
        assert mgr.layer_lens(layer, 3) == want, layer
    assert mgr.ctx_lens[:, :3].cpu().tolist() == [want] * mgr.num_layers


def _check_ragged(name, codec, chunk, backend, dev, side, pass_positions=True, **kw):
    from kvecc.ecc_shim import patch_model_with_ecc_attention, reset_ecc_cache, set_ecc_query_spans
    model = MODELS[name]().to(dev)
    cfg = _cfg(codec, chunk, backend, **kw)
    solo = _solo(model, cfg, dev)
    prompts, steps = _tokens()
    firsts = _firsts(side)
    ids, pos = _padded(prompts, firsts)
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=32):
        reset_ecc_cache(model)
        mgr = model._ecc_block_manager
        set_ecc_query_spans(model, LENS, firsts)
        args = dict(position_ids=pos.to(dev)) if pass_positions else {}
        logits = model(ids.to(dev), **args).logits.float().cpu()
        assert bool(logits.isfinite().all())  # padding positions included
        for b, (f, n) in enumerate(zip(firsts, LENS)):
            err = float((logits[b, f:f + n] - solo[b][0]).abs().max())
            print(f"prefill sequence {b}: max logit err {err:.3e}")
            assert err <= LOGIT_ATOL, (b, err)
        _check_lens(mgr, LENS)
        assert _blocks(mgr) == [cdiv(n, BS) for n in LENS]
        lens, seen = list(LENS), [0, 0, 0]
        for s in range(STEPS):
            counts = STEP_COUNTS[s]
            set_ecc_query_spans(model, counts)
            tok = steps[:, s].view(3, 1)
            args = dict(position_ids=torch.tensor(lens).view(3, 1).to(dev)) if pass_positions else {}
            blocks_before = _blocks(mgr)
            out = model(tok.to(dev), **args).logits.float().cpu()
            assert bool(out.isfinite().all())
            for b in range(3):
                if counts[b]:
                    err = float((out[b, 0] - solo[b][1][seen[b]]).abs().max())
                    print(f"step {s} sequence {b}: max logit err {err:.3e}")
                    assert err <= LOGIT_ATOL, (s, b, err)
                    seen[b] += 1
                    lens[b] += 1
                else:
                    assert _blocks(mgr)[b] == blocks_before[b]
            _check_lens(mgr, lens)
            assert _blocks(mgr) == [cdiv(n, BS) for n in lens]
        assert lens == [10, 5, 4]


CASES = [(n, c, ch, side) for n in MODELS for c in CODECS for ch in (True, False) for side in ("left", "right")]
CASE_IDS = [f"{n}-{c}-{'chunk' if ch else 'read'}-{side}" for n, c, ch, side in CASES]


@pytest.mark.parametrize("name,codec,chunk,side", CASES, ids=CASE_IDS)
def test_ragged_cpu(name, codec, chunk, side):
    _check_ragged(name, codec, chunk, "cpu", "cpu", side)


@pytest.mark.gpu
@pytest.mark.parametrize("name,codec,chunk,side", CASES, ids=CASE_IDS)
def test_ragged_hip(gpu, name, codec, chunk, side):
    _check_ragged(name, codec, chunk, "hip", gpu, side)


@pytest.mark.parametrize("side", ["left", "right"])
def test_ragged_counting_path_cpu(side):
    _check_ragged("gpt2", "hamming84", True, "cpu", "cpu", side, use_interpolation=True)


@pytest.mark.gpu
def test_ragged_counting_path_hip(gpu):
    _check_ragged("llama", "hamming84", True, "hip", gpu, "left", use_interpolation=True)


def _check_never_started(backend, dev, **kw):
    """A sequence with count 0 from the start holds nothing: its rows stay finite on every path."""
    from kvecc.ecc_shim import patch_model_with_ecc_attention, reset_ecc_cache, set_ecc_query_spans
    model = _gpt2().to(dev)
    ids = torch.randint(1, 101, (2, 3), generator=torch.Generator().manual_seed(6)).to(dev)
    pos = torch.arange(4).unsqueeze(0).expand(2, -1).to(dev)
    with torch.no_grad(), patch_model_with_ecc_attention(model, _cfg("hamming84", True, backend, **kw), num_blocks=32):
        reset_ecc_cache(model)
        set_ecc_query_spans(model, [3, 0])
        a = model(ids, position_ids=pos[:, :3]).logits
        set_ecc_query_spans(model, [1, 0])
        b = model(ids[:, :1], position_ids=pos[:, 3:]).logits
        assert bool(a.isfinite().all()) and bool(b.isfinite().all())
        lens = model._ecc_block_manager.layer_lens(1, 2)
        assert lens == [4, 0] and 1 not in model._ecc_block_manager.seq_to_blocks


@pytest.mark.parametrize("kw", [{}, dict(use_interpolation=True), dict(decode_stats=True)], ids=["kernel", "interp", "stats"])
def test_never_started_sequence_cpu(kw):
    _check_never_started("cpu", "cpu", **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [{}, dict(decode_stats=True)], ids=["kernel", "stats"])
def test_never_started_sequence_hip(gpu, kw):
    _check_never_started("hip", gpu, **kw)


# ---- LLaMA given no position_ids: token t of row b sits at start_b + max(t - first_b, 0) ---------
# (an HF model always hands its layers position_ids, so the attention module is called directly)
def _check_derived_positions(backend, dev, side):
    from kvecc.ecc_shim import patch_model_with_ecc_attention, reset_ecc_cache, set_ecc_query_spans
    model = MODELS["llama"]().to(dev)
    firsts = _firsts(side)
    h = torch.randn(3, QMAX + 1, 128, generator=torch.Generator().manual_seed(4)).to(dev)
    pos = (torch.arange(QMAX).unsqueeze(0) - torch.tensor(firsts).unsqueeze(1)).clamp(min=0).to(dev)
    runs = []
    with torch.no_grad(), patch_model_with_ecc_attention(model, _cfg("golay", True, backend), num_blocks=32):
        attn, mgr = model.model.layers[0].self_attn, model._ecc_block_manager
        for given in (True, False):
            reset_ecc_cache(model)
            set_ecc_query_spans(model, LENS, firsts)
            a = attn(h[:, :QMAX], position_ids=pos if given else None)[0]
            set_ecc_query_spans(model, [1, 0, 1])
            b = attn(h[:, QMAX:], position_ids=torch.tensor(LENS).view(3, 1).to(dev) if given else None)[0]
            runs.append([a.cpu(), b.cpu(), mgr.k_cache.cpu().clone(), mgr.k_scales.cpu().clone()])
    given, derived = runs
    assert torch.equal(given[2], derived[2]) and torch.equal(given[3], derived[3])  # the rotated keys
    for b, (f, n) in enumerate(zip(firsts, LENS)):
        assert torch.equal(given[0][b, f:f + n], derived[0][b, f:f + n]), b
    assert torch.equal(given[1][[0, 2]], derived[1][[0, 2]])
    assert bool(derived[0].isfinite().all()) and bool(derived[1].isfinite().all())


@pytest.mark.parametrize("side", ["left", "right"])
def test_llama_derives_positions_cpu(side):
    _check_derived_positions("cpu", "cpu", side)


@pytest.mark.gpu
def test_llama_derives_positions_hip(gpu):
    _check_derived_positions("hip", gpu, "left")


# ---- injection on: counters follow the valid tokens; all-full spans change nothing --------------
def _check_counters(name, codec, backend, dev):
    from kvecc.ecc_shim import get_ecc_stats, patch_model_with_ecc_attention, reset_ecc_cache, set_ecc_query_spans
    model = MODELS[name]().to(dev)
    prompts, _ = _tokens()
    firsts = _firsts("left")
    ids, pos = _padded(prompts, firsts)
    with torch.no_grad(), patch_model_with_ecc_attention(model, _cfg(codec, True, backend, ber=1e-2), num_blocks=32):
        reset_ecc_cache(model)
        set_ecc_query_spans(model, LENS, firsts)
        model(ids.to(dev), position_ids=pos.to(dev))
        st = get_ecc_stats(model)
        layers, rows = model._ecc_block_manager.num_layers, sum(LENS) * HKV[name]
        assert st["injection_count"] == layers * rows
        assert st["total_values"] == layers * 2 * rows * D
        set_ecc_query_spans(model, [1, 0, 1])
        model(ids[:, :1].to(dev), position_ids=torch.tensor(LENS).view(3, 1).to(dev))
        st = get_ecc_stats(model)
        assert st["injection_count"] == layers * (rows + 2 * HKV[name])
        assert st["total_values"] == layers * 2 * (rows + 2 * HKV[name]) * D


def _full_run(model, cfg, dev, spans):
    from kvecc.ecc_shim import get_ecc_stats, patch_model_with_ecc_attention, reset_ecc_cache, set_ecc_query_spans
    ids = torch.randint(1, 101, (3, QMAX), generator=torch.Generator().manual_seed(2)).to(dev)
    pos = torch.arange(QMAX + 1).unsqueeze(0).expand(3, -1).to(dev)
    with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=32):
        reset_ecc_cache(model)
        if spans:
            set_ecc_query_spans(model, [QMAX] * 3)
        a = model(ids, position_ids=pos[:, :QMAX]).logits.cpu()
        if spans:
            set_ecc_query_spans(model, [1] * 3)
        b = model(ids[:, :1], position_ids=pos[:, QMAX:]).logits.cpu()
        mgr = model._ecc_block_manager
        return [a, b] + [t.cpu().clone() for t in (mgr.k_cache, mgr.v_cache, mgr.k_scales, mgr.v_scales)], \
            get_ecc_stats(model)


def _check_full_spans(name, codec, chunk, backend, dev):
    model = MODELS[name]().to(dev)
    cfg = _cfg(codec, chunk, backend, ber=1e-2)
    with_spans, st1 = _full_run(model, cfg, dev, True)
    without, st0 = _full_run(model, cfg, dev, False)
    assert st1 == st0
    for a, b in zip(with_spans, without):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name,codec", [("gpt2", "hamming84"), ("llama", "golay_packed")])
def test_counters_cpu(name, codec):
    _check_counters(name, codec, "cpu", "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name,codec", [("gpt2", "golay"), ("llama", "hamming84")])
def test_counters_hip(gpu, name, codec):
    _check_counters(name, codec, "hip", gpu)


@pytest.mark.parametrize("name,codec,chunk", [("gpt2", "hamming84", True), ("llama", "golay", True),
                                              ("llama", "golay_packed", False)])
def test_full_spans_change_nothing_cpu(name, codec, chunk):
    _check_full_spans(name, codec, chunk, "cpu", "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name,codec,chunk", [("gpt2", "golay", True), ("llama", "hamming84", True),
                                              ("gpt2", "hamming84", False)])
def test_full_spans_change_nothing_hip(gpu, name, codec, chunk):
    _check_full_spans(name, codec, chunk, "hip", gpu)


# ---- errors ----------------------------------------------------------------------------------------
def test_errors():
    import kvecc
    from kvecc.ecc_shim import patch_model_with_ecc_attention, reset_ecc_cache, set_ecc_query_spans
    model = _gpt2()
    ids = torch.randint(1, 101, (3, QMAX), generator=torch.Generator().manual_seed(2))
    pos = torch.arange(QMAX).unsqueeze(0).expand(3, -1)
    with pytest.raises(ValueError):
        set_ecc_query_spans(model, [1])  # not patched
    with torch.no_grad(), patch_model_with_ecc_attention(model, _cfg("hamming84", False, "cpu", overwrite=True),
                                                         num_blocks=32):
        with pytest.raises(ValueError):
            set_ecc_query_spans(model, LENS)  # overwrite mode
    with torch.no_grad(), patch_model_with_ecc_attention(model, _cfg("hamming84", True, "cpu"), num_blocks=32):
        mgr = model._ecc_block_manager
        for bad in (dict(counts=[-1, 1, 1]), dict(counts=[1, 1, 1], firsts=[0, -2, 0]), dict(counts=[1] * 33),
                    dict(counts=[1, 1], firsts=[0])):
            with pytest.raises(ValueError):
                set_ecc_query_spans(model, **bad)
        set_ecc_query_spans(model, [7, 4])  # another batch
        with pytest.raises(ValueError):
            model(ids, position_ids=pos)
        set_ecc_query_spans(model, [7, 4, 1], [0, 4, 0])  # 4 + 4 > 7
        with pytest.raises(ValueError):
            model(ids, position_ids=pos)
        assert not bool(mgr.k_cache.any()) and not bool(mgr.k_scales.any()) and mgr.layer_lens(0, 3) == [0, 0, 0]
        assert mgr.seq_to_blocks == {}  # nothing was written or allocated
        set_ecc_query_spans(model, [7, 4, 1])
        model(ids, position_ids=pos)
        assert mgr.layer_lens(1, 3) == [7, 4, 1]
        reset_ecc_cache(model)  # clears the spans: a uniform forward of another batch runs
        assert model._ecc_backend._spans is None
        model(ids[:2], position_ids=pos[:2])
        assert mgr.layer_lens(1, 3) == [7, 7, 0]
        set_ecc_query_spans(model, [1, 1])
        set_ecc_query_spans(model, None)
        assert model._ecc_backend._spans is None
    with pytest.raises(ValueError):
        kvecc.query_spans_from_mask(torch.tensor([[1, 1, 0, 1], [1, 1, 1, 1]]))
    counts, firsts = kvecc.query_spans_from_mask(torch.tensor([[0, 0, 1, 1], [1, 1, 1, 1], [0, 0, 0, 0]]))
    assert (counts, firsts) == ([2, 4, 0], [2, 0, 0])
