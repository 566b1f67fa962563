"""scrub_ecc_cache / age_ecc_cache / ECCBackend.scrub on patched models (kvecc/ecc_shim.py).

Models: the tiny GPT-2 and GQA LLaMA of tests/test_shim_chunk.py (2 layers, head_dim 32; 4 and 2
cache heads), append mode, batch 2, block_size 4: a 9-token prefill and 3 generated tokens written
at ber = 0, so every cached codeword is clean and 12 tokens per sequence and layer are resident.

Ageing (age_ecc_cache) and the scrub are restated in numpy from the oracle alone -- oracle.inject
over the whole K tensor with `seed` and the whole V tensor with `seed + V_SEED_OFFSET`, then the
restatement of tests/test_cache_scrub.py over the valid tokens -- and the product's caches must
match bit for bit.  The host backend runs everywhere, the HIP kernels under the gpu marker.
"""

import numpy as np
import pytest
import torch

from tests.test_cache_scrub import _expect, _unpack3, _valid
from tests.test_generation_append import _forwards
from tests.test_shim_chunk import MODELS

BS, D, PREFILL, STEPS, NBLK = 4, 32, 9, 3, 32
TOKENS = PREFILL + STEPS
CODECS = ["hamming84", "golay", "golay_packed"]
N_BITS = {"hamming74": 7, "hamming84": 8, "golay": 24, "golay_packed": 8}
SINGLES_BER, SINGLES_SEED = 3e-4, 11


@pytest.fixture(params=["cpu", pytest.param("hip", marks=pytest.mark.gpu)])
def be(request):
    """(backend name, device) of the host twin / the HIP kernels."""
    if request.param == "cpu":
        return "cpu", torch.device("cpu")
    return "hip", request.getfixturevalue("gpu")


def _cfg(codec, backend, mode="append", **kw):
    from kvecc.ecc_shim import ECCShimConfig
    storage = "packed" if codec == "golay_packed" else "int32"
    return ECCShimConfig(codec=codec.replace("_packed", ""), ber=0.0, inject_errors=False, seed=42, block_size=BS,
                         backend=backend, golay_storage=storage, cache_mode=mode, **kw)


def _ids(n=TOKENS + 2):
    return torch.randint(0, 101, (2, n), generator=torch.Generator().manual_seed(23))


def _fill(model, dev):
    """Prefill and generated tokens of both sequences on a freshly reset patched model."""
    from kvecc.ecc_shim import reset_ecc_cache
    reset_ecc_cache(model)
    _forwards(model, _ids()[:, :TOKENS].to(dev), [0, 0], [PREFILL] + [1] * STEPS)


def _next(model, dev, n):
    """Logits of the next n-token forward (n 1: the decode step; n 2: a chunk)."""
    return _forwards(model, _ids()[:, TOKENS:TOKENS + n].to(dev), [TOKENS, TOKENS], [n]).cpu()


def _np(mgr):
    """K and V caches as numpy [blocks, layers, heads, block_size, per]"""
    return [mgr.view5(c).cpu().numpy().copy() for c in (mgr.k_cache, mgr.v_cache)]


def _mask(mgr, batch=2, layers=None):
    nl = mgr.num_layers
    lens = [mgr.layer_lens(layer, batch) for layer in range(nl)]
    v = _valid(mgr.block_table[:batch].cpu().numpy(), lens, 0, nl, mgr.num_blocks, nl, mgr.num_kv_heads, mgr.block_size)
    if layers is not None:
        for layer in range(nl):
            if layer not in layers:
                v[:, layer] = False
    return v


def _age_np(oracle, caches, codec, ber, seed):
    from kvecc.ecc_shim import V_SEED_OFFSET
    return [oracle.inject(c, ber, N_BITS[codec], seed=seed + i * V_SEED_OFFSET)[0].reshape(c.shape)
            for i, c in enumerate(caches)]


def _codewords(codec, c):
    """The codeword bits alone: packed rows without their pad bytes, int32 Golay words without bits 24..31."""
    if codec == "golay_packed":
        return _unpack3(c, (D + 2) // 3)
    return c & 0xFFFFFF if codec == "golay" else c


def _flips_per_word(codec, a, b):
    x = (_codewords(codec, a) ^ _codewords(codec, b)).astype(np.uint32)
    return np.array([bin(int(w)).count("1") for w in x.reshape(-1)]).reshape(x.shape)


def _nibbles(oracle, codec, c):
    w = _codewords(codec, c)
    if codec == "hamming84":
        return oracle.hamming84_decode(w)[0].reshape(w.shape)
    return oracle.golay_decode(w.astype(np.int32))[0].reshape(*w.shape, 3)


def _patched(name, cfg, dev):
    from kvecc.ecc_shim import patch_model_with_ecc_attention
    model = MODELS[name]().to(dev)
    return model, patch_model_with_ecc_attention(model, cfg, num_blocks=NBLK)


# ---- clean cache ---------------------------------------------------------------------------

@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("name", list(MODELS))
def test_clean_cache_scrubs_to_nothing(be, name, codec):
    from kvecc.ecc_shim import scrub_ecc_cache
    backend, dev = be
    model, ctx = _patched(name, _cfg(codec, backend), dev)
    with torch.no_grad(), ctx:
        _fill(model, dev)
        mgr = model._ecc_block_manager
        before = _np(mgr)
        got = scrub_ecc_cache(model)
        words = 2 * mgr.num_layers * 2 * TOKENS * mgr.num_kv_heads * (D if codec == "hamming84" else (D + 2) // 3)
        assert got == {"corrected": 0, "detected": 0, "rewritten": 0, "scanned": words}
        for a, b in zip(before, _np(mgr)):
            assert np.array_equal(a, b)


# ---- repair after ageing ---------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [False, True], ids=["decode", "chunk"])
@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("name", list(MODELS))
def test_scrub_repairs_single_errors(be, oracle, name, codec, chunk):
    """Single errors only among the valid tokens (asserted from the oracle restatement of this seed):
    one scrub restores every valid codeword, and the next forward's logits are the never-aged
    model's, exactly -- on the decode step and on the chunked attention kernel."""
    from kvecc.ecc_shim import age_ecc_cache, scrub_ecc_cache
    backend, dev = be
    n = 2 if chunk else 1
    model, ctx = _patched(name, _cfg(codec, backend, chunk_attention=chunk), dev)
    with torch.no_grad(), ctx:
        _fill(model, dev)
        want_logits = _next(model, dev, n)
        _fill(model, dev)
        mgr = model._ecc_block_manager
        clean = _np(mgr)
        valid = _mask(mgr)
        aged = _age_np(oracle, clean, codec, SINGLES_BER, SINGLES_SEED)
        flips = [_flips_per_word(codec, a, c)[valid] for a, c in zip(aged, clean)]
        assert max(int(f.max()) for f in flips) == 1 and min(int(f.sum()) for f in flips) > 0  # the precondition
        age_ecc_cache(model, SINGLES_BER, SINGLES_SEED)
        for a, b in zip(aged, _np(mgr)):
            assert np.array_equal(a, b)  # the ageing itself is the oracle's injection
        got = scrub_ecc_cache(model)
        n_flips = sum(int(f.sum()) for f in flips)
        assert got["rewritten"] == n_flips and got["detected"] == 0
        after = _np(mgr)
        for a, c, x in zip(after, clean, aged):
            assert np.array_equal(_codewords(codec, a)[valid], _codewords(codec, c)[valid])
            assert np.array_equal(a[~valid], x[~valid])  # unused slots and blocks stay aged
        assert torch.equal(_next(model, dev, n), want_logits)


# ---- the accumulation experiment ---------------------------------------------------------------

ACC = {"hamming84": (2e-2, 8, 5), "golay": (1e-2, 8, 5), "golay_packed": (1e-2, 8, 5)}  # codec -> (p, rounds, seed)


@pytest.mark.parametrize("codec", list(ACC))
def test_scrubbing_every_round_beats_never_scrubbing(be, oracle, codec):
    """R rounds of age_ecc_cache(p, seed + r) on the GPT-2 cache, scrubbing after every round
    against never: both trajectories are restated from the oracle and match the product bit for bit,
    and the scrubbed cache ends with strictly fewer wrong nibbles among the valid tokens (decoded
    against the pre-ageing decode).  Oracle restatement, seed 5, K and V of both layers: 12,288
    valid nibbles for hamming84, 12,672 for Golay (11 codewords of 3 per 32-value row):
      hamming84,    p 2e-2, R 8: 3270 wrong nibbles never scrubbed, 736 scrubbed every round;
      golay,        p 1e-2, R 8:  776 wrong nibbles never scrubbed,   7 scrubbed every round;
      golay packed, p 1e-2, R 8:  806 wrong nibbles never scrubbed,   3 scrubbed every round
    (the packed layout holds the same codewords but draws 8 bits per byte, another flip pattern).
    Wrong nibbles depend on the flip pattern alone (the codes are linear), so the counts hold for any
    model; the second assertion asks for a factor of 2, the smallest gap above being 4.4."""
    from kvecc.ecc_shim import age_ecc_cache, scrub_ecc_cache
    backend, dev = be
    p, rounds, seed = ACC[codec]
    model, ctx = _patched("gpt2", _cfg(codec, backend), dev)
    residual = {}
    with torch.no_grad(), ctx:
        for scrub in (False, True):
            _fill(model, dev)
            mgr = model._ecc_block_manager
            want = _np(mgr)
            valid = _mask(mgr)
            truth = [_nibbles(oracle, codec, c) for c in want]
            for r in range(rounds):
                want = _age_np(oracle, want, codec, p, seed + r)
                age_ecc_cache(model, p, seed + r)
                if scrub:
                    want = [_expect(oracle, codec, D, c, valid)[0] for c in want]
                    scrub_ecc_cache(model)
            for a, b in zip(want, _np(mgr)):
                assert np.array_equal(a, b)
            residual[scrub] = sum(int((_nibbles(oracle, codec, c)[valid] != t[valid]).sum()) for c, t in zip(want, truth))
    print(f"{codec}: wrong nibbles never scrubbed {residual[False]}, scrubbed every round {residual[True]}")
    assert residual[True] < residual[False]
    assert 2 * residual[True] < residual[False]  # a clear gap, not a tie broken by chance


# ---- overwrite mode, layer subsets -----------------------------------------------------------

@pytest.mark.parametrize("codec", ["hamming84", "golay_packed"])
def test_overwrite_mode_scrubs_sequence_zero(be, oracle, codec):
    from kvecc.ecc_shim import age_ecc_cache, reset_ecc_cache, scrub_ecc_cache
    backend, dev = be
    model, ctx = _patched("gpt2", _cfg(codec, backend, mode="overwrite"), dev)
    with torch.no_grad(), ctx:
        reset_ecc_cache(model)
        model(_ids()[:1, :PREFILL].to(dev))
        mgr = model._ecc_block_manager
        nl = mgr.num_layers
        valid = _valid(mgr.block_table[:1].cpu().numpy(), [[PREFILL]] * nl, 0, nl, mgr.num_blocks, nl, mgr.num_kv_heads, BS)
        aged = _age_np(oracle, _np(mgr), codec, 2e-2, 3)
        age_ecc_cache(model, 2e-2, 3)
        want = [_expect(oracle, codec, D, c, valid) for c in aged]
        got = scrub_ecc_cache(model)
        for (w, _), b in zip(want, _np(mgr)):
            assert np.array_equal(w, b)
        tot = [sum(s[k] for _, s in want) for k in range(4)]
        assert got == dict(zip(("corrected", "detected", "rewritten", "scanned"), tot)) and tot[2] > 0


@pytest.mark.parametrize("layers", [[1], [0], range(0, 2), 1])
def test_layer_subset(be, oracle, layers):
    from kvecc.ecc_shim import age_ecc_cache, scrub_ecc_cache
    backend, dev = be
    codec = "golay"
    model, ctx = _patched("llama", _cfg(codec, backend), dev)
    with torch.no_grad(), ctx:
        _fill(model, dev)
        mgr = model._ecc_block_manager
        aged = _age_np(oracle, _np(mgr), codec, 1e-2, 9)
        age_ecc_cache(model, 1e-2, 9)
        valid = _mask(mgr, layers=[layers] if isinstance(layers, int) else list(layers))
        want = [_expect(oracle, codec, D, c, valid) for c in aged]
        got = scrub_ecc_cache(model, layers=layers)
        for (w, _), b in zip(want, _np(mgr)):
            assert np.array_equal(w, b)
        assert got["scanned"] == sum(s[3] for _, s in want) and got["rewritten"] == sum(s[2] for _, s in want) > 0
    with torch.no_grad(), _patched("llama", _cfg(codec, backend), dev)[1] as m2:
        with pytest.raises(ValueError):
            scrub_ecc_cache(m2, layers=[2])


# ---- errors, counters --------------------------------------------------------------------------

@pytest.mark.parametrize("codec", ["fp16", "fp8", "int4"])
def test_codecs_without_ecc_raise(codec):
    from kvecc.ecc_shim import ECCShimConfig, age_ecc_cache, patch_model_with_ecc_attention, scrub_ecc_cache
    model = MODELS["gpt2"]()
    with patch_model_with_ecc_attention(model, ECCShimConfig(codec=codec, backend="cpu", block_size=BS), num_blocks=NBLK):
        with pytest.raises(ValueError):
            scrub_ecc_cache(model)
        with pytest.raises(ValueError):
            age_ecc_cache(model, 1e-2, 0)
    with pytest.raises(ValueError):
        scrub_ecc_cache(model)  # not patched


def test_scrub_counters_are_their_own(be):
    """Scrub counts go to a buffer of their own: get_ecc_stats is unchanged by a scrub (and by
    ageing), and reset_ecc_cache clears the cumulative scrub counters."""
    from kvecc.ecc_shim import age_ecc_cache, get_ecc_stats, reset_ecc_cache, scrub_ecc_cache
    backend, dev = be
    model, ctx = _patched("gpt2", _cfg("hamming84", backend), dev)
    with torch.no_grad(), ctx:
        _fill(model, dev)
        base = get_ecc_stats(model)
        age_ecc_cache(model, 2e-2, 1)
        a = scrub_ecc_cache(model)
        b = scrub_ecc_cache(model)
        assert a["rewritten"] > 0 and a["corrected"] > 0 and a["detected"] > 0
        assert b["rewritten"] == 0 and b["detected"] == a["detected"] and b["scanned"] == a["scanned"]
        assert get_ecc_stats(model) == base
        tot = model._ecc_backend.scrub_totals().tolist()
        assert tot == [a[k] + b[k] for k in ("corrected", "detected", "rewritten", "scanned")]
        reset_ecc_cache(model)
        assert model._ecc_backend.scrub_totals().tolist() == [0, 0, 0, 0]
        assert scrub_ecc_cache(model) == {"corrected": 0, "detected": 0, "rewritten": 0, "scanned": 0}


@pytest.mark.gpu
@pytest.mark.parametrize("codec", ["hamming84", "golay_packed"])
def test_scrub_launch_replays_in_a_hip_graph(gpu, oracle, codec):
    """ECCBackend.scrub reads nothing back and copies nothing from the host: captured once, every
    replay scrubs whatever the cache then holds and adds into the scrub counters."""
    from kvecc.ecc_shim import age_ecc_cache
    model, ctx = _patched("gpt2", _cfg(codec, "hip"), gpu)
    with torch.no_grad(), ctx:
        _fill(model, gpu)
        be_, mgr = model._ecc_backend, model._ecc_block_manager
        valid = _mask(mgr)
        be_.scrub()  # allocates the counters, outside the capture
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            be_.scrub()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            be_.scrub()
        base = be_.scrub_totals().tolist()
        for r in range(2):
            aged = _age_np(oracle, _np(mgr), codec, 5e-3, 40 + r)
            age_ecc_cache(model, 5e-3, 40 + r)
            want = [_expect(oracle, codec, D, c, valid) for c in aged]
            g.replay()
            torch.cuda.synchronize()
            for (w, _), b in zip(want, _np(mgr)):
                assert np.array_equal(w, b)
            tot = be_.scrub_totals().tolist()
            assert [t - b for t, b in zip(tot, base)] == [sum(s[k] for _, s in want) for k in range(4)]
            base = tot
