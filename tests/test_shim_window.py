"""ECCShimConfig(attention_window, attention_sinks, evict_blocks): sliding-window attention and
block eviction through a patched append-mode model.

Models: the random-init 2-layer GPT-2 (4 heads) and LLaMA (4 query / 2 KV heads) of
tests/test_shim_chunk.py and tests/test_shim_llama.py, head_dim 32.  Schedule: batch 2, a 20-token
prompt (ragged: 20 and 13 tokens, right-padded, held as query spans) and single-token steps with
explicit position_ids; block_size 8.  Every case runs on the cpu backend and, marked gpu, on hip.

  (i)   a window larger than the run: hamming84 / golay logits are bit for bit those of the same
        config without a window on the kernel path (chunk_attention: the windowed entry forwards to
        the plain one); hamming74 / int4 are within the shim tolerance of the unwindowed read + SDPA.
  (ii)  W 24, S 4, 60 steps: per-step logits with evict_blocks=True are bit for bit those without.
  (iii) a pool the unevicted run overflows: `Out of blocks` without eviction, a finished run with it;
        what was released is what the rule (from the host lengths) releases, never a sink block or a
        block inside a window; the free list is sorted; evict_ecc_cache reports its blocks.
  (iv)  scrub_ecc_cache and age_ecc_cache on the holed cache: the scrub scans the resident tokens' words.
  (v)   the illegal flag combinations raise ValueError.
"""

import pytest
import torch
import torch.nn.functional as F

from tests.test_shim_chunk import _gpt2
from tests.test_shim_llama import LOGIT_ATOL, _llama

BS, D, LAYERS = 8, 32, 2
PROMPT, SHORT, STEPS = 20, 13, 60
W, S = 24, 4
MODELS = {"gpt2": _gpt2, "llama": lambda: _llama()[0]}
HKV = {"gpt2": 4, "llama": 2}


@pytest.fixture(params=["cpu", pytest.param("hip", marks=pytest.mark.gpu)])
def be(request):
    """(backend name, device)."""
    if request.param == "cpu":
        return "cpu", torch.device("cpu")
    return "hip", request.getfixturevalue("gpu")


def _cfg(codec, backend, window=0, sinks=0, evict=False, ber=1e-2, **kw):
    from kvecc.ecc_shim import ECCShimConfig
    storage = "packed" if codec == "golay_packed" else "int32"
    return ECCShimConfig(codec=codec.replace("_packed", ""), ber=ber, inject_errors=ber > 0, seed=42, block_size=BS,
                         backend=backend, golay_storage=storage, cache_mode="append", attention_window=window,
                         attention_sinks=sinks, evict_blocks=evict, **kw)


def _tokens(steps):
    g = torch.Generator().manual_seed(11)
    return torch.randint(1, 101, (2, PROMPT), generator=g), torch.randint(1, 101, (2, steps), generator=g)


def _generate(model, cfg, dev, num_blocks, steps=STEPS, ragged=False, each=None):
    """Prefill + `steps` single-token forwards on a fresh patched model -> the valid logits of every
    forward, concatenated per sequence; each(model, step) runs after every forward, inside the patch."""
    from kvecc.ecc_shim import patch_model_with_ecc_attention, reset_ecc_cache, set_ecc_query_spans
    ids, nxt = _tokens(steps)
    lens = [PROMPT, SHORT if ragged else PROMPT]
    outs = [[], []]
    with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=num_blocks):
        reset_ecc_cache(model)
        if ragged:
            set_ecc_query_spans(model, lens)
        pos = torch.arange(PROMPT).unsqueeze(0).expand(2, -1)
        logits = model(ids.to(dev), position_ids=pos.to(dev)).logits.float().cpu()
        for b in range(2):
            outs[b].append(logits[b, :lens[b]])
        if each is not None:
            each(model, -1)
        if ragged:
            set_ecc_query_spans(model, [1, 1])
        for s in range(steps):
            p = torch.tensor(lens).view(2, 1)
            logits = model(nxt[:, s:s + 1].to(dev), position_ids=p.to(dev)).logits.float().cpu()
            for b in range(2):
                outs[b].append(logits[b])
                lens[b] += 1
            if each is not None:
                each(model, s)
    return [torch.cat(o) for o in outs]


# ---- (v) the config ------------------------------------------------------------------------------
def test_flag_combinations():
    from kvecc.ecc_shim import ECCShimConfig
    ok = ECCShimConfig(codec="golay", cache_mode="append", attention_window=16, attention_sinks=2, evict_blocks=True)
    assert (ok.attention_window, ok.attention_sinks, ok.evict_blocks) == (16, 2, True)
    d = ECCShimConfig()
    assert (d.attention_window, d.attention_sinks, d.evict_blocks) == (0, 0, False)
    a = dict(cache_mode="append", attention_window=16)
    bad = [dict(attention_window=16),  # overwrite mode
           dict(a, use_interpolation=True), dict(a, decode_stats=True),
           dict(a, use_interpolation=True, interp_attention=True), dict(a, stats_attention=True),
           dict(a, counted_attention=True), dict(a, repair_attention=True),
           dict(a, codec="golay", counted_attention=True),
           dict(cache_mode="append", evict_blocks=True),  # no window
           dict(cache_mode="append", attention_window=-1), dict(a, attention_sinks=-2),
           dict(cache_mode="append", attention_window=1.5), dict(cache_mode="append", attention_window=True)]
    for kw in bad:
        with pytest.raises(ValueError):
            ECCShimConfig(**kw)
    for codec in ("int4", "hamming74", "hamming84", "golay"):  # all four append codecs
        ECCShimConfig(codec=codec, **a)
    ECCShimConfig(codec="hamming74", kernel_attention=True, chunk_attention=True, **a)
    ECCShimConfig(cache_mode="append", attention_sinks=3)  # sinks without a window: ignored


def test_eviction_needs_a_window_and_a_patched_model():
    from kvecc.ecc_shim import evict_ecc_cache, patch_model_with_ecc_attention
    model = _gpt2()
    with pytest.raises(ValueError):
        evict_ecc_cache(model)
    with torch.no_grad(), patch_model_with_ecc_attention(model, _cfg("hamming84", "cpu"), num_blocks=8):
        with pytest.raises(ValueError):
            evict_ecc_cache(model)


# ---- (i) a window larger than the run ----------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("codec", ["hamming84", "golay", "golay_packed"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_covering_window_is_the_kernel_path(be, name, codec, ragged):
    backend, dev = be
    model = MODELS[name]().to(dev)
    plain = _generate(model, _cfg(codec, backend, chunk_attention=True), dev, 32, steps=12, ragged=ragged)
    for w, s in ((1000, 0), (PROMPT + 12, 5)):
        got = _generate(model, _cfg(codec, backend, w, s), dev, 32, steps=12, ragged=ragged)
        for b in range(2):
            assert torch.equal(got[b], plain[b]), (w, s, b)


@pytest.mark.parametrize("codec", ["hamming74", "int4"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_covering_window_is_close_to_read_and_sdpa(be, name, codec):
    backend, dev = be
    model = MODELS[name]().to(dev)
    plain = _generate(model, _cfg(codec, backend), dev, 32, steps=12, ragged=True)
    got = _generate(model, _cfg(codec, backend, 1000, 3), dev, 32, steps=12, ragged=True)
    for b in range(2):
        err = float((got[b] - plain[b]).abs().max())
        print(f"{name} {codec} sequence {b}: max logit err {err:.3e}")
        assert err <= LOGIT_ATOL, (b, err)


def test_a_real_window_changes_the_logits_only_past_it():
    """The window is applied: with W = 24 and no sinks the logits of positions < 24 are the unwindowed
    kernel path's, bit for bit (up to a length of W the call is forwarded to the plain entry), and later
    ones differ."""
    model = MODELS["llama"]()
    plain = _generate(model, _cfg("hamming84", "cpu", chunk_attention=True), torch.device("cpu"), 32, steps=12)
    got = _generate(model, _cfg("hamming84", "cpu", W, 0), torch.device("cpu"), 32, steps=12)
    for b in range(2):
        assert not torch.equal(got[b][W:], plain[b][W:])
        assert torch.equal(got[b][:W], plain[b][:W])


# ---- (ii) eviction changes no logit ------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("codec", ["hamming84", "golay_packed", "hamming74"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_eviction_is_bit_equal(be, name, codec, ragged):
    backend, dev = be
    model = MODELS[name]().to(dev)
    kept = _generate(model, _cfg(codec, backend, W, S), dev, 32, ragged=ragged)
    gone = _generate(model, _cfg(codec, backend, W, S, evict=True), dev, 32, ragged=ragged)
    for b in range(2):
        assert bool(gone[b].isfinite().all())
        assert torch.equal(gone[b], kept[b]), b


# ---- (iii) the pool, the rule, the free list -----------------------------------------------------
def _releasable(length, w, s):
    """The rule, restated: logical blocks lb with lb * bs >= S and (lb + 1) * bs - 1 <= Lmin - W."""
    return {lb for lb in range(-(-length // BS)) if lb * BS >= s and (lb + 1) * BS - 1 <= length - w}


def _check_manager(mgr, before_last):
    """The manager's state after a forward against the rule from the host lengths: everything releasable
    before the last forward (lengths `before_last`) is gone, nothing beyond the rule at the lengths now."""
    resident = []
    for seq, blocks in mgr.seq_to_blocks.items():
        lens = [mgr.layer_lens(layer, seq + 1)[seq] for layer in range(mgr.num_layers)]
        assert len(set(lens)) == 1 and len(blocks) == -(-lens[0] // BS)  # logical positions kept
        gone = {lb for lb, x in enumerate(blocks) if x < 0}
        assert _releasable(before_last[seq], W, S) <= gone <= _releasable(min(lens), W, S), seq
        for lb in gone:  # no sink block, no block that meets the window of any position from min(lens) on
            assert lb * BS >= S and (lb + 1) * BS - 1 <= min(lens) - W
        assert mgr.block_table[seq, :len(blocks)].cpu().tolist() == blocks
        assert mgr._host_table[seq] == blocks
        resident += [x for x in blocks if x >= 0]
    assert mgr.free_blocks == sorted(mgr.free_blocks)
    assert sorted(resident + mgr.free_blocks) == list(range(mgr.num_blocks))  # nothing lost, nothing twice
    return resident


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_eviction_bounds_the_pool(be, name, ragged):
    from kvecc.ecc_shim import get_ecc_stats
    backend, dev = be
    model = MODELS[name]().to(dev)
    total = [PROMPT + STEPS, (SHORT if ragged else PROMPT) + STEPS]
    pool = 14
    assert sum(-(-n // BS) for n in total) > pool  # resident need without eviction
    with pytest.raises(RuntimeError, match="Out of blocks"):
        _generate(model, _cfg("hamming84", backend, W, S), dev, pool, ragged=ragged)
    prompts = [PROMPT, SHORT if ragged else PROMPT]
    peak = []

    def each(model, step):  # after the prefill (step -1) and after every step
        before = [n + step for n in prompts] if step >= 0 else [0, 0]  # the lengths the forward's eviction saw
        resident = _check_manager(model._ecc_block_manager, before)
        peak.append(len(resident))
        assert get_ecc_stats(model)["allocated_blocks"] == len(resident)

    got =_generate(model, _cfg("hamming84", backend, W, S, evict=True), dev, pool, ragged=ragged, each=each)
    assert all(bool(g.isfinite().all()) for g in got)
    # about S + W tokens per sequence: the sink block, the window's blocks and the one being filled
    assert max(peak) <= 2 * (-(-S // BS) + W // BS + 2) <= pool


def test_evict_ecc_cache_reports_its_blocks(be):
    from kvecc.ecc_shim import evict_ecc_cache
    backend, dev = be
    model = MODELS["llama"]().to(dev)
    seen = []

    def each(model, step):
        if step in (9, 39):  # lengths 30 and 60: nothing to give at first, then blocks 1..3 (tokens 8..31 <= 60 - 24)
            mgr = model._ecc_block_manager
            free = len(mgr.free_blocks)
            n = evict_ecc_cache(model)
            seen.append(n)
            assert len(mgr.free_blocks) == free + n and mgr.free_blocks == sorted(mgr.free_blocks)
            assert evict_ecc_cache(model) == 0  # nothing more until the sequences grow
            for seq in (0, 1):
                gone = {lb for lb, x in enumerate(mgr.seq_to_blocks[seq]) if x < 0}
                assert gone == _releasable(PROMPT + step + 1, W, S)
                assert bool((mgr.block_table[seq, sorted(gone)] == -1).all()) if gone else True
            # a released block is zeroed, as free() leaves it
            idx = torch.tensor(mgr.free_blocks, device=mgr.k_cache.device)
            assert not bool(mgr.k_cache[idx].any()) and not bool(mgr.v_scales[idx].any())

    kept = _generate(model, _cfg("hamming84", backend, W, S, ber=0.0), dev, 32, steps=45)
    got = _generate(model, _cfg("hamming84", backend, W, S, ber=0.0), dev, 32, steps=45, each=each)
    assert seen == [0, 2 * 3]
    for b in range(2):
        assert torch.equal(got[b], kept[b])  # the manual eviction changed no logit either


def test_a_refused_forward_releases_nothing():
    """At length 39 logical block 1 (tokens 8..15 <= 39 - 24) has become releasable.  A forward that the
    span check refuses must not have evicted it; the next good forward does."""
    from kvecc.ecc_shim import set_ecc_query_spans
    model = MODELS["llama"]()
    seen = []

    def each(model, step):
        mgr = model._ecc_block_manager
        if step == 18:
            assert _releasable(39, W, S) == {1} and mgr.seq_to_blocks[0][1] >= 0
            free = list(mgr.free_blocks)
            set_ecc_query_spans(model, [1])  # a batch of 1 held for a forward of 2
            with pytest.raises(ValueError):
                model(torch.ones(2, 1, dtype=torch.long), position_ids=torch.full((2, 1), 39))
            assert mgr.free_blocks == free and mgr.seq_to_blocks[0][1] >= 0 and mgr.layer_lens(0, 2) == [39, 39]
            set_ecc_query_spans(model, None)
            seen.append(step)
        if step == 19:
            assert mgr.seq_to_blocks[0][1] == -1 and mgr.seq_to_blocks[1][1] == -1
            seen.append(step)

    _generate(model, _cfg("hamming84", "cpu", W, S, evict=True), torch.device("cpu"), 32, steps=21, each=each)
    assert seen == [18, 19]


# ---- (iv) the scrubber and ageing on a cache with holes -----------------------------------------
@pytest.mark.parametrize("codec", ["hamming84", "golay_packed"])
def test_scrub_and_age_on_the_holed_cache(be, codec):
    from kvecc.ecc_shim import age_ecc_cache, scrub_ecc_cache
    backend, dev = be
    model = MODELS["llama"]().to(dev)
    words = D if codec == "hamming84" else (D + 2) // 3
    checked = []

    def each(model, step):
        if step != 49:
            return
        mgr = model._ecc_block_manager
        tokens = 0
        for seq, blocks in mgr.seq_to_blocks.items():
            n = mgr.layer_lens(0, seq + 1)[seq]
            assert any(x < 0 for x in blocks)
            tokens += sum(min(BS, n - lb * BS) for lb, x in enumerate(blocks) if x >= 0)
        first = scrub_ecc_cache(model)
        assert first["scanned"] == 2 * LAYERS * HKV["llama"] * tokens * words  # K and V, the resident tokens only
        assert scrub_ecc_cache(model)["rewritten"] == 0
        age_ecc_cache(model, 2e-3, 5)
        aged = scrub_ecc_cache(model)
        assert aged["scanned"] == first["scanned"] and aged["corrected"] > 0 and aged["rewritten"] > 0
        checked.append(step)

    got = _generate(model, _cfg(codec, backend, W, S, evict=True, ber=0.0), dev, 14, ragged=True, each=each)
    assert checked == [49] and all(bool(g.isfinite().all()) for g in got)


# ---- head_dim > 256: the rule in the read + SDPA mask ----------------------------------------------
def test_wide_heads_apply_the_rule_in_the_mask(be):
    from kvecc.ecc_shim import ECCBackend, SimpleBlockManager
    backend, dev = be
    d, n, t = 260, 40, 5
    g = torch.Generator().manual_seed(3)
    k, v = torch.randn(2, 1, n, 1, d, generator=g).to(dev)
    q = torch.randn(1, 1, t, d, generator=g).to(dev)
    outs = {}
    for w, s in ((0, 0), (8, 2)):
        mgr = SimpleBlockManager(8, 16, 1, 1, d, device=dev, codec="hamming84")
        eb = ECCBackend(mgr, _cfg("hamming84", backend, w, s, ber=0.0), num_heads=1)
        eb._append_write(k, v, 0)
        outs[w] = eb._append_attend(q, 0)
        if w == 0:
            k_t, v_t = eb.codec_backend.shim_read_batch(mgr.k_cache, mgr.v_cache, mgr.k_scales, mgr.v_scales,
                                                        mgr.block_table[:1], n, d, 0, "hamming84", q.dtype)
    keys, qpos = torch.arange(n, device=dev).view(1, n), (n - t + torch.arange(t, device=dev)).view(t, 1)
    for w, s in ((0, 0), (8, 2)):
        mask = keys <= qpos
        if w:
            mask = mask & ((keys > qpos - w) | (keys < s))
            assert [int(x) for x in mask.sum(1)] == [w + s] * t
        want = F.scaled_dot_product_attention(q, k_t, v_t, attn_mask=mask.view(1, 1, t, n))
        assert torch.allclose(outs[w], want, atol=1e-5, rtol=1e-5), w
    assert not torch.allclose(outs[0], outs[8], atol=1e-3)
