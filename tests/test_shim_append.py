"""Append-mode cache write (kvecc_shim_append / kvecc_cpu_shim_append) at the ops level.

Every sequence of a batch writes through its own block-table row, behind its
own start position.  The anchor is the existing write: sequence b of an append
at start_pos 0 must hold the bits kvecc_shim_write stores for a batch of b + 1
(same quantization, encoding, seeds), and that write is pinned to the
reference's fixtures elsewhere (tests/test_shim.py).

Grid: block_size 4, 2 layers (layer 1 written), 3 KV heads, head_dim 128 and 20
(Golay's zero padding to 21), every shim codec, fp32 / fp16 / bf16, batch 3 at
start positions [0, 3, 6] (6 or 18 rows per side: not a multiple of the
workgroup's waves; tokens 3..5 straddle a block boundary), q_len 1 and 3,
shuffled non-contiguous physical block ids, injection on (BER 5e-2) and off.
The host twin runs everywhere, the HIP kernel under the gpu marker.
"""

import pytest
import torch

BS, NL, LAYER, HKV = 4, 2, 1, 3
NBLOCKS, NPER = 16, 3           # physical blocks; table entries per sequence
START = [0, 3, 6]
BER, SEED0 = 5e-2, 1234
CODECS = ["int4", "hamming74", "hamming84", "golay", "golay_packed"]
N_BITS = {"int4": 4, "hamming74": 7, "hamming84": 8, "golay": 24, "golay_packed": 24}
DTYPES = [torch.float32, torch.float16, torch.bfloat16]

GRID = [(codec, d, dt, q, inj) for codec in CODECS for d in (128, 20) for dt in DTYPES for q in (1, 3)
        for inj in (True, False)]
GRID_IDS = [f"{c}-d{d}-{str(dt)[6:]}-q{q}-{'inj' if inj else 'clean'}" for c, d, dt, q, inj in GRID]


@pytest.fixture(params=["cpu", pytest.param("hip", marks=pytest.mark.gpu)])
def be(request):
    """(backend module, device) of the host twin / the HIP kernels."""
    if request.param == "cpu":
        from kvecc import cpu_ops
        return cpu_ops, torch.device("cpu")
    from kvecc import ops
    return ops, request.getfixturevalue("gpu")


def _row_words(codec, d):
    g = (d + 2) // 3
    return {"golay": g, "golay_packed": (3 * g + 3) // 4 * 4}.get(codec, d)


def _written_words(codec, d):
    """Words of a token row a write touches (packed rows end in untouched padding)."""
    return 3 * ((d + 2) // 3) if codec == "golay_packed" else _row_words(codec, d)


def _caches(codec, d, device, sentinel=False):
    per = _row_words(codec, d)
    dt = torch.int32 if codec == "golay" else torch.uint8
    fill = (0x5A5A5A5A if dt == torch.int32 else 0xA5) if sentinel else 0
    return [torch.full((NBLOCKS, NL, HKV, BS * per), fill, dtype=dt, device=device),
            torch.full((NBLOCKS, NL, HKV, BS * per), fill, dtype=dt, device=device),
            torch.full((NBLOCKS, NL, HKV, BS), -3.0 if sentinel else 0.0, device=device),
            torch.full((NBLOCKS, NL, HKV, BS), -3.0 if sentinel else 0.0, device=device)]


def _tables(batch, device):
    perm = torch.randperm(NBLOCKS, generator=torch.Generator().manual_seed(5))[:batch * NPER]
    return perm.view(batch, NPER).to(torch.int32).to(device)


def _kv(batch, q_len, d, dtype, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(batch, q_len, HKV, d, generator=g).to(dtype).to(device)
    v = (2 * torch.randn(batch, q_len, HKV, d, generator=g)).to(dtype).to(device)
    return k, v


def _append(mod, k, v, caches, table, start, codec, d, inject, **kw):
    mod.shim_append_tensors(k, v, *caches, table, start, NL, BS, HKV, d, LAYER, codec, N_BITS[codec], inject, BER,
                            SEED0, **kw)


def _rows(cache, table_row, positions, per):
    """Rows [len(positions), HKV, per] of layer LAYER through one block-table row."""
    pos = torch.as_tensor(positions, dtype=torch.long, device=cache.device)
    blk = table_row.to(torch.long)[pos // BS]
    return cache.view(NBLOCKS, NL, HKV, BS, per)[blk, LAYER, :, pos % BS, :]


def _target_mask(table, start, q_len, device, skipped=()):
    """[blocks, NL, HKV, BS] mask of the slots an append writes."""
    m = torch.zeros(NBLOCKS, NL, HKV, BS, dtype=torch.bool, device=device)
    tab = table.cpu().tolist()
    for b, s in enumerate(start):
        for t in range(q_len):
            if (b, t) not in skipped:
                m[tab[b][(s + t) // BS], LAYER, :, (s + t) % BS] = True
    return m


def _i32(x, device):
    return torch.tensor(x, dtype=torch.int32, device=device)


# ---- 1. anchored to the existing write --------------------------------------------
@pytest.mark.parametrize("codec,d,dtype,q_len,inject", GRID, ids=GRID_IDS)
def test_append_matches_shim_write(be, codec, d, dtype, q_len, inject):
    mod, dev = be
    k, v = _kv(3, q_len, d, dtype, dev)
    table, caches = _tables(3, dev), _caches(codec, d, dev)
    _append(mod, k, v, caches, table, _i32(START, dev), codec, d, inject)
    per = _row_words(codec, d)
    straight = torch.arange(NBLOCKS, dtype=torch.int32, device=dev)
    for b in range(3):
        scratch = _caches(codec, d, dev)
        mod.shim_write_tensors(k[:b + 1], v[:b + 1], *scratch, straight, NL, BS, HKV, d, LAYER, codec,
                               N_BITS[codec], inject, BER, SEED0)
        there = range(START[b], START[b] + q_len)
        for got, want, w in zip(caches, scratch, (per, per, 1, 1)):
            assert torch.equal(_rows(got, table[b], there, w), _rows(want, straight, range(q_len), w)), b


# ---- 2. growth equals one shot ---------------------------------------------------
@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("d,dtype", [(128, torch.float16), (20, torch.float32), (128, torch.bfloat16)])
def test_growth_equals_one_shot(be, codec, d, dtype):
    from kvecc.ecc_shim import SimpleBlockManager
    mod, dev = be
    storage = "packed" if codec == "golay_packed" else "int32"
    mk = lambda: SimpleBlockManager(8, BS, NL, HKV, d, device=dev, codec=codec.replace("_packed", ""),
                                    golay_storage=storage)
    one, grown = mk(), mk()
    k, v = _kv(1, 11, d, dtype, dev, seed=3)
    one.allocate(0, 11)
    mod.shim_write(k, v, one, LAYER, codec, N_BITS[codec], False, 0.0, SEED0)
    at = 0
    for n in (5, 1, 1, 1, 1, 1, 1):
        grown.extend(0, at + n)
        mod.shim_append_tensors(k[:, at:at + n], v[:, at:at + n], grown.k_cache, grown.v_cache, grown.k_scales,
                                grown.v_scales, grown.block_table[:1], grown.ctx_lens[LAYER, :1], NL, BS, HKV, d,
                                LAYER, codec, N_BITS[codec], False, 0.0, SEED0)
        grown.advance(LAYER, 1, n)
        at += n
    assert grown.layer_lens(LAYER, 1) == [11] and grown.ctx_lens[LAYER, 0].item() == 11
    assert grown.ctx_lens[0, 0].item() == 0  # the other layer's length is its own
    assert torch.equal(one.block_table, grown.block_table)
    for name in ("k_cache", "v_cache", "k_scales", "v_scales"):
        assert torch.equal(getattr(one, name), getattr(grown, name)), name


# ---- 3. nothing else is touched ----------------------------------------------------
@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("d,q_len", [(128, 3), (20, 1)])
def test_only_target_rows_change(be, codec, d, q_len):
    mod, dev = be
    k, v = _kv(3, q_len, d, torch.float16, dev)
    table = _tables(3, dev)
    clean, marked, untouched = _caches(codec, d, dev), _caches(codec, d, dev, True), _caches(codec, d, dev, True)
    _append(mod, k, v, clean, table, _i32(START, dev), codec, d, True)
    _append(mod, k, v, marked, table, _i32(START, dev), codec, d, True)
    _check_targets(marked, clean, untouched, _target_mask(table, START, q_len, dev), codec, d)


def _check_targets(got, want, untouched, mask, codec, d):
    """Target slots of `got` hold `want`'s bits, everything else `untouched`'s:
    other layers, other blocks, a packed row's padding bytes."""
    per, wr = _row_words(codec, d), _written_words(codec, d)
    for g, w, u in zip(got[:2], want[:2], untouched[:2]):
        g5, w5, u5 = (x.view(NBLOCKS, NL, HKV, BS, per) for x in (g, w, u))
        assert torch.equal(g5[mask][:, :wr], w5[mask][:, :wr])
        assert torch.equal(g5[mask][:, wr:], u5[mask][:, wr:])
        assert torch.equal(g5[~mask], u5[~mask])
    for g, w, u in zip(got[2:], want[2:], untouched[2:]):
        assert torch.equal(g[mask], w[mask]) and torch.equal(g[~mask], u[~mask])


# ---- 4. skip rules -----------------------------------------------------------------
@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("rule", ["inactive", "no_block", "no_block_partial", "past_table"])
@pytest.mark.parametrize("q_len", [1, 3])
def test_skipped_rows(be, codec, rule, q_len):
    """Sequence 1 is skipped (wholly, or its tokens in the missing block); the
    others are written with the seeds they have when nothing is skipped."""
    mod, dev = be
    d = 20
    k, v = _kv(3, q_len, d, torch.bfloat16, dev)
    table, start = _tables(3, dev), list(START)
    clean = _caches(codec, d, dev)
    _append(mod, k, v, clean, table, _i32(start, dev), codec, d, True)
    skipped = {(1, t) for t in range(q_len)}
    table2 = table.clone()
    if rule == "inactive":
        start[1] = -1
    elif rule == "no_block":
        table2[1, :] = -1
    elif rule == "no_block_partial":  # position 3 is in logical block 0, 4 and 5 in block 1
        table2[1, 1] = -1
        skipped = {(1, t) for t in range(q_len) if (START[1] + t) // BS == 1}
    else:
        start[1] = NPER * BS
    marked, untouched = _caches(codec, d, dev, True), _caches(codec, d, dev, True)
    _append(mod, k, v, marked, table2, _i32(start, dev), codec, d, True)
    _check_targets(marked, clean, untouched, _target_mask(table, START, q_len, dev, skipped), codec, d)


# ---- 5. strided input ----------------------------------------------------------------
@pytest.mark.parametrize("codec", ["hamming84", "golay", "golay_packed"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_input(be, codec, dtype):
    mod, dev = be
    d, q_len = 128, 3
    k, v = _kv(3, q_len, d, dtype, dev)
    kt = k.transpose(1, 2).contiguous().transpose(1, 2)  # [b, h, s, d] storage, seen as [b, s, h, d]
    vt = v.transpose(1, 2).contiguous().transpose(1, 2)
    assert not kt.is_contiguous()
    table = _tables(3, dev)
    a, b = _caches(codec, d, dev), _caches(codec, d, dev)
    _append(mod, k, v, a, table, _i32(START, dev), codec, d, True)
    _append(mod, kt, vt, b, table, _i32(START, dev), codec, d, True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- 6. HIP equals the host twin --------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("codec,d,dtype,q_len,inject", GRID, ids=GRID_IDS)
def test_hip_equals_host_twin(gpu, codec, d, dtype, q_len, inject):
    from kvecc import cpu_ops, ops
    k, v = _kv(3, q_len, d, dtype, "cpu")
    table = _tables(3, "cpu")
    host, hip = _caches(codec, d, "cpu", True), _caches(codec, d, gpu, True)
    _append(cpu_ops, k, v, host, table, _i32(START, "cpu"), codec, d, inject, scale_rule="mul_inv7")
    _append(ops, k.to(gpu), v.to(gpu), hip, table.to(gpu), _i32(START, gpu), codec, d, inject,
            scale_rule="mul_inv7")
    for x, y in zip(host, hip):
        assert torch.equal(x, y.cpu())


# ---- 7. wrapper validation -----------------------------------------------------------------
def test_wrapper_validation(be):
    mod, dev = be
    d, codec = 128, "hamming84"
    other = torch.device("cpu") if dev.type != "cpu" else torch.device("meta")
    k, v = _kv(3, 1, d, torch.float16, dev)
    table, start = _tables(3, dev), _i32(START, dev)
    caches, before = _caches(codec, d, dev, True), _caches(codec, d, dev, True)
    wide = torch.zeros(3, 2 * NPER, dtype=torch.int32, device=dev)
    bad = {
        "cache dtype": dict(caches=[caches[0].view(torch.int8), caches[1].view(torch.int8)] + caches[2:]),
        "golay cache for a byte codec": dict(caches=_caches("golay", d, dev)),
        "short scales": dict(caches=caches[:2] + [caches[2][:-1], caches[3]]),
        "start_pos dtype": dict(start=start.to(torch.int64)),
        "start_pos length": dict(start=_i32(START + [0], dev)),
        "start_pos device": dict(start=start.to(other)),
        "cache device": dict(caches=[caches[0].to(other)] + caches[1:]),
        "table stride": dict(table=wide[:, ::2]),
        "table rows": dict(table=table[:2]),
        "table dtype": dict(table=table.to(torch.int64)),
    }
    for what, kw in bad.items():
        args = dict(caches=caches, table=table, start=start)
        args.update(kw)
        with pytest.raises(ValueError):
            _append(mod, k, v, args["caches"], args["table"], args["start"], codec, d, True)
            pytest.fail(what)
    for x, y in zip(caches, before):
        assert torch.equal(x, y)
    _append(mod, k, v, caches, table, start, codec, d, True)  # and the good call goes through
    assert not torch.equal(caches[0], before[0])


# ---- 8. dispatcher operator ------------------------------------------------------------------
@pytest.mark.parametrize("codec", ["hamming74", "golay_packed"])
def test_dispatcher_op_cpu(codec):
    from kvecc import cpu_ops, torch_ops
    assert "shim_append" in torch_ops.OPS
    d = 20
    k, v = _kv(3, 3, d, torch.float32, "cpu")
    table, start = _tables(3, "cpu"), _i32(START, "cpu")
    a, b = _caches(codec, d, "cpu"), _caches(codec, d, "cpu")
    _append(cpu_ops, k, v, a, table, start, codec, d, True)
    torch.ops.kvecc.shim_append(k, v, *b, table, start, NL, BS, HKV, d, LAYER, codec, N_BITS[codec], True, BER,
                                SEED0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert a[0].any()


@pytest.mark.gpu
def test_dispatcher_op_compiles_hip(gpu):
    codec, d = "golay", 128
    k, v = _kv(3, 3, d, torch.float16, gpu)
    table, start = _tables(3, gpu), _i32(START, gpu)

    def step(k, v, kc, vc, ks, vs, table, start):
        torch.ops.kvecc.shim_append(k * 1.0, v, kc, vc, ks, vs, table, start, NL, BS, HKV, d, LAYER, codec,
                                    N_BITS[codec], True, BER, SEED0)
        return start + k.shape[1]

    eager, comp = _caches(codec, d, gpu), _caches(codec, d, gpu)
    nxt_e = step(k, v, *eager, table, start)
    torch._dynamo.reset()
    nxt_c = torch.compile(step, fullgraph=True)(k, v, *comp, table, start)
    assert torch.equal(nxt_e, nxt_c)
    for x, y in zip(eager, comp):
        assert torch.equal(x, y)
    assert eager[0].any()
