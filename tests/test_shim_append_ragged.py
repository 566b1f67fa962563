"""Ragged append (kvecc_shim_append_ragged / kvecc_cpu_shim_append_ragged) at the ops level.

Contract (include/kvecc.h, "Query spans"): q_spans[b] = (first, count, row_base); valid token t of
sequence b goes to start_pos[b] + (t - first) under the injection row (row_base + t - first) * hkv
+ h, dense over the valid tokens; a padding token writes nothing and is never loaded.  Two
properties pin every bit to the uniform append (itself anchored to kvecc_shim_write in
tests/test_shim_append.py):
  1. all spans (0, q_max, b * q_max) write what shim_append_tensors writes;
  2. sequence b holds what a batch-1 shim_append_tensors of x[b, first:first + count] writes
     through table row b at start_pos[b] with seed0 + row_base[b] * hkv.

Geometry: batch 4, q_max 5, 2 KV heads, block_size 4 (spans cross blocks), 2 layers (layer 1
written), injection on at BER 0.05.  Spans / start positions: (0,5)/0 full row, (2,3)/3 left pad,
(0,0)/6 inactive, (1,2)/2 pad on both sides.  The host twin runs everywhere, the HIP kernel under
the gpu marker.
"""

import ctypes

import pytest
import torch

BS, NL, LAYER, HKV = 4, 2, 1, 2
NBLOCKS, NPER = 16, 3
BATCH, QMAX = 4, 5
SPANS = [(0, 5), (2, 3), (0, 0), (1, 2)]
START = [0, 3, 6, 2]
BER, SEED0 = 5e-2, 4321
N_BITS = {"int4": 4, "hamming74": 7, "hamming84": 8, "golay": 24, "golay_packed": 24}
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
# head_dim 7: Golay rows of 3 codewords with zero padding, packed rows of 9 bytes + 3 pad bytes
GRID = [(c, 32, dt) for c in N_BITS for dt in DTYPES] + [(c, 7, dt) for c in ("golay", "golay_packed") for dt in DTYPES]
IDS = [f"{c}-d{d}-{str(dt)[6:]}" for c, d, dt in GRID]


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


def _caches(codec, d, device):
    per = _row_words(codec, d)
    dt = torch.int32 if codec == "golay" else torch.uint8
    return [torch.zeros((NBLOCKS, NL, HKV, BS * per), dtype=dt, device=device),
            torch.zeros((NBLOCKS, NL, HKV, BS * per), dtype=dt, device=device),
            torch.zeros((NBLOCKS, NL, HKV, BS), device=device), torch.zeros((NBLOCKS, NL, HKV, BS), device=device)]


def _tables(device):
    perm = torch.randperm(NBLOCKS, generator=torch.Generator().manual_seed(5))[:BATCH * NPER]
    return perm.view(BATCH, NPER).to(torch.int32).to(device)


def _span_tensor(spans, device):
    rows, base = [], 0
    for f, c in spans:
        rows.append((f, c, base))
        base += max(min(f + c, QMAX) - f, 0) if f >= 0 else 0
    return torch.tensor(rows, dtype=torch.int32, device=device)


def _kv(d, dtype, device, spans=None):
    """K, V [BATCH, QMAX, HKV, d]; with spans, every padding element is NaN."""
    g = torch.Generator().manual_seed(d)
    k = torch.randn(BATCH, QMAX, HKV, d, generator=g)
    v = 2 * torch.randn(BATCH, QMAX, HKV, d, generator=g)
    if spans is not None:
        for b, (f, c) in enumerate(spans):
            for x in (k, v):
                x[b, :f] = float("nan")
                x[b, f + c:] = float("nan")
    return k.to(dtype).to(device), v.to(dtype).to(device)


def _i32(x, device):
    return torch.tensor(x, dtype=torch.int32, device=device)


def _ragged(mod, k, v, caches, table, start, spans, codec, d, seed0=SEED0):
    mod.shim_append_ragged_tensors(k, v, *caches, table, start, NL, BS, HKV, d, LAYER, codec, N_BITS[codec], True, BER,
                                   seed0, spans)


def _uniform(mod, k, v, caches, table, start, codec, d, seed0=SEED0):
    mod.shim_append_tensors(k, v, *caches, table, start, NL, BS, HKV, d, LAYER, codec, N_BITS[codec], True, BER, seed0)


def _per_sequence(mod, dev, k, v, table, codec, d, spans):
    """Property 2's right-hand side: one batch-1 uniform append per non-empty sequence."""
    want = _caches(codec, d, dev)
    base = 0
    for b, (f, c) in enumerate(spans):
        if c > 0:
            _uniform(mod, k[b:b + 1, f:f + c], v[b:b + 1, f:f + c], want, table[b:b + 1], _i32([START[b]], dev), codec, d,
                     SEED0 + base * HKV)
        base += c
    return want


@pytest.mark.parametrize("codec,d,dtype", GRID, ids=IDS)
def test_each_sequence_is_its_own_batch_one_append(be, codec, d, dtype):
    mod, dev = be
    k, v = _kv(d, dtype, dev, SPANS)
    table, got = _tables(dev), _caches(codec, d, dev)
    _ragged(mod, k, v, got, table, _i32(START, dev), _span_tensor(SPANS, dev), codec, d)
    want = _per_sequence(mod, dev, k, v, table, codec, d, SPANS)
    for g, w, name in zip(got, want, ("k_cache", "v_cache", "k_scales", "v_scales")):
        assert torch.equal(g, w), name  # whole tensors: nothing else was written, no NaN scale
    assert bool(got[2].isfinite().all()) and int((got[2] != 0).sum()) == sum(c for _, c in SPANS) * HKV


@pytest.mark.parametrize("codec,d,dtype", GRID, ids=IDS)
def test_full_spans_are_the_uniform_append(be, codec, d, dtype):
    mod, dev = be
    k, v = _kv(d, dtype, dev)
    table, got, want = _tables(dev), _caches(codec, d, dev), _caches(codec, d, dev)
    start = _i32(START, dev)
    _ragged(mod, k, v, got, table, start, _span_tensor([(0, QMAX)] * BATCH, dev), codec, d)
    _uniform(mod, k, v, want, table, start, codec, d)
    for g, w in zip(got, want):
        assert torch.equal(g, w)


@pytest.mark.parametrize("codec,d,dtype", [("hamming84", 32, torch.float16), ("golay_packed", 7, torch.float32)])
def test_strided_views_are_read_in_place(be, codec, d, dtype):
    mod, dev = be
    k, v = _kv(d, dtype, dev, SPANS)
    kt, vt = (x.transpose(1, 2).contiguous().transpose(1, 2) for x in (k, v))  # [b, h, s, d] transposed
    assert not kt.is_contiguous()
    table, got, want = _tables(dev), _caches(codec, d, dev), _caches(codec, d, dev)
    spans, start = _span_tensor(SPANS, dev), _i32(START, dev)
    _ragged(mod, kt, vt, got, table, start, spans, codec, d)
    _ragged(mod, k, v, want, table, start, spans, codec, d)
    for g, w in zip(got, want):
        assert torch.equal(g, w)


def _abi_call(mod, dev, k, v, caches, table, start, spans, codec, d):
    """Straight to the C ABI: spans the Python layer's helpers would refuse."""
    from kvecc import _lib
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())  # noqa: E731
    codes = {"hamming84": _lib.CODEC_H84, "golay_packed": _lib.CODEC_GOLAY_PACKED}
    lib = _lib.load()
    rule = _lib.SCALE_RULES[mod.DEFAULT_SCALE_RULE]  # what _per_sequence's Python calls pass
    if dev.type == "cpu":
        return lib.kvecc_cpu_shim_append_ragged(p(k), p(v), _lib.F32, BATCH, QMAX, HKV, d, codes[codec], rule,
                                                N_BITS[codec], 1, BER, SEED0, *[p(c) for c in caches], p(table), NPER,
                                                p(start), p(spans), NL, BS, LAYER, 1)
    rc = lib.kvecc_shim_append_ragged(p(k), p(v), k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1),
                                      v.stride(2), _lib.F32, BATCH, QMAX, HKV, d, codes[codec], rule, N_BITS[codec], 1,
                                      BER, SEED0, *[p(c) for c in caches], p(table), NPER, p(start), p(spans), NL,
                                      BS, LAYER, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("codec,d", [("hamming84", 32), ("golay_packed", 7)])
def test_spans_are_clamped_and_null_is_einval(be, codec, d):
    mod, dev = be
    # (3, 9): tokens 3, 4 only; (-1, 3): nothing; (0, -2): nothing; (4, 1): the last token
    raw = [(3, 9, 0), (-1, 3, 2), (0, -2, 2), (4, 1, 2)]
    clamped = [(3, 2), (0, 0), (0, 0), (4, 1)]
    k, v = _kv(d, torch.float32, dev, clamped)
    table, got = _tables(dev), _caches(codec, d, dev)
    start = _i32(START, dev)
    spans = torch.tensor(raw, dtype=torch.int32, device=dev)
    assert _abi_call(mod, dev, k, v, got, table, start, spans, codec, d) == 0
    want = _per_sequence(mod, dev, k, v, table, codec, d, clamped)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    before = [g.clone() for g in got]
    assert _abi_call(mod, dev, k, v, got, table, start, None, codec, d) == -1  # KVECC_EINVAL
    from kvecc import _lib
    assert "q_spans" in _lib.load().kvecc_last_error().decode()
    for g, w in zip(got, before):
        assert torch.equal(g, w)


def test_validation(be):
    mod, dev = be
    codec, d = "hamming84", 32
    k, v = _kv(d, torch.float16, dev)
    table, caches, start = _tables(dev), _caches(codec, d, dev), _i32(START, dev)
    sp = _span_tensor(SPANS, dev)
    bad = [sp.to(torch.int64), sp[:, :2].contiguous(), sp[:3].contiguous(), sp.reshape(-1), sp.tolist(), None,
           torch.zeros((BATCH, 6), dtype=torch.int32, device=dev)[:, ::2]]
    if dev.type != "cpu":
        bad.append(sp.cpu())
    for spans in bad:
        with pytest.raises(ValueError):
            _ragged(mod, k, v, caches, table, start, spans, codec, d)
    with pytest.raises(ValueError):  # the uniform entry's checks still hold
        _ragged(mod, k, v, caches, table, start.to(torch.int64), sp, codec, d)
    assert all(not bool(c.any()) for c in caches)  # nothing was written


@pytest.mark.parametrize("codec,d", [("hamming84", 32), ("golay", 7)])
def test_dispatcher_op(be, codec, d):
    import kvecc  # noqa: F401
    from kvecc import torch_ops
    assert "shim_append_ragged" in torch_ops.OPS
    mod, dev = be
    k, v = _kv(d, torch.float16, dev, SPANS)
    table, got, want = _tables(dev), _caches(codec, d, dev), _caches(codec, d, dev)
    spans, start = _span_tensor(SPANS, dev), _i32(START, dev)
    args = lambda c: (k, v, *c, table, start, spans, NL, BS, HKV, d, LAYER, codec, N_BITS[codec], True, BER,  # noqa: E731
                      SEED0)
    torch.ops.kvecc.shim_append_ragged(*args(got))
    _ragged(mod, k, v, want, table, start, spans, codec, d)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    torch.library.opcheck(torch.ops.kvecc.shim_append_ragged.default, args(_caches(codec, d, dev)))
