"""Paged attention over Hamming(7,4) and unprotected INT4 caches (the byte family).

Contract (include/kvecc.h, "Byte caches without SECDED"): a stored byte b is worth
(data(b) - 8) * scale, data = h74_decode4's nibble of the low 7 bits (hamming74: bit 7
ignored, doubles miscorrected) or b & 15 (int4); layout, head_dim rule, dtypes, GQA map, -1
blocks, the max_context_len clamp and the empty value (-8.0) are Hamming(8,4)'s, and so is the
launch geometry: the kernels are a sibling family over the Hamming(8,4) bodies with another
decode table.  Every case runs on the host twin and, marked gpu, on the device.

The shapes, tables, lengths and queries are those of tests/test_attention_paths.py and
tests/test_attention_chunk.py (their Hamming(8,4) entries, taken from their cached bundles);
the caches are written through the host backend's shim write at BER 1e-2.  The float64
reference is those files' `_ref64` / `_ref_chunk` over the cache restated as a clean
Hamming(8,4) cache: cpu_ops' row decode of every stored byte (hamming74_decode, pinned to the
oracle by tests/test_cpu_backend.py; b & 15), re-encoded, which Hamming(8,4) decodes back to
exactly those nibbles.  Tolerances are the suite's TOL per query dtype.
"""

import functools
import math

import numpy as np
import pytest
import torch

import tests.test_attention_decode_probe as probe
from tests import test_attention_chunk as chunk
from tests import test_attention_paths as paths
from tests.test_attention_chunk import GENERAL_PATHS, MFMA_PATHS, Q_LENS, _attend_chunk, _ref_chunk
from tests.test_attention_chunk_ragged import _span_tensor, _valid
from tests.test_attention_paths import (BF16, F16, F32, PATHS, TOL, _TNAME, _attend, _cdiv, _close, _err, _query,
                                        _ref64)

CODECS = ("hamming74", "int4")
N_BITS = {"hamming74": 7, "int4": 4}  # the shim's injection widths
EMPTY = -8.0
LAYERS, LAYER = paths.LAYERS, paths.LAYER

H84_PATHS = [p for p in PATHS if p[0] == "hamming84"]
H84_BF16 = [p for p in H84_PATHS if p[1] == BF16]
H84_CHUNK = [p for p in MFMA_PATHS + GENERAL_PATHS if p[0] == "hamming84"]
MFMA_SHAPE, SPLIT_SHAPE = (F16, 128, 8, 2), (F32, 100, 6, 2)  # one matrix-core and one split shape


def _mods(gpu):
    from kvecc import cpu_ops, ops
    return (cpu_ops, None) if gpu is None else (ops, gpu)


def _sid(p):
    return f"{_TNAME[p[1]].strip('_')}-d{p[2]}-{p[3]}q{p[4]}kv"


def test_the_shapes_are_the_hamming84_entries():
    assert len(H84_PATHS) == 69 and len(H84_BF16) == 18 and len(H84_CHUNK) == 10
    assert ("hamming84",) + MFMA_SHAPE in MFMA_PATHS and ("hamming84",) + SPLIT_SHAPE in GENERAL_PATHS
    assert paths._select("hamming84", *MFMA_SHAPE)[0] == "paged_attn_h84_mfma_kernel<128, 4>"
    assert "split_kernel<float" in paths._select("hamming84", *SPLIT_SHAPE)[0]


# ---- data -----------------------------------------------------------------------------------
def _nibbles(codec, cache):
    """cpu_ops' row decode of every stored byte -> the data nibbles, same shape."""
    from kvecc import cpu_ops
    return cpu_ops.hamming74_decode(cache)[0] if codec == "hamming74" else cache & 15


def _as_h84(codec, cache):
    """The clean Hamming(8,4) cache that decodes to the nibbles `cache` decodes to."""
    from kvecc import cpu_ops
    return cpu_ops.hamming84_encode(_nibbles(codec, cache).contiguous()).view(cache.shape)


@functools.lru_cache(maxsize=None)
def _caches(codec, d, kvh, bs, num_blocks, layers, seed, pin_last_row, ber=0.01):
    """Every block of every layer written through the host backend's shim write (one sequence over
    blocks 0..n-1), injected at `ber` -> kc, vc [blocks, layers, kvh, bs * d] uint8, ks, vs.
    pin_last_row: the buffer's last row (last block, layer, cache head, slot) is written from one
    value at the largest magnitude, so that it holds nibble 15 at the largest scale before injection."""
    from kvecc import cpu_ops
    g = torch.Generator().manual_seed(seed)
    kc = torch.zeros(num_blocks, layers, kvh, bs * d, dtype=torch.uint8)
    vc = torch.zeros_like(kc)
    ks = torch.zeros(num_blocks, layers, kvh, bs)
    vs = torch.zeros_like(ks)
    table = torch.arange(num_blocks, dtype=torch.int32)
    for layer in range(layers):
        x = torch.randn(2, 1, num_blocks * bs, kvh, d, generator=g) * 0.7  # scales about 0.2-0.35
        if pin_last_row and layer == layers - 1:
            x[:, 0, -1, -1, :] = 2.45
        cpu_ops.shim_write_tensors(x[0].reshape(1, num_blocks * bs, kvh * d), x[1].reshape(1, num_blocks * bs, kvh * d),
                                   kc, vc, ks, vs, table, layers, bs, kvh, d, layer, codec, N_BITS[codec], ber > 0,
                                   ber, 1000 * seed + 100 * layer)
    return kc, vc, ks, vs


@pytest.mark.parametrize("codec", CODECS)
def test_the_caches_hold_corrected_and_miscorrected_words(codec):
    from kvecc import cpu_ops
    args = (codec, 128, 2, 16, 12, LAYERS, 228, True)
    noisy, clean = _caches(*args)[0], _caches(*args, ber=0.0)[0]
    assert int((noisy != clean).sum()) > 100 and int(noisy.max()) < (128 if codec == "hamming74" else 16)
    wrong = int((_nibbles(codec, noisy) != _nibbles(codec, clean)).sum())
    assert wrong > 0  # hamming74: doubles, miscorrected; int4: every flipped bit
    if codec == "hamming74":
        assert cpu_ops.hamming74_decode(noisy)[1][0] > 10 * wrong  # most flagged words are corrected
    assert float(_caches(*args)[2][-1, -1, -1, -1]) == pytest.approx(0.35, abs=1e-6)  # the pinned row's scale


# ---- 1. the bundles -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decode_bundle(codec, dtype, d, heads, kvh, bs):
    """tests/test_attention_paths.py's edge bundle (its table, lengths and query) over byte caches."""
    h = paths._bundle("hamming84", dtype, d, heads, kvh, bs)
    kc, vc, ks, vs = _caches(codec, d, kvh, bs, h["kc"].shape[0], LAYERS, 100 + d, True)
    ref = _ref64(h["q"], _as_h84(codec, kc), _as_h84(codec, vc), h["table"], h["lens"], ks, vs, LAYER, bs, "hamming84")
    return dict(q=h["q"], table=h["table"], lens=h["lens"], kc=kc, vc=vc, ks=ks, vs=vs, ref=ref)


def _check_decode_bundle(mod, dev, codec, path, bs):
    _, dtype, d, heads, kvh, _, _ = path
    c = _decode_bundle(codec, dtype, d, heads, kvh, bs)
    for mcl in (0, int(c["lens"].max())):  # the default, and what append mode passes
        got = _attend(mod, dev, codec, c["q"], c["kc"], c["vc"], c["table"], c["lens"], c["ks"], c["vs"], LAYER, bs, mcl)
        print(f"{codec} mcl {mcl}: max err {_err(got, c['ref']):.3e}")
        assert torch.equal(got[2], torch.full((heads, d), EMPTY, dtype=torch.float64)), mcl
        assert _close(got, c["ref"], dtype), (mcl, _err(got, c["ref"]))


@pytest.mark.parametrize("path", H84_PATHS, ids=_sid)
@pytest.mark.parametrize("codec", CODECS)
def test_cpu_decode_bundle(codec, path):
    _check_decode_bundle(*_mods(None), codec, path, 16)


@pytest.mark.parametrize("path", H84_BF16, ids=_sid)
@pytest.mark.parametrize("codec", CODECS)
def test_cpu_decode_bundle_last_block_only(codec, path):
    _check_decode_bundle(*_mods(None), codec, path, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("path", H84_PATHS, ids=_sid)
@pytest.mark.parametrize("codec", CODECS)
def test_hip_decode_bundle(gpu, codec, path):
    _check_decode_bundle(*_mods(gpu), codec, path, 16)


@pytest.mark.gpu
@pytest.mark.parametrize("path", H84_BF16, ids=_sid)
@pytest.mark.parametrize("codec", CODECS)
def test_hip_decode_bundle_last_block_only(gpu, codec, path):
    _check_decode_bundle(*_mods(gpu), codec, path, 4)


@functools.lru_cache(maxsize=None)
def _chunk_bundle(codec, dtype, d, heads, kvh, q_len):
    """tests/test_attention_chunk.py's edge bundle over byte caches."""
    h = chunk._bundle("hamming84", dtype, d, heads, kvh, q_len)
    kc, vc, ks, vs = _caches(codec, d, kvh, chunk.BS, h["kc"].shape[0], LAYERS, 200 + d, True)
    return dict(h, kc=kc, vc=vc, ks=ks, vs=vs)


def _check_chunk(mod, dev, codec, dtype, c, mcls=(0,)):
    """The chunk call against the float64 reference; rows without a visible key are exactly empty."""
    hk, hv = _as_h84(codec, c["kc"]), _as_h84(codec, c["vc"])
    for mcl in mcls:
        ref = _ref_chunk(c["q"], hk, hv, c["table"], c["lens"], c["ks"], c["vs"], c["layer"], c["bs"], "hamming84", mcl)
        got, _ = _attend_chunk(mod, dev, codec, c["q"], c["kc"], c["vc"], c["table"], c["lens"], c["ks"], c["vs"],
                               c["layer"], c["bs"], mcl)
        print(f"{codec} mcl {mcl}: chunk max err {_err(got, ref):.3e}")
        empty = (ref == EMPTY).all(-1).all(-1)  # [B, T]
        assert bool(empty.any()) and torch.equal(got[empty], ref[empty]), mcl
        assert _close(got, ref, dtype), (mcl, _err(got, ref))


def _check_chunk_bundle(mod, dev, codec, path, q_len):
    _, dtype, d, heads, kvh = path
    c = _chunk_bundle(codec, dtype, d, heads, kvh, q_len)
    _check_chunk(mod, dev, codec, dtype, c, (0, int(c["lens"].max())))


@pytest.mark.parametrize("q_len", Q_LENS)
@pytest.mark.parametrize("path", H84_CHUNK, ids=_sid)
@pytest.mark.parametrize("codec", CODECS)
def test_cpu_chunk_bundle(codec, path, q_len):
    _check_chunk_bundle(*_mods(None), codec, path, q_len)


@pytest.mark.gpu
@pytest.mark.parametrize("q_len", Q_LENS)
@pytest.mark.parametrize("path", H84_CHUNK, ids=_sid)
@pytest.mark.parametrize("codec", CODECS)
def test_hip_chunk_bundle(gpu, codec, path, q_len):
    _check_chunk_bundle(*_mods(gpu), codec, path, q_len)


# the max_context_len contract of tests/test_attention_paths.py, at a split GQA and a matrix-core shape
CONTRACT = [(F32, 64, 8, 2), MFMA_SHAPE]


def _check_contract(mod, dev, codec, shape):
    dtype, d, heads, kvh = shape
    h = paths._contract(("hamming84",) + shape)
    kc, vc, ks, vs = _caches(codec, d, kvh, 16, h["kc"].shape[0], 2, 7 + d, False)
    hk, hv = _as_h84(codec, kc), _as_h84(codec, vc)

    def run(lens, mcl):
        return _attend(mod, dev, codec, h["q"], kc, vc, h["table"], torch.tensor(lens, dtype=torch.int32), ks, vs, 1,
                       16, mcl)

    def ref(lens):
        return _ref64(h["q"], hk, hv, h["table"], torch.tensor(lens, dtype=torch.int32), ks, vs, 1, 16, "hamming84")

    got = run([100, 93], 50)  # context_lens above max_context_len are attended up to it
    assert _close(got, ref([50, 50]), dtype), _err(got, ref([50, 50]))
    assert not _close(ref([100, 93]), ref([50, 50]), dtype)
    got = run([100, 200], 300)  # max_context_len past the table: 7 blocks of 16 bound the context
    assert _close(got, ref([100, 112]), dtype) and _close(got, run([100, 200], 0), dtype)
    got = run([-5, 93], 0)  # a negative length is an empty context
    assert torch.equal(got[0], torch.full(got[0].shape, EMPTY, dtype=torch.float64))
    assert _close(got, ref([0, 93]), dtype)


@pytest.mark.parametrize("shape", CONTRACT, ids=lambda s: _sid((None,) + s))
@pytest.mark.parametrize("codec", CODECS)
def test_cpu_max_context_len_contract(codec, shape):
    _check_contract(*_mods(None), codec, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CONTRACT, ids=lambda s: _sid((None,) + s))
@pytest.mark.parametrize("codec", CODECS)
def test_hip_max_context_len_contract(gpu, codec, shape):
    _check_contract(*_mods(gpu), codec, shape)


# ---- 2. every byte value ------------------------------------------------------------------------
# The probes of tests/test_attention_decode_probe.py (V exact; K the nearest of 16 candidates, under
# its margin assertion) over its Hamming(8,4) probe rows -- the 256 byte values in 4 permutations --
# read as hamming74 / int4 bytes: only the expectation and the constant rows are this codec's.
def _expected_nibbles(codec, cw):
    """What a stored byte is worth, from the oracle (hamming74: its decode of the low 7 bits) or
    the contract's own statement (int4: b & 15)."""
    if codec == "int4":
        return cw & 15
    return probe._oracle().hamming74_decode(cw & 0x7F)[0]


_H84_ROWS = probe._rows  # the probe rows themselves (the probes are later pointed at _byte_rows)


@functools.lru_cache(maxsize=None)
def _byte_rows(codec, d):
    words, _, cw, _, kinds = _H84_ROWS("hamming84", d)
    assert all(np.array_equal(np.sort(cw[256 * i:256 * i + 256]), np.arange(256)) for i in range(4))
    return words, _expected_nibbles(codec, words), cw, _expected_nibbles(codec, cw), kinds


def _const_row(codec, d, nibble):
    row = np.full(d, nibble, np.uint8)
    return row if codec == "int4" else probe._oracle().hamming74_encode(row)


def _probe_as(monkeypatch, codec):
    """tests/test_attention_decode_probe.py's probes over this codec's expectation."""
    monkeypatch.setattr(probe, "_base", lambda c: "hamming84")
    monkeypatch.setattr(probe, "_rows", lambda base, d: _byte_rows(codec, d))
    monkeypatch.setattr(probe, "_const_row", lambda base, d, nibble: _const_row(codec, d, nibble))


def test_hamming74_ignores_bit_7_in_the_shim_read_too():
    """Before any attention call: the host shim read of all 256 byte values is the oracle's
    Hamming(7,4) decode of the low 7 bits, bit 7 set or not."""
    from kvecc import cpu_ops
    o = probe._oracle()
    b = np.arange(256, dtype=np.uint8)
    exp = _expected_nibbles("hamming74", b)
    assert np.array_equal(exp[128:], exp[:128]) and np.array_equal(o.hamming74_decode(b)[0][:128], exp[:128])
    cache = torch.from_numpy(b.copy()).view(1, 1, 1, 256)  # one block of 16 tokens, head_dim 16
    ones = torch.ones(1, 1, 1, 16)
    k, _ = cpu_ops.shim_read_tensors(cache, cache, ones, ones, torch.zeros(1, dtype=torch.int32), 16, 1, 16, 1, 16, 0,
                                     "hamming74", False, F32)
    assert np.array_equal(k.reshape(-1).numpy() + 8.0, exp.astype(np.float32))
    # and the contract's stated difference: the shim read dequantizes an int4 byte raw
    k, _ = cpu_ops.shim_read_tensors(cache, cache, ones, ones, torch.zeros(1, dtype=torch.int32), 16, 1, 16, 1, 16, 0,
                                     "int4", False, F32)
    raw = k.reshape(-1).numpy() + 8.0
    assert np.array_equal(raw[:16], np.arange(16.0)) and not np.array_equal(raw[16:], (b & 15)[16:].astype(np.float32))


def _probe_path(codec, shape):
    return (codec,) + shape + (4, "")


@pytest.mark.parametrize("shape", [MFMA_SHAPE, SPLIT_SHAPE], ids=lambda s: _sid((None,) + s))
@pytest.mark.parametrize("codec", CODECS)
def test_cpu_every_byte_value(monkeypatch, codec, shape):
    _probe_as(monkeypatch, codec)
    probe._check_v(*_mods(None), _probe_path(codec, shape))
    probe._check_k(*_mods(None), _probe_path(codec, shape))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [MFMA_SHAPE, SPLIT_SHAPE], ids=lambda s: _sid((None,) + s))
@pytest.mark.parametrize("codec", CODECS)
def test_hip_every_byte_value(gpu, monkeypatch, codec, shape):
    _probe_as(monkeypatch, codec)
    probe._check_v(*_mods(gpu), _probe_path(codec, shape))
    probe._check_k(*_mods(gpu), _probe_path(codec, shape))


# ---- 3. same body, same bits ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _same_case(shape):
    """One nibble tensor as int4 bytes, as Hamming(7,4) and as Hamming(8,4) codewords, no injection."""
    from kvecc import cpu_ops
    dtype, d, heads, kvh = shape
    g = torch.Generator().manual_seed(d)
    nblk, bs = 7, 16
    nib = torch.randint(0, 16, (3 * nblk + 1, LAYERS, kvh, bs * d), generator=g, dtype=torch.uint8)
    caches = {"int4": nib, "hamming74": cpu_ops.hamming74_encode(nib), "hamming84": cpu_ops.hamming84_encode(nib)}
    ks, vs = (torch.rand(3 * nblk + 1, LAYERS, kvh, bs, generator=g) * 0.3 + 0.05 for _ in range(2))
    table = torch.randperm(3 * nblk + 1, generator=g)[:3 * nblk].to(torch.int32).view(3, nblk).contiguous()
    table[1, 2] = -1
    lens = torch.tensor([100, 41, 6], dtype=torch.int32)
    return dict(caches=caches, ks=ks, vs=vs, table=table, lens=lens, q1=_query(3, heads, d, dtype, seed=3),
                q5=torch.randn(3, 5, heads, d, generator=g).to(dtype))


def _check_same_bits(mod, dev, shape):
    c = _same_case(shape)
    outs = {}
    for codec, cache in c["caches"].items():
        one = _attend(mod, dev, codec, c["q1"], cache, cache, c["table"], c["lens"], c["ks"], c["vs"], LAYER, 16)
        five = _attend_chunk(mod, dev, codec, c["q5"], cache, cache, c["table"], c["lens"], c["ks"], c["vs"], LAYER,
                             16)[1]
        outs[codec] = (one, five)
    for codec in CODECS:
        assert torch.equal(outs[codec][0], outs["hamming84"][0]), codec
        assert torch.equal(outs[codec][1], outs["hamming84"][1]), codec


@pytest.mark.parametrize("shape", [MFMA_SHAPE, SPLIT_SHAPE], ids=lambda s: _sid((None,) + s))
def test_cpu_clean_caches_return_hamming84_bits(shape):
    _check_same_bits(*_mods(None), shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [MFMA_SHAPE, SPLIT_SHAPE], ids=lambda s: _sid((None,) + s))
def test_hip_clean_caches_return_hamming84_bits(gpu, shape):
    _check_same_bits(*_mods(gpu), shape)


# ---- 4. ragged spans ------------------------------------------------------------------------------
COUNTS = (7, 4, 1, 0)
RAGGED = {"right-padded": (0, 0, 0, 0), "left-padded": (0, 3, 6, 0)}
EXTRA = (20, 0, 41, 9)  # context before the span's own tokens; sequence 3 has no query row over a non-empty cache


@functools.lru_cache(maxsize=None)
def _ragged_case(codec, shape, firsts):
    dtype, d, heads, kvh = shape
    spans = tuple(zip(firsts, COUNTS))
    lens = torch.tensor([c + e for c, e in zip(COUNTS, EXTRA)], dtype=torch.int32)
    nblk = [_cdiv(int(n), 16) for n in lens]
    num_blocks = sum(nblk) + 1
    kc, vc, ks, vs = _caches(codec, d, kvh, 16, num_blocks, LAYERS, 300 + d, False)
    ids = torch.randperm(num_blocks, generator=torch.Generator().manual_seed(d)).to(torch.int32).tolist()
    table = torch.full((4, max(nblk) + 1), -1, dtype=torch.int32)
    for b in range(4):
        table[b, :nblk[b]] = torch.tensor([ids.pop() for _ in range(nblk[b])], dtype=torch.int32)
    table[2, 1] = -1  # tokens inside sequence 2's context are skipped
    q = torch.randn(4, 7, heads, d, generator=torch.Generator().manual_seed(7)).to(dtype)
    q[~_valid(spans, 7)] = float("nan")
    return dict(q=q, kc=kc, vc=vc, ks=ks, vs=vs, table=table, lens=lens, spans=spans)


def _check_ragged(mod, dev, codec, shape, firsts):
    dtype, d = shape[0], shape[1]
    c = _ragged_case(codec, shape, firsts)
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    dev_c = {k: t(c[k]) for k in ("kc", "vc", "table", "lens", "ks", "vs")}

    def call(q, rows, spans):
        out = torch.empty(q.shape, dtype=dtype, device=dev)
        mod.paged_attention_chunk_into(t(q), dev_c["kc"], dev_c["vc"], dev_c["table"][rows].contiguous(),
                                       dev_c["lens"][rows].contiguous(), dev_c["ks"], dev_c["vs"], out, LAYER, 16,
                                       1 / math.sqrt(d), codec, q_spans=None if spans is None else t(_span_tensor(spans)))
        return out.cpu().double()

    got = call(c["q"], slice(0, 4), c["spans"])
    valid = _valid(c["spans"], 7)
    assert not bool(got.isnan().any())  # NaN in padding query rows reaches no output
    assert bool((got[~valid] == EMPTY).all()) and not bool(valid[3].any())
    hk, hv = _as_h84(codec, c["kc"]), _as_h84(codec, c["vc"])
    for b, (f, n) in enumerate(c["spans"]):
        if n == 0:
            continue
        solo = call(c["q"][b:b + 1, f:f + n].contiguous(), slice(b, b + 1), None)[0]  # the batch-1 uniform call
        ref = _ref_chunk(c["q"][b:b + 1, f:f + n], hk, hv, c["table"][b:b + 1], c["lens"][b:b + 1], c["ks"], c["vs"],
                         LAYER, 16, "hamming84")[0]
        print(f"sequence {b}: against its batch-1 call {_err(got[b, f:f + n], solo):.3e}, against float64 "
              f"{_err(got[b, f:f + n], ref):.3e}")
        assert _close(got[b, f:f + n], solo, dtype) and _close(got[b, f:f + n], ref, dtype)


@pytest.mark.parametrize("pad", sorted(RAGGED))
@pytest.mark.parametrize("shape", [MFMA_SHAPE, SPLIT_SHAPE], ids=lambda s: _sid((None,) + s))
@pytest.mark.parametrize("codec", CODECS)
def test_cpu_ragged_spans(codec, shape, pad):
    _check_ragged(*_mods(None), codec, shape, RAGGED[pad])


@pytest.mark.gpu
@pytest.mark.parametrize("pad", sorted(RAGGED))
@pytest.mark.parametrize("shape", [MFMA_SHAPE, SPLIT_SHAPE], ids=lambda s: _sid((None,) + s))
@pytest.mark.parametrize("codec", CODECS)
def test_hip_ragged_spans(gpu, codec, shape, pad):
    _check_ragged(*_mods(gpu), codec, shape, RAGGED[pad])


# ---- 5. validation, the dispatcher ------------------------------------------------------------------
def _small(codec, dev=None, d=32):
    kc, vc, ks, vs = _caches(codec, d, 2, 16, 7, 1, 13, False)
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    q = torch.randn(1, 5, 2, d, generator=torch.Generator().manual_seed(6)).half()
    return dict(q=t(q), kc=t(kc), vc=t(vc), table=t(torch.arange(6, dtype=torch.int32).view(1, 6)),
                lens=t(torch.tensor([86], dtype=torch.int32)), ks=t(ks), vs=t(vs),
                out=torch.full(q.shape, 77.0, dtype=q.dtype, device=dev))


def _call(mod, a, codec, **kw):
    return mod.paged_attention_chunk_into(a["q"], a["kc"], a["vc"], a["table"], a["lens"], a["ks"], a["vs"], a["out"],
                                          0, 16, 1 / math.sqrt(a["q"].shape[-1]), codec, **kw)


def _check_validation(mod, dev, codec):
    a = _small(codec, dev)
    with pytest.raises(ValueError, match="interp needs hamming84"):
        _call(mod, a, codec, interp=True)
    with pytest.raises(ValueError, match="interp needs hamming84"):
        mod.paged_attention_into(a["q"][:, 0].contiguous(), a["kc"], a["vc"], a["table"], a["lens"], a["ks"], a["vs"],
                                 a["out"][:, 0].contiguous(), 0, 16, 0.25, codec, interp=True)
    with pytest.raises(ValueError, match="must be torch.uint8"):
        _call(mod, dict(a, kc=a["kc"].to(torch.int32)), codec)
    with pytest.raises(ValueError, match="int4, hamming74, hamming84, golay or golay_packed"):
        _call(mod, a, "fp8")
    assert bool((a["out"] == 77.0).all())  # nothing was launched
    # head_dim 30 (rows of 30 bytes: a consistent cache): the library refuses it, both entries
    b = _small(codec, dev, d=32)
    for k in ("kc", "vc"):
        b[k] = b[k].view(7, 1, 2, 16, 32)[..., :30].reshape(7, 1, 2, 16 * 30).contiguous()
    b["q"], b["out"] = b["q"][..., :30].contiguous(), b["out"][..., :30].contiguous()
    with pytest.raises((ValueError, RuntimeError), match="multiple of 4"):
        _call(mod, b, codec)
    with pytest.raises((ValueError, RuntimeError), match="multiple of 4"):
        mod.paged_attention_into(b["q"][:, 0].contiguous(), b["kc"], b["vc"], b["table"], b["lens"], b["ks"], b["vs"],
                                 b["out"][:, 0].contiguous(), 0, 16, 0.25, codec)
    if dev is not None:
        torch.cuda.synchronize()
    assert bool((b["out"] == 77.0).all())
    _call(mod, a, codec)
    assert not bool((a["out"] == 77.0).any())


@pytest.mark.parametrize("codec", CODECS)
def test_cpu_validation(codec):
    _check_validation(*_mods(None), codec)


@pytest.mark.gpu
@pytest.mark.parametrize("codec", CODECS)
def test_hip_validation(gpu, codec):
    _check_validation(*_mods(gpu), codec)


@pytest.mark.parametrize("codec", CODECS)
def test_dispatcher_ops_on_the_host_are_cpu_ops(codec):
    import kvecc
    from kvecc import cpu_ops
    a = _small(codec)
    sm = 1 / math.sqrt(32)
    rest = (a["ks"], a["vs"], 0, 16, sm, codec)
    got = torch.ops.kvecc.paged_attention_chunk(a["q"], a["kc"], a["vc"], a["table"], a["lens"], *rest)
    _call(cpu_ops, a, codec)
    assert torch.equal(got, a["out"])
    assert torch.equal(kvecc.paged_attention_chunk(a["q"], a["kc"], a["vc"], a["table"], a["lens"], a["ks"], a["vs"], 0,
                                                   16, codec=codec), got)
    spans = _span_tensor([(2, 3)])
    got = torch.ops.kvecc.paged_attention_chunk_ragged(a["q"], a["kc"], a["vc"], a["table"], a["lens"], spans, *rest)
    _call(cpu_ops, a, codec, q_spans=spans)
    assert torch.equal(got, a["out"]) and bool((got[0, :2] == EMPTY).all())
    q1 = a["q"][:, 0].contiguous()
    got = torch.ops.kvecc.paged_attention(q1, a["kc"], a["vc"], a["table"], a["lens"], *rest)
    out1 = torch.empty_like(q1)
    cpu_ops.paged_attention_into(q1, a["kc"], a["vc"], a["table"], a["lens"], a["ks"], a["vs"], out1, 0, 16, sm, codec)
    assert torch.equal(got, out1)
    with pytest.raises(ValueError):  # the reference-named entry keeps its two codecs
        cpu_ops.paged_attention_ecc(q1, a["kc"], a["vc"], a["table"], a["lens"], a["ks"], 0, 16, codec=codec)


@pytest.mark.parametrize("codec", CODECS)
def test_dispatcher_ops_trace_to_the_right_shape(codec):
    from torch._subclasses.fake_tensor import FakeTensorMode
    import kvecc  # noqa: F401
    a = _small(codec)
    with FakeTensorMode() as mode:
        f = {k: mode.from_tensor(v) for k, v in a.items()}
        rest = (f["ks"], f["vs"], 0, 16, 0.25, codec)
        spans = mode.from_tensor(_span_tensor([(2, 3)]))
        assert torch.ops.kvecc.paged_attention_chunk(f["q"], f["kc"], f["vc"], f["table"], f["lens"], *rest).shape == \
            a["q"].shape
        assert torch.ops.kvecc.paged_attention_chunk_ragged(f["q"], f["kc"], f["vc"], f["table"], f["lens"], spans,
                                                            *rest).shape == a["q"].shape
        out = torch.ops.kvecc.paged_attention(f["q"][:, 0], f["kc"], f["vc"], f["table"], f["lens"], *rest)
        assert out.shape == (1, 2, 32) and out.dtype == torch.float16
