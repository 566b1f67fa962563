"""Dequantize and quantize at the ends of the scale range, bit for bit.

Dequantize: decode_dequant_h84_into and shim_read_batch (Hamming(8,4) and Golay)
into fp16 and bf16 at scales 2^-24, 2^-17, 2^-14, 2^12 and 2^13, every nibble:
subnormal results, the largest finite fp16 result 7 * 2^13, and -8 * 2^13 =
-65536, which rounds to -inf in fp16 as torch's .to(float16) does.  Expectation:
((q - 8).float() * scale).to(dtype) computed by torch on the host.

Quantize: fp32 rows (the IEEE-division path; tests/test_quant_exhaustive.py
covers 16-bit inputs only) whose maxima are 2^-140 (subnormal), 2^-126, 2^-100,
2^100 and the largest finite float, through quantize_encode_rows_into and, for
the other quantizer path, one shim_append call; both scale rules, nibbles and
scales against that file's `_reference` run on the host.

Every case runs on the host twin and, marked gpu, on the device.
"""

import functools

import pytest
import torch

from tests.test_quant_exhaustive import _reference

F16, BF16 = torch.float16, torch.bfloat16
SCALES = [2.0 ** -24, 2.0 ** -17, 2.0 ** -14, 2.0 ** 12, 2.0 ** 13]
BS = 8  # block size: the five rows and three unwritten slots


def _mods(gpu):
    from kvecc import cpu_ops, ops
    return (cpu_ops, None) if gpu is None else (ops, gpu)


def _bits(x):
    return x.contiguous().view(torch.int16)


# ---- dequantize -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nibble_rows(d):
    """[5, d] nibbles: 0..15 in the first 16 lanes of every row, then 15, 0, ..."""
    return (torch.arange(d) % 16).to(torch.uint8).repeat(len(SCALES), 1).contiguous()


def _expected(d, dtype):
    scale = torch.tensor(SCALES, dtype=torch.float32).unsqueeze(-1)
    return ((_nibble_rows(d).float() - 8.0) * scale).to(dtype)


def test_the_expectation_holds_the_edges():
    e = _expected(16, F16)
    assert float(e[4, 0]) == float("-inf") and float(e[4, 15]) == 7 * 2.0 ** 13 and bool(e[4, 1:].isfinite().all())
    assert float(e[0, 9]) == 2.0 ** -24 and float(e[1, 9]) == 2.0 ** -17  # fp16 subnormals
    assert bool((e[:3, 9:].float().abs() < 2.0 ** -14).any()) and bool((e[:2] != 0)[:, 9:].all())
    b = _expected(16, BF16)
    assert float(b[4, 0]) == -65536.0 and bool(b.isfinite().all())


def _check_dequant_rows(mod, dev, dtype):
    from kvecc import cpu_ops
    cw = cpu_ops.hamming84_encode(_nibble_rows(16))
    sc = torch.tensor(SCALES, dtype=torch.float32)
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    out = torch.zeros(len(SCALES), 16, dtype=dtype, device=dev)
    mod.decode_dequant_h84_into(t(cw), t(sc), out)
    assert torch.equal(_bits(out.cpu()), _bits(_expected(16, dtype)))


def _check_shim_read(mod, dev, codec, dtype):
    from kvecc import cpu_ops
    d = 16 if codec == "hamming84" else 17  # Golay: six codewords, the last one padded
    nib = _nibble_rows(d)
    enc = cpu_ops.hamming84_encode(nib) if codec == "hamming84" else cpu_ops.golay_encode_rows(nib)
    cache = torch.zeros(1, 1, 1, BS, enc.shape[-1], dtype=enc.dtype)
    cache[0, 0, 0, :len(SCALES)] = enc
    cache = cache.view(1, 1, 1, -1).contiguous()
    sc = torch.zeros(1, 1, 1, BS)
    sc[0, 0, 0, :len(SCALES)] = torch.tensor(SCALES)
    table = torch.zeros(1, 1, dtype=torch.int32)
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    k, v = mod.shim_read_batch(t(cache), t(cache), t(sc), t(sc), t(table), len(SCALES), d, 0, codec, dtype)
    want = _bits(_expected(d, dtype))
    assert torch.equal(_bits(k.cpu()[0, 0]), want) and torch.equal(_bits(v.cpu()[0, 0]), want)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["half", "bfloat16"])
def test_cpu_dequant_rows(dtype):
    _check_dequant_rows(*_mods(None), dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["half", "bfloat16"])
def test_hip_dequant_rows(gpu, dtype):
    _check_dequant_rows(*_mods(gpu), dtype)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["half", "bfloat16"])
@pytest.mark.parametrize("codec", ["hamming84", "golay"])
def test_cpu_shim_read(codec, dtype):
    _check_shim_read(*_mods(None), codec, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["half", "bfloat16"])
@pytest.mark.parametrize("codec", ["hamming84", "golay"])
def test_hip_shim_read(gpu, codec, dtype):
    _check_shim_read(*_mods(gpu), codec, dtype)


# ---- quantize -------------------------------------------------------------------------------------
MAXIMA = [2.0 ** -140, 2.0 ** -126, 2.0 ** -100, 2.0 ** 100, torch.finfo(torch.float32).max]
D = 32


@functools.lru_cache(maxsize=None)
def _rows():
    """fp32 [5, 32]: row i holds +-MAXIMA[i] and fractions of it on and beside the rounding ties."""
    ties = (torch.arange(1, 8) - 0.5) / 7.0  # x / scale = 0.5 .. 6.5
    f = torch.cat([torch.tensor([1.0, -1.0, 0.0, 0.5, -0.5]), ties, -ties, -(torch.arange(1, 14) + 0.4999) / 14.0])
    assert f.numel() == D
    x = (torch.tensor(MAXIMA, dtype=torch.float64).unsqueeze(-1) * f.double()).float()
    assert [float(r.abs().max()) for r in x] == MAXIMA and bool(x.isfinite().all())
    return x.contiguous()


def test_the_reference_sees_the_rows():
    x = _rows()
    for rule in ("div7", "mul_inv7"):
        nib, scale = _reference(x, rule)
        assert float(scale[0]) < 2.0 ** -126 and float(scale[0]) > 0  # a subnormal scale
        assert bool(scale.isfinite().all())
        assert all(int(r.max()) == 15 and int(r.min()) == 1 for r in nib)  # +-7 scales in every row


def _same(nib, scales, rule):
    want_nib, want_scale = _reference(_rows(), rule)
    bad = (nib.cpu() != want_nib).nonzero()
    assert len(bad) == 0, (rule, bad[:8].tolist())
    assert torch.equal(scales.cpu().view(torch.int32), want_scale.view(torch.int32)), (scales.tolist(), want_scale.tolist())


def _check_quantize(mod, dev, rule):
    from kvecc import _lib
    x = _rows() if dev is None else _rows().to(dev)
    nib = torch.zeros(len(MAXIMA), D, dtype=torch.uint8, device=dev)
    scales = torch.zeros(len(MAXIMA), dtype=torch.float32, device=dev)
    mod.quantize_encode_rows_into(x, _lib.CODEC_NONE, nib, scales, rule)
    _same(nib, scales, rule)


def _check_append(mod, dev, rule):
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    x = t(_rows().view(1, len(MAXIMA), D))
    kc, vc = (torch.zeros(1, 1, 1, BS * D, dtype=torch.uint8, device=dev) for _ in range(2))
    ks, vs = (torch.zeros(1, 1, 1, BS, device=dev) for _ in range(2))
    mod.shim_append_tensors(x, x, kc, vc, ks, vs, t(torch.zeros(1, 1, dtype=torch.int32)),
                            t(torch.zeros(1, dtype=torch.int32)), 1, BS, 1, D, 0, "int4", 4, False, 0.0, 0, rule)
    for cache, sc in ((kc, ks), (vc, vs)):
        _same(cache.view(BS, D)[:len(MAXIMA)] & 15, sc.view(BS)[:len(MAXIMA)], rule)
        assert not bool(cache.view(BS, D)[len(MAXIMA):].any())  # the unwritten slots


@pytest.mark.parametrize("rule", ["div7", "mul_inv7"])
def test_cpu_quantize_fp32_rows(rule):
    _check_quantize(*_mods(None), rule)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["div7", "mul_inv7"])
def test_hip_quantize_fp32_rows(gpu, rule):
    _check_quantize(*_mods(gpu), rule)


@pytest.mark.parametrize("rule", ["div7", "mul_inv7"])
def test_cpu_append_fp32_rows(rule):
    _check_append(*_mods(None), rule)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["div7", "mul_inv7"])
def test_hip_append_fp32_rows(gpu, rule):
    _check_append(*_mods(gpu), rule)
