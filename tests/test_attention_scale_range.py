"""Paged attention across the KV scale range.

Every other attention test draws its cache scales from one narrow band around
0.1 .. 1 and is judged by a tolerance whose absolute term dominates, so a kernel
whose relative accuracy depends on the magnitude of `p * v_scale` passes them
all.  Here the cases those files build are run with `v_scales` multiplied by
2^kv and / or `k_scales` by 2^kk (powers of two: the multiplication is exact),
against the same float64 references computed on the inputs actually passed.

Criterion: the suite's own, made scale-relative, no new tolerance --
    |got - ref| <= 2^kv * atol + rtol * |ref|   with (atol, rtol) = TOL[dtype]
element-wise over every element of every sequence; the empty-sequence value
stays exact.

Ladder: fp16 queries kv in {-12, -8, -4, +8, +14} (at -12 the smallest outputs
go fp16-subnormal, at most 2^-25 * 2^12 = 1.2e-4 un-scaled, an eighth of atol;
at +14 the largest output is about 4e4 < 65504); fp32 / bf16 queries kv in
{-24, -12, +14, +24}; every dtype kk in {-6, +6} (a flat and a near one-hot
softmax) and the joint rung (kv, kk) = (-12, +6).

Each test prints `scale-range <family> <rung> <max |got - ref| / 2^kv>` before it
asserts; profiles/scale_range/README.md is that output, tabulated.
"""

import functools
import math

import pytest
import torch

from tests import test_attention_bytes as tbytes
from tests import test_attention_chunk as tchunk
from tests import test_attention_chunk_ragged as tragged
from tests import test_attention_golay_stats as tgstats
from tests import test_attention_interp as tinterp
from tests import test_attention_repair as trepair
from tests import test_attention_stats as tstats
from tests.test_attention_paths import (BF16, EMPTY, F16, F32, LAYER, PATHS, TOL, _TNAME, _attend, _base, _bundle,
                                        _caches, _cdiv, _geometry, _query, _ref64, _select)

# (kv, kk): v_scales * 2^kv, k_scales * 2^kk
V_F16, V_WIDE = (-12, -8, -4, 8, 14), (-24, -12, 14, 24)
K_SIDE, JOINT = ((0, -6), (0, 6)), ((-12, 6),)


def _rungs(dtype):
    return [(kv, 0) for kv in (V_F16 if dtype == F16 else V_WIDE)] + list(K_SIDE) + list(JOINT)


def _rid(r):
    return f"kv{r[0]:+d}-kk{r[1]:+d}"


def _mods(gpu):
    from kvecc import cpu_ops, ops
    return (cpu_ops, None) if gpu is None else (ops, gpu)


def _scaled(c, rung):
    """The case with its scales multiplied (a shallow copy; derived entries such as a cached
    dense read, keyed by a tuple, are dropped)."""
    kv, kk = rung
    out = {k: v for k, v in c.items() if isinstance(k, str)}
    out["vs"], out["ks"] = c["vs"] * 2.0 ** kv, c["ks"] * 2.0 ** kk
    return out


def _check(got, ref, dtype, rung, family, empty_value):
    """The criterion of the module docstring; prints the un-scaled error first."""
    got, kv = got.double(), rung[0]
    atol, rtol = TOL[dtype]
    err = (got - ref).abs()
    print(f"scale-range {family} {_rid(rung)} {float(err.max()) / 2.0 ** kv:.3e}")
    assert not bool(got.isnan().any())
    empty = (ref == empty_value).all(-1)
    assert torch.equal(got[empty], ref[empty])  # the empty value is exact
    excess = err - (2.0 ** kv * atol + rtol * ref.abs())
    assert bool((excess <= 0).all()), (float(err.max()) / 2.0 ** kv, int((excess > 0).sum()))


def _cases(paths, pid):
    return [pytest.param(p, r, id=f"{pid(p)}-{_rid(r)}") for p in paths for r in _rungs(_dtype_of(p))]


def _dtype_of(p):
    return next(x for x in p if isinstance(x, torch.dtype))


# ---- 1. the decode entry ----------------------------------------------------------------------
def _pick(codec, dtype, d, heads):
    return next(p for p in PATHS if p[:4] == (codec, dtype, d, heads))


DECODE_MFMA = [_pick("hamming84", F16, d, h) for d in (32, 64, 128) for h in (2, 8, 32)] + \
              [_pick(c, F16, 128, h) for c in ("golay", "golay_packed") for h in (4, 32)]
# the fp16 ones by PATHS' own trick (a group of 3, or head_dim 100) so they stay off the matrix cores
DECODE_SPLIT = [_pick("hamming84", F32, 64, 8), _pick("hamming84", F16, 128, 6), _pick("hamming84", BF16, 64, 8),
                _pick("golay", F32, 64, 8), _pick("golay", F16, 100, 8), _pick("golay", BF16, 64, 8),
                _pick("golay_packed", F32, 128, 8), _pick("golay_packed", F16, 100, 4),
                _pick("golay_packed", BF16, 128, 8)]
DECODE = DECODE_MFMA + DECODE_SPLIT


def _did(p):
    return f"{p[0]}-{_TNAME[p[1]].strip('_')}-d{p[2]}-{p[3]}q{p[4]}kv"


def _kind(name):
    return "split" if "split_kernel" in name else "golay_mfma" if "golay_mfma" in name else "h84_mfma"


def test_the_decode_paths_are_what_they_say():
    names = [p[6] for p in DECODE_MFMA]
    assert names[:9] == [f"paged_attn_h84_mfma_kernel<{d}, {g}>" for d in (32, 64, 128) for g in (1, 4, 16)]
    assert names[9:] == [f"paged_attn_golay_mfma_kernel<{g}, {pk}>" for pk in ("false", "true") for g in (2, 16)]
    assert all("split_kernel" in p[6] for p in DECODE_SPLIT)
    assert {(p[0], p[1]) for p in DECODE_SPLIT} == {(c, t) for c in ("hamming84", "golay", "golay_packed")
                                                    for t in (F32, F16, BF16)}
    # the bundle's four splits meet in the one-wave combine (or the counted one), the long case's 33 in the block one
    assert _geometry(*DECODE_MFMA[1][:6], 128)[1:] == (4, "paged_attn_combine_wave_kernel<__half>")
    for case in LONG:
        assert _select(*case[:5])[0] == case[6]
        assert _geometry(*case[:6], _cdiv(LONG_LENS[0], 16) * 16)[1:] == (33, "paged_attn_combine_kernel<__half>")


@functools.lru_cache(maxsize=None)
def _decode_ref(path, rung):
    codec, dtype, d, heads, kvh = path[:5]
    c = _scaled(_bundle(codec, dtype, d, heads, kvh, 16), rung)
    return c, _ref64(c["q"], c["kc"], c["vc"], c["table"], c["lens"], c["ks"], c["vs"], LAYER, 16, _base(codec))


def _check_decode(mod, dev, path, rung):
    codec, dtype = path[0], path[1]
    c, ref = _decode_ref(path, rung)
    got = _attend(mod, dev, codec, c["q"], c["kc"], c["vc"], c["table"], c["lens"], c["ks"], c["vs"], LAYER, 16)
    assert bool((ref[2] == EMPTY[codec]).all())  # sequence 2 is empty
    _check(got, ref, dtype, rung, f"decode/{_kind(path[6])}/{_did(path)}", EMPTY[codec])


@pytest.mark.parametrize("path,rung", _cases(DECODE, _did))
def test_cpu_decode(path, rung):
    _check_decode(*_mods(None), path, rung)


@pytest.mark.gpu
@pytest.mark.parametrize("path,rung", _cases(DECODE, _did))
def test_hip_decode(gpu, path, rung):
    _check_decode(*_mods(gpu), path, rung)


# ---- 2. 1030 tokens per matrix-core body: many splits, the fp32 workspace, the block combine -------
LONG = [("hamming84", F16, 128, 8, 2, 2, "paged_attn_h84_mfma_kernel<128, 4>"),
        ("golay", F16, 128, 8, 2, 2, "paged_attn_golay_mfma_kernel<4, false>")]
LONG_LENS = (1030, 513)


@functools.lru_cache(maxsize=None)
def _long_ref(case, rung):
    codec, dtype, d, heads, kvh, batch, _ = case
    nblk = _cdiv(max(LONG_LENS), 16)
    kc, vc, ks, vs = _caches(_base(codec), d, kvh, 16, batch * nblk + 1, 1, 0.01, 11, False)
    table = torch.randperm(batch * nblk + 1, generator=torch.Generator().manual_seed(2))[:batch * nblk]
    table = table.to(torch.int32).view(batch, nblk).contiguous()
    table[0, 1] = -1
    c = _scaled(dict(q=_query(batch, heads, d, dtype, seed=9), kc=kc, vc=vc, ks=ks, vs=vs, table=table,
                     lens=torch.tensor(LONG_LENS, dtype=torch.int32)), rung)
    return c, _ref64(c["q"], kc, vc, table, c["lens"], c["ks"], c["vs"], 0, 16, _base(codec))


def _check_long(mod, dev, case, rung):
    c, ref = _long_ref(case, rung)
    got = _attend(mod, dev, case[0], c["q"], c["kc"], c["vc"], c["table"], c["lens"], c["ks"], c["vs"], 0, 16)
    _check(got, ref, case[1], rung, f"decode-1030/{_kind(case[6])}/{_did(case)}", EMPTY[case[0]])


@pytest.mark.parametrize("case,rung", _cases(LONG, _did))
def test_cpu_long(case, rung):
    _check_long(*_mods(None), case, rung)


@pytest.mark.gpu
@pytest.mark.parametrize("case,rung", _cases(LONG, _did))
def test_hip_long(gpu, case, rung):
    _check_long(*_mods(gpu), case, rung)


# ---- 3. zero V scales ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _zero_case(path):
    """The edge bundle with every V scale of sequence 0's blocks exactly 0 (unwritten slots of a
    zeroed cache) and every other slot of sequence 3's."""
    codec, dtype, d, heads, kvh = path[:5]
    c = dict(_bundle(codec, dtype, d, heads, kvh, 16))
    vs = c["vs"].clone()
    t0 = c["table"][0][c["table"][0] >= 0].long()
    t3 = c["table"][3][c["table"][3] >= 0].long()
    assert not set(t0.tolist()) & set(t3.tolist())
    vs[t0] = 0.0
    vs[t3, :, :, ::2] = 0.0
    c["vs"] = vs
    c["ref"] = _ref64(c["q"], c["kc"], c["vc"], c["table"], c["lens"], c["ks"], vs, LAYER, 16, _base(codec))
    return c


def _check_zero(mod, dev, path):
    codec, dtype = path[0], path[1]
    c = _zero_case(path)
    got = _attend(mod, dev, codec, c["q"], c["kc"], c["vc"], c["table"], c["lens"], c["ks"], c["vs"], LAYER, 16)
    assert bool((c["ref"][0] == 0).all()) and bool((c["ref"][3] != 0).any())
    assert bool((got[0] == 0).all())  # exactly 0 in every lane (which excludes NaN)
    _check(got, c["ref"], dtype, (0, 0), f"zero-v/{_kind(path[6])}/{_did(path)}", EMPTY[codec])


@pytest.mark.parametrize("path", DECODE, ids=_did)
def test_cpu_zero_v_scales(path):
    _check_zero(*_mods(None), path)


@pytest.mark.gpu
@pytest.mark.parametrize("path", DECODE, ids=_did)
def test_hip_zero_v_scales(gpu, path):
    _check_zero(*_mods(gpu), path)


# ---- 4. the chunk entry ------------------------------------------------------------------------------
CHUNK = [p for p in tchunk.MFMA_PATHS if (p[3], p[4]) == (8, 2)] + tchunk.GENERAL_PATHS
CHUNK_Q = (5, 17)


def _ckind(p):
    return _kind(tchunk._chunk_select(*p)[0])


def test_the_chunk_paths_are_what_they_say():
    assert [_ckind(p) for p in CHUNK] == ["h84_mfma"] * 3 + ["golay_mfma"] * 2 + ["split"] * 3


@functools.lru_cache(maxsize=None)
def _chunk_ref(path, q_len, rung):
    c = _scaled(tchunk._bundle(*path, q_len), rung)
    return c, tchunk._ref_chunk(c["q"], c["kc"], c["vc"], c["table"], c["lens"], c["ks"], c["vs"], c["layer"],
                                c["bs"], _base(path[0]))


def _check_chunk(mod, dev, path, q_len, rung):
    codec, dtype = path[0], path[1]
    c, ref = _chunk_ref(path, q_len, rung)
    got, _ = tchunk._attend_chunk(mod, dev, codec, c["q"], c["kc"], c["vc"], c["table"], c["lens"], c["ks"], c["vs"],
                                  c["layer"], c["bs"])
    _check(got, ref, dtype, rung, f"chunk-q{q_len}/{_ckind(path)}/{tchunk._pid(path)}", EMPTY[codec])


@pytest.mark.parametrize("q_len", CHUNK_Q)
@pytest.mark.parametrize("path,rung", _cases(CHUNK, tchunk._pid))
def test_cpu_chunk(path, rung, q_len):
    _check_chunk(*_mods(None), path, q_len, rung)


@pytest.mark.gpu
@pytest.mark.parametrize("q_len", CHUNK_Q)
@pytest.mark.parametrize("path,rung", _cases(CHUNK, tchunk._pid))
def test_hip_chunk(gpu, path, rung, q_len):
    _check_chunk(*_mods(gpu), path, q_len, rung)


# one ragged call: the ragged file's 33-token span table over a matrix-core path
RAGGED_PATH, RAGGED_Q = ("hamming84", F16, 128, 8, 2), 33


@functools.lru_cache(maxsize=None)
def _ragged_ref(rung):
    c = _scaled(tragged._case(*RAGGED_PATH, RAGGED_Q), rung)
    ref = torch.full(c["q"].shape, EMPTY["hamming84"], dtype=torch.float64)
    for b, (f, n) in enumerate(c["spans"]):  # _ref_chunk per sequence on its valid tokens, as the ragged file does
        if n > 0:
            ref[b, f:f + n] = tchunk._ref_chunk(c["q"][b:b + 1, f:f + n], c["kc"], c["vc"], c["table"][b:b + 1],
                                                c["lens"][b:b + 1], c["ks"], c["vs"], c["layer"], c["bs"],
                                                "hamming84")[0]
    return c, ref


def _check_ragged(mod, dev, rung):
    c, ref = _ragged_ref(rung)
    got = tragged._run(mod, dev, RAGGED_PATH[0], c, c["spans"])
    _check(got, ref, F16, rung, f"ragged-q{RAGGED_Q}/h84_mfma/{tchunk._pid(RAGGED_PATH)}", EMPTY["hamming84"])


@pytest.mark.parametrize("rung", _rungs(F16), ids=_rid)
def test_cpu_ragged(rung):
    _check_ragged(*_mods(None), rung)


@pytest.mark.gpu
@pytest.mark.parametrize("rung", _rungs(F16), ids=_rid)
def test_hip_ragged(gpu, rung):
    _check_ragged(*_mods(gpu), rung)


# ---- 5. interp=True on the cache with planted doubles ----------------------------------------------------
INTERP = [tinterp.MFMA_PATHS[1], tinterp.GENERAL_PATHS[0]]  # (F16, 64, 8, 2) matrix-core, (F32, 100, 6, 2) split
INTERP_Q = 5
INTERP_LONG = (F16, 128, 8, 2, 0)  # 1030 tokens through the interpolating matrix-core body


def _ikind(p):
    return "h84_mfma_interp" if tchunk._chunk_mfma_heads("hamming84", *p[:4]) and not p[4] else "split_interp"


def test_the_interp_paths_are_what_they_say():
    assert [_ikind(p) for p in INTERP + [INTERP_LONG]] == ["h84_mfma_interp", "split_interp", "h84_mfma_interp"]


@functools.lru_cache(maxsize=None)
def _interp_ref(path, rung, long):
    dtype, d, heads, kvh, off = path
    q_len = 1 if long else INTERP_Q
    lens = (1030, q_len, 33, 0) if long else tinterp._lens(q_len)
    c = _scaled(tinterp._bundle(d, kvh, lens), rung)
    q = tinterp._query(4, q_len, heads, d, dtype, off, q_len)
    return c, q, tinterp._expect(q, c)


def _check_interp(mod, dev, path, rung, long=False):
    c, q, ref = _interp_ref(path, rung, long)
    assert c["planted"]
    got = tinterp._run(mod, dev, q, c)
    _check(got, ref, path[0], rung, f"interp{'-1030' if long else ''}/{_ikind(path)}/{tinterp._pid(path)}",
           tinterp.EMPTY)


@pytest.mark.parametrize("path,rung", _cases(INTERP, tinterp._pid))
def test_cpu_interp(path, rung):
    _check_interp(*_mods(None), path, rung)


@pytest.mark.gpu
@pytest.mark.parametrize("path,rung", _cases(INTERP, tinterp._pid))
def test_hip_interp(gpu, path, rung):
    _check_interp(*_mods(gpu), path, rung)


@pytest.mark.parametrize("rung", _rungs(F16), ids=_rid)
def test_cpu_interp_long(rung):
    _check_interp(*_mods(None), INTERP_LONG, rung, True)


@pytest.mark.gpu
@pytest.mark.parametrize("rung", _rungs(F16), ids=_rid)
def test_hip_interp_long(gpu, rung):
    _check_interp(*_mods(gpu), INTERP_LONG, rung, True)


# ---- 6. the counted and repairing entries: same counts and cache bytes as at unit scale --------------------
COUNTED_PATH, COUNTED_Q = tinterp.MFMA_PATHS[1], 5
COUNTED_RUNGS = ((-12, 0), (14, 0))


def _check_stats(mod, dev, rung, interp):
    c, q, want = tstats._case(COUNTED_PATH, COUNTED_Q, False)
    cs = _scaled(c, rung)
    got, counts = tstats._run(mod, dev, q, cs, interp)
    assert counts == want and want[0] > 0 and want[1] > 0
    _check(got, tstats._ref(q, cs, interp), COUNTED_PATH[0], rung,
           f"stats-{'interp' if interp else 'plain'}/h84_mfma/{tinterp._pid(COUNTED_PATH)}", tinterp.EMPTY)


@pytest.mark.parametrize("interp", [0, 1], ids=["plain", "interp"])
@pytest.mark.parametrize("rung", COUNTED_RUNGS, ids=_rid)
def test_cpu_stats(rung, interp):
    _check_stats(*_mods(None), rung, interp)


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [0, 1], ids=["plain", "interp"])
@pytest.mark.parametrize("rung", COUNTED_RUNGS, ids=_rid)
def test_hip_stats(gpu, rung, interp):
    _check_stats(*_mods(gpu), rung, interp)


def _check_repair(mod, dev, rung, interp):
    c, q = trepair._case(COUNTED_PATH, COUNTED_Q, False)
    cs = _scaled(c, rung)
    unit_counts = tstats._case(COUNTED_PATH, COUNTED_Q, False)[2]
    want_k, want_v, rewritten = trepair._scrubbed(c)
    assert rewritten > 0
    # the sibling's assertion on the scaled case: the counted entry's output bit for bit, the
    # scrubbed copy's bytes, the scales untouched ...
    call = trepair._check_call(mod, dev, q, cs, interp)
    out, counts = call.run(interp)  # ... and a second call finds the doubles only and rewrites nothing
    assert counts == [unit_counts[0], 2 * unit_counts[1], rewritten]
    kc, vc = call.caches()
    assert torch.equal(kc, want_k) and torch.equal(vc, want_v)  # as at unit scale
    _check(out, tstats._ref(q, cs, interp), COUNTED_PATH[0], rung,  # a repaired byte decodes to what it did
           f"repair-{'interp' if interp else 'plain'}/h84_mfma/{tinterp._pid(COUNTED_PATH)}", tinterp.EMPTY)


@pytest.mark.parametrize("interp", [0, 1], ids=["plain", "interp"])
@pytest.mark.parametrize("rung", COUNTED_RUNGS, ids=_rid)
def test_cpu_repair(rung, interp):
    _check_repair(*_mods(None), rung, interp)


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [0, 1], ids=["plain", "interp"])
@pytest.mark.parametrize("rung", COUNTED_RUNGS, ids=_rid)
def test_hip_repair(gpu, rung, interp):
    _check_repair(*_mods(gpu), rung, interp)


GOLAY_COUNTED = [_pick("golay", F16, 128, 8), _pick("golay_packed", F16, 128, 8)]


def _check_golay_counted(mod, dev, path, rung):
    codec, dtype, d, heads, kvh = path[:5]
    c, q, want, _ = tgstats._case(path, COUNTED_Q, "planted", 0)
    cs = _scaled(c, rung)
    got, counts = tgstats._run(mod, dev, codec, q, cs)
    assert counts == want and want[0] > 0 and want[1] > 0
    _check(got, tgstats._ref_chunk(q, cs), dtype, rung, f"golay-counted/golay_mfma/{_did(path)}", 0.0)


@pytest.mark.parametrize("rung", COUNTED_RUNGS, ids=_rid)
@pytest.mark.parametrize("path", GOLAY_COUNTED, ids=_did)
def test_cpu_golay_counted(path, rung):
    _check_golay_counted(*_mods(None), path, rung)


@pytest.mark.gpu
@pytest.mark.parametrize("rung", COUNTED_RUNGS, ids=_rid)
@pytest.mark.parametrize("path", GOLAY_COUNTED, ids=_did)
def test_hip_golay_counted(gpu, path, rung):
    _check_golay_counted(*_mods(gpu), path, rung)


# ---- 7. the byte codecs, one matrix-core path each -------------------------------------------------------
BYTE_PATH = _pick("hamming84", F16, 128, 8)


@functools.lru_cache(maxsize=None)
def _byte_ref(codec, rung):
    _, dtype, d, heads, kvh = BYTE_PATH[:5]
    c = _scaled(tbytes._decode_bundle(codec, dtype, d, heads, kvh, 16), rung)
    return c, _ref64(c["q"], tbytes._as_h84(codec, c["kc"]), tbytes._as_h84(codec, c["vc"]), c["table"], c["lens"],
                     c["ks"], c["vs"], LAYER, 16, "hamming84")


def _check_bytes(mod, dev, codec, rung):
    c, ref = _byte_ref(codec, rung)
    got = _attend(mod, dev, codec, c["q"], c["kc"], c["vc"], c["table"], c["lens"], c["ks"], c["vs"], LAYER, 16)
    _check(got, ref, F16, rung, f"bytes-{codec}/h84_mfma/{_did(BYTE_PATH)}", tbytes.EMPTY)


@pytest.mark.parametrize("rung", _rungs(F16), ids=_rid)
@pytest.mark.parametrize("codec", tbytes.CODECS)
def test_cpu_bytes(codec, rung):
    _check_bytes(*_mods(None), codec, rung)


@pytest.mark.gpu
@pytest.mark.parametrize("rung", _rungs(F16), ids=_rid)
@pytest.mark.parametrize("codec", tbytes.CODECS)
def test_hip_bytes(gpu, codec, rung):
    _check_bytes(*_mods(gpu), codec, rung)
