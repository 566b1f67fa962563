"""kvecc_paged_attention_chunk_ragged: per-sequence query spans over the chunk kernels.

Contract (include/kvecc.h, "Query spans"): q_spans[b] = (first, count, row_base); token t of row b
is valid iff first >= 0 and first <= t < min(first + count, q_max).  context_lens[b] counts the
sequence's own valid tokens; valid token t sits at p = context_lens[b] - count + (t - first) and
attends as a chunk row at p does.  A padding row gets the empty value in every lane and its query
elements (NaN here) reach no output.  All-full spans return the uniform entry's bits.

Every case runs on the host twin and, marked gpu, on the device.  The reference is
tests/test_attention_chunk.py's float64 `_ref_chunk`, applied per sequence to
q[b, first:first + count] with T = count, under that file's TOL; padding rows and the all-full
equality are exact.

Geometry: batch 6, block_size 16, 2 layers (layer 1), caches noisy at BER 0.01.  context_lens =
count + (0, 41, 5, 96, 50, 0): sequence 0's first valid row sees exactly one key, sequence 4 has
count 0 over a non-empty cache, sequence 3 has a -1 block inside its context.
"""

import ctypes
import functools
import math

import pytest
import torch

from tests.test_attention_chunk import BS, CHUNK_PATHS, LAYER, LAYERS, _bundle, _pid, _ref_chunk
from tests.test_attention_paths import EMPTY, F16, _attend, _base, _caches, _cdiv, _close, _err, _for_codec

SPANS = {
    33: [(0, 33), (16, 17), (13, 20), (0, 7), (0, 0), (32, 1)],  # full, one padded tile, mid-tile, right pad,
    5: [(0, 5), (2, 3), (0, 0), (4, 1), (1, 3), (0, 2)],         # inactive, single last token
}
EXTRA = (0, 41, 5, 96, 50, 0)  # context before the span's own tokens


def _mods(gpu):
    from kvecc import cpu_ops, ops
    return (cpu_ops, None) if gpu is None else (ops, gpu)


def _span_tensor(spans):
    rows, base = [], 0
    for f, c in spans:
        rows.append((f, c, base))
        base += max(c, 0)
    return torch.tensor(rows, dtype=torch.int32)


def _valid(spans, q_max):
    """bool [B, q_max]: the contract's rule, restated."""
    v = torch.zeros(len(spans), q_max, dtype=torch.bool)
    for b, (f, c) in enumerate(spans):
        if f >= 0:
            v[b, f:max(min(f + c, q_max), f)] = True
    return v


def _run(mod, dev, codec, c, spans=None, mcl=0, q=None):
    """paged_attention_chunk_into with q_spans (None: the uniform call) -> the raw output on the host."""
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    q = c["q"] if q is None else q
    pk, pv = _for_codec(codec, q.shape[-1], c["kc"], c["vc"])
    out = torch.empty(q.shape, dtype=q.dtype, device=dev)
    mod.paged_attention_chunk_into(t(q), t(pk), t(pv), t(c["table"]), t(c["lens"]), t(c["ks"]), t(c["vs"]), out,
                                   c["layer"], c["bs"], 1 / math.sqrt(q.shape[-1]), codec, max_context_len=mcl,
                                   q_spans=None if spans is None else t(_span_tensor(spans)))
    return out.cpu()


@functools.lru_cache(maxsize=None)
def _case(codec, dtype, d, heads, kvh, q_max, spans=None):
    """Inputs shared by the host and the device run: padding query elements are NaN."""
    spans = tuple(SPANS[q_max]) if spans is None else spans
    base = _base(codec)
    lens = torch.tensor([c + e for (_, c), e in zip(spans, EXTRA)], dtype=torch.int32)
    nblk = [_cdiv(int(n), BS) for n in lens]
    num_blocks = sum(nblk) + 2
    kc, vc, ks, vs = _caches(base, d, kvh, BS, num_blocks, LAYERS, 0.01, 300 + d, False)
    ids = torch.randperm(num_blocks, generator=torch.Generator().manual_seed(d + q_max)).to(torch.int32).tolist()
    table = torch.full((6, max(nblk) + 1), -1, dtype=torch.int32)
    for b in range(6):
        table[b, :nblk[b]] = torch.tensor([ids.pop() for _ in range(nblk[b])], dtype=torch.int32)
    table[3, nblk[3] // 2] = -1  # tokens inside sequence 3's context are skipped
    q = torch.randn(6, q_max, heads, d, generator=torch.Generator().manual_seed(q_max)).to(dtype)
    q[~_valid(spans, q_max)] = float("nan")
    return dict(q=q, kc=kc, vc=vc, ks=ks, vs=vs, table=table, lens=lens, layer=LAYER, bs=BS, spans=spans)


@functools.lru_cache(maxsize=None)
def _reference(codec, dtype, d, heads, kvh, q_max, mcl, spans=None):
    """float64 [6, q_max, H, d]: _ref_chunk per sequence on its valid tokens, the empty value elsewhere."""
    c = _case(codec, dtype, d, heads, kvh, q_max, spans)
    base = _base(codec)
    ref = torch.full(c["q"].shape, EMPTY[base], dtype=torch.float64)
    for b, (f, n) in enumerate(c["spans"]):
        if n > 0:
            ref[b, f:f + n] = _ref_chunk(c["q"][b:b + 1, f:f + n], c["kc"], c["vc"], c["table"][b:b + 1],
                                         c["lens"][b:b + 1], c["ks"], c["vs"], LAYER, BS, base, mcl)[0]
    return ref


def _check_against_reference(got, ref, valid, codec, dtype):
    got = got.double()
    assert not bool(got.isnan().any())
    assert bool((got[~valid] == EMPTY[_base(codec)]).all())  # padding rows: the empty value, exactly
    print(f"valid rows max err {_err(got[valid], ref[valid]):.3e}")
    assert _close(got[valid], ref[valid], dtype), _err(got[valid], ref[valid])


# ---- 1. the span tables against the reference, max_context_len at its default and below the longest context
def _check_spans(mod, dev, path, q_max):
    codec, dtype = path[0], path[1]
    c = _case(*path, q_max)
    valid = _valid(c["spans"], q_max)
    assert int(c["lens"].max()) > 64
    for mcl in (0, 64):
        got = _run(mod, dev, codec, c, c["spans"], mcl)
        _check_against_reference(got, _reference(*path, q_max, mcl), valid, codec, dtype)


def test_the_cases_are_what_they_say():
    for q_max, spans in SPANS.items():
        v = _valid(spans, q_max)
        assert [int(n) for n in v.sum(1)] == [c for _, c in spans]
        assert not bool(v[[b for b, s in enumerate(spans) if s[1] == 0]].any())
    assert not bool(_valid(SPANS[33], 33)[1, :16].any())  # a whole 16-token tile of padding
    ref = _reference(*CHUNK_PATHS[0], 33, 0)
    c = _case(*CHUNK_PATHS[0], 33)
    assert int(c["lens"][0]) == 33 and int(c["lens"][4]) == 50 and bool((c["table"][3, :6] == -1).any())
    assert bool((ref[4] == EMPTY["hamming84"]).all()) and not bool((ref[0, 0] == EMPTY["hamming84"]).all())


@pytest.mark.parametrize("q_max", sorted(SPANS))
@pytest.mark.parametrize("path", CHUNK_PATHS, ids=_pid)
def test_cpu_spans(path, q_max):
    _check_spans(*_mods(None), path, q_max)


@pytest.mark.gpu
@pytest.mark.parametrize("q_max", sorted(SPANS))
@pytest.mark.parametrize("path", CHUNK_PATHS, ids=_pid)
def test_hip_spans(gpu, path, q_max):
    _check_spans(*_mods(gpu), path, q_max)


def test_matrix_core_paths_ran_the_ragged_kernels():
    """profiles/ragged_attention/kernels.txt is the kernel trace of this file's gpu tests: every
    matrix-core path's ragged call ran the ragged matrix-core kernel of its codec and head_dim, the
    general paths the split chunk kernels, and the uniform calls of section 2 the uniform kernels."""
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ragged_attention",
                        "kernels.txt")
    traced = {ln.strip() for ln in open(path) if ln.strip()}
    want = set()
    for codec, dtype, d, heads, kvh in CHUNK_PATHS:
        if dtype != F16:
            continue
        for kind, args in (("ragged", "RaggedArgs"), ("chunk", "ChunkArgs")):
            name = (f"paged_attn_h84_mfma_{kind}_kernel<{d}>" if codec == "hamming84" else
                    f"paged_attn_golay_mfma_{kind}_kernel<{'true' if codec == 'golay_packed' else 'false'}>")
            want.add(f"void kvecc::{name}(kvecc::{args})")
    assert len(want) == 10 and want <= traced, sorted(want - traced)
    assert {t for t in traced if "mfma_ragged" in t or "mfma_chunk" in t} == want
    general = {t for t in traced if "split_chunk_kernel" in t}
    assert {t.split("<")[1].split(",")[0] for t in general} >= {"float", "__hip_bfloat16"}
    assert all(t.endswith("(kvecc::RaggedArgs)") for t in general)


# ---- 2. all-full spans are the uniform call, bit for bit ----------------------------------------
def _check_full(mod, dev, path):
    c = _bundle(*path, 17)  # the chunk tests' edge bundle, batch 5
    spans = [(0, 17)] * 5
    for mcl in (0, int(c["lens"].max())):
        assert torch.equal(_run(mod, dev, path[0], c, spans, mcl), _run(mod, dev, path[0], c, None, mcl)), mcl


@pytest.mark.parametrize("path", CHUNK_PATHS, ids=_pid)
def test_cpu_full_spans_are_the_uniform_call(path):
    _check_full(*_mods(None), path)


@pytest.mark.gpu
@pytest.mark.parametrize("path", CHUNK_PATHS, ids=_pid)
def test_hip_full_spans_are_the_uniform_call(gpu, path):
    _check_full(*_mods(gpu), path)


# ---- 3. a span that moves changes its own sequence only -----------------------------------------
SENSITIVE = [CHUNK_PATHS[4], CHUNK_PATHS[9], CHUNK_PATHS[15]]  # 4 and 16 tokens per tile, the general path


def _check_sensitivity(mod, dev, path):
    c = _case(*path, 33)
    moved = list(c["spans"])
    moved[2] = (12, 20)  # was (13, 20): row 12 becomes a query row, row 32 padding
    q = c["q"].clone()
    q[2, 12] = torch.randn(q.shape[2:], generator=torch.Generator().manual_seed(5)).to(q.dtype)
    a = _run(mod, dev, path[0], c, c["spans"], q=q)
    b = _run(mod, dev, path[0], c, moved, q=q)
    others = [0, 1, 3, 4, 5]
    assert torch.equal(a[others], b[others])
    empty = EMPTY[_base(path[0])]
    assert bool((a[2, 12] == empty).all()) and not bool((b[2, 12] == empty).all())
    assert bool((b[2, 32] == empty).all()) and not bool((a[2, 32] == empty).all())
    assert not torch.equal(a[2, 13:32], b[2, 13:32])  # every row moved one position down
    assert not bool(b.double().isnan().any())


@pytest.mark.parametrize("path", SENSITIVE, ids=_pid)
def test_cpu_sensitivity(path):
    _check_sensitivity(*_mods(None), path)


@pytest.mark.gpu
@pytest.mark.parametrize("path", SENSITIVE, ids=_pid)
def test_hip_sensitivity(gpu, path):
    _check_sensitivity(*_mods(gpu), path)


# ---- 4. one chunk beside single tokens: the single rows are decode steps -------------------------
def _check_mixed(mod, dev, path):
    codec, dtype = path[0], path[1]
    for firsts in ((0, 15, 15, 15), (0, 0, 0, 0)):  # right- and left-aligned
        spans = tuple((f, n) for f, n in zip(firsts, (16, 1, 1, 1))) + ((0, 0), (0, 0))
        c = _case(*path, 16, spans)
        got = _run(mod, dev, codec, c, spans)
        _check_against_reference(got, _reference(*path, 16, 0, spans), _valid(spans, 16), codec, dtype)
        rows = torch.stack([c["q"][b, firsts[b]] for b in (1, 2, 3)])  # [3, H, d]
        dec = _attend(mod, dev, codec, rows, c["kc"], c["vc"], c["table"][1:4].contiguous(), c["lens"][1:4].clone(),
                      c["ks"], c["vs"], LAYER, BS)
        mine = torch.stack([got[b, firsts[b]] for b in (1, 2, 3)]).double()
        print(f"single-token rows against the decode entry: max err {_err(mine, dec):.3e}")
        assert _close(mine, dec, dtype), _err(mine, dec)


@pytest.mark.parametrize("path", CHUNK_PATHS, ids=_pid)
def test_cpu_mixed_batch(path):
    _check_mixed(*_mods(None), path)


@pytest.mark.gpu
@pytest.mark.parametrize("path", CHUNK_PATHS, ids=_pid)
def test_hip_mixed_batch(gpu, path):
    _check_mixed(*_mods(gpu), path)


# ---- 5. q_max 1 ------------------------------------------------------------------------------------
ONE = [CHUNK_PATHS[1], CHUNK_PATHS[10], CHUNK_PATHS[16]]


def _check_one(mod, dev, path):
    spans = ((0, 1), (0, 0), (0, 1), (0, 1), (0, 0), (0, 1))
    c = _case(*path, 1, spans)
    got = _run(mod, dev, path[0], c, spans)
    _check_against_reference(got, _reference(*path, 1, 0, spans), _valid(spans, 1), path[0], path[1])


@pytest.mark.parametrize("path", ONE, ids=_pid)
def test_cpu_one_token_rows(path):
    _check_one(*_mods(None), path)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ONE, ids=_pid)
def test_hip_one_token_rows(gpu, path):
    _check_one(*_mods(gpu), path)


# ---- 6. the Python layer, the dispatcher and the C ABI ------------------------------------------
SMALL = ("hamming84", F16, 32, 2, 2)


def _small(dev=None):
    c = _case(*SMALL, 5)
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    a = {k: t(c[k]) for k in ("q", "kc", "vc", "table", "lens", "ks", "vs")}
    a["spans"] = t(_span_tensor(c["spans"]))
    a["out"] = torch.full(c["q"].shape, 77.0, dtype=c["q"].dtype, device=dev)
    return a


def _call(mod, a, spans):
    return mod.paged_attention_chunk_into(a["q"], a["kc"], a["vc"], a["table"], a["lens"], a["ks"], a["vs"],
                                          a["out"], LAYER, BS, 1 / math.sqrt(32), "hamming84", q_spans=spans)


def _check_validation(mod, dev, other=None):
    a = _small(dev)
    sp = a["spans"]
    bad = [sp.to(torch.int64), sp[:, :2].contiguous(), sp[:5].contiguous(), sp.reshape(-1),
           torch.zeros((6, 6), dtype=torch.int32, device=dev)[:, ::2], sp.tolist()]
    if other is not None:
        bad.append(sp.to(other))
    for spans in bad:
        with pytest.raises(ValueError):
            _call(mod, a, spans)
        assert bool((a["out"] == 77.0).all())  # nothing was launched
    _call(mod, a, sp)
    assert not bool((a["out"] == 77.0).any())


def test_cpu_validation():
    _check_validation(*_mods(None))


@pytest.mark.gpu
def test_hip_validation(gpu):
    _check_validation(*_mods(gpu), other="cpu")


def _op_args(a):
    return (a["q"], a["kc"], a["vc"], a["table"], a["lens"], a["spans"], a["ks"], a["vs"], LAYER, BS,
            1 / math.sqrt(32), "hamming84")


def _check_dispatcher(mod, dev):
    import kvecc
    from kvecc import torch_ops
    assert "paged_attention_chunk_ragged" in torch_ops.OPS
    a = _small(dev)
    got = torch.ops.kvecc.paged_attention_chunk_ragged(*_op_args(a))
    _call(mod, a, a["spans"])
    assert torch.equal(got, a["out"])
    pub = kvecc.paged_attention_chunk(a["q"], a["kc"], a["vc"], a["table"], a["lens"], a["ks"], a["vs"], LAYER, BS,
                                      q_spans=a["spans"])
    assert torch.equal(pub, got)
    torch.library.opcheck(torch.ops.kvecc.paged_attention_chunk_ragged.default, _op_args(a))


def test_cpu_dispatcher_op():
    _check_dispatcher(*_mods(None))


@pytest.mark.gpu
def test_hip_dispatcher_op(gpu):
    _check_dispatcher(*_mods(gpu))


def _abi_args(a, spans, tail):
    from kvecc import _lib
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())  # noqa: E731
    q = a["q"]
    return [p(q), q.stride(0), q.stride(1), q.stride(2), _lib.F16, p(a["kc"]), p(a["vc"]), p(a["table"]),
            p(a["lens"]), p(spans), p(a["ks"]), p(a["vs"]), p(a["out"]), 6, 5, 2, 2, 32, a["kc"].shape[0], LAYERS,
            LAYER, BS, a["table"].shape[1], 0, 1 / math.sqrt(32), _lib.CODEC_H84] + tail


def test_cpu_null_spans_are_einval():
    from kvecc import _lib
    lib = _lib.load()
    a = _small()
    assert lib.kvecc_cpu_paged_attention_chunk_ragged(*_abi_args(a, None, [1])) == -1  # KVECC_EINVAL
    assert "q_spans" in lib.kvecc_last_error().decode()
    assert bool((a["out"] == 77.0).all())
    assert lib.kvecc_cpu_paged_attention_chunk_ragged(*_abi_args(a, a["spans"], [1])) == 0
    assert not bool((a["out"] == 77.0).any())


@pytest.mark.gpu
def test_hip_null_spans_are_einval(gpu):
    from kvecc import _lib
    lib = _lib.load()
    a = _small(gpu)
    n = lib.kvecc_paged_attention_chunk_workspace(6, 5, 2, 32, a["table"].shape[1] * BS)
    ws = torch.empty(n, dtype=torch.float32, device=gpu)
    tail = [ctypes.c_void_p(ws.data_ptr()), n, None]
    assert lib.kvecc_paged_attention_chunk_ragged(*_abi_args(a, None, tail)) == -1  # KVECC_EINVAL
    assert "q_spans" in lib.kvecc_last_error().decode()
    torch.cuda.synchronize()
    assert bool((a["out"] == 77.0).all())
    assert lib.kvecc_paged_attention_chunk_ragged(*_abi_args(a, a["spans"], tail)) == 0
    torch.cuda.synchronize()
    assert not bool((a["out"] == 77.0).any())


def test_query_spans_helpers():
    import kvecc
    t = kvecc.query_spans([5, 3, 0, 2], firsts=[0, 2, 0, 1], q_max=5)
    assert t.dtype == torch.int32 and t.tolist() == [[0, 5, 0], [2, 3, 5], [0, 0, 8], [1, 2, 8]]
    assert kvecc.query_spans([2, 1]).tolist() == [[0, 2, 0], [0, 1, 2]]
    for bad in (dict(counts=[-1]), dict(counts=[1], firsts=[-1]), dict(counts=[3], firsts=[3], q_max=5),
                dict(counts=[1, 2], firsts=[0])):
        with pytest.raises(ValueError):
            kvecc.query_spans(**bad)
    mask = torch.tensor([[1, 1, 1], [0, 1, 1], [0, 0, 0], [0, 1, 0]])
    assert kvecc.query_spans_from_mask(mask) == ([3, 2, 0, 1], [0, 1, 0, 1])
    with pytest.raises(ValueError):
        kvecc.query_spans_from_mask(torch.tensor([[1, 0, 1]]))
    with pytest.raises(ValueError):
        kvecc.query_spans_from_mask(torch.ones(3))
