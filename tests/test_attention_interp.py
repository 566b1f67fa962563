"""kvecc_paged_attention_interp: paged attention over a Hamming(8,4) cache whose
detected double errors are interpolated from the neighbouring tokens inside the
kernel (include/kvecc.h "Interpolated attention").

Expectation: a float64 attention over K / V read per sequence by
cpu_ops.shim_read_batch(table[b:b+1], ctx = n_b, interp=True, float32) -- the
host read the golden tests pin to the reference's interpolating shim -- with the
rows of -1 blocks masked out.  Tolerance: the suite's TOL of the query dtype.
Every case runs on the host twin and, marked gpu, on the device.

The planted bundle: batch 4, block_size 16, 2 layers (layer 1 read), lengths
[q_len + 70, q_len, 33, 0].  The caches hold valid codewords, about 5 % of them
with one flipped bit; whole token rows of seeded random bytes (every kv head, K
and V) are planted at
  sequence 0: 0, 1 (consecutive doubles, left clamp), 15, 16 (block and tile
              boundary), 31, 32 (step boundary, split boundary at the smallest
              split), 47 (its right neighbour lies in the -1 block 48..63), 64
              (its left neighbour does), n - 2, n - 1 (the key whose right
              neighbour is a later chunk token, and the right clamp);
  sequence 1: 0, 1, n - 2, n - 1 where they exist -- at q_len 1 none: a
              sequence of one token interpolates from itself alone, which changes
              nothing, so it holds no planted row;
  sequence 2: 0, 1, 15, 16, 31, 32 = n - 2, n - 1; its block 1 is the cache's
              last block, so position 31 of the last kv head is the buffer's last row.
"""

import ctypes
import functools
import math

import pytest
import torch

from tests.test_attention_chunk import _chunk_geometry, _chunk_mfma_heads, _ref_chunk
from tests.test_attention_paths import BF16, F16, F32, TOL, _TNAME, _caches, _cdiv, _close, _err, _for_codec

LAYERS, LAYER, BS = 2, 1, 16
CODEC = "hamming84"
EMPTY = -8.0

# (query dtype, head_dim, heads, kv_heads, query offset in elements from a 16-byte boundary)
MFMA_PATHS = [(F16, 128, 4, 4, 0), (F16, 64, 8, 2, 0), (F16, 32, 16, 1, 0)]  # 16 / 4 / 1 tokens per tile
GENERAL_PATHS = [(F32, 100, 6, 2, 0), (BF16, 20, 2, 2, 0), (F16, 128, 8, 2, 4)]  # the last: 8 bytes off alignment
PATHS = MFMA_PATHS + GENERAL_PATHS
Q_LENS = [1, 2, 5, 16, 17]


def _pid(p):
    return f"{_TNAME[p[0]].strip('_')}-d{p[1]}-{p[2]}q{p[3]}kv" + ("-unaligned" if p[4] else "")


def _mods(gpu):
    from kvecc import cpu_ops, ops
    return (cpu_ops, None) if gpu is None else (ops, gpu)


def test_paths_are_what_they_say():
    assert [_chunk_mfma_heads(CODEC, p[0], p[1], p[2], p[3]) for p in MFMA_PATHS] == [1, 4, 16]
    assert [_chunk_mfma_heads(CODEC, p[0], p[1], p[2], p[3]) for p in GENERAL_PATHS[:2]] == [0, 0]
    assert _chunk_mfma_heads(CODEC, *GENERAL_PATHS[2][:4]) == 4 and GENERAL_PATHS[2][4] * 2 % 16 == 8


# ---- caches ---------------------------------------------------------------------------------------
def _random_rows(n_bytes, seed):
    """Seeded random bytes in which every run of 256 is a permutation of 0..255."""
    g = torch.Generator().manual_seed(seed)
    runs = [torch.randperm(256, generator=g) for _ in range(_cdiv(n_bytes, 256))]
    return torch.cat(runs)[:n_bytes].to(torch.uint8)


def _types(x):
    from kvecc import cpu_ops
    return cpu_ops.hamming84_decode(x.contiguous(), return_error_types=True)[1]


def _planted_positions(lens):
    n0, n1, n2 = lens[0], lens[1], lens[2]
    p1 = sorted({p for p in (0, 1, n1 - 2, n1 - 1) if 0 <= p < n1}) if n1 > 1 else []
    return {0: sorted({0, 1, 15, 16, 31, 32, 47, 64, n0 - 2, n0 - 1}), 1: p1,
            2: sorted({0, 1, 15, 16, 31, 32, n2 - 2, n2 - 1})}


@functools.lru_cache(maxsize=None)
def _bundle(d, kvh, lens, random_cache=False, plant=True):
    """-> dict(kc, vc, ks, vs, table, lens, planted): the module docstring's bundle at these lengths."""
    lens = list(lens)
    nblk = [_cdiv(n, BS) for n in lens]
    num_blocks = sum(nblk) + 3
    kc, vc, ks, vs = _caches(CODEC, d, kvh, BS, num_blocks, LAYERS, 0.0, 400 + d, False)
    kc, vc = kc.clone(), vc.clone()
    g = torch.Generator().manual_seed(d + sum(lens))
    if random_cache:
        for c in (kc, vc):
            c.copy_(torch.randint(0, 256, c.shape, generator=g, dtype=torch.uint8))
    else:  # one flipped bit in about 5 % of the codewords
        for c in (kc, vc):
            hit = torch.rand(c.shape, generator=g) < 0.05
            bit = torch.randint(0, 8, c.shape, generator=g)
            c ^= torch.where(hit, 1 << bit, 0).to(torch.uint8)
            assert not bool((_types(c) == 2).any())
    ids = (1 + torch.randperm(num_blocks - 2, generator=torch.Generator().manual_seed(d))).to(torch.int32).tolist()
    table = torch.full((4, max(nblk) + 2), -1, dtype=torch.int32)
    for b in range(4):
        for j in range(nblk[b]):
            table[b, j] = ids.pop()
    if nblk[2] > 1:
        table[2, 1] = num_blocks - 1  # positions 16..31: the buffer's last row is position 31, last kv head
    if nblk[0] > 4:
        table[0, 3] = -1  # positions 48..63 are skipped; 47 and 64 have a neighbour there
    planted = []
    if plant and not random_cache:
        rows = [(b, p) for b, ps in _planted_positions(lens).items() for p in ps if int(table[b, p // BS]) >= 0]
        data = _random_rows(2 * len(rows) * kvh * d, 7 * d + len(rows)).view(2, len(rows), kvh, d)
        for i, (b, p) in enumerate(rows):
            blk = int(table[b, p // BS])
            for side, c in enumerate((kc, vc)):
                c.view(num_blocks, LAYERS, kvh, BS, d)[blk, LAYER, :, p % BS] = data[side, i]
        planted = rows
    return dict(kc=kc, vc=vc, ks=ks, vs=vs, table=table, lens=torch.tensor(lens, dtype=torch.int32),
                planted=planted, planted_bytes=data if planted else None)


def _query(batch, q_len, heads, d, dtype, off, seed, nan_where=None):
    """[batch, q_len, heads, d] random query `off` elements past a 16-byte boundary."""
    buf = torch.zeros(off + batch * q_len * heads * d + 16, dtype=dtype)
    skew = (-buf.data_ptr() % 16) // buf.element_size()  # elements to the next 16-byte boundary
    q = buf[skew + off:skew + off + batch * q_len * heads * d].view(batch, q_len, heads, d)
    q.copy_(torch.randn(batch, q_len, heads, d, generator=torch.Generator().manual_seed(seed)).to(dtype))
    if nan_where is not None:
        q[nan_where] = float("nan")
    assert q.data_ptr() % 16 == off * buf.element_size() % 16
    return q


# ---- the expectation ---------------------------------------------------------------------------------
def _expect(q, c, spans=None, mcl=0):
    """float64 [B, T, H, d]: per sequence, K / V = the interpolating host read at ctx = n_b; token t
    of span (first, count) sits at lens[b] - count + (t - first) and sees the keys at or before it
    whose block is not -1; rows without a key, and padding rows, hold the empty value."""
    from kvecc import cpu_ops
    b_, t_, h_, d = q.shape
    kvh = c["kc"].shape[2]
    table, lens = c["table"], c["lens"]
    cap = table.shape[1] * BS if mcl <= 0 else min(mcl, table.shape[1] * BS)
    out = torch.full((b_, t_, h_, d), EMPTY, dtype=torch.float64)
    for b in range(b_):
        first, count = (0, t_) if spans is None else spans[b]
        nb = min(max(int(lens[b]), 0), cap)
        if nb == 0 or count <= 0:
            continue
        k, v = cpu_ops.shim_read_batch(c["kc"], c["vc"], c["ks"], c["vs"], table[b:b + 1].contiguous(), nb, d, LAYER,
                                       CODEC, torch.float32, interp=True)
        k, v = k[0].double(), v[0].double()  # [kvh, nb, d]
        pos = torch.arange(nb)
        has_block = table[b, pos // BS] >= 0
        t = torch.arange(first, min(first + count, t_))
        qpos = int(lens[b]) - count + (t - first)
        seen = (pos[None, :] <= qpos[:, None]) & has_block[None, :]  # [T', nb]
        qb = torch.nan_to_num(q[b, t].double()).view(len(t), kvh, h_ // kvh, d)
        s = torch.einsum("tkgd,knd->tkgn", qb, k) / math.sqrt(d)
        s = s.masked_fill(~seen[:, None, None, :], -math.inf)
        live = seen.any(1)
        o = torch.einsum("tkgn,knd->tkgd", torch.softmax(s[live], dim=-1), v).reshape(-1, h_, d)
        out[b, t[live]] = o
    return out


def _run(mod, dev, q, c, spans=None, mcl=0, interp=True):
    """paged_attention_chunk_into(interp=...) on q as given (strides and offset from a 16-byte
    boundary kept) -> the raw output on the host."""
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    if dev is not None:
        off = (q.data_ptr() % 16) // q.element_size()
        qd = torch.empty(off + q.numel() + 16, dtype=q.dtype, device=dev)
        skew = (-qd.data_ptr() % 16) // q.element_size()
        qd = qd[skew + off:skew + off + q.numel()].view(q.shape)
        qd.copy_(q)
        assert qd.data_ptr() % 16 == q.data_ptr() % 16
    else:
        qd = q
    sp = None
    if spans is not None:
        rows, base = [], 0
        for f, n in spans:
            rows.append((f, n, base))
            base += max(n, 0)
        sp = t(torch.tensor(rows, dtype=torch.int32))
    out = torch.full(q.shape, 77.0, dtype=q.dtype, device=dev)
    mod.paged_attention_chunk_into(qd, t(c["kc"]), t(c["vc"]), t(c["table"]), t(c["lens"]), t(c["ks"]), t(c["vs"]),
                                   out, LAYER, BS, 1 / math.sqrt(q.shape[-1]), CODEC, max_context_len=mcl,
                                   q_spans=sp, interp=interp)
    return out.cpu()


def _check(got, ref, dtype, what=""):
    got = got.double()
    assert not bool(got.isnan().any()), what
    empty = (ref == EMPTY).all(-1)
    assert torch.equal(got[empty], ref[empty]), what  # the empty value is exact
    print(f"{what} max err {_err(got, ref):.3e}")
    assert _close(got, ref, dtype), (what, _err(got, ref))


# ---- 1. the planted edge bundle ------------------------------------------------------------------
def _lens(q_len):
    return (q_len + 70, q_len, 33, 0)


@functools.lru_cache(maxsize=None)
def _planted_case(path, q_len):
    dtype, d, heads, kvh, off = path
    c = _bundle(d, kvh, _lens(q_len))
    q = _query(4, q_len, heads, d, dtype, off, q_len)
    return c, q, _expect(q, c)


def test_planted_rows_are_what_they_say():
    for path in PATHS:
        dtype, d, heads, kvh, _ = path
        atol, rtol = TOL[dtype]
        for q_len in Q_LENS:
            c, q, ref = _planted_case(path, q_len)
            rows = c["planted"]
            got = {b: [p for bb, p in rows if bb == b] for b in range(3)}
            assert got == _planted_positions(list(_lens(q_len)))
            assert {47, 64} <= set(got[0]) and int(c["table"][0, 3]) == -1
            assert int(c["table"][2, 1]) == c["kc"].shape[0] - 1  # position 31: the buffer's last row
            data = c["planted_bytes"]
            assert len(torch.unique(data)) == 256
            doubles = int((_types(data) == 2).sum())
            assert doubles >= 100, doubles
            # ... and the cache holds them: the planted rows read back
            blk = int(c["table"][2, 1])
            i = rows.index((2, 31))
            assert torch.equal(c["vc"].view(-1, LAYERS, kvh, BS, d)[blk, LAYER, :, 15], data[1, i])
            # a kernel that ignores doubles cannot pass: the expectation moves by more than 10 x TOL
            plain = _ref_chunk(q, c["kc"], c["vc"], c["table"], c["lens"], c["ks"], c["vs"], LAYER, BS, CODEC)
            for b in range(3):
                if not got[b]:
                    assert (b, q_len) == (1, 1)
                    continue
                excess = ((ref[b] - plain[b]).abs() / (atol + rtol * ref[b].abs())).max()
                assert float(excess) > 10, (path, q_len, b, float(excess))


def _check_planted(mod, dev, path, q_len):
    c, q, ref = _planted_case(path, q_len)
    for mcl in (0, int(c["lens"].max()) - 1):  # the default bound, and one that cuts the longest sequence's last token
        r = ref if mcl == 0 else _expect(q, c, mcl=mcl)
        _check(_run(mod, dev, q, c, mcl=mcl), r, path[0], f"mcl {mcl}")


@pytest.mark.parametrize("q_len", Q_LENS)
@pytest.mark.parametrize("path", PATHS, ids=_pid)
def test_cpu_planted_bundle(path, q_len):
    _check_planted(*_mods(None), path, q_len)


@pytest.mark.gpu
@pytest.mark.parametrize("q_len", Q_LENS)
@pytest.mark.parametrize("path", PATHS, ids=_pid)
def test_hip_planted_bundle(gpu, path, q_len):
    _check_planted(*_mods(gpu), path, q_len)


# ---- 2. a cache of random bytes: 44 % doubles, consecutive doubles the norm --------------------
def _check_random(mod, dev, path):
    dtype, d, heads, kvh, off = path
    c = _bundle(d, kvh, _lens(16), random_cache=True)
    frac = float((_types(c["kc"]) == 2).float().mean())
    assert 0.40 < frac < 0.48, frac  # 112 / 256
    q = _query(4, 16, heads, d, dtype, off, 3)
    _check(_run(mod, dev, q, c), _expect(q, c), dtype, "random bytes")


@pytest.mark.parametrize("path", PATHS, ids=_pid)
def test_cpu_random_byte_cache(path):
    _check_random(*_mods(None), path)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS, ids=_pid)
def test_hip_random_byte_cache(gpu, path):
    _check_random(*_mods(gpu), path)


# ---- 3. a larger split: neighbours cross wave steps inside a workgroup, and workgroups ---------
BIG = dict(batch=32, heads=16, kvh=16, d=32, ctx=128)


def _check_larger_split(mod, dev):
    split, nsplit = _chunk_geometry(CODEC, F16, BIG["d"], BIG["heads"], BIG["kvh"], BIG["batch"], 1, BIG["ctx"])
    assert split >= 64 and nsplit >= 2, (split, nsplit)
    nblk = BIG["ctx"] // BS
    g = torch.Generator().manual_seed(11)
    num_blocks = BIG["batch"] * nblk
    kc = torch.randint(0, 256, (num_blocks, LAYERS, BIG["kvh"], BS * BIG["d"]), generator=g, dtype=torch.uint8)
    vc = torch.randint(0, 256, kc.shape, generator=g, dtype=torch.uint8)
    ks = torch.rand(num_blocks, LAYERS, BIG["kvh"], BS, generator=g) * 0.3 + 0.05
    vs = torch.rand(num_blocks, LAYERS, BIG["kvh"], BS, generator=g) * 0.3 + 0.05
    table = torch.randperm(num_blocks, generator=g).to(torch.int32).view(BIG["batch"], nblk).contiguous()
    lens = torch.full((BIG["batch"],), BIG["ctx"], dtype=torch.int32)
    lens[:6] = torch.tensor([127, 100, 65, 64, 33, 1], dtype=torch.int32)
    c = dict(kc=kc, vc=vc, ks=ks, vs=vs, table=table, lens=lens)
    q = _query(BIG["batch"], 1, BIG["heads"], BIG["d"], F16, 0, 5)
    _check(_run(mod, dev, q, c, mcl=BIG["ctx"]), _expect(q, c, mcl=BIG["ctx"]), F16, "larger split")


def test_cpu_larger_split():
    _check_larger_split(*_mods(None))


@pytest.mark.gpu
def test_hip_larger_split(gpu):
    _check_larger_split(*_mods(gpu))


# ---- 4. a cache without doubles: the plain chunk entry ----------------------------------------
def _check_double_free(mod, dev, path):
    dtype, d, heads, kvh, off = path
    c = _bundle(d, kvh, _lens(5), plant=False)
    assert not bool((_types(c["kc"]) == 2).any()) and bool((_types(c["kc"]) == 1).any())
    q = _query(4, 5, heads, d, dtype, off, 9)
    got, plain = _run(mod, dev, q, c), _run(mod, dev, q, c, interp=False)
    print(f"max |interp - plain| {_err(got.double(), plain.double()):.3e}")
    assert _close(got.double(), plain.double(), dtype)
    _check(got, _expect(q, c), dtype, "double-free")


@pytest.mark.parametrize("path", PATHS, ids=_pid)
def test_cpu_double_free_cache_is_the_chunk_entry(path):
    _check_double_free(*_mods(None), path)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS, ids=_pid)
def test_hip_double_free_cache_is_the_chunk_entry(gpu, path):
    _check_double_free(*_mods(gpu), path)


# ---- 5. ragged calls ---------------------------------------------------------------------------
# (q_max, spans (first, count), context before the span's own tokens)
RAGGED = [
    (17, ((0, 17), (16, 1), (3, 9), (0, 0)), (54, 20, 24, 33)),  # first > 0, a padding tile (16 per tile), count 0
    (5, ((1, 4), (4, 1), (0, 0), (0, 2)), (66, 0, 33, 31)),     # a padding tile at 1 and 4 tokens per tile
    (1, ((0, 1), (0, 0), (0, 1), (0, 1)), (70, 12, 32, 0)),     # q_max 1: the decode step over spans
]


def _valid(spans, q_max):
    v = torch.zeros(len(spans), q_max, dtype=torch.bool)
    for b, (f, n) in enumerate(spans):
        v[b, f:f + n] = True
    return v


def _check_ragged(mod, dev, path, case):
    dtype, d, heads, kvh, off = path
    q_max, spans, extra = case
    lens = tuple(n + e for (_, n), e in zip(spans, extra))
    c = _bundle(d, kvh, lens)
    valid = _valid(spans, q_max)
    q = _query(4, q_max, heads, d, dtype, off, q_max, nan_where=~valid)  # padding query elements are NaN
    got = _run(mod, dev, q, c, spans)
    assert bool((got[~valid].double() == EMPTY).all())
    _check(got, _expect(q, c, spans), dtype, f"ragged q_max {q_max}")


@pytest.mark.parametrize("case", RAGGED, ids=lambda c: f"qmax{c[0]}")
@pytest.mark.parametrize("path", PATHS, ids=_pid)
def test_cpu_ragged(path, case):
    _check_ragged(*_mods(None), path, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", RAGGED, ids=lambda c: f"qmax{c[0]}")
@pytest.mark.parametrize("path", PATHS, ids=_pid)
def test_hip_ragged(gpu, path, case):
    _check_ragged(*_mods(gpu), path, case)


def _check_full_spans(mod, dev, path):
    c, q, _ = _planted_case(path, 17)
    assert torch.equal(_run(mod, dev, q, c, [(0, 17)] * 4), _run(mod, dev, q, c))


@pytest.mark.parametrize("path", PATHS, ids=_pid)
def test_cpu_full_spans_are_the_uniform_call(path):
    _check_full_spans(*_mods(None), path)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS, ids=_pid)
def test_hip_full_spans_are_the_uniform_call(gpu, path):
    _check_full_spans(*_mods(gpu), path)


# ---- 6. the one-token wrapper, argument errors, the dispatcher operator -----------------------
def _check_decode_wrapper(mod, dev):
    path = MFMA_PATHS[1]
    c, q, ref = _planted_case(path, 1)
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    out = torch.empty(q[:, 0].shape, dtype=q.dtype, device=dev)
    mod.paged_attention_into(t(q[:, 0].contiguous()), t(c["kc"]), t(c["vc"]), t(c["table"]), t(c["lens"]), t(c["ks"]),
                             t(c["vs"]), out, LAYER, BS, 1 / math.sqrt(path[1]), CODEC, interp=True)
    _check(out.cpu().unsqueeze(1), ref, path[0], "paged_attention_into(interp=True)")


def test_cpu_decode_wrapper():
    _check_decode_wrapper(*_mods(None))


@pytest.mark.gpu
def test_hip_decode_wrapper(gpu):
    _check_decode_wrapper(*_mods(gpu))


def _check_errors(mod, dev):
    from tests.test_attention_paths import _caches as golay_caches
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    kc, vc, ks, vs = golay_caches("golay", 32, 2, BS, 4, LAYERS, 0.0, 1, False)
    table = torch.tensor([[0, 1]], dtype=torch.int32)
    lens = torch.tensor([20], dtype=torch.int32)
    q = torch.randn(1, 3, 2, 32).to(F16)
    for codec in ("golay", "golay_packed"):
        pk, pv = _for_codec(codec, 32, kc, vc)
        out = torch.empty(q.shape, dtype=q.dtype, device=dev)
        with pytest.raises(ValueError, match="interp needs hamming84"):
            mod.paged_attention_chunk_into(t(q), t(pk), t(pv), t(table), t(lens), t(ks), t(vs), out, LAYER, BS, 0.1,
                                           codec, interp=True)
        with pytest.raises(ValueError, match="interp needs hamming84"):
            mod.paged_attention_into(t(q[:, 0].contiguous()), t(pk), t(pv), t(table), t(lens), t(ks), t(vs),
                                     out[:, 0].contiguous(), LAYER, BS, 0.1, codec, interp=True)


def test_cpu_argument_errors():
    _check_errors(*_mods(None))


@pytest.mark.gpu
def test_hip_argument_errors(gpu):
    _check_errors(*_mods(gpu))


def test_c_entries_reject_other_codecs_and_negative_sizes():
    """Validation precedes any device work: both entries, no GPU needed."""
    from kvecc import _lib
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.float32)
    p = ctypes.c_void_p(buf.data_ptr())
    for name, tail in (("kvecc_paged_attention_interp", [p, 64, None]), ("kvecc_cpu_paged_attention_interp", [1])):
        fn = getattr(lib, name)

        def call(batch, q_max, heads, kvh, d, codec):
            return fn(p, 64, 32, 8, _lib.F16, p, p, p, p, None, p, p, p, batch, q_max, heads, kvh, d, 4, LAYERS, LAYER,
                      BS, 2, 0, 0.1, codec, *tail)
        for bad in ((-1, 2, 4, 4, 8), (1, -2, 4, 4, 8), (1, 2, -4, 4, 8), (1, 2, 4, -4, 8), (1, 2, 4, 4, -8)):
            assert call(*bad, _lib.CODEC_H84) == -1, (name, bad)  # KVECC_EINVAL
            assert "negative" in lib.kvecc_last_error().decode()
        for codec in (_lib.CODEC_GOLAY, 4, 1, 0):  # Golay (int32, packed), Hamming(7,4), raw
            assert call(1, 2, 4, 4, 8, codec) == -1, (name, codec)
            assert "hamming84" in lib.kvecc_last_error().decode()


def _small(dev=None):
    c, q, _ = _planted_case(MFMA_PATHS[2], 5)
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    return dict(q=t(q.contiguous()), kc=t(c["kc"]), vc=t(c["vc"]), table=t(c["table"]), lens=t(c["lens"]),
                ks=t(c["ks"]), vs=t(c["vs"]))


def _op_args(a, spans):
    return (a["q"], a["kc"], a["vc"], a["table"], a["lens"], spans, a["ks"], a["vs"], LAYER, BS,
            1 / math.sqrt(32), CODEC)


def _check_dispatcher(mod, dev):
    import kvecc
    from kvecc import torch_ops
    assert "paged_attention_interp" in torch_ops.OPS
    a = _small(dev)
    spans = torch.tensor([[1, 4, 0], [0, 5, 4], [2, 2, 9], [0, 0, 11]], dtype=torch.int32, device=dev)
    for sp in (None, spans):
        got = torch.ops.kvecc.paged_attention_interp(*_op_args(a, sp))
        out = torch.empty_like(got)
        mod.paged_attention_chunk_into(a["q"], a["kc"], a["vc"], a["table"], a["lens"], a["ks"], a["vs"], out, LAYER,
                                       BS, 1 / math.sqrt(32), CODEC, q_spans=sp, interp=True)
        assert torch.equal(got, out)
        pub = kvecc.paged_attention_chunk(a["q"], a["kc"], a["vc"], a["table"], a["lens"], a["ks"], a["vs"], LAYER,
                                          BS, q_spans=sp, interp=True)
        assert torch.equal(pub, got)
        torch.library.opcheck(torch.ops.kvecc.paged_attention_interp.default, _op_args(a, sp))


def test_cpu_dispatcher_op():
    _check_dispatcher(*_mods(None))


@pytest.mark.gpu
def test_hip_dispatcher_op(gpu):
    _check_dispatcher(*_mods(gpu))


def test_dispatcher_op_traces_under_compile():
    a = _small()
    fn = torch.compile(lambda *x: torch.ops.kvecc.paged_attention_interp(*x) * 2, fullgraph=True, backend="eager")
    assert torch.equal(fn(*_op_args(a, None)), torch.ops.kvecc.paged_attention_interp(*_op_args(a, None)) * 2)
