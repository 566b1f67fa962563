"""kvecc_paged_attention_window: sliding-window paged attention with sink tokens.

Contract (include/kvecc.h, "Windowed attention"): a valid query row at position p (the ragged
entry's rule) sees key j iff 0 <= j <= p, j < ctx_cap = min(max_context_len, max_blocks *
block_size), its block-table entry is >= 0, and j < S or j > p - W.  A row without a visible key
gets the entry's empty value.  W == 0 is the plain call; so is a window that covers every key
(W >= ctx_cap): both return the plain entry's bits.

The host twin is checked against a float64 restatement (the dense decode tests/test_attention_chunk.py's
`_ref_chunk` uses, plus the visibility rule), the HIP entry (marked gpu) against the twin and the
restatement, under tests/test_attention_paths.py's TOL.  Geometry: block_size 16, 9 blocks per
sequence, batch 3 with contexts of q_len + (70, 96, 121) tokens, 2 layers (layer 1 read); block 0
of the caches belongs to no sequence, so row 0 of the cache -- what a masked lane reads -- is never
a visible row.  The exact split-boundary cases run on tests/test_attention_chunk.py's SPLITS
(batch 1, splits of 32 tokens).
"""

import ctypes
import functools
import math

import pytest
import torch

from tests.test_attention_bytes import _as_h84
from tests.test_attention_bytes import _caches as _byte_caches
from tests.test_attention_chunk import SPLITS, _decode_rows, _pid, _split_case
from tests.test_attention_chunk_ragged import SPANS, _span_tensor, _valid
from tests.test_attention_chunk_ragged import _case as _ragged_case
from tests.test_attention_chunk_ragged import _run as _ragged_run
from tests.test_attention_paths import BF16, EMPTY, F16, F32, FAMILIES, TOL, _base, _caches, _close, _err, _for_codec

LAYERS, LAYER, BS, NBLK = 2, 1, 16, 9
CAP = NBLK * BS
EXTRA = (70, 96, 121)  # context before the chunk's own tokens
BYTES = ("hamming74", "int4")
# the four kernel families, the int32 Golay matrix-core kernel, one case per byte table, one bf16 split case
CASES = FAMILIES + [("golay", F16, 128, 4, 2), ("hamming74", F16, 128, 8, 2), ("int4", F32, 64, 8, 2),
                    ("golay_packed", BF16, 20, 2, 2)]
Q_LENS = (1, 5, 16, 17)


def _mods(gpu):
    from kvecc import cpu_ops, ops
    return (cpu_ops, None) if gpu is None else (ops, gpu)


def _ref_base(codec):
    return "hamming84" if codec in BYTES else _base(codec)


def _store(codec, d, kvh, num_blocks, layers, seed):
    """-> the caches as stored (Golay: int32, packed at the call), k_scales, v_scales."""
    if codec in BYTES:
        return _byte_caches(codec, d, kvh, BS, num_blocks, layers, seed, False)
    return _caches(_base(codec), d, kvh, BS, num_blocks, layers, 0.01, seed, False)


def _ref_caches(codec, kc, vc):
    """What the restatement decodes: a byte cache as the clean Hamming(8,4) cache of the same nibbles."""
    return (_as_h84(codec, kc), _as_h84(codec, vc)) if codec in BYTES else (kc, vc)


@functools.lru_cache(maxsize=None)
def _wcase(family, q_len):
    codec, dtype, d, heads, kvh = family
    num_blocks = 3 * NBLK + 2
    kc, vc, ks, vs = _store(codec, d, kvh, num_blocks, LAYERS, 400 + d)
    ids = 1 + torch.randperm(num_blocks - 1, generator=torch.Generator().manual_seed(d + q_len))[:3 * NBLK]
    q = torch.randn(3, q_len, heads, d, generator=torch.Generator().manual_seed(q_len)).to(dtype)
    return dict(q=q, kc=kc, vc=vc, ks=ks, vs=vs, table=ids.to(torch.int32).view(3, NBLK).contiguous(),
                lens=torch.tensor([q_len + e for e in EXTRA], dtype=torch.int32), layer=LAYER, bs=BS, codec=codec)


def _positions(c, spans=None):
    """-> per sequence (token indices, their positions), the contract's rule."""
    t_ = c["q"].shape[1]
    out = []
    for b in range(c["q"].shape[0]):
        f, n = (0, t_) if spans is None else spans[b]
        ts = torch.arange(f, max(min(f + n, t_), f)) if f >= 0 else torch.arange(0)
        out.append((ts, int(c["lens"][b]) - n + (ts - f)))
    return out


def _seen(pos, p, w, s):
    """bool [rows, keys]: the visibility rule for keys at `pos` (all < ctx_cap) and rows at `p`."""
    seen = pos[None, :] <= p[:, None]
    if w > 0:
        seen &= (pos[None, :] > p[:, None] - w) | (pos[None, :] < s)
    return seen


def _ref_window(c, w, s, mcl=0, spans=None):
    """float64 restatement, q [B, T, H, d] -> [B, T, H, d]; padding rows and rows without a visible key: empty."""
    codec, q, table, bs = c["codec"], c["q"], c["table"], c["bs"]
    base = _ref_base(codec)
    kc, vc = _ref_caches(codec, c["kc"], c["vc"])
    b_, t_, h_, d = q.shape
    kvh = kc.shape[2]
    cap = table.shape[1] * bs if mcl <= 0 else min(mcl, table.shape[1] * bs)
    w = 0 if w >= cap else w  # a window of ctx_cap keys or more is no window
    out = torch.full((b_, t_, h_, d), EMPTY[base], dtype=torch.float64)
    for b, (ts, p) in enumerate(_positions(c, spans)):
        n = min(max(int(c["lens"][b]), 0), cap)
        pos = torch.arange(n)
        blk = table[b, pos // bs].long()
        pos, blk = pos[blk >= 0], blk[blk >= 0]
        if len(ts) == 0 or len(pos) == 0:
            continue
        k = _decode_rows(kc, c["ks"], blk, pos % bs, c["layer"], bs, base, d)
        v = _decode_rows(vc, c["vs"], blk, pos % bs, c["layer"], bs, base, d)
        sc = torch.einsum("tkgd,nkd->tkgn", q[b, ts].double().view(len(ts), kvh, h_ // kvh, d), k) / math.sqrt(d)
        seen = _seen(pos, p, w, s)
        live = seen.any(1)
        sc = sc.masked_fill(~seen[:, None, None, :], -math.inf)[live]
        out[b, ts[live]] = torch.einsum("tkgn,nkd->tkgd", torch.softmax(sc, dim=-1), v).reshape(-1, h_, d)
    return out


def _run(mod, dev, c, w, s, mcl=0, spans=None, **over):
    """paged_attention_chunk_into(window=w, sinks=s) -> the raw output on the host."""
    c = dict(c, **over)
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    q = c["q"]
    pk, pv = _for_codec(c["codec"], q.shape[-1], c["kc"], c["vc"])
    out = torch.empty(q.shape, dtype=q.dtype, device=dev)
    mod.paged_attention_chunk_into(t(q), t(pk), t(pv), t(c["table"]), t(c["lens"]), t(c["ks"]), t(c["vs"]), out,
                                   c["layer"], c["bs"], 1 / math.sqrt(q.shape[-1]), c["codec"], max_context_len=mcl,
                                   q_spans=None if spans is None else t(_span_tensor(spans)), window=w, sinks=s)
    return out.cpu()


def _check(got, ref, dtype, what):
    got = got.double()
    assert bool(got.isfinite().all()), what
    print(f"{what}: max err {_err(got, ref):.3e}")
    assert _close(got, ref, dtype), (what, _err(got, ref))


def _check_empty_rows(got, ref, base, what):
    empty = (ref == EMPTY[base]).all(-1).all(-1)  # [B, T]: rows without a visible key, every head
    assert torch.equal(got.double()[empty], ref[empty]), what  # the empty value is exact
    return empty


# ---- 1. the twin against the restatement, the device against both -------------------------------
def _ws(q_len):
    """(W, S): W 1; W = block_size with S 0, 3 (no block multiple) and block_size; sequence 0's last row
    (p = q_len + 69) with its lower bound p - W + 1 on 64 -- a split boundary at splits of 32 and 64 --
    and one key before and after it; a sink range that overlaps every window (S > p - W: p <= 137);
    W larger than every context."""
    p0 = q_len + EXTRA[0] - 1
    return [(1, 0), (BS, 0), (BS, 3), (BS, BS), (24, 4), (p0 - 63, 3), (p0 - 62, 3), (p0 - 64, 3), (100, 40),
            (1000, 3)]


def test_the_cases_are_what_they_say():
    from kvecc import cpu_ops
    c = _wcase(CASES[0], 17)
    # the twin under the boundary window of _ws: sequence 0's last row starts at key 64 and the call meets the restatement
    assert _close(_run(cpu_ops, None, c, 17 + 70 - 1 - 63, 3).double(), _ref_window(c, 17 + 70 - 1 - 63, 3), CASES[0][1])
    assert int(c["lens"].max()) == 138 <= CAP and not bool((c["table"] == 0).any())
    p = _positions(c)[0][1]
    assert int(p[-1]) == 86 and int(p[-1]) - (17 + 70 - 1 - 63) + 1 == 64
    # overlap: with (100, 40) every row's window starts inside the sink range
    assert all(int(pp.max()) - 100 < 40 for _, pp in _positions(c))
    # the restatement at W 0 is test_attention_chunk's reference
    from tests.test_attention_chunk import _ref_chunk
    kc, vc = _ref_caches(c["codec"], c["kc"], c["vc"])
    assert torch.equal(_ref_window(c, 0, 0), _ref_chunk(c["q"], kc, vc, c["table"], c["lens"], c["ks"], c["vs"], LAYER,
                                                        BS, _ref_base(c["codec"])))


@functools.lru_cache(maxsize=None)
def _restated(family, q_len, w, s):
    return _ref_window(_wcase(family, q_len), w, s)


def _check_restatement(mod, dev, family, q_len):
    from kvecc import cpu_ops
    c, dtype, base = _wcase(family, q_len), family[1], _ref_base(family[0])
    for w, s in _ws(q_len):
        ref = _restated(family, q_len, w, s)
        got = _run(mod, dev, c, w, s)
        _check(got, ref, dtype, f"W {w} S {s}")
        _check_empty_rows(got, ref, base, (w, s))
        if dev is not None:  # the device against the twin
            twin = _run(cpu_ops, None, c, w, s).double()
            assert _close(got.double(), twin, dtype), (w, s, _err(got.double(), twin))


@pytest.mark.parametrize("q_len", Q_LENS)
@pytest.mark.parametrize("family", CASES, ids=_pid)
def test_cpu_window_against_restatement(family, q_len):
    _check_restatement(*_mods(None), family, q_len)


@pytest.mark.gpu
@pytest.mark.parametrize("q_len", Q_LENS)
@pytest.mark.parametrize("family", CASES, ids=_pid)
def test_hip_window_against_restatement_and_twin(gpu, family, q_len):
    _check_restatement(*_mods(gpu), family, q_len)


# ---- 2. a lower bound on, before and after a split boundary (splits of 32: test_split_geometry_of_the_split_cases)
SPLIT_CASES = [s for s in SPLITS if s[3] == 6]


def _check_split_boundary(mod, dev, case):
    path, q_len, n, nblk = case
    c = dict(_split_case(*case), codec=path[0])
    for t in (0, q_len - 1):  # the first and the last row's bound on the boundary; the others' fall around it
        p = n - q_len + t
        for lo in (31, 32, 33, 63, 64, 65):
            if lo > p:
                continue
            w = p - lo + 1
            for s in (0, 3):
                ref = _ref_window(c, w, s)
                got = _run(mod, dev, c, w, s)
                _check(got, ref, path[1], f"row {t} lo {lo} W {w} S {s}")


@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: f"{_pid(c[0])}-len{c[2]}")
def test_cpu_lower_bound_across_splits(case):
    _check_split_boundary(*_mods(None), case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: f"{_pid(c[0])}-len{c[2]}")
def test_hip_lower_bound_across_splits(gpu, case):
    _check_split_boundary(*_mods(gpu), case)


# ---- 2b. a long context: the grid planned by the window, the splits placed by each workgroup -----
LONG = [("hamming84", F16, 128, 8, 2), ("golay_packed", F16, 128, 8, 2), ("golay", F32, 64, 2, 2),
        ("int4", F32, 64, 8, 2)]


@functools.lru_cache(maxsize=None)
def _long_case(family, q_len):
    """Contexts of 4096 and 2999 + q_len tokens (the windows of the two sequences start in different
    splits, neither on a split boundary), 256 table columns, one layer."""
    codec, dtype, d, heads, kvh = family
    nblk = 256
    kc, vc, ks, vs = _store(codec, d, kvh, 2 * nblk + 1, 1, 600 + d)
    ids = 1 + torch.randperm(2 * nblk, generator=torch.Generator().manual_seed(9))
    q = torch.randn(2, q_len, heads, d, generator=torch.Generator().manual_seed(q_len)).to(dtype)
    return dict(q=q, kc=kc, vc=vc, ks=ks, vs=vs, table=ids.to(torch.int32).view(2, nblk).contiguous(),
                lens=torch.tensor([4096, 2999 + q_len], dtype=torch.int32), layer=0, bs=BS, codec=codec)


@pytest.mark.gpu
@pytest.mark.parametrize("q_len", (1, 17))
@pytest.mark.parametrize("family", LONG, ids=_pid)
def test_hip_long_context_against_the_twin(gpu, family, q_len):
    from kvecc import cpu_ops, ops
    c = _long_case(family, q_len)
    for w, s in ((1024, 4), (100, 0), (1500, 40), (4000, 3)):
        twin = _run(cpu_ops, None, c, w, s).double()
        got = _run(ops, gpu, c, w, s).double()
        print(f"W {w} S {s}: max |hip - twin| {_err(got, twin):.3e}")
        assert bool(got.isfinite().all()) and _close(got, twin, family[1]), (w, s, _err(got, twin))
    # a workspace too small for anything but the coarsest plan still gives the twin's values: mcl below the longest
    twin = _run(cpu_ops, None, c, 1024, 4, mcl=3500).double()
    assert _close(_run(ops, gpu, c, 1024, 4, mcl=3500).double(), twin, family[1])


@pytest.mark.gpu
@pytest.mark.parametrize("q_len", (1, 16))
def test_hip_plan_does_not_depend_on_the_workspace_passed(gpu, q_len):
    """[8, 2048, 32 | 8, 128], W 1024, S 4: the split the window asks for is finer than the dense plan's,
    so the workspace bound decides the plan.  It is the contract's size that decides, not the buffer's: the
    same call over a workspace of exactly kvecc_paged_attention_chunk_workspace floats, over one eight
    times as large, and through the Python layer before and after its cached workspace has grown, returns
    the same bits."""
    from kvecc import _lib, ops
    lib = _lib.load()
    g = torch.Generator(device=gpu).manual_seed(0)
    batch, ctx, heads, kvh, d = 8, 2048, 32, 8, 128
    nb = ctx // BS
    kc, vc = (torch.randint(0, 256, (batch * nb, 1, kvh, BS * d), device=gpu, generator=g, dtype=torch.uint8)
              for _ in range(2))
    ks, vs = (torch.rand(batch * nb, 1, kvh, BS, device=gpu, generator=g) * 0.3 + 0.05 for _ in range(2))
    table = torch.randperm(batch * nb, device=gpu, generator=g).to(torch.int32).view(batch, nb).contiguous()
    lens = torch.full((batch,), ctx, dtype=torch.int32, device=gpu)
    q = torch.randn(batch, q_len, heads, d, device=gpu, generator=g).half()
    need = lib.kvecc_paged_attention_chunk_workspace(batch, q_len, heads, d, ctx)
    outs = []
    for n in (need, 8 * need):
        ws = torch.empty(n, dtype=torch.float32, device=gpu)
        out = torch.empty_like(q)
        args = ops._chunk_entry_args("window", q, kc, vc, table, lens, ks, vs, out, 0, BS, 1 / math.sqrt(d), "hamming84",
                                     ctx, None, False, None, window=(1024, 4))
        assert lib.kvecc_paged_attention_window(*args, ctypes.c_void_p(ws.data_ptr()), n, ops._stream(gpu)) == 0
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert bool(outs[0].float().isfinite().all()) and torch.equal(outs[0], outs[1])

    def wrapped():
        out = torch.empty_like(q)
        ops.paged_attention_chunk_into(q, kc, vc, table, lens, ks, vs, out, 0, BS, 1 / math.sqrt(d), "hamming84",
                                       max_context_len=ctx, window=1024, sinks=4)
        return out.cpu()

    first = wrapped()
    ops._attn_workspace(gpu, 16 * need)  # what an earlier, larger call leaves behind
    assert torch.equal(wrapped(), first) and torch.equal(first, outs[0])


# ---- 3. bit equality with the unwindowed entries ------------------------------------------------
def _check_plain_bits(mod, dev, family, q_len):
    c = _wcase(family, q_len)
    for mcl, cap in ((0, CAP), (64, 64)):
        plain = _run(mod, dev, c, 0, 0, mcl)
        for w, s in ((0, 7), (cap, 0), (cap + 5, 3), (10 ** 12, 10 ** 12)):
            assert torch.equal(_run(mod, dev, c, w, s, mcl), plain), (mcl, w, s)
        # one key short of covering everything is the windowed call: its last row loses key 0 or keeps it as a sink
        assert _close(_run(mod, dev, c, cap - 1, 1, mcl).double(), _ref_window(c, cap - 1, 1, mcl), family[1])


@pytest.mark.parametrize("q_len", Q_LENS)
@pytest.mark.parametrize("family", CASES, ids=_pid)
def test_cpu_covering_window_returns_the_plain_bits(family, q_len):
    _check_plain_bits(*_mods(None), family, q_len)


@pytest.mark.gpu
@pytest.mark.parametrize("q_len", Q_LENS)
@pytest.mark.parametrize("family", CASES, ids=_pid)
def test_hip_covering_window_returns_the_plain_bits(gpu, family, q_len):
    _check_plain_bits(*_mods(gpu), family, q_len)


def _check_ragged_bits(mod, dev, family, q_max):
    """The left- and right-padded spans of tests/test_attention_chunk_ragged.py: a covering window and
    window 0 return the ragged entry's bits; a real window meets the restatement, padding rows empty."""
    c = dict(_ragged_case(*family, q_max), codec=family[0])
    cap = c["table"].shape[1] * BS
    plain = _ragged_run(mod, dev, family[0], c, c["spans"])
    q = c["q"].nan_to_num(0.0)  # the restatement multiplies: padding elements are NaN in the case
    for w, s in ((0, 5), (cap, 0), (cap + 1, 9)):
        got = _run(mod, dev, c, w, s, spans=c["spans"])
        assert torch.equal(got.view(torch.uint8), plain.view(torch.uint8)), (w, s)
    valid = _valid(c["spans"], q_max)
    for w, s in ((BS, 3), (40, 0)):
        got = _run(mod, dev, c, w, s, spans=c["spans"]).double()
        ref = _ref_window(dict(c, q=q), w, s, spans=c["spans"])
        assert bool((got[~valid] == EMPTY[_base(family[0])]).all())
        assert _close(got[valid], ref[valid], family[1]), (w, s, _err(got[valid], ref[valid]))


@pytest.mark.parametrize("q_max", sorted(SPANS))
@pytest.mark.parametrize("family", FAMILIES, ids=_pid)
def test_cpu_ragged_spans(family, q_max):
    _check_ragged_bits(*_mods(None), family, q_max)


@pytest.mark.gpu
@pytest.mark.parametrize("q_max", sorted(SPANS))
@pytest.mark.parametrize("family", FAMILIES, ids=_pid)
def test_hip_ragged_spans(gpu, family, q_max):
    _check_ragged_bits(*_mods(gpu), family, q_max)


# ---- 4. mask sensitivity, per row of a 16-token chunk -------------------------------------------
MASK_W, MASK_S, MASK_T, MASK_LEN = 24, 4, 16, 86  # rows at p = 70..85: windows start at 47..62
BIG = 3.0  # against scales of 0.05-0.35


def _strong_rows(codec, d, kvh):
    """One token row of nibble 15 (+7 scales) in every lane -> the codec's stored words [kvh, words]."""
    from kvecc import cpu_ops
    q = torch.full((1, kvh, d), 15, dtype=torch.uint8)
    if codec == "int4":
        return q[0]
    if codec == "hamming74":
        return cpu_ops.hamming74_encode(q)[0]
    return (cpu_ops.hamming84_encode(q) if _base(codec) == "hamming84" else cpu_ops.golay_encode_rows(q))[0]


@functools.lru_cache(maxsize=None)
def _mask_case(family):
    codec, dtype, d, heads, kvh = family
    nblk = 7
    kc, vc, ks, vs = _store(codec, d, kvh, nblk + 1, LAYERS, 17)
    q = torch.randn(1, MASK_T, heads, d, generator=torch.Generator().manual_seed(8)).abs().mul(0.5).to(dtype)
    return dict(q=q, kc=kc, vc=vc, ks=ks, vs=vs, table=(1 + torch.arange(nblk, dtype=torch.int32)).view(1, nblk),
                lens=torch.tensor([MASK_LEN], dtype=torch.int32), layer=LAYER, bs=BS, codec=codec)


def _with_strong_key(c, j):
    """Key j's K and V rows <- +7 scales at scale BIG (K against non-negative queries: the largest score)."""
    codec, d, kvh = c["codec"], c["q"].shape[-1], c["kc"].shape[2]
    blk, slot = int(c["table"][0, j // BS]), j % BS
    out = dict(c)
    row = _strong_rows(codec, d, kvh)
    for name in ("kc", "vc"):
        cache = c[name].clone()
        cache.view(cache.shape[0], LAYERS, kvh, BS, -1)[blk, LAYER, :, slot] = row
        out[name] = cache
    for name in ("ks", "vs"):
        sc = c[name].clone()
        sc[blk, LAYER, :, slot] = BIG
        out[name] = sc
    return out


def _moved(a, b, dtype, n=10):
    atol, rtol = TOL[dtype]
    return float(((a - b).abs() - n * (atol + rtol * b.abs())).max()) >= 0


def _check_mask(mod, dev, family):
    c, dtype = _mask_case(family), family[1]
    base = _run(mod, dev, c, MASK_W, MASK_S)
    p = _positions(c)[0][1]
    # every row's four boundaries: p - W, p - W + 1 (46..62), S and S - 1
    keys = sorted({int(x) - MASK_W for x in p} | {int(x) - MASK_W + 1 for x in p} | {MASK_S, MASK_S - 1})
    assert keys[:2] == [3, 4] and keys[2] == 46 and keys[-1] == 62
    hit = {t: [] for t in range(MASK_T)}
    for j in keys:
        got = _run(mod, dev, _with_strong_key(c, j), MASK_W, MASK_S)
        vis = _seen(torch.tensor([j]), p, MASK_W, MASK_S)[:, 0]
        for t in range(MASK_T):
            if bool(vis[t]):  # moves by far more than the tolerance
                assert _moved(got[0, t].double(), base[0, t].double(), dtype), (j, t)
            else:  # bit for bit
                assert torch.equal(got[0, t], base[0, t]), (j, t)
            hit[t].append((j, bool(vis[t])))
    for t in range(MASK_T):  # each row met its own four boundaries, two on each side
        pt = int(p[t])
        assert {(pt - MASK_W, False), (pt - MASK_W + 1, True), (MASK_S, False), (MASK_S - 1, True)} <= set(hit[t]), t


@pytest.mark.parametrize("family", CASES, ids=_pid)
def test_cpu_window_mask_sensitivity(family):
    _check_mask(*_mods(None), family)


@pytest.mark.gpu
@pytest.mark.parametrize("family", CASES, ids=_pid)
def test_hip_window_mask_sensitivity(gpu, family):
    _check_mask(*_mods(gpu), family)


# ---- 5. holes -----------------------------------------------------------------------------------
HOLE_W, HOLE_S = 24, 3


def _visible_rows(c, w, s, spans=None):
    """bool [B, max_blocks * bs]: the positions some query row of the sequence sees (the rule, no table)."""
    cap = c["table"].shape[1] * c["bs"]
    vis = torch.zeros(c["q"].shape[0], cap, dtype=torch.bool)
    for b, (_, p) in enumerate(_positions(c, spans)):
        if len(p):
            vis[b] = _seen(torch.arange(cap), p, w, s).any(0)
    return vis


def _check_holes(mod, dev, family, q_len):
    c, dtype, base = _wcase(family, q_len), family[1], _ref_base(family[0])
    vis = _visible_rows(c, HOLE_W, HOLE_S)
    vis_blocks = vis.view(3, NBLK, BS).any(-1)
    assert bool(vis_blocks[:, 0].all()) and not bool(vis_blocks[:, 1].any())  # sinks, then blocks nobody sees
    # every visible key in a -1 block: the empty value, exactly, whatever the blocks between hold
    table = torch.where(vis_blocks, torch.full_like(c["table"], -1), c["table"])
    got = _run(mod, dev, c, HOLE_W, HOLE_S, table=table)
    assert bool((got.double() == EMPTY[base]).all())
    # the sink block at -1 is skipped: the rows see their windows alone
    table = c["table"].clone()
    table[:, 0] = -1
    got = _run(mod, dev, c, HOLE_W, HOLE_S, table=table)
    ref = _ref_window(dict(c, table=table), HOLE_W, HOLE_S)
    _check(got, ref, dtype, "sink block missing")
    assert _close(ref, _ref_window(c, HOLE_W, 0), F32)  # (the restatement: the same keys as without sinks)
    # rows before position 0 (context_lens < q_len) get the empty value, the others the restatement's
    if q_len > 1:
        lens = torch.tensor([q_len - 2, q_len + 40, 0], dtype=torch.int32)
        got = _run(mod, dev, c, 5, 1, lens=lens)
        ref = _ref_window(dict(c, lens=lens), 5, 1)
        empty = _check_empty_rows(got, ref, base, "p < 0")
        assert bool(empty[0, :2].all()) and bool(empty[2].all()) and not bool(empty[1].any())
        _check(got, ref, dtype, "p < 0")


@pytest.mark.parametrize("q_len", (1, 17))
@pytest.mark.parametrize("family", CASES, ids=_pid)
def test_cpu_holes(family, q_len):
    _check_holes(*_mods(None), family, q_len)


@pytest.mark.gpu
@pytest.mark.parametrize("q_len", (1, 17))
@pytest.mark.parametrize("family", CASES, ids=_pid)
def test_hip_holes(gpu, family, q_len):
    _check_holes(*_mods(gpu), family, q_len)


def _poisoned(c, vis):
    """Every stored row outside `vis` (and every row of the blocks no sequence owns), in every layer:
    0xFF bytes and NaN scales."""
    kvh = c["kc"].shape[2]
    keep = torch.zeros(c["kc"].shape[0], BS, dtype=torch.bool)
    for b in range(vis.shape[0]):
        pos = vis[b].nonzero()[:, 0]
        keep[c["table"][b, pos // BS].long(), pos % BS] = True
    out = dict(c)
    for name in ("kc", "vc"):
        cache = c[name].clone()
        rows = cache.view(cache.shape[0], LAYERS, kvh, BS, -1)
        bad = torch.full_like(rows, -1 if cache.dtype == torch.int32 else 0xFF)
        out[name] = torch.where(keep[:, None, None, :, None], rows, bad).view(cache.shape).contiguous()
    for name in ("ks", "vs"):
        out[name] = torch.where(keep[:, None, None, :], c[name], torch.full_like(c[name], float("nan")))
    assert not bool(keep[0].any()) and bool(out["ks"][0].isnan().all())  # block 0: the masked lanes' stand-in row
    return out


def _check_poison(mod, dev, family, q_len):
    c = _wcase(family, q_len)
    clean = _run(mod, dev, c, HOLE_W, HOLE_S)
    got = _run(mod, dev, _poisoned(c, _visible_rows(c, HOLE_W, HOLE_S)), HOLE_W, HOLE_S)
    assert bool(got.double().isfinite().all())
    assert torch.equal(got, clean)


@pytest.mark.parametrize("q_len", Q_LENS)
@pytest.mark.parametrize("family", CASES, ids=_pid)
def test_cpu_poisoned_invisible_rows_reach_no_output(family, q_len):
    _check_poison(*_mods(None), family, q_len)


@pytest.mark.gpu
@pytest.mark.parametrize("q_len", Q_LENS)
@pytest.mark.parametrize("family", CASES, ids=_pid)
def test_hip_poisoned_invisible_rows_reach_no_output(gpu, family, q_len):
    _check_poison(*_mods(gpu), family, q_len)


# ---- 6. validation, the dispatcher operator -----------------------------------------------------
def _small(dev=None):
    c = _wcase(FAMILIES[2], 5)  # hamming84 fp16 d128
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    return {k: (t(v) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def _abi(mod, a, w, s, ws_floats=None, d=None):
    """The raw entry of `mod`'s backend -> its status."""
    from kvecc import _lib, ops
    lib = _lib.load()
    q = a["q"]
    out = torch.empty_like(q)
    args = ops._chunk_entry_args("window", q, a["kc"], a["vc"], a["table"], a["lens"], a["ks"], a["vs"], out, LAYER, BS,
                                 0.1, "hamming84", 0, None, False, None, window=(0, 0))
    args[-2:] = [w, s]
    if d is not None:
        args[17] = d  # head_dim (query, 3 strides, dtype, 8 pointers, batch, q_len, heads, kv_heads, head_dim)
    if mod.__name__.endswith("cpu_ops"):
        return lib.kvecc_cpu_paged_attention_window(*args, 1)
    n = lib.kvecc_paged_attention_chunk_workspace(q.shape[0], q.shape[1], q.shape[2], q.shape[3], CAP)
    ws = torch.empty(n, dtype=torch.float32, device=q.device)
    return lib.kvecc_paged_attention_window(*args, ctypes.c_void_p(ws.data_ptr()), n if ws_floats is None else ws_floats,
                                            None)


def _check_validation(mod, dev):
    from kvecc import _lib
    a = _small(dev)
    einval = -1
    assert _abi(mod, a, 16, 3) == 0
    for w, s in ((-1, 0), (16, -1), (-5, -5), (0, -1)):
        assert _abi(mod, a, w, s) == einval, (w, s)
        assert b"negative" in _lib.load().kvecc_last_error()
        with pytest.raises(ValueError):
            _run(mod, dev, a, w, s)
    assert _abi(mod, a, 16, 3, d=260) == einval and b"head_dim" in _lib.load().kvecc_last_error()
    if dev is not None:
        assert _abi(mod, a, 16, 3, ws_floats=8) == einval and b"workspace" in _lib.load().kvecc_last_error()
    for bad in (dict(window=1.5), dict(window=True), dict(sinks="3"), dict(window=8, interp=True),
                dict(window=8, stats=torch.zeros(4096, dtype=torch.int64, device=dev)), dict(window=8, repair=True)):
        with pytest.raises(ValueError):
            mod.paged_attention_chunk_into(a["q"], a["kc"], a["vc"], a["table"], a["lens"], a["ks"], a["vs"],
                                           torch.empty_like(a["q"]), LAYER, BS, 0.1, "hamming84", **bad)
    wide = torch.zeros(1, 1, 1, 260, dtype=torch.float32, device=dev)
    kc = torch.zeros(2, 1, 1, BS * 260, dtype=torch.uint8, device=dev)
    sc = torch.ones(2, 1, 1, BS, device=dev)
    one = torch.ones(1, 1, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="head_dim"):
        mod.paged_attention_chunk_into(wide, kc, kc, one, one.view(1), sc, sc, torch.empty_like(wide), 0, BS, 0.1,
                                       "hamming84", window=4)


def test_cpu_validation():
    _check_validation(*_mods(None))


@pytest.mark.gpu
def test_hip_validation(gpu):
    _check_validation(*_mods(gpu))


def test_the_library_and_the_registry_carry_the_entry():
    from kvecc import _lib, backends, cpu_ops, ops, torch_ops
    assert "kvecc_paged_attention_window" in _lib.SIGNATURES and "kvecc_cpu_paged_attention_window" in _lib.SIGNATURES
    assert "paged_attention_window_into" in backends.NATIVE_FUNCTIONS and "paged_attention_window" in torch_ops.OPS
    assert hasattr(ops, "paged_attention_window_into") and hasattr(cpu_ops, "paged_attention_window_into")


def test_dispatcher_op_on_the_host_is_cpu_ops():
    import kvecc
    from kvecc import cpu_ops
    a = _small()
    d = a["q"].shape[-1]
    for spans in (None, _span_tensor([(0, 5), (2, 3), (4, 1)])):
        got = torch.ops.kvecc.paged_attention_window(a["q"], a["kc"], a["vc"], a["table"], a["lens"], spans, a["ks"],
                                                     a["vs"], LAYER, BS, 1 / math.sqrt(d), "hamming84", 24, 4)
        want = torch.empty_like(a["q"])
        cpu_ops.paged_attention_window_into(a["q"], a["kc"], a["vc"], a["table"], a["lens"], a["ks"], a["vs"], want,
                                            LAYER, BS, 1 / math.sqrt(d), "hamming84", 24, 4, q_spans=spans)
        assert torch.equal(got, want)
    assert torch.equal(kvecc.paged_attention_chunk(a["q"], a["kc"], a["vc"], a["table"], a["lens"], a["ks"], a["vs"],
                                                   LAYER, BS, window=24, sinks=4),
                       _run(cpu_ops, None, a, 24, 4))


@pytest.mark.gpu
def test_hip_dispatcher_op_compiles(gpu):
    import kvecc  # noqa: F401
    from kvecc import ops
    a = _small(gpu)
    d = a["q"].shape[-1]

    def f(q):
        return torch.ops.kvecc.paged_attention_window(q * 1.0, a["kc"], a["vc"], a["table"], a["lens"], None, a["ks"],
                                                      a["vs"], LAYER, BS, 1 / math.sqrt(d), "hamming84", 24, 4) + 0.0

    eager = f(a["q"])
    assert torch.equal(torch.compile(f, fullgraph=True)(a["q"]), eager)
    assert torch.equal(eager.cpu(), _run(ops, gpu, a, 24, 4))
