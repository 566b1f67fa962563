"""kvecc_paged_attention_golay_stats: paged attention over a Golay(24,12) cache (int32 or packed) that
adds the decoder's counts of every codeword it attends over -- bits corrected, uncorrectable words --
to a statistics buffer, exactly once (include/kvecc.h "Counted attention").

Paths: every Golay instantiation of the launcher's table in tests/test_attention_paths.py (matrix-core
groups 2 / 4 / 8 / 16, the split kernels at a group of 1 and 3, head_dim 4 .. 256, fp32 / fp16 / bf16),
on that file's edge bundle: batch 4, 2 layers with the last read, block 16, context_lens [96, 1, 0, 41],
a -1 block inside sequence 3, sequence 0's last token in the buffer's last row, a table two columns
wider.  Counts: per sequence with a valid query token, what cpu_ops.shim_read_tensors(ctx = n_b,
stats) adds, summed and compared EXACTLY.  Outputs: that file's float64 restatement (_ref64's
operation, every query token at its own key limit), within TOL of the query dtype; rows without a key are
exactly 0.  Every case runs on the host twin and, marked gpu, on the device.
"""

import ctypes
import functools
import itertools
import math

import pytest
import torch

from tests.test_attention_paths import (EMPTY, LAYER, LAYERS, PATHS, _bundle, _caches, _close, _err,
                                        _for_codec, _id)

GOLAY_PATHS = [p for p in PATHS if p[0] in ("golay", "golay_packed")]
BS = 16
Q_LENS = [1, 2, 5, 16, 17]
CLAMP = 90  # a max_context_len below sequence 0's 96 tokens and above the others'
assert {p[2] for p in GOLAY_PATHS} >= {100, 128, 256} and {p[3] // p[4] for p in GOLAY_PATHS} == {1, 2, 4, 8, 16}


def _mods(gpu):
    from kvecc import cpu_ops, ops
    return (cpu_ops, None) if gpu is None else (ops, gpu)


# ---- caches ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weight4():
    """A 4-bit error pattern that the host decoder reports as count 4 (searched, not assumed)."""
    from kvecc import cpu_ops
    for bits in itertools.combinations(range(24), 4):
        e = sum(1 << i for i in bits)
        cnt = cpu_ops.golay_decode(torch.tensor([e], dtype=torch.int32), return_error_counts=True)[1]
        if int(cnt[0]) == 4:
            return e
    raise AssertionError("no weight-4 pattern of count 4")


def _patterns():
    # data-bit flips of weight 1, 2, 3; parity-only flips of weight 1, 2, 3; an uncorrectable word
    return [0x001, 0x810, 0x124, 0x001000, 0x804000, 0x250000, _weight4()]


@functools.lru_cache(maxsize=None)
def _cache(d, kvh, kind):
    """The edge bundle's table and lengths over a clean cache with planted words ("planted": BER 0)
    or an all-random one ("random": injection at BER 5e-2).  int32 layout; -> dict and the planted words'
    (clean, stored) values."""
    b = _bundle("golay", torch.float32, d, 2 * kvh, kvh, BS)  # table / lens only (its caches hold BER 1e-2)
    table, lens = b["table"], b["lens"]
    nblk = int(b["kc"].shape[0])
    g = (d + 2) // 3
    kc, vc, ks, vs = _caches("golay", d, kvh, BS, nblk, LAYERS, 0.0 if kind == "planted" else 5e-2, 300 + d, True)
    kc, vc = kc.clone(), vc.clone()
    planted = []
    if kind == "planted":
        pats = _patterns()
        for x in (kc, vc):
            v = x.view(nblk, LAYERS, kvh, BS, g)
            where = []
            blk0 = int(table[0, 0])
            for i, p in enumerate(pats):  # codeword g - 1 of a row, codeword 0 of the following row
                where.append((blk0, 2 + i, g - 1, p))
                where.append((blk0, 3 + i, 0, pats[(i + 3) % len(pats)]))
            for i, p in enumerate(pats[:g]):
                where.append((nblk - 1, BS - 1, g - 1 - i, p))  # the buffer's last row (sequence 0's last token)
                where.append((0, 0, i, pats[(i + 1) % len(pats)] if g > 1 else p))  # row 0 of block 0 (sequence 1)
            where.append((int(table[3, 0]), 1, 0, pats[1]))  # sequence 3 holds errors too
            for blk, slot, cw, p in where:
                clean = v[blk, LAYER, :, slot, cw].clone()
                v[blk, LAYER, :, slot, cw] ^= p
                planted.append((clean, v[blk, LAYER, :, slot, cw].clone()))
    return dict(kc=kc, vc=vc, ks=ks, vs=vs, table=table, lens=lens, d=d), planted


def test_planted_words_are_what_they_say():
    """The planted cache holds words of count 1, 2, 3 and 4 and a parity-only word (count > 0, data
    unchanged); the random one holds uncorrectable words.  Otherwise the cases below prove nothing."""
    from kvecc import cpu_ops
    for d, kvh in sorted({(p[2], p[4]) for p in GOLAY_PATHS}):
        _, planted = _cache(d, kvh, "planted")
        clean = torch.cat([c for c, _ in planted])
        stored = torch.cat([s for _, s in planted])
        t0, c0, _ = cpu_ops.golay_decode(clean, return_error_counts=True)
        t1, c1, _ = cpu_ops.golay_decode(stored, return_error_counts=True)
        assert not bool(c0.any())
        assert {1, 2, 3, 4} <= set(c1.tolist()), (d, set(c1.tolist()))
        flipped = clean ^ stored
        data = (flipped & 0xFFF) != 0  # the data bits are the codeword's low 12
        for n in (1, 2, 3):
            assert bool((data & (c1 == n)).any()) and bool((~data & (c1 == n)).any()), (d, n)  # data / parity only
        assert bool((t0 == t1)[c1 < 4].all())  # corrected back: the outputs are the clean cache's there
        c, _ = _cache(d, kvh, "random")
        assert _expected_counts(c, "golay", d)[1] > 0, d


def _layout(codec, d, c):
    """The bundle in the codec's layout (packed: 3-byte codewords, rows padded to whole dwords)."""
    pk, pv = _for_codec(codec, d, c["kc"], c["vc"])
    out = dict(c)
    out["kc"], out["vc"] = pk, pv
    return out


# ---- expectations -----------------------------------------------------------------------------------
def _cap(c, mcl):
    full = c["table"].shape[1] * BS
    return full if mcl <= 0 else min(mcl, full)


def _seq_counts(c, codec, d, b, mcl=0):
    """[bits corrected, uncorrectable] that the counting host read adds for sequence b alone, K and V."""
    from kvecc import cpu_ops
    nb = min(max(int(c["lens"][b]), 0), _cap(c, mcl))
    if nb == 0:
        return [0, 0]
    st = cpu_ops.new_stats()
    kvh = c["kc"].shape[2]
    lay = _layout(codec, d, c)
    cpu_ops.shim_read_tensors(lay["kc"], lay["vc"], c["ks"], c["vs"], c["table"][b].contiguous(), nb, kvh, d, LAYERS,
                              BS, LAYER, codec, False, torch.float32, st)
    return cpu_ops.read_stats(st)


def _expected_counts(c, codec, d, spans=None, mcl=0):
    tot = [0, 0]
    for b in range(c["table"].shape[0]):
        if spans is not None and (spans[b][1] <= 0 or spans[b][0] < 0 or spans[b][0] >= spans[b][2]):
            continue  # no valid token: the sequence is not read
        n = _seq_counts(c, codec, d, b, mcl)
        tot = [tot[0] + n[0], tot[1] + n[1]]
    return tot


def _spans3(spans, q_max):
    return None if spans is None else [(f, n, q_max) for f, n in spans]


def _valid(spans, batch, q_max):
    v = torch.zeros(batch, q_max, dtype=torch.bool)
    for b in range(batch):
        f, n = (0, q_max) if spans is None else spans[b]
        if f >= 0 and n > 0:
            v[b, f:min(f + n, q_max)] = True
    return v


def _dense(c, b):
    """Sequence b's K and V as _ref64 reads them (cpu_ops.golay_decode_rows, dequantized, float64):
    the positions whose block is not -1, K [n, Hkv, d], V [n, Hkv, d]."""
    from kvecc import cpu_ops
    key = ("dense", b)
    if key not in c:
        kc, table = c["kc"], c["table"]
        nb_, nl_, kvh, _ = kc.shape
        n = min(max(int(c["lens"][b]), 0), table.shape[1] * BS)
        pos = torch.arange(n)
        blk = table[b, pos // BS].long()
        ok = blk >= 0
        pos, blk, slot = pos[ok], blk[ok], (pos % BS)[ok]
        f = []
        for cache, sc in ((kc, c["ks"]), (c["vc"], c["vs"])):
            rows = cache.view(nb_, nl_, kvh, BS, -1)[blk, LAYER, :, slot].contiguous()
            dec = cpu_ops.golay_decode_rows(rows, c["d"]) if len(pos) else torch.zeros(0, kvh, c["d"], dtype=torch.uint8)
            f.append((dec.double() - 8.0) * sc[blk, LAYER, :, slot].double().unsqueeze(-1))
        c[key] = (pos, f[0], f[1])
    return c[key]


def _ref_chunk(q, c, spans=None, mcl=0):
    """float64 [B, T, H, d], _ref64's operation per query token: token t of span (first, count) sits
    at position lens[b] - count + (t - first) and sees the keys at or before it, below
    max_context_len, whose block is not -1.  Padding rows, and rows without a key, hold 0."""
    b_, t_, h_, d = q.shape
    cap = _cap(c, mcl)
    valid = _valid(spans, b_, t_)
    out = torch.zeros(b_, t_, h_, d, dtype=torch.float64)
    qz = torch.nan_to_num(q.float()).double()
    for b in range(b_):
        pos, k, v = _dense(c, b)
        kvh = k.shape[1]
        f, n = (0, t_) if spans is None else spans[b]
        lim = torch.tensor([min(max(int(c["lens"][b]) - n + 1 + (t - f), 0), cap) if bool(valid[b, t]) else 0
                            for t in range(t_)])
        seen = pos.view(1, -1) < lim.view(-1, 1)  # [T, n]
        if not bool(seen.any()):
            continue
        s = torch.einsum("tkgd,nkd->tkgn", qz[b].view(t_, kvh, h_ // kvh, d), k) / math.sqrt(d)
        s = s.masked_fill(~seen.view(t_, 1, 1, -1), float("-inf"))
        p = torch.softmax(s, dim=-1).nan_to_num(0.0)  # a row without a key: 0
        out[b] = torch.einsum("tkgn,nkd->tkgd", p, v).reshape(t_, h_, d)
    return out


def _query(batch, q_len, heads, d, dtype, seed, nan_where=None):
    q = torch.randn(batch, q_len, heads, d, generator=torch.Generator().manual_seed(seed)).to(dtype)
    if nan_where is not None:
        q[nan_where] = float("nan")
    return q


def _run(mod, dev, codec, q, c, spans=None, mcl=0, stats=None):
    """paged_attention_counted_into on the bundle in the codec's layout -> (output on the host, counts)."""
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    d = q.shape[-1]
    lay = _layout(codec, d, c)
    sp = None
    if spans is not None:
        rows, base = [], 0
        for f, n in spans:
            rows.append((f, n, base))
            base += max(n, 0)
        sp = t(torch.tensor(rows, dtype=torch.int32))
    if stats is None:
        stats = mod.new_stats(dev)
    out = torch.full(q.shape, 77.0, dtype=q.dtype, device=dev)
    mod.paged_attention_counted_into(t(q), t(lay["kc"]), t(lay["vc"]), t(c["table"]), t(c["lens"]), t(c["ks"]),
                                     t(c["vs"]), out, LAYER, BS, 1 / math.sqrt(d), codec, stats, max_context_len=mcl,
                                     q_spans=sp)
    return out.cpu(), mod.read_stats(stats)


def _check(got, ref, dtype, what=""):
    got = got.double()
    assert not bool(got.isnan().any()), what
    empty = (ref == 0.0).all(-1)
    assert torch.equal(got[empty], ref[empty]), what  # the empty value is exact
    print(f"{what} max err {_err(got, ref):.3e}")
    assert _close(got, ref, dtype), (what, _err(got, ref))


# ---- 1. exact counts, outputs within tolerance -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(path, q_len, kind, mcl):
    codec, dtype, d, heads, kvh, _, _ = path
    c, _ = _cache(d, kvh, kind)
    q = _query(4, q_len, heads, d, dtype, q_len)
    return c, q, _expected_counts(c, codec, d, mcl=mcl), _ref_chunk(q, c, mcl=mcl)


def _check_counts_and_outputs(mod, dev, path, q_len):
    codec, dtype = path[0], path[1]
    for kind in ("planted", "random"):
        for mcl in (0, CLAMP):
            c, q, want, ref = _case(path, q_len, kind, mcl)
            assert want[0] > 0 and want[1] > 0, want
            got, counts = _run(mod, dev, codec, q, c, mcl=mcl)
            print(f"{kind} mcl {mcl}: counts {counts} expected {want}")
            assert counts == want, (kind, mcl, counts, want)
            assert torch.equal(got[2].double(), torch.zeros_like(ref[2]))  # sequence 2 is empty
            _check(got, ref, dtype, f"{kind} mcl {mcl}")
    assert _case(path, q_len, "planted", CLAMP)[2] != _case(path, q_len, "planted", 0)[2]  # the clamp cuts counts


@pytest.mark.parametrize("q_len", Q_LENS)
@pytest.mark.parametrize("path", GOLAY_PATHS, ids=_id)
def test_cpu_counts_and_outputs(path, q_len):
    _check_counts_and_outputs(*_mods(None), path, q_len)


@pytest.mark.gpu
@pytest.mark.parametrize("q_len", Q_LENS)
@pytest.mark.parametrize("path", GOLAY_PATHS, ids=_id)
def test_hip_counts_and_outputs(gpu, path, q_len):
    _check_counts_and_outputs(*_mods(gpu), path, q_len)


# ---- 2. what must not be counted --------------------------------------------------------------------
def _dirty_layout(codec, d, c):
    """The bundle in the codec's layout with error bits wherever no count may come from: bits 24..31
    of every int32 word / the pad bytes of every packed row; the slots at or past each sequence's
    length in its last block; the other layer; the blocks no table row names (the buffer's row 0,
    which a -1 entry's lanes read in its place, lies in the other layer of block 0)."""
    kvh = c["kc"].shape[2]
    g = (d + 2) // 3
    bad = _weight4()
    named = set(int(x) for x in c["table"].flatten() if int(x) >= 0)
    out = dict(c)
    for key in ("kc", "vc"):
        x = c[key].clone()
        v = x.view(-1, LAYERS, kvh, BS, g)
        v[:, 1 - LAYER] ^= bad
        for blk in range(v.shape[0]):
            if blk not in named:
                v[blk, LAYER] ^= bad
        for b in range(c["table"].shape[0]):
            n = int(c["lens"][b])
            if n // BS < c["table"].shape[1] and int(c["table"][b, n // BS]) >= 0:
                v[int(c["table"][b, n // BS]), LAYER, :, n % BS:] ^= bad
        out[key] = x
    out = _layout(codec, d, out)
    for key in ("kc", "vc"):
        if codec == "golay":
            out[key] = out[key] | torch.tensor(0xFF000000 - (1 << 32), dtype=torch.int32)
        else:
            row = (3 * g + 3) // 4 * 4
            out[key] = out[key].clone()
            out[key].view(-1, row)[:, 3 * g:] = 0xFF
    return out


def _check_not_counted(mod, dev, path, q_len):
    codec, dtype, d, heads, kvh, _, _ = path
    assert LAYER == 1  # the buffer's row 0 is the other layer's
    for mcl in (0, CLAMP):
        c, q, want, ref = _case(path, q_len, "planted", mcl)
        assert int(c["table"][3, 1]) == -1  # a -1 block inside sequence 3
        dirty = _dirty_layout(codec, d, c)
        assert int((dirty["kc"] != _layout(codec, d, c)["kc"]).sum()) > 1000
        t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
        stats = mod.new_stats(dev)
        out = torch.full(q.shape, 77.0, dtype=q.dtype, device=dev)
        mod.paged_attention_counted_into(t(q), t(dirty["kc"]), t(dirty["vc"]), t(c["table"]), t(c["lens"]),
                                         t(c["ks"]), t(c["vs"]), out, LAYER, BS, 1 / math.sqrt(d), codec, stats,
                                         max_context_len=mcl)
        counts = mod.read_stats(stats)
        assert counts == want, (mcl, counts, want)
        clean_out, _ = _run(mod, dev, codec, q, c, mcl=mcl)
        assert torch.equal(out.cpu(), clean_out)  # outputs as on the undirtied cache
        _check(out.cpu(), ref, dtype, f"dirty mcl {mcl}")


@pytest.mark.parametrize("q_len", [1, 17])
@pytest.mark.parametrize("path", GOLAY_PATHS, ids=_id)
def test_cpu_uncounted_regions(path, q_len):
    _check_not_counted(*_mods(None), path, q_len)


@pytest.mark.gpu
@pytest.mark.parametrize("q_len", [1, 17])
@pytest.mark.parametrize("path", GOLAY_PATHS, ids=_id)
def test_hip_uncounted_regions(gpu, path, q_len):
    _check_not_counted(*_mods(gpu), path, q_len)


# ---- 3. ragged spans ----------------------------------------------------------------------------------
# (q_max, spans of sequences of lengths [96, 1, 0, 41]); a span's count never exceeds its sequence's length
RAGGED = [
    (17, ((0, 17), (16, 1), (0, 0), (3, 9))),   # full, first > 0 in a second tile, zero count, short
    (5, ((1, 4), (4, 1), (0, 0), (-1, 3))),     # first < 0: sequence 3, whose cache holds errors, is all padding
    (5, ((3, 4), (0, 1), (0, 0), (2, 9))),      # spans that overrun q_max (sequences 0 and 3)
    (1, ((0, 1), (0, 0), (0, 0), (0, 1))),      # q_max 1: the decode step over spans
]


def _check_ragged(mod, dev, path, case):
    codec, dtype, d, heads, kvh, _, _ = path
    q_max, spans = case
    c, _ = _cache(d, kvh, "planted")
    valid = _valid(spans, 4, q_max)
    q = _query(4, q_max, heads, d, dtype, q_max, nan_where=~valid)  # padding query elements are NaN
    want = _expected_counts(c, codec, d, _spans3(spans, q_max))
    idle = [b for b, (f, n) in enumerate(spans) if (n <= 0 or f < 0) and int(c["lens"][b]) > 0]
    assert idle or case is not RAGGED[1]
    assert all(sum(_seq_counts(c, codec, d, b)) > 0 for b in idle)  # an idle sequence whose cache holds errors
    for b, (f, n) in enumerate(spans):  # an overrunning span: positions past its last token's limit are counted
        if f >= 0 and f + n > q_max:
            assert int(c["lens"][b]) - n + (q_max - 1 - f) + 1 < int(c["lens"][b])
    got, counts = _run(mod, dev, codec, q, c, spans)
    assert counts == want, (counts, want)
    assert bool((got[~valid].double() == EMPTY[codec]).all())
    _check(got, _ref_chunk(q, c, spans), dtype, f"ragged q_max {q_max}")


@pytest.mark.parametrize("case", RAGGED, ids=lambda c: f"qmax{c[0]}-first{c[1][0][0]}")
@pytest.mark.parametrize("path", GOLAY_PATHS, ids=_id)
def test_cpu_ragged(path, case):
    _check_ragged(*_mods(None), path, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", RAGGED, ids=lambda c: f"qmax{c[0]}-first{c[1][0][0]}")
@pytest.mark.parametrize("path", GOLAY_PATHS, ids=_id)
def test_hip_ragged(gpu, path, case):
    _check_ragged(*_mods(gpu), path, case)


# ---- 4. accumulation ----------------------------------------------------------------------------------
ACC_PATHS = [p for p in GOLAY_PATHS if p[2] == 128 and p[3] in (2, 8) and p[1] == torch.float16]


def _check_accumulation(mod, dev, path):
    codec = path[0]
    c, q, want, _ = _case(path, 5, "planted", 0)
    st = mod.new_stats(dev)
    _, once = _run(mod, dev, codec, q, c, stats=st)
    _, twice = _run(mod, dev, codec, q, c, stats=st)
    assert once == want and twice == [2 * want[0], 2 * want[1]]
    pre = mod.new_stats(dev)
    pre[0] += 1000  # a pre-loaded buffer is added to
    pre[1] += 7
    assert _run(mod, dev, codec, q, c, stats=pre)[1] == [1000 + want[0], 7 + want[1]]


@pytest.mark.parametrize("path", ACC_PATHS, ids=_id)
def test_cpu_accumulation(path):
    _check_accumulation(*_mods(None), path)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ACC_PATHS, ids=_id)
def test_hip_accumulation(gpu, path):
    _check_accumulation(*_mods(gpu), path)


# ---- 5. the device against the host twin --------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("path", GOLAY_PATHS, ids=_id)
def test_hip_equals_host_twin(gpu, path):
    from kvecc import cpu_ops, ops
    c, q, _, _ = _case(path, 17, "random", 0)
    host, host_counts = _run(cpu_ops, None, path[0], q, c)
    dev, dev_counts = _run(ops, gpu, path[0], q, c)
    assert dev_counts == host_counts
    print(f"max |device - host| {_err(dev.double(), host.double()):.3e}")
    assert _close(dev.double(), host.double(), path[1])


# ---- 6. validation ------------------------------------------------------------------------------------
def test_c_entries_need_stats_and_golay():
    """Validation precedes any device work: both entries, no GPU needed."""
    from kvecc import _lib
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.float32)
    stats = torch.zeros(512, dtype=torch.int64)
    p, sp = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(stats.data_ptr())
    for name, tail in (("kvecc_paged_attention_golay_stats", [p, 64, None]),
                       ("kvecc_cpu_paged_attention_golay_stats", [1])):
        fn = getattr(lib, name)

        def call(codec, st):
            return fn(p, 64, 32, 8, _lib.F16, p, p, p, p, None, p, p, p, 1, 2, 4, 4, 8, 4, LAYERS, LAYER, BS, 2, 0,
                      0.1, codec, st, *tail)
        for codec in (_lib.CODEC_GOLAY, 4):
            assert call(codec, None) == -1, name  # KVECC_EINVAL
            assert "stats" in lib.kvecc_last_error().decode()
        for codec in (_lib.CODEC_H84, 1, 0):  # Hamming(8,4), Hamming(7,4), raw
            assert call(codec, sp) == -1, (name, codec)
            assert "golay" in lib.kvecc_last_error().decode()
    assert not bool(buf.any()) and not bool(stats.any())


def _check_errors(mod, dev):
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    c, _ = _cache(32, 2, "planted")
    q = _query(4, 5, 2, 32, torch.float16, 5)
    args = [t(c[k]) for k in ("kc", "vc", "table", "lens", "ks", "vs")]
    out = torch.full(q.shape, 77.0, dtype=q.dtype, device=dev)
    good = mod.new_stats(dev)
    n = good.numel()
    bad = [torch.zeros(n, dtype=torch.int32, device=dev),  # dtype
           torch.zeros(n - 1 if n > 2 else 1, dtype=torch.int64, device=dev),  # length
           torch.zeros(n, dtype=torch.int64, device="meta" if dev is None else "cpu")]  # device
    for st in bad:
        with pytest.raises(ValueError, match="stats must be"):
            mod.paged_attention_counted_into(t(q), *args, out, LAYER, BS, 0.1, "golay", st)
    assert not any(bool(st.any()) for st in bad if st.device.type != "meta")
    for codec in ("golay", "golay_packed"):
        pk, pv = _for_codec(codec, 32, c["kc"], c["vc"])
        with pytest.raises(ValueError, match="interp"):
            mod.paged_attention_counted_into(t(q), t(pk), t(pv), *args[2:], out, LAYER, BS, 0.1, codec, good,
                                             interp=True)
    h84 = torch.zeros(c["kc"].shape[0], LAYERS, 2, BS * 32, dtype=torch.uint8)
    for codec in ("hamming74", "int4"):
        with pytest.raises(ValueError, match="counted attention kernels"):
            mod.paged_attention_counted_into(t(q), t(h84), t(h84), *args[2:], out, LAYER, BS, 0.1, codec, good)
    with pytest.raises(ValueError, match="hamming84"):  # the pinned entry keeps refusing Golay
        mod.paged_attention_chunk_into(t(q), *args, out, LAYER, BS, 0.1, "golay", stats=good)
    assert bool((out == 77.0).all()) and mod.read_stats(good) == [0, 0]


def test_cpu_argument_errors():
    _check_errors(*_mods(None))


@pytest.mark.gpu
def test_hip_argument_errors(gpu):
    _check_errors(*_mods(gpu))


def _check_hamming84_forwards(mod, dev):
    """'hamming84' through the counted name is paged_attention_chunk_into(..., stats=), bit for bit."""
    from tests.test_attention_stats import _case as h84_case
    from tests.test_attention_interp import MFMA_PATHS
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    c, q, want = h84_case(MFMA_PATHS[2], 5, False)
    args = [t(c[k]) for k in ("kc", "vc", "table", "lens", "ks", "vs")]
    for interp in (False, True):
        outs, counts = [], []
        for counted in (False, True):
            st = mod.new_stats(dev)
            out = torch.full(q.shape, 77.0, dtype=q.dtype, device=dev)
            if counted:
                mod.paged_attention_counted_into(t(q.contiguous()), *args, out, LAYER, BS, 0.1, "hamming84", st,
                                                 interp=interp)
            else:
                mod.paged_attention_chunk_into(t(q.contiguous()), *args, out, LAYER, BS, 0.1, "hamming84",
                                               interp=interp, stats=st)
            outs.append(out.cpu())
            counts.append(mod.read_stats(st))
        assert torch.equal(outs[0], outs[1]) and counts[0] == counts[1] == want


def test_cpu_hamming84_forwards():
    _check_hamming84_forwards(*_mods(None))


@pytest.mark.gpu
def test_hip_hamming84_forwards(gpu):
    _check_hamming84_forwards(*_mods(gpu))


# ---- 7. the dispatcher operator -------------------------------------------------------------------------
OP_PATH = next(p for p in GOLAY_PATHS if p[0] == "golay_packed" and p[2] == 128 and p[3] == 8 and p[1] == torch.float16)


def _op_args(dev, spans, stats):
    codec, dtype, d, heads, kvh, _, _ = OP_PATH
    c, q, _, _ = _case(OP_PATH, 5, "planted", 0)
    lay = _layout(codec, d, c)
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    return (t(q), t(lay["kc"]), t(lay["vc"]), t(c["table"]), t(c["lens"]), spans, t(c["ks"]), t(c["vs"]), stats,
            LAYER, BS, 1 / math.sqrt(d), codec)


def _check_dispatcher(mod, dev):
    import kvecc
    from kvecc import torch_ops
    assert "paged_attention_golay_stats" in torch_ops.OPS
    codec, dtype, d = OP_PATH[:3]
    c, q, want, _ = _case(OP_PATH, 5, "planted", 0)
    spans = torch.tensor([[1, 4, 0], [4, 1, 4], [0, 0, 5], [2, 3, 5]], dtype=torch.int32, device=dev)
    for sp in (None, spans):
        st = mod.new_stats(dev)
        a = _op_args(dev, sp, st)
        got = torch.ops.kvecc.paged_attention_golay_stats(*a)
        assert mod.read_stats(st) == want  # sequence 2 is empty either way
        st2 = mod.new_stats(dev)
        out = torch.full(q.shape, 77.0, dtype=q.dtype, device=dev)
        mod.paged_attention_counted_into(a[0], a[1], a[2], a[3], a[4], a[6], a[7], out, LAYER, BS, a[11], codec, st2,
                                         q_spans=sp)
        assert torch.equal(out, got) and mod.read_stats(st2) == want
        st3 = mod.new_stats(dev)
        pub = kvecc.paged_attention_counted(a[0], a[1], a[2], a[3], a[4], a[6], a[7], LAYER, BS, st3, codec=codec,
                                            q_spans=sp)
        assert torch.equal(pub, got) and mod.read_stats(st3) == want
        torch.library.opcheck(torch.ops.kvecc.paged_attention_golay_stats.default, a)


def test_cpu_dispatcher_op():
    _check_dispatcher(*_mods(None))


@pytest.mark.gpu
def test_hip_dispatcher_op(gpu):
    _check_dispatcher(*_mods(gpu))


def test_dispatcher_op_traces_under_compile():
    from kvecc import cpu_ops
    want = _case(OP_PATH, 5, "planted", 0)[2]
    fn = torch.compile(lambda *x: torch.ops.kvecc.paged_attention_golay_stats(*x) * 2, fullgraph=True,
                       backend="eager")
    st, st2 = cpu_ops.new_stats(), cpu_ops.new_stats()
    assert torch.equal(fn(*_op_args(None, None, st)),
                       torch.ops.kvecc.paged_attention_golay_stats(*_op_args(None, None, st2)) * 2)
    assert cpu_ops.read_stats(st) == want == cpu_ops.read_stats(st2)
