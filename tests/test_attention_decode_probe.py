"""Every inline ECC decoder of kvecc_paged_attention, on every syndrome.

The attention kernels do not call the library's shared decoder: each
instantiation stages tables of its own and decodes with its own bit arithmetic
(csrc/attention.hip).  tests/test_attention_paths.py sees those decoders only
through a tolerance on a softmax blend of random tokens.  Here paged attention
is turned into an exact reader of single K and V rows, and every entry of PATHS
reads rows that hold every syndrome.

Probe rows (per head_dim d, seeded):
- Golay: 4096 words, encode(random data) ^ (s << 12) for every syndrome s (H is
  [B^T | I12], so the word's syndrome is s), in a seeded order, plus padding
  words with random syndromes up to a multiple of g = ceil(d / 3): R =
  ceil(4096 / g) rows.  Packed rows carry 0xFF in the bytes after their last
  codeword (the layout leaves them undefined).
- Hamming(8,4): the 256 byte values in 4 seeded permutations, cut into rows of d.
The expected nibbles come from the oracle (the C restatement of the reference,
pinned by the golden fixtures), never from kvecc.  Cache head k holds the rows
rotated by 7k.

V probe: block_size 1, one block per row, a 256-column table that is -1 except
column b % 256, context_lens 256.  One token is valid, its weight is 1, so
out[b, h] = (nibble - 8) * v_scale of cache head h / group, exactly.

K probe: column b % 256 holds the probed row (V all nibble 15 at scale S_V),
the next column a shared reference block (K all nibble N_REF, V all nibble 8 =
0).  Query head h of sequence b is one-hot at one element, so every lane of
out[b, h] is 7 * S_V * sigmoid(SM_SCALE * (nibble - N_REF)): 16 candidate
values, of which the nearest must be the expected nibble's.  SM_SCALE, N_REF
and S_V are chosen so that half the gap between adjacent candidates is at least
4 tolerances of the query dtype (test_margins asserts it before any kernel runs).

Sequences wrap over the rows where a path has fewer than 256 of them, so that
every token column 0..255 holds a probed row for every path.
"""

import functools

import numpy as np
import pytest
import torch

from tests.test_attention_paths import (BF16, F16, F32, FAMILIES, PATHS, TOL, _base, _cdiv, _id, _pack_golay,
                                        _select)
from tests.test_shim_read_batch import oracle_read

SM_SCALE, N_REF, S_V = 0.25, 15, 16.0
LAYERS, LAYER = 2, 1  # layer 0 of every cache is zero, layer 1 is read
ROT = 7  # cache head k holds row (r + ROT * k) % R in block r
COLS = 256
MAX_WG = 4096  # batch x heads per launch: the counted combine's limit (kCtrPerSlot)
CAND = 7.0 * S_V / (1.0 + np.exp(-SM_SCALE * (np.arange(16.0) - N_REF)))  # increasing in the nibble
MIDS = (CAND[1:] + CAND[:-1]) / 2


def _oracle():
    from oracle import oracle as o
    o.lib()
    return o


# ---- probe rows -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rows(base, d):
    """-> (words [R, per] int32 / uint8, expected nibbles [R, d] uint8, flat codewords, flat
    oracle decode [n, 3] / [n], what each word is one of: its syndrome / its byte value [R, per]);
    asserts the set and the expectation's semantics."""
    o = _oracle()
    rng = np.random.default_rng(1000 * (base == "golay") + d)
    if base == "golay":
        g = (d + 2) // 3
        rows = _cdiv(4096, g)
        n = rows * g
        syn = np.concatenate([rng.permutation(4096), rng.integers(0, 4096, n - 4096)]).astype(np.int64)
        data = rng.integers(0, 16, (n, 3)).astype(np.uint8)
        cw = (o.golay_encode(data).astype(np.int64) ^ (syn << 12)).astype(np.int32)
        trip, cnt, _ = o.golay_decode(cw)
        # all 4096 syndromes (recomputed from the parity-check rows), 1771 of them uncorrectable
        h = o.golay_h_row_masks().astype(np.int64)
        par = np.zeros((n, 12), np.int64)
        for bit in range(24):
            par ^= ((cw.astype(np.int64)[:, None] & h[None, :]) >> bit) & 1
        got_syn = (par << np.arange(12)).sum(1)
        assert np.array_equal(got_syn, syn)
        assert np.array_equal(np.sort(got_syn[:4096]), np.arange(4096))
        assert int((cnt[:4096] == 4).sum()) == 1771 and int((cnt[:4096] == 3).sum()) == 2024
        # an uncorrectable word keeps its received data nibbles
        recv = np.stack([cw & 15, cw >> 4 & 15, cw >> 8 & 15], 1).astype(np.uint8)
        assert np.array_equal(trip[cnt == 4], recv[cnt == 4])
        assert not np.array_equal(trip[cnt == 3], recv[cnt == 3])
        nib = trip.reshape(rows, 3 * g)[:, :d]
        return cw.reshape(rows, g), np.ascontiguousarray(nib), cw, trip, syn.reshape(rows, g)
    rows = _cdiv(1024, d)
    cw = np.concatenate([rng.permutation(256) for _ in range(4)] + [rng.integers(0, 256, rows * d - 1024)])
    cw = cw.astype(np.uint8)
    dec, et, _ = o.hamming84_decode(cw)
    assert all(np.array_equal(np.sort(cw[256 * i:256 * i + 256]), np.arange(256)) for i in range(4))
    # double errors keep their data (include/kvecc.h, kvecc_paged_attention); 112 of 256 bytes
    assert int((et[:256] == 2).sum()) == 112
    assert np.array_equal(dec[et == 2], cw[et == 2] & 15)
    return cw.reshape(rows, d), dec.reshape(rows, d), cw, dec, cw.reshape(rows, d)


def _per_head(a, kvh):
    """[R, ...] -> [R, kvh, ...]: head k of block r holds a[(r + ROT * k) % R]."""
    return np.stack([np.roll(a, -ROT * k, axis=0) for k in range(kvh)], axis=1)


def _const_row(base, d, nibble):
    o = _oracle()
    if base == "golay":
        return o.golay_encode(np.full(((d + 2) // 3, 3), nibble, np.uint8))
    return o.hamming84_encode(np.full(d, nibble, np.uint8))


def _cache(codec, d, words):
    """words [blocks, kvh, bs, per] -> the cache [blocks, LAYERS, kvh, bs * row] kvecc reads
    (layer 0 zero); packed rows get 0xFF in the bytes after the last codeword."""
    nb, kvh, bs, per = words.shape
    c = torch.zeros(nb, LAYERS, kvh, bs * per, dtype=torch.from_numpy(words).dtype)
    c[:, LAYER] = torch.from_numpy(words.reshape(nb, kvh, bs * per))
    if codec == "golay_packed":
        c = _pack_golay(c, d)
        c.view(nb, LAYERS, kvh, bs, -1)[..., 3 * per:] = 0xFF
    return c.contiguous()


def _flip_words(words, flip):
    if flip is not None:
        blk, head, word, bit = flip
        words[blk, head, 0, word] ^= words.dtype.type(1 << bit)


def _table(blocks, bs, ref_block=None):
    """Sequence j: block blocks[j] in column j % 256 (and ref_block in the next) of 256 columns
    (bs 1), or in its only column (bs 16)."""
    n = len(blocks)
    if bs != 1:
        return torch.from_numpy(blocks.astype(np.int32)).view(n, 1).contiguous()
    t = np.full((n, COLS), -1, np.int32)
    j = np.arange(n)
    t[j, j % COLS] = blocks
    if ref_block is not None:
        t[j, (j + 1) % COLS] = ref_block
    return torch.from_numpy(t)


def _launch(mod, dev, codec, dtype, q, kc, vc, table, lens, ks, vs, bs, mcl, step=MAX_WG):
    """paged_attention_into in chunks of at most step and MAX_WG // heads sequences -> float64 on the host."""
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    kc, vc, ks, vs = t(kc), t(vc), t(ks), t(vs)
    step = min(step, MAX_WG // q.shape[1])  # batch x heads <= MAX_WG in every launch
    outs = []
    for s in range(0, q.shape[0], step):
        qs = t(q[s:s + step].to(dtype).contiguous())
        out = torch.empty(qs.shape, dtype=dtype, device=dev)
        mod.paged_attention_into(qs, kc, vc, t(table[s:s + step].contiguous()), t(lens[s:s + step].contiguous()),
                                 ks, vs, out, LAYER, bs, SM_SCALE, codec, max_context_len=mcl)
        outs.append(out.cpu())
    out = torch.cat(outs)
    return out.double().numpy(), out


def _sites(bad, blocks, group, elem=None):
    """Positions of a [seq, head, lane or nothing] mask as sorted (block, cache head, element)."""
    idx = np.argwhere(bad)
    e = idx[:, 2] if elem is None else elem[idx[:, 0], idx[:, 1] % group]
    return sorted({(int(b), int(k), int(x)) for b, k, x in zip(blocks[idx[:, 0]], idx[:, 1] // group, e)})


# ---- the V probe ------------------------------------------------------------------------------
def _v_probe(mod, dev, path, bs=1, flip=None):
    """-> dict(bad, far: sites whose nibble / whose value is off, err, bit_equal)."""
    codec, dtype, d, heads, kvh = path[:5]
    base, group = _base(codec), heads // kvh
    words, nib, _, _, kinds = _rows(base, d)
    rows = len(words)
    nseq = max(rows, COLS) if bs == 1 else rows
    blocks = np.arange(nseq) % rows
    w = np.zeros((rows, kvh, bs, words.shape[1]), words.dtype)
    w[:, :, 0] = _per_head(words, kvh)
    _flip_words(w, flip)
    vc = _cache(codec, d, w)
    vs = torch.ones(rows, LAYERS, kvh, bs)
    vs[:] = (2.0 ** -(torch.arange(rows) % 4)).view(rows, 1, 1, 1)
    q = torch.randn(nseq, heads, d, generator=torch.Generator().manual_seed(d))
    lens = torch.full((nseq,), COLS if bs == 1 else 1, dtype=torch.int32)
    # one launch per pass over the rows: a path with few rows keeps its small batch, at which the
    # launcher splits the 256 columns into 8 (choose_split), 7 of them without a valid token
    got, raw = _launch(mod, dev, codec, dtype, q, vc, vc, _table(blocks, bs), lens, torch.ones_like(vs), vs, bs,
                       0 if bs == 1 else 1, rows)
    # coverage: every row of both cache heads, so every syndrome / byte value; every column
    assert len(np.unique(kinds[np.unique(blocks)])) == (4096 if base == "golay" else 256)
    if bs == 1:
        assert set(np.arange(nseq) % COLS) == set(range(COLS))
    scale = vs[blocks, LAYER, 0, 0].double().numpy()[:, None, None]
    exp_nib = np.repeat(_per_head(nib, kvh)[blocks], group, axis=1)  # [seq, heads, d]
    exp = (exp_nib.astype(np.float64) - 8.0) * scale
    atol, rtol = TOL[dtype]
    diff = np.abs(got - exp)
    return dict(bad=_sites(np.rint(got / scale) + 8 != exp_nib, blocks, group),
                far=_sites(~(diff <= atol + rtol * np.abs(exp)), blocks, group), err=float(diff.max()),
                bit_equal=bool(torch.equal(raw, torch.from_numpy(exp).to(dtype))))


# ---- the K probe ------------------------------------------------------------------------------
def _margin(dtype):
    """min over adjacent candidates of (half their gap) / (the tolerance at the larger one)."""
    atol, rtol = TOL[dtype]
    return float(((CAND[1:] - CAND[:-1]) / 2 / (atol + rtol * CAND[1:])).min())


def _k_probe(mod, dev, path, bs=1, flip=None):
    codec, dtype, d, heads, kvh = path[:5]
    assert _margin(dtype) >= 4
    base, group = _base(codec), heads // kvh
    words, nib, _, _, kinds = _rows(base, d)
    rows, per_row = len(words), _cdiv(d, group)
    n = rows * per_row
    nseq = max(n, COLS) if bs == 1 else n
    j = np.arange(nseq) % n
    blocks = j // per_row
    elem = np.minimum((j % per_row)[:, None] * group + np.arange(group), d - 1)  # [seq, member of the group]
    ref_block = rows if bs == 1 else None
    nb = rows + (bs == 1)
    kw = np.zeros((nb, kvh, bs, words.shape[1]), words.dtype)
    vw = np.zeros_like(kw)
    kw[:rows, :, 0] = _per_head(words, kvh)
    vw[:rows, :, 0] = _const_row(base, d, 15)
    kw[rows:, :, 0] = _const_row(base, d, N_REF)  # bs 1: the shared reference block
    vw[rows:, :, 0] = _const_row(base, d, 8)
    if bs != 1:  # the reference row in slot 1 of the probed row's block
        kw[:, :, 1] = _const_row(base, d, N_REF)
        vw[:, :, 1] = _const_row(base, d, 8)
    _flip_words(kw, flip)
    q = torch.zeros(nseq, heads, d)
    hh = np.arange(heads)
    q[torch.arange(nseq)[:, None], torch.arange(heads)[None, :], torch.from_numpy(elem[:, hh % group])] = 1.0
    ones = torch.ones(nb, LAYERS, kvh, bs)
    lens = torch.full((nseq,), COLS if bs == 1 else 2, dtype=torch.int32)
    got, _ = _launch(mod, dev, codec, dtype, q, _cache(codec, d, kw), _cache(codec, d, vw),
                     _table(blocks, bs, ref_block), lens, ones, ones * S_V, bs, 0 if bs == 1 else 2)
    # coverage: every element of every row of both cache heads, once or (wrapped) more; every column
    seen = np.zeros((rows, d), bool)
    seen[blocks[:, None], elem] = True
    assert seen.all() and len(np.unique(kinds[np.unique(blocks)])) == (4096 if base == "golay" else 256)
    if bs == 1:
        assert set(np.arange(nseq) % COLS) == set(range(COLS))
    exp_nib = _per_head(nib, kvh)[blocks[:, None], hh[None, :] // group, elem[:, hh % group]]  # [seq, heads]
    exp = CAND[exp_nib][:, :, None]
    atol, rtol = TOL[dtype]
    diff = np.abs(got - exp)
    return dict(bad=_sites((np.searchsorted(MIDS, got) != exp_nib[:, :, None]).any(-1), blocks, group, elem),
                far=_sites((~(diff <= atol + rtol * exp)).any(-1), blocks, group, elem), err=float(diff.max()))


def test_margins():
    """Half the gap between adjacent K-probe candidates, in tolerances of the query dtype."""
    m = {dt: _margin(dt) for dt in (F32, F16, BF16)}
    print("K-probe margins (fp32, fp16, bf16):", [round(m[dt], 1) for dt in (F32, F16, BF16)],
          "smallest gap", float((CAND[1:] - CAND[:-1]).min()))
    assert all(v >= 4 for v in m.values())
    assert 300 < m[F32] < 320 and 60 < m[F16] < 62 and 6.0 < m[BF16] < 6.2
    # the obvious choice (reference nibble 8, V scale 1) would not do for bf16
    cand = 7.0 / (1.0 + np.exp(-SM_SCALE * (np.arange(16.0) - 8)))
    assert ((cand[1:] - cand[:-1]) / 2 / (TOL[BF16][0] + TOL[BF16][1] * cand[1:])).min() < 2


def _check_v(mod, dev, path, bs=1):
    r = _v_probe(mod, dev, path, bs)
    print(f"V probe {_id(path)} bs {bs}: max |out - expected| {r['err']:.3e}, bit-equal {r['bit_equal']}")
    assert r["bad"] == [], r["bad"][:8]
    assert r["far"] == [], (r["far"][:8], r["err"])
    if dev is None:  # 4-bit integers times powers of two: exact in every dtype on the host twin
        assert r["bit_equal"]


def _check_k(mod, dev, path, bs=1):
    r = _k_probe(mod, dev, path, bs)
    print(f"K probe {_id(path)} bs {bs}: max |out - expected| {r['err']:.3e}")
    assert r["bad"] == [], r["bad"][:8]
    assert r["far"] == [], (r["far"][:8], r["err"])


@pytest.mark.parametrize("path", PATHS, ids=_id)
def test_cpu_v_probe(path):
    from kvecc import cpu_ops
    _check_v(cpu_ops, None, path)


@pytest.mark.parametrize("path", PATHS, ids=_id)
def test_cpu_k_probe(path):
    from kvecc import cpu_ops
    _check_k(cpu_ops, None, path)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS, ids=_id)
def test_hip_v_probe(gpu, path):
    from kvecc import ops
    _check_v(ops, gpu, path)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS, ids=_id)
def test_hip_k_probe(gpu, path):
    from kvecc import ops
    _check_k(ops, gpu, path)


# ---- the normal block size --------------------------------------------------------------------
# block_size 16, the probed row in slot 0 and the reference row in slot 1 of one block,
# context_lens 1 (V) / 2 (K), max_context_len passed as append mode passes it: one entry per
# kernel family, a packed split path whose rows end in 3 bytes of padding, and a bf16 path
BS16 = [p for p in PATHS if p[:5] in FAMILIES + [("golay_packed", F32, 7, 2, 2), ("golay", BF16, 128, 8, 2)]]


def test_bs16_entries():
    assert len(BS16) == 6 and set(FAMILIES) <= {p[:5] for p in BS16}
    assert _select("golay_packed", F32, 7, 2, 2)[0] == "paged_attn_split_kernel<float, 4, 3, 1, true, 1, 0, 0>"


@pytest.mark.parametrize("path", BS16, ids=_id)
def test_cpu_probes_block_size_16(path):
    from kvecc import cpu_ops
    _check_v(cpu_ops, None, path, 16)
    _check_k(cpu_ops, None, path, 16)


@pytest.mark.gpu
@pytest.mark.parametrize("path", BS16, ids=_id)
def test_hip_probes_block_size_16(gpu, path):
    from kvecc import ops
    _check_v(ops, gpu, path, 16)
    _check_k(ops, gpu, path, 16)


# ---- the same rows through the fused reads ------------------------------------------------------
FUSED = [("golay", 128, False), ("golay_packed", 128, False), ("golay", 100, False), ("golay_packed", 100, False),
         ("hamming84", 64, False), ("hamming84", 64, True)]


@functools.lru_cache(maxsize=None)
def _fused_case(codec, d, interp):
    """The probe rows as the tokens of a block_size 16 cache, two cache heads, two sequences (the
    second reads the blocks in reverse order) -> caches, scales, table, ctx and the oracle's
    (K, V, statistics) per output dtype."""
    words = _rows(_base(codec), d)[0]
    rows, per = words.shape
    nb = _cdiv(rows, 16)
    caches = []
    for shift in (0, 3):  # V holds the rows three further on
        w = np.zeros((nb * 16, 2, per), words.dtype)
        w[:rows] = _per_head(np.roll(words, -shift, axis=0), 2)
        caches.append(_cache(codec, d, np.ascontiguousarray(w.reshape(nb, 16, 2, per).transpose(0, 2, 1, 3))))
    g = torch.Generator().manual_seed(d)
    ks, vs = (torch.rand(nb, LAYERS, 2, 16, generator=g) * 0.5 + 0.01 for _ in range(2))
    table = torch.stack([torch.arange(nb), torch.arange(nb).flip(0)]).to(torch.int32).contiguous()
    exp = {}
    for dt in (F32, F16):
        ek, sk = oracle_read(_oracle(), caches[0], ks, table, rows, d, LAYER, codec, dt, interp)
        ev, sv = oracle_read(_oracle(), caches[1], vs, table, rows, d, LAYER, codec, dt, interp)
        exp[dt] = (ek, ev, [sk[0] + sv[0], sk[1] + sv[1]])
    assert exp[F32][2][1] > 0  # uncorrectable words / double errors were read
    return caches[0], caches[1], ks, vs, table, rows, exp


def _check_fused(mod, dev, codec, d, interp):
    kc, vc, ks, vs, table, ctx, exp = _fused_case(codec, d, interp)
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    for dt in (F32, F16):
        st = mod.new_stats(dev) if dev is not None else mod.new_stats()
        k, v = mod.shim_read_batch(t(kc), t(vc), t(ks), t(vs), t(table), ctx, d, LAYER, codec, dt, stats=st,
                                   interp=interp)
        assert torch.equal(k.cpu(), exp[dt][0]) and torch.equal(v.cpu(), exp[dt][1])
        assert mod.read_stats(st) == exp[dt][2]


@pytest.mark.parametrize("codec,d,interp", FUSED)
def test_cpu_fused_read_of_the_probe_rows(codec, d, interp):
    from kvecc import cpu_ops
    _check_fused(cpu_ops, None, codec, d, interp)


@pytest.mark.gpu
@pytest.mark.parametrize("codec,d,interp", FUSED)
def test_hip_fused_read_of_the_probe_rows(gpu, codec, d, interp):
    from kvecc import ops
    _check_fused(ops, gpu, codec, d, interp)


# ---- sensitivity ----------------------------------------------------------------------------------
SELF = [p for p in PATHS if p[:5] in [("golay", F32, 20, 2, 2), ("golay_packed", F16, 100, 4, 2),
                                      ("hamming84", BF16, 52, 2, 2)]]


def _one_nibble_flip(base, d):
    """The first stored codeword of cache head 0 whose decode changes in exactly one live element
    when its data bit 0 flips -> ((block, head 0, word, bit 0), (block, 0, element))."""
    o = _oracle()
    words, _, cw, dec, _ = _rows(base, d)
    per = words.shape[1]
    if base == "golay":
        changed = (o.golay_decode(cw ^ 1)[0] != dec).reshape(len(words), per * 3)
    else:
        changed = (o.hamming84_decode(cw ^ 1)[0] != dec).reshape(len(words), per)
    span = 3 if base == "golay" else 1
    for blk, word in np.argwhere(changed.reshape(len(words), per, span).sum(-1) == 1):
        e = word * span + int(np.argmax(changed[blk, word * span:word * span + span]))
        if e < d:
            return (int(blk), 0, int(word), 0), (int(blk), 0, int(e))
    raise AssertionError("no such codeword")


@pytest.mark.parametrize("path", SELF, ids=_id)
def test_probes_name_one_flipped_bit(path):
    """One data bit of one stored codeword flipped after the expectation was computed: both
    probes report that (block, cache head, element) and nothing else."""
    from kvecc import cpu_ops
    assert len(SELF) == 3
    flip, site = _one_nibble_flip(_base(path[0]), path[2])
    for probe in (_v_probe, _k_probe):
        r = probe(cpu_ops, None, path, 1, flip)
        assert r["bad"] == [site] and r["far"] == [site], (probe.__name__, r["bad"][:8], r["far"][:8])
