"""In-place cache scrub (kvecc_cache_scrub / kvecc_cpu_cache_scrub) at the ops level.

Contract (include/kvecc.h, "Cache scrub"): every codeword of every valid token of the layer range,
K and V, is decoded; a correctable word whose stored codeword bits differ from encode(decoded data)
is replaced by that codeword, an uncorrectable word (H84 double, Golay count 4) and every bit
outside the codewords stay.  The expectation is restated in numpy from the oracle codecs alone:
    where(valid & correctable & dirty, canonical codeword with the outside bits kept, stored)
and every byte of both caches is compared, bit for bit, together with the four statistics.

Geometry: batch 4, 2 KV heads, block_size 4, 16 physical blocks, a randperm table of 3 blocks per
sequence, 3 layers of which [1, 3) is scrubbed; lengths [12, 5, 0, 9] for layer 1 and other ones
for layer 2 (lens_layer_stride); one -1 and one id >= num_blocks inside live sequences.  The whole
cache tensors hold valid codewords, then flips at BER 5e-2 everywhere, packed pad bytes 0xFF,
random H74 bit 7 / Golay bits 24..31.  The host twin runs everywhere, the HIP kernel under the
gpu marker.
"""

import ctypes

import numpy as np
import pytest
import torch

import kvecc

NB, NL, HKV, BS = 16, 3, 2, 4
BATCH, NPER = 4, 3
FIRST, COUNT = 1, 2
LENS = [[12, 5, 0, 9], [7, 12, 3, 0]]  # row i: layer FIRST + i
BER = 5e-2
GRID = [("hamming74", 32), ("hamming84", 32), ("golay", 32), ("golay_packed", 32), ("golay", 7),
        ("golay_packed", 7), ("hamming84", 4)]
IDS = [f"{c}-d{d}" for c, d in GRID]
N_BITS = {"hamming74": 7, "hamming84": 8, "golay": 24, "golay_packed": 8}


@pytest.fixture(params=["cpu", pytest.param("hip", marks=pytest.mark.gpu)])
def be(request):
    """(backend module, device) of the host twin / the HIP kernels."""
    if request.param == "cpu":
        from kvecc import cpu_ops
        return cpu_ops, torch.device("cpu")
    from kvecc import ops
    return ops, request.getfixturevalue("gpu")


def _per(codec, d):
    g = (d + 2) // 3
    return {"golay": g, "golay_packed": (3 * g + 3) // 4 * 4}.get(codec, d)


# ---- the oracle restatement ------------------------------------------------------------------

def _unpack3(rows, g):
    """packed rows [..., rowb] uint8 -> int32 codewords [..., g]"""
    b = rows[..., :3 * g].reshape(*rows.shape[:-1], g, 3).astype(np.uint32)
    return (b[..., 0] | b[..., 1] << 8 | b[..., 2] << 16).astype(np.int32)


def _pack3(rows, cw, g):
    """rows with the codewords cw [..., g] written over their 3 bytes each (pad bytes kept)"""
    out = rows.copy()
    u = cw.astype(np.uint32)
    b = np.stack([u & 0xFF, u >> 8 & 0xFF, u >> 16 & 0xFF], axis=-1).astype(np.uint8)
    out[..., :3 * g] = b.reshape(*rows.shape[:-1], 3 * g)
    return out


def _words(oracle, codec, stored):
    """Per codeword of `stored` (uint8 bytes, or int32 Golay words): (the word to store when it is
    rewritten, correctable, statistic-0 contribution, statistic-1 contribution)."""
    if codec == "hamming84":
        data, et, _ = oracle.hamming84_decode(stored)
        return oracle.hamming84_encode(data).reshape(stored.shape), et.reshape(stored.shape) != 2, \
            (et == 1).reshape(stored.shape).astype(np.int64), (et == 2).reshape(stored.shape).astype(np.int64)
    if codec == "hamming74":
        data, flag, _ = oracle.hamming74_decode(stored & 0x7F)  # bit 7 is not part of the code
        canon = oracle.hamming74_encode(data).reshape(stored.shape) | (stored & 0x80)
        return canon, np.ones(stored.shape, bool), flag.reshape(stored.shape).astype(np.int64), \
            np.zeros(stored.shape, np.int64)
    u = stored.astype(np.uint32)
    trip, cnt, _ = oracle.golay_decode((u & 0xFFFFFF).astype(np.int32))
    cnt = cnt.reshape(stored.shape).astype(np.int64)
    canon = oracle.golay_encode(trip).reshape(stored.shape).astype(np.uint32) | (u & 0xFF000000)
    return canon.astype(np.int32), cnt < 4, np.where(cnt < 4, cnt, 0), (cnt == 4).astype(np.int64)


def _expect(oracle, codec, d, cache, valid):
    """cache [NB', NL', HKV', BS', per] (numpy), valid [NB', NL', HKV', BS'] bool ->
    (scrubbed cache, [corrected, detected, rewritten, scanned])."""
    g = (d + 2) // 3
    stored = _unpack3(cache, g) if codec == "golay_packed" else cache
    canon, ok, s0, s1 = _words(oracle, codec, stored)
    m = valid[..., None]
    rewrite = m & ok & (canon != stored)
    new = np.where(rewrite, canon, stored)
    stats = [int((s0 * m).sum()), int((s1 * m).sum()), int(rewrite.sum()), int(m.sum()) * stored.shape[-1]]
    return (_pack3(cache, new, g) if codec == "golay_packed" else new.astype(cache.dtype)), stats


def _valid(table, lens, first, count, nb, nl, hkv, bs, mcl=0):
    """Token rows a scrub of layers [first, first + count) covers: lens[i][b] tokens of sequence
    b in layer first + i, clamped to min(mcl, table width * bs); ids outside [0, nb) skipped."""
    v = np.zeros((nb, nl, hkv, bs), bool)
    bound = table.shape[1] * bs
    if mcl > 0:
        bound = min(bound, mcl)
    for i in range(count):
        for b in range(table.shape[0]):
            for p in range(max(min(lens[i][b], bound), 0)):
                blk = int(table[b, p // bs])
                if 0 <= blk < nb:
                    v[blk, first + i, :, p % bs] = True
    return v


# ---- the shared, never modified inputs ---------------------------------------------------------

def _table():
    t = torch.randperm(NB, generator=torch.Generator().manual_seed(5))[:BATCH * NPER].view(BATCH, NPER)
    t = t.to(torch.int32).numpy().copy()
    t[0, 1] = -1       # a missing block inside the full sequence
    t[3, 0] = NB + 3   # an id past the cache inside a live sequence
    return t


_INPUTS = {}


def _inputs(oracle, codec, d):
    """(k, v) numpy caches [NB, NL, HKV, BS, per] of injected valid codewords, built once per case."""
    key = (codec, d)
    if key not in _INPUTS:
        rng = np.random.default_rng(100 + d + 7 * len(codec))
        g, per = (d + 2) // 3, _per(codec, d)
        out = []
        for side in range(2):
            shape = (NB, NL, HKV, BS)
            if codec in ("hamming74", "hamming84"):
                nib = rng.integers(0, 16, (*shape, d), dtype=np.uint8)
                c = (oracle.hamming84_encode if codec == "hamming84" else oracle.hamming74_encode)(nib).reshape(nib.shape)
                if codec == "hamming74":
                    c = c | (rng.integers(0, 2, c.shape, dtype=np.uint8) << 7)
            else:
                trip = rng.integers(0, 16, (int(np.prod(shape)) * g, 3), dtype=np.uint8)
                cw = oracle.golay_encode(trip).reshape(*shape, g)
                if codec == "golay":
                    hi = rng.integers(0, 256, cw.shape, dtype=np.uint32) << 24
                    c = (cw.astype(np.uint32) | hi).astype(np.int32)
                else:
                    c = _pack3(np.full((*shape, per), 0xFF, np.uint8), cw, g)
            c = oracle.inject(c, BER, N_BITS[codec], seed=31 + side)[0].reshape(c.shape)
            if codec == "golay_packed":
                c[..., 3 * g:] = 0xFF
            out.append(c)
        _INPUTS[key] = tuple(out)
    return _INPUTS[key]


def _t(a, dev):
    """numpy [NB', NL', HKV', BS', per] -> the torch cache tensor [NB', NL', HKV', BS' * per]"""
    return torch.from_numpy(a.reshape(*a.shape[:3], -1).copy()).to(dev)


def _back(t, like):
    return t.cpu().numpy().reshape(like.shape)


def _totals(mod, st):
    return [int(x) for x in mod.stats_totals(st, 4).tolist()]


def _scrub(mod, k, v, table, lens, codec, d, stats, first=FIRST, count=COUNT, mcl=0, nl=NL, bs=BS):
    mod.cache_scrub_tensors(k, v, table, lens, d, bs, nl, codec, layer_first=first, layer_count=count,
                            max_context_len=mcl, stats=stats)


# ---- the main property ---------------------------------------------------------------------

@pytest.mark.parametrize("codec,d", GRID, ids=IDS)
def test_scrub_matches_oracle_restatement(be, oracle, codec, d):
    mod, dev = be
    k0, v0 = _inputs(oracle, codec, d)
    table = _table()
    valid = _valid(table, LENS, FIRST, COUNT, NB, NL, HKV, BS)
    assert valid[:, 0].sum() == 0 and valid.sum() > 0
    (wk, sk), (wv, sv) = _expect(oracle, codec, d, k0, valid), _expect(oracle, codec, d, v0, valid)
    want = [a + b for a, b in zip(sk, sv)]
    assert want[2] > 0 and want[0] > 0 and (codec == "hamming74" or want[1] > 0)  # the case exercises every branch
    k, v = _t(k0, dev), _t(v0, dev)
    tt, ll = torch.from_numpy(table).to(dev), torch.tensor(LENS, dtype=torch.int32, device=dev)
    st = mod.new_scrub_stats(dev)
    _scrub(mod, k, v, tt, ll, codec, d, st)
    assert np.array_equal(_back(k, k0), wk) and np.array_equal(_back(v, v0), wv)  # every byte of both caches
    assert _totals(mod, st) == want
    # [0] and [1] are the reader's counts over the same tokens (the pre-scrub cache)
    if codec != "hamming74":
        rst = mod.new_stats(dev)
        kd, vd = _t(k0, dev), _t(v0, dev)
        sc = torch.zeros((NB, NL, HKV, BS), device=dev)
        safe = np.where((table >= 0) & (table < NB), table, -1).astype(np.int32)
        bound = NPER * BS
        for i in range(COUNT):
            for b in range(BATCH):
                ctx = min(LENS[i][b], bound)
                if ctx > 0:
                    mod.shim_read_batch(kd, vd, sc, sc, torch.from_numpy(safe[b:b + 1]).to(dev), ctx, d, FIRST + i,
                                        codec, torch.float32, stats=rst)
        assert mod.read_stats(rst, 2) == want[:2]
    # idempotent: a second pass changes nothing and rewrites nothing
    st2 = mod.new_scrub_stats(dev)
    _scrub(mod, k, v, tt, ll, codec, d, st2)
    assert np.array_equal(_back(k, k0), wk) and np.array_equal(_back(v, v0), wv)
    got2 = _totals(mod, st2)
    assert got2[2] == 0 and got2[3] == want[3] and got2[1] == want[1]
    # NULL statistics
    k, v = _t(k0, dev), _t(v0, dev)
    _scrub(mod, k, v, tt, ll, codec, d, None)
    assert np.array_equal(_back(k, k0), wk) and np.array_equal(_back(v, v0), wv)


@pytest.mark.parametrize("codec,d", [("hamming84", 32), ("golay", 7), ("golay_packed", 7)], ids=["h84", "golay7", "packed7"])
def test_public_call_and_one_row_of_lengths(be, oracle, codec, d):
    """kvecc.cache_scrub: layers=, a [batch] length row for every layer, totals as a device tensor,
    accumulation into a caller's buffer; unaligned cache bases (a view one row into a buffer)."""
    mod, dev = be
    k0, v0 = _inputs(oracle, codec, d)
    table = _table()
    valid = _valid(table, [LENS[0]] * NL, 0, NL, NB, NL, HKV, BS)
    (wk, sk), (wv, sv) = _expect(oracle, codec, d, k0, valid), _expect(oracle, codec, d, v0, valid)
    per = _per(codec, d)
    # bases 4 bytes past a fresh allocation: unaligned heads, 16-byte vectors and tails all occur
    off = 1 if codec == "golay" else 4
    bufk = torch.zeros(k0.size + off, dtype=_t(k0, "cpu").dtype, device=dev)
    bufv = torch.zeros(k0.size + off, dtype=bufk.dtype, device=dev)
    k, v = bufk[off:].view(NB, NL, HKV, BS * per), bufv[off:].view(NB, NL, HKV, BS * per)
    k.copy_(_t(k0, dev))
    v.copy_(_t(v0, dev))
    acc = mod.new_scrub_stats(dev)
    tot = kvecc.cache_scrub(k, v, torch.from_numpy(table).to(dev), torch.tensor(LENS[0], dtype=torch.int32, device=dev),
                            head_dim=d, block_size=BS, num_layers=NL, codec=codec, stats=acc)
    assert tot.device.type == dev.type and tot.dtype == torch.int64 and tot.shape == (4,)
    assert tot.tolist() == [a + b for a, b in zip(sk, sv)] == _totals(mod, acc)
    assert np.array_equal(_back(k, k0), wk) and np.array_equal(_back(v, v0), wv)
    assert int(bufk[:off].sum()) == 0 and int(bufv[:off].sum()) == 0
    tot = kvecc.cache_scrub(k, v, torch.from_numpy(table).to(dev), torch.tensor(LENS[0], dtype=torch.int32, device=dev),
                            head_dim=d, block_size=BS, num_layers=NL, codec=codec, layers=[1], stats=acc)
    assert tot.tolist()[2] == 0 and _totals(mod, acc)[3] == (sk[3] + sv[3]) * (NL + 1) // NL


# ---- every syndrome ------------------------------------------------------------------------

@pytest.mark.parametrize("codec", ["golay", "golay_packed", "hamming84", "hamming74"])
def test_every_syndrome(be, oracle, codec):
    """All 4096 Golay syndromes as encode(random) ^ (s << 12), all 256 H84 bytes, all 128 H74
    values under both values of bit 7, laid out as the rows of one sequence."""
    mod, dev = be
    rng = np.random.default_rng(9)
    if codec in ("golay", "golay_packed"):
        d, g, hkv, bs, nb = 12, 4, 4, 16, 16
        cw = oracle.golay_encode(rng.integers(0, 16, (4096, 3), dtype=np.uint8)).astype(np.uint32)
        cw ^= np.arange(4096, dtype=np.uint32) << 12
        if codec == "golay":
            cache = (cw | rng.integers(0, 256, 4096, dtype=np.uint32) << 24).astype(np.int32).reshape(nb, 1, hkv, bs, g)
        else:
            cache = _pack3(np.zeros((nb, 1, hkv, bs, 12), np.uint8), cw.astype(np.int32).reshape(nb, 1, hkv, bs, g), g)
    else:
        d, hkv, bs, nb = 4, 1, 16, 4
        cache = np.arange(256, dtype=np.uint8).reshape(nb, 1, hkv, bs, d)
    table = np.arange(nb, dtype=np.int32).reshape(1, nb)
    valid = np.ones((nb, 1, hkv, bs), bool)
    want, stats = _expect(oracle, codec, d, cache, valid)
    if codec in ("golay", "golay_packed"):
        assert stats[1] == 1771 and stats[3] == 4096  # uncorrectable syndromes
        trip, cnt, _ = oracle.golay_decode(cw.astype(np.int32))
        unc = (cnt == 4).reshape(nb, 1, hkv, bs, g)
        stored = _unpack3(cache, g) if codec == "golay_packed" else cache
        assert np.array_equal((_unpack3(want, g) if codec == "golay_packed" else want)[unc], stored[unc])
        assert stats[2] == 4095 - 1771  # every correctable non-zero syndrome is rewritten
    elif codec == "hamming84":
        # 16 codewords, 112 singles in bits 0..6, 16 overall-parity flips (type 3), 112 doubles
        assert stats == [112, 112, 128, 256]
    else:
        assert stats[0] == 2 * 112 and stats[2] == 2 * 112 and stats[3] == 256
    k, v = _t(cache, dev), _t(cache, dev)
    st = mod.new_scrub_stats(dev)
    lens = torch.tensor([nb * bs], dtype=torch.int32, device=dev)
    _scrub(mod, k, v, torch.from_numpy(table).to(dev), lens, codec, d, st, first=0, count=1, nl=1, bs=bs)
    assert np.array_equal(_back(k, cache), want) and np.array_equal(_back(v, cache), want)
    assert _totals(mod, st) == [2 * s for s in stats]


# ---- clamps ----------------------------------------------------------------------------------

@pytest.mark.parametrize("codec,d", [("hamming84", 4), ("golay_packed", 7)], ids=["h84", "packed7"])
def test_lengths_clamp_to_table_and_max_context_len(be, oracle, codec, d):
    mod, dev = be
    k0, v0 = _inputs(oracle, codec, d)
    table = _table()
    tt = torch.from_numpy(table).to(dev)
    for lens, mcl, eff in (([100, 5, 1 << 30, 9], 0, [12, 5, 12, 9]), ([100, 9, 6, 2], 6, [6, 6, 6, 2]),
                           ([100, 9, 6, 2], 1000, [12, 9, 6, 2])):
        valid = _valid(table, [eff], 2, 1, NB, NL, HKV, BS)
        (wk, sk), (wv, sv) = _expect(oracle, codec, d, k0, valid), _expect(oracle, codec, d, v0, valid)
        assert _valid(table, [lens], 2, 1, NB, NL, HKV, BS, mcl).tolist() == valid.tolist()
        k, v = _t(k0, dev), _t(v0, dev)
        st = mod.new_scrub_stats(dev)
        _scrub(mod, k, v, tt, torch.tensor(lens, dtype=torch.int32, device=dev), codec, d, st, first=2, count=1, mcl=mcl)
        assert np.array_equal(_back(k, k0), wk) and np.array_equal(_back(v, v0), wv)
        assert _totals(mod, st) == [a + b for a, b in zip(sk, sv)]


def test_shared_blocks_and_empty_calls(be, oracle):
    """Two table rows naming the same block both scrub it (same values); batch 0 / no layers / all
    lengths 0 touch nothing."""
    mod, dev = be
    codec, d = "golay", 7
    k0, v0 = _inputs(oracle, codec, d)
    table = np.array([[3, 4, 5], [3, 4, 9]], np.int32)
    lens = [[12, 8]]
    valid = _valid(table, lens, 1, 1, NB, NL, HKV, BS)
    wk, _ = _expect(oracle, codec, d, k0, valid)
    wv, _ = _expect(oracle, codec, d, v0, valid)
    k, v = _t(k0, dev), _t(v0, dev)
    _scrub(mod, k, v, torch.from_numpy(table).to(dev), torch.tensor(lens, dtype=torch.int32, device=dev), codec, d, None,
           first=1, count=1)
    assert np.array_equal(_back(k, k0), wk) and np.array_equal(_back(v, v0), wv)
    k, v = _t(k0, dev), _t(v0, dev)
    st = mod.new_scrub_stats(dev)
    tt = torch.from_numpy(table).to(dev)
    _scrub(mod, k, v, tt[:0], torch.zeros(0, dtype=torch.int32, device=dev), codec, d, st)
    _scrub(mod, k, v, tt, torch.tensor([12, 8], dtype=torch.int32, device=dev), codec, d, st, first=1, count=0)
    _scrub(mod, k, v, tt, torch.tensor([0, -5], dtype=torch.int32, device=dev), codec, d, st)
    assert np.array_equal(_back(k, k0), k0) and np.array_equal(_back(v, v0), v0) and _totals(mod, st) == [0, 0, 0, 0]


# ---- validation --------------------------------------------------------------------------------

def test_python_validation(be, oracle):
    mod, dev = be
    codec, d = "hamming84", 32
    k0, v0 = _inputs(oracle, codec, d)
    k, v = _t(k0, dev), _t(v0, dev)
    tt = torch.from_numpy(_table()).to(dev)
    ll = torch.tensor(LENS, dtype=torch.int32, device=dev)
    ok = dict(head_dim=d, block_size=BS, num_layers=NL, codec=codec, layer_first=FIRST, layer_count=COUNT)

    def bad(k_=k, v_=v, t_=tt, l_=ll, **kw):
        with pytest.raises(ValueError):
            mod.cache_scrub_tensors(k_, v_, t_, l_, **{**ok, **kw})

    bad(codec="int4")                        # no ECC: nothing to scrub
    bad(codec="fp16")
    bad(layer_first=2, layer_count=2)        # layer_first + layer_count > num_layers
    bad(layer_first=-1)
    bad(k_=k.to(torch.int32))                # wrong cache dtype
    bad(codec="golay")                       # uint8 caches are not int32 Golay ones
    bad(head_dim=30)                         # rows do not match / not a multiple of 4
    bad(block_size=8)
    bad(num_layers=4)
    bad(k_=k.transpose(1, 2))                # not contiguous / wrong shape
    bad(t_=tt.to(torch.int64))
    bad(t_=tt.t())
    bad(l_=ll.to(torch.int64))
    bad(l_=ll[:1])                           # fewer length rows than layers
    bad(l_=ll[:, :3])                        # narrower than the batch
    bad(l_=ll[0, :3])
    other = torch.device("cpu") if dev.type == "cuda" else None
    if other is not None:
        bad(t_=tt.to(other))
        bad(l_=ll.to(other))
        bad(v_=v.to(other))
    # statistics buffers
    if dev.type == "cuda":
        good = mod.new_stats(dev)
        for st in (good[:100], good.to(torch.int32), good.view(32, 16)[:, :8], torch.zeros(512, dtype=torch.int64),
                   torch.zeros(2 * good.numel(), dtype=torch.int64, device=dev)[::2]):
            bad(stats=st)
    else:
        for st in (torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.int32),
                   torch.zeros(8, dtype=torch.int64)[::2]):
            bad(stats=st)
    with pytest.raises(ValueError):
        kvecc.cache_scrub(k, v, tt, ll, head_dim=d, block_size=BS, num_layers=NL, codec=codec, layers=[0, 2])
    assert np.array_equal(_back(k, k0), k0)  # nothing was touched


def test_abi_validation():
    """The C entries: codec none, bad codec, negative sizes, geometry and (twin) null pointers are
    KVECC_EINVAL with a message naming the function, before any work."""
    from kvecc import _lib
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 4096)()
    tab = (ctypes.c_int32 * 4)(0, 1, 2, 3)
    lens = (ctypes.c_int32 * 2)(4, 4)
    p = lambda x: ctypes.cast(x, ctypes.c_void_p)  # noqa: E731

    def call(name, k=buf, v=buf, t=tab, ln=lens, tstride=2, lstride=0, batch=2, hkv=2, d=4, nb=4, nl=2, first=0,
             count=2, bs=4, mcl=0, codec=_lib.CODEC_H84):
        last = None if name == "kvecc_cache_scrub" else 1
        return getattr(lib, name)(p(k) if k is not None else None, p(v) if v is not None else None,
                                  p(t) if t is not None else None, tstride, p(ln) if ln is not None else None,
                                  lstride, batch, hkv, d, nb, nl, first, count, bs, mcl, codec, None, last)

    for name in ("kvecc_cache_scrub", "kvecc_cpu_cache_scrub"):
        for kw in (dict(codec=_lib.CODEC_NONE), dict(codec=9), dict(codec=-1), dict(batch=-1), dict(hkv=-1), dict(d=-4),
                   dict(nb=-1), dict(nl=-1), dict(first=-1), dict(count=-1), dict(bs=-1), dict(tstride=-1),
                   dict(lstride=-1), dict(first=1, count=2), dict(d=6), dict(d=516), dict(tstride=0), dict(bs=0),
                   dict(k=None), dict(v=None), dict(t=None), dict(ln=None)):
            assert call(name, **kw) == -1, (name, kw)
            assert "cache_scrub" in lib.kvecc_last_error().decode(), (name, kw)
        assert call(name, batch=0, k=None) == 0 and call(name, count=0, k=None) == 0  # empty: nothing enqueued
    assert call("kvecc_cpu_cache_scrub") == 0  # zero codewords are clean


# ---- dispatcher ------------------------------------------------------------------------------

def _check_dispatcher(mod, dev, oracle):
    codec, d = "golay_packed", 7
    k0, v0 = _inputs(oracle, codec, d)
    tt, ll = torch.from_numpy(_table()).to(dev), torch.tensor(LENS, dtype=torch.int32, device=dev)
    want_k, want_v, got_k, got_v = _t(k0, dev), _t(v0, dev), _t(k0, dev), _t(v0, dev)
    ws, gs = mod.new_scrub_stats(dev), mod.new_scrub_stats(dev)
    _scrub(mod, want_k, want_v, tt, ll, codec, d, ws)
    args = lambda k, v, st: (k, v, tt, ll, d, BS, NL, codec, FIRST, COUNT, 0, st)  # noqa: E731
    assert torch.ops.kvecc.cache_scrub(*args(got_k, got_v, gs)) is None
    assert torch.equal(got_k, want_k) and torch.equal(got_v, want_v) and torch.equal(gs, ws)
    assert not torch.equal(got_k, _t(k0, dev))
    torch.library.opcheck(torch.ops.kvecc.cache_scrub.default, args(_t(k0, dev), _t(v0, dev), mod.new_scrub_stats(dev)))
    torch.library.opcheck(torch.ops.kvecc.cache_scrub.default, args(_t(k0, dev), _t(v0, dev), None))


def test_cpu_dispatcher_op(oracle):
    from kvecc import cpu_ops, torch_ops
    assert "cache_scrub" in torch_ops.OPS
    _check_dispatcher(cpu_ops, torch.device("cpu"), oracle)


@pytest.mark.gpu
def test_hip_dispatcher_op(gpu, oracle):
    from kvecc import ops
    _check_dispatcher(ops, gpu, oracle)


def test_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        k = torch.empty(NB, NL, HKV, BS * 32, dtype=torch.uint8)
        out = torch.ops.kvecc.cache_scrub(k, torch.empty_like(k), torch.empty(BATCH, NPER, dtype=torch.int32),
                                          torch.empty(BATCH, dtype=torch.int32), 32, BS, NL, "hamming84", 0, NL, 0,
                                          torch.empty(512, dtype=torch.int64))
        assert out is None


def test_backends_expose_the_scrub():
    import importlib
    from kvecc import backends
    assert "cache_scrub_tensors" in backends.NATIVE_FUNCTIONS
    for name in ("hip", "cpu"):
        assert hasattr(importlib.import_module(backends.CODEC_BACKENDS[name]), "cache_scrub_tensors")
    assert hasattr(kvecc.get_codec_backend("cpu"), "cache_scrub_tensors")
