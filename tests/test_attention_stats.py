"""kvecc_paged_attention_stats: paged attention over a Hamming(8,4) cache that adds the
SINGLE_CORRECTED / DOUBLE_DETECTED classification of every stored byte it attends over to a
statistics buffer, exactly once (include/kvecc.h "Counted attention").

Counts: per sequence with a valid query token, what cpu_ops.shim_read_batch(table[b:b+1],
ctx = n_b, stats=...) adds for K and V, summed and compared EXACTLY.  Outputs: the existing
float64 expectations at the suite's TOL of the query dtype -- test_attention_interp's _expect
for interp 1, the chunk tests' _ref_chunk (per sequence, on its valid tokens) for interp 0.
Every case runs on the host twin and, marked gpu, on the device.  The bundles, queries and
paths are test_attention_interp's.
"""

import ctypes
import functools
import math

import pytest
import torch

from tests.test_attention_chunk import _ref_chunk
from tests.test_attention_interp import (BS, CODEC, EMPTY, GENERAL_PATHS, LAYER, LAYERS, MFMA_PATHS, PATHS, Q_LENS,
                                         RAGGED, _bundle, _check, _expect, _lens, _mods, _pid, _query, _random_rows,
                                         _types, _valid)
from tests.test_attention_paths import _close, _err

assert PATHS == MFMA_PATHS + GENERAL_PATHS and Q_LENS == [1, 2, 5, 16, 17]
DOUBLE = 0x03  # codeword 0 with two flipped bits: a type-2 byte


# ---- expectations -------------------------------------------------------------------------------
def _nb(c, b, mcl=0):
    cap = c["table"].shape[1] * BS if mcl <= 0 else min(mcl, c["table"].shape[1] * BS)
    return min(max(int(c["lens"][b]), 0), cap)


def _seq_counts(c, b, mcl=0):
    """[corrected, detected] that the counting host read adds for sequence b alone, K and V."""
    from kvecc import cpu_ops
    nb = _nb(c, b, mcl)
    if nb == 0:
        return [0, 0]
    st = cpu_ops.new_stats()
    d = c["kc"].shape[3] // BS
    cpu_ops.shim_read_batch(c["kc"], c["vc"], c["ks"], c["vs"], c["table"][b:b + 1].contiguous(), nb, d, LAYER, CODEC,
                            torch.float32, stats=st)
    return cpu_ops.read_stats(st)


def _expected_counts(c, spans=None, mcl=0):
    tot = [0, 0]
    for b in range(c["table"].shape[0]):
        if spans is not None and (spans[b][1] <= 0 or spans[b][0] < 0):
            continue  # no valid token: the sequence is not read
        n = _seq_counts(c, b, mcl)
        tot = [tot[0] + n[0], tot[1] + n[1]]
    return tot


def _expect_plain(q, c, spans=None, mcl=0):
    """float64 [B, T, H, d]: _ref_chunk per sequence on its valid tokens, the empty value elsewhere."""
    ref = torch.full(q.shape, EMPTY, dtype=torch.float64)
    for b in range(q.shape[0]):
        f, n = (0, q.shape[1]) if spans is None else spans[b]
        if n > 0:
            ref[b, f:f + n] = _ref_chunk(torch.nan_to_num(q[b:b + 1, f:f + n]), c["kc"], c["vc"], c["table"][b:b + 1],
                                         c["lens"][b:b + 1], c["ks"], c["vs"], LAYER, BS, CODEC, mcl)[0]
    return ref


def _ref(q, c, interp, spans=None, mcl=0):
    return _expect(q, c, spans, mcl) if interp else _expect_plain(q, c, spans, mcl)


def _run(mod, dev, q, c, interp, spans=None, mcl=0, stats=None):
    """paged_attention_chunk_into(stats=...) on q as given -> (raw output on the host, [corrected, detected])."""
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    if dev is not None:
        off = (q.data_ptr() % 16) // q.element_size()
        qd = torch.empty(off + q.numel() + 16, dtype=q.dtype, device=dev)
        skew = (-qd.data_ptr() % 16) // q.element_size()
        qd = qd[skew + off:skew + off + q.numel()].view(q.shape)
        qd.copy_(q)
    else:
        qd = q
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
    mod.paged_attention_chunk_into(qd, t(c["kc"]), t(c["vc"]), t(c["table"]), t(c["lens"]), t(c["ks"]), t(c["vs"]),
                                   out, LAYER, BS, 1 / math.sqrt(q.shape[-1]), CODEC, max_context_len=mcl,
                                   q_spans=sp, interp=bool(interp), stats=stats)
    return out.cpu(), mod.read_stats(stats)


# ---- 1. exact counts, outputs within tolerance -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(path, q_len, random_cache):
    dtype, d, heads, kvh, off = path
    c = _bundle(d, kvh, _lens(q_len), random_cache=random_cache)
    q = _query(4, q_len, heads, d, dtype, off, q_len)
    return c, q, _expected_counts(c)


@functools.lru_cache(maxsize=None)
def _case_ref(path, q_len, random_cache, interp):
    c, q, _ = _case(path, q_len, random_cache)
    return _ref(q, c, interp)


def _check_counts_and_outputs(mod, dev, path, q_len, interp, random_cache):
    c, q, want = _case(path, q_len, random_cache)
    assert want[0] > 0 and want[1] > 0, want  # both kinds of byte are there to count
    got, counts = _run(mod, dev, q, c, interp)
    print(f"counts {counts} expected {want}")
    assert counts == want
    _check(got, _case_ref(path, q_len, random_cache, interp), path[0], f"interp {interp}")


@pytest.mark.parametrize("random_cache", [False, True], ids=["planted", "random"])
@pytest.mark.parametrize("interp", [0, 1], ids=["plain", "interp"])
@pytest.mark.parametrize("q_len", Q_LENS)
@pytest.mark.parametrize("path", PATHS, ids=_pid)
def test_cpu_counts_and_outputs(path, q_len, interp, random_cache):
    _check_counts_and_outputs(*_mods(None), path, q_len, interp, random_cache)


@pytest.mark.gpu
@pytest.mark.parametrize("random_cache", [False, True], ids=["planted", "random"])
@pytest.mark.parametrize("interp", [0, 1], ids=["plain", "interp"])
@pytest.mark.parametrize("q_len", Q_LENS)
@pytest.mark.parametrize("path", PATHS, ids=_pid)
def test_hip_counts_and_outputs(gpu, path, q_len, interp, random_cache):
    _check_counts_and_outputs(*_mods(gpu), path, q_len, interp, random_cache)


# ---- 2. every byte value ----------------------------------------------------------------------------
def _every_byte_case(path):
    """One sequence of 32 tokens whose K and V rows are _random_rows: every run of 256 bytes a permutation."""
    dtype, d, heads, kvh, off = path
    n, nblk = 32, 2
    g = torch.Generator().manual_seed(d)
    kc = _random_rows((nblk + 1) * LAYERS * kvh * BS * d, 3 * d).view(nblk + 1, LAYERS, kvh, BS * d).clone()
    vc = _random_rows((nblk + 1) * LAYERS * kvh * BS * d, 5 * d).view(nblk + 1, LAYERS, kvh, BS * d).clone()
    ks = torch.rand(nblk + 1, LAYERS, kvh, BS, generator=g) * 0.3 + 0.05
    vs = torch.rand(nblk + 1, LAYERS, kvh, BS, generator=g) * 0.3 + 0.05
    table = torch.tensor([[2, 0]], dtype=torch.int32)
    c = dict(kc=kc, vc=vc, ks=ks, vs=vs, table=table, lens=torch.tensor([n], dtype=torch.int32))
    read = torch.cat([x.view(nblk + 1, LAYERS, kvh, BS, d)[[2, 0], LAYER].reshape(-1) for x in (kc, vc)])
    ty = _types(read)
    return c, _query(1, 3, heads, d, dtype, off, 2), [int((ty == 1).sum()), int((ty == 2).sum())], read


def _check_every_byte(mod, dev, path, interp):
    c, q, want, read = _every_byte_case(path)
    assert len(torch.unique(read)) == 256 and min(want) > 0
    got, counts = _run(mod, dev, q, c, interp)
    assert counts == want, (counts, want)
    _check(got, _ref(q, c, interp), path[0], "every byte")


@pytest.mark.parametrize("interp", [0, 1], ids=["plain", "interp"])
@pytest.mark.parametrize("path", PATHS, ids=_pid)
def test_cpu_every_byte_value(path, interp):
    _check_every_byte(*_mods(None), path, interp)


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [0, 1], ids=["plain", "interp"])
@pytest.mark.parametrize("path", PATHS, ids=_pid)
def test_hip_every_byte_value(gpu, path, interp):
    _check_every_byte(*_mods(gpu), path, interp)


# ---- 3. what must not be counted --------------------------------------------------------------------
def _polluted(c):
    """The bundle with type-2 bytes wherever no count may come from: the rows at or past each
    sequence's length in its last block, the other layer, the blocks no table row names (the
    slots a -1 entry could stand for among them)."""
    kvh, d = c["kc"].shape[2], c["kc"].shape[3] // BS
    out = dict(c)
    named = set(int(x) for x in c["table"].flatten() if int(x) >= 0)
    for key in ("kc", "vc"):
        x = c[key].clone()
        v = x.view(-1, LAYERS, kvh, BS, d)
        v[:, 1 - LAYER] = DOUBLE
        for blk in range(v.shape[0]):
            if blk not in named:
                v[blk] = DOUBLE
        for b in range(c["table"].shape[0]):
            n = int(c["lens"][b])
            if n % BS and int(c["table"][b, n // BS]) >= 0:
                v[int(c["table"][b, n // BS]), LAYER, :, n % BS:] = DOUBLE
        out[key] = x
    return out


def _check_not_counted(mod, dev, path, q_len, interp):
    assert int(_types(torch.tensor([DOUBLE], dtype=torch.uint8))[0]) == 2
    c, q, want = _case(path, q_len, False)
    assert int(c["table"][0, 3]) == -1  # a -1 block inside sequence 0
    p = _polluted(c)
    assert int((p["kc"] != c["kc"]).sum()) > 1000
    got, counts = _run(mod, dev, q, p, interp)
    assert counts == want, (counts, want)
    _check(got, _case_ref(path, q_len, False, interp), path[0], "polluted")
    # max_context_len below the longest sequence: only the bytes below it
    mcl = int(c["lens"].max()) - 7
    want_cut = _expected_counts(c, mcl=mcl)
    assert want_cut[0] < want[0] or want_cut[1] < want[1]
    got, counts = _run(mod, dev, q, p, interp, mcl=mcl)
    assert counts == want_cut, (counts, want_cut)
    _check(got, _ref(q, c, interp, mcl=mcl), path[0], f"mcl {mcl}")


@pytest.mark.parametrize("interp", [0, 1], ids=["plain", "interp"])
@pytest.mark.parametrize("q_len", [1, 17])
@pytest.mark.parametrize("path", PATHS, ids=_pid)
def test_cpu_uncounted_regions(path, q_len, interp):
    _check_not_counted(*_mods(None), path, q_len, interp)


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [0, 1], ids=["plain", "interp"])
@pytest.mark.parametrize("q_len", [1, 17])
@pytest.mark.parametrize("path", PATHS, ids=_pid)
def test_hip_uncounted_regions(gpu, path, q_len, interp):
    _check_not_counted(*_mods(gpu), path, q_len, interp)


# ---- 4. ragged calls --------------------------------------------------------------------------------
def _check_ragged(mod, dev, path, case, interp):
    dtype, d, heads, kvh, off = path
    q_max, spans, extra = case
    lens = tuple(n + e for (_, n), e in zip(spans, extra))
    c = _bundle(d, kvh, lens)
    valid = _valid(spans, q_max)
    q = _query(4, q_max, heads, d, dtype, off, q_max, nan_where=~valid)  # padding query elements are NaN
    want = _expected_counts(c, spans)
    idle = [b for b, (_, n) in enumerate(spans) if n == 0 and lens[b] > 0]
    assert idle and all(sum(_seq_counts(c, b)) > 0 for b in idle)  # an inactive sequence whose cache holds errors
    got, counts = _run(mod, dev, q, c, interp, spans)
    assert counts == want, (counts, want)
    assert bool((got[~valid].double() == EMPTY).all())
    _check(got, _ref(q, c, interp, spans), dtype, f"ragged q_max {q_max}")


@pytest.mark.parametrize("interp", [0, 1], ids=["plain", "interp"])
@pytest.mark.parametrize("case", RAGGED, ids=lambda c: f"qmax{c[0]}")
@pytest.mark.parametrize("path", PATHS, ids=_pid)
def test_cpu_ragged(path, case, interp):
    _check_ragged(*_mods(None), path, case, interp)


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [0, 1], ids=["plain", "interp"])
@pytest.mark.parametrize("case", RAGGED, ids=lambda c: f"qmax{c[0]}")
@pytest.mark.parametrize("path", PATHS, ids=_pid)
def test_hip_ragged(gpu, path, case, interp):
    _check_ragged(*_mods(gpu), path, case, interp)


def _check_overrunning_span(mod, dev, path, interp):
    """A span that overruns q_max is clamped: its last valid token sees fewer than n_b keys, and
    the sequence's n_b rows are still counted once."""
    dtype, d, heads, kvh, off = path
    c = _bundle(d, kvh, (40, 9, 33, 0))
    spans = ((3, 4), (0, 5), (1, 2), (0, 0))  # sequence 0: first 3 + count 4 > q_max 5
    q = _query(4, 5, heads, d, dtype, off, 5)
    want = _expected_counts(c, spans)
    got, counts = _run(mod, dev, q, c, interp, spans)
    assert counts == want, (counts, want)
    assert not bool(got.double().isnan().any())


@pytest.mark.parametrize("interp", [0, 1], ids=["plain", "interp"])
@pytest.mark.parametrize("path", [MFMA_PATHS[1], GENERAL_PATHS[0]], ids=_pid)
def test_cpu_overrunning_span(path, interp):
    _check_overrunning_span(*_mods(None), path, interp)


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [0, 1], ids=["plain", "interp"])
@pytest.mark.parametrize("path", [MFMA_PATHS[1], GENERAL_PATHS[0]], ids=_pid)
def test_hip_overrunning_span(gpu, path, interp):
    _check_overrunning_span(*_mods(gpu), path, interp)


# ---- 5. accumulation --------------------------------------------------------------------------------
def _check_accumulation(mod, dev, path):
    dtype, d, heads, kvh, off = path
    c, q, want = _case(path, 5, False)
    st = mod.new_stats(dev)
    _, once = _run(mod, dev, q, c, 0, stats=st)
    _, twice = _run(mod, dev, q, c, 0, stats=st)
    assert once == want and twice == [2 * want[0], 2 * want[1]]
    _, third = _run(mod, dev, q, c, 1, stats=st)  # the same cache through the interpolating kernels
    assert third == [3 * want[0], 3 * want[1]]
    clean = dict(c)
    clean["kc"], clean["vc"] = torch.zeros_like(c["kc"]), torch.zeros_like(c["vc"])  # codeword 0 everywhere
    for interp in (0, 1):
        assert _run(mod, dev, q, clean, interp)[1] == [0, 0]


@pytest.mark.parametrize("path", [MFMA_PATHS[1], GENERAL_PATHS[1]], ids=_pid)
def test_cpu_accumulation(path):
    _check_accumulation(*_mods(None), path)


@pytest.mark.gpu
@pytest.mark.parametrize("path", [MFMA_PATHS[1], GENERAL_PATHS[1]], ids=_pid)
def test_hip_accumulation(gpu, path):
    _check_accumulation(*_mods(gpu), path)


# ---- 6. the device against the host twin --------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("interp", [0, 1], ids=["plain", "interp"])
@pytest.mark.parametrize("path", PATHS, ids=_pid)
def test_hip_equals_host_twin(gpu, path, interp):
    from kvecc import cpu_ops, ops
    c, q, _ = _case(path, 17, True)
    host, host_counts = _run(cpu_ops, None, q, c, interp)
    dev, dev_counts = _run(ops, gpu, q, c, interp)
    assert dev_counts == host_counts
    print(f"max |device - host| {_err(dev.double(), host.double()):.3e}")
    assert _close(dev.double(), host.double(), path[0])


# ---- 7. validation, the dispatcher operator -----------------------------------------------------------
def test_c_entries_need_stats_and_hamming84():
    """Validation precedes any device work: both entries, no GPU needed."""
    from kvecc import _lib
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.float32)
    stats = torch.zeros(512, dtype=torch.int64)
    p, sp = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(stats.data_ptr())
    for name, tail in (("kvecc_paged_attention_stats", [p, 64, None]), ("kvecc_cpu_paged_attention_stats", [1])):
        fn = getattr(lib, name)

        def call(codec, st, interp=0):
            return fn(p, 64, 32, 8, _lib.F16, p, p, p, p, None, p, p, p, 1, 2, 4, 4, 8, 4, LAYERS, LAYER, BS, 2, 0,
                      0.1, codec, interp, st, *tail)
        for interp in (0, 1):
            assert call(_lib.CODEC_H84, None, interp) == -1, name  # KVECC_EINVAL
            assert "stats" in lib.kvecc_last_error().decode()
            for codec in (_lib.CODEC_GOLAY, 4, 1, 0):  # Golay (int32, packed), Hamming(7,4), raw
                assert call(codec, sp, interp) == -1, (name, codec)
                assert "hamming84" in lib.kvecc_last_error().decode()
    assert not bool(buf.any()) and not bool(stats.any())


def _check_errors(mod, dev):
    from tests.test_attention_paths import _caches, _for_codec
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    c, q, _ = _case(MFMA_PATHS[2], 5, False)
    args = [t(c[k]) for k in ("kc", "vc", "table", "lens", "ks", "vs")]
    out = torch.full(q.shape, 77.0, dtype=q.dtype, device=dev)
    good = mod.new_stats(dev)
    n = good.numel()
    bad = [torch.zeros(n, dtype=torch.int32, device=dev),  # dtype
           torch.zeros(n - 1, dtype=torch.int64, device=dev),  # length
           torch.zeros(n, dtype=torch.int64, device="meta" if dev is None else "cpu")]  # device
    for st in bad:
        with pytest.raises(ValueError, match="stats must be"):
            mod.paged_attention_chunk_into(t(q), *args, out, LAYER, BS, 0.1, CODEC, stats=st)
    assert not any(bool(st.any()) for st in bad if st.device.type != "meta")
    kc, vc, ks, vs = _caches("golay", 32, 1, BS, int(c["kc"].shape[0]), LAYERS, 0.0, 1, False)
    for codec in ("golay", "golay_packed", "hamming74", "int4"):
        pk, pv = _for_codec(codec, 32, kc, vc) if codec.startswith("golay") else (c["kc"], c["vc"])
        for interp in (False, True):
            with pytest.raises(ValueError, match="hamming84"):
                mod.paged_attention_chunk_into(t(q), t(pk), t(pv), t(c["table"]), t(c["lens"]), t(ks), t(vs), out,
                                               LAYER, BS, 0.1, codec, interp=interp, stats=good)
    assert bool((out == 77.0).all()) and mod.read_stats(good) == [0, 0]


def test_cpu_argument_errors():
    _check_errors(*_mods(None))


@pytest.mark.gpu
def test_hip_argument_errors(gpu):
    _check_errors(*_mods(gpu))


def _op_args(dev, spans, stats, interp):
    c, q, _ = _case(MFMA_PATHS[2], 5, False)
    t = (lambda x: x.to(dev)) if dev is not None else (lambda x: x)
    return (t(q.contiguous()), t(c["kc"]), t(c["vc"]), t(c["table"]), t(c["lens"]), spans, t(c["ks"]), t(c["vs"]),
            stats, LAYER, BS, 1 / math.sqrt(32), CODEC, interp)


def _check_dispatcher(mod, dev):
    import kvecc
    from kvecc import torch_ops
    assert "paged_attention_stats" in torch_ops.OPS
    c, q, want = _case(MFMA_PATHS[2], 5, False)
    spans = torch.tensor([[1, 4, 0], [0, 5, 4], [2, 2, 9], [0, 0, 11]], dtype=torch.int32, device=dev)
    for sp in (None, spans):
        for interp in (False, True):
            st = mod.new_stats(dev)
            a = _op_args(dev, sp, st, interp)
            got = torch.ops.kvecc.paged_attention_stats(*a)
            assert mod.read_stats(st) == want  # sequence 3 holds no token either way
            st2 = mod.new_stats(dev)
            pub = kvecc.paged_attention_chunk(a[0], a[1], a[2], a[3], a[4], a[6], a[7], LAYER, BS, q_spans=sp,
                                              interp=interp, stats=st2)
            assert torch.equal(pub, got) and mod.read_stats(st2) == want
            torch.library.opcheck(torch.ops.kvecc.paged_attention_stats.default, a)


def test_cpu_dispatcher_op():
    _check_dispatcher(*_mods(None))


@pytest.mark.gpu
def test_hip_dispatcher_op(gpu):
    _check_dispatcher(*_mods(gpu))


def test_dispatcher_op_traces_under_compile():
    from kvecc import cpu_ops
    c, q, want = _case(MFMA_PATHS[2], 5, False)
    fn = torch.compile(lambda *x: torch.ops.kvecc.paged_attention_stats(*x) * 2, fullgraph=True, backend="eager")
    st, st2 = cpu_ops.new_stats(), cpu_ops.new_stats()
    assert torch.equal(fn(*_op_args(None, None, st, True)),
                       torch.ops.kvecc.paged_attention_stats(*_op_args(None, None, st2, True)) * 2)
    assert cpu_ops.read_stats(st) == want == cpu_ops.read_stats(st2)
