"""The paged-cache kernels on caches around the 4 GiB addressing switch.

Every paged-cache kernel of csrc/attention.hip exists in two addressing forms,
chosen by attn_setup (`fits`: one cache's bytes and one scale array's bytes both
fit 32 bits): buffer descriptors with 32-bit offsets below the switch, 64-bit
pointers at and above it.  The rest of the suite runs caches of a few hundred
KiB, where no buffer offset has bit 31 set, and one decode shape over 4 GiB.

Nothing here is a new attention case.  `Placed` wraps a backend (ops on the
device, cpu_ops for the stand-in) so that every paged-cache argument of a call
-- the caches, their scale arrays, the block table -- is placed sparsely in four
shared big buffers before the call and taken out again after it: the small
case's blocks land at the ids `choose_ids` picks (block 0, the cache's last block,
the blocks around byte 2^31 and, over the switch, around byte 2^32, the rest
spread with a fixed seed, at least half of them above 2^31), everything else in
the big cache is zero, and the table is remapped through the same map.  The
existing checkers of tests/test_attention_*.py then run unchanged with that
backend, so the reference of every case stays the small case's own float64
restatement and the host twin over the compact cache; the big cache never
leaves the GPU.  After the call the placed blocks are copied back over the
small tensors the caller passed (a repairing call's writes are then visible to
its checker) and zeroed in the big buffers; the module's last test asserts that
all four buffers are zero again, which catches a write outside the placed blocks
and a forgotten restore.

Block counts, for a geometry of `block_bytes` per block and R scale rows per
block: N_u = min(0xFFFFFFFF // block_bytes, 0xFFFFFFFF // (4 R)), the largest
cache that still takes the buffer kernels ("under"); N_u + 1, the smallest that
does not ("switch"); N_u + 17, with blocks wholly past byte 2^32 ("over").

The buffers: two uint8 buffers of 2^32 + 2^26 bytes (K, V) and two float32
buffers of the same byte size (the head_dim 4 Hamming(8,4) rows are 4 bytes, so
its scale arrays are as large as its caches): about 17 GiB of HBM, allocated
once per module.
"""

import functools
import inspect
import random

import pytest
import torch

from tests import test_attention_bytes as tbytes
from tests import test_attention_chunk as tchunk
from tests import test_attention_chunk_ragged as tragged
from tests import test_attention_golay_stats as tgstats
from tests import test_attention_interp as tinterp
from tests import test_attention_paths as tpaths
from tests import test_attention_repair as trepair
from tests import test_attention_stats as tstats
from tests import test_attention_window as twindow
from tests import test_shim_append as tappend
from tests import test_shim_read_batch as tread
from tests.test_attention_paths import BF16, BF16_PATHS, F16, F32, PATHS, _TNAME, _select

TWO31, TWO32 = 1 << 31, 1 << 32
BUF_BYTES = TWO32 + (1 << 26)
OVER_EXTRA = 17
STAND_IN_BLOCKS = 64  # the host stand-in's block count


# ---- sizes and the id chooser ------------------------------------------------------------------
def fits(n, block_bytes, rows):
    """attn_setup's rule, restated: a cache of n blocks is buffer-addressable."""
    return n * block_bytes <= 0xFFFFFFFF and n * rows * 4 <= 0xFFFFFFFF


def n_under(block_bytes, rows):
    return min(0xFFFFFFFF // block_bytes, 0xFFFFFFFF // (4 * rows))


def block_count(which, block_bytes, rows):
    n = n_under(block_bytes, rows)
    return {"under": n, "switch": n + 1, "over": n + OVER_EXTRA}[which]


def marks(n, block_bytes):
    """The big ids that some small block must land on, besides 0 and n - 1: the block holding byte
    2^31 of the cache and the one before it; in a cache that reaches past byte 2^32, the block
    holding that byte and the next one, which lies wholly past it.  (Those that would collide with
    0 or n - 1 -- the stand-in, the exact switch -- are left out.)"""
    out = []
    b31 = TWO31 // block_bytes
    out += [b for b in (b31, b31 - 1) if 0 < b < n - 1]
    if n * block_bytes > TWO32:
        b32 = TWO32 // block_bytes
        out += [b for b in (b32, b32 + 1) if 0 < b < n - 1 and b not in out]
    return out


def choose_ids(small_n, used, n, block_bytes, seed=0):
    """An injective map small block id -> big block id, as a list.  `used`: the small ids the table
    names, in table order -- the marks go to those first, so that the call reads them."""
    assert 2 <= small_n <= n
    ids = {0: 0, small_n - 1: n - 1}
    order = [b for b in dict.fromkeys(used) if b not in ids and 0 <= b < small_n]
    order += [b for b in range(small_n) if b not in ids and b not in order]
    taken = {0, n - 1}
    for big in marks(n, block_bytes):
        if order:
            ids[order.pop(0)] = big
            taken.add(big)
    rng = random.Random(seed)
    b31 = min(TWO31 // block_bytes, n - 1)
    for i, small in enumerate(order):  # alternately above and below byte 2^31, above first
        lo, hi = (b31 + 1, n - 2) if i % 2 == 0 else (1, b31 - 2)
        if hi - lo < small_n:  # no room on that side (the stand-in): anywhere
            lo, hi = 1, n - 2
        big = rng.randint(lo, hi)
        while big in taken:
            big = rng.randint(lo, hi)
        ids[small] = big
        taken.add(big)
    return [ids[b] for b in range(small_n)]


# ---- the shared buffers and the placing backend ------------------------------------------------
class Buffers:
    def __init__(self, device, nbytes, count=block_count):
        self.k = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self.v = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self.ks = torch.zeros(nbytes // 4, dtype=torch.float32, device=device)
        self.vs = torch.zeros(nbytes // 4, dtype=torch.float32, device=device)
        self.count = count
        self.calls = 0

    def all(self):
        return (self.k, self.v, self.ks, self.vs)

    def nonzero(self):
        return [int(t.view(torch.int64).count_nonzero()) for t in self.all()]


class Placed:
    """A backend module whose paged-cache entries run over the big buffers (the module docstring).
    which: "under", "switch" or "over".  last: the (n, ids) of the latest call."""
    ENTRIES = ("paged_attention_into", "paged_attention_chunk_into", "paged_attention_window_into",
               "paged_attention_repair_into", "paged_attention_counted_into", "shim_append_tensors",
               "shim_append_ragged_tensors", "shim_read_batch", "cache_scrub_tensors")

    def __init__(self, mod, bufs, which):
        self.mod, self.bufs, self.which, self.last = mod, bufs, which, None
        self.__name__ = mod.__name__

    def __getattr__(self, name):
        fn = getattr(self.mod, name)
        if name not in self.ENTRIES:
            return fn
        return functools.partial(self._call, fn)

    def _call(self, fn, *args, **kw):
        bound = inspect.signature(fn).bind(*args, **kw)
        a = bound.arguments
        kc, vc, table = a["k_cache"], a["v_cache"], a["block_table"]
        ks, vs = a.get("k_scales"), a.get("v_scales")
        bs = int(a["block_size"]) if "block_size" in a else ks.shape[-1]
        small_n, layers, kvh, row = kc.shape
        block_bytes = layers * kvh * row * kc.element_size()
        rows = layers * kvh * bs
        n = self.bufs.count(self.which, block_bytes, rows)
        used = [int(b) for b in table.flatten().tolist() if b >= 0]
        ids = choose_ids(small_n, used, n, block_bytes, seed=small_n + row)
        self.last = (n, ids)
        idx = torch.tensor(ids, dtype=torch.int64, device=kc.device)
        pairs = [(self.bufs.k[:n * block_bytes].view(kc.dtype).view(n, layers, kvh, row), kc),
                 (self.bufs.v[:n * block_bytes].view(vc.dtype).view(n, layers, kvh, row), vc)]
        if ks is not None:
            pairs += [(self.bufs.ks[:n * rows].view(n, layers, kvh, bs), ks),
                      (self.bufs.vs[:n * rows].view(n, layers, kvh, bs), vs)]
        remap = torch.cat([idx, idx.new_full((1,), -1)]).to(torch.int32)  # -1 stays -1
        a["block_table"] = remap[table.long().clamp(min=-1)].view(table.shape).contiguous()
        try:
            for (big, small), name in zip(pairs, ("k_cache", "v_cache", "k_scales", "v_scales")):
                big[idx] = small
                a[name] = big
            self.bufs.calls += 1
            return fn(*bound.args, **bound.kwargs)
        finally:
            if kc.is_cuda:
                torch.cuda.synchronize()
            for big, small in pairs:
                small.copy_(big[idx])  # what a writing entry left in the placed blocks
                big[idx] = 0


# ---- CPU: the arithmetic -----------------------------------------------------------------------
def _geometry(codec, d, kvh, bs=16, layers=2):
    """-> (block_bytes, scale rows per block) of a cache in the layout `codec` is stored in."""
    g = (d + 2) // 3
    row = {"golay": 4 * g, "golay_packed": (3 * g + 3) // 4 * 4}.get(codec, d)
    return layers * kvh * bs * row, layers * kvh * bs


def _geometries():
    geo = {_geometry(p[0], p[2], p[4]) for p in PATHS + OVER_DECODE}
    geo |= {_geometry(p[0], p[2], p[4], 4) for p in BF16_PATHS}
    geo |= {_geometry(p[0], p[2], p[4]) for p in tchunk.CHUNK_PATHS + OVER_CHUNK + twindow.CASES}
    geo |= {_geometry(c, 32, 2, 8) for c in ("hamming84", "golay", "golay_packed")}  # the shim's LLaMA, the writers
    geo |= {_geometry(c, 64, 2, 16) for c in ("hamming84", "golay", "golay_packed")}  # the dense read
    return sorted(geo)


def test_block_counts_sit_on_the_switch():
    for block_bytes, rows in _geometries():
        n = n_under(block_bytes, rows)
        assert fits(n, block_bytes, rows) and not fits(n + 1, block_bytes, rows)
        assert block_count("under", block_bytes, rows) == n and block_count("switch", block_bytes, rows) == n + 1
        n_o = block_count("over", block_bytes, rows)
        assert (n_o - 1) * block_bytes >= TWO32  # the last block lies wholly past byte 2^32
        assert n_o * block_bytes <= BUF_BYTES and n_o * rows * 4 <= BUF_BYTES  # the views fit the buffers
        assert n_o * rows <= 0x7FFFFFFF  # attn_setup: cache rows fit int32
    # the head_dim 4 Hamming(8,4) rows: the scale arrays are as large as the caches
    block_bytes, rows = _geometry("hamming84", 4, 2)
    assert block_bytes == 4 * rows and block_count("over", block_bytes, rows) * rows * 4 > TWO32


def test_id_chooser():
    for block_bytes, rows in _geometries():
        for which in ("under", "switch", "over"):
            n = block_count(which, block_bytes, rows)
            for small_n, used in ((13, [5, 7, 1, 12, 0, 9, 3]), (16, list(range(15, 0, -1))), (29, [4, 2, 27, 11, 28])):
                ids = choose_ids(small_n, used, n, block_bytes, seed=small_n)
                assert len(set(ids)) == small_n and all(0 <= b < n for b in ids)
                assert ids[0] == 0 and ids[-1] == n - 1
                first = [b for b in used if b not in (0, small_n - 1)]
                # the first blocks the table names straddle byte 2^31 and sit before it
                a, b = ids[first[0]], ids[first[1]]
                assert a * block_bytes <= TWO31 < (a + 1) * block_bytes and b == a - 1
                if which == "over":  # one block holds byte 2^32, one lies wholly past it (and so does the last)
                    c, e = ids[first[2]], ids[first[3]] if len(first) > 3 else n - 1
                    assert c * block_bytes <= TWO32 < (c + 1) * block_bytes
                    assert e * block_bytes >= TWO32 and (n - 1) * block_bytes >= TWO32
                elif which == "switch":  # the last block ends on or straddles byte 2^32
                    assert (n - 1) * block_bytes < TWO32 <= n * block_bytes or n * rows * 4 > 0xFFFFFFFF
                rest = [ids[s] for s in range(1, small_n - 1) if ids[s] not in marks(n, block_bytes)]
                assert all(1 <= b <= n - 2 for b in rest)
                assert 2 * sum(b > TWO31 // block_bytes for b in rest) >= len(rest)  # at least half above 2^31
                assert ids == choose_ids(small_n, used, n, block_bytes, seed=small_n)  # a fixed seed
    assert marks(STAND_IN_BLOCKS, 8192) == []


# ---- CPU: the placement through the host twin, on a 64-block stand-in ---------------------------
@pytest.fixture(scope="module")
def stand_in():
    return Buffers("cpu", STAND_IN_BLOCKS * 32768, count=lambda which, block_bytes, rows: STAND_IN_BLOCKS)


def _twin(stand_in):
    from kvecc import cpu_ops
    return cpu_ops, Placed(cpu_ops, stand_in, "under")


def test_placement_decode_is_the_compact_call(stand_in):
    mod, placed = _twin(stand_in)
    for path in (PATHS[2], PATHS[16], PATHS[63], PATHS[100]):
        c = tpaths._bundle(*path[:5], 16)
        args = (path[0], c["q"], c["kc"], c["vc"], c["table"], c["lens"], c["ks"], c["vs"], tpaths.LAYER, 16)
        assert torch.equal(tpaths._attend(placed, None, *args), tpaths._attend(mod, None, *args))
        n, ids = placed.last
        assert n == STAND_IN_BLOCKS and ids[0] == 0 and ids[-1] == n - 1 and sorted(ids) != list(range(len(ids)))
    assert stand_in.nonzero() == [0, 0, 0, 0]


def test_placement_chunk_ragged_window_bytes_are_the_compact_calls(stand_in):
    mod, placed = _twin(stand_in)
    for path in (tchunk.CHUNK_PATHS[4], tchunk.GENERAL_PATHS[1], tchunk.GENERAL_PATHS[2]):
        c = tchunk._bundle(*path, 5)
        args = (path[0], c["q"], c["kc"], c["vc"], c["table"], c["lens"], c["ks"], c["vs"], c["layer"], c["bs"])
        assert torch.equal(tchunk._attend_chunk(placed, None, *args)[1], tchunk._attend_chunk(mod, None, *args)[1])
        c = tragged._case(*path, 5)
        assert torch.equal(tragged._run(placed, None, path[0], c, c["spans"]).nan_to_num(),
                           tragged._run(mod, None, path[0], c, c["spans"]).nan_to_num())
    for family in (twindow.CASES[0], twindow.CASES[5]):
        c = twindow._wcase(family, 17)
        assert torch.equal(twindow._run(placed, None, c, 24, 4), twindow._run(mod, None, c, 24, 4))
    for codec in tbytes.CODECS:
        c = tbytes._decode_bundle(codec, F32, 64, 8, 2, 16)
        args = (codec, c["q"], c["kc"], c["vc"], c["table"], c["lens"], c["ks"], c["vs"], tpaths.LAYER, 16)
        assert torch.equal(tpaths._attend(placed, None, *args), tpaths._attend(mod, None, *args))
    assert stand_in.nonzero() == [0, 0, 0, 0] and stand_in.calls >= 10


def test_placement_of_a_writer_is_the_compact_write(stand_in):
    """shim_append_tensors through the placing backend leaves in the small tensors what the twin
    writes into the compact cache, and nothing in the stand-in."""
    mod, placed = _twin(stand_in)
    kvh, d, bs, layers, nb = 2, 32, 8, 2, 9
    g = torch.Generator().manual_seed(3)
    k, v = torch.randn(2, 2, 11, kvh * d, generator=g)
    table = torch.tensor([[3, 8, 0, -1], [5, 1, 7, -1]], dtype=torch.int32)
    start = torch.tensor([5, 9], dtype=torch.int32)
    got = []
    for m in (mod, placed):
        kc = torch.zeros(nb, layers, kvh, bs * d, dtype=torch.uint8)
        t = [kc, torch.zeros_like(kc), torch.zeros(nb, layers, kvh, bs), torch.zeros(nb, layers, kvh, bs)]
        m.shim_append_tensors(k, v, *t, table, start, layers, bs, kvh, d, 1, "hamming84", 8, True, 1e-2, 77)
        got.append(t)
    assert all(torch.equal(a, b) for a, b in zip(*got)) and bool(got[1][0].any()) and bool(got[1][2].any())
    assert stand_in.nonzero() == [0, 0, 0, 0]


# ---- the launcher over the switch, restated -----------------------------------------------------
# Decode entry, at "over": one entry per unbuffered instantiation (codec, query dtype, VEC, W).
# Hamming(8,4): VEC 1 at W 1..64 (head_dim 4, 8, 12, 20, 52, 100, 252) and VEC 4 at W 1..16 (16, 32,
# 64, 128, 256); Golay, both forms: W 1..32 (7, 12, 20, 64, 100, 256), head_dim 100 with its
# clamped last lane (34 codewords, 34 % 3 != 0).  Groups of 1, 4, 3 and 2 query heads per cache
# head in turn: over the switch every one of them runs one head per workgroup.
_H84_D = (4, 8, 12, 20, 52, 100, 252, 16, 32, 64, 128, 256)
_GOLAY_D = (7, 12, 20, 64, 100, 256)
_GROUPS = (1, 4, 3, 2)


def _over_decode():
    out = []
    for dtype in (F32, F16, BF16):
        for codec, dims in (("hamming84", _H84_D), ("golay", _GOLAY_D), ("golay_packed", _GOLAY_D)):
            for d in dims:
                heads = 2 * _GROUPS[len(out) % 4]
                out.append((codec, dtype, d, heads, 2, 4, _select(codec, dtype, d, heads, 2, buf=False)[0]))
    return out


OVER_DECODE = _over_decode()
# Chunk and ragged entries over the switch: the general paths, and shapes that take the matrix
# cores below the switch and must not above it
OVER_CHUNK = tchunk.GENERAL_PATHS + [(c, F16, 128, 8, 2) for c in ("hamming84", "golay", "golay_packed")]
OVER_WINDOW = [("hamming84", F16, 128, 8, 2), ("golay", F16, 128, 4, 2), ("golay_packed", BF16, 20, 2, 2),
               ("hamming74", F16, 128, 8, 2), ("int4", F32, 64, 8, 2)]
WS = [(twindow.BS, 3), (24, 4), (100, 40)]
SWITCH = [("hamming84", F32, 64, 8, 2), ("golay", F16, 100, 6, 2), ("golay_packed", BF16, 20, 2, 2)]


def _unbuffered_sweep():
    found = set()
    for codec in ("hamming84", "golay", "golay_packed"):
        for dtype in (F32, F16, BF16):
            for d in range(1, 257):
                if codec == "hamming84" and d % 4:
                    continue
                for group in (1, 2, 3, 4, 8, 16):
                    found.add(_select(codec, dtype, d, 2 * group, 2, buf=False)[0])
    return found


def test_over_table_reaches_every_unbuffered_instantiation():
    names = [p[6] for p in OVER_DECODE]
    assert len(set(names)) == len(names) == 3 * (12 + 6 + 6)
    assert set(names) == _unbuffered_sweep()
    for name in names:  # one head per workgroup, no buffer addressing, never the matrix cores
        assert "split_kernel" in name and ", false, 1, 0, 0>" in name
    assert "paged_attn_split_kernel<float, 2, 4, 16, false, 1, 0, 0>" in names  # head_dim 256
    assert "paged_attn_split_kernel<__half, 2, 1, 64, false, 1, 0, 0>" in names  # head_dim 252
    assert "paged_attn_split_kernel<__hip_bfloat16, 4, 3, 32, false, 1, 0, 0>" in names
    shapes = {(p[0], p[2]) for p in OVER_DECODE}
    assert {("golay", 100), ("golay_packed", 100), ("hamming84", 4), ("hamming84", 256)} <= shapes
    assert {p[3] // p[4] for p in OVER_DECODE} == {1, 2, 3, 4} and {p[1] for p in OVER_DECODE} == {F32, F16, BF16}
    # the shapes the matrix cores and the GQA kernels take below the switch lose them above it
    for p in OVER_CHUNK[3:]:
        assert "mfma" in tchunk._chunk_select(*p)[0]
        name, g, _ = tchunk._chunk_select(*p, buf=False)
        assert "split_kernel" in name and ", false, 1," in name and g == 1
    assert _select("hamming84", F32, 128, 8, 2)[1] == 4 and _select("hamming84", F32, 128, 8, 2, buf=False)[1] == 1
    # the chunk entry's unbuffered instantiations are the decode entry's: OVER_CHUNK names a subset
    assert {tchunk._chunk_select(*p, buf=False)[0] for p in OVER_CHUNK} <= set(names)
    # the default is the buffer-addressed choice, as before
    assert all(_select(*p[:5])[0] == _select(*p[:5], buf=True)[0] == p[6] for p in PATHS)


def _traced_name(name, kernel, args):
    """A restated decode-entry name as the kernel trace spells the same instantiation of `kernel`."""
    body = name[len("paged_attn_split_kernel<"):].replace(", 0, 0>", ">")
    if "byte" in kernel:  # the byte family has no codec parameter
        t, _, rest = body.partition(", ")
        body = t + ", " + rest.partition(", ")[2]
    return f"void kvecc::{kernel}<{body}(kvecc::{args})"


def test_restated_unbuffered_names_are_in_the_kernel_trace():
    """profiles/large_cache/kernels.txt is the kernel trace of this file's gpu tests (every kvecc
    kernel they launched, by name): every unbuffered instantiation the sweep lists ran, and so did
    the unbuffered chunk, window and byte kernels of the over-size cases."""
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "large_cache",
                        "kernels.txt")
    traced = {ln.strip() for ln in open(path) if ln.strip()}
    want = {f"void kvecc::{n}(kvecc::AttnArgs)" for n in _unbuffered_sweep()}
    assert len(want) == 72
    for p in OVER_CHUNK:
        want.add(_traced_name(_select(*p, buf=False)[0], "paged_attn_split_chunk_kernel", "RaggedArgs"))
    for codec, dtype, d, heads, kvh in OVER_WINDOW:
        base = codec if codec in tpaths._CODEC else "hamming84"
        want.add(_traced_name(_select(base, dtype, d, heads, kvh, buf=False)[0], "paged_attn_split_window_kernel",
                              "WindowArgs"))
    for p in BYTE_DECODE:
        want.add(_traced_name(_select(*p[:5], buf=False)[0], "paged_attn_split_byte_kernel", "ByteAttnArgs"))
    want.add(_traced_name(_select(*BYTE_CHUNK, buf=False)[0], "paged_attn_split_byte_chunk_kernel", "ByteChunkArgs"))
    assert want <= traced, sorted(want - traced)
    # and nothing unbuffered ran that is not one head per workgroup
    assert all(", false, 1" in t for t in traced if "paged_attn_split" in t and "false" in t)
    # under the switch the file reaches the matrix-core kernels of every entry and the repairing kernels
    for kernel in ("h84_mfma_kernel", "golay_mfma_kernel", "h84_mfma_chunk_kernel", "h84_mfma_ragged_kernel",
                   "h84_mfma_window_kernel", "h84_mfma_interp_kernel", "h84_mfma_stats_kernel",
                   "h84_mfma_stats_interp_kernel", "h84_mfma_repair_kernel", "h84_mfma_repair_interp_kernel",
                   "golay_mfma_stats_kernel", "split_repair_kernel", "split_interp_kernel", "split_stats_kernel",
                   "split_golay_stats_kernel", "byte_mfma_kernel", "shim_append_kernel", "shim_append_ragged_kernel",
                   "cache_scrub_kernel"):
        assert any(f"paged_attn_{kernel}<" in t or f"::{kernel}<" in t for t in traced), kernel


# ---- GPU ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(gpu):
    bufs = Buffers(gpu, BUF_BYTES)
    yield bufs
    del bufs.k, bufs.v, bufs.ks, bufs.vs
    torch.cuda.empty_cache()


def _ops(big, which):
    from kvecc import ops
    return Placed(ops, big, which)


def _did(p):
    return f"{p[0]}-{_TNAME[p[1]].strip('_')}-d{p[2]}-{p[3]}q{p[4]}kv"


# -- 2. under the switch: every buffer-addressed kernel at offsets above 2^31
@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS, ids=_did)
def test_under_decode(gpu, big, path):
    mod = _ops(big, "under")
    tpaths._check_bundle(mod, gpu, path, 16)
    n, ids = mod.last
    block_bytes, rows = _geometry(path[0], path[2], path[4])
    assert n == n_under(block_bytes, rows) and fits(n, block_bytes, rows)
    assert sum((b + 1) * block_bytes > TWO31 for b in ids) >= len(ids) // 2  # blocks that reach past byte 2^31


@pytest.mark.gpu
@pytest.mark.parametrize("path", BF16_PATHS, ids=_did)
def test_under_decode_last_block_only(gpu, big, path):
    tpaths._check_bundle(_ops(big, "under"), gpu, path, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("q_len", [5, 17])
@pytest.mark.parametrize("path", tchunk.CHUNK_PATHS, ids=_did)
def test_under_chunk(gpu, big, path, q_len):
    tchunk._check_bundle(_ops(big, "under"), gpu, path, q_len)


@pytest.mark.gpu
@pytest.mark.parametrize("path", tchunk.CHUNK_PATHS, ids=_did)
def test_under_ragged(gpu, big, path):
    tragged._check_spans(_ops(big, "under"), gpu, path, 5)


def _check_window(mod, dev, family, q_len=17):
    from kvecc import cpu_ops
    c, dtype, base = twindow._wcase(family, q_len), family[1], twindow._ref_base(family[0])
    for w, s in WS:
        ref = twindow._restated(family, q_len, w, s)
        got = twindow._run(mod, dev, c, w, s)
        twindow._check(got, ref, dtype, f"W {w} S {s}")
        twindow._check_empty_rows(got, ref, base, (w, s))
        twin = twindow._run(cpu_ops, None, c, w, s).double()
        assert tpaths._close(got.double(), twin, dtype), (w, s, tpaths._err(got.double(), twin))


@pytest.mark.gpu
@pytest.mark.parametrize("family", twindow.CASES, ids=_did)
def test_under_window(gpu, big, family):
    _check_window(_ops(big, "under"), gpu, family)


BYTE_DECODE = tbytes.H84_PATHS  # tests/test_attention_bytes.py's decode bundle: every Hamming(8,4) shape
BYTE_CHUNK = ("hamming84",) + tbytes.MFMA_SHAPE


@pytest.mark.gpu
@pytest.mark.parametrize("path", BYTE_DECODE, ids=_did)
@pytest.mark.parametrize("codec", tbytes.CODECS)
def test_under_bytes_decode(gpu, big, codec, path):
    tbytes._check_decode_bundle(_ops(big, "under"), gpu, codec, path, 16)


@pytest.mark.gpu
@pytest.mark.parametrize("codec", tbytes.CODECS)
def test_under_bytes_chunk(gpu, big, codec):
    tbytes._check_chunk_bundle(_ops(big, "under"), gpu, codec, BYTE_CHUNK, 17)


# the interpolating, counted, counted + interpolating, Golay-counted and repairing kernels: one matrix-core
# and one general path each, on those files' planted-error cases
ECC_PATHS = [tinterp.MFMA_PATHS[1], tinterp.GENERAL_PATHS[0]]  # fp16 d64 8q/2kv, fp32 d100 6q/2kv
GOLAY_ECC_PATHS = [p for p in tgstats.GOLAY_PATHS if (p[1], p[2], p[3]) in ((F16, 128, 8), (F32, 20, 2))]


def test_ecc_paths_are_what_they_say():
    assert [tchunk._chunk_select("hamming84", *p[:4])[0] for p in ECC_PATHS] == [
        "paged_attn_h84_mfma_chunk_kernel<64>", "paged_attn_split_kernel<float, 2, 1, 32, true, 1, 0, 0>"]
    names = [tchunk._chunk_select(*p[:5])[0] for p in GOLAY_ECC_PATHS]
    assert len(names) == 4 and sum("mfma" in n for n in names) == 2 and {p[0] for p in GOLAY_ECC_PATHS} == {
        "golay", "golay_packed"}


@pytest.mark.gpu
@pytest.mark.parametrize("path", ECC_PATHS, ids=tinterp._pid)
def test_under_interp(gpu, big, path):
    tinterp._check_planted(_ops(big, "under"), gpu, path, 17)


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [0, 1], ids=["plain", "interp"])
@pytest.mark.parametrize("path", ECC_PATHS, ids=tinterp._pid)
def test_under_counted(gpu, big, path, interp):
    """Output under TOL, the counts those of the twin's counting read, exactly."""
    tstats._check_counts_and_outputs(_ops(big, "under"), gpu, path, 17, interp, False)


@pytest.mark.gpu
@pytest.mark.parametrize("path", GOLAY_ECC_PATHS, ids=_did)
def test_under_golay_counted(gpu, big, path):
    tgstats._check_counts_and_outputs(_ops(big, "under"), gpu, path, 17)


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [0, 1], ids=["plain", "interp"])
@pytest.mark.parametrize("path", ECC_PATHS, ids=tinterp._pid)
def test_under_repair(gpu, big, path, interp):
    """The counted entry's output and counts, and the placed blocks after the call are the
    twin's scrubbed compact cache bit for bit: the repairing stores at offsets above 2^31."""
    trepair._check_main(_ops(big, "under"), gpu, path, 17, interp, False)


# -- 3. over the switch: every BUF = false instantiation
@pytest.mark.gpu
@pytest.mark.parametrize("path", OVER_DECODE, ids=_did)
def test_over_decode(gpu, big, path):
    mod = _ops(big, "over")
    tpaths._check_bundle(mod, gpu, path, 16)
    n, ids = mod.last
    block_bytes, rows = _geometry(path[0], path[2], path[4])
    assert n == n_under(block_bytes, rows) + OVER_EXTRA and not fits(n, block_bytes, rows)
    assert sum(b * block_bytes >= TWO32 for b in ids) >= 2 and ids[-1] == n - 1


@pytest.mark.gpu
@pytest.mark.parametrize("q_len", [5, 17])
@pytest.mark.parametrize("path", OVER_CHUNK, ids=_did)
def test_over_chunk(gpu, big, path, q_len):
    tchunk._check_bundle(_ops(big, "over"), gpu, path, q_len)


@pytest.mark.gpu
@pytest.mark.parametrize("path", OVER_CHUNK, ids=_did)
def test_over_ragged(gpu, big, path):
    tragged._check_spans(_ops(big, "over"), gpu, path, 5)


@pytest.mark.gpu
def test_over_chunk_strided_query(gpu, big):
    """The [B, H, T, D] tensor transposed, on a shape that takes the matrix cores below the switch."""
    path = OVER_CHUNK[3]
    c = dict(tchunk._bundle(*path, 5))
    c["q"] = c["q"].transpose(1, 2).contiguous().transpose(1, 2)
    assert not c["q"].is_contiguous()
    tchunk._check_both(_ops(big, "over"), gpu, path[0], path[1], c)


@pytest.mark.gpu
@pytest.mark.parametrize("family", OVER_WINDOW, ids=_did)
def test_over_window(gpu, big, family):
    _check_window(_ops(big, "over"), gpu, family)


@pytest.mark.gpu
@pytest.mark.parametrize("path", BYTE_DECODE, ids=_did)
@pytest.mark.parametrize("codec", tbytes.CODECS)
def test_over_bytes_decode(gpu, big, codec, path):
    tbytes._check_decode_bundle(_ops(big, "over"), gpu, codec, path, 16)


@pytest.mark.gpu
@pytest.mark.parametrize("codec", tbytes.CODECS)
def test_over_bytes_chunk(gpu, big, codec):
    tbytes._check_chunk_bundle(_ops(big, "over"), gpu, codec, BYTE_CHUNK, 17)


# -- the exact switch: the smallest cache that is not buffer-addressable, five codecs
@pytest.mark.gpu
@pytest.mark.parametrize("path", SWITCH, ids=_did)
def test_switch_decode_and_chunk(gpu, big, path):
    mod = _ops(big, "switch")
    tpaths._check_bundle(mod, gpu, path + (4, None), 16)
    n, _ = mod.last
    block_bytes, rows = _geometry(path[0], path[2], path[4])
    assert fits(n - 1, block_bytes, rows) and not fits(n, block_bytes, rows)
    tchunk._check_bundle(mod, gpu, path, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("codec", tbytes.CODECS)
def test_switch_bytes_decode_and_chunk(gpu, big, codec):
    mod = _ops(big, "switch")
    tbytes._check_decode_bundle(mod, gpu, codec, ("hamming84", F32, 64, 8, 2, 4, None), 16)
    tbytes._check_chunk_bundle(mod, gpu, codec, BYTE_CHUNK, 5)


# -- 5. the refusals: the interpolating, counted and repairing entries have no 64-bit kernels
REFUSED = {
    "interp": ("hamming84", dict(interp=True)),
    "stats": ("hamming84", dict(stats=True)),
    "stats-interp": ("hamming84", dict(stats=True, interp=True)),
    "repair": ("hamming84", dict(stats=True, repair=True)),
    "golay-counted": ("golay", dict(stats=True)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(REFUSED))
def test_over_refusals(gpu, big, mode):
    """Each raises KveccError naming the 4 GiB limit and launches nothing: `out` keeps its sentinel,
    the statistics buffer stays zero and the placed blocks come back as they went in."""
    import math
    from kvecc import ops
    from kvecc._lib import KveccError
    codec, kw = REFUSED[mode]
    kw = dict(kw)
    path = (codec, F16, 128, 8, 2)
    c = tchunk._bundle(*path, 5)
    mod = _ops(big, "over")
    stats = ops.new_stats(gpu) if kw.pop("stats", False) else None
    dev = [c[k].to(gpu) for k in ("kc", "vc", "table", "lens", "ks", "vs")]
    out = torch.full(c["q"].shape, 77.0, dtype=F16, device=gpu)
    args = (c["q"].to(gpu), dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], out, c["layer"], c["bs"],
            1 / math.sqrt(128), codec)
    with pytest.raises(KveccError, match="4 GiB"):
        if codec == "golay":
            mod.paged_attention_counted_into(*args, stats)
        else:
            mod.paged_attention_chunk_into(*args, stats=stats, **kw)
    torch.cuda.synchronize()
    assert bool((out == 77.0).all())
    assert stats is None or not bool(stats.any())
    for name, t in zip(("kc", "vc", "table", "lens", "ks", "vs"), dev):
        assert torch.equal(t.cpu(), c[name]), name
    n, ids = mod.last
    assert not fits(n, *_geometry(codec, 128, 2))


# -- 4. the writers and the dense read on the same caches
W_LAYERS, W_KVH, W_BS, W_D, W_NB = 2, 2, 8, 32, 6
# logical blocks -> small ids.  Sequence 0's span starts in small block 2 and ends in small block 5, the
# cache's last: in the big cache from the block before the one holding byte 2^31 into block N - 1.
# Sequence 1's crosses from small block 3 into 4: over the switch, from the block holding byte 2^32
# into the one after it.  (choose_ids gives the marks to the table's ids in order: 1, 2, 3, 4.)
W_TABLE = [[1, 2, 5], [3, 4, -1]]
W_START, W_QLEN = [W_BS + 5, 3], 7
W_SPANS = [(1, 6), (0, 7)]
APPEND_CODECS = ["int4", "hamming74", "hamming84", "golay", "golay_packed"]
SCRUB_CODECS = ["hamming74", "hamming84", "golay", "golay_packed"]


def _w_caches(codec, device):
    per = tappend._row_words(codec, W_D)
    dt = torch.int32 if codec == "golay" else torch.uint8
    return [torch.zeros(W_NB, W_LAYERS, W_KVH, W_BS * per, dtype=dt, device=device) for _ in range(2)] + [
        torch.zeros(W_NB, W_LAYERS, W_KVH, W_BS, device=device) for _ in range(2)]


def _w_append(mod, dev, codec, ragged, caches=None):
    """One injected append into layer 1 -> the four cache tensors on the host."""
    g = torch.Generator().manual_seed(7)
    k, v = torch.randn(2, 2, W_QLEN, W_KVH, W_D, generator=g).half()
    caches = _w_caches(codec, dev) if caches is None else caches
    table = torch.tensor(W_TABLE, dtype=torch.int32, device=dev)
    start = torch.tensor(W_START, dtype=torch.int32, device=dev)
    args = (k.to(dev), v.to(dev), *caches, table, start, W_LAYERS, W_BS, W_KVH, W_D, 1, codec,
            tappend.N_BITS[codec], True, 5e-2, 1234)
    if ragged:
        rows = torch.tensor([(f, c, b) for (f, c), b in zip(W_SPANS, (0, W_SPANS[0][1]))], dtype=torch.int32)
        mod.shim_append_ragged_tensors(*args, rows.to(dev), scale_rule="mul_inv7")
    else:
        mod.shim_append_tensors(*args, scale_rule="mul_inv7")
    return [c.cpu() for c in caches]


def _check_append(mod, dev, codec, ragged):
    from kvecc import cpu_ops
    want = _w_append(cpu_ops, "cpu", codec, ragged)
    got = _w_append(mod, dev, codec, ragged)
    for g, w, name in zip(got, want, ("k_cache", "v_cache", "k_scales", "v_scales")):
        assert torch.equal(g, w), name
    assert all(bool(w[b, 1].any()) for w in want for b in (2, 3, 4, 5)) and not bool(want[0][:, 0].any())


def _check_w_ids(mod, which, codec):
    n, ids = mod.last
    block_bytes = W_LAYERS * W_KVH * W_BS * tappend._row_words(codec, W_D) * (4 if codec == "golay" else 1)
    assert ids[5] == n - 1 and (ids[2] + 1) * block_bytes <= TWO31 < (ids[1] + 1) * block_bytes
    if which == "over":
        assert ids[3] * block_bytes <= TWO32 < ids[4] * block_bytes and not fits(n, block_bytes, W_LAYERS * W_KVH * W_BS)


def test_writers_through_the_stand_in(stand_in):
    mod, placed = _twin(stand_in)
    for codec in APPEND_CODECS:
        for ragged in (False, True):
            _check_append(placed, "cpu", codec, ragged)
    for codec in SCRUB_CODECS:
        _check_scrub(placed, "cpu", codec)
        _check_read(placed, "cpu", codec, False)
    _check_read(placed, "cpu", "hamming84", True)
    assert stand_in.nonzero() == [0, 0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["under", "over"])
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("codec", APPEND_CODECS)
def test_append(gpu, big, codec, ragged, which):
    """The placed blocks and scale rows are, bit for bit, what the twin writes into the compact cache
    (the module's last test: and nothing else was written)."""
    mod = _ops(big, which)
    _check_append(mod, gpu, codec, ragged)
    _check_w_ids(mod, which, codec)


def _planted_cache(codec):
    """A clean two-layer cache written by the twin's append, then singles, doubles and (Golay) 3- and
    4-bit errors planted in layer 1 of every block, the last word of the last row included."""
    from kvecc import cpu_ops
    kc, vc, _, _ = _w_append(cpu_ops, "cpu", codec, False)
    g = torch.Generator().manual_seed(5)
    full = torch.randn(2, 1, W_NB * W_BS, W_KVH, W_D, generator=g).half()
    caches = _w_caches(codec, "cpu")
    table = torch.arange(W_NB, dtype=torch.int32).view(1, W_NB)
    for layer in range(W_LAYERS):
        cpu_ops.shim_append_tensors(full[0], full[1], *caches, table, torch.zeros(1, dtype=torch.int32), W_LAYERS,
                                    W_BS, W_KVH, W_D, layer, codec, tappend.N_BITS[codec], False, 0.0, 1)
    kc, vc = caches[0], caches[1]
    golay = codec in ("golay", "golay_packed")
    flips = [0x01, 0x03] + ([0x07, 0x0F] if golay else [])  # 1, 2, 3, 4 bits of one byte of a codeword
    for cache in (kc, vc):
        rows = cache.view(W_NB, W_LAYERS, W_KVH, W_BS, -1)
        per = rows.shape[-1]
        last = per - 1 if codec != "golay_packed" else 3 * ((W_D + 2) // 3) - 3  # the last codeword's first byte
        for blk in range(W_NB):
            for i, f in enumerate(flips):
                slot, word = (blk + 3 * i) % W_BS, (5 * blk + 7 * i) % (last + 1)
                if codec == "golay_packed":
                    word -= word % 3
                rows[blk, 1, i % W_KVH, slot, word] ^= f
        rows[-1, -1, -1, -1, last] ^= 0x01  # the buffer's last word: a single, which the scrub rewrites
        rows[-1, -1, -1, -2, last] ^= flips[-1]  # and the largest error planted in the row before it
    return kc, vc


def _check_scrub(mod, dev, codec):
    from kvecc import cpu_ops
    kc, vc = _planted_cache(codec)
    table = torch.tensor([[1, 2, 5], [3, 4, 0]], dtype=torch.int32)
    lens = torch.tensor([3 * W_BS, 3 * W_BS - 3], dtype=torch.int32)
    out = []
    for m, d_ in ((cpu_ops, "cpu"), (mod, dev)):
        k, v = kc.clone().to(d_), vc.clone().to(d_)
        st = m.new_scrub_stats(d_)
        m.cache_scrub_tensors(k, v, table.to(d_), lens.to(d_), W_D, W_BS, W_LAYERS, codec, layer_first=1,
                              layer_count=1, stats=st)
        out.append((k.cpu(), v.cpu(), [int(x) for x in m.stats_totals(st, 4).tolist()]))
    (wk, wv, want), (gk, gv, got) = out
    print(f"{codec}: scrub counts {got}, twin {want}")
    assert want[0] > 0 and want[2] > 0 and (codec == "hamming74" or want[1] > 0) and not torch.equal(wk, kc)
    assert torch.equal(gk, wk) and torch.equal(gv, wv) and got == want
    last_row = lambda c: c.view(W_NB, W_LAYERS, W_KVH, W_BS, -1)[-1, -1, -1, -1]  # noqa: E731
    assert int((last_row(wk) != last_row(kc)).sum()) == 1  # the buffer's last codeword was rewritten


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["under", "over"])
@pytest.mark.parametrize("codec", SCRUB_CODECS)
def test_scrub(gpu, big, codec, which):
    _check_scrub(_ops(big, which), gpu, codec)


def _check_read(mod, dev, codec, interp):
    from kvecc import cpu_ops
    kc, vc, ks, vs, table = tread.make_cache(codec, 2, 37, 2, 64, 16, seed=101)
    st, gst = cpu_ops.new_stats(), mod.new_stats(dev)
    ek, ev = cpu_ops.shim_read_batch(kc, vc, ks, vs, table, 37, 64, 1, codec, torch.float16, stats=st, interp=interp)
    t = lambda x: x.to(dev)  # noqa: E731
    k, v = mod.shim_read_batch(t(kc), t(vc), t(ks), t(vs), t(table), 37, 64, 1, codec, torch.float16, stats=gst,
                               interp=interp)
    assert torch.equal(k.cpu(), ek) and torch.equal(v.cpu(), ev)
    assert mod.read_stats(gst) == cpu_ops.read_stats(st) and sum(cpu_ops.read_stats(st)) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["under", "over"])
@pytest.mark.parametrize("codec,interp", [(c, False) for c in SCRUB_CODECS] + [("hamming84", True)])
def test_read_batch(gpu, big, codec, interp, which):
    _check_read(_ops(big, which), gpu, codec, interp)


# -- 5. the shim over a manager cache past the switch: the size predicate and the fall-back
SHIM_STEPS, SHIM_BLOCKS = 12, 8  # 20 + 12 tokens of two sequences at block_size 8
FALLBACKS = {
    "stats": ("hamming84", dict(stats_attention=True), {}),
    "counted-h84": ("hamming84", dict(counted_attention=True), {}),
    "counted-golay": ("golay", dict(counted_attention=True), {}),
    "interp": ("hamming84", dict(interp_attention=True, use_interpolation=True), dict(use_interpolation=True)),
    "repair": ("hamming84", dict(repair_attention=True), {}),
}
KEYS = ("errors_corrected", "errors_detected", "injection_count")


def test_size_predicate_thresholds():
    from kvecc.ecc_shim import SimpleBlockManager
    f = SimpleBlockManager.fits_buffer_kernels
    for codec, storage, d, kvh, bs, layers in (("hamming84", "int32", 32, 2, 8, 2), ("golay", "int32", 32, 2, 8, 2),
                                               ("golay", "packed", 100, 2, 16, 2), ("hamming74", "int32", 128, 8, 16, 4),
                                               ("int4", "int32", 4, 2, 16, 2), ("golay", "packed", 1, 1, 16, 1)):
        block_bytes, rows = _geometry("golay_packed" if storage == "packed" else codec, d, kvh, bs, layers)
        n = n_under(block_bytes, rows)
        assert f(n, layers, kvh, bs, d, codec, storage) and not f(n + 1, layers, kvh, bs, d, codec, storage)
        assert fits(n, block_bytes, rows) and not fits(n + 1, block_bytes, rows)
    # head_dim 4: the cache and the scale array reach 4 GiB together; one byte per row more and the cache is first
    assert f((1 << 32) // 256 - 1, 2, 2, 16, 4) and not f((1 << 32) // 256, 2, 2, 16, 4)
    mgr = SimpleBlockManager(4, 8, 2, 2, 32, device="cpu")
    assert mgr.buffer_addressable is True


def _shim_cfg(codec, backend, **kw):
    from tests.test_shim_window import _cfg
    return _cfg(codec, backend, **kw)


def _shim_run(model, cfg, dev, num_blocks, ragged, prepare=None):
    """tests/test_shim_window.py's schedule at 12 steps -> (the valid logits per sequence, the
    statistics after every forward); prepare(manager) runs before the first forward."""
    from kvecc.ecc_shim import get_ecc_stats, patch_model_with_ecc_attention, reset_ecc_cache, set_ecc_query_spans
    from tests.test_shim_window import PROMPT, SHORT, _tokens
    ids, nxt = _tokens(SHIM_STEPS)
    lens = [PROMPT, SHORT if ragged else PROMPT]
    outs, stats = [[], []], []
    with torch.no_grad(), patch_model_with_ecc_attention(model, cfg, num_blocks=num_blocks):
        reset_ecc_cache(model)
        if prepare is not None:
            prepare(model._ecc_block_manager)
        if ragged:
            set_ecc_query_spans(model, lens)
        pos = torch.arange(PROMPT).unsqueeze(0).expand(2, -1)
        logits = model(ids.to(dev), position_ids=pos.to(dev)).logits.float().cpu()
        for b in range(2):
            outs[b].append(logits[b, :lens[b]])
        stats.append({k: get_ecc_stats(model)[k] for k in KEYS})
        if ragged:
            set_ecc_query_spans(model, [1, 1])
        for s_ in range(SHIM_STEPS):
            p_ = torch.tensor(lens).view(2, 1)
            logits = model(nxt[:, s_:s_ + 1].to(dev), position_ids=p_.to(dev)).logits.float().cpu()
            for b in range(2):
                outs[b].append(logits[b])
                lens[b] += 1
            stats.append({k: get_ecc_stats(model)[k] for k in KEYS})
    return [torch.cat(o) for o in outs], stats


@functools.lru_cache(maxsize=None)
def _shim_ref(codec, ragged, kw):
    """The same model over a 32-block cache on the cpu backend."""
    from tests.test_shim_llama import _llama
    return _shim_run(_llama()[0], _shim_cfg(codec, "cpu", **dict(kw)), torch.device("cpu"), 32, ragged)


def test_forced_fall_back_is_decode_stats_bit_for_bit(monkeypatch):
    """With the size predicate false on a small manager, a stats_attention model takes the read +
    SDPA path on every forward: the logits and the counts of decode_stats=True, bit for bit."""
    from kvecc import cpu_ops, ecc_shim
    from tests.test_shim_llama import _llama
    want, want_st = _shim_ref("hamming84", True, (("decode_stats", True),))
    assert want_st[0]["errors_corrected"] > 0 and want_st[-1]["errors_detected"] > 0
    calls = []
    real = cpu_ops.paged_attention_chunk_into
    monkeypatch.setattr(cpu_ops, "paged_attention_chunk_into", lambda *a, **k: calls.append(1) or real(*a, **k))
    model = _llama()[0]
    on, st_on = _shim_run(model, _shim_cfg("hamming84", "cpu", stats_attention=True), torch.device("cpu"), 32, True)
    assert len(calls) == 2 * (1 + SHIM_STEPS) and st_on == want_st  # the counted kernels, the same counts
    calls.clear()

    def forced(mgr):
        assert mgr.buffer_addressable is False

    monkeypatch.setattr(ecc_shim.SimpleBlockManager, "fits_buffer_kernels", staticmethod(lambda *a, **k: False))
    for flags in (dict(stats_attention=True), dict(repair_attention=True), dict(counted_attention=True)):
        got, st = _shim_run(model, _shim_cfg("hamming84", "cpu", **flags), torch.device("cpu"), 32, True,
                            prepare=forced)
        assert calls == [] and st == want_st
        assert all(torch.equal(g, w) for g, w in zip(got, want))


def _big_shim_run(monkeypatch, gpu, big, codec, ragged, **kw):
    """The LLaMA over a manager whose caches are views of the big buffers, num_blocks the smallest
    count that is not buffer-addressable, the free list the ids of choose_ids."""
    from kvecc import ecc_shim
    from tests.test_shim_llama import _llama
    store = codec.replace("_packed", "")
    block_bytes, rows = _geometry(codec, 32, 2, 8, 2)
    n = block_count("switch", block_bytes, rows)
    ids = sorted(choose_ids(SHIM_BLOCKS, range(SHIM_BLOCKS), n, block_bytes, seed=3))
    views = []

    real_pair = ecc_shim.kv_cache_pair

    def pair(shape, dtype, device):
        nbytes = n * block_bytes
        if tuple(shape)[0] != n:  # (some other manager: a reference run's)
            return real_pair(shape, dtype, device)
        assert not bool(big.k[:nbytes].view(torch.int64).any())
        views.extend(b[:nbytes].view(dtype).view(tuple(shape)) for b in (big.k, big.v))
        return views[0], views[1]

    def prepare(mgr):
        assert mgr.buffer_addressable is False and mgr.num_blocks == n and mgr.k_cache is views[0]
        assert not ecc_shim.SimpleBlockManager.fits_buffer_kernels(n, 2, 2, 8, 32, store, "int32")
        assert ecc_shim.SimpleBlockManager.fits_buffer_kernels(n - 1, 2, 2, 8, 32, store, "int32")
        mgr.free_blocks = list(ids)

    try:
        big.calls += 1
        with monkeypatch.context() as mp:
            mp.setattr(ecc_shim, "kv_cache_pair", pair)
            return _shim_run(_llama()[0].to(gpu), _shim_cfg(codec, "hip", **kw), gpu, n, ragged, prepare=prepare), ids
    finally:
        torch.cuda.synchronize()
        idx = torch.tensor(ids, device=gpu)
        for v in views:
            v[idx] = 0


def _close_logits(got, want):
    from tests.test_shim_llama import LOGIT_ATOL
    for b in range(2):
        err = float((got[b] - want[b]).abs().max())
        print(f"sequence {b}: max logit err {err:.3e}")
        assert bool(got[b].isfinite().all()) and err <= LOGIT_ATOL, (b, err)


def test_shim_ids_straddle_the_marks():
    for codec in ("hamming84", "golay"):
        block_bytes, rows = _geometry(codec, 32, 2, 8, 2)
        n = block_count("switch", block_bytes, rows)
        ids = sorted(choose_ids(SHIM_BLOCKS, range(SHIM_BLOCKS), n, block_bytes, seed=3))
        b31 = TWO31 // block_bytes
        assert ids[0] == 0 and ids[-1] == n - 1 and {b31 - 1, b31} <= set(ids) and n * block_bytes >= TWO32


@pytest.mark.gpu
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("codec,kw", [("hamming84", dict(chunk_attention=True)), ("golay", dict(chunk_attention=True)),
                                      ("hamming84", dict(window=24, sinks=4))], ids=["h84", "golay", "window"])
def test_shim_kernel_path_over_the_switch(gpu, big, monkeypatch, codec, kw, ragged):
    """The plain and the windowed kernel path have 64-bit kernels: the run is on them and meets the
    same model over a 32-block cache on the cpu backend."""
    (got, _), ids = _big_shim_run(monkeypatch, gpu, big, codec, ragged, **kw)
    _close_logits(got, _shim_ref(codec, ragged, tuple(sorted(kw.items())))[0])


@pytest.mark.gpu
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("mode", sorted(FALLBACKS))
def test_shim_falls_back_over_the_switch(gpu, big, monkeypatch, mode, ragged):
    """The interpolating, counted and repairing routes have no 64-bit kernels: over a manager cache
    of 4 GiB or more the shim takes the read + SDPA path, as it does above head_dim 256 -- the run
    finishes, and its logits and decode statistics are those of decode_stats=True over a small cache.
    (Before the size predicate these raised KveccError on the first forward.)"""
    codec, kw, ref_kw = FALLBACKS[mode]
    (got, stats), ids = _big_shim_run(monkeypatch, gpu, big, codec, ragged, **kw)
    want, want_stats = _shim_ref(codec, ragged, tuple(sorted(dict(ref_kw, decode_stats=True).items())))
    _close_logits(got, want)
    assert stats == want_stats and stats[-1]["errors_corrected"] > 0


# -- the module's last test: nothing was written outside the placed blocks, every placement was undone
@pytest.mark.gpu
def test_the_buffers_are_zero_again(gpu, big):
    assert big.calls > 0
    assert big.nonzero() == [0, 0, 0, 0]
