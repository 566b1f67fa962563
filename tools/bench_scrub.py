"""In-place cache scrub (kvecc_cache_scrub): what a patrol pass over a resident cache costs.

Shape [8 sequences, ctx 4096, block 16, head_dim 128] with 32 and 8 cache heads, Hamming(8,4), Golay
int32 and packed Golay caches of encoded random INT4 values, 1 layer and 12 layers scrubbed in ONE
launch.  Three cases per configuration, in one process on the same cache:

  clean  a pass over a cache without errors: nothing is written.  Warm-up of >= --warmup calls (and
         >= --warmup-s seconds), then --passes passes of --iters calls bracketed by events; the
         median pass and the spread max - min are reported (the method of tools/bench_attention.py).
  dirty  the cache injected in place at BER 1e-3 (H84) / 1e-2 (Golay, 8 bits per byte for the packed
         layout), restored from a saved copy before EVERY timed launch and timed per launch with
         ops.time_next_launch, so the restore is not in the figure; --passes passes of --dirty-iters
         launches each.
  read   shim_read_batch over the same layers (one call per layer: it takes one), today's only other
         way to learn how many errors a resident cache holds; timed as `clean`.

Per case: microseconds and (cache bytes read + bytes written) / time / 8 TB/s.  `clean` writes
nothing; `dirty` writes the 16-byte vectors (12-byte groups for the packed layout) that hold a
rewritten word, counted from the bytes that differ after the pass; `read` reads the scales too and
writes 2 fp16 bytes per decoded value.  One JSON line per configuration.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "quantized-kv-cache-ecc-protection_amd"))

import torch  # noqa: E402

HBM_PEAK = 8e12  # bytes / s


def _fill(ops, cache, codec, d, gen):
    """Encoded random INT4 values into every row of a cache [blocks, layers, heads, bs * per]."""
    nb, nl, hkv, row = cache.shape
    g = (d + 2) // 3
    per = {"golay": g, "golay_packed": (3 * g + 3) // 4 * 4}.get(codec, d)
    bs = row // per
    for layer in range(nl):  # a layer at a time bounds the temporaries
        x = torch.randint(0, 16, (nb, hkv, bs, d), device=cache.device, generator=gen, dtype=torch.uint8)
        if codec == "hamming84":
            cache[:, layer] = ops.hamming84_encode(x.view(-1)).view(nb, hkv, row)
        else:
            cw = ops.golay_encode_rows(x)
            if codec == "golay":
                cache[:, layer] = cw.view(nb, hkv, row)
            else:
                b3 = torch.stack([(cw >> (8 * k)) & 0xFF for k in range(3)], -1).to(torch.uint8)
                cache[:, layer].view(nb, hkv, bs, per)[..., :3 * g] = b3.view(nb, hkv, bs, 3 * g)
        del x


def _written_bytes(before, after, codec, per):
    """Bytes of the store pieces (16-byte vectors; 12-byte groups of a packed row) that changed."""
    diff = (before.view(torch.uint8) != after.view(torch.uint8))
    if codec == "golay_packed":
        rows = diff.view(-1, per)
        n = 0
        for q in range(0, per, 12):
            piece = rows[:, q:q + 12]
            n += int(piece.any(1).sum()) * piece.shape[1]
        return n
    return int(diff.view(-1, 16).any(1).sum()) * 16


def run(args, codec, kv_heads, layers):
    from kvecc import ops
    from kvecc.memory_layout import kv_cache_pair
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    d, bs = args.d, args.bs
    nbl = (args.ctx + bs - 1) // bs
    blocks = args.batch * nbl
    g = (d + 2) // 3
    per = {"golay": g, "golay_packed": (3 * g + 3) // 4 * 4}.get(codec, d)
    dt = torch.int32 if codec == "golay" else torch.uint8
    kc, vc = kv_cache_pair((blocks, layers, kv_heads, bs * per), dt, dev)
    for c in (kc, vc):
        _fill(ops, c, codec, d, gen)
    table = torch.randperm(blocks, device=dev, generator=gen).to(torch.int32).view(args.batch, nbl)
    lens = torch.full((layers, args.batch), args.ctx, dtype=torch.int32, device=dev)
    stats = ops.new_stats(dev)
    cache_bytes = 2 * kc.numel() * kc.element_size()

    def scrub():
        ops.cache_scrub_tensors(kc, vc, table, lens, d, bs, layers, codec, 0, layers, args.ctx, stats)

    def timed(fn):
        t0 = time.perf_counter()
        while True:
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= args.warmup_s:
                break
        passes = []
        for _ in range(args.passes):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            passes.append(e0.elapsed_time(e1) * 1e3 / args.iters)
        return passes

    def entry(passes, nbytes):
        us = statistics.median(passes)
        return {"us": round(us, 2), "spread_us": round(max(passes) - min(passes), 2),
                "pass_us": [round(x, 2) for x in passes], "bytes": nbytes,
                "hbm_frac": round(nbytes / (us * 1e-6) / HBM_PEAK, 4)}

    res = {}
    # ---- (a) clean
    stats.zero_()
    scrub()
    first = ops.read_stats(stats, 4)
    assert first[2] == 0 and first[0] == 0, first
    res["clean"] = entry(timed(scrub), cache_bytes)
    # ---- (c) the counting read over the same cache
    ks = torch.rand(blocks, layers, kv_heads, bs, device=dev, generator=gen)
    vs = torch.rand_like(ks)
    out = (torch.empty((args.batch, kv_heads, args.ctx, d), dtype=torch.float16, device=dev),
           torch.empty((args.batch, kv_heads, args.ctx, d), dtype=torch.float16, device=dev))
    rstats = ops.new_stats(dev)

    def read():
        for layer in range(layers):
            ops.shim_read_batch(kc, vc, ks, vs, table, args.ctx, d, layer, codec, torch.float16, stats=rstats, out=out)

    values = 2 * layers * args.batch * args.ctx * kv_heads * d
    res["read"] = entry(timed(read), cache_bytes + 2 * ks.numel() * 4 + 2 * values)
    del out, ks, vs
    # ---- (b) dirty, restored before every timed launch
    ber = 1e-3 if codec == "hamming84" else 1e-2
    n_bits = {"hamming84": 8, "golay": 24, "golay_packed": 8}[codec]
    for i, c in enumerate((kc, vc)):
        f = c.view(-1)
        ops.inject_into(f, f, ber, n_bits, seed=7 + i)
    sk, sv = kc.clone(), vc.clone()
    stats.zero_()
    scrub()
    torch.cuda.synchronize()
    dirty = ops.read_stats(stats, 4)
    written = _written_bytes(sk, kc, codec, per) + _written_bytes(sv, vc, codec, per)
    start, stop = ops.kernel_timer(dev)
    passes = []
    for p in range(args.passes + 1):  # the first pass is the warm-up of this case
        tot = 0.0
        for _ in range(args.dirty_iters):
            kc.copy_(sk)
            vc.copy_(sv)
            ops.time_next_launch(start, stop)
            scrub()
            torch.cuda.synchronize()
            tot += start.elapsed_time(stop) * 1e3
        if p:
            passes.append(tot / args.dirty_iters)
    res["dirty"] = entry(passes, cache_bytes + written)
    res["dirty"].update(ber=ber, written_bytes=written,
                        stats=dict(zip(("corrected", "detected", "rewritten", "scanned"), dirty)))
    worse = max(res["clean"]["spread_us"], res["read"]["spread_us"])
    line = {"kernel": "cache_scrub", "codec": codec, "batch": args.batch, "ctx": args.ctx, "block_size": bs,
            "head_dim": d, "kv_heads": kv_heads, "layers": layers, **res,
            "clean_below_read_by_more_than_spread": res["read"]["us"] - res["clean"]["us"] > worse,
            "clean_vs_decode_kernels_0.77": round(res["clean"]["hbm_frac"] / 0.77, 3),
            "dirty_over_clean": round(res["dirty"]["us"] / res["clean"]["us"], 3)}
    print(json.dumps(line), flush=True)
    del kc, vc, sk, sv
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codecs", default="hamming84,golay,golay_packed")
    ap.add_argument("--kv-heads", default="32,8")
    ap.add_argument("--layers", default="1,12")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--ctx", type=int, default=4096)
    ap.add_argument("--bs", type=int, default=16)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--dirty-iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--warmup-s", type=float, default=0.5)
    ap.add_argument("--passes", type=int, default=5)
    args = ap.parse_args()
    for codec in args.codecs.split(","):
        for h in (int(x) for x in args.kv_heads.split(",")):
            for nl in (int(x) for x in args.layers.split(",")):
                run(args, codec, h, nl)


if __name__ == "__main__":
    main()
