"""INT4 paged attention: the product's table form against the table-free fork.

The product decodes an unprotected INT4 byte through the byte family's 256-entry LDS table
(entry b = b & 15); tools/exp/attn_int4_tf.hip (libattn_int4tf.so: make -C tools/exp
libattn_int4tf.so) masks the nibble in registers instead.  Both run through the library's own
entries -- kvecc_paged_attention and kvecc_paged_attention_chunk with KVECC_CODEC_NONE -- so the
launch geometry is the same.  fp16, [8 seq, ctx 4096, block 16, d 128], 32 and 8 cache heads, a
decode step and a 16-token chunk; the two forms, and the product's Hamming(8,4) kernel over the
same nibbles encoded, alternate inside every pass of one process, after a warm-up of each.  All
three outputs must be bit-equal (the same arithmetic on the same nibbles).
One JSON line per case.

usage: python tools/exp/run_int4_table_free.py [--iters N] [--passes N]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, os.path.join(REPO, "quantized-kv-cache-ecc-protection_amd"))
import torch  # noqa: E402

from kvecc import _lib, ops  # noqa: E402
from kvecc.memory_layout import kv_cache_pair  # noqa: E402

B, CTX, D, BS, HEADS = 8, 4096, 128, 16, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--warmup-s", type=float, default=0.5)
    ap.add_argument("--passes", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    fork = ctypes.CDLL(os.path.join(REPO, "tools", "exp", "libattn_int4tf.so"))
    vp, i64, ci, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    dec = fork.kvecc_paged_attention
    dec.argtypes = [vp, ci] + [vp] * 7 + [i64] * 10 + [f32, ci, vp, i64, vp]
    chk = fork.kvecc_paged_attention_chunk
    chk.argtypes = [vp, i64, i64, i64, ci] + [vp] * 7 + [i64] * 11 + [f32, ci, vp, i64, vp]
    fork.kvecc_paged_attention_chunk_workspace.restype = i64
    fork.kvecc_paged_attention_chunk_workspace.argtypes = [i64] * 5
    sm = 1 / math.sqrt(D)
    nb = CTX // BS
    blocks = B * nb
    for kvh in (32, 8):
        g = torch.Generator(device=dev).manual_seed(0)
        kc, vc = kv_cache_pair((blocks, 1, kvh, BS * D), torch.uint8, dev)
        kc.random_(0, 16, generator=g)  # the bytes an INT4 cache holds
        vc.copy_(kc.roll(1, 0))
        # the same nibbles as Hamming(8,4) codewords: the product's Hamming(8,4) kernel in the same passes
        hk, hv = kv_cache_pair((blocks, 1, kvh, BS * D), torch.uint8, dev)
        hk.view(-1).copy_(ops.hamming84_encode(kc.view(-1)))
        hv.view(-1).copy_(ops.hamming84_encode(vc.view(-1)))
        ks = torch.rand(blocks, 1, kvh, BS, device=dev, generator=g)
        vs = torch.rand_like(ks)
        table = torch.randperm(blocks, device=dev, generator=g).to(torch.int32).view(B, nb)
        lens = torch.full((B,), CTX, dtype=torch.int32, device=dev)
        ws = torch.empty(fork.kvecc_paged_attention_chunk_workspace(B, 16, HEADS, D, CTX) + 1, dtype=torch.float32,
                         device=dev)
        s = torch.cuda.current_stream().cuda_stream
        for n in (1, 16):
            qc = torch.randn(B, HEADS, n, D, device=dev, generator=g).half()
            qt = qc.transpose(1, 2)  # [B, n, H, D] in place, as the shim passes it
            q1 = qc[:, :, 0].contiguous()
            ref = torch.empty(qt.shape if n > 1 else q1.shape, dtype=torch.float16, device=dev)
            out = torch.empty_like(ref)

            def table_form():
                if n == 1:
                    ops.paged_attention_into(q1, kc, vc, table, lens, ks, vs, ref, 0, BS, sm, "int4", CTX)
                else:
                    ops.paged_attention_chunk_into(qt, kc, vc, table, lens, ks, vs, ref, 0, BS, sm, "int4", CTX)

            def table_free():
                if n == 1:
                    rc = dec(q1.data_ptr(), _lib.F16, kc.data_ptr(), vc.data_ptr(), table.data_ptr(), lens.data_ptr(),
                             ks.data_ptr(), vs.data_ptr(), out.data_ptr(), B, HEADS, kvh, D, blocks, 1, 0, BS, nb, CTX,
                             sm, _lib.CODEC_NONE, ws.data_ptr(), ws.numel(), s)
                else:
                    rc = chk(qt.data_ptr(), qt.stride(0), qt.stride(1), qt.stride(2), _lib.F16, kc.data_ptr(),
                             vc.data_ptr(), table.data_ptr(), lens.data_ptr(), ks.data_ptr(), vs.data_ptr(),
                             out.data_ptr(), B, n, HEADS, kvh, D, blocks, 1, 0, BS, nb, CTX, sm, _lib.CODEC_NONE,
                             ws.data_ptr(), ws.numel(), s)
                assert rc == 0, rc

            h84 = torch.empty_like(ref)

            def hamming84():
                if n == 1:
                    ops.paged_attention_into(q1, hk, hv, table, lens, ks, vs, h84, 0, BS, sm, "hamming84", CTX)
                else:
                    ops.paged_attention_chunk_into(qt, hk, hv, table, lens, ks, vs, h84, 0, BS, sm, "hamming84", CTX)

            cases = {"table": table_form, "table_free": table_free, "hamming84": hamming84}
            for fn in cases.values():
                t0 = time.perf_counter()
                while True:
                    for _ in range(args.warmup):
                        fn()
                    torch.cuda.synchronize()
                    if time.perf_counter() - t0 >= args.warmup_s:
                        break
            passes = {k: [] for k in cases}
            for _ in range(args.passes):
                for k, fn in cases.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.iters):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    passes[k].append(e0.elapsed_time(e1) / args.iters * 1e3)
            res = {k: {"us_per_call": round(statistics.median(p), 2), "pass_us": [round(x, 2) for x in p],
                       "spread_us": round(max(p) - min(p), 2)} for k, p in passes.items()}
            print(json.dumps({"kernel": "paged_attention_int4_table_ab", "q_len": n, "heads": HEADS, "kv_heads": kvh,
                              "head_dim": D, "ctx": CTX, "batch": B, **res,
                              "table_minus_table_free_us": round(res["table"]["us_per_call"] -
                                                                 res["table_free"]["us_per_call"], 2),
                              "hamming84_minus_table_us": round(res["hamming84"]["us_per_call"] -
                                                                res["table"]["us_per_call"], 2),
                              "hamming84_minus_table_free_us": round(res["hamming84"]["us_per_call"] -
                                                                     res["table_free"]["us_per_call"], 2),
                              "bit_equal": bool(torch.equal(out, ref) and torch.equal(h84, ref))}), flush=True)
        del kc, vc, hk, hv, ws


if __name__ == "__main__":
    main()
