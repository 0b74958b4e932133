#!/usr/bin/env python3
"""block_sparse_decode (rsa_block_sparse_decode) next to the existing call on the same inputs, on one
device, interleaved in one process, medians of device-event timings (the methodology of tools/perf_gqa.py).

Shapes: bf16, D = 128, H = 32 query heads over Hkv = 8 K/V heads, 128-token blocks, one list per K/V head made by select_blocks
(causal, top_k 16 and 64); Sq = 1 at (B, Sk) = (1, 131072) and (8, 32768), one Sq = 4 row and one paged row.

  existing   rsa_block_sparse_gqa_fwd with the causal row ranges -- what block_sparse_attention(..., causal=True) launches; its
             kernels are untouched by the decode call, so it is the baseline
  decode     rsa_block_sparse_decode at the library's default split size and at every blocks_per_split of --sweep

Both time the C entry alone, on lists built beforehand.  All forms of a shape are timed interleaved, the order rotating, in
--rounds rounds of --reps launches each; a round gives one median per form.  Reported per shape: the median of the rounds' medians
of every form, the SPREAD of the existing call (largest minus smallest of its rounds' medians: a difference below it is not a
difference), the bytes of the kept K and V blocks over the decode call's time beside the 6.3 TB/s the microarchitecture guide gives
as achievable (a description, not a gate), and the largest difference between the two calls' outputs.
Prints one line per measurement and a final JSON line; --out FILE appends the lines there.

    python tools/perf_decode.py [--reps 8] [--rounds 5] [--out profiles/decode_perf.txt]

--kv8 times instead, on the same six shapes and by the same method, rsa_block_sparse_decode_kv8 over an
e4m3 cache (filled by rsa_kv8_append, k_scale 0.5, v_scale 2) next to rsa_block_sparse_decode over the dequantised bf16 cache
code * scale -- the two outputs must be byte-equal -- then the writer at a prefill-sized append (bytes read and written over its
time) and rsa_pool_keys_kv8 next to rsa_pool_keys at prefill.

    python tools/perf_decode.py --kv8 [--out profiles/decode_kv8_perf.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rectified_spaattn_amd import _core, _lib, block_sparse  # noqa: E402

HBM_TBS = 6.3


def _ev(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def _round(fns, reps):
    """One median (ms) per function: reps launches each, interleaved, the order rotating."""
    evs = [[] for _ in fns]
    for i in range(reps):
        for j in range(len(fns)):
            w = (i + j) % len(fns)
            evs[w].append(_ev(fns[w]))
    torch.cuda.synchronize()
    return [statistics.median(a.elapsed_time(b) for a, b in e) for e in evs]


def shape_row(say, args, name, B, Sk, Sq, top_k, paged, sweep):
    dev = torch.device("cuda:0")
    L = _lib.lib()
    H, Hkv, D, blk = 32, 8, 128, 128
    NK = Sk // blk
    g = torch.Generator(device=dev).manual_seed(B * 7 + Sq + top_k)
    q = torch.randn(B, H, Sq, D, device=dev, generator=g).to(torch.bfloat16)
    k = torch.randn(B, Hkv, Sk, D, device=dev, generator=g).to(torch.bfloat16)
    v = torch.randn(B, Hkv, Sk, D, device=dev, generator=g).to(torch.bfloat16)
    lists = block_sparse.select_blocks(q, k, top_k, causal=True, as_lists=True)
    cols, counts = lists["cols"], lists["counts"]
    kept_blocks = int(counts.sum())
    kv_bytes = kept_blocks * blk * D * 2 * 2
    _, hi = block_sparse._window_ranges(dev, B, Sq, Sk, [Sk] * B, -1, 0)
    hi = hi.contiguous()
    tpart = block_sparse._tail_buffer(dev)
    outs = [torch.zeros((B, H, Sq, D), dtype=q.dtype, device=dev) for _ in range(2)]
    o4 = [_lib.RsaOut4(o.data_ptr(), o.stride(0), o.stride(1), o.stride(2)) for o in outs]
    dt = _core.dtype_code(q.dtype)
    st = _core._stream()
    scale = D ** -0.5
    tq, tk, tv = _core._t4(q), _core._t4(k), _core._t4(v)
    table = None
    if paged:       # the same cache as a pool of pages behind a random table
        P = B * NK
        perm = torch.randperm(P, device=dev, generator=g)
        seq_k = k.view(B, Hkv, NK, blk, D).permute(0, 2, 1, 3, 4).reshape(P, Hkv, blk, D)
        seq_v = v.view(B, Hkv, NK, blk, D).permute(0, 2, 1, 3, 4).reshape(P, Hkv, blk, D)
        kp, vp = torch.empty_like(seq_k), torch.empty_like(seq_v)
        kp[perm], vp[perm] = seq_k, seq_v
        table = perm.view(B, NK).to(torch.int32).contiguous()
        del seq_k, seq_v
        tkd, tvd = _core._t4(kp), _core._t4(vp)
    else:
        tkd, tvd = tk, tv

    def existing():
        _lib.check(L.rsa_block_sparse_gqa_fwd(B, H, Hkv, Hkv, Sq, Sk, D, dt, blk, 1, NK, Sk, scale, tq, tk, tv, cols.data_ptr(),
                                              counts.data_ptr(), None, hi.data_ptr(), 0 if hi.shape[0] == 1 else Sq,
                                              tpart.data_ptr(), tpart.numel() * 4, o4[0], st), "rsa_block_sparse_gqa_fwd")

    def decode(bps):
        need = ctypes.c_size_t(0)
        _lib.check(L.rsa_block_sparse_decode_bytes(B, H, Hkv, Hkv, Sq, D, NK, bps, ctypes.byref(need)), "decode_bytes")
        ws = torch.empty((need.value,), dtype=torch.uint8, device=dev)

        def run():
            _lib.check(L.rsa_block_sparse_decode(B, H, Hkv, Hkv, Sq, Sk, D, dt, blk, NK, None, Sk, 1, scale, tq, tkd, tvd,
                                                 table.data_ptr() if table is not None else None, NK if table is not None else 0,
                                                 B * NK if table is not None else 0, cols.data_ptr(), counts.data_ptr(), bps,
                                                 ws.data_ptr(), need.value, o4[1], None, st), "rsa_block_sparse_decode")
        return run

    forms = [0] + [c for c in sweep if c <= NK]
    fns = [existing] + [decode(c) for c in forms]
    for _ in range(2):
        for f in fns:
            f()
    fns[1]()
    torch.cuda.synchronize()
    diff = float((outs[0].float() - outs[1].float()).abs().max())
    rounds = [_round(fns, args.reps) for _ in range(args.rounds)]
    med = [statistics.median(r[i] for r in rounds) for i in range(len(fns))]
    spread = max(r[0] for r in rounds) - min(r[0] for r in rounds)
    say(f"{name}: B = {B}, Sk = {Sk} ({NK} blocks), Sq = {Sq}, top_k = {top_k}{', paged' if paged else ''}; "
        f"{kept_blocks} kept blocks = {kv_bytes / 1e6:.1f} MB of K and V")
    say(f"  existing call (ranged, causal): {1e3 * med[0]:.1f} us   (rounds: {' '.join(f'{1e3 * r[0]:.1f}' for r in rounds)}; "
        f"spread {1e3 * spread:.1f} us)")
    say(f"  decode call, default split:     {1e3 * med[1]:.1f} us   (rounds: {' '.join(f'{1e3 * r[1]:.1f}' for r in rounds)}) = "
        f"{kv_bytes / med[1] / 1e9:.3f} TB/s of kept K and V (achievable HBM: {HBM_TBS} TB/s)")
    say("  decode call by blocks_per_split: " + "  ".join(f"{c}: {1e3 * med[2 + i]:.1f}" for i, c in enumerate(forms[1:])) + "  (us)")
    gain = med[0] - med[1]
    say(f"  existing - decode = {1e3 * gain:+.1f} us ({med[0] / med[1]:.2f} x); faster by more than the spread: {gain > spread}; "
        f"largest |existing - decode| of the outputs: {diff:.3e}")
    return dict(name=name, B=B, Sk=Sk, Sq=Sq, top_k=top_k, paged=paged, existing_us=round(1e3 * med[0], 2),
                decode_us=round(1e3 * med[1], 2), spread_us=round(1e3 * spread, 2), kv_mb=round(kv_bytes / 1e6, 2),
                sweep_us={str(c): round(1e3 * med[2 + i], 2) for i, c in enumerate(forms[1:])}, faster=bool(gain > spread),
                out_diff=diff)


K_SCALE, V_SCALE = 0.5, 2.0


def _kv8_cache(B, Hkv, Sk, D, g, dev):
    """(k8, v8, kd, vd, append): e4m3 caches written by the writer from N(0, 1) bf16 rows, their dequantised bf16 twins, and
    the writer call as a function (for its own timing)."""
    L = _lib.lib()
    E4M3 = torch.float8_e4m3fn
    new = [torch.randn(B, Hkv, Sk, D, device=dev, generator=g).to(torch.bfloat16) for _ in range(2)]
    c8 = [torch.empty((B, Hkv, Sk, D), dtype=torch.uint8, device=dev).view(E4M3) for _ in range(2)]
    sc = [torch.full((Hkv,), s, dtype=torch.float32, device=dev) for s in (K_SCALE, V_SCALE)]
    o4 = [_lib.RsaOut4(t.data_ptr(), t.stride(0), t.stride(1), t.stride(2)) for t in c8]

    def append():
        _lib.check(L.rsa_kv8_append(B, Hkv, Sk, Sk, D, _lib.RSA_BF16, 128, _core._t4(new[0]), _core._t4(new[1]), o4[0], o4[1], None, 0,
                                    0, None, 0, None, Sk, sc[0].data_ptr(), sc[1].data_ptr(), _core._stream()), "rsa_kv8_append")
    append()
    lut = torch.arange(256, dtype=torch.uint8).view(E4M3).float().to(dev)       # (the value of every code, from torch's CPU cast)
    deq = []
    for t, s in zip(c8, (K_SCALE, V_SCALE)):
        d = torch.empty((B, Hkv, Sk, D), dtype=torch.bfloat16, device=dev)
        for b in range(B):
            for h in range(Hkv):
                d[b, h] = (lut[t[b, h].view(torch.uint8).long()] * s).to(torch.bfloat16)
        deq.append(d)
    return c8[0], c8[1], deq[0], deq[1], sc, append


def kv8_row(say, args, name, B, Sk, Sq, top_k, paged):
    dev = torch.device("cuda:0")
    L = _lib.lib()
    H, Hkv, D, blk = 32, 8, 128, 128
    NK = Sk // blk
    g = torch.Generator(device=dev).manual_seed(B * 7 + Sq + top_k)
    q = torch.randn(B, H, Sq, D, device=dev, generator=g).to(torch.bfloat16)
    k8, v8, kd, vd, sc, _ = _kv8_cache(B, Hkv, Sk, D, g, dev)
    lists = block_sparse.select_blocks(q, kd, top_k, causal=True, as_lists=True)
    cols, counts = lists["cols"], lists["counts"]
    kept_blocks = int(counts.sum())
    kv_bytes = kept_blocks * blk * D * 2 * 2
    outs = [torch.zeros((B, H, Sq, D), dtype=q.dtype, device=dev) for _ in range(2)]
    lses = [torch.zeros((B, H, Sq), dtype=torch.float32, device=dev) for _ in range(2)]
    o4 = [_lib.RsaOut4(o.data_ptr(), o.stride(0), o.stride(1), o.stride(2)) for o in outs]
    st = _core._stream()
    table = None
    if paged:
        P = B * NK
        perm = torch.randperm(P, device=dev, generator=g)
        table = perm.view(B, NK).to(torch.int32).contiguous()

        def pages(t):
            seq = t.view(B, Hkv, NK, blk, D).permute(0, 2, 1, 3, 4).reshape(P, Hkv, blk, D)
            out = torch.empty_like(seq)
            out[perm] = seq
            return out
        k8, v8 = (pages(t.view(torch.uint8)).view(torch.float8_e4m3fn) for t in (k8, v8))
        kd, vd = pages(kd), pages(vd)
    targs = (table.data_ptr(), NK, B * NK) if table is not None else (None, 0, 0)
    need = ctypes.c_size_t(0)
    _lib.check(L.rsa_block_sparse_decode_bytes(B, H, Hkv, Hkv, Sq, D, NK, 0, ctypes.byref(need)), "decode_bytes")
    ws = torch.empty((need.value,), dtype=torch.uint8, device=dev)
    head = (B, H, Hkv, Hkv, Sq, Sk, D, _lib.RSA_BF16, blk, NK, None, Sk, 1, D ** -0.5, _core._t4(q))

    def two_byte():
        _lib.check(L.rsa_block_sparse_decode(*head, _core._t4(kd), _core._t4(vd), *targs, cols.data_ptr(), counts.data_ptr(), 0,
                                             ws.data_ptr(), need.value, o4[0], lses[0].data_ptr(), st), "rsa_block_sparse_decode")

    def e4m3():
        _lib.check(L.rsa_block_sparse_decode_kv8(*head, _core._t4(k8), _core._t4(v8), *targs, cols.data_ptr(), counts.data_ptr(), 0,
                                                 ws.data_ptr(), need.value, o4[1], lses[1].data_ptr(), sc[0].data_ptr(),
                                                 sc[1].data_ptr(), st), "rsa_block_sparse_decode_kv8")
    fns = [two_byte, e4m3]
    for _ in range(2):
        for f in fns:
            f()
    torch.cuda.synchronize()
    equal = bool(torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)) and torch.equal(lses[0], lses[1]))
    rounds = [_round(fns, args.reps) for _ in range(args.rounds)]
    med = [statistics.median(r[i] for r in rounds) for i in range(2)]
    spread = max(r[0] for r in rounds) - min(r[0] for r in rounds)
    say(f"{name}: B = {B}, Sk = {Sk} ({NK} blocks), Sq = {Sq}, top_k = {top_k}{', paged' if paged else ''}; "
        f"{kept_blocks} kept blocks = {kv_bytes / 1e6:.1f} MB of bf16 K and V, {kv_bytes / 2e6:.1f} MB of e4m3")
    say(f"  2-byte call on the dequantised cache: {1e3 * med[0]:.1f} us   (rounds: {' '.join(f'{1e3 * r[0]:.1f}' for r in rounds)}; "
        f"spread {1e3 * spread:.1f} us) = {kv_bytes / med[0] / 1e9:.3f} TB/s of kept K and V")
    say(f"  e4m3 call:                            {1e3 * med[1]:.1f} us   (rounds: {' '.join(f'{1e3 * r[1]:.1f}' for r in rounds)}) = "
        f"{kv_bytes / 2 / med[1] / 1e9:.3f} TB/s of kept codes")
    gain = med[0] - med[1]
    say(f"  2-byte - e4m3 = {1e3 * gain:+.1f} us ({med[0] / med[1]:.2f} x); faster by more than the spread: {gain > spread}; "
        f"slower by more than the spread: {-gain > spread}; outputs and log-sum-exp byte-equal: {equal}")
    return dict(name=name, B=B, Sk=Sk, Sq=Sq, top_k=top_k, paged=paged, two_byte_us=round(1e3 * med[0], 2),
                e4m3_us=round(1e3 * med[1], 2), spread_us=round(1e3 * spread, 2), kv_mb=round(kv_bytes / 1e6, 2),
                faster=bool(gain > spread), slower=bool(-gain > spread), byte_equal=equal)


def kv8_writer_and_pool(say, args, B, Sk):
    """The writer at a prefill-sized append, and pool_keys at prefill from the e4m3 and from the bf16 cache."""
    dev = torch.device("cuda:0")
    L = _lib.lib()
    Hkv, D, blk = 8, 128, 128
    NK = Sk // blk
    g = torch.Generator(device=dev).manual_seed(B)
    k8, _, kd, _, sc, append = _kv8_cache(B, Hkv, Sk, D, g, dev)
    out = torch.empty((B, Hkv, NK, D), dtype=torch.float32, device=dev)
    st = _core._stream()

    def pool2():
        _lib.check(L.rsa_pool_keys(B, Hkv, Sk, D, _lib.RSA_BF16, blk, NK, _core._t4(kd), None, 0, 0, None, Sk, None, 0, 0,
                                   out.data_ptr(), st), "rsa_pool_keys")

    def pool8():
        _lib.check(L.rsa_pool_keys_kv8(B, Hkv, Sk, D, blk, NK, _core._t4(k8), None, 0, 0, None, Sk, None, 0, 0, out.data_ptr(),
                                       sc[0].data_ptr(), st), "rsa_pool_keys_kv8")
    fns = [append, pool2, pool8]
    for _ in range(2):
        for f in fns:
            f()
    rounds = [_round(fns, args.reps) for _ in range(args.rounds)]
    med = [statistics.median(r[i] for r in rounds) for i in range(3)]
    spread = [max(r[i] for r in rounds) - min(r[i] for r in rounds) for i in range(3)]
    elems = 2 * B * Hkv * Sk * D        # K and V
    say(f"writer, B = {B}, Hkv = {Hkv}, T = Sk = {Sk}, D = {D} (prefill): {1e3 * med[0]:.1f} us (spread {1e3 * spread[0]:.1f}); "
        f"{elems * 2 / 1e6:.1f} MB read + {elems / 1e6:.1f} MB written = {elems * 3 / med[0] / 1e9:.3f} TB/s")
    say(f"pool_keys at prefill, same shape: bf16 cache {1e3 * med[1]:.1f} us (spread {1e3 * spread[1]:.1f}) = "
        f"{elems / med[1] / 1e9:.3f} TB/s of K; e4m3 cache {1e3 * med[2]:.1f} us (spread {1e3 * spread[2]:.1f}) = "
        f"{elems / 2 / med[2] / 1e9:.3f} TB/s of codes")
    return dict(B=B, Sk=Sk, writer_us=round(1e3 * med[0], 2), pool_bf16_us=round(1e3 * med[1], 2), pool_e4m3_us=round(1e3 * med[2], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sweep", default="1,2,4,8,16,32,64")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kv8", action="store_true", help="the e4m3 cache next to the 2-byte call, the writer and pool_keys")
    args = ap.parse_args()
    sweep = [int(x) for x in args.sweep.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    res = dict(reps=args.reps, rounds=args.rounds, device=torch.cuda.get_device_name(0), rows=[])
    rows = [("long-16", 1, 131072, 1, 16, False), ("long-64", 1, 131072, 1, 64, False), ("batch-16", 8, 32768, 1, 16, False),
            ("batch-64", 8, 32768, 1, 64, False), ("batch-64-Sq4", 8, 32768, 4, 64, False), ("batch-64-paged", 8, 32768, 1, 64, True)]
    if args.kv8:
        say(f"block_sparse_decode over an e4m3 cache against the 2-byte call on the dequantised cache: bf16 q, D = 128, H = 32 over "
            f"Hkv = 8, 128-token blocks, lists per K/V head, default split; {args.rounds} rounds x {args.reps} launches per form, "
            "interleaved")
        for row in rows:
            res["rows"].append(kv8_row(say, args, *row))
            torch.cuda.empty_cache()
        res["writer_pool"] = [kv8_writer_and_pool(say, args, B, Sk) for B, Sk in ((8, 32768), (1, 131072))]
        say(json.dumps(res))
        if args.out:
            with open(args.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    say(f"block_sparse_decode against block_sparse_attention(causal=True): bf16, D = 128, H = 32 over Hkv = 8, 128-token blocks, "
        f"lists per K/V head; {args.rounds} rounds x {args.reps} launches per form, interleaved")
    for name, B, Sk, Sq, top_k, paged in rows:
        res["rows"].append(shape_row(say, args, name, B, Sk, Sq, top_k, paged, sweep))
        torch.cuda.empty_cache()
    say(json.dumps(res))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
