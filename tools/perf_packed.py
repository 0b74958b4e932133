#!/usr/bin/env python3
"""The packed extend call (rsa_block_sparse_extend_packed[_kv8]) next to the ragged call on the padded copy
and next to the separate calls, on one device, interleaved in one process, medians of device-event timings (the method and the
cache of tools/perf_extend.py, the entries' wrapper of tools/perf_ragged.py).

Shapes: bf16 q, D = 128, H = 32 over Hkv = 8, 128-token blocks, B = 8 x 32 768 keys, paged bf16 and e4m3, lists per K/V head from
select_blocks_pooled(causal=True, keep_first=1, keep_local=1, q_len=) at top_k 16 / 64, C entries on prebuilt lists.

  (i)   mixed     one item of 512 rows and seven of one row: packed T = 576, M = 512
  (ii)  decode    eight items of one row: packed T = 8, M = 1 (the step's own shape: qg = 1, decode's kernels and split)
  (iii) decode in the mixed step's graph shape: eight items of one row, packed T = 576, M = 512

Each against, in the same run: the ragged entry at padded Sq = 512 with q_len; the separate calls (rsa_block_sparse_extend at
B = 1 plus rsa_block_sparse_decode at B = 7; rsa_block_sparse_decode at B = 8).  All at the library's default split.  Reported:
the median of the rounds' medians of every form, the round-median spreads, the ratios, and whether the packed rows are the ragged
call's and the separate calls' bytes (None where the default split sizes differ: bytes are promised at equal splits).

    python tools/perf_packed.py [--reps 5] [--rounds 3] [--out profiles/extend_packed_perf.txt]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import perf_extend as pe  # noqa: E402
import perf_ragged as pr  # noqa: E402
from rectified_spaattn_amd import _core, _lib, block_sparse  # noqa: E402

H, HKV, D, BLK, SQ = pr.H, pr.HKV, pr.D, pr.BLK, pr.SQ


class Calls(pr.Calls):
    def packed(self, q, T, B, M, cu, cols, counts, bps, out):
        """rsa_block_sparse_extend_packed[_kv8] on q, out [T, H, D] -> the launch."""
        c, L = self.c, self.L
        need = ctypes.c_size_t(0)
        _lib.check(L.rsa_block_sparse_extend_packed_bytes(T, B, H, HKV, HKV, M, D, BLK, c.NK, bps, ctypes.byref(need), None), "bytes")
        ws = torch.empty((need.value,), dtype=torch.uint8, device=q.device)
        tq, tk, tv = block_sparse._t3(q), _core._t4(self.kp), _core._t4(self.vp)
        o4 = _lib.RsaOut4(out.data_ptr(), 0, out.stride(1), out.stride(0))
        fn = getattr(L, "rsa_block_sparse_extend_packed" + self.sfx)

        def run():
            rc = fn(T, B, H, HKV, HKV, M, c.Sk, D, _lib.RSA_BF16, BLK, c.NK, None, c.Sk, 1, D ** -0.5, tq, tk, tv, c.table.data_ptr(),
                    c.NK, c.B * c.NK, cols.data_ptr(), counts.data_ptr(), bps, ws.data_ptr(), need.value, o4, None, *self.tail,
                    cu.data_ptr(), self.st)
            assert rc == 0, rc
        run.keep = (ws, cu, cols, counts)
        return run


def shape_rows(say, args, cache, form, top_k):
    dev = torch.device("cuda:0")
    B, NK = cache.B, cache.NK
    NQ = SQ // BLK
    calls = Calls(_lib.lib(), cache, form)
    q = torch.randn(B, H, SQ, D, device=dev, generator=cache.gen).to(torch.bfloat16)
    sel = dict(causal=True, keep_first=1, keep_local=1, as_lists=True)
    res = []
    cases = (("(i) 512 + 7 x 1 rows, T = 576, M = 512", [SQ] + [1] * (B - 1), 576, SQ),
             ("(ii) 8 x 1 rows, T = 8, M = 1", [1] * B, 8, 1),
             ("(iii) 8 x 1 rows, T = 576, M = 512", [1] * B, 576, SQ))
    for label, ns, T, M in cases:
        q_len = torch.tensor(ns, dtype=torch.int32, device=dev)
        lists = block_sparse.select_blocks_pooled(q, cache.pooled[form], top_k, q_len=q_len, **sel)
        cols, counts = lists["cols"], lists["counts"]          # [B * HKV, NQ, NK], [B * HKV, NQ]
        cols1 = cols.view(B, HKV, NQ, NK)[:, :, 0].contiguous()
        counts1 = counts.view(B, HKV, NQ)[:, :, 0].contiguous()
        starts = [0]
        for n in ns:
            starts.append(starts[-1] + n)
        cu = torch.tensor(starts, dtype=torch.int32, device=dev)
        qp = torch.full((T, H, D), float("nan"), dtype=q.dtype, device=dev)
        for b, n in enumerate(ns):
            qp[starts[b]:starts[b] + n] = q[b, :, :n].transpose(0, 1)
        out_p = torch.full((T, H, D), float("nan"), dtype=q.dtype, device=dev)
        out_r, out_e, out_d = (torch.zeros((B, H, SQ, D), dtype=q.dtype, device=dev) for _ in range(3))
        pc, pn = (cols1, counts1) if M == 1 else (cols, counts)
        names = ["packed", "ragged"]
        fns = [calls.packed(qp, T, B, M, cu, pc, pn, 0, out_p), calls.attend("extend_ragged", q, 0, B, SQ, cols, counts, 0, out_r, q_len)]
        b0 = 1 if ns[0] == SQ else 0            # the decode items
        dec = calls.attend("decode", q[b0:, :, :1], b0, B - b0, 1, cols1[b0:].contiguous(), counts1[b0:].contiguous(), 0,
                           out_d[b0:, :, :1])
        if b0:
            ext1 = calls.attend("extend", q[:1], 0, 1, SQ, cols, counts, 0, out_e[:1])

            def separate():
                ext1()
                dec()
            names += ["separate", "extend B=1", "decode B=7"]
            fns += [separate, ext1, dec]
        else:
            names.append("separate")
            fns.append(dec)
        med, spread = pr._measure(names, fns, args)
        g = block_sparse.packed_row_groups(T, B, H, HKV, HKV, M, BLK)
        live = [out_p[starts[b]:starts[b] + n].transpose(0, 1) for b, n in enumerate(ns)]
        # bytes are compared where the default split sizes agree.  The ragged call's is one split (2048 row groups); the packed one's
        # is one split from 256 workgroups on and decode's min(8, NK) below; extend at B = 1 has 256 row groups: one split
        one_split = g["groups"] >= 256
        same_r = all(torch.equal(live[b].contiguous().view(torch.int16), out_r[b, :, :n].contiguous().view(torch.int16))
                     for b, n in enumerate(ns)) if one_split else None
        same_e = bool(torch.equal(live[0].contiguous().view(torch.int16), out_e[0].view(torch.int16))) if b0 else None
        same_d = all(torch.equal(live[b].contiguous().view(torch.int16), out_d[b, :, :1].contiguous().view(torch.int16))
                     for b in range(b0, B)) if not one_split else None
        slack = bool((out_p[starts[-1]:] == 0).all())
        us = {n: round(1e3 * t, 2) for n, t in med.items()}
        sp = {n: round(1e3 * s, 2) for n, s in spread.items()}
        say(f"B = {B} x {cache.Sk} keys, {form} paged, top_k = {top_k}; {label}; packed: {g['pieces']} pieces, {g['groups']} workgroups "
            f"per split, qg = {g['qg']}; ragged: {block_sparse.extend_row_groups(B, H, HKV, HKV, SQ, BLK)['groups']} row groups; "
            f"kept pairs {int(counts.sum())}")
        say("  " + ";  ".join(f"{n}: {us[n]:.1f} us (+- {sp[n]:.1f})" for n in names))
        say(f"  ragged / packed = {med['ragged'] / med['packed']:.2f} (ragged - packed = {us['ragged'] - us['packed']:.1f} us against the "
            f"ragged spread {sp['ragged']:.1f} us); packed / separate = {med['packed'] / med['separate']:.2f}; packed rows byte-equal to "
            f"ragged: {same_r}, to extend B=1: {same_e}, to decode: {same_d}; slack rows zero: {slack}")
        res.append(dict(form=form, top_k=top_k, case=label, us=us, spread_us=sp, same_ragged=same_r, same_extend=same_e,
                        same_decode=same_d, slack_zero=slack))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--top-ks", default="16,64")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    res = dict(reps=args.reps, rounds=args.rounds, device=torch.cuda.get_device_name(0))
    say(f"packed extend against the ragged call and the separate calls: bf16 q, D = {D}, H = {H} over Hkv = {HKV}, {BLK}-token blocks, "
        f"causal, B = 8 x 32768 keys paged; {args.rounds} rounds x {args.reps} launches per form, interleaved; default splits")
    cache = pe.Cache(8, 32768, torch.device("cuda:0"))
    res["rows"] = []
    for form in ("bf16", "e4m3"):
        for top_k in [int(x) for x in args.top_ks.split(",")]:
            res["rows"] += shape_rows(say, args, cache, form, top_k)
    say(json.dumps(res))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
