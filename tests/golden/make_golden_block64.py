"""Fixtures of the 64-token-block path (block_size_M = block_size_N = 64), produced by the REFERENCE operator itself.

Build-machine only, like make_golden.py, whose shims it imports without changing them (stub modules, TRITON_INTERPRET=1,
the varlen SDPA stand-in, the fp16 cast around the Triton kernel).  The oracle is written for 128-token blocks, so nothing
here cross-checks the reference: instead every discrete decision of a case -- the top-k boundary, the cumulative-probability
threshold, each GAPR comparison -- is re-derived in fp64 from the reference's own probabilities and the inputs, and a seed
whose smallest relative margin is below MIN_MARGIN is skipped (near-ties are where two correct fp32 implementations may
differ).  The accepted seed and its margin go into each file's meta.

    python tests/golden/make_golden_block64.py          # writes tests/golden/op_b64_*.npz and gapr_b64.npz
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (sets TRITON_INTERPRET=1 before triton is imported)

import numpy as np  # noqa: E402
import torch  # noqa: E402

BLK = 64
MIN_MARGIN = 1e-5
FIRST_SEED = mg.FIRST_SEED    # the op_* convention (tests/test_oracle_golden.py): a skipped seed is recorded in meta
OUT_ROWS = 4096


def _margins(q, k, probs, one_hot_unused, nogapr_unused, NBv, top_k, p, n_txt):
    """Smallest relative margin of the selection decisions, in fp64.  q, k: [B, H, S, D] fp32 arrays; probs: the reference's
    [B, H, NBv, L] (after IPAR)."""
    m = np.inf
    B, H = probs.shape[:2]
    for b in range(B):
        for h in range(H):
            pr = probs[b, h].astype(np.float64)
            for i in range(NBv):
                row = pr[i]
                srt = np.sort(row)[::-1]
                # top-k boundary (ties at the k-th value decide which block is kept)
                if 0 < top_k < len(srt):
                    m = min(m, (srt[top_k - 1] - srt[top_k]) / max(abs(srt[top_k - 1]), 1e-30))
                # cumulative threshold: distance of every prefix sum from p
                cs = np.cumsum(srt)
                m = min(m, float(np.min(np.abs(cs - p))) / max(p, 1e-30))
            # GAPR: |s| against the pooling error, s = qbar . kbar (the common scale cancels)
            pad = max(0, NBv * BLK - q.shape[2])     # (the reference zero-pads a partial last block)
            qv = np.pad(q[b, h].astype(np.float64), ((0, pad), (0, 0)))[:NBv * BLK].reshape(NBv, BLK, -1)
            kv = np.pad(k[b, h].astype(np.float64), ((0, pad), (0, 0)))[:NBv * BLK].reshape(NBv, BLK, -1)
            qb, kb = qv.mean(1), kv.mean(1)
            aq, ak = np.abs(qv - qb[:, None]).mean(1), np.abs(kv - kb[:, None]).mean(1)
            s = np.abs(qb @ kb.T)
            err = np.abs(aq @ kb.T) + np.abs(qb @ ak.T)
            m = min(m, float(np.min(np.abs(s - err) / np.maximum(np.maximum(s, err), 1e-30))))
    return float(m)


def main():
    mg._install_stubs()
    import rectified_spaattn.attn as ref_attn
    import rectified_spaattn.gapr_mask as ref_gapr
    import rectified_spaattn.rectified_hunyuan_attn as ref_hy
    import rectified_spaattn.rectified_flux_attn as ref_fx
    import rectified_spaattn.rectified_wan21_attn as ref_wan
    import rectified_spaattn.rectified_cogvideo_attn as ref_cog
    from rectified_spaattn_amd import synth

    ref_attn.flash_attn_varlen_func = mg._varlen_sdpa
    for mod_ in (ref_hy, ref_fx, ref_wan, ref_cog):
        mg._wrap_kernel(mod_)
    torch.set_num_threads(8)

    def run_case(variant, B, H, S, D, top_k, p, nb_width, seed, rejected=(), **kw):
        q, k, v = synth.structured_qkv(seed, B, H, S, D, block=BLK)
        tq, tk, tv = (torch.from_numpy(x.copy()) for x in (q, k, v))
        if variant == "hunyuan":
            num_true = kw["num_true"]
            mask = torch.zeros(B, 1, 1, S, dtype=torch.bool)
            mask[..., :num_true] = True
            cu = torch.tensor([0, num_true, S], dtype=torch.int32)
            mod, extra = ref_hy, {}
            call = dict(attn_mask=mask, cu_seqlens_q=cu, cu_seqlens_kv=cu, max_seqlen_q=S, max_seqlen_kv=S)
            NBv = S // BLK - 256 // BLK
            n_txt = 256 - (S - num_true)
        elif variant == "flux":
            cu = torch.tensor([0, S, S], dtype=torch.int32)
            mod, extra = ref_fx, dict(text_length=kw["text_length"])
            call = dict(attn_mask=None, cu_seqlens_q=cu, cu_seqlens_kv=cu, max_seqlen_q=S, max_seqlen_kv=S)
            NBv = S // BLK - kw["text_length"] // BLK
            n_txt = kw["text_length"]
        elif variant == "cogvideo":
            cuq = torch.tensor([0, S, S * B], dtype=torch.int32)
            mod, extra = ref_cog, dict(text_length=kw["text_length"])
            call = dict(attn_mask=None, cu_seqlens_q=cuq, cu_seqlens_kv=cuq, max_seqlen_q=S, max_seqlen_kv=S)
            NB = (S + BLK - 1) // BLK
            NBv = NB - (kw["text_length"] + NB * BLK - S) // BLK
            n_txt = kw["text_length"]
        elif variant == "wan":
            cu = torch.tensor([0, S, S], dtype=torch.int32)
            mod, extra = ref_wan, dict(first_frame_blocks=kw.get("ffb", 0))
            call = dict(attn_mask=None, cu_seqlens_q=cu, cu_seqlens_kv=cu, max_seqlen_q=S, max_seqlen_kv=S)
            NBv = (S + BLK - 1) // BLK
            n_txt = 0
        else:
            raise ValueError(variant)
        nbr = synth.banded_neighbors(NBv, nb_width) if nb_width >= 0 else None
        tnbr = torch.from_numpy(nbr) if nbr is not None else None
        captured = {}
        orig_builder = mod._build_block_index_with_importance_optimized

        def spy(*a, **k_):
            r = orig_builder(*a, **k_)
            captured["one_hot"], captured["probs"], captured["nogapr"] = (x.clone() for x in r)
            return r

        mod._build_block_index_with_importance_optimized = spy
        try:
            out = mod.rectified_block_sparse_attention(tq.clone(), tk.clone(), tv.clone(), top_k=top_k, block_size_M=BLK,
                                                       block_size_N=BLK, block_neighbor_list=tnbr, p_remain_rates=p,
                                                       **call, **extra)
        finally:
            mod._build_block_index_with_importance_optimized = orig_builder
        one_hot = captured["one_hot"].numpy().astype(np.uint8)
        probs = captured["probs"].numpy().astype(np.float32)
        nogapr = captured["nogapr"].numpy().astype(np.uint8)
        assert one_hot.shape[-2] == NBv, (one_hot.shape, NBv)
        margin = _margins(q, k, probs, one_hot, nogapr, NBv, top_k, p, n_txt)
        out = out.float().numpy()
        if S > 8192:   # long cases: the first OUT_ROWS rows of O, as fp16 (every committed file stays under 1 MiB)
            out = out[:, :OUT_ROWS].astype(np.float16)
            kw = dict(kw, out_rows=OUT_ROWS)
        meta = dict(variant=variant, B=B, H=H, S=S, D=D, top_k=top_k, p=p, nb_width=nb_width, seed=seed, smooth=0.0,
                    block=BLK, margin=margin, rejected_seeds=list(rejected), NB_total=int(one_hot.shape[-1]), NBv=int(NBv), L=int(probs.shape[-1]),
                    **kw)
        return margin, dict(meta=np.array(repr(meta)), one_hot=np.packbits(one_hot, axis=-1), probs=probs,
                            nogapr=np.packbits(nogapr, axis=-1), out=out,
                            one_hot_shape=np.array(one_hot.shape), nogapr_shape=np.array(nogapr.shape))

    cases = [
        # name, variant, B, H, S, D, top_k, p, neighbour band, kwargs
        ("b64_wan_pad_1450", "wan", 1, 2, 1450, 128, 4, 0.3, 1, dict(ffb=3)),
        ("b64_hunyuan_1280", "hunyuan", 1, 2, 1280, 128, 3, 0.3, 1, dict(num_true=1024 + 200)),
        ("b64_flux_1536", "flux", 1, 1, 1536, 128, 3, 0.3, 1, dict(text_length=512)),
        # 832 visual tokens: a multiple of 64, not of 128 (refused at block 128)
        ("b64_cogvideo_1058", "cogvideo", 1, 2, 1058, 64, 3, 0.3, 1, dict(text_length=226)),
        ("b64_wan_d64_1100", "wan", 1, 2, 1100, 64, 3, 0.5, 1, dict(ffb=0)),
        ("b64_b2_hunyuan_1280", "hunyuan", 2, 1, 1280, 128, 3, 0.3, 1, dict(num_true=1024 + 150)),
        # 260 blocks: a selection row longer than 256 columns (K3's sorted-head path)
        ("b64_big_wan_16640", "wan", 1, 1, 16640, 64, 20, 0.3, 1, dict(ffb=3)),
    ]
    only = os.environ.get("RSA_GOLDEN_ONLY")
    for name, variant, B, H, S, D, top_k, p, nbw, kw in cases:
        if only and not name.startswith(only):
            continue
        rejected = []
        for seed in range(FIRST_SEED, FIRST_SEED + 20):
            margin, res = run_case(variant, B, H, S, D, top_k, p, nbw, seed, rejected=rejected, **kw)
            print(f"{name}: seed {seed} smallest relative decision margin {margin:.2e}", flush=True)
            if margin >= MIN_MARGIN:
                np.savez_compressed(os.path.join(HERE, f"op_{name}.npz"), **res)
                break
            rejected.append(dict(seed=seed, rows=[dict(smallest_relative_margin=margin)]))
        else:
            raise SystemExit(f"no seed with a margin >= {MIN_MARGIN} for {name}")
    if only:
        return
    # estimate_pr_gain on 64-token blocks (gapr_mask.py:4)
    from rectified_spaattn_amd import synth as sy
    q, k, _ = sy.structured_qkv(9, 1, 2, 1024, 128, block=BLK)
    Qb = torch.from_numpy(q).reshape(1, 2, 16, BLK, 128)
    Kb = torch.from_numpy(k).reshape(1, 2, 16, BLK, 128)
    qp, kp = Qb.mean(-2), Kb.mean(-2)
    sc = torch.matmul(qp, kp.transpose(-1, -2))
    g = ref_gapr.estimate_pr_gain(Qb, Kb, qp, kp, sc)
    err = (torch.abs(Qb.double() - qp.double()[..., None, :]).mean(-2) @ kp.double().transpose(-1, -2)).abs() + \
        (qp.double() @ torch.abs(Kb.double() - kp.double()[..., None, :]).mean(-2).transpose(-1, -2)).abs()
    margin = float(((sc.double().abs() - err).abs() / torch.maximum(sc.double().abs(), err)).min())
    np.savez_compressed(os.path.join(HERE, "gapr_b64.npz"), seed=9, block=BLK, margin=margin,
                        mask=np.packbits(g.numpy(), axis=-1), shape=np.array(g.shape), q_pools=qp.numpy(),
                        k_pools=kp.numpy(), scores=sc.numpy())
    print("gapr_b64: unreliable fraction", float(g.float().mean()), "margin", margin)


if __name__ == "__main__":
    main()
