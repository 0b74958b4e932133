"""select_blocks_antidiag without a device: the vectorised reference against the four-loop evaluation of the
contract's steps 1-4, and the refusals of the Python call and of the C entries."""
import ctypes
import os

import numpy as np
import pytest
import torch

import antidiag_ref as aref


@pytest.mark.parametrize("s", [8, 16])
@pytest.mark.parametrize("causal", [False, True])
def test_the_vectorised_reference_is_the_four_loops(s, causal):
    blk, B, H, Hkv, D = 64, 2, 2, 1, 8
    S = 2 * blk + s + 3
    rng = np.random.default_rng(s + causal)
    q, k = rng.standard_normal((B, H, S, D)), rng.standard_normal((B, Hkv, S, D))
    lens = [S, blk + 5]
    k[1, :, lens[1]:] = np.nan
    for heads in ("kv", "q"):
        P, Pn = (f(q, k, lens, s, blk, causal, mask_heads=heads) for f in (aref.mass, aref.naive_mass))
        assert np.isfinite(P).all() and np.abs(P - Pn).max() < 1e-12
        # every live row group that sees a key group spreads a mass of 1 over its row
        want = np.array([[aref.group_visible(S, S, ln, s, causal).any(-1)[i * blk // s:(i + 1) * blk // s].sum()
                          for i in range(P.shape[2])] for ln in lens]) * (H // P.shape[1])
        assert np.abs(P.sum(-1) - want[:, None]).max() < 1e-9


def test_python_refusals():
    from rectified_spaattn_amd import select_blocks_antidiag as sel
    q, k = torch.zeros(2, 4, 200, 64, dtype=torch.bfloat16), torch.zeros(2, 2, 300, 64, dtype=torch.bfloat16)
    for kw in (dict(stride=4), dict(stride=32), dict(block_size=32), dict(q_len=[1, 2]), dict(max_q_len=3),
               dict(cu_seqlens_q=torch.zeros(3, dtype=torch.int32)), dict(block_table=torch.zeros(2, 3, dtype=torch.int32))):
        with pytest.raises(NotImplementedError, match=next(iter(kw)) if "block_size" not in kw else "block_size"):
            sel(q, k, 2, **kw)
    with pytest.raises(NotImplementedError, match="float8_e4m3fn"):
        sel(q, k.to(torch.float8_e4m3fn), 2)
    for D in (16, 32):
        with pytest.raises(NotImplementedError, match="head dim"):
            sel(q[..., :D], k[..., :D], 2)
    for kw in (dict(stride=True), dict(sm_scale=0.0), dict(sm_scale=float("nan")), dict(sm_scale=float("inf")), dict(top_k=-1),
               dict(mask_heads="all"), dict(kv_len=301), dict(top_p=1.5), dict(score_scale=1.0), dict(return_mass=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            sel(q, k, **{"top_k": 2, **kw})
    with pytest.raises(ValueError, match="Hkv"):
        sel(q, torch.zeros(2, 3, 300, 64, dtype=torch.bfloat16), 2)
    from rectified_spaattn_amd import _lib      # a well-formed call on CPU tensors reaches the device check and no further
    with pytest.raises(_lib.RsaError):
        sel(q, k, 2, stride=16, causal=True, kv_len=[300, 17], top_p=0.9, return_mass=True, return_scores=True, as_lists=True)


def test_c_refusals():
    from rectified_spaattn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librsa_hip.so is not built")
    L = _lib.lib()
    OK, BAD, UNSUP, WS = 0, -1, -2, -3
    n = ctypes.c_size_t(0)
    size = dict(B=2, H=4, Hkv=2, Hl=2, Sq=200, D=64, block=128, stride=8, NQ=2, NK=3)
    assert L.rsa_block_select_antidiag_bytes(*size.values(), ctypes.byref(n)) == OK and n.value == 2 * 2 * 2 * 3 * 4
    for kw, want in ((dict(stride=4), UNSUP), (dict(D=32), UNSUP), (dict(block=32), UNSUP), (dict(NK=8193), UNSUP), (dict(NQ=3), BAD),
                     (dict(Hl=3), BAD), (dict(B=0), BAD)):
        assert L.rsa_block_select_antidiag_bytes(*dict(size, **kw).values(), ctypes.byref(n)) == want, kw
    t = _lib.RsaTensor4(256, 0, 0, 64)          # (never dereferenced: every call below is refused before the first HIP call)
    call = dict(B=2, H=4, Hkv=2, Hl=2, Sq=200, Sk=300, D=64, dtype=0, block=128, stride=8, NQ=2, NK=3, q=t, k=t, kv_len=None,
                kv_valid=300, causal=1, sm_scale=0.125, top_k=2, keep_first=0, keep_local=0, ws=256, ws_bytes=16, bitmask=256,
                cols=256, counts=256, scores=None, p16=-1, c=0.0, mass=None, stream=None)
    for kw, want in ((dict(), WS), (dict(stride=12), UNSUP), (dict(D=32), UNSUP), (dict(sm_scale=0.0), BAD),
                     (dict(sm_scale=float("nan")), BAD), (dict(sm_scale=float("inf")), BAD), (dict(p16=70000), BAD),
                     (dict(B=0, stride=12), BAD), (dict(block=32, stride=12), UNSUP), (dict(kv_valid=301), BAD), (dict(ws=None), BAD),
                     (dict(k=_lib.RsaTensor4(None, 0, 0, 64)), BAD), (dict(cols=None), BAD), (dict(NK=4), BAD)):
        assert L.rsa_block_select_antidiag(*dict(call, **kw).values()) == want, kw
