"""select_blocks_observed without a device: the vectorised reference against the four loops, the mass a
row spreads, the names in the header and the table, and the refusals of the Python call and of the C entries."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import observed_ref as oref


@pytest.mark.parametrize("causal", [False, True])
def test_the_vectorised_reference_is_the_four_loops(causal):
    blk, B, H, Hkv, W, D = 64, 2, 4, 2, 5, 8
    Sk = 2 * blk + 37
    rng = np.random.default_rng(causal)
    q, k = rng.standard_normal((B, H, W, D)), rng.standard_normal((B, Hkv, Sk, D))
    lens = [Sk, 3]          # (the second item under causal: rows 0 and 1 see nothing)
    k[1, :, lens[1]:] = np.nan
    for heads in ("kv", "q"):
        P, Pn = (f(q, k, lens, blk, causal, 0.7, heads) for f in (oref.mass, oref.naive_mass))
        assert np.isfinite(P).all() and np.abs(P - Pn).max() < 1e-12
        # every live row spreads a mass of exactly 1 over its list row
        live = np.array([oref.row_visible(W, Sk, n, causal).any(-1).sum() for n in lens]) * (H // P.shape[1])
        assert np.abs(P.sum(-1) - live[:, None]).max() < 1e-9
    assert not causal or live[1] == 3       # (mask_heads "q": one head a list row)


def test_python_refusals():
    from rectified_spaattn_amd import select_blocks_observed as sel
    q, k = torch.zeros(2, 4, 17, 64, dtype=torch.bfloat16), torch.zeros(2, 2, 300, 64, dtype=torch.bfloat16)
    for W in (0, 65):
        with pytest.raises(ValueError, match="q_obs"):
            sel(torch.zeros(2, 4, W, 64, dtype=torch.bfloat16), k, 2)
    for D in (16, 32):
        with pytest.raises(NotImplementedError, match="head dim"):
            sel(q[..., :D], k[..., :D], 2)
    with pytest.raises(NotImplementedError, match="float8_e4m3fn"):
        sel(q, k.to(torch.float8_e4m3fn), 2)
    with pytest.raises(NotImplementedError):        # MXFP4 codes
        sel(q, torch.zeros(2, 2, 300, 32, dtype=torch.uint8), 2)
    with pytest.raises(NotImplementedError, match="block_size"):
        sel(q, k, 2, block_size=32)
    for kw in (dict(q_len=[1, 2]), dict(cu_seqlens_q=torch.zeros(3, dtype=torch.int32))):        # no such arguments
        with pytest.raises(TypeError):
            sel(q, k, 2, **kw)
    for scale in (0.0, float("nan")):
        with pytest.raises(ValueError, match="sm_scale"):
            sel(q, k, 2, sm_scale=scale)
    from rectified_spaattn_amd import _lib      # a well-formed call on CPU tensors reaches the device check and no further
    with pytest.raises(_lib.RsaError):
        sel(q, k, 2, causal=True, kv_len=[300, 17], top_p=0.9, return_mass=True, return_scores=True, as_lists=True, score_splits=3)


def test_the_c_names_follow_the_antidiag_pair():
    from rectified_spaattn_amd import _lib
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "rsa.h")).read()
    names = re.findall(r"^int (rsa_\w+)\(", header, re.M)
    want = ["rsa_block_select_antidiag_bytes", "rsa_block_select_antidiag", "rsa_block_select_observed_bytes",
            "rsa_block_select_observed"]
    for seq in (names, list(_lib.EXPORTED)):
        i = seq.index(want[0])
        assert seq[i:i + 4] == want


def test_c_refusals():
    from rectified_spaattn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librsa_hip.so is not built")
    L = _lib.lib()
    OK, BAD, UNSUP, WS = 0, -1, -2, -3
    n = ctypes.c_size_t(0)
    size = dict(B=2, H=4, Hkv=2, Hl=2, W=17, D=64, block=128, NQ=1, NK=3)
    assert L.rsa_block_select_observed_bytes(*size.values(), ctypes.byref(n)) == OK
    assert n.value == 2 * 2 * 3 * 4 + 2 * 4 * (3 + 1) * 17 * 2 * 4      # the keys (48 bytes), the pairs, the row statistics
    for kw, want in ((dict(D=32), UNSUP), (dict(block=32), UNSUP), (dict(NK=8193), UNSUP), (dict(NQ=2), BAD), (dict(W=65), BAD),
                     (dict(W=0), BAD), (dict(Hl=3), BAD), (dict(B=0), BAD)):
        assert L.rsa_block_select_observed_bytes(*dict(size, **kw).values(), ctypes.byref(n)) == want, kw
    t = _lib.RsaTensor4(256, 0, 0, 64)          # (never dereferenced: every call below is refused before the first HIP call)
    call = dict(B=2, H=4, Hkv=2, Hl=2, W=17, Sk=300, D=64, dtype=0, block=128, NQ=1, NK=3, q=t, k=t, table=None, tsb=0, pages=0,
                kv_len=None, kv_valid=300, causal=1, sm_scale=0.125, top_k=2, keep_first=0, keep_local=0, splits=0, ws=256,
                ws_bytes=16, bitmask=256, cols=256, counts=256, scores=None, p16=-1, c=0.0, mass=None, stream=None)
    for kw, want in ((dict(), WS), (dict(D=32), UNSUP), (dict(sm_scale=0.0), BAD), (dict(sm_scale=float("nan")), BAD),
                     (dict(p16=70000), BAD), (dict(B=0), BAD), (dict(block=32), UNSUP), (dict(kv_valid=301), BAD), (dict(ws=None), BAD),
                     (dict(k=_lib.RsaTensor4(None, 0, 0, 64)), BAD), (dict(cols=None), BAD), (dict(NK=4), BAD), (dict(W=65), BAD),
                     (dict(splits=257), BAD), (dict(table=256, pages=0), BAD), (dict(table=258, pages=4), BAD)):
        assert L.rsa_block_select_observed(*dict(call, **kw).values()) == want, kw
