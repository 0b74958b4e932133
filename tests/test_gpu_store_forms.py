"""Both store forms of the 2-byte K5 kernels write the same bytes.

The rectified store of an output tile (rsa_attn.h::rsa_out_tile) has two forms: 16-byte stores after a lane regroup when the
output rows are 16-byte aligned -- what every contiguous [B, S, H, D] output of the package gets -- and 8-byte stores otherwise.
Here each call runs twice: into its own contiguous output, then into a view of a larger buffer that starts 8 bytes past a
16-byte boundary with strides that are multiples of 4 but not of 8 elements, which only the 8-byte form can serve.  The two
outputs must agree bit for bit, and nothing outside the view may be touched."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.0   # exact in bf16 and fp16, and not the zero a padded text row is stored as


def misaligned_view(B, S, H, D, dtype):
    """A [B, S, H, D] view, 4 elements into a sentinel-filled buffer, every stride above the head dim 4 (mod 8) elements; also
    the buffer and the mask of its elements outside the view."""
    sh, ss = D + 4, H * (D + 4) + 4
    sb = S * ss + 4
    assert all(x % 8 == 4 for x in (sh, ss, sb))
    buf = torch.full((4 + B * sb + 4,), SENTINEL, dtype=dtype, device=DEV)
    view = buf.as_strided((B, S, H, D), (sb, ss, sh, 1), 4)
    assert view.data_ptr() % 16 == 8
    outside = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
    outside.as_strided((B, S, H, D), (sb, ss, sh, 1), 4).fill_(False)
    return view, buf, outside


def assert_same_bytes_and_untouched(wide, view, buf, outside):
    assert torch.equal(view.view(torch.int16), wide.view(torch.int16))
    assert bool((buf[outside] == SENTINEL).all())


@pytest.fixture(scope="module")
def qkv():
    from rectified_spaattn_amd import synth
    made = {}

    def get(D):
        if D not in made:
            made[D] = tuple(torch.from_numpy(x).to(DEV) for x in synth.structured_qkv(6, 1, 2, 1280, D))
        return made[D]
    return get


@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("block", [128, 64])
def test_sparse_store_forms_agree(qkv, block, dtype, D):
    """HunyuanVideo layout with rectified visual rows, text rows and padded text rows (stored as zeros); 128-token blocks run the
    64-row kernel, 64-token blocks the 32-row kernel."""
    from rectified_spaattn_amd import _core, _lib, synth
    q, k, v = (x.to(dtype) for x in qkv(D))
    spec = _core.LayoutSpec.hunyuan(1280, 1224, block=block)
    nbr = torch.from_numpy(synth.banded_neighbors(spec.NBv, 1))
    call = _core.StagedCall(q, k, v, spec, 2, 0.3, nbr)
    call.select()
    wide = call.attend().clone()
    assert call.out.data_ptr() % 16 == 0
    assert bool((wide[:, 1224:] == 0).all()) and bool((wide[:, :1224] != 0).any())
    view, buf, outside = misaligned_view(1, 1280, 2, D, dtype)
    call.out = view
    call.o4 = _lib.RsaOut4(view.data_ptr(), view.stride(0), view.stride(2), view.stride(1))
    call.attend()
    assert_same_bytes_and_untouched(wide, view, buf, outside)


def test_dense_store_forms_agree():
    """A dense call whose last query tile is partial (300 rows: the 256-row tiles of the 64-row kernel)."""
    from rectified_spaattn_amd import _core, _lib
    L = _lib.lib()
    B, H, S, D = 1, 2, 300, 128
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn(B, H, S, D, generator=g).to(DEV, torch.bfloat16) for _ in range(3))

    def run(out):
        o4 = _lib.RsaOut4(out.data_ptr(), out.stride(0), out.stride(2), out.stride(1))
        _lib.check(L.rsa_dense_fwd(B, H, S, S, D, 0, _core._t4(q), _core._t4(k), _core._t4(v), S, S, o4, _core._stream()),
                   "rsa_dense_fwd")

    wide = torch.full((B, S, H, D), SENTINEL, dtype=torch.bfloat16, device=DEV)
    run(wide)
    assert bool((wide != SENTINEL).any())
    view, buf, outside = misaligned_view(B, S, H, D, torch.bfloat16)
    run(view)
    assert_same_bytes_and_untouched(wide, view, buf, outside)
