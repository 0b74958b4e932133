"""The one plan behind rsa_block_sparse_decode_bytes, rsa_block_sparse_extend_bytes and rsa_block_sparse_extend_packed_bytes against
its Python mirrors (extend_row_groups, packed_row_groups, extend_default_split), over a grid that crosses every branch of it, and
the status of every refusal.  Host code only: no device is touched."""
import ctypes
import itertools
import os

import pytest

from rectified_spaattn_amd import _lib
from rectified_spaattn_amd.block_sparse import extend_default_split, extend_row_groups, packed_row_groups

OK, BAD, UNS = 0, -1, -2
NK, D = 11, 128
HEADS = ((2, 2, 2), (1, 1, 1), (128, 2, 2), (64, 1, 1), (130, 2, 1), (65, 1, 1))    # (H, Hkv, Hl): gu = 1, 1, 64, 64, 65, 65
SPLITS = (0, 1, NK + 3)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librsa_hip.so is not built")
    return _lib.lib()


def _rows16(rows):
    return 16 if rows <= 16 else (32 if rows <= 32 else 64)


def _partials(groups, C, rows16, d=D):
    return groups * -(-NK // C) * rows16 * (d + 2) * 4


def test_decode_bytes_is_one_group_per_unit(L):
    n = ctypes.c_size_t(0)
    for (H, Hkv, Hl), Sq, B, bps in itertools.product(HEADS, (1, 63, 64, 65), (1, 200), SPLITS):
        U, gu = max(Hl, Hkv), H // max(Hl, Hkv)
        st = L.rsa_block_sparse_decode_bytes(B, H, Hkv, Hl, Sq, D, NK, bps, ctypes.byref(n))
        if Sq * gu > 64:        # a unit's rows fill at most four row tiles
            assert st == UNS, (H, Hkv, Hl, Sq)
            continue
        assert st == OK, (H, Hkv, Hl, Sq, B, bps)
        C = min(bps, NK) if bps else min(8, NK)     # (decode splits whatever the number of units)
        assert n.value == _partials(B * U, C, _rows16(Sq * gu)), (H, Hkv, Hl, Sq, B, bps)


@pytest.mark.parametrize("blk", (64, 128))
def test_extend_bytes_follows_the_row_groups(L, blk):
    n = ctypes.c_size_t(0)
    seen = set()
    for (H, Hkv, Hl), Sq, B, bps in itertools.product(HEADS, (1, blk - 1, blk, blk + 1), (1, 200), SPLITS):
        g = extend_row_groups(B, H, Hkv, Hl, Sq, blk)
        assert L.rsa_block_sparse_extend_bytes(B, H, Hkv, Hl, Sq, D, blk, NK, bps, ctypes.byref(n)) == OK
        C = min(bps, NK) if bps else extend_default_split(g["groups"], NK)
        assert n.value == _partials(g["groups"], C, g["rows16"]), (H, Hkv, Hl, Sq, B, bps)
        seen.add((g["head_chunks"], g["groups"] < 256))
    assert seen == {(1, True), (1, False), (2, True), (2, False)}       # both head-chunk counts on both sides of the fill


@pytest.mark.parametrize("blk", (64, 128))
def test_packed_bytes_follows_the_piece_bound(L, blk):
    n, p = ctypes.c_size_t(0), ctypes.c_int64(0)
    seen = set()
    for (H, Hkv, Hl), M, bps in itertools.product(HEADS, (1, blk - 1, blk, blk + 1), SPLITS):
        for T, B in ((M + 1, M + 4), (3 * M + 7, 3), (200 * M + 1, 200)):      # T < B; T > B * M, few and many row groups
            g = packed_row_groups(T, B, H, Hkv, Hl, M, blk)
            st = L.rsa_block_sparse_extend_packed_bytes(T, B, H, Hkv, Hl, M, D, blk, NK, bps, ctypes.byref(n), ctypes.byref(p))
            assert st == OK and p.value == g["pieces"], (H, Hkv, Hl, M, T, B)
            C = min(bps, NK) if bps else extend_default_split(g["groups"], NK)
            head = (2 * (B + 1) * 4 + 15) // 16 * 16
            assert n.value == head + _partials(g["groups"], C, g["rows16"]), (H, Hkv, Hl, M, T, B, bps)
            seen.add((T < B, g["groups"] < 256))
    assert {(True, True), (False, True), (False, False)} <= seen


def test_refusals_keep_their_status_and_their_order(L):
    n, p = ctypes.c_size_t(0), ctypes.c_int64(0)
    good = dict(B=4, H=8, Hkv=2, Hl=2, Sq=8, D=128, blk=128, NK=6, bps=0)

    def dec(**kw):
        a = dict(good, **kw)
        return L.rsa_block_sparse_decode_bytes(a["B"], a["H"], a["Hkv"], a["Hl"], a["Sq"], a["D"], a["NK"], a["bps"], ctypes.byref(n))

    def ext(**kw):
        a = dict(good, **kw)
        return L.rsa_block_sparse_extend_bytes(a["B"], a["H"], a["Hkv"], a["Hl"], a["Sq"], a["D"], a["blk"], a["NK"], a["bps"],
                                               ctypes.byref(n))

    def pk(T=300, **kw):
        a = dict(good, **kw)
        return L.rsa_block_sparse_extend_packed_bytes(T, a["B"], a["H"], a["Hkv"], a["Hl"], a["Sq"], a["D"], a["blk"], a["NK"],
                                                      a["bps"], ctypes.byref(n), ctypes.byref(p))

    for call in (dec, ext, pk):
        assert call() == OK
        assert call(H=7) == BAD                 # H % Hkv
        assert call(Hl=4) == BAD                # a list head count that is neither 1, Hkv nor H
        assert call(NK=8193) == BAD
        assert call(D=96) == UNS
        assert call(bps=-1) == BAD
        assert call(B=0) == BAD and call(Sq=0) == BAD and call(NK=0) == BAD
        assert call(D=96, NK=8193) == BAD       # wrong in two ways: the argument before the shape
        assert call(D=96, H=7) == BAD
    for call in (ext, pk):
        assert call(blk=32) == UNS
        assert call(blk=32, D=96) == UNS and call(blk=32, NK=8193) == BAD
    assert dec(Sq=33) == UNS                    # 33 rows x 2 heads of a unit: more than 64
    assert dec(Sq=33, D=96) == UNS and dec(Sq=33, NK=8193) == BAD
    assert pk(T=7) == BAD and pk(T=0) == BAD    # M = 8 > T
    assert pk(T=7, D=96) == BAD and pk(T=7, blk=32) == BAD
    assert L.rsa_block_sparse_decode_bytes(4, 8, 2, 2, 8, 128, 6, 0, None) == BAD
    assert L.rsa_block_sparse_extend_bytes(4, 8, 2, 2, 8, 128, 128, 6, 0, None) == BAD
    assert L.rsa_block_sparse_extend_packed_bytes(300, 4, 8, 2, 2, 8, 128, 128, 6, 0, None, None) == BAD
    assert L.rsa_block_sparse_extend_packed_bytes(300, 4, 8, 2, 2, 8, 128, 128, 6, 0, ctypes.byref(n), None) == OK
