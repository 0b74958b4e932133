"""Block-sparse attention over caller-supplied block masks, and the reference's two building blocks on top of it.

The reference composes its operator from `_build_block_index_with_importance_optimized` (the selection: one-hot block mask,
implicit full-attention probabilities, GAPR mask) and `_triton_block_sparse_attention_onehot` (plain block-sparse attention over
any boolean block mask), rectified_hunyuan_attn.py:108-280 and the same in the flux / cogvideo / wan21 files.  Here:

    block_sparse_attention   K5 without the rectifying epilogue (rsa_block_sparse_plain_fwd) over the lists
                             rsa_block_mask_to_lists makes from the caller's mask; with causal= / window= / row_range= a key
                             range per query row on top of the mask (rsa_block_sparse_ranged_fwd, one launch per batch)
                             k / v may hold fewer heads than q (GQA / MQA: query head h reads K/V head h // (H // Hkv)) and
                             the mask one row per K/V head: rsa_block_sparse_gqa_fwd, no repeated K/V and no repeated lists
    block_sparse_decode      the decode half: a few query rows (one query block) over a contiguous or PAGED K/V cache, split over
                             the kept list and merged, with an optional log-sum-exp (rsa_block_sparse_decode, kernels of its own)
    select_blocks            a selection of the library's own for that call: pooled scores and a plain top-k per K/V head, with
                             the call's kv_len and causal alignment, written as lists on the device (rsa_block_select)
    pool_keys                the cache of pooled keys of that selection, made once and updated block by block as the K/V cache
                             grows, directly or through a block table (rsa_pool_keys)
    select_blocks_pooled     select_blocks from that cache instead of K: the same bytes without a pass over K
                             (rsa_block_select_pooled)
    pool_key_bounds          the cache of per-channel key minima and maxima, pool_keys' twin with its argument contract
                             (rsa_pool_key_bounds)
    select_blocks_bound      select_blocks_pooled from that cache: a block scores by the upper bound of q . k over its keys
                             (rsa_block_select_bound), everything behind the score unchanged
    append_kv_e4m3           the writer of a one-byte K/V cache: new rows become e4m3 codes under one static fp32 scale per K/V
                             head (rsa_kv8_append); block_sparse_decode and pool_keys read such a cache in place
                             (k_scale= / v_scale=: rsa_block_sparse_decode_kv8, rsa_pool_keys_kv8)
    merge_partials           the merge of N (out, lse) partials of block_sparse_decode / block_sparse_extend over disjoint key sets,
                             with optional sink logits: one launch, no copy (rsa_merge_partials)
    block_sparse_attention_backward   dq, dk, dv of block_sparse_attention (mask, kv_len, causal, GQA): row statistics recomputed,
                             two sweeps, no float atomics (rsa_block_sparse_bwd), and
                             block_sparse_attention_autograd, the torch.autograd.Function over the two
    build_block_index        K1..K3 of the rectified call (pooling, pooled scores + GAPR, selection), then
                             rsa_lists_to_block_mask for the reference's dense one-hot form

The calls above build_block_index share one argument layer, below _mask_u8: _check_operands (ranks, head counts, shapes, the
one 2-byte dtype, the head dims a call serves), _check_limit / _device_limit (kv_len and start: host ints, or a device tensor that
is never read on the host), _check_block_table / _table_args, _check_cache (a cache is not copied: the negation of what
_core._as_bhsd copies), _empty_lists and _out4.  Every check runs on CPU tensors, before _core._require_device.  select_blocks and
select_blocks_pooled are one body (_select); every K5 launch of block_sparse_attention, with ranges or without, grouped or not,
leaves from _k5_launch.

Difference from the reference kept on purpose: a query row that sees no key (no kept block, or every kept key at or beyond
kv_len) is 0 here; the reference's Triton kernel divides 0 by 0 there and returns NaN.  In the rectified call over a caller's mask
(the variants' block_mask=) such a visual row therefore comes out as comp alone, 0 * R + comp."""
from __future__ import annotations

import ctypes
import math
from types import SimpleNamespace
from typing import Dict, Optional

import torch

from . import _core, _lib
from ._lib import RsaOut4, RsaTensor4


def _check_block_pair(block_size_M: int, block_size_N: int) -> int:
    if block_size_M != block_size_N or block_size_M not in _lib.BLOCKS:
        raise NotImplementedError(f"block-sparse attention on the HIP path: block_size_M = block_size_N in {_lib.BLOCKS}, "
                                  f"got {block_size_M} / {block_size_N}")
    return int(block_size_M)


MAX_KEY_BLOCKS = 8192   # K5's key-block limit (its kept list lives in LDS as u16)


def _mask_u8(block_mask: torch.Tensor) -> torch.Tensor:
    """bool / uint8 mask with a contiguous key axis, as uint8 bytes (a bool tensor is reinterpreted, not copied)."""
    m = block_mask
    if m.stride(-1) != 1 and m.shape[-1] > 1:
        m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


# ---- the argument layer of the five public calls: every check below runs on CPU tensors, before the device is asked for ----------
HEAD_DIMS = (16, 32, 64, 128)


def _check_block(what: str, block_size) -> int:
    if block_size not in _lib.BLOCKS:
        raise NotImplementedError(f"{what} on the HIP path: block_size in {_lib.BLOCKS}, got {block_size}")
    return int(block_size)


def _check_count(name: str, val, lo: int, hi: Optional[int] = None, optional: bool = False):
    """An int option in [lo, hi] (bool is refused); with optional, None passes."""
    if val is None and optional:
        return
    if not isinstance(val, int) or isinstance(val, bool) or val < lo or (hi is not None and val > hi):
        raise ValueError(f"{name}: {'None or ' if optional else ''}an int {f'in {lo}..{hi}' if hi is not None else f'>= {lo}'}, "
                         f"got {val!r}")


def _key_blocks(Sk: int, blk: int) -> int:
    NK = -(-Sk // blk)
    if NK > MAX_KEY_BLOCKS:
        raise ValueError(f"Sk = {Sk} is {NK} key blocks of {blk}: at most {MAX_KEY_BLOCKS}")
    return NK


def _check_block_table(block_table, B: Optional[int] = None):
    """int32 [B, NKt] (B: q's batch; None: the table gives it) -> its shape."""
    ok = isinstance(block_table, torch.Tensor) and block_table.dtype == torch.int32 and block_table.dim() == 2
    if not ok or block_table.shape[1] < 1 or (block_table.shape[0] < 1 if B is None else block_table.shape[0] != B):
        raise ValueError(f"block_table: an int32 tensor [{'B' if B is None else B}, NKt], got "
                         f"{getattr(block_table, 'dtype', type(block_table))} {tuple(getattr(block_table, 'shape', ()))}")
    return block_table.shape


def _table_args(block_table, pool):
    """The C entries' (block_table, table_stride_b, num_pages) of a device table over the page pool, or of no table; and the
    table they point into, for the caller to hold until the launch."""
    if block_table is None:
        return (None, 0, 0), None
    _core._require_device(block_table)
    table = block_table if block_table.stride(1) == 1 else block_table.contiguous()
    return (table.data_ptr(), table.stride(0), pool.shape[0]), table


E4M3 = torch.float8_e4m3fn
KV8_HEAD_DIMS = (64, 128)


def _check_operands(q, k, v=None, *, dims=HEAD_DIMS, block_table=None, blk: int = 0, pooled: bool = False, kv8_ok: bool = False,
                    bounds: bool = False):
    """The tensor operands a call takes -> (B, H, Hkv, Sq, Sk, D).  q [B,H,Sq,D] or None (pool_keys: B from k, H = Hkv, Sq = 1);
    k [B,Hkv,Sk,D], or with a block_table [B, NKt] a page pool [P,Hkv,blk,D] of capacity Sk = NKt * blk, or with pooled the
    fp32 cache [B,Hkv,NK,D] of pool_keys (Sk is then NK); v like k, or None.  One 2-byte dtype -- or, where the call serves it
    (kv8_ok), k and v both float8_e4m3fn beside a 2-byte q; D among dims, the head dims the call serves (another of HEAD_DIMS is
    NotImplementedError); nothing empty.  bounds (beside pooled): k is the fp32 cache [B,Hkv,NK,2,D] of pool_key_bounds, held
    whole to that form here and read below as the [B,Hkv,NK,D] of its minima."""
    kname = "key_bounds" if bounds else "pooled_k" if pooled else "k"
    if bounds:
        if (not isinstance(k, torch.Tensor) or k.dim() != 5 or k.shape[3] != 2 or k.dtype != torch.float32
                or not k.is_contiguous()):
            raise ValueError(f"key_bounds: a contiguous float32 tensor [B, Hkv, NK, 2, D] (pool_key_bounds' result; the 4-d cache "
                             f"[B, Hkv, NK, D] of pool_keys belongs to select_blocks_pooled), got "
                             f"{getattr(k, 'dtype', type(k))} {tuple(getattr(k, 'shape', ()))}, strides "
                             f"{tuple(k.stride()) if isinstance(k, torch.Tensor) else ()}")
        k = k[:, :, :, 0]
    for t in (q, k, v):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dim() != 4):
            raise ValueError(f"{_names(q, kname, v)}: 4-d tensors -- q [B, H, Sq, D], k / v [B, Hkv, Sk, D] or with block_table "
                             "page pools [P, Hkv, block_size, D], pooled_k [B, Hkv, NK, D] (the 5-d cache [B, Hkv, NK, 2, D] of "
                             "pool_key_bounds belongs to select_blocks_bound)")
    kB, Hkv, Sk, kD = k.shape
    B, H, Sq, D = (kB, Hkv, 1, kD) if q is None else q.shape
    if v is not None and v.shape[1] != Hkv:
        raise ValueError(f"k has Hkv = {Hkv} heads, v {v.shape[1]}: k and v must hold the same K/V heads")
    if q is not None and (Hkv <= 0 or H % Hkv):
        raise ValueError(f"Hkv = {Hkv} K/V heads do not divide the {H} query heads (query head h uses K/V head h // (H // Hkv))")
    if block_table is not None:
        fits = Sk == blk
        B, NKt = _check_block_table(block_table, None if q is None else B)
        Sk = NKt * blk
    else:
        fits = kB == B
    if not fits or kD != D or (v is not None and v.shape != k.shape):
        raise ValueError(f"{kname} {tuple(k.shape)}{'' if v is None else f' / v {tuple(v.shape)}'} does not match"
                         f"{'' if q is None else f' q {tuple(q.shape)}'}"
                         + (f": with a block_table k / v are page pools [P, Hkv, {blk}, {D}]" if block_table is not None else ""))
    dt = k.dtype if q is None else q.dtype
    if kv8_ok and not pooled and E4M3 in (k.dtype, getattr(v, "dtype", None)):
        if k.dtype != E4M3 or (v is not None and v.dtype != E4M3) or (q is not None and dt not in (torch.bfloat16, torch.float16)):
            raise ValueError(f"{_names(q, kname, v)}: an e4m3 cache is k and v both float8_e4m3fn beside a bfloat16 / float16 q, got "
                             f"{', '.join(str(t.dtype) for t in (q, k, v) if t is not None)}")
        if D not in KV8_HEAD_DIMS:
            if D in HEAD_DIMS:
                raise NotImplementedError(f"head dim {D}: an e4m3 cache serves {KV8_HEAD_DIMS}")
            raise ValueError(f"head dim {D}: one of {KV8_HEAD_DIMS}")
    elif dt not in (torch.bfloat16, torch.float16) or (not pooled and k.dtype != dt) or (v is not None and v.dtype != dt):
        raise ValueError(f"{_names(q, kname, v)}: one dtype, bfloat16 or float16 (pooled_k apart), got "
                         f"{', '.join(str(t.dtype) for t in (q, k, v) if t is not None)}")
    if pooled and not bounds and (k.dtype != torch.float32 or not k.is_contiguous()):
        raise ValueError(f"pooled_k: a contiguous float32 tensor (pool_keys' result), got dtype {k.dtype}, "
                         f"strides {tuple(k.stride())}")
    if D not in dims:
        if D in HEAD_DIMS:
            raise NotImplementedError(f"head dim {D}: this call serves {dims} (padding a cache would copy it)")
        raise ValueError(f"head dim {D}: one of {dims}")
    if B <= 0 or Hkv <= 0 or Sq <= 0 or Sk <= 0:
        raise ValueError(f"empty operands (B = {B}, Hkv = {Hkv}, Sq = {Sq}, {'NK' if pooled else 'Sk'} = {Sk})")
    return B, H, Hkv, Sq, Sk, D


def _names(q, kname: str, v) -> str:
    return ", ".join(n for n, t in (("q", q), (kname, True), ("v", v)) if t is not None)


def _check_cache(k, v=None):
    """A K/V cache is read where it lies: what _core._as_bhsd would copy is refused.  An e4m3 cache: K is loaded 8 bytes a lane,
    V 16 -- pointer and strides are multiples of that."""
    for name, t, align in (("k", k, 8), ("v", v, 16)):
        if t is not None and t.dtype == E4M3:
            *outer, inner = t.stride()
            if inner != 1 or any(st % align for st in outer) or t.data_ptr() % align:
                raise ValueError(f"{name}: a contiguous head dim, strides that are multiples of {align} bytes and a {align}-byte "
                                 f"aligned pointer (a cache is not copied), got strides {tuple(t.stride())}, pointer % {align} = "
                                 f"{t.data_ptr() % align}")
    if k.dtype == E4M3:
        return
    for name, t in (("k", k), ("v", v)):
        if t is not None and not _core._read_in_place(t):
            raise ValueError(f"{name}: a contiguous head dim, strides that are multiples of 8 elements and a 16-byte aligned "
                             f"pointer (a cache is not copied), got strides {tuple(t.stride())}, pointer % 16 = {t.data_ptr() % 16}")


def _check_limit(name: str, val, B: int, Sk: int, default: int, device_ok: bool = True):
    """A key limit (kv_len, start): None (= default) | int | per-batch sequence | host tensor (one host read) -> list of B ints
    in [0, Sk].  A device tensor is checked and passed on unread -- or, where the call has no device form (device_ok False),
    read like a host tensor."""
    if device_ok and isinstance(val, torch.Tensor) and val.is_cuda:
        if val.numel() not in (1, B) or val.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{name}: an int32 / int64 tensor of 1 or {B} values, got {val.dtype} {tuple(val.shape)}")
        return val
    if val is None:
        lens = [default] * B
    elif isinstance(val, int):
        lens = [int(val)] * B
    else:
        vals = val.reshape(-1).tolist() if isinstance(val, torch.Tensor) else list(val)
        if len(vals) == 1:
            vals = vals * B
        if len(vals) != B:
            raise ValueError(f"{name}: {len(vals)} values for a batch of {B}")
        lens = [int(x) for x in vals]
    if any(n < 0 or n > Sk for n in lens):
        raise ValueError(f"{name} {lens} outside [0, {Sk}]")
    return lens


def _device_limit(val, B: int, Sk: int, dev):
    """What _check_limit returned, for the C entries: (device int32 [B] | None, host int, host list | None).  A device tensor is
    clamped into [0, Sk] on the device and never read on the host."""
    if isinstance(val, torch.Tensor):
        return val.to(dev).reshape(-1).clamp(0, Sk).to(torch.int32).expand(B).contiguous(), Sk, None
    if len(set(val)) == 1:
        return None, val[0], val
    return torch.tensor(val, dtype=torch.int32, device=dev), Sk, val


def _row_limit(val, B: int, Sq: int, dev):
    """q_len as _check_limit("q_len", ...) returned it, for the ragged C entries: DEVICE int32 [B], or None where every item has
    Sq rows (None, or host values that all equal Sq: the existing entries).  A device tensor is never read on the host."""
    if isinstance(val, list) and all(n == Sq for n in val):
        return None
    q_dev, q_host, _ = _device_limit(val, B, Sq, dev)
    return torch.full((B,), q_host, dtype=torch.int32, device=dev) if q_dev is None else q_dev


def _packed_view(name: str, x, cu, keys, block_table):
    """The packed form of a call: x [T, H, D] beside cu (cu_seqlens_q / cu_seqlens) -> (the [B, H, T, D]
    view of x with batch stride 0 that _check_operands reads, B).  x is 3-d if and only if cu is given; B, the number of items,
    comes from the block table, else from the cache (k, the pooled keys) -- the lists and kv_len are then held to it."""
    if cu is None:          # (a 3-d tensor without cu_seqlens is refused by _check_operands, in its own words)
        return x, None
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError(f"{name}: a packed [T, H, D] tensor if and only if its cu_seqlens is given (a padded [B, H, S, D] one "
                         f"otherwise), got {tuple(getattr(x, 'shape', ()))} with cu_seqlens")
    if isinstance(block_table, torch.Tensor) and block_table.dim() == 2:
        B = block_table.shape[0]
    elif isinstance(keys, torch.Tensor) and keys.dim() in (4, 5):       # (5: the bounds cache [B, Hkv, NK, 2, D])
        B = keys.shape[0]
    else:
        raise ValueError("packed call: the number of items comes from block_table [B, NKt] or from the cache [B, Hkv, Sk, D]")
    if B < 1 or x.shape[0] < 1:
        raise ValueError(f"empty operands (B = {B}, T = {x.shape[0]})")
    return x.permute(1, 0, 2).unsqueeze(0).expand(B, -1, -1, -1), B


def _check_packed(name: str, cu, max_len, B: int, T: int, need_max: bool = True):
    """cu_seqlens_q (or the append's cu_seqlens) and max_q_len of a packed call -> (the int32 [B + 1] tensor, M).  The values of cu
    are never read on the host: the device sanitises them.  M: a host int in [1, T] (flash-attn's max_seqlen_q)."""
    if not isinstance(cu, torch.Tensor) or cu.dtype != torch.int32 or cu.numel() != B + 1:
        raise ValueError(f"{name}: a device int32 tensor of B + 1 = {B + 1} values, got {getattr(cu, 'dtype', type(cu))} "
                         f"{tuple(getattr(cu, 'shape', ()))}")
    if need_max:
        if not isinstance(max_len, int) or isinstance(max_len, bool) or not 1 <= max_len <= T:
            raise ValueError(f"max_q_len: an int in 1..T = {T} (the rows of the longest item; required with {name}), got {max_len!r}")
    elif max_len is not None:
        raise ValueError(f"max_q_len belongs to {name}")
    return cu.reshape(-1), (int(max_len) if need_max else T)


def _query_rows(q, q_len, cu_seqlens_q, max_q_len, keys, block_table, check_operands):
    """Where a call's query rows come from, for _select and _sparse_rows: "padded" (q [B, H, Sq, D]), "counted" (with q_len) or "packed"
    (q [T, H, D], cu_seqlens_q, max_q_len).  -> the kind, q as a 4-d view (q4; q3: the caller's tensor), the
    shapes of check_operands(q4), the caller's _check_operands call (Sq is M = max_q_len when packed), T and the checked cu."""
    q4, Bp = _packed_view("q", q, cu_seqlens_q, keys, block_table)
    if Bp is not None and q_len is not None:
        raise ValueError("q_len belongs to a padded q: with cu_seqlens_q the rows of an item are cu_seqlens_q[b + 1] - cu_seqlens_q[b]")
    if Bp is None and max_q_len is not None:
        raise ValueError("max_q_len belongs to cu_seqlens_q")
    B, H, Hkv, Sq, Sk, D = check_operands(q4)
    T = cu = None
    if Bp is not None:      # T: the rows of q; Sq is M from here on, the rows of an item at most
        T, (cu, Sq) = Sq, _check_packed("cu_seqlens_q", cu_seqlens_q, max_q_len, B, Sq)
    kind = "packed" if Bp is not None else "counted" if q_len is not None else "padded"
    return SimpleNamespace(kind=kind, q4=q4, q3=q, B=B, H=H, Hkv=Hkv, Sq=Sq, Sk=Sk, D=D, T=T, cu=cu)


def _packed_on_device(r):      # what a packed call holds: q [T, H, D] as the kernels read it and cu_seqlens_q, contiguous
    _core._require_device(r.cu)
    return (r.q3 if _core._read_in_place(r.q3) else r.q3.contiguous()), r.cu.contiguous()


def _t3(t: torch.Tensor) -> RsaTensor4:
    """A packed [T, H, D] tensor as the packed C entries read it: stride_s the row's, stride_h the head's, stride_b unread."""
    return RsaTensor4(t.data_ptr(), 0, t.stride(1), t.stride(0))


def _check_scales(k, Hkv: int, **scales):
    """k_scale= / v_scale= of a call over the cache k: required with an e4m3 cache, refused with a 2-byte one.  A scale is a
    positive finite Python float or a float32 tensor of 1 or Hkv values on the cache's device (its values are not read)."""
    if k.dtype != E4M3:
        given = [n for n, s in scales.items() if s is not None]
        if given:
            raise ValueError(f"{', '.join(given)}: scales belong to a float8_e4m3fn cache, k is {k.dtype}")
        return
    for name, sc in scales.items():
        if sc is None:
            raise ValueError(f"{name}: required with a float8_e4m3fn cache (one fp32 scale per K/V head, or one for all)")
        if isinstance(sc, torch.Tensor):
            if sc.dtype != torch.float32 or sc.numel() not in (1, Hkv):
                raise ValueError(f"{name}: a float32 tensor of 1 or {Hkv} values, got {sc.dtype} {tuple(sc.shape)}")
            if sc.device != k.device:
                raise ValueError(f"{name} is on {sc.device}, the cache on {k.device}")
        elif isinstance(sc, bool) or not isinstance(sc, (int, float)) or not 0.0 < float(sc) < float("inf"):
            raise ValueError(f"{name}: a positive finite float or a float32 tensor of 1 or {Hkv} values, got {sc!r}")


def _scale_arg(sc, Hkv: int, dev) -> torch.Tensor:
    """What _check_scales passed, as the C entries' DEVICE fp32 [Hkv]: a Python float is filled in by torch (capturable)."""
    if isinstance(sc, torch.Tensor):
        return sc.reshape(-1).expand(Hkv).contiguous()
    return torch.full((Hkv,), float(sc), dtype=torch.float32, device=dev)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _out4(t: torch.Tensor) -> RsaOut4:
    return RsaOut4(t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))


def _empty_lists(rows: int, NQ: int, NK: int, dev) -> Dict[str, torch.Tensor]:
    """Unwritten kept lists of rows list heads (the rsa_buffers format block_mask_to_lists describes)."""
    return dict(bitmask=torch.empty((rows, NQ, (NK + 31) // 32), dtype=torch.int32, device=dev),
                cols=torch.empty((rows, NQ, NK), dtype=torch.int32, device=dev),
                counts=torch.empty((rows, NQ), dtype=torch.int32, device=dev))


def block_mask_to_lists(block_mask: torch.Tensor, B: int, H: int) -> Dict[str, torch.Tensor]:
    """[B|1, H|1, NQ, NK] bool / uint8 device mask (nonzero = kept) -> K5's kept lists, the rsa_buffers format:
    bitmask int32 [B*H, NQ, ceil(NK/32)], cols int32 [B*H, NQ, NK] (ascending, first counts entries written), counts [B*H, NQ]."""
    if block_mask.dtype not in (torch.bool, torch.uint8) or block_mask.dim() != 4:
        raise ValueError(f"block_mask: a 4-d bool or uint8 tensor, got {block_mask.dtype} {tuple(block_mask.shape)}")
    if block_mask.shape[0] not in (1, B) or block_mask.shape[1] not in (1, H):
        raise ValueError(f"block_mask {tuple(block_mask.shape)} does not broadcast over B = {B}, H = {H}")
    if not 1 <= block_mask.shape[3] <= MAX_KEY_BLOCKS or block_mask.shape[2] < 1:
        raise ValueError(f"block_mask {tuple(block_mask.shape)}: 1..{MAX_KEY_BLOCKS} key blocks and at least one query block")
    _core._require_device(block_mask)
    m = _mask_u8(block_mask)
    NQ, NK = m.shape[2], m.shape[3]
    strides = [0 if m.shape[i] == 1 else m.stride(i) for i in range(3)]
    dev = m.device
    out = _empty_lists(B * H, NQ, NK, dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().rsa_block_mask_to_lists(B, H, NQ, NK, m.data_ptr(), *strides, out["bitmask"].data_ptr(),
                                                      out["cols"].data_ptr(), out["counts"].data_ptr(), _core._stream()),
                   "rsa_block_mask_to_lists")
    return out


def lists_to_block_mask(bitmask: torch.Tensor, B: int, H: int, NQ: int, NK: int) -> torch.Tensor:
    """bitmask words [B*H, NQ, ceil(NK/32)] -> uint8 [B, H, NQ, NK] of 0 / 1 (view it as bool for the reference's one-hot form)."""
    _core._require_device(bitmask)
    if bitmask.numel() != B * H * NQ * ((NK + 31) // 32) or not bitmask.is_contiguous():
        raise ValueError(f"bitmask {tuple(bitmask.shape)} is not a contiguous [{B * H}, {NQ}, {(NK + 31) // 32}] word array")
    out = torch.empty((B, H, NQ, NK), dtype=torch.uint8, device=bitmask.device)
    with torch.cuda.device(bitmask.device):
        _lib.check(_lib.lib().rsa_lists_to_block_mask(B, H, NQ, NK, bitmask.data_ptr(), out.data_ptr(), _core._stream()),
                   "rsa_lists_to_block_mask")
    return out


def gqa_kv_head(h: int, H: int, Hkv: int) -> int:
    """The K/V head query head h reads when k / v hold Hkv heads for H query heads: h // (H // Hkv), flash-attn's and torch's
    enable_gqa convention -- what k.repeat_interleave(H // Hkv, dim=1)[:, h] holds.  The same map takes h to its list head."""
    if H <= 0 or Hkv <= 0 or H % Hkv or not 0 <= h < H:
        raise ValueError(f"head {h} of H = {H} query heads over Hkv = {Hkv} heads: Hkv must divide H")
    return h // (H // Hkv)


def gqa_pairable(H: int, Hkv: int, Hl: int, block: int) -> bool:
    """Whether a grouped-query call can run two query heads per workgroup on one K/V ring (form (b)):
    128-token blocks, and heads 2p and 2p + 1 share both their K/V head (H // Hkv even) and their list row (H // Hl even, Hl = the
    mask's head axis).  Everything else runs one walk per query head (form (a)); so does every call unless the tuning key
    k5_gqa_pair is 1."""
    if min(H, Hkv, Hl) <= 0 or H % Hkv or H % Hl:
        raise ValueError(f"H = {H} query heads over Hkv = {Hkv} K/V heads and Hl = {Hl} list heads: both must divide H")
    return block == _lib.BLOCK and (H // Hkv) % 2 == 0 and (H // Hl) % 2 == 0


_TAIL_CACHE: "Dict[tuple, torch.Tensor]" = {}


def _tail_buffer(device) -> torch.Tensor:
    """The tail split's partial buffer ([RSA_TAIL_PIECES, 128, 130] fp32, 34 MB), one per (device, stream) and reused in stream
    order as _core.cached_buffers reuses the rectified call's (and like those, never during a HIP-graph capture)."""
    dev = torch.device(device)
    shape = (_lib.TAIL_PIECES, _lib.BLOCK, 128 + 2)
    if not _core.BUFFER_CACHE or torch.cuda.is_current_stream_capturing():
        return torch.empty(shape, dtype=torch.float32, device=dev)
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    buf = _TAIL_CACHE.get(key)
    if buf is None:
        buf = _TAIL_CACHE[key] = torch.empty(shape, dtype=torch.float32, device=dev)
    return buf


_RANGE_CACHE: "Dict[tuple, tuple]" = {}
_RANGE_CACHE_MAX = 64


def _check_window(window):
    if not isinstance(window, (tuple, list)) or len(window) != 2 or not all(isinstance(w, int) and w >= -1 for w in window):
        raise ValueError(f"window: (left, right), ints >= 0 or -1 for unbounded, got {window!r}")
    return int(window[0]), int(window[1])


def _check_row_range(row_range, B: int, Sq: int, device):
    """(lo | None, hi): int32 tensors [B|1, Sq] on q's device."""
    if not isinstance(row_range, (tuple, list)) or len(row_range) != 2:
        raise ValueError("row_range: a pair (lo | None, hi) of int32 tensors [B|1, Sq]")
    lo, hi = row_range
    if hi is None:
        raise ValueError("row_range: hi is required (lo may be None = 0)")
    for name, t in (("lo", lo), ("hi", hi)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
            raise ValueError(f"row_range {name}: an int32 tensor, got {getattr(t, 'dtype', type(t))}")
        if t.dim() != 2 or t.shape[0] not in (1, B) or t.shape[1] != Sq:
            raise ValueError(f"row_range {name} {tuple(t.shape)}: expected [{B}|1, {Sq}]")
        if t.device != device:
            raise ValueError(f"row_range {name} is on {t.device}, q on {device}")
    return lo, hi


def _window_ranges(device, B: int, Sq: int, Sk: int, lens, left: int, right: int):
    """lo (None: 0) and hi, int32 [B|1, Sq] on the device, of window (left, right) aligned bottom-right per batch item:
    lo = r + off_b - left, hi = r + off_b + right + 1 with off_b = kv_len[b] - Sq, hi folded with kv_len[b]; clipped into [0, Sk]
    (the kernel clamps into [0, kv_valid] anyway).  lens: a list of B host ints -- cached per (device, stream, Sq, lens, window)
    as _tail_buffer caches, never during a graph capture -- or an integer device tensor [B|1], which is never read on the host."""
    dev = torch.device(device)
    r = torch.arange(Sq, dtype=torch.int64, device=dev)

    def rows(off):    # off = kv_len - Sq: a host int (-> [Sq]) or a device tensor [n, 1] (-> [n, Sq])
        lo = None if left < 0 else (r + (off - left)).clamp(0, Sk).to(torch.int32)
        hi = r + (off + right + 1) if right >= 0 else r * 0 + (off + Sq)
        hi = hi.clamp(max=off + Sq) if isinstance(off, int) else torch.minimum(hi, off + Sq)
        return lo, hi.clamp(0, Sk).to(torch.int32)
    if isinstance(lens, torch.Tensor):
        return rows(lens.reshape(-1, 1).to(torch.int64) - Sq)
    capturing = torch.cuda.is_current_stream_capturing()
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, Sq, Sk, tuple(lens), left, right)
    if _core.BUFFER_CACHE and not capturing and key in _RANGE_CACHE:
        return _RANGE_CACHE[key]
    per = [rows(n - Sq) for n in (lens if len(set(lens)) > 1 else lens[:1])]
    lo = None if left < 0 else torch.stack([p[0] for p in per])
    out = (lo, torch.stack([p[1] for p in per]))
    if _core.BUFFER_CACHE and not capturing:
        if len(_RANGE_CACHE) >= _RANGE_CACHE_MAX:
            _RANGE_CACHE.pop(next(iter(_RANGE_CACHE)))
        _RANGE_CACHE[key] = out
    return out


def _k5_launch(q, k, v, block_mask, blk: int, scale: float, groups, lo=None, hi=None) -> torch.Tensor:
    """block_sparse_attention's launches.  groups: (b0, b1, key limit) runs of batch items, one launch each -- a call with
    ranges (hi given; lo None = 0; int32 [B|1, Sq]) has one for the whole batch.  The C entry: rsa_block_sparse_gqa_fwd iff k / v
    hold fewer heads than q, else rsa_block_sparse_ranged_fwd iff there are ranges, else rsa_block_sparse_plain_fwd."""
    B, H, Sq, D = q.shape
    if D in _core._PAD_HEAD_DIM:   # zero columns add exact zeros to every dot product; the caller's scale is kept
        pad = (0, _core._PAD_HEAD_DIM[D] - D)
        F = torch.nn.functional
        return _k5_launch(F.pad(q, pad), F.pad(k, pad), F.pad(v, pad), block_mask, blk, scale, groups, lo, hi)[..., :D].contiguous()
    Hkv, Sk = k.shape[1], k.shape[2]
    ranges = ()
    if hi is not None:
        if lo is not None and lo.shape[0] != hi.shape[0]:
            lo = lo.expand(hi.shape[0], Sq) if lo.shape[0] == 1 else lo
            hi = hi.expand(lo.shape[0], Sq) if hi.shape[0] == 1 else hi
        lo, hi = None if lo is None else lo.contiguous(), hi.contiguous()
        ranges = (_ptr(lo), hi.data_ptr(), 0 if hi.shape[0] == 1 else Sq)
    L = _lib.lib()
    q, k, v = _core._as_bhsd(q), _core._as_bhsd(k), _core._as_bhsd(v)
    NQ, NK = -(-Sq // blk), block_mask.shape[3]
    # list heads per batch item: H with as many K/V heads as query heads (a mask head axis of 1 is expanded); with fewer, the
    # mask's own head axis -- 1, Hkv or H -- so that shared lists are built and kept once
    Hl = H if Hkv == H else int(block_mask.shape[1])
    lists = block_mask_to_lists(block_mask, B, Hl)
    out = torch.empty((B, H, Sq, D), dtype=q.dtype, device=q.device)
    # the tail split's partial buffer (head dim 128, 128-token blocks: the rectified call's K5 gets the same)
    tpart = _tail_buffer(q.device) if D == 128 and blk == _lib.BLOCK else None
    tp, tpb = (tpart.data_ptr(), tpart.numel() * 4) if tpart is not None else (None, 0)
    dt = _core.dtype_code(q.dtype)
    if Hkv != H:
        entry, heads, ranges = "rsa_block_sparse_gqa_fwd", (H, Hkv, Hl), ranges or (None, None, 0)
    else:
        entry, heads = "rsa_block_sparse_ranged_fwd" if ranges else "rsa_block_sparse_plain_fwd", (H,)
    with torch.cuda.device(q.device):
        for b0, b1, n in groups:
            if n == 0:   # no visible key at all
                out[b0:b1].zero_()
                continue
            row = Hl * NQ * b0
            _lib.check(getattr(L, entry)(b1 - b0, *heads, Sq, Sk, D, dt, blk, NQ, NK, n, scale, _core._t4(q[b0:b1]),
                                         _core._t4(k[b0:b1]), _core._t4(v[b0:b1]), lists["cols"].data_ptr() + row * NK * 4,
                                         lists["counts"].data_ptr() + row * 4, *ranges, tp, tpb, _out4(out[b0:b1]),
                                         _core._stream()), entry)
    return out


def block_sparse_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, block_mask: torch.Tensor, *, kv_len=None,
                           sm_scale: Optional[float] = None, block_size: int = 128, causal: bool = False, window=None,
                           row_range=None) -> torch.Tensor:
    """softmax(sm_scale q k^T) v restricted, per query block i, to the key blocks j with block_mask[b, h, i, j] set and to the
    keys < kv_len.  q [B,H,Sq,D], k / v [B,H,Sk,D] or with fewer K/V heads (last paragraph); any strides with a contiguous head
    dim: [B,S,H,D] views need no copy;
    block_mask bool / uint8 [B|1, H|1, ceil(Sq/block), NK] with NK <= ceil(Sk/block) (keys past NK * block are never visited);
    kv_len None (= Sk), an int, or one value per batch item (a tensor costs one host read; distinct values run one launch per
    batch item); sm_scale defaults to D ** -0.5.  Returns [B,H,Sq,D] in the input dtype.  A row without a visible key is 0
    (the reference's kernel gives NaN there).  Asynchronous on the current stream.  Head dims 64 / 128 run natively, 16 / 32
    zero-padded (exact); bf16 and fp16.

    Per-row key ranges (at most one of the three; 128-token blocks only): row r of batch item b then sees key j iff
    block_mask[b, h, r // 128, j // 128] and lo[b, r] <= j < hi[b, r] and j < kv_len[b] and j < NK * 128.
      row_range=(lo | None, hi)   int32 device tensors [B|1, Sq]; any values (clamped into [0, kv_len[b]] on the device), hi <= lo
                                  is an empty row (0), the same ranges for every head, no order along the rows required
      window=(left, right)        flash-attn's sliding window, -1 = unbounded, aligned bottom-right per batch item:
                                  lo = r + off_b - left, hi = r + off_b + right + 1 with off_b = kv_len[b] - Sq
      causal=True                 window=(-1, 0)
    With a range the call is ONE launch for the whole batch whatever kv_len holds: host values are folded into hi, and a kv_len
    that is a device tensor is folded on the device and never read on the host.  Without one nothing changes.

    Grouped-query K/V heads (GQA; MQA with one): k / v [B,Hkv,Sk,D] with H % Hkv == 0.  Query head h reads K/V head
    h // (H // Hkv) -- flash-attn's and torch's enable_gqa convention, the result of k.repeat_interleave(H // Hkv, dim=1) without
    the g-fold K/V memory and traffic; q, k, v as head-strided views of one fused projection [B, S, (H + 2 Hkv) D] need no copy.
    The mask's head axis is then H (one row per query head), Hkv (one per K/V head, shared by its H // Hkv query heads: the lists
    are built once per K/V head) or 1.  Both block sizes; ranges with 128-token blocks as above.  With Hkv == H nothing changes.
    Only this call is grouped: triton_block_sparse_attention_onehot, build_block_index, the rectified_* calls and the fp8
    switches stay MHA-only (the selection statistics pool K per head, and the reference has no grouped form)."""
    blk = _check_block_pair(block_size, block_size)
    if int(bool(causal)) + (window is not None) + (row_range is not None) > 1:
        raise ValueError("causal, window and row_range exclude one another: give at most one")
    ranged = bool(causal) or window is not None or row_range is not None
    if ranged and blk != _lib.BLOCK:
        raise NotImplementedError(f"causal / window / row_range need block_size = {_lib.BLOCK}: 64-token blocks run the "
                                  "32-rows-per-wave kernel, which has one key limit per launch and no per-row range")
    if window is not None:
        window = _check_window(window)
    B, H, Hkv, Sq, Sk, D = _check_operands(q, k, v)
    NQ, NKmax = -(-Sq // blk), -(-Sk // blk)
    if block_mask.dim() != 4 or block_mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"block_mask: a 4-d bool or uint8 tensor, got {block_mask.dtype} {tuple(block_mask.shape)}")
    if Hkv != H and block_mask.shape[1] not in (1, Hkv, H):
        raise ValueError(f"block_mask {tuple(block_mask.shape)}: a head axis of {H} (per query head), Hkv = {Hkv} (per K/V head) "
                         "or 1")
    if (block_mask.shape[0] not in (1, B) or block_mask.shape[1] not in (1, Hkv, H) or block_mask.shape[2] != NQ
            or not 1 <= block_mask.shape[3] <= min(NKmax, MAX_KEY_BLOCKS)):
        raise ValueError(f"block_mask {tuple(block_mask.shape)}: expected [{B}|1, {H}|1, {NQ}, 1..{min(NKmax, MAX_KEY_BLOCKS)}] "
                         f"for block {blk} (at most {MAX_KEY_BLOCKS} key blocks)")
    if row_range is not None:
        row_range = _check_row_range(row_range, B, Sq, q.device)
    # with a range a device kv_len is folded on the device and not read; without one every kv_len becomes host ints
    lens = _check_limit("kv_len", kv_len, B, Sk, Sk, device_ok=ranged)
    _core._require_device(q, k, v)
    scale = float(D) ** -0.5 if sm_scale is None else float(sm_scale)
    if block_mask.device != q.device:
        block_mask = block_mask.to(q.device)
    if not ranged:   # one launch for the whole batch when the key limits agree, else one per batch item
        groups = [(0, B, lens[0])] if len(set(lens)) == 1 else [(b, b + 1, lens[b]) for b in range(B)]
        return _k5_launch(q, k, v, block_mask, blk, scale, groups)
    on_device = isinstance(lens, torch.Tensor)
    if on_device:
        lens = lens.to(q.device).reshape(-1)
    if row_range is None:
        lo, hi = _window_ranges(q.device, B, Sq, Sk, lens, *((-1, 0) if causal else window))
    else:
        lo, hi = row_range
        if on_device:
            hi = torch.minimum(hi, lens.reshape(-1, 1).clamp(0, Sk).to(torch.int32))
        elif any(n != Sk for n in lens):     # fold the host limits: one small device op per distinct limit, no host read
            hi = torch.stack([hi[b if hi.shape[0] > 1 else 0].clamp(max=lens[b]) for b in range(B)])
    kv_valid = Sk if on_device else max(lens)
    if kv_valid == 0:   # no visible key at all
        return torch.zeros((B, H, Sq, D), dtype=q.dtype, device=q.device)
    return _k5_launch(q, k, v, block_mask, blk, scale, [(0, B, kv_valid)], lo, hi)


def _check_no_ranges(what: str, window, row_range):
    if window is not None or row_range is not None:
        raise NotImplementedError(f"{what}: window= and row_range= have no backward yet (the backward serves the block mask, kv_len "
                                  "and causal=; DESIGN.md section 5.21)")


def _bwd_launch(dout, q, k, v, out, block_mask, blk: int, scale: float, lens, causal: bool):
    """block_sparse_attention_backward's launch sequence (rsa_block_sparse_bwd: row statistics, dq, dk / dv) for the whole batch."""
    B, H, Sq, D = q.shape
    if D in _core._PAD_HEAD_DIM:   # zero columns add exact zeros to every dot product; the caller's scale is kept
        pad = (0, _core._PAD_HEAD_DIM[D] - D)
        F = torch.nn.functional
        res = _bwd_launch(*(F.pad(t, pad) for t in (dout, q, k, v, out)), block_mask, blk, scale, lens, causal)
        return tuple(t[..., :D].contiguous() for t in res)
    Hkv, Sk = k.shape[1], k.shape[2]
    dev = q.device
    L = _lib.lib()
    dout, q, k, v, out = (_core._as_bhsd(t) for t in (dout, q, k, v, out))
    NQ, NK, Hl = -(-Sq // blk), block_mask.shape[3], int(block_mask.shape[1])
    # the row lists (the key blocks a query block keeps) and the column lists (the query blocks that keep a key block): the same
    # conversion on the mask and on its transpose
    rows = block_mask_to_lists(block_mask, B, Hl)
    cols = block_mask_to_lists(block_mask.transpose(-1, -2).contiguous(), B, Hl)
    len_dev, kv_valid, _ = _device_limit(lens, B, Sk, dev)
    dq = torch.empty((B, H, Sq, D), dtype=q.dtype, device=dev)
    dk = torch.empty((B, Hkv, Sk, D), dtype=q.dtype, device=dev)
    dv = torch.empty((B, Hkv, Sk, D), dtype=q.dtype, device=dev)
    shape = (B, H, Hkv, Hl, Sq, Sk, D)
    need = ctypes.c_size_t(0)
    _lib.check(L.rsa_block_sparse_bwd_bytes(*shape, blk, NQ, NK, ctypes.byref(need)), "rsa_block_sparse_bwd_bytes")
    ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.rsa_block_sparse_bwd(*shape, _core.dtype_code(q.dtype), blk, NQ, NK, kv_valid, _ptr(len_dev), int(causal), scale,
                                          _core._t4(q), _core._t4(k), _core._t4(v), _core._t4(out), _core._t4(dout),
                                          rows["cols"].data_ptr(), rows["counts"].data_ptr(), cols["cols"].data_ptr(),
                                          cols["counts"].data_ptr(), ws.data_ptr(), ws.numel(), _out4(dq), _out4(dk), _out4(dv),
                                          _core._stream()), "rsa_block_sparse_bwd")
    return dq, dk, dv


def block_sparse_attention_backward(dout: torch.Tensor, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor,
                                    block_mask: torch.Tensor, *, kv_len=None, sm_scale: Optional[float] = None,
                                    block_size: int = 128, causal: bool = False, window=None, row_range=None):
    """The gradients (dq, dk, dv) of out = block_sparse_attention(q, k, v, block_mask, kv_len=, sm_scale=, block_size=, causal=)
    for the upstream gradient dout; every argument means what it means there.  q, out, dout [B,H,Sq,D]; k, v [B,Hkv,Sk,D] with
    H % Hkv == 0; block_mask bool / uint8 [B|1, Hl, ceil(Sq/block), NK] with Hl in {1, Hkv, H}; both block sizes; causal (aligned
    bottom-right, j <= r + kv_len[b] - Sq) at 128-token blocks as the forward; bf16 / fp16; head dims 64 / 128 native, 16 / 32
    zero-padded.  Any strides with a contiguous head dim run without a copy.  kv_len None, an int, one value per item or a device
    tensor: all become one device int32 [B] array, the call is ONE launch sequence for the whole batch, and a device tensor is never
    read on the host.  Returns dq [B,H,Sq,D] and dk, dv [B,Hkv,Sk,D] in the input dtype.

    The row statistics are recomputed from q and k (the forward keeps none): two sweeps over the kept tiles, no float atomics --
    two calls give the same bytes.  Keys at or beyond kv_len are never multiplied (k / v may hold NaN
    there) and get zero dk / dv rows, as do key blocks no query block keeps; a query row that sees no key gets a zero dq row.
    window= and row_range= are not served (NotImplementedError), nor are the rectified calls, the fp8 forms and paged caches."""
    blk = _check_block_pair(block_size, block_size)
    _check_no_ranges("block_sparse_attention_backward", window, row_range)
    if causal and blk != _lib.BLOCK:
        raise NotImplementedError(f"causal needs block_size = {_lib.BLOCK}, as in block_sparse_attention")
    B, H, Hkv, Sq, Sk, D = _check_operands(q, k, v)
    for name, t in (("out", out), ("dout", dout)):
        if not isinstance(t, torch.Tensor) or t.shape != q.shape or t.dtype != q.dtype:
            raise ValueError(f"{name}: a {q.dtype} tensor {tuple(q.shape)} like q, got {getattr(t, 'dtype', type(t))} "
                             f"{tuple(getattr(t, 'shape', ()))}")
    NQ, NKmax = -(-Sq // blk), -(-Sk // blk)
    if not isinstance(block_mask, torch.Tensor) or block_mask.dim() != 4 or block_mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"block_mask: a 4-d bool or uint8 tensor, got {getattr(block_mask, 'dtype', type(block_mask))} "
                         f"{tuple(getattr(block_mask, 'shape', ()))}")
    if (block_mask.shape[0] not in (1, B) or block_mask.shape[1] not in (1, Hkv, H) or block_mask.shape[2] != NQ
            or not 1 <= block_mask.shape[3] <= min(NKmax, MAX_KEY_BLOCKS) or NQ > MAX_KEY_BLOCKS):
        raise ValueError(f"block_mask {tuple(block_mask.shape)}: expected [{B}|1, {H}|{Hkv}|1, {NQ}, 1..{min(NKmax, MAX_KEY_BLOCKS)}] "
                         f"for block {blk} (at most {MAX_KEY_BLOCKS} query and key blocks)")
    lens = _check_limit("kv_len", kv_len, B, Sk, Sk)
    _core._require_device(dout, q, k, v, out)
    scale = float(D) ** -0.5 if sm_scale is None else float(sm_scale)
    if block_mask.device != q.device:
        block_mask = block_mask.to(q.device)
    return _bwd_launch(dout, q, k, v, out, block_mask, blk, scale, lens, bool(causal))


class _BlockSparseAttention(torch.autograd.Function):
    """block_sparse_attention with block_sparse_attention_backward behind it; the mask and kv_len get no gradient."""

    @staticmethod
    def forward(ctx, q, k, v, block_mask, kv_len, sm_scale, block_size, causal):
        out = block_sparse_attention(q, k, v, block_mask, kv_len=kv_len, sm_scale=sm_scale, block_size=block_size, causal=causal)
        ctx.save_for_backward(q, k, v, out, block_mask)
        ctx.opts = (kv_len, sm_scale, block_size, causal)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, block_mask = ctx.saved_tensors
        kv_len, sm_scale, block_size, causal = ctx.opts
        dq, dk, dv = block_sparse_attention_backward(dout, q, k, v, out, block_mask, kv_len=kv_len, sm_scale=sm_scale,
                                                     block_size=block_size, causal=causal)
        return dq, dk, dv, None, None, None, None, None


def block_sparse_attention_autograd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, block_mask: torch.Tensor, *, kv_len=None,
                                    sm_scale: Optional[float] = None, block_size: int = 128, causal: bool = False, window=None,
                                    row_range=None) -> torch.Tensor:
    """block_sparse_attention(q, k, v, block_mask, kv_len=, sm_scale=, block_size=, causal=) as a torch.autograd.Function: the
    forward is that call (the same bytes), the backward block_sparse_attention_backward; q, k and v get gradients, the mask and
    kv_len none.  Under torch.no_grad() it is the forward.  window= and row_range= are not served (NotImplementedError).
    block_sparse_attention itself stays as it is: it builds no graph."""
    _check_no_ranges("block_sparse_attention_autograd", window, row_range)
    return _BlockSparseAttention.apply(q, k, v, block_mask, kv_len, sm_scale, block_size, bool(causal))


def select_blocks(q: torch.Tensor, k: torch.Tensor, top_k: int, *, block_size: int = 128, kv_len=None, causal: bool = False,
                  keep_first: int = 0, keep_local: int = 0, mask_heads: str = "kv", return_scores: bool = False,
                  as_lists: bool = False, top_p: Optional[float] = None, score_scale: Optional[float] = None,
                  return_mass: bool = False, q_len=None):
    """Top-k key blocks per query block by pooled scores, per K/V head, on the device (MoBA-style): the
    block_mask of a following block_sparse_attention(q, k, v, mask, kv_len=..., causal=..., block_size=...).
    q [B,H,Sq,D], k [B,Hkv,Sk,D] with H % Hkv == 0 (query head h belongs to K/V head h // (H // Hkv)), bf16 or fp16, head dim 16,
    32, 64 or 128 (all native, nothing is padded), any strides block_sparse_attention accepts; block_size 64 or 128;
    NK = ceil(Sk/block) <= 8192.  kv_len as in block_sparse_attention (None, int, one value per batch item, or an int32 / int64
    device tensor of 1 or B values, which is read on the device only); off_b = kv_len[b] - Sq.
      pooling   qbar / kbar: the fp32 mean of a block's rows < Sq / of its keys < kv_len[b]
      score     t[b, hl, i, j] = sum over the list head's query heads, ascending, of <qbar[b, h, i], kbar[b, h // g, j]>, fp32, no
                sm_scale.  mask_heads="kv": one list head per K/V head (its H // Hkv query heads summed); "q": one per query head
      visible   j * block < kv_len[b]; with causal also j * block <= r1 + off_b (r0 .. r1 = the rows of query block i): the blocks
                in which block_sparse_attention(causal=True) lets some row of the block see some key
      forced    the visible j < keep_first, and with keep_local >= 1 the visible j in [jd_lo - (keep_local - 1), jd_hi] (without
                causal: up to jd_hi + (keep_local - 1)), jd_lo = max(r0 + off_b, 0) // block,
                jd_hi = min(max(r1 + off_b, 0), kv_len[b] - 1) // block
      kept      forced and the best max(top_k - |forced|, 0) visible unforced blocks, by t descending, the lower j on equal t:
                |kept| = min(max(top_k, |forced|), |visible|); top_k = 0 keeps the forced blocks alone
    Returns the bool mask [B, Hl, NQ, NK] (Hl = Hkv or H), or with as_lists=True the dict block_mask_to_lists returns for it
    (bitmask, cols, counts; row (b * Hl + hl) * NQ + i); with return_scores=True a pair, the second the fp32 scores
    [B, Hl, NQ, NK] with -inf at invisible blocks.  Two calls on the same inputs give the same bytes.  With non-finite scores
    which blocks win is unspecified; the rows stay well formed.  Asynchronous on the current stream.

    top_p in [0, 1] (rsa_block_select_p): a budget per row.  Everything above stands, except that top_k
    becomes the cap on |kept| and the row keeps the forced blocks and the shortest prefix of the ranking above (t descending, the
    lower j on equal t) whose softmax mass reaches top_p:
      weight    u_j = floor(exp2((t_j - t_max) * c) * 2^18 + 0.5), an integer, t_max over the row's visible blocks, c =
                float32(score_scale * log2(e)); score_scale defaults to 1 / ((H // Hl) * sqrt(D)) -- the logit is then the mean
                pooled logit of the list head's query heads at block_sparse_attention's default sm_scale -- and must be finite, > 0
      target    (total * round(top_p * 65536) + 65535) >> 16, total = the sum of u_j over the visible blocks
      kept      forced and the first min(n_p, max(top_k - |forced|, 0)) visible unforced blocks, n_p = the length of the shortest
                prefix with sum(forced u) + sum(prefix u) >= target.  top_p = 0 keeps the forced blocks alone, top_p = 1 every
                block of non-zero weight, up to the cap
    return_mass=True appends the fp32 tensor [B, Hl, NQ] of float(sum of kept u) / float(total) (0 for a row that sees nothing)
    to the return value.  Integer sums: two calls give the same bytes.  score_scale and return_mass are refused without top_p.

    q_len (rsa_block_select_ragged): the query rows of each batch item in a ragged batch padded to Sq rows
    -- None (= Sq), an int, one value per batch item, or an int32 / int64 device tensor of 1 or B values, which is clamped into
    [0, Sq] on the device and never read on the host (kv_len's forms).  With n_b = q_len[b] everything above stands with n_b in
    place of Sq wherever Sq counts rows: qbar is the mean over the rows < n_b of the block, off_b = kv_len[b] - n_b (kv_len[b]
    includes the item's n_b new tokens) and r1 = min((i + 1) * block, n_b) - 1, so item b's query blocks i < ceil(n_b / block)
    carry the bytes of the call on q[b:b+1, :, :n_b].  A query block i >= ceil(n_b / block) has no row: counts 0, mask row clear,
    scores -inf, mass 0, its cols unspecified.  q's rows at or beyond n_b are never read and may hold NaN."""
    return _select("select_blocks", q, k, False, top_k, block_size, kv_len, causal, keep_first, keep_local, mask_heads,
                   return_scores, as_lists, None, top_p, score_scale, return_mass, q_len)


MAX_SCORE_SPLITS = 256  # score workgroups per list row of select_blocks_pooled, at most (rsa_block_select.hip)
LOG2_E = 1.4426950408889634     # c = float32(score_scale * LOG2_E), the product formed in double (ctypes rounds it once)


def _check_top_p(top_p, score_scale, return_mass):
    """The budget options of the two selections: top_p None or a real in [0, 1]; score_scale None or a finite real > 0 whose c
    is still a finite float32 > 0; score_scale and return_mass belong to top_p."""
    def real(x):
        return isinstance(x, (int, float)) and not isinstance(x, bool)
    if top_p is None:
        if score_scale is not None:
            raise ValueError(f"score_scale: belongs to top_p (top_p is None), got {score_scale!r}")
        if return_mass:
            raise ValueError("return_mass: belongs to top_p (top_p is None)")
        return
    if not real(top_p) or not 0.0 <= float(top_p) <= 1.0:
        raise ValueError(f"top_p: None or a number in [0, 1], got {top_p!r}")
    if score_scale is not None:
        c = ctypes.c_float(float(score_scale) * LOG2_E).value if real(score_scale) else float("nan")
        if not 0.0 < c < float("inf"):
            raise ValueError(f"score_scale: None or a finite number > 0 (and score_scale * log2(e) a finite float32 > 0), "
                             f"got {score_scale!r}")


def _select(what: str, q, keys, pooled: bool, top_k, block_size, kv_len, causal, keep_first, keep_local, mask_heads,
            return_scores, as_lists, score_splits=None, top_p=None, score_scale=None, return_mass=False, q_len=None,
            cu_seqlens_q=None, max_q_len=None, bound: bool = False):
    """select_blocks (keys = k, rsa_block_select) and select_blocks_pooled (keys = pool_keys' cache, rsa_block_select_pooled,
    with its score_splits): the two differ in where kbar comes from and in nothing else.  With top_p the entries are their _p
    forms, which take (p16, c, mass) in front of the stream.  With q_len the entries are their _ragged forms: the _p argument
    lists (p16 = -1: top-k) and the device row counts in front of the stream.  With cu_seqlens_q (pooled only) the entry is
    rsa_block_select_pooled_packed: q [T, H, D], the ragged argument list with T in front and M for Sq.  bound (beside pooled):
    select_blocks_bound -- keys = pool_key_bounds' cache; rsa_block_select_bound has the ragged argument list alone (p16 = -1:
    top-k; no row counts: NULL) and rsa_block_select_bound_packed the packed one."""
    blk = _check_block(what, block_size)
    if mask_heads not in ("kv", "q"):
        raise ValueError(f"mask_heads: 'kv' (one selection per K/V head) or 'q' (one per query head), got {mask_heads!r}")
    for name, val in (("top_k", top_k), ("keep_first", keep_first), ("keep_local", keep_local)):
        _check_count(name, val, 0)
    _check_count("score_splits", score_splits, 1, MAX_SCORE_SPLITS, optional=True)
    _check_top_p(top_p, score_scale, return_mass)
    r = _query_rows(q, q_len, cu_seqlens_q, max_q_len, keys, None, lambda q4: _check_operands(q4, keys, pooled=pooled, bounds=bound))
    packed, q, B, H, Hkv, Sq, Sk, D = r.kind == "packed", r.q4, r.B, r.H, r.Hkv, r.Sq, r.Sk, r.D
    if pooled:      # the cache holds NK blocks: the capacity is taken as NK * block
        Sk *= blk
    NQ, NK = -(-Sq // blk), _key_blocks(Sk, blk)
    Hl = Hkv if mask_heads == "kv" else H
    lens = _check_limit("kv_len", kv_len, B, Sk, Sk)
    rows = _check_limit("q_len", q_len, B, Sq, Sq)
    _core._require_device(q, keys)
    dev = q.device
    if pooled and keys.data_ptr() % 16:
        raise ValueError(f"{'key_bounds' if bound else 'pooled_k'}: 16-byte aligned")
    kv_dev, kv_valid, _ = _device_limit(lens, B, Sk, dev)
    q_dev = _row_limit(rows, B, Sq, dev)
    L = _lib.lib()
    if packed:
        q, cu = _packed_on_device(r)
    else:
        q, keys = _core._as_bhsd(q), keys if pooled else _core._as_bhsd(keys)
    base = "rsa_block_select_bound" if bound else "rsa_block_select_pooled" if pooled else "rsa_block_select"
    entry = base + ("" if top_p is None or bound else "_p")
    need = ctypes.c_size_t(0)
    _lib.check(getattr(L, entry + "_bytes")(B, Hkv, Hl, D, NQ, NK, ctypes.byref(need)), entry + "_bytes")
    if q_dev is not None and not bound:
        entry = base + "_ragged"
    ws = torch.empty((need.value,), dtype=torch.uint8, device=dev)
    out = _empty_lists(B * Hl, NQ, NK, dev)
    scores = torch.empty((B, Hl, NQ, NK), dtype=torch.float32, device=dev) if return_scores else None
    if pooled:
        shape, source = (B, H, Hkv, Hl, Sq, D), keys.data_ptr()
        splits = (0 if score_splits is None else int(score_splits),)
    else:
        shape, source, splits = (B, H, Hkv, Hl, Sq, Sk, D), _core._t4(keys), ()
    mass, budget = None, ()
    if top_p is not None:
        mass = torch.empty((B, Hl, NQ), dtype=torch.float32, device=dev) if return_mass else None
        scale = 1.0 / ((H // Hl) * math.sqrt(D)) if score_scale is None else float(score_scale)
        budget = (int(round(float(top_p) * 65536.0)), scale * LOG2_E, _ptr(mass))
    if q_dev is not None or (bound and not packed):
        budget = (budget or (-1, 0.0, None)) + (_ptr(q_dev),)
    tq = _t3(q) if packed else _core._t4(q)
    if packed:              # T in front, M where Sq stood, cu_seqlens_q and the scan's scratch where q_len stood
        entry, shape = base + "_packed", (r.T,) + shape
        items = torch.empty((2 * (B + 1),), dtype=torch.int32, device=dev)
        budget = (budget or (-1, 0.0, None)) + (cu.data_ptr(), items.data_ptr())
    with torch.cuda.device(dev):
        _lib.check(getattr(L, entry)(*shape, _core.dtype_code(q.dtype), blk, NQ, NK, tq, source, _ptr(kv_dev), kv_valid,
                                     int(bool(causal)), min(top_k, NK), min(keep_first, NK), min(keep_local, NK + 1), *splits,
                                     ws.data_ptr(), need.value, out["bitmask"].data_ptr(), out["cols"].data_ptr(),
                                     out["counts"].data_ptr(), _ptr(scores), *budget, _core._stream()), entry)
    sel = out if as_lists else lists_to_block_mask(out["bitmask"], B, Hl, NQ, NK).view(torch.bool)
    extra = tuple(t for t in (scores, mass) if t is not None)
    return (sel,) + extra if extra else sel


def pool_keys(k: torch.Tensor, *, block_size: int = 128, kv_len=None, block_table=None, out: Optional[torch.Tensor] = None,
              start=None, workgroups_per_head: Optional[int] = None, k_scale=None) -> torch.Tensor:
    """The cache of pooled keys select_blocks_pooled reads: per key block the kbar of select_blocks, the
    fp32 sum of the block's keys below kv_len[b] divided once by their count, in select_blocks' summation order.
    k [B,Hkv,Sk,D], any strides block_sparse_decode accepts (a cache is never copied), or with block_table int32 [B, NKt] a page
    pool [P, Hkv, block_size, D] (one page = one key block, as in block_sparse_decode); bf16 / fp16; head dim 16, 32, 64 or 128;
    block_size 64 or 128; NKt = ceil(Sk/block) or the table's width, at most 8192.  Returns (and fills) out, fp32
    [B, Hkv, NKt, D] contiguous: 1/64 of K's bytes at 128-token blocks.
    kv_len, start: None (= Sk / 0), an int, one value per batch item, or an int32 / int64 device tensor of 1 or B values, which is
    clamped into [0, Sk] on the device and never read on the host.  The call writes exactly the blocks j with
    start[b] // block <= j < ceil(kv_len[b] / block) and leaves every other element of out untouched:
      start=None             everything below kv_len (prefill); out may be None, the result is then new (and unwritten beyond)
      start=the old length   after an append: the tail block again and every block the append opened
      start=kv_len           the ragged tail block alone (after a rollback of rejected speculative tokens)
      start > kv_len         nothing
    out is required when start is given.  Keys at or beyond kv_len[b] are never loaded and may hold NaN.  The table is read only
    for blocks the call writes; an entry outside [0, P) gives a block of zeros.
    workgroups_per_head: workgroups per (b, K/V head) that stride over the block range -- a performance hint, any count >= 1
    gives the same bytes.  None: the exact count when both limits are host values, NKt with start=None, else 2 (an append of
    at most block tokens touches at most two blocks).  Asynchronous on the current stream, no host synchronisation, capturable.
    An e4m3 cache: k float8_e4m3fn, contiguous or paged, head dim 64 / 128, strides multiples of 8 bytes,
    with k_scale a positive float or a float32 device tensor of 1 or Hkv values (required then, refused otherwise).  The value of
    a block is the fp32 sum of float(code) over its keys below kv_len[b], in the same order, divided once by their count and
    multiplied once by k_scale[hkv]; every other clause above holds.  select_blocks_pooled reads the result as before."""
    return _pool_cache("pool_keys", (), k, block_size, kv_len, block_table, out, start, workgroups_per_head, k_scale)


def _pool_cache(what: str, pair, k, block_size, kv_len, block_table, out, start, workgroups_per_head, k_scale) -> torch.Tensor:
    """pool_keys (pair = (): the cache [B, Hkv, NK, D], rsa_pool_keys[_kv8]) and pool_key_bounds (pair = (2,): the cache
    [B, Hkv, NK, 2, D], rsa_pool_key_bounds[_kv8]): one argument contract, and C entries with the same argument lists."""
    blk = _check_block(what, block_size)
    _check_count("workgroups_per_head", workgroups_per_head, 1, optional=True)
    B, _, Hkv, _, Sk, D = _check_operands(None, k, block_table=block_table, blk=blk, kv8_ok=True)
    _check_scales(k, Hkv, k_scale=k_scale)
    NK = _key_blocks(Sk, blk)
    if start is not None and out is None:
        raise ValueError("out: required when start is given (an update writes into the cache it is given)")
    shape = (B, Hkv, NK) + pair + (D,)
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != shape
                            or not out.is_contiguous()):
        raise ValueError(f"out: a contiguous float32 tensor {list(shape)}, got {getattr(out, 'dtype', type(out))} "
                         f"{tuple(getattr(out, 'shape', ()))}")
    lens = _check_limit("kv_len", kv_len, B, Sk, Sk)
    starts = _check_limit("start", start, B, Sk, 0)
    _check_cache(k)
    _core._require_device(k)
    dev = k.device
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    else:
        _core._require_device(out)
    if out.data_ptr() % 16:
        raise ValueError("out: 16-byte aligned")
    table, _held = _table_args(block_table, k)
    kv_dev, kv_valid, lens = _device_limit(lens, B, Sk, dev)
    st_dev, st_host, starts = _device_limit(starts, B, Sk, dev)
    if workgroups_per_head is not None:
        wph = int(workgroups_per_head)
    elif lens is not None and starts is not None:     # the exact count: the grid is sized from host values alone
        wph = max([1] + [-(-n // blk) - s // blk for n, s in zip(lens, starts) if s <= n])
    else:
        wph = NK if start is None else 2
    entry = ("rsa_pool_key_bounds" if pair else "rsa_pool_keys") + ("_kv8" if k.dtype == E4M3 else "")
    with torch.cuda.device(dev):
        if k.dtype == E4M3:
            ks = _scale_arg(k_scale, Hkv, dev)
            _lib.check(getattr(_lib.lib(), entry)(B, Hkv, Sk, D, blk, NK, _core._t4(k), *table, _ptr(kv_dev), kv_valid,
                                                  _ptr(st_dev), st_host, wph, out.data_ptr(), ks.data_ptr(), _core._stream()), entry)
        else:
            _lib.check(getattr(_lib.lib(), entry)(B, Hkv, Sk, D, _core.dtype_code(k.dtype), blk, NK, _core._t4(k), *table,
                                                  _ptr(kv_dev), kv_valid, _ptr(st_dev), st_host, wph, out.data_ptr(),
                                                  _core._stream()), entry)
    return out


def pool_key_bounds(k: torch.Tensor, *, block_size: int = 128, kv_len=None, block_table=None, out: Optional[torch.Tensor] = None,
                    start=None, workgroups_per_head: Optional[int] = None, k_scale=None) -> torch.Tensor:
    """The cache of per-channel key bounds select_blocks_bound reads: per key block and channel the
    minimum and the maximum of the block's keys below kv_len[b].  Returns (and fills) out, fp32 [B, Hkv, NKt, 2, D] contiguous:
    out[..., 0, :] the minima, out[..., 1, :] the maxima; 1/32 of K's bytes at 128-token blocks of bf16.
    The argument contract is pool_keys' word for word: k [B,Hkv,Sk,D] or page pools behind block_table, bf16 / fp16 at head dim
    16, 32, 64 or 128, float8_e4m3fn with k_scale at head dim 64 / 128; kv_len / start in all their forms, device tensors clamped
    on the device and never read on the host; the call writes exactly the blocks start[b] // block <= j < ceil(kv_len[b] / block)
    and no other byte of out (out is required when start is given); a table entry outside [0, P) gives a block of zeros, min and
    max alike; keys at or beyond kv_len[b] are never loaded and may hold NaN; out is 16-byte aligned; workgroups_per_head is a
    performance hint; asynchronous on the current stream, capturable.
    An e4m3 cache: min and max are taken over float(code) and each is multiplied once by k_scale[hkv] (positive: the order is
    kept).  Keys below kv_len are taken to be finite: a NaN there gives an unspecified value (and forms no address).
    min and max are exact and order-free, so every workgroups_per_head gives the same values and two calls the same bytes; one
    pass over K writes both halves."""
    return _pool_cache("pool_key_bounds", (2,), k, block_size, kv_len, block_table, out, start, workgroups_per_head, k_scale)


def append_kv_e4m3(k_new: torch.Tensor, v_new: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, *, start, k_scale,
                   v_scale, n_new=None, block_size: int = 128, block_table=None, cu_seqlens=None) -> None:
    """The writer of an e4m3 K/V cache: new K / V rows become one-byte codes under one static fp32 scale
    per K/V head and land where block_sparse_decode and pool_keys read them.
    k_new / v_new [B,Hkv,T,D], bf16 / fp16, through any strides block_sparse_decode accepts for k / v (head-strided views of a
    fused projection included; the inputs are never copied).  k_cache / v_cache float8_e4m3fn: [B,Hkv,Sk,D], or with block_table
    int32 [B, NKt] page pools [P,Hkv,block_size,D] of capacity Sk = NKt * block_size (one page = one key block); strides and
    pointers multiples of 8 bytes (block_sparse_decode asks 16 of V).  Head dim 64 or 128.
    Token t < n_new[b] (default T) of batch item b goes to position start[b] + t.  start, n_new: an int, one value per batch item,
    or an int32 / int64 device tensor of 1 or B values, which is clamped on the device (into [0, Sk] / [0, T]) and never read on
    the host; the grid is sized from T alone.  Prefill is the call with start=0.
    k_scale / v_scale: a positive finite float, or a float32 device tensor of 1 or Hkv values.  Per element
        code = (x.float() / scale[hkv]).clamp(-448, 448).to(torch.float8_e4m3fn)
    bit for bit: one IEEE fp32 division, round to nearest even, subnormals kept, +-Inf saturates, a NaN stays a NaN code (0x7F or
    0xFF by the sign bit of the input).  The
    values of a scale tensor are not checked and no address depends on them: a zero, negative or non-finite scale garbles that
    head's rows only.
    The call writes exactly the D bytes of every placed row and no other byte.  A position at or beyond the capacity is dropped,
    and so is one whose table entry lies outside [0, P).  Two batch items whose table entries name the same page race: keeping
    pages apart is the caller's business.  Static scales mean an append never re-quantises what the page already holds.
    Asynchronous on the current stream, no host synchronisation, capturable.
    cu_seqlens (rsa_kv8_append_packed): the packed batch -- k_new / v_new [T, Hkv, D] (row and head strides
    multiples of 8 elements), cu_seqlens a device int32 tensor of B + 1 values (B from block_table, else from k_cache), sanitised on
    the device as block_sparse_extend(cu_seqlens_q=) describes, with M = T: token t < n_b = s_{b+1} - s_b of item b is row s_b + t
    and goes to position start[b] + t.  Placed and untouched bytes are those of the padded call.  k_new is 3-d if and only if
    cu_seqlens is given; n_new= beside it is refused.  Two launches; the grid is sized from T."""
    blk = _check_block("append_kv_e4m3", block_size)
    packed = cu_seqlens is not None
    if packed and n_new is not None:
        raise ValueError("n_new belongs to a padded k_new: with cu_seqlens the tokens of an item are cu_seqlens[b + 1] - cu_seqlens[b]")
    k3, v3 = k_new, v_new
    k_new, Bp = _packed_view("k_new", k_new, cu_seqlens, k_cache, block_table)
    v_new, _ = _packed_view("v_new", v_new, cu_seqlens, k_cache, block_table)
    B, _, Hkv, T, _, D = _check_operands(k_new, k_new, v_new, dims=KV8_HEAD_DIMS)
    if packed:
        cu, _ = _check_packed("cu_seqlens", cu_seqlens, None, B, T, need_max=False)
    _, _, _, _, Sk, _ = _check_operands(None, k_cache, v_cache, dims=KV8_HEAD_DIMS, block_table=block_table, blk=blk, kv8_ok=True)
    if k_cache.dtype != E4M3:
        raise ValueError(f"k_cache, v_cache: float8_e4m3fn, got {k_cache.dtype}")
    if (k_cache.shape[1], k_cache.shape[3]) != (Hkv, D) or (block_table is None and k_cache.shape[0] != B):
        raise ValueError(f"k_cache {tuple(k_cache.shape)} does not match k_new {tuple(k_new.shape)}")
    if block_table is not None:
        _check_block_table(block_table, B)
    _check_scales(k_cache, Hkv, k_scale=k_scale, v_scale=v_scale)
    starts = _check_limit("start", start, B, Sk, 0)
    counts = _check_limit("n_new", n_new, B, T, T)
    _check_cache(k_new, v_new)
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        *outer, inner = t.stride()
        if inner != 1 or any(st % 8 for st in outer) or t.data_ptr() % 8:
            raise ValueError(f"{name}: a contiguous head dim, strides that are multiples of 8 bytes and an 8-byte aligned pointer, "
                             f"got strides {tuple(t.stride())}, pointer % 8 = {t.data_ptr() % 8}")
    _core._require_device(k_new, v_new, k_cache, v_cache)
    dev = k_cache.device
    table, _held = _table_args(block_table, k_cache)
    st_dev, st_host, _ = _device_limit(starts, B, Sk, dev)
    n_dev, n_host, _ = _device_limit(counts, B, T, dev)
    ks, vs = _scale_arg(k_scale, Hkv, dev), _scale_arg(v_scale, Hkv, dev)
    if packed:
        _core._require_device(cu)
        cu, items = cu.contiguous(), torch.empty((B + 1,), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().rsa_kv8_append_packed(B, Hkv, T, Sk, D, _core.dtype_code(k3.dtype), blk, _t3(k3), _t3(v3),
                                                        _out4(k_cache), _out4(v_cache), *table, _ptr(st_dev), st_host,
                                                        cu.data_ptr(), items.data_ptr(), ks.data_ptr(), vs.data_ptr(),
                                                        _core._stream()), "rsa_kv8_append_packed")
        return
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().rsa_kv8_append(B, Hkv, T, Sk, D, _core.dtype_code(k_new.dtype), blk, _core._t4(k_new),
                                             _core._t4(v_new), _out4(k_cache), _out4(v_cache), *table, _ptr(st_dev), st_host,
                                             _ptr(n_dev), n_host, ks.data_ptr(), vs.data_ptr(), _core._stream()),
                   "rsa_kv8_append")


def select_blocks_pooled(q: torch.Tensor, pooled_k: torch.Tensor, top_k: int, *, block_size: int = 128, kv_len=None,
                         causal: bool = False, keep_first: int = 0, keep_local: int = 0, mask_heads: str = "kv",
                         return_scores: bool = False, as_lists: bool = False, score_splits: Optional[int] = None,
                         top_p: Optional[float] = None, score_scale: Optional[float] = None, return_mass: bool = False,
                         q_len=None, cu_seqlens_q=None, max_q_len: Optional[int] = None):
    """select_blocks from a cache of pooled keys: q [B,H,Sq,D] (any Sq), pooled_k fp32 [B, Hkv, NK, D]
    contiguous as pool_keys returns it, Sk taken as NK * block_size.  Visible set, forced blocks, top-k, ties and the returned
    mask / lists / scores are select_blocks' contract word for word, and on inputs both calls accept
        select_blocks_pooled(q, pool_keys(k, kv_len=L, ...), top_k, kv_len=L, ...)
    gives the bytes of select_blocks(q, k, top_k, kv_len=L, ...): the query pooling, the score arithmetic and the select body are
    one device code.  Only the visible prefix of pooled_k is read: entries at or beyond ceil(kv_len[b] / block) may hold anything,
    NaN included.  kv_len: None (= NK * block), an int, one value per batch item, or an int32 / int64 device tensor (read on the
    device only).
    score_splits: workgroups per list row that compute the row's scores before the select workgroup ranks them (few list rows,
    many key blocks: a decode step); 1 = inside the select workgroup; None = the library's choice, a function of the shapes alone
    (measured: DESIGN.md 5.13).  Every value gives the same bytes.  Asynchronous on the current stream, capturable.
    top_p, score_scale, return_mass: select_blocks' (rsa_block_select_pooled_p), with the same bytes.
    q_len: select_blocks' (rsa_block_select_pooled_ragged), with the same bytes: the rows of each batch item
    of a ragged batch, the selection half of the continuous-batching step block_sparse_extend(q_len=) describes.
    cu_seqlens_q, max_q_len (rsa_block_select_pooled_packed): the packed batch block_sparse_extend describes --
    q [T, H, D], cu_seqlens_q a device int32 tensor of B + 1 values (B = pooled_k.shape[0]) that is sanitised on the device and never
    read on the host, max_q_len = M a host int in [1, T].  The result keeps the padded layout [B, Hl, NQ, NK] with
    NQ = ceil(M / block) and holds the bytes of the q_len= call on the padded copy of q with q_len[b] = n_b.  q is 3-d if and only
    if cu_seqlens_q is given; q_len= beside it is refused.  One launch more than the q_len= call (the scan of cu_seqlens_q)."""
    return _select("select_blocks_pooled", q, pooled_k, True, top_k, block_size, kv_len, causal, keep_first, keep_local, mask_heads,
                   return_scores, as_lists, score_splits, top_p, score_scale, return_mass, q_len, cu_seqlens_q, max_q_len)


def select_blocks_bound(q: torch.Tensor, key_bounds: torch.Tensor, top_k: int, *, block_size: int = 128, kv_len=None,
                        causal: bool = False, keep_first: int = 0, keep_local: int = 0, mask_heads: str = "kv",
                        return_scores: bool = False, as_lists: bool = False, score_splits: Optional[int] = None,
                        top_p: Optional[float] = None, score_scale: Optional[float] = None, return_mass: bool = False,
                        q_len=None, cu_seqlens_q=None, max_q_len: Optional[int] = None):
    """select_blocks_pooled with one thing changed, the score (Quest's criterion): key_bounds is the fp32
    cache [B, Hkv, NK, 2, D] of pool_key_bounds (contiguous, 16-byte aligned) and list row (b, hl, i) scores key block j by the
    upper bound of qs . k over every key the block could hold,
        t = sum over d of max(qs_d * mn_d, qs_d * mx_d)
    with qs the pooled query of select_blocks (the sum over the list head's query heads, ascending, of each head's fp32 row mean;
    the bound of the summed query, not the sum of per-head bounds) and mn / mx the block's per-channel minimum / maximum.  A
    block that holds one key aligned with the query among many that are not keeps a high score, where its mean is near zero:
    the criterion for training-free sparse decode of a dense model.  fp32 in a fixed order (rsa.h): two calls, the same bytes.
    Everything else is select_blocks_pooled's contract and device code: the visible prefix and the forced blocks, top-k with
    ties to the lower block, top_p / score_scale / return_mass with the top_k cap, as_lists, return_scores (-inf where a block is
    not visible), q_len and the packed cu_seqlens_q / max_q_len layout, kv_len never read on the host, only the visible prefix of
    the cache read (the rest may hold NaN), capture in a graph.  score_splits: workgroups per list row of the score pass, which
    here is a launch of its own at every count, 1 included; every value gives the same bytes; None = select_blocks_pooled's
    choice (measured for this form too: DESIGN.md section 5.19).  Where every key of a block is the same the bound is the mean
    score: select_blocks_pooled's result up to fp32 rounding, and its bytes where the sums are exact."""
    return _select("select_blocks_bound", q, key_bounds, True, top_k, block_size, kv_len, causal, keep_first, keep_local, mask_heads,
                   return_scores, as_lists, score_splits, top_p, score_scale, return_mass, q_len, cu_seqlens_q, max_q_len, bound=True)


DECODE_MAX_ROWS = 64    # rows of a decode unit: four 16-row MFMA tiles (rsa_decode.hip)


def block_sparse_decode(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, block_mask, *, kv_len=None,
                        sm_scale: Optional[float] = None, block_size: int = 128, causal: bool = False, block_table=None,
                        return_lse: bool = False, blocks_per_split: Optional[int] = None, k_scale=None, v_scale=None):
    """Block-sparse attention of a few query rows (decode: one token, or a handful of speculative ones) over a long K/V cache:
    block_sparse_attention's result at one query block, from kernels built for it.
    q [B,H,Sq,D] with Sq <= block_size; k / v [B,Hkv,Sk,D], H % Hkv == 0, query head h reads K/V head h // (H // Hkv); any strides
    with a contiguous head dim and 16-byte aligned rows (a cache is never copied: other strides are refused); bf16 / fp16; head
    dim 64 or 128 (16 / 32 are refused: padding a cache would copy it); block_size 64 or 128.
    block_mask: bool / uint8 [B|1, Hl, 1, NK], Hl in {1, Hkv, H}, NK <= min(ceil(Sk/block), 8192) -- what
    select_blocks(q, k, top_k, causal=True, kv_len=...) returns for Sq <= block -- or the dict select_blocks(..., as_lists=True)
    returns with one query block (Hl = cols.shape[0] // B; used as it is, no conversion launch).
    A unit is the H // max(Hl, Hkv) query heads that share a K/V head and a list row; its Sq * H // max(Hl, Hkv) rows share every
    K / V block read, and more than 64 of them are refused (use block_sparse_attention).
    Row r of (b, h) sees key j iff mask[b, hl(h), 0, j // block] and j < kv_len[b] and j < NK * block and, with causal=True,
    j <= r + kv_len[b] - Sq (bottom-right aligned; both block sizes).  A row without a visible key is 0, its log-sum-exp -inf.
    kv_len: None (= Sk), an int, one value per batch item, or an int32 / int64 device tensor of 1 or B values, which is clamped
    into [0, Sk] on the device and never read on the host.  Keys at or beyond kv_len[b] may hold anything, NaN included.
    block_table: int32 device tensor [B, NKt], NKt >= NK; k / v are then page pools [P, Hkv, block_size, D], the capacity is
    Sk = NKt * block_size and key j of batch item b is row j % block of page block_table[b, j // block].  The table is read only
    for kept blocks that hold a key below kv_len[b]; a kept block whose entry lies outside [0, P) contributes no key, as if its
    mask bit were clear (and so does an entry of a caller's lists outside [0, NK)).
    return_lse=True: (out, lse), lse fp32 [B,H,Sq] = ln sum over the visible keys of exp(sm_scale q . k).
    blocks_per_split: kept-list entries per workgroup; None = the library's choice, min(8, NK) (measured: DESIGN.md 5.12).  The result may
    depend on it through the summation order of the merge; for one value two calls give the same bytes.  Asynchronous on the
    current stream, no host synchronisation, capturable in a HIP graph (the workspace comes from torch inside the capture).
    An e4m3 cache: k and v float8_e4m3fn (append_kv_e4m3 writes them), contiguous or paged, with k_scale
    and v_scale each a positive float or a float32 device tensor of 1 or Hkv values -- both required then, and refused with a
    2-byte cache; q and the output stay bf16 / fp16.  The value of a code is float(code) * scale[hkv].  The codes become q's type in
    registers (exact), the K scale multiplies each fp32 score once, the V scale the merged row once; the log-sum-exp carries the K
    scale through the scores and does not see v_scale.  With power-of-two scales the bytes are those of this call on the
    dequantised 2-byte cache.  Every rule above holds unchanged; K views need strides and a pointer that are multiples of 8 bytes, V
    views of 16 (others are refused, never copied).  The scales' values are not checked: a zero, negative or non-finite one garbles
    its head's rows only.
    There is no q_len here: a ragged decode or draft-verification batch (items of different row counts in one padded q) is
    block_sparse_extend(..., q_len=), which gives this call's bytes on every shape this call serves."""
    return _sparse_rows(False, q, k, v, block_mask, kv_len, sm_scale, block_size, causal, block_table, return_lse, blocks_per_split,
                        k_scale, v_scale)


EXTEND_FILL_GROUPS = 256    # row groups from which block_sparse_extend's default is one split (rsa_decode.hip: EXT_FILL_GROUPS)


def extend_row_groups(B: int, H: int, Hkv: int, Hl: int, Sq: int, block_size: int) -> Dict[str, int]:
    """How block_sparse_extend cuts a call into row groups, from the shapes alone: gu = H // max(Hl, Hkv)
    heads share a K/V head and a list row; a group is gh = ceil(gu / ceil(gu / 64)) of them x qg = min(64 // gh, Sq, block_size)
    consecutive query rows of one query block.  -> dict(gh, qg, head_chunks, query_chunks, groups, rows16): groups = B *
    max(Hl, Hkv) * head_chunks * query_chunks workgroups per split, rows16 = gh * qg rounded up to 16, 32 or 64."""
    U = max(Hl, Hkv)
    gu = H // U
    HC = -(-gu // DECODE_MAX_ROWS)
    gh = -(-gu // HC)
    qmax = min(Sq, block_size)
    qg = min(DECODE_MAX_ROWS // gh, qmax)
    NQ = -(-Sq // block_size)
    QC = (NQ - 1) * (-(-qmax // qg)) + -(-(Sq - (NQ - 1) * block_size) // qg)
    rows = gh * qg
    return dict(gh=gh, qg=qg, head_chunks=HC, query_chunks=QC, groups=B * U * HC * QC,
                rows16=16 if rows <= 16 else (32 if rows <= 32 else 64))


def extend_default_split(groups: int, NK: int) -> int:
    """block_sparse_extend's blocks_per_split=None: min(8, NK) while the launch has fewer than 256 row groups (one per CU), NK --
    one split -- from there on."""
    return min(8, NK) if groups < EXTEND_FILL_GROUPS else NK


def block_sparse_extend(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, block_mask, *, kv_len=None,
                        sm_scale: Optional[float] = None, block_size: int = 128, causal: bool = False, block_table=None,
                        return_lse: bool = False, blocks_per_split: Optional[int] = None, k_scale=None, v_scale=None,
                        q_len=None, cu_seqlens_q=None, max_q_len: Optional[int] = None):
    """Block-sparse attention of a chunk of new tokens over a K/V cache that already holds a prefix ("extend": chunked prefill, a
    second turn on a cached conversation, a prefix-cache hit, verification of a speculative draft): block_sparse_decode with the
    one-query-block limit and the 64-row limit lifted.  Everything not said here is block_sparse_decode's
    as documented: operand strides and alignment, every kv_len form (a device kv_len is clamped on the device and never read on
    the host), NaN beyond kv_len, out-of-range table or list entries as cleared bits, the paged pools, the e4m3 cache with k_scale /
    v_scale, bf16 / fp16, head dim 64 / 128, block_size 64 / 128, the same bytes from two calls, asynchronous on the current
    stream and capturable in a HIP graph.
    q [B,H,Sq,D] with any Sq >= 1; NQ = ceil(Sq / block_size); query block i is rows [i * block, min((i + 1) * block, Sq)) of q,
    counted from q's row 0 (as block_sparse_attention and select_blocks count them).
    block_mask: bool / uint8 [B|1, Hl, NQ, NK], Hl in {1, Hkv, H}, or the dict select_blocks(_pooled)(..., as_lists=True) returns
    for NQ query blocks: cols int32 [B * Hl, NQ, NK] and counts int32 [B * Hl, NQ], contiguous, used as they are (no conversion
    launch).
    Row r of (b, h) sees key j iff mask[b, hl(h), r // block, j // block] and j < kv_len[b] and j < NK * block and, with
    causal=True, j <= r + kv_len[b] - Sq: block_sparse_attention(causal=True)'s rule, bottom-right aligned, at both block sizes.  A
    row without a visible key -- every row with r + kv_len[b] - Sq < 0 among them -- is 0 and its log-sum-exp -inf.
    Any H // max(Hl, Hkv) is served, more than 64 query heads in a unit included.  The kernels are the decode kernels' body: a
    unit's query block is cut into row groups of at most 64 rows (extend_row_groups), one workgroup per (row group, split); on
    shapes block_sparse_decode serves, at an equal explicit blocks_per_split, the bytes are that call's.
    return_lse=True: (out, lse), lse fp32 [B,H,Sq].
    blocks_per_split: None = min(8, NK) while the launch has fewer than 256 row groups, NK (one split) from there on: a function of
    the shapes alone (extend_default_split).  The workspace, taken from torch, is groups * ceil(NK / blocks_per_split) * rows16 *
    (D + 2) * 4 bytes.
    Grid limits, refused before the first HIP call: at most 2^31 - 1 row groups, and B * H * Sq * D / 1024 <= 2^31 - 1.
    When to use it (measured, profiles/extend_perf.txt; H = 32 over 8 K/V heads, D = 128, paged bf16 / e4m3 caches): against
    gathering the cache through the table (and dequantising it) for block_sparse_attention, this call is faster at every measured
    shape up to Sq = 512 and at Sq = 2048 over a 131 072-key cache; over 8 x 32 768 keys the crossover lies near Sq = 512 at top_k
    64 and near 1 300 at top_k 16 -- beyond it gather once and call block_sparse_attention.  Against block_sparse_attention on a
    cache that is already contiguous and 2-byte it is faster up to Sq = 128 and slower from 512 rows on (every 64-row group
    re-reads its kept blocks).

    q_len (rsa_block_sparse_extend_ragged[_kv8]): a ragged batch -- prefill chunks, second turns, decode
    items and draft verifications in one q padded to Sq rows.  None (= Sq), an int, one value per batch item, or an int32 / int64
    device tensor of 1 or B values, which is clamped into [0, Sq] on the device and never read on the host (kv_len's forms).  With
    n_b = q_len[b], and kv_len[b] the length AFTER the append (it includes the n_b new tokens): row r < n_b of (b, h) sees key j
    iff mask[b, hl(h), r // block, j // block] and j < kv_len[b] and j < NK * block and, with causal=True,
    j <= r + kv_len[b] - n_b -- what this call computes on q[b:b+1, :, :n_b] with mask[b:b+1, :, :ceil(n_b / block)], and at an
    explicit blocks_per_split with the same bytes.  Rows r >= n_b come out 0 with log-sum-exp -inf (written, not left
    unwritten); q's rows there are never loaded and may hold NaN; mask / list rows of query blocks i >= ceil(n_b / block) are
    never read.  A row group of padding rows leaves before it reads a list entry, a table entry or a K/V byte.  The grid, the row
    groups, the default split and the workspace are those of the padded shapes (extend_row_groups, extend_default_split): the call
    is capturable and a replay follows q_len, kv_len, the cache and the table as they change in place.  The ragged step on a paged
    e4m3 cache, every length on the device:
        append_kv_e4m3(k_new, v_new, kc, vc, start=prev, n_new=q_len, ...); pool_keys(kc, out=pooled, start=prev, kv_len=prev + q_len, ...)
        lists = select_blocks_pooled(q, pooled, top_k, kv_len=prev + q_len, q_len=q_len, causal=True, as_lists=True)
        out = block_sparse_extend(q, kc, vc, lists, kv_len=prev + q_len, q_len=q_len, causal=True, block_table=..., ...)
    What the padding costs (measured, profiles/extend_ragged_perf.txt; 8 x 32 768 keys, padded Sq = 512, top_k 16 / 64): eight
    one-token items take 3.1x to 5.3x block_sparse_decode's time, a 512-row chunk beside seven one-token items 3.1x to 3.7x the
    two separate calls.  The call buys one graph of fixed shape, not speed: pad to the longest chunk a step really holds
     -- or pack the batch, below.

    cu_seqlens_q, max_q_len (rsa_block_sparse_extend_packed[_kv8]): the packed batch of a continuous-batching
    step, flash-attn's varlen layout.  q is [T, H, D] -- T the token budget, any row and head strides that are multiples of 8
    elements, so a view of a fused projection [T, (H + 2 Hkv) D] runs without a copy --, cu_seqlens_q a device int32 tensor of B + 1
    values (B from block_table, else from k), max_q_len = M a host int in [1, T].  The device sanitises cu_seqlens_q once and the
    host never reads it: s_b = the running maximum of clamp(cu[b], 0, T), n_b = min(s_{b+1} - s_b, M), item b = rows
    [s_b, s_b + n_b).  Returns out [T, H, D] (and lse fp32 [T, H]); every row is written exactly once whatever cu_seqlens_q
    holds, rows of no item -- behind s_B, in front of s_0, an item's rows beyond M -- as 0 / -inf, and q is never loaded there
    (NaN allowed).  block_mask / lists keep the padded layout [B|1, Hl, NQ, NK] with NQ = ceil(M / block); rows of query blocks
    i >= ceil(n_b / block) are never read.  Item b is this call on q[s_b : s_b + n_b] seen as [1, H, n_b, D] with its list rows
    and kv_len[b] (the length after the append; causal: j <= r + kv_len[b] - n_b): at an equal explicit blocks_per_split its
    bytes, and the bytes of the q_len= call on the padded copy.  q is 3-d if and only if cu_seqlens_q is given; q_len= beside it is
    refused.  Grid and workspace depend on (T, B, M) and the head counts alone (packed_row_groups): row groups are gh heads x
    qg = min(64 // gh, block, M) rows, so M = 1 runs the kernels block_sparse_decode runs; the launch holds one workgroup per
    (row group the bound QP allows, unit, head chunk, split), the live ones first, and blocks_per_split=None is
    extend_default_split(QP * units * head chunks, NK).  Three launches, capturable, a replay follows cu_seqlens_q.  The step:
        append_kv_e4m3(k_new, v_new, kc, vc, start=prev, cu_seqlens=cu, block_table=table, ...)       # k_new [T, Hkv, D]
        pool_keys(kc, kv_len=kv_len, start=prev, block_table=table, out=pooled, ...)
        lists = select_blocks_pooled(q, pooled, 16, kv_len=kv_len, cu_seqlens_q=cu, max_q_len=M, causal=True, as_lists=True)
        out, lse = block_sparse_extend(q, kc, vc, lists, kv_len=kv_len, cu_seqlens_q=cu, max_q_len=M, causal=True, ...)"""
    return _sparse_rows(True, q, k, v, block_mask, kv_len, sm_scale, block_size, causal, block_table, return_lse, blocks_per_split,
                        k_scale, v_scale, q_len, cu_seqlens_q, max_q_len)


def packed_row_groups(T: int, B: int, H: int, Hkv: int, Hl: int, max_q_len: int, block_size: int) -> Dict[str, int]:
    """How the packed block_sparse_extend sizes its launch, from host values alone: extend_row_groups'
    gh, and qg = min(64 // gh, block, M) rows per group.  An item of n rows holds pieces(n) = (n // block) * cpb +
    ceil(n % block / qg) row groups per (unit, head chunk), cpb = ceil(min(M, block) / qg).  QP bounds their sum over every
    cu_seqlens_q the device can sanitise (sum n_b <= T, n_b <= M): piece j of an item starts at row >= j * min(M, block) / cpb,
    so k non-empty items holding J pieces own at least k + (J - k) * min(M, block) / cpb rows, whence
        QP = min(B * pieces(M), k + (T - k) * cpb // min(M, block)),  k = min(B, T).
    -> dict(gh, qg, head_chunks, pieces_per_block, pieces (QP), groups (QP * max(Hl, Hkv) * head_chunks workgroups per split),
    rows16)."""
    U = max(Hl, Hkv)
    gu = H // U
    HC = -(-gu // DECODE_MAX_ROWS)
    gh = -(-gu // HC)
    qmax = min(max_q_len, block_size)
    qg = min(DECODE_MAX_ROWS // gh, qmax)
    cpb = -(-qmax // qg)
    per_item = (max_q_len // block_size) * cpb + -(-(max_q_len % block_size) // qg)
    k = min(B, T)
    QP = min(B * per_item, k + (T - k) * cpb // qmax)
    rows = gh * qg
    return dict(gh=gh, qg=qg, head_chunks=HC, pieces_per_block=cpb, pieces=QP, groups=QP * U * HC,
                rows16=16 if rows <= 16 else (32 if rows <= 32 else 64))


def _sparse_rows(ext: bool, q, k, v, block_mask, kv_len, sm_scale, block_size, causal, block_table, return_lse, blocks_per_split,
                 k_scale, v_scale, q_len=None, cu_seqlens_q=None, max_q_len=None):
    """block_sparse_decode (ext False) and block_sparse_extend: one argument layer, the C entries of either; with row counts
    (q_len, extend only) the _ragged entries, which take them in front of the stream; with cu_seqlens_q (extend only) the _packed
    entries: q [T, H, D], T in front, M = max_q_len where Sq stood, cu_seqlens_q where q_len stood."""
    blk = _check_block("block-sparse extend" if ext else "block-sparse decode", block_size)
    _check_count("blocks_per_split", blocks_per_split, 1, optional=True)
    r = _query_rows(q, q_len, cu_seqlens_q if ext else None, max_q_len, k, block_table,
                    lambda q4: _check_operands(q4, k, v, dims=(64, 128), block_table=block_table, blk=blk, kv8_ok=True))
    packed, q, B, H, Hkv, Sq, Sk, D, T = r.kind == "packed", r.q4, r.B, r.H, r.Hkv, r.Sq, r.Sk, r.D, r.T
    _check_scales(k, Hkv, k_scale=k_scale, v_scale=v_scale)
    NQ = -(-Sq // blk) if ext else 1
    if Sq > blk and not ext:
        raise ValueError(f"Sq = {Sq}: block_sparse_decode serves one query block, Sq <= block_size = {blk}")
    NKmax = min(-(-Sk // blk), MAX_KEY_BLOCKS)
    if isinstance(block_mask, dict):
        cols, counts = block_mask.get("cols"), block_mask.get("counts")
        if (not isinstance(cols, torch.Tensor) or not isinstance(counts, torch.Tensor) or cols.dtype != torch.int32
                or counts.dtype != torch.int32 or cols.dim() != 3 or cols.shape[1] != NQ or cols.shape[0] % B
                or counts.numel() != cols.shape[0] * NQ or not cols.is_contiguous() or not counts.is_contiguous()):
            if ext:
                raise ValueError(f"block_mask: a bool / uint8 tensor, or the lists of {NQ} query block(s) of {blk}: cols int32 "
                                 f"[B * Hl, {NQ}, NK] and counts int32 [B * Hl, {NQ}], contiguous (select_blocks(..., as_lists=True))")
            raise ValueError("block_mask: a bool / uint8 tensor, or the lists of one query block: cols int32 [B * Hl, 1, NK] and "
                             "counts int32 [B * Hl, 1], contiguous (select_blocks(..., as_lists=True))")
        Hl, NK = cols.shape[0] // B, cols.shape[2]
        mask = None
    else:
        mask = block_mask
        if not isinstance(mask, torch.Tensor) or mask.dim() != 4 or mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"block_mask: a 4-d bool or uint8 tensor, got {getattr(mask, 'dtype', type(mask))} "
                             f"{tuple(getattr(mask, 'shape', ()))}")
        Hl, NK = mask.shape[1], mask.shape[3]
        if mask.shape[0] not in (1, B) or mask.shape[2] != NQ:
            raise ValueError(f"block_mask {tuple(mask.shape)}: expected [{B}|1, Hl, {NQ}, 1..{NKmax}] for block {blk} "
                             + (f"(Sq = {Sq}: {NQ} query block(s))" if ext else "(one query block)"))
    if Hl not in (1, Hkv, H):
        raise ValueError(f"block_mask: a head axis of {H} (per query head), Hkv = {Hkv} (per K/V head) or 1, got {Hl}")
    if not 1 <= NK <= NKmax:
        raise ValueError(f"block_mask: {NK} key blocks, expected 1..{NKmax} for block {blk} (at most {MAX_KEY_BLOCKS} key blocks)")
    rows = Sq * (H // max(Hl, Hkv))
    if rows > DECODE_MAX_ROWS and not ext:
        raise NotImplementedError(f"Sq * H // max(Hl, Hkv) = {rows} rows share a K/V head and a list row: block_sparse_decode "
                                  f"serves at most {DECODE_MAX_ROWS}; use block_sparse_attention")
    lens = _check_limit("kv_len", kv_len, B, Sk, Sk)
    nrows = _check_limit("q_len", q_len, B, Sq, Sq)
    _check_cache(k, v)
    _core._require_device(q, k, v)
    dev = q.device
    kv_dev, kv_valid, _ = _device_limit(lens, B, Sk, dev)
    q_dev = _row_limit(nrows, B, Sq, dev) if ext else None
    scale = float(D) ** -0.5 if sm_scale is None else float(sm_scale)
    if mask is not None:
        lists = block_mask_to_lists(mask.to(dev) if mask.device != dev else mask, B, Hl)
        cols, counts = lists["cols"], lists["counts"]
    else:
        _core._require_device(cols, counts)
    table, _held = _table_args(block_table, k)
    L = _lib.lib()
    bps = 0 if blocks_per_split is None else int(blocks_per_split)
    need = ctypes.c_size_t(0)
    kv8 = k.dtype == E4M3
    if packed:
        q, cu = _packed_on_device(r)
        _lib.check(L.rsa_block_sparse_extend_packed_bytes(T, B, H, Hkv, Hl, Sq, D, blk, NK, bps, ctypes.byref(need), None),
                   "rsa_block_sparse_extend_packed_bytes")
        shape, entry = (T, H, D), "rsa_block_sparse_extend_packed"
    else:
        q = _core._as_bhsd(q)
        if ext:
            _lib.check(L.rsa_block_sparse_extend_bytes(B, H, Hkv, Hl, Sq, D, blk, NK, bps, ctypes.byref(need)),
                       "rsa_block_sparse_extend_bytes")
        else:
            _lib.check(L.rsa_block_sparse_decode_bytes(B, H, Hkv, Hl, Sq, D, NK, bps, ctypes.byref(need)),
                       "rsa_block_sparse_decode_bytes")
        shape = (B, H, Sq, D)
        entry = ("rsa_block_sparse_extend" if ext else "rsa_block_sparse_decode") + ("_ragged" if q_dev is not None else "")
    entry += "_kv8" if kv8 else ""
    ws = torch.empty((need.value,), dtype=torch.uint8, device=dev)
    out = torch.empty(shape, dtype=q.dtype, device=dev)
    lse = torch.empty(shape[:-1], dtype=torch.float32, device=dev) if return_lse else None
    held = [_scale_arg(sc, Hkv, dev) for sc in (k_scale, v_scale)] if kv8 else []
    if packed:      # T in front, M where Sq stood, q and out by their row and head strides, cu_seqlens_q where q_len stood
        lead, tq, to, held = (T,), _t3(q), RsaOut4(out.data_ptr(), 0, out.stride(1), out.stride(0)), held + [cu]
    else:
        lead, tq, to, held = (), _core._t4(q), _out4(out), held + ([q_dev] if q_dev is not None else [])
    with torch.cuda.device(dev):
        _lib.check(getattr(L, entry)(*lead, B, H, Hkv, Hl, Sq, Sk, D, _core.dtype_code(q.dtype), blk, NK, _ptr(kv_dev), kv_valid,
                                     int(bool(causal)), scale, tq, _core._t4(k), _core._t4(v), *table, cols.data_ptr(),
                                     counts.data_ptr(), bps, ws.data_ptr(), need.value, to, _ptr(lse),
                                     *[t.data_ptr() for t in held], _core._stream()), entry)
    return (out, lse) if return_lse else out


MERGE_MAX_PARTIALS = 8      # partials of one merge_partials call (rsa_merge.hip: MERGE_MAX_N)
MERGE_MAX_GRID = 2048       # workgroups of its launch, at most; 256 / (D / 8) rows each and pass, 256 / (D / 4) in the 8-byte form


def _merge_span(t: torch.Tensor):
    """The bytes a strided view touches, as [lo, hi)."""
    lo = t.data_ptr()
    return lo, lo + (sum((n - 1) * st for n, st in zip(t.shape, t.stride())) + 1) * t.element_size()


def _merge_alias(name: str, res, parts, others, pname: str):
    """A result of merge_partials against what the call reads: it may be one partial exactly, and meets nothing else."""
    lo, hi = _merge_span(res)
    for i, p in enumerate(parts):
        plo, phi = _merge_span(p)
        if lo < phi and plo < hi and not (p.data_ptr() == res.data_ptr() and p.stride() == res.stride()):
            raise ValueError(f"{name}: overlaps {pname}[{i}] without being it (the result may alias one partial exactly: the same "
                             f"pointer and the same strides)")
    for oname, o in others:
        if o is not None and o.device == res.device:
            olo, ohi = _merge_span(o)
            if lo < ohi and olo < hi:
                raise ValueError(f"{name}: overlaps {oname}")


def merge_partials(outs, lses, *, sink=None, out: Optional[torch.Tensor] = None, lse: Optional[torch.Tensor] = None,
                   return_lse: bool = True):
    """The merge of N attention partials over disjoint key sets into the result over their union (rsa_merge_partials, DESIGN.md
    section 5.20): another rank's share of a key-sharded cache, a shared prefix beside each item's suffix (cascade), a dense local
    branch beside the selected blocks, attention-sink logits.  Partial i is what block_sparse_decode / block_sparse_extend return
    with return_lse=True: out_i (bf16 or fp16, one type for all) and lse_i (fp32, natural log).
    outs: a sequence of 1 <= N <= 8 tensors of one shape, dtype and device -- [B,H,Sq,D] or packed [T,H,D], D in {64, 128} -- or
    one stacked tensor [N, ...] (what all_gather_into_tensor fills); lses matches it: [B,H,Sq] / [T,H] each, or stacked.
    sink: None, a float (-inf: no sink), or a float32 device tensor of 1 or H values: one more partial whose out is zero and whose
    lse is sink[h] for every row of head h.
    Per row, in fp32, the partials in ascending order and the sink last: m* = max of the live lse_i (live: > -inf), w_i =
    exp2((lse_i - m*) * log2 e), acc = fmaf(w_i, out_i, acc) and l = l + w_i over the live partials -- one that is not live is
    skipped, never multiplied: its out may hold NaN (the rows extend writes as 0 / -inf, rows of padding) --, the sink's weight into
    l alone, out = acc / l rounded once, lse = m* + ln 2 * log2 l; a row without a live entry is 0 / -inf.  A row with exactly one
    live entry returns that partial's bytes; two calls give the same bytes.  A +inf lse is the caller's error and garbles its
    own row alone.
    No copies: views go through as strides -- a contiguous head dim, every other stride a multiple of 4 elements, the pointer
    8-byte aligned (where every pointer is 16-byte aligned and every stride a multiple of 8 a lane moves 16 bytes, else 8: the
    same bytes); the lse tensors take any strides.  A tensor outside that is refused (ValueError naming it), not made contiguous.
    out= / lse=: preallocated results under the same rule; out may be one of outs and lse one of lses (an in-place accumulate),
    any other overlap is refused.  Returns (out, lse), or out with return_lse=False (lse= is then not written).
    One launch, no workspace, no host read: asynchronous on the current stream and capturable in a HIP graph.  CPU tensors are
    refused: there is no fallback."""
    def parts(name, x, ranks):
        if isinstance(x, torch.Tensor):
            if x.dim() - 1 not in ranks:
                raise ValueError(f"{name}: a sequence of tensors or one stacked tensor [N, ...], got a tensor {tuple(x.shape)}")
            x = x.unbind(0)
        elif not isinstance(x, (list, tuple)) or not all(isinstance(t, torch.Tensor) for t in x):
            raise ValueError(f"{name}: a sequence of tensors or one stacked tensor [N, ...], got {type(x).__name__}")
        return list(x)
    po, pl = parts("outs", outs, (3, 4)), parts("lses", lses, (2, 3))
    N = len(po)
    if not 1 <= N <= MERGE_MAX_PARTIALS:
        raise ValueError(f"outs: 1..{MERGE_MAX_PARTIALS} partials, got {N}")
    if len(pl) != N:
        raise ValueError(f"lses: {len(pl)} log-sum-exps for {N} partials")
    o0 = po[0]
    if o0.dim() not in (3, 4):
        raise ValueError(f"outs[0]: [B, H, Sq, D] or packed [T, H, D], got {tuple(o0.shape)}")
    if o0.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"outs: one dtype, bfloat16 or float16 (the partials decode and extend return), got {o0.dtype}")
    shape, D, H = tuple(o0.shape), o0.shape[-1], o0.shape[1]       # ([B, H, Sq, D] and packed [T, H, D] alike)
    if D not in (64, 128):
        if D in HEAD_DIMS:
            raise NotImplementedError(f"head dim {D}: this call serves (64, 128)")
        raise ValueError(f"head dim {D}: one of (64, 128)")
    if 0 in shape:
        raise ValueError(f"empty operands {shape}")

    def held(name, t, want_shape, want_dtype, two_byte, result=False):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != want_shape or t.dtype != want_dtype or t.device != o0.device:
            raise ValueError(f"{name}: a {want_dtype} tensor {want_shape} on {o0.device}, got {getattr(t, 'dtype', type(t))} "
                             f"{tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}")
        if two_byte:
            *outer, inner = t.stride()
            if inner != 1 or any(st % 4 or st < 0 for st in outer) or t.data_ptr() % 8:
                raise ValueError(f"{name}: a contiguous head dim, strides that are non-negative multiples of 4 elements and an 8-byte "
                                 f"aligned pointer (a partial is not copied), got strides {tuple(t.stride())}, pointer % 8 = "
                                 f"{t.data_ptr() % 8}")
        elif any(st < 0 for st in t.stride()):
            raise ValueError(f"{name}: non-negative strides, got {tuple(t.stride())}")
        if result and any(st <= 0 for n, st in zip(t.shape, t.stride()) if n > 1):
            raise ValueError(f"{name}: a result is written once per element: positive strides, got {tuple(t.stride())}")
    for i in range(N):
        held(f"outs[{i}]", po[i], shape, o0.dtype, True)
        held(f"lses[{i}]", pl[i], shape[:-1], torch.float32, False)
    if isinstance(sink, torch.Tensor):
        if sink.dtype != torch.float32 or sink.numel() not in (1, H):
            raise ValueError(f"sink: a float32 tensor of 1 or {H} values, got {sink.dtype} {tuple(sink.shape)}")
        if sink.device != o0.device:
            raise ValueError(f"sink is on {sink.device}, the partials on {o0.device}")
    elif sink is not None and (isinstance(sink, bool) or not isinstance(sink, (int, float)) or not float(sink) < float("inf")):
        raise ValueError(f"sink: None, a float below +inf or a float32 tensor of 1 or {H} values, got {sink!r}")
    if out is not None:
        held("out", out, shape, o0.dtype, True, result=True)
        _merge_alias("out", out, po, [(f"lses[{i}]", t) for i, t in enumerate(pl)] + [("sink", sink if isinstance(sink, torch.Tensor) else None)],
                     "outs")
    if lse is not None:
        if not return_lse:
            raise ValueError("lse= belongs to return_lse=True")
        held("lse", lse, shape[:-1], torch.float32, False, result=True)
        _merge_alias("lse", lse, pl, [(f"outs[{i}]", t) for i, t in enumerate(po)] + [("out", out), ("sink", sink if isinstance(sink, torch.Tensor) else None)],
                     "lses")
    _core._require_device(*po, *pl)
    dev = o0.device
    if out is None:
        out = torch.empty(shape, dtype=o0.dtype, device=dev)
    if lse is None and return_lse:
        lse = torch.empty(shape[:-1], dtype=torch.float32, device=dev)
    sink_dev = None
    if isinstance(sink, torch.Tensor):
        sink_dev = sink.reshape(-1).expand(H).contiguous()
    elif sink is not None and float(sink) > float("-inf"):      # (a Python float is filled in by torch: capturable)
        sink_dev = torch.full((H,), float(sink), dtype=torch.float32, device=dev)
    if len(shape) == 4:
        B, S = shape[0], shape[2]
        t4 = lambda t: (t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))        # noqa: E731
        l3 = lambda t: (t.stride(0), t.stride(1), t.stride(2))                      # noqa: E731
    else:       # packed [T, H, D] / [T, H]: one item of T rows, stride_s the row's and stride_h the head's
        B, S = 1, shape[0]
        t4 = lambda t: (t.data_ptr(), 0, t.stride(1), t.stride(0))                  # noqa: E731
        l3 = lambda t: (0, t.stride(1), t.stride(0))                                # noqa: E731
    c_outs = (RsaTensor4 * N)(*[RsaTensor4(*t4(t)) for t in po])
    c_lses = (ctypes.c_void_p * N)(*[t.data_ptr() for t in pl])
    c_strides = (ctypes.c_int64 * (3 * N))(*[st for t in pl for st in l3(t)])
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().rsa_merge_partials(N, B, H, S, D, _core.dtype_code(o0.dtype), c_outs, c_lses, c_strides, _ptr(sink_dev),
                                                 RsaOut4(*t4(out)), _ptr(lse), *(l3(lse) if lse is not None else (0, 0, 0)),
                                                 _core._stream()), "rsa_merge_partials")
    return (out, lse) if return_lse else out


def build_block_index(query: torch.Tensor, key: torch.Tensor, top_k: int, block_size_M: int = 128, block_size_N: int = 128,
                      text_start_block=None, text_end_block=None, num_blocks=None, prob_threshold: float = 0.7,
                      block_neighbor_list=None, attenable=None, first_frame_blocks=None, text: bool = True):
    """The reference's _build_block_index_with_importance_optimized on the rectified call's selection pass (K1..K3).
    query [B,H,NQ*block,D] (the visual rows), key [B,H,S,D] -> (one_hot bool [B,H,NQ,num_blocks], probs fp32 [B,H,NQ,L],
    nogapr bool [B,H,NQ,NQ]).  text=True: the hunyuan / flux / cogvideo form (`attenable` text tokens after the visual blocks are
    scored one by one, text blocks [NQ, text_end_block) kept by every row, L = NQ + 1); text=False: the wan21 form (L = NQ,
    `first_frame_blocks` square kept).  K1 pools V as well: K stands in for it and its pool is dropped.  The inputs are not
    modified (the reference's callers zero masked K rows themselves beforehand)."""
    blk = _check_block_pair(block_size_M, block_size_N)
    if query.dim() != 4 or key.dim() != 4:
        raise ValueError("query, key: [B, H, S, D] tensors")
    B, H, Sq, D = query.shape
    S = key.shape[2]
    if key.shape[0] != B or key.shape[1] != H or key.shape[3] != D:
        raise ValueError(f"key {tuple(key.shape)} does not match query {tuple(query.shape)}")
    if query.dtype not in (torch.bfloat16, torch.float16) or key.dtype != query.dtype:
        raise ValueError(f"query, key: one dtype, bfloat16 or float16 (got {query.dtype}, {key.dtype})")
    if D not in (16, 32, 64, 128):
        raise ValueError(f"head dim {D}: 16, 32, 64 or 128")
    NQ = -(-Sq // blk)
    NB = -(-S // blk)
    as_int = lambda x: int(x.reshape(-1)[0].item()) if isinstance(x, torch.Tensor) else int(x)   # noqa: E731
    if num_blocks is not None and as_int(num_blocks) != NB:
        raise ValueError(f"num_blocks = {as_int(num_blocks)}, but key has {S} rows = {NB} blocks of {blk}")
    if text_start_block is not None and as_int(text_start_block) != NQ:
        raise ValueError(f"text_start_block = {as_int(text_start_block)}: the selection pass starts the text at the end of the "
                         f"{NQ} query blocks")
    if Sq % blk and Sq != S:
        raise ValueError(f"query: {Sq} rows are not whole blocks of {blk} and not the whole key sequence ({S})")
    if NQ > NB:
        raise ValueError(f"query has {NQ} blocks, key only {NB}")
    if text:
        n_txt = 0 if attenable is None else as_int(attenable)
        teb = NB if text_end_block is None else min(max(as_int(text_end_block), NQ), NB)
        ffb = 0
        if n_txt < 0 or NQ * blk + n_txt > S:
            raise ValueError(f"attenable = {n_txt} text tokens do not fit behind {NQ} blocks of {blk} in {S} key rows")
    else:
        if NQ != NB:
            raise ValueError(f"wan21 selection: query blocks ({NQ}) and key blocks ({NB}) must agree")
        n_txt, teb, ffb = 0, NB, 0 if first_frame_blocks is None else as_int(first_frame_blocks)
    _core._require_device(query, key)
    if D in _core._PAD_HEAD_DIM:   # (bit-identical selection: see _core._PAD_HEAD_DIM)
        query, key, _ = _core.pad_small_head_dim(query, key, key)
        D = query.shape[-1]
    query, key = _core._as_bhsd(query), _core._as_bhsd(key)
    spec = _core.LayoutSpec(S, NB, NQ, n_txt, S, S, teb, ffb, 0, S, blk)
    dev = query.device
    names = ("qbar", "aq", "kbar", "ak", "vbar", "scores", "unrel", "probs", "w", "R", "bitmask", "cols", "counts")
    shapes = _core.buffer_shapes(spec, B, H, D)
    bufs = {n: torch.empty(shapes[n], dtype=_core._BUF_DTYPES[n], device=dev) for n in names}
    cb = _lib.RsaBuffers(*[bufs[n].data_ptr() if n in bufs and bufs[n].numel() else None for n in _lib.BUFFER_NAMES], 0)
    nbr = _core.neighbor_on_device(block_neighbor_list, NQ, dev)
    L = _lib.lib()
    tq, tk = _core._t4(query), _core._t4(key)
    ex = blk != _lib.BLOCK
    lay = spec.to_c_ex(B, H, D, query.dtype) if ex else spec.to_c(B, H, D, query.dtype)
    sfx = "_ex" if ex else ""
    st, lp, cbp = _core._stream(), ctypes.byref(lay), ctypes.byref(cb)
    with torch.cuda.device(dev):
        _lib.check(getattr(L, "rsa_pool_stats" + sfx)(lp, tq, tk, tk, cbp, st), "rsa_pool_stats")
        _lib.check(getattr(L, "rsa_pooled_scores" + sfx)(lp, tk, cbp, st), "rsa_pooled_scores")
        _lib.check(getattr(L, "rsa_select_mask" + sfx)(lp, nbr.data_ptr() if nbr is not None else None, int(top_k),
                                                       float(prob_threshold), cbp, st), "rsa_select_mask")
    one_hot = lists_to_block_mask(bufs["bitmask"], B, H, NQ, NB).view(torch.bool)
    probs = bufs["probs"].view(B, H, NQ, spec.L)
    nogapr = bufs["unrel"].view(B, H, NQ, NQ).view(torch.bool)
    return one_hot, probs, nogapr


def triton_block_sparse_attention_onehot(q, k, v, seqlens, block_mask, sm_scale, block_size_M=128, block_size_N=128):
    """The reference's _triton_block_sparse_attention_onehot: [B,H,S,D] x3, seqlens [B] (the key limit per batch item),
    block_mask [B,H,NQ,NB] -> [B,H,S,D].  Query blocks come from block_mask.shape[-2]: rows past NQ * block are 0, as the
    reference's zero-initialised output leaves them."""
    blk = _check_block_pair(block_size_M, block_size_N)
    Sq = q.shape[2]
    NQ = block_mask.shape[-2]
    rows = min(Sq, NQ * blk)
    nq = -(-rows // blk)
    if nq < NQ:
        block_mask = block_mask[:, :, :nq]
    o = block_sparse_attention(q[:, :, :rows], k, v, block_mask, kv_len=seqlens, sm_scale=sm_scale, block_size=blk)
    if rows == Sq:
        return o
    full = torch.zeros_like(q, memory_format=torch.contiguous_format)
    full[:, :, :rows] = o
    return full
