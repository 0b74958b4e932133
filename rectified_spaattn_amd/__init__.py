"""rectified_spaattn_amd -- MI355X-native Rectified SpaAttn attention path.

Module names mirror the reference package `rectified_spaattn`:
    attn                      fullattn, get_cu_seqlens, get_attn_mask, get_flash_attn_params, MEMORY_LAYOUT
    gapr_mask                 estimate_pr_gain
    rectified_hunyuan_attn    rectified_block_sparse_attention, RectifiedHunyuanVideoSpaAttnProcessor2_0
    rectified_flux_attn       rectified_block_sparse_attention, RectifiedFluxSpaAttnProcessor2_0
    rectified_wan21_attn      rectified_block_sparse_attention, RectifiedWan{T2V,I2V}SpaAttnProcessor2_0
    rectified_wan22_attn      RectifiedWan{TI2V,T2V,I2V}SpaAttnProcessor2_0
    rectified_cogvideo_attn   rectified_block_sparse_attention, RectifiedCogVideoXVideoSpaAttnProcessor2_0
    attn_processor            get_attn_processors, set_attn_processor
    block_sparse              block_sparse_attention over a caller's block mask, block_sparse_decode (its decode half: few query rows over a
                              (paged) K/V cache, with log-sum-exp; 2-byte or e4m3 with append_kv_e4m3 as its writer), block_sparse_extend (the same
                              over a chunk of any number of query rows: chunked prefill, a second turn, a draft's verification) and select_blocks, the top-k block selection
                              per K/V head that makes one (both also exported here), the mask <-> list conversions; the four rectified_*_attn modules above also carry the reference's
                              _build_block_index_with_importance_optimized and _triton_block_sparse_attention_onehot
    teacache                  TeaCache step-skipping controller (scripts' teacache_forward bookkeeping), rel_l1_distance
Device work goes through librsa_hip.so (C-ABI in include/rsa.h): the attention operators and fullattn never fall back to
PyTorch kernels for device tensors (they raise).  Two deliberate uses of plain PyTorch expressions remain and are the
reference's own code paths: fullattn(mode="torch" | "vanilla") on CPU tensors (BASELINE config 1) and
teacache.rel_l1_distance for CPU tensors / small fp32 inputs such as timestep embeddings (bf16 / fp16 device tensors take
the one-pass HIP reduction rsa_rel_l1).
"""
__version__ = "0.5.0"


def set_qkv_fp8(enabled):
    """Run the block-sparse kernel of every sparse operator / processor call on e4m3 operands (fp8 MFMA): True = e4m3 images of
    Q, K, V (head dim 64 / 128; relative L1 distance 0.12 of the layer output from the 2-byte path), "pv" = Q . K^T on the 2-byte
    inputs and only P . V on e4m3 (head dims 64 and 128; relative L1 0.04, within SURVEY 8(d)'s 8e-2 of the bf16 oracle); returns the
    previous setting.  Default off = the reference's input-dtype behaviour."""
    from . import _operator
    return _operator.set_qkv_fp8(enabled)


def set_dense_fp8(enabled) -> bool:
    """Run fullattn's device path (dense attention, head dims 64 / 128) on e4m3 images of Q, K, V (True), or -- "pv" -- take the
    scores from the 2-byte q and k and use e4m3 only for P and V (relative L1 0.04 instead of 0.12); returns the previous setting.
    Default off."""
    from . import _operator
    return _operator.set_dense_fp8(enabled)


def block_sparse_attention(q, k, v, block_mask, *, kv_len=None, sm_scale=None, block_size=128, causal=False, window=None,
                           row_range=None):
    """Block-sparse attention over a block mask of the caller's own: q [B,H,Sq,D], k / v [B,H,Sk,D], block_mask bool / uint8
    [B|1, H|1, ceil(Sq/block), NK] -> [B,H,Sq,D]; causal / window=(left, right) / row_range=(lo, hi) add a key range per query
    row; k / v may hold Hkv < H heads (GQA / MQA: query head h reads K/V head h // (H // Hkv); mask head axis H, Hkv or 1).
    See rectified_spaattn_amd.block_sparse.block_sparse_attention."""
    from . import block_sparse
    return block_sparse.block_sparse_attention(q, k, v, block_mask, kv_len=kv_len, sm_scale=sm_scale, block_size=block_size,
                                               causal=causal, window=window, row_range=row_range)


def select_blocks(q, k, top_k, *, block_size=128, kv_len=None, causal=False, keep_first=0, keep_local=0, mask_heads="kv",
                  return_scores=False, as_lists=False, top_p=None, score_scale=None, return_mass=False, q_len=None):
    """Top-k key blocks per query block by pooled scores, per K/V head (mask_heads="q": per query head), on the device: q
    [B,H,Sq,D], k [B,Hkv,Sk,D] -> bool block mask [B, Hkv|H, ceil(Sq/block), ceil(Sk/block)] for block_sparse_attention with
    the same kv_len / causal / block_size; keep_first / keep_local force the first blocks and the diagonal band.  top_p in
    [0, 1]: a budget per row, the shortest prefix of the ranking whose softmax mass (at score_scale) reaches top_p, capped at
    top_k; return_mass=True adds the kept mass, fp32 [B, Hkv|H, NQ].  q_len (kv_len's forms): the rows of each item of a ragged
    batch padded to Sq -- item b is selected as q[b, :, :q_len[b]] would be, its query blocks without a row keep nothing.
    See rectified_spaattn_amd.block_sparse.select_blocks."""
    from . import block_sparse
    return block_sparse.select_blocks(q, k, top_k, block_size=block_size, kv_len=kv_len, causal=causal, keep_first=keep_first,
                                      keep_local=keep_local, mask_heads=mask_heads, return_scores=return_scores,
                                      as_lists=as_lists, top_p=top_p, score_scale=score_scale, return_mass=return_mass,
                                      q_len=q_len)


def block_sparse_decode(q, k, v, block_mask, *, kv_len=None, sm_scale=None, block_size=128, causal=False, block_table=None,
                        return_lse=False, blocks_per_split=None, k_scale=None, v_scale=None):
    """Block-sparse decode attention: q [B,H,Sq,D] with Sq <= block over a K/V cache [B,Hkv,Sk,D], or over page pools
    [P,Hkv,block,D] behind block_table int32 [B,NKt]; block_mask bool / uint8 [B|1, Hl, 1, NK] or select_blocks' lists;
    return_lse=True adds the fp32 log-sum-exp [B,H,Sq].  k / v float8_e4m3fn with k_scale / v_scale (one fp32 scale per K/V
    head): the one-byte cache append_kv_e4m3 writes.  No q_len: a ragged decode batch is block_sparse_extend(q_len=), with this
    call's bytes.  See rectified_spaattn_amd.block_sparse.block_sparse_decode."""
    from . import block_sparse
    return block_sparse.block_sparse_decode(q, k, v, block_mask, kv_len=kv_len, sm_scale=sm_scale, block_size=block_size,
                                            causal=causal, block_table=block_table, return_lse=return_lse,
                                            blocks_per_split=blocks_per_split, k_scale=k_scale, v_scale=v_scale)


def block_sparse_extend(q, k, v, block_mask, *, kv_len=None, sm_scale=None, block_size=128, causal=False, block_table=None,
                        return_lse=False, blocks_per_split=None, k_scale=None, v_scale=None, q_len=None,
                        cu_seqlens_q=None, max_q_len=None):
    """Block-sparse extend attention: a chunk q [B,H,Sq,D] of any length over a K/V cache that already holds a prefix --
    block_sparse_decode without the one-query-block and 64-row limits; block_mask bool / uint8 [B|1, Hl, ceil(Sq/block), NK] or
    select_blocks' lists for that many query blocks; causal is bottom-right aligned; return_lse=True adds the fp32 log-sum-exp
    [B,H,Sq].  q_len (kv_len's forms; a device tensor is never read on the host): the rows of each item of a ragged batch padded
    to Sq -- prefill chunks, decode items and draft verifications in one call of fixed shape; item b's rows < q_len[b] are this
    call on q[b, :, :q_len[b]], the rows beyond are 0 / -inf.  cu_seqlens_q (device int32 [B + 1], sanitised on the device, never
    read on the host) with max_q_len: the packed batch -- q [T, H, D], out [T, H, D], lse [T, H], item b = rows cu[b] .. cu[b + 1]
    with this call's bytes, the grid sized from T.  See rectified_spaattn_amd.block_sparse.block_sparse_extend."""
    from . import block_sparse
    return block_sparse.block_sparse_extend(q, k, v, block_mask, kv_len=kv_len, sm_scale=sm_scale, block_size=block_size,
                                            causal=causal, block_table=block_table, return_lse=return_lse,
                                            blocks_per_split=blocks_per_split, k_scale=k_scale, v_scale=v_scale, q_len=q_len,
                                            cu_seqlens_q=cu_seqlens_q, max_q_len=max_q_len)


def pool_keys(k, *, block_size=128, kv_len=None, block_table=None, out=None, start=None, workgroups_per_head=None, k_scale=None):
    """The cache of pooled keys for select_blocks_pooled: k [B,Hkv,Sk,D] (or a page pool behind block_table) -> fp32
    [B, Hkv, ceil(Sk/block), D]; with start= and out= only the blocks from start // block up to kv_len are written again; k
    float8_e4m3fn with k_scale: from the one-byte cache.  See rectified_spaattn_amd.block_sparse.pool_keys."""
    from . import block_sparse
    return block_sparse.pool_keys(k, block_size=block_size, kv_len=kv_len, block_table=block_table, out=out, start=start,
                                  workgroups_per_head=workgroups_per_head, k_scale=k_scale)


def append_kv_e4m3(k_new, v_new, k_cache, v_cache, *, start, k_scale, v_scale, n_new=None, block_size=128, block_table=None,
                   cu_seqlens=None):
    """The writer of the one-byte K/V cache: k_new / v_new [B,Hkv,T,D] (bf16 / fp16) become float8_e4m3fn codes under one static
    fp32 scale per K/V head, at positions start[b] + t of k_cache / v_cache [B,Hkv,Sk,D] or of page pools behind block_table.
    cu_seqlens (device int32 [B + 1]): the packed form, k_new / v_new [T,Hkv,D].
    See rectified_spaattn_amd.block_sparse.append_kv_e4m3."""
    from . import block_sparse
    return block_sparse.append_kv_e4m3(k_new, v_new, k_cache, v_cache, start=start, k_scale=k_scale, v_scale=v_scale,
                                       n_new=n_new, block_size=block_size, block_table=block_table, cu_seqlens=cu_seqlens)


def select_blocks_pooled(q, pooled_k, top_k, *, block_size=128, kv_len=None, causal=False, keep_first=0, keep_local=0,
                         mask_heads="kv", return_scores=False, as_lists=False, score_splits=None, top_p=None, score_scale=None,
                         return_mass=False, q_len=None, cu_seqlens_q=None, max_q_len=None):
    """select_blocks from a cache of pooled keys (pool_keys) in place of k: the same bytes without a pass over K, with top_p and
    q_len too; with cu_seqlens_q / max_q_len for a packed q [T, H, D] (block_sparse_extend's packed batch).
    See rectified_spaattn_amd.block_sparse.select_blocks_pooled."""
    from . import block_sparse
    return block_sparse.select_blocks_pooled(q, pooled_k, top_k, block_size=block_size, kv_len=kv_len, causal=causal,
                                             keep_first=keep_first, keep_local=keep_local, mask_heads=mask_heads,
                                             return_scores=return_scores, as_lists=as_lists, score_splits=score_splits,
                                             top_p=top_p, score_scale=score_scale, return_mass=return_mass, q_len=q_len,
                                             cu_seqlens_q=cu_seqlens_q, max_q_len=max_q_len)


def pool_key_bounds(k, *, block_size=128, kv_len=None, block_table=None, out=None, start=None, workgroups_per_head=None,
                    k_scale=None):
    """The cache of per-channel key bounds for select_blocks_bound: pool_keys' arguments -> fp32 [B, Hkv, ceil(Sk/block), 2, D],
    [..., 0, :] the minimum and [..., 1, :] the maximum of each block's keys below kv_len; updated block by block with start= and
    out= as pool_keys is.  See rectified_spaattn_amd.block_sparse.pool_key_bounds."""
    from . import block_sparse
    return block_sparse.pool_key_bounds(k, block_size=block_size, kv_len=kv_len, block_table=block_table, out=out, start=start,
                                        workgroups_per_head=workgroups_per_head, k_scale=k_scale)


def select_blocks_bound(q, key_bounds, top_k, *, block_size=128, kv_len=None, causal=False, keep_first=0, keep_local=0,
                        mask_heads="kv", return_scores=False, as_lists=False, score_splits=None, top_p=None, score_scale=None,
                        return_mass=False, q_len=None, cu_seqlens_q=None, max_q_len=None):
    """select_blocks_pooled from the cache of pool_key_bounds: a key block scores by the upper bound of q . k over every key it
    could hold, sum_d max(q_d min_d, q_d max_d) (Quest's criterion: training-free sparse decode of a dense model); everything
    behind the score is select_blocks_pooled's.  See rectified_spaattn_amd.block_sparse.select_blocks_bound."""
    from . import block_sparse
    return block_sparse.select_blocks_bound(q, key_bounds, top_k, block_size=block_size, kv_len=kv_len, causal=causal,
                                            keep_first=keep_first, keep_local=keep_local, mask_heads=mask_heads,
                                            return_scores=return_scores, as_lists=as_lists, score_splits=score_splits,
                                            top_p=top_p, score_scale=score_scale, return_mass=return_mass, q_len=q_len,
                                            cu_seqlens_q=cu_seqlens_q, max_q_len=max_q_len)


def merge_partials(outs, lses, *, sink=None, out=None, lse=None, return_lse=True):
    """The merge of N <= 8 attention partials (out_i, lse_i) over disjoint key sets -- what block_sparse_decode / block_sparse_extend
    return with return_lse=True -- into the result over their union, with optional attention-sink logits: one launch, no copy, the
    same bytes from two calls.  See rectified_spaattn_amd.block_sparse.merge_partials."""
    from . import block_sparse
    return block_sparse.merge_partials(outs, lses, sink=sink, out=out, lse=lse, return_lse=return_lse)


def block_sparse_attention_backward(dout, q, k, v, out, block_mask, *, kv_len=None, sm_scale=None, block_size=128, causal=False,
                                    window=None, row_range=None):
    """(dq, dk, dv) of block_sparse_attention(q, k, v, block_mask, ...) for the upstream gradient dout of its result out: three
    launches for the whole batch, no float atomics, the same bytes from two calls.  See
    rectified_spaattn_amd.block_sparse.block_sparse_attention_backward."""
    from . import block_sparse
    return block_sparse.block_sparse_attention_backward(dout, q, k, v, out, block_mask, kv_len=kv_len, sm_scale=sm_scale,
                                                        block_size=block_size, causal=causal, window=window, row_range=row_range)


def block_sparse_attention_autograd(q, k, v, block_mask, *, kv_len=None, sm_scale=None, block_size=128, causal=False, window=None,
                                    row_range=None):
    """block_sparse_attention as a differentiable call: the forward's bytes, and .backward() fills q.grad, k.grad and v.grad through
    block_sparse_attention_backward.  See rectified_spaattn_amd.block_sparse.block_sparse_attention_autograd."""
    from . import block_sparse
    return block_sparse.block_sparse_attention_autograd(q, k, v, block_mask, kv_len=kv_len, sm_scale=sm_scale,
                                                        block_size=block_size, causal=causal, window=window, row_range=row_range)


def clear_buffer_cache() -> None:
    """Drops the intermediate buffers the operators keep per (geometry, device, stream) between calls (about 0.45 GB per
    set at the HunyuanVideo shape; `_core.BUFFER_CACHE_MAX_BYTES` bounds the total, `_core.BUFFER_CACHE = False` turns the
    cache off).  Calls inside a HIP-graph capture never use the cache."""
    from . import _core
    _core.clear_buffer_cache()
