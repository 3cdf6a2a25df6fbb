"""Host wrappers for the fused decode-step neighbours of the QLinear calls (csrc/decode_ops.hip,
SURVEY.md 8f row N1).  Each replaces a handful of tiny torch launches with one HIP launch and keeps the
model graph's rounding sequence (chatglm_q/model.py, lines cited in include/qlinear_hip.h)."""
from __future__ import annotations

import os

import numpy as np
import torch
from torch import Tensor

from . import _lib


def rmsnorm(x: Tensor, weight: Tensor, eps: float) -> Tensor:
    lib = _lib.get_lib()
    x2 = x.reshape(-1, x.shape[-1])
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    out = torch.empty((x2.shape[0], x2.shape[1]), device=x.device, dtype=x.dtype)
    with torch.cuda.device(x.device):
        st = lib.qlinear_rmsnorm(x2.data_ptr(), weight.data_ptr(), out.data_ptr(), x2.shape[0], x2.shape[1],
                                 x2.stride(0) if x2.shape[0] > 1 else x2.shape[1], x2.shape[1], float(eps),
                                 _lib.dtype_code(x.dtype), _lib.stream_ptr(x.device))
    _lib.check(st, "qlinear_rmsnorm")
    return out.reshape(x.shape)


def add_rmsnorm(x: Tensor, delta: Tensor, weight: Tensor, eps: float):
    """h = x + delta (rounded), out = rmsnorm(h) * weight in ONE launch.  Returns (h, out)."""
    lib = _lib.get_lib()
    shape = x.shape
    x2 = x.reshape(-1, shape[-1]).contiguous()
    d2 = delta.reshape(-1, shape[-1]).contiguous()
    h = torch.empty_like(x2)
    out = torch.empty_like(x2)
    with torch.cuda.device(x.device):
        st = lib.qlinear_add_rmsnorm(x2.data_ptr(), d2.data_ptr(), weight.data_ptr(), h.data_ptr(), out.data_ptr(),
                                     x2.shape[0], x2.shape[1], x2.shape[1], float(eps), _lib.dtype_code(x.dtype),
                                     _lib.stream_ptr(x.device))
    _lib.check(st, "qlinear_add_rmsnorm")
    return h.reshape(shape), out.reshape(shape)


def rmsnorm_quant(x: Tensor, weight: Tensor, eps: float, delta: Tensor | None = None, want_out: bool = False):
    """RMSNorm (of ``x + delta`` when ``delta`` is given) emitted as int8 rows + one fp32 scale per row in the SAME launch
    (``qlinear_rmsnorm_quant_i8``): bit for bit ``act_quant_rowwise(rmsnorm(...))``.  Returns ``(h, a_q, a_scale, out)``:
    ``h`` = the rounded ``x + delta`` (``x`` itself without delta), ``out`` = the 16-bit row only with ``want_out``."""
    lib = _lib.get_lib()
    shape = x.shape
    x2 = x.reshape(-1, shape[-1]).contiguous()
    rows, dim = x2.shape
    d2 = delta.reshape(-1, dim).contiguous() if delta is not None else None
    h = torch.empty_like(x2) if d2 is not None else x2
    out = torch.empty_like(x2) if want_out else None
    a_q = torch.empty((rows, dim), device=x.device, dtype=torch.int8)
    a_s = torch.empty((rows,), device=x.device, dtype=torch.float32)
    if rows:
        with torch.cuda.device(x.device):
            st = lib.qlinear_rmsnorm_quant_i8(x2.data_ptr(), _lib.ptr(d2), weight.data_ptr(), h.data_ptr() if d2 is not None else None,
                                              _lib.ptr(out), a_q.data_ptr(), a_s.data_ptr(), rows, dim, dim, float(eps),
                                              _lib.dtype_code(x.dtype), _lib.stream_ptr(x.device))
        _lib.check(st, "qlinear_rmsnorm_quant_i8")
    return h.reshape(shape), a_q, a_s, (out.reshape(shape) if out is not None else None)


def silu_mul_quant(x: Tensor, hidden: int, want_out: bool = False):
    """``silu(x[..., :hidden]) * x[..., hidden:]`` as int8 rows + scales in one launch (``qlinear_silu_mul_quant_i8``): bit for
    bit ``act_quant_rowwise(silu_mul(x, hidden))``.  Returns ``(a_q, a_scale, out_or_None)``."""
    lib = _lib.get_lib()
    x2 = x.reshape(-1, x.shape[-1])
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    rows = x2.shape[0]
    out = torch.empty((rows, hidden), device=x.device, dtype=x.dtype) if want_out else None
    a_q = torch.empty((rows, hidden), device=x.device, dtype=torch.int8)
    a_s = torch.empty((rows,), device=x.device, dtype=torch.float32)
    if rows:
        with torch.cuda.device(x.device):
            st = lib.qlinear_silu_mul_quant_i8(x2.data_ptr(), _lib.ptr(out), a_q.data_ptr(), a_s.data_ptr(), rows, hidden,
                                               x2.stride(0) if rows > 1 else 2 * hidden, hidden, _lib.dtype_code(x.dtype),
                                               _lib.stream_ptr(x.device))
        _lib.check(st, "qlinear_silu_mul_quant_i8")
    return a_q, a_s, (out.reshape(*x.shape[:-1], hidden) if out is not None else None)


def _check_rope_table(table: Tensor, k_cache: Tensor, d_head: int):
    """The kernels clamp positions to [0, capacity] (1-based positions: row r holds position <= r + 1) and skip cache
    rows outside the cache - the ABI carries no table length - so the rotary table must hold capacity + 1 positions."""
    if table.numel() < (k_cache.shape[1] + 1) * d_head:
        raise ValueError(f"rotary table of {table.numel() // d_head} positions does not cover a cache of {k_cache.shape[1]} rows "
                         f"(positions 0..{k_cache.shape[1]})")


def rope_kv_write(qkv: Tensor, table: Tensor, pos: Tensor, write_index: Tensor, k_cache: Tensor, v_cache: Tensor,
                  n_head: int, n_groups: int, d_head: int) -> Tensor:
    """qkv (B, S, (H+2G) D) -> rotated q (B, S, H*D); rotated k and v are written into the caches in place."""
    lib = _lib.get_lib()
    B, S, W = qkv.shape
    _check_rope_table(table, k_cache, d_head)
    qkv = qkv.contiguous()
    q = torch.empty((B, S, n_head * d_head), device=qkv.device, dtype=qkv.dtype)
    with torch.cuda.device(qkv.device):
        st = lib.qlinear_rope_kv_write(qkv.data_ptr(), table.data_ptr(), pos.contiguous().data_ptr(),
                                       write_index.data_ptr(), q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                                       B, S, n_head, n_groups, d_head, k_cache.shape[1], W,
                                       _lib.dtype_code(qkv.dtype), _lib.stream_ptr(qkv.device))
    _lib.check(st, "qlinear_rope_kv_write")
    return q


def decode_attention(q: Tensor, k_cache: Tensor, v_cache: Tensor, mask: Tensor, n_head: int, n_groups: int,
                     d_head: int) -> Tensor:
    """q (B, 1, H*D), caches (B, capacity, G, D), mask (B, 1, capacity) additive fp32 -> (B, 1, H*D)."""
    lib = _lib.get_lib()
    B = q.shape[0]
    out = torch.empty_like(q)
    with torch.cuda.device(q.device):
        st = lib.qlinear_decode_attention(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), mask.data_ptr(),
                                          out.data_ptr(), B, n_head, n_groups, d_head, k_cache.shape[1],
                                          _lib.dtype_code(q.dtype), _lib.stream_ptr(q.device))
    _lib.check(st, "qlinear_decode_attention")
    return out


def group_attention() -> bool:
    """False when QLINEAR_DISPATCH (include/qlinear_hip.h) turns the grouped MFMA decode attention off - asked of the library, which
    parses the variable once (``qlinear_dispatch_reload`` parses again): the split / workspace choice made here and the kernel the
    library launches cannot disagree after an environment change."""
    return not (_lib.get_lib().qlinear_dispatch_flags() & 16)


PREFETCH_NEXT = os.environ.get("QLINEAR_ATTENTION_PREFETCH", "1") != "0"   # spare workgroups warm the next linear's weights
SPLIT_ATTENTION_FROM = int(os.environ.get("QLINEAR_SPLIT_ATTENTION_FROM", "448"))   # cache capacity from which windows are split


def decode_attention_rope(qkv: Tensor, table: Tensor, pos: Tensor, write_index: Tensor, k_cache: Tensor, v_cache: Tensor,
                          mask: Tensor, n_head: int, n_groups: int, d_head: int, split: bool | None = None,
                          prefetch: tuple | None = None, plan_out: list | None = None) -> Tensor:
    """``decode_attention(rope_kv_write(qkv, ...), ...)`` for one position per sequence in a single launch:
    qkv (B, 1, (H+2G) D) -> (B, 1, H*D); the rotated key and the value are written into the caches at
    ``write_index[0]``.  ``prefetch = (weights, kind, N, K)``: the weights of the next one-row linear on the stream
    (kind ``_lib.NEXT_W4G32_PACKED`` / ``_lib.NEXT_W8_ROWS``) are pulled into the caches by spare workgroups of this
    launch (include/qlinear_hip.h).  ``plan_out``: a list receiving a pre-bound launch ``run(qkv)`` (``_lib.make_plan``) that
    is valid while table / pos / write_index / caches / mask / prefetched weights stay at their addresses - the caller's key.
    Cache rows behind ``write_index[0]`` hold nothing of the sequence (the reference appends the step's key / value at the end of its
    cache, chatglm_q/model.py:148-151): ``mask`` must hide them, and the 16-heads-per-group kernel skips them whatever it says."""
    lib = _lib.get_lib()
    B, S, W = qkv.shape
    if S != 1:
        raise ValueError("decode_attention_rope serves one position per sequence")
    _check_rope_table(table, k_cache, d_head)
    qkv = qkv.contiguous()
    out = torch.empty((B, 1, n_head * d_head), device=qkv.device, dtype=qkv.dtype)
    capacity = k_cache.shape[1]
    # the kernel reads mask row b at b * capacity: a mask sliced to the filled prefix and compacted would make rows b >= 1
    # read other sequences' columns
    if mask.dtype != torch.float32 or mask.numel() != B * capacity or mask.shape[-1] != capacity or not mask.is_contiguous():
        raise ValueError(f"decode_attention_rope: mask must be a contiguous fp32 (B, 1, capacity) = ({B}, 1, {capacity}) tensor, "
                         f"got {tuple(mask.shape)} {mask.dtype}")
    if split is None:
        # 16 heads per key/value group (16-bit, D = 128): the group kernel takes one 256-position window per block
        group_kernel = qkv.dtype != torch.float32 and d_head == 128 and n_head == 16 * n_groups and group_attention()
        split = capacity > 256 if group_kernel else capacity >= SPLIT_ATTENTION_FROM
    pos_c = pos.contiguous()
    with torch.cuda.device(qkv.device):
        ws_bytes = int(lib.qlinear_decode_attention_split_bytes(B, n_head, d_head, capacity)) if split else 0
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=qkv.device) if ws_bytes else None
        const = (table.data_ptr(), pos_c.data_ptr(), write_index.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), mask.data_ptr())
        shape = (B, n_head, n_groups, d_head, capacity, W, _lib.dtype_code(qkv.dtype))
        if prefetch is not None and PREFETCH_NEXT:
            weights, kind, n_next, k_next = prefetch
            name, tail = "qlinear_decode_attention_rope_prefetch", (weights.data_ptr(), kind, n_next, k_next)
        else:
            weights, name, tail = None, "qlinear_decode_attention_rope", ()
        st = getattr(lib, name)(qkv.data_ptr(), *const, out.data_ptr(), *shape, _lib.ptr(ws), ws_bytes, *tail, _lib.stream_ptr(qkv.device))
        _lib.check(st, name)
    if plan_out is not None and pos_c is pos:
        plan_out.append(_lib.make_plan(name, (None, *const, None, *shape, None, ws_bytes, *tail, None), 0, 7, 17 + len(tail), B, W,
                                       n_head * d_head, qkv.dtype, qkv.device, (), ws_slot=15 if ws_bytes else None, ws_bytes=ws_bytes,
                                       keep=(table, pos, write_index, k_cache, v_cache, mask, weights)))
    return out


def masked_softmax(scores: Tensor, mask: Tensor | None) -> Tensor:
    """``softmax(scores.float() + mask, -1).to(scores.dtype)`` in one launch.  scores (..., S, T) contiguous, mask
    (S, T) fp32 shared by all leading dims (or None)."""
    lib = _lib.get_lib()
    S, T = scores.shape[-2:]
    scores = scores.contiguous()
    out = torch.empty_like(scores)
    rows = scores.numel() // T
    if mask is not None:
        if mask.shape != (S, T) or mask.dtype != torch.float32:
            raise ValueError("mask must be an fp32 (S, T) tensor")
        if mask.stride(1) != 1:
            mask = mask.contiguous()
    with torch.cuda.device(scores.device):
        st = lib.qlinear_masked_softmax(scores.data_ptr(), _lib.ptr(mask), out.data_ptr(), rows, T, S, T,
                                        mask.stride(0) if mask is not None else T, T, _lib.dtype_code(scores.dtype),
                                        _lib.stream_ptr(scores.device))
    _lib.check(st, "qlinear_masked_softmax")
    return out


_PF_TILES = None


def prefill_attention_tiles():
    """(query positions per workgroup, keys per tile) of qlinear_prefill_attention: the granularity of its tile flags."""
    global _PF_TILES
    if _PF_TILES is None:
        import ctypes
        qb, kb = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(_lib.get_lib().qlinear_prefill_attention_tiles(ctypes.byref(qb), ctypes.byref(kb)), "qlinear_prefill_attention_tiles")
        _PF_TILES = (int(qb.value), int(kb.value))
    return _PF_TILES


def attention_tile_flags(mask: Tensor) -> Tensor:
    """Per (sequence, query block, key tile) of an additive fp32 mask (B, S, T): 0 = the tile can be skipped (every entry
    <= -1e9 and every row of the block has an entry >= -1e6: the probabilities are exactly 0 in fp32), 2 = every entry is 0
    (no mask loads), 1 = otherwise.  One pass over the mask per prefill chunk, shared by all layers."""
    QB, KB = prefill_attention_tiles()
    B, S, T = mask.shape
    nq, nk = (S + QB - 1) // QB, (T + KB - 1) // KB
    blocked, zero, row_ok = mask <= -1e9, mask == 0, (mask >= -1e6).any(dim=-1)
    if nq * QB != S or nk * KB != T:                       # rows / keys past the end never force a load or forbid a skip
        pad = (0, nk * KB - T, 0, nq * QB - S)
        blocked = torch.nn.functional.pad(blocked, pad, value=True)
        zero = torch.nn.functional.pad(zero, pad, value=True)
        row_ok = torch.nn.functional.pad(row_ok, (0, nq * QB - S), value=True)
    skip = blocked.view(B, nq, QB, nk, KB).all(dim=4).all(dim=2) & row_ok.view(B, nq, QB).all(dim=2)[:, :, None]
    clear = zero.view(B, nq, QB, nk, KB).all(dim=4).all(dim=2)
    # (torch.where, not masked assignment: no host synchronisation, capturable)
    return torch.where(skip, 0, torch.where(clear, 2, 1)).to(torch.uint8).contiguous()


def prefill_attention_supported(q_dtype, H: int, G: int, D: int) -> bool:
    return D == 128 and H == 16 * G and q_dtype in (torch.float16, torch.bfloat16)


def prefill_attention(q: Tensor, k_cache: Tensor, v_cache: Tensor, mask: Tensor | None, flags: Tensor | None, T: int,
                      H: int, G: int, D: int) -> Tensor:
    """softmax(round(q / sqrt(D)) k^T + mask) v for S new positions against cache rows [0, T) in one launch
    (chatglm_q/model.py:157-175).  q (B, S, H * D) rotated queries, caches (B, capacity, G, D), mask (B, S, T) additive fp32
    (or None), flags from attention_tile_flags(mask) (or None: every tile is processed with its mask).  Returns (B, S, H * D)."""
    lib = _lib.get_lib()
    B, S = q.shape[0], q.shape[1]
    if not (q.is_contiguous() and k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise ValueError("prefill_attention: q and the caches must be contiguous")
    if k_cache.shape != v_cache.shape or k_cache.shape[0] != B or tuple(k_cache.shape[2:]) != (G, D) or q.numel() != B * S * H * D:
        raise ValueError("prefill_attention: shape mismatch")
    if k_cache.dtype != q.dtype or v_cache.dtype != q.dtype:
        raise ValueError("prefill_attention: dtype mismatch")
    ldm = 0
    if mask is not None:
        if mask.dtype != torch.float32 or tuple(mask.shape) != (B, S, T):
            raise ValueError("mask must be an fp32 (B, S, T) tensor")
        mask = mask.contiguous()
        ldm = T
    if flags is not None:
        QB, KB = prefill_attention_tiles()
        if mask is None or flags.dtype != torch.uint8 or tuple(flags.shape) != (B, (S + QB - 1) // QB, (T + KB - 1) // KB):
            raise ValueError("tile flags do not match the mask's shape")
        flags = flags.contiguous()
    out = torch.empty((B, S, H * D), device=q.device, dtype=q.dtype)
    with torch.cuda.device(q.device):
        st = lib.qlinear_prefill_attention(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), _lib.ptr(mask), _lib.ptr(flags),
                                           out.data_ptr(), B, S, T, H, G, D, k_cache.shape[1], ldm, _lib.dtype_code(q.dtype),
                                           _lib.stream_ptr(q.device))
    _lib.check(st, "qlinear_prefill_attention")
    return out


def silu_mul(x: Tensor, hidden: int) -> Tensor:
    lib = _lib.get_lib()
    x2 = x.reshape(-1, x.shape[-1])
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    out = torch.empty((x2.shape[0], hidden), device=x.device, dtype=x.dtype)
    with torch.cuda.device(x.device):
        st = lib.qlinear_silu_mul(x2.data_ptr(), out.data_ptr(), x2.shape[0], hidden,
                                  x2.stride(0) if x2.shape[0] > 1 else 2 * hidden, hidden,
                                  _lib.dtype_code(x.dtype), _lib.stream_ptr(x.device))
    _lib.check(st, "qlinear_silu_mul")
    return out.reshape(*x.shape[:-1], hidden)


def greedy_advance(logits: Tensor, tok: Tensor, write_index: Tensor, pos: Tensor, mask: Tensor):
    """In place: tok = argmax(logits), pos += 1, write_index += 1, mask[..., new write_index] = 0 - one launch."""
    lib = _lib.get_lib()
    B, N = logits.shape
    with torch.cuda.device(logits.device):
        st = lib.qlinear_greedy_advance(logits.data_ptr(), B, N, logits.stride(0), tok.data_ptr(), write_index.data_ptr(),
                                        pos.data_ptr(), mask.data_ptr(), mask.shape[-1], _lib.dtype_code(logits.dtype),
                                        _lib.stream_ptr(logits.device))
    _lib.check(st, "qlinear_greedy_advance")


SAMPLER_MAX_TOP_K = 1024     # csrc/sampler.hip S_KMAX


def new_rng_state(batch: int, seed: int, device) -> Tensor:
    """Device state of qlinear_top_p_sample's generator: int64[1 + batch] = (seed, one draw counter per row)."""
    st = torch.zeros(1 + batch, dtype=torch.int64)
    st[0] = int(seed) & 0x7FFFFFFFFFFFFFFF
    return st.to(device)


def top_p_sample(logits: Tensor, tok: Tensor, rng_state: Tensor | None = None, top_k: int = 100, top_p: float = 0.8,
                 temperature: float = 1.0, dev_params: Tensor | None = None, write_index: Tensor | None = None,
                 pos: Tensor | None = None, mask: Tensor | None = None, return_distribution: bool = False):
    """chatglm_q/decoder.py:12-27 in one launch: ``tok[b] = top_p_sampling(logits[b], top_k, top_p, temperature)`` for every row of
    `logits` (B, N), drawing from the counter-based generator in `rng_state` (new_rng_state; None: seed 0, counter 0).  With
    write_index / pos / mask the launch also does a decode step's bookkeeping (greedy_advance).  dev_params: device float32[3] =
    (top_k, top_p, temperature) read by the kernel instead of the arguments (a captured graph then serves any setting).
    return_distribution: also return (probs (B, k), indices (B, k), u (B,)) - the filtered distribution in sorted order (ties: lowest
    index first), its token ids and the uniform number each row drew."""
    lib = _lib.get_lib()
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("top_p_sample: logits must be (B, N) with unit column stride")
    B, N = logits.shape
    if tok.dtype != torch.int64 or tok.numel() != B or not tok.is_contiguous():
        raise ValueError("top_p_sample: tok must be a contiguous int64 tensor of B elements")
    if dev_params is None and not (1 <= top_k and temperature > 0):
        raise ValueError("top_p_sample: top_k >= 1 and temperature > 0")
    if rng_state is not None and (rng_state.dtype != torch.int64 or rng_state.numel() < 1 + B or not rng_state.is_contiguous()):
        raise ValueError("top_p_sample: rng_state must be int64[1 + B] (new_rng_state)")
    if dev_params is not None and (dev_params.dtype != torch.float32 or dev_params.numel() < 3 or not dev_params.is_contiguous()):
        raise ValueError("top_p_sample: dev_params must be float32[3]")
    k_out = min(SAMPLER_MAX_TOP_K if dev_params is not None else top_k, N)
    probs = idx = u = None
    if return_distribution:
        probs = torch.zeros((B, k_out), device=logits.device, dtype=torch.float32)
        idx = torch.zeros((B, k_out), device=logits.device, dtype=torch.int64)
        u = torch.zeros(B, device=logits.device, dtype=torch.float32)
    with torch.cuda.device(logits.device):
        st = lib.qlinear_top_p_sample(logits.data_ptr(), B, N, logits.stride(0), int(top_k), float(top_p), float(temperature),
                                      _lib.ptr(dev_params), _lib.ptr(rng_state), tok.data_ptr(), _lib.ptr(write_index), _lib.ptr(pos),
                                      _lib.ptr(mask), mask.shape[-1] if mask is not None else 0, _lib.ptr(probs), _lib.ptr(idx),
                                      _lib.ptr(u), k_out, _lib.dtype_code(logits.dtype), _lib.stream_ptr(logits.device))
    _lib.check(st, "qlinear_top_p_sample")
    if return_distribution:
        return probs, idx, u


def token_logprob(logits: Tensor, targets: Tensor, ignore_index: int = -100, return_lse: bool = False, return_argmax: bool = False):
    """Per-token log-probabilities of given ids - the per-row tail of the reference's loss (chatglm_q/model.py:384-390:
    ``logits.float()``, then ``F.cross_entropy``) in one launch and one pass over the rows (``qlinear_token_logprob``):
    ``logprob[r] = log_softmax(logits[r].float())[targets[r]]`` as fp32, 0 where ``targets[r] == ignore_index``, NaN where it is
    any other value outside [0, N).  logits (R, N) fp16 / bf16 / fp32 with unit column stride (rows may be strided), targets (R,)
    int64 on the same device.  Returns ``logprob`` (R,), or the tuple ``(logprob[, lse][, argmax])`` with ``return_lse`` (the
    log-sum-exp of every row, fp32) / ``return_argmax`` (lowest index of every row's maximum, int64).  CPU tensors take the dense
    formula, as the modules do."""
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError(f"token_logprob: logits must be (R, N) with N >= 1, got {tuple(logits.shape)}")
    R, N = logits.shape
    if targets.dtype != torch.int64 or tuple(targets.shape) != (R,):
        raise ValueError(f"token_logprob: targets must be an int64 tensor of shape ({R},), got {tuple(targets.shape)} {targets.dtype}")
    if targets.device != logits.device:
        raise ValueError(f"token_logprob: logits on {logits.device}, targets on {targets.device}")
    if not logits.is_cuda:
        x = logits.float()
        lse = torch.logsumexp(x, dim=-1)
        inside = (targets >= 0) & (targets < N)
        picked = torch.log_softmax(x, dim=-1).gather(1, targets.clamp(0, N - 1)[:, None])[:, 0]
        lp = torch.where(targets == ignore_index, torch.zeros_like(picked),
                         torch.where(inside, picked, torch.full_like(picked, float("nan"))))
        amax = x.argmax(dim=-1) if return_argmax else None
    else:
        lib = _lib.get_lib()
        code = _lib.dtype_code(logits.dtype)
        if logits.stride(1) != 1 or (R > 1 and logits.stride(0) < N):
            logits = logits.contiguous()
        targets = targets.contiguous()
        lp = torch.empty(R, device=logits.device, dtype=torch.float32)
        lse = torch.empty(R, device=logits.device, dtype=torch.float32) if return_lse else None
        amax = torch.empty(R, device=logits.device, dtype=torch.int64) if return_argmax else None
        if R:
            with torch.cuda.device(logits.device):
                st = lib.qlinear_token_logprob(logits.data_ptr(), R, N, logits.stride(0) if R > 1 else N, targets.data_ptr(),
                                               int(ignore_index), lp.data_ptr(), _lib.ptr(lse), _lib.ptr(amax), code,
                                               _lib.stream_ptr(logits.device))
            _lib.check(st, "qlinear_token_logprob")
    if not (return_lse or return_argmax):
        return lp
    return (lp,) + ((lse,) if return_lse else ()) + ((amax,) if return_argmax else ())


_SEED_MASK = 0x7FFFFFFFFFFFFFFF


def batch_rng_state(seeds, device) -> Tensor:
    """Device generator state of qlinear_batch_sample_advance: int64 (B, 2) = (seed of row b, draw counter 0) - row b's key is
    ``seeds[b]`` (taken modulo 2^63), whichever batch position it holds."""
    st = torch.zeros((len(seeds), 2), dtype=torch.int64)
    for b, s in enumerate(seeds):
        st[b, 0] = int(s) & _SEED_MASK
    return st.to(device)


class BatchRows:
    """Per-row generation state of ``batch_sample_advance`` (static device buffers a captured step reads and updates):
    ``row_params`` (B, 3) float32 = top_k, top_p, temperature; ``row_rng`` (B, 2) int64 = seed, draw counter; ``row_state`` (B, 2)
    int32 = tokens generated, flags (bit 0 finished, bit 1 invalid logits); ``budget`` (B,) int32; ``out_tokens`` (B, out_ld) int64;
    ``live`` (1,) int32 = rows not finished; ``stop_id`` (a host int: -1 = none)."""
    FINISHED, INVALID = 1, 2

    def __init__(self, batch: int, out_ld: int, device):
        if batch < 1 or out_ld < 1:
            raise ValueError(f"BatchRows: batch >= 1 and out_ld >= 1 (got {batch}, {out_ld})")
        self.batch, self.out_ld, self.device = batch, out_ld, torch.device(device)
        self.row_params = torch.zeros((batch, 3), dtype=torch.float32, device=device)
        self.row_rng = torch.zeros((batch, 2), dtype=torch.int64, device=device)
        self.row_state = torch.zeros((batch, 2), dtype=torch.int32, device=device)
        self.budget = torch.zeros(batch, dtype=torch.int32, device=device)
        self.out_tokens = torch.zeros((batch, out_ld), dtype=torch.int64, device=device)
        self.live = torch.zeros(1, dtype=torch.int32, device=device)
        self.stop_id = -1

    def arm(self, params, seeds, budgets, stop_id: int | None = None):
        """Set the state for a new generation, in place (the buffers keep their addresses).  ``params``: one (top_k, top_p,
        temperature) per row; ``seeds`` / ``budgets``: one int per row; ``stop_id`` None / < 0: no stop token.  A row with
        budget 0 starts finished."""
        B = self.batch
        if len(params) != B or len(seeds) != B or len(budgets) != B:
            raise ValueError(f"BatchRows.arm: params, seeds and budgets need {B} entries each")
        for k, p, t in params:
            if not (int(k) >= 1 and float(t) > 0):
                raise ValueError(f"BatchRows.arm: top_k >= 1 and temperature > 0 per row (got top_k {k}, temperature {t})")
        if any(int(n) < 0 or int(n) >= 2 ** 31 for n in budgets):
            raise ValueError("BatchRows.arm: budgets must be in [0, 2^31)")
        self.row_params.copy_(torch.tensor([[float(k), float(p), float(t)] for k, p, t in params], dtype=torch.float32))
        self.row_rng.copy_(batch_rng_state(seeds, "cpu"))
        st = torch.zeros((B, 2), dtype=torch.int32)
        st[:, 1] = torch.tensor([self.FINISHED if int(n) == 0 else 0 for n in budgets], dtype=torch.int32)
        self.row_state.copy_(st)
        self.budget.copy_(torch.tensor([int(n) for n in budgets], dtype=torch.int32))
        self.live.fill_(sum(1 for n in budgets if int(n) > 0))
        self.stop_id = -1 if stop_id is None or stop_id < 0 else int(stop_id)
        return self

    def tensors(self):
        return (self.row_params, self.row_rng, self.row_state, self.budget, self.out_tokens, self.live)


def _batch_sample_advance_host(logits: Tensor, tok: Tensor, rows: BatchRows, write_index, pos, mask):
    """CPU form of qlinear_batch_sample_advance: the same per-row rules, selection by torch ops - argmax for top_k == 1, the
    reference's filtered distribution and one multinomial draw from a generator seeded by (seed, counter) of the row otherwise."""
    from .decoder import filtered_distribution
    B, N = logits.shape
    out_ld = rows.out_ld
    for b in range(B):
        n, flags = int(rows.row_state[b, 0]), int(rows.row_state[b, 1])
        if flags & BatchRows.FINISHED:
            tok[b] = rows.stop_id if rows.stop_id >= 0 else (int(rows.out_tokens[b, n - 1]) if 0 < n <= out_ld else 0)
            continue
        if n >= int(rows.budget[b]) or n >= out_ld:
            rows.row_state[b, 1] = flags | BatchRows.FINISHED
            rows.live.sub_(1)
            tok[b] = rows.stop_id if rows.stop_id >= 0 else (int(rows.out_tokens[b, n - 1]) if 0 < n <= out_ld else 0)
            continue
        kf, top_p, temperature = (float(v) for v in rows.row_params[b])
        k = 1 if not kf >= 1 else min(int(kf), SAMPLER_MAX_TOP_K, N)
        seed, ctr = int(rows.row_rng[b, 0]), int(rows.row_rng[b, 1])
        x = logits[b].float()
        invalid = not temperature > 0
        t = -1
        if not invalid and k > 1:
            probs, idx = filtered_distribution(x, k, top_p, temperature)
            if bool(torch.isfinite(probs).all()) and float(probs.sum()) > 0:
                g = torch.Generator().manual_seed((seed * 1000003 + ctr) & _SEED_MASK)
                t = int(idx[torch.multinomial(probs, 1, generator=g)[0]])
            else:
                invalid = True
        if invalid or k == 1:
            nan = bool(torch.isnan(x).any())
            xs = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)
            t = int(xs.argmax())                                 # lowest index of the largest non-NaN value (all NaN: 0)
            best = float(xs[t])
            if not invalid:
                invalid = nan or not (float("-inf") < best < float("inf"))
        rows.out_tokens[b, n] = t
        n += 1
        fin = invalid or (rows.stop_id >= 0 and t == rows.stop_id) or n >= int(rows.budget[b]) or n >= out_ld
        rows.row_state[b, 0] = n
        rows.row_state[b, 1] = flags | (BatchRows.FINISHED if fin else 0) | (BatchRows.INVALID if invalid else 0)
        rows.row_rng[b, 1] = ctr + 1
        if fin:
            rows.live.sub_(1)
        tok[b] = t
    if write_index is not None:
        write_index.add_(1)
        pos.add_(1)
        mask.index_fill_(-1, torch.clamp(write_index.view(-1), max=mask.shape[-1] - 1), 0.0)


def batch_sample_advance(logits: Tensor, tok: Tensor, rows: BatchRows, write_index: Tensor | None = None, pos: Tensor | None = None,
                         mask: Tensor | None = None, return_distribution: bool = False):
    """One batched generation step's selection and bookkeeping in one launch (``qlinear_batch_sample_advance``): row b of `logits`
    (B, N) is selected with its own sampler settings and generator (``rows``: BatchRows), recorded in ``rows.out_tokens`` and
    stopped on ``rows.stop_id`` or its budget; ``tok`` (B,) int64 gets the next input ids (a finished row: the fill id).  With
    write_index / pos / mask (all or none) the decode step's bookkeeping is done as ``greedy_advance`` does it.
    return_distribution: also return (probs (B, k), indices (B, k), u (B,)) with k = min(1024, N), as ``top_p_sample`` does
    (entries past a row's own top_k are 0).  CPU tensors take the host form (torch ops, the same per-row rules)."""
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError(f"batch_sample_advance: logits must be (B, N) with N >= 1, got {tuple(logits.shape)}")
    B, N = logits.shape
    if B != rows.batch:
        raise ValueError(f"batch_sample_advance: {B} logits rows for a BatchRows of {rows.batch}")
    if tok.dtype != torch.int64 or tok.numel() != B or not tok.is_contiguous():
        raise ValueError("batch_sample_advance: tok must be a contiguous int64 tensor of B elements")
    book = (write_index is not None, pos is not None, mask is not None)
    if any(book) and not all(book):
        raise ValueError("batch_sample_advance: write_index, pos and mask go together")
    if rows.stop_id >= N:
        raise ValueError(f"batch_sample_advance: stop id {rows.stop_id} outside the vocabulary of {N}")
    for t in (tok,) + rows.tensors():
        if t.device != logits.device:
            raise ValueError(f"batch_sample_advance: logits on {logits.device}, state on {t.device}")
    if not logits.is_cuda:
        if return_distribution:
            raise ValueError("batch_sample_advance: return_distribution needs the GPU kernel")
        _batch_sample_advance_host(logits, tok.view(-1), rows, write_index, pos, mask)
        return None
    lib = _lib.get_lib()
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    k_out = min(SAMPLER_MAX_TOP_K, N)
    probs = idx = u = None
    if return_distribution:
        probs = torch.zeros((B, k_out), device=logits.device, dtype=torch.float32)
        idx = torch.zeros((B, k_out), device=logits.device, dtype=torch.int64)
        u = torch.zeros(B, device=logits.device, dtype=torch.float32)
    with torch.cuda.device(logits.device):
        st = lib.qlinear_batch_sample_advance(logits.data_ptr(), B, N, logits.stride(0) if B > 1 else N, rows.row_params.data_ptr(),
                                              rows.row_rng.data_ptr(), rows.row_state.data_ptr(), rows.budget.data_ptr(),
                                              rows.out_tokens.data_ptr(), rows.out_ld, rows.live.data_ptr(), rows.stop_id,
                                              tok.data_ptr(), _lib.ptr(write_index), _lib.ptr(pos), _lib.ptr(mask),
                                              mask.shape[-1] if mask is not None else 0, _lib.ptr(probs), _lib.ptr(idx), _lib.ptr(u),
                                              k_out, _lib.dtype_code(logits.dtype), _lib.stream_ptr(logits.device))
    _lib.check(st, "qlinear_batch_sample_advance")
    if return_distribution:
        return probs, idx, u
    return None


# ---- sampling controls: repetition / presence / frequency penalties and a logit bias (csrc/logit_penalties.hip) -----------------------
LOGIT_BIAS_MAX = 64          # entries of one row's logit-bias list (QL_LOGIT_BIAS_MAX, include/qlinear_hip.h); more raise a ValueError
_PROMPT_BIT = -(2 ** 31)     # bit 31 of a state word as an int32


def _finite(v) -> bool:
    return v == v and v not in (float("inf"), float("-inf"))


def _check_step_logits(name: str, logits: Tensor, batch: int, tok, row_state, state_tensor: Tensor, kind: str | None = None):
    """The argument checks the step's logit stages share (``name``: the caller, the prefix of every message): `logits` (B, N) with unit
    column stride and rows that do not overlap, ``tok`` / ``row_state`` of B rows, everything on the logits' device.  ``kind`` (the state's
    class name): B must be ``batch``; None: the caller compares the shape itself.  Returns (B, N)."""
    if logits.dim() != 2 or logits.shape[1] < 1 or logits.stride(1) != 1:
        raise ValueError(f"{name}: logits must be (B, N) with N >= 1 and unit column stride, got {tuple(logits.shape)}")
    B, N = logits.shape
    if kind is not None and B != batch:
        raise ValueError(f"{name}: {B} logits rows for a {kind} of {batch}")
    if B > 1 and logits.stride(0) < N:
        raise ValueError(f"{name}: overlapping logits rows")
    if tok is not None and (tok.dtype != torch.int64 or tok.numel() != B or not tok.is_contiguous()):
        raise ValueError(f"{name}: tok must be a contiguous int64 tensor of B elements")
    if row_state is not None and (row_state.dtype != torch.int32 or tuple(row_state.shape) != (B, 2) or not row_state.is_contiguous()):
        raise ValueError(f"{name}: row_state must be a contiguous int32 (B, 2) tensor (BatchRows.row_state)")
    for t in (state_tensor, tok, row_state):
        if t is not None and t.device != logits.device:
            raise ValueError(f"{name}: logits on {logits.device}, state on {t.device}")
    return B, N


class PenaltyState:
    """Static buffers of ``logit_penalties`` for a batch of rows (a captured step reads and updates them in place): ``counts``
    (batch, ld) int32 - bit 31: the entry is one of the row's prompt ids, bits 0..30: how often the row has generated it;
    ``settings`` (batch, 3) float32 = repetition, presence, frequency penalty; ``bias_ids`` / ``bias_vals`` (batch, LOGIT_BIAS_MAX)
    int32 / float32 and ``bias_len`` (batch,) int32: every row's sparse logit bias.  ``active``: whether the last ``arm`` set anything
    that changes a logit (all defaults: nothing has to be launched)."""

    def __init__(self, batch: int, vocab: int, device):
        if batch < 1 or vocab < 1:
            raise ValueError(f"PenaltyState: batch >= 1 and vocab >= 1 (got {batch}, {vocab})")
        self.batch, self.vocab, self.device = batch, vocab, torch.device(device)
        self.ld = -(-vocab // 4) * 4                            # rows of the state stay 16-byte aligned
        self.counts = torch.zeros((batch, self.ld), dtype=torch.int32, device=device)
        self.settings = torch.tensor([[1.0, 0.0, 0.0]] * batch, dtype=torch.float32, device=device)
        self.bias_ids = torch.zeros((batch, LOGIT_BIAS_MAX), dtype=torch.int32, device=device)
        self.bias_vals = torch.zeros((batch, LOGIT_BIAS_MAX), dtype=torch.float32, device=device)
        self.bias_len = torch.zeros(batch, dtype=torch.int32, device=device)
        self.active = False

    @staticmethod
    def check(batch: int, vocab: int, settings, biases):
        """Validate one (repetition, presence, frequency) triple and one bias dict (or None) per row; returns them normalised:
        a list of float triples and a list of [(id, value), ...] lists.  A ValueError names the offending row."""
        if len(settings) != batch or len(biases) != batch:
            raise ValueError(f"penalties: {len(settings)} settings and {len(biases)} bias lists for {batch} rows")
        out_s, out_b = [], []
        for b, (s, bias) in enumerate(zip(settings, biases)):
            r, p, f = (float(v) for v in s)
            if not (_finite(r) and r > 0):
                raise ValueError(f"penalties: row {b}: repetition_penalty must be finite and > 0 (got {r})")
            if not _finite(p):
                raise ValueError(f"penalties: row {b}: presence_penalty must be finite (got {p})")
            if not _finite(f):
                raise ValueError(f"penalties: row {b}: frequency_penalty must be finite (got {f})")
            pairs = []
            if bias:
                items = list(bias.items()) if hasattr(bias, "items") else [tuple(e) for e in bias]
                if len(items) > LOGIT_BIAS_MAX:
                    raise ValueError(f"penalties: row {b}: {len(items)} logit_bias entries, at most {LOGIT_BIAS_MAX} (LOGIT_BIAS_MAX)")
                seen = set()
                for i, v in items:
                    if int(i) != i or not 0 <= int(i) < vocab:
                        raise ValueError(f"penalties: row {b}: logit_bias id {i} outside the vocabulary [0, {vocab})")
                    if int(i) in seen:
                        raise ValueError(f"penalties: row {b}: logit_bias id {int(i)} given twice")
                    seen.add(int(i))
                    v = float(v)
                    if v != v or v == float("inf"):
                        raise ValueError(f"penalties: row {b}: logit_bias value for id {int(i)} must be finite or -inf (got {v})")
                    pairs.append((int(i), v))
            out_s.append((r, p, f))
            out_b.append(pairs)
        return out_s, out_b

    @staticmethod
    def neutral(settings, biases) -> bool:
        """True when the (validated) settings change no logit: every row at (1, 0, 0) with an empty bias list."""
        return all(s == (1.0, 0.0, 0.0) for s in settings) and not any(biases)

    def arm(self, prompts_or_mask, settings, biases=None):
        """Start a generation, in place (the buffers keep their addresses): the counts go to 0, the prompt flags are set from
        ``prompts_or_mask`` - one sequence of REAL prompt ids per row (no pads), or a bool (batch, vocab) membership tensor - and
        the settings (one (repetition, presence, frequency) per row) and bias dicts ``{id: value}`` (one per row or None) are
        validated and stored."""
        B, N = self.batch, self.vocab
        settings, biases = self.check(B, N, settings, [None] * B if biases is None else biases)
        self.counts.zero_()
        if isinstance(prompts_or_mask, Tensor):
            if prompts_or_mask.dtype != torch.bool or tuple(prompts_or_mask.shape) != (B, N):
                raise ValueError(f"PenaltyState.arm: a prompt mask must be a bool ({B}, {N}) tensor")
            self.counts[:, :N].masked_fill_(prompts_or_mask.to(self.device), _PROMPT_BIT)
        else:
            if len(prompts_or_mask) != B:
                raise ValueError(f"PenaltyState.arm: {len(prompts_or_mask)} prompts for {B} rows")
            flat = []
            for b, ids in enumerate(prompts_or_mask):
                for i in ids:
                    if not 0 <= int(i) < N:
                        raise ValueError(f"PenaltyState.arm: row {b}: prompt id {int(i)} outside the vocabulary [0, {N})")
                    flat.append(b * self.ld + int(i))
            if flat:
                self.counts.view(-1).index_fill_(0, torch.tensor(flat, dtype=torch.long).to(self.device), _PROMPT_BIT)
        ids = torch.zeros((B, LOGIT_BIAS_MAX), dtype=torch.int32)
        vals = torch.zeros((B, LOGIT_BIAS_MAX), dtype=torch.float32)
        for b, pairs in enumerate(biases):
            for j, (i, v) in enumerate(pairs):
                ids[b, j], vals[b, j] = i, v
        self.settings.copy_(torch.tensor(settings, dtype=torch.float32))
        self.bias_ids.copy_(ids)
        self.bias_vals.copy_(vals)
        self.bias_len.copy_(torch.tensor([len(p) for p in biases], dtype=torch.int32))
        self.active = not self.neutral(settings, biases)
        return self

    def generated(self) -> Tensor:
        """(batch, vocab) int32: how often every row has generated every id so far."""
        return self.counts[:, :self.vocab] & 0x7FFFFFFF

    def tensors(self):
        """What a step changes (a capture saves and restores it)."""
        return (self.counts,)


def _logit_penalties_host(logits: Tensor, state: PenaltyState, tok, row_state):
    """CPU form of qlinear_logit_penalties: the same rules with torch ops, every op one fp32 rounding (torch does not fuse them)."""
    B, N = logits.shape
    live = torch.ones(B, dtype=torch.bool) if row_state is None else (row_state[:, 1] & BatchRows.FINISHED) == 0
    words = state.counts[:, :N]
    if tok is not None:
        for b in range(B):
            t = int(tok[b])
            if bool(live[b]) and 0 <= t < N:
                words[b, t] += 1
    g = words & 0x7FFFFFFF
    seen, counted = words != 0, g > 0
    r, p, f = (state.settings[:, k:k + 1] for k in range(3))
    x = logits.float()
    x = torch.where(seen, torch.where(x > 0, x / r, x * r), x)
    m = f * g.float()
    x = torch.where(counted, (x - m) - p, x)
    biased = torch.zeros((B, N), dtype=torch.bool)
    bias = torch.zeros((B, N), dtype=torch.float32)
    for b in range(B):
        n = int(state.bias_len[b])
        if n:
            ids = state.bias_ids[b, :n].long()
            biased[b, ids] = True
            bias[b, ids] = state.bias_vals[b, :n]
    x = torch.where(biased, x + bias, x)
    touched = (seen | biased) & live[:, None]
    logits.copy_(torch.where(touched, x.to(logits.dtype), logits))


def logit_penalties(logits: Tensor, state: PenaltyState, tok: Tensor | None = None, row_state: Tensor | None = None) -> Tensor:
    """Apply ``state``'s repetition / presence / frequency penalties and logit bias to `logits` (B, N) IN PLACE and advance the
    token history, in one launch (``qlinear_logit_penalties``, whose comment in include/qlinear_hip.h holds the rules).  ``tok`` (B,)
    int64: the ids fed into this step - counted before the rules are applied; None (the first token after a prefill): nothing is
    counted.  ``row_state``: a ``BatchRows.row_state``; rows whose FINISHED bit is set are left untouched.  Returns `logits`.  CPU
    tensors take the host form (torch ops, the same rules bit for bit)."""
    B, N = _check_step_logits("logit_penalties", logits, state.batch, tok, row_state, state.counts)
    if B != state.batch or N != state.vocab:
        raise ValueError(f"logit_penalties: logits {tuple(logits.shape)} for a PenaltyState of ({state.batch}, {state.vocab})")
    if not logits.is_cuda:
        _logit_penalties_host(logits, state, None if tok is None else tok.view(-1), row_state)
        return logits
    lib = _lib.get_lib()
    with torch.cuda.device(logits.device):
        st = lib.qlinear_logit_penalties(logits.data_ptr(), B, N, logits.stride(0) if B > 1 else N, state.settings.data_ptr(),
                                         state.bias_ids.data_ptr(), state.bias_vals.data_ptr(), state.bias_len.data_ptr(),
                                         LOGIT_BIAS_MAX, state.counts.data_ptr(), state.ld, _lib.ptr(tok), _lib.ptr(row_state),
                                         _lib.dtype_code(logits.dtype), _lib.stream_ptr(logits.device))
    _lib.check(st, "qlinear_logit_penalties")
    return logits


# ---- history constraints: no-repeat n-grams, banned / stop sequences, minimum length (csrc/history_constraints.hip) ------------------
CONSTRAINT_SEQS_MAX = 32     # sequences of one row, all kinds together (QL_CONSTRAINT_SEQS_MAX, include/qlinear_hip.h); more raise a ValueError
CONSTRAINT_SEQ_LEN_MAX = 16  # ids of one sequence, and the largest no-repeat n-gram size (QL_CONSTRAINT_SEQ_LEN_MAX)


def _is_seq(v) -> bool:
    return isinstance(v, (list, tuple))


def per_row(name: str, v, batch: int, who: str = "constraints", what: str = "rows"):
    """A scalar setting for every row, or one per row: a list of ``batch`` values (``who`` / ``what``: the caller's words in the error)."""
    if _is_seq(v):
        if len(v) != batch:
            raise ValueError(f"{who}: {name} has {len(v)} entries for {batch} {what}")
        return list(v)
    return [v] * batch


def _is_int(v) -> bool:
    """An integer value of any numeric type (3, 3.0, a numpy integer); None, strings and bools are not."""
    if isinstance(v, bool) or isinstance(v, str) or v is None:
        return False
    try:
        return int(v) == v
    except (TypeError, ValueError, OverflowError):
        return False


class ConstraintState:
    """Static buffers of ``history_constraints`` for a batch of rows (a captured step reads and updates them in place): ``hist``
    (batch, hist_ld) int32 - every row's real prompt ids, then its generated ids, in order; ``hist_len`` / ``prompt_len`` (batch,)
    int32; ``cfg`` (batch, 2) int32 = no-repeat n-gram size (0 = off), min_new; and every row's sequence table ``seq_tok`` (batch,
    CONSTRAINT_SEQS_MAX, CONSTRAINT_SEQ_LEN_MAX) int32, ``seq_len`` / ``seq_kind`` (batch, CONSTRAINT_SEQS_MAX) int32, ``seq_count``
    (batch,) int32 - kinds BAN (the last id is banned behind the others), STOP (the row finishes once it has generated the sequence)
    and MIN (one id, banned until min_new tokens are generated).  ``active``: whether the last ``arm`` set anything."""
    BAN, STOP, MIN = 0, 1, 2

    def __init__(self, batch: int, hist_ld: int, device):
        if batch < 1 or hist_ld < 1:
            raise ValueError(f"ConstraintState: batch >= 1 and hist_ld >= 1 (got {batch}, {hist_ld})")
        self.batch, self.hist_ld, self.device = batch, hist_ld, torch.device(device)
        i32 = dict(dtype=torch.int32, device=device)
        self.hist = torch.zeros((batch, hist_ld), **i32)
        self.hist_len = torch.zeros(batch, **i32)
        self.prompt_len = torch.zeros(batch, **i32)
        self.cfg = torch.zeros((batch, 2), **i32)
        self.seq_tok = torch.zeros((batch, CONSTRAINT_SEQS_MAX, CONSTRAINT_SEQ_LEN_MAX), **i32)
        self.seq_len = torch.zeros((batch, CONSTRAINT_SEQS_MAX), **i32)
        self.seq_kind = torch.zeros((batch, CONSTRAINT_SEQS_MAX), **i32)
        self.seq_count = torch.zeros(batch, **i32)
        self.active = False

    @staticmethod
    def per_row(name: str, v, batch: int):
        """A scalar setting for every row, or one per row."""
        return per_row(name, v, batch)

    @staticmethod
    def per_row_sequences(name: str, v, batch: int):
        """A sequence argument for every row: None, a list of id lists (every row gets it) or a list of ``batch`` such lists (or
        None) - the nesting depth decides.  Returns one list of id lists per row."""
        if v is None:
            return [[] for _ in range(batch)]
        if not _is_seq(v):
            raise ValueError(f"constraints: {name} must be a list of token-id lists (got {type(v).__name__})")
        nested = any(e is None or (_is_seq(e) and len(e) > 0 and _is_seq(e[0])) for e in v)
        if not nested:
            if any(not _is_seq(e) for e in v):
                raise ValueError(f"constraints: {name} must be a list of token-id lists")
            return [[list(e) for e in v] for _ in range(batch)]
        if len(v) != batch:
            raise ValueError(f"constraints: {name} has {len(v)} entries for {batch} rows")
        out = []
        for b, e in enumerate(v):
            if e is not None and (not _is_seq(e) or any(not _is_seq(q) for q in e)):
                raise ValueError(f"constraints: row {b}: {name} must be a list of token-id lists or None")
            out.append([] if e is None else [list(q) for q in e])
        return out

    @staticmethod
    def check(batch: int, no_repeat_ngram_size=0, bad_words_ids=None, stop_sequences=None, min_new_tokens=0, eos_id=None,
              vocab: int | None = None):
        """Validate the four controls - each one value for every row or one per row (the sequence arguments: see
        ``per_row_sequences``) - and return them normalised: per row ``(n, min_new, [(kind, ids), ...])``, the table in the order
        BAN, STOP, MIN.  ``min_new_tokens`` with no ``eos_id`` arms nothing.  A ValueError names the offending row."""
        ns = ConstraintState.per_row("no_repeat_ngram_size", no_repeat_ngram_size, batch)
        mins = ConstraintState.per_row("min_new_tokens", min_new_tokens, batch)
        eos = ConstraintState.per_row("eos_id", eos_id, batch)
        bans = ConstraintState.per_row_sequences("bad_words_ids", bad_words_ids, batch)
        stops = ConstraintState.per_row_sequences("stop_sequences", stop_sequences, batch)
        out = []
        for b in range(batch):
            n, mn = ns[b], mins[b]
            if not _is_int(n) or n < 0:
                raise ValueError(f"constraints: row {b}: no_repeat_ngram_size must be an integer >= 0 (got {n})")
            if n > CONSTRAINT_SEQ_LEN_MAX:
                raise ValueError(f"constraints: row {b}: no_repeat_ngram_size {n}, at most {CONSTRAINT_SEQ_LEN_MAX} (CONSTRAINT_SEQ_LEN_MAX)")
            if not _is_int(mn) or mn < 0 or mn >= 2 ** 31:
                raise ValueError(f"constraints: row {b}: min_new_tokens must be an integer in [0, 2^31) (got {mn})")
            table = []
            for kind, name, seqs in ((ConstraintState.BAN, "bad_words_ids", bans[b]), (ConstraintState.STOP, "stop_sequences", stops[b])):
                for q in seqs:
                    if len(q) == 0:
                        raise ValueError(f"constraints: row {b}: an empty sequence in {name}")
                    if len(q) > CONSTRAINT_SEQ_LEN_MAX:
                        raise ValueError(f"constraints: row {b}: a sequence of {len(q)} ids in {name}, at most {CONSTRAINT_SEQ_LEN_MAX} "
                                         "(CONSTRAINT_SEQ_LEN_MAX)")
                    for i in q:
                        if not _is_int(i) or not 0 <= int(i) < (2 ** 31 if vocab is None else vocab):
                            raise ValueError(f"constraints: row {b}: id {i!r} in {name} outside the vocabulary")
                    table.append((kind, [int(i) for i in q]))
            if int(mn) > 0 and eos[b] is not None:
                e = eos[b]
                if not _is_int(e) or not 0 <= int(e) < (2 ** 31 if vocab is None else vocab):
                    raise ValueError(f"constraints: row {b}: eos_id {e} outside the vocabulary")
                table.append((ConstraintState.MIN, [int(e)]))
            if len(table) > CONSTRAINT_SEQS_MAX:
                raise ValueError(f"constraints: row {b}: {len(table)} sequences (banned, stop and the end id of min_new_tokens together), "
                                 f"at most {CONSTRAINT_SEQS_MAX} (CONSTRAINT_SEQS_MAX)")
            out.append((int(n), int(mn), table))
        return out

    @staticmethod
    def neutral(settings) -> bool:
        """True when the (validated) settings arm nothing: every row with n = 0 and an empty table."""
        return all(n == 0 and not table for n, _, table in settings)

    def arm(self, prompts, settings):
        """Start a generation, in place (the buffers keep their addresses): row b's history becomes ``prompts[b]`` - its REAL prompt
        ids, no pads - and its controls ``settings[b]`` = ``(n, min_new, [(kind, ids), ...])`` as ``check`` returns them."""
        B = self.batch
        if len(prompts) != B or len(settings) != B:
            raise ValueError(f"ConstraintState.arm: {len(prompts)} prompts and {len(settings)} settings for {B} rows")
        hist = torch.zeros((B, self.hist_ld), dtype=torch.int32)
        seq_tok = torch.zeros((B, CONSTRAINT_SEQS_MAX, CONSTRAINT_SEQ_LEN_MAX), dtype=torch.int32)
        seq_len = torch.zeros((B, CONSTRAINT_SEQS_MAX), dtype=torch.int32)
        seq_kind = torch.zeros((B, CONSTRAINT_SEQS_MAX), dtype=torch.int32)
        cfg = torch.zeros((B, 2), dtype=torch.int32)
        for b, (ids, (n, mn, table)) in enumerate(zip(prompts, settings)):
            ids = [int(i) for i in ids]
            if len(ids) > self.hist_ld:
                raise ValueError(f"ConstraintState.arm: row {b}: a prompt of {len(ids)} ids for a history of {self.hist_ld}")
            if not 0 <= n <= CONSTRAINT_SEQ_LEN_MAX or mn < 0 or len(table) > CONSTRAINT_SEQS_MAX:
                raise ValueError(f"ConstraintState.arm: row {b}: settings outside the caps (ConstraintState.check validates them)")
            if ids:
                hist[b, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
            cfg[b, 0], cfg[b, 1] = n, mn
            for s, (kind, q) in enumerate(table):
                if not 1 <= len(q) <= CONSTRAINT_SEQ_LEN_MAX or kind not in (self.BAN, self.STOP, self.MIN):
                    raise ValueError(f"ConstraintState.arm: row {b}: sequence {s} outside the caps (ConstraintState.check validates them)")
                seq_tok[b, s, :len(q)] = torch.tensor(q, dtype=torch.int32)
                seq_len[b, s], seq_kind[b, s] = len(q), kind
        self.hist.copy_(hist)
        self.hist_len.copy_(torch.tensor([len(p) for p in prompts], dtype=torch.int32))
        self.prompt_len.copy_(self.hist_len)
        self.cfg.copy_(cfg)
        self.seq_tok.copy_(seq_tok)
        self.seq_len.copy_(seq_len)
        self.seq_kind.copy_(seq_kind)
        self.seq_count.copy_(torch.tensor([len(t) for _, _, t in settings], dtype=torch.int32))
        self.active = not self.neutral(settings)
        return self

    def tensors(self):
        """What a step changes and a capture saves and restores (what a warm-up wrote past ``hist_len`` is overwritten by the
        steps that follow)."""
        return (self.hist_len,)


def _clamp(v: int, lo: int, hi: int) -> int:
    return lo if v < lo else (hi if v > hi else v)


def _history_constraints_host(logits: Tensor, state: ConstraintState, tok, row_state, live):
    """CPU form of qlinear_history_constraints: rules 0 - 3 of its comment in include/qlinear_hip.h, row by row in Python."""
    B, N = logits.shape
    for b in range(B):
        if row_state is not None and int(row_state[b, 1]) & BatchRows.FINISHED:
            continue
        L = _clamp(int(state.hist_len[b]), 0, state.hist_ld)
        if tok is not None and L < state.hist_ld:
            t = int(tok[b])
            state.hist[b, L] = t if -2 ** 31 <= t < 2 ** 31 else -1
            L += 1
            state.hist_len[b] = L
        n = _clamp(int(state.cfg[b, 0]), 0, CONSTRAINT_SEQ_LEN_MAX)
        min_new = int(state.cfg[b, 1])
        count = _clamp(int(state.seq_count[b]), 0, CONSTRAINT_SEQS_MAX)
        if n == 0 and count == 0:
            continue
        h = state.hist[b, :L].tolist()
        g = L - _clamp(int(state.prompt_len[b]), 0, L)
        table = []
        for s in range(count):
            m = _clamp(int(state.seq_len[b, s]), 0, CONSTRAINT_SEQ_LEN_MAX)
            if m > 0:
                table.append((int(state.seq_kind[b, s]), state.seq_tok[b, s, :m].tolist()))
        if row_state is not None and any(kind == ConstraintState.STOP and len(q) <= g and h[L - len(q):] == q for kind, q in table):
            row_state[b, 1] |= BatchRows.FINISHED
            live.sub_(1)
            continue
        banned = []
        for kind, q in table:
            m = len(q)
            if kind == ConstraintState.BAN and L >= m - 1 and h[L - (m - 1):L] == q[:m - 1]:
                banned.append(q[m - 1])
            if kind == ConstraintState.MIN and g < min_new:
                banned.append(q[0])
        if n >= 1 and L >= n:
            w = n - 1
            key = h[L - w:L]
            banned.extend(h[i + w] for i in range(L - n + 1) if h[i:i + w] == key)
        ids = sorted({v for v in banned if 0 <= v < N})
        if ids:
            logits[b, torch.tensor(ids, dtype=torch.long)] = float("-inf")


def history_constraints(logits: Tensor, state: ConstraintState, tok: Tensor | None = None, row_state: Tensor | None = None,
                        live: Tensor | None = None) -> Tensor:
    """Apply ``state``'s no-repeat n-gram rule, banned sequences and minimum length to `logits` (B, N) IN PLACE (-inf into every banned
    entry), advance the token history and finish rows that have generated a stop sequence, in one launch
    (``qlinear_history_constraints``, whose comment in include/qlinear_hip.h holds the rules).  ``tok`` (B,) int64: the ids fed into
    this step, appended first; None (the first token after a prefill): nothing is appended.  ``row_state`` / ``live`` (together or
    not at all): a ``BatchRows``' - finished rows are left untouched, and stop sequences are evaluated only with them.  Returns
    `logits`.  CPU tensors take the host form (Python, the same rules)."""
    if (row_state is None) != (live is None):
        raise ValueError("history_constraints: row_state and live go together")
    B, N = _check_step_logits("history_constraints", logits, state.batch, tok, row_state, state.hist, "ConstraintState")
    if live is not None and (live.dtype != torch.int32 or live.numel() != 1):
        raise ValueError("history_constraints: live must be an int32 tensor of one element (BatchRows.live)")
    if live is not None and live.device != logits.device:
        raise ValueError(f"history_constraints: logits on {logits.device}, state on {live.device}")
    if not logits.is_cuda:
        _history_constraints_host(logits, state, None if tok is None else tok.view(-1), row_state, live)
        return logits
    lib = _lib.get_lib()
    with torch.cuda.device(logits.device):
        st = lib.qlinear_history_constraints(logits.data_ptr(), B, N, logits.stride(0) if B > 1 else N, state.hist.data_ptr(),
                                             state.hist_ld, state.hist_len.data_ptr(), state.prompt_len.data_ptr(), state.cfg.data_ptr(),
                                             state.seq_tok.data_ptr(), state.seq_len.data_ptr(), state.seq_kind.data_ptr(),
                                             state.seq_count.data_ptr(), _lib.ptr(tok), _lib.ptr(row_state), _lib.ptr(live),
                                             _lib.dtype_code(logits.dtype), _lib.stream_ptr(logits.device))
    _lib.check(st, "qlinear_history_constraints")
    return logits


# ---- regex-constrained generation: the mask of a byte-level DFA over the vocabulary (csrc/grammar_mask.hip, chatglm_q_amd/grammar.py) ------
GRAMMAR_TABLE_MAX = 16384    # entries of one row's transition table (QL_GRAMMAR_TABLE_MAX, include/qlinear_hip.h): n_states * n_classes
GRAMMAR_STATES_MAX = 4095    # states of one row's automaton (QL_GRAMMAR_STATES_MAX)
GRAMMAR_CHUNK = 256          # tokens one workgroup of the launch walks (QL_GRAMMAR_CHUNK): the grid is ceil(N / GRAMMAR_CHUNK) x batch
GRAMMAR_DEAD = 0xFFFF


class _AutomatonState:
    """What ``GrammarState`` and ``PdaState`` share.  Per session: the vocabulary's byte table ``tok_off`` (n_tok + 1,) int32 / ``tok_bytes``
    uint8 (``grammar.TokenBytes``).  Per row: ``class_of`` (batch, 256) uint8, ``table`` (batch, GRAMMAR_TABLE_MAX) uint16 bit patterns
    (held as int16), ``accept`` (batch, GRAMMAR_STATES_MAX + 1) uint8, ``cfg`` (batch, n_cfg) int32 starting with n_states (0: the row has
    no grammar), eos_id (-1: none), ``state`` (batch,) int32 (-1 = dead) and ``ticket`` (batch,) int32.  ``active``: whether any row has a
    grammar."""

    def __init__(self, batch: int, token_bytes, device, n_cfg: int):
        from .grammar import TokenBytes
        name = type(self).__name__
        if batch < 1:
            raise ValueError(f"{name}: batch >= 1 (got {batch})")
        if not isinstance(token_bytes, TokenBytes):
            raise ValueError(f"{name}: token_bytes must be a grammar.TokenBytes (grammar.token_byte_table builds one)")
        self.batch, self.device, self.token_bytes = batch, torch.device(device), token_bytes
        self.n_tok, self.n_bytes = len(token_bytes), int(token_bytes.bytes.size)
        self.tok_off = torch.from_numpy(token_bytes.off.copy()).to(device)
        self.tok_bytes = torch.from_numpy(token_bytes.bytes.copy() if self.n_bytes else np.zeros(1, dtype=np.uint8)).to(device)
        self.class_of = torch.zeros((batch, 256), dtype=torch.uint8, device=device)
        self.table = torch.full((batch, GRAMMAR_TABLE_MAX), -1, dtype=torch.int16, device=device)
        self.accept = torch.zeros((batch, GRAMMAR_STATES_MAX + 1), dtype=torch.uint8, device=device)
        self.cfg = torch.zeros((batch, n_cfg), dtype=torch.int32, device=device)
        self.state = torch.zeros(batch, dtype=torch.int32, device=device)
        self.ticket = torch.zeros(batch, dtype=torch.int32, device=device)
        self.active = False

    @staticmethod
    def _check_eos(b: int, e, vocab: int | None) -> int:
        """Row b's end id as an int, -1 for None."""
        if e is None:
            e = -1
        if not _is_int(e) or not -1 <= int(e) < (2 ** 31 if vocab is None else vocab):
            raise ValueError(f"grammar: row {b}: eos_id {e!r} outside the vocabulary")
        return int(e)

    def _arm_tables(self, automata, eos, cfg_tail=None):
        """The common half of ``arm``: every row's tables and ``cfg`` (behind n_states and the end id: ``cfg_tail(automaton)``) stored,
        every state and ticket back to 0."""
        B = self.batch
        class_of = np.zeros((B, 256), dtype=np.uint8)
        table = np.full((B, GRAMMAR_TABLE_MAX), GRAMMAR_DEAD, dtype=np.uint16)
        accept = np.zeros((B, GRAMMAR_STATES_MAX + 1), dtype=np.uint8)
        cfg = np.zeros(tuple(self.cfg.shape), dtype=np.int32)
        for b, d in enumerate(automata):
            cfg[b, 1] = eos[b]
            if d is None:
                continue
            cfg[b, 0] = d.n_states
            if cfg_tail is not None:
                cfg[b, 2:] = cfg_tail(d)
            class_of[b] = d.class_of
            table[b, :d.table.size] = d.table.reshape(-1)
            accept[b, :d.n_states] = d.accept
        self.class_of.copy_(torch.from_numpy(class_of))
        self.table.copy_(torch.from_numpy(table.view(np.int16)))
        self.accept.copy_(torch.from_numpy(accept))
        self.cfg.copy_(torch.from_numpy(cfg))
        self.state.zero_()
        self.ticket.zero_()
        self.active = any(d is not None for d in automata)

    def states(self):
        """Every row's current state, read back: a list of ints, -1 = dead."""
        return self.state.cpu().tolist()


class GrammarState(_AutomatonState):
    """Static buffers of ``grammar_mask`` for a batch of rows (a captured step reads and updates them in place): ``_AutomatonState``'s, with
    ``cfg`` (batch, 2) int32 = n_states, eos_id and the table indexed ``state * n_classes + class``.  ``dfas``: what the last ``arm`` armed."""

    def __init__(self, batch: int, token_bytes, device):
        super().__init__(batch, token_bytes, device, n_cfg=2)
        self.dfas = [None] * batch

    @staticmethod
    def check(batch: int, dfas, eos_ids, vocab: int | None = None):
        """Validate one ``ByteDFA`` or None per row (or one for every row) and the end ids (one, one per row, None = none); returns
        (dfas, eos_ids) as lists, eos -1 for none.  A ValueError names the offending row."""
        from .grammar import ByteDFA
        dfas = ConstraintState.per_row("grammar", dfas, batch)
        eos = ConstraintState.per_row("eos_id", eos_ids, batch)
        out = []
        for b in range(batch):
            d = dfas[b]
            if d is not None and not isinstance(d, ByteDFA):
                raise ValueError(f"grammar: row {b}: a ByteDFA or None (got {type(d).__name__})")
            if d is not None and (d.n_states > GRAMMAR_STATES_MAX or d.n_states * d.n_classes > GRAMMAR_TABLE_MAX):
                raise ValueError(f"grammar: row {b}: {d.n_states} states x {d.n_classes} byte classes outside the caps "
                                 f"({GRAMMAR_STATES_MAX} states, {GRAMMAR_TABLE_MAX} table entries)")
            out.append(_AutomatonState._check_eos(b, eos[b], vocab))
        return dfas, out

    def arm(self, dfas, eos_ids=None):
        """Start a generation, in place (the buffers keep their addresses): row b follows ``dfas[b]`` (None: no grammar) from its start
        state, ``eos_ids[b]`` is the id allowed exactly in an accepting state.  Every state goes to 0, every ticket to 0."""
        dfas, eos = self.check(self.batch, dfas, eos_ids)
        self._arm_tables(dfas, eos)
        self.dfas = list(dfas)
        return self

    def tensors(self):
        """What a step changes and a capture saves and restores (the tickets are back at 0 behind every launch)."""
        return (self.state,)


def _host_token_bytes(state: _AutomatonState, N: int):
    """``token(i)`` of the host forms: (id i's bytes, whether its offsets are sound) - an id outside the logits or the table has no bytes."""
    off, data = state.tok_off.numpy(), state.tok_bytes.numpy()
    n_tok, n_bytes = state.n_tok, state.n_bytes

    def token(i):
        if not 0 <= i < min(N, n_tok):
            return b"", True
        o0, o1 = int(off[i]), int(off[i + 1])
        if o0 < 0 or o1 < o0 or o1 > n_bytes:
            return b"", False                                  # corrupt offsets: masked (the fed id: the row dies)
        return data[o0:o1].tobytes(), True

    return token


def _grammar_mask_host(logits: Tensor, state: GrammarState, tok, row_state):
    """CPU form of qlinear_grammar_mask: rules 0 - 3 of its comment in include/qlinear_hip.h, row by row in Python."""
    B, N = logits.shape
    token = _host_token_bytes(state, N)

    for b in range(B):
        if row_state is not None and int(row_state[b, 1]) & BatchRows.FINISHED:
            continue
        ns = _clamp(int(state.cfg[b, 0]), 0, GRAMMAR_STATES_MAX)
        if ns == 0:
            continue
        eos = int(state.cfg[b, 1])
        cls = state.class_of[b].tolist()
        nc = max(cls) + 1
        ns = min(ns, GRAMMAR_TABLE_MAX // nc)
        tbl = (state.table[b, :ns * nc].numpy().view(np.uint16)).tolist()

        def walk(s, bs):
            for v in bs:
                if s < 0:
                    break
                t = tbl[s * nc + cls[v]]
                s = t if t < ns else -1
            return s

        s = int(state.state[b])
        s = s if 0 <= s < ns else -1
        if tok is not None:
            fed, ok = token(int(tok[b]))
            s = walk(s, fed) if ok else -1
        banned = []
        for i in range(N):
            if i == eos:
                if s >= 0 and not int(state.accept[b, s]):
                    banned.append(i)
                continue
            bs, ok = token(i)
            if s < 0 or not ok or not bs or walk(s, bs) < 0:
                banned.append(i)
        if banned:
            logits[b, torch.tensor(banned, dtype=torch.long)] = float("-inf")
        state.state[b] = s


def grammar_mask(logits: Tensor, state: GrammarState, tok: Tensor | None = None, row_state: Tensor | None = None) -> Tensor:
    """Apply every row's automaton to `logits` (B, N) IN PLACE - -inf into every id whose bytes the row's state does not survive, and
    into the end id unless the state is accepting - and advance the state by the id the step was fed, in one launch
    (``qlinear_grammar_mask``, whose comment in include/qlinear_hip.h holds the rules).  ``tok`` (B,) int64: the ids fed into this step,
    walked first; None (the first token after a prefill): the state stays.  ``row_state``: a ``BatchRows``' - finished rows are left
    untouched.  Returns `logits`.  CPU tensors take the host form (Python, the same rules)."""
    if not isinstance(state, GrammarState):
        raise ValueError("grammar_mask: state must be a GrammarState")
    B, N = _check_step_logits("grammar_mask", logits, state.batch, tok, row_state, state.state, "GrammarState")
    if not logits.is_cuda:
        _grammar_mask_host(logits, state, None if tok is None else tok.view(-1), row_state)
        return logits
    lib = _lib.get_lib()
    with torch.cuda.device(logits.device):
        st = lib.qlinear_grammar_mask(logits.data_ptr(), B, N, logits.stride(0) if B > 1 else N, state.tok_off.data_ptr(),
                                      state.tok_bytes.data_ptr(), state.n_tok, state.n_bytes, state.class_of.data_ptr(),
                                      state.table.data_ptr(), state.accept.data_ptr(), state.cfg.data_ptr(), state.state.data_ptr(),
                                      state.ticket.data_ptr(), _lib.ptr(tok), _lib.ptr(row_state), _lib.dtype_code(logits.dtype),
                                      _lib.stream_ptr(logits.device))
    _lib.check(st, "qlinear_grammar_mask")
    return logits


# ---- JSON-constrained generation: the mask of a byte-level pushdown automaton over the vocabulary (csrc/pda_mask.hip, grammar.BytePDA) ------
PDA_DEPTH_MAX = 64           # symbols one row's stack holds (QL_PDA_DEPTH_MAX, include/qlinear_hip.h)
PDA_LOCAL_MAX = 32           # symbols one token's walk may hold above the lowest depth it reached (QL_PDA_LOCAL_MAX): the window rule
PDA_SYMS_MAX = 3             # stack symbols 1..n_syms (QL_PDA_SYMS_MAX)


class PdaState(_AutomatonState):
    """Static buffers of ``pda_mask`` for a batch of rows (a captured step reads and updates them in place): ``_AutomatonState``'s (the
    table indexed ``(state * (n_syms + 1) + top) * n_classes + class``, entries as ``grammar.pda_entry`` packs them), with ``cfg`` (batch, 4)
    int32 = n_states, eos_id, n_syms, max_depth, and per row besides ``depth`` (batch,) int32 and ``stack`` (batch, PDA_DEPTH_MAX) uint8,
    bottom first.  ``pdas``: what the last ``arm`` armed."""

    def __init__(self, batch: int, token_bytes, device):
        super().__init__(batch, token_bytes, device, n_cfg=4)
        self.depth = torch.zeros(batch, dtype=torch.int32, device=device)
        self.stack = torch.zeros((batch, PDA_DEPTH_MAX), dtype=torch.uint8, device=device)
        self.pdas = [None] * batch

    @staticmethod
    def check(batch: int, pdas, eos_ids, vocab: int | None = None):
        """Validate one ``BytePDA`` / ``ByteDFA`` (lifted: ``BytePDA.from_dfa``) or None per row (or one for every row) and the end ids
        (one, one per row, None = none); returns (pdas, eos_ids) as lists, eos -1 for none.  A ValueError names the offending row."""
        from .grammar import ByteDFA, BytePDA
        pdas = ConstraintState.per_row("grammar", pdas, batch)
        eos = ConstraintState.per_row("eos_id", eos_ids, batch)
        out_p, out_e, lifted = [], [], {}
        for b in range(batch):
            d = pdas[b]
            if isinstance(d, ByteDFA):
                d = lifted[id(d)] if id(d) in lifted else lifted.setdefault(id(d), BytePDA.from_dfa(d))
            if d is not None and not isinstance(d, BytePDA):
                raise ValueError(f"grammar: row {b}: a BytePDA, a ByteDFA or None (got {type(d).__name__})")
            if d is not None and (d.n_states > GRAMMAR_STATES_MAX or d.n_states * (d.n_syms + 1) * d.n_classes > GRAMMAR_TABLE_MAX
                                  or d.n_syms > PDA_SYMS_MAX or d.max_depth > PDA_DEPTH_MAX):
                raise ValueError(f"grammar: row {b}: {d.n_states} states x {d.n_syms + 1} stack tops x {d.n_classes} byte classes, depth "
                                 f"{d.max_depth} outside the caps ({GRAMMAR_STATES_MAX} states, {GRAMMAR_TABLE_MAX} table entries, "
                                 f"{PDA_SYMS_MAX} symbols, depth {PDA_DEPTH_MAX})")
            out_p.append(d)
            out_e.append(_AutomatonState._check_eos(b, eos[b], vocab))
        return out_p, out_e

    def arm(self, pdas, eos_ids=None):
        """Start a generation, in place (the buffers keep their addresses): row b follows ``pdas[b]`` (None: no grammar) from its start
        configuration - state 0, an empty stack - and ``eos_ids[b]`` is the id allowed exactly in an accepting state with an empty
        stack.  Every ticket goes to 0."""
        pdas, eos = self.check(self.batch, pdas, eos_ids)
        self._arm_tables(pdas, eos, lambda d: (d.n_syms, d.max_depth))
        self.depth.zero_()
        self.stack.zero_()
        self.pdas = list(pdas)
        return self

    def configs(self):
        """Every row's configuration, read back: (state, tuple of symbols), or None for a dead row."""
        s, d, k = self.state.cpu().tolist(), self.depth.cpu().tolist(), self.stack.cpu().tolist()
        return [None if s[b] < 0 else (s[b], tuple(k[b][:d[b]])) for b in range(self.batch)]

    def tensors(self):
        """What a step changes and a capture saves and restores (the tickets are back at 0 behind every launch)."""
        return (self.state, self.depth, self.stack)


def _pda_mask_host(logits: Tensor, state: PdaState, tok, row_state):
    """CPU form of qlinear_pda_mask: rules 0 - 6 of its comment in include/qlinear_hip.h, row by row in Python."""
    B, N = logits.shape
    token = _host_token_bytes(state, N)

    for b in range(B):
        if row_state is not None and int(row_state[b, 1]) & BatchRows.FINISHED:
            continue
        ns = min(int(state.cfg[b, 0]), GRAMMAR_STATES_MAX)
        if ns <= 0:
            continue
        eos = int(state.cfg[b, 1])
        nsy, maxd = _clamp(int(state.cfg[b, 2]), 0, PDA_SYMS_MAX), _clamp(int(state.cfg[b, 3]), 0, PDA_DEPTH_MAX)
        cls = state.class_of[b].tolist()
        nc = max(cls) + 1
        ns = min(ns, GRAMMAR_TABLE_MAX // ((nsy + 1) * nc))
        tbl = (state.table[b, :ns * (nsy + 1) * nc].numpy().view(np.uint16)).tolist()
        old = state.stack[b].tolist()

        def walk(s, low, stack, bs):
            """(s, low, own) behind ``bs`` from state s over stack[:low] (never changed) and no pushes of the walk's own; s = -1: dead."""
            own = []
            for v in bs:
                top = own[-1] if own else (stack[low - 1] if low else 0)
                e = tbl[(s * (nsy + 1) + top) * nc + cls[v]]
                t, op, sym = e & 0xFFF, (e >> 12) & 3, e >> 14
                if t >= ns or op == 3:
                    return -1, low, own
                if op == 2:
                    if sym == 0 or sym > nsy or low + len(own) >= maxd or len(own) >= PDA_LOCAL_MAX:
                        return -1, low, own
                    own.append(sym)
                elif op == 1:
                    if own:
                        own.pop()
                    elif low:
                        low -= 1
                    else:
                        return -1, low, own
                    if not own and low and not 1 <= stack[low - 1] <= nsy:
                        return -1, low, own
                s = t
            return s, low, own

        s, d = int(state.state[b]), int(state.depth[b])
        if not 0 <= s < ns or not 0 <= d <= maxd or (d > 0 and not 1 <= old[d - 1] <= nsy):
            s, d = -1, 0
        low, own = d, []
        if tok is not None and s >= 0:
            fed, ok = token(int(tok[b]))
            if not ok:
                s = -1
            elif fed:
                s, low, own = walk(s, d, old, fed)
        new = old[:low] + own if s >= 0 else old
        d = low + len(own) if s >= 0 else 0
        banned = []
        for i in range(N):
            if i == eos:
                if s >= 0 and not (int(state.accept[b, s]) and d == 0):
                    banned.append(i)
                continue
            bs, ok = token(i)
            if s < 0 or not ok or not bs or walk(s, d, new, bs)[0] < 0:
                banned.append(i)
        if banned:
            logits[b, torch.tensor(banned, dtype=torch.long)] = float("-inf")
        state.state[b] = s
        if s >= 0:
            state.depth[b] = d
            if own:
                state.stack[b, low:d] = torch.tensor(own, dtype=torch.uint8)


def pda_mask(logits: Tensor, state: PdaState, tok: Tensor | None = None, row_state: Tensor | None = None) -> Tensor:
    """Apply every row's pushdown automaton to `logits` (B, N) IN PLACE - -inf into every id whose bytes the row's configuration does
    not survive, and into the end id unless the state is accepting and the stack empty - and advance the configuration by the id the
    step was fed, in one launch (``qlinear_pda_mask``, whose comment in include/qlinear_hip.h holds the rules).  ``tok`` (B,) int64: the
    ids fed into this step, walked first; None (the first token after a prefill): nothing moves.  ``row_state``: a ``BatchRows``' -
    finished rows are left untouched.  Returns `logits`.  CPU tensors take the host form (Python, the same rules)."""
    if not isinstance(state, PdaState):
        raise ValueError("pda_mask: state must be a PdaState")
    B, N = _check_step_logits("pda_mask", logits, state.batch, tok, row_state, state.state, "PdaState")
    if not logits.is_cuda:
        _pda_mask_host(logits, state, None if tok is None else tok.view(-1), row_state)
        return logits
    lib = _lib.get_lib()
    with torch.cuda.device(logits.device):
        st = lib.qlinear_pda_mask(logits.data_ptr(), B, N, logits.stride(0) if B > 1 else N, state.tok_off.data_ptr(),
                                  state.tok_bytes.data_ptr(), state.n_tok, state.n_bytes, state.class_of.data_ptr(),
                                  state.table.data_ptr(), state.accept.data_ptr(), state.cfg.data_ptr(), state.state.data_ptr(),
                                  state.depth.data_ptr(), state.stack.data_ptr(), state.ticket.data_ptr(), _lib.ptr(tok),
                                  _lib.ptr(row_state), _lib.dtype_code(logits.dtype), _lib.stream_ptr(logits.device))
    _lib.check(st, "qlinear_pda_mask")
    return logits


# ---- log-probabilities during generation: the chosen token's and the most likely alternatives' (csrc/logprob.hip) -------------------------
TOP_LOGPROBS_MAX = 20        # alternatives one step can record (QL_TOP_LOGPROBS_MAX, include/qlinear_hip.h)


class StepLogprobs:
    """The record ``step_logprobs`` appends to (static device buffers a captured step reads and updates): ``count`` (batch,) int32 =
    entries recorded per row; ``chosen`` (batch, cap) float32 = log-prob of every recorded token; ``top_ids`` / ``top_lp`` (batch,
    cap, n_top) int32 / float32 = the ``n_top`` most likely ids of that step (value descending, ties: lowest index first) and their
    log-probs.  The width ``n_top`` defaults to TOP_LOGPROBS_MAX, so one captured graph serves every number of alternatives asked
    for; ``read`` slices."""

    def __init__(self, batch: int, cap: int, device, n_top: int = TOP_LOGPROBS_MAX):
        if batch < 1 or cap < 1 or not 0 <= n_top <= TOP_LOGPROBS_MAX:
            raise ValueError(f"StepLogprobs: batch >= 1, cap >= 1, 0 <= n_top <= {TOP_LOGPROBS_MAX} (got {batch}, {cap}, {n_top})")
        self.batch, self.cap, self.n_top, self.device = batch, cap, n_top, torch.device(device)
        self.count = torch.zeros(batch, dtype=torch.int32, device=device)
        self.chosen = torch.zeros((batch, cap), dtype=torch.float32, device=device)
        self.top_ids = torch.zeros((batch, cap, n_top), dtype=torch.int32, device=device)
        self.top_lp = torch.zeros((batch, cap, n_top), dtype=torch.float32, device=device)

    def arm(self):
        """Start a generation: nothing recorded (the buffers keep their addresses and, past ``count``, their old contents)."""
        self.count.zero_()
        return self

    def tensors(self):
        return (self.count, self.chosen, self.top_ids, self.top_lp)

    def fetch(self):
        """The whole record on the host, one copy per buffer: what ``read`` slices (pass it as ``host`` when reading several rows)."""
        return tuple(t.cpu() for t in self.tensors())

    def read(self, b: int, n: int | None = None, limit: int | None = None, host=None):
        """Row b's first ``min(count[b], limit)`` entries with ``n`` alternatives each (default: all ``n_top``), as lists:
        ``(token_logprobs, top_ids, top_logprobs)``."""
        n = self.n_top if n is None else int(n)
        if not 0 <= n <= self.n_top:
            raise ValueError(f"StepLogprobs.read: 0 <= n <= {self.n_top} (got {n})")
        count, chosen, ids, lps = self.fetch() if host is None else host
        k = min(int(count[b]), self.cap)
        if limit is not None:
            k = min(k, max(0, int(limit)))
        return chosen[b, :k].tolist(), ids[b, :k, :n].tolist(), lps[b, :k, :n].tolist()


def _step_logprobs_host(logits: Tensor, tok: Tensor, state: StepLogprobs, row_state):
    """CPU form of qlinear_step_logprobs: the same rules, torch's fp32 log_softmax and a stable descending sort for the order."""
    B, N = logits.shape
    n_top = state.n_top
    k = min(n_top, N)
    xf = logits.float()
    lsm_rows = torch.log_softmax(xf, dim=-1)                     # the call token_logprob's CPU branch makes
    for b in range(B):
        c = int(state.count[b])
        if row_state is not None and int(row_state[b, 0]) <= c:
            continue                                             # the row recorded no token in this step
        if c >= state.cap:
            continue
        x, lsm = xf[b], lsm_rows[b]
        t = int(tok[b])
        state.chosen[b, c] = lsm[t] if 0 <= t < N else float("nan")
        if n_top:
            order = torch.sort(torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x), descending=True, stable=True)[1][:k]
            state.top_ids[b, c, :k] = order.to(torch.int32)
            state.top_lp[b, c, :k] = lsm[order]
            state.top_ids[b, c, k:] = -1
            state.top_lp[b, c, k:] = float("-inf")
        state.count[b] = c + 1


def step_logprobs(logits: Tensor, tok: Tensor, state: StepLogprobs, row_state: Tensor | None = None) -> None:
    """Record one generation step in ``state`` (``qlinear_step_logprobs``, one launch behind the step's selection; its comment in
    include/qlinear_hip.h holds the rules): for every row of `logits` (B, N) - the row the selection read - the log-prob of the id
    just chosen, ``tok`` (B,) int64, and the ``state.n_top`` most likely ids with theirs, appended at ``state.count[b]``.
    ``row_state``: a ``BatchRows.row_state``; a row whose token count has not moved past its recorded entries (finished, out of
    budget) records nothing.  A full record (``state.cap`` entries) records nothing either.  On a GPU every value is bit-equal to
    ``token_logprob(logits, that id)``.  CPU tensors take the host form (torch ops, the same rules)."""
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError(f"step_logprobs: logits must be (B, N) with N >= 1, got {tuple(logits.shape)}")
    B, N = logits.shape
    if B != state.batch:
        raise ValueError(f"step_logprobs: {B} logits rows for a StepLogprobs of {state.batch}")
    if tok.dtype != torch.int64 or tok.numel() != B or not tok.is_contiguous():
        raise ValueError("step_logprobs: tok must be a contiguous int64 tensor of B elements")
    if row_state is not None and (row_state.dtype != torch.int32 or tuple(row_state.shape) != (B, 2) or not row_state.is_contiguous()):
        raise ValueError("step_logprobs: row_state must be a contiguous int32 (B, 2) tensor (BatchRows.row_state)")
    for t in (tok, row_state) + state.tensors():
        if t is not None and t.device != logits.device:
            raise ValueError(f"step_logprobs: logits on {logits.device}, state on {t.device}")
    if not logits.is_cuda:
        _step_logprobs_host(logits, tok.view(-1), state, row_state)
        return None
    lib = _lib.get_lib()
    if logits.stride(1) != 1 or (B > 1 and logits.stride(0) < N):
        logits = logits.contiguous()
    n_top = state.n_top
    with torch.cuda.device(logits.device):
        st = lib.qlinear_step_logprobs(logits.data_ptr(), B, N, logits.stride(0) if B > 1 else N, tok.data_ptr(), _lib.ptr(row_state),
                                       state.count.data_ptr(), state.chosen.data_ptr(), state.top_ids.data_ptr() if n_top else None,
                                       state.top_lp.data_ptr() if n_top else None, state.cap, n_top, _lib.dtype_code(logits.dtype),
                                       _lib.stream_ptr(logits.device))
    _lib.check(st, "qlinear_step_logprobs")
    return None


# ---- beam search: cross-beam selection and the cache reorder by parent beam (csrc/beam_search.hip) ---------------------------------
BEAMS_MAX = 10               # QL_BEAMS_MAX (include/qlinear_hip.h): a row supplies 2 * num_beams <= TOP_LOGPROBS_MAX candidates


def beam_norm_table(cap: int, length_penalty: float) -> Tensor:
    """norm[len] = float32(float64(len) ** length_penalty) for len = 0 .. cap: the device divides by it and never calls powf."""
    lp = float(length_penalty)
    if not _finite(lp):
        raise ValueError(f"beam search: length_penalty must be finite (got {length_penalty})")
    zero = 1.0 if lp == 0 else (0.0 if lp > 0 else float("inf"))
    return torch.tensor([zero] + [float(n) ** lp for n in range(1, cap + 1)], dtype=torch.float64).float()


class BeamState:
    """Static device buffers of a beam search over ``rows`` = P prompts x B beams batch rows (a captured step reads and updates them in
    place; rows g*B .. g*B+B-1 are group g): ``beam_score`` (rows,) float32 - the running beams' summed log-probs; ``parent`` (rows,)
    int32 - the row every row's beam came from in the last step; ``trellis`` (cap, rows, 2) int32 - (token, parent row) per step and
    row, read once at the end; ``steps`` / ``fin_count`` / ``done`` (rows,) int32, the first P entries used - per group the steps taken,
    the finished hypotheses held and whether the group is done; ``fin_score`` / ``fin_sum`` (rows,) float32 and ``fin_len`` / ``fin_row``
    (rows,) int32, read as (P, B) - the finished heap: normalised score, summed log-prob, length and parent row; ``live`` (1,) int32 -
    groups not done; ``norm`` (cap + 1,) float32 - len ** length_penalty; ``cfg`` (2,) int32 - end id (-1: none), early_stopping;
    ``first`` (1,) int32 - the first cache position the step's gather moves (the prompt length); ``cand`` - the one-slot ``StepLogprobs``
    record (2B alternatives) that supplies every row's candidates, reallocated when B changes."""

    def __init__(self, rows: int, cap: int, device):
        if rows < 1 or cap < 1:
            raise ValueError(f"BeamState: rows >= 1 and cap >= 1 (got {rows}, {cap})")
        self.rows, self.cap, self.device = rows, cap, torch.device(device)
        f32, i32 = dict(dtype=torch.float32, device=device), dict(dtype=torch.int32, device=device)
        self.beam_score = torch.zeros(rows, **f32)
        self.parent = torch.arange(rows, **i32)
        self.trellis = torch.zeros((cap, rows, 2), **i32)
        self.steps, self.fin_count, self.done = (torch.zeros(rows, **i32) for _ in range(3))
        self.fin_score, self.fin_sum = torch.zeros(rows, **f32), torch.zeros(rows, **f32)
        self.fin_len, self.fin_row = torch.zeros(rows, **i32), torch.zeros(rows, **i32)
        self.live = torch.zeros(1, **i32)
        self.norm = torch.ones(cap + 1, **f32)
        self.cfg = torch.zeros(2, **i32)
        self.first = torch.zeros(1, **i32)
        self.cand = None
        self.P = self.B = 0
        self.eos = -1

    def arm(self, P: int, B: int, eos=None, length_penalty: float = 1.0, early_stopping: bool = True, first: int = 0):
        """Start a search of P prompts x B beams, in place (the buffers keep their addresses; only ``cand`` is reallocated when B
        changes): scores 0 for every group's first row and -inf for the others, nothing finished, nothing recorded."""
        if not 1 <= B <= BEAMS_MAX:
            raise ValueError(f"BeamState.arm: num_beams must be in [1, {BEAMS_MAX}] (got {B})")
        if P < 1 or P * B != self.rows:
            raise ValueError(f"BeamState.arm: {P} prompts x {B} beams for a state of {self.rows} rows")
        if not 0 <= int(first) <= 2 ** 31 - 1:
            raise ValueError(f"BeamState.arm: first must be a cache position (got {first})")
        norm = beam_norm_table(self.cap, length_penalty)
        if self.cand is None or B != self.B:
            self.cand = StepLogprobs(self.rows, 1, self.device, n_top=2 * B)
        self.cand.arm()
        self.P, self.B = P, B
        self.eos = -1 if eos is None or int(eos) < 0 else int(eos)
        score = torch.full((self.rows,), float("-inf"), dtype=torch.float32)
        score[::B] = 0.0
        self.beam_score.copy_(score)
        self.parent.copy_(torch.arange(self.rows, dtype=torch.int32))
        for t in (self.steps, self.fin_count, self.done, self.fin_score, self.fin_sum, self.fin_len, self.fin_row):
            t.zero_()
        self.live.fill_(P)
        self.norm.copy_(norm)
        self.cfg.copy_(torch.tensor([self.eos, 1 if early_stopping else 0], dtype=torch.int32))
        self.first.fill_(int(first))
        return self

    def tensors(self):
        """What a step changes besides the trellis (a capture saves and restores it; the trellis slots its warm-up runs write are
        written again by the steps that follow)."""
        return (self.beam_score, self.parent, self.steps, self.fin_count, self.done, self.fin_score, self.fin_sum, self.fin_len,
                self.fin_row, self.live, self.cand.count)

    def fetch(self) -> dict:
        """Everything the host needs at the end of a search, one copy per buffer."""
        names = ("beam_score", "parent", "trellis", "steps", "fin_count", "done", "fin_score", "fin_sum", "fin_len", "fin_row", "live")
        return {k: getattr(self, k).cpu() for k in names}


def _beam_advance_host(state: BeamState, tok: Tensor, write_index, pos, mask):
    """CPU form of qlinear_beam_advance: the same rules, every score one fp32 torch operation."""
    P, B = state.P, state.B
    eos, early = int(state.cfg[0]), bool(int(state.cfg[1]))
    ids, lps = state.cand.top_ids[:, 0], state.cand.top_lp[:, 0]
    neg = torch.tensor(float("-inf"), dtype=torch.float32)
    for g in range(P):
        r0 = g * B
        st = int(state.steps[g])
        state.cand.count[r0:r0 + B] = 0
        if int(state.done[g]) != 0 or st >= state.cap:
            tok[r0:r0 + B] = eos if eos >= 0 else 0
            state.parent[r0:r0 + B] = torch.arange(r0, r0 + B, dtype=torch.int32)
            continue
        scores = (state.beam_score[r0:r0 + B, None] + lps[r0:r0 + B]).reshape(-1)            # one fp32 add each
        keys = torch.where(torch.isnan(scores), neg, scores).tolist()
        order = sorted(range(B * 2 * B), key=lambda c: (-keys[c], c))[:2 * B]
        t = st + 1
        nrm = state.norm[t]
        cnt = int(state.fin_count[g])
        heap = state.fin_score[r0:r0 + B]

        def worst_slot():
            worst = 0
            for q in range(1, B):
                if bool(heap[q] <= heap[worst]):
                    worst = q
            return worst

        nxt = []
        for j, c in enumerate(order):
            if len(nxt) == B:
                break
            sc, i, r = scores[c], int(ids.reshape(-1)[r0 * 2 * B + c]), r0 + c // (2 * B)
            if eos >= 0 and i == eos:
                if j < B:
                    hs = sc / nrm
                    slot = -1
                    if cnt < B:
                        slot, cnt = cnt, cnt + 1
                    else:
                        w = worst_slot()
                        if bool(hs > heap[w]):
                            slot = w
                    if slot >= 0:
                        state.fin_score[r0 + slot], state.fin_sum[r0 + slot] = hs, sc
                        state.fin_len[r0 + slot], state.fin_row[r0 + slot] = t, r
                continue
            nxt.append((i, r, sc))
        while len(nxt) < B:                                      # (cannot happen with 2B candidates per row)
            nxt.append((eos if eos >= 0 else 0, r0 + len(nxt), neg))
        state.fin_count[g] = cnt
        fin = cnt == B
        if fin and not early:
            fin = bool(heap[worst_slot()] >= nxt[0][2] / nrm)
        for n, (i, r, sc) in enumerate(nxt):
            tok[r0 + n], state.parent[r0 + n], state.beam_score[r0 + n] = i, r, sc
            state.trellis[st, r0 + n, 0], state.trellis[st, r0 + n, 1] = i, r
        state.steps[g] = t
        if fin:
            state.done[g] = 1
            state.live.sub_(1)
    if write_index is not None:
        write_index.add_(1)
        pos.add_(1)
        nw = int(write_index.view(-1)[0])
        if 0 <= nw < mask.shape[-1]:
            mask[..., nw] = 0.0


def beam_advance(state: BeamState, tok: Tensor, write_index: Tensor | None = None, pos: Tensor | None = None, mask: Tensor | None = None):
    """One beam step's cross-beam selection in one launch (``qlinear_beam_advance``; the rules: include/qlinear_hip.h and
    tests/_beam_oracle.py) from the candidates ``step_logprobs(logits, tok, state.cand)`` has just recorded: the merge of every group's
    B x 2B candidates, the walk, the finished heap, done / ``live``, the trellis append, the next ``tok`` (rows,) int64, ``parent`` and
    ``beam_score``.  With write_index / pos / mask (all or none) the decode step's bookkeeping is done as ``greedy_advance`` does it.
    CPU tensors take the host form (the same rules bit for bit)."""
    if state.B < 1 or state.cand is None:
        raise ValueError("beam_advance: the BeamState is not armed")
    R = state.rows
    if tok.dtype != torch.int64 or tok.numel() != R or not tok.is_contiguous():
        raise ValueError(f"beam_advance: tok must be a contiguous int64 tensor of {R} elements")
    book = (write_index is not None, pos is not None, mask is not None)
    if any(book) and not all(book):
        raise ValueError("beam_advance: write_index, pos and mask go together")
    if all(book):
        if write_index.dtype != torch.int64 or pos.dtype != torch.int64 or pos.numel() != R or not pos.is_contiguous():
            raise ValueError(f"beam_advance: write_index and pos must be int64, pos of {R} elements")
        if mask.dtype != torch.float32 or mask.numel() != R * mask.shape[-1] or not mask.is_contiguous():
            raise ValueError(f"beam_advance: mask must be a contiguous fp32 ({R}, 1, capacity) tensor")
    for t in (tok, write_index, pos, mask):
        if t is not None and t.device != state.beam_score.device:
            raise ValueError(f"beam_advance: state on {state.beam_score.device}, step tensors on {t.device}")
    if not tok.is_cuda:
        _beam_advance_host(state, tok.view(-1), write_index, pos, mask)
        return None
    lib = _lib.get_lib()
    c = state.cand
    with torch.cuda.device(tok.device):
        st = lib.qlinear_beam_advance(state.P, state.B, c.top_ids.data_ptr(), c.top_lp.data_ptr(), c.count.data_ptr(),
                                      state.beam_score.data_ptr(), tok.data_ptr(), state.parent.data_ptr(), state.trellis.data_ptr(),
                                      state.cap, state.steps.data_ptr(), state.fin_score.data_ptr(), state.fin_sum.data_ptr(),
                                      state.fin_len.data_ptr(), state.fin_row.data_ptr(), state.fin_count.data_ptr(), state.done.data_ptr(),
                                      state.live.data_ptr(), state.norm.data_ptr(), state.cfg.data_ptr(), _lib.ptr(write_index), _lib.ptr(pos),
                                      _lib.ptr(mask), mask.shape[-1] if mask is not None else 0, _lib.stream_ptr(tok.device))
    _lib.check(st, "qlinear_beam_advance")
    return None


class BeamGatherTable:
    """The buffers one ``beam_gather`` launch reorders: tensors of one shape (rows, capacity, ...), dtype and device, each contiguous -
    a session's ``cache.k`` and ``cache.v`` of every layer (any other per-row, per-position state of that layout can be added) - and,
    on a GPU, the device table of their base addresses.  The tensors are kept alive with the table."""

    def __init__(self, buffers):
        buffers = list(buffers)
        if not buffers:
            raise ValueError("BeamGatherTable: at least one buffer")
        b0 = buffers[0]
        if b0.dim() < 2:
            raise ValueError("BeamGatherTable: buffers must be (rows, capacity, ...)")
        for b in buffers:
            if b.shape != b0.shape or b.dtype != b0.dtype or b.device != b0.device or not b.is_contiguous():
                raise ValueError("BeamGatherTable: every buffer must be contiguous, of one shape, dtype and device")
        self.buffers = buffers
        self.rows, self.capacity = int(b0.shape[0]), int(b0.shape[1])
        self.pos_bytes = (b0[0, 0].numel() if b0.dim() > 2 else 1) * b0.element_size()
        if self.pos_bytes < 2 or self.pos_bytes % 2:
            raise ValueError(f"BeamGatherTable: a position of {self.pos_bytes} bytes (an even size of at least 2 is served)")
        chunk = 16 if self.pos_bytes % 16 == 0 else (4 if self.pos_bytes % 4 == 0 else 2)
        if any(b.data_ptr() % chunk for b in buffers):
            raise ValueError(f"BeamGatherTable: every buffer must be aligned to {chunk} bytes")
        self.device = b0.device
        self.table = torch.tensor([b.data_ptr() for b in buffers], dtype=torch.int64).to(b0.device) if b0.is_cuda else None


def beam_gather(table: BeamGatherTable, parent: Tensor, first: Tensor, end: Tensor, num_beams: int) -> None:
    """Reorder every buffer of ``table`` by parent beam IN PLACE, in one launch (``qlinear_beam_gather``): ``buf[r, p] = buf[parent[r],
    p]`` for every row r and every position p in [first[0], end[0]) (clamped to the capacity).  ``parent`` (rows,) int32 - absolute
    rows, clamped to the row's own group of ``num_beams`` rows; ``first`` (1,) int32 and ``end`` (1,) int64 live on the device, so one
    captured launch serves every range.  CPU tensors take an ``index_select`` copy."""
    B = int(num_beams)
    if not 1 <= B <= BEAMS_MAX or table.rows % B:
        raise ValueError(f"beam_gather: num_beams in [1, {BEAMS_MAX}] dividing the {table.rows} rows (got {num_beams})")
    if parent.dtype != torch.int32 or parent.numel() != table.rows or not parent.is_contiguous():
        raise ValueError(f"beam_gather: parent must be a contiguous int32 tensor of {table.rows} elements")
    if first.dtype != torch.int32 or first.numel() != 1 or end.dtype != torch.int64 or end.numel() != 1:
        raise ValueError("beam_gather: first must be int32[1] and end int64[1]")
    for t in (parent, first, end):
        if t.device != table.device:
            raise ValueError(f"beam_gather: buffers on {table.device}, arguments on {t.device}")
    if table.table is None:
        lo, hi = max(int(first.view(-1)[0]), 0), min(int(end.view(-1)[0]), table.capacity)
        base = torch.arange(table.rows, dtype=torch.int64) // B * B
        src = base + (parent.view(-1).long() - base).clamp(0, B - 1)
        if lo < hi and not torch.equal(src, torch.arange(table.rows)):
            for b in table.buffers:
                b[:, lo:hi] = b.index_select(0, src)[:, lo:hi]
        return None
    lib = _lib.get_lib()
    with torch.cuda.device(table.device):
        st = lib.qlinear_beam_gather(table.table.data_ptr(), len(table.buffers), table.rows // B, B, table.capacity, table.pos_bytes,
                                     parent.data_ptr(), first.data_ptr(), end.data_ptr(), _lib.stream_ptr(table.device))
    _lib.check(st, "qlinear_beam_gather")
    return None


# ---- GPTQ: the column walk of one block (csrc/gptq.hip) ------------------------------------------------------------------------------
GPTQ_MAX_BLOCK = 128


def _gptq_block_host(weight: Tensor, c0: int, bc: int, hinv: Tensor, bits: int, scale: Tensor, group: int):
    """The column walk with torch ops, all rows at once and one column per iteration: the reference's inner loop
    (chatglm_q/int4/quantizer.py:151-167, chatglm_q/int8/quantizer.py:126-137).  Every op is one fp32 rounding."""
    qmax = 7 if bits == 4 else 127
    w = weight[:, c0:c0 + bc].clone()
    h = hinv[c0:c0 + bc, c0:c0 + bc]
    Q, Err, Loss = torch.empty_like(w), torch.empty_like(w), torch.empty_like(w)
    s = scale if bits == 8 else None
    for j in range(bc):
        if bits == 4 and j % group == 0:
            s = torch.clamp(w[:, j:j + group].abs().amax(dim=1) / qmax, min=1e-10)
            scale[(c0 + j) // group] = s
        d = h[j, j]
        col = w[:, j]
        q = s * torch.clamp(torch.round(col / s), -qmax, qmax)
        e = col - q
        err = e / d
        Q[:, j], Err[:, j], Loss[:, j] = q, err, ((e * e) / (d * d)) * 0.5
        if j + 1 < bc:
            w[:, j + 1:] -= err[:, None] * h[j, j + 1:][None, :]
    return Q, Err, Loss


def gptq_block(weight: Tensor, c0: int, bc: int, hinv: Tensor, bits: int, scale: Tensor, group: int = 32, use_kernel: bool | None = None):
    """GPTQ over the input columns [c0, c0 + bc) of ``weight`` (n_rows, n_columns; nn.Linear layout, fp32), bc <= 128, with the
    upper Cholesky factor ``hinv`` (n_columns, n_columns) of the inverse Hessian: returns ``(Q, Err, Loss)``, each (n_rows, bc) -
    the grid values, the scaled errors and the loss terms (the rules: qlinear_gptq_block in include/qlinear_hip.h).  ``bits`` 4:
    ``scale`` (n_columns / group, n_rows) gets its rows c0 / group ... WRITTEN; ``bits`` 8: ``scale`` (n_rows) is read.  ``weight``
    is not modified: the caller subtracts ``Err @ hinv[c0:c0+bc, c0+bc:]`` from the columns to the right before the next block.
    GPU tensors take ONE launch of the HIP kernel, anything else the same formula in torch ops (``use_kernel`` forces either)."""
    if bits not in (4, 8):
        raise ValueError(f"gptq_block: bits must be 4 or 8, got {bits}")
    if weight.dim() != 2 or hinv.dim() != 2 or hinv.shape[0] != hinv.shape[1] or hinv.shape[0] != weight.shape[1]:
        raise ValueError(f"gptq_block: weight {tuple(weight.shape)} does not go with a factor of {tuple(hinv.shape)}")
    n_rows, n_cols = weight.shape
    if not (1 <= bc <= GPTQ_MAX_BLOCK and 0 <= c0 and c0 + bc <= n_cols):
        raise ValueError(f"gptq_block: columns [{c0}, {c0 + bc}) of {n_cols} (at most {GPTQ_MAX_BLOCK} per block)")
    if bits == 4:
        if group < 2 or group % 2 or bc % group or c0 % group or n_cols % group:
            raise ValueError(f"gptq_block: group {group} does not divide columns [{c0}, {c0 + bc}) of {n_cols}")
        want = (n_cols // group, n_rows)
    else:
        want = (n_rows,)
    if tuple(scale.shape) != want or scale.dtype != torch.float32 or not scale.is_contiguous():
        raise ValueError(f"gptq_block: scale must be a contiguous float32 tensor of shape {want}")
    for t in (weight, hinv):
        if t.dtype != torch.float32 or t.stride(1) != 1:
            raise ValueError("gptq_block: weight and hinv must be float32 with unit column stride")
    if hinv.device != weight.device or scale.device != weight.device:
        raise ValueError("gptq_block: weight, hinv and scale must be on one device")
    if use_kernel is None:
        use_kernel = weight.is_cuda
    if not use_kernel:
        return _gptq_block_host(weight, c0, bc, hinv, bits, scale, group)
    if not weight.is_cuda:
        raise ValueError("gptq_block: the kernel needs GPU tensors")
    lib = _lib.get_lib()
    Q, Err, Loss = (torch.empty((n_rows, bc), dtype=torch.float32, device=weight.device) for _ in range(3))
    ldw = weight.stride(0) if n_rows > 1 else n_cols
    ldh = hinv.stride(0) if n_cols > 1 else 1
    with torch.cuda.device(weight.device):
        st = lib.qlinear_gptq_block(weight.data_ptr(), n_rows, ldw, c0, bc, hinv.data_ptr() + 4 * (c0 * ldh + c0), ldh, bits, group,
                                    Q.data_ptr(), Err.data_ptr(), Loss.data_ptr(), scale.data_ptr(), n_rows,
                                    _lib.dtype_code(weight.dtype), _lib.stream_ptr(weight.device))
    _lib.check(st, "qlinear_gptq_block")
    return Q, Err, Loss
