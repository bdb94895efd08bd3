"""Document masking and per-document positions for packed sequences: the rules, in plain torch, and the bounds
kernel's binding.

A training row is a fixed window of a token stream, so it usually holds several unrelated documents separated by an
end-of-text token. With document masking a token attends only to the earlier tokens of its own document
(block-diagonal causal attention). This module states the contract of the kernels that implement it
(csrc/packing.hip, the ``_doc`` entries of csrc/attention.hip, csrc/fp32.hip and csrc/norm_embed.hip) as pure-torch
functions.

The mask. Row ``b`` of a batch is partitioned into documents, contiguous intervals ``[s, e)``. ``DocBounds(start, end)``
holds two contiguous int32 ``[B, T]`` device tensors with, for every ``t``::

    0 <= start[b, t] <= t < end[b, t] <= T,     start and end constant over [start[b, t], end[b, t])

Query ``t`` attends key ``k`` iff ``start[b, t] <= k <= t``; given ``k <= t`` that is the same as ``t < end[b, k]``
(the forward and dQ kernels, which own queries, read ``start``; the dK/dV kernel, which owns keys, reads ``end``). The
softmax, its fp32 statistics and the dropout decision of a pair (query, key) are those of the unmasked kernels, and
no row is ever fully masked: key ``t`` is visible to query ``t``.

Positions. By default they stay absolute: token ``t`` of a row takes ``wpe[t]`` whatever document it is in. The option
(``reset_positions=True`` beside ``doc_bounds``) restarts them at every document, ``doc_positions(bounds)``::

    pos[b, t] = t - start[b, t]
    x[b, t]   = drop(wte[idx[b, t]] + wpe[pos[b, t]])                       for t < T_valid
    dwte[idx[b, t]] += g[b, t],   dwpe[p] += sum of g[b, t] over the (b, t) with t < T_valid and pos[b, t] == p

with ``g = drop'(dres)``. With it, and with dropout off, a document inside a packed row produces the activations, logits
and loss terms it produces alone in a row, up to rounding. The dropout decision of an element stays the hash of
``(seed, row * C + e)``: it depends on the row, not on the position. Padding rows ``t >= T_valid`` are exact zeros with no
table read, whatever the bounds say there. Rows of ``wpe`` and ``dwpe`` from the longest document's length on are
neither read nor written. ``dwpe`` is summed without floating-point atomics, in an order fixed by the inputs: two runs give the same
bits. A ``start`` outside ``[0, t]`` is clamped into it where it is read (``gpt2mi_embed_fwd_doc`` /
``gpt2mi_embed_bwd_doc``), as the attention kernels clamp it: wrong bounds give wrong numbers, never an access out of
range.

Bounds from tokens. A document begins at position ``p`` when ``idx[p - 1]`` is the separator (``eot="end"``: the
separator is the last token of the document it closes, nanoGPT's data preparation) or when ``idx[p]`` is
(``eot="begin"``: it opens a document, llm.c's). Then ``start[t]`` is the last beginning ``<= t`` (0 if none) and
``end[t]`` the first beginning ``> t`` (``T_valid`` if none). Positions ``>= T_valid`` are the engine's padding to the
64-token attention tile: they form one document ``[T_valid, T)`` of their own, and real documents end at ``T_valid``.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

EOT_POSITIONS = ("end", "begin")


class DocBounds(NamedTuple):
    start: torch.Tensor  # int32 [B, T]: first position of the document holding t
    end: torch.Tensor    # int32 [B, T]: one past its last position


def _eot_begin(eot: str) -> bool:
    if eot not in EOT_POSITIONS:
        raise ValueError(f"eot must be one of {EOT_POSITIONS}, got {eot!r}")
    return eot == "begin"


def _check_idx(idx: torch.Tensor, T_valid: Optional[int]) -> int:
    if idx.dim() != 2 or idx.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"idx must be an integer [B, T] tensor, got {idx.dtype} {tuple(idx.shape)}")
    T = idx.shape[1]
    tv = T if T_valid is None else int(T_valid)
    if not 1 <= tv <= T:
        raise ValueError(f"T_valid={tv} must be in [1, T={T}]")
    return tv


def doc_bounds_reference(idx: torch.Tensor, eot_token_id: int, eot: str = "end",
                         T_valid: Optional[int] = None) -> DocBounds:
    """The bounds of ``idx`` [B, T] from its separator tokens, in plain torch on idx's device (the module docstring
    is the rule; ``gpt2mi_doc_bounds`` gives the same integers)."""
    begin = _eot_begin(eot)
    tv = _check_idx(idx, T_valid)
    B, T = idx.shape
    pos = torch.arange(T, device=idx.device).expand(B, T)
    sep = idx == int(eot_token_id)
    if begin:
        boundary = sep.clone()
    else:
        boundary = torch.zeros_like(sep)
        boundary[:, 1:] = sep[:, :-1]
    boundary &= pos < tv
    # start: running maximum of the boundary positions; end: running minimum, from the right, of those after t
    start = torch.where(boundary, pos, torch.zeros_like(pos)).cummax(dim=1).values
    nxt = torch.where(boundary, pos, torch.full_like(pos, tv))
    at_or_after = nxt.flip(1).cummin(dim=1).values.flip(1)  # first boundary >= t
    end = torch.full_like(pos, tv)
    end[:, :-1] = at_or_after[:, 1:]
    pad = pos >= tv
    start = torch.where(pad, torch.full_like(pos, tv), start)
    end = torch.where(pad, torch.full_like(pos, T), end)
    return DocBounds(start.to(torch.int32).contiguous(), end.to(torch.int32).contiguous())


def doc_bounds(idx: torch.Tensor, eot_token_id: int, eot: str = "end", T_valid: Optional[int] = None) -> DocBounds:
    """``doc_bounds_reference`` by the device kernel (``gpt2mi_doc_bounds``): one launch on the current stream, no
    host synchronisation. ``idx`` is a cuda [B, T] tensor."""
    from . import _lib as K
    begin = _eot_begin(eot)
    tv = _check_idx(idx, T_valid)
    if not idx.is_cuda:
        raise ValueError("doc_bounds runs on the device: idx must be a cuda tensor (doc_bounds_reference runs anywhere)")
    idx = idx.long().contiguous()
    start = torch.empty(idx.shape, dtype=torch.int32, device=idx.device)
    end = torch.empty_like(start)
    K.doc_bounds(idx, int(eot_token_id), begin, start, end, T_valid=tv)
    return DocBounds(start, end)


def doc_bounds_from_ids(doc_ids: torch.Tensor) -> DocBounds:
    """The bounds of rows whose tokens carry a document id, ``doc_ids`` integer [B, T]: a document is a maximal run of
    equal ids. Raises ValueError when an id's positions are not contiguous (synchronises the host)."""
    if doc_ids.dim() != 2 or doc_ids.dtype.is_floating_point or doc_ids.dtype == torch.bool:
        raise ValueError(f"doc_ids must be an integer [B, T] tensor, got {doc_ids.dtype} {tuple(doc_ids.shape)}")
    B, T = doc_ids.shape
    pos = torch.arange(T, device=doc_ids.device).expand(B, T)
    boundary = torch.ones(B, T, dtype=torch.bool, device=doc_ids.device)
    boundary[:, 1:] = doc_ids[:, 1:] != doc_ids[:, :-1]
    runs = boundary.sum(dim=1)
    for b in range(B):
        if int(runs[b]) != int(torch.unique(doc_ids[b]).numel()):
            raise ValueError(f"doc_ids row {b}: the positions of a document id are not contiguous")
    start = torch.where(boundary, pos, torch.zeros_like(pos)).cummax(dim=1).values
    nxt = torch.where(boundary, pos, torch.full_like(pos, T))
    at_or_after = nxt.flip(1).cummin(dim=1).values.flip(1)
    end = torch.full_like(pos, T)
    end[:, :-1] = at_or_after[:, 1:]
    return DocBounds(start.to(torch.int32).contiguous(), end.to(torch.int32).contiguous())


def check_bounds_meta(bounds, B: int, T: int, device=None) -> DocBounds:
    """What can be checked of a bounds pair without reading it: a pair of contiguous int32 [B, T] tensors (on
    ``device`` if given). Raises ValueError; no host synchronisation."""
    try:
        start, end = bounds
    except (TypeError, ValueError):
        raise ValueError("doc_bounds must be a DocBounds(start, end) pair of int32 [B, T] tensors") from None
    for name, t in (("start", start), ("end", end)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"doc_bounds.{name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.int32:
            raise ValueError(f"doc_bounds.{name} must be int32, got {t.dtype}")
        if tuple(t.shape) != (B, T):
            raise ValueError(f"doc_bounds.{name} has shape {tuple(t.shape)}, expected {(B, T)} (the shape of idx)")
        if not t.is_contiguous():
            raise ValueError(f"doc_bounds.{name} must be contiguous")
        if device is not None and t.device != torch.device(device):
            raise ValueError(f"doc_bounds.{name} is on {t.device}, expected {torch.device(device)}")
    return DocBounds(start, end)


def check_bounds(bounds) -> DocBounds:
    """Validate a hand-made pair against the contract of the module docstring. Opt-in: it reads the tensors, so it
    synchronises the host. Raises ValueError naming the first violation."""
    try:
        start, end = bounds
    except (TypeError, ValueError):
        raise ValueError("doc_bounds must be a DocBounds(start, end) pair of int32 [B, T] tensors") from None
    if not isinstance(start, torch.Tensor) or start.dim() != 2:
        raise ValueError("doc_bounds.start must be an int32 [B, T] tensor")
    B, T = start.shape
    start, end = check_bounds_meta(bounds, B, T)
    s, e = start.long(), end.long()
    pos = torch.arange(T, device=s.device).expand(B, T)
    if bool(((s < 0) | (s > pos)).any()):
        raise ValueError("doc_bounds: start[b, t] must be in [0, t]")
    if bool(((e <= pos) | (e > T)).any()):
        raise ValueError("doc_bounds: end[b, t] must be in [t + 1, T]")
    # constant over [start, end): the first position of the interval is its own start, the last its own end - 1,
    # and neighbours inside one interval agree
    same = (s[:, 1:] == s[:, :-1]) & (e[:, 1:] == e[:, :-1])
    new = (s[:, 1:] == pos[:, 1:]) & (e[:, :-1] == pos[:, 1:])
    if bool((s[:, 0] != 0).any()) or bool((e[:, -1] != T).any()) or not bool((same | new).all()):
        raise ValueError("doc_bounds: start and end must be constant over [start[b, t], end[b, t]) "
                         "(the documents must partition the row)")
    return DocBounds(start, end)


def pad_bounds(bounds: DocBounds, Tp: int) -> DocBounds:
    """Bounds of rows padded from T to Tp positions: the padding is one document [T, Tp) of its own."""
    start, end = bounds
    B, T = start.shape
    if Tp == T:
        return DocBounds(start, end)
    ps = torch.full((B, Tp - T), T, dtype=torch.int32, device=start.device)
    pe = torch.full((B, Tp - T), Tp, dtype=torch.int32, device=start.device)
    return DocBounds(torch.cat([start, ps], dim=1).contiguous(), torch.cat([end, pe], dim=1).contiguous())


def doc_mask(bounds: DocBounds) -> torch.Tensor:
    """The visible (query, key) pairs as bool [B, T(query), T(key)]: start[b, t] <= k <= t."""
    start = bounds.start.long()
    T = start.shape[1]
    k = torch.arange(T, device=start.device)
    return (k[None, None, :] >= start[:, :, None]) & (k[None, None, :] <= k[None, :, None])


def doc_positions(bounds: DocBounds) -> torch.Tensor:
    """The position of every token in its own document, int32 [B, T]: ``pos[b, t] = t - start[b, t]`` (0 at the first
    token of every document). What ``reset_positions=True`` indexes ``wpe`` with."""
    start = bounds.start
    T = start.shape[1]
    t = torch.arange(T, dtype=torch.int32, device=start.device)
    return (t[None, :] - start.to(torch.int32)).contiguous()


def doc_attention_reference(q, k, v, bounds: DocBounds, dO=None, scale=None, dtype=torch.float64):
    """Document-masked attention of q, k, v [B, H, T, D] and its backward in ``dtype``: the reference the kernels are
    tested against. scores = q k^T / sqrt(D), -inf outside the mask; P = softmax; out = (P * scale) v with ``scale``
    the ``keep / (1 - p)`` dropout multipliers [B, H, T, T] (None: no dropout); lse = logsumexp of the masked scores.
    Returns ``(out, lse, dq, dk, dv)``; the gradients are None without ``dO``."""
    D = q.shape[-1]
    qr, kr, vr = (t.detach().to(dtype).clone().requires_grad_(dO is not None) for t in (q, k, v))
    mask = doc_mask(bounds).to(qr.device)[:, None]  # [B, 1, T, T]
    s = (qr @ kr.transpose(-2, -1)) / math.sqrt(D)
    s = s.masked_fill(~mask, float("-inf"))
    p = torch.softmax(s, dim=-1)
    if scale is not None:
        p = p * scale.to(dtype)
    out = p @ vr
    lse = torch.logsumexp(s.detach(), dim=-1)
    if dO is None:
        return out.detach(), lse, None, None, None
    out.backward(dO.to(dtype))
    return out.detach(), lse, qr.grad, kr.grad, vr.grad
