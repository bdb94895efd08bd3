"""Shared pieces of the per-document position tests (tests/test_docpos_*.py) — not a test module.

Positions by a Python loop over the documents, the document layouts of a row given as lengths over ``T_valid``, and
``docmask_helpers.gpt2_fp64`` with ``wpe[pos]`` in place of ``wpe[:T]``.
"""
from __future__ import annotations

import torch

from gpt_2_distributed_amd import packing
from tests.docmask_helpers import _gelu, _ln, attention_fp64, bounds_from_lengths


def loop_positions(bounds: packing.DocBounds) -> torch.Tensor:
    """pos[b, t] = offset of t in its document, by hopping through the documents of every row (start, end)."""
    B, T = bounds.start.shape
    pos = torch.full((B, T), -1, dtype=torch.int32)
    for b in range(B):
        t0 = 0
        while t0 < T:
            s, e = int(bounds.start[b, t0]), int(bounds.end[b, t0])
            assert s == t0 < e <= T
            for t in range(s, e):
                pos[b, t] = t - s
            t0 = e
    return pos


LAYOUT_NAMES = ("one", "ones", "head1", "tail1", "mixed")


def layout_lengths(name: str, T_valid: int, seed: int = 0):
    """Document lengths summing to T_valid: one document, all ones, [1, T_valid - 1], [T_valid - 1, 1], a seeded mix."""
    if name == "one" or T_valid == 1:
        return (T_valid,)
    if name == "ones":
        return (1,) * T_valid
    if name == "head1":
        return (1, T_valid - 1)
    if name == "tail1":
        return (T_valid - 1, 1)
    assert name == "mixed"
    g = torch.Generator().manual_seed(1000 + seed)
    lens, left = [], T_valid
    while left > 0:
        n = min(left, int(torch.randint(1, 8, (1,), generator=g)))
        lens.append(n)
        left -= n
    return tuple(lens)


def padded_bounds(rows, T: int) -> packing.DocBounds:
    """Bounds [B, T] of rows of document lengths over T_valid <= T; the padding is one document [T_valid, T)."""
    return packing.pad_bounds(bounds_from_lengths(rows), T)


def batch_layouts(B: int, T_valid: int, first: str):
    """The layouts of a batch: row b takes layout (first + b) of LAYOUT_NAMES, so rows differ in document count."""
    i0 = LAYOUT_NAMES.index(first)
    return [layout_lengths(LAYOUT_NAMES[(i0 + b) % len(LAYOUT_NAMES)], T_valid, seed=b) for b in range(B)]


def gpt2_fp64_pos(state_dict, cfg, idx, labels, mask, pos):
    """``docmask_helpers.gpt2_fp64`` with the position table indexed by ``pos`` int [B, T]: (loss or None, gradients or
    None, logits [B, T, V]) in fp64 with the attention mask ``mask`` bool [B, T, T] (dropout 0)."""
    P = {n: t.detach().double().cpu().clone().requires_grad_(labels is not None) for n, t in state_dict.items()
         if n != "lm_head.weight"}
    idx = idx.cpu()
    B, T = idx.shape
    x = P["transformer.wte.weight"][idx] + P["transformer.wpe.weight"][pos.long().cpu()]
    for l in range(cfg.n_layer):
        pre = f"transformer.h.{l}."
        h = _ln(x, P[pre + "ln1.weight"], P[pre + "ln1.bias"], cfg.layer_norm_eps)
        x = x + attention_fp64(h, P[pre + "attn.qkv.weight"], P[pre + "attn.qkv.bias"], P[pre + "attn.proj.weight"],
                               P[pre + "attn.proj.bias"], cfg.n_head, mask)
        h = _ln(x, P[pre + "ln2.weight"], P[pre + "ln2.bias"], cfg.layer_norm_eps)
        h = _gelu(h @ P[pre + "mlp.fc1.weight"].T + P[pre + "mlp.fc1.bias"])
        x = x + h @ P[pre + "mlp.fc2.weight"].T + P[pre + "mlp.fc2.bias"]
    x = _ln(x, P["transformer.ln_f.weight"], P["transformer.ln_f.bias"], cfg.layer_norm_eps)
    logits = x @ P["transformer.wte.weight"].T
    if labels is None:
        return None, None, logits.detach()
    loss = torch.nn.functional.cross_entropy(logits.view(B * T, -1), labels.cpu().view(-1), ignore_index=-100)
    loss.backward()
    return loss.detach(), {n: t.grad for n, t in P.items()}, logits.detach()
