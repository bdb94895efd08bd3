"""Shared pieces of the document-masking tests (tests/test_docmask_*.py) — not a test module.

The three document layouts of a T = 320 row, bounds built from document lengths, ``oracle.attn_stress.bf16_model``
restated with the document mask (the yardstick of the bf16 tolerances), one cached case per (layout, dropout, family)
with the fp64 reference and the yardstick's own error, and a small fp64 torch GPT-2 forward with a boolean attention
mask built from a model's ``state_dict``.
"""
from __future__ import annotations

import functools
import math

import torch

from gpt_2_distributed_amd import packing
from oracle import attn_stress as A
from oracle import dropout_ref

D = 64
T_LAYOUT = 320
# lengths of the documents of a T = 320 row; row 1 of a batch uses the layout reversed
LAYOUTS = {
    # a length-1 document; boundaries on a 16-query group (16), a 32-query wave (32) and a 64-key tile (64); a boundary
    # one key before a 128-query block (127); a document that starts on tile 3 (192): the last block skips tiles 0-2
    "L1": (1, 15, 16, 32, 63, 65, 128),
    # wave 64..95 holds queries of the documents starting at 32 and at 80: a whole 16-query group sees no key in tile 0
    "L2": (32, 48, 48, 64, 1, 127),
    # a boundary at 88 inside a 16-query group: single lanes of a group see no key in a visited tile
    "L3": (40, 48, 104, 128),
}


EOT = 7  # the separator of the hand-made token rows


def bounds_rows(T=16):
    """Rows of T tokens (no token is EOT unless placed): no separator, one at 0, one at T - 1, consecutive separators,
    all separators, and a mixed row."""
    base = torch.arange(100, 100 + T)
    rows = [base.clone() for _ in range(6)]
    rows[1][0] = EOT
    rows[2][T - 1] = EOT
    rows[3][4:7] = EOT
    rows[4][:] = EOT
    rows[5][[2, 3, 9, T - 1]] = EOT
    return torch.stack(rows)


def bounds_from_lengths(rows) -> packing.DocBounds:
    """DocBounds (CPU) of rows given as lists of document lengths, every row summing to the same T."""
    T = sum(rows[0])
    start = torch.empty(len(rows), T, dtype=torch.int32)
    end = torch.empty(len(rows), T, dtype=torch.int32)
    for b, lens in enumerate(rows):
        assert sum(lens) == T and min(lens) >= 1
        s = 0
        for n in lens:
            start[b, s:s + n] = s
            end[b, s:s + n] = s + n
            s += n
    return packing.DocBounds(start, end)


def layout_bounds(name: str, B: int = 2) -> packing.DocBounds:
    lens = LAYOUTS[name]
    return bounds_from_lengths([lens if b % 2 == 0 else lens[::-1] for b in range(B)])


def random_lengths(T: int, mean: int, seed: int):
    """Seeded random document lengths (geometric, mean about ``mean``) summing to T."""
    g = torch.Generator().manual_seed(seed)
    lens, left = [], T
    while left > 0:
        n = int(torch.empty(1).exponential_(1.0 / mean, generator=g).item()) + 1
        n = min(n, left)
        lens.append(n)
        left -= n
    return tuple(lens)


def single_document(B: int, T: int) -> packing.DocBounds:
    return packing.DocBounds(torch.zeros(B, T, dtype=torch.int32), torch.full((B, T), T, dtype=torch.int32))


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def doc_bf16_model(q, k, v, dO, bounds, mask=None, p: float = 0.0) -> dict:
    """``attn_stress.bf16_model`` with the document mask in place of the causal one: fp32 with only the roundings a
    bf16 flash kernel cannot avoid (see there). mask: kept pairs, bool [B, H, T, T], or None."""
    q, k, v, dO = (t.float() for t in (q, k, v, dO))
    sc = 1.0 / math.sqrt(D)
    ik = 1.0 / (1.0 - p) if p > 0 else 1.0
    keep = torch.ones(1, dtype=torch.float32) if mask is None else mask.float()
    s = (q @ k.transpose(-2, -1)) * sc
    s = s.masked_fill(~packing.doc_mask(bounds)[:, None], float("-inf"))
    mx = s.max(-1, keepdim=True).values
    e = _bf(torch.exp(s - mx))
    l = e.sum(-1, keepdim=True)
    lse = mx + torch.log(l)
    out = _bf((e * keep) @ v * (ik / l))
    P = torch.exp(s - lse)
    delta = (dO * out).sum(-1, keepdim=True)
    dOs = _bf(dO * ik) if p > 0 else dO
    Vs = _bf(v * ik) if p > 0 else v
    dS = _bf(P * (keep * (dOs @ v.transpose(-2, -1)) - delta))
    dS_k = dS if p <= 0 else _bf(P * (keep * (dO @ Vs.transpose(-2, -1)) - delta))
    Pk = _bf(P * keep)
    return {"out": out, "lse": lse.squeeze(-1), "dq": _bf(dS @ k * sc), "dk": _bf(dS_k.transpose(-2, -1) @ q * sc),
            "dv": _bf(Pk.transpose(-2, -1) @ dO * ik)}


def overflow_qkv(qkv: torch.Tensor, bounds: packing.DocBounds, B: int, T: int, H: int) -> torch.Tensor:
    """qkv with channel 0 set so that every query of a row's SECOND document scores 200 * 4 / 8 = 100 nats against
    every even key of its FIRST (k0 = 200 there, -200 on the odd keys, which score -100; q0 = 4 here), while scores
    inside a document keep their size: the first document's queries get q0 = 0 and the second's keys k0 = 0. All
    values are bf16-exact. The signs alternate so that channel 0 of the first document's dq, k0 / 8 times a sum of dS,
    is a well-conditioned number: with one sign it is 25 times the row sum of dS, which is 0, i.e. pure rounding
    residue, and the bf16 yardstick's own dq error is then 0.1.
    The large factor sits on the keys: in row 1 of L2 the second document is a single token, the one place where the
    dK/dV kernel visits such pairs (queries 96..127 against the wave's keys 96..127), and that token's dS is exactly 0
    (one key: P = 1, dP = delta), so its dk is the rounding residue of dP - delta times q / 8. A large q0 there would
    amplify a residue that plain fp32 autograd, which forms dS = P (dP - sum P dP) = 0 exactly, does not have; a large
    k0 on the first document amplifies only the row sums of dS, which every yardstick here carries too."""
    x = qkv.float().view(B, T, 3, H, D).clone()
    for b in range(B):
        e0 = int(bounds.end[b, 0])
        e1 = int(bounds.end[b, e0])
        x[b, :e0, 1, :, 0] = 200.0
        x[b, 1:e0:2, 1, :, 0] = -200.0
        x[b, :e0, 0, :, 0] = 0.0
        x[b, e0:e1, 0, :, 0] = 4.0
        x[b, e0:e1, 1, :, 0] = 0.0
    out = x.to(torch.bfloat16)
    assert torch.equal(out.float(), x)
    return out.reshape(B * T, 3 * H * D)


@functools.lru_cache(maxsize=None)
def case(layout: str, p: float = 0.0, f32: bool = False, overflow: bool = False) -> dict:
    """One attention case (callers must not modify it): layout "L1" / "L2" / "L3" (B = 2, T = 320, H = 3) or "random"
    (B = 1, T = 1024, H = 3, seeded lengths of mean about 100). qkv bf16 [B*T, 3C], dO [B, H, T, 64], bounds (CPU), the
    fp64 reference under the kernels' own dropout mask, and ``model_err``: the worst 32-row block error per tensor (and
    worst |lse - ref|) of the yardstick against the reference — ``doc_bf16_model``, or with f32 plain fp32 torch."""
    H = 3
    if layout == "random":
        B, T = 1, 1024
        bounds = bounds_from_lengths([random_lengths(T, 100, seed=11)])
    else:
        B, T = 2, T_LAYOUT
        bounds = layout_bounds(layout, B)
    seed = A.SEED_HI if p > 0 else A.SEED_LO
    qkv = A.build("plain", B, T, H)
    if overflow:
        qkv = overflow_qkv(qkv, bounds, B, T, H)
    q, k, v = (t.float() for t in A.split(qkv, B, T, H))
    dO = A.grad_out(B, T, H)
    scale = dropout_ref.attn_scale(seed, B * H, T, p).view(B, H, T, T) if p > 0 else None
    names = ("out", "lse", "dq", "dk", "dv")
    ref = dict(zip(names, packing.doc_attention_reference(q, k, v, bounds, dO, scale)))
    if f32:
        model = dict(zip(names, packing.doc_attention_reference(q, k, v, bounds, dO, scale, dtype=torch.float32)))
    else:
        model = doc_bf16_model(q, k, v, dO, bounds, None if scale is None else scale != 0, p)
    err = {n: float(A.block_err(model[n], ref[n]).max()) for n in ("out", "dq", "dk", "dv")}
    err["lse"] = float((model["lse"].double() - ref["lse"]).abs().max())
    return {"qkv": qkv, "dO": dO, "bounds": bounds, "ref": ref, "model_err": err, "B": B, "T": T, "H": H, "p": p,
            "seed": seed}


# ---------------------------------------------------------------------------------------------------------------------
# a small fp64 GPT-2 with a boolean attention mask, from a model's state_dict (model.py's module tree)
# ---------------------------------------------------------------------------------------------------------------------
def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _gelu(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def attention_fp64(x, qkv_w, qkv_b, proj_w, proj_b, n_head, mask):
    """CausalMultiHeadSelfAttention.forward in the dtype of x with the visible pairs ``mask`` bool [B, T, T]."""
    B, T, C = x.shape
    hd = C // n_head
    q, k, v = (x @ qkv_w.T + qkv_b).view(B, T, 3, n_head, hd).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) / math.sqrt(hd)
    s = s.masked_fill(~mask[:, None], float("-inf"))
    y = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, T, C)
    return y @ proj_w.T + proj_b


def gpt2_fp64(state_dict, cfg, idx, labels, mask):
    """(loss, {parameter name: gradient}) of GPT2.forward(idx, labels) in fp64 with the attention mask ``mask`` bool
    [B, T, T] (dropout 0). The lm_head is tied to wte, whose gradient holds both contributions."""
    P = {n: t.detach().double().cpu().clone().requires_grad_(True) for n, t in state_dict.items()
         if n != "lm_head.weight"}
    idx, labels = idx.cpu(), labels.cpu()
    B, T = idx.shape
    x = P["transformer.wte.weight"][idx] + P["transformer.wpe.weight"][:T]
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
    loss = torch.nn.functional.cross_entropy(logits.view(B * T, -1), labels.view(-1), ignore_index=-100)
    loss.backward()
    return loss.detach(), {n: t.grad for n, t in P.items()}
