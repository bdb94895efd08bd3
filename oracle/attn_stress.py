"""Stress inputs, a rounding model and a per-block metric for the attention kernels — TEST ORACLE.

Test infrastructure only (see ``oracle/__init__.py``); CPU, numpy / torch.

`randn` q/k/v at unit scale never move the running max of a flash-attention forward by more than a few
log2 units after the first key tile, so the deferred-max rescale of ``csrc/attention.hip`` (taken when a
row of a 16-query group grows by more than 8 log2 units) runs only against an empty accumulator. The
builders here overwrite channel 0 of q and k (score = randn part + q0 * k0 / 8, head_dim 64) to force
the paths a trained model reaches: rescales with old tiles still carrying weight, a rescale at every
tile, a rescale triggered by a single row, late keys that underflow, and future keys far above a row's
LSE. All overwrite values are multiples of 0.25 and stay within 8 significant bits, so bf16 holds them
exactly; each head gets its own pattern offset so that heads are not copies of one another.

``rescale_events`` restates the kernel's decision rule so that CPU tests can pin which inputs reach the
branch; ``bf16_model`` is the same operation with only the roundings a bf16 flash kernel cannot avoid
(the yardstick for tolerances, not a copy of the kernel's schedule); ``block_err`` is the relative error
per 32-row block, the unit of work of one wave, so that one wrong wave is not averaged away.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from oracle import dropout_ref, model_ref

D = 64
KINDS = ("step", "stairs", "spikes", "falling", "plain", "cliff")
LOG2E = 1.4426950408889634
RESCALE_THR = 8.0  # csrc/attention.hip kRescaleThr (log2 units)
SEED_LO = 5
SEED_HI = (0x9E3779B9 << 32) | 77  # non-zero high word: its own second-round multiplier (common.h seed_kx)


def _bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(torch.float32)


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def build(kind: str, B: int, T: int, H: int, seed: int = 0) -> torch.Tensor:
    """bf16 qkv [B*T, 3C] (C = 64 H) of one stress pattern. Channel 0 of q and k per head bh = b*H + h, with
    o = bh % 4 the head's pattern offset:

    step     q0 = 8; k0 = 0 for keys < T/2 + 16 o, 7 after; v of the early keys x 8
    stairs   q0 = 8; k0 = 6 (key // 64 - (T // 64 - 3)): the same level for every head, the last stair at 12. q0 is
             one constant, so a level offset changes no probability, but dq's channel 0 is sum dS k0 / 8 and a
             large |k0| there amplifies the bf16 rounding of dS past the well-conditioned limit of the CPU
             tests; the heads still differ in every randn channel
    spikes   q0 = 8 for one query in 32 (another lane and query group per wave), else 0;
             k0 = 6 (tile + 1) on one key per 64-key tile, else 0
    falling  q0 = 8; k0 = -6 (key // 64 + o)
    plain    none (randn)
    cliff    q0 = 8 + 2 o; k0 = 4 key (T <= 256): 4-7 nats per key, so the future keys of a diagonal tile lie
             hundreds of nats above the row's LSE and their exponentials overflow before they are masked
    """
    if kind not in KINDS:
        raise ValueError(f"unknown stress input {kind!r}")
    C = H * D
    g = torch.Generator().manual_seed(1000003 * KINDS.index(kind) + 7919 * T + 31 * B * H + seed)
    x = _bf(torch.randn(B, T, 3, H, D, generator=g))
    key = torch.arange(T)
    for b in range(B):
        for h in range(H):
            o = (b * H + h) % 4
            q0 = torch.full((T,), 8.0)
            if kind == "step":
                ks = T // 2 + 16 * o
                k0 = torch.where(key < ks, 0.0, 7.0)
                x[b, :ks, 2, h] *= 8.0
            elif kind == "stairs":
                k0 = 6.0 * (key // 64 - (T // 64 - 3))
            elif kind == "falling":
                k0 = -6.0 * (key // 64 + o)
            elif kind == "spikes":
                wv = key // 32
                spike_q = 32 * wv + 16 * ((wv + o) % 2) + (5 * wv + 3 * o) % 16
                q0 = torch.where(key == spike_q, 8.0, 0.0)
                t = key // 64
                spike_k = 64 * t + (7 * t + 11 * o) % 64
                k0 = torch.where(key == spike_k, 6.0 * (t + 1), 0.0)
            elif kind == "cliff":
                if T > 256:
                    raise ValueError("cliff: 4 * key needs T <= 256 to stay bf16-exact")
                q0 = torch.full((T,), 8.0 + 2.0 * o)
                k0 = 4.0 * key
            else:
                continue
            x[b, :, 0, h, 0] = q0
            x[b, :, 1, h, 0] = k0.to(torch.float32)
    out = x.to(torch.bfloat16)
    assert torch.equal(out.float(), x), "stress inputs must be bf16-exact"
    return out.reshape(B * T, 3 * C)


def split(qkv: torch.Tensor, B: int, T: int, H: int):
    """q, k, v [B, H, T, 64] views of qkv [B*T, 3C]."""
    return qkv.view(B, T, 3, H, D).transpose(1, 3).unbind(2)


def merge(x: torch.Tensor) -> torch.Tensor:
    """[B, H, T, 64] -> the kernels' head-merged [B*T, C]."""
    B, H, T, _ = x.shape
    return x.transpose(1, 2).reshape(B * T, H * D).contiguous()


def unmerge(y: torch.Tensor, B: int, T: int, H: int) -> torch.Tensor:
    """The kernels' [B*T, C] -> [B, H, T, 64]."""
    return y.view(B, T, H, D).transpose(1, 2)


def grad_out(B: int, T: int, H: int, seed: int = 1) -> torch.Tensor:
    """bf16-exact dO [B, H, T, 64] (fp32)."""
    g = torch.Generator().manual_seed(424243 + 7919 * T + 31 * B * H + seed)
    return _bf(torch.randn(B, H, T, D, generator=g))


def scores(q: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
    """Scaled, causally masked scores in fp64 (nats; future keys -inf), [..., T, T]."""
    T = q.shape[-2]
    s = q.double() @ k.double().transpose(-2, -1) / math.sqrt(D)
    return s.masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool)), float("-inf"))


def keep_mask(seed: int, bh: int, T: int, p: float, q=None) -> torch.Tensor:
    """The kept (query, key) pairs of ONE head as bool [T(q), T(key)] (or the rows `q`): head bh's slice of
    ``dropout_ref.attn_scale(...) != 0`` without forming the other heads."""
    qs = np.arange(T, dtype=np.uint64) if q is None else np.atleast_1d(np.asarray(q, dtype=np.uint64))
    qq = qs[:, None]
    kk = np.arange(T, dtype=np.uint64)[None, :]
    x = ((np.uint64(bh) * np.uint64(T) + (qq & ~np.uint64(16))) * np.uint64(T) + kk) & dropout_ref.M32
    keep = dropout_ref._keep(dropout_ref.drop_hash(seed, x), (qq >> np.uint64(4)) & np.uint64(1),
                             dropout_ref.threshold(p))
    return torch.from_numpy(keep)


# ---------------------------------------------------------------------------------------------
# the forward kernel's rescale decision
# ---------------------------------------------------------------------------------------------
def rescale_events(s: torch.Tensor):
    """The deferred-max decisions of ``attn_fwd_kernel`` on masked scores s [..., T, T] (nats, future = -inf):
    32-query waves as two 16-query groups, 64-key tiles; a group moves its running maxima m (log2 units) to
    max(m, tile max) when ANY of its 16 rows has tile max > m + 8. Returns (events, waves), each an int64
    tensor [...]: the rescales taken after key tile 0 (tile 0 always "rescales" an empty accumulator), and the
    number of waves with at least one of them."""
    T = s.shape[-1]
    lead = s.shape[:-2]
    tmax = (s.reshape(-1, T, T // 64, 64).max(-1).values * LOG2E).reshape(-1, T // 16, 16, T // 64)
    m = torch.full(tmax.shape[:-1], float("-inf"), dtype=s.dtype)
    events = torch.zeros(tmax.shape[0], T // 16, dtype=torch.int64)
    for j in range(T // 64):
        x = tmax[..., j]  # -inf where the tile is wholly in the row's future: never above m + 8
        trig = (x > m + RESCALE_THR).any(-1)
        m = torch.where(trig[..., None], torch.maximum(m, x), m)
        if j > 0:
            events += trig
    waves = (events.view(-1, T // 32, 2).sum(-1) > 0).sum(-1)
    return events.sum(-1).reshape(lead), waves.reshape(lead)


# ---------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------
def reference(q, k, v, dO, scale=None, dtype=torch.float64) -> dict:
    """model_ref.causal_attention and its autograd backward in `dtype` (fp64: the oracle; fp32: the yardstick of
    the fp32 kernels). scale: keep / (1 - p) multipliers [B, H, T, T] or None. Returns out, lse, dq, dk, dv."""
    qr, kr, vr = (t.to(dtype).clone().requires_grad_(True) for t in (q, k, v))
    out = model_ref.causal_attention(qr, kr, vr, "fp32", drop=None if scale is None else scale.to(dtype))
    out.backward(dO.to(dtype))
    lse = torch.logsumexp(scores(q, k).to(dtype), -1)
    return {"out": out.detach(), "lse": lse, "dq": qr.grad, "dk": kr.grad, "dv": vr.grad}


def bf16_model(q, k, v, dO, mask=None, p: float = 0.0) -> dict:
    """Causal attention forward and backward in fp32 with only the roundings a bf16 flash kernel cannot avoid:
    e = exp(s - rowmax) rounded to bf16 and the normaliser l the sum of the rounded e; out rounded to bf16;
    P = exp(s - lse) from that lse; delta = sum dO . out of the rounded out; under dropout dO / (1 - p) and
    V / (1 - p) rounded to bf16; dS and the kept P rounded to bf16; dq, dk, dv rounded to bf16.
    mask: kept pairs, bool [B, H, T, T], or None. Returns out, lse, dq, dk, dv (fp32)."""
    q, k, v, dO = (t.float() for t in (q, k, v, dO))
    T = q.shape[-2]
    sc = 1.0 / math.sqrt(D)
    ik = 1.0 / (1.0 - p) if p > 0 else 1.0
    keep = torch.ones(1, dtype=torch.float32) if mask is None else mask.float()
    s = (q @ k.transpose(-2, -1)) * sc
    s = s.masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool)), float("-inf"))
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
    dS_k = dS if p <= 0 else _bf(P * (keep * (dO @ Vs.transpose(-2, -1)) - delta))  # the dK pass scales V, not dO
    Pk = _bf(P * keep)
    return {"out": out, "lse": lse.squeeze(-1), "dq": _bf(dS @ k * sc), "dk": _bf(dS_k.transpose(-2, -1) @ q * sc),
            "dv": _bf(Pk.transpose(-2, -1) @ dO * ik)}


def block_err(x: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """Relative error per (b, h, 32-row block) of x [B, H, T, 64] against ref, in fp64:
    |x - ref| / max(|ref_blk|, 2^-10 max_blk |ref_blk|). The floor keeps blocks that the input drives to
    ~1e-40 (dk / dv of late keys that underflow) from dividing rounding noise by nothing."""
    B, H, T, d = ref.shape
    x, ref = x.double().reshape(B, H, T // 32, 32 * d), ref.double().reshape(B, H, T // 32, 32 * d)
    rn = ref.norm(dim=-1)
    return (x - ref).norm(dim=-1) / torch.clamp(rn, min=float(rn.max()) * 2.0 ** -10)


# ---------------------------------------------------------------------------------------------
# one cached case per (input, shape, dropout): the inputs, the fp64 oracle and the model's own error
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)  # a case keeps [B, H, T, 64] tensors only, no T x T one
def case(kind: str, B: int, T: int, H: int, p: float = 0.0, seed: int = SEED_LO, f32: bool = False) -> dict:
    """Inputs (qkv bf16 [B*T, 3C], dO [B, H, T, 64]), the fp64 oracle `ref` under the kernels' own dropout mask,
    and `model_err`: the worst block_err per tensor (and worst |lse - ref|) of the yardstick against the oracle —
    ``bf16_model``, or with f32 = True plain fp32 torch. Callers must not modify what they get."""
    if p > 0 and B * H * T * T > 3 * 1024 * 1024:
        raise ValueError("attention mask of more than 3 * 1024 * 1024 elements")
    qkv = build(kind, B, T, H)
    q, k, v = (t.float() for t in split(qkv, B, T, H))
    dO = grad_out(B, T, H)
    scale = dropout_ref.attn_scale(seed, B * H, T, p).view(B, H, T, T) if p > 0 else None
    ref = reference(q, k, v, dO, scale)
    if f32:
        model = reference(q, k, v, dO, scale, torch.float32)
    else:
        model = bf16_model(q, k, v, dO, None if scale is None else scale != 0, p)
    err = {n: float(block_err(model[n], ref[n]).max()) for n in ("out", "dq", "dk", "dv")}
    err["lse"] = float((model["lse"].double() - ref["lse"]).abs().max())
    return {"qkv": qkv, "dO": dO, "ref": ref, "model_err": err, "B": B, "T": T, "H": H, "p": p, "seed": seed}
