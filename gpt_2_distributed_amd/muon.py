"""Muon, stated once in plain torch: the rule the HIP kernels (csrc/muon.hip) are tested against.

Muon (Jordan et al., the nanoGPT speedrun optimizer) keeps momentum on every hidden weight matrix and replaces the
update by an approximately orthogonal matrix: five Newton-Schulz iterations of the quintic ``p(s) = a s + b s^3 + c s^5``
applied to the singular values of the normalised update. Everything that is not a hidden weight matrix (the tied
embedding / lm_head, the position table, LayerNorms, biases) stays on AdamW.

The functions here run on any device in any dtype; ``muon_tables`` builds the device tables of the kernels' batch.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

NS_COEFFS = (3.4445, -4.7750, 2.0315)
EPS = 1e-7


def newton_schulz_reference(X, steps: int = 5, coeffs=NS_COEFFS, dtype=torch.bfloat16):
    """X [m, n], m <= n. ``steps`` x { A = X X^T; B = b A + c A A; X = a X + B X }. dtype=bfloat16: A, B and X are
    rounded to bf16 after each line, the sums are fp32 (what the kernels compute, up to the order of the sums);
    dtype=float64 (or float32): nothing is rounded below that type."""
    assert X.dim() == 2 and X.shape[0] <= X.shape[1], "newton_schulz_reference takes the wide form"
    a, b, c = coeffs
    if dtype == torch.bfloat16:
        acc, rnd = torch.float32, (lambda t: t.to(torch.bfloat16).to(torch.float32))
    else:
        acc, rnd = dtype, (lambda t: t)
    X = rnd(X.to(acc))
    for _ in range(steps):
        A = rnd(X @ X.T)
        B = rnd(b * A + c * (A @ A))
        X = rnd(a * X + B @ X)
    return X.to(dtype)


def muon_x0(u):
    """The normalised update in wide form: u / (||u||_F + 1e-7), transposed if rows > cols."""
    x = u / (u.norm() + EPS)
    return x.T if u.shape[0] > u.shape[1] else x


def muon_reference(W, g, buf, lr, momentum=0.95, nesterov=True, ns_steps=5, weight_decay=0.0, dtype=torch.bfloat16):
    """One Muon step of one matrix; returns (W, buf) and changes neither argument. ``dtype`` is the Newton-Schulz
    precision (newton_schulz_reference); the elementwise arithmetic runs in W's dtype."""
    buf = momentum * buf + g
    u = g + momentum * buf if nesterov else buf
    rows, cols = W.shape
    O = newton_schulz_reference(muon_x0(u), ns_steps, dtype=dtype).to(W.dtype)
    if rows > cols:
        O = O.T
    return W * (1 - lr * weight_decay) - lr * max(1.0, rows / cols) ** 0.5 * O, buf


def muon_matrices(model) -> List[Tuple[str, int, int, int]]:
    """The ``(name, row_offset, rows, cols)`` list Muon owns: per block q, k and v (rows 0, C, 2C of attn.qkv.weight,
    C x C each), attn.proj.weight, mlp.fc1.weight (4C x C) and mlp.fc2.weight (C x 4C). Everything else is AdamW's."""
    out = []
    for name, sl in model.layout.slots.items():
        if ".h." not in name or len(sl.shape) != 2:
            continue
        rows, cols = sl.shape
        if name.endswith("attn.qkv.weight"):
            out += [(name, i * cols, cols, cols) for i in range(3)]
        elif name.endswith(("attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")):
            out.append((name, 0, rows, cols))
    return out


def muon_tables(mats: Sequence[Tuple[int, int, int, int]], device):
    """The kernels' batch (include/gpt2mi.h v24.8) for matrices given as (arena offset, rows, cols, ld): a dict with
    ``mats`` (int64 [count, 8]), the item tables ``tiles64`` (prepare / update), ``sym`` (gram / poly) and ``full``
    (apply) (int32 [n, 4]), and the element counts ``x_numel`` / ``a_numel`` / ``p_numel`` of the compact buffers.
    Every matrix's tiles are consecutive in each item table."""
    rows_, t64, sym, full = [], [], [], []
    xoff = aoff = pstart = 0
    for i, (off, rows, cols, ld) in enumerate(mats):
        if min(off, rows, cols) < 0 or rows % 64 or cols % 64 or ld % 64 or off % 64 or ld < cols or rows == 0 or cols == 0:
            raise ValueError(f"Muon matrix {i}: offset {off}, {rows} x {cols}, ld {ld}: the kernels take multiples of 64")
        m, n = min(rows, cols), max(rows, cols)
        ptiles = (rows // 64) * (cols // 64)
        rows_.append((off, rows, cols, ld, xoff, aoff, pstart, ptiles))
        t64 += [(i, r, c, 0) for r in range(rows // 64) for c in range(cols // 64)]
        tm, tn = (m + 127) // 128, (n + 127) // 128
        sym += [(i, r, c, 0) for r in range(tm) for c in range(r, tm)]
        full += [(i, r, c, 0) for r in range(tm) for c in range(tn)]
        xoff, aoff, pstart = xoff + m * n, aoff + m * m, pstart + ptiles
    if not rows_:
        raise ValueError("Muon: no matrices")
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(device)  # noqa: E731
    return dict(mats=torch.tensor(rows_, dtype=torch.int64).to(device), tiles64=i32(t64), sym=i32(sym), full=i32(full),
                x_numel=xoff, a_numel=aoff, p_numel=pstart, count=len(rows_))
