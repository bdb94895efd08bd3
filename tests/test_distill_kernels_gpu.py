"""The distillation head (csrc/distill_loss.hip: gpt2mi_distill_fwd / _f32) against distill.distill_reference in fp64 with
autograd, on the logits as the kernel sees them (the padding [V, ld) of both inputs NaN-filled), at the smallest shapes
that reach each of its code paths, for both directions, tau = 1 and tau != 1 and the three coefficient mixes.

Bounds, the sibling heads' (tests/test_policy_kernels_gpu.py): ce and kd per row 1e-5 max(1, |ref|); dlogits by
rel_err < 4e-3 (bf16) / 1e-5 (fp32) over the counted rows; loss and metrics 1e-5 relative."""
import math

import pytest
import torch

from gpt_2_distributed_amd.distill import distill_reference
from tests.test_decode_kernels_gpu import BF16, bits
from tests.test_kernels_gpu import rel_err
from tests.test_row_kernels_gpu import SLACK, check_elements, sentinel, untouched

pytestmark = pytest.mark.gpu

dev = "cuda"
# (M, V, ld, ldd, dtype): one trip of the two-pass loop with V no multiple of 8, three trips, the register kernel, the
# register kernel with its seventh chunk nearly empty, fp32
SHAPES = [(9, 130, 136, 136, BF16), (5, 5000, 5008, 5120, BF16), (8, 50257, 50304, 50432, BF16),
          (3, 49160, 49160, 49160, BF16), (5, 5000, 5008, 5120, torch.float32)]
SHAPE_IDS = ["two-pass-130", "two-pass-5000", "row-kernel", "row-kernel-49160", "f32"]
COEFS = [(1.0, 0.0), (0.0, 1.0), (0.5, 0.5)]
_inputs, _wants = {}, {}


def inputs(k):
    """Student logits, teacher = student + 0.5 randn (KL well away from 0) and labels of shape k: CPU, never modified."""
    if k not in _inputs:
        M, V, ld, ldd, dtype = SHAPES[k]
        g = torch.Generator().manual_seed(M * 3 + V)
        s, t = torch.full((M, ld), math.nan), torch.full((M, ld), math.nan)
        s[:, :V] = torch.randn(M, V, generator=g) * 3
        t[:, :V] = s[:, :V] + 0.5 * torch.randn(M, V, generator=g)
        labels = torch.randint(0, V, (M,), generator=g)
        labels[0], labels[1], labels[2] = V - 1, 0, -100
        _inputs[k] = (s.to(dtype), t.to(dtype), labels)
    return _inputs[k]


def want(k, kind, tau, coefs):
    """The fp64 reference of a case and its unscaled dlogits, computed once."""
    key = (k, kind, tau, coefs)
    if key not in _wants:
        s, t, labels = inputs(k)
        V = SHAPES[k][1]
        z = s[:, :V].double().requires_grad_(True)
        w = distill_reference(z, labels, t[:, :V].double(), tau, *coefs, kind)
        w.loss.backward()
        _wants[key] = (w, z.grad * int((labels != -100).sum()))
    return _wants[key]


def run(K, k, kind, tau, coefs, labels=None, with_dlogits=True):
    M, V, ld, ldd, dtype = SHAPES[k]
    s, t, lab = inputs(k)
    rows = [sentinel(M + SLACK) for _ in range(3)]  # loss_rows, ce, kd
    dl = sentinel(M * ldd + SLACK, dtype) if with_dlogits else None
    scal = sentinel(4 + SLACK)  # loss, inv_count, metrics[2]
    K.distill_fwd(s.to(dev), ld, t.to(dev), ld, (lab if labels is None else labels).to(dev), tau, *coefs, kind, *rows,
                  dl, ldd, M, V, scal[0:], scal[1:], scal[2:])
    torch.cuda.synchronize()
    assert all(untouched(r[M:]) for r in rows) and untouched(scal[4:]), "wrote past M rows / the four scalars"
    assert dl is None or untouched(dl[M * ldd:]), "dlogits written past M*ldd"
    return [r[:M].cpu() for r in rows], None if dl is None else dl[:M * ldd].view(M, ldd).cpu(), scal[:4].cpu()


@pytest.mark.parametrize("coefs", COEFS, ids=["ce", "kd", "mix"])
@pytest.mark.parametrize("tau", [1.0, 2.0])
@pytest.mark.parametrize("kind", ["forward", "reverse"])
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=SHAPE_IDS)
def test_distill_head_against_fp64(k, kind, tau, coefs):
    from gpt_2_distributed_amd import _lib as K
    M, V, ld, ldd, dtype = SHAPES[k]
    labels = inputs(k)[2]
    w, d64 = want(k, kind, tau, coefs)
    rows, dl, scal = run(K, k, kind, tau, coefs)
    loss_rows, ce, kd = rows
    bound = lambda ref: 1e-5 * ref.abs().clamp_min(1.0)
    worst = {"ce": check_elements("ce", ce, w.ce, bound(w.ce)), "kd": check_elements("kd", kd, w.kd, bound(w.kd))}
    live = labels != -100
    n = int(live.sum())
    for name, got, ref in zip(("loss", "inv_count", "ce", "kd"), scal.tolist(),
                              (float(w.loss.detach()), 1.0 / n, float(w.ce[live].mean()), float(w.kd[live].mean()))):
        assert abs(got - ref) <= 1e-5 * abs(ref), (name, got, ref)
    err = rel_err(dl[live][:, :V], d64[live])
    print(f"distill {SHAPE_IDS[k]} {kind} tau {tau} coefs {coefs}: err/bound "
          + " ".join(f"{a} {b:.3f}" for a, b in worst.items()) + f"; dlogits rel_err {err:.3e}")
    assert err < (1e-5 if dtype == torch.float32 else 4e-3), err
    assert not bool(torch.isnan(dl).any()), "NaN in dlogits"
    assert bool((bits(dl[:, V:]) == 0).all()), "dlogits columns [V, ldd) are not +0"
    assert bool((bits(dl[~live]) == 0).all()) and all(bool((bits(r[~live]) == 0).all()) for r in rows), \
        "an ignored row is not +0"
    # the same call again, and without dlogits: equal bits
    rows2, dl2, scal2 = run(K, k, kind, tau, coefs)
    rows3, none, scal3 = run(K, k, kind, tau, coefs, with_dlogits=False)
    assert none is None and torch.equal(bits(dl2), bits(dl))
    for a, b, d in zip(rows + [scal], rows2 + [scal2], rows3 + [scal3]):
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(d))


@pytest.mark.parametrize("kind, tau", [("forward", 1.0), ("reverse", 2.0)])
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=SHAPE_IDS)
def test_label_outside_the_vocabulary_poisons_its_row_only(k, kind, tau):
    from gpt_2_distributed_amd import _lib as K
    M, V, ld, ldd, dtype = SHAPES[k]
    labels = inputs(k)[2].clone()
    labels[M - 2], labels[M - 1] = V, max(V, ld - 1)  # in the row's allocation: a kernel that reads them reads its NaNs
    rows, dl, scal = run(K, k, kind, tau, COEFS[2], labels=labels)
    good_rows, good_dl, _ = run(K, k, kind, tau, COEFS[2])
    bad = torch.zeros(M, dtype=torch.bool)
    bad[M - 2:] = True
    assert bool(torch.isnan(dl[bad][:, :V]).all()) and all(bool(torch.isnan(r[bad]).all()) for r in rows)
    n = int((labels != -100).sum())
    assert bool(torch.isnan(scal[[0, 2, 3]]).all()) and abs(float(scal[1]) - 1.0 / n) <= 1e-6
    assert torch.equal(bits(dl[~bad]), bits(good_dl[~bad])) and bool((bits(dl[:, V:]) == 0).all())
    assert all(torch.equal(bits(r[~bad]), bits(q[~bad])) for r, q in zip(rows, good_rows))
