"""The distillation head without a device: the C entries' refusals, and the rule of distill.distill_reference in fp64
against an independent formula (F.kl_div + F.cross_entropy) and against the closed-form gradient the kernels implement
(csrc/distill_loss.hip)."""
import pytest
import torch
import torch.nn.functional as F

from gpt_2_distributed_amd.distill import distill_reference

P = 8  # a non-NULL pointer no refused call dereferences


def call(lib, name, ld=136, ldt=136, ldd=136, teacher=P, tau=1.0, ce_coef=0.5, reverse=0, metrics=None, ce=None):
    return getattr(lib, name)(P, ld, teacher, ldt, P, tau, ce_coef, 0.5, reverse, P, ce, None, P, ldd, 9, 130, -100, P,
                              P, metrics, None)


@pytest.mark.parametrize("name", ["gpt2mi_distill_fwd", "gpt2mi_distill_fwd_f32"])
@pytest.mark.parametrize("kw,words", [(dict(ld=132), b"multiples of 8"), (dict(ldt=128), b"multiples of 8"),
                                      (dict(ldd=129), b"multiples of 8"), (dict(tau=0.0), b"finite and > 0"),
                                      (dict(tau=float("inf")), b"finite and > 0"),
                                      (dict(ce_coef=float("nan")), b"must be finite"),
                                      (dict(teacher=None), b"must not be NULL"), (dict(reverse=2), b"must be 0"),
                                      (dict(metrics=P, ce=P), b"pass both")])
def test_entries_refuse_before_any_launch(name, kw, words):
    from gpt_2_distributed_amd import _lib
    lib = _lib.load()
    assert call(lib, name, **kw) == 22
    msg = lib.gpt2mi_last_error()
    assert b"distill_fwd" in msg and words in msg, msg


@pytest.mark.parametrize("coefs", [(1.0, 0.0), (0.0, 1.0), (0.3, 0.7)])
@pytest.mark.parametrize("tau", [1.0, 2.0, 0.7])
@pytest.mark.parametrize("kind", ["forward", "reverse"])
def test_rule_against_kl_div_and_the_closed_form(kind, tau, coefs):
    g = torch.Generator().manual_seed(3)
    M, V = 12, 37
    z = (3 * torch.randn(M, V, generator=g, dtype=torch.float64)).requires_grad_(True)
    t = z.detach() + 0.5 * torch.randn(M, V, generator=g, dtype=torch.float64)
    y = torch.randint(0, V, (M,), generator=g)
    y[4], y[9] = -100, -100
    keep = y != -100
    out = distill_reference(z, y, t, tau, *coefs, kind)
    out.loss.backward()
    # the independent formula, on the counted rows only
    zs, ts = z.detach()[keep] / tau, t[keep] / tau
    a, b = (zs, ts) if kind == "forward" else (ts, zs)  # kl_div(log softmax(a), softmax(b)) = KL(b || a)
    kd = tau * tau * F.kl_div(torch.log_softmax(a, -1), torch.softmax(b, -1), reduction="none").sum(-1)
    ce = F.cross_entropy(z.detach()[keep], y[keep], reduction="none")
    n = int(keep.sum())
    assert n == M - 2
    torch.testing.assert_close(out.loss.detach(), (coefs[0] * ce + coefs[1] * kd).sum() / n, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(out.ce[keep], ce, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(out.kd[keep], kd, rtol=1e-11, atol=1e-14)
    assert bool((out.ce[~keep] == 0).all()) and bool((out.kd[~keep] == 0).all())
    # the closed form of the header
    p, lpt, lq = torch.softmax(z.detach(), -1), torch.log_softmax(z.detach() / tau, -1), torch.log_softmax(t / tau, -1)
    onehot = torch.zeros_like(p).scatter_(1, y.clamp(0)[:, None], 1.0)
    if kind == "forward":
        dkd = tau * (lpt.exp() - lq.exp())
    else:
        kl = (lpt.exp() * (lpt - lq)).sum(-1, keepdim=True)
        dkd = tau * lpt.exp() * (lpt - lq - kl)
    want = (coefs[0] * (p - onehot) + coefs[1] * dkd) / n
    want[~keep] = 0
    torch.testing.assert_close(z.grad, want, rtol=1e-11, atol=1e-14)


def test_reference_refuses_bad_arguments():
    z, y = torch.zeros(2, 5), torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError, match="kind"):
        distill_reference(z, y, z, kind="jsd")
    with pytest.raises(ValueError, match="temperature"):
        distill_reference(z, y, z, temperature=0.0)
