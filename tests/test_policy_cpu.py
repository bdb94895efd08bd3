"""The policy-gradient head without a device: the C entries' refusals, and the rule of policy.policy_reference against the
closed-form gradient the kernels implement (csrc/policy_loss.hip), in fp64."""
import pytest
import torch

from gpt_2_distributed_amd.policy import policy_reference
from tests.test_policy_kernels_gpu import CLIPS, SHAPES, policy_case

ENTRIES = ("gpt2mi_policy_fwd", "gpt2mi_policy_fwd_f32")
P = 8  # a non-NULL pointer no refused call dereferences


def call(lib, name, ld=136, ldd=136, labels=P, clip_low=0.2, clip_high=0.2, metrics=None, ratio=None):
    return getattr(lib, name)(P, ld, labels, P, None, None, clip_low, clip_high, 0.0, 0.0, P, None, ratio, None, None,
                              None, P, ldd, 9, 130, -100, P, P, metrics, None)


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("kw,words", [(dict(ld=132), b"multiples of 8"), (dict(ld=128), b"multiples of 8"),
                                      (dict(ldd=129), b"multiples of 8"), (dict(clip_low=-0.1), b"must be >= 0"),
                                      (dict(clip_high=float("nan")), b"must be >= 0"),
                                      (dict(labels=None), b"must not be NULL"),
                                      (dict(metrics=P, ratio=P), b"pass all four")])
def test_entries_refuse_before_any_launch(name, kw, words):
    from gpt_2_distributed_amd import _lib
    lib = _lib.load()
    assert call(lib, name, **kw) == 22
    msg = lib.gpt2mi_last_error()
    assert b"policy_fwd" in msg and words in msg, msg


@pytest.mark.parametrize("opts", [dict(), dict(clip_low=0.2, clip_high=0.28), dict(kl_coef=0.3),
                                  dict(entropy_coef=0.05), dict(clip_high=0.28, kl_coef=0.3, entropy_coef=0.05)])
def test_autograd_of_the_rule_is_the_closed_form(opts):
    """dloss/dlogits_v = (1/N) [c (p_v - [v = y]) + entropy_coef p_v (log p_v + H)] with
    c = (r A if the unclipped term is the minimum, else 0) - kl_coef (1 - exp(ref - logp))."""
    g = torch.Generator().manual_seed(3)
    M, V = 12, 37
    z = (3 * torch.randn(M, V, generator=g, dtype=torch.float64)).requires_grad_(True)
    y = torch.randint(0, V, (M,), generator=g)
    y[4] = -100
    adv = torch.randn(M, generator=g, dtype=torch.float64)
    logp = torch.log_softmax(z.detach(), -1).gather(1, y.clamp(0)[:, None])[:, 0]
    old = logp + torch.tensor([-0.5, -0.1, 0.0, 0.1, 0.5], dtype=torch.float64).repeat(3)[:M]
    ref = logp + 0.3 * torch.randn(M, generator=g, dtype=torch.float64)
    out = policy_reference(z, y, adv, old, ref, **opts)
    out.loss.backward()
    cl, ch = opts.get("clip_low", 0.2), opts.get("clip_high", 0.2)
    r = torch.exp(logp - old)
    u, v = r * adv, r.clamp(1 - cl, 1 + ch) * adv
    c = torch.where(u <= v, u, torch.zeros_like(u)) - opts.get("kl_coef", 0.0) * (1 - torch.exp(ref - logp))
    lp = torch.log_softmax(z.detach(), -1)
    p = lp.exp()
    H = -(p * lp).sum(-1, keepdim=True)
    onehot = torch.zeros_like(p).scatter_(1, y.clamp(0)[:, None], 1.0)
    want = c[:, None] * (p - onehot) + opts.get("entropy_coef", 0.0) * p * (lp + H)
    want[y == -100] = 0
    want /= (y != -100).sum()
    assert (r.clamp(1 - cl, 1 + ch) != r).any() and (v < u).any() and (u < v).any()  # both branches of the min occur
    torch.testing.assert_close(z.grad, want, rtol=1e-12, atol=1e-14)
    assert torch.equal(out.clipped, torch.where(y == -100, 0.0, (r.clamp(1 - cl, 1 + ch) != r).double()))
    torch.testing.assert_close(out.entropy, torch.where(y == -100, 0.0, H[:, 0].double()), rtol=1e-12, atol=0)


def test_kernel_cases_keep_their_ratios_off_the_clip_bounds():
    """The GPU test's inputs, on the reference alone: every ratio at least 0.08 from either bound (the kernel's fp32
    error in logp, below 1e-4, cannot flip a clip decision), and over the shapes both branches of the min occur among the
    clipped rows for each sign of the advantage."""
    seen = set()
    for k in range(len(SHAPES)):
        c = policy_case(k, "all")
        live = c["labels"] != -100
        r, adv = c["want"].ratio[live], c["adv"][live].double()
        lo, hi = 1 - CLIPS["clip_low"], 1 + CLIPS["clip_high"]
        assert float(torch.minimum((r - lo).abs(), (r - hi).abs()).min()) >= 0.08
        out = (r < lo) | (r > hi)
        assert torch.equal(out.double(), c["want"].clipped[live])
        active = r * adv <= r.clamp(lo, hi) * adv
        seen |= {(bool(a > 0), bool(t)) for a, t in zip(adv[out], active[out])}
    assert seen == {(True, True), (True, False), (False, True), (False, False)}
