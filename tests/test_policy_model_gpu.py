"""GPT2.policy_loss end to end on a tiny model (L2 H2 C128 V509, B = 3, T = 70: padded to the attention tile, some labels
ignored, dropout 0, every option on): the loss and every parameter gradient against the fp32 oracle's logits put through
policy.policy_reference and autograd. E = the largest relative error over the loss and the gradients. fp32: E <= 1e-4,
the goldens' figure. bf16: E_policy <= 2 E_xent, E_xent the same comparison for forward(idx, labels) on the same model
and tokens, measured here (the project's rule for a new path beside an existing one, as decode's E_dec <= 2 E_full).
The old log-probabilities put every ratio at least 0.08 from a clip bound (tests/test_policy_kernels_gpu.py), far more
than bf16 logits move it, so the model and the oracle take the same clip decisions."""
import dataclasses

import pytest
import torch

from gpt_2_distributed_amd.policy import policy_reference
from tests.test_model_gpu import TINY, prec_ctx, rel_err
from tests.test_policy_kernels_gpu import CLIPS, DELTAS

pytestmark = pytest.mark.gpu
dev = "cuda"
OPTS = dict(kl_coef=0.3, entropy_coef=0.05, **CLIPS)


def errors(m, loss, ref_loss, params):
    e = {n: rel_err(p.grad.cpu(), params[n].grad) for n, p in m.named_parameters()}
    e["loss"] = abs(loss.item() - ref_loss.item()) / abs(ref_loss.item())
    return e


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_policy_step_vs_oracle(prec):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_2_distributed_amd.model import GPT2, GPT2Config
    from oracle import model_ref
    cfg = GPT2Config(**dict(TINY, n_positions=128))
    rcfg = model_ref.Cfg(**dataclasses.asdict(cfg))
    m = GPT2(cfg).to(dev)
    B, T = 3, 70
    g = torch.Generator().manual_seed(21)
    idx = torch.randint(0, cfg.vocab_size, (B, T), generator=g)
    labels = torch.randint(0, cfg.vocab_size, (B, T), generator=g)
    labels[:, :9], labels[1, 40:] = -100, -100
    adv = torch.randn(B, T, generator=g) + 1.0  # both signs, mean 1: the loss is not a difference of near-equal sums

    def oracle():
        params = {n: p.detach().cpu().clone().requires_grad_(True) for n, p in m.named_parameters()}
        logits, ce = model_ref.forward(params, rcfg, idx, labels, "fp32")
        return params, logits, ce

    params, logits, _ = oracle()
    logp = torch.log_softmax(logits.detach(), -1).gather(2, labels.clamp(0)[..., None])[..., 0]
    old = logp + torch.tensor(DELTAS).repeat(B * T // 5).view(B, T)
    ref = logp + 0.3 * torch.randn(B, T, generator=g)
    want = policy_reference(logits, labels, adv, old, ref, **OPTS)
    want.loss.backward()
    eng = m.engine()
    seed0 = eng._step_seed
    with prec_ctx(prec):
        _, ce = m(idx.to(dev), labels=labels.to(dev))
    ce.backward()
    ce_params, _, ref_ce = oracle()
    ref_ce.backward()
    e_xent = errors(m, ce, ref_ce, ce_params)
    m.zero_grad()
    with prec_ctx(prec):
        out = m.policy_loss(idx.to(dev), labels.to(dev), adv.to(dev), old.to(dev), ref.to(dev), **OPTS)
    out.loss.backward()
    e_pol = errors(m, out.loss, want.loss, params)
    assert eng._step_seed == seed0 + 2, "a policy step must advance the dropout stream as a plain step does"
    assert out.logprobs.shape == (B, T) and out.logprobs.dtype == torch.float32 and not out.ratio.requires_grad
    assert torch.equal(out.clipped.cpu().double(), want.clipped), "a clip decision differs from the oracle's"
    assert bool((out.logprobs.cpu()[labels == -100] == 0).all())
    assert list(out.metrics) == ["ratio", "clip_fraction", "kl", "entropy"]
    assert all(v.shape == () and bool(torch.isfinite(v)) for v in out.metrics.values())
    E_pol, E_xent = max(e_pol.values()), max(e_xent.values())
    print(f"policy model [{prec}]: E_policy {E_pol:.3e} ({max(e_pol, key=e_pol.get)}), E_xent {E_xent:.3e} "
          f"({max(e_xent, key=e_xent.get)}); loss {e_pol['loss']:.3e} / {e_xent['loss']:.3e}")
    assert E_pol <= (2 * E_xent if prec == "bf16" else 1e-4), (E_pol, E_xent)
    # an optimizer step on the policy gradient, then a plain step: still finite
    opt = m.configure_optimizers()
    opt.step()
    opt.zero_grad()
    with prec_ctx(prec):
        _, ce = m(idx.to(dev), labels=labels.to(dev))
    ce.backward()
    assert bool(torch.isfinite(ce)) and all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
