"""GPT2.distill_loss end to end on a tiny model (L2 H2 C128 V509, B = 2, T = 70: padded to the attention tile, some
labels ignored, dropout 0), the teacher's logits from a second tiny model's forward: the loss and every parameter gradient
against distill.distill_reference applied to the student's own returned logits with torch autograd, which reaches the
parameters through the same backward. E = the largest relative error over the loss and the gradients. The bounds are
those of tests/test_policy_model_gpu.py: fp32 E <= 1e-4; bf16 E <= 2 E_xent, E_xent the same comparison for
forward(idx, labels) against F.cross_entropy on the returned logits, measured here on the same model and tokens."""
import pytest
import torch
import torch.nn.functional as F

from gpt_2_distributed_amd.distill import distill_reference
from tests.test_model_gpu import TINY, prec_ctx, rel_err

pytestmark = pytest.mark.gpu
dev = "cuda"
B, T = 2, 70
PRECISIONS = pytest.mark.parametrize("prec", ["bf16", "fp32"])


def setup():
    """(student, idx, labels, a teacher whose weights are the student's moved by N(0, 0.05^2))."""
    from gpt_2_distributed_amd.model import GPT2, GPT2Config
    cfg = GPT2Config(**dict(TINY, n_positions=128))
    student, teacher = GPT2(cfg).to(dev), GPT2(cfg).to(dev)
    g = torch.Generator().manual_seed(23)
    with torch.no_grad():
        teacher.arena.add_(0.05 * torch.randn(teacher.arena.shape, generator=g).to(dev))
    teacher.engine().refresh_shadow()
    idx = torch.randint(0, cfg.vocab_size, (B, T), generator=g).to(dev)
    labels = torch.randint(0, cfg.vocab_size, (B, T), generator=g)
    labels[:, :9], labels[1, 40:] = -100, -100
    return student, idx, labels.to(dev), teacher


def step(m, loss_fn, prec):
    """One forward + backward; (loss, gradients) on the CPU."""
    m.zero_grad()
    with prec_ctx(prec):
        loss = loss_fn()
    loss.backward()
    return loss.detach().cpu().double(), {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}


def worst(got, ref):
    e = {n: rel_err(got[1][n], ref[1][n]) for n in ref[1]}
    e["loss"] = abs(float(got[0]) - float(ref[0])) / abs(float(ref[0]))
    return max(e.values()), max(e, key=e.get)


def xent_error(m, idx, labels, prec):
    fused = step(m, lambda: m(idx, labels=labels)[1], prec)
    via = step(m, lambda: F.cross_entropy(m(idx)[0].double().view(B * T, -1), labels.view(-1)), prec)
    return worst(fused, via)[0], fused


@PRECISIONS
@pytest.mark.parametrize("kind, tau, coefs", [("forward", 2.0, (0.5, 0.5)), ("reverse", 1.0, (0.0, 1.0)),
                                              ("forward", 1.0, (1.0, 0.0))])
def test_distill_step_vs_reference_on_the_returned_logits(prec, kind, tau, coefs):
    m, idx, labels, teacher = setup()
    with torch.no_grad(), prec_ctx(prec):
        t_logits = teacher(idx)[0]
    seed0 = m.engine()._step_seed
    got = step(m, lambda: m.distill_loss(idx, labels, t_logits, tau, *coefs, kind).loss, prec)
    assert m.engine()._step_seed == seed0 + 1, "a distillation step must advance the dropout stream as a plain step does"
    ref = step(m, lambda: distill_reference(m(idx)[0].double(), labels, t_logits.double(), tau, *coefs, kind).loss, prec)
    E_xent, fused = xent_error(m, idx, labels, prec)
    E, where = worst(got, ref)
    print(f"distill model [{prec} {kind} tau {tau} {coefs}]: E {E:.3e} ({where}), E_xent {E_xent:.3e}")
    bound = 2 * E_xent if prec == "bf16" else 1e-4
    assert E <= bound, (E, where, E_xent)
    if coefs == (1.0, 0.0):  # the cross entropy alone: forward(idx, labels) itself
        assert worst(got, fused)[0] <= bound, (worst(got, fused), E_xent)
    with prec_ctx(prec):
        out = m.distill_loss(idx, labels, t_logits, tau, *coefs, kind)
    live = labels != -100
    assert out.ce.shape == (B, T) and out.kd.dtype == torch.float32 and not out.ce.requires_grad
    assert bool((out.ce[~live] == 0).all()) and bool((out.kd[~live] == 0).all()) and bool((out.kd[live] > 0).all())
    assert list(out.metrics) == ["ce", "kd"]
    torch.testing.assert_close(out.metrics["kd"], out.kd[live].mean(), rtol=1e-5, atol=0)


@PRECISIONS
def test_distill_between_training_steps_and_deterministic(prec):
    def run():
        m, idx, labels, teacher = setup()
        m.precision, m.deterministic = prec, True
        with torch.no_grad():
            t_logits = teacher(idx)[0].float()  # fp32 whatever the student computes in: cast once under bf16
        opt = m.configure_optimizers(learning_rate=1e-3)
        losses = []
        for distill in (False, True, False):
            opt.zero_grad()
            loss = m.distill_loss(idx, labels, t_logits, 2.0, kind="reverse").loss if distill else m(idx, labels=labels)[1]
            loss.backward()
            opt.step()
            losses.append(loss.detach().clone())
        return losses + [p.detach().clone() for p in m.parameters()]
    a, b = run(), run()
    assert all(bool(torch.isfinite(x).all()) for x in a)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_bad_arguments_and_the_ddp_wrapper(tmp_path):
    import torch.distributed as dist
    from gpt_2_distributed_amd.parallel import DistributedDataParallel
    m, idx, labels, teacher = setup()
    with torch.no_grad():
        t_logits = teacher(idx)[0]
    for bad in (dict(teacher_logits=t_logits[:, :-1]), dict(teacher_logits=t_logits[..., :-1]), dict(temperature=0.0),
                dict(kind="jsd")):
        with pytest.raises(ValueError):
            m.distill_loss(**dict(dict(idx=idx, labels=labels, teacher_logits=t_logits), **bad))
    plain = step(m, lambda: m.distill_loss(idx, labels, t_logits).loss, "fp32")
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        ddp = DistributedDataParallel(m)
        wrapped = step(m, lambda: ddp.distill_loss(idx, labels, t_logits).loss, "fp32")
    finally:
        dist.destroy_process_group()
        m.engine().grad_sync = None
    assert worst(wrapped, plain)[0] <= 1e-6
