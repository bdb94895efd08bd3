"""The policy-gradient head (csrc/policy_loss.hip: gpt2mi_policy_fwd / _f32) against policy.policy_reference in fp64
with autograd, on the logits as the kernel sees them, at the smallest shapes that reach each of its code paths (the cross
entropy's cases of tests/test_row_kernels_gpu.py) under every option set.

Bounds: logp, kl and entropy per row by the cross entropy's figure for lse, 1e-5 max(1, |ref|); the ratio by 1e-5
relative; the clipped flag equal; dlogits by rel_err < 4e-3 (bf16) / 1e-5 (fp32), the cross entropy's numbers; loss and
metrics 1e-5 relative. old = logp64 + delta with delta cycling through DELTAS puts every ratio at least 0.08 from either
clip bound (tests/test_policy_cpu.py checks that, and that the cases cover both branches of the min for each sign of the
advantage, on the reference alone), so the kernel's fp32 error in logp (< 1e-4) cannot flip a decision."""
import math

import pytest
import torch

from gpt_2_distributed_amd.policy import policy_reference
from tests.test_decode_kernels_gpu import BF16, bits
from tests.test_kernels_gpu import rel_err
from tests.test_row_kernels_gpu import SLACK, check_elements, sentinel, untouched

pytestmark = pytest.mark.gpu

dev = "cuda"
# (M, V, ld, ldd, dtype): one trip of the two-pass loop, three trips, the register-resident row kernel, fp32
SHAPES = [(9, 130, 136, 136, BF16), (5, 5000, 5008, 5120, BF16), (8, 50257, 50304, 50432, BF16),
          (5, 5000, 5008, 5120, torch.float32)]
SHAPE_IDS = ["two-pass-130", "two-pass-5000", "row-kernel", "f32"]
CLIPS = dict(clip_low=0.2, clip_high=0.28)
OPTIONS = {"neutral": dict(), "clip": dict(old=True, **CLIPS), "kl": dict(ref=True, kl_coef=0.3),
           "entropy": dict(entropy_coef=0.05),
           "all": dict(old=True, ref=True, kl_coef=0.3, entropy_coef=0.05, **CLIPS)}
DELTAS = (-0.5, -0.1, 0.0, 0.1, 0.5)  # r = 1.65, 1.105, 1, 0.905, 0.607
_cases = {}


def policy_case(k, option):
    """Inputs of shape k under an option set and their fp64 reference, computed once (CPU tensors, never modified)."""
    if (k, option) in _cases:
        return _cases[k, option]
    M, V, ld, ldd, dtype = SHAPES[k]
    o = dict(OPTIONS[option])
    g = torch.Generator().manual_seed(M * 3 + V)
    logits = torch.full((M, ld), math.nan)  # the padding [V, ld) poisons a kernel that reads it as logits
    logits[:, :V] = torch.randn(M, V, generator=g) * 3
    logits = logits.to(dtype)
    labels = torch.randint(0, V, (M,), generator=g)
    labels[0], labels[1], labels[2] = V - 1, 0, -100
    z = logits[:, :V].double().requires_grad_(True)
    logp = torch.log_softmax(z.detach(), -1).gather(1, labels.clamp(0)[:, None])[:, 0]
    sign = torch.tensor([1.0 if (i + k) % 2 == 0 else -1.0 for i in range(M)])
    adv = torch.ones(M) if option == "neutral" else sign * (0.5 + torch.rand(M, generator=g))
    old = (logp + torch.tensor([DELTAS[i % 5] for i in range(M)])).float() if o.pop("old", False) else None
    ref = (logp + 0.3 * torch.randn(M, generator=g)).float() if o.pop("ref", False) else None
    want = policy_reference(z, labels, adv, old, ref, **o)
    want.loss.backward()
    n = int((labels != -100).sum())
    c = dict(logits=logits, labels=labels, adv=adv, old=old, ref=ref, opts=o, want=want, d64=z.grad * n, n=n)
    _cases[k, option] = c
    return c


def run(K, k, c, labels=None, with_dlogits=True):
    M, V, ld, ldd, dtype = SHAPES[k]
    rows = [sentinel(M + SLACK) for _ in range(6)]  # loss_rows, logp, ratio, kl, entropy, clipped
    dl = sentinel(M * ldd + SLACK, dtype) if with_dlogits else None
    scal = sentinel(6 + SLACK)  # loss, inv_count, metrics[4]
    o = c["opts"]
    to = lambda t: None if t is None else t.to(dev)
    K.policy_fwd(c["logits"].to(dev), ld, (c["labels"] if labels is None else labels).to(dev), to(c["adv"]),
                 to(c["old"]), to(c["ref"]), o.get("clip_low", 0.2), o.get("clip_high", 0.2), o.get("kl_coef", 0.0),
                 o.get("entropy_coef", 0.0), *rows, dl, ldd, M, V, scal[0:], scal[1:], scal[2:])
    torch.cuda.synchronize()
    assert all(untouched(r[M:]) for r in rows) and untouched(scal[6:]), "wrote past M rows / the six scalars"
    assert dl is None or untouched(dl[M * ldd:]), "dlogits written past M*ldd"
    return [r[:M].cpu() for r in rows], None if dl is None else dl[:M * ldd].view(M, ldd).cpu(), scal[:6].cpu()


@pytest.mark.parametrize("option", list(OPTIONS))
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=SHAPE_IDS)
def test_policy_head_against_fp64(k, option):
    from gpt_2_distributed_amd import _lib as K
    M, V, ld, ldd, dtype = SHAPES[k]
    c = policy_case(k, option)
    w, labels, n = c["want"], c["labels"], c["n"]
    rows, dl, scal = run(K, k, c)
    loss_rows, logp, ratio, kl, ent, clipped = rows
    bound = lambda ref: 1e-5 * ref.abs().clamp_min(1.0)
    worst = {"logp": check_elements("logp", logp, w.logp, bound(w.logp)),
             "kl": check_elements("kl", kl, w.kl, bound(w.kl)),
             "entropy": check_elements("entropy", ent, w.entropy, bound(w.entropy)),
             "ratio": check_elements("ratio", ratio, w.ratio, 1e-5 * w.ratio.abs())}
    assert torch.equal(clipped.double(), w.clipped), (clipped, w.clipped)
    live = labels != -100
    means = [float(t[live].mean()) for t in (w.ratio, w.clipped, w.kl, w.entropy)]
    for name, got, ref in zip(("loss", "inv_count", "ratio", "clip_fraction", "kl", "entropy"), scal.tolist(),
                              [float(w.loss.detach()), 1.0 / n] + means):
        assert abs(got - ref) <= 1e-5 * abs(ref), (name, got, ref)
    err = rel_err(dl[live][:, :V], c["d64"][live])
    print(f"policy {SHAPE_IDS[k]} {option}: err/bound " + " ".join(f"{a} {b:.3f}" for a, b in worst.items())
          + f"; dlogits rel_err {err:.3e}")
    assert err < (1e-5 if dtype == torch.float32 else 4e-3), err
    assert not bool(torch.isnan(dl).any()), "NaN in dlogits"
    assert bool((bits(dl[:, V:]) == 0).all()), "dlogits columns [V, ldd) are not +0"
    assert bool((bits(dl[~live]) == 0).all()) and all(bool((bits(r[~live]) == 0).all()) for r in rows), \
        "an ignored row is not +0"
    # the same call again, and without dlogits: equal bits
    rows2, dl2, scal2 = run(K, k, c)
    rows3, none, scal3 = run(K, k, c, with_dlogits=False)
    assert none is None and torch.equal(bits(dl2), bits(dl))
    for a, b, d in zip(rows + [scal], rows2 + [scal2], rows3 + [scal3]):
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(d))


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=SHAPE_IDS)
def test_label_outside_the_vocabulary_poisons_its_row_only(k):
    from gpt_2_distributed_amd import _lib as K
    M, V, ld, ldd, dtype = SHAPES[k]
    c = policy_case(k, "all")
    labels = c["labels"].clone()
    labels[3], labels[4] = V, ld - 1  # inside the row's allocation: a kernel that reads them reads its own NaN padding
    rows, dl, scal = run(K, k, c, labels=labels)
    good_rows, good_dl, _ = run(K, k, c)
    bad = torch.zeros(M, dtype=torch.bool)
    bad[3:5] = True
    assert bool(torch.isnan(dl[bad][:, :V]).all()) and all(bool(torch.isnan(r[bad]).all()) for r in rows)
    assert bool(torch.isnan(scal[[0, 2, 3, 4, 5]]).all()) and abs(float(scal[1]) - 1.0 / c["n"]) <= 1e-6
    assert torch.equal(bits(dl[~bad]), bits(good_dl[~bad])) and bool((bits(dl[:, V:]) == 0).all())
    assert all(torch.equal(bits(r[~bad]), bits(q[~bad])) for r, q in zip(rows, good_rows))
