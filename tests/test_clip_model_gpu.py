"""configure_optimizers(max_grad_norm=...) on the model: the reference's clipped, cosine-scheduled trajectory
(tests/golden/tiny_clip_traj.json: torch clip_grad_norm_(1.0) + AdamW on the reference model), the unchanged default
path, agreement with torch's own clip + AdamW on our parameters, and the optimizer state dict."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN

from gpt_2_distributed_amd.lr_schedule import lr_at

pytestmark = pytest.mark.gpu
dev = "cuda"

# trajectory loss and grad-norm gates of tests/test_model_gpu.py; final parameters as tests/test_ddp_gpu.py
TOL = {"bf16": (2e-2, 5e-2), "fp32": (1e-4, 1e-3)}
REF = json.load(open(os.path.join(GOLDEN, "tiny_clip_traj.json")))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _tiny_model():
    from gpt_2_distributed_amd.model import GPT2, GPT2Config
    return GPT2(GPT2Config(**REF["config"])).to(dev)


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_clipped_cosine_trajectory_vs_reference_golden(prec):
    t_loss, t_norm = TOL[prec]
    m = _tiny_model()
    opt = m.configure_optimizers(weight_decay=0.1, learning_rate=REF["lr"], betas=(0.9, 0.95),
                                 max_grad_norm=REF["max_grad_norm"])
    toks, GA = torch.tensor(REF["tokens"], dtype=torch.int64), REF["grad_accum"]
    losses, norms, lrs, coefs = [], [], [], []
    for s in range(REF["steps"]):
        for a in range(GA):
            t = toks[s * GA + a].to(dev)
            with torch.autocast("cuda", dtype=torch.bfloat16) if prec == "bf16" else contextlib.nullcontext():
                _, loss = m(t[:, :-1], labels=t[:, 1:])
                loss = loss / GA
            loss.backward()
        opt.param_groups[0]["lr"] = lr_at(s, **REF["schedule"])
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        opt.zero_grad()
        losses.append(loss.item() * GA)
        norms.append(opt.grad_norm.item())
        coefs.append(opt.clip_coef.item())
    rl = np.abs(np.array(losses) - np.array(REF["losses"])) / np.array(REF["losses"])
    rn = np.abs(np.array(norms) - np.array(REF["grad_norms"])) / np.array(REF["grad_norms"])
    print(prec, "loss rel err", rl.max(), "norm rel err", rn.max())
    assert rl.max() < t_loss, rl
    assert rn.max() < t_norm, rn  # the norm before clipping
    np.testing.assert_allclose(lrs, REF["lrs"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(coefs, [min(1.0, REF["max_grad_norm"] / (n + 1e-6)) for n in REF["grad_norms"]],
                               rtol=t_norm)
    if prec == "fp32":
        tot, tot_ref = 0.0, 0.0
        for n, p in m.named_parameters():
            g = REF["params"][n]
            d = p.detach().double().cpu()
            ss = float((d * d).sum())
            tot, tot_ref = tot + ss, tot_ref + g["sumsq"]
            assert abs(ss - g["sumsq"]) <= 1e-4 * g["sumsq"] + 1e-12, n
            np.testing.assert_allclose(d.reshape(-1)[:16].numpy(), g["head"], rtol=1e-4, atol=1e-2 * REF["lr"],
                                       err_msg=n)
        assert abs(tot - tot_ref) <= 1e-2 * tot_ref


def _fwd_bwd(m, t):
    _, loss = m(t[:, :-1], labels=t[:, 1:])
    loss.backward()
    return loss


@pytest.mark.parametrize("off", [None, float("inf")])
def test_max_grad_norm_off_is_the_default_path_bitwise(off):
    """max_grad_norm=None / inf: fed the same gradient arena, parameters, moments, shadow and reported norm are the
    bits configure_optimizers() without the keyword gives. (One model's gradients are copied into the other's: the
    embedding backward's float atomics make two backward passes differ in the last bits.)"""
    toks = torch.tensor(REF["tokens"], dtype=torch.int64)
    a, b = _tiny_model(), _tiny_model()
    with torch.no_grad():
        b.arena.copy_(a.arena)
    b.engine().refresh_shadow()
    oa = a.configure_optimizers(learning_rate=1e-3)
    ob = b.configure_optimizers(learning_rate=1e-3, max_grad_norm=off)
    assert ob.param_groups[0]["max_grad_norm"] == off and oa.param_groups[0]["max_grad_norm"] is None
    for s in range(2):
        t = toks[s].to(dev)
        _fwd_bwd(a, t)
        _fwd_bwd(b, t)
        b.engine().grad.copy_(a.engine().grad)
        oa.step()
        ob.step()
        oa.zero_grad()
        ob.zero_grad()
        torch.cuda.synchronize()
        assert torch.equal(a.arena, b.arena) and torch.equal(a.engine().shadow, b.engine().shadow), s
        assert torch.equal(oa.exp_avg, ob.exp_avg) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq), s
        assert torch.equal(oa.grad_norm, ob.grad_norm) and ob.clip_coef.item() == 1.0, s
    assert oa.grad_norm.item() > 1.0  # a finite max_grad_norm of 1 would have clipped here


def test_fused_clipping_agrees_with_torch_clip_and_adamw():
    """A twin stepping with torch's clip_grad_norm_(params, 1.0) + torch.optim.AdamW on our parameters agrees with the
    fused clipped optimizer over 3 steps (the bounds of test_torch_optimizer_and_clip_grad_norm_interop)."""
    g = np.load(os.path.join(GOLDEN, "tiny_fwd_bwd.npz"))
    idx = torch.from_numpy(g["idx"]).to(dev)
    labels = torch.from_numpy(g["labels"]).to(dev)
    a, b = _tiny_model(), _tiny_model()
    oa = torch.optim.AdamW(a.parameters(), lr=1e-3, weight_decay=0.1, betas=(0.9, 0.95))
    ob = b.configure_optimizers(learning_rate=1e-3, max_grad_norm=1.0)
    clipped = 0
    for _ in range(3):
        _, la = a(idx, labels=labels)
        la.backward()
        na = torch.nn.utils.clip_grad_norm_(a.parameters(), 1.0)
        oa.step()
        oa.zero_grad()
        _, lb = b(idx, labels=labels)
        lb.backward()
        ob.step()
        ob.zero_grad()
        assert abs(na.item() - ob.grad_norm.item()) < 2e-3 * na.item()
        want = min(1.0, 1.0 / (na.item() + 1e-6))
        assert abs(ob.clip_coef.item() - want) < 2e-3 * want
        clipped += want < 1.0
        assert abs(la.item() - lb.item()) < 1e-4 * la.item()
    assert clipped >= 2
    assert rel_err(a.arena.cpu(), b.arena.cpu()) < 2e-3


def test_state_dict_round_trip_keeps_max_grad_norm():
    m = _tiny_model()
    opt = m.configure_optimizers(learning_rate=1e-3, max_grad_norm=1.0)
    sd = opt.state_dict()
    assert sd["param_groups"][0]["max_grad_norm"] == 1.0
    fresh = m.configure_optimizers(learning_rate=1e-3)
    fresh.load_state_dict(sd)
    assert fresh.param_groups[0]["max_grad_norm"] == 1.0 and fresh._max_norm() == 1.0
    # a state dict from before the keyword existed: loads, and the constructor's value stays
    old = dict(sd, param_groups=[{k: v for k, v in sd["param_groups"][0].items() if k != "max_grad_norm"}])
    kept = m.configure_optimizers(learning_rate=1e-3, max_grad_norm=0.5)
    kept.load_state_dict(old)
    assert kept.param_groups[0]["max_grad_norm"] == 0.5
    with pytest.raises(ValueError):
        m.configure_optimizers(max_grad_norm=-1.0)
