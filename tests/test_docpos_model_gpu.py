"""Positions per document through the public surface on the MI355X: GPT2.forward / score / evaluate, the backbone and
the DDP wrapper with ``doc_bounds`` and ``reset_positions=True`` on the tiny model of tests/test_docmask_model_gpu.py
(L2 H2 C128 V509), against a small fp64 torch GPT-2 with the boolean mask and ``wpe[pos]``
(docpos_helpers.gpt2_fp64_pos). Gates are the project's: fp32 loss and gradients 1e-4 relative, bf16 loss 2e-2.

The property the option exists for: a document inside a packed row gives the logits it gives alone in a row."""
import json
import os
import subprocess
import sys

import pytest
import torch

from gpt_2_distributed_amd import packing as P
from tests import docmask_helpers as H
from tests import docpos_helpers as D
from tests.conftest import REPO
from tests.test_docmask_model_gpu import TINY, bf16, make_model, rel_err

pytestmark = pytest.mark.gpu
dev = "cuda"
B, T = 2, 150  # the engine pads to 192: the padding document is in play
ROWS = [(70, 80), (1, 64, 85)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def batch(seed=41, Bn=B, Tn=T):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(4, 509, (Bn, Tn + 1), generator=g)
    return t[:, :-1].contiguous(), t[:, 1:].contiguous()


def on_dev(bounds):
    return P.DocBounds(bounds.start.to(dev), bounds.end.to(dev))


@pytest.fixture(scope="module")
def reference():
    """The fp64 loss and gradients of the sharp model under the document mask with restarting positions, once; the
    fp64 loss with absolute positions differs by far more than the fp32 gate."""
    cpu = make_model(device="cpu")
    x, y = batch()
    bounds = H.bounds_from_lengths(ROWS)
    mask = P.doc_mask(bounds)
    loss, grads, _ = D.gpt2_fp64_pos(cpu.state_dict(), cpu.config, x, y, mask, P.doc_positions(bounds))
    absolute, _ = H.gpt2_fp64(cpu.state_dict(), cpu.config, x, y, mask)
    print(f"fp64 loss with positions per document {float(loss):.9f}, absolute {float(absolute):.9f}")
    assert abs(float(loss) - float(absolute)) > 1e-3 * float(absolute)
    return x, y, bounds, float(loss), grads


def test_fp32_loss_and_gradients_against_the_fp64_model(reference):
    x, y, bounds, loss64, grads = reference
    m = make_model()
    m.precision = "fp32"
    _, loss = m(x.to(dev), labels=y.to(dev), doc_bounds=on_dev(bounds), reset_positions=True)
    loss.backward()
    rel = abs(loss.item() - loss64) / loss64
    print(f"fp32 loss {loss.item():.7f} fp64 {loss64:.7f} rel {rel:.2e}")
    assert rel < 1e-4
    for n, p in m.named_parameters():
        e = rel_err(p.grad.cpu(), grads[n])
        print(f"  {n}: {e:.2e}")
        assert e < 1e-4, (n, e)
    # rows of wpe from the longest document's length on receive no gradient at all
    assert not bool(m.transformer.wpe.weight.grad[85:].any())


def test_bf16_loss_within_the_bf16_gate(reference):
    x, y, bounds, loss64, _ = reference
    m = make_model()
    with bf16():
        _, loss = m(x.to(dev), labels=y.to(dev), doc_bounds=on_dev(bounds), reset_positions=True)
    loss.backward()
    rel = abs(loss.item() - loss64) / loss64
    print(f"bf16 loss {loss.item():.6f} fp64 {loss64:.6f} rel {rel:.2e}")
    assert rel < 2e-2
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def test_a_packed_document_gives_the_logits_it_gives_alone():
    """Rows [docA | docB] of 70 + 58 tokens: with the restart, docB's 58 logit rows are the fp64 model's on docB alone
    as a 58-token row, within the fp32 gate; with the keyword off (absolute positions) they miss it by far."""
    na, nb = 70, 58
    x, _ = batch(seed=43, Tn=na + nb)
    cpu = make_model(device="cpu")
    alone = H.single_document(B, nb)
    _, _, want = D.gpt2_fp64_pos(cpu.state_dict(), cpu.config, x[:, na:], None, P.doc_mask(alone), P.doc_positions(alone))
    m = make_model().eval()
    m.precision = "fp32"
    doc = on_dev(H.bounds_from_lengths([(na, nb)] * B))
    with torch.no_grad():
        on = m(x.to(dev), doc_bounds=doc, reset_positions=True)[0][:, na:].cpu()
        off = m(x.to(dev), doc_bounds=doc)[0][:, na:].cpu()
    e_on, e_off = rel_err(on, want), rel_err(off, want)
    print(f"docB logits against docB alone: with the restart {e_on:.2e}, without {e_off:.2e}")
    assert e_on < 1e-4
    assert e_off > 1e-2  # a hundred times the gate: absolute positions are another input


def test_score_and_evaluate_with_the_restart(reference):
    """score(reduction="none", reset_positions=True) rows against the per-token losses of forward under the same bounds
    and flag, within 2^-8 max|logit| (the bound of test_score_and_evaluate_under_the_mask); evaluate(eot_token_id=,
    reset_positions=True) is the token-weighted mean of the scores; the restart moves the score."""
    EOT = 3
    m = make_model()
    tok = []
    for seed, seps in ((51, ((69,), (0, 64))), (52, ((30, 99), (120,)))):
        x, y = batch(seed)
        full = torch.cat([x, y[:, -1:]], dim=1)
        for b, s in enumerate(seps):
            full[b, list(s)] = EOT
        tok.append((full[:, :-1].contiguous().to(dev), full[:, 1:].contiguous().to(dev)))
    (xd, yd), (x2, y2) = tok
    y2 = y2.clone()
    y2[0, :40] = -100
    doc, doc2 = P.doc_bounds(xd, EOT), P.doc_bounds(x2, EOT)
    m.eval()
    with bf16(), torch.no_grad():
        logits, loss = m(xd, labels=yd, doc_bounds=doc, reset_positions=True)
    per_token = torch.nn.functional.cross_entropy(logits.float().view(B * T, -1), yd.view(-1), reduction="none")
    m.train()
    with bf16():
        rows = m.score(xd, yd, reduction="none", doc_bounds=doc, reset_positions=True)
        mean = m.score(xd, yd, doc_bounds=doc, reset_positions=True)
        absolute = m.score(xd, yd, doc_bounds=doc)
        sums = [m.score(a, b, reduction="sum", doc_bounds=d, reset_positions=True).double().item()
                for a, b, d in ((xd, yd, doc), (x2, y2, doc2))]
        r = m.evaluate(iter([(xd, yd), (x2, y2)]), eot_token_id=EOT, reset_positions=True)
        r_abs = m.evaluate(iter([(xd, yd), (x2, y2)]), eot_token_id=EOT)
    bound = 2.0 ** -8 * logits.float().abs().max().item()
    worst = float((rows.view(-1) - per_token).abs().max())
    print(f"score rows against forward's per-token losses: worst {worst:.3e} bound {bound:.3e}; mean {mean.item():.6f} "
          f"forward {loss.item():.6f} absolute positions {absolute.item():.6f}")
    assert rows.shape == (B, T) and worst <= bound
    assert abs(mean.item() - loss.item()) <= bound
    assert mean.item() != absolute.item()
    counts = [B * T, int((y2 != -100).sum())]
    want = sum(sums) / sum(counts)
    assert r["tokens"] == sum(counts)
    assert abs(r["loss"] - want) <= 3 * torch.finfo(torch.float32).eps * want
    assert r["loss"] != r_abs["loss"]


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_one_document_per_row_is_the_call_without_bounds(prec):
    """The positions are the same integers: bitwise the logits of doc_bounds alone, which are bitwise those of the call
    without bounds (test_one_document_per_row_gives_the_same_logits_bit_for_bit), so the fp32 gate holds trivially."""
    x, _ = batch()
    m = make_model(sharp=False).eval()
    if prec == "fp32":
        m.precision = "fp32"
    doc = on_dev(H.single_document(B, T))
    with (bf16() if prec == "bf16" else torch.no_grad()), torch.no_grad():
        plain = m(x.to(dev))[0]
        masked = m(x.to(dev), doc_bounds=doc)[0]
        reset = m(x.to(dev), doc_bounds=doc, reset_positions=True)[0]
        feats = m.transformer(x.to(dev), doc_bounds=doc)
        feats_reset = m.transformer(x.to(dev), doc_bounds=doc, reset_positions=True)
    assert rel_err(reset.float(), plain.float()) < 1e-4
    assert torch.equal(reset, masked) and torch.equal(feats, feats_reset)


def test_a_step_with_the_keyword_off_is_untouched_by_one_with_it_on(reference):
    """Two fresh models run the same keyword-off training step (forward, backward, AdamW), one of them having first run
    and discarded a keyword-on forward / backward. fp32, dropout 0. Bit for bit: the loss, and the gradient and the
    stepped weight of every tensor whose gradient is formed in a fixed order (wpe, whose sum is what this option
    touches, and the GEMM weights of the blocks). Two runs of a training step are not bit-reproducible in the
    gradients that LayerNorm, the bias column sums and the wte scatter add with fp32 atomics (engine.score's docstring),
    without this option as with it, and AdamW's first step turns a last-bit change of a gradient near zero into a
    sign. Those gradients are held to 2e-4 relative: each run is within the project's fp32 gate, 1e-4, of the same fp64
    gradient (test_fp32_loss_and_gradients_against_the_fp64_model), so two runs are within twice that of each other."""
    x, y, bounds, _, _ = reference
    xd, yd, doc = x.to(dev), y.to(dev), on_dev(bounds)

    def step(first_on):
        m = make_model()
        m.precision = "fp32"
        opt = m.configure_optimizers()
        if first_on:
            _, l0 = m(xd, labels=yd, doc_bounds=doc, reset_positions=True)
            l0.backward()
            opt.zero_grad(set_to_none=True)
        _, loss = m(xd, labels=yd, doc_bounds=doc)
        loss.backward()
        grads = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}
        opt.step()
        torch.cuda.synchronize()
        return loss.detach().cpu(), grads, {n: p.detach().cpu().clone() for n, p in m.named_parameters()}

    la, ga, wa = step(False)
    lb, gb, wb = step(True)
    assert torch.equal(la, lb)
    fixed = [n for n in ga if n == "transformer.wpe.weight" or (".h." in n and ga[n].dim() == 2)]
    assert len(fixed) == 1 + 4 * TINY["n_layer"]
    print("gradients that differ in some bit:", [n for n in ga if not torch.equal(ga[n], gb[n])])
    for n in ga:
        if n in fixed:
            assert torch.equal(ga[n], gb[n]) and torch.equal(wa[n], wb[n]), n
        else:
            assert rel_err(gb[n], ga[n]) < 2e-4, n


DDP = r"""
import os, sys, json, torch, torch.distributed as dist
sys.path.insert(0, os.environ["REPO"])
from gpt_2_distributed_amd.parallel import init_distributed, DistributedDataParallel
from gpt_2_distributed_amd.model import GPT2, GPT2Config
from gpt_2_distributed_amd import packing
init_distributed()  # a world of one rank, collectives forced on
cfg = GPT2Config(**json.loads(os.environ["CFG"]))
t = torch.load(os.environ["BATCH"])
x, y = t["x"].cuda(), t["y"].cuda()
doc = packing.DocBounds(t["start"].cuda(), t["end"].cuda())
res = {}
for name, wrap in (("plain", lambda m: m), ("ddp", DistributedDataParallel)):
    model = wrap(GPT2(cfg).to("cuda:0"))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with torch.no_grad():
            _, absolute = model(x, labels=y, doc_bounds=doc)
        _, loss = model(x, labels=y, doc_bounds=doc, reset_positions=True)
    loss.backward()
    res[name] = {"loss": loss.item(), "absolute": absolute.item()}
print("RESULT", json.dumps(res), flush=True)
dist.barrier(); dist.destroy_process_group()
"""


def test_ddp_wrapper_forwards_the_keyword(tmp_path):
    """DistributedDataParallel(model)(x, labels=y, doc_bounds=..., reset_positions=True) at world size 1 over RCCL: the
    loss of the unwrapped model, and not the one with absolute positions."""
    x, y = batch()
    bounds = H.bounds_from_lengths(ROWS)
    torch.save({"x": x, "y": y, "start": bounds.start, "end": bounds.end}, tmp_path / "batch.pt")
    script = tmp_path / "ddp.py"
    script.write_text(DDP)
    env = dict(os.environ, REPO=REPO, CFG=json.dumps(TINY), BATCH=str(tmp_path / "batch.pt"),
               GPT2MI_FORCE_COLLECTIVES="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29588", RANK="0", WORLD_SIZE="1",
               LOCAL_RANK="0")
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT")][0][7:])
    assert res["ddp"]["loss"] == res["plain"]["loss"], res
    assert res["ddp"]["loss"] != res["ddp"]["absolute"], res
