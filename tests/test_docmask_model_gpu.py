"""Document masking through the public surface on the MI355X: GPT2.forward / score / evaluate, the backbone, block and
attention modules and the DDP wrapper with ``doc_bounds``, on the tiny model (L2 H2 C128 V509) at B = 2, T = 150 (the
engine pads to 192, so the padding document is in play) with separators placed to give three documents per row.

The reference is a small fp64 torch GPT-2 with the boolean mask (docmask_helpers.gpt2_fp64) built from the model's own
state_dict. Gates are the project's: fp32 loss 1e-4 and gradients 1e-4 relative (tests/test_model_gpu.py TOL["fp32"]),
bf16 loss 2e-2."""
import contextlib
import json
import os
import subprocess
import sys

import pytest
import torch

from gpt_2_distributed_amd import packing as P
from tests import docmask_helpers as H
from tests.conftest import REPO

pytestmark = pytest.mark.gpu
dev = "cuda"

TINY = dict(n_layer=2, n_head=2, n_embd=128, vocab_size=509, n_positions=256, resid_pdrop=0.0, attn_pdrop=0.0)
B, T, EOT = 2, 150, 3
SEPS = ((40, 99), (63, 64))  # eot="end": documents [0, 41) [41, 100) [100, 150) and [0, 64) [64, 65) [65, 150)
bf16 = lambda: torch.autocast("cuda", dtype=torch.bfloat16)  # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def make_model(sharp=True, device=dev):
    """The seed-42 init; sharp: with the attention weights (qkv, proj) of every block scaled by 16, so that the
    softmax is far from uniform and the mask matters (the fp64 loss moves by 1.4e-3 relative between the document and
    the causal mask, 14 times the fp32 gate; at the plain init it moves by 1.4e-5)."""
    from gpt_2_distributed_amd.model import GPT2, GPT2Config
    m = GPT2(GPT2Config(**TINY))
    if sharp:
        with torch.no_grad():
            for blk in m.transformer.h:
                blk.attn.qkv.weight.mul_(16.0)
                blk.attn.proj.weight.mul_(16.0)
    return m.to(device)


def batch(seed=31):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(4, 509, (B, T + 1), generator=g)  # no accidental separator
    for b, seps in enumerate(SEPS):
        t[b, list(seps)] = EOT
    return t[:, :-1].contiguous(), t[:, 1:].contiguous()


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def reference():
    """The fp64 loss and gradients of the sharp model on the batch under the document mask, computed once."""
    cpu = make_model(device="cpu")
    cfg = cpu.config
    x, y = batch()
    bounds = P.doc_bounds_reference(x, EOT)
    assert [len(r.unique()) for r in bounds.start] == [3, 3]
    loss, grads = H.gpt2_fp64(cpu.state_dict(), cfg, x, y, P.doc_mask(bounds))
    causal, _ = H.gpt2_fp64(cpu.state_dict(), cfg, x, y, P.doc_mask(H.single_document(B, T)))
    print(f"fp64 loss under the document mask {float(loss):.9f}, under the causal mask {float(causal):.9f}")
    assert abs(float(loss) - float(causal)) > 1e-3 * float(causal)  # the fp32 gate tells the two masks apart
    return x, y, bounds, float(loss), grads


def test_fp32_loss_and_gradients_against_the_fp64_model(reference):
    x, y, bounds, loss64, grads = reference
    m = make_model()
    m.precision = "fp32"
    doc = P.doc_bounds(x.to(dev), EOT)
    assert torch.equal(doc.start.cpu(), bounds.start) and torch.equal(doc.end.cpu(), bounds.end)
    _, loss = m(x.to(dev), labels=y.to(dev), doc_bounds=doc)
    loss.backward()
    rel = abs(loss.item() - loss64) / loss64
    print(f"fp32 masked loss {loss.item():.7f} fp64 {loss64:.7f} rel {rel:.2e}")
    assert rel < 1e-4
    for n, p in m.named_parameters():
        e = rel_err(p.grad.cpu(), grads[n])
        assert e < 1e-4, (n, e)


def test_bf16_loss_within_the_bf16_gate(reference):
    x, y, _, loss64, _ = reference
    m = make_model()
    with bf16():
        _, loss = m(x.to(dev), labels=y.to(dev), doc_bounds=P.doc_bounds(x.to(dev), EOT))
    loss.backward()
    rel = abs(loss.item() - loss64) / loss64
    print(f"bf16 masked loss {loss.item():.6f} fp64 {loss64:.6f} rel {rel:.2e}")
    assert rel < 2e-2
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def test_packed_equals_separate_at_the_attention_module(reference):
    """The attention module has no positional term, so a document's rows of attn(x, doc_bounds) must be what the
    unmasked module gives for that document alone. E_packed: rel_err of the packed rows against an fp64 torch
    computation of the module; E_sep: the same for each document run alone. E_packed <= 2 E_sep, the form of the
    decode parity test."""
    x, _, bounds, _, _ = reference
    m = make_model()
    attn = m.transformer.h[0].attn
    g = torch.Generator().manual_seed(9)
    h = torch.randn(B, T, TINY["n_embd"], generator=g)
    sd = {n: t.detach().double().cpu() for n, t in attn.state_dict().items()}
    want = H.attention_fp64(h.double(), sd["qkv.weight"], sd["qkv.bias"], sd["proj.weight"], sd["proj.bias"],
                            TINY["n_head"], P.doc_mask(bounds))
    doc = P.DocBounds(bounds.start.to(dev), bounds.end.to(dev))
    with bf16(), torch.no_grad():
        packed = attn(h.to(dev), doc_bounds=doc).float().cpu()
        alone = torch.zeros_like(packed)
        for b in range(B):
            for s in bounds.start[b].unique().tolist():
                e = int(bounds.end[b, s])
                alone[b, s:e] = attn(h[b:b + 1, s:e].to(dev)).float().cpu()[0]
    e_packed, e_sep = rel_err(packed, want), rel_err(alone, want)
    print(f"attention module: E_packed {e_packed:.3e} E_sep {e_sep:.3e}")
    assert e_packed <= 2 * e_sep


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_one_document_per_row_gives_the_same_logits_bit_for_bit(prec):
    x, _ = batch()
    m = make_model(sharp=False).eval()
    one = H.single_document(B, T)
    doc = P.DocBounds(one.start.to(dev), one.end.to(dev))
    with (bf16() if prec == "bf16" else contextlib.nullcontext()), torch.no_grad():
        plain = m(x.to(dev))[0]
        masked = m(x.to(dev), doc_bounds=doc)[0]
        feats = m.transformer(x.to(dev))
        feats_doc = m.transformer(x.to(dev), doc_bounds=doc)
    assert torch.equal(plain, masked) and torch.equal(feats, feats_doc)


def test_score_and_evaluate_under_the_mask(reference):
    """score(mean, doc_bounds) against forward(idx, labels, doc_bounds)[1] in eval mode within 2^-8 max|logit|, the
    per-token bound tests/test_eval_gpu.py holds that relation to without bounds; evaluate(eot_token_id=) is the
    token-weighted mean of the masked scores; the mask moves the score."""
    x, y, _, _, _ = reference
    m = make_model()
    xd, yd = x.to(dev), y.to(dev)
    x2, y2 = (t.to(dev) for t in batch(seed=32))
    y2 = y2.clone()
    y2[0, :40] = -100
    doc, doc2 = P.doc_bounds(xd, EOT), P.doc_bounds(x2, EOT)
    m.eval()
    with bf16(), torch.no_grad():
        logits, loss = m(xd, labels=yd, doc_bounds=doc)
    m.train()
    with bf16():
        mean = m.score(xd, yd, doc_bounds=doc)
        unmasked = m.score(xd, yd)
        rows = m.score(xd, yd, reduction="none", doc_bounds=doc)
        sums = [m.score(a, b, reduction="sum", doc_bounds=d).double().item() for a, b, d in ((xd, yd, doc), (x2, y2, doc2))]
        r = m.evaluate(iter([(xd, yd), (x2, y2)]), eot_token_id=EOT)
        r_plain = m.evaluate(iter([(xd, yd), (x2, y2)]))
    bound = 2.0 ** -8 * logits.float().abs().max().item()
    print(f"masked score {mean.item():.6f} forward loss {loss.item():.6f} bound {bound:.3e}; unmasked {unmasked.item():.6f}")
    assert abs(mean.item() - loss.item()) <= bound
    assert rows.shape == (B, T) and abs(rows.double().mean().item() - mean.item()) <= 1e-6 * mean.item()
    assert mean.item() != unmasked.item()
    counts = [B * T, int((y2 != -100).sum())]
    want = sum(sums) / sum(counts)
    assert r["tokens"] == sum(counts)
    assert abs(r["loss"] - want) <= 3 * torch.finfo(torch.float32).eps * want
    assert r["loss"] != r_plain["loss"]


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
res = {}
for name, wrap in (("plain", lambda m: m), ("ddp", DistributedDataParallel)):
    model = wrap(GPT2(cfg).to("cuda:0"))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with torch.no_grad():
            _, causal = model(x, labels=y)
        _, loss = model(x, labels=y, doc_bounds=packing.doc_bounds(x, 3))
    loss.backward()
    res[name] = {"loss": loss.item(), "causal": causal.item()}
print("RESULT", json.dumps(res), flush=True)
dist.barrier(); dist.destroy_process_group()
"""


def test_ddp_wrapper_forwards_the_keyword(tmp_path):
    """DistributedDataParallel(model)(x, labels=y, doc_bounds=...) at world size 1 over RCCL (the one-rank set-up of
    the wrapper tests): the same loss as the unwrapped model, and not the causal one."""
    x, y = batch()
    torch.save({"x": x, "y": y}, tmp_path / "batch.pt")
    script = tmp_path / "ddp.py"
    script.write_text(DDP)
    env = dict(os.environ, REPO=REPO, CFG=json.dumps(TINY), BATCH=str(tmp_path / "batch.pt"),
               GPT2MI_FORCE_COLLECTIVES="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29587", RANK="0", WORLD_SIZE="1",
               LOCAL_RANK="0")
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT")][0][7:])
    assert res["ddp"]["loss"] == res["plain"]["loss"], res
    assert res["ddp"]["loss"] != res["ddp"]["causal"], res
