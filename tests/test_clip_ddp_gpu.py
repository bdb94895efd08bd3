"""Global-norm clipping through the data-parallel wrappers against the REFERENCE: 2 gloo ranks sharing the GPU
(GPT2MI_SINGLE_DEVICE=1, tests/test_ddp_gpu.py's set-up and bucket size) run the reference loop with
configure_optimizers(max_grad_norm=1.2) and are compared with tests/golden/clip_ddp_golden.json: the reference model,
single-process on the concatenated batch, with torch's clip_grad_norm_(params, 1.2) before torch AdamW. Two of the
three steps clip. Loss and the reported (pre-clip, global) norm at every step and the final parameters must match at
tests/test_ddp_gpu.py's fp32 tolerances; the golden's clipped and unclipped final parameters are 34x that gate apart
(tests/test_clip_cpu.py), so a per-shard clip under FSDP, a missing clip, or an update issued before DDP's deferred
bucket has arrived fails here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

WORKER = r"""
import os, sys, json, torch, torch.distributed as dist
sys.path.insert(0, os.environ["REPO"])
from gpt_2_distributed_amd.parallel import init_distributed, DistributedDataParallel, FullyShardedDataParallel
from gpt_2_distributed_amd.model import GPT2, GPT2Config
init_distributed()
r, w = dist.get_rank(), dist.get_world_size()
G = json.load(open(os.environ["GOLDEN"]))
cfg = GPT2Config(**G["config"])
S, GA = G["steps"], G["grad_accum"]
P = G["world"] * G["per_rank"] // w
toks = torch.tensor(G["tokens"], dtype=torch.int64)
res = {}
for variant in os.environ["VARIANTS"].split(","):
    mode, kind = variant.split("/")
    m = GPT2(cfg).to("cuda:0")
    wrap = FullyShardedDataParallel(m, overlap_optimizer=kind == "overlap", reshard_after_forward=kind == "reshard") \
        if mode == "fsdp" else DistributedDataParallel(m, bucket_mb=0.25, overlap_optimizer=kind == "overlap")
    opt = wrap.configure_optimizers(learning_rate=G["lr"], max_grad_norm=G["max_grad_norm"])
    losses, norms, coefs = [], [], []
    for s in range(S):
        for a in range(GA):
            t = toks[s, a, r * P:(r + 1) * P].cuda()
            _, loss = wrap(t[:, :-1], labels=t[:, 1:])
            loss = loss / GA
            loss.backward()
        opt.step()
        opt.zero_grad()
        lt = (loss.detach() * GA).reshape(1).clone(); dist.all_reduce(lt)
        losses.append(lt.item() / w); norms.append(float(opt.grad_norm)); coefs.append(float(opt.clip_coef))
    sd = wrap.state_dict()
    fp = {}
    for n in G["params"]:
        d = sd[n].detach().double().cpu()
        fp[n] = [float(d.sum()), float((d * d).sum()), [float(v) for v in d.reshape(-1)[:16]]]
    res[variant] = {"losses": losses, "norms": norms, "coefs": coefs, "params": fp}
if r == 0:
    print("RESULT", json.dumps(res), flush=True)
dist.barrier(); dist.destroy_process_group()
"""

VARIANTS = ["ddp/fused", "ddp/overlap", "fsdp/fused", "fsdp/overlap", "fsdp/reshard"]
GOLD = json.load(open(os.path.join(GOLDEN, "clip_ddp_golden.json")))
T_LOSS, T_NORM, T_PAR = 1e-4, 1e-3, 1e-4  # tests/test_ddp_gpu.py TOL["fp32"]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    tmp = tmp_path_factory.mktemp("clipddp")
    script = tmp / "w.py"
    script.write_text(WORKER)
    env = dict(os.environ, REPO=REPO, GOLDEN=os.path.join(GOLDEN, "clip_ddp_golden.json"),
               VARIANTS=",".join(VARIANTS), GPT2MI_SINGLE_DEVICE="1", GPT2MI_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", "--master-port=29595", str(script)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT")][0][7:])


@pytest.mark.parametrize("variant", VARIANTS)
def test_two_ranks_clipped_vs_reference_concatenated_batch(results, variant):
    r = results[variant]
    rl = np.abs(np.array(r["losses"]) - GOLD["losses"]) / np.array(GOLD["losses"])
    assert rl.max() < T_LOSS, (variant, r["losses"], GOLD["losses"])
    rn = np.abs(np.array(r["norms"]) - GOLD["grad_norms"]) / np.array(GOLD["grad_norms"])
    assert rn.max() < T_NORM, (variant, r["norms"], GOLD["grad_norms"])  # fsdp: the global norm, not the shard's
    want = [min(1.0, GOLD["max_grad_norm"] / (n + 1e-6)) for n in GOLD["grad_norms"]]
    np.testing.assert_allclose(r["coefs"], want, rtol=T_NORM)
    assert sum(c < 1.0 for c in r["coefs"]) >= 2 and sum(c == 1.0 for c in r["coefs"]) >= 1
    tot, tot_ref = 0.0, 0.0
    for n, (s, ss, head) in r["params"].items():
        g = GOLD["params"][n]
        tot, tot_ref = tot + ss, tot_ref + g["sumsq"]
        assert abs(ss - g["sumsq"]) <= T_PAR * g["sumsq"] + 1e-12, (variant, n)
        np.testing.assert_allclose(head, g["head"], rtol=T_PAR, atol=1e-2 * GOLD["lr"], err_msg=f"{variant} {n}")
    assert abs(tot - tot_ref) <= 1e-2 * tot_ref, variant
