"""--doc_mask --reset_positions in the trainer and the evaluation CLI, end to end on the GPU (subprocesses under their
own time limits, as tests/test_docmask_trainer_gpu.py): four optimizer steps at 124M on the synthetic Zipf shards with
token 3 as the separator and validation every two steps; finite losses and val_loss lines; a step-1 loss that differs
from the run with --doc_mask alone and equals ``model(x, y, doc_bounds=..., reset_positions=True)`` on the first batch
within the bf16 gate (2e-2 relative; the trainer runs under bf16 autocast; --dropout 0 so that the comparison needs no
dropout stream); and ``evaluate --doc_mask --reset_positions`` on the checkpoint prints the trainer's last val_loss."""
import dataclasses
import json
import math
import pathlib
import subprocess
import sys

import pytest
import torch

from tests.conftest import REPO

pytestmark = pytest.mark.gpu

EOT = 3
STEPS, BATCH, SEQ = 4, 4, 128


def _cmd(data, save, steps, *extra):
    return [sys.executable, "-m", "gpt_2_distributed_amd.train_gpt2_distributed", "--data_dir", str(data),
            "--model", "124M", "--seq_len", str(SEQ), "--batch", str(BATCH), "--synthetic", "2",
            "--synthetic_tokens", "60000", "--max_steps", str(steps), "--grad_accum_steps", "1", "--workers", "0",
            "--log_every", "1", "--training_mode", "local", "--save_every", str(steps), "--save_dir", str(save),
            "--dropout", "0", "--doc_mask", "--eot_token_id", str(EOT), *extra]


def _run(cmd):
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    return r, [l for l in lines if "loss" in l], {l["step"]: l for l in lines if "val_loss" in l}


def test_trainer_and_evaluator_with_reset_positions(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    r, train, val = _run(_cmd(tmp_path / "data", tmp_path / "ck", STEPS, "--reset_positions", "--eval_every", "2",
                              "--eval_steps", "2"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert [s["step"] for s in train] == [1, 2, 3, 4] and sorted(val) == [2, 4]
    assert all(math.isfinite(s["loss"]) and 0.0 < s["loss"] < 20.0 for s in train), train
    assert all(math.isfinite(v["val_loss"]) and 0.0 < v["val_loss"] < 20.0 for v in val.values()), val
    assert val[4]["val_tokens"] == 2 * BATCH * SEQ
    # the same command without --reset_positions: another first loss
    r2, absolute, _ = _run(_cmd(tmp_path / "data2", tmp_path / "ck2", 1))
    assert r2.returncode == 0, r2.stderr[-3000:]
    print(f"step-1 loss with --reset_positions {train[0]['loss']!r}, with --doc_mask alone {absolute[0]['loss']!r}")
    assert train[0]["loss"] != absolute[0]["loss"]
    # the first batch through the model itself (the seed-42 init the trainer starts from, bf16 autocast, dropout 0)
    from gpt_2_distributed_amd import dataloader
    from gpt_2_distributed_amd.model import GPT2, GPT2Config, MODEL_SIZES
    from gpt_2_distributed_amd.packing import doc_bounds
    paths = dataloader.get_shard_paths(pathlib.Path(tmp_path / "data"), split="train")
    x, y = next(iter(dataloader.iter_batches(paths, SEQ, BATCH, 1, epoch=0)))
    over = dict(MODEL_SIZES["124M"], resid_pdrop=0.0, attn_pdrop=0.0)
    m = GPT2(dataclasses.replace(GPT2Config(), n_positions=SEQ, **over)).to("cuda:0")
    x, y = x.to("cuda:0"), y.to("cuda:0")
    doc = doc_bounds(x, EOT)
    assert min(len(row.unique()) for row in doc.start.cpu()) >= 2
    with torch.autocast("cuda", dtype=torch.bfloat16), torch.no_grad():
        m.train()
        _, loss = m(x, labels=y, doc_bounds=doc, reset_positions=True)
    rel = abs(loss.item() - train[0]["loss"]) / loss.item()
    print(f"step-1 loss of the trainer {train[0]['loss']!r}, of the model on the first batch {loss.item()!r}")
    assert rel < 2e-2
    del m
    # the CLI on the checkpoint prints the trainer's val_loss at that step
    cmd = [sys.executable, "-m", "gpt_2_distributed_amd.evaluate", "--checkpoint",
           str(tmp_path / "ck" / f"step_{STEPS:07d}"), "--model", "124M", "--data_dir", str(tmp_path / "data"),
           "--batch", str(BATCH), "--max_batches", "2", "--seq_len", str(SEQ), "--doc_mask", "--eot_token_id", str(EOT),
           "--reset_positions"]
    e = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert e.returncode == 0, e.stderr[-3000:]
    res = json.loads([l for l in e.stdout.splitlines() if l.startswith("{")][0])
    assert res["loss"] == val[4]["val_loss"] and res["tokens"] == val[4]["val_tokens"]
    e2 = subprocess.run(cmd[:-1], cwd=REPO, capture_output=True, text=True, timeout=240)
    assert e2.returncode == 0, e2.stderr[-3000:]
    assert json.loads([l for l in e2.stdout.splitlines() if l.startswith("{")][0])["loss"] != res["loss"]
