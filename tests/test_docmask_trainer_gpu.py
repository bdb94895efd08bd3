"""--doc_mask in the trainer and the evaluation CLI, end to end on the GPU (subprocesses, as
tests/test_eval_trainer_gpu.py): three optimizer steps at 124M on the synthetic Zipf shards with token 3 as the
separator (frequency 0.035 in the shard of seed 1234: a mean document of about 28 tokens), finite losses, a step-1 loss
that differs from the same command without the flag, and ``evaluate --doc_mask`` on the written checkpoint."""
import json
import math
import os
import pathlib
import subprocess
import sys

import pytest
import torch

from tests.conftest import REPO

pytestmark = pytest.mark.gpu

EOT = 3
# one micro-batch per step: the run trains on the first three batches of iter_batches' order, whose twelve rows hold 3 to
# 9 documents each (the sixth batch has a row without a separator, so a longer run would not meet the CPU assertion)
STEPS, ACCUM, BATCH, SEQ = 3, 1, 4, 128


def _cmd(data, save, *extra):
    return [sys.executable, "-m", "gpt_2_distributed_amd.train_gpt2_distributed", "--data_dir", str(data),
            "--model", "124M", "--seq_len", str(SEQ), "--batch", str(BATCH), "--synthetic", "2",
            "--synthetic_tokens", "60000", "--max_steps", str(STEPS), "--grad_accum_steps", str(ACCUM), "--workers", "0",
            "--log_every", "1", "--training_mode", "local", "--save_every", str(STEPS), "--save_dir", str(save), *extra]


def _run(cmd):
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    return r, [l for l in lines if "loss" in l]


def test_trainer_and_evaluator_with_doc_mask(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    r, masked = _run(_cmd(tmp_path / "data", tmp_path / "ck", "--doc_mask", "--eot_token_id", str(EOT)))
    assert r.returncode == 0, r.stderr[-3000:]
    assert [s["step"] for s in masked] == [1, 2, 3]
    assert all(math.isfinite(s["loss"]) and 0.0 < s["loss"] < 20.0 for s in masked), masked
    # on the CPU: every row the run trained on holds at least two documents (the order is iter_batches', --workers 0)
    from gpt_2_distributed_amd import dataloader
    from gpt_2_distributed_amd.packing import doc_bounds_reference
    paths = dataloader.get_shard_paths(pathlib.Path(tmp_path / "data"), split="train")
    seen = 0
    for x, _ in dataloader.iter_batches(paths, SEQ, BATCH, 1, epoch=0):
        docs = [len(row.unique()) for row in doc_bounds_reference(x, EOT).start]
        assert min(docs) >= 2, docs
        seen += 1
        if seen == STEPS * ACCUM:
            break
    assert seen == STEPS * ACCUM
    r2, plain = _run(_cmd(tmp_path / "data2", tmp_path / "ck2"))
    assert r2.returncode == 0, r2.stderr[-3000:]
    print(f"step-1 loss with --doc_mask {masked[0]['loss']!r}, without {plain[0]['loss']!r}")
    assert masked[0]["loss"] != plain[0]["loss"]
    cmd = [sys.executable, "-m", "gpt_2_distributed_amd.evaluate", "--checkpoint",
           str(tmp_path / "ck" / f"step_{STEPS:07d}"), "--model", "124M", "--data_dir", str(tmp_path / "data"),
           "--split", "train", "--batch", "4", "--max_batches", "2", "--seq_len", str(SEQ), "--doc_mask",
           "--eot_token_id", str(EOT)]
    e = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert e.returncode == 0, e.stderr[-3000:]
    res = json.loads([l for l in e.stdout.splitlines() if l.startswith("{")][0])
    assert math.isfinite(res["loss"]) and 0.0 < res["loss"] < 20.0 and res["tokens"] == 2 * 4 * SEQ
    e2 = subprocess.run(cmd[:-3], cwd=REPO, capture_output=True, text=True, timeout=240)
    assert e2.returncode == 0, e2.stderr[-3000:]
    plain_eval = json.loads([l for l in e2.stdout.splitlines() if l.startswith("{")][0])
    assert plain_eval["loss"] != res["loss"]
