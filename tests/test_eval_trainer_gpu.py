"""Validation in the trainer and the stand-alone evaluation CLI, end to end on the GPU (subprocesses, as
tests/test_trainer_gpu.py): --eval_every prints val_loss lines without changing the training run, a resumed run prints
the uninterrupted run's val_loss, missing val shards stop the run before it starts, and
``python -m gpt_2_distributed_amd.evaluate`` on a checkpoint prints the trainer's val_loss.

Losses compared between two trainer PROCESSES are held to 1e-4 relative, the bound tests/test_trainer_gpu.py sets for the
same logged losses across processes, not to equality of every printed digit: the parent's training steps differ in the
last bits from run to run (float atomics in the LayerNorm and embedding backwards) and AdamW at lr 1e-4 amplifies that.
Measured on an MI355X, this command twice WITHOUT evaluation: steps 1-3 print the same loss / grad_norm, step 4 prints
loss 8.08383 vs 8.08404 and grad_norm 4.83961 vs 4.83973; twice with --eval_every 2: 8.08397 / 4.83966 and 8.08387 /
4.83973 (val_loss at step 4: 7.7594738 vs 7.7594609); another time a run with evaluation printed 8.38371 at step 3
where two runs without printed 8.38369. A dropout stream moved by the evaluation (the parent's no-grad forward) would
change the losses of the following steps in the third digit. What evaluation computes from given weights IS exact: the
CLI on a checkpoint prints the trainer's val_loss to the last digit. The logged grad_norm is held to 2e-4 relative: its
run-to-run spread is larger than the loss's (3.7e-5 at step 4 above, 5.5e-5 in one pair of runs at --lr 1e-5), and 2e-4
is the loss bound doubled, about four times the largest spread seen."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from tests.conftest import REPO

pytestmark = pytest.mark.gpu


def _cmd(data, save, *extra):
    return [sys.executable, "-m", "gpt_2_distributed_amd.train_gpt2_distributed", "--data_dir", str(data),
            "--synthetic", "2", "--synthetic_tokens", "60000", "--seq_len", "128", "--batch", "4",
            "--grad_accum_steps", "2", "--workers", "1", "--log_every", "1", "--training_mode", "local",
            "--max_steps", "4", "--save_dir", str(save), *extra]


def _run(cmd):
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    return r, [l for l in lines if "loss" in l], {l["step"]: l for l in lines if "val_loss" in l}


@pytest.fixture(scope="module")
def evaluated(tmp_path_factory):
    """The run with validation on: 4 steps, val at 2 and 4, checkpoints at 2 and 4."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    tmp = tmp_path_factory.mktemp("evalrun")
    r, train, val = _run(_cmd(tmp / "data", tmp / "ck", "--save_every", "2", "--eval_every", "2", "--eval_steps", "2"))
    assert r.returncode == 0, r.stderr[-3000:]
    return tmp, train, val


def test_eval_lines_and_an_unchanged_training_run(evaluated, tmp_path):
    tmp, train, val = evaluated
    assert sorted(val) == [2, 4]
    for v in val.values():
        assert set(v) == {"step", "val_loss", "val_ppl", "val_tokens", "eval_s"}
        assert math.isfinite(v["val_loss"]) and 0.0 < v["val_loss"] < 20.0 and v["val_ppl"] == math.exp(v["val_loss"])
        assert v["val_tokens"] == 2 * 4 * 128 and v["eval_s"] > 0
    assert val[4]["val_loss"] != val[2]["val_loss"]  # two optimizer steps apart
    assert os.path.exists(tmp / "data" / "val_000000.bin")
    r, plain, no_val = _run(_cmd(tmp_path / "data", tmp_path / "ck", "--save_every", "100", "--eval_every", "0"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert not no_val and sorted(os.listdir(tmp_path / "data")) == ["train_000000.bin", "train_000001.bin"]
    assert [s["step"] for s in train] == [s["step"] for s in plain] == [1, 2, 3, 4]
    assert set(train[0]) == set(plain[0])  # the training lines keep their keys
    for on, off in zip(train, plain):
        for key in ("loss", "grad_norm"):
            print(f"step {on['step']} {key}: with evaluation {on[key]!r}, without {off[key]!r}")
            assert abs(on[key] - off[key]) <= (1e-4 if key == "loss" else 2e-4) * off[key], (on["step"], key)
    assert train[0]["loss"] == plain[0]["loss"]  # (one forward from the same init: no atomics yet)


def test_resumed_run_prints_the_same_val_loss(evaluated, tmp_path):
    tmp, _, val = evaluated
    r, _, resumed = _run(_cmd(tmp / "data", tmp_path / "ck", "--save_every", "100", "--eval_every", "2",
                              "--eval_steps", "2", "--resume", str(tmp / "ck" / "step_0000002")))
    assert r.returncode == 0, r.stderr[-3000:]
    assert sorted(resumed) == [4]
    print(f"val_loss at step 4: resumed {resumed[4]['val_loss']!r}, uninterrupted {val[4]['val_loss']!r}")
    # two training steps lie between the checkpoint and this evaluation: the bound of the resumed training losses
    # (tests/test_trainer_gpu.py); evaluation adds no state of its own (test_cli_prints_the_trainers_val_loss is exact)
    assert abs(resumed[4]["val_loss"] - val[4]["val_loss"]) <= 1e-4 * val[4]["val_loss"]
    assert resumed[4]["val_tokens"] == val[4]["val_tokens"]


def test_missing_val_shards_stop_the_run_before_it_starts(tmp_path):
    from gpt_2_distributed_amd.synthetic import write_shards
    write_shards(tmp_path / "data", 1, 3000, split="train")
    cmd = [sys.executable, "-m", "gpt_2_distributed_amd.train_gpt2_distributed", "--data_dir", str(tmp_path / "data"),
           "--seq_len", "128", "--batch", "4", "--max_steps", "2", "--eval_every", "2", "--save_dir",
           str(tmp_path / "ck")]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode != 0
    assert "no 'val' shard" in r.stderr and "--eval_every" in r.stderr
    assert "started rank" not in r.stdout and not os.path.exists(tmp_path / "ck")


def test_cli_prints_the_trainers_val_loss(evaluated, tmp_path):
    tmp, _, val = evaluated
    out = tmp_path / "rows.npy"
    cmd = [sys.executable, "-m", "gpt_2_distributed_amd.evaluate", "--checkpoint", str(tmp / "ck" / "step_0000004"),
           "--model", "124M", "--data_dir", str(tmp / "data"), "--batch", "4", "--max_batches", "2", "--seq_len", "128",
           "--per_token", str(out)]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert res["loss"] == val[4]["val_loss"] and res["tokens"] == val[4]["val_tokens"] and res["batches"] == 2
    assert res["ppl"] == math.exp(res["loss"])
    import numpy as np
    rows = np.load(out)
    assert rows.shape == (8, 128) and rows.dtype == np.float32
    assert abs(rows.astype(np.float64).mean() - res["loss"]) <= 1e-6 * res["loss"]
