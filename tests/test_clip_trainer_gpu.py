"""The trainer's recipe flags end to end (--max_grad_norm, --lr_schedule cosine, --warmup_steps, --lr_decay_steps) on
synthetic shards with tests/test_trainer_gpu.py::test_trainer_cli_end_to_end's shape: the logged lr is lr_at's, the
logged clip_coef is the clip_grad_norm_ coefficient of the logged norm, a resumed run continues the schedule, and with
no new flag the lr is --lr at every step."""
import json
import subprocess
import sys

import pytest
import torch

from tests.conftest import REPO

from gpt_2_distributed_amd.lr_schedule import lr_at

pytestmark = pytest.mark.gpu

LR = 1e-4  # the trainer's default --lr
RECIPE = ["--max_grad_norm", "1.0", "--lr_schedule", "cosine", "--warmup_steps", "2", "--lr_decay_steps", "6",
          "--max_steps", "6", "--log_every", "1"]


def _run(tmp_path, save_dir, *extra):
    cmd = [sys.executable, "-m", "gpt_2_distributed_amd.train_gpt2_distributed", "--data_dir", str(tmp_path / "data"),
           "--synthetic", "2", "--synthetic_tokens", "60000", "--seq_len", "128", "--batch", "4",
           "--grad_accum_steps", "2", "--workers", "1", "--training_mode", "local", "--save_dir",
           str(tmp_path / save_dir), *extra]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    return {s["step"]: s for s in (json.loads(l) for l in r.stdout.splitlines() if l.startswith("{"))}


@pytest.fixture(scope="module")
def full_run(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    tmp = tmp_path_factory.mktemp("cliptrainer")
    return tmp, _run(tmp, "a", *RECIPE, "--save_every", "3")


def test_trainer_cli_clip_and_cosine_flags(full_run):
    _, steps = full_run
    assert sorted(steps) == [1, 2, 3, 4, 5, 6]
    for n, s in steps.items():
        assert s["lr"] == lr_at(n - 1, LR, 2, 6, LR / 10, "cosine"), (n, s["lr"])  # n - 1 steps were taken before it
        assert 0.0 < s["loss"] < 20.0 and 0.0 < s["clip_coef"] <= 1.0
        want = min(1.0, 1.0 / (s["grad_norm"] + 1e-6))
        # the log rounds the norm to 5 decimals (moves the coefficient by <= 5e-6 coef^2) and the coefficient to 6
        assert abs(s["clip_coef"] - want) <= 5e-6 * want * want + 5e-7 + 2e-7, (n, s["clip_coef"], want)
    assert any(s["clip_coef"] < 1.0 for s in steps.values())  # an untrained model's gradients: the clip is active
    assert steps[1]["lr"] < steps[2]["lr"] < steps[3]["lr"] > steps[4]["lr"] > steps[6]["lr"]
    assert steps[3]["lr"] == pytest.approx(LR, rel=1e-12)


def test_trainer_cli_resume_continues_the_schedule(full_run):
    tmp, full = full_run
    resumed = _run(tmp, "b", *RECIPE, "--save_every", "100", "--resume", str(tmp / "a" / "step_0000003"))
    assert sorted(resumed) == [4, 5, 6]
    for n in (4, 5, 6):
        assert resumed[n]["lr"] == full[n]["lr"], n
        assert abs(resumed[n]["loss"] - full[n]["loss"]) <= 1e-4 * full[n]["loss"], (n, resumed[n], full[n])


def test_trainer_cli_without_the_new_flags_keeps_lr_constant(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    steps = _run(tmp_path, "c", "--max_steps", "3", "--log_every", "1", "--lr", "3e-4")
    assert sorted(steps) == [1, 2, 3]
    assert all(s["lr"] == 3e-4 and "clip_coef" not in s for s in steps.values())
