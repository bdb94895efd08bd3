"""--optimizer muon through the trainer on synthetic shards (tests/test_clip_trainer_gpu.py's shape)."""
import json
import math
import subprocess
import sys

import pytest
import torch

from tests.conftest import REPO

pytestmark = pytest.mark.gpu


def _run(tmp_path, save_dir, *extra):
    cmd = [sys.executable, "-m", "gpt_2_distributed_amd.train_gpt2_distributed", "--data_dir", str(tmp_path / "data"),
           "--synthetic", "2", "--synthetic_tokens", "60000", "--seq_len", "128", "--batch", "4",
           "--grad_accum_steps", "2", "--workers", "1", "--training_mode", "local", "--log_every", "1", "--save_dir",
           str(tmp_path / save_dir), *extra]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    return {s["step"]: s for s in (json.loads(l) for l in r.stdout.splitlines() if l.startswith("{"))}


def test_muon_runs_resumes_and_adamw_is_the_default_path(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    tmp = tmp_path
    full = _run(tmp, "a", "--optimizer", "muon", "--max_steps", "4", "--save_every", "2")
    assert sorted(full) == [1, 2, 3, 4]
    assert all(math.isfinite(s["loss"]) and 0.0 < s["loss"] < 20.0 and math.isfinite(s["grad_norm"])
               for s in full.values())
    resumed = _run(tmp, "b", "--optimizer", "muon", "--max_steps", "4", "--save_every", "100", "--resume",
                   str(tmp / "a" / "step_0000002"))
    assert sorted(resumed) == [3, 4] and resumed[3]["loss"] == full[3]["loss"], (resumed, full)
    runs = [_run(tmp, d, "--max_steps", "2", "--deterministic", *flag)
            for d, flag in (("c", ()), ("d", ("--optimizer", "adamw")))]
    for n in (1, 2):
        assert runs[0][n].keys() == runs[1][n].keys()
        assert all(runs[0][n][k] == runs[1][n][k] for k in ("loss", "grad_norm", "lr")), n
