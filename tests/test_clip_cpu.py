"""Gradient clipping and the lr schedule, the parts that need no GPU: lr_schedule.lr_at against closed forms, the
trainer's flags, the optimizer keyword, and the separation conditions of the clip goldens re-asserted from the numbers
they store (tests/golden/make_clip_golden.py)."""
import inspect
import json
import math
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN

from gpt_2_distributed_amd.lr_schedule import lr_at


def test_cosine_schedule_closed_form_values():
    lr, w, d, lo = 6e-4, 10, 110, 6e-5
    at = lambda s: lr_at(s, lr, w, d, lo, "cosine")  # noqa: E731
    assert at(0) == pytest.approx(lr * 1 / 11, rel=1e-15)
    assert at(w - 1) == pytest.approx(lr * 10 / 11, rel=1e-15)
    assert at(w) == pytest.approx(lr, rel=1e-15)  # the cosine starts at its peak
    assert at((w + d) // 2) == pytest.approx((lr + lo) / 2, rel=1e-12)  # the midpoint: cos(pi/2) = 0
    assert at(w + 25) == pytest.approx(lo + 0.5 * (1 + math.sqrt(0.5)) * (lr - lo), rel=1e-12)  # a quarter in
    assert at(d) == pytest.approx(lo, rel=1e-12)
    assert at(d + 5) == lo
    vals = [at(s) for s in range(d + 6)]
    assert all(a < b for a, b in zip(vals[:w], vals[1:w + 1]))  # warmup rises
    assert all(a > b for a, b in zip(vals[w:d], vals[w + 1:d + 1]))  # then the rate falls


def test_cosine_schedule_without_warmup_and_constant():
    assert lr_at(0, 1e-3, 0, 10, 1e-4, "cosine") == pytest.approx(1e-3, rel=1e-15)
    assert lr_at(10, 1e-3, 0, 10, 1e-4, "cosine") == pytest.approx(1e-4, rel=1e-12)
    assert lr_at(5, 1e-3, 0, 10, 0.0, "cosine") == pytest.approx(5e-4, rel=1e-12)
    for s in (0, 7, 10 ** 6):
        assert lr_at(s, 3e-4, kind="constant") == 3e-4
        assert lr_at(s, 3e-4, 5, 2, 1.0, "constant") == 3e-4  # the cosine's arguments are not looked at


@pytest.mark.parametrize("kw", [dict(warmup_steps=10, decay_steps=10), dict(warmup_steps=10, decay_steps=5),
                                dict(warmup_steps=-1, decay_steps=5), dict(warmup_steps=0, decay_steps=0),
                                dict(warmup_steps=0, decay_steps=5, min_lr=-1e-5),
                                dict(warmup_steps=0, decay_steps=5, min_lr=2e-3),
                                dict(warmup_steps=0, decay_steps=5, kind="linear")])
def test_schedule_argument_errors(kw):
    with pytest.raises(ValueError):
        lr_at(0, 1e-3, **dict(dict(min_lr=1e-4, kind="cosine"), **kw))


def test_trainer_flags_default_to_off():
    from gpt_2_distributed_amd.train_gpt2_distributed import build_parser, schedule_from_args
    a = build_parser().parse_args([])
    assert (a.max_grad_norm, a.lr_schedule, a.warmup_steps, a.lr_decay_steps, a.min_lr) == (0.0, "constant", 0, 0, None)
    assert schedule_from_args(a) == dict(lr=a.lr, kind="constant")
    a = build_parser().parse_args(["--lr", "1e-3", "--lr_schedule", "cosine", "--warmup_steps", "2", "--max_steps", "6"])
    s = schedule_from_args(a)
    assert s == dict(lr=1e-3, warmup_steps=2, decay_steps=6, min_lr=1e-4, kind="cosine")  # decay = max_steps, lr/10
    a = build_parser().parse_args(["--lr_schedule", "cosine", "--lr_decay_steps", "9", "--min_lr", "0", "--max_steps", "6"])
    assert schedule_from_args(a)["decay_steps"] == 9 and schedule_from_args(a)["min_lr"] == 0.0
    for bad in (["--lr_schedule", "cosine"], ["--lr_schedule", "cosine", "--warmup_steps", "6", "--max_steps", "6"],
                ["--max_grad_norm", "-1"]):
        with pytest.raises(SystemExit):
            schedule_from_args(build_parser().parse_args(bad))


def test_configure_optimizers_accept_max_grad_norm():
    from gpt_2_distributed_amd.model import GPT2
    from gpt_2_distributed_amd.optim import FusedAdamW, ShardedAdamW
    from gpt_2_distributed_amd.parallel import FullyShardedDataParallel
    for fn in (GPT2.configure_optimizers, FullyShardedDataParallel.configure_optimizers, FusedAdamW.__init__,
               ShardedAdamW.__init__):
        p = inspect.signature(fn).parameters["max_grad_norm"]
        assert p.default is None, fn


def test_clip_trajectory_golden_separates_clipping_and_schedule():
    g = json.load(open(os.path.join(GOLDEN, "tiny_clip_traj.json")))
    on, off = np.array(g["losses"]), np.array(g["losses_unclipped"])
    assert len(on) == g["steps"] == 12 and g["grad_accum"] == 2 and g["batch"] == 2
    sep = np.abs(on - off) / off
    assert sep[3:].min() >= 10 * 1e-4, sep  # 10x the fp32 loss gate from step 3 (counted from 0) on
    assert all(n > g["max_grad_norm"] for n in g["grad_norms"])  # every step clipped
    assert g["lrs"] == [lr_at(s, **g["schedule"]) for s in range(g["steps"])]
    assert min(g["lrs"]) < 0.3 * g["lr"] and max(g["lrs"]) == g["lr"]
    assert np.array(g["tokens"]).shape == (24, 2, 65)


def test_clip_ddp_golden_separates_clipped_from_unclipped():
    g = json.load(open(os.path.join(GOLDEN, "clip_ddp_golden.json")))
    base = json.load(open(os.path.join(GOLDEN, "ddp_golden.json")))
    assert g["config"] == base["config"] and g["lr"] == base["lr"] and g["steps"] >= 3
    assert g["losses"][0] == base["losses"][0] and g["grad_norms"][0] == base["grad_norms"][0]  # the same data
    mx = g["max_grad_norm"]
    assert sum(n > mx for n in g["grad_norms"]) >= 2 and sum(n < mx for n in g["grad_norms"]) >= 1
    # the distance to the unclipped run in units of the gate tests/test_clip_ddp_gpu.py applies to the leading values
    worst = 0.0
    for n, r in g["params"].items():
        a, b = np.array(r["head"]), np.array(g["params_unclipped_head"][n])
        worst = max(worst, float((np.abs(a - b) / (1e-2 * g["lr"] + 1e-4 * np.abs(b))).max()))
    assert worst >= 10, worst
    assert worst == pytest.approx(g["separation_over_gate"]["param_head"], rel=1e-6)
