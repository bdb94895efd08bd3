"""The CPU side of evaluation: the validation windows (dataloader.iter_eval_batches), the trainer's flag checks, and
the fused lm_head loss kernel's register budget (cross-compiled for gfx950, no GPU)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from gpt_2_distributed_amd import dataloader as dl

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpt_2_distributed_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
T, B = 16, 3


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    """Two val shards of unequal length (token value = a global counter, so a window names its own position) and a
    train shard that must not be picked up."""
    d = tmp_path_factory.mktemp("val")
    a, b = np.arange(0, 403, dtype="<u2"), np.arange(1000, 1000 + 215, dtype="<u2")
    a.tofile(d / "val_000000.bin")
    b.tofile(d / "val_000001.bin")
    np.zeros(500, dtype="<u2").tofile(d / "train_000000.bin")
    paths = dl.get_shard_paths(d, split="val")
    assert [p.name for p in paths] == ["val_000000.bin", "val_000001.bin"]
    windows = [a[o:o + T + 1] for o in range(0, len(a) - (T + 1), T)] + \
              [b[o:o + T + 1] for o in range(0, len(b) - (T + 1), T)]
    assert len(windows) == 25 + 13
    return paths, [w.astype(np.int64) for w in windows]


@pytest.mark.parametrize("world", [1, 2, 3])
def test_windows_are_dealt_round_robin_and_every_rank_gets_as_many_batches(shards, world):
    paths, windows = shards
    n_batches = (len(windows) // world) // B
    seen = []
    for rank in range(world):
        got = list(dl.iter_eval_batches(list(reversed(paths)), T, B, rank, world))  # (sorted inside)
        assert len(got) == n_batches
        for k, (x, y) in enumerate(got):
            assert x.shape == y.shape == (B, T) and x.dtype == y.dtype == torch.int64
            for j in range(B):
                i = (k * B + j) * world + rank  # window i belongs to rank i % world
                assert i % world == rank
                assert np.array_equal(x[j].numpy(), windows[i][:-1]) and np.array_equal(y[j].numpy(), windows[i][1:])
                seen.append(i)
    assert len(seen) == len(set(seen)) == n_batches * B * world  # no window twice across ranks
    assert sorted(seen) == list(range(len(seen)))  # the first windows, in order, none skipped


def test_max_batches_caps_and_a_large_world_yields_nothing(shards):
    paths, windows = shards
    assert len(list(dl.iter_eval_batches(paths, T, B, 0, 1, max_batches=5))) == 5
    assert len(list(dl.iter_eval_batches(paths, T, B, 0, 1, max_batches=500))) == len(windows) // B
    assert len(list(dl.iter_eval_batches(paths, T, B, 0, 1, max_batches=0))) == 0
    a = [x for x, _ in dl.iter_eval_batches(paths, T, B, 1, 2, max_batches=2)]
    b = [x for x, _ in dl.iter_eval_batches(paths, T, B, 1, 2, max_batches=2)]
    assert all(torch.equal(p, q) for p, q in zip(a, b))  # a pure function of its arguments
    world = len(windows) + 1
    for rank in (0, world - 1):
        assert list(dl.iter_eval_batches(paths, T, B, rank, world)) == []
    with pytest.raises(ValueError):
        list(dl.iter_eval_batches(paths, T, B, 2, 2))


def _args(*argv):
    from gpt_2_distributed_amd.train_gpt2_distributed import build_parser
    return build_parser().parse_args(list(argv))


def test_trainer_eval_flags(tmp_path):
    from gpt_2_distributed_amd.train_gpt2_distributed import eval_from_args, val_shards
    a = _args()
    assert (a.eval_every, a.eval_steps, a.eval_batch, a.val_split) == (0, 20, None, "val")
    assert eval_from_args(a) == {}  # off by default
    assert eval_from_args(_args("--eval_every", "5", "--batch", "6")) == dict(every=5, steps=20, batch=6, split="val")
    assert eval_from_args(_args("--eval_every", "5", "--eval_batch", "2", "--eval_steps", "3", "--val_split", "dev")) == \
        dict(every=5, steps=3, batch=2, split="dev")
    for bad in (["--eval_every", "-1"], ["--eval_every", "2", "--eval_steps", "0"],
                ["--eval_every", "2", "--eval_batch", "0"], ["--eval_every", "2", "--val_split", "train"],
                ["--eval_every", "2", "--val_split", ""]):
        with pytest.raises(SystemExit):
            eval_from_args(_args(*bad))
    ev = eval_from_args(_args("--eval_every", "2"))
    np.zeros(4000, dtype="<u2").tofile(tmp_path / "train_000000.bin")
    with pytest.raises(SystemExit, match="no 'val' shard"):
        val_shards(tmp_path, ev, 128, 1)
    with pytest.raises(SystemExit, match="no 'val' shard"):
        val_shards(tmp_path / "missing", ev, 128, 1)
    np.zeros(128 * 9 + 2, dtype="<u2").tofile(tmp_path / "val_000000.bin")  # 9 windows
    assert [p.name for p in val_shards(tmp_path, ev, 128, 2)] == ["val_000000.bin"]  # 4 per rank = one batch of 4
    with pytest.raises(SystemExit, match="fewer than one batch"):
        val_shards(tmp_path, ev, 128, 3)


def test_main_rejects_eval_without_val_shards_before_anything_is_built(tmp_path, monkeypatch):
    """--eval_every with a data dir that holds no val shard: SystemExit from main() before the process group, the
    device or the model are touched (this test runs without a GPU)."""
    from gpt_2_distributed_amd import train_gpt2_distributed as t
    np.zeros(4000, dtype="<u2").tofile(tmp_path / "train_000000.bin")
    # main() seeds torch and sets an allocator default in the environment: both are put back after the test
    monkeypatch.setenv("PYTORCH_CUDA_ALLOC_CONF", os.environ.get("PYTORCH_CUDA_ALLOC_CONF", ""))
    rng = torch.get_rng_state()
    monkeypatch.setattr(t, "init_distributed", lambda: pytest.fail("built something"))
    monkeypatch.setattr(t, "GPT2", lambda *a, **k: pytest.fail("built the model"))
    with pytest.raises(SystemExit, match="--eval_every 2: no 'val' shard"):
        t.main(["--data_dir", str(tmp_path), "--eval_every", "2", "--training_mode", "ddp"])
    torch.set_rng_state(rng)


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_lm_loss_kernels_compile_without_scratch_or_spills():
    """csrc/lm_loss.hip under the Makefile's default flags: zero scratch, no VGPR spills, and the two workgroups per
    CU its launch bounds promise (the parse of tests/test_kernel_resources.py)."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", f"-I{CSRC}/../../include", "-c",
           os.path.join(CSRC, "lm_loss.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"SGPRs Spill|VGPRs Spill): (\S+)", line)
        if not m:
            continue
        key, val = m.groups()
        if key == "Function Name":
            name = val
            kernels[name] = {}
        elif name:
            kernels[name][key] = int(val)
    for sub, occ in (("lm_loss_partial_kernel", 2), ("lm_loss_finish_kernel", 4)):
        found = {k: v for k, v in kernels.items() if sub in k}
        assert found, f"{sub} not found"
        for k, v in found.items():
            assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (k, v)
            assert v["Occupancy [waves/SIMD]"] >= occ, (k, v)
