"""bench.py's contract: a plain run measures the headline figure only, --full adds the per-kernel figures, and
--dump-outputs writes what the last timed step returned (loss, sampled logits rows, sampled master weights)."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import REPO

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
B, T, V, STEPS = 2, 128, 50257, 3


def _bench(*extra):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1",
           "--batch", str(B), "--seq_len", str(T), *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    """dump_outputs on CPU tensors: float32 files, the same seeded rows / elements on every call, every row and
    element when there are fewer than the sample, and under 64 MB at the flagship's sizes by construction."""
    monkeypatch.setenv("HIP_FORCE_DEV_KERNARG", os.environ.get("HIP_FORCE_DEV_KERNARG", "1"))  # (bench sets it at import)
    bench = importlib.import_module("bench")
    assert 4 * (bench.DUMP_LOGIT_ROWS * V + bench.DUMP_PARAMS + 1) <= 64e6
    g = torch.Generator().manual_seed(3)
    padded = torch.randn(4, 96, 24, generator=g).bfloat16()
    logits = padded[..., :19]  # a view of a padded-vocab buffer, as the engine returns it
    arena = torch.randn(5000, generator=g)
    kept = {"logits": logits, "loss": torch.tensor(2.5)}
    monkeypatch.setattr(bench, "DUMP_PARAMS", 1000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), kept, arena)
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("loss", "logits", "params")}
    for n, v in a.items():
        assert v.dtype == np.float32
        np.testing.assert_array_equal(v, np.load(tmp_path / "b" / f"{n}.npy"))
    assert a["loss"].tolist() == [2.5]
    assert a["logits"].shape == (bench.DUMP_LOGIT_ROWS, 19) and a["params"].shape == (1000,)
    flat = logits.float().reshape(-1, 19).numpy()
    rows = {r.tobytes() for r in flat}
    assert all(r.tobytes() in rows for r in a["logits"])  # rows of the logits, whole
    assert len({r.tobytes() for r in a["logits"]}) == bench.DUMP_LOGIT_ROWS  # distinct ones
    assert np.isin(a["params"], arena.numpy()).all()
    # fewer rows / elements than the sample: everything, in order
    monkeypatch.setattr(bench, "DUMP_PARAMS", 10 ** 6)
    bench.dump_outputs(str(tmp_path / "c"), {"logits": logits[:1], "loss": kept["loss"]}, arena)
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "logits.npy"), flat[:96])
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "params.npy"), arena.numpy())


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain run: exactly --steps timed steps, the headline fields, none of the --full figures; --dump-outputs
    writes the last step's loss, 128 rows of its logits and a sample of the updated weights as float32."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    line = _bench("--dump-outputs", str(tmp_path / "out"))
    assert all(k in line for k in HEADLINE)
    assert line["steps"] == STEPS and line["unit"] == "tokens/s" and line["dtype"] == "bf16"
    assert line["higher_is_better"] is True
    assert line["value"] == pytest.approx(B * T / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert line["kernels"] == {} and line["roofline"] is None and line["cpu_baseline"] is None
    out = {n: np.load(tmp_path / "out" / f"{n}.npy") for n in ("loss", "logits", "params")}
    assert sorted(os.listdir(tmp_path / "out")) == ["logits.npy", "loss.npy", "params.npy"]
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in out.values())
    assert out["logits"].shape == (128, V) and out["params"].shape == (4_000_000,)
    assert sum(v.nbytes for v in out.values()) <= 64e6
    assert float(out["loss"][0]) == pytest.approx(line["final_loss"], abs=1e-4)
    # uniform random tokens and a fresh model 4 steps in: the cross-entropy is still near ln V
    assert abs(float(out["loss"][0]) - np.log(V)) < 2.0


@pytest.mark.gpu
def test_full_run_adds_kernel_figures():
    """--full: the per-kernel probes and the roofline of the dominant family ride the timed steps as before."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    line = _bench("--full", "--no-cpu-baseline", "--probe-every", "1")
    assert all(k in line for k in HEADLINE) and line["steps"] == STEPS
    assert {"lm_head_fwd", "lm_head_dgrad", "lm_head_wgrad", "fc1_fwd", "attn_fwd", "wgrad"} <= set(line["kernels"])
    assert line["kernels"]["lm_head_fwd"]["launches"] == STEPS
    assert line["roofline"]["kernel"] in line["kernels"] and line["cpu_baseline"] is None
