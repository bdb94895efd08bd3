"""The deferred weight-gradient family without a GPU: the planner (_lib.wgrad_batch_plan), the engine's mode decision
(engine.wgrad_mode), the C ABI addition (v24.3) and the register budget of the batched kernel instantiation."""
import os
import re
import shutil
import subprocess

import pytest

from gpt_2_distributed_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "gpt_2_distributed_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

C = 768
LAYER = [(C, 4 * C), (4 * C, C), (C, C), (3 * C, C)]  # fc2, fc1, proj, qkv: 36 + 36 + 9 + 27 = 108 tiles
TOKENS = 65536


def tiles(shapes, idx):
    return sum((shapes[i][0] // 256) * (shapes[i][1] // 256) for i in idx)


def check_partition(shapes, body, tail):
    assert sorted(body + tail) == list(range(len(shapes)))  # every problem, so every tile, exactly once


def test_plan_124m_five_rounds_and_a_one_round_tail():
    shapes = LAYER * 12
    body, tail, split = _lib.wgrad_batch_plan(shapes, TOKENS)
    check_partition(shapes, body, tail)
    assert 1278 <= tiles(shapes, body) <= 1280  # five rounds of 256 CUs
    assert -(-tiles(shapes, body) // 256) == 5
    assert 0 < tiles(shapes, tail) * split <= 256  # one round
    assert tiles(shapes, tail) * (split + 1) > 256  # ... that the split fills
    assert len(tail) <= _lib.GROUP_MAX  # one grouped launch
    assert TOKENS // split >= 256


@pytest.mark.parametrize("layers", [2, 3])
def test_plan_two_and_three_layers(layers):
    shapes = LAYER * layers
    body, tail, split = _lib.wgrad_batch_plan(shapes, TOKENS)
    check_partition(shapes, body, tail)
    total = tiles(shapes, range(len(shapes)))
    if total < 256:  # 216 tiles: no whole round, everything is split
        assert not body and split == _lib.wgrad_group_splits(shapes, TOKENS)
    else:  # 324 tiles: one whole round at most in the body, the rest (>= 68 tiles) in the tail
        assert 0 < tiles(shapes, body) <= 256
        assert tiles(shapes, tail) >= total - 256
        # no smaller cover of the 68 remaining tiles exists: tile counts are multiples of 9
        assert tiles(shapes, tail) == 72
        assert split == _lib.wgrad_group_splits([shapes[i] for i in tail], TOKENS)


def test_plan_one_layer_is_all_tail_at_todays_split():
    body, tail, split = _lib.wgrad_batch_plan(LAYER, TOKENS)
    assert body == [] and tail == [0, 1, 2, 3]
    assert split == _lib.wgrad_group_splits(LAYER, TOKENS) == 7


@pytest.mark.parametrize("shapes", [
    [(256, 256)] * 8,                                                   # exactly one round: no tail
    [(256, 256)] * 9,                                                   # one tile over
    [(512, 256), (256, 768), (768, 256), (512, 512), (256, 256)] * 3,   # 39 tiles: 4 rounds + 7
    [(512, 512)] * 3,                                                   # 12 tiles: remainder 4 = one problem
    [(768, 768)],                                                       # 9 tiles in one problem: remainder 1 takes it all
    [(256, 256)] * 3,                                                   # fewer tiles than CUs: all tail
])
@pytest.mark.parametrize("K", [256, 1024, 65536])
def test_plan_toy_device_every_tile_once(shapes, K):
    cus = 8
    body, tail, split = _lib.wgrad_batch_plan(shapes, K, cus=cus)
    check_partition(shapes, body, tail)
    total = tiles(shapes, range(len(shapes)))
    need = total if total < cus else total % cus
    assert tiles(shapes, tail) >= need
    assert (tiles(shapes, tail) == 0) == (need == 0)
    # the tail is a smallest cover: dropping any one of its problems uncovers the remainder
    for i in tail:
        if need < total:
            assert tiles(shapes, tail) - tiles(shapes, [i]) < need
    assert split >= 1 and (split == 1 or K // split >= 256)
    if not tail:
        assert split == 1


def test_plan_never_splits_below_256_tokens():
    for K in (256, 384, 512, 1024, 4096):
        for shapes in ([(256, 256)], LAYER, LAYER * 3, [(768, 768)] * 2):
            _, tail, split = _lib.wgrad_batch_plan(shapes, K)
            assert K // split >= 256, (K, shapes, split)


def test_engine_mode_decision():
    from gpt_2_distributed_amd.engine import DEFER_CAP_BYTES, deferred_bytes, wgrad_mode
    from gpt_2_distributed_amd.model import GPT2Config
    ok = dict(group=True, defer=True, bf16=True, n_embd=768, M=65536, bf16_slabs=False, hooks=False, extra_bytes=1 << 30)
    mode = lambda **kw: wgrad_mode(**{**ok, **kw})  # noqa: E731
    assert mode() == "deferred"
    assert mode(hooks=True) == "pairs"               # DDP / FSDP wrappers keep the per-block launches
    assert mode(defer=False) == "pairs"              # the knob off: today's two pairs
    assert mode(group=False) == "four"               # GROUP_WGRADS off: the four launches, whatever the other knob
    assert mode(group=False, defer=False) == "four"
    assert mode(bf16=False) == "four"                # fp32 mode
    assert mode(n_embd=1600) == "four"               # 1.5B widths: not multiples of 256
    assert mode(M=64) == "four"
    assert mode(bf16_slabs=True) == "four"
    assert mode(extra_bytes=DEFER_CAP_BYTES) == "deferred"
    assert mode(extra_bytes=DEFER_CAP_BYTES + 1) == "pairs"
    # the cap covers GPT-2 124M at B = 64 (10.9 GB) and 350M at B = 32, not 350M at B = 64
    assert DEFER_CAP_BYTES == 16 << 30
    assert round(deferred_bytes(GPT2Config(), 64 * 1024) / 1e9, 1) == 10.9
    assert deferred_bytes(GPT2Config(n_layer=24, n_head=16, n_embd=1024), 32 * 1024) <= DEFER_CAP_BYTES
    assert deferred_bytes(GPT2Config(n_layer=24, n_head=16, n_embd=1024), 64 * 1024) > DEFER_CAP_BYTES


def test_abi_exports_the_batch_entries():
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "gpt2mi.h")).read()
    assert int(re.search(r"#define GPT2MI_ABI_MINOR (\d+)", hdr).group(1)) == lib.gpt2mi_abi_minor() >= 3
    assert _lib.ABI_MINOR >= 3
    for name in ("gpt2mi_gemm_wgrad_batch", "gpt2mi_gemm_wgrad_batch_scratch", "gpt2mi_gemm_wgrad_batch_max"):
        assert name in _lib.EXPORTED and hasattr(lib, name) and _lib._SINCE_MINOR[name] == 3 and name in hdr
    assert _lib.gemm_wgrad_batch_max() >= 4 * 36
    assert _lib.gemm_wgrad_batch_scratch(0) == 0 and _lib.gemm_wgrad_batch_scratch(_lib.gemm_wgrad_batch_max() + 1) == 0
    one, two = _lib.gemm_wgrad_batch_scratch(1), _lib.gemm_wgrad_batch_scratch(2)
    assert 0 < one < two and _lib.gemm_wgrad_batch_scratch(144) == one + 143 * (two - one)


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_batch_instantiation_resources():
    """The batched instantiation (template flags GRP and BAT) compiles with no scratch, no spills, two waves per SIMD
    and within the 256 VGPRs the hand-counted waits assume; the single-problem weight-gradient kernel it shares its body
    with keeps the same."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", f"-I{REPO}/include", "-fno-slp-vectorize", "-c",
           os.path.join(CSRC, "gemm_pp.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs|"
                      r"SGPRs Spill|VGPRs Spill): (\S+)", line)
        if not m:
            continue
        key, val = m.groups()
        if key == "Function Name":
            name = val
            kernels[name] = {}
        elif name:
            kernels[name][key] = int(val)
    # <A_T, B_T, EPI, MAP, PERSIST, BND, DYN, GRP, BAT>
    pat = r"gemm_pp_kernelILb1ELb1ELi1ELi3ELb0ELb0ELb0ELb%dELb%dEE"
    batch = [v for k, v in kernels.items() if re.search(pat % (1, 1), k)]
    single = [v for k, v in kernels.items() if re.search(pat % (0, 0), k)]
    assert len(batch) == 1 and len(single) == 1, sorted(kernels)
    for v in batch + single:
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, v
        assert v["Occupancy [waves/SIMD]"] >= 2 and v["VGPRs"] <= 256, v
