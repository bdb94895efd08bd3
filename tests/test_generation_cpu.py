"""Generation without a GPU: the sampling rule on CPU logits, the argument checks of the decode entries (through the
built library with NULL pointers: nothing is launched), and the register budget of csrc/decode.hip."""
import os
import shutil

import pytest
import torch

from gpt_2_distributed_amd.generation import sample_next
from tests.conftest import REPO
from tests.test_kernel_resources import HIPCC, _instantiation, _resources

LIB = os.path.join(REPO, "gpt_2_distributed_amd", "libgpt2mi.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libgpt2mi.so not built (run __graft_entry__.build())")


# ---- sample_next ---------------------------------------------------------------------------------------------------
def _logits(B=6, V=50, seed=0):
    return torch.randn(B, V, generator=torch.Generator().manual_seed(seed)) * 3


def test_greedy_and_top1_are_argmax():
    lg = _logits()
    assert torch.equal(sample_next(lg, temperature=0.0), lg.argmax(-1))
    g = torch.Generator().manual_seed(1)
    assert torch.equal(sample_next(lg, temperature=1.0, top_k=1, generator=g), lg.argmax(-1))
    assert torch.equal(sample_next(lg, temperature=0.7, top_k=1, generator=g), lg.argmax(-1))


def test_top_k_draws_stay_in_the_top_k_set():
    lg = _logits(B=4, V=40, seed=2)
    top5 = lg.topk(5, dim=-1).indices
    g = torch.Generator().manual_seed(3)
    for _ in range(500):  # 4 rows x 500 = 2,000 draws
        t = sample_next(lg, temperature=1.3, top_k=5, generator=g)
        assert bool((t[:, None] == top5).any(-1).all())


def test_same_seed_same_draws():
    lg = _logits(B=8, V=100, seed=4)
    a = [sample_next(lg, 1.0, None, torch.Generator().manual_seed(11)) for _ in range(2)]
    assert torch.equal(a[0], a[1])
    g1, g2 = torch.Generator().manual_seed(12), torch.Generator().manual_seed(12)
    s1 = torch.stack([sample_next(lg, 0.9, 20, g1) for _ in range(10)])
    s2 = torch.stack([sample_next(lg, 0.9, 20, g2) for _ in range(10)])
    assert torch.equal(s1, s2)


def test_frequencies_follow_the_softmax():
    p = torch.tensor([0.5, 0.25, 0.15, 0.1])
    lg = p.log().repeat(2000, 1)  # 2,000 rows x 10 calls = 20,000 draws
    g = torch.Generator().manual_seed(5)
    counts = torch.zeros(4)
    for _ in range(10):
        counts += torch.bincount(sample_next(lg, 1.0, None, g), minlength=4).float()
    freq = counts / counts.sum()
    assert counts.sum() == 20000
    assert float((freq - p).abs().max()) < 0.02, freq


def test_sample_next_rejects_bad_arguments():
    with pytest.raises(ValueError):
        sample_next(torch.zeros(5))
    with pytest.raises(ValueError):
        sample_next(torch.zeros(1, 5), temperature=-1.0)
    with pytest.raises(ValueError):
        sample_next(torch.zeros(1, 5), top_k=0)


# ---- argument checks of the C entries (no launch: every pointer is NULL) -------------------------------------------
@pytest.fixture()
def lib():
    from gpt_2_distributed_amd import _lib
    return _lib.load()


def _skinny(lib, M, N, K, ws_floats=0):
    return lib.gpt2mi_gemm_skinny(0, M, N, K, None, K, None, K, None, N, None, None, None, ws_floats, None)


@needs_lib
def test_gemm_skinny_refuses_bad_shapes(lib):
    assert _skinny(lib, 65, 768, 768) == 22
    assert b"M=65" in lib.gpt2mi_last_error()
    assert _skinny(lib, 0, 768, 768) == 22
    for N, K in ((100, 768), (768, 96), (32, 64), (64, 0)):
        assert _skinny(lib, 8, N, K) == 22, (N, K)
        assert b"multiples of 64" in lib.gpt2mi_last_error()
    assert lib.gpt2mi_gemm_skinny(7, 8, 64, 64, None, 64, None, 64, None, 64, None, None, None, 0, None) == 22
    assert b"epilogue" in lib.gpt2mi_last_error()


@needs_lib
def test_gemm_skinny_refuses_a_small_workspace(lib):
    # N = 768: 48 strips of 16 columns, so K is split over blocks and the partial sums need a workspace
    need = lib.gpt2mi_gemm_skinny_workspace(8, 768, 768)
    assert need > 0 and need % (8 * 768) == 0
    assert _skinny(lib, 8, 768, 768, ws_floats=need - 1) == 22
    assert b"workspace too small" in lib.gpt2mi_last_error()
    # the lm_head shape has strips enough: no workspace, and the size does not depend on M beyond the row count
    assert lib.gpt2mi_gemm_skinny_workspace(64, 50432, 768) == 0
    assert lib.gpt2mi_gemm_skinny_workspace(16, 768, 768) == 2 * need


@needs_lib
def test_attn_decode_refuses_bad_arguments(lib):
    B, H, Tcap = 2, 4, 256
    ws = lib.gpt2mi_attn_decode_workspace(B, H, Tcap)
    assert ws > 0

    def call(head_dim=64, pos=0, ws_floats=ws, tcap=Tcap):
        return lib.gpt2mi_attn_decode(None, None, None, None, None, ws_floats, B, H, head_dim, tcap, pos, None)
    assert call(head_dim=32) == 22
    assert b"head_dim=32" in lib.gpt2mi_last_error()
    for pos in (-1, Tcap, Tcap + 5):
        assert call(pos=pos) == 22
        assert b"pos=" in lib.gpt2mi_last_error()
    assert call(ws_floats=ws - 1) == 22
    assert b"workspace too small" in lib.gpt2mi_last_error()


@needs_lib
def test_kv_store_refuses_bad_arguments(lib):
    def call(n=64, t0=0, head_dim=64, T_src=64, Tcap=128):
        return lib.gpt2mi_kv_store(None, None, None, 2, T_src, n, t0, 4, head_dim, Tcap, None)
    assert call(head_dim=128) == 22
    assert b"head_dim=128" in lib.gpt2mi_last_error()
    assert call(n=64, t0=65) == 22  # t0 + n > Tcap
    assert b"exceeds the cache length" in lib.gpt2mi_last_error()
    assert call(n=100, T_src=128, t0=29) == 22
    assert call(n=65, T_src=64) == 22  # more rows than a sequence of the buffer has
    assert call(t0=-1) == 22


@needs_lib
def test_embed_decode_and_decode_step_refuse_bad_arguments(lib):
    from gpt_2_distributed_amd import _lib
    import ctypes
    assert lib.gpt2mi_embed_decode(None, None, None, None, 2, 128, -1, None) == 22
    assert b"pos=-1" in lib.gpt2mi_last_error()
    plan = _lib.DecodePlan()
    plan.B, plan.C, plan.H, plan.L, plan.Vp, plan.Tcap = 65, 128, 2, 1, 512, 64

    def step(pos=0):
        return lib.gpt2mi_decode_step(ctypes.byref(plan), None, pos, None)
    assert step() == 22 and b"B=65" in lib.gpt2mi_last_error()
    plan.B, plan.H = 2, 4
    assert step() == 22 and b"head_dim" in lib.gpt2mi_last_error()
    plan.H = 2
    assert step(pos=64) == 22 and b"pos=64" in lib.gpt2mi_last_error()
    assert step(pos=-1) == 22
    assert step() == 22 and b"workspace too small" in lib.gpt2mi_last_error()  # attn_ws_floats = 0
    assert lib.gpt2mi_decode_step(None, None, 0, None) == 22


@needs_lib
def test_abi_is_v14_or_later_and_binds_the_decode_entries(lib):
    from gpt_2_distributed_amd import _lib
    assert lib.gpt2mi_abi_version() == _lib.ABI_VERSION >= 14  # (the decode entries arrived with v14)
    for name in ("gpt2mi_gemm_skinny", "gpt2mi_kv_store", "gpt2mi_attn_decode", "gpt2mi_attn_decode_workspace",
                 "gpt2mi_embed_decode", "gpt2mi_decode_step"):
        assert name in _lib.EXPORTED and hasattr(lib, name)


# ---- register budget -----------------------------------------------------------------------------------------------
@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_decode_kernels_have_no_scratch_and_no_spills():
    """The streaming kernels keep their operands in registers: any scratch use is an HBM round trip per element."""
    kernels = _resources("decode.hip")
    for sub in ("skinny_gemm_kernel", "skinny_reduce_kernel", "attn_combine_kernel", "embed_decode_kernel"):
        assert any(sub in k for k in kernels), f"{sub} not found in decode.hip"
    for family in ("kv_store_kernel", "attn_decode_kernel"):  # (templates over the cache type: the bf16 cache's)
        _instantiation(kernels, family, "KvBf16")
    for k, v in kernels.items():
        assert v["ScratchSize [bytes/lane]"] == 0, f"{k}: scratch {v}"
        assert v["VGPRs Spill"] == 0, f"{k}: spills {v}"
