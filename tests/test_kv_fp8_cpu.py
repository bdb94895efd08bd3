"""The fp8 key/value cache without a GPU: the quantiser's rule (generation.kv_quantize / kv_dequantize, which the
kernels of csrc/decode.hip are held to bit for bit in tests/test_kv_fp8_kernels_gpu.py) on random and constructed rows,
the argument checks of the v23 entries (through the built library with NULL pointers: nothing is launched) and the
register budget of the new kernels."""
import ctypes
import math
import os
import shutil

import pytest
import torch

from gpt_2_distributed_amd.generation import check_kv_dtype, kv_dequantize, kv_quantize
from tests.conftest import REPO
from tests.test_kernel_resources import HIPCC, _instantiation, _resources

LIB = os.path.join(REPO, "gpt_2_distributed_amd", "libgpt2mi.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libgpt2mi.so not built (run __graft_entry__.build())")
BF16 = torch.bfloat16


# ---- rows -------------------------------------------------------------------------------------------------------------
def constructed_rows() -> dict:
    """The named edge rows, bf16 [64] each (tests/test_kv_fp8_kernels_gpu.py mixes them into its inputs)."""
    g = torch.Generator().manual_seed(5)
    small = torch.randn(64, generator=g)
    rows = {
        "zeros": torch.zeros(64),
        "amax_1.75": torch.cat([torch.tensor([1.75 * 2.0 ** 3]), small[1:] * 0.5]),        # 448 * 2^-5: no bump
        "amax_1.7578125": torch.cat([torch.tensor([1.7578125 * 2.0 ** 3]), small[1:] * 0.5]),  # the next bf16: e bumps
        "outlier": torch.cat([small[:17].clamp(-1.8, 1.8), torch.tensor([3e4]), small[18:].clamp(-1.8, 1.8)]),
        "negative_amax": torch.cat([small[:40] * 0.1, torch.tensor([-5.5]), small[41:] * 0.1]),
        # amax 1: scale 2^-8, a subnormal step is 2^-9 scale; then 1/2, -1/2 and 3/2 steps
        "tie": torch.cat([torch.tensor([1.0, 2.0 ** -18, -(2.0 ** -18), 3 * 2.0 ** -18]), torch.zeros(60)]),
        "tiny": small * 2.0 ** -120,                                                       # e clamps at -100
        "huge": small * 2.0 ** 120,
    }
    return {k: v.to(BF16) for k, v in rows.items()}


def random_rows(n=4000, seed=0) -> torch.Tensor:
    """bf16 [n, 64] at magnitudes from 2^-20 to 2^20 per row, a few entries zeroed."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 64, generator=g) * 2.0 ** torch.randint(-20, 21, (n, 1), generator=g).float()
    x[torch.rand(n, 64, generator=g) < 0.05] = 0.0
    return x.to(BF16)


def exponent_by_frexp(amax: float) -> int:
    """The scale exponent of the rule, from math.frexp: the smallest e >= -100 with amax <= 448 * 2^e."""
    if amax == 0:
        return -100
    f, ex = math.frexp(amax)  # amax = f 2^ex, f in [0.5, 1)
    e = ex - 9 + (1 if f > 0.875 else 0)
    assert amax <= 448 * 2.0 ** e and (amax > 448 * 2.0 ** (e - 1))  # (the smallest such e, before the clamp)
    return max(e, -100)


def all_rows() -> torch.Tensor:
    return torch.cat([torch.stack(list(constructed_rows().values())), random_rows()])


# ---- the quantiser's properties -------------------------------------------------------------------------------------
def test_scale_is_the_smallest_power_of_two_that_holds_amax():
    x = all_rows()
    codes, scale = kv_quantize(x)
    assert codes.dtype == torch.uint8 and codes.shape == x.shape
    assert scale.dtype == torch.float32 and scale.shape == x.shape[:-1]
    amax = x.float().abs().amax(-1)
    for a, s in zip(amax.tolist(), scale.tolist()):
        f, ex = math.frexp(s)
        assert f == 0.5, s  # a power of two
        assert ex - 1 == exponent_by_frexp(a), (a, s)
        assert a <= 448 * s


def test_no_nan_code_and_the_error_bound():
    x = all_rows()
    codes, scale = kv_quantize(x)
    assert not bool(((codes & 0x7F) == 0x7F).any())  # 0x7F / 0xFF: e4m3fn's NaN
    xf = x.double()
    back = kv_dequantize(codes, scale)
    assert back.dtype == torch.float32
    # 3 mantissa bits under RNE: half an ulp is 2^-4 relative; below the normal range half a subnormal step, 2^-10 scale
    bound = torch.maximum(2.0 ** -4 * xf.abs(), 2.0 ** -10 * scale.double()[:, None])
    assert bool(((xf - back.double()).abs() <= bound).all())
    assert torch.equal(back.to(BF16).float(), back)  # every dequantised value is a bf16 number


def test_rows_on_the_grid_round_trip_exactly():
    g = torch.Generator().manual_seed(9)
    codes = torch.randint(0, 256, (500, 64), generator=g).to(torch.uint8)
    codes[(codes & 0x7F) == 0x7F] = 0x11
    codes[:, 0] = 0x7E  # 448: the row's amax sits at the top of the grid, so its scale comes back
    scale = 2.0 ** torch.randint(-100, 100, (500,), generator=g).float()
    x = kv_dequantize(codes, scale)
    assert torch.equal(x.to(BF16).float(), x)
    c2, s2 = kv_quantize(x.to(BF16))
    assert torch.equal(s2, scale)
    assert torch.equal(kv_dequantize(c2, s2), x)
    assert torch.equal(c2 & 0x7F, codes & 0x7F) and torch.equal((c2 >> 7)[codes & 0x7F != 0], (codes >> 7)[codes & 0x7F != 0])


def test_constructed_rows():
    rows = constructed_rows()
    q = {k: kv_quantize(v) for k, v in rows.items()}
    codes, scale = q["zeros"]
    assert not bool(codes.any()) and float(scale) == 2.0 ** -100
    codes, scale = q["amax_1.75"]
    assert int(codes[0]) == 0x7E and float(scale) == 2.0 ** -5  # 14 = 448 * 2^-5 exactly: no bump
    codes, scale = q["amax_1.7578125"]
    assert float(scale) == 2.0 ** -4 and int(codes[0]) == 0x76  # 14.0625 * 16 = 225 -> 224 = 1.75 * 2^7
    codes, scale = q["outlier"]
    assert float(scale) == 2.0 ** 7  # 3e4 = 1.83 * 2^14: e = 14 - 8 + 1
    others = torch.cat([codes[:17], codes[18:]])
    assert bool(((others & 0x7F) < 0x08).all())  # O(1) values / 128: subnormal codes (exponent field 0) or zero
    assert bool(((others & 0x7F) > 0).any())
    codes, scale = q["negative_amax"]
    assert float(scale) == 2.0 ** -6 and int(codes[40]) == 0x80 | 0x7B  # -5.5 * 64 = -352 = -1.375 * 2^8
    codes, scale = q["tie"]
    assert float(scale) == 2.0 ** -8 and int(codes[0]) == 0x78  # 256 = 2^8
    assert int(codes[1]) == 0x00 and int(codes[2]) == 0x80  # 2^-10 scale, half a step: to even, code 0 (the sign stays)
    assert int(codes[3]) == 0x02                            # one and a half steps: to even, 2
    codes, scale = q["tiny"]
    assert float(scale) == 2.0 ** -100 and not bool((codes & 0x7F).any())
    assert float(q["huge"][1]) <= 2.0 ** 120


def test_quantise_is_a_function_of_the_row():
    x = random_rows(64, seed=3)
    codes, scale = kv_quantize(x.view(2, 4, 8, 64))
    for i in (0, 17, 63):
        c, s = kv_quantize(x[i])
        assert torch.equal(c, codes.view(64, 64)[i]) and torch.equal(s, scale.view(64)[i])
    with pytest.raises(ValueError):
        kv_quantize(torch.zeros(4, 32))


def test_kv_dtype_names():
    assert check_kv_dtype("bf16") == 0 and check_kv_dtype("fp8") == 1
    for bad in ("int4", "fp16", None, 1):
        with pytest.raises(ValueError, match="bf16.*fp8"):
            check_kv_dtype(bad)


def test_generate_refuses_an_unknown_kv_dtype_before_anything_else():
    """The keyword is checked first, so the refusal needs neither a GPU nor a model."""
    from gpt_2_distributed_amd import generation
    with pytest.raises(ValueError, match="int4"):
        generation.generate(None, torch.zeros(1, 3, dtype=torch.int64), 4, kv_dtype="int4")
    with pytest.raises(ValueError, match="int4"):
        generation.generate_many(None, [torch.zeros(3, dtype=torch.int64)], 4, kv_dtype="int4")
    with pytest.raises(ValueError, match="int4"):
        generation.DecodeSession(None, 1, kv_dtype="int4")


# ---- argument checks of the C entries (no launch: every pointer is NULL) -------------------------------------------
@pytest.fixture()
def lib():
    from gpt_2_distributed_amd import _lib
    return _lib.load()


B, H, TCAP = 2, 4, 256


@needs_lib
def test_abi_is_v23_or_later_and_binds_the_fp8_entries(lib):
    from gpt_2_distributed_amd import _lib
    assert lib.gpt2mi_abi_version() == _lib.ABI_VERSION >= 23
    for name in ("gpt2mi_kv_store_fp8", "gpt2mi_attn_decode_fp8_ragged", "gpt2mi_attn_extend_fp8"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    # appended behind `rows`, in the struct's former tail padding: no earlier offset moved, the size did not change
    assert _lib.DecodePlan.KV_FORMAT_OFFSET == _lib.DecodePlan.rows.offset + 4
    assert _lib.DecodePlan.KV_FORMAT_OFFSET + 4 <= ctypes.sizeof(_lib.DecodePlan)
    plan = _lib.DecodePlan()
    assert plan.kv_format == 0 and plan.rows == 0
    plan.kv_format = 1
    assert (plan.kv_format, plan.rows, plan.logits) == (1, 0, None)
    assert [n for n, _ in _lib.DecodeLayer._fields_][-4:] == ["kcache", "vcache", "kscale", "vscale"]


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


@needs_lib
def test_kv_store_fp8_refuses_bad_arguments(lib):
    def call(n=64, t0=0, head_dim=64, T_src=64, Tcap=128):
        return lib.gpt2mi_kv_store_fp8(None, None, None, None, None, 2, T_src, n, t0, 4, head_dim, Tcap, None)
    assert call(head_dim=128) == 22
    assert b"kv_store_fp8: head_dim=128" in lib.gpt2mi_last_error()
    assert call(n=64, t0=65) == 22
    assert b"exceeds the cache length" in lib.gpt2mi_last_error()
    assert call(n=65, T_src=64) == 22
    assert call(t0=-1) == 22
    assert call() == 22  # the shapes are fine: the scales are NULL
    assert b"kscale and vscale" in lib.gpt2mi_last_error()


@needs_lib
def test_attn_decode_fp8_ragged_refuses_bad_arguments(lib):
    ws = lib.gpt2mi_attn_decode_workspace(B, H, TCAP)

    def call(head_dim=64, pos=(0, 5), ws_floats=ws):
        return lib.gpt2mi_attn_decode_fp8_ragged(None, None, None, None, None, None, None, ws_floats, B, H, head_dim,
                                                 TCAP, _ints(pos), None)
    assert call(head_dim=32) == 22
    assert b"attn_decode_fp8_ragged: head_dim=32" in lib.gpt2mi_last_error()
    for pos in ((0, TCAP), (-1, 0)):
        assert call(pos=pos) == 22
        assert b"pos[" in lib.gpt2mi_last_error()
    assert call(ws_floats=ws - 1) == 22
    assert b"workspace too small" in lib.gpt2mi_last_error()
    assert call() == 22
    assert b"kscale and vscale" in lib.gpt2mi_last_error()
    assert lib.gpt2mi_attn_decode_fp8_ragged(None, None, None, None, None, None, None, ws, B, H, 64, TCAP, None,
                                             None) == 22


@needs_lib
def test_attn_extend_fp8_refuses_bad_arguments(lib):
    R = 4
    ws = lib.gpt2mi_attn_decode_workspace(R, H, TCAP)

    def call(head_dim=64, seq=(0, 0, 1, 1), pos=(3, 4, 0, 1), ws_floats=ws):
        return lib.gpt2mi_attn_extend_fp8(None, None, None, None, None, None, None, ws_floats, R, B, H, head_dim, TCAP,
                                          _ints(seq), _ints(pos), None)
    assert call(head_dim=128) == 22
    assert b"attn_extend_fp8: head_dim=128" in lib.gpt2mi_last_error()
    assert call(pos=(TCAP - 1, TCAP, 0, 1)) == 22
    assert b"pos[1]" in lib.gpt2mi_last_error()
    assert call(pos=(3, 5, 0, 1)) == 22
    assert b"does not follow" in lib.gpt2mi_last_error()
    assert call(seq=(0, 0, 2, 2)) == 22
    assert call(ws_floats=ws - 1) == 22
    assert b"workspace too small" in lib.gpt2mi_last_error()
    assert call() == 22
    assert b"kscale and vscale" in lib.gpt2mi_last_error()


def _plan(K, L=2):
    """A plan whose integer fields pass every check and whose buffers are NULL, with its host layer array."""
    layers = (K.DecodeLayer * L)()
    plan = K.DecodePlan()
    plan.B, plan.C, plan.H, plan.L, plan.Vp, plan.Tcap = 2, 128, 2, L, 512, 64
    plan.layers = ctypes.cast(layers, ctypes.POINTER(K.DecodeLayer))
    plan.attn_ws_floats = plan.gemm_ws_floats = 1 << 30
    return plan, layers


@needs_lib
def test_plan_kv_format_is_checked_by_every_plan_entry(lib):
    from gpt_2_distributed_amd import _lib as K
    plan, layers = _plan(K)
    assert plan.kv_format == 0  # a zero-initialised plan still means bf16 ...
    pos, seq = _ints([1, 1]), _ints([0, 1])
    entries = {
        "decode_step": lambda: lib.gpt2mi_decode_step(ctypes.byref(plan), None, 1, None),
        "decode_step_ragged": lambda: lib.gpt2mi_decode_step_ragged(ctypes.byref(plan), None, pos, None),
        "decode_extend": lambda: lib.gpt2mi_decode_extend(ctypes.byref(plan), 2, None, seq, pos, None),
    }
    for name, call in entries.items():
        plan.kv_format = 0
        assert call() == 22 and b"layers and tok must not be NULL" in lib.gpt2mi_last_error(), name  # ... and passes
        plan.kv_format = 2
        assert call() == 22 and b"kv_format=2" in lib.gpt2mi_last_error(), name
        plan.kv_format = -1
        assert call() == 22 and b"kv_format=-1" in lib.gpt2mi_last_error(), name
        plan.kv_format = 1  # fp8 with NULL scales
        assert call() == 22 and b"kscale" in lib.gpt2mi_last_error(), name
        layers[0].kscale = layers[0].vscale = 64  # (never dereferenced: the next layer's are still NULL)
        assert call() == 22 and b"layers[1].kscale" in lib.gpt2mi_last_error(), name
        layers[0].kscale = layers[0].vscale = None


@needs_lib
def test_generate_entries_check_kv_format_before_the_first_draw(lib):
    """The loops sample before they step: the plan check must not wait for the first step. Reaching it needs non-NULL
    tok and logits, which nothing dereferences before the refusal: a host buffer stands in."""
    from gpt_2_distributed_amd import _lib as K
    plan, layers = _plan(K)
    buf = (ctypes.c_int64 * 8)()
    plan.logits = ctypes.addressof(buf)
    pos0 = _ints([1, 1])
    tok = ctypes.cast(buf, ctypes.c_void_p)

    def loops():
        yield "decode_generate", lib.gpt2mi_decode_generate(ctypes.byref(plan), 500, 1.0, 0, 1.0, 0, -1, 1, 2, tok, None,
                                                             0, None, None)
        yield "decode_generate_ragged", lib.gpt2mi_decode_generate_ragged(ctypes.byref(plan), 500, 1.0, 0, 1.0, 0, -1,
                                                                           pos0, None, 2, tok, None, 0, None, None)
        yield "decode_generate_penalized", lib.gpt2mi_decode_generate_penalized(
            ctypes.byref(plan), 500, 1.0, 0, 1.0, 0, -1, pos0, None, 2, tok, None, 0, None, None, 1.0, 0.0, 0.0, None)
    plan.kv_format = 2
    for name, rc in loops():
        assert rc == 22 and b"kv_format=2" in lib.gpt2mi_last_error(), name
    plan.kv_format = 1
    for name, rc in loops():
        assert rc == 22 and b"kscale" in lib.gpt2mi_last_error(), name


# ---- register budget -----------------------------------------------------------------------------------------------
@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_fp8_kernels_have_no_scratch_and_no_spills():
    kernels = _resources("decode.hip")
    for family in ("kv_store_kernel", "attn_decode_kernel", "attn_extend_kernel"):
        k, v = _instantiation(kernels, family, "KvFp8")
        assert v["ScratchSize [bytes/lane]"] == 0, f"{k}: scratch {v}"
        assert v["VGPRs Spill"] == 0, f"{k}: spills {v}"
