"""C ABI v24 without a GPU: the share map (share_group, share_len) of gpt2mi_attn_decode_shared and of a plan is checked
before any launch. Every device pointer is NULL, so an accepted map is refused by the first later check and nothing runs."""
import ctypes
import os
import re

import pytest

from tests.conftest import REPO

HEADER = os.path.join(REPO, "include", "gpt2mi.h")
LIB = os.path.join(REPO, "gpt_2_distributed_amd", "libgpt2mi.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libgpt2mi.so not built (run __graft_entry__.build())")

B, H, TCAP = 5, 2, 160
POS = (100, 100, 100, 100, 100)
GROUP, LEN = (0, 1, 0, 0, 4), (70, 0, 70, 70, 0)  # rows {0, 2, 3} share 70 positions, rows 1 and 4 are alone

# (share_group, share_len, pos, the index the message names, words of the message)
MALFORMED = {
    "group_above_row": ((0, 2, 0, 0, 4), LEN, POS, 1, b"share_group[1]=2 not in [0, 1]"),
    "group_negative": ((0, 1, -1, 0, 4), LEN, POS, 2, b"share_group[2]=-1 not in [0, 2]"),
    "group_not_lowest": ((0, 1, 0, 2, 4), LEN, POS, 3, b"share_group[3]=2 is not its group's lowest row"),
    "len_negative": (GROUP, (70, -1, 70, 70, 0), POS, 1, b"share_len[1]=-1 is negative"),
    "len_above_pos": (GROUP, LEN, (100, 100, 69, 100, 100), 2, b"share_len[2]=70 exceeds pos[2]=69"),
    "len_differs": (GROUP, (70, 0, 70, 64, 0), POS, 3, b"share_len[3]=64 differs from its group's share_len[0]=70"),
    "len_of_a_row_alone": (GROUP, (70, 0, 70, 70, 8), POS, 4, b"share_len[4]=8 for a row alone"),
}


def _ints(v):
    return None if v is None else (ctypes.c_int * len(v))(*v)


@pytest.fixture()
def lib():
    from gpt_2_distributed_amd import _lib
    return _lib.load()


@needs_lib
def test_abi_is_v24_and_binds_the_shared_entries(lib):
    from gpt_2_distributed_amd import _lib
    hdr = re.search(r"#define GPT2MI_ABI_VERSION (\d+)", open(HEADER).read())
    assert lib.gpt2mi_abi_version() == _lib.ABI_VERSION == int(hdr.group(1)) == 24
    for name in ("gpt2mi_attn_decode_shared", "gpt2mi_attn_decode_shared_fp8"):
        assert name in _lib.EXPORTED and hasattr(lib, name)


def test_plan_appends_the_two_pointers_and_moves_nothing():
    """The C struct grew by two pointers behind kv_format; the ctypes field list is still v21's, an instance lies over a
    zeroed buffer of the C size and the new fields are properties over its tail."""
    from gpt_2_distributed_amd import _lib as K
    assert K.DecodePlan.SHARE_GROUP_OFFSET == ctypes.sizeof(K.DecodePlan) >= K.DecodePlan.KV_FORMAT_OFFSET + 4
    assert K.DecodePlan.SHARE_GROUP_OFFSET % ctypes.sizeof(ctypes.c_void_p) == 0
    assert K.DecodePlan.SHARE_LEN_OFFSET == K.DecodePlan.SHARE_GROUP_OFFSET + 8
    assert K.DecodePlan.PLAN_BYTES == K.DecodePlan.SHARE_LEN_OFFSET + 8
    plan = K.DecodePlan()
    assert (plan.share_group, plan.share_len, plan.rows, plan.kv_format) == (None, None, 0, 0)
    sg, sl = _ints(GROUP), _ints(LEN)
    plan.set_share(sg, sl)
    plan.kv_format, plan.rows = 1, 7
    assert (plan.share_group, plan.share_len) == (ctypes.addressof(sg), ctypes.addressof(sl))
    assert (plan.kv_format, plan.rows, plan.logits) == (1, 7, None)
    plan.set_share(None, None)
    assert (plan.share_group, plan.share_len) == (None, None)
    with pytest.raises(K.KernelError):
        plan.set_share(sg, None)
    # the header: the two fields are the last of the struct, behind kv_format
    body = re.search(r"typedef struct gpt2mi_decode_plan \{(.*?)\} gpt2mi_decode_plan;", open(HEADER).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert fields[-3:] == ["int kv_format", "const int* share_group", "const int* share_len"]


def test_a_plan_without_the_tail_is_refused_by_the_bindings():
    """ctypes.sizeof(DecodePlan) is 16 bytes short of the C struct, so an object that DecodePlan() did not make (an array
    element, a from_buffer_copy) must not reach the library, which would read past its end: ``ref()``, through which
    every binding passes its plan, refuses it, and so do the tail's properties."""
    import copy
    from gpt_2_distributed_amd import _lib as K
    assert K.DecodePlan.PLAN_BYTES == ctypes.sizeof(K.DecodePlan) + 16
    assert K.DecodePlan().ref() is not None
    short = [(K.DecodePlan * 2)()[1], K.DecodePlan.from_buffer_copy(bytes(ctypes.sizeof(K.DecodePlan)))]
    for plan in short:
        with pytest.raises(K.KernelError, match="DecodePlan\\(\\)"):
            plan.ref()
        with pytest.raises(K.KernelError):
            plan.share_group
        with pytest.raises(K.KernelError):
            plan.set_share(_ints(GROUP), _ints(LEN))
        with pytest.raises(K.KernelError):  # refused before the library is so much as loaded
            K.decode_step(plan, None, 0)
    with pytest.raises(ValueError):  # (ctypes itself refuses to copy a structure that holds pointers)
        copy.copy(K.DecodePlan())


def _attn(lib, fp8, group, length, pos=POS, ws=None):
    ws = lib.gpt2mi_attn_decode_workspace(B, H, TCAP) if ws is None else ws
    if fp8:
        return lib.gpt2mi_attn_decode_shared_fp8(None, None, None, None, None, None, None, ws, B, H, 64, TCAP, _ints(pos),
                                                 _ints(group), _ints(length), None)
    return lib.gpt2mi_attn_decode_shared(None, None, None, None, None, ws, B, H, 64, TCAP, _ints(pos), _ints(group),
                                         _ints(length), None)


@needs_lib
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_attn_decode_shared_refuses_a_malformed_map(lib, case, fp8):
    group, length, pos, index, words = MALFORMED[case]
    name = b"attn_decode_shared_fp8: " if fp8 else b"attn_decode_shared: "
    assert _attn(lib, fp8, group, length, pos) == 22
    msg = lib.gpt2mi_last_error()
    assert msg.startswith(name) and words in msg and b"[%d]" % index in msg, msg


@needs_lib
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_attn_decode_shared_takes_both_arrays_or_neither(lib, fp8):
    assert _attn(lib, fp8, GROUP, None) == 22
    assert b"share_len is NULL" in lib.gpt2mi_last_error()
    assert _attn(lib, fp8, None, LEN) == 22
    assert b"share_group is NULL" in lib.gpt2mi_last_error()
    later = b"kscale and vscale" if fp8 else b"must not be NULL"
    for group, length in ((None, None), (GROUP, LEN), ((0, 1, 2, 3, 4), (0, 0, 0, 0, 0)), ((0, 0, 0, 0, 0), (100,) * 5)):
        assert _attn(lib, fp8, group, length) == 22  # the map passes: the first later check refuses the NULL pointers
        assert later in lib.gpt2mi_last_error(), (group, length, lib.gpt2mi_last_error())
    # the position checks come first, as in attn_decode_ragged, and the workspace check after the map
    assert _attn(lib, fp8, GROUP, LEN, pos=(100, 100, 100, 100, TCAP)) == 22
    assert b"pos[4]" in lib.gpt2mi_last_error()
    assert _attn(lib, fp8, GROUP, LEN, ws=lib.gpt2mi_attn_decode_workspace(B, H, TCAP) - 1) == 22
    assert b"workspace too small" in lib.gpt2mi_last_error()


def _plan(K, L=2):
    layers = (K.DecodeLayer * L)()
    plan = K.DecodePlan()
    plan.B, plan.C, plan.H, plan.L, plan.Vp, plan.Tcap = B, 128, 2, L, 512, TCAP
    plan.layers = ctypes.cast(layers, ctypes.POINTER(K.DecodeLayer))
    plan.attn_ws_floats = plan.gemm_ws_floats = 1 << 30
    return plan, layers


@needs_lib
@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_plan_entries_refuse_a_malformed_map(lib, case):
    from gpt_2_distributed_amd import _lib as K
    group, length, pos, index, words = MALFORMED[case]
    plan, layers = _plan(K)
    sg, sl, pos_a = _ints(group), _ints(length), _ints(pos)
    plan.set_share(sg, sl)
    buf = (ctypes.c_int64 * 8)()  # stands in for tok and logits: nothing dereferences them before the refusal
    plan.logits = ctypes.addressof(buf)
    tok = ctypes.cast(buf, ctypes.c_void_p)
    calls = {
        b"decode_step_ragged": lambda: lib.gpt2mi_decode_step_ragged(ctypes.byref(plan), None, pos_a, None),
        b"decode_generate_ragged": lambda: lib.gpt2mi_decode_generate_ragged(
            ctypes.byref(plan), 500, 1.0, 0, 1.0, 0, -1, pos_a, None, 2, tok, None, 0, None, None),
        b"decode_generate_penalized": lambda: lib.gpt2mi_decode_generate_penalized(
            ctypes.byref(plan), 500, 1.0, 0, 1.0, 0, -1, pos_a, None, 2, tok, None, 0, None, None, 1.0, 0.0, 0.0, None),
    }
    for name, call in calls.items():
        assert call() == 22
        msg = lib.gpt2mi_last_error()
        assert msg.startswith(name + b": ") and words in msg and b"[%d]" % index in msg, msg


@needs_lib
def test_plan_map_is_optional_and_the_extend_ignores_it(lib):
    from gpt_2_distributed_amd import _lib as K
    plan, layers = _plan(K)
    pos_a = _ints(POS)
    step = lambda: lib.gpt2mi_decode_step_ragged(ctypes.byref(plan), None, pos_a, None)  # noqa: E731
    same = lambda: lib.gpt2mi_decode_step(ctypes.byref(plan), None, 100, None)  # noqa: E731
    for call in (step, same):
        assert call() == 22 and b"layers and tok must not be NULL" in lib.gpt2mi_last_error()  # both NULL: v23
    sg, sl = _ints(GROUP), _ints(LEN)
    plan.set_share(sg, sl)
    for call in (step, same):
        assert call() == 22 and b"layers and tok must not be NULL" in lib.gpt2mi_last_error()  # a good map passes
    sl[3] = 64
    for call, name in ((step, b"decode_step_ragged: "), (same, b"decode_step: ")):
        assert call() == 22 and lib.gpt2mi_last_error().startswith(name + b"share_len[3]=64")
    seq, pos = _ints([0, 1]), _ints([100, 100])
    assert lib.gpt2mi_decode_extend(ctypes.byref(plan), 2, None, seq, pos, None) == 22
    assert b"layers and tok must not be NULL" in lib.gpt2mi_last_error()  # the malformed map is not looked at
