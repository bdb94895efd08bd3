"""ABI v24.9 (prefill over a live cache) without a device: the bindings' argument lists against the header."""
import os
import re

from tests.conftest import REPO

NEW = ("gpt2mi_attn_chunk", "gpt2mi_attn_chunk_fp8", "gpt2mi_attn_chunk_workspace", "gpt2mi_attn_chunk_splits",
       "gpt2mi_embed_fwd_at")


def test_bindings_match_the_header():
    from gpt_2_distributed_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gpt2mi.h")).read(), flags=re.S)
    assert int(re.search(r"#define GPT2MI_ABI_MINOR (\d+)", hdr).group(1)) == _lib.ABI_MINOR == 9
    for name in NEW:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1).split(",")
        assert len(args) == len(_lib._SIGS[name]) and _lib._SINCE_MINOR[name] == 9, name
        for decl, ctype in zip(args, _lib._SIGS[name]):  # a pointer where the header has one, and nowhere else
            assert ("*" in decl) == (ctype is _lib._p), (name, decl)
    # the fp8 form is the bf16 list with (kscale, vscale) behind the caches
    assert len(_lib._SIGS["gpt2mi_attn_chunk_fp8"]) == len(_lib._SIGS["gpt2mi_attn_chunk"]) + 2
    assert _lib._FP8_ENTRY["gpt2mi_attn_chunk"] == "gpt2mi_attn_chunk_fp8"
    assert _lib._RESTYPES["gpt2mi_attn_chunk_workspace"] is _lib._c_size
