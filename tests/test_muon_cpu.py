"""Muon without a GPU: the rule against its singular-value polynomial, the matrices Muon owns, the C ABI minor."""
import os
import re

import torch

from tests.conftest import REPO

from gpt_2_distributed_amd.muon import NS_COEFFS, muon_matrices, newton_schulz_reference

ENTRIES = ("gpt2mi_muon_prepare", "gpt2mi_muon_gram", "gpt2mi_muon_poly", "gpt2mi_muon_apply", "gpt2mi_muon_update")


def test_newton_schulz_is_the_quintic_on_the_singular_values():
    """The iteration keeps the singular vectors and maps s to p(s) = a s + b s^3 + c s^5: U diag(p^5(s)) V^T."""
    X = torch.randn(64, 256, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    X = X / (X.norm() + 1e-7)
    U, S, Vh = torch.linalg.svd(X, full_matrices=False)
    a, b, c = NS_COEFFS
    for _ in range(5):
        S = a * S + b * S ** 3 + c * S ** 5
    out = newton_schulz_reference(X, dtype=torch.float64)
    assert out.dtype == torch.float64
    assert torch.allclose(out, U @ torch.diag(S) @ Vh, rtol=0, atol=1e-12)
    got = torch.linalg.svdvals(out)
    assert S.min() - 1e-12 <= got.min() and got.max() <= S.max() + 1e-12


def test_muon_matrices_of_the_tiny_model():
    from gpt_2_distributed_amd.model import GPT2, GPT2Config
    m = GPT2(GPT2Config(n_layer=2, n_head=2, n_embd=128, vocab_size=509, n_positions=64))
    C, owned = 128, muon_matrices(m)
    for i in range(2):
        h = f"transformer.h.{i}."
        assert owned[6 * i:6 * i + 6] == [(h + "attn.qkv.weight", 0, C, C), (h + "attn.qkv.weight", C, C, C),
                                          (h + "attn.qkv.weight", 2 * C, C, C), (h + "attn.proj.weight", 0, C, C),
                                          (h + "mlp.fc1.weight", 0, 4 * C, C), (h + "mlp.fc2.weight", 0, C, 4 * C)]
    assert len(owned) == 12
    seen = torch.zeros(m.layout.total, dtype=torch.int32)  # every listed element once
    for name, r0, rows, cols in owned:
        off = m.layout.slots[name].offset + r0 * cols
        seen[off:off + rows * cols] += 1
    names = {n for n, *_ in owned}
    assert int(seen.max()) == 1 and int(seen.sum()) == sum(m.layout.slots[n].numel for n in names)
    rest = {n for n, _ in m.named_parameters()} - names  # the embeddings, every LayerNorm and every bias
    assert len(rest) == 4 + 2 * 8 and all("wte" in n or "wpe" in n or ".ln" in n or n.endswith(".bias") for n in rest)


def test_abi_minor_carries_the_muon_entries():
    from gpt_2_distributed_amd import _lib
    hdr = open(os.path.join(REPO, "include", "gpt2mi.h")).read()
    minor = int(re.search(r"#define GPT2MI_ABI_MINOR (\d+)", hdr).group(1))
    lib = _lib.load()
    assert minor == lib.gpt2mi_abi_minor() == _lib.ABI_MINOR and minor >= 8
    for name in ENTRIES:
        assert name in _lib.EXPORTED and hasattr(lib, name) and name + "(" in hdr and _lib._SINCE_MINOR[name] == 8
