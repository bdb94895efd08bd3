"""Device-side sampling without a GPU: the hash behind the draw, the PyTorch statements of the sampling rule
(sample_next with top_p, sample_reference), the argument checks of gpt2mi_sample / gpt2mi_decode_generate (NULL
pointers: nothing is launched) and the register budget of csrc/sample.hip."""
import ctypes
import inspect
import os
import shutil

import pytest
import torch

from gpt_2_distributed_amd import generation
from gpt_2_distributed_amd.generation import sample_next, sample_reference, uniform_at
from tests.conftest import REPO
from tests.test_kernel_resources import HIPCC, _resources

LIB = os.path.join(REPO, "gpt_2_distributed_amd", "libgpt2mi.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libgpt2mi.so not built (run __graft_entry__.build())")


def _logits(B=6, V=50, seed=0):
    return torch.randn(B, V, generator=torch.Generator().manual_seed(seed)) * 3


# ---- uniform_at ------------------------------------------------------------------------------------------------------
def test_uniform_at_is_a_pure_function_of_seed_row_and_position():
    a = [uniform_at(3, b, p) for b in range(4) for p in range(8)]
    assert a == [uniform_at(3, b, p) for b in range(4) for p in range(8)]
    assert all(0.0 <= u < 1.0 and u * 2 ** 24 == int(u * 2 ** 24) for u in a)  # 24 bits in [0, 1)
    assert len(set(a)) == len(a)                                                # distinct across b and pos
    assert uniform_at(3, 1, 0) != uniform_at(3, 0, 1)                           # (b, pos) is not b + pos
    assert len({uniform_at(s, 2, 5) for s in range(64)}) == 64                  # distinct across seeds
    # the constants of the contract (include/gpt2mi.h), restated
    c = (7 + 0x9E3779B97F4A7C15 * (1 + ((2 << 32) | 9))) % 2 ** 64
    c ^= c >> 30
    c = c * 0xBF58476D1CE4E5B9 % 2 ** 64
    c ^= c >> 27
    c = c * 0x94D049BB133111EB % 2 ** 64
    c ^= c >> 31
    assert uniform_at(7, 2, 9) == (c >> 40) / 2 ** 24


def test_uniform_at_is_uniform():
    """64 bins over 65,536 draws (64 rows x 1024 positions): chi-square below 120, the 1e-5 tail of 63 degrees of
    freedom; and adjacent draws uncorrelated."""
    u = torch.tensor([uniform_at(0, b, p) for b in range(64) for p in range(1024)], dtype=torch.float64)
    counts = torch.bincount((u * 64).long(), minlength=64).double()
    chi2 = float(((counts - 1024) ** 2 / 1024).sum())
    corr = float(torch.corrcoef(torch.stack([u[:-1], u[1:]]))[0, 1])
    print(f"chi2 {chi2:.1f}, adjacent correlation {corr:.4f}")
    assert chi2 < 120
    assert abs(corr) < 0.02  # 5 / sqrt(65536)


# ---- sample_next -----------------------------------------------------------------------------------------------------
def _sample_next_before(logits, temperature=1.0, top_k=None, generator=None):
    """sample_next as it was before top_p existed, statement for statement."""
    logits = logits.float()
    if temperature == 0:
        return logits.argmax(dim=-1)
    logits = logits / temperature
    if top_k is not None and top_k < logits.size(-1):
        kth = torch.topk(logits, top_k, dim=-1).values[:, -1:]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    probs = torch.softmax(logits, dim=-1)
    return torch.multinomial(probs, num_samples=1, generator=generator).squeeze(1)


@pytest.mark.parametrize("temperature,top_k", [(1.0, None), (0.7, 20), (1.5, 1), (0.0, None)])
def test_sample_next_without_top_p_is_bit_identical_to_before(temperature, top_k):
    lg = _logits(B=8, V=100, seed=4)
    g1, g2 = torch.Generator().manual_seed(12), torch.Generator().manual_seed(12)
    for _ in range(5):
        assert torch.equal(sample_next(lg, temperature, top_k, g1), _sample_next_before(lg, temperature, top_k, g2))
    assert torch.equal(g1.get_state(), g2.get_state())  # the same number of draws taken from the generator
    assert list(inspect.signature(sample_next).parameters)[:4] == ["logits", "temperature", "top_k", "generator"]
    assert inspect.signature(sample_next).parameters["top_p"].default is None


def test_sample_next_top_p_draws_stay_in_the_nucleus():
    p = torch.tensor([0.4, 0.3, 0.2, 0.06, 0.04])
    lg = p.log().repeat(500, 1)
    g = torch.Generator().manual_seed(1)
    seen = torch.bincount(sample_next(lg, 1.0, None, g, top_p=0.75), minlength=5)
    assert seen[3] == 0 and seen[4] == 0 and (seen[:3] > 0).all()  # 0.4 + 0.3 < 0.75 keeps the third token too
    assert torch.equal(sample_next(lg, 1.0, None, g, top_p=1e-6), torch.zeros(500, dtype=torch.long))
    for bad in (0.0, -0.5, float("nan")):
        with pytest.raises(ValueError):
            sample_next(lg, top_p=bad)


# ---- sample_reference ------------------------------------------------------------------------------------------------
def test_reference_top1_and_tiny_top_p_are_the_argmax():
    lg = _logits(B=6, V=300, seed=2)
    u = torch.tensor([uniform_at(5, b, 3) for b in range(6)])
    for kw in (dict(top_k=1, top_p=None), dict(top_k=None, top_p=1e-6), dict(top_k=1, top_p=0.5)):
        tok, probs = sample_reference(lg, 0.8, kw["top_k"], kw["top_p"], u)
        assert torch.equal(tok, lg.argmax(-1))
        assert torch.equal(probs, torch.zeros(6, 300, dtype=torch.float64).scatter_(1, tok[:, None], 1.0))
    tok, _ = sample_reference(lg, 0.0, None, None, u)
    assert torch.equal(tok, lg.argmax(-1))
    dup = lg.clone()
    dup[:, 200] = dup[:, 17] = lg.max() + 1  # greedy with a duplicated maximum: the lowest index
    assert sample_reference(dup, 0.0, None, None, u)[0].tolist() == [17] * 6


def test_reference_keeps_every_tie_at_the_kth_value():
    lg = _logits(B=1, V=40, seed=3)
    order = lg[0].argsort(descending=True)
    lg[0, order[4]] = lg[0, order[5]] = lg[0, order[3]]  # ranks 4, 5, 6 are equal
    _, probs = sample_reference(lg, 1.3, 4, None, torch.tensor([0.5]))
    assert sorted(probs[0].nonzero().flatten().tolist()) == sorted(order[:6].tolist())
    _, probs = sample_reference(lg, 1.3, 3, None, torch.tensor([0.5]))
    assert sorted(probs[0].nonzero().flatten().tolist()) == sorted(order[:3].tolist())
    assert abs(float(probs.sum()) - 1) < 1e-12


@pytest.mark.parametrize("top_k,top_p", [(None, 0.9), (30, 0.6), (None, 0.3)])
def test_reference_nucleus_matches_a_brute_force_sort(top_k, top_p):
    lg = _logits(B=5, V=200, seed=6)
    lg[2, 50] = lg[2, 60] = lg[2].max()  # a tie at the top
    T = 0.9
    u = torch.tensor([uniform_at(1, b, 0) for b in range(5)])
    tok, probs = sample_reference(lg, T, top_k, top_p, u)
    for b in range(5):
        x = [float(v) for v in (lg[b] / T)]
        kept = list(range(200))
        if top_k is not None:
            kth = sorted(x, reverse=True)[top_k - 1]
            kept = [i for i in kept if x[i] >= kth]
        m = max(x)
        w = {i: torch.tensor(x[i] - m, dtype=torch.float64).exp().item() for i in kept}
        z = sum(w.values())
        nucleus = [i for i in kept if sum(w[j] for j in kept if x[j] > x[i]) / z < top_p]
        assert sorted(probs[b].nonzero().flatten().tolist()) == sorted(nucleus)
        zk = sum(w[i] for i in nucleus)
        acc, want = 0.0, None
        for i in sorted(nucleus):  # inverse CDF in vocabulary order
            acc += w[i] / zk
            if acc > float(u[b]):
                want = i
                break
        assert int(tok[b]) == want
        assert abs(float(probs[b, want]) - w[want] / zk) < 1e-12


# ---- argument checks of the C entries (no launch) ----------------------------------------------------------------------
@pytest.fixture()
def lib():
    from gpt_2_distributed_amd import _lib
    return _lib.load()


def _sample(lib, ldl=50432, B=1, V=50257, temperature=1.0, top_k=0, top_p=1.0, pos=0, eos=-1, ld_seq=0, seq=None):
    return lib.gpt2mi_sample(None, ldl, B, V, temperature, top_k, top_p, 0, pos, eos, None, None, seq, ld_seq, None, None)


@needs_lib
def test_sample_refuses_bad_arguments(lib):
    from gpt_2_distributed_amd import _lib
    hdr = open(os.path.join(REPO, "include", "gpt2mi.h")).read()
    cap = int(hdr.split("#define GPT2MI_SAMPLE_MAX_V")[1].split()[0])
    assert cap == _lib.SAMPLE_MAX_V >= 50257
    for kw, msg in ((dict(B=0), b"B=0"), (dict(V=0), b"V=0"), (dict(ldl=50256), b"ldl=50256"),
                    (dict(temperature=-0.5), b"temperature"), (dict(temperature=float("nan")), b"temperature"),
                    (dict(top_p=0.0), b"top_p"), (dict(top_p=-1.0), b"top_p"), (dict(top_p=float("nan")), b"top_p"),
                    (dict(pos=-1), b"pos=-1"), (dict(V=cap + 1, ldl=cap + 1), b"capacity"),
                    (dict(eos=50257), b"eos"), (dict(eos=-2), b"eos"),
                    (dict(seq=ctypes.c_void_p(8), ld_seq=4, pos=4), b"ld_seq")):
        assert _sample(lib, **kw) == 22, kw
        assert msg in lib.gpt2mi_last_error(), (kw, lib.gpt2mi_last_error())
    # valid scalars reach the pointer check, still before any launch
    assert _sample(lib) == 22 and b"NULL" in lib.gpt2mi_last_error()
    assert _sample(lib, V=cap, ldl=cap) == 22 and b"NULL" in lib.gpt2mi_last_error()


@needs_lib
def test_decode_generate_refuses_bad_arguments(lib):
    from gpt_2_distributed_amd import _lib
    plan = _lib.DecodePlan()
    plan.B, plan.C, plan.H, plan.L, plan.Vp, plan.Tcap = 2, 128, 2, 1, 512, 64

    def gen(V=509, pos0=5, n=4, ld_seq=64, seq=None):
        return lib.gpt2mi_decode_generate(ctypes.byref(plan), V, 1.0, 0, 1.0, 0, -1, pos0, n, None, seq, ld_seq, None,
                                          None)
    assert lib.gpt2mi_decode_generate(None, 509, 1.0, 0, 1.0, 0, -1, 5, 4, None, None, 0, None, None) == 22
    assert gen(V=513) == 22 and b"V=513" in lib.gpt2mi_last_error()
    assert gen(n=-1) == 22
    assert gen(pos0=0) == 22 and b"prefill" in lib.gpt2mi_last_error()
    assert gen(pos0=61, n=4) == 22 and b"cache length" in lib.gpt2mi_last_error()
    assert gen(seq=ctypes.c_void_p(8), ld_seq=8) == 22 and b"ld_seq" in lib.gpt2mi_last_error()
    assert gen() == 22 and b"NULL" in lib.gpt2mi_last_error()
    assert lib.gpt2mi_abi_version() == _lib.ABI_VERSION >= 17
    for name in ("gpt2mi_sample", "gpt2mi_decode_generate"):
        assert name in _lib.EXPORTED and hasattr(lib, name)


# ---- the public interface, as far as it goes without a GPU -------------------------------------------------------------
def test_generate_takes_top_p_and_seed_and_refuses_bad_combinations():
    from gpt_2_distributed_amd.model import GPT2
    for fn in (GPT2.generate, generation.generate):
        params = inspect.signature(fn).parameters
        assert params["top_p"].default is None and params["seed"].default is None
    from gpt_2_distributed_amd.model import GPT2Config
    model = GPT2(GPT2Config(n_layer=1, n_head=1, n_embd=64, vocab_size=64, n_positions=16))
    idx = torch.zeros(1, 2, dtype=torch.long)
    with pytest.raises(ValueError, match="generator"):
        model.generate(idx, 2, seed=0, generator=torch.Generator())
    with pytest.raises(ValueError, match="top_p"):
        model.generate(idx, 2, seed=0, top_p=0.0)
    with pytest.raises(ValueError, match="top_p"):
        model.generate(idx, 2, top_p=float("nan"))
    with pytest.raises(RuntimeError, match="cuda"):  # _check_model's refusals apply unchanged (a CPU model)
        model.generate(idx, 2, temperature=0.0, seed=0)


def test_cli_has_the_sampler_switch():
    from gpt_2_distributed_amd.generate import parse_args
    a = parse_args(["--checkpoint", "x"])
    assert a.sampler == "torch" and a.top_p is None
    a = parse_args(["--checkpoint", "x", "--sampler", "device", "--top_p", "0.9"])
    assert a.sampler == "device" and a.top_p == 0.9


# ---- register budget ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_sample_kernel_has_no_scratch_and_no_spills():
    """The row lives in registers: scratch would put it back in memory, 50 round trips per probe of the searches."""
    kernels = {k: v for k, v in _resources("sample.hip").items() if "sample_kernel" in k}
    assert len(kernels) == 2, kernels  # the sampling kernel and the greedy one
    for k, v in kernels.items():
        assert v["ScratchSize [bytes/lane]"] == 0, f"{k}: scratch {v}"
        assert v["VGPRs Spill"] == 0, f"{k}: spills {v}"
