"""Ragged batched generation without a GPU: the v19 entries' argument checks (through the built library with NULL or
dummy pointers: nothing is launched), the argument errors of generate / generate_many, the bookkeeping of
generate_many's serving loop against a stub session that emits scripted tokens, and the new kernels' register budget."""
import ctypes
import inspect
import os
import shutil

import pytest
import torch

from gpt_2_distributed_amd import generation
from tests.conftest import REPO
from tests.test_kernel_resources import HIPCC, _instantiation, _resources

LIB = os.path.join(REPO, "gpt_2_distributed_amd", "libgpt2mi.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libgpt2mi.so not built (run __graft_entry__.build())")
SOME = ctypes.c_void_p(8)  # a non-NULL pointer for an argument whose check comes after the one under test

RAGGED = ("gpt2mi_attn_decode_ragged", "gpt2mi_embed_decode_ragged", "gpt2mi_sample_ragged",
          "gpt2mi_decode_step_ragged", "gpt2mi_decode_generate_ragged")


@pytest.fixture()
def lib():
    from gpt_2_distributed_amd import _lib
    return _lib.load()


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def refused(lib, rc, *words):
    msg = lib.gpt2mi_last_error()
    assert rc == 22 and all(w in msg for w in words), (rc, msg)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
@needs_lib
def test_abi_is_v19_or_later_and_binds_the_ragged_entries(lib):
    from gpt_2_distributed_amd import _lib
    assert lib.gpt2mi_abi_version() == _lib.ABI_VERSION >= 19
    for name in RAGGED:
        assert name in _lib.EXPORTED and hasattr(lib, name)
    hdr = open(os.path.join(REPO, "include", "gpt2mi.h")).read()
    assert int(hdr.split("#define GPT2MI_DECODE_MAX_B")[1].split()[0]) == _lib.DECODE_MAX_B == generation.MAX_BATCH == 64


@needs_lib
def test_attn_decode_ragged_refuses_bad_arguments(lib):
    H, Tcap = 4, 256

    def call(pos, B=2, head_dim=64, ws_floats=None, tcap=Tcap):
        ws = lib.gpt2mi_attn_decode_workspace(B, H, tcap) if ws_floats is None else ws_floats
        return lib.gpt2mi_attn_decode_ragged(None, None, None, None, None, ws, B, H, head_dim, tcap, pos, None)
    refused(lib, call(ints(0, 1), head_dim=32), b"head_dim=32")
    refused(lib, call(ints(0), B=0), b"B=0")
    refused(lib, call(ints(*[0] * 65), B=65), b"B=65")
    refused(lib, call(None), b"position array", b"NULL")
    for bad in (-1, Tcap, Tcap + 5):
        refused(lib, call(ints(3, bad)), b"pos[1]=%d" % bad)
        refused(lib, call(ints(bad, 3)), b"pos[0]=%d" % bad)
    refused(lib, call(ints(0, 255), ws_floats=lib.gpt2mi_attn_decode_workspace(2, H, Tcap) - 1), b"workspace too small")
    refused(lib, call(ints(0, 255)), b"NULL")  # valid scalars and positions reach the pointer check: still no launch


@needs_lib
def test_embed_decode_ragged_refuses_bad_arguments(lib):
    def call(pos, B=2, C=128):
        return lib.gpt2mi_embed_decode_ragged(None, None, None, None, B, C, pos, None)
    refused(lib, call(ints(0), B=0), b"B=0")
    refused(lib, call(ints(*[0] * 65), B=65), b"B=65")
    refused(lib, call(ints(0, 0), C=130), b"C=130")
    refused(lib, call(None), b"position array", b"NULL")
    refused(lib, call(ints(5, -1)), b"pos[1]=-1")
    refused(lib, call(ints(5, 6)), b"NULL")


@needs_lib
def test_sample_ragged_refuses_bad_arguments(lib):
    def call(pos=ints(0), ldl=50432, B=1, V=50257, temperature=1.0, top_k=0, top_p=1.0, eos=-1, ld_seq=0, seq=None,
             row_id=None):
        return lib.gpt2mi_sample_ragged(None, ldl, B, V, temperature, top_k, top_p, 0, pos, row_id, eos, None, None, seq,
                                        ld_seq, None, None)
    from gpt_2_distributed_amd import _lib
    cap = _lib.SAMPLE_MAX_V
    # what the scalar twin refuses
    for kw, msg in ((dict(B=0), b"B=0"), (dict(V=0), b"V=0"), (dict(ldl=50256), b"ldl=50256"),
                    (dict(temperature=-0.5), b"temperature"), (dict(temperature=float("nan")), b"temperature"),
                    (dict(top_p=0.0), b"top_p"), (dict(top_p=float("nan")), b"top_p"),
                    (dict(V=cap + 1, ldl=cap + 1), b"capacity"), (dict(eos=50257), b"eos"), (dict(eos=-2), b"eos")):
        refused(lib, call(**kw), msg)
    # and what the position array adds
    refused(lib, call(pos=ints(*[0] * 65), B=65), b"B=65")
    refused(lib, call(pos=None), b"position array", b"NULL")
    refused(lib, call(pos=ints(3, -1), B=2), b"pos[1]=-1")
    refused(lib, call(pos=ints(3, 4), B=2, seq=SOME, ld_seq=4), b"ld_seq=4", b"pos[1]=4")
    refused(lib, call(pos=ints(4, 3), B=2, seq=SOME, ld_seq=4), b"ld_seq=4", b"pos[0]=4")
    refused(lib, call(pos=ints(3, 4), B=2, seq=SOME, ld_seq=5), b"NULL")  # reaches the pointer check
    refused(lib, call(pos=ints(3, 4), B=2, row_id=(ctypes.c_uint32 * 2)(7, 9)), b"NULL")


@needs_lib
def test_scalar_entries_forward_and_take_at_most_64_rows(lib):
    """v20: gpt2mi_attn_decode and gpt2mi_sample are forwarders to the per-row implementation, so B stops at
    GPT2MI_DECODE_MAX_B (before: B * H <= 65535, any B); B = 64 still reaches the pointer check."""
    from gpt_2_distributed_amd import _lib
    assert lib.gpt2mi_abi_version() == _lib.ABI_VERSION >= 20
    H, Tcap = 4, 256

    def attn(B):
        return lib.gpt2mi_attn_decode(None, None, None, None, None, lib.gpt2mi_attn_decode_workspace(B, H, Tcap), B, H,
                                      64, Tcap, 5, None)

    def sample(B):
        return lib.gpt2mi_sample(None, 50432, B, 50257, 1.0, 0, 1.0, 0, 3, -1, None, None, None, 0, None, None)
    for call in (attn, sample):
        refused(lib, call(65), b"B=65")
        refused(lib, call(1000), b"B=1000")
        refused(lib, call(64), b"NULL")
    refused(lib, lib.gpt2mi_embed_decode(None, None, None, None, 65, 128, 0, None), b"B=65")


def _plan(B=2, Tcap=64):
    from gpt_2_distributed_amd import _lib
    plan = _lib.DecodePlan()
    plan.B, plan.C, plan.H, plan.L, plan.Vp, plan.Tcap = B, 128, 2, 1, 512, Tcap
    return plan


@needs_lib
def test_decode_step_ragged_refuses_bad_arguments(lib):
    plan = _plan(B=65)

    def step(pos):
        return lib.gpt2mi_decode_step_ragged(ctypes.byref(plan), None, pos, None)
    refused(lib, lib.gpt2mi_decode_step_ragged(None, None, ints(0), None), b"plan is NULL")
    refused(lib, step(ints(*[0] * 65)), b"B=65")
    plan.B, plan.H = 2, 4
    refused(lib, step(ints(0, 0)), b"head_dim")
    plan.H = 2
    refused(lib, step(None), b"position array", b"NULL")
    refused(lib, step(ints(0, 64)), b"pos[1]=64")
    refused(lib, step(ints(-1, 0)), b"pos[0]=-1")
    refused(lib, step(ints(0, 63)), b"workspace too small")  # attn_ws_floats = 0: the scalar twin's next check


@needs_lib
def test_decode_generate_ragged_refuses_bad_arguments(lib):
    plan = _plan()

    def gen(pos0=ints(5, 9), V=509, n=4, ld_seq=64, seq=None):
        return lib.gpt2mi_decode_generate_ragged(ctypes.byref(plan), V, 1.0, 0, 1.0, 0, -1, pos0, None, n, None, seq,
                                                 ld_seq, None, None)
    refused(lib, lib.gpt2mi_decode_generate_ragged(None, 509, 1.0, 0, 1.0, 0, -1, ints(5, 9), None, 4, None, None, 0,
                                                   None, None), b"plan is NULL")
    refused(lib, gen(V=513), b"V=513")
    refused(lib, gen(n=-1), b"n=-1")
    refused(lib, gen(pos0=None), b"position array", b"NULL")
    refused(lib, gen(pos0=ints(5, 64)), b"pos[1]=64")
    refused(lib, gen(pos0=ints(0, 9)), b"prefill")
    refused(lib, gen(pos0=ints(5, 61)), b"cache length")  # max pos0 + n = 65 > Tcap
    refused(lib, gen(pos0=ints(61, 5)), b"cache length")
    refused(lib, gen(seq=SOME, ld_seq=12), b"ld_seq")    # 9 + 4 > 12
    refused(lib, gen(), b"NULL")
    plan.B = 65
    refused(lib, gen(pos0=ints(*[5] * 65)), b"B=65")


# ---- generate / generate_many: argument errors -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_model():
    from gpt_2_distributed_amd.model import GPT2, GPT2Config
    return GPT2(GPT2Config(n_layer=1, n_head=1, n_embd=64, vocab_size=64, n_positions=16))


def test_generate_takes_prompt_lens_and_refuses_bad_ones(cpu_model):
    from gpt_2_distributed_amd.model import GPT2
    for fn in (GPT2.generate, generation.generate):
        params = inspect.signature(fn).parameters
        assert params["prompt_lens"].default is None and params["pad_token_id"].default is None
    idx = torch.zeros(3, 5, dtype=torch.long)
    with pytest.raises(ValueError, match="prompt lengths"):
        cpu_model.generate(idx, 2, prompt_lens=[1, 2])             # wrong length
    for bad in ([1, 2, 0], [1, 6, 2], [-1, 2, 3]):
        with pytest.raises(ValueError, match="prompt lengths"):
            cpu_model.generate(idx, 2, prompt_lens=bad)            # out of [1, P]
    with pytest.raises(ValueError, match="n_positions"):
        cpu_model.generate(idx, 12, prompt_lens=[1, 5, 2])         # 5 + 12 > 16
    with pytest.raises(ValueError, match="n_positions"):
        cpu_model.generate([torch.zeros(2, dtype=torch.long), torch.zeros(9, dtype=torch.long)], 8)
    with pytest.raises(ValueError, match="pad_token_id"):
        cpu_model.generate(idx, 2, prompt_lens=[1, 5, 2], pad_token_id=64)
    with pytest.raises(ValueError, match="prompt_lens"):
        cpu_model.generate([torch.zeros(2, dtype=torch.long)], 2, prompt_lens=[2])
    # the padding is not counted: max(prompt_lens) + n fits although P + n does not
    with pytest.raises(RuntimeError, match="cuda"):                # (valid arguments reach _check_model: a CPU model)
        cpu_model.generate(idx, 12, prompt_lens=[1, 4, 2])


def test_generate_many_refuses_bad_arguments(cpu_model):
    import gpt_2_distributed_amd as pkg
    from gpt_2_distributed_amd.model import GPT2
    assert pkg.generate_many is generation.generate_many and "generate_many" in pkg.__all__
    params = inspect.signature(GPT2.generate_many).parameters
    assert params["batch_size"].default == 32 and params["seed"].default == 0
    prompts = [torch.zeros(n, dtype=torch.long) for n in (2, 9, 4)]
    with pytest.raises(ValueError, match="Generator"):
        cpu_model.generate_many(prompts, 4, generator=torch.Generator())
    with pytest.raises(ValueError, match="n_positions"):
        cpu_model.generate_many(prompts, 8)                        # 9 + 8 > 16
    with pytest.raises(ValueError, match="batch_size"):
        cpu_model.generate_many(prompts, 4, batch_size=65)
    with pytest.raises(ValueError, match="1-D"):
        cpu_model.generate_many([torch.zeros(2, 2, dtype=torch.long)], 4)
    with pytest.raises(ValueError, match="top_p"):
        cpu_model.generate_many(prompts, 4, top_p=0.0)
    with pytest.raises(ValueError, match="eos_token_id"):
        cpu_model.generate_many(prompts, 4, eos_token_id=64)
    with pytest.raises(RuntimeError, match="cuda"):
        cpu_model.generate_many(prompts, 7)
    assert cpu_model.generate_many([], 4) == []


def test_cli_takes_several_prompts(tmp_path):
    from gpt_2_distributed_amd.generate import parse_args
    a = parse_args(["--checkpoint", "x"])
    assert a.prompt_ids is None and a.prompts_file is None
    a = parse_args(["--checkpoint", "x", "--prompt_ids", "1,2", "--prompt_ids", "3", "--prompts_file", "p.txt"])
    assert a.prompt_ids == ["1,2", "3"] and a.prompts_file == "p.txt"


# ---- the serving loop against a stub session ---------------------------------------------------------------------------
EOS = 99


class StubSession:
    """DecodeSession's surface as serve_prompts uses it, on the CPU. The token of the sequence with draw key r at
    position p is script(r, p): a function of the key and the position, as the device sampler's is of (seed, key,
    position) and the sequence's own past. Checks the session's own rules (capacity, flush before a refill)."""

    def __init__(self, B, Tcap, script):
        self.B, self.Tcap, self.script = B, Tcap, script
        self.lens, self.device = [0] * B, torch.device("cpu")
        self.drawn = False
        self.refills, self.keys_seen, self.chunks = [], set(), []

    def refill(self, row, prompt):
        assert not self.drawn, "refill with an unstepped token"
        assert prompt.dim() == 1 and 1 <= prompt.numel() <= self.Tcap
        self.lens[row] = prompt.numel()
        self.refills.append((row, prompt.tolist()))

    def flush(self):
        if self.drawn:
            self.lens = [n + 1 for n in self.lens]
            self.drawn = False

    def generate(self, n, temperature, top_k, top_p, seed, eos_token_id, seq, done, row_id=None):
        self.flush()
        assert min(self.lens) >= 1 and n >= 1 and max(self.lens) + n <= self.Tcap, (self.lens, n, self.Tcap)
        assert len(row_id) == self.B
        self.chunks.append(n)
        for b in range(self.B):
            self.keys_seen.add((b, row_id[b], self.lens[b]))
            for i in range(n):
                t = self.script(row_id[b], self.lens[b] + i)
                if eos_token_id is not None:
                    if done[b]:
                        t = eos_token_id
                    elif t == eos_token_id:
                        done[b] = 1
                seq[b, self.lens[b] + i] = t
        self.lens = [m + n - 1 for m in self.lens]
        self.drawn = True


def script(key, pos):
    """The sequence with draw key `key` emits 1000 * key + pos, and EOS at position 7 * key + 4 (if it gets there)."""
    return EOS if pos == 7 * key + 4 else 1000 * (key % 1000) + pos


def expected(i, prompt, n, eos):
    new = []
    for p in range(len(prompt), len(prompt) + n):
        new.append(script(i, p))
        if eos is not None and new[-1] == eos:
            break
    return prompt + new


@pytest.mark.parametrize("eos", [None, EOS])
@pytest.mark.parametrize("batch_size", [1, 3, 7, 10])
def test_serving_loop_bookkeeping(batch_size, eos):
    """7 prompts through `batch_size` rows: input order kept, every prompt served exactly once with row_id = its index,
    outputs cut after EOS, whatever the batch size (more rows than prompts: the rest are dummies)."""
    n = 40
    lens = [1, 5, 12, 3, 9, 20, 2]
    prompts = [torch.arange(30 * i + 1, 30 * i + 1 + L) for i, L in enumerate(lens)]  # (no token 0: the dummy's)
    sess = StubSession(batch_size, max(lens) + n, script)
    outs = generation.serve_prompts(sess, prompts, n, generation.Sampler.of(0.8, 20, None, 3, eos))
    assert len(outs) == 7
    for i, (o, p) in enumerate(zip(outs, prompts)):
        assert o.dtype == torch.int64 and o.tolist() == expected(i, p.tolist(), n, eos), i
        if eos is not None and EOS in o.tolist():
            assert o.tolist().index(EOS) == len(o) - 1
    if eos is not None:
        assert sum(EOS in o.tolist() for o in outs) >= 4 and any(EOS not in o.tolist() for o in outs)
    real = [(row, p) for row, p in sess.refills if p != [0]]
    assert sorted(p for _, p in real) == sorted(p.tolist() for p in prompts)      # each prompt entered exactly once
    assert [p for _, p in real] == [p.tolist() for p in prompts]                  # ... in input order
    keys = {k for _, k, _ in sess.keys_seen if k != 0xFFFFFFFF}
    assert keys == set(range(7))                                                  # row_id = the prompt's index
    assert all(c <= generation.EOS_CHUNK for c in sess.chunks)


def test_serving_loop_at_the_end_of_the_cache():
    """Prompt + n fills the cache exactly (the last token sits at Tcap - 1) beside shorter sequences and dummies."""
    n = 5
    prompts = [torch.arange(1, 12), torch.arange(1, 3), torch.arange(1, 8)]
    sess = StubSession(4, 16, script)
    outs = generation.serve_prompts(sess, prompts, n, generation.Sampler.of(1.0, None, None, 0, None))
    assert [o.tolist() for o in outs] == [expected(i, p.tolist(), n, None) for i, p in enumerate(prompts)]


# ---- register budget ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_ragged_kernels_have_no_scratch_and_no_spills():
    """The position arrays arrive as kernel arguments and are indexed by blockIdx: a scalar load, not a private array.
    The per-row kernels are the only ones (the scalar entries forward to them), under the plain names."""
    subs = ("attn_combine_kernel", "embed_decode_kernel", "sample_kernel")
    found = {}
    for src in ("decode.hip", "sample.hip"):
        res = _resources(src)
        assert not any("ragged" in k for k in res), sorted(res)
        found.update({k: v for k, v in res.items() if any(sub in k for sub in subs)})
        if src == "decode.hip":  # (a template over the cache type: the bf16 cache's)
            found.update([_instantiation(res, "attn_decode_kernel", "KvBf16")])
    for sub in subs:
        assert any(sub in k for k in found), f"{sub} not found"
    assert len(found) == 5, sorted(found)  # (the sampler: greedy and sampling)
    for k, v in found.items():
        assert v["ScratchSize [bytes/lane]"] == 0, f"{k}: scratch {v}"
        assert v["VGPRs Spill"] == 0, f"{k}: spills {v}"
