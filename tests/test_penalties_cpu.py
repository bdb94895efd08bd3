"""Repetition, presence and frequency penalties without a GPU: the rule (generation.apply_penalties) against a
brute-force loop in numpy.float32, the argument checks of gpt2mi_sample_penalized / gpt2mi_decode_generate_penalized
(NULL pointers: nothing is launched), the register budget of the penalised kernels, and the history bookkeeping of
serve_prompts and speculate_loop over stub sessions."""
import ctypes
import inspect
import os
import shutil

import numpy as np
import pytest
import torch

from gpt_2_distributed_amd import generation
from gpt_2_distributed_amd.generation import apply_penalties
from tests.conftest import REPO
from tests.test_kernel_resources import HIPCC, _resources

LIB = os.path.join(REPO, "gpt_2_distributed_amd", "libgpt2mi.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libgpt2mi.so not built (run __graft_entry__.build())")


# ---- the rule ----------------------------------------------------------------------------------------------------------
def brute_force(logits, history, lens, gen_start, rp, pp, fp):
    """The issue's statement, one row and one vocabulary index at a time, every operation a numpy.float32 one."""
    f = np.float32
    x = logits.numpy().astype(np.float32).copy()
    B, V = x.shape
    with np.errstate(all="ignore"):
        for b in range(B):
            h = [int(t) for t in history[b, :lens[b]]]
            for i in range(V):
                seen = i in h
                c = sum(1 for t in h[gen_start[b]:] if t == i)
                v = x[b, i]
                if rp != 1 and seen:
                    v = f(v * f(rp)) if v < 0 else f(v / f(rp))
                if fp != 0 and c > 0:
                    v = f(v - f(f(fp) * f(c)))
                if pp != 0 and c > 0:
                    v = f(v - f(pp))
                x[b, i] = v
    return torch.from_numpy(x)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def random_case(seed, B=5, V=37, T=24):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, V, generator=g) * 4
    logits[:, 3] = 0.0
    logits[:, 4] = -0.0
    logits[:, 5] = float("-inf")
    logits[:, 6] = -2.5
    history = torch.randint(0, 12, (B, T), generator=g)      # a small range: many duplicates, and tokens 3..6 occur
    history[:, 1] = -1
    history[:, 2] = V                                           # out of range on both sides
    history[:, 7] = 2 ** 40
    history[:, 0] = 30                                          # in the prompt part only wherever gen_start > 0
    lens = [T, 0, 9, T - 1, 13][:B]
    gen_start = [0, 0, 9, 5, 4][:B]                             # 0, == lens, in the middle
    return logits, history, lens, gen_start


@pytest.mark.parametrize("rp,pp,fp", [(1.3, 0.0, 0.0), (1.0, 0.5, 0.0), (1.0, 0.0, 0.2), (1.3, 0.5, 0.2),
                                      (0.7, -0.4, -0.1), (3.0, 1e-3, 7.25)])
@pytest.mark.parametrize("seed", [0, 1])
def test_apply_penalties_equals_a_brute_force_loop_in_float32(seed, rp, pp, fp):
    logits, history, lens, gen_start = random_case(seed)
    got = apply_penalties(logits, history, lens, gen_start, rp, pp, fp)
    want = brute_force(logits, history, lens, gen_start, rp, pp, fp)
    assert got.dtype == torch.float32 and same_bits(got, want)
    assert same_bits(got[1], logits[1])                         # an empty history
    if rp != 1 and pp != 0:
        # token 30 sits at position 0 only: with gen_start > 0 it is a prompt token, repetition alone applies
        b = 3
        assert 30 not in history[b, gen_start[b]:lens[b]].tolist()
        only_rp = apply_penalties(logits, history, lens, gen_start, rp, 0.0, 0.0)
        assert same_bits(got[b, 30], only_rp[b, 30]) and not same_bits(got[b, 30], logits[b, 30])
    # tensors for lens / gen_start, and None for gen_start (= 0)
    again = apply_penalties(logits, history, torch.tensor(lens), torch.tensor(gen_start), rp, pp, fp)
    assert same_bits(again, got)
    zero = apply_penalties(logits, history, lens, None, rp, pp, fp)
    assert same_bits(zero, brute_force(logits, history, lens, [0] * len(lens), rp, pp, fp))


def test_sign_rule_and_the_order_of_the_steps():
    """HF's sign rule (negative: multiplied, otherwise divided, 0 included) and repetition -> frequency -> presence,
    on numbers whose roundings differ with the order."""
    f = np.float32
    logits = torch.tensor([[2.0, -2.0, 0.0, 1.0, 0.1, 5.0]])
    history = torch.tensor([[0, 1, 2, 4, 4, 4, 3]])
    got = apply_penalties(logits, history, [7], [3], 1.5, 0.25, 0.3)[0]
    assert float(got[0]) == float(f(2.0) / f(1.5))               # prompt only: divided, nothing subtracted
    assert float(got[1]) == float(f(-2.0) * f(1.5))              # negative: multiplied
    assert float(got[2]) == 0.0 and float(got[5]) == 5.0         # 0 / rp; an absent token
    assert float(got[3]) == float(f(f(f(1.0) / f(1.5)) - f(f(0.3) * f(1))) - f(0.25))
    step = f(f(f(0.1) / f(1.5)) - f(f(0.3) * f(3)))             # three generated occurrences
    assert float(got[4]) == float(f(step - f(0.25)))
    # the other orders give other bits here, so the assertion above pins the order
    other = f(f(f(f(0.1) - f(f(0.3) * f(3))) - f(0.25)) * f(1.5))
    assert float(got[4]) != float(other)
    # x - fp * c is two roundings: the fused form differs for these numbers
    x, fp, c = f(1.0), f(0.2), f(5)
    fused = f(np.float64(x) - np.float64(fp) * np.float64(c))
    two = f(x - f(fp * c))
    assert float(two) == 0.0 and float(fused) == -(2.0 ** -26)   # fp32(0.2) * 5 rounds to 1, the exact product is above
    got = apply_penalties(torch.tensor([[1.0]]), torch.tensor([[0, 0, 0, 0, 0]]), [5], [0], 1.0, 0.0, 0.2)
    assert float(got[0, 0]) == 0.0


def test_neutral_values_return_the_input_bits():
    logits, history, lens, gen_start = random_case(3)
    logits[0, 7] = float("nan")
    assert same_bits(apply_penalties(logits, history, lens, gen_start, 1.0, 0.0, 0.0), logits)
    assert same_bits(apply_penalties(logits, history, lens, gen_start), logits)
    bf = apply_penalties(logits.bfloat16(), history, lens, gen_start)
    assert bf.dtype == torch.float32 and torch.equal(bf.nan_to_num(7.0), logits.bfloat16().float().nan_to_num(7.0))


@pytest.mark.parametrize("kw", [dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0),
                                dict(repetition_penalty=float("nan")), dict(repetition_penalty=float("inf")),
                                dict(presence_penalty=float("inf")), dict(presence_penalty=float("nan")),
                                dict(frequency_penalty=float("-inf")), dict(frequency_penalty=float("nan"))])
def test_bad_values_are_refused_everywhere(kw):
    from gpt_2_distributed_amd.model import GPT2, GPT2Config
    name = next(iter(kw))
    logits, history, lens, gen_start = random_case(0)
    with pytest.raises(ValueError, match=name):
        apply_penalties(logits, history, lens, gen_start, **kw)
    model = GPT2(GPT2Config(n_layer=1, n_head=1, n_embd=64, vocab_size=64, n_positions=16))
    idx = torch.zeros(1, 2, dtype=torch.long)
    with pytest.raises(ValueError, match=name):
        model.generate(idx, 2, seed=0, **kw)
    with pytest.raises(ValueError, match=name):
        model.generate(idx, 2, **kw)
    with pytest.raises(ValueError, match=name):
        model.generate_many([idx[0]], 2, **kw)


def test_interface_has_the_parameters():
    from gpt_2_distributed_amd.model import GPT2
    from gpt_2_distributed_amd.generation import DecodeSession
    neutral = dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0)
    for fn in (GPT2.generate, GPT2.generate_many, generation.generate, generation.generate_many,
               DecodeSession.sample, DecodeSession.generate, DecodeSession.speculate):
        params = inspect.signature(fn).parameters
        assert {k: params[k].default for k in neutral} == neutral, fn
    for fn in (DecodeSession.sample, DecodeSession.generate, DecodeSession.speculate):
        assert inspect.signature(fn).parameters["gen_start"].default is None
    assert inspect.signature(DecodeSession.sample).parameters["history"].default is None
    # valid values reach _check_model's refusal of a CPU model unchanged
    from gpt_2_distributed_amd.model import GPT2Config
    model = GPT2(GPT2Config(n_layer=1, n_head=1, n_embd=64, vocab_size=64, n_positions=16))
    with pytest.raises(RuntimeError, match="cuda"):
        model.generate(torch.zeros(1, 2, dtype=torch.long), 2, seed=0, repetition_penalty=1.3)


def test_cli_has_the_three_flags():
    from gpt_2_distributed_amd.generate import parse_args
    a = parse_args(["--checkpoint", "x"])
    assert (a.repetition_penalty, a.presence_penalty, a.frequency_penalty) == (1.0, 0.0, 0.0)
    a = parse_args(["--checkpoint", "x", "--sampler", "device", "--repetition_penalty", "1.3", "--presence_penalty",
                    "0.5", "--frequency_penalty", "0.2", "--batch", "4", "--draft_tokens", "3"])
    assert (a.repetition_penalty, a.presence_penalty, a.frequency_penalty) == (1.3, 0.5, 0.2)
    assert a.sampler == "device" and a.batch == 4 and a.draft_tokens == 3


# ---- argument checks of the C entries (no launch) ----------------------------------------------------------------------
@pytest.fixture()
def lib():
    from gpt_2_distributed_amd import _lib
    return _lib.load()


def _pen(rp=1.3, pp=0.5, fp=0.2, hist=8, ld_hist=64, hist_rows=2, hist_row=None, gen_start=None):
    from gpt_2_distributed_amd import _lib
    keep = [None if a is None else (ctypes.c_int * len(a))(*a) for a in (hist_row, gen_start)]
    pen = _lib.Penalties(rp, pp, fp, hist, ld_hist, hist_rows, *[None if k is None else ctypes.cast(k, ctypes.c_void_p)
                                                              for k in keep])
    pen._keep = keep
    return pen


def _sample(lib, pen, B=2, V=509, ldl=512, pos=(5, 9)):
    pos_a = (ctypes.c_int * B)(*pos)
    return lib.gpt2mi_sample_penalized(None, ldl, B, V, 1.0, 0, 1.0, 0, pos_a, None, -1, None, None, None, 0, None,
                                       None if pen is None else ctypes.byref(pen), None, None)


@needs_lib
def test_sample_penalized_refuses_bad_arguments(lib):
    from gpt_2_distributed_amd import _lib
    hdr = open(os.path.join(REPO, "include", "gpt2mi.h")).read()
    cap = int(hdr.split("#define GPT2MI_PENALTY_MAX_HISTORY")[1].split()[0])
    assert cap == _lib.PENALTY_MAX_HISTORY >= 1024
    assert int(hdr.split("#define GPT2MI_ABI_VERSION")[1].split()[0]) == lib.gpt2mi_abi_version() == _lib.ABI_VERSION >= 22
    for name in ("gpt2mi_sample_penalized", "gpt2mi_decode_generate_penalized"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    nan, inf = float("nan"), float("inf")
    for kw, msg in ((dict(rp=0.0), b"repetition"), (dict(rp=-1.0), b"repetition"), (dict(rp=nan), b"repetition"),
                    (dict(pp=inf), b"presence"), (dict(pp=nan), b"presence"),
                    (dict(fp=-inf), b"frequency"), (dict(fp=nan), b"frequency"),
                    (dict(hist=None), b"hist is NULL"),
                    (dict(ld_hist=8), b"ld_hist=8"),
                    (dict(hist_row=[0, 2]), b"hist_row[1]=2"), (dict(hist_row=[-1, 0]), b"hist_row[0]=-1"),
                    (dict(hist_rows=1), b"hist_row[1]=1"),
                    (dict(gen_start=[6, 0]), b"gen_start[0]=6"), (dict(gen_start=[0, -1]), b"gen_start[1]=-1")):
        assert _sample(lib, _pen(**kw)) == 22, kw
        assert msg in lib.gpt2mi_last_error(), (kw, lib.gpt2mi_last_error())
    assert _sample(lib, _pen(ld_hist=cap + 8), pos=(5, cap + 1)) == 22 and b"cap" in lib.gpt2mi_last_error()
    # bad values are refused with a neutral rest too; gpt2mi_sample_ragged's own checks come first
    assert _sample(lib, _pen(rp=1.0, pp=nan, fp=0.0, hist=None)) == 22 and b"presence" in lib.gpt2mi_last_error()
    assert _sample(lib, _pen(), ldl=500) == 22 and b"ldl=500" in lib.gpt2mi_last_error()
    # valid arguments reach the pointer check, still before any launch: penalised, at the boundaries, neutral (where hist
    # may be NULL and the arrays are not read) and without the struct
    for pen in (_pen(), _pen(gen_start=[5, 0], hist_row=[1, 1]), _pen(ld_hist=9), _pen(ld_hist=cap, hist_rows=2),
                _pen(1.0, 0.0, 0.0, hist=None, ld_hist=0, hist_rows=0), None):
        assert _sample(lib, pen) == 22 and b"must not be NULL" in lib.gpt2mi_last_error(), lib.gpt2mi_last_error()
    assert _sample(lib, _pen(ld_hist=cap), pos=(5, cap)) == 22 and b"must not be NULL" in lib.gpt2mi_last_error()


@needs_lib
def test_decode_generate_penalized_refuses_bad_arguments(lib):
    from gpt_2_distributed_amd import _lib
    plan = _lib.DecodePlan()
    plan.B, plan.C, plan.H, plan.L, plan.Vp, plan.Tcap = 2, 128, 2, 1, 512, 64
    cap = _lib.PENALTY_MAX_HISTORY

    def gen(rp=1.3, pp=0.5, fp=0.2, seq=8, ld_seq=64, pos0=(5, 9), n=4, gen_start=None):
        pos_a = (ctypes.c_int * 2)(*pos0)
        gs = None if gen_start is None else (ctypes.c_int * 2)(*gen_start)
        return lib.gpt2mi_decode_generate_penalized(ctypes.byref(plan), 509, 1.0, 0, 1.0, 0, -1, pos_a, None, n, None, seq,
                                                    ld_seq, None, None, rp, pp, fp, gs)
    nan = float("nan")
    for kw, msg in ((dict(rp=0.0), b"repetition"), (dict(rp=nan), b"repetition"), (dict(pp=float("inf")), b"presence"),
                    (dict(fp=nan), b"frequency"), (dict(seq=None), b"seq"), (dict(gen_start=[6, 0]), b"gen_start[0]=6"),
                    (dict(gen_start=[0, -2]), b"gen_start[1]=-2"), (dict(pos0=(0, 9)), b"prefill"),
                    (dict(ld_seq=12), b"ld_seq")):
        assert gen(**kw) == 22, kw
        assert msg in lib.gpt2mi_last_error(), (kw, lib.gpt2mi_last_error())
    plan.Tcap = cap + 64
    assert gen(pos0=(5, cap), n=2, ld_seq=cap + 64) == 22 and b"cap" in lib.gpt2mi_last_error()
    plan.Tcap = 64
    # valid: the pointer check; neutral values need no seq
    assert gen() == 22 and b"NULL" in lib.gpt2mi_last_error() and b"seq" not in lib.gpt2mi_last_error()
    assert gen(gen_start=[5, 0]) == 22 and b"must not be NULL" in lib.gpt2mi_last_error()
    assert gen(1.0, 0.0, 0.0, seq=None) == 22 and b"must not be NULL" in lib.gpt2mi_last_error()


# ---- register budget ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_penalised_kernels_have_no_scratch_and_no_spills():
    """Whatever the new kernels are called: every kernel of sample.hip but the two plain ones, of which there must be
    two (greedy and sampled), keeps the row in registers; and the plain ones are still there under their names."""
    res = _resources("sample.hip")
    plain = {k: v for k, v in res.items() if "sample_kernel" in k}
    new = {k: v for k, v in res.items() if k not in plain}
    assert len(plain) == 2 and len(new) == 2, sorted(res)
    for k, v in res.items():
        assert v["ScratchSize [bytes/lane]"] == 0, f"{k}: scratch {v}"
        assert v["VGPRs Spill"] == 0, f"{k}: spills {v}"


# ---- the serving loop and the speculative loop over stub sessions ------------------------------------------------------
class ServeStub:
    """DecodeSession's surface as serve_prompts uses it, on the CPU, with the penalty keywords. The token at position p
    of a row is 1 + (the sum of the row's history seq[b, :p], which must be its prompt and its own tokens) % 97: a
    function of the whole history, so a prompt missing from the buffer or another row's tokens in it change the output."""

    def __init__(self, B, Tcap):
        self.B, self.Tcap = B, Tcap
        self.lens, self.device = [0] * B, torch.device("cpu")
        self.drawn = False
        self.prompt = [None] * B
        self.seen = []

    def refill(self, row, prompt):
        self.lens[row] = prompt.numel()
        self.prompt[row] = prompt.tolist()

    def flush(self):
        if self.drawn:
            self.lens = [n + 1 for n in self.lens]
            self.drawn = False

    def generate(self, n, temperature, top_k, top_p, seed, eos_token_id, seq, done, row_id=None,
                 repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, gen_start=None):
        self.flush()
        self.seen.append((repetition_penalty, presence_penalty, frequency_penalty, list(gen_start)))
        for b in range(self.B):
            P = len(self.prompt[b])
            assert gen_start[b] == P                                         # the prompt's length
            assert seq[b, :P].tolist() == self.prompt[b], (b, seq[b, :P].tolist(), self.prompt[b])  # ... and it is there
            for i in range(n):
                p = self.lens[b] + i
                seq[b, p] = 1 + int(seq[b, :p].sum()) % 97
        self.lens = [m + n - 1 for m in self.lens]
        self.drawn = True


def serve_expected(prompt, n):
    out = list(prompt)
    for _ in range(n):
        out.append(1 + sum(out) % 97)
    return out


@pytest.mark.parametrize("batch_size", [1, 2, 5])
def test_serving_loop_keeps_each_rows_prompt_in_the_history(batch_size):
    n = 40                                                                    # more than one chunk: rows finish apart
    lens = [3, 11, 1, 7, 20]
    prompts = [torch.arange(100 * i + 1, 100 * i + 1 + L) for i, L in enumerate(lens)]
    sess = ServeStub(batch_size, max(lens) + n)
    outs = generation.serve_prompts(sess, prompts, n, generation.Sampler.of(0.8, 20, None, 3, None, 1.3, 0.5, 0.2))
    assert [o.tolist() for o in outs] == [serve_expected(p.tolist(), n) for p in prompts]
    assert all(s[:3] == (1.3, 0.5, 0.2) for s in sess.seen) and len(sess.seen) >= 2 * -(-len(lens) // batch_size)


def test_serving_loop_without_penalties_calls_generate_as_before():
    """Neutral values: no penalty keyword reaches the session (test_ragged_cpu's stub, which takes none, keeps working)
    and the buffer holds generated tokens only."""
    from tests.test_ragged_cpu import StubSession, expected, script
    prompts = [torch.arange(1, 6), torch.arange(1, 3)]
    sess = StubSession(2, 16, script)
    outs = generation.serve_prompts(sess, prompts, 5, generation.Sampler.of(1.0, None, None, 0, None, 1.0, 0.0, 0.0))
    assert [o.tolist() for o in outs] == [expected(i, p.tolist(), 5, None) for i, p in enumerate(prompts)]


class SpecStub:
    """DecodeSession's surface as speculate_loop uses it, with Sampler.write_verify_history doing what the session's
    _verify does before it samples. The token after a history h is nxt(h): the whole history decides it, as under
    penalties, so a verify row draws the loop's token iff seq holds the sequence's tokens up to and including its own."""

    def __init__(self, seq, lens):
        self.B, self.lens, self.seq = len(lens), list(lens), seq
        self.rows = []

    def _verify(self, toks, seqs, poss, ks, sampler):
        record, seq, gen_start = sampler
        pen = record.write_verify_history(seq, torch.tensor(toks, dtype=torch.int64), seqs, poss, gen_start)
        assert pen["hist"] is self.seq and pen["hist_row"] == list(seqs)
        assert pen["gen_start"] == [GEN_START[b] for b in seqs] and pen["repetition"] == 1.3
        out = []
        for r, (t, b, p) in enumerate(zip(toks, seqs, poss)):
            h = self.seq[b, :p + 1].tolist()
            assert h[-1] == t                                                # the row's own token is in its history
            self.rows.append((b, p, h))
            out.append(nxt(h))
        return out

    def _accept(self, src, dst):
        pass


GEN_START = [4, 2]


def nxt(h):
    return 1 + (sum(h) * 7 + len(h)) % 89


def loop_tokens(prompt, n):
    h = list(prompt)
    for _ in range(n):
        h.append(nxt(h))
    return h


@pytest.mark.parametrize("how", ["right", "wrong", "mixed"])
def test_speculative_verify_reads_the_current_token_and_the_drafts(how):
    n, k = 12, 3
    prompts = [[5, 6, 7, 8], [9, 10]]
    want = [loop_tokens(p, n) for p in prompts]
    seq = torch.full((2, 4 + n), -5, dtype=torch.int64)
    for b, p in enumerate(prompts):
        seq[b, :len(p)] = torch.tensor(p)
    calls = dict(n=0)

    def draft(history, m):
        calls["n"] += 1
        b = 0 if history[0] == 5 else 1
        right = want[b][len(history):len(history) + m]
        bad = how == "wrong" or (how == "mixed" and calls["n"] % 2 == 0)
        return [right[0] + 1] + right[1:] if bad and right else right
    sess = SpecStub(seq, [4, 2])
    first = [want[0][4], want[1][2]]
    record = generation.Sampler.of(0.8, None, None, 0, None, 1.3, 0.5, 0.2)
    new, stats = generation.speculate_loop(sess, n, k, draft, None, [list(p) for p in prompts], first, [0, 1],
                                           (record, seq, list(GEN_START)))
    assert [p + t for p, t in zip(prompts, new)] == want               # exactly the one-token loop's tokens
    assert stats["accepted"] == (stats["drafted"] if how == "right" else 0 if how == "wrong" else stats["accepted"])
    if how == "right":
        assert stats["calls"] < n - 1
    assert {b for b, _, _ in sess.rows} == {0, 1} and len(sess.rows) > stats["calls"]   # (runs of several rows)
    # a record without penalties writes nothing and returns {}
    before = seq.clone()
    plain = generation.Sampler.of(0.8, None, None, 0)
    assert plain.write_verify_history(seq, torch.tensor([1]), [0], [0], [0]) == {} and torch.equal(seq, before)
