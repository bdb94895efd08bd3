"""Logit bias, min-p, minimum length and stop sequences without a GPU: the three rules (generation.apply_constraints,
sample_reference's min_p, stop_match) on hand-made rows, every ValueError of _check_constraints, the minor ABI number
and the two new entries, every refusal of gpt2mi_sample_constrained / gpt2mi_decode_generate_constrained (NULL or
never-dereferenced pointers: nothing is launched), the CLI's four flags, the stop bookkeeping of speculate_loop over a
stub session and the register budget of the constrained kernels."""
import ctypes
import os
import shutil

import numpy as np
import pytest
import torch

from gpt_2_distributed_amd import generation
from gpt_2_distributed_amd.generation import (_check_constraints, apply_constraints, apply_penalties, first_stop,
                                              log_min_p, sample_reference, stop_match)
from tests.conftest import REPO
from tests.test_kernel_resources import HIPCC, _resources

LIB = os.path.join(REPO, "gpt_2_distributed_amd", "libgpt2mi.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libgpt2mi.so not built (run __graft_entry__.build())")
INF = float("inf")


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the rules ---------------------------------------------------------------------------------------------------------
def test_the_bias_comes_after_the_penalties():
    """A penalised and biased token where (x / rp) + b and (x + b) / rp differ: the rule is the first."""
    f = np.float32
    x, rp, b = f(3.3), f(1.3), f(0.7)
    first, second = f(f(x / rp) + b), f(f(x + b) / rp)
    assert first != second
    logits = torch.tensor([[1.0, float(x), -2.0, 0.5]])
    hist = torch.tensor([[1, 0, 0]])
    pen = apply_penalties(logits, hist, [1], [0], float(rp), 0.0, 0.0)
    bias = torch.tensor([[0.0, float(b), 0.0, 0.0]])
    got = apply_constraints(pen, [1], [0], bias)
    assert got[0, 1].item() == float(first)
    assert same_bits(got[:, [0, 2, 3]], logits[:, [0, 2, 3]])  # (x + 0.0 keeps a non-zero x)


def test_bias_rows_none_shared_and_own():
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(4, 9, generator=g)
    logits[0, 0], logits[1, 1] = -0.0, 0.0
    bias = torch.randn(2, 9, generator=g)
    bias[0, 3], bias[1, 4], bias[0, 0] = -INF, -0.0, -0.0
    got = apply_constraints(logits, [5] * 4, None, bias, [-1, 0, 0, 1])
    assert same_bits(got[0], logits[0])                      # no bias row: the bits, -0.0 included
    want = torch.from_numpy(logits.numpy()[[1, 2, 3]] + bias.numpy()[[0, 0, 1]])
    assert same_bits(got[1:], want)
    assert got[1, 3] == -INF and got[2, 3] == -INF and got[3, 4] == logits[3, 4]
    ident = apply_constraints(logits[:2], [5, 5], None, bias)  # bias_row None: row b reads row b
    assert same_bits(ident, torch.from_numpy(logits.numpy()[:2] + bias.numpy()))
    assert same_bits(apply_constraints(logits, [5] * 4, None), logits)
    assert apply_constraints(logits.bfloat16(), [5] * 4, None).dtype == torch.float32


def test_eos_is_held_back_below_min_new_tokens_and_not_from_it_on():
    logits = torch.tensor([[0.5, 2.0, 1.0]] * 3)
    # pos - gen_start = min_new - 2, min_new - 1 (the last suppressed draw) and min_new (the first free one)
    got = apply_constraints(logits, [5, 6, 7], [3, 3, 3], min_new_tokens=4, eos_token_id=1)
    assert got[:, 1].tolist() == [-INF, -INF, 2.0]
    assert same_bits(got[:, [0, 2]], logits[:, [0, 2]])
    # gen_start None: 0
    assert apply_constraints(logits, [5, 6, 7], None, min_new_tokens=6, eos_token_id=1)[:, 1].tolist() == [-INF, 2.0, 2.0]
    assert same_bits(apply_constraints(logits, [5, 6, 7], [3, 3, 3], min_new_tokens=0, eos_token_id=1), logits)
    with pytest.raises(ValueError, match="eos_token_id"):
        apply_constraints(logits, [5, 6, 7], None, min_new_tokens=2)
    # the bias is added first: a biased eos is still held back
    got = apply_constraints(logits, [3] * 3, [3] * 3, torch.tensor([[0.0, 50.0, 0.0]]), [0, 0, -1], 1, 1)
    assert got[:, 1].tolist() == [-INF] * 3


def test_stop_match_positions_lengths_and_the_min_new_gate():
    h = list(range(100, 120))                                # 20 tokens, gen_start 4 below
    assert stop_match(h, 4, [[119]]) and stop_match(h, 19, [[119]]) and not stop_match(h, 20, [[119]])
    assert stop_match(h, 4, [[118, 119]]) and stop_match(h, 18, [[118, 119]])
    assert not stop_match(h, 19, [[118, 119]])               # straddles gen_start: its first token is a prompt token
    assert not stop_match(h, 20, [[118, 119]])               # beyond it
    long16 = h[4:]
    assert len(long16) == 16 and stop_match(h, 4, [long16]) and not stop_match(h, 5, [long16])
    assert not stop_match(h[4:], 1, [long16]) and stop_match(h[4:], 0, [long16])  # pos - n + 1 = 0
    assert not stop_match(h[5:], 0, [long16])                # pos = 14 with a 16-token sequence: nothing before 0 is read
    assert not stop_match([], 0, [[1]]) and not stop_match(h, 4, []) and not stop_match(h, 4, [[118]])
    assert stop_match(h, 4, [[7], [118, 119]])               # any of several
    # the gate: honoured once the row holds min_new generated tokens including this one (here 16)
    assert stop_match(h, 4, [[119]], 16) and not stop_match(h, 4, [[119]], 17)
    assert first_stop(h, 4, [[110], [105, 106]]) == 6 and first_stop(h, 4, [[110]], 8) is None
    assert first_stop(h, 4, [[110]], 7) == 10 and first_stop(h, 4, [[110]], 0, eos_token_id=108) is None


def test_min_p_keeps_exactly_the_tokens_at_or_above_the_threshold():
    lmp = np.float32(log_min_p(0.1))
    assert lmp == np.float32(np.log(np.float64(np.float32(0.1)))) and log_min_p(0) == -INF and log_min_p(1.0) == 0.0
    x = torch.tensor([[0.0, float(lmp), float(np.nextafter(lmp, np.float32(-INF))), -1.0, -9.0]])
    tok, probs = sample_reference(x, 1.0, None, None, torch.tensor([0.999]), min_p=0.1)
    assert (probs > 0).tolist() == [[True, True, False, True, False]] and tok.item() == 3
    assert abs(probs.sum().item() - 1) < 1e-12
    # intersected with top-k, independent of it; greedy and None ignore it
    _, pk = sample_reference(x, 1.0, 2, None, torch.tensor([0.5]), min_p=0.1)
    assert (pk > 0).tolist() == [[True, False, False, True, False]]
    for off in (None, 0, 0.0):
        assert torch.equal(sample_reference(x, 1.0, None, None, torch.tensor([0.5]), min_p=off)[1],
                           sample_reference(x, 1.0, None, None, torch.tensor([0.5]))[1])
    assert sample_reference(x, 0.0, None, None, torch.tensor([0.5]), min_p=1.0)[0].item() == 0
    # a row with nothing finite: token 0 in both forms
    dead = torch.full((1, 5), -INF)
    assert sample_reference(dead, 0.0, None, None, torch.tensor([0.5]))[0].item() == 0
    assert sample_reference(dead, 0.8, None, None, torch.tensor([0.5]), min_p=0.1)[0].item() == 0
    # the host sampler's form keeps the same set
    g = torch.Generator().manual_seed(0)
    seen = {generation.sample_next(x, 1.0, generator=g, min_p=0.1).item() for _ in range(200)}
    assert seen == {0, 1, 3}


def test_check_constraints_raises_every_value_error():
    ok = dict(eos_token_id=5, vocab_size=10)
    assert _check_constraints(None, None, 0, None) == (0.0, 0, [])
    assert _check_constraints({3: -INF, 4: 2.5}, 0.25, 2, [[1, 2], (3,)], **ok) == (0.25, 2, [[1, 2], [3]])
    assert _check_constraints(torch.zeros(2, 10), 1.0, 0, [], **ok) == (1.0, 0, [])
    nan = float("nan")
    for kw, msg in ((dict(min_p=-0.1), "min_p"), (dict(min_p=1.5), "min_p"), (dict(min_p=nan), "min_p"),
                    (dict(min_new_tokens=-1), "min_new_tokens"),
                    (dict(min_new_tokens=1, eos_token_id=None), "eos_token_id"),
                    (dict(stop=[[1]], eos_token_id=None), "eos_token_id"),
                    (dict(stop=[[1]] * 9), "at most 8"), (dict(stop=[[]]), "1 to 16"),
                    (dict(stop=[list(range(10)) + list(range(7))]), "1 to 16"),
                    (dict(stop=[[10]]), "stop tokens"), (dict(stop=[[1, -1]]), "stop tokens"),
                    (dict(logit_bias={10: 1.0}), "logit_bias tokens"), (dict(logit_bias={-1: 1.0}), "logit_bias tokens"),
                    (dict(logit_bias={1: INF}), "finite or -inf"), (dict(logit_bias={1: nan}), "finite or -inf"),
                    (dict(logit_bias=torch.tensor([0.0] * 9 + [INF])), "finite or -inf"),
                    (dict(logit_bias=torch.tensor([nan] + [0.0] * 9)), "finite or -inf"),
                    (dict(logit_bias=torch.zeros(9)), "logit_bias must be")):
        with pytest.raises(ValueError, match=msg):
            _check_constraints(**{**ok, **kw})


def test_generate_refuses_bad_constraints_before_it_needs_a_gpu():
    from gpt_2_distributed_amd.model import GPT2, GPT2Config
    model = GPT2(GPT2Config(n_layer=1, n_head=1, n_embd=64, vocab_size=64, n_positions=16))
    idx = torch.zeros(2, 2, dtype=torch.long)
    for kw, msg in ((dict(min_p=2.0), "min_p"), (dict(min_new_tokens=2), "eos_token_id"), (dict(stop=[[1]]), "eos_token_id"),
                    (dict(logit_bias={64: 0.0}), "logit_bias tokens"), (dict(logit_bias=torch.zeros(3, 64)), "logit_bias"),
                    (dict(allowed_token_ids=[]), "allowed_token_ids"), (dict(allowed_token_ids=[64]), "allowed_token_ids"),
                    (dict(num_beams=2, min_p=0.1), "num_beams"), (dict(num_beams=2, stop=[[1]]), "num_beams"),
                    (dict(num_beams=2, logit_bias={1: 1.0}), "num_beams"),
                    (dict(num_beams=2, min_new_tokens=1), "num_beams")):
        with pytest.raises(ValueError, match=msg):
            model.generate(idx, 2, seed=None if "num_beams" in kw else 0, **kw)
    with pytest.raises(ValueError, match="logit_bias"):
        model.generate_many([idx[0]], 2, logit_bias=torch.zeros(1, 64))  # one row for every prompt: a dict or [V]
    with pytest.raises(RuntimeError, match="cuda"):  # valid values reach _check_model's refusal of a CPU model
        model.generate(idx, 2, seed=0, eos_token_id=3, min_p=0.1, min_new_tokens=1, stop=[[1, 2]], logit_bias={1: -INF},
                       allowed_token_ids=[1, 2, 3])


def test_cli_parses_the_four_flags():
    from gpt_2_distributed_amd.generate import parse_args
    a = parse_args(["--checkpoint", "x"])
    assert (a.logit_bias, a.min_p, a.min_new_tokens, a.stop) == (None, None, 0, None)
    a = parse_args(["--checkpoint", "x", "--logit_bias", "50256:-100,198:2.5", "--min_p", "0.05", "--min_new_tokens", "8",
                    "--stop", "198,198", "--stop", "13", "--sampler", "device"])
    assert a.logit_bias == {50256: -100.0, 198: 2.5} and a.min_p == 0.05 and a.min_new_tokens == 8
    assert a.stop == [[198, 198], [13]] and a.sampler == "device"
    assert parse_args(["--checkpoint", "x", "--logit_bias", "7:-inf"]).logit_bias == {7: -INF}
    for bad in (["--logit_bias", "7"], ["--logit_bias", "a:1"], ["--stop", "1,x"]):
        with pytest.raises(SystemExit):
            parse_args(["--checkpoint", "x"] + bad)


# ---- the C entries (no launch) -----------------------------------------------------------------------------------------
@pytest.fixture()
def lib():
    from gpt_2_distributed_amd import _lib
    return _lib.load()


NEW = ("gpt2mi_sample_constrained", "gpt2mi_decode_generate_constrained")


@needs_lib
def test_abi_minor_and_the_two_entries(lib):
    from gpt_2_distributed_amd import _lib
    hdr = open(os.path.join(REPO, "include", "gpt2mi.h")).read()
    assert int(hdr.split("#define GPT2MI_ABI_MINOR")[1].split()[0]) == lib.gpt2mi_abi_minor() >= 4
    assert _lib.ABI_MINOR >= 4 and lib.gpt2mi_abi_version() == _lib.ABI_VERSION == 24
    for name in NEW:
        assert name in _lib.EXPORTED and hasattr(lib, name) and _lib._SINCE_MINOR[name] == 4 and name + "(" in hdr
    assert int(hdr.split("#define GPT2MI_STOP_MAX_SEQS")[1].split()[0]) == _lib.STOP_MAX_SEQS == 8
    assert int(hdr.split("#define GPT2MI_STOP_MAX_LEN")[1].split()[0]) == _lib.STOP_MAX_LEN == 16
    assert ctypes.sizeof(_lib.Constraints) == 56  # the header's layout on LP64


def _con(bias=None, ld_bias=512, bias_rows=2, bias_row=None, min_p=0.0, min_new=0, stop=None, stop_len=None, n_stop=None):
    """A gpt2mi_constraints; `bias` is a fake address (never dereferenced: every call below is refused)."""
    from gpt_2_distributed_amd import _lib
    stop = stop or []
    lens = [len(s) for s in stop] if stop_len is None else stop_len
    table = (ctypes.c_int32 * (max(len(stop), 1) * 16))()
    for i, s in enumerate(stop):
        table[i * 16:i * 16 + min(len(s), 16)] = s[:16]
    keep = [None if bias_row is None else (ctypes.c_int * len(bias_row))(*bias_row), table,
            (ctypes.c_int * max(len(lens), 1))(*lens)]
    n = len(stop) if n_stop is None else n_stop
    con = _lib.Constraints(bias, ld_bias, bias_rows, None if keep[0] is None else ctypes.cast(keep[0], ctypes.c_void_p),
                           min_p, min_new, n, ctypes.cast(keep[1], ctypes.c_void_p) if n else None,
                           ctypes.cast(keep[2], ctypes.c_void_p) if n else None)
    con._keep = keep
    return con


def _pen(hist=8, ld_hist=64, hist_rows=2, gen_start=None, hist_row=None, rp=1.0):
    from gpt_2_distributed_amd import _lib
    keep = [None if a is None else (ctypes.c_int * len(a))(*a) for a in (hist_row, gen_start)]
    pen = _lib.Penalties(rp, 0.0, 0.0, hist, ld_hist, hist_rows,
                         *[None if k is None else ctypes.cast(k, ctypes.c_void_p) for k in keep])
    pen._keep = keep
    return pen


def _sample(lib, con, pen="default", B=2, V=509, ldl=512, pos=(5, 9), eos=7, done=8, entry=NEW[0]):
    pos_a = (ctypes.c_int * B)(*pos)
    pen = _pen() if pen == "default" else pen
    head = (None, ldl, B, V, 1.0, 0, 1.0, 0, pos_a, None, eos, done, None, None, 0, None,
            None if pen is None else ctypes.byref(pen), None, None)
    if entry == NEW[0]:
        return lib.gpt2mi_sample_constrained(*head, None if con is None else ctypes.byref(con), None)
    return lib.gpt2mi_sample_logprobs(*head, None)


REFUSALS = (  # (constraint keywords, call keywords, what the message names)
    (dict(min_p=-0.5), {}, [b"min_p"]), (dict(min_p=1.5), {}, [b"min_p"]), (dict(min_p=float("nan")), {}, [b"min_p"]),
    (dict(min_new=-1), {}, [b"min_new=-1"]), (dict(min_new=2), dict(eos=-1), [b"min_new=2", b"eos"]),
    (dict(n_stop=9, stop=[[1]]), {}, [b"n_stop=9"]), (dict(n_stop=-1), {}, [b"n_stop=-1"]),
    (dict(stop=[[1], []]), {}, [b"stop_len[1]=0"]), (dict(stop=[[1] * 16], stop_len=[17]), {}, [b"stop_len[0]=17"]),
    (dict(stop=[[1, 2], [3, 509]]), {}, [b"stop[1][1]=509"]), (dict(stop=[[-1]]), {}, [b"stop[0][0]=-1"]),
    (dict(stop=[[1]]), dict(eos=-1), [b"eos"]), (dict(stop=[[1]]), dict(done=None), [b"done is NULL"]),
    (dict(bias=8, ld_bias=500), {}, [b"ld_bias=500"]), (dict(bias=8, bias_rows=0), {}, [b"bias_rows=0"]),
    (dict(bias=8, bias_row=[0, 2]), {}, [b"bias_row[1]=2"]), (dict(bias=8, bias_row=[-2, 0]), {}, [b"bias_row[0]=-2"]),
    (dict(bias=8, bias_rows=1), {}, [b"bias_rows=1", b"B=2"]),
)


@needs_lib
def test_sample_constrained_refuses_bad_arguments(lib):
    for ckw, kw, words in REFUSALS:
        assert _sample(lib, _con(**ckw), **kw) == 22, (ckw, kw)
        msg = lib.gpt2mi_last_error()
        assert msg.startswith(b"sample_constrained: ") and all(w in msg for w in words), (ckw, kw, msg)
    # the history of the stop sequences, whatever the penalty values
    for pen, words in ((None, [b"hist is NULL"]), (_pen(hist=None), [b"hist is NULL"]), (_pen(ld_hist=8), [b"ld_hist=8"]),
                       (_pen(hist_row=[0, 2]), [b"hist_row[1]=2"]), (_pen(hist_rows=1), [b"hist_row[1]=1"]),
                       (_pen(gen_start=[6, 0]), [b"gen_start[0]=6"]), (_pen(gen_start=[0, -1]), [b"gen_start[1]=-1"])):
        assert _sample(lib, _con(stop=[[1, 2]]), pen=pen) == 22
        msg = lib.gpt2mi_last_error()
        assert msg.startswith(b"sample_constrained: ") and all(w in msg for w in words), msg
    assert _sample(lib, _con(min_new=3), pen=_pen(gen_start=[6, 0])) == 22 and b"gen_start[0]=6" in lib.gpt2mi_last_error()
    # the forwarded checks come first, under this entry's name
    assert _sample(lib, _con(min_p=0.5), ldl=500) == 22 and b"sample_constrained: ldl=500" in lib.gpt2mi_last_error()
    assert _sample(lib, _con(min_p=0.5), pen=_pen(rp=0.0)) == 22 and b"repetition" in lib.gpt2mi_last_error()
    # valid arguments reach the pointer check, still before any launch: at the boundaries, and with no history at all
    for con, kw in ((_con(min_p=1.0), {}), (_con(min_p=0.25, min_new=4, stop=[[1] * 16, [508]] + [[2]] * 6), {}),
                    (_con(bias=8, ld_bias=509, bias_rows=1, bias_row=[-1, 0]), {}), (_con(bias=8), dict(pen=None)),
                    (_con(min_new=5), dict(pen=None)), (_con(min_p=0.5), dict(pen=None, eos=-1, done=None)),
                    (_con(stop=[[1]]), dict(pen=_pen(ld_hist=9, gen_start=[5, 9], hist_row=[1, 1]))),
                    (_con(), {}), (None, {})):
        assert _sample(lib, con, **kw) == 22 and b"must not be NULL" in lib.gpt2mi_last_error(), lib.gpt2mi_last_error()


@needs_lib
def test_neutral_constraints_refuse_with_sample_logprobs_words(lib):
    """con NULL or all-neutral is gpt2mi_sample_logprobs: the same refusals word for word, under this entry's name."""
    for con in (None, _con(), _con(bias=8, bias_row=[-1, -1])):
        for kw in (dict(ldl=500), dict(pos=(5, -1)), dict(pen=_pen(rp=1.3, hist=None)), dict(pen=_pen(rp=1.3, ld_hist=8)), {}):
            assert _sample(lib, con, **kw) == 22
            mine = lib.gpt2mi_last_error()
            assert _sample(lib, None, entry="gpt2mi_sample_logprobs", **kw) == 22
            theirs = lib.gpt2mi_last_error()
            assert mine.startswith(b"sample_constrained: ") and theirs.startswith(b"sample_logprobs: ")
            assert mine.split(b": ", 1)[1] == theirs.split(b": ", 1)[1]


@needs_lib
def test_decode_generate_constrained_refuses_bad_arguments(lib):
    from gpt_2_distributed_amd import _lib
    plan = _lib.DecodePlan()
    plan.B, plan.C, plan.H, plan.L, plan.Vp, plan.Tcap = 2, 128, 2, 1, 512, 64

    def gen(con, entry=NEW[1], seq=8, ld_seq=64, pos0=(5, 9), n=4, eos=7, done=8, gen_start=None, rp=1.0):
        pos_a = (ctypes.c_int * 2)(*pos0)
        gs = None if gen_start is None else (ctypes.c_int * 2)(*gen_start)
        head = (ctypes.byref(plan), 509, 1.0, 0, 1.0, 0, eos, pos_a, None, n, None, seq, ld_seq, done, None, rp, 0.0, 0.0, gs,
                None)
        if entry == NEW[1]:
            return lib.gpt2mi_decode_generate_constrained(*head, None if con is None else ctypes.byref(con))
        return lib.gpt2mi_decode_generate_logprobs(*head)
    for ckw, kw, words in REFUSALS:
        assert gen(_con(**ckw), **kw) == 22, (ckw, kw)
        msg = lib.gpt2mi_last_error()
        assert msg.startswith(b"decode_generate_constrained: ") and all(w in msg for w in words), (ckw, kw, msg)
    for ckw, kw, words in ((dict(stop=[[1]]), dict(seq=None), [b"seq", b"NULL"]),
                           (dict(min_new=2), dict(gen_start=[6, 0]), [b"gen_start[0]=6"]),
                           (dict(min_p=0.5), dict(ld_seq=12), [b"ld_seq"]), (dict(min_p=0.5), dict(pos0=(0, 9)), [b"prefill"]),
                           (dict(min_p=0.5), dict(rp=0.0), [b"repetition"])):
        assert gen(_con(**ckw), **kw) == 22, (ckw, kw)
        msg = lib.gpt2mi_last_error()
        assert msg.startswith(b"decode_generate_constrained: ") and all(w in msg for w in words), (ckw, kw, msg)
    # valid: the pointer check (tok is NULL); without stop sequences no seq is needed
    for con, kw in ((_con(min_p=0.5, min_new=3, stop=[[1, 2]], bias=8), {}), (_con(min_p=0.5), dict(seq=None, ld_seq=0)),
                    (_con(), {}), (None, {})):
        assert gen(con, **kw) == 22 and b"must not be NULL" in lib.gpt2mi_last_error(), lib.gpt2mi_last_error()
    # neutral: gpt2mi_decode_generate_logprobs' refusals word for word
    for kw in (dict(ld_seq=12), dict(pos0=(0, 9)), dict(rp=1.3, seq=None), {}):
        assert gen(_con(), **kw) == 22
        mine = lib.gpt2mi_last_error()
        assert gen(None, entry="gpt2mi_decode_generate_logprobs", **kw) == 22
        theirs = lib.gpt2mi_last_error()
        assert mine.split(b": ", 1)[1] == theirs.split(b": ", 1)[1] and mine.startswith(b"decode_generate_constrained: ")


# ---- register budget ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_constrained_kernels_have_no_scratch_and_no_spills():
    """The constrained kernels are a unit of their own (sample.hip and sample_lp.hip keep the kernels they had: their
    own tests count them): one per (greedy, penalised, LP) form, each with the row in registers."""
    res = _resources("sample_con.hip")
    assert len(res) == 8 and all("constrained_kernel" in k for k in res), sorted(res)
    for k, v in res.items():
        assert v["ScratchSize [bytes/lane]"] == 0, f"{k}: scratch {v}"
        assert v["VGPRs Spill"] == 0, f"{k}: spills {v}"


# ---- the speculative loop over a stub session ----------------------------------------------------------------------------
class SpecStub:
    """speculate_loop's session surface on the CPU: the token after a history is a fixed function of its last token."""

    def __init__(self, lens):
        self.B, self.lens = len(lens), list(lens)
        self.accepted = []

    @staticmethod
    def nxt(t):
        return (3 * t + 1) % 211

    def _verify(self, toks, seqs, poss, keys, sampler):
        return [self.nxt(t) for t in toks]

    def _accept(self, src, dst):
        self.accepted.append((list(src), list(dst)))


@pytest.mark.parametrize("k", [0, 1, 4])
def test_speculate_loop_ends_a_run_at_the_token_that_completes_a_stop(k):
    prompts = [[1, 2, 5], [7]]
    n = 12
    chain = lambda t, m: [t] if m == 1 else [t] + chain(SpecStub.nxt(t), m - 1)  # noqa: E731
    plain = [chain(SpecStub.nxt(p[-1]), n) for p in prompts]
    # row 0 stops in the middle of what a 4-token draft run accepts; row 1 has no match in its generated part
    stops = [plain[0][5:7], [prompts[1][-1], plain[1][0]]]
    want0 = plain[0][:7]
    assert first_stop(prompts[0] + plain[0], 3, stops) == 3 + 6 and first_stop(prompts[1] + plain[1], 1, stops) is None

    def draft(history, m):  # always right
        return chain(SpecStub.nxt(history[-1]), m) if m > 0 else []
    sess = SpecStub([len(p) for p in prompts])
    stopped = [False, False]
    new, stats = generation.speculate_loop(sess, n, k, draft, None, [list(p) for p in prompts],
                                           [plain[0][0], plain[1][0]], [0, 1], (0.0, None, None, 0),
                                           stop=(stops, [3, 1], 0), stopped=stopped)
    assert new[0] == want0 and new[1] == plain[1] and stopped == [True, False]
    assert sess.lens[0] == len(prompts[0]) + len(want0) - 1 and stats["tokens"] == len(want0) + n
    # the gate: with min_new_tokens above the match the row runs on
    sess = SpecStub([len(p) for p in prompts])
    new, _ = generation.speculate_loop(sess, n, k, draft, None, [list(p) for p in prompts], [plain[0][0], plain[1][0]],
                                       [0, 1], (0.0, None, None, 0), stop=(stops, [3, 1], 8))
    assert new == plain
    # a stop completed by the first token, drawn before the loop
    sess = SpecStub([len(p) for p in prompts])
    stopped = [False, False]
    new, _ = generation.speculate_loop(sess, n, k, draft, None, [list(p) for p in prompts], [plain[0][0], plain[1][0]],
                                       [0, 1], (0.0, None, None, 0), stop=([[plain[0][0]]], [3, 1], 0), stopped=stopped)
    assert new[0] == plain[0][:1] and stopped[0]
