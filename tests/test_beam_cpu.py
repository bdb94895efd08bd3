"""Beam search without a GPU: the selection rule (generation.beam_select) on hand-worked cases, the final ranking
(generation.beam_rank) and what is returned of it (generation.beam_pick), every argument refusal of
generate(num_beams=) and of the C entries (called with NULL pointers, so nothing launches), the ABI numbers, and the
register budget of the kernels of csrc/beam.hip."""
import ctypes
import os
import re
import shutil
import types

import numpy as np
import pytest
import torch

from gpt_2_distributed_amd import _lib, generation
from gpt_2_distributed_amd.generation import beam_rank, beam_select
from tests.conftest import REPO
from tests.test_kernel_resources import HIPCC, _resources

LIB = os.path.join(REPO, "gpt_2_distributed_amd", "libgpt2mi.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libgpt2mi.so not built (run __graft_entry__.build())")
NINF = float("-inf")


def f32(*v):
    return np.array(v, dtype=np.float32)


def select(cum, done, ids, lps, eos, W):
    return [a.tolist() for a in beam_select(cum, done, ids, lps, eos, W)]


# ---- the rule ---------------------------------------------------------------------------------------------------------
def test_one_beam_is_the_argmax():
    tok, parent, cum, done = select([-1.5, -0.25], [0, 0], [[7], [3]], [[-0.5], [-2.0]], -1, 1)
    assert tok == [7, 3] and parent == [0, 1] and done == [0, 0]
    assert cum == [float(np.float32(-1.5) + np.float32(-0.5)), float(np.float32(-0.25) + np.float32(-2.0))]


def test_the_first_step_expands_only_beam_zero():
    ids = [[4, 9, 2]] * 3  # forks of one prefill: identical rows
    lps = [[-0.1, -1.0, -3.0]] * 3
    tok, parent, cum, done = select([0.0, NINF, NINF], [0, 0, 0], ids, lps, -1, 3)
    assert tok == [4, 9, 2] and parent == [0, 0, 0] and done == [0, 0, 0]
    assert cum == f32(-0.1, -1.0, -3.0).tolist()


def test_a_finished_beam_keeps_its_score_and_emits_eos():
    # beam 0 is finished at -1.0; beam 1 offers -0.5 - 0.2 = -0.7 and -0.5 - 2.0 = -2.5
    tok, parent, cum, done = select([-1.0, -0.5], [1, 0], [[8, 9], [5, 6]], [[-0.1, -0.2], [-0.2, -2.0]], 3, 2)
    assert tok == [5, 3] and parent == [1, 0] and done == [0, 1]
    assert cum == [float(np.float32(-0.5) + np.float32(-0.2)), -1.0]


def test_a_beam_that_draws_eos_finishes():
    tok, parent, cum, done = select([0.0, -9.0], [0, 0], [[3, 1], [1, 2]], [[-0.5, -0.7], [-0.1, -0.2]], 3, 2)
    assert tok == [3, 1] and parent == [0, 0] and done == [1, 0]


def test_without_eos_nothing_is_finished():
    # eos = -1: the done flags are not read and none is set, even for a token that equals -1's stand-in
    tok, parent, cum, done = select([-1.0, -0.5], [1, 0], [[8, 9], [5, 6]], [[-0.1, -0.2], [-0.2, -2.0]], -1, 2)
    assert tok == [5, 8] and parent == [1, 0] and done == [0, 0]
    assert select([-1.0, -0.5], [1, 0], [[8, 9], [5, 6]], [[-0.1, -0.2], [-0.2, -2.0]], None, 2)[0] == [5, 8]


def test_equal_scores_resolve_by_beam_then_rank():
    # all four candidates score -1: (beam 0, rank 0), (0, 1), (1, 0), (1, 1)
    tok, parent, cum, done = select([-0.5, -0.5], [0, 0], [[10, 11], [12, 13]], [[-0.5, -0.5]] * 2, -1, 2)
    assert tok == [10, 11] and parent == [0, 0]
    # beam 1's best ties with beam 0's second: beam 0 goes first although its token id is the larger
    tok, parent, cum, done = select([-0.5, -1.0], [0, 0], [[99, 98], [1, 2]], [[-0.25, -1.0], [-0.5, -0.75]], -1, 2)
    assert cum == [-0.75, -1.5] and tok == [99, 98] and parent == [0, 0]
    # -0.0 and +0.0 are one score
    tok, parent, cum, done = select([0.0, -0.0], [0, 0], [[5, 6], [7, 8]], [[-0.0, -1.0], [0.0, -1.0]], -1, 2)
    assert tok == [5, 7] and parent == [0, 1]
    # -inf scores come last, by (beam, rank)
    tok, parent, cum, done = select([NINF, -3.0, NINF], [0] * 3, [[1, 2, 3]] * 3, [[-0.1, -0.2, NINF]] * 3, -1, 3)
    assert tok == [1, 2, 1] and parent == [1, 1, 0] and cum[2] == NINF


def test_two_ranks_of_one_beam_can_round_to_one_score():
    """|cum| = 4096 has an fp32 spacing of 2^-11 there: two log-probabilities one ulp apart give one score, and the
    lower rank goes first. A rule over token ids would pick token 3 before token 40."""
    a = np.float32(-1.0)
    b = np.nextafter(a, np.float32(-2.0))
    assert a != b and np.float32(-4096.0) + a == np.float32(-4096.0) + b
    tok, parent, cum, done = select([-4096.0, -4096.0], [0, 0], [[40, 3], [40, 3]], [[a, b]] * 2, -1, 2)
    assert tok == [40, 3] and parent == [0, 0] and cum[0] == cum[1] == -4097.0


def test_groups_are_independent():
    one = beam_select([0.0, NINF], [0, 0], [[4, 9]] * 2, [[-0.1, -1.0]] * 2, -1, 2)
    two = beam_select([-2.0, -1.0], [0, 0], [[1, 2], [3, 4]], [[-0.5, -0.6], [-0.1, -3.0]], -1, 2)
    both = beam_select([0.0, NINF, -2.0, -1.0], [0] * 4, [[4, 9]] * 2 + [[1, 2], [3, 4]],
                       [[-0.1, -1.0]] * 2 + [[-0.5, -0.6], [-0.1, -3.0]], -1, 2)
    assert both[0].tolist() == one[0].tolist() + two[0].tolist()
    assert both[1].tolist() == one[1].tolist() + (two[1] + 2).tolist()
    assert both[2].tolist() == one[2].tolist() + two[2].tolist()
    with pytest.raises(ValueError, match="G \\* W"):
        beam_select([0.0] * 3, [0] * 3, [[1, 2]] * 3, [[0.0, 0.0]] * 3, -1, 2)


# ---- the final ranking ------------------------------------------------------------------------------------------------
def test_ranking_with_the_length_penalty():
    cum, lengths = [[-6.0, -4.0, -4.5]], [[6, 2, 3]]
    order, score = beam_rank(cum, lengths, 0.0)  # the raw sum
    assert order.tolist() == [[1, 2, 0]] and score.tolist() == [[-6.0, -4.0, -4.5]]
    order, score = beam_rank(cum, lengths, 1.0)  # the mean
    assert order.tolist() == [[0, 2, 1]] and score.tolist() == [[-1.0, -2.0, -1.5]]
    order, score = beam_rank(cum, lengths, 2.0)
    assert order.tolist() == [[0, 2, 1]] and score.tolist() == [[-6.0 / 36, -1.0, -0.5]]
    assert score.dtype == torch.float64
    order, score = beam_rank([[-1.0, -2.0, -1.0]], [[1, 2, 1]], 1.0)  # equal scores: by beam index
    assert order.tolist() == [[0, 1, 2]]
    assert beam_rank([[-3.0]], [[0]], 1.0)[1].tolist() == [[-3.0]]  # max(length, 1)


def test_what_is_returned_is_the_head_of_the_ranking():
    """beam_pick: every field of entry [b, i] belongs to the beam that beam_rank puts i-th, and fewer returned
    sequences are the first entries of more. The penalty reorders the beams, and differently per prompt."""
    W, T = 4, 6
    tokens = torch.arange(2 * W * T).view(2 * W, T)  # row r holds r * T ..: a row names its beam
    cum = torch.tensor([-6.0, -4.0, -4.5, -9.0, -2.0, -8.0, -3.0, -2.5])
    lengths = torch.tensor([6, 2, 3, 3, 1, 6, 3, 2])
    for lp, want in ((0.0, [[1, 2, 0, 3], [0, 3, 2, 1]]), (1.0, [[0, 2, 1, 3], [2, 3, 1, 0]]),
                     (2.0, [[0, 2, 1, 3], [1, 2, 3, 0]])):
        full = generation.beam_pick(tokens, cum, lengths, W, lp, W)
        order, score = beam_rank(cum.view(2, W), lengths.view(2, W), lp)
        assert order.tolist() == want, lp
        for b in range(2):
            for i, j in enumerate(want[b]):
                r = b * W + j
                assert torch.equal(full.tokens[b, i], tokens[r]) and full.cum_logprob[b, i] == cum[r]
                assert full.lengths[b, i] == lengths[r] and full.scores[b, i] == score[b, j]
                assert full.scores[b, i] == float(cum[r]) / float(lengths[r]) ** lp
            assert bool((full.scores[b, :-1] >= full.scores[b, 1:]).all())
        for r in (1, 2, 3):
            part = generation.beam_pick(tokens, cum, lengths, W, lp, r)
            assert part.tokens.shape == (2, r, T) and part.scores.dtype == torch.float64
            for got, ref in zip(part, full):
                assert torch.equal(got, ref[:, :r]), (lp, r)
    assert generation.beam_pick(tokens, cum, lengths, W).tokens.shape == (2, 1, T)  # the defaults: the best beam, mean
    assert torch.equal(generation.beam_pick(tokens, cum, lengths, W).tokens[:, 0], tokens[[0, 6]])
    for bad in (dict(W=3), dict(W=4, num_return_sequences=0), dict(W=4, num_return_sequences=5)):
        with pytest.raises(ValueError, match="beam_pick"):
            generation.beam_pick(tokens, cum, lengths, **bad)


# ---- generate's refusals: a stub model, no device ----------------------------------------------------------------------
STUB = types.SimpleNamespace(config=types.SimpleNamespace(vocab_size=12, n_positions=64))
IDX = torch.zeros(4, 3, dtype=torch.int64)


@pytest.mark.parametrize("kw, words", [
    (dict(num_beams=0), "num_beams"), (dict(num_beams=21), "num_beams"), (dict(num_beams=13), "vocab_size"),
    (dict(num_beams=4, num_return_sequences=0), "num_return_sequences"),
    (dict(num_beams=4, num_return_sequences=5), "num_return_sequences"),
    (dict(num_beams=2, length_penalty=float("inf")), "length_penalty"),
    (dict(num_beams=2, length_penalty=float("nan")), "length_penalty"),
    (dict(num_beams=2, seed=0), "seed"), (dict(num_beams=2, generator=torch.Generator()), "generator"),
    (dict(num_beams=2, temperature=0.5), "temperature"), (dict(num_beams=2, temperature=0.0), "temperature"),
    (dict(num_beams=2, top_k=5), "top_k"), (dict(num_beams=2, top_p=0.9), "top_p"),
    (dict(num_beams=2, repetition_penalty=1.1), "repetition_penalty"),
    (dict(num_beams=2, presence_penalty=0.5), "presence_penalty"),
    (dict(num_beams=2, frequency_penalty=0.5), "frequency_penalty"),
    (dict(num_beams=2, draft_tokens=2), "draft_tokens"), (dict(num_beams=2, num_samples=2), "num_samples"),
    (dict(num_beams=2, logprobs=True), "logprobs"), (dict(num_beams=2, logprobs=0), "logprobs"),
    (dict(length_penalty=2.0), "num_beams"), (dict(num_return_sequences=2), "num_beams"),
])
def test_generate_refuses_by_name(kw, words):
    with pytest.raises(ValueError, match=words):
        generation.generate(STUB, IDX, 4, **kw)


def test_generate_refuses_more_than_64_rows():
    big = types.SimpleNamespace(config=types.SimpleNamespace(vocab_size=100, n_positions=64))
    with pytest.raises(ValueError, match="num_beams=17.*64"):
        generation.generate(big, IDX, 4, num_beams=17)
    with pytest.raises(ValueError, match="num_beams=20.*80 rows"):
        generation.generate(big, IDX, 4, num_beams=20)


def test_cli_flags_and_lines():
    from gpt_2_distributed_amd import generate as cli
    a = cli.parse_args(["--checkpoint", "x", "--num_beams", "4", "--length_penalty", "0.5", "--num_return_sequences", "2"])
    assert (a.num_beams, a.length_penalty, a.num_return_sequences) == (4, 0.5, 2)
    assert cli.parse_args(["--checkpoint", "x"]).num_beams is None
    out = generation.BeamOutput(torch.tensor([[[5, 6, 7, 0], [5, 8, 9, 1]]]), torch.tensor([[-0.5, -1.0]], dtype=torch.float64),
                                torch.tensor([[-1.0, -2.0]]), torch.tensor([[1, 2]]))
    assert cli.beam_lines(out, [2]) == [
        {"prompt": 0, "beam": 0, "tokens": [5, 6, 7], "score": -0.5, "cum_logprob": -1.0},
        {"prompt": 0, "beam": 1, "tokens": [5, 8, 9, 1], "score": -1.0, "cum_logprob": -2.0}]


def test_cli_refuses_the_device_sampler_by_its_own_name():
    from gpt_2_distributed_amd import generate as cli
    with pytest.raises(SystemExit, match="--sampler device"):  # (before the checkpoint is opened)
        cli.main(["--checkpoint", "nowhere", "--num_beams", "4", "--sampler", "device"])


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
ENTRIES = ("gpt2mi_beam_select", "gpt2mi_beam_reorder", "gpt2mi_decode_beam_search", "gpt2mi_beam_reorder_workspace")


@needs_lib
def test_abi_numbers_and_exports():
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "gpt2mi.h")).read()
    assert lib.gpt2mi_abi_version() == 24
    minor = int(re.search(r"#define GPT2MI_ABI_MINOR (\d+)", hdr).group(1))
    assert lib.gpt2mi_abi_minor() == minor >= 2 and _lib.ABI_MINOR >= 2
    raw = ctypes.CDLL(LIB)
    for name in ENTRIES:
        assert hasattr(raw, name) and name in _lib.EXPORTED and _lib._SINCE_MINOR[name] == 2
        assert getattr(lib, name).argtypes == _lib._SIGS[name]
    assert lib.gpt2mi_beam_reorder_workspace.restype is ctypes.c_size_t
    loop = int(re.search(r"#define GPT2MI_DECODE_MAX_B (\d+)", hdr).group(1)) * (
        8 * int(re.search(r"#define GPT2MI_LOGPROBS_MAX_TOP (\d+)", hdr).group(1)) + 4)
    assert _lib.BEAM_LOOP_BYTES == loop and loop % 16 == 0


@needs_lib
def test_reorder_workspace_query():
    q = _lib.beam_reorder_workspace
    # R rows x window positions of: L layers x (K, V) x H heads of 128-byte rows (bf16), or 64 + 4 (fp8); 8 per token
    assert q(_lib.KV_BF16, 2, 3, 4, 65) == 4 * 65 * (2 * 2 * 3 * 128 + 8)
    assert q(_lib.KV_FP8, 2, 3, 4, 65) == 4 * 65 * (2 * 2 * 3 * 68 + 8)
    assert q(_lib.KV_BF16, 12, 12, 64, 0) == 0
    for bad in ((2, 1, 1, 1, 1), (0, 0, 1, 1, 1), (0, 1, 0, 1, 1), (0, 1, 1, 0, 1), (0, 1, 1, 1, -1)):
        assert q(*bad) == 0


def refused(lib, name, rc, words=()):
    msg = lib.gpt2mi_last_error()
    assert rc == 22 and name.encode() in msg and all(w.encode() in msg for w in words), (name, rc, msg)


@needs_lib
def test_select_refusals():
    lib = _lib.load()
    nul = (None,) * 4

    def call(G, W, eos):
        return lib.gpt2mi_beam_select(*nul, G, W, eos, *nul, None)
    for W in (0, 21, -1):
        refused(lib, "beam_select", call(1, W, -1), ["W="])
    for G, W in ((0, 4), (17, 4), (4, 17), (-1, 2)):
        refused(lib, "beam_select", call(G, W, -1), ["rows"])
    refused(lib, "beam_select", call(2, 4, -2), ["eos"])
    refused(lib, "beam_select", call(2, 4, 5), ["NULL"])


@needs_lib
def test_reorder_refusals():
    lib = _lib.load()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    ok = dict(fmt=0, L=2, rows=4 * 3 * 96, B=4, H=3, Tcap=96, ld=96, G=2, W=2, lo=ints(5, 5, 7, 7), hi=ints(70, 70, 9, 9), ws=1 << 30)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gpt2mi_beam_reorder(None, None, None, None, a["fmt"], a["L"], a["rows"], a["B"], a["H"], a["Tcap"], None,
                                       a["ld"], None, a["G"], a["W"], a["lo"], a["hi"], None, a["ws"], None)
    refused(lib, "beam_reorder", call(W=0), ["W="])
    refused(lib, "beam_reorder", call(W=21, G=1), ["W="])
    refused(lib, "beam_reorder", call(G=0), ["rows"])
    refused(lib, "beam_reorder", call(G=33), ["rows"])
    refused(lib, "beam_reorder", call(fmt=2), ["kv_format"])
    refused(lib, "beam_reorder", call(B=3), ["B=3"])
    refused(lib, "beam_reorder", call(H=0), ["H=0"])
    refused(lib, "beam_reorder", call(rows=4 * 3 * 96 - 1), ["layer_rows"])
    refused(lib, "beam_reorder", call(lo=None), ["lo and hi"])
    refused(lib, "beam_reorder", call(hi=ints(70, 70, 9, 97)), ["hi[3]=97"])
    refused(lib, "beam_reorder", call(lo=ints(5, 5, 10, 10)), ["lo[2]=10"])
    refused(lib, "beam_reorder", call(lo=ints(-1, -1, 7, 7)), ["lo[0]=-1"])
    refused(lib, "beam_reorder", call(hi=ints(70, 69, 9, 9)), ["differs from its group"])
    refused(lib, "beam_reorder", call(ws=100), ["workspace too small"])
    refused(lib, "beam_reorder", call(), ["NULL"])
    refused(lib, "beam_reorder", call(fmt=1), ["kscale"])


@needs_lib
def test_loop_refusals():
    lib = _lib.load()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    plan = _lib.DecodePlan()
    plan.B, plan.C, plan.H, plan.L, plan.Vp, plan.Tcap = 4, 128, 2, 2, 512, 96

    def call(P=plan, V=509, W=2, eos=-1, pos0=ints(9, 9, 5, 5), lo=ints(9, 9, 3, 3), n=4, ld=96):
        return lib.gpt2mi_decode_beam_search(None if P is None else P.ref(), V, W, eos, pos0, lo, n, None, None, ld, None,
                                             None, None, None, 0, None)
    name = "decode_beam_search"
    refused(lib, name, call(P=None), ["plan is NULL"])
    refused(lib, name, call(W=3), ["groups of W=3"])
    refused(lib, name, call(W=0), ["W=0"])
    refused(lib, name, call(V=0), ["V=0"])
    refused(lib, name, call(V=513), ["V=513"])
    refused(lib, name, call(V=1, W=2), ["above V"])
    refused(lib, name, call(eos=509), ["eos"])
    refused(lib, name, call(eos=-2), ["eos"])
    refused(lib, name, call(n=-1), ["n=-1"])
    refused(lib, name, call(pos0=None), ["pos0 and lo"])
    refused(lib, name, call(pos0=ints(0, 0, 5, 5)), ["pos0[0]=0"])
    refused(lib, name, call(lo=ints(10, 10, 3, 3)), ["lo[0]=10"])
    refused(lib, name, call(lo=ints(9, 9, 0, 0)), ["lo[2]=0"])
    refused(lib, name, call(pos0=ints(9, 10, 5, 5)), ["differs from its group"])
    refused(lib, name, call(n=88), ["Tcap"])
    refused(lib, name, call(ld=12), ["ld_seq"])
    refused(lib, name, call(), ["NULL"])
    wide = _lib.DecodePlan()
    wide.B, wide.C, wide.H, wide.L, wide.Vp, wide.Tcap = 63, 128, 2, 2, 512, 96
    refused(lib, name, lib.gpt2mi_decode_beam_search(wide.ref(), 509, 21, -1, None, None, 1, None, None, 96, None, None,
                                                     None, None, 0, None), ["W=21"])


# ---- the kernels' register budget -------------------------------------------------------------------------------------
@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_beam_kernels_have_no_scratch_and_no_spills():
    kernels = {k: v for k, v in _resources("beam.hip").items() if "beam_" in k}
    assert len(kernels) == 6, sorted(kernels)  # top-W, select, and the two halves of the reorder per cache format
    for k, v in kernels.items():
        assert v["ScratchSize [bytes/lane]"] == 0, f"{k}: scratch {v}"
        assert v["VGPRs Spill"] == 0, f"{k}: spills {v}"
        # the top-W kernel is a 1024-thread workgroup like the sampler (4 waves a SIMD); the others are small
        assert v["Occupancy [waves/SIMD]"] >= (4 if "topw" in k else 8), f"{k}: occupancy {v}"
