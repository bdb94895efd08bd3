"""Token log-probabilities without a GPU: the rule (generation.token_logprobs) against torch.log_softmax in float64 and
its tie order, the minor ABI number and the two new entries, every refusal of gpt2mi_sample_logprobs /
gpt2mi_decode_generate_logprobs (NULL or never-dereferenced pointers: nothing is launched), the bookkeeping of
speculate_loop and serve_prompts with log-probabilities over stub sessions, and the register budget of every sampling
kernel."""
import ctypes
import inspect
import os
import shutil

import pytest
import torch

from gpt_2_distributed_amd import generation
from gpt_2_distributed_amd.generation import LogprobBuffer, token_logprobs
from tests.conftest import REPO
from tests.test_kernel_resources import HIPCC, _resources

LIB = os.path.join(REPO, "gpt_2_distributed_amd", "libgpt2mi.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libgpt2mi.so not built (run __graft_entry__.build())")


# ---- the rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 2, 37, 509])
def test_token_logprobs_is_log_softmax_in_float64(V):
    g = torch.Generator().manual_seed(V)
    logits = torch.randn(6, V, generator=g) * 3
    tokens = torch.randint(0, V, (6,), generator=g)
    want = torch.log_softmax(logits.double(), dim=-1)
    n = min(5, V)
    lp, ids, top = token_logprobs(logits, tokens, n)
    assert lp.dtype == top.dtype == torch.float64 and ids.dtype == torch.int64
    assert lp.shape == (6,) and ids.shape == top.shape == (6, n)
    torch.testing.assert_close(lp, want.gather(1, tokens[:, None])[:, 0], rtol=0, atol=1e-12)
    order = torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, :n]
    assert torch.equal(ids, order)
    torch.testing.assert_close(top, want.gather(1, order), rtol=0, atol=1e-12)
    assert bool((top[:, :-1] >= top[:, 1:]).all())
    # without tokens; several leading dimensions; bf16 logits are taken as the fp32 values they are
    none, ids2, top2 = token_logprobs(logits, None, n)
    assert none is None and torch.equal(ids2, ids) and torch.equal(top2, top)
    lp3, ids3, top3 = token_logprobs(logits.view(2, 3, V), tokens.view(2, 3), n)
    assert torch.equal(lp3.view(6), lp) and torch.equal(ids3.view(6, n), ids) and torch.equal(top3.view(6, n), top)
    assert torch.equal(token_logprobs(logits.bfloat16(), tokens, n)[0], token_logprobs(logits.bfloat16().float(), tokens, n)[0])
    if V == 1:
        assert float(lp[0]) == 0.0 and float(top[0, 0]) == 0.0


def test_value_does_not_depend_on_anything_but_the_row():
    """Large logits do not overflow (the maximum is subtracted first) and a row gives the same bits alone and in a batch."""
    logits = torch.tensor([[80.0, -80.0, 79.0, 0.0], [-80.0, -80.0, -80.0, -80.0]])
    lp, ids, top = token_logprobs(logits, torch.tensor([0, 3]), 2)
    assert torch.isfinite(lp).all() and abs(float(lp[1]) + 1.3862943611198906) < 1e-12
    assert ids.tolist() == [[0, 2], [0, 1]]
    alone = token_logprobs(logits[:1], torch.tensor([0]), 2)
    assert torch.equal(alone[0], lp[:1]) and torch.equal(alone[2], top[:1])


def test_equal_values_are_ordered_by_index_and_minus_inf_comes_last():
    ninf = float("-inf")
    #                      0    1    2    3     4    5    6    7     8
    row = torch.tensor([[1.0, 5.0, 5.0, ninf, 0.0, -0.0, 5.0, ninf, 1.0]])
    _, ids, top = token_logprobs(row, None, 9)
    assert ids.tolist() == [[1, 2, 6, 0, 8, 4, 5, 3, 7]]      # -0 == +0: by index; the -inf entries last, by index
    assert top[0, -2:].tolist() == [ninf, ninf] and bool(torch.isfinite(top[0, :7]).all())
    # a tie that straddles the n-th place: the lower indices are taken
    assert token_logprobs(row, None, 2)[1].tolist() == [[1, 2]]
    assert token_logprobs(row, None, 4)[1].tolist() == [[1, 2, 6, 0]]
    # duplicates injected into random rows
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(4, 300, generator=g) * 3
    where = logits.argmax(dim=1).tolist()
    logits[:, 200] = logits[:, 17] = logits.max(dim=1).values   # the maximum, three times
    logits[:, [250, 40, 41]] = logits[:, [7]]
    _, ids, top = token_logprobs(logits, None, 20)
    for b in range(4):
        assert ids[b, :3].tolist() == sorted({17, 200, where[b]}) and len({17, 200, where[b]}) == 3
        want = sorted(range(300), key=lambda i: (-float(logits[b, i]), i))[:20]
        assert ids[b].tolist() == want


def test_top_n_bounds():
    logits = torch.zeros(2, 7)
    assert token_logprobs(logits, None, 0)[1].shape == (2, 0) and token_logprobs(logits, None, 7)[1].shape == (2, 7)
    for bad in (-1, 8):
        with pytest.raises(ValueError, match="top_n"):
            token_logprobs(logits, None, bad)
    with pytest.raises(ValueError, match="tokens"):
        token_logprobs(logits, torch.zeros(3, dtype=torch.long))
    with pytest.raises(ValueError, match="top_n"):
        LogprobBuffer(1, 4, 21, "cpu")
    with pytest.raises(ValueError, match="top_n"):
        LogprobBuffer(1, 4, -1, "cpu")
    buf = LogprobBuffer(2, 4, 20, "cpu")
    assert buf.logprob.shape == (2, 4) and buf.top_ids.shape == buf.top_logprobs.shape == (2, 4, 20)
    assert buf.top_ids.dtype == torch.int32 and buf.logprob.dtype == buf.top_logprobs.dtype == torch.float32


def test_interface_has_the_parameter_and_it_is_off_by_default():
    from gpt_2_distributed_amd.model import GPT2, GPT2Config
    from gpt_2_distributed_amd.generation import DecodeSession
    for fn in (GPT2.generate, GPT2.generate_many, generation.generate, generation.generate_many, DecodeSession.sample,
               DecodeSession.generate, DecodeSession.speculate, generation.speculate_loop, generation.serve_prompts):
        assert inspect.signature(fn).parameters["logprobs"].default is None, fn
    model = GPT2(GPT2Config(n_layer=1, n_head=1, n_embd=64, vocab_size=64, n_positions=16))
    idx = torch.zeros(1, 2, dtype=torch.long)
    for bad in (21, -1):
        with pytest.raises(ValueError, match="logprobs"):
            model.generate(idx, 2, seed=0, logprobs=bad)
        with pytest.raises(ValueError, match="logprobs"):
            model.generate_many([idx[0]], 2, logprobs=bad)
    with pytest.raises(RuntimeError, match="cuda"):           # valid values reach _check_model's refusal of a CPU model
        model.generate(idx, 2, seed=0, logprobs=5)
    # nothing to generate: the tokens, and no values
    out = model.generate_many([idx[0]], 0, logprobs=True)[0]
    assert torch.equal(out.tokens, idx[0]) and out.logprobs.shape == (2,) and out.top_ids.shape == (2, 0)
    assert out._fields == ("tokens", "logprobs", "top_ids", "top_logprobs")
    out = model.generate_many([idx[0]], 0, logprobs=3)[0]
    assert torch.equal(out.tokens, idx[0]) and out.top_logprobs.shape == (2, 3) and float(out.logprobs.sum()) == 0.0


def test_cli_has_the_flag():
    from gpt_2_distributed_amd.generate import parse_args, with_logprobs
    assert parse_args(["--checkpoint", "x"]).logprobs is None
    assert parse_args(["--checkpoint", "x", "--logprobs"]).logprobs == 0
    assert parse_args(["--checkpoint", "x", "--logprobs", "5", "--sampler", "device"]).logprobs == 5
    out = generation.GenerateOutput(torch.tensor([[7, 8, 9, 3]]), torch.tensor([[0.0, 0.0, -1.5, -0.25]]),
                                    torch.tensor([[[0, 0], [0, 0], [9, 1], [2, 3]]], dtype=torch.int32),
                                    torch.tensor([[[0.0, 0.0], [0.0, 0.0], [-1.5, -2.0], [-0.125, -0.25]]]))
    line = with_logprobs([7, 8, 9, 3], out, 0, 2, 4, 2)
    assert line == {"tokens": [7, 8, 9, 3], "logprobs": [-1.5, -0.25], "cum_logprob": -1.75,
                    "top_logprobs": [[[9, -1.5], [1, -2.0]], [[2, -0.125], [3, -0.25]]]}
    line = with_logprobs({"prompt": 0, "sample": 1, "tokens": [7, 8, 9]}, out, 0, 2, 3, 0)
    assert line == {"prompt": 0, "sample": 1, "tokens": [7, 8, 9], "logprobs": [-1.5], "cum_logprob": -1.5}


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
@pytest.fixture()
def lib():
    from gpt_2_distributed_amd import _lib
    return _lib.load()


NEW = ("gpt2mi_sample_logprobs", "gpt2mi_decode_generate_logprobs")


@needs_lib
def test_abi_version_stays_and_the_minor_counts_the_addition(lib):
    from gpt_2_distributed_amd import _lib
    hdr = open(os.path.join(REPO, "include", "gpt2mi.h")).read()
    assert lib.gpt2mi_abi_version() == 24 == _lib.ABI_VERSION
    assert lib.gpt2mi_abi_minor() >= 1 and _lib.ABI_MINOR >= 1
    assert int(hdr.split("#define GPT2MI_ABI_MINOR")[1].split()[0]) == lib.gpt2mi_abi_minor()
    assert int(hdr.split("#define GPT2MI_LOGPROBS_MAX_TOP")[1].split()[0]) == _lib.LOGPROBS_MAX_TOP == 20
    for name in NEW + ("gpt2mi_abi_minor",):
        assert name in _lib.EXPORTED and hasattr(lib, name), name
    assert ctypes.sizeof(_lib.Logprobs) == 40                 # float*, int, int, int32_t*, float*, const int*


def test_a_library_without_the_minor_is_a_kernel_error_that_says_rebuild(monkeypatch):
    """A v24.0 build (no gpt2mi_abi_minor, no logprob entries) is refused by name, not by an AttributeError."""
    from gpt_2_distributed_amd import _lib

    class Fn:
        def __init__(self, value=0):
            self.value = value

        def __call__(self, *a):
            return self.value

    class Old:                                                  # a ctypes.CDLL stand-in: every v24.0 symbol, none newer
        def __init__(self, path):
            for name in _lib._SIGS:
                if name not in NEW + ("gpt2mi_abi_minor",):
                    setattr(self, name, Fn(24 if name == "gpt2mi_abi_version" else 0))

    monkeypatch.setattr(_lib.ctypes, "CDLL", Old)
    with pytest.raises(_lib.KernelError, match=r"v24\.0.*rebuild"):
        _lib.open_library("old.so")
    assert isinstance(_lib.open_library("old.so", min_minor=0), Old)    # an A/B tool may still load it


def _lp(logprob=0x1000, ld=16, top_n=5, top_id=0x2000, top_logprob=0x3000, col=None):
    """A gpt2mi_logprobs whose device pointers are never dereferenced: every call below is refused before any launch."""
    from gpt_2_distributed_amd import _lib
    keep = None if col is None else (ctypes.c_int * len(col))(*col)
    lp = _lib.Logprobs(logprob, ld, top_n, top_id, top_logprob, None if keep is None else ctypes.cast(keep, ctypes.c_void_p))
    lp._keep = keep
    return lp


def _sample(lib, lp, B=2, V=509, ldl=512, pos=(5, 9), entry="gpt2mi_sample_logprobs", pen=None):
    pos_a = (ctypes.c_int * B)(*pos)
    args = [None, ldl, B, V, 1.0, 0, 1.0, 0, pos_a, None, -1, None, None, None, 0, None,
            None if pen is None else ctypes.byref(pen), None]
    if entry == "gpt2mi_sample_logprobs":
        args.append(None if lp is None else ctypes.byref(lp))
    return getattr(lib, entry)(*args, None)


@needs_lib
def test_sample_logprobs_refuses_bad_arguments(lib):
    for kw, words in ((dict(top_n=-1), (b"top_n=-1",)), (dict(top_n=21), (b"top_n=21", b"20")),
                      (dict(logprob=None), (b"logprob is NULL",)),
                      (dict(top_id=None), (b"top_n=5", b"NULL")), (dict(top_logprob=None), (b"top_n=5", b"NULL")),
                      (dict(ld=9), (b"pos[1]=9", b"ld=9")), (dict(ld=0), (b"pos[0]=5", b"ld=0")),
                      (dict(col=[0, 16]), (b"col[1]=16", b"ld=16")), (dict(col=[-1, 0]), (b"col[0]=-1",))):
        assert _sample(lib, _lp(**kw)) == 22, kw
        msg = lib.gpt2mi_last_error()
        assert b"sample_logprobs" in msg and all(w in msg for w in words), (kw, msg)
    assert _sample(lib, _lp(top_n=4), V=3, ldl=8) == 22                  # top_n above V
    assert b"top_n=4" in lib.gpt2mi_last_error() and b"V=3" in lib.gpt2mi_last_error()
    # the forwarded checks come first, under this entry's name
    assert _sample(lib, _lp(), ldl=500) == 22 and b"sample_logprobs: ldl=500" in lib.gpt2mi_last_error()
    # valid arguments reach the pointer check, still before any launch: at the boundaries, and with top_n = 0 (the top
    # arrays are then not read)
    for lp in (_lp(), _lp(ld=10), _lp(col=[15, 0]), _lp(ld=1, col=[0, 0]), _lp(top_n=20),
               _lp(top_n=0, top_id=None, top_logprob=None)):
        assert _sample(lib, lp) == 22 and b"must not be NULL" in lib.gpt2mi_last_error(), lib.gpt2mi_last_error()
    assert _sample(lib, _lp(top_n=3), V=3, ldl=8) == 22 and b"must not be NULL" in lib.gpt2mi_last_error()


@needs_lib
def test_lp_null_refuses_with_sample_penalizeds_words_under_its_own_name(lib):
    from gpt_2_distributed_amd import _lib
    nan = float("nan")
    cases = [dict(), dict(ldl=500), dict(V=0), dict(V=60000, ldl=60000), dict(pos=(5, -1)), dict(B=65, pos=(0,) * 65),
             dict(pen=_lib.Penalties(nan, 0.0, 0.0, None, 0, 0, None, None)),
             dict(pen=_lib.Penalties(1.3, 0.0, 0.0, None, 0, 0, None, None)),
             dict(pen=_lib.Penalties(1.3, 0.0, 0.0, 8, 4, 2, None, None))]
    for kw in cases:
        assert _sample(lib, None, **kw) == 22
        mine = lib.gpt2mi_last_error()
        assert _sample(lib, None, entry="gpt2mi_sample_penalized", **kw) == 22
        theirs = lib.gpt2mi_last_error()
        assert mine.startswith(b"sample_logprobs: ") and theirs.startswith(b"sample_penalized: ")
        assert mine.split(b": ", 1)[1] == theirs.split(b": ", 1)[1], (mine, theirs)


@needs_lib
def test_decode_generate_logprobs_refuses_bad_arguments(lib):
    from gpt_2_distributed_amd import _lib
    plan = _lib.DecodePlan()
    plan.B, plan.C, plan.H, plan.L, plan.Vp, plan.Tcap = 2, 128, 2, 1, 512, 64

    def gen(lp, entry="gpt2mi_decode_generate_logprobs", pos0=(5, 9), n=4, rp=1.0, seq=None, ld_seq=0, V=509):
        pos_a = (ctypes.c_int * 2)(*pos0)
        args = [ctypes.byref(plan), V, 1.0, 0, 1.0, 0, -1, pos_a, None, n, None, seq, ld_seq, None, None, rp, 0.0, 0.0, None]
        if entry == "gpt2mi_decode_generate_logprobs":
            args.append(None if lp is None else ctypes.byref(lp))
        return getattr(lib, entry)(*args)
    for kw, words in ((dict(top_n=-1), (b"top_n=-1",)), (dict(top_n=21), (b"top_n=21",)),
                      (dict(logprob=None), (b"logprob is NULL",)), (dict(top_id=None), (b"NULL",)),
                      (dict(top_logprob=None), (b"NULL",)), (dict(col=[0, 0]), (b"col must be NULL",)),
                      (dict(ld=12), (b"max pos0=9", b"n=4", b"ld=12"))):
        assert gen(_lp(**kw)) == 22, kw
        msg = lib.gpt2mi_last_error()
        assert b"decode_generate_logprobs" in msg and all(w in msg for w in words), (kw, msg)
    assert gen(_lp(top_n=4), V=3) == 22 and b"V=3" in lib.gpt2mi_last_error()
    # valid, at the boundary ld = max pos0 + n: the pointer check, before any launch
    for lp in (_lp(), _lp(ld=13), _lp(top_n=0, top_id=None, top_logprob=None)):
        assert gen(lp) == 22 and b"must not be NULL" in lib.gpt2mi_last_error(), lib.gpt2mi_last_error()
    # lp = NULL: gpt2mi_decode_generate_penalized's refusals, word for word, under this entry's name
    for kw in (dict(), dict(pos0=(0, 9)), dict(n=-1), dict(n=60), dict(rp=float("nan")), dict(rp=1.3),
               dict(rp=1.3, seq=8, ld_seq=12), dict(V=600)):
        assert gen(None, **kw) == 22
        mine = lib.gpt2mi_last_error()
        assert gen(None, entry="gpt2mi_decode_generate_penalized", **kw) == 22
        theirs = lib.gpt2mi_last_error()
        assert mine.startswith(b"decode_generate_logprobs: ") and theirs.startswith(b"decode_generate_penalized: ")
        assert mine.split(b": ", 1)[1] == theirs.split(b": ", 1)[1], (mine, theirs)


# ---- register budget ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_every_sampling_kernel_has_no_scratch_and_no_spills():
    """The four kernels of sample.hip and the four LP ones of sample_lp.hip (the same sample_row, compiled with the
    Makefile's flags): the row stays in registers beside the prologue, whose keys must not become a second array."""
    res = {src: _resources(src) for src in ("sample.hip", "sample_lp.hip")}
    assert len(res["sample.hip"]) == 4 and len(res["sample_lp.hip"]) == 4, res
    assert sum("sample_lp_kernel" in k for k in res["sample_lp.hip"]) == 2
    assert sum("penalized_lp_kernel" in k for k in res["sample_lp.hip"]) == 2
    for src, kernels in res.items():
        for k, v in kernels.items():
            assert v["ScratchSize [bytes/lane]"] == 0, f"{src} {k}: scratch {v}"
            assert v["VGPRs Spill"] == 0, f"{src} {k}: spills {v}"
            assert v["Occupancy [waves/SIMD]"] >= 4, f"{src} {k}: occupancy {v}"   # one 1024-thread workgroup: 4 a SIMD


# ---- the speculative loop and the serving loop over stub sessions ------------------------------------------------------
def nxt(h):
    return 1 + (sum(h) * 7 + len(h)) % 89


def value(b, col, tok):
    """The stub's 'log-probability' of the token at column col of sequence b: every entry decides it, so a value in the
    wrong column or of a rejected draft shows."""
    return -(1.0 + b * 1000 + col + tok / 128.0)


class SpecStub:
    """DecodeSession's surface as speculate_loop uses it. ``want[b]`` is sequence b's true token sequence; a verify row
    sees the true tokens below the span's first position and the span's own tokens (current token, drafts) from there, so
    its token is the loop's iff the drafts before it were right. Its value is that of (sequence, the column the token
    would go to, the token)."""

    def __init__(self, want, lens):
        self.B, self.lens, self.want = len(lens), list(lens), want
        self.calls = []

    def _verify(self, toks, seqs, poss, ks, sampler, **kw):
        self.calls.append(dict(kw))
        out = []
        for r, (t, b, p) in enumerate(zip(toks, seqs, poss)):
            r0 = seqs.index(b)
            assert poss[r0] == self.lens[b] and p == self.lens[b] + r - r0
            out.append(nxt(self.want[b][:self.lens[b]] + toks[r0:r + 1]))
        if not kw:
            return out
        n = kw["logprobs"]
        vals = torch.tensor([value(b, p + 1, t) for t, b, p in zip(out, seqs, poss)], dtype=torch.float64)
        ids = torch.tensor([[t + j for j in range(n)] for t in out], dtype=torch.int64).reshape(len(out), n)
        return out, (vals, ids, vals[:, None] - torch.arange(n)[None])

    def _accept(self, src, dst):
        pass


def loop_tokens(prompt, n, eos=None):
    h = list(prompt)
    for _ in range(n):
        h.append(nxt(h))
        if h[-1] == eos:
            break
    return h


PROMPTS = [[5, 6, 7, 8], [9, 10]]


@pytest.mark.parametrize("how", ["right", "wrong", "mixed"])
@pytest.mark.parametrize("top_n", [0, 3])
def test_speculative_loop_puts_each_value_in_its_tokens_column(how, top_n):
    n, k = 12, 3
    want = [loop_tokens(p, n) for p in PROMPTS]
    calls = dict(n=0)

    def draft(history, m):
        calls["n"] += 1
        b = 0 if history[0] == 5 else 1
        right = want[b][len(history):len(history) + m]
        bad = how == "wrong" or (how == "mixed" and calls["n"] % 2 == 0)
        return [right[0] + 1] + right[1:] if bad and right else right
    sess = SpecStub(want, [4, 2])
    first = [want[0][4], want[1][2]]
    buf = LogprobBuffer(2, 4 + n + 2, top_n, "cpu")
    buf.logprob.fill_(7.0)                                     # what the loop does not write stays
    for b, p in enumerate(PROMPTS):                            # the first draw's value: the session's speculate puts it
        buf.logprob[b, len(p)] = value(b, len(p), first[b])
    before = buf.logprob.clone()
    got, stats = generation.speculate_loop(sess, n, k, draft, None, [list(p) for p in PROMPTS], first, [0, 1],
                                           (0.8, None, None, 0), logprobs=buf)
    assert [p + t for p, t in zip(PROMPTS, got)] == want
    assert sess.calls and all(c == {"logprobs": top_n} for c in sess.calls)
    if how == "wrong":
        assert stats["accepted"] == 0 and stats["drafted"] > 0       # every draft's value was dropped with its token
    if how == "right":
        assert stats["accepted"] == stats["drafted"] > 0 and stats["calls"] < n - 1
    for b, p in enumerate(PROMPTS):
        P = len(p)
        for c in range(P, P + n):
            assert float(buf.logprob[b, c]) == pytest.approx(value(b, c, want[b][c])), (b, c)
            if top_n and c > P:
                assert buf.top_ids[b, c].tolist() == [want[b][c] + j for j in range(top_n)]
                assert float(buf.top_logprobs[b, c, 1]) == pytest.approx(value(b, c, want[b][c]) - 1)
        untouched = torch.ones(buf.T, dtype=torch.bool)
        untouched[P + 1:P + n] = False
        assert torch.equal(buf.logprob[b][untouched], before[b][untouched])


def test_speculative_loop_without_logprobs_calls_verify_as_before():
    """Off: _verify gets its five positional arguments and no keyword, and returns the tokens alone (the stubs of
    tests/test_extend_cpu.py and tests/test_penalties_cpu.py, which take no more, keep working)."""
    want = [loop_tokens(p, 6) for p in PROMPTS]
    sess = SpecStub(want, [4, 2])
    got, _ = generation.speculate_loop(sess, 6, 2, lambda history, m: [], None, [list(p) for p in PROMPTS],
                                       [want[0][4], want[1][2]], [0, 1], (0.8, None, None, 0))
    assert [p + t for p, t in zip(PROMPTS, got)] == want
    assert sess.calls and all(c == {} for c in sess.calls)


def test_speculative_loop_cuts_a_row_at_eos():
    n = 12
    free = [loop_tokens(p, n) for p in PROMPTS]
    eos = free[0][4 + 5]                                        # row 0's sixth token
    want = [loop_tokens(p, n, eos) for p in PROMPTS]
    assert len(want[0]) < len(free[0])
    sess = SpecStub(free, [4, 2])
    first = [want[0][4], want[1][2]]

    def draft(history, m):
        b = 0 if history[0] == 5 else 1
        return free[b][len(history):len(history) + m]           # always right: the drafts run past the eos
    buf = LogprobBuffer(2, 4 + n, 0, "cpu")
    got, _ = generation.speculate_loop(sess, n, 3, draft, eos, [list(p) for p in PROMPTS], first, [0, 1],
                                       (0.8, None, None, 0), logprobs=buf)
    assert [p + t for p, t in zip(PROMPTS, got)] == want
    for b, p in enumerate(PROMPTS):
        for c in range(len(p) + 1, len(want[b])):
            assert float(buf.logprob[b, c]) == pytest.approx(value(b, c, want[b][c]))
        assert float(buf.logprob[b, len(want[b]):].abs().sum()) == 0.0      # nothing behind a row's eos


class ServeStub:
    """DecodeSession's surface as serve_prompts uses it, with a LogprobBuffer. The token at position p of prompt i is
    1 + (7 i + p) % 11, its value -(i + p / 64); a slot's row of the buffer must be clean when its prompt starts."""

    def __init__(self, B, Tcap):
        self.B, self.Tcap = B, Tcap
        self.lens, self.device = [0] * B, torch.device("cpu")
        self.drawn = False
        self.fresh = [False] * B
        self.kw = []

    def refill(self, row, prompt):
        self.lens[row] = prompt.numel()
        self.fresh[row] = True

    def flush(self):
        if self.drawn:
            self.lens = [n + 1 for n in self.lens]
            self.drawn = False

    def generate(self, n, temperature, top_k, top_p, seed, eos_token_id, seq, done, row_id=None, **kw):
        self.flush()
        self.kw.append(sorted(kw))
        buf = kw.get("logprobs")
        for b in range(self.B):
            if buf is not None and self.fresh[b]:
                assert float(buf.logprob[b].abs().sum()) == 0.0 and int(buf.top_ids[b].abs().sum()) == 0, b
            self.fresh[b] = False
            for i in range(n):
                p = self.lens[b] + i
                if done[b]:
                    seq[b, p] = eos_token_id
                    continue
                seq[b, p] = 1 + (7 * row_id[b] + p) % 11
                if seq[b, p] == eos_token_id:
                    done[b] = 1
                if buf is not None:
                    buf.logprob[b, p] = -(row_id[b] % 1000 + p / 64)
                    if buf.top_n:
                        buf.top_ids[b, p] = torch.arange(buf.top_n, dtype=torch.int32) + int(seq[b, p])
                        buf.top_logprobs[b, p] = buf.logprob[b, p] - torch.arange(buf.top_n)
        self.lens = [m + n - 1 for m in self.lens]
        self.drawn = True


@pytest.mark.parametrize("batch_size", [1, 2, 5])
@pytest.mark.parametrize("eos", [None, 4])
def test_serving_loop_returns_each_prompts_values_cut_where_its_tokens_are(batch_size, eos):
    n = 40                                                     # more than one chunk: rows finish apart and are refilled
    lens = [3, 11, 1, 7, 20]
    prompts = [torch.arange(100 * i + 20, 100 * i + 20 + L) for i, L in enumerate(lens)]
    sess = ServeStub(batch_size, max(lens) + n)
    outs = generation.serve_prompts(sess, prompts, n, generation.Sampler.of(0.8, 20, None, 3, eos), logprobs=2)
    plain = generation.serve_prompts(ServeStub(batch_size, max(lens) + n), prompts, n,
                                    generation.Sampler.of(0.8, 20, None, 3, eos))
    assert all(k == ["logprobs"] for k in sess.kw)
    for i, (out, L) in enumerate(zip(outs, lens)):
        assert torch.equal(out.tokens, plain[i])               # the tokens of the call without
        new = [1 + (7 * i + p) % 11 for p in range(L, L + n)]
        if eos in new:
            new = new[:new.index(eos) + 1]
        assert out.tokens.tolist() == prompts[i].tolist() + new
        T = L + len(new)
        assert out.logprobs.shape == (T,) and out.top_ids.shape == out.top_logprobs.shape == (T, 2)
        assert float(out.logprobs[:L].abs().sum()) == 0.0 and int(out.top_ids[:L].abs().sum()) == 0
        assert out.logprobs[L:].tolist() == [pytest.approx(-(i + p / 64)) for p in range(L, T)]
        assert out.top_ids[L:, 1].tolist() == [t + 1 for t in new]


def test_serving_loop_without_logprobs_calls_generate_as_before():
    """Off: no new keyword reaches the session (test_ragged_cpu's stub, which takes none, keeps working) and the result
    is the list of token tensors."""
    from tests.test_ragged_cpu import StubSession, expected, script
    prompts = [torch.arange(1, 6), torch.arange(1, 3)]
    sess = StubSession(2, 16, script)
    outs = generation.serve_prompts(sess, prompts, 5, generation.Sampler.of(1.0, None, None, 0, None))
    assert [o.tolist() for o in outs] == [expected(i, p.tolist(), 5, None) for i, p in enumerate(prompts)]
    sess = ServeStub(2, 16)
    generation.serve_prompts(sess, prompts, 5, generation.Sampler.of(1.0, None, None, 0, None))
    assert sess.kw and all(k == [] for k in sess.kw)
