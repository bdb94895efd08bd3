"""Multi-token decode and speculative generation without a GPU: the v21 entries' argument checks (through the built
library with NULL or dummy pointers: nothing is launched), ngram_draft, the acceptance bookkeeping of speculate against
a stub session that emits scripted tokens, the argument errors of generate(draft_tokens=...), and the new kernel's
register budget."""
import ctypes
import inspect
import os
import shutil

import pytest
import torch

from gpt_2_distributed_amd import generation
from gpt_2_distributed_amd.generation import ngram_draft, speculate_loop
from tests.conftest import REPO
from tests.test_kernel_resources import HIPCC, _instantiation, _resources

LIB = os.path.join(REPO, "gpt_2_distributed_amd", "libgpt2mi.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libgpt2mi.so not built (run __graft_entry__.build())")


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
def test_abi_is_v21_or_later_and_binds_the_extend_entries(lib):
    from gpt_2_distributed_amd import _lib
    assert lib.gpt2mi_abi_version() == _lib.ABI_VERSION >= 21
    for name in ("gpt2mi_attn_extend", "gpt2mi_decode_extend"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    # the row capacity is appended: no earlier field of the plan moved
    fields = [f[0] for f in _lib.DecodePlan._fields_]
    assert fields[-2:] == ["logits", "rows"] and _lib.DecodePlan.rows.offset > _lib.DecodePlan.logits.offset
    assert _lib.DecodePlan().rows == 0


# seq, pos, the words of the refusal: every rule of the row map, with B = 3 sequences and Tcap = 70
BAD_MAPS = [
    ((0, 3), (5, 6), (b"seq[1]=3", b"[0, B=3)")),
    ((-1, 0), (5, 6), (b"seq[0]=-1",)),
    ((1, 0), (5, 6), (b"seq[1]=0", b"decrease")),
    ((0, 1), (5, 70), (b"pos[1]=70",)),
    ((0, 1), (-1, 6), (b"pos[0]=-1",)),
    ((0, 0), (5, 7), (b"pos[1]=7", b"does not follow")),
    ((0, 0), (5, 5), (b"pos[1]=5", b"does not follow")),
    ((0, 0, 1, 1), (5, 6, 9, 8), (b"pos[3]=8", b"does not follow")),
]


@needs_lib
def test_attn_extend_refuses_bad_arguments(lib):
    B, H, Tcap = 3, 2, 70

    def call(seq, pos, R=None, head_dim=64, ws_floats=None, nseq=B):
        R = len(pos) if R is None else R
        ws = lib.gpt2mi_attn_decode_workspace(max(R, 1), H, Tcap) if ws_floats is None else ws_floats
        return lib.gpt2mi_attn_extend(None, None, None, None, None, ws, R, nseq, H, head_dim, Tcap,
                                      seq if seq is None else ints(*seq), pos if pos is None else ints(*pos), None)
    refused(lib, call((0,), (0,), head_dim=32), b"head_dim=32")
    refused(lib, call((0,), (0,), nseq=0), b"B=0")
    refused(lib, call((0,), (0,), R=0), b"R=0")
    refused(lib, call((0,) * 65, tuple(range(65)), R=65), b"R=65")
    refused(lib, call(None, (0,), R=1), b"sequence array", b"NULL")
    refused(lib, call((0,), None, R=1), b"position array", b"NULL")
    for seq, pos, words in BAD_MAPS:
        refused(lib, call(seq, pos), *words)
    good = ((0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2), (30, 31, 32, 33, 0, 1, 2, 66, 67, 68, 69))
    refused(lib, call(*good, ws_floats=lib.gpt2mi_attn_decode_workspace(11, H, Tcap) - 1), b"workspace too small")
    refused(lib, call(*good), b"NULL")                    # a valid map reaches the pointer check: still no launch
    refused(lib, call((0, 0, 2), (0, 1, 69)), b"NULL")    # a sequence may be absent, a run may start at 0
    refused(lib, call((0,) * 64, tuple(range(64))), b"NULL")


def _plan(B=3, Tcap=70, rows=0):
    from gpt_2_distributed_amd import _lib
    plan = _lib.DecodePlan()
    plan.B, plan.C, plan.H, plan.L, plan.Vp, plan.Tcap, plan.rows = B, 128, 2, 1, 512, Tcap, rows
    return plan


@needs_lib
def test_decode_extend_refuses_bad_arguments(lib):
    plan = _plan(rows=8)

    def ext(seq, pos, R=None):
        return lib.gpt2mi_decode_extend(ctypes.byref(plan), len(pos) if R is None else R, None,
                                        seq if seq is None else ints(*seq), pos if pos is None else ints(*pos), None)
    refused(lib, lib.gpt2mi_decode_extend(None, 1, None, ints(0), ints(0), None), b"plan is NULL")
    refused(lib, ext((0,), (0,), R=0), b"R=0")
    refused(lib, ext((0,) * 65, tuple(range(65)), R=65), b"R=65")
    refused(lib, ext(None, (0,), R=1), b"sequence array", b"NULL")
    refused(lib, ext((0,), None, R=1), b"position array", b"NULL")
    for seq, pos, words in BAD_MAPS:
        refused(lib, ext(seq, pos), *words)
    refused(lib, ext((0,) * 9, tuple(range(9))), b"R=9", b"row capacity 8")
    refused(lib, ext((0, 0, 2), (0, 1, 69)), b"workspace too small")  # attn_ws_floats = 0: the step's next check
    plan.rows = 0                                                      # 0 means B rows
    refused(lib, ext((0, 0, 1, 2), (4, 5, 0, 9)), b"R=4", b"row capacity 3")
    refused(lib, ext((0, 1, 2), (4, 0, 9)), b"workspace too small")
    plan.H = 4
    refused(lib, ext((0,), (0,)), b"head_dim")
    plan.H, plan.B = 2, 65
    refused(lib, ext((0,), (0,)), b"B=65")


@needs_lib
def test_existing_plan_entries_ignore_the_row_capacity(lib):
    """The appended field is read by gpt2mi_decode_extend only: the step validates as before whatever it holds."""
    for rows in (0, 1, 64):
        plan = _plan(B=2, Tcap=64, rows=rows)
        refused(lib, lib.gpt2mi_decode_step_ragged(ctypes.byref(plan), None, ints(0, 64), None), b"pos[1]=64")
        refused(lib, lib.gpt2mi_decode_step_ragged(ctypes.byref(plan), None, ints(0, 63), None), b"workspace too small")


# ---- ngram_draft -------------------------------------------------------------------------------------------------------
def test_ngram_draft():
    assert ngram_draft([1, 2, 3, 4], 3) == []                                  # no earlier occurrence
    assert ngram_draft([], 3) == [] and ngram_draft([7], 3) == []
    # the longest n-gram wins: the suffix (1, 2, 3) occurred at 0 (followed by 8), the suffix (3) later (followed by 9)
    assert ngram_draft([1, 2, 3, 8, 5, 3, 9, 1, 2, 3], 1) == [8]
    assert ngram_draft([1, 2, 3, 8, 5, 3, 9, 1, 2, 3], 1, max_ngram=1) == [9]
    # the most recent occurrence wins
    assert ngram_draft([4, 5, 6, 0, 4, 5, 7, 0, 4, 5], 2) == [7, 0]
    # fewer than k followers
    assert ngram_draft([1, 2, 9, 1, 2], 5) == [9, 1, 2]
    assert ngram_draft([3, 3], 4) == [3]
    assert ngram_draft([1, 2, 9, 1, 2], 0) == [] and ngram_draft([1, 2, 9, 1, 2], -1) == []
    h = [1, 2, 9, 1, 2]
    ngram_draft(h, 2)
    assert h == [1, 2, 9, 1, 2]                                                # the history is not modified


# ---- the acceptance bookkeeping against a stub session -----------------------------------------------------------------
EOS = 99


def script(key, pos):
    """The token of the sequence with draw key `key` at position `pos`: EOS at position 9 * key + 14 (if it gets there)."""
    return EOS if pos == 9 * key + 14 else (31 * key + 7 * pos) % 90


class StubSession:
    """DecodeSession's surface as speculate_loop uses it. The token drawn from the logits after a row at position p is
    script(key, p + 1) provided every token of the sequence up to p is the scripted one: a verify row whose prefix holds
    a wrong draft draws a token no script emits (-1), which the loop must never let out. Checks the row map's rules."""

    def __init__(self, lens, keys):
        self.B, self.lens, self.keys = len(lens), list(lens), keys
        self.calls, self.accepts = [], []

    def _verify(self, toks, seqs, poss, ks, sampler):
        assert 1 <= len(toks) <= 64 and len(toks) == len(seqs) == len(poss) == len(ks)
        out, good = [], False
        for r, (t, b, p, key) in enumerate(zip(toks, seqs, poss, ks)):
            run_start = r == 0 or seqs[r - 1] != b
            assert run_start or (seqs[r - 1] == b and poss[r - 1] == p - 1)
            assert not run_start or (p == self.lens[b] and (r == 0 or seqs[r - 1] < b))
            assert key == self.keys[b]
            good = t == script(key, p) and (run_start or good)  # (the run so far is the scripted one)
            out.append(script(key, p + 1) if good else -1)
        self.calls.append(list(seqs))
        return out

    def _accept(self, src, dst):
        self.accepts.append((list(src), list(dst)))


def oracle_draft(keys_by_first, wrong_every=0):
    """draft_fn that knows the script: right always (wrong_every = 0), never (1), or wrong at every m-th call."""
    state = dict(calls=0)

    def fn(history, m):
        state["calls"] += 1
        key, lens0 = keys_by_first[history[0]]
        pos = lens0 + len(history) - 1          # the position of the history's last token
        out = [script(key, pos + 1 + i) for i in range(m)]
        if wrong_every and state["calls"] % wrong_every == 0 and out:
            out[0] = 91                          # (no script token: 0..89 and EOS)
        return out
    return fn


def run_loop(lens, n, k, wrong_every, eos, keys=None):
    keys = keys or list(range(len(lens)))
    sess = StubSession(lens, keys)
    first = [script(key, p) for key, p in zip(keys, lens)]
    by_first = {f: (key, p) for f, key, p in zip(first, keys, lens)}
    assert len(by_first) == len(lens)
    new, stats = speculate_loop(sess, n, k, oracle_draft(by_first, wrong_every), eos, [[] for _ in lens], first, keys,
                                (0.0, None, None, 0))
    return sess, new, stats


def expected_tokens(key, p0, n, eos):
    out = []
    for p in range(p0, p0 + n):
        out.append(script(key, p))
        if eos is not None and out[-1] == eos:
            break
    return out


@pytest.mark.parametrize("eos", [None, EOS])
@pytest.mark.parametrize("wrong_every", [0, 1, 2, 3])
@pytest.mark.parametrize("k", [1, 4, 7])
def test_speculate_bookkeeping(k, wrong_every, eos):
    """Accept all / none / some: the tokens are the script's whatever the drafts, no row passes n, an eos inside an
    accepted run ends the row there, and lens / the accepted logits row follow the accepted count."""
    lens, n = [3, 20, 5], 23                    # row 0 meets EOS at position 14 (its 12th token), row 1 at 23, row 2 not
    sess, new, stats = run_loop(lens, n, k, wrong_every, eos)
    for b, p0 in enumerate(lens):
        want = expected_tokens(b, p0, n, eos)
        assert new[b] == want, (b, new[b], want)
        assert sess.lens[b] == p0 + len(want) - 1  # every token but the last is stepped
    if eos is not None:
        assert new[0][-1] == EOS and len(new[0]) == 12 and new[1][-1] == EOS and len(new[1]) == 4 and len(new[2]) == n
    assert stats["tokens"] == sum(len(t) for t in new) and stats["calls"] == len(sess.calls) == len(sess.accepts)
    assert 0 <= stats["accepted"] <= stats["drafted"]
    if wrong_every == 1:
        assert stats["accepted"] == 0 and stats["calls"] == max(len(t) for t in new) - 1
    if wrong_every == 0 and eos is None:
        assert stats["accepted"] == stats["drafted"] and stats["calls"] == -(-(n - 1) // (k + 1))
    for rows in sess.calls:                     # a finished row is not stepped again; at most k + 1 rows per sequence
        assert all(rows.count(b) <= k + 1 for b in set(rows))
    for (src, dst), rows in zip(sess.accepts, sess.calls):
        assert dst == sorted(set(rows)) and all(rows[s] == d for s, d in zip(src, dst))


def test_speculate_drafts_are_capped_at_what_the_row_needs():
    """n = 6 with k = 7: the first call carries 1 + min(k, n - 2) rows, and a draft function that returns more than it
    was asked for is cut."""
    sess = StubSession([4], [0])
    seen = []

    def greedy_fn(history, m):
        seen.append(m)
        return [script(0, 4 + len(history) + i) for i in range(m + 5)]
    new, stats = speculate_loop(sess, 6, 7, greedy_fn, None, [[]], [script(0, 4)], [0], (0.0, None, None, 0))
    assert new == [expected_tokens(0, 4, 6, None)] and seen == [4] and sess.calls == [[0] * 5]
    assert stats == dict(calls=1, drafted=4, accepted=4, tokens=6) and sess.lens == [9]
    # n = 1: the first token is all there is; nothing is stepped
    sess = StubSession([4], [0])
    new, stats = speculate_loop(sess, 1, 4, greedy_fn, None, [[]], [script(0, 4)], [0], (0.0, None, None, 0))
    assert new == [[script(0, 4)]] and stats["calls"] == 0 and sess.lens == [4]


def test_speculate_passes_the_history_and_the_draw_keys():
    seen = []

    def fn(history, m):
        seen.append(list(history))
        return []
    sess = StubSession([2, 6], [40, 7])
    first = [script(40, 2), script(7, 6)]
    new, stats = speculate_loop(sess, 4, 2, fn, None, [[11, 12], [1, 2, 3, 4, 5, 6]], first, [40, 7],
                                (0.0, None, None, 0))
    assert new == [expected_tokens(40, 2, 4, None), expected_tokens(7, 6, 4, None)]
    assert seen[0] == [11, 12, first[0]] and seen[1] == [1, 2, 3, 4, 5, 6, first[1]]
    assert seen[2] == [11, 12] + new[0][:2] and len(seen) == 4  # (the last call needs one token: nothing to draft)
    assert stats["calls"] == 3 and stats["drafted"] == 0


# ---- generate(draft_tokens=...): argument errors -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_model():
    from gpt_2_distributed_amd.model import GPT2, GPT2Config
    return GPT2(GPT2Config(n_layer=1, n_head=1, n_embd=64, vocab_size=64, n_positions=16))


def test_generate_takes_draft_tokens_and_refuses_bad_ones(cpu_model):
    from gpt_2_distributed_amd.model import GPT2
    for fn in (GPT2.generate, generation.generate):
        params = inspect.signature(fn).parameters
        assert params["draft_tokens"].default is None and params["draft_fn"].default is None
    sig = inspect.signature(generation.DecodeSession.speculate).parameters
    assert list(sig)[1:4] == ["n", "k", "draft_fn"] and "row_id" in sig
    assert list(inspect.signature(generation.DecodeSession.extend).parameters)[1:] == ["tokens", "counts"]
    idx = torch.zeros(3, 5, dtype=torch.long)
    with pytest.raises(ValueError, match="seed"):
        cpu_model.generate(idx, 4, draft_tokens=4)                                   # the host sampler
    with pytest.raises(ValueError, match="seed"):
        cpu_model.generate(idx, 4, draft_tokens=4, generator=torch.Generator())
    with pytest.raises(ValueError, match="64 rows"):
        cpu_model.generate(idx, 4, seed=1, draft_tokens=21)                          # 3 * 22 = 66 rows
    with pytest.raises(ValueError, match="draft_tokens"):
        cpu_model.generate(idx, 4, seed=1, draft_tokens=0)
    with pytest.raises(ValueError, match="draft_tokens"):
        cpu_model.generate(idx, 4, seed=1, draft_fn=ngram_draft)                     # a draft_fn without draft_tokens
    with pytest.raises(RuntimeError, match="cuda"):                                  # valid: reaches _check_model
        cpu_model.generate(idx, 4, seed=1, draft_tokens=20)                          # 3 * 21 = 63 rows


def test_cli_takes_draft_tokens():
    from gpt_2_distributed_amd.generate import parse_args
    assert parse_args(["--checkpoint", "x"]).draft_tokens is None
    assert parse_args(["--checkpoint", "x", "--sampler", "device", "--draft_tokens", "4"]).draft_tokens == 4


# ---- register budget ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_attn_extend_kernel_has_no_scratch_and_no_spills():
    """The row map arrives as a kernel argument and is indexed by blockIdx: scalar loads, not a private array."""
    k, v = _instantiation(_resources("decode.hip"), "attn_extend_kernel", "KvBf16")
    assert v["ScratchSize [bytes/lane]"] == 0, f"{k}: scratch {v}"
    assert v["VGPRs Spill"] == 0, f"{k}: spills {v}"
