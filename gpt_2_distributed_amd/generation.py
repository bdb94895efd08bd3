"""Autoregressive generation: a per-layer key/value cache, one-token decode steps and nanoGPT's ``generate``.

The reference (model.py, train_gpt2_distributed.py) trains and evaluates only; continuing a prompt with it means
calling ``model(idx)`` on the whole growing sequence for every new token. Here a prompt is run once through the
engine's trunk forward (``DecodeSession.prefill``), its keys and values are copied into the cache, and every further
token is one call of ``gpt2mi_decode_step_ragged`` (csrc/decode.hip): weight-streaming skinny GEMMs and single-query
attention over the cache, about 10 launches per layer issued from C. The next token is drawn either on the host side in
PyTorch (``sample_next``, from a ``torch.Generator``) or, with a ``seed``, by ``gpt2mi_sample_ragged`` on the device
(csrc/sample.hip; ``sample_reference`` and ``uniform_at`` state what it computes), in which case the whole loop is one
C call (``gpt2mi_decode_generate_ragged``).

Every row of a session has its own position: ``DecodeSession.lens`` holds one per row, ``prefill`` takes right-padded
prompts with their lengths, ``refill`` replaces one row while the others go on, and ``generate_many`` serves any number
of prompts through one session that way. Equally long sequences are the case where the positions agree: there is one
set of kernels and one code path (the ``gpt2mi_*_ragged`` entries; DESIGN.md "Ragged batches").

A step appends one token per row. ``DecodeSession.extend`` appends several to a live row in one pass over the weights
(``gpt2mi_decode_extend``: the rows of a launch may be consecutive positions of one sequence), with the bits of as many
steps; ``DecodeSession.speculate`` uses it to verify drafted tokens (``ngram_draft``, or any callable) and returns
exactly the tokens of the device loop (DESIGN.md "Multi-token decode step").

With ``logprobs=`` the device sampler also returns, from the launch that draws a token, the token's log-probability
under the model's own distribution and the most likely alternatives (``gpt2mi_sample_logprobs``; ``token_logprobs`` is
the rule, ``LogprobBuffer`` where a session puts them; DESIGN.md "Token log-probabilities").

With ``logit_bias=``, ``min_p=``, ``min_new_tokens=`` and ``stop=`` the sampler is constrained, on the device in the same
launch (``gpt2mi_sample_constrained``; ``apply_constraints``, ``sample_reference``'s ``min_p`` and ``stop_match`` are the
rule; DESIGN.md "Constraints in the sampler").

With ``num_beams=`` ``generate`` searches: the W beams of a prompt are W rows forked from one prefill, and each token
is chosen by ``gpt2mi_decode_beam_search`` on the device (the rows' top-W log-probabilities, the selection, the move of
the generated suffix of the cache rows to their new parents, the step), nothing read back in between. ``beam_select``
is the selection rule, ``beam_rank`` the final ranking and ``beam_pick`` what is returned of it (DESIGN.md "Beam
search").

Numerics are the autocast path's whatever the autocast state: bf16 GEMM operands from the engine's weight shadow, fp32
accumulation, fp32 residual stream / LayerNorm / softmax, dropout off (p = 0 whatever ``model.training`` is, and
``.training`` is not touched). Logits are fp32. ``model.precision == "fp32"`` has no decode kernels and raises.

Generation leaves training untouched: it does not advance the engine's dropout stream (``_step_seed``) or its forward
token, and does not replace the activations record a pending backward reads. It does run the prompt through the
engine's workspace, so (a) it may evict the training workspace of another (B, T) shape, which the next training
forward re-allocates, and (b) it must not be called between a forward and its backward.
"""
from __future__ import annotations

import ctypes
import inspect
from dataclasses import dataclass, field, replace
from typing import List, NamedTuple, Optional, Sequence

import torch

from . import _lib as K

BF16 = torch.bfloat16
F32 = torch.float32
MAX_BATCH = 64  # rows of the skinny GEMM (gpt2mi_gemm_skinny)
SCRATCH = ("x", "xmid", "ln", "qkv", "ao", "h", "mean", "rstd", "attn_ws", "gemm_ws", "logits")  # a plan's buffers


def _nucleus_keep(key: torch.Tensor, probs: torch.Tensor, top_p: float) -> torch.Tensor:
    """The top-p rule on probabilities [B, V] (rows summing to 1), tokens ordered by ``key`` [B, V] (the probabilities
    themselves, or the values they were formed from): token i is kept iff the total probability of the tokens with a
    strictly larger key is < top_p (ties at the threshold all kept, the largest always kept)."""
    sk, order = torch.sort(key, dim=-1, descending=True)
    sp = probs.gather(-1, order)
    before = sp.cumsum(-1) - sp                                  # mass ahead of each sorted position
    pos = torch.arange(sk.size(-1), device=sk.device).expand_as(sk)
    new = torch.ones_like(sk, dtype=torch.bool)
    new[:, 1:] = sk[:, 1:] != sk[:, :-1]
    first = torch.where(new, pos, torch.zeros_like(pos)).cummax(-1).values  # where a position's run of equals starts
    keep_sorted = before.gather(-1, first) < top_p
    return torch.zeros_like(keep_sorted).scatter(-1, order, keep_sorted)


def sample_next(logits: torch.Tensor, temperature: float = 1.0, top_k: Optional[int] = None,
                generator: Optional[torch.Generator] = None, top_p: Optional[float] = None,
                min_p: Optional[float] = None) -> torch.Tensor:
    """Next token ids [B] from logits [B, V] (nanoGPT's rule; pure torch, any device).

    ``temperature == 0`` is greedy argmax. Otherwise ``logits / temperature``, optionally everything below the
    ``top_k``-th largest logit of a row set to -inf, softmax, optionally (``top_p`` in (0, 1)) every token dropped whose
    strictly more probable tokens already weigh ``top_p`` or more, and one ``torch.multinomial`` draw per row from
    ``generator``. ``min_p`` in (0, 1] also drops every token whose value lies below the row maximum +
    ``log_min_p(min_p)`` (``sample_reference``'s rule: p_i < min_p * p_max); greedy ignores it."""
    if logits.dim() != 2:
        raise ValueError(f"sample_next takes logits [B, V] (got {tuple(logits.shape)})")
    if temperature < 0:
        raise ValueError(f"temperature must be >= 0 (got {temperature})")
    if top_k is not None and top_k < 1:
        raise ValueError(f"top_k must be >= 1 (got {top_k})")
    _check_top_p(top_p)
    logits = logits.float()
    if temperature == 0:
        return logits.argmax(dim=-1)
    logits = logits / temperature
    floor = None if not min_p else logits.max(-1, keepdim=True).values + log_min_p(min_p)
    if top_k is not None and top_k < logits.size(-1):
        kth = torch.topk(logits, top_k, dim=-1).values[:, -1:]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    probs = torch.softmax(logits, dim=-1)
    if top_p is not None and top_p < 1:
        probs = probs.masked_fill(~_nucleus_keep(probs, probs, top_p), 0.0)  # (multinomial normalises what is left)
    if floor is not None:
        probs = probs.masked_fill(logits < floor, 0.0)
    return torch.multinomial(probs, num_samples=1, generator=generator).squeeze(1)


def _check_top_p(top_p):
    if top_p is not None and not top_p > 0:  # (NaN too)
        raise ValueError(f"top_p must be > 0 (got {top_p}); >= 1 or None turns it off")


# ---- the device sampler's contract (gpt2mi_sample, csrc/sample.hip), executable -------------------------------------
_M64 = (1 << 64) - 1


def uniform_at(seed: int, b: int, pos: int) -> float:
    """The uniform in [0, 1) that row ``b`` draws with at position ``pos``: 24 bits of splitmix64's finaliser over
    ``seed + 0x9E3779B97F4A7C15 * (1 + (b << 32 | pos))``. A pure function: no state, no dependence on the batch."""
    c = ((seed & _M64) + 0x9E3779B97F4A7C15 * (1 + (((b & 0xFFFFFFFF) << 32) | (pos & 0xFFFFFFFF)))) & _M64
    c ^= c >> 30
    c = (c * 0xBF58476D1CE4E5B9) & _M64
    c ^= c >> 27
    c = (c * 0x94D049BB133111EB) & _M64
    c ^= c >> 31
    return (c >> 40) * 2.0 ** -24


def log_min_p(min_p: float) -> float:
    """``lmp`` of the min-p rule: fp32(log(double(fp32(min_p)))), formed on the host (-inf for 0)."""
    import math
    import numpy as np
    m = float(np.float32(min_p))
    return float(np.float32(math.log(m))) if m > 0 else float("-inf")


def sample_reference(logits: torch.Tensor, temperature: float, top_k: Optional[int], top_p: Optional[float],
                     u: torch.Tensor, min_p: Optional[float] = None):
    """What gpt2mi_sample computes, in float64 (any device): ``(tokens [B], probs [B, V])`` from logits [B, V] and the
    uniforms ``u`` [B] (``uniform_at``'s for the device's draw).

    ``temperature == 0``: argmax, the lowest index among equal maxima (probs one-hot). Otherwise x = fp32
    ``logits / temperature``; top-k keeps x >= the k-th largest value; top-p, on the softmax p of what top-k kept, keeps
    token i iff the tokens with a strictly larger value weigh < top_p; the token is the first index, in vocabulary
    order, whose inclusive cumulative kept probability exceeds u * Z (Z the kept mass). probs = p_i / Z, 0 if filtered.

    ``min_p`` in (0, 1] (None or 0: off; greedy ignores it): with mx the row maximum of x, token i is also dropped unless
    ``x_i >= fl32(mx + log_min_p(min_p))``, one fp32 add. The ratio of a token to the maximum does not depend on what
    else was filtered, so this is HF's and vLLM's "p_i >= min_p * p_max", stated on the values so that it is exact. A
    row with no finite value gives token 0."""
    B, V = logits.shape
    x = logits.float()
    if temperature == 0:
        mx = x.max(-1, keepdim=True).values
        tok = (x == mx).int().argmax(-1)  # argmax of a 0/1 tensor: the first 1
        return tok, torch.zeros(B, V, dtype=torch.float64, device=x.device).scatter_(1, tok[:, None], 1.0)
    x = x / temperature
    keep = torch.ones_like(x, dtype=torch.bool)
    if top_k is not None and 1 <= top_k < V:
        keep = x >= torch.topk(x, top_k, dim=-1).values[:, -1:]
    xd = x.double()
    p = torch.softmax(xd.masked_fill(~keep, float("-inf")), dim=-1)
    if top_p is not None and top_p < 1:
        keep = keep & _nucleus_keep(xd, p, top_p)  # (ties decided by the value, not by the p it rounds to)
    if min_p:
        keep = keep & (x >= x.max(-1, keepdim=True).values + torch.full((), log_min_p(min_p), dtype=F32, device=x.device))
    pk = p * keep
    Z = pk.sum(-1, keepdim=True)
    cdf = pk.cumsum(-1)
    tok = (cdf > u.double().to(x.device)[:, None] * Z).int().argmax(-1)  # (a row of NaN: no crossing, token 0)
    return tok, pk / Z


# ---- penalties: the rule gpt2mi_sample_penalized applies in front of sample_reference, executable ---------------------
def _check_penalties(repetition_penalty, presence_penalty, frequency_penalty):
    """The three values as floats and whether any is non-neutral, or a ValueError."""
    rp, pp, fp = float(repetition_penalty), float(presence_penalty), float(frequency_penalty)
    if not 0 < rp < float("inf"):  # (NaN too)
        raise ValueError(f"repetition_penalty must be finite and > 0 (got {repetition_penalty}); 1 turns it off")
    if not abs(pp) < float("inf"):
        raise ValueError(f"presence_penalty must be finite (got {presence_penalty}); 0 turns it off")
    if not abs(fp) < float("inf"):
        raise ValueError(f"frequency_penalty must be finite (got {frequency_penalty}); 0 turns it off")
    return rp, pp, fp, (rp, pp, fp) != (1.0, 0.0, 0.0)


def apply_penalties(logits: torch.Tensor, history: torch.Tensor, lens, gen_start, repetition_penalty: float = 1.0,
                    presence_penalty: float = 0.0, frequency_penalty: float = 0.0) -> torch.Tensor:
    """The logits a penalised draw is made from: fp32 [B, V] from logits [B, V] and the rows' token histories (pure
    torch, any device; what csrc/sample.hip computes bit for bit).

    Row b's history is ``history[b, :lens[b]]`` (integer [B, T]); entries outside [0, V) are ignored. For vocabulary
    index i, seen_i = i occurs in it (prompt and generated tokens: the scope of HF's ``repetition_penalty``) and c_i =
    its occurrences in ``history[b, gen_start[b]:lens[b]]`` (generated tokens: the OpenAI / vLLM scope of the other
    two; ``gen_start`` None: 0). In this order, each operation one fp32 operation rounded to nearest:
    ``repetition_penalty != 1`` and seen_i: ``x = x * rp if x < 0 else x / rp`` (0 is divided);
    ``frequency_penalty != 0`` and c_i > 0: ``x = x - (fp * float(c_i))``; ``presence_penalty != 0`` and c_i > 0:
    ``x = x - pp``. Neutral values (1, 0, 0) return the logits' bits."""
    rp, pp, fp, on = _check_penalties(repetition_penalty, presence_penalty, frequency_penalty)
    if logits.dim() != 2 or history.dim() != 2 or history.size(0) != logits.size(0):
        raise ValueError(f"apply_penalties takes logits [B, V] and history [B, T] (got {tuple(logits.shape)}, "
                         f"{tuple(history.shape)})")
    x = logits.float()
    if not on:
        return x
    B, V = x.shape
    dev = x.device
    as_t = lambda v: torch.as_tensor(v, device=dev).long().reshape(B)  # noqa: E731
    lens_t = as_t(lens)
    start_t = torch.zeros_like(lens_t) if gen_start is None else as_t(gen_start)
    if bool((lens_t < 0).any() | (lens_t > history.size(1)).any() | (start_t < 0).any() | (start_t > lens_t).any()):
        raise ValueError(f"lens must lie in [0, T={history.size(1)}] and gen_start in [0, lens]")
    hist = history.to(dev).long()
    at = torch.arange(hist.size(1), device=dev)[None]
    valid = (at < lens_t[:, None]) & (hist >= 0) & (hist < V)
    idx = hist.clamp(0, V - 1)
    seen = torch.zeros(B, V, dtype=torch.int64, device=dev).scatter_add_(1, idx, valid.long()) > 0
    generated = valid & (at >= start_t[:, None])
    count = torch.zeros(B, V, dtype=torch.int64, device=dev).scatter_add_(1, idx, generated.long())
    # (0-dim tensors: a Python scalar divisor would become a multiplication by its reciprocal on the device)
    f32 = lambda v: torch.full((), v, dtype=F32, device=dev)  # noqa: E731
    if rp != 1.0:
        x = torch.where(seen, torch.where(x < 0, x * f32(rp), x / f32(rp)), x)
    if fp != 0.0:
        x = torch.where(count > 0, x - (f32(fp) * count.float()), x)
    if pp != 0.0:
        x = torch.where(count > 0, x - f32(pp), x)
    return x


# ---- constraints: the rule gpt2mi_sample_constrained applies between the penalties and the draw, executable -----------
STOP_MAX_SEQS, STOP_MAX_LEN = K.STOP_MAX_SEQS, K.STOP_MAX_LEN


def _check_constraints(logit_bias=None, min_p=None, min_new_tokens=0, stop=None, eos_token_id=None,
                       vocab_size: Optional[int] = None):
    """(min_p as a float, 0.0: off; min_new_tokens as an int; stop as a list of int lists), or a ValueError. logit_bias
    is a tensor [..., V] or a ``{token: value}`` dict (None: none); only its values and tokens are checked here."""
    mp = 0.0 if min_p is None else float(min_p)
    if not 0 <= mp <= 1:  # (NaN too)
        raise ValueError(f"min_p must lie in [0, 1] (got {min_p}); 0 or None turns it off")
    mn = int(min_new_tokens)
    if mn < 0:
        raise ValueError(f"min_new_tokens must be >= 0 (got {min_new_tokens})")
    stops = [[int(t) for t in s] for s in (stop or [])]
    if (mn > 0 or stops) and eos_token_id is None:
        raise ValueError("min_new_tokens and stop need an eos_token_id: the first holds eos back, a row that completes a "
                         "stop sequence goes on emitting it")
    if len(stops) > STOP_MAX_SEQS:
        raise ValueError(f"at most {STOP_MAX_SEQS} stop sequences (got {len(stops)})")
    for s in stops:
        if not 1 <= len(s) <= STOP_MAX_LEN:
            raise ValueError(f"a stop sequence holds 1 to {STOP_MAX_LEN} tokens (got {len(s)})")
        if vocab_size is not None and not all(0 <= t < vocab_size for t in s):
            raise ValueError(f"stop tokens must lie in [0, vocab_size={vocab_size}) (got {s})")
    if isinstance(logit_bias, dict):
        toks, vals = [int(t) for t in logit_bias], [float(v) for v in logit_bias.values()]
        if vocab_size is not None and not all(0 <= t < vocab_size for t in toks):
            raise ValueError(f"logit_bias tokens must lie in [0, vocab_size={vocab_size}) (got {toks})")
        if any(v != v or v == float("inf") for v in vals):
            raise ValueError("logit_bias values must be finite or -inf (which bans the token)")
    elif logit_bias is not None:
        if vocab_size is not None and logit_bias.size(-1) != vocab_size:
            raise ValueError(f"logit_bias must be [.., V={vocab_size}] (got {tuple(logit_bias.shape)})")
        if bool((torch.isnan(logit_bias) | (logit_bias == float("inf"))).any()):
            raise ValueError("logit_bias values must be finite or -inf (which bans the token)")
    return mp, mn, stops


def apply_constraints(logits: torch.Tensor, pos, gen_start, logit_bias: Optional[torch.Tensor] = None, bias_row=None,
                      min_new_tokens: int = 0, eos_token_id: Optional[int] = None) -> torch.Tensor:
    """The row a constrained draw dumps and goes on from: fp32 [B, V] from the (penalised) logits [B, V] (pure torch, any
    device; what csrc/sample_con.hip computes bit for bit). In this order:
    bias: ``x = x + logit_bias[bias_row[b]]`` (one fp32 add per element) for a row with ``bias_row[b] >= 0``
    (``bias_row`` None: row b reads row b; ``logit_bias`` fp32 [rows, V], -inf bans a token); a row without a bias row
    keeps its bits. Minimum length: ``min_new_tokens > 0`` and ``pos[b] - gen_start[b] < min_new_tokens`` (``pos[b]`` the
    column being drawn, ``gen_start`` None: 0): ``x[eos_token_id] = -inf``."""
    if logits.dim() != 2:
        raise ValueError(f"apply_constraints takes logits [B, V] (got {tuple(logits.shape)})")
    x = logits.float()
    B, V = x.shape
    dev = x.device
    if logit_bias is not None:
        _check_constraints(logit_bias, vocab_size=V)
        rows = torch.arange(B, device=dev) if bias_row is None else torch.as_tensor(bias_row, device=dev).long().reshape(B)
        if bool((rows < -1).any() | (rows >= logit_bias.size(0)).any()):
            raise ValueError(f"bias_row must lie in [-1, {logit_bias.size(0)})")
        bias = logit_bias.to(dev).float()[rows.clamp_min(0)]
        x = torch.where((rows >= 0)[:, None], x + bias, x)
    mn = int(min_new_tokens)
    if mn > 0:
        if eos_token_id is None or not 0 <= int(eos_token_id) < V:
            raise ValueError(f"min_new_tokens needs an eos_token_id in [0, V={V}) (got {eos_token_id})")
        pos_t = torch.as_tensor(pos, device=dev).long().reshape(B)
        start_t = torch.zeros_like(pos_t) if gen_start is None else torch.as_tensor(gen_start, device=dev).long().reshape(B)
        held = (pos_t - start_t) < mn
        x = x.clone()
        x[:, int(eos_token_id)] = torch.where(held, torch.full_like(x[:, 0], float("-inf")), x[:, int(eos_token_id)])
    return x


def stop_match(history: List[int], gen_start: int, stops, min_new_tokens: int = 0) -> bool:
    """Whether the last token of ``history`` (the row's tokens so far, the one just drawn at ``pos = len(history) - 1``
    last) completes a stop sequence: for some s in ``stops`` of length n, ``history[pos - n + 1 .. pos] == s``, the match
    wholly in the generated part (``pos - n + 1 >= gen_start``), and the row then holds at least ``min_new_tokens``
    generated tokens (``pos - gen_start + 1 >= min_new_tokens``)."""
    pos = len(history) - 1
    if pos < 0 or pos - gen_start + 1 < min_new_tokens:
        return False
    for s in stops:
        n = len(s)
        if n >= 1 and pos - n + 1 >= gen_start >= 0 and [int(t) for t in history[pos - n + 1:]] == [int(t) for t in s]:
            return True
    return False


def first_stop(tokens: List[int], gen_start: int, stops, min_new_tokens: int = 0, eos_token_id=None) -> Optional[int]:
    """The index in ``tokens`` (a row's prompt and new tokens) of the first generated token that completes a stop
    sequence (``stop_match``) before any eos, or None: where the sampler set the row's done flag for one."""
    for i in range(gen_start, len(tokens)):
        if tokens[i] == eos_token_id:
            return None
        if stop_match(tokens[:i + 1], gen_start, stops, min_new_tokens):
            return i
    return None


# ---- log-probabilities: the rule gpt2mi_sample_logprobs states beside the token it draws, executable -------------------
def token_logprobs(logits: torch.Tensor, tokens: Optional[torch.Tensor] = None, top_n: int = 0):
    """The raw model distribution's log-probabilities, in float64 (pure torch, any device): ``(logprob, top_ids,
    top_logprobs)`` from logits [..., V]; what csrc/sample.hip computes beside a draw, and what the host sampler path
    returns.

    Per row of fp32 logits l: M = max l, S = sum exp(l_i - M), lse = M + log(S), logprob(i) = l_i - lse. The row is
    the model's own: no penalty, temperature or top-k / top-p filter enters, so the value depends on the row and V only.
    ``logprob`` [...] is that of ``tokens`` [...] (None without tokens). ``top_ids`` (int64) / ``top_logprobs``
    [..., top_n] are the ``top_n`` largest l_i in descending order, equal values by ascending index; the order compares
    the fp32 values and is exact, -inf entries come after every finite one, by index. NaN logits are outside the
    contract, as in the sampler."""
    V = logits.size(-1)
    top_n = int(top_n)
    if not 0 <= top_n <= V:
        raise ValueError(f"top_n must lie in [0, V={V}] (got {top_n})")
    l32 = logits.float()
    l = l32.double()
    M = l.max(-1, keepdim=True).values
    lse = M + torch.log(torch.exp(l - M).sum(-1, keepdim=True))
    logprob = None
    if tokens is not None:
        if tokens.shape != logits.shape[:-1]:
            raise ValueError(f"tokens {tuple(tokens.shape)} must be one per row of logits {tuple(logits.shape)}")
        logprob = (l.gather(-1, tokens.to(l.device).long()[..., None]) - lse)[..., 0]
    # (a stable sort keeps equal values, -0 and +0 among them, in index order)
    top_ids = torch.sort(l32, dim=-1, descending=True, stable=True).indices[..., :top_n]
    return logprob, top_ids, l.gather(-1, top_ids) - lse


class LogprobBuffer:
    """Where ``DecodeSession.generate`` / ``speculate`` put log-probabilities, column-aligned with ``seq``: the value of
    the token in ``seq[b, c]`` is ``logprob[b, c]`` (fp32 [B, T]) and its alternatives ``top_ids`` (int32) /
    ``top_logprobs`` (fp32) ``[b, c, :top_n]``. Columns nothing wrote hold 0."""

    def __init__(self, B: int, T: int, top_n: int = 0, device="cuda"):
        top_n = int(top_n)
        if not 0 <= top_n <= K.LOGPROBS_MAX_TOP:
            raise ValueError(f"top_n must lie in [0, {K.LOGPROBS_MAX_TOP}] (GPT2MI_LOGPROBS_MAX_TOP; got {top_n})")
        self.B, self.T, self.top_n = B, T, top_n
        self.logprob = torch.zeros(B, T, dtype=F32, device=device)
        self.top_ids = torch.zeros(B, T, top_n, dtype=torch.int32, device=device)
        self.top_logprobs = torch.zeros(B, T, top_n, dtype=F32, device=device)

    def tensors(self) -> dict:
        """The sampler bindings' keywords."""
        return dict(logprob=self.logprob, top_ids=self.top_ids if self.top_n else None,
                    top_logprobs=self.top_logprobs if self.top_n else None)

    def put(self, rows: Sequence[int], cols: Sequence[int], values, src: Sequence[int]) -> None:
        """``[rows[i], cols[i]]`` = row ``src[i]`` of ``values`` = (logprob [R], top_ids [R, n], top_logprobs [R, n]):
        index writes, nothing read back."""
        dev = self.logprob.device
        r, c, j = (torch.tensor(list(v), dtype=torch.int64, device=dev) for v in (rows, cols, src))
        self.logprob[r, c] = values[0].to(dev)[j].float()
        if self.top_n:
            self.top_ids[r, c] = values[1].to(dev)[j].to(torch.int32)
            self.top_logprobs[r, c] = values[2].to(dev)[j].float()

    def clear(self, row: Optional[int] = None) -> None:
        for t in (self.logprob, self.top_ids, self.top_logprobs):
            (t if row is None else t[row]).zero_()


class GenerateOutput(NamedTuple):
    """``generate(..., logprobs=)``: the tokens it returns without, and per column the raw log-probability of a generated
    token (0 in prompt and pad columns and after a row's eos) and its alternatives."""
    tokens: torch.Tensor
    logprobs: torch.Tensor
    top_ids: torch.Tensor
    top_logprobs: torch.Tensor


def _check_logprobs(logprobs) -> Optional[int]:
    """``logprobs=None | True | int`` of generate / generate_many as top_n (None: off)."""
    if logprobs is None or logprobs is False:
        return None
    n = 0 if logprobs is True else int(logprobs)
    if not 0 <= n <= K.LOGPROBS_MAX_TOP:
        raise ValueError(f"logprobs must be None, True or an int in [0, {K.LOGPROBS_MAX_TOP}] alternatives per token "
                         f"(got {logprobs!r})")
    return n


# ---- beam search: the rule gpt2mi_beam_select applies, executable, and the final ranking ---------------------------------
def _host_array(v, dtype):
    import numpy as np
    return np.ascontiguousarray((v.detach().cpu() if isinstance(v, torch.Tensor) else torch.as_tensor(v)).numpy()).astype(
        dtype, copy=False)


def beam_select(cum, done, top_ids, top_logprobs, eos, W: int):
    """One step of beam search over groups of ``W`` rows, in numpy float32: what gpt2mi_beam_select computes bit for bit.
    ``(tok int64 [R], parent int32 [R], cum float32 [R], done uint8 [R])`` from ``cum`` [R], ``done`` [R] and the rows'
    ``top_ids`` / ``top_logprobs`` [R, W] (``token_logprobs(row, top_n=W)``'s order: value descending, equal values by
    ascending index); R = G W, group g in rows g W .. g W + W - 1. ``eos`` -1 (or None): no eos, nothing is finished.

    Candidates of a group: a live beam j offers its W tokens, rank r at score ``cum[j] + top_logprobs[j][r]`` (one fp32
    add); a finished beam offers ``eos`` at score ``cum[j]``, rank 0. They are ordered by (score descending, beam j
    ascending, rank r ascending), comparing fp32 values (-0 == +0; -inf scores come last, by (j, r)); NaN is outside the
    contract. The tie-break is the rank within the beam and not the token id: ``fl(cum + lp)`` can map two distinct
    log-probabilities to one score, and a rule stated over token ids of the whole vocabulary would then disagree with
    one that sees each beam's W best. The W first candidates become the new beams, best first: ``tok``, ``parent`` (an
    absolute row), the score as the new ``cum`` and ``done = parent's done or tok == eos``.

    At the first step the state is ``cum = [0, -inf, ..., -inf]`` per group: the rows are forks of one prefill, so only
    beam 0 may expand. A finished beam stays in the set, emitting eos, and competes on its raw ``cum``: no length
    penalty enters here (see ``beam_rank``)."""
    import numpy as np
    W = int(W)
    eos = -1 if eos is None else int(eos)
    cum, done = _host_array(cum, np.float32).reshape(-1), _host_array(done, np.uint8).reshape(-1)
    R = cum.size
    if W < 1 or R % W or done.size != R:
        raise ValueError(f"beam_select takes R = G * W rows of cum and done (got {R} and {done.size}, W={W})")
    ids, lps = _host_array(top_ids, np.int64).reshape(R, W), _host_array(top_logprobs, np.float32).reshape(R, W)
    tok, parent = np.zeros(R, np.int64), np.zeros(R, np.int32)
    cum_out, done_out = np.zeros(R, np.float32), np.zeros(R, np.uint8)
    for g0 in range(0, R, W):
        cands = []  # (score, beam, rank, token, finished)
        for j in range(W):
            row = g0 + j
            if eos >= 0 and done[row]:
                cands.append((cum[row], j, 0, eos, True))
            else:
                cands += [(np.float32(cum[row] + lps[row, r]), j, r, int(ids[row, r]), False) for r in range(W)]
        cands.sort(key=lambda c: (-float(c[0]), c[1], c[2]))  # (-0.0 == 0.0 as floats; inf, a -inf score, sorts last)
        for slot, (score, j, _, t, fin) in enumerate(cands[:W]):
            tok[g0 + slot], parent[g0 + slot], cum_out[g0 + slot] = t, g0 + j, score
            done_out[g0 + slot] = fin or (eos >= 0 and t == eos)
    return tok, parent, cum_out, done_out


def beam_rank(cum, lengths, length_penalty: float = 1.0):
    """The final ranking of beam search, on the host in float64: ``(order, score)`` for ``cum`` and ``lengths`` [..., W]
    (a beam's length: its generated tokens up to and including its first eos). ``score = cum / max(length, 1) **
    length_penalty``; ``order`` lists each group's beams by score descending, equal scores by beam index.

    The length penalty enters only here. Inside the loop finished and live beams compete on their raw cumulative
    log-probability and a finished beam stays in the set (``beam_select``): this is not HF's hypothesis heap, which takes
    a finished hypothesis out of the beams, scores it with the penalty at once and can stop early."""
    cum = torch.as_tensor(cum).double().cpu()
    length = torch.as_tensor(lengths).double().cpu().clamp_min(1.0)
    score = cum / length ** float(length_penalty)
    return torch.sort(score, dim=-1, descending=True, stable=True).indices, score


class BeamOutput(NamedTuple):
    """``generate(..., num_beams=W)``: per prompt its ``num_return_sequences`` best beams, best first. ``tokens`` int64
    [B, r, P + m] (a row as ``generate`` lays it out: the prompt, the beam's tokens, pad after its first eos), ``scores``
    float64 [B, r] (``beam_rank``), ``cum_logprob`` fp32 [B, r] (the sum the loop formed) and ``lengths`` int64 [B, r]."""
    tokens: torch.Tensor
    scores: torch.Tensor
    cum_logprob: torch.Tensor
    lengths: torch.Tensor


def beam_pick(tokens, cum, lengths, W: int, length_penalty: float = 1.0, num_return_sequences: int = 1) -> "BeamOutput":
    """The result of a search from its final state: ``tokens`` [B W, T], ``cum`` [B W] and ``lengths`` [B W], row
    ``b W + j`` beam j of prompt b, as the ``BeamOutput`` of each prompt's ``num_return_sequences`` best beams in
    ``beam_rank``'s order. Pure indexing on whatever device the state is on: entry ``[b, i]`` of every field belongs to the
    same beam, and the result for r beams is the first r entries of the result for W."""
    R, W, r = tokens.size(0), int(W), int(num_return_sequences)
    if W < 1 or R % W or cum.shape != (R,) or lengths.shape != (R,) or not 1 <= r <= W:
        raise ValueError(f"beam_pick takes B * W rows of tokens, cum and lengths and 1 <= num_return_sequences <= W (got "
                         f"{R}, {tuple(cum.shape)}, {tuple(lengths.shape)}, W={W}, num_return_sequences={r})")
    B, dev = R // W, tokens.device
    order, score = beam_rank(cum.view(B, W), lengths.view(B, W), length_penalty)
    order = order[:, :r]
    rows = (torch.arange(B)[:, None] * W + order).reshape(-1).to(dev)
    return BeamOutput(tokens[rows].view(B, r, -1), score.gather(1, order).to(dev), cum[rows].view(B, r),
                      lengths[rows].view(B, r))


WITH_BEAMS = ("model", "idx", "max_new_tokens", "eos_token_id", "prompt_lens", "pad_token_id", "kv_dtype", "num_beams",
              "length_penalty", "num_return_sequences")  # (of generate's parameters)


def _check_beams(num_beams, length_penalty, num_return_sequences, B: int, vocab_size: int, given: dict):
    """``generate``'s beam keywords as (W, length_penalty, num_return_sequences), or the ValueError naming the one that is
    wrong. Of ``given``, ``generate``'s arguments by name, all but ``WITH_BEAMS`` must be neutral (``Sampler()``'s value)."""
    W = int(num_beams)
    if not 1 <= W <= K.LOGPROBS_MAX_TOP:
        raise ValueError(f"num_beams must lie in [1, {K.LOGPROBS_MAX_TOP}] (got {num_beams})")
    if W > vocab_size:
        raise ValueError(f"num_beams={W} exceeds vocab_size={vocab_size}")
    if B * W > MAX_BATCH:
        raise ValueError(f"{B} prompts x num_beams={W} = {B * W} rows exceed the {MAX_BATCH} rows of a decode session "
                         f"(MAX_BATCH)")
    r = int(num_return_sequences)
    if not 1 <= r <= W:
        raise ValueError(f"num_return_sequences must lie in [1, num_beams={W}] (got {num_return_sequences})")
    lp = float(length_penalty)
    if not abs(lp) < float("inf"):  # (NaN too)
        raise ValueError(f"length_penalty must be finite (got {length_penalty})")
    neutral = Sampler()
    for name, p in inspect.signature(generate).parameters.items():
        value = "given" if name in ("logit_bias", "allowed_token_ids") and given[name] is not None else given[name]
        if name not in WITH_BEAMS and value is not None and value != p.default and value != getattr(neutral, name, p.default):
            raise ValueError(f"{name} does not go with num_beams: beam search is deterministic and ranks the model's own "
                             f"distribution (got {name}={value!r})")
    return W, lp, r


# ---- the fp8 key/value cache: the rule gpt2mi_kv_store_fp8 and the fp8 attention kernels quantise by, executable -------
KV_DTYPES = ("bf16", "fp8")
KV_MIN_EXP = -100  # the smallest scale exponent (an all-zero row has it)


def check_kv_dtype(kv_dtype) -> int:
    """gpt2mi_decode_plan.kv_format of a ``kv_dtype`` string (0 bf16, 1 fp8 e4m3), or a ValueError naming the choices."""
    if kv_dtype not in KV_DTYPES:
        raise ValueError(f'kv_dtype must be "bf16" or "fp8" (got {kv_dtype!r})')
    return KV_DTYPES.index(kv_dtype)


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """fp32 2^e for integer e in [-126, 127], from the exponent bits."""
    return ((e.to(torch.int32) + 127) << 23).view(F32)


def kv_quantize(x: torch.Tensor):
    """``(codes uint8 [..., 64], scale fp32 [...])`` of key or value rows x [..., 64] (pure torch, any device): what
    gpt2mi_kv_store_fp8 and the fp8 attention kernels store, bit for bit.

    One scale per 64-wide row, a power of two: with amax = max |x| over the row (the values widened to fp32) written
    m * 2^k, m in [1, 2), the exponent is e = k - 8 + (m > 1.75), the smallest with amax <= 448 * 2^e, clamped to
    e >= -100 (amax == 0: e = -100). ``codes`` are OCP e4m3 (``torch.float8_e4m3fn``) bytes of x * 2^-e rounded to
    nearest even, ``scale`` = 2^e. Scaling by a power of two is exact and |x * 2^-e| <= 448, so the cast never saturates
    and never gives NaN: a row's codes and scale are a pure function of its 64 values. NaN / Inf inputs are outside
    the contract."""
    if x.size(-1) != 64:
        raise ValueError(f"kv_quantize takes rows of 64 values [..., 64] (got {tuple(x.shape)})")
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    f, ex = torch.frexp(amax)  # amax = f * 2^ex with f in [0.5, 1): m = 2 f, k = ex - 1
    e = ex.to(torch.int32) - 9 + (f > 0.875).to(torch.int32)
    e = torch.where(amax == 0, torch.full_like(e, KV_MIN_EXP), e).clamp_min(KV_MIN_EXP)
    codes = (xf * _pow2(-e)[..., None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes, _pow2(e)


def kv_dequantize(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """fp32 [..., 64]: ``code * scale``, the value every fp8 kernel uses for a cached key or value (exact: an e4m3 value
    times a power of two is an fp32, and a bf16, number)."""
    return codes.view(torch.float8_e4m3fn).float() * scale[..., None]


def _check_token(name: str, token: int, vocab_size: int) -> None:
    if not 0 <= int(token) < vocab_size:
        raise ValueError(f"{name} {token} not in [0, vocab_size={vocab_size})")


@dataclass(frozen=True, eq=False)
class Sampler:
    """What decides a draw: the checked values (``of`` checks) that make a token a function of (logits, this record,
    draw key, position). The defaults are neutral; ``seed`` None is the host sampler (``sample_next`` from a
    ``torch.Generator``), ``logit_bias`` a device fp32 [rows, V] tensor read by row ``bias_row[b]`` (None: row b; -1:
    none). What belongs to one call is not here and stays an argument: ``gen_start``, ``row_id``, the history / ``seq``
    buffer, ``done`` and the ``LogprobBuffer`` (an output, not a rule)."""
    temperature: float = 1.0
    top_k: Optional[int] = None
    top_p: Optional[float] = None
    seed: Optional[int] = None
    eos_token_id: Optional[int] = None
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    min_p: float = 0.0
    min_new_tokens: int = 0
    stop: List[List[int]] = field(default_factory=list)
    logit_bias: Optional[torch.Tensor] = None
    bias_row: Optional[List[int]] = None

    @classmethod
    def of(cls, temperature=1.0, top_k=None, top_p=None, seed=None, eos_token_id=None, repetition_penalty=1.0,
           presence_penalty=0.0, frequency_penalty=0.0, min_p=None, min_new_tokens=0, stop=None, logit_bias=None,
           bias_row=None, *, vocab_size: Optional[int] = None, allowed_token_ids=None, rows: Optional[int] = None,
           device=None, per_row: bool = True) -> "Sampler":
        """The record of these values, or the ValueError naming the one that is wrong; ``vocab_size`` bounds the stop and
        bias tokens. A session passes ``logit_bias`` / ``bias_row`` as its C entries read them; that tensor lies on the
        device, and its values are read back and checked where it is bound (``DecodeSession._bind``), after the host-side
        checks, which then run beside the previous launch. ``generate`` / ``generate_many`` pass ``rows``, the number of
        prompts: ``logit_bias`` is then a ``{token: value}`` dict, a [V] tensor or (``per_row``) a [rows, V] tensor, and
        ``allowed_token_ids`` adds -inf everywhere else: one row on ``device`` that every prompt reads (``bias_row`` all
        0), or with a [rows, V] tensor prompt b's own. With a ``seed`` that form also checks ``eos_token_id``'s range."""
        if temperature < 0:
            raise ValueError(f"temperature must be >= 0 (got {temperature})")
        _check_top_p(top_p)
        if seed is not None and not isinstance(seed, int):
            raise ValueError(f"seed must be an int (got {seed!r})")
        rp, pp, fp, _ = _check_penalties(repetition_penalty, presence_penalty, frequency_penalty)
        mp, mn, stops = _check_constraints(logit_bias if rows is not None or isinstance(logit_bias, dict) else None, min_p,
                                           min_new_tokens, stop, eos_token_id, vocab_size)
        if rows is not None:
            V = vocab_size
            if seed is not None and eos_token_id is not None:
                _check_token("eos_token_id", eos_token_id, V)
            bias = None
            if isinstance(logit_bias, dict):
                bias = torch.zeros(1, V, dtype=F32)
                for t, v in logit_bias.items():
                    bias[0, int(t)] = float(v)
            elif logit_bias is not None:
                if logit_bias.dim() not in (1, 2) or (logit_bias.dim() == 2 and (not per_row or logit_bias.size(0) != rows)):
                    raise ValueError(f"logit_bias must be a dict, a [V={V}] tensor"
                                     f"{f' or a [B={rows}, V] tensor' if per_row else ''} (got {tuple(logit_bias.shape)})")
                bias = logit_bias.detach().float().reshape(-1, V).clone()
            if allowed_token_ids is not None:
                allowed = [int(t) for t in allowed_token_ids]
                if not allowed or not all(0 <= t < V for t in allowed):
                    raise ValueError(f"allowed_token_ids must be a non-empty list of tokens in [0, vocab_size={V}) (got "
                                     f"{allowed})")
                mask = torch.full((1, V), float("-inf"), dtype=F32)
                mask[0, allowed] = 0.0
                bias = mask if bias is None else bias + mask.to(bias.device)
            logit_bias = bias
            if bias is not None:
                logit_bias, bias_row = bias.to(device).contiguous(), range(rows) if bias.size(0) > 1 else [0] * rows
        return cls(temperature, top_k, top_p, seed, eos_token_id, rp, pp, fp, mp, mn, stops, logit_bias,
                   None if bias_row is None else [int(r) for r in bias_row])

    @property
    def penalised(self) -> bool:
        return (self.repetition_penalty, self.presence_penalty, self.frequency_penalty) != (1.0, 0.0, 0.0)

    @property
    def constrained(self) -> bool:
        return bool(self.min_p > 0 or self.min_new_tokens > 0 or self.stop or (
            self.logit_bias is not None and (self.bias_row is None or any(r >= 0 for r in self.bias_row))))

    def blocks(self, gen_start: List[int], bias_row: Optional[List[int]] = None, seqs: Optional[List[int]] = None,
               hist: Optional[torch.Tensor] = None):
        """The sampler bindings' two keyword blocks (penalties, constraints), ``{}`` for a neutral one; ``gen_start`` and
        ``bias_row`` one per row of the call. With
        ``seqs`` the call is a verify call whose row r is a position of sequence ``seqs[r]`` and the two tables are the
        sequences': row r reads its sequence's entries, and its history is row ``seqs[r]`` of ``hist``. The bias, min-p
        and the minimum length are functions of (row, position) and stay; the stop sequences are left out,
        ``speculate_loop`` matches them in the tokens it reads back."""
        pen = con = {}
        pick = (lambda t: t) if seqs is None else (lambda t: t and [t[b] for b in seqs])  # a table, by sequence
        if self.penalised:
            pen = dict(repetition=self.repetition_penalty, presence=self.presence_penalty,
                       frequency=self.frequency_penalty, gen_start=pick(gen_start))
            if seqs is not None:
                pen.update(hist=hist, hist_row=list(seqs))
        if self.constrained:
            bias = {} if self.logit_bias is None else dict(logit_bias=self.logit_bias, bias_row=pick(bias_row))
            con = dict(bias, min_p=self.min_p, min_new_tokens=self.min_new_tokens,
                       stop=self.stop if seqs is None else [], gen_start=pick(gen_start))
        return pen, con

    def keywords(self, gen_start) -> dict:
        """``DecodeSession.generate`` / ``speculate``'s keywords after ``eos_token_id``, the rows' generated parts starting
        at ``gen_start``: ``blocks`` under the session's names, so a neutral family is left out, ``gen_start`` with both."""
        pen, con = self.blocks(list(gen_start), self.bias_row)
        return {**{k + "_penalty" * (k != "gen_start"): v for k, v in pen.items()}, **con}

    def write_verify_history(self, seq: torch.Tensor, tok_t: torch.Tensor, seqs: List[int], poss: List[int],
                             gen_start: List[int]) -> dict:
        """The penalty block of a verify call, after writing the history it reads (``{}`` and nothing written without
        penalties): row r draws at ``poss[r] + 1`` from the tokens of sequence ``seqs[r]`` up to and including its own,
        ``tok_t[r]``, which one index write puts at ``seq[seqs[r], poss[r]]`` (a rejected draft stays above ``lens``,
        where nothing reads it before it is overwritten). That is the history the one-token loop has at that position,
        so the draws stay those of the loop. Returns ``blocks``' first, over ``hist = seq`` and ``hist_row = seqs``."""
        if not self.penalised:
            return {}
        seq.index_put_((torch.tensor(seqs, device=seq.device), torch.tensor(poss, device=seq.device)), tok_t)
        return self.blocks(gen_start, None, seqs, seq)[0]


def _check_lens(lens, B: int, P: int) -> List[int]:
    """``lens`` as a list of B ints in [1, P], or a ValueError."""
    lens = [int(n) for n in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
    if len(lens) != B:
        raise ValueError(f"{len(lens)} prompt lengths for B={B} rows")
    if not all(1 <= n <= P for n in lens):
        raise ValueError(f"prompt lengths {lens} not all in [1, P={P}]")
    return lens


def _check_row_id(row_id, B: int) -> Optional[List[int]]:
    if row_id is None:
        return None
    row_id = [int(r) for r in row_id]
    if len(row_id) != B or not all(0 <= r < 1 << 32 for r in row_id):
        raise ValueError(f"row_id must be B={B} ints in [0, 2^32) (got {row_id})")
    return row_id


def _check_model(model):
    """The engine of a model generation can run on (see the module docstring), or the reason it cannot."""
    if getattr(model, "precision", "auto") == "fp32":
        raise NotImplementedError('generation computes in bf16 with fp32 accumulation; model.precision == "fp32" has '
                                  "no decode kernels")
    if not model.arena.is_cuda:
        raise RuntimeError("gpt_2_distributed_amd runs only on the MI355X HIP path: move the model to a cuda device "
                           "(there is no CPU fallback)")
    eng = model.engine()
    if eng.param_provider is not None or eng.store is not None:
        raise NotImplementedError("generation needs the whole model's parameters on this rank: a "
                                  "FullyShardedDataParallel-wrapped model keeps only its shard (gather a state_dict into "
                                  "an unwrapped GPT2 and generate with that)")
    cfg = model.config
    if cfg.n_embd != 64 * cfg.n_head:
        raise NotImplementedError(f"the decode kernels implement head_dim 64 (n_embd {cfg.n_embd} / n_head {cfg.n_head})")
    return eng


class ShareGroups:
    """Which rows of a session share a prompt: the bookkeeping of ``DecodeSession.fork``, pure host logic.

    A share group is a set of rows and a length ``shared_len``: every member's cache holds identical bits at positions
    ``[0, shared_len)`` (with fp8 the codes and the scales). A row is in at most one group. ``group[b]`` is the lowest
    member of b's group, or b when b is alone; ``length[b]`` is the group's shared length, or 0 when b is alone: the
    two host arrays gpt2mi_decode_plan.share_group / share_len point at (include/gpt2mi.h, v24)."""

    def __init__(self, B: int):
        self.B = int(B)
        self.clear()

    def clear(self) -> None:
        """Dissolve every group (``prefill``, ``reset``)."""
        self.group, self.length = list(range(self.B)), [0] * self.B

    def members(self, b: int) -> List[int]:
        return [m for m in range(self.B) if self.group[m] == self.group[b]]

    @property
    def any(self) -> bool:
        return any(self.length)

    def leave(self, b: int) -> None:
        """Take row b out of its group (``refill``, a ``fork`` destination): if b was the lowest member the next lowest
        becomes the source, and a group left with one member dissolves."""
        rest = [m for m in self.members(b) if m != b]
        self.group[b], self.length[b] = b, 0
        if len(rest) == 1:
            self.group[rest[0]], self.length[rest[0]] = rest[0], 0
        else:
            for m in rest:
                self.group[m] = rest[0]

    def fork(self, src: int, dst_rows: Sequence[int], src_len: int, share: bool = True) -> None:
        """``dst_rows`` have become copies of ``src``'s first ``src_len`` positions. Each first leaves its group; with
        ``share`` they then join src's group at its length, or, src being alone, form a new group with it at
        ``src_len``."""
        for d in dst_rows:
            self.leave(d)
        if not share:
            return
        old = self.members(src)
        n = self.length[src] if len(old) > 1 else src_len
        rows = sorted(set(old) | set(dst_rows))
        for m in rows if len(rows) > 1 else ():  # (no destinations: src stays as it is)
            self.group[m], self.length[m] = rows[0], n


def _entry(pen: dict, lp: Optional[dict], con: Optional[dict]) -> str:
    """Which of the four sampler entries / generate loops a call goes to: the first that takes everything that is on
    (``pen`` and ``con`` empty when neutral, ``lp`` None without log-probabilities); it names itself in refusals."""
    return "constrained" if con else "logprobs" if lp is not None else "penalized" if pen else "ragged"


class _Call(NamedTuple):
    """A ``Sampler`` bound to a session for one call (``DecodeSession._bind``): the record, the bindings' keyword blocks
    ``pen`` / ``con`` (over the checked ``gen_start`` and bias rows) / ``ends``, the draw keys and the history buffer."""
    sampler: Sampler
    pen: dict
    con: dict
    ends: dict
    row_id: Optional[List[int]]
    hist: Optional[torch.Tensor]


class DecodeSession:
    """The key/value cache of ``batch_size`` sequences of up to ``max_len`` tokens, and the step that extends them.

    Cache: per layer ``kcache`` and ``vcache``, bf16 ``[B][H][Tcap][64]`` (a (b, h) stream is contiguous 128-byte rows).
    With ``kv_dtype="fp8"`` they are the uint8 e4m3 codes of ``kv_quantize`` (64-byte rows) and ``kscale`` / ``vscale``,
    fp32 ``[B][H][Tcap]``, hold a scale per row: 68 bytes per (head, position) and tensor where bf16 takes 128
    (``cache_bytes``). ``prefill`` and ``refill`` then quantise what they store, and every step attends over quantised
    keys and values, its own token's included (csrc/decode.hip attn_row), so a cached row has the bits ``kv_quantize``
    gives the bf16 row whichever call wrote it. The prompt's own attention runs in the bf16 trunk, unquantised: only
    what later steps read is quantised, and the logits ``prefill`` returns are those of the bf16 session.
    ``prefill(idx)`` starts the sequences from a prompt, ``step(tokens)`` appends one token to each; both return the fp32
    logits ``[B, V]`` of the newest position. ``lens`` (a host list of B ints) is the number of cached tokens of each
    row; ``pos`` is their common value (None while the rows disagree: ``prefill`` with ``lens``, ``refill``). Every call
    goes through the per-row C entries (``gpt2mi_*_ragged``) with ``lens``, whether the rows agree or not: a row's bits
    depend on its own position only.

    ``fork(src, dst_rows)`` makes rows copies of another (several samples of one prompt). Every row still has a complete
    cache of its own, so every method works on forked rows as on any other; what the session remembers (``share``, a
    ``ShareGroups``) is which rows hold identical bits below which length, and ``step`` / ``generate`` hand that to the
    attention kernel, which then reads those keys and values once per group (csrc/decode.hip attn_shared): the same
    bits, fewer bytes. ``share_group`` / ``share_len`` are the two host arrays."""

    def __init__(self, model, batch_size: int, max_len: Optional[int] = None, kv_dtype: str = "bf16"):
        self.kv_format = check_kv_dtype(kv_dtype)
        self.kv_dtype = kv_dtype
        eng = _check_model(model)
        cfg = model.config
        Tcap = cfg.n_positions if max_len is None else int(max_len)
        if not 1 <= batch_size <= MAX_BATCH:
            raise ValueError(f"batch_size {batch_size} not in [1, {MAX_BATCH}] (the decode GEMM's row limit)")
        if not 1 <= Tcap <= cfg.n_positions:
            raise ValueError(f"max_len {Tcap} not in [1, n_positions={cfg.n_positions}]")
        self.model, self.engine, self.cfg = model, eng, cfg
        self.B, self.Tcap = int(batch_size), Tcap
        self.lens: List[int] = [0] * self.B
        B, C, H, L, Vp = self.B, cfg.n_embd, cfg.n_head, cfg.n_layer, model.vpad
        dev = eng.device
        e = lambda *s, dt=BF16: torch.empty(*s, dtype=dt, device=dev)  # noqa: E731
        if self.kv_format == K.KV_FP8:
            self.kcache, self.vcache = e(L, B, H, Tcap, 64, dt=torch.uint8), e(L, B, H, Tcap, 64, dt=torch.uint8)
            self.kscale, self.vscale = e(L, B, H, Tcap, dt=F32), e(L, B, H, Tcap, dt=F32)
        else:
            self.kcache, self.vcache = e(L, B, H, Tcap, 64), e(L, B, H, Tcap, 64)
            self.kscale = self.vscale = None
        for name, t in self._scratch(B).items():  # x, xmid, ln, qkv, ao, h, mean, rstd, attn_ws, gemm_ws, logits
            setattr(self, name, t)
        self._tok = e(B, dt=torch.int64)  # the device loop's newest tokens (DecodeSession.generate)
        self._drawn = False               # True: generate() drew _tok from the logits in place and has not stepped it
        self._refill_ws = None            # (Tp, engine.Workspace) of the last refill's one-sequence prefill
        self._plan = self._build_plan({n: getattr(self, n) for n in SCRATCH}, 0)
        self._rows = None                 # (scratch of MAX_BATCH rows, its plan): extend / speculate, on first use
        self._last = None                 # (the sampling keywords of the last call, their Sampler): _record
        self._beam_ws = None              # beam_search's workspace (top-W, parents, the reorder's staging), on first use
        self.share = ShareGroups(self.B)
        self._share_arrays = ((ctypes.c_int * self.B)(), (ctypes.c_int * self.B)())  # what the plan points at

    def _scratch(self, M: int) -> dict:
        """The buffers a step over M rows writes (gpt2mi_decode_plan's x .. logits)."""
        cfg = self.cfg
        C, H, Vp = cfg.n_embd, cfg.n_head, self.model.vpad
        e = lambda *s, dt=BF16: torch.empty(*s, dtype=dt, device=self.engine.device)  # noqa: E731
        shapes = [(3 * C, C), (C, C), (4 * C, C), (C, 4 * C), (Vp, C)]
        return dict(x=e(M, C, dt=F32), xmid=e(M, C, dt=F32), ln=e(M, C), qkv=e(M, 3 * C), ao=e(M, C), h=e(M, 4 * C),
                    mean=e(M, dt=F32), rstd=e(M, dt=F32),
                    attn_ws=e(max(K.attn_decode_workspace(M, H, self.Tcap), 1), dt=F32),
                    gemm_ws=e(max(max(K.gemm_skinny_workspace(M, n, k) for n, k in shapes), 1), dt=F32),
                    logits=e(M, Vp, dt=F32))

    @property
    def pos(self) -> Optional[int]:
        """The number of cached tokens when every row has the same, else None (see ``lens``)."""
        return self.lens[0] if self.uniform else None

    @pos.setter
    def pos(self, value: int) -> None:
        self.lens = [int(value)] * self.B

    @property
    def uniform(self) -> bool:
        return min(self.lens) == max(self.lens)

    @property
    def device(self):
        return self.logits.device

    @property
    def cache_bytes(self) -> int:
        """The bytes of the key/value cache: the two tensors of every layer and, with fp8, their scales."""
        return sum(t.numel() * t.element_size() for t in (self.kcache, self.vcache, self.kscale, self.vscale)
                   if t is not None)

    def _store(self, l: int, qkv, row: Optional[int], B: int, Tp: int, P: int) -> None:
        """The K / V columns of the first P rows of each of qkv's B sequences of Tp rows into layer l's cache from
        position 0: every sequence of the session, or with ``row`` that one (B = 1)."""
        at = (l,) if row is None else (l, row)
        kc, vc, ks, vs = (t if t is None else t[at] for t in (self.kcache, self.vcache, self.kscale, self.vscale))
        K.kv_store(qkv, kc, vc, B, Tp, P, 0, self.cfg.n_head, 64, self.Tcap, kscale=ks, vscale=vs)

    def _build_plan(self, scratch: dict, rows: int) -> K.DecodePlan:
        """The plan over the session's weights and caches with ``scratch`` as its buffers, holding ``rows`` rows (0: B)."""
        eng, cfg = self.engine, self.cfg
        p = lambda n: eng.p(n).data_ptr()  # noqa: E731  fp32 master view
        w = lambda n: eng.w16(n).data_ptr()  # noqa: E731  bf16 shadow
        self._layers = (K.DecodeLayer * cfg.n_layer)()  # host array the plan points at: kept alive with the session
        for l, Y in enumerate(self._layers):
            pre = f"transformer.h.{l}."
            Y.ln1_w, Y.ln1_b, Y.ln2_w, Y.ln2_b = (p(pre + s) for s in ("ln1.weight", "ln1.bias", "ln2.weight",
                                                                         "ln2.bias"))
            Y.qkv_w, Y.proj_w, Y.fc1_w, Y.fc2_w = (w(pre + s) for s in ("attn.qkv.weight", "attn.proj.weight",
                                                                         "mlp.fc1.weight", "mlp.fc2.weight"))
            Y.qkv_b, Y.proj_b, Y.fc1_b, Y.fc2_b = (p(pre + s) for s in ("attn.qkv.bias", "attn.proj.bias",
                                                                         "mlp.fc1.bias", "mlp.fc2.bias"))
            Y.kcache, Y.vcache = self.kcache[l].data_ptr(), self.vcache[l].data_ptr()
            if self.kv_format == K.KV_FP8:
                Y.kscale, Y.vscale = self.kscale[l].data_ptr(), self.vscale[l].data_ptr()
        P = K.DecodePlan()
        P.B, P.C, P.H, P.L, P.Vp, P.Tcap = self.B, cfg.n_embd, cfg.n_head, cfg.n_layer, self.model.vpad, self.Tcap
        P.eps = cfg.layer_norm_eps
        P.wte, P.wpe = p("transformer.wte.weight"), p("transformer.wpe.weight")
        P.lnf_w, P.lnf_b = p("transformer.ln_f.weight"), p("transformer.ln_f.bias")
        P.wte_bf16 = w("transformer.wte.weight")  # the zero-padded [Vp, C] slot: the tied lm_head
        P.layers = ctypes.cast(self._layers, ctypes.POINTER(K.DecodeLayer))
        for n in SCRATCH:
            setattr(P, n, scratch[n].data_ptr())
        P.attn_ws_floats, P.gemm_ws_floats = scratch["attn_ws"].numel(), scratch["gemm_ws"].numel()
        P.rows = rows
        P.kv_format = self.kv_format
        return P

    def _ready(self, sync: bool):
        if self.model._engine is not self.engine:
            raise RuntimeError("the model was moved or copied after this DecodeSession was created: call "
                               "model.decoder() again")
        if sync:  # a foreign in-place update of the weights since the last forward: re-cast the bf16 shadow
            self.engine._sync_shadows(BF16, False)

    def reset(self) -> None:
        """Rewind to an empty cache (the next call is ``prefill``)."""
        self.pos, self._drawn = 0, False
        self.share.clear()
        self._sync_share()

    # ---- rows that share a prompt (gpt2mi_decode_plan.share_group / share_len) ----------------------------------------
    @property
    def share_group(self) -> List[int]:
        return list(self.share.group)

    @property
    def share_len(self) -> List[int]:
        return list(self.share.length)

    def _sync_share(self) -> None:
        """The step plan's view of ``share``: the two host arrays, or NULL while no row shares (v23's launches)."""
        sg, sl = self._share_arrays
        sg[:], sl[:] = self.share.group, self.share.length
        self._plan.set_share(*((sg, sl) if self.share.any else (None, None)))

    @torch.no_grad()
    def fork(self, src: int, dst_rows: Sequence[int], share: bool = True) -> None:
        """Make every row of ``dst_rows`` a copy of row ``src``: its cache below ``lens[src]`` (with fp8 codes and
        scales), its logits and its length. Several samples of one prompt then cost one prefill (``refill(src)``, then
        one ``fork``), and with ``share`` the rows form a share group, whose shared keys and values every later ``step``
        / ``generate`` reads once per group. A token ``generate`` drew and has not stepped is stepped first (``flush``).

        ``src`` alone: ``src`` and ``dst_rows`` form a new group with ``shared_len = lens[src]``; ``src`` already in a
        group: ``dst_rows`` join it at that group's length (a copy of ``src`` agrees with every member below it). A
        destination first leaves the group it was in. ``share=False`` copies and leaves the destinations alone (the
        baseline of tools/share_bench.py and of the equality tests). The copies are torch indexing on the cache tensors:
        once per prompt, not a hot path. ``ValueError``: ``src`` in ``dst_rows``, a row outside [0, B), duplicates in
        ``dst_rows``, ``lens[src] == 0``."""
        src, dst = int(src), [int(d) for d in dst_rows]
        if not all(0 <= r < self.B for r in [src] + dst):
            raise ValueError(f"fork rows src={src}, dst_rows={dst} not all in [0, B={self.B})")
        if src in dst:
            raise ValueError(f"fork: src={src} is among dst_rows={dst}")
        if len(set(dst)) != len(dst):
            raise ValueError(f"fork: duplicates in dst_rows={dst}")
        if self.lens[src] == 0:
            raise ValueError(f"fork: row src={src} is empty (lens[src] == 0): prefill or refill it first")
        self.flush()
        n = self.lens[src]
        if dst:
            at = torch.tensor(dst, device=self.device)
            for t in (self.kcache, self.vcache, self.kscale, self.vscale):
                if t is not None:  # [L][B][H][Tcap](...): the rows `at` of dim 1, positions below n
                    t[:, at, :, :n] = t[:, src:src + 1, :, :n]
            self.logits[at] = self.logits[src].clone()  # (torch refuses a source inside the written tensor)
            for d in dst:
                self.lens[d] = n
        self.share.fork(src, dst, n, share)
        self._sync_share()

    @torch.no_grad()
    def prefill(self, idx: torch.Tensor, lens: Optional[Sequence[int]] = None) -> torch.Tensor:
        """Run the prompt ``idx`` [B, P] and cache its keys and values; fp32 logits [B, V] of its last position.

        The prompt goes through the engine's trunk forward (the training kernels at bf16, p = 0, padded to the attention
        tile), the K / V columns of each layer's qkv activations are copied into the cache, and the lm_head runs on the
        last valid row of each sequence only.

        With ``lens`` (B ints, ``1 <= lens[b] <= P``) row b's prompt is ``idx[b, :lens[b]]`` and the rest of the row is
        padding: any valid token id. The trunk runs once on the padded batch (causal attention keeps positions
        ``< lens[b]`` independent of what follows them) and all P positions are copied into the cache: positions
        ``>= lens[b]`` then hold the padding's keys and values, which no step reads (row b attends over
        ``0..lens[b]`` only) and which are overwritten one by one as the row grows. The logits are those of position
        ``lens[b] - 1`` of each row."""
        eng, cfg = self.engine, self.cfg
        if idx.dim() != 2 or idx.size(0) != self.B:
            raise ValueError(f"prefill takes idx [B={self.B}, P] (got {tuple(idx.shape)})")
        P = idx.size(1)
        if not 1 <= P <= self.Tcap:
            raise ValueError(f"prompt length {P} not in [1, max_len={self.Tcap}]")
        if lens is not None:
            lens = _check_lens(lens, self.B, P)
        if not idx.is_cuda:
            raise RuntimeError("gpt_2_distributed_amd runs only on the MI355X HIP path: move the inputs to a cuda device")
        self._ready(True)
        self.share.clear()
        self._sync_share()
        eng.gemm_sched = eng.base_sched
        idx_p, _, _ = eng._pad(idx, None)
        B, Tp = idx_p.shape
        C, Vp = cfg.n_embd, self.model.vpad
        ws = eng.workspace(B, Tp, BF16)
        # p = 0: no dropout site reads its seed, so the step's dropout stream is not advanced
        eng._trunk_fwd(ws, idx_p, B, Tp, P, BF16, 0.0, 0.0, eng._seeds(0))
        for l in range(cfg.n_layer):
            self._store(l, ws.blocks[l].qkv, None, B, Tp, P)
        if lens is None:
            last = ws.lnf.view(B, Tp, C)[:, P - 1]  # rows b*Tp + P-1: row stride Tp*C
            K.gemm_skinny(K.EPI_F32, B, Vp, C, last, Tp * C, eng.w16("transformer.wte.weight"), C, self.logits, Vp,
                          workspace=self.gemm_ws)
            self.pos = P
        else:  # rows b*Tp + lens[b]-1, gathered into the session's [B, C] buffer
            rows = torch.tensor([b * Tp + n - 1 for b, n in enumerate(lens)], device=idx.device)
            torch.index_select(ws.lnf, 0, rows, out=self.ln)
            K.gemm_skinny(K.EPI_F32, B, Vp, C, self.ln, C, eng.w16("transformer.wte.weight"), C, self.logits, Vp,
                          workspace=self.gemm_ws)
            self.lens = lens
        self._drawn = False
        return self.logits[:, :cfg.vocab_size].clone()

    def _one_sequence_workspace(self, Tp: int):
        """The trunk workspace of refill's one-sequence prefill: the session's own (the engine's holds one shape at a
        time, the training step's), kept while the padded length repeats."""
        if self._refill_ws is None or self._refill_ws[0] != Tp:
            from .engine import Workspace
            self._refill_ws = None
            self._refill_ws = (Tp, Workspace(self.cfg, 1, Tp, self.model.vpad, self.engine.device, BF16))
        return self._refill_ws[1]

    @torch.no_grad()
    def refill(self, row: int, prompt: torch.Tensor) -> None:
        """Replace sequence ``row`` by the 1-D ``prompt`` while the other rows keep their cache, logits and position.

        The prompt runs as a prefill of one sequence: its keys and values go to the row's slices of the caches
        (contiguous ``[H][Tcap][64]``: kv_store at B = 1), its last position's logits to ``logits[row]`` (gemm_skinny at
        M = 1) and ``lens[row]`` becomes its length. Every shape of that prefill depends on the prompt alone, so the
        row's cache and logits are a function of (weights, prompt) only: not of the row, the batch size or what the
        other rows hold. ``generate_many``'s guarantee rests on this. A token ``generate`` drew and has not stepped is
        stepped first (``flush``), so that afterwards every row's logits are those of its next position."""
        eng, cfg = self.engine, self.cfg
        if not 0 <= int(row) < self.B:
            raise ValueError(f"row {row} not in [0, B={self.B})")
        if prompt.dim() != 1 or not 1 <= prompt.numel() <= self.Tcap:
            raise ValueError(f"refill takes a 1-D prompt of 1..max_len={self.Tcap} tokens (got {tuple(prompt.shape)})")
        if not prompt.is_cuda:
            raise RuntimeError("gpt_2_distributed_amd runs only on the MI355X HIP path: move the inputs to a cuda device")
        self.flush()
        self._ready(True)
        self.share.leave(int(row))  # (after the flush: that step still reads the row as a member)
        self._sync_share()
        eng.gemm_sched = eng.base_sched
        row, P = int(row), prompt.numel()
        idx_p, _, _ = eng._pad(prompt.view(1, P), None)
        Tp = idx_p.size(1)
        C, Vp = cfg.n_embd, self.model.vpad
        ws = self._one_sequence_workspace(Tp)
        eng._trunk_fwd(ws, idx_p, 1, Tp, P, BF16, 0.0, 0.0, eng._seeds(0))
        for l in range(cfg.n_layer):
            self._store(l, ws.blocks[l].qkv, row, 1, Tp, P)
        K.gemm_skinny(K.EPI_F32, 1, Vp, C, ws.lnf[P - 1], Tp * C, eng.w16("transformer.wte.weight"), C, self.logits[row],
                      Vp, workspace=self.gemm_ws)
        self.lens[row] = P

    @torch.no_grad()
    def flush(self) -> None:
        """Step the token the last ``generate`` ended on, if it has not been (the next ``generate`` would do it first)."""
        if self._drawn:
            self._step(self._tok)
            self._drawn = False

    def _step(self, tok: torch.Tensor) -> None:
        K.decode_step_ragged(self._plan, tok, self.lens)
        self.lens = [n + 1 for n in self.lens]

    @torch.no_grad()
    def step(self, tokens: torch.Tensor) -> torch.Tensor:
        """Append ``tokens`` [B] (one per sequence) at position ``lens[b]``; fp32 logits [B, V] for the position after."""
        if min(self.lens) == 0:
            raise RuntimeError("step before prefill: the cache is empty")
        if max(self.lens) >= self.Tcap:
            raise ValueError(f"the cache is full ({self.Tcap} positions): reset() or a larger max_len")
        if tokens.shape != (self.B,):
            raise ValueError(f"step takes tokens [B={self.B}] (got {tuple(tokens.shape)})")
        if not tokens.is_cuda:
            raise RuntimeError("gpt_2_distributed_amd runs only on the MI355X HIP path: move the inputs to a cuda device")
        self._ready(False)  # (the weights are those of the prefill: the shadow is synced there)
        tok = tokens.contiguous() if tokens.dtype == torch.int64 else tokens.long()
        self._step(tok)
        self._drawn = False
        return self.logits[:, :self.cfg.vocab_size].clone()

    # ---- device-side sampling (gpt2mi_sample_ragged, gpt2mi_decode_generate_ragged): nothing below returns to the host ----
    def _check_history(self, hist, name: str, reader: str, last: Optional[int] = None):
        """``hist`` (argument ``name``) as the history buffer of what ``reader`` names; with ``last``, reaching it."""
        if hist is None:
            raise ValueError(f"{reader} the rows' tokens: pass {name}, int64 [B={self.B}, T], holding row b's "
                             f"tokens at [0, lens[b])")
        if (hist.dtype != torch.int64 or hist.dim() != 2 or hist.size(0) != self.B or hist.stride(1) != 1
                or not hist.is_cuda or (last is not None and hist.size(1) < last)):
            shape = f"[B={self.B}, T]" if last is None else f"[B={self.B}, >= {last}]"
            raise ValueError(f"{name} must be a device int64 {shape} with contiguous rows")

    def _record(self, *values) -> Sampler:
        """``Sampler.of`` of a call's sampling keywords. A token loop passes the same values call after call: the last record
        is returned while they compare equal; none with a stop table or a bias, which a caller can change in place."""
        fixed = not values[10] and values[11] is None and values[12] is None
        if fixed and self._last is not None and self._last[0] == values:
            return self._last[1]
        s = Sampler.of(*values, vocab_size=self.cfg.vocab_size)
        self._last = (values, s) if fixed else None
        return s

    def _check_start(self, start: List[int]) -> None:
        if len(start) != self.B or not all(0 <= g <= m for g, m in zip(start, self.lens)):
            raise ValueError(f"gen_start {start} must be B={self.B} ints in [0, lens={self.lens}]")

    def _bind(self, s: Sampler, n: Optional[int], hist, row_id, gen_start, done, logprobs=None) -> "_Call":
        """A record bound to this session for one call: ``sample`` (``n`` None: one draw at ``lens``, ``hist`` its
        ``history``) or a run of ``n`` tokens (``generate`` / ``speculate``, ``hist`` their ``seq``; the token the previous
        call ended on is flushed). Every check that needs the session, in the order they always had, then ``_Call``."""
        V, name = self.cfg.vocab_size, "history" if n is None else "seq"
        if min(self.lens) == 0:
            raise RuntimeError("sampling before prefill: there are no logits")
        if s.seed is None:
            raise ValueError(f"seed must be an int (got {s.seed!r})")
        if V > K.SAMPLE_MAX_V:
            raise NotImplementedError(f"the sampling kernel holds rows of up to {K.SAMPLE_MAX_V} logits (vocab_size {V})")
        self._ready(False)
        row_id = _check_row_id(row_id, self.B)
        pen_on, con_on = s.penalised, s.constrained
        start = [0] * self.B if gen_start is None else [int(g) for g in gen_start]
        if n is None:
            if self._drawn:
                raise RuntimeError("the logits are those generate() drew its last token from: step() that token first")
            last = max(self.lens) if pen_on or s.stop else None  # (the position the history is read up to)
        else:
            reach = max(self.lens) + int(self._drawn) + n
            if reach > self.Tcap:
                raise ValueError(f"{n} more tokens do not fit the cache ({self.Tcap} positions): reset() or a larger max_len")
            if hist is not None and (hist.dtype != torch.int64 or hist.dim() != 2 or hist.size(0) != self.B
                                     or hist.stride(1) != 1):
                raise ValueError(f"seq must be int64 [B={self.B}, T] with contiguous rows")
            if s.eos_token_id is not None and (done is None or done.dtype != torch.uint8 or done.shape != (self.B,)):
                raise ValueError(f"eos_token_id needs done, uint8 [B={self.B}]")
            last = reach - 1
        if pen_on:
            self._check_history(hist, name, "penalties read")
            if last > K.PENALTY_MAX_HISTORY:
                raise NotImplementedError(f"the penalised sampler reads a history of up to {K.PENALTY_MAX_HISTORY} tokens "
                                          f"(GPT2MI_PENALTY_MAX_HISTORY); this call reaches position {last}")
            if hist.size(1) < last:
                raise ValueError(f"{name} holds {hist.size(1)} positions, the call reads up to {last}")
            self._check_start(start)
        if logprobs is not None and (not isinstance(logprobs, LogprobBuffer) or logprobs.B != self.B
                                     or logprobs.T < last + 1):
            raise ValueError(f"logprobs must be a LogprobBuffer of B={self.B} rows and at least {last + 1} columns")
        if n is not None:
            self.flush()  # the token the previous call ended on: what follows sees lens with it, as before
        bias, rows = s.logit_bias, None
        if bias is not None:
            _check_constraints(bias, vocab_size=V)  # (reads the device back: after the host-side checks above)
            if (not isinstance(bias, torch.Tensor) or bias.dtype != F32 or bias.dim() != 2 or bias.stride(1) != 1
                    or not bias.is_cuda):
                raise ValueError(f"logit_bias must be a device fp32 [rows, V={V}] tensor with contiguous rows")
            rows = list(range(self.B)) if s.bias_row is None else s.bias_row
            if len(rows) != self.B or not all(-1 <= r < bias.size(0) for r in rows):
                raise ValueError(f"bias_row {rows} must be B={self.B} ints in [-1, {bias.size(0)}) (None: row b reads "
                                 f"bias row b)")
        elif s.bias_row is not None:
            raise ValueError("bias_row goes with logit_bias")
        if con_on and s.stop:
            self._check_history(hist, name, "stop sequences are matched in", last)
            if done is None:
                raise ValueError(f"stop sequences need done, uint8 [B={self.B}]")
        if con_on and not pen_on:  # (with penalties it was checked against the shorter lens before the flush)
            self._check_start(start)
        pen, con = s.blocks(start, rows) if pen_on or con_on else ({}, {})
        ends = {} if s.eos_token_id is None else dict(eos=s.eos_token_id, done=done)
        return _Call(s, pen, con, ends, row_id, hist)

    def _draw(self, logits, pos, out, call: "_Call", lp: Optional[dict] = None) -> None:
        """One token per row of ``logits`` at ``pos`` into ``out``: gpt2mi_sample_ragged, or with ``call.pen`` (not
        empty) gpt2mi_sample_penalized over the history ``call.hist``. With ``lp`` (logprob, top_ids, top_logprobs,
        optionally col) gpt2mi_sample_logprobs: the draw and its values. With ``call.con`` gpt2mi_sample_constrained."""
        s, history = call.sampler, {"hist": call.hist} if call.pen or call.con else {}
        getattr(K, "sample_" + _entry(call.pen, lp, call.con))(
            logits, self.cfg.vocab_size, s.temperature, s.top_k, s.top_p, s.seed, pos, out,
            **{"row_id": call.row_id, **call.ends, **(lp or {}), **history, **call.pen, **call.con})

    def _draw_new(self, logits, pos, call: "_Call", top_n: Optional[int]):
        """``_draw`` into a new tensor [R]: (the tokens, None), or with ``top_n`` (the tokens, their values (logprob [R],
        top_ids [R, n], top_logprobs [R, n])) from buffers of R rows and one column (col 0, ld 1)."""
        R = logits.size(0)
        out = torch.empty(R, dtype=torch.int64, device=self.device)
        buf = None if top_n is None else LogprobBuffer(R, 1, top_n, self.device)
        self._draw(logits, pos, out, call, None if buf is None else dict(buf.tensors(), col=[0] * R))
        return out, None if buf is None else (buf.logprob[:, 0], buf.top_ids[:, 0], buf.top_logprobs[:, 0])

    def _loop(self, n: int, call: "_Call", lp: Optional[dict] = None) -> None:
        """``n`` sample-then-step rounds from ``lens`` into ``_tok``: gpt2mi_decode_generate_ragged, or its penalized form
        with ``call.pen``, logprobs form with ``lp`` (a LogprobBuffer's tensors), constrained form with ``call.con``."""
        s = call.sampler
        getattr(K, "decode_generate_" + _entry(call.pen, lp, call.con))(
            self._plan, self.cfg.vocab_size, s.temperature, s.top_k, s.top_p, s.seed, self.lens, n, self._tok,
            **{"row_id": call.row_id, "seq": call.hist, **call.ends, **(lp or {}), **call.pen, **call.con})

    @torch.no_grad()
    def sample(self, temperature: float = 1.0, top_k: Optional[int] = None, top_p: Optional[float] = None,
               seed: int = 0, row_id: Optional[Sequence[int]] = None, repetition_penalty: float = 1.0,
               presence_penalty: float = 0.0, frequency_penalty: float = 0.0, gen_start: Optional[Sequence[int]] = None,
               history: Optional[torch.Tensor] = None, logprobs: Optional[int] = None,
               logit_bias: Optional[torch.Tensor] = None, bias_row: Optional[Sequence[int]] = None,
               min_p: Optional[float] = None, min_new_tokens: int = 0, stop=None, eos_token_id: Optional[int] = None,
               done: Optional[torch.Tensor] = None):
        """Tokens [B] (int64, device) for position ``lens[b]`` from the logits of the last ``prefill`` / ``step``: one
        launch, no host synchronisation. Row b's token is a function of (its logits, the parameters, seed, its draw key,
        its position): ``sample_reference`` with ``uniform_at(seed, row_id[b], lens[b])``; ``row_id`` (B ints, default
        the row numbers) lets a sequence keep its draw stream whichever row it sits in.

        With a non-neutral ``repetition_penalty`` / ``presence_penalty`` / ``frequency_penalty`` the logits are first
        moved by ``apply_penalties`` over ``history[b, :lens[b]]`` (device int64 [B, T], required then: ``ValueError``
        without), the generated part from ``gen_start[b]`` (default 0); ``logits`` itself is not modified.

        ``logprobs=n`` (0 <= n <= 20) returns ``(tokens, logprob [B], top_ids [B, n], top_logprobs [B, n])``: the raw
        distribution's values of ``token_logprobs``, from the same launch (gpt2mi_sample_logprobs); the tokens are those
        of the call without.

        Constraints (gpt2mi_sample_constrained; ``apply_constraints``, ``sample_reference``'s ``min_p`` and
        ``stop_match`` are the rule), after the penalties: ``logit_bias`` (device fp32 [rows, V]) adds row
        ``bias_row[b]`` (None: b; -1: none) to row b's logits, -inf banning a token; ``min_new_tokens`` holds
        ``eos_token_id`` back while ``lens[b] - gen_start[b]`` is below it; ``min_p`` drops the tokens less than that
        fraction as likely as the most likely one; ``stop`` (up to 8 lists of up to 16 tokens) sets ``done[b]`` (uint8
        [B]) when the drawn token completes one of them inside ``history[b, gen_start[b]:]``. With ``eos_token_id`` and
        ``done`` a row whose flag is set draws eos, and one that draws eos gets it set."""
        s = self._record(temperature, top_k, top_p, seed, eos_token_id, repetition_penalty, presence_penalty,
                         frequency_penalty, min_p, min_new_tokens, stop, logit_bias, bias_row)
        call = self._bind(s, None, history, row_id, gen_start, done)
        out, values = self._draw_new(self.logits, self.lens, call, logprobs)
        return out if values is None else (out, *values)

    @torch.no_grad()
    def generate(self, n: int, temperature: float = 1.0, top_k: Optional[int] = None, top_p: Optional[float] = None,
                 seed: int = 0, eos_token_id: Optional[int] = None, seq: Optional[torch.Tensor] = None,
                 done: Optional[torch.Tensor] = None, row_id: Optional[Sequence[int]] = None,
                 repetition_penalty: float = 1.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
                 gen_start: Optional[Sequence[int]] = None, logprobs: Optional["LogprobBuffer"] = None,
                 logit_bias: Optional[torch.Tensor] = None, bias_row: Optional[Sequence[int]] = None,
                 min_p: Optional[float] = None, min_new_tokens: int = 0, stop=None) -> torch.Tensor:
        """Draw row b's tokens of positions ``lens[b] .. lens[b] + n - 1`` in one C call (gpt2mi_decode_generate_ragged:
        sample, step, sample, ... on the stream, no Python and no synchronisation in between). The tokens go to column
        ``lens[b] + i`` of ``seq`` (int64 [B, >= max(lens) + n], optional); with ``eos_token_id``, ``done`` (uint8 [B])
        marks finished rows, which keep emitting eos. Returns the newest tokens [B] (a buffer the next call overwrites).
        The last token drawn is not stepped until the next ``generate`` (which does it first), ``flush`` or ``step``.
        ``row_id`` as for ``sample``.

        With non-neutral penalties (as for ``sample``) ``seq`` is the history and is required (``ValueError`` without):
        row b holds its tokens at ``seq[b, :lens[b]]`` on entry, prompt included, and the loop reads what it appends
        (gpt2mi_decode_generate_penalized); ``gen_start[b]`` (default 0) is where the row's generated part begins.

        ``logprobs`` (a ``LogprobBuffer`` of B rows and as many columns as the call reaches) receives, in the column each
        token goes to in ``seq``, the token's raw log-probability and alternatives (gpt2mi_decode_generate_logprobs: the
        same launches with the sampling kernel's LP form, nothing more read back); a finished row's eos has 0.

        ``logit_bias`` / ``bias_row`` / ``min_p`` / ``min_new_tokens`` / ``stop`` as for ``sample``, still one C call
        (gpt2mi_decode_generate_constrained): ``seq`` is the history the stop sequences are matched in (required with
        them, as ``eos_token_id`` and ``done`` are), ``gen_start[b]`` where the row's generated part begins; a row that
        completes a stop sequence keeps its tokens and emits eos from the next position on."""
        s = self._record(temperature, top_k, top_p, seed, eos_token_id, repetition_penalty, presence_penalty,
                         frequency_penalty, min_p, min_new_tokens, stop, logit_bias, bias_row)
        n = int(n)
        if n < 1:
            raise ValueError(f"generate takes n >= 1 (got {n})")
        call = self._bind(s, n, seq, row_id, gen_start, done, logprobs)
        self._loop(n, call, None if logprobs is None else logprobs.tensors())
        self.lens = [m + n - 1 for m in self.lens]
        self._drawn = True
        return self._tok

    # ---- beam search (gpt2mi_decode_beam_search) ------------------------------------------------------------------------
    @torch.no_grad()
    def beam_search(self, n: int, num_beams: int, eos_token_id: Optional[int], seq: torch.Tensor, cum: torch.Tensor,
                    done: torch.Tensor, parents: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``n`` tokens of beam search over the session's rows in one C call (gpt2mi_decode_beam_search): rows
        ``g W .. g W + W - 1`` (W = ``num_beams``) are the beams of prompt g, made by ``refill(g W)`` and
        ``fork(g W, the others)``, so that they are one share group whose shared length is the prompt's. Per token: the
        rows' top-W log-probabilities, ``beam_select``, the move of positions [prompt length, lens) of the cache rows
        and of ``seq`` to the new parents, and the step; nothing is synchronised or read back. ``seq`` (int64 [B, >=
        max(lens) + n]) holds row b's tokens and receives the new ones at columns ``lens[b] + i``; ``cum`` (fp32 [B])
        and ``done`` (uint8 [B]) carry the state: ``[0, -inf, ...]`` per group and 0 before the first call. With
        ``eos_token_id`` finished beams keep emitting it. ``parents`` (int32 [n, B], optional) receives each step's
        parent rows. As after ``generate`` the last token is not stepped (``flush``); returns the newest tokens [B]."""
        n, W = int(n), int(num_beams)
        if n < 1:
            raise ValueError(f"beam_search takes n >= 1 (got {n})")
        if not 1 <= W <= K.LOGPROBS_MAX_TOP or self.B % W or W > self.cfg.vocab_size:
            raise ValueError(f"num_beams={num_beams} must lie in [1, {K.LOGPROBS_MAX_TOP}], divide B={self.B} and not "
                             f"exceed vocab_size={self.cfg.vocab_size}")
        if min(self.lens) == 0:
            raise RuntimeError("beam_search before prefill: there are no logits")
        if self.cfg.vocab_size > K.SAMPLE_MAX_V:
            raise NotImplementedError(f"the top-W kernel holds rows of up to {K.SAMPLE_MAX_V} logits "
                                      f"(vocab_size {self.cfg.vocab_size})")
        if eos_token_id is not None and not 0 <= int(eos_token_id) < self.cfg.vocab_size:
            raise ValueError(f"eos_token_id {eos_token_id} not in [0, vocab_size={self.cfg.vocab_size})")
        lo = list(self.lens)  # W = 1: a row is its own parent for ever, nothing moves
        for g in range(0, self.B if W > 1 else 0, W):
            rows = list(range(g, g + W))
            if (any(self.share.group[b] != g or self.share.length[b] < 1 for b in rows)
                    or len({self.lens[b] for b in rows}) != 1):
                raise ValueError(f"rows {g}..{g + W - 1} are not the beams of one prompt: refill({g}) and "
                                 f"fork({g}, the others) first (share_group {self.share.group[g:g + W]}, share_len "
                                 f"{self.share.length[g:g + W]}, lens {self.lens[g:g + W]})")
            lo[g:g + W] = self.share.length[g:g + W]
        if max(self.lens) + int(self._drawn) + n > self.Tcap:
            raise ValueError(f"{n} more tokens do not fit the cache ({self.Tcap} positions): reset() or a larger max_len")
        if (seq is None or seq.dtype != torch.int64 or seq.dim() != 2 or seq.size(0) != self.B or seq.stride(1) != 1
                or seq.size(1) < max(self.lens) + int(self._drawn) + n):
            raise ValueError(f"seq must be int64 [B={self.B}, >= {max(self.lens) + int(self._drawn) + n}] with contiguous "
                             f"rows")
        if cum is None or cum.dtype != F32 or cum.shape != (self.B,) or not cum.is_contiguous():
            raise ValueError(f"cum must be fp32 [B={self.B}]")
        if done is None or done.dtype != torch.uint8 or done.shape != (self.B,) or not done.is_contiguous():
            raise ValueError(f"done must be uint8 [B={self.B}]")
        if parents is not None and (parents.dtype != torch.int32 or not parents.is_contiguous()
                                    or parents.numel() < n * self.B):
            raise ValueError(f"parents must be a contiguous int32 [n={n}, B={self.B}]")
        self._ready(False)
        self.flush()
        window = max(m + n - 1 - l for m, l in zip(self.lens, lo))
        need = K.BEAM_LOOP_BYTES + K.beam_reorder_workspace(self.kv_format, self.cfg.n_layer, self.cfg.n_head, self.B, window)
        if self._beam_ws is None or self._beam_ws.numel() < need:
            self._beam_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        K.decode_beam_search(self._plan, self.cfg.vocab_size, W, self.lens, lo, n, self._tok, seq, cum, done,
                             self._beam_ws, eos=eos_token_id, parents=parents)
        self.lens = [m + n - 1 for m in self.lens]
        self._drawn = True
        return self._tok

    # ---- several tokens of a sequence per launch (gpt2mi_decode_extend) ----------------------------------------------
    def _rows_plan(self):
        """The plan whose buffers hold MAX_BATCH rows (same weights and caches), allocated on first use."""
        if self._rows is None:
            scratch = self._scratch(MAX_BATCH)
            self._rows = (scratch, self._build_plan(scratch, MAX_BATCH))
        return self._rows

    @torch.no_grad()
    def extend(self, tokens: torch.Tensor, counts: Optional[Sequence[int]] = None) -> torch.Tensor:
        """Append ``tokens[b, :counts[b]]`` (int64 [B, n] on the device; ``counts[b]`` in [0, n], default n) to row b at
        positions ``lens[b] ..``; fp32 logits [B, n, V] after each appended position, NaN where ``j >= counts[b]``.

        The rows of a call are (sequence, position) pairs of one ``gpt2mi_decode_extend``: the weights stream once for
        up to 64 of them, and a call is split along the token axis when ``sum(counts) > 64``. Every logits row, the
        cache and the final state (``lens[b] += counts[b]``, ``logits[b]`` those of the last appended position) have the
        bits of ``counts[b]`` ``step`` calls; a row with count 0 keeps its cache, logits and length. Works from an empty
        cache (``prefill`` is the fast path for long prompts: this one runs every position as a decode row). A token
        ``generate`` drew and has not stepped is stepped first, as in ``refill``."""
        if tokens.dim() != 2 or tokens.size(0) != self.B or tokens.dtype != torch.int64:
            raise ValueError(f"extend takes int64 tokens [B={self.B}, n] (got {tokens.dtype} {tuple(tokens.shape)})")
        if not tokens.is_cuda:
            raise RuntimeError("gpt_2_distributed_amd runs only on the MI355X HIP path: move the inputs to a cuda device")
        n = tokens.size(1)
        counts = [n] * self.B if counts is None else [int(c) for c in counts]
        if len(counts) != self.B or not all(0 <= c <= n for c in counts):
            raise ValueError(f"counts {counts} must be B={self.B} ints in [0, n={n}]")
        drawn = int(self._drawn)
        if any(m + drawn + c > self.Tcap for m, c in zip(self.lens, counts)):
            raise ValueError(f"lens {self.lens} + counts {counts} do not fit the cache ({self.Tcap} positions)")
        self.flush()
        self._ready(True)
        V = self.cfg.vocab_size
        out = torch.full((self.B, n, V), float("nan"), dtype=F32, device=self.device)
        scratch, plan = self._rows_plan()
        flat = tokens.reshape(-1)
        j0 = 0
        while j0 < max(counts, default=0):
            w = 1  # the widest slice of token columns whose rows fit one call
            while sum(max(0, min(c, j0 + w + 1) - j0) for c in counts) <= MAX_BATCH and j0 + w < max(counts):
                w += 1
            rows = [(b, j) for b in range(self.B) for j in range(j0, min(counts[b], j0 + w))]
            at = torch.tensor([b * n + j for b, j in rows], device=self.device)
            K.decode_extend(plan, flat[at], [b for b, _ in rows], [self.lens[b] + j for b, j in rows])
            got = scratch["logits"][:len(rows)]
            out.view(self.B * n, V)[at] = got[:, :V]
            last = [(r, b) for r, (b, j) in enumerate(rows) if j == counts[b] - 1]
            if last:
                self._accept([r for r, _ in last], [b for _, b in last])
            j0 += w
        self.lens = [m + c for m, c in zip(self.lens, counts)]
        return out

    def _accept(self, src: List[int], dst: List[int]) -> None:
        """``logits[dst[i]]`` = row ``src[i]`` of the last extend call's logits."""
        rows = self._rows[0]["logits"]
        self.logits.index_copy_(0, torch.tensor(dst, device=self.device),
                                rows.index_select(0, torch.tensor(src, device=self.device)))

    def _verify(self, toks: List[int], seqs: List[int], poss: List[int], keys: List[int], call: _Call,
                logprobs: Optional[int] = None):
        """One ``gpt2mi_decode_extend`` over the rows (token, sequence, position) and one ``gpt2mi_sample_ragged`` over
        their logits, row r at position ``poss[r] + 1`` with draw key ``keys[r]``; the R tokens, read back.

        ``call`` is the run's bound call, whose per-row tables the record re-indexes by ``seqs`` (``Sampler.blocks``). With
        ``logprobs=n`` the draw is gpt2mi_sample_logprobs and the result (the tokens, their values left on the device)."""
        V = self.cfg.vocab_size
        if not all(0 <= t < V for t in toks):
            raise ValueError(f"draft tokens must lie in [0, vocab_size={V}) (got {toks})")
        scratch, plan = self._rows_plan()
        R = len(toks)
        tok_t = torch.tensor(toks, dtype=torch.int64, device=self.device)
        K.decode_extend(plan, tok_t, seqs, poss)
        s, start = call.sampler, (call.pen or call.con).get("gen_start")
        pen = s.write_verify_history(call.hist, tok_t, seqs, poss, start)
        con = s.blocks(start, call.con.get("bias_row"), seqs)[1]
        rows = call._replace(pen=pen, con=con, ends={"eos": s.eos_token_id} if con else {}, row_id=keys, hist=None)
        out, values = self._draw_new(scratch["logits"][:R], [p + 1 for p in poss], rows, logprobs)
        return out.tolist() if values is None else (out.tolist(), values)

    @torch.no_grad()
    def speculate(self, n: int, k: int, draft_fn=None, temperature: float = 1.0, top_k: Optional[int] = None,
                  top_p: Optional[float] = None, seed: int = 0, eos_token_id: Optional[int] = None,
                  seq: Optional[torch.Tensor] = None, done: Optional[torch.Tensor] = None,
                  row_id: Optional[Sequence[int]] = None, repetition_penalty: float = 1.0,
                  presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
                  gen_start: Optional[Sequence[int]] = None, logprobs: Optional["LogprobBuffer"] = None,
                  logit_bias: Optional[torch.Tensor] = None, bias_row: Optional[Sequence[int]] = None,
                  min_p: Optional[float] = None, min_new_tokens: int = 0, stop=None) -> dict:
        """``generate(n, ...)`` with up to ``k`` drafted tokens of every row verified per pass over the weights: the same
        tokens in ``seq``, the same ``done`` flags and, with the last token drawn and not stepped, the same ``_tok``,
        ``lens`` and ``logits``, in fewer passes when the drafts are right. ``B * (k + 1) <= 64``.

        Each iteration, for every live row, ``draft_fn(history, m)`` (default ``ngram_draft``) proposes up to
        ``m = min(k, tokens the row still needs - 1)`` tokens; one ``gpt2mi_decode_extend`` runs the rows [the row's
        current token, its drafts ...], one ``gpt2mi_sample_ragged`` draws a token from each of their logits rows at the
        position after it with the sequence's draw key, and the tokens are read back. A draft is right iff it equals
        the token drawn before it: the sampler's token is a function of (logits row, parameters, seed, key, position)
        and a logits row has the bits the one-token step gives it, so the comparison of integers is exact for greedy and
        sampled decoding alike. The row advances by the accepted drafts + 1; cache entries of rejected drafts stay above
        ``lens[b]``, where no kernel reads them before they are overwritten. ``history`` is the row's tokens so far:
        ``seq[b, :lens[b]]`` on entry if ``seq`` is given (else empty), then what this call drew.

        A row that draws eos stops being stepped: its ``lens`` is then the position of that eos and its ``logits`` those
        the eos was drawn from (the plain call goes on stepping eos to ``lens + n - 1``); ``seq`` holds eos from there on
        as after the plain call. One host synchronisation per iteration is inherent: the positions of the next call are
        host arrays that depend on the tokens read back. Returns ``{"calls", "drafted", "accepted", "tokens"}``: verify
        calls, draft tokens proposed and accepted, tokens drawn.

        Penalties as for ``generate`` (``seq`` required), and as exact: the verify call's row r draws at ``poss[r] + 1``
        from the history of its sequence up to and including the row's token (``_verify``), which is the history the
        one-token loop has there.

        ``logprobs`` as for ``generate``, with the same bits: the first draw and every verify call run the sampler's LP
        form, an accepted row's value goes to its token's column and a rejected draft's is dropped with its token; the
        columns after a row's eos hold 0.

        Constraints as for ``generate``, and as exact: the bias, min-p and the minimum length are functions of (row,
        position), so a verify call applies them to its rows as the loop does at those positions; stop sequences are
        matched on the host (``stop_match``) in the tokens read back, and an accepted run ends at the token that
        completes one, as it does at eos."""
        n, k = int(n), int(k)
        if n < 1 or k < 0:
            raise ValueError(f"speculate takes n >= 1 and k >= 0 (got n={n}, k={k})")
        if self.B * (k + 1) > MAX_BATCH:
            raise ValueError(f"B={self.B} rows of {k} drafts + 1 exceed the {MAX_BATCH} rows of a call")
        s = self._record(temperature, top_k, top_p, seed, eos_token_id, repetition_penalty, presence_penalty,
                         frequency_penalty, min_p, min_new_tokens, stop, logit_bias, bias_row)
        call = self._bind(s, n, seq, row_id, gen_start, done, logprobs)
        lens0 = list(self.lens)
        if logprobs is not None:  # the call's columns: what no accepted row writes (after a row's eos) is 0
            at = torch.arange(logprobs.T, device=self.device)[None] - torch.tensor(lens0, device=self.device)[:, None]
            keep = (at < 0) | (at >= n)
            for t in (logprobs.logprob, logprobs.top_ids, logprobs.top_logprobs):
                t.masked_fill_(~keep if t.dim() == 2 else ~keep[..., None], 0)
        self._draw(self.logits, self.lens, self._tok, call, None if logprobs is None else logprobs.tensors())
        first = self._tok.tolist()
        history = [[] for _ in range(self.B)] if seq is None else [r[:m] for r, m in zip(seq.tolist(), lens0)]
        keys = list(range(self.B)) if call.row_id is None else call.row_id
        more = {} if logprobs is None else {"logprobs": logprobs}
        stopped = [False] * self.B
        if s.constrained and s.stop:
            more.update(stop=(s.stop, call.con["gen_start"], s.min_new_tokens), stopped=stopped)
        new, stats = speculate_loop(self, n, k, draft_fn or ngram_draft, eos_token_id, history, first, keys, call, **more)
        self._tok.copy_(torch.tensor([t[-1] for t in new], dtype=torch.int64))
        self._drawn = True
        if eos_token_id is not None:
            new = [t + [eos_token_id] * (n - len(t)) for t in new]  # a finished row keeps emitting eos
            done.copy_(torch.tensor([int(eos_token_id in t or stopped[b]) for b, t in enumerate(new)],
                                    dtype=torch.uint8))
        if seq is not None:
            cols = torch.tensor(lens0, device=self.device)[:, None] + torch.arange(n, device=self.device)[None]
            seq.scatter_(1, cols, torch.tensor(new, dtype=torch.int64, device=self.device))
        return stats


def ngram_draft(history: List[int], k: int, max_ngram: int = 3) -> List[int]:
    """Prompt-lookup drafting: the longest suffix of ``history`` of g tokens, g from ``max_ngram`` down to 1, that also
    occurs earlier; of its earlier occurrences the most recent; the (up to) k tokens that followed it. ``[]`` if no
    suffix recurs or k < 1."""
    n = len(history)
    if k < 1 or n < 2:
        return []
    # where an earlier occurrence of a suffix can end: the earlier positions of the last token, the latest first
    ends = [j for j in range(n - 2, -1, -1) if history[j] == history[-1]]
    for g in range(min(max_ngram, n - 1), 0, -1):
        tail = history[n - g:]
        for j in ends:
            if j + 1 >= g and history[j + 1 - g:j + 1] == tail:
                return history[j + 1:j + 1 + k]
    return []


def speculate_loop(sess, n: int, k: int, draft_fn, eos_token_id, history, first, keys, sampler, logprobs=None,
                   stop=None, stopped=None):
    """The bookkeeping of ``DecodeSession.speculate`` over a session (anything with ``B``, ``lens``, ``_verify`` and
    ``_accept``): ``first[b]`` is row b's first token, drawn and not stepped. Returns (the tokens of each row: n of
    them, or fewer ending in eos; the stats). A draft counts as accepted iff it equals the token drawn before it and
    that token is not eos; the row then advances by accepted + 1 and takes the logits row of its last accepted draft.

    With ``logprobs`` (a ``LogprobBuffer``; the first tokens' values are in it already) ``_verify`` is asked for the
    values too (``logprobs=top_n``, returning (tokens, values)); the value of the token drawn from row r belongs to
    column ``poss[r] + 1`` of its sequence and is put there iff the token is taken.

    With ``stop`` = (the stop sequences, each row's ``gen_start``, ``min_new_tokens``) a row also ends, as at eos, at
    the token that completes a stop sequence (``stop_match`` over ``history[b]`` and the row's tokens): an accepted run
    is cut there. ``stopped`` (a list of B bools) is set for such a row."""
    B = sess.B
    new = [[int(first[b])] for b in range(B)]
    stats = dict(calls=0, drafted=0, accepted=0, tokens=0)
    stopped = [False] * B if stopped is None else stopped

    def hit(b, toks):
        return stop is not None and toks[-1] != eos_token_id and stop_match(history[b] + toks, stop[1][b], stop[0], stop[2])

    for b in range(B):
        stopped[b] = hit(b, new[b])

    def live(b):
        return len(new[b]) < n and new[b][-1] != eos_token_id and not stopped[b]

    while any(live(b) for b in range(B)):
        toks, seqs, poss, ks, spans = [], [], [], [], []
        for b in filter(live, range(B)):
            m = min(k, n - len(new[b]) - 1)
            drafts = [int(t) for t in draft_fn(history[b] + new[b], m)][:m] if m > 0 else []
            spans.append((b, len(toks), drafts))
            for i, t in enumerate([new[b][-1]] + drafts):
                toks.append(t), seqs.append(b), poss.append(sess.lens[b] + i), ks.append(keys[b])
        if logprobs is None:
            drawn = sess._verify(toks, seqs, poss, ks, sampler)
        else:
            drawn, values = sess._verify(toks, seqs, poss, ks, sampler, logprobs=logprobs.top_n)
        src, dst, taken = [], [], []
        for b, r0, drafts in spans:
            a = 0
            while a < len(drafts) and drafts[a] == drawn[r0 + a] != eos_token_id:
                a += 1
            for i in range(a + 1 if stop is not None else 0):  # the run ends at the first token that completes a stop
                if hit(b, new[b] + [int(t) for t in drawn[r0:r0 + i + 1]]):
                    a, stopped[b] = i, True
                    break
            new[b] += [int(t) for t in drawn[r0:r0 + a + 1]]
            sess.lens[b] += a + 1
            src.append(r0 + a), dst.append(b)
            taken += range(r0, r0 + a + 1)
            stats["drafted"] += len(drafts)
            stats["accepted"] += a
        sess._accept(src, dst)
        if logprobs is not None:
            logprobs.put([seqs[r] for r in taken], [poss[r] + 1 for r in taken], values, taken)
        stats["calls"] += 1
    stats["tokens"] = sum(len(t) for t in new)
    return new, stats


EOS_CHUNK = 32  # device loop with eos_token_id: tokens issued between two reads of the done flags


def _pad_prompts(prompts, pad: int):
    """A list of 1-D token tensors as one right-padded [B, Pmax] int64 tensor and the list of their lengths."""
    if not prompts or any(p.dim() != 1 or p.numel() < 1 for p in prompts):
        raise ValueError("prompts must be a non-empty list of non-empty 1-D token tensors")
    lens = [p.numel() for p in prompts]
    idx = torch.full((len(prompts), max(lens)), pad, dtype=torch.int64, device=prompts[0].device)
    for b, p in enumerate(prompts):
        idx[b, :lens[b]] = p
    return idx, lens


def _prompts(model, idx, max_new_tokens, prompt_lens, pad_token_id, eos_token_id, samples: int = 1, pad_always=False):
    """``generate``'s prompts as ``(idx, lens, B, P, n, pad)``: ``idx`` int64 [B, P] (a list of 1-D prompts right-padded
    with ``pad``: the pad token, else eos, else 0; checked with ``prompt_lens`` or ``pad_always``), ``lens`` the prompt
    lengths (None: every row holds P tokens). With ``samples`` s > 1 row b * s + j is sample j of prompt b; B: the rows."""
    pad = pad_token_id if pad_token_id is not None else (eos_token_id if eos_token_id is not None else 0)
    if isinstance(idx, (list, tuple)):
        if prompt_lens is not None:
            raise ValueError("a list of prompts carries its own lengths: prompt_lens goes with a padded idx [B, P]")
        idx, prompt_lens = _pad_prompts(idx, pad)
    if idx.dim() != 2:
        raise ValueError(f"generate takes idx [B, P] (got {tuple(idx.shape)})")
    B, P = idx.shape
    if samples > 1:
        if B * samples > MAX_BATCH:
            raise ValueError(f"{B} prompts x num_samples={samples} = {B * samples} rows exceed the {MAX_BATCH} rows of a "
                             f"decode session (MAX_BATCH)")
        idx = idx.repeat_interleave(samples, dim=0)
        if prompt_lens is not None:
            prompt_lens = [int(m) for m in (prompt_lens.tolist() if isinstance(prompt_lens, torch.Tensor)
                                            else prompt_lens) for _ in range(samples)]
        B *= samples
    n = int(max_new_tokens)
    if n < 0:
        raise ValueError(f"max_new_tokens must be >= 0 (got {n})")
    if prompt_lens is not None:
        prompt_lens = _check_lens(prompt_lens, B, P)
        P = max(prompt_lens)
        idx = idx[:, :P]
    if prompt_lens is not None or pad_always:
        _check_token("pad_token_id", pad, model.config.vocab_size)
    if P + n > model.config.n_positions:
        raise ValueError(f"prompt length {P} + max_new_tokens {n} > n_positions {model.config.n_positions}")
    return idx.long(), prompt_lens, B, P, n, pad


def _chunks(n: int, eos_token_id, done, step) -> int:
    """``step(m)`` until ``n`` tokens are issued; their number. Without eos one call and nothing read back; with eos
    EOS_CHUNK at a time, ``done`` read once per chunk, until every row has emitted it (the caller cuts the result)."""
    made = 0
    while made < n:
        m = n - made if eos_token_id is None else min(EOS_CHUNK, n - made)
        step(m)
        made += m
        if eos_token_id is not None and bool(done.all()):
            break
    return made


@torch.no_grad()
def generate(model, idx, max_new_tokens: int, temperature: float = 1.0, top_k: Optional[int] = None,
             generator: Optional[torch.Generator] = None, eos_token_id: Optional[int] = None,
             top_p: Optional[float] = None, seed: Optional[int] = None, prompt_lens: Optional[Sequence[int]] = None,
             pad_token_id: Optional[int] = None, draft_tokens: Optional[int] = None, draft_fn=None,
             repetition_penalty: float = 1.0, presence_penalty: float = 0.0,
             frequency_penalty: float = 0.0, kv_dtype: str = "bf16", num_samples: int = 1, logprobs=None,
             num_beams: Optional[int] = None, length_penalty: float = 1.0, num_return_sequences: int = 1,
             logit_bias=None, allowed_token_ids=None, min_p: Optional[float] = None, min_new_tokens: int = 0, stop=None):
    """``GPT2.generate``: see there."""
    given = dict(locals())  # (the arguments by name: what the beam path refuses)
    check_kv_dtype(kv_dtype)
    rules = (temperature, top_k, top_p, seed, eos_token_id, repetition_penalty, presence_penalty, frequency_penalty,
             min_p, min_new_tokens, stop, logit_bias)
    if num_beams is not None:
        return _generate_beams(model, idx, max_new_tokens, num_beams, length_penalty, num_return_sequences, eos_token_id,
                               prompt_lens, pad_token_id, kv_dtype, given)
    if length_penalty != 1.0 or num_return_sequences != 1:
        raise ValueError("length_penalty and num_return_sequences go with num_beams")
    top_n = _check_logprobs(logprobs)
    s = int(num_samples)
    if s < 1:
        raise ValueError(f"num_samples must be >= 1 (got {num_samples})")
    idx, lens, B, P, n, pad = _prompts(model, idx, max_new_tokens, prompt_lens, pad_token_id, eos_token_id, s)
    sampler = Sampler.of(*rules, vocab_size=model.config.vocab_size, allowed_token_ids=allowed_token_ids, rows=B // s,
                         device=idx.device)
    if s > 1 and sampler.bias_row is not None:  # a prompt's bias row is its samples'
        sampler = replace(sampler, bias_row=[r for r in sampler.bias_row for _ in range(s)])
    if seed is not None and generator is not None:
        raise ValueError("seed selects the device sampler, which draws from (seed, row, position): it takes no generator")
    if draft_tokens is None and draft_fn is not None:
        raise ValueError("draft_fn goes with draft_tokens=k")
    if draft_tokens is not None:
        if seed is None:
            raise ValueError("draft_tokens needs the device sampler (seed=int): a draft is accepted by comparing it with "
                             "the token drawn at its position, which the host sampler's torch.Generator, a stream and "
                             "not a function of the position, cannot reproduce")
        if int(draft_tokens) < 1 or B * (int(draft_tokens) + 1) > MAX_BATCH:
            raise ValueError(f"draft_tokens={draft_tokens} must be >= 1 with B * (draft_tokens + 1) <= {MAX_BATCH} rows "
                             f"(B={B})")
    _check_model(model)
    if lens is None and n == 0:
        return idx.clone() if top_n is None else _no_logprobs(idx.clone(), top_n)
    return _generate(model, idx, lens, n, sampler, generator, pad,
                     None if draft_tokens is None else (int(draft_tokens), draft_fn), kv_dtype, s, top_n)


def _generate_beams(model, idx, max_new_tokens, num_beams, length_penalty, num_return_sequences, eos_token_id,
                    prompt_lens, pad_token_id, kv_dtype, given: dict) -> BeamOutput:
    """``generate(num_beams=W)``: every prompt through ``refill`` once and forked to its W rows (the ``num_samples``
    path), ``DecodeSession.beam_search`` in one call, or with eos in chunks (``_chunks``), then ``beam_rank`` on the host."""
    V = model.config.vocab_size
    idx, lens, B, P, n, pad = _prompts(model, idx, max_new_tokens, prompt_lens, pad_token_id, eos_token_id, pad_always=True)
    W, lp, nret = _check_beams(num_beams, length_penalty, num_return_sequences, B, V, given)
    if eos_token_id is not None:
        _check_token("eos_token_id", eos_token_id, V)
    _check_model(model)
    lens = lens or [P] * B
    dev, R = idx.device, B * W
    lens_t = torch.tensor(lens, device=dev).repeat_interleave(W)  # per row
    cols = torch.arange(P + n, device=dev)[None]
    seq = torch.full((R, P + n), pad, dtype=torch.int64, device=dev)
    seq[:, :P] = torch.where(cols[:, :P] < lens_t[:, None], idx.repeat_interleave(W, dim=0), seq[:, :P])
    cum = torch.full((R,), float("-inf"), dtype=F32, device=dev)
    cum[::W] = 0.0
    done = torch.zeros(R, dtype=torch.uint8, device=dev)
    made = 0
    if n > 0:
        sess = DecodeSession(model, R, P + n, kv_dtype)
        for b in range(B):
            sess.refill(b * W, idx[b, :lens[b]])
            sess.fork(b * W, range(b * W + 1, b * W + W))
        made = _chunks(n, eos_token_id, done, lambda m: sess.beam_search(m, W, eos_token_id, seq, cum, done))
    else:
        cum[:] = 0.0  # (nothing generated: every returned beam is the prompt)
    new = seq.gather(1, lens_t[:, None] + torch.arange(made, device=dev)[None])  # [R, made]
    length = torch.full((R,), made, dtype=torch.int64, device=dev)
    if eos_token_id is not None and made:
        hit = new == eos_token_id
        length = torch.where(hit.any(1), hit.int().argmax(1) + 1, length)
        made = int(length.max())  # the column by which every beam has emitted eos (or the last one issued)
    keep = cols[:, :P + made] < (lens_t + length)[:, None]
    tokens = torch.where(keep, seq[:, :P + made], torch.full_like(seq[:, :P + made], pad))
    return beam_pick(tokens, cum, length, W, lp, nret)


def _no_logprobs(tokens: torch.Tensor, top_n: int) -> GenerateOutput:
    """``tokens`` with the values of columns nothing was generated in."""
    shape, dev = tuple(tokens.shape), tokens.device
    return GenerateOutput(tokens, torch.zeros(shape, dtype=F32, device=dev),
                          torch.zeros(shape + (top_n,), dtype=torch.int32, device=dev),
                          torch.zeros(shape + (top_n,), dtype=F32, device=dev))


def _generate(model, idx, lens, n, s: Sampler, generator, pad, draft=None, kv_dtype="bf16", samples=1, top_n=None):
    """The token loop of ``generate``: [B, P + m], row b = its prompt, its m new tokens from column lens[b] on, then
    ``pad`` (``lens`` None: every row holds P tokens and nothing is padded). m = n, or with eos the number of tokens by
    which every row has emitted it. Host sampler: new tokens are collected per step and scattered into the buffer that
    holds the prompts; device sampler: gpt2mi_sample_ragged writes row b's token of step i to column lens[b] + i of it.
    With penalties that buffer is the history too, with the generated part starting at lens[b]; the host sampler writes
    each step's tokens into it as it goes and passes its logits through apply_penalties.
    ``top_n`` (None: off) returns a ``GenerateOutput``: the device sampler writes each token's log-probability and
    ``top_n`` alternatives to the token's column of a ``LogprobBuffer``, the host sampler takes them from
    ``token_logprobs`` of the step's logits, before the penalties; columns that hold no generated token (prompt, pad,
    after a row's eos) are 0.
    Constraints: the device sampler takes them as keywords and matches the stop sequences in the buffer; the host
    sampler passes its logits through ``apply_constraints`` after the penalties, gives ``min_p`` to ``sample_next`` and
    matches the stop sequences with ``stop_match`` in the tokens it has drawn."""
    eos_token_id = s.eos_token_id
    B, P = idx.shape
    dev = idx.device
    lens_t = torch.tensor([P] * B if lens is None else lens, device=dev)
    cols = torch.arange(P + n, device=dev)[None]
    seq = torch.full((B, P + n), pad, dtype=torch.int64, device=dev)
    seq[:, :P] = torch.where(cols[:, :P] < lens_t[:, None], idx, seq[:, :P])  # the callers' padding may be anything
    if n == 0:
        return seq if top_n is None else _no_logprobs(seq, top_n)
    buf = None if top_n is None else LogprobBuffer(B, P + n, top_n, dev)
    lp = {} if buf is None else {"logprobs": buf}
    idx = torch.where(cols[:, :P] < lens_t[:, None], idx, torch.zeros_like(idx))  # (a valid token id as padding)
    sess = DecodeSession(model, B, P + n, kv_dtype)
    if samples == 1:
        logits = sess.prefill(idx, lens)
    else:  # each distinct prompt once, by the prefill of one sequence generate_many uses, then copied to its samples
        for b in range(0, B, samples):
            sess.refill(b, idx[b, :P if lens is None else lens[b]])
            sess.fork(b, range(b + 1, b + samples))
        logits = sess.logits[:, :model.config.vocab_size].clone()
    if s.seed is not None:
        kw = s.keywords(lens_t.tolist())
        done = None if eos_token_id is None else torch.zeros(B, dtype=torch.uint8, device=dev)
        if draft is None:
            made = _chunks(n, eos_token_id, done, lambda m: sess.generate(
                m, s.temperature, s.top_k, s.top_p, s.seed, eos_token_id, seq, done, **kw, **lp))
        else:  # (draft = (k, draft_fn): the same tokens, up to k + 1 of a row per pass over the weights)
            sess.speculate(n, *draft, s.temperature, s.top_k, s.top_p, s.seed, eos_token_id, seq, done, **kw, **lp)
            made = n
        if eos_token_id is None:
            return seq if buf is None else GenerateOutput(seq, buf.logprob, buf.top_ids, buf.top_logprobs)
        new = seq.gather(1, lens_t[:, None] + torch.arange(made, device=dev)[None])
    else:
        toks = []
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        on, starts = s.penalised, lens_t.tolist()
        told = [r[:m] for r, m in zip(seq.tolist(), starts)] if s.constrained and s.stop else None  # the rows' tokens
        for i in range(n):
            raw = logits  # (the model's own row: what the log-probabilities are taken from)
            if on:
                logits = apply_penalties(logits, seq, lens_t + i, lens_t, s.repetition_penalty, s.presence_penalty,
                                         s.frequency_penalty)
            if s.constrained:
                logits = apply_constraints(logits, lens_t + i, lens_t, s.logit_bias, s.bias_row, s.min_new_tokens,
                                           eos_token_id)
            nxt = sample_next(logits, s.temperature, s.top_k, generator, s.top_p, s.min_p)
            if eos_token_id is not None:
                nxt = torch.where(done, torch.full_like(nxt, eos_token_id), nxt)  # a finished row keeps emitting eos
            if told is not None:  # a row that completes a stop sequence is finished from the next step on
                was, hits = done.tolist(), []
                for b, t in enumerate(nxt.tolist()):
                    told[b].append(t)
                    hits.append(not was[b] and stop_match(told[b], starts[b], s.stop, s.min_new_tokens))
                stop_hit = torch.tensor(hits, device=dev)
            if buf is not None:  # (a row finished before this step: 0, as the device sampler writes)
                live = list(range(B)) if eos_token_id is None else (~done).nonzero()[:, 0].tolist()
                buf.put(live, [int(m) + i for m in lens_t[live].tolist()], token_logprobs(raw, nxt, top_n), live)
            if eos_token_id is not None:
                done = done | (nxt == eos_token_id)
            if told is not None:
                done = done | stop_hit
            toks.append(nxt)
            if on:  # the next step's history
                seq.scatter_(1, (lens_t + i)[:, None], nxt[:, None])
            if eos_token_id is not None and bool(done.all()):
                break
            if i + 1 < n:
                logits = sess.step(nxt)
        new = torch.stack(toks, dim=1)
        made = new.size(1)
        seq.scatter_(1, lens_t[:, None] + torch.arange(made, device=dev)[None], new)
    if eos_token_id is not None:
        ended = (new == eos_token_id).cumsum(1) > 0
        if s.constrained and s.stop:  # a row that completed a stop sequence has ended from that column on
            rows = seq[:, :P + made].tolist()
            for b, m in enumerate(lens_t.tolist()):
                at = first_stop(rows[b][:m + made], m, s.stop, s.min_new_tokens, eos_token_id)
                if at is not None:
                    ended[b, at - m:] = True
        finished = ended.all(0)  # steps by which every row has emitted eos (or completed a stop sequence)
        if bool(finished.any()):
            made = int(finished.int().argmax()) + 1
    keep = cols[:, :P + made] < (lens_t + made)[:, None]
    tokens = torch.where(keep, seq[:, :P + made], torch.full_like(seq[:, :P + made], pad))
    if buf is None:
        return tokens
    if eos_token_id is not None:  # a finished row's further columns: 0 in the alternatives as in the value
        gen = cols[:, :P + made] >= lens_t[:, None]
        keep = keep & ~(((tokens == eos_token_id) & gen).cumsum(1) - ((tokens == eos_token_id) & gen).long() > 0)
    return GenerateOutput(tokens, *(torch.where(keep if t.dim() == 2 else keep[..., None], t[:, :P + made],
                                                torch.zeros_like(t[:, :P + made]))
                                    for t in (buf.logprob, buf.top_ids, buf.top_logprobs)))


@torch.no_grad()
def generate_many(model, prompts, max_new_tokens: int, batch_size: int = 32, temperature: float = 1.0,
                  top_k: Optional[int] = None, top_p: Optional[float] = None, seed: int = 0,
                  eos_token_id: Optional[int] = None, generator: Optional[torch.Generator] = None,
                  repetition_penalty: float = 1.0, presence_penalty: float = 0.0,
                  frequency_penalty: float = 0.0, kv_dtype: str = "bf16", logprobs=None, logit_bias=None,
                  allowed_token_ids=None, min_p: Optional[float] = None, min_new_tokens: int = 0, stop=None) -> list:
    """``GPT2.generate_many``: see there."""
    check_kv_dtype(kv_dtype)
    top_n = _check_logprobs(logprobs)
    if generator is not None:
        raise ValueError("generate_many draws on the device from (seed, prompt index, position): a torch.Generator is "
                         "one stream shared by the rows of a batch, so its draws would depend on the batching")
    prompts = list(prompts)
    if any(not isinstance(p, torch.Tensor) or p.dim() != 1 or p.numel() < 1 for p in prompts):
        raise ValueError("prompts must be non-empty 1-D token tensors")
    n = int(max_new_tokens)
    if n < 0:
        raise ValueError(f"max_new_tokens must be >= 0 (got {n})")
    if not 1 <= int(batch_size) <= MAX_BATCH:
        raise ValueError(f"batch_size {batch_size} not in [1, {MAX_BATCH}] (the decode GEMM's row limit)")
    longest = max((p.numel() for p in prompts), default=0)
    if longest + n > model.config.n_positions:
        raise ValueError(f"prompt length {longest} + max_new_tokens {n} > n_positions {model.config.n_positions}")
    if not isinstance(seed, int):
        raise ValueError(f"seed must be an int (got {seed!r})")
    sampler = Sampler.of(temperature, top_k, top_p, seed, eos_token_id, repetition_penalty, presence_penalty,
                         frequency_penalty, min_p, min_new_tokens, stop, logit_bias, vocab_size=model.config.vocab_size,
                         allowed_token_ids=allowed_token_ids, rows=int(batch_size), device=model.arena.device,
                         per_row=False)
    if not prompts or n == 0:
        return [p.long().clone() if top_n is None else _no_logprobs(p.long().clone(), top_n) for p in prompts]
    _check_model(model)
    # (at least a chunk and two positions, so that a dummy row of one token need not start over within a chunk)
    sess = DecodeSession(model, int(batch_size), min(model.config.n_positions, max(longest + n, EOS_CHUNK + 2)),
                         kv_dtype)
    return serve_prompts(sess, [p.long() for p in prompts], n, sampler, top_n)


def serve_prompts(sess, prompts, n: int, sampler: Sampler, logprobs: Optional[int] = None) -> list:
    """The loop of ``generate_many`` over a session (anything with DecodeSession's ``B``, ``Tcap``, ``lens``,
    ``device``, ``refill``, ``generate`` and ``flush``). Rows are slots: a slot holds prompt ``owner[row]`` (None: a
    dummy of one token whose output is dropped) and draws with ``row_id = owner[row]``. The device loop runs in chunks
    of at most EOS_CHUNK tokens, cut so that no live row passes its ``n`` tokens; after a chunk the done flags and the
    tokens are read once, finished rows (eos, or n tokens) are harvested, cut after their first eos, and refilled with
    the next pending prompt.

    With penalties in ``sampler`` ``seq`` is the history the sampler reads: a slot's prompt is written to
    ``seq[row, :len]`` when it is filled (otherwise seq holds generated tokens only) and the generated part starts at
    the prompt's length. A row reads its own row below its own position only, so a prompt's continuation still does
    not depend on what it is batched with.

    ``logprobs=top_n`` (None: off) gives ``generate`` a ``LogprobBuffer`` beside ``seq``; a harvested prompt is then a
    ``GenerateOutput`` cut where its tokens are cut (0 in the prompt's columns), and a slot's row of the buffer is
    cleared when the slot is filled.

    With constraints in ``sampler`` every slot reads the one bias row, the generated part starts at the prompt's length,
    and with stop sequences ``seq`` holds the prompts as with penalties; a harvested prompt is cut after the token that
    completed a stop sequence, as after eos."""
    B, dev = sess.B, sess.device
    eos_token_id, stops = sampler.eos_token_id, sampler.stop
    on = sampler.penalised or bool(stops)
    out: List[Optional[torch.Tensor]] = [None] * len(prompts)
    pending = list(range(len(prompts)))[::-1]  # (pop() serves them in input order)
    owner: List[Optional[int]] = [None] * B
    start, made = [0] * B, [0] * B  # the prompt length and the tokens drawn so far of each slot
    seq = torch.zeros(B, sess.Tcap, dtype=torch.int64, device=dev)
    done = torch.zeros(B, dtype=torch.uint8, device=dev)
    dummy = torch.zeros(1, dtype=torch.int64, device=dev)
    DUMMY_ID = 0xFFFFFFFF
    buf = None if logprobs is None else LogprobBuffer(B, sess.Tcap, logprobs, dev)
    lp = {} if buf is None else {"logprobs": buf}

    def fill(row):
        owner[row] = pending.pop() if pending else None
        prompt = dummy if owner[row] is None else prompts[owner[row]].to(dev)
        sess.refill(row, prompt)
        start[row], made[row] = prompt.numel(), 0
        done[row] = 0
        if on:
            seq[row, :prompt.numel()] = prompt
        if buf is not None:
            buf.clear(row)

    for row in range(B):
        fill(row)
    while any(o is not None for o in owner):
        m = min([EOS_CHUNK] + [n - made[r] for r in range(B) if owner[r] is not None])
        for r in range(B):  # a dummy row that a chunk would take past the cache starts over
            if owner[r] is None and sess.lens[r] + m + 1 > sess.Tcap:
                fill(r)
        sess.generate(m, sampler.temperature, sampler.top_k, sampler.top_p, sampler.seed, eos_token_id, seq, done,
                      row_id=[DUMMY_ID if o is None else o for o in owner], **sampler.keywords(start), **lp)
        sess.flush()  # every row's logits are now those of its next position: a refilled row joins on equal terms
        host = torch.cat([done.to(torch.int64)[:, None], seq], dim=1).cpu()  # the one read of the chunk
        for r in range(B):
            made[r] += m
            if owner[r] is None or not (made[r] >= n or (eos_token_id is not None and bool(host[r, 0]))):
                continue
            new = host[r, 1 + start[r]:1 + start[r] + made[r]]
            if eos_token_id is not None:
                hits = (new == eos_token_id).nonzero()
                if hits.numel():
                    new = new[:int(hits[0]) + 1]
                at = first_stop(new.tolist(), 0, stops, sampler.min_new_tokens, eos_token_id) if stops else None
                if at is not None:
                    new = new[:at + 1]
            out[owner[r]] = torch.cat([prompts[owner[r]].to(dev), new.to(dev)])
            if buf is not None:  # (device slices: nothing more is read back)
                end = start[r] + new.numel()
                out[owner[r]] = GenerateOutput(out[owner[r]], *(
                    torch.cat([torch.zeros_like(t[r, :start[r]]), t[r, start[r]:end]])
                    for t in (buf.logprob, buf.top_ids, buf.top_logprobs)))
            fill(r)
    return out
