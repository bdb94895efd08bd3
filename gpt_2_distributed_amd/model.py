"""GPT-2 with the reference's module surface, running on hand-written MI355X kernels.

Drop-in for `/root/reference/model.py`: same ``GPT2Config`` (frozen dataclass, same fields and
defaults, model.py:26-57), same module tree and parameter names (``transformer.wte/wpe/h[i].{ln1,
attn.{qkv,proj},ln2,mlp.{fc1,fc2}}/ln_f``, tied ``lm_head``; 148 parameters, 149 state_dict keys),
the same seed-42 private-generator init (model.py:249-268), and
``GPT2.forward(idx, labels=None) -> (logits, loss)`` (model.py:335-361). nanoGPT-style aliases the
north star names are exported too: ``GPT = GPT2``, ``forward(idx, targets=...)`` and
``configure_optimizers``.

What differs underneath (MI355X-first):
* all parameters live in one flat fp32 arena (``arena.py``) so AdamW / grad-norm / collectives are
  single passes; ``wte`` is padded to a multiple of 256 rows for the lm_head tiling;
* ``GPT2.forward`` is ONE autograd node: forward and backward of the whole network are explicit
  sequences of HIP kernels (``engine.py``) with bf16 MFMA GEMMs, fused epilogues, flash attention;
  under ``torch.autocast("cuda", torch.bfloat16)`` (the reference trainer,
  train_gpt2_distributed.py:404) it computes with CUDA-autocast-bf16 numerics (bf16 MFMA operands,
  fp32 LayerNorm/softmax/loss/residual); without autocast it computes in fp32 like the plain
  reference module (fp32 MFMA GEMMs, fp32 attention). ``model.precision = "bf16" | "fp32"``
  overrides the autocast-following default ``"auto"``;
* no [T,T] ``mask`` buffer (model.py:105-108): causality comes from tile indices (the buffer was
  non-persistent, so state_dicts are unchanged);
* the sub-modules of a GPT2 are callable on their own (``GPT2Backbone.forward(idx)`` -> ln_f output,
  ``GPT2Block.forward(x)``, ``MLP.forward(x)``, ``CausalMultiHeadSelfAttention.forward(x)``) and
  differentiable, through the same kernels; they read the parameters from the owning GPT2's arena, so a
  block constructed outside a GPT2 has no MI355X path (it raises).
The GPU path has no CPU fallback: a CPU ``forward`` raises.
"""
from __future__ import annotations

import math
import weakref
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn as nn

from .arena import ArenaLayout, round_up
from .packing import EOT_POSITIONS, DocBounds, check_bounds_meta
from .packing import doc_bounds as _doc_bounds


@dataclass(frozen=True)
class GPT2Config:
    """Configuration for the GPT-2 model (model.py:26-57)."""
    vocab_size: int = 50257
    n_positions: int = 1024
    n_embd: int = 768
    n_layer: int = 12
    n_head: int = 12
    resid_pdrop: float = 0.1
    attn_pdrop: float = 0.1
    layer_norm_eps: float = 1e-5
    initializer_range: float = 0.02


# Model sizes of BASELINE.json configs (the reference hard-codes 124M).
MODEL_SIZES = {
    "124M": dict(n_layer=12, n_head=12, n_embd=768),
    "350M": dict(n_layer=24, n_head=16, n_embd=1024),
    "1.5B": dict(n_layer=48, n_head=25, n_embd=1600),
}


class NewGELU(nn.Module):
    """tanh GELU (model.py:63-77). In the training step it is fused into the fc1 GEMM epilogue."""

    def forward(self, input):
        return 0.5 * input * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (input + 0.044715 * torch.pow(input, 3.0))))


class _OwnedByGPT2:
    """Sub-modules of a GPT2 run through the owner's engine (parameters live in its flat arena)."""

    def _bind_owner(self, owner: "GPT2", layer: Optional[int]):
        self._owner_ref = weakref.ref(owner)
        self._layer = layer

    def _owner_engine(self):
        ref = getattr(self, "_owner_ref", None)
        owner = ref() if ref is not None else None
        if owner is None:
            raise RuntimeError(f"{type(self).__name__} runs on the MI355X engine only as a sub-module of a GPT2 "
                               "model (its parameters live in the GPT2's flat arena)")
        if not owner.arena.is_cuda:
            raise RuntimeError("gpt_2_distributed_amd runs only on the MI355X HIP path: move the model to a cuda "
                               "device (there is no CPU fallback)")
        return owner.engine()


def _checked_reset(reset_positions, given: bool, needs: str) -> bool:
    """``reset_positions`` as a bool; ValueError when it is on without the bounds it restarts at."""
    if reset_positions and not given:
        raise ValueError(f"reset_positions=True needs {needs}: positions restart at document boundaries")
    return bool(reset_positions)


def _checked_bounds(doc_bounds, x) -> Optional[DocBounds]:
    """``doc_bounds`` checked against the leading [B, T] of ``x`` (idx or activations) and its device: ValueError on a
    wrong shape, dtype or device; the tensors are not read."""
    if doc_bounds is None:
        return None
    if x.dim() < 2:
        raise ValueError(f"doc_bounds go with a [B, T, ...] input, got shape {tuple(x.shape)}")
    return check_bounds_meta(doc_bounds, x.shape[0], x.shape[1], x.device)


class CausalMultiHeadSelfAttention(_OwnedByGPT2, nn.Module):
    """Causal multi-head self-attention (model.py:80-159): qkv, proj, attn/resid dropout. ``forward(x)``
    takes the ln1 output [B,T,C] and returns drop(proj(attention)) (bf16 under autocast). ``doc_bounds``: a
    ``packing.DocBounds`` of the rows, for document-masked attention (every ``doc_bounds`` keyword of this module:
    int32 [B, T] tensors on the input's device, checked by shape, dtype and device without a host synchronisation;
    ``packing.check_bounds`` validates the values)."""

    def __init__(self, cfg: GPT2Config):
        super().__init__()
        assert cfg.n_embd % cfg.n_head == 0
        self.n_head = cfg.n_head
        self.head_dim = cfg.n_embd // cfg.n_head
        self.qkv = nn.Linear(cfg.n_embd, 3 * cfg.n_embd)
        self.proj = nn.Linear(cfg.n_embd, cfg.n_embd)
        self.attn_drop = nn.Dropout(cfg.attn_pdrop)
        self.resid_drop = nn.Dropout(cfg.resid_pdrop)

    def forward(self, x, doc_bounds: Optional[DocBounds] = None):
        doc_bounds = _checked_bounds(doc_bounds, x)
        return self._owner_engine().sub_forward("attn", self._layer, x, doc_bounds)


class MLP(_OwnedByGPT2, nn.Module):
    """MLP (model.py:162-192): fc1 -> NewGELU -> drop1 -> fc2 -> drop2. ``forward(x)`` takes the ln2
    output [B,T,C] (bf16 under autocast)."""

    def __init__(self, cfg: GPT2Config):
        super().__init__()
        hidden = 4 * cfg.n_embd
        self.fc1 = nn.Linear(cfg.n_embd, hidden)
        self.fc2 = nn.Linear(hidden, cfg.n_embd)
        self.act = NewGELU()
        self.drop1 = nn.Dropout(cfg.resid_pdrop)
        self.drop2 = nn.Dropout(cfg.resid_pdrop)

    def forward(self, x):
        return self._owner_engine().sub_forward("mlp", self._layer, x)


class GPT2Block(_OwnedByGPT2, nn.Module):
    """One transformer block (model.py:195-219); the unit the FSDP mode shards by. ``forward(x)``:
    x + attn(ln1(x)), then x + mlp(ln2(x)) on the fp32 residual stream [B,T,C]."""

    def __init__(self, cfg: GPT2Config):
        super().__init__()
        self.ln1 = nn.LayerNorm(cfg.n_embd, eps=cfg.layer_norm_eps)
        self.attn = CausalMultiHeadSelfAttention(cfg)
        self.ln2 = nn.LayerNorm(cfg.n_embd, eps=cfg.layer_norm_eps)
        self.mlp = MLP(cfg)

    def forward(self, x, doc_bounds: Optional[DocBounds] = None):
        doc_bounds = _checked_bounds(doc_bounds, x)
        return self._owner_engine().sub_forward("block", self._layer, x, doc_bounds)


class GPT2Backbone(_OwnedByGPT2, nn.Module):
    """Embeddings + blocks + ln_f (model.py:225-313), same init (model.py:249-268)."""

    def __init__(self, cfg: GPT2Config):
        super().__init__()
        self.cfg = cfg
        self.wte = nn.Embedding(cfg.vocab_size, cfg.n_embd)
        self.wpe = nn.Embedding(cfg.n_positions, cfg.n_embd)
        self.drop = nn.Dropout(cfg.resid_pdrop)
        self.h = nn.ModuleList([GPT2Block(cfg) for _ in range(cfg.n_layer)])
        self.ln_f = nn.LayerNorm(cfg.n_embd, eps=cfg.layer_norm_eps)
        self.init_rng = torch.Generator()
        self.init_rng.manual_seed(42)
        self.apply(self._init_weights)

    def _init_weights(self, module):
        if isinstance(module, (nn.Linear, nn.Embedding)):
            nn.init.normal_(module.weight, mean=0.0, std=self.cfg.initializer_range, generator=self.init_rng)
        if isinstance(module, nn.Linear) and module.bias is not None:
            nn.init.zeros_(module.bias)

    @property
    def max_seq_len(self):
        return self.cfg.n_positions

    def forward(self, idx: torch.Tensor, doc_bounds: Optional[DocBounds] = None,
                reset_positions: bool = False) -> torch.Tensor:
        """Embeddings -> blocks -> ln_f (model.py:275-313); returns the fp32 ln_f output [B,T,C]. ``doc_bounds`` and
        ``reset_positions`` as in ``GPT2.forward``."""
        reset_positions = _checked_reset(reset_positions, doc_bounds is not None, "doc_bounds")
        doc_bounds = _checked_bounds(doc_bounds, idx)
        B, T = idx.size()
        if T > self.cfg.n_positions:
            raise ValueError(f"Sequence length {T} > model max {self.cfg.n_positions}")
        eng = self._owner_engine()
        if not idx.is_cuda:
            raise RuntimeError("gpt_2_distributed_amd runs only on the MI355X HIP path: move the inputs to a cuda "
                               "device (there is no CPU fallback)")
        return eng.backbone_forward(idx, doc_bounds, reset_positions)


class GPT2(nn.Module):
    """GPT-2 backbone + tied language-model head (model.py:316-361)."""

    def __init__(self, cfg: GPT2Config):
        super().__init__()
        self.config = cfg
        self.transformer = GPT2Backbone(cfg)
        self.lm_head = nn.Linear(cfg.n_embd, cfg.vocab_size, bias=False)
        self.lm_head.weight = self.transformer.wte.weight
        self._pack_arena()
        self._engine = None
        self.precision = "auto"
        self._bind_submodules()

    def _bind_submodules(self):
        self.transformer._bind_owner(self, None)
        for i, blk in enumerate(self.transformer.h):
            blk._bind_owner(self, i)
            blk.attn._bind_owner(self, i)
            blk.mlp._bind_owner(self, i)

    # copies (copy.deepcopy / pickling) get their own engine and re-point their sub-modules at themselves
    def __getstate__(self):
        st = self.__dict__.copy()
        st["_engine"] = None
        return st

    def __setstate__(self, st):
        super().__setstate__(st)
        self._rebind(self._arena)  # a copied Parameter is a clone, no longer a view of the copied arena
        self._bind_submodules()  # "auto": follow torch.autocast("cuda"); or force "bf16" / "fp32"

    # ---- flat arena ------------------------------------------------------------------------------
    def _pack_arena(self):
        cfg = self.config
        self.vpad = round_up(cfg.vocab_size, 256)
        names = [n for n, _ in self.named_parameters()]
        shapes = {n: tuple(p.shape) for n, p in self.named_parameters()}
        from collections import OrderedDict
        self.layout = ArenaLayout(OrderedDict((n, shapes[n]) for n in names), self.vpad)
        arena = torch.zeros(self.layout.total, dtype=torch.float32)
        for n, p in self.named_parameters():
            self.layout.view(arena, n).copy_(p.detach())
        self._arena = arena
        self._rebind(arena)

    def _rebind(self, arena: torch.Tensor):
        self._arena = arena
        for name in self.layout.slots:
            mod_path, attr = name.rsplit(".", 1)
            mod = self.get_submodule(mod_path)
            old = getattr(mod, attr)
            newp = nn.Parameter(self.layout.view(arena, name), requires_grad=old.requires_grad)
            setattr(mod, attr, newp)
        self.lm_head.weight = self.transformer.wte.weight

    def _apply(self, fn, recurse=True):
        # Move the arena as a whole so parameters stay views of one buffer.
        new = fn(self._arena)
        if new.dtype != torch.float32:
            raise TypeError("GPT2 keeps fp32 master weights in one arena; only device moves are supported "
                            "(the bf16 compute copy is managed by the engine)")
        if new.data_ptr() != self._arena.data_ptr():
            self._rebind(new)
            self._engine = None
        for m in self.children():
            for sub in m.modules():
                for k, b in list(sub._buffers.items()):
                    if b is not None:
                        sub._buffers[k] = fn(b)
        return self

    @property
    def arena(self) -> torch.Tensor:
        return self._arena

    def engine(self):
        if self._engine is None:
            from .engine import Engine
            self._engine = Engine(self)
        return self._engine

    # ---- forward -----------------------------------------------------------------------------------
    def forward(self, idx: torch.Tensor, labels: Optional[torch.Tensor] = None,
                targets: Optional[torch.Tensor] = None, *,
                doc_bounds: Optional[DocBounds] = None,
                reset_positions: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """``doc_bounds``: the ``packing.DocBounds`` of ``idx`` (``packing.doc_bounds(idx, eot_token_id)`` forms them on
        the device): every token attends only to the earlier tokens of its own document. ``None``: plain causal
        attention, the kernel launches as they were. Positions stay absolute (``wpe[t]``) unless ``reset_positions``:
        then, with ``doc_bounds``, a token takes the position embedding of its offset in its document
        (``packing.doc_positions``), so a document sees the inputs it would see alone in the row; ValueError without
        ``doc_bounds``. Off, the embedding launches are the ones they were."""
        reset_positions = _checked_reset(reset_positions, doc_bounds is not None, "doc_bounds")
        if targets is not None:
            if labels is not None:
                raise ValueError("pass labels or targets, not both")
            labels = targets
        doc_bounds = _checked_bounds(doc_bounds, idx)
        B, T = idx.size()
        if T > self.config.n_positions:
            raise ValueError(f"Sequence length {T} > model max {self.config.n_positions}")
        if not idx.is_cuda or not self._arena.is_cuda:
            raise RuntimeError("gpt_2_distributed_amd.GPT2 runs only on the MI355X HIP path: move the model and "
                               "inputs to a cuda device (there is no CPU fallback)")
        return self.engine().forward(idx, labels, doc_bounds, reset_positions)

    # ---- evaluation (the reference has none) ----------------------------------------------------------------
    def _check_inputs(self, idx):
        B, T = idx.size()
        if T > self.config.n_positions:
            raise ValueError(f"Sequence length {T} > model max {self.config.n_positions}")
        if not idx.is_cuda or not self._arena.is_cuda:
            raise RuntimeError("gpt_2_distributed_amd.GPT2 runs only on the MI355X HIP path: move the model and "
                               "inputs to a cuda device (there is no CPU fallback)")

    def score(self, idx: torch.Tensor, labels: torch.Tensor, reduction: str = "mean",
              doc_bounds: Optional[DocBounds] = None, reset_positions: bool = False) -> torch.Tensor:
        """The negative log-likelihood of ``labels`` [B, T] under the model, forward only: ``"none"`` the fp32 per-token
        values [B, T] (0 where the label is -100), ``"sum"`` their sum, ``"mean"`` sum / number of labels != -100 (what
        ``forward(idx, labels)[1]`` computes in eval mode). Same argument checks as ``forward``; ``doc_bounds`` and
        ``reset_positions`` as there.

        Under bf16 autocast (or ``precision == "bf16"``) the lm_head runs fused with the cross-entropy
        (``gpt2mi_lm_loss``): no logits tensor exists and the label's logit and the log-sum-exp are taken from the fp32
        accumulators, not from bf16-rounded logits. It needs neither the training workspace nor ``model.eval()``:
        dropout is off whatever ``self.training`` is, which is not changed, and the dropout stream and everything a
        later backward needs are left alone: a call between two training steps changes no state that a later step
        reads (weights, shadows, gradients, optimizer state, dropout stream, training workspace). Not differentiable: the results carry no graph, whatever the grad mode."""
        if reduction not in ("mean", "sum", "none"):
            raise ValueError(f"reduction must be 'mean', 'sum' or 'none' (got {reduction!r})")
        reset_positions = _checked_reset(reset_positions, doc_bounds is not None, "doc_bounds")
        doc_bounds = _checked_bounds(doc_bounds, idx)
        self._check_inputs(idx)
        rows, s, _, mean = self.engine().score(idx, labels, doc=doc_bounds, reset=reset_positions)
        if reduction == "none":
            return rows.clone()
        return (s if reduction == "sum" else mean).reshape(()).clone()

    def evaluate(self, batches, max_batches: Optional[int] = None, eot_token_id: Optional[int] = None,
                 eot: str = "end", reset_positions: bool = False) -> dict:
        """``{"loss", "ppl", "tokens"}`` over the ``(idx, labels)`` pairs of ``batches`` (at most ``max_batches``):
        loss = sum of the token losses / number of tokens over ALL batches (token-weighted, not a mean of batch means),
        ppl = exp(loss). The sums stay on the device (``gpt2mi_lm_loss``'s accumulate mode) and the host synchronises
        once, at the end. With ``torch.distributed`` initialised the two sums are all-reduced before the division, so
        every rank returns the same numbers; every rank must then be given the same number of batches (a collective).
        With ``eot_token_id`` every batch is scored under document masking: its bounds are formed on the device from its
        ``idx`` (``packing.doc_bounds(idx, eot_token_id, eot)``, ``eot`` = ``"end"`` or ``"begin"``), and with
        ``reset_positions`` also with positions restarting at every document (ValueError without ``eot_token_id``)."""
        import torch.distributed as dist
        reset_positions = _checked_reset(reset_positions, eot_token_id is not None, "eot_token_id")
        if eot not in EOT_POSITIONS:
            raise ValueError(f"eot must be one of {EOT_POSITIONS}, got {eot!r}")
        if eot_token_id is not None and (isinstance(eot_token_id, bool) or not isinstance(eot_token_id, int)
                                         or eot_token_id < 0):
            raise ValueError(f"eot_token_id must be a non-negative int or None, got {eot_token_id!r}")
        dev = self._arena.device
        eng = self.engine()
        acc = (torch.zeros(1, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev))
        total = torch.zeros(2, dtype=torch.float64, device=dev)
        pending = 0
        for n, (idx, labels) in enumerate(batches):
            if max_batches is not None and n >= max_batches:
                break
            idx, labels = idx.to(dev, non_blocking=True), labels.to(dev, non_blocking=True)
            self._check_inputs(idx)
            # the kernel adds into fp32 running sums; they move to fp64 before they pass 2^20 tokens (a batch of the
            # bench shape: every batch), so the count stays exact and a batch's sum is rounded against a small total
            if pending and pending + idx.numel() > 1 << 20:
                total += torch.cat(acc).double()
                acc[0].zero_()
                acc[1].zero_()
                pending = 0
            doc = None if eot_token_id is None else _doc_bounds(idx, eot_token_id, eot)
            eng.score(idx, labels, acc=acc, doc=doc, reset=reset_positions)
            pending += idx.numel()
        total += torch.cat(acc).double()
        if dist.is_available() and dist.is_initialized():
            from .parallel import use_collectives
            if use_collectives(dist.get_world_size()):
                dist.all_reduce(total)
        s, c = total.tolist()  # the one host sync
        loss = s / c if c else float("nan")
        return {"loss": loss, "ppl": math.exp(loss) if loss < 700 else float("inf"), "tokens": int(c)}

    # ---- generation (nanoGPT's surface; the reference has none) ----------------------------------------
    def decoder(self, batch_size: int, max_len: Optional[int] = None, kv_dtype: str = "bf16"):
        """A ``generation.DecodeSession``: the per-layer key/value cache (L x 2 x bf16 ``[B][H][Tcap][64]``,
        ``Tcap = max_len or n_positions``) of ``batch_size`` sequences with ``prefill(idx)`` / ``step(tokens)``.
        ``kv_dtype="fp8"``: the cache as e4m3 codes with one power-of-two scale per 64-wide row, 0.53 x the bytes
        (``generation.kv_quantize``)."""
        from .generation import DecodeSession
        return DecodeSession(self, batch_size, max_len, kv_dtype)

    def generate(self, idx, max_new_tokens: int, temperature: float = 1.0, top_k: Optional[int] = None,
                 generator: Optional[torch.Generator] = None, eos_token_id: Optional[int] = None,
                 top_p: Optional[float] = None, seed: Optional[int] = None, prompt_lens=None,
                 pad_token_id: Optional[int] = None, draft_tokens: Optional[int] = None,
                 draft_fn=None, repetition_penalty: float = 1.0, presence_penalty: float = 0.0,
                 frequency_penalty: float = 0.0, kv_dtype: str = "bf16", num_samples: int = 1, logprobs=None,
                 num_beams: Optional[int] = None, length_penalty: float = 1.0, num_return_sequences: int = 1,
                 logit_bias=None, allowed_token_ids=None, min_p: Optional[float] = None, min_new_tokens: int = 0,
                 stop=None):
        """nanoGPT's ``generate``: continue the prompts ``idx`` [B, P] by ``max_new_tokens`` tokens; returns the int64
        sequences [B, P + n]. ``temperature == 0`` is greedy; otherwise ``logits / temperature``, optional ``top_k``
        filter, softmax, optional nucleus (``top_p``) filter and ``torch.multinomial`` with ``generator``
        (``generation.sample_next``). With ``eos_token_id`` a finished row keeps emitting it and generation stops once
        every row has finished (n is then smaller). ``P + max_new_tokens > n_positions`` raises ``ValueError``.

        With an integer ``seed`` the tokens are drawn on the device instead (``gpt2mi_sample``; the rule is
        ``generation.sample_reference`` with ``generation.uniform_at(seed, row, position)``: reproducible per row and
        position whatever the batch) and the whole loop is issued from C: without ``eos_token_id`` nothing synchronises
        the host before the return, with it the done flags are read once per 32 tokens. Same output shape and padding.
        ``seed`` together with ``generator``, or ``top_p <= 0``, raises ``ValueError``.

        Prompts of unequal length: ``prompt_lens`` (B ints, ``1 <= prompt_lens[b] <= P``) says that row b's prompt is
        ``idx[b, :prompt_lens[b]]`` and the rest of the row padding; ``idx`` may also be a list of 1-D tensors, which is
        padded here. The result is then ``[B, Pmax + m]`` with ``Pmax = max(prompt_lens)``: row b holds its prompt, its
        m new tokens from column ``prompt_lens[b]`` on, and ``pad_token_id`` (default ``eos_token_id``, else 0) after
        them; m = ``max_new_tokens`` unless every row emitted eos earlier. Both samplers work; with ``seed`` row b's
        tokens are those it gets in an equal-length batch (one position per row: ``gpt2mi_decode_step_ragged``).
        ``Pmax + max_new_tokens > n_positions`` raises ``ValueError``. Without ``prompt_lens`` nothing changes.

        Speculative generation: with ``seed`` and ``draft_tokens=k`` up to k drafted tokens of every row are verified
        per pass over the weights (``DecodeSession.speculate``, ``gpt2mi_decode_extend``) and the result is
        ``torch.equal`` to the call without ``draft_tokens``, for greedy and sampled decoding alike. ``draft_fn(history,
        k) -> tokens`` proposes them (default ``generation.ngram_draft``: what followed the most recent earlier
        occurrence of the sequence's last tokens). Without ``seed``, or with ``B * (k + 1) > 64``, ``ValueError``.

        Penalties, for both samplers, ``prompt_lens`` and ``draft_tokens`` alike (``generation.apply_penalties`` is the
        rule; with ``seed`` it runs inside the sampling kernel, from the token buffer the device loop already keeps):
        ``repetition_penalty`` (HF: a token that occurs in the row's prompt or among its new tokens has its logit
        divided by it, multiplied if negative; 1 off), then ``frequency_penalty`` times the number of times the token
        was generated in this call and ``presence_penalty`` if it was at all are subtracted (the OpenAI / vLLM
        convention: the prompt does not count; 0 off). They move the logits in front of the greedy argmax, temperature,
        ``top_k`` and ``top_p``. A value that is not finite, or ``repetition_penalty <= 0``, raises ``ValueError``.

        Constraints, for both samplers, ``prompt_lens``, ``draft_tokens``, ``num_samples``, ``kv_dtype`` and
        ``logprobs`` alike (``generation.apply_constraints``, ``sample_reference``'s ``min_p`` and
        ``generation.stop_match`` are the rule; with ``seed`` they run inside the sampling kernel and the loop still
        never returns to the host), applied after the penalties in this order: ``logit_bias``, a ``{token: value}``
        dict, a ``[V]`` tensor or a ``[B, V]`` tensor, is added to the logits (-inf bans a token; +inf and NaN raise
        ``ValueError``; a dict or ``[V]`` is one device row every row reads), ``allowed_token_ids=[...]`` being short
        for -inf everywhere else; ``min_new_tokens=n`` keeps ``eos_token_id`` at -inf until a row holds n new tokens;
        then temperature, ``top_k`` and ``top_p`` as ever; ``min_p`` in (0, 1] also drops every token less than
        ``min_p`` times as likely as the most likely one (greedy ignores it); ``stop=[[ids], ...]`` (at most 8
        sequences of at most 16 tokens) ends a row at the token that completes one of them inside its new tokens, once
        it holds ``min_new_tokens``: the stop tokens stay in the output and the row goes on as after eos.
        ``min_new_tokens`` and ``stop`` need an ``eos_token_id``. The log-probabilities stay those of the raw row.

        ``kv_dtype="fp8"`` keeps the key/value cache as OCP e4m3 codes with one power-of-two scale per (layer, K or V,
        sequence, head, position): 68 bytes where bf16 takes 128 (``generation.kv_quantize`` is the rule). Every key and
        value a step attends over is the quantised one, the new token's own included, so everything stated above holds
        as it does with the default ``"bf16"`` (a row's tokens do not depend on its batch, ``draft_tokens`` is exact);
        the prompt's own attention runs unquantised in the trunk. The logits move by about the error of e4m3's 3
        mantissa bits (DESIGN.md "FP8 key/value cache"). Any other string raises ``ValueError``.

        ``num_samples=s`` draws s continuations of every prompt (best-of-n, self-consistency): the result is
        ``[B * s, P + n]``, prompt-major (row ``b * s + j`` is sample j of prompt b), and a row's draw key is its output
        row number. Each distinct prompt is run once (``DecodeSession.refill`` into row ``b * s``) and copied to its
        other rows (``DecodeSession.fork``); the rows of a prompt then form a share group, whose prompt keys and values
        every step reads once for the group (DESIGN.md "Shared prompt cache"). Everything above works with it
        (``draft_tokens`` verifies unshared). Without eos the result equals the continuations ``generate_many`` returns
        for the list in which each prompt appears s times in a row, at ``batch_size = B * s`` with the same ``seed``.
        ``B * s > 64`` raises ``ValueError``; ``num_samples=1`` is the call without it, on the same code path.

        ``logprobs=True`` or an int n in [0, 20] returns the named tuple ``(tokens, logprobs, top_ids, top_logprobs)``
        in place of the tensor (``None``, the default: the tensor, as before). ``tokens`` is that tensor;
        ``logprobs`` (fp32, its shape) holds each generated token's log-probability under the model's own
        distribution, ``log_softmax`` of the logits row before penalties, temperature and filters (the OpenAI
        convention; ``generation.token_logprobs`` is the rule), and 0 in prompt columns, pad columns and after a row's
        eos, so ``out.logprobs.sum(1)`` is the continuation's log-likelihood and
        ``out.logprobs.sum(1).view(B, s).argmax(1)`` the best of ``num_samples=s``. ``top_ids`` (int32) and
        ``top_logprobs`` ``[rows, P + m, n]`` are the n most likely tokens of each such row, descending, equal values
        by index. With ``seed`` the values come out of the sampling kernel, from the row it drew from: a function of
        that logits row alone, so everything above holds for them bit for bit (batch independence, ``draft_tokens``,
        ``num_samples``, ``kv_dtype``); the host sampler takes them from the same rule in float64.

        ``num_beams=W`` (1 <= W <= 20) searches instead of drawing and returns the named tuple ``BeamOutput(tokens
        [B, r, P + m], scores [B, r], cum_logprob [B, r], lengths [B, r])``, per prompt its r =
        ``num_return_sequences`` (default 1, at most W) best beams, best first; a row of ``tokens`` is laid out as
        above, with pad after the beam's first eos. Each prompt is run once and forked to its W rows (the
        ``num_samples`` path: the rows share the prompt's cache), and every token is chosen on the device by
        ``gpt2mi_decode_beam_search``: each row's W most likely tokens under the model's own distribution (the values
        ``logprobs=`` reports), ``generation.beam_select`` (the W best of the up to W * W candidates by cumulative
        fp32 log-probability; equal scores by beam, then by rank within the beam), the move of the generated suffix of
        the cache rows to their new parents, and the step. Nothing is read back in between (with ``eos_token_id`` the
        done flags once per 32 tokens), a prompt's result does not depend on its batch, and ``kv_dtype="fp8"``,
        ``prompt_lens`` and a list of prompts work. ``num_beams=1`` gives the greedy tokens. A finished beam stays in
        the set, emitting eos, and competes on its raw cumulative log-probability; ``length_penalty`` (default 1.0)
        enters only the final ranking, ``score = cum_logprob / max(length, 1) ** length_penalty`` with ``length`` the
        beam's tokens up to and including its first eos (``generation.beam_rank``). This is not HF's hypothesis heap:
        there is no ``early_stopping`` and a finished hypothesis is not scored, with the penalty, at the moment it
        finishes. ``ValueError``, naming the argument: ``num_beams`` outside [1, 20] or above ``vocab_size``,
        ``B * num_beams > 64``, ``num_return_sequences`` outside [1, num_beams], a non-finite ``length_penalty``, and
        any of ``seed``, ``generator``, ``temperature != 1``, ``top_k``, ``top_p``, the penalties, ``draft_tokens``,
        ``num_samples > 1``, ``logprobs`` and the constraints given with ``num_beams``. Not offered: beams in
        ``generate_many``, the per-token log-probabilities of a beam, sampling and diverse beam search, and constraints
        (``logit_bias``, ``min_p``, ``min_new_tokens``, ``stop``) on beams. ``num_beams=None`` (the default) is
        the call without it, on the same code path.

        Always computes in bf16 with fp32 accumulation and the fp32 residual stream (the autocast path), whatever
        the autocast state, with dropout off whatever ``self.training`` is; ``precision == "fp32"`` raises
        ``NotImplementedError``. It does not advance the dropout stream or touch what a later backward needs, so a
        training run with a ``generate`` between two steps is bit-identical to one without, but it may evict the
        engine's training workspace (re-allocated by the next forward) and must not run between a forward and its
        backward. Through ``DistributedDataParallel`` call ``.module.generate``; a ``FullyShardedDataParallel``-wrapped
        model holds only a shard of the parameters and raises ``NotImplementedError``."""
        from .generation import generate
        return generate(self, idx, max_new_tokens, temperature, top_k, generator, eos_token_id, top_p, seed,
                        prompt_lens, pad_token_id, draft_tokens, draft_fn, repetition_penalty, presence_penalty,
                        frequency_penalty, kv_dtype, num_samples, logprobs, num_beams, length_penalty,
                        num_return_sequences, logit_bias, allowed_token_ids, min_p, min_new_tokens, stop)

    def generate_many(self, prompts, max_new_tokens: int, batch_size: int = 32, temperature: float = 1.0,
                      top_k: Optional[int] = None, top_p: Optional[float] = None, seed: int = 0,
                      eos_token_id: Optional[int] = None, generator=None, repetition_penalty: float = 1.0,
                      presence_penalty: float = 0.0, frequency_penalty: float = 0.0, kv_dtype: str = "bf16",
                      logprobs=None, logit_bias=None, allowed_token_ids=None, min_p: Optional[float] = None,
                      min_new_tokens: int = 0, stop=None):
        """Continue any number of 1-D ``prompts`` of any lengths by up to ``max_new_tokens`` tokens each; returns a list
        in input order, each entry the prompt plus its new tokens, cut after the first ``eos_token_id``.

        One ``DecodeSession`` of ``batch_size`` rows serves them all (continuous batching): every prompt enters a row
        through ``DecodeSession.refill``, the device loop runs in chunks of up to 32 tokens, and after each chunk the
        rows that have finished (eos, or ``max_new_tokens``) are harvested and refilled with the next prompt while the
        others go on. Prompt i draws with ``generation.uniform_at(seed, i, position)``.

        Guarantee: prompt i's output is a function of (weights, prompt i, the sampler parameters, seed, i). It does not
        depend on ``batch_size``, on the other prompts or on the order in which they finish (every kernel of the
        decode step forms a row from that row's data alone, in an order that does not depend on the batch; a refill's
        shapes depend on its prompt alone). Device sampler only: ``generator=`` raises ``ValueError``.
        ``max(len) + max_new_tokens > n_positions`` raises ``ValueError``. Training is left untouched as by
        ``generate``. ``repetition_penalty`` / ``presence_penalty`` / ``frequency_penalty`` as for ``generate``: a row's
        history is its own prompt and new tokens, so the guarantee holds with them. ``kv_dtype`` as for ``generate``: a
        row of the fp8 cache is a function of that row's values alone, so the guarantee holds with it too.
        ``logprobs`` as for ``generate``: each entry is then such a tuple for its prompt, cut where its tokens are cut;
        the values are functions of the row's logits, so the guarantee covers them. ``logit_bias`` (a dict or a ``[V]``
        tensor: one row for every prompt), ``allowed_token_ids``, ``min_p``, ``min_new_tokens`` and ``stop`` as for
        ``generate``: functions of the row's own logits, position and tokens, so the guarantee holds with them; an entry
        is cut after the token that completes a stop sequence, as after eos."""
        from .generation import generate_many
        return generate_many(self, prompts, max_new_tokens, batch_size, temperature, top_k, top_p, seed, eos_token_id,
                             generator, repetition_penalty, presence_penalty, frequency_penalty, kv_dtype, logprobs,
                             logit_bias, allowed_token_ids, min_p, min_new_tokens, stop)

    # ---- optimizer (nanoGPT-style name the north star uses) -----------------------------------------
    def configure_optimizers(self, weight_decay: float = 0.1, learning_rate: float = 1e-4,
                             betas=(0.9, 0.95), device_type: Optional[str] = None, eps: float = 1e-8,
                             max_grad_norm: Optional[float] = None):
        """The reference builds ``torch.optim.AdamW(model.parameters(), lr, weight_decay=0.1,
        betas=(0.9, 0.95), fused=True)`` inline (train_gpt2_distributed.py:356-362): ONE param group,
        so decay also hits biases/LayerNorm/embeddings. This returns the same optimizer as one fused
        HIP kernel over the flat arena. ``max_grad_norm``: ``clip_grad_norm_(parameters, max_grad_norm)`` folded
        into ``step()`` (None or inf: off, the reference's clip at inf)."""
        from .optim import FusedAdamW
        return FusedAdamW(self, lr=learning_rate, betas=betas, eps=eps, weight_decay=weight_decay,
                          max_grad_norm=max_grad_norm)


GPT = GPT2  # nanoGPT alias used by the north star
