"""Token log-probabilities on the MI355X: the LP forms of the sampling kernel (gpt2mi_sample_logprobs) against their
executable specification, generation.token_logprobs in float64 on the CPU.

Values: the drawn token's logprob and every top-n logprob are held to 1e-5 + 4 * 2^-23 * max(|l|, |lse|): 1e-5 is the
project's criterion for probs_out (1e-5 relative) carried to the logarithm, the second term covers the three fp32
roundings (the sum's logarithm, M + log S, l - lse) at the magnitude of the operands. top_id is the reference's exactly:
ordering fp32 values is exact. Everything else is bitwise: the LP call's tokens, seq_out, done and probs_out are the
lp = NULL call's, and a row's logprob / top_* bits do not depend on B, the kernel form, the sampler's values, the seed or
the run."""
import functools

import pytest
import torch

from gpt_2_distributed_amd import _lib as K
from gpt_2_distributed_amd.generation import LogprobBuffer, token_logprobs
from tests.test_sampling_gpu import TINY, make_logits, make_model, padded

pytestmark = pytest.mark.gpu

dev = "cuda"
VS = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 50257, 51199, 51200)   # wave, chunk and capacity seams
BS, TOPS = (1, 3, 64), (0, 1, 5, 20)
PEN = dict(repetition=1.3, presence=0.5, frequency=0.2)
FORMS = {"greedy": dict(temperature=0.0, top_k=None, top_p=None),
         "sampled": dict(temperature=0.8, top_k=50, top_p=0.95),
         "greedy_pen": dict(temperature=0.0, top_k=None, top_p=None, **PEN),
         "sampled_pen": dict(temperature=0.8, top_k=50, top_p=0.95, **PEN)}
HIST_T = 16
SENT = -12345.0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def bits(t):
    return t.contiguous().view(torch.int32)


def tolerance(l, lse):
    return 1e-5 + 4 * 2.0 ** -23 * torch.maximum(l.abs(), lse.abs())


@functools.lru_cache(maxsize=None)
def case(B, V):
    """(logits [B, V] on the CPU, the device buffer with ldl > V and NaN / inf padding, log_softmax in float64, the
    reference's 20 first ids): computed once per shape and shared, never modified."""
    lg = make_logits(B, V, seed=1000 * B + V % 997)
    ref = lg.double() - torch.logsumexp(lg.double(), dim=-1, keepdim=True)
    ids = token_logprobs(lg, None, min(20, V))[1]
    return lg, padded(lg, V + 3 + (-V) % 4), ref, ids


def history(B, V):
    g = torch.Generator().manual_seed(B * 7 + V)
    hist = torch.randint(0, V, (B, HIST_T), generator=g)
    pos = [1 + (5 * b) % (HIST_T - 1) for b in range(B)]
    return hist.to(dev), pos


def run(buf, V, form, top_n, lp=True, pos=None, hist=None, seed=3, eos=None, done=None, col=None, ld=None, probs=False,
        seq=None, out=None):
    """One gpt2mi_sample_logprobs call (lp False: with lp = NULL); everything it writes, on the CPU."""
    B = buf.size(0)
    kw = dict(FORMS[form]) if isinstance(form, str) else dict(form)
    if "repetition" in kw:
        kw.update(hist=hist, gen_start=[0] * B)
    tok = torch.full((B,), -7, dtype=torch.int64, device=dev)
    pr = torch.full((B, V), -1.0, device=dev) if probs else None
    ld = ld or (max(col if col is not None else pos) + 1)
    if out is None:
        out = (torch.full((B, ld), SENT, device=dev), torch.full((B, ld, top_n), -5, dtype=torch.int32, device=dev),
               torch.full((B, ld, top_n), SENT, device=dev))
    lpk = dict(logprob=out[0], top_ids=out[1] if top_n else None, top_logprobs=out[2] if top_n else None, col=col)
    K.sample_logprobs(buf, V, kw.pop("temperature"), kw.pop("top_k"), kw.pop("top_p"), seed, pos, tok, eos=eos, done=done,
                      seq_out=seq, probs_out=pr, **(lpk if lp else {}), **kw)
    torch.cuda.synchronize()
    return dict(tok=tok.cpu(), probs=None if pr is None else pr.cpu(), logprob=out[0].cpu(), top_ids=out[1].cpu(),
                top_logprobs=out[2].cpu())


def check_values(got, lg, ref, ids, cols, top_n, done_rows=()):
    """The drawn tokens' values and the alternatives of every row against the float64 rule."""
    B, V = lg.shape
    rows = torch.arange(B)
    lse = torch.logsumexp(lg.double(), dim=-1)
    lp = got["logprob"][rows, torch.tensor(cols)].double()
    tok = got["tok"]
    live = torch.tensor([b not in done_rows for b in range(B)])
    err = (lp - ref[rows, tok]).abs()
    tol = tolerance(lg[rows, tok].double(), lse)
    print(f"  logprob: max err {float(err[live].max()) if live.any() else 0.0:.2e} (tol >= 1e-5)")
    assert bool((err <= tol)[live].all()), (err.max(), tok.tolist())
    if top_n:
        tid = got["top_ids"][rows, torch.tensor(cols)].long()
        assert torch.equal(tid, ids[:, :top_n]), (tid.tolist(), ids[:, :top_n].tolist())
        tl = got["top_logprobs"][rows, torch.tensor(cols)].double()
        want = ref.gather(1, tid)
        l = lg.double().gather(1, tid)
        fin = torch.isfinite(want)
        assert torch.equal(tl[~fin], want[~fin])                           # -inf stays -inf
        assert bool(((tl - want).abs()[fin] <= tolerance(l, lse[:, None].expand_as(l))[fin]).all())


# ---- the values at every seam, batch size, top_n and kernel form -------------------------------------------------------
@pytest.mark.parametrize("V", VS)
def test_values_and_alternatives_match_the_rule(V):
    for B in BS:
        lg, buf, ref, ids = case(B, V)
        before = buf.clone()
        hist, pos = history(B, V)
        seq0 = torch.full((B, HIST_T + 1), -3, dtype=torch.int64, device=dev)
        for form in FORMS:
            seq = seq0.clone()
            plain = run(buf, V, form, 0, lp=False, pos=pos, hist=hist, probs=True, seq=seq)
            plain_seq = seq.cpu()
            keep = {}
            for top_n in sorted({min(n, V) for n in TOPS}):
                seq = seq0.clone()
                got = run(buf, V, form, top_n, pos=pos, hist=hist, probs=top_n == min(5, V), seq=seq)
                print(f"V={V} B={B} {form} top_n={top_n}")
                # the draw is the lp = NULL call's, bit for bit
                assert torch.equal(got["tok"], plain["tok"]) and torch.equal(seq.cpu(), plain_seq)
                if got["probs"] is not None:
                    assert torch.equal(bits(got["probs"]), bits(plain["probs"]))
                check_values(got, lg, ref, ids, pos, top_n)
                if V == 1:
                    assert bool((got["logprob"][torch.arange(B), torch.tensor(pos)] == 0.0).all())
                    if top_n:
                        assert bool((got["top_logprobs"][torch.arange(B), torch.tensor(pos)] == 0.0).all())
                keep[top_n] = got
            # a shorter list is the head of a longer one, bit for bit
            ns = sorted(keep)
            for a, b in zip(ns[1:], ns[2:]):
                at = (torch.arange(B), torch.tensor(pos))
                assert torch.equal(bits(keep[a]["top_logprobs"][at]), bits(keep[b]["top_logprobs"][at][:, :a]))
        assert torch.equal(bits(buf), bits(before))                        # the logits buffer is never written


# ---- edge rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [63, 2049])
def test_edge_rows(V):
    ninf = float("-inf")
    g = torch.Generator().manual_seed(V)
    lg = torch.randn(6, V, generator=g) * 3
    lg[0, ::2], lg[0, 1::2] = 80.0, -80.0                                   # +-80: no overflow, lse = 80 + log(V/2 ..)
    lg[0, 5] = 79.5
    lg[1, torch.randperm(V, generator=g)[:V - 13]] = ninf                   # 13 finite entries: -inf among the top 20
    lg[2, [7, V - 1, 40]] = lg[2].max() + 1                                 # the maximum three times
    srt = lg[3].sort(descending=True).values
    lg[3, [50, 3, 61, 20]] = srt[4]                                         # ties that straddle the 5th place
    lg[4, [9, 2, 33]] = srt[19]                                             # ... and the 20th
    lg[5, 10], lg[5, 11], lg[5, 30] = 0.0, -0.0, 0.0                        # -0 equals +0: by index
    lg[5, (lg[5] > 0)] *= -1                                                # (zeros are the maximum here)
    buf = padded(lg, V + 7)
    ref = lg.double() - torch.logsumexp(lg.double(), dim=-1, keepdim=True)
    pos = [3] * 6
    for top_n in (5, 20):
        ids = token_logprobs(lg, None, top_n)[1]
        assert ids[5, :3].tolist() == [10, 11, 30] and ids[2, :3].tolist() == [7, 40, V - 1]
        for form in ("greedy", "sampled"):
            got = run(buf, V, form, top_n, pos=pos)
            check_values(got, lg, ref, ids, pos, top_n)
    got20 = got["top_logprobs"][1, 3]
    assert bool(torch.isfinite(got20[:13]).all()) and got20[13:].tolist() == [ninf] * 7
    assert got["top_ids"][1, 3, 13:].tolist() == sorted(got["top_ids"][1, 3, 13:].tolist())   # the -inf ones by index


# ---- a row's bits depend on the row alone --------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [65, 2049, 50257])
def test_a_rows_bits_do_not_depend_on_batch_form_sampler_seed_or_run(V):
    lg, buf, ref, ids = case(64, V)
    hist, pos = history(64, V)
    n = min(20, V)
    base = run(buf, V, "greedy", n, pos=pos, hist=hist)
    at = (torch.arange(64), torch.tensor(pos))
    want_lp, want_id = bits(base["top_logprobs"][at]), base["top_ids"][at]
    # greedy without penalties draws the first alternative: its value is that entry's, bit for bit
    assert torch.equal(base["tok"], want_id[:, 0].long())
    assert torch.equal(bits(base["logprob"][at]), want_lp[:, 0])
    variants = [("greedy", {}), ("greedy", {}), ("sampled", {}), ("sampled", dict(seed=99)), ("greedy_pen", {}),
                ("sampled_pen", {}), (dict(temperature=1.7, top_k=None, top_p=None), {}),
                (dict(temperature=0.3, top_k=7, top_p=None), {}), (dict(temperature=1.0, top_k=None, top_p=0.5), {}),
                (dict(temperature=1.0, top_k=min(20, V), top_p=None, **PEN), dict(seed=5))]
    for form, kw in variants:
        got = run(buf, V, form, n, pos=pos, hist=hist, **kw)
        assert torch.equal(bits(got["top_logprobs"][at]), want_lp) and torch.equal(got["top_ids"][at], want_id), form
        # whatever was drawn: where it is one of the alternatives, its value has that alternative's bits
        hit = got["top_ids"][at].long() == got["tok"][:, None]
        rows = hit.any(1)
        assert torch.equal(bits(got["logprob"][at])[rows], want_lp[hit])
        if isinstance(form, dict) and form.get("top_k") and "repetition" not in form:
            assert bool(rows.all())                                         # top-k <= 20: always one of them
    # the same rows alone and in a batch of 3, at other positions and columns
    for b in (0, 37, 63):
        one = run(buf[b:b + 1], V, "sampled", n, pos=[pos[b]], hist=hist[b:b + 1], col=[0], ld=1)
        assert torch.equal(bits(one["top_logprobs"][0, 0]), want_lp[b]) and torch.equal(one["top_ids"][0, 0], want_id[b])
    three = run(buf[[5, 37, 9]].contiguous(), V, "greedy", n, pos=[2, 9, 4], col=[1, 0, 2], ld=3)
    for r, b in enumerate((5, 37, 9)):
        assert torch.equal(bits(three["top_logprobs"][r, (1, 0, 2)[r]]), want_lp[b])
        assert torch.equal(bits(three["logprob"][r, (1, 0, 2)[r]]), want_lp[b, 0])


# ---- done rows, and what a call writes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_a_done_row_writes_eos_and_zero(form):
    V, B = 1025, 5
    lg, buf, ref, ids = case(3, V)
    lg, buf = torch.cat([lg, lg[:2]]), torch.cat([buf, buf[:2]]).contiguous()
    ref, ids = torch.cat([ref, ref[:2]]), torch.cat([ids, ids[:2]])
    hist, pos = history(B, V)
    eos = 17
    flags = torch.tensor([0, 1, 0, 1, 0], dtype=torch.uint8)
    d_lp, d_plain = flags.to(dev), flags.to(dev)
    plain = run(buf, V, form, 0, lp=False, pos=pos, hist=hist, eos=eos, done=d_plain)
    got = run(buf, V, form, 5, pos=pos, hist=hist, eos=eos, done=d_lp)
    assert torch.equal(got["tok"], plain["tok"]) and torch.equal(d_lp, d_plain)
    assert got["tok"][[1, 3]].tolist() == [eos, eos]
    at = (torch.arange(B), torch.tensor(pos))
    assert bits(got["logprob"][at])[[1, 3]].tolist() == [0, 0]             # +0.0
    check_values(got, lg, ref, ids, pos, 5, done_rows=(1, 3))              # the alternatives as for any row
    # a row that draws eos now keeps its value and sets its flag
    tok = int(got["tok"][0])
    d = torch.zeros(B, dtype=torch.uint8, device=dev)
    again = run(buf, V, form, 5, pos=pos, hist=hist, eos=tok, done=d)
    assert int(d[0]) == 1 and torch.equal(bits(again["logprob"][at][0]), bits(got["logprob"][at][0]))


@pytest.mark.parametrize("with_col", [False, True])
def test_writes_exactly_its_outputs(with_col):
    """Sentinel-filled buffers: row b writes logprob[b, c] and top_*[b, c, :top_n] with c = col[b] (pos[b] without col),
    and nothing else; two runs give the same bits."""
    V, B, n, ld = 2049, 3, 5, 12
    lg, buf, ref, ids = case(B, V)
    pos = [4, 11, 0]
    col = [7, 0, 11] if with_col else None
    cols = col or pos
    runs = []
    for _ in range(2):
        out = (torch.full((B, ld), SENT, device=dev), torch.full((B, ld, n), -5, dtype=torch.int32, device=dev),
               torch.full((B, ld, n), SENT, device=dev))
        runs.append(run(buf, V, "sampled", n, pos=pos, col=col, ld=ld, out=out))
    a, b = runs
    for k in ("logprob", "top_ids", "top_logprobs"):
        assert torch.equal(bits(a[k]) if a[k].dtype == torch.float32 else a[k],
                           bits(b[k]) if b[k].dtype == torch.float32 else b[k])
    written = torch.zeros(B, ld, dtype=torch.bool)
    written[torch.arange(B), torch.tensor(cols)] = True
    assert bool((a["logprob"][~written] == SENT).all()) and bool((a["logprob"][written] != SENT).all())
    assert bool((a["top_ids"][~written] == -5).all()) and bool((a["top_logprobs"][~written] == SENT).all())
    assert bool((a["top_ids"][written] >= 0).all()) and bool((a["top_logprobs"][written] != SENT).all())
    check_values(a, lg, ref, ids, cols, n)
    # top_n = 0: the two arrays are not touched (they may be NULL)
    out = run(buf, V, "sampled", 0, pos=pos, col=col, ld=ld)
    assert torch.equal(bits(out["logprob"]), bits(a["logprob"]))


def test_generate_loop_writes_column_pos0_plus_i_on_ragged_rows():
    """gpt2mi_decode_generate_logprobs on a session with ragged positions: step i of row b writes column lens[b] + i of
    the buffer, as of seq, and nothing else; the tokens are those of the loop without."""
    model = make_model()
    V = TINY["vocab_size"]
    S = torch.randint(0, V, (3, 12), generator=torch.Generator().manual_seed(4)).to(dev)
    lens, n, T = [12, 3, 7], 6, 24
    seqs, bufs = [], []
    for lp in (False, True):
        sess = model.decoder(3, T)
        sess.prefill(S, lens)
        seq = torch.full((3, T), -1, dtype=torch.int64, device=dev)
        buf = LogprobBuffer(3, T, 5, dev)
        for t in (buf.logprob, buf.top_logprobs):
            t.fill_(SENT)
        buf.top_ids.fill_(-5)
        sess.generate(n, 0.8, 50, 0.95, 11, seq=seq, **({"logprobs": buf} if lp else {}))
        torch.cuda.synchronize()
        seqs.append(seq.cpu()), bufs.append(buf)
    assert torch.equal(seqs[0], seqs[1])
    buf = bufs[1]
    written = torch.zeros(3, T, dtype=torch.bool)
    for b, m in enumerate(lens):
        written[b, m:m + n] = True
    assert torch.equal(seqs[1] >= 0, written)
    lp, ti, tl = buf.logprob.cpu(), buf.top_ids.cpu(), buf.top_logprobs.cpu()
    assert bool((lp[~written] == SENT).all()) and bool((ti[~written] == -5).all()) and bool((tl[~written] == SENT).all())
    assert bool((lp[written] < 0).all()) and bool((lp[written] > -30).all())
    assert bool((ti[written] >= 0).all()) and bool((ti[written] < V).all())
    assert bool((tl[written][:, :-1] >= tl[written][:, 1:]).all())
    # a drawn token that is one of its alternatives has that alternative's value
    hit = ti[written].long() == seqs[1][written][:, None]
    assert bool(hit.any()) and torch.equal(bits(lp[written][hit.any(1)]), bits(tl[written][hit]))
    assert bufs[0].logprob.eq(SENT).all()                                   # without the keyword nothing is written
