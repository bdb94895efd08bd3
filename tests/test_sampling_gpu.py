"""Device-side sampling on the MI355X: gpt2mi_sample against its executable specification, and the device token loop.

The reference is generation.sample_reference (float64, CPU) fed generation.uniform_at's uniforms. Two kinds of case:

exact   top-k <= 50 (or V = 509): the test first checks on the CPU, in the float64 reference, that every row's u is at
        least 1e-5 from every CDF boundary and no token's exclusive mass is within 1e-5 of top_p (fp32 rounding over
        <= 50 kept terms is ~1e-6), choosing the seed so that this holds. Then every row's token must equal the
        reference's, the support of probs_out must be the reference's kept set and its values agree to 1e-5 relative.
wide    V = 50257 without top-k: boundaries are denser than fp32 resolves, so the kernel's token t is accepted iff
        cdf64[t-1] - delta <= u <= cdf64[t] + delta, delta = 8 x the largest |cumsum_fp32 - cumsum_fp64| of the same
        probabilities under torch.cumsum on the CPU (x 8: the kernel's summation order is not torch's), computed here
        from the test's own inputs and printed (DESIGN.md "Decode" notes the measured value).
seams   u values at which one level of the kernel's chunk / wave / lane CDF finds no crossing, found with a CPU
        restatement of its sums: held to the wide cases' band.
probs_out is e / Z stored from the registers the kernel builds its CDF from."""
import json
import os
import subprocess
import sys

import pytest
import torch

from gpt_2_distributed_amd import _lib as K
from gpt_2_distributed_amd.generation import sample_reference, uniform_at
from tests.conftest import REPO

pytestmark = pytest.mark.gpu

dev = "cuda"
TINY = dict(n_layer=2, n_head=2, n_embd=128, vocab_size=509, n_positions=192, resid_pdrop=0.1, attn_pdrop=0.1)
BS, TEMPS = (1, 3, 64), (0.7, 1.0, 1.5)
MARGIN = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---- helpers -----------------------------------------------------------------------------------------------------------
def make_logits(B, V, seed):
    return torch.randn(B, V, generator=torch.Generator().manual_seed(seed)) * 3


def padded(lg, ldl):
    """The logits in a [B, ldl] device buffer whose padding columns hold NaN (every third row: +inf)."""
    B, V = lg.shape
    buf = torch.full((B, ldl), float("nan"))
    buf[::3, V:] = float("inf")
    buf[:, :V] = lg
    return buf.to(dev)


def device_sample(buf, V, temperature, top_k, top_p, seed, pos, eos=None, done=None, seq=None, want_probs=True):
    B = buf.size(0)
    tok = torch.full((B,), -7, dtype=torch.int64, device=dev)
    probs = torch.full((B, V), -1.0, device=dev) if want_probs else None
    K.sample(buf, V, temperature, top_k, top_p, seed, pos, tok, eos=eos, done=done, seq_out=seq, probs_out=probs)
    torch.cuda.synchronize()
    return tok.cpu(), (probs.cpu() if want_probs else None)


def uniforms(seed, B, pos):
    return torch.tensor([uniform_at(seed, b, pos) for b in range(B)], dtype=torch.float64)


def exclusive_mass(lg, temperature, top_k):
    """float64: (p [B, V] after top-k, the mass of the tokens with a strictly larger value, per token; inf where top-k
    filtered)."""
    x = lg.float() / temperature
    keep = torch.ones_like(x, dtype=torch.bool)
    if top_k is not None and 1 <= top_k < x.size(1):
        keep = x >= torch.topk(x, top_k, dim=-1).values[:, -1:]
    xd = x.double().masked_fill(~keep, float("-inf"))
    p = torch.softmax(xd, dim=-1)
    sx, order = torch.sort(xd, dim=-1, descending=True)
    sp = p.gather(-1, order)
    before = sp.cumsum(-1) - sp
    pos = torch.arange(sx.size(-1)).expand_as(sx)
    new = torch.ones_like(sx, dtype=torch.bool)
    new[:, 1:] = sx[:, 1:] != sx[:, :-1]
    first = torch.where(new, pos, torch.zeros_like(pos)).cummax(-1).values
    excl = torch.zeros_like(before).scatter(-1, order, before.gather(-1, first))
    return p, excl.masked_fill(~keep, float("inf"))


def margins(lg, temperature, top_k, top_p, u):
    """(min over rows of the distance of u from the reference CDF's boundaries, min distance of an exclusive mass from
    top_p), float64 on the CPU."""
    _, probs = sample_reference(lg, temperature, top_k, top_p, u)
    cdf = probs.cumsum(-1)
    cdf = cdf[:, :-1]  # (the last boundary is 1: u < 1 - 2^-24 by construction, checked through the others' margin)
    d = (cdf - u[:, None]).abs() + (probs[:, :-1] == 0) * 1.0  # boundaries of kept tokens only
    d_u = float(d.min()) if d.numel() else float("inf")
    d_p = float("inf")
    if top_p is not None and top_p < 1:
        _, excl = exclusive_mass(lg, temperature, top_k)
        d_p = float((excl - top_p).abs().min())
    return d_u, d_p


def pick_seed(lg, temperature, top_k, top_p, pos):
    for seed in range(40):
        d_u, d_p = margins(lg, temperature, top_k, top_p, uniforms(seed, lg.size(0), pos))
        if d_u >= MARGIN and d_p >= MARGIN:
            return seed, d_u, d_p
    raise AssertionError("no seed in 0..39 keeps every row 1e-5 away from a boundary")


def check_exact(lg, ldl, temperature, top_k, top_p, pos=11):
    B, V = lg.shape
    seed, d_u, d_p = pick_seed(lg, temperature, top_k, top_p, pos)
    want_tok, want_probs = sample_reference(lg, temperature, top_k, top_p, uniforms(seed, B, pos))
    tok, probs = device_sample(padded(lg, ldl), V, temperature, top_k, top_p, seed, pos)
    print(f"V={V} B={B} T={temperature} k={top_k} p={top_p}: seed {seed}, margins u {d_u:.2e} top_p {d_p:.2e}")
    assert torch.equal(tok, want_tok), (tok.tolist(), want_tok.tolist())
    # support: exactly the reference's kept set. fp32 holds no probability below 1.2e-38 (logits 160 apart): where the
    # float64 reference keeps such a token, the kernel's value may have underflowed to 0.
    big = want_probs >= 2e-38
    assert bool((probs[big] > 0).all()) and bool((probs[want_probs == 0] == 0).all())
    assert bool((probs[~big] <= 4e-38).all())
    rel = (probs.double() - want_probs).abs()[big] / want_probs[big]
    assert float(rel.max()) <= 1e-5, float(rel.max())


# ---- exact cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_p", [None, 0.9], ids=["p-off", "p0.9"])
@pytest.mark.parametrize("top_k", [1, 8, 50])
def test_exact_small_vocab(top_k, top_p):
    for B in BS:
        lg = make_logits(B, 509, seed=100 + B)
        for T in TEMPS:
            check_exact(lg, 512 if B != 3 else 509, T, top_k, top_p)  # (an unpadded, 4-byte aligned row stride too)


@pytest.fixture(scope="module")
def gpt2_logits():
    return {B: make_logits(B, 50257, seed=200 + B) for B in BS}


@pytest.mark.parametrize("top_k", [1, 8, 50])
def test_exact_gpt2_vocab(gpt2_logits, top_k):
    for B in BS:
        for T in TEMPS:
            check_exact(gpt2_logits[B], 50432, T, top_k, None)


# ---- wide cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_p", [None, 0.9], ids=["p-off", "p0.9"])
def test_wide_gpt2_vocab(gpt2_logits, top_p):
    V, pos, seed = 50257, 3, 0
    for B in BS:
        lg = gpt2_logits[B]
        buf = padded(lg, 50432)
        for T in TEMPS:
            u = uniforms(seed, B, pos)
            _, want = sample_reference(lg, T, None, top_p, u)
            cdf = want.cumsum(-1)
            delta = 8 * float((want.float().cumsum(-1).double() - cdf).abs().max())
            tok, probs = device_sample(buf, V, T, None, top_p, seed, pos)
            lo = torch.where(tok > 0, cdf.gather(1, (tok - 1).clamp_min(0)[:, None]).squeeze(1), torch.zeros(B).double())
            hi = cdf.gather(1, tok[:, None]).squeeze(1)
            print(f"wide B={B} T={T} p={top_p}: delta {delta:.2e}, worst slack "
                  f"{float(torch.maximum(lo - u, u - hi).max()):.2e}")
            assert bool(((lo - delta <= u) & (u <= hi + delta)).all()), (tok.tolist(), (lo - u).tolist(), (u - hi).tolist())
            assert bool((probs.gather(1, tok[:, None]) > 0).all())  # the token is one the kernel kept
            if top_p is None:
                assert torch.equal(probs > 0, want > 0)
            else:
                _, excl = exclusive_mass(lg, T, None)
                differs = (probs > 0) != (want > 0)
                assert bool(((excl - top_p).abs()[differs] <= delta).all()), int(differs.sum())
            same = (probs > 0) & (want > 0)
            rel = ((probs.double() - want).abs() / want.clamp_min(1e-300))[same & (want > 1e-30)]
            assert float(rel.max()) <= 1e-4  # (values: a loose cross-check; the exact cases hold them to 1e-5)


# ---- draws at the seams of the kernel's three-level CDF -------------------------------------------------------------------
class KernelSums:
    """The fp32 sums of csrc/sample.hip's draw, restated on the CPU for one row of kept exponentials e [V] (float32):
    token c * 1024 + w * 64 + lane; a wave sum is an xor butterfly (32 .. 1), a chunk total its 16 wave sums added from
    0, the chunk level a running sum of the totals, the wave level the wave sums added onto the chunk's base, the lane
    level a Hillis-Steele scan. decide(u) follows the kernel's search and says whether a level found no crossing."""

    def __init__(self, e):
        import numpy as np
        self.np = np
        g = torch.zeros(50 * 1024)
        g[:e.numel()] = e
        self.g = g.view(50, 16, 64)
        lanes = torch.arange(64)
        r = self.g.clone()
        for o in (32, 16, 8, 4, 2, 1):
            r = r + r[..., lanes ^ o]
        self.csum = r[..., 0].numpy().astype(np.float32)          # [chunk][wave]
        ctot = np.zeros(50, np.float32)
        for k in range(16):
            ctot = ctot + self.csum[:, k]
        self.ctot = ctot
        z = np.float32(0)
        for c in range(50):
            z = np.float32(z + ctot[c])
        self.Z = z

    def boundaries(self):
        """Every chunk's and wave's upper boundary as the kernel's levels form them, as fractions of Z."""
        np = self.np
        out, run = [], np.float32(0)
        for c in range(50):
            r = run
            for k in range(16):
                r = np.float32(r + self.csum[c, k])
                out.append(float(r) / float(self.Z))
            run = np.float32(run + self.ctot[c])
            out.append(float(run) / float(self.Z))
        return out

    def decide(self, u_bits):
        """(the level that found no crossing, or None; the token the kernel's rule gives) for u = u_bits / 2^24."""
        np = self.np
        t = np.float32(np.float32(u_bits * 2.0 ** -24) * self.Z)
        run, c = np.float32(0), -1
        for i in range(50):
            nr = np.float32(run + self.ctot[i])
            if nr > t:
                c, base = i, run
                break
            run = nr
        if c < 0:
            return "chunk", None
        run, ws = base, -1
        for k in range(16):
            nr = np.float32(run + self.csum[c, k])
            if nr > t:
                ws, base = k, run
                break
            run = nr
        if ws < 0:
            k = max(k for k in range(16) if self.csum[c, k] > 0)
            return "wave", c * 1024 + k * 64 + int(self.g[c, k].nonzero().max())
        ec = self.g[c, ws]
        inc = ec.clone()
        for o in (1, 2, 4, 8, 16, 32):
            nxt = inc.clone()
            nxt[o:] = inc[o:] + inc[:-o]
            inc = nxt
        hit = ((ec > 0) & ((inc + float(base)).float() > float(t))).nonzero()  # (fp32 add of base, as the kernel's)
        if hit.numel() == 0:
            return "lane", c * 1024 + ws * 64 + int(ec.nonzero().max())
        return None, c * 1024 + ws * 64 + int(hit.min())


def seeds_drawing(targets, pos, n=1 << 22):
    """[(seed, u_bits)] for the seeds < n whose draw for row 0 at `pos` is one of the 24-bit values in `targets`."""
    import numpy as np
    c = np.arange(n, dtype=np.uint64) + np.uint64((0x9E3779B97F4A7C15 * (1 + pos)) % 2 ** 64)
    c ^= c >> np.uint64(30)
    c *= np.uint64(0xBF58476D1CE4E5B9)
    c ^= c >> np.uint64(27)
    c *= np.uint64(0x94D049BB133111EB)
    c ^= c >> np.uint64(31)
    bits = c >> np.uint64(40)
    idx = np.nonzero(np.isin(bits, np.array(sorted(targets), dtype=np.uint64)))[0]
    return [(int(i), int(bits[i])) for i in idx]


@pytest.mark.parametrize("T", [0.8, 1.5])
def test_draws_at_chunk_and_wave_seams_stay_on_the_cdf(gpt2_logits, T):
    """The kernel's chunk, wave and lane levels add the same terms in different orders, so for u * Z within rounding of a
    chunk's or wave's upper boundary a lower level finds no crossing. It must then stay in that chunk and wave (its last
    token with mass), not jump elsewhere: the token obeys the wide cases' band like any other. The u values where that
    happens are found with a CPU restatement of the kernel's sums, and seeds whose hash draws them by search."""
    V = 50257
    lg = gpt2_logits[1]
    x = lg.to(dev) / T
    sums = KernelSums(torch.exp(x - x.max()).cpu()[0])  # fp32 on the device: the kernel's operations on the same values
    cands = {int(f * 2 ** 24) + d for f in sums.boundaries() for d in range(-3, 4)}
    seams = {}
    for ub in sorted(cands):
        if 0 <= ub < 2 ** 24:
            level, tok = sums.decide(ub)
            if level in ("wave", "lane"):
                seams[ub] = (level, tok)
    print(f"T={T}: {len(seams)} of 2^24 u values have a level without a crossing: {sorted(seams.items())[:6]} ...")
    assert seams, "the restated sums show no seam: they no longer restate the kernel"
    draws = []
    for pos in range(8):
        draws += [(seed, pos, ub) for seed, ub in seeds_drawing(seams, pos)]
        if len(draws) >= 6:
            break
    assert draws, "no seed below 2^22 at positions 0..7 draws a seam value"
    _, want = sample_reference(lg, T, None, None, torch.zeros(1))
    cdf = want.cumsum(-1)[0]
    delta = 8 * float((want.float().cumsum(-1).double() - want.cumsum(-1)).abs().max())
    buf = padded(lg, 50432)
    for seed, pos, ub in draws[:6]:
        assert uniform_at(seed, 0, pos) == ub / 2 ** 24
        tok, _ = device_sample(buf, V, T, None, None, seed, pos, want_probs=False)
        t, u = int(tok[0]), ub / 2 ** 24
        lo, hi = (float(cdf[t - 1]) if t else 0.0), float(cdf[t])
        print(f"  seed {seed} pos {pos} u {u:.8f} ({seams[ub][0]} level): token {t} (restated {seams[ub][1]}), "
              f"cdf [{lo:.8f}, {hi:.8f}], delta {delta:.2e}")
        assert lo - delta <= u <= hi + delta, (seed, pos, t, lo, u, hi, delta)


# ---- edges -------------------------------------------------------------------------------------------------------------
def test_rows_with_minus_inf_and_large_logits():
    lg = make_logits(3, 509, seed=7)
    lg[0, ::2] = float("-inf")
    lg[1, :] = float("-inf")
    lg[1, [5, 77, 300]] = torch.tensor([1.0, 2.0, 1.5])
    lg[2, 10], lg[2, 400], lg[2, 401] = 80.0, -80.0, 79.0  # +-80: exp(x - max) must not overflow
    for top_k, top_p in ((None, None), (8, None), (None, 0.9), (600, None)):  # (top_k >= V: off)
        check_exact(lg, 512, 1.0, top_k, top_p)
    tok, probs = device_sample(padded(lg, 512), 509, 1.0, None, None, 0, 0)
    assert bool(torch.isfinite(probs).all()) and bool((probs[0, ::2] == 0).all())
    assert set(probs[1].nonzero().flatten().tolist()) == {5, 77, 300}


def test_ties_at_the_kth_value_are_all_kept():
    lg = make_logits(2, 509, seed=8)
    order = lg[0].argsort(descending=True)
    lg[0, order[7]] = lg[0, order[8]] = lg[0, order[9]] = lg[0, order[6]]  # ranks 7..10 equal: top-8 keeps 10
    _, probs = device_sample(padded(lg, 512), 509, 0.7, 8, None, 0, 0)
    assert sorted(probs[0].nonzero().flatten().tolist()) == sorted(order[:10].tolist())
    assert int((probs[1] > 0).sum()) == 8
    check_exact(lg, 512, 0.7, 8, None)
    check_exact(lg, 512, 0.7, 8, 0.9)


def test_greedy_picks_the_lowest_index_of_a_duplicated_maximum():
    lg = make_logits(3, 50257, seed=9)
    top = float(lg.max()) + 1
    lg[0, 40000], lg[0, 1234], lg[0, 1235] = top, top, top
    lg[1, 50256] = top
    lg[2, 0], lg[2, 50256] = top, top
    tok, probs = device_sample(padded(lg, 50432), 50257, 0.0, 5, 0.5, 3, 2)
    assert tok.tolist() == [1234, 50256, 0]
    assert torch.equal(tok, sample_reference(lg, 0.0, None, None, uniforms(0, 3, 0))[0])
    assert torch.equal(probs, torch.zeros(3, 50257).scatter_(1, tok[:, None], 1.0))


@pytest.mark.parametrize("V", [1, 63, 64, 65, 1023, 1024, 1025, 2049, 51199, 51200])
def test_chunk_and_capacity_boundaries(V):
    """The kernel's width is a 1024-token chunk (and a 64-lane wave inside it); its capacity 51200."""
    lg = make_logits(3, V, seed=300 + V % 97)
    lg[0, V - 1] = float(lg.max()) + 4   # mass on the last valid token
    lg[1, (V - 1) // 1024 * 1024] = float(lg.max()) + 4  # and on the first of the last chunk
    ldl = V + 3
    for top_k, top_p in ((None, None), (50, None), (50, 0.9)):
        if top_k is None and V > 1100:
            continue  # (dense boundaries: the wide cases)
        check_exact(lg, ldl, 1.0, top_k, top_p)
    tok, _ = device_sample(padded(lg, ldl), V, 0.0, None, None, 0, 0, want_probs=False)
    assert tok.tolist() == lg.argmax(-1).tolist()


def test_eos_and_done_flags():
    lg = make_logits(4, 509, seed=10)
    buf = padded(lg, 512)
    greedy = lg.argmax(-1)
    eos = int(greedy[2])
    done = torch.tensor([0, 1, 0, 0], dtype=torch.uint8, device=dev)
    tok, _ = device_sample(buf, 509, 0.0, None, None, 0, 4, eos=eos, done=done, want_probs=False)
    want = greedy.clone()
    want[1] = eos                                   # a done row emits eos whatever its logits say
    assert tok.tolist() == want.tolist()
    assert done.cpu().tolist() == [0, 1, 1, int(greedy[3]) == eos]  # row 2 drew eos: its flag is set
    # without done nothing is forced
    tok, _ = device_sample(buf, 509, 0.0, None, None, 0, 4, eos=eos, want_probs=False)
    assert tok.tolist() == greedy.tolist()


def test_writes_exactly_its_outputs():
    B, V, L, pos = 5, 509, 9, 6
    buf = padded(make_logits(B, V, seed=11), 512)
    tok_store = torch.full((B + 4,), -99, dtype=torch.int64, device=dev)
    seq_store = torch.full((B + 2, L), -99, dtype=torch.int64, device=dev)
    probs_store = torch.full((B + 2, V), -5.0, device=dev)
    K.sample(buf, V, 0.9, 8, 0.9, 1, pos, tok_store[2:2 + B], seq_out=seq_store[1:1 + B], probs_out=probs_store[1:1 + B])
    torch.cuda.synchronize()
    tok = tok_store.cpu()
    assert tok[:2].tolist() == [-99, -99] and tok[2 + B:].tolist() == [-99, -99]
    assert bool(((tok[2:2 + B] >= 0) & (tok[2:2 + B] < V)).all())
    seq = seq_store.cpu()
    assert seq[1:1 + B, pos].tolist() == tok[2:2 + B].tolist()
    seq[1:1 + B, pos] = -99
    assert bool((seq == -99).all())
    probs = probs_store.cpu()
    assert bool((probs[0] == -5).all()) and bool((probs[-1] == -5).all()) and bool((probs[1:1 + B] >= 0).all())
    assert bool(torch.isnan(buf[:, V:]).logical_or(torch.isinf(buf[:, V:])).all())  # the padding is as it was


@pytest.mark.parametrize("V,ldl,top_k,top_p", [(509, 512, 8, 0.9), (50257, 50432, None, 0.9), (50257, 50432, 50, None)])
def test_two_runs_are_bit_identical(V, ldl, top_k, top_p):
    buf = padded(make_logits(5, V, seed=12), ldl)
    a = device_sample(buf, V, 0.8, top_k, top_p, 4, 9)
    b = device_sample(buf, V, 0.8, top_k, top_p, 4, 9)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # and a row's draw does not depend on the batch it is in
    one = device_sample(buf[:1], V, 0.8, top_k, top_p, 4, 9)
    assert torch.equal(one[0], a[0][:1]) and torch.equal(one[1], a[1][:1])


# ---- frequencies -------------------------------------------------------------------------------------------------------
def test_draw_frequencies_follow_the_kept_distribution():
    """One row, top_k = 8, drawn at 64 rows x 64 positions: every kept token's count within 5 sigma of N p."""
    row = make_logits(1, 509, seed=13)
    lg = row.repeat(64, 1)
    buf = padded(lg, 512)
    _, probs = sample_reference(row, 1.0, 8, None, torch.tensor([0.5]))
    p = probs[0]
    N = 64 * 64
    tol = 5 * (N * p * (1 - p)).sqrt()
    ref_counts, dev_counts = torch.zeros(509), torch.zeros(509)
    tok = torch.empty(64, dtype=torch.int64, device=dev)
    for pos in range(64):
        ref_counts += torch.bincount(sample_reference(lg, 1.0, 8, None, uniforms(21, 64, pos))[0], minlength=509)
        K.sample(buf, 509, 1.0, 8, None, 21, pos, tok)
        dev_counts += torch.bincount(tok.cpu(), minlength=509)
    assert int((p > 0).sum()) == 8
    assert bool(((ref_counts - N * p).abs() <= tol).all()), (ref_counts[p > 0], N * p[p > 0])  # the reference itself
    assert bool(((dev_counts - N * p).abs() <= tol).all()), (dev_counts[p > 0], N * p[p > 0])
    assert dev_counts.sum() == N and bool((dev_counts[p == 0] == 0).all())


# ---- the device loop ---------------------------------------------------------------------------------------------------
def make_model(cfg=TINY):
    from gpt_2_distributed_amd.model import GPT2, GPT2Config
    return GPT2(GPT2Config(**cfg)).to(dev)


@pytest.fixture(scope="module")
def tiny():
    model = make_model()
    S = torch.randint(0, TINY["vocab_size"], (3, 150), generator=torch.Generator().manual_seed(17)).to(dev)
    return model, S[:, :5].contiguous()


def test_device_greedy_equals_the_host_loop(tiny):
    model, prompt = tiny
    want = model.generate(prompt, 40, temperature=0.0)
    got = model.generate(prompt, 40, temperature=0.0, seed=0)
    assert got.shape == (3, 45) and got.dtype == torch.int64 and torch.equal(got, want)
    assert model.training


def test_device_sampling_is_reproducible_and_batch_independent(tiny):
    model, prompt = tiny
    kw = dict(temperature=0.8, top_k=50, top_p=0.9, seed=7)
    a = model.generate(prompt, 40, **kw)
    assert torch.equal(a, model.generate(prompt, 40, **kw))
    assert torch.equal(a[:, :5], prompt) and int(a.min()) >= 0 and int(a.max()) < TINY["vocab_size"]
    assert not torch.equal(a, model.generate(prompt, 40, **dict(kw, seed=8)))
    assert torch.equal(model.generate(prompt[:1], 40, **kw), a[:1])  # row 0 alone: the same tokens


def test_device_loop_equals_a_manual_loop_with_the_reference(tiny):
    """prefill + (sample_reference on the session's logits + step) per token, with the exact-case margins checked on the
    CPU copy of every step's logits; the seed is the first for which they hold at every step."""
    model, prompt = tiny
    n, T, k, p = 16, 0.8, 50, 0.9
    P = prompt.size(1)
    for seed in range(20):
        sess = model.decoder(3, P + n)
        logits = sess.prefill(prompt)
        toks, ok = [], True
        for i in range(n):
            lg = logits.cpu()
            u = uniforms(seed, 3, P + i)
            d_u, d_p = margins(lg, T, k, p, u)
            if d_u < MARGIN or d_p < MARGIN:
                ok = False
                break
            nxt = sample_reference(lg, T, k, p, u)[0].to(dev)
            toks.append(nxt)
            if i + 1 < n:
                logits = sess.step(nxt)
        if ok:
            break
    assert ok, "no seed in 0..19 keeps every step 1e-5 away from a boundary"
    want = torch.cat([prompt, torch.stack(toks, dim=1)], dim=1)
    got = model.generate(prompt, n, temperature=T, top_k=k, top_p=p, seed=seed)
    assert torch.equal(got, want), (seed, got.tolist(), want.tolist())
    # the session interface gives the same tokens: sample() + step(), and generate() in two calls
    sess = model.decoder(3, P + n)
    sess.prefill(prompt)
    first = sess.sample(T, k, p, seed)
    assert torch.equal(first, want[:, P])
    sess.step(first)
    seq = torch.zeros(3, P + n, dtype=torch.int64, device=dev)
    sess.generate(6, T, k, p, seed, seq=seq)
    sess.generate(n - 7, T, k, p, seed, seq=seq)
    assert torch.equal(seq[:, P + 1:], want[:, P + 1:]) and sess.pos == P + n - 1


def test_device_eos_matches_the_host_loop(tiny):
    model, prompt = tiny
    greedy = model.generate(prompt, 40, temperature=0.0)
    for eos in {int(greedy[0, 5]), int(greedy[1, 20]), int(greedy[2, 39])}:
        want = model.generate(prompt, 40, temperature=0.0, eos_token_id=eos)
        got = model.generate(prompt, 40, temperature=0.0, eos_token_id=eos, seed=0)
        assert got.shape == want.shape and torch.equal(got, want), eos
    one = model.generate(prompt[:1], 12, temperature=0.0, eos_token_id=int(greedy[0, 5]), seed=0)
    assert one.shape == (1, 6) and int(one[0, 5]) == int(greedy[0, 5])
    # without eos_token_id no flag exists: the full length comes back even where a row repeats a token
    assert model.generate(prompt, 40, temperature=0.0, seed=0).shape == (3, 45)
    with pytest.raises(ValueError, match="eos_token_id"):
        model.generate(prompt, 4, seed=0, eos_token_id=TINY["vocab_size"])


def _train_step(model, opt, batch):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        _, loss = model(batch[:, :-1], labels=batch[:, 1:])
    loss.backward()
    opt.step()
    opt.zero_grad()
    return loss.detach().clone()


def test_device_generation_between_steps_leaves_training_bit_identical():
    batches = torch.randint(0, 509, (2, 2, 65), generator=torch.Generator().manual_seed(3)).to(dev)
    prompt = batches[0, :, :5].contiguous()
    runs = []
    for with_generate in (False, True):
        model = make_model()
        opt = model.configure_optimizers(learning_rate=1e-2)
        _train_step(model, opt, batches[0])
        if with_generate:
            seed, token = model.engine()._step_seed, model.engine()._fwd_token
            model.generate(prompt, 20, temperature=1.0, top_k=10, top_p=0.9, seed=1)
            model.generate(prompt, 20, temperature=0.0, seed=1, eos_token_id=3)
            assert (model.engine()._step_seed, model.engine()._fwd_token) == (seed, token)
            assert model.training
        loss = _train_step(model, opt, batches[1])
        runs.append((loss, model.transformer.h[0].attn.qkv.weight.detach().clone(), model.engine()._step_seed))
    (l0, w0, s0), (l1, w1, s1) = runs
    assert torch.equal(l0, l1) and torch.equal(w0, w1) and s0 == s1


def test_cli_device_sampler(tmp_path):
    from gpt_2_distributed_amd.train_gpt2_distributed import save_checkpoint
    model = make_model()
    ckpt = save_checkpoint(model, model.configure_optimizers(), 3, str(tmp_path))
    cmd = [sys.executable, "-m", "gpt_2_distributed_amd.generate", "--checkpoint", ckpt, "--model", "auto",
           "--prompt_ids", "11,12,13", "--max_new_tokens", "9", "--batch", "2", "--temperature", "0.8", "--seed", "5",
           "--sampler", "device", "--top_p", "0.9"]
    out = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("[")]
    assert len(rows) == 2
    idx = torch.tensor([[11, 12, 13]] * 2, device=dev)
    want = model.generate(idx, 9, temperature=0.8, top_p=0.9, seed=5).tolist()
    for row, w in zip(rows, want):
        assert len(row) == 12 and row[:3] == [11, 12, 13]
        assert all(isinstance(t, int) and 0 <= t < TINY["vocab_size"] for t in row)
        assert row == w  # (seed, row, position) decide the draw: the CLI's process gives this one's tokens
