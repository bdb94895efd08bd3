"""Attention kernels (csrc/attention.hip, and the fp32 family of csrc/fp32.hip) on the MI355X at the inputs, shapes
and seeds where they can be wrong without tests/test_kernels_gpu.py noticing: the forward's deferred-max rescale
against a non-empty accumulator, future keys whose exponentials overflow before they are masked, dropout compared
element for element with the oracle's restated mask, workgroups whose last waves hold no query or key, and one
error figure per 32-row block (the work of one wave) instead of one norm over the tensor.

The inputs, the fp64 oracle, the rounding model and the metric are oracle/attn_stress.py; that the inputs reach the
paths they are built for and are well conditioned is asserted on the CPU by tests/test_attn_stress_cpu.py.

Bounds are computed in each test from the oracle alone, never from the kernel's result: for the bf16 kernels
3 x the worst block error of ``attn_stress.bf16_model`` on that input and tensor (the model leaves out the fp32
accumulation order of the MFMAs and the hardware exp2; the global tolerances of test_kernels_gpu.py stand in about
that ratio to the model's global error), for the fp32 kernels 4 x the worst block error of plain fp32 torch on the
CPU. The lse of the bf16 forward gets 2^-8 + 1e-4 per row (each P of the row sum is rounded to bf16, relative error
<= 2^-8 whichever rounding the pack uses, so the sum and its log are off by at most that); the fp32 forward has no
such rounding and gets 1e-4.

Measured on the MI355X (ranges over the cases of each test; ratio = kernel / model on the same case, worst case named):
  test_forward_rescale_paths     bf16 out: model 2.08e-3..2.35e-3, kernel 2.08e-3..2.47e-3, ratio <= 1.09 (spikes T=320);
                                 lse: kernel <= 2.78e-3 (spikes T=1024; the model, which always takes the true row max,
                                 1.41e-3: the stale max leaves P up to 2^8, same relative rounding), bound 4.01e-3
                                 fp32 out: model 2.5e-7..1.3e-6, kernel 5.0e-7..1.0e-6, ratio <= 2.50 (spikes); lse <= 2.7e-6
  test_backward_large_scores     bf16 parity dq: model 2.86e-3..8.38e-3 (stairs), kernel the same to 3 digits, ratio <= 1.07;
                                 dk: model 2.64e-3..4.32e-3, kernel 2.67e-3..4.12e-3, ratio <= 1.13 (step T=320);
                                 dv: model 2.44e-3..3.04e-3, kernel 2.44e-3..3.05e-3, ratio <= 1.04
                                 bf16 reduced dv: model 2.10e-3..3.02e-3, kernel 2.10e-3..3.55e-3, ratio <= 1.32 (spikes T=1024)
                                 fp32 dq / dk / dv: model 2.7e-7..2.9e-6, kernel 5.1e-7..2.1e-6, ratio <= 2.14 / 1.74 / 1.72 (plain)
  test_dropout_same_mask_parity  out ratio <= 1.10, dq <= 1.00, dk <= 1.38 (B=2 T=192 p=0.1 seed 5: kernel 6.27e-3, model
                                 4.55e-3), dv <= 1.04; lse <= 1.34e-3; colsum vs the stored 32-row sums <= 1.4e-9
  test_dropout_mask_exact_*      exact: no count and no kept set differs
Checked against builds with one arithmetic change each: rescaling one query group only, or not the row-sum row, fails the
forward test on step / stairs / spikes (and the old tests of tests/test_kernels_gpu.py pass); a causal multiply-by-mask in
the backward fails on `cliff` alone; the default multiplier for every seed in dK/dV, bh dropped from the forward's mask
index, or dO not pre-scaled in dQ fail the parity and the exact-mask tests.
"""
import pytest
import torch

from oracle import attn_stress as A
from oracle import dropout_ref

pytestmark = pytest.mark.gpu

dev = "cuda"
D = 64
LSE_BOUND = {False: 2.0 ** -8 + 1e-4, True: 1e-4}  # by f32
MARGIN = {False: 3.0, True: 4.0}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_2_distributed_amd import _lib
    _lib.load()
    return _lib


def L():
    from gpt_2_distributed_amd import _lib
    return _lib


def _act(x, f32):
    return (x.float() if f32 else x.to(torch.bfloat16)).contiguous().to(dev)


def _forward(qd, B, T, H, p, seed):
    C = H * D
    out = torch.empty(B * T, C, dtype=qd.dtype, device=dev)
    lse = torch.empty(B * H, T, device=dev)
    L().attn_fwd(qd, out, lse, B, T, H, D, p, seed)
    return out, lse


def _backward(qd, out, lse, dod, B, T, H, p, seed, colsum=None):
    dqkv = torch.empty(B * T, 3 * H * D, dtype=qd.dtype, device=dev)
    delta = torch.empty(B * H, T, device=dev)
    L().attn_bwd(qd, out, dod, lse, delta, dqkv, B, T, H, D, p, seed, colsum=colsum)
    return dqkv


def _run_case(c, f32=False, backward=True):
    """The kernels on a cached attn_stress case -> out / dq / dk / dv [B, H, T, 64] and lse [B, H, T] on the CPU."""
    B, T, H, p, seed = c["B"], c["T"], c["H"], c["p"], c["seed"]
    qd = _act(c["qkv"], f32)
    out, lse = _forward(qd, B, T, H, p, seed)
    got = {"out": A.unmerge(out.cpu().float(), B, T, H), "lse": lse.cpu().view(B, H, T)}
    if backward:
        dqkv = _backward(qd, out, lse, _act(A.merge(c["dO"]), f32), B, T, H, p, seed)
        got["dq"], got["dk"], got["dv"] = A.split(dqkv.cpu().float(), B, T, H)
    torch.cuda.synchronize()
    return got


def _judge(label, c, got, names, f32=False):
    """Print every figure, then assert: block errors within MARGIN x the model's, lse within its absolute bound."""
    bad = []
    for n in names:
        if n == "lse":
            err, bound = float((got[n].double() - c["ref"][n]).abs().max()), LSE_BOUND[f32]
            print(f"EDGE {label} lse: worst |d lse| {err:.3e} (model {c['model_err'][n]:.3e}, bound {bound:.3e})")
        else:
            e = A.block_err(got[n], c["ref"][n])
            err, bound = float(e.max()), MARGIN[f32] * c["model_err"][n]
            print(f"EDGE {label} {n}: kernel {err:.3e} model {c['model_err'][n]:.3e} ratio "
                  f"{err / c['model_err'][n]:.2f} (worst block {tuple(int(i) for i in (e == e.max()).nonzero()[0])})")
        if not err <= bound:  # also true for NaN
            bad.append((n, err, bound))
    assert not bad, f"{label}: (tensor, worst error, bound) {bad}"


def _finite(label, got):
    for n, t in got.items():
        assert bool(torch.isfinite(t).all()), f"{label}: {n} holds NaN or inf"


def _seed(p):
    return A.SEED_HI if p > 0 else A.SEED_LO


# -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,T,H,f32", [(1, 320, 3, False), (1, 1024, 3, False), (1, 320, 3, True)])
@pytest.mark.parametrize("kind", ["step", "stairs", "spikes", "falling"])
def test_forward_rescale_paths(kind, B, T, H, f32, p):
    """The forward against the fp64 oracle per 32-row block, on inputs that rescale a non-empty accumulator (`step`
    once per wave with the early keys still holding 7-12 % of |out|, `stairs` at every tile, `spikes` through the
    wave-wide vote of one row of one query group) or keep P far from 1 without a rescale (`falling`).
    Fails if the kernel is subtly wrong: with the `corr` multiply skipped or applied to one query group only, the
    `step` rows past the step are off by the early keys' share of out (0.07-0.12 against a bound of 0.007); with only
    o[qg][0..3] scaled and not the row-sum row that is read, the normaliser and the lse are off by the same share; on
    `spikes` one row moves the max of its whole group, so a correction applied to the voting row only, or a max moved
    for one row only, shows in its 15 quiet neighbours; a max moved after the exponentials shows on `stairs` at every
    tile. A wave that takes the wrong branch is one block of 32 rows: 1 % of a global norm at T = 1024 and B*H = 3, the
    whole figure here."""
    c = A.case(kind, B, T, H, p, _seed(p), f32=f32)
    got = _run_case(c, f32, backward=False)
    label = f"fwd {'f32' if f32 else 'bf16'} {kind} T={T} p={p}"
    _finite(label, got)
    _judge(label, c, got, ("out", "lse"), f32)


PARITY = ([(kind, 1, T, 3, f32) for kind in ("step", "falling", "plain") for T, f32 in ((320, False), (1024, False), (320, True))]
          + [("stairs", 1, 320, 3, False), ("stairs", 1, 320, 3, True)])
# dq / dk ill-conditioned (the model's own block error is far above 1e-2: test_attn_stress_cpu.py): finite + dv only
REDUCED = [("stairs", 1, 1024, 3, False), ("spikes", 1, 1024, 3, False), ("spikes", 1, 320, 3, False),
           ("cliff", 1, 256, 3, False)]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("kind,B,T,H,f32", PARITY + REDUCED)
def test_backward_large_scores(kind, B, T, H, f32, p):
    """dq, dk, dv against fp64 autograd under the same dropout mask, per 32-row block, with score ranges of tens of
    nats: P recomputed from the saved lse spans 2^-130 .. 1, and on `cliff` (4-7 nats per key) the future keys of every
    diagonal tile lie more than 128 log2 units above the row's lse, so their exp2 is +inf before the causal select.
    Fails if the kernel is subtly wrong: a causal select turned into a multiply by a 0/1 mask gives inf * 0 = NaN in
    dq / dk / dv of `cliff` (the finite check); an lse that is off by the forward's rescale error scales every P of the
    row; a dS or dP - delta formed for a dropped key with the kept-key value shows in the dq / dk blocks at p = 0.1.
    Where dq / dk are ill-conditioned (near-one-hot rows: dP - delta cancels against the bf16 rounding of out) the check
    is every output finite and dv within its bound; dv stays well conditioned on every input."""
    c = A.case(kind, B, T, H, p, _seed(p), f32=f32)
    got = _run_case(c, f32)
    label = f"bwd {'f32' if f32 else 'bf16'} {kind} T={T} p={p}"
    _finite(label, got)
    full = (kind, B, T, H, f32) in PARITY
    _judge(label, c, got, ("dq", "dk", "dv") if full else ("dv",), f32)


@pytest.mark.parametrize("seed", [A.SEED_LO, A.SEED_HI], ids=["seed_lo", "seed_hi"])
@pytest.mark.parametrize("p", [0.1, 0.25])
@pytest.mark.parametrize("B,T,H", [(2, 192, 3), (1, 1024, 3), (3, 256, 5)])
def test_dropout_same_mask_parity(B, T, H, p, seed):
    """out, dq, dk, dv under dropout against the fp64 oracle run with ``dropout_ref.attn_scale``'s restated mask, per
    block, at a partial-workgroup T with B*H = 6, at T = 1024 with bh > 0 (mask index (bh T + q) T + key up to 3 * 2^20)
    and at B*H = 15; with a seed whose high word selects its own second-round multiplier. Fails if the kernel is subtly
    wrong: one of forward / dQ / dK-dV hashing another index, half or multiplier than the others drops other pairs in
    that tensor only (error ~ sqrt(2p), not 3e-3); the dO / (1 - p) or V / (1 - p) pre-scaling applied twice or not at all
    scales dq / dk by 1 / (1 - p). The fused bias-gradient partials must leave dqkv bitwise unchanged and equal the 32-row
    sums of what was stored, here with invalid waves in the last workgroup."""
    c = A.case("plain", B, T, H, p, seed)
    C = H * D
    qd = _act(c["qkv"], False)
    dod = _act(A.merge(c["dO"]), False)
    out, lse = _forward(qd, B, T, H, p, seed)
    d1 = _backward(qd, out, lse, dod, B, T, H, p, seed)
    cs = torch.full((B * T // 32, 3 * C), float("nan"), device=dev)
    d2 = _backward(qd, out, lse, dod, B, T, H, p, seed, colsum=cs)
    torch.cuda.synchronize()
    got = {"out": A.unmerge(out.cpu().float(), B, T, H), "lse": lse.cpu().view(B, H, T)}
    got["dq"], got["dk"], got["dv"] = A.split(d1.cpu().float(), B, T, H)
    label = f"drop B={B} T={T} H={H} p={p} seed={seed:#x}"
    _finite(label, got)
    _judge(label, c, got, ("out", "lse", "dq", "dk", "dv"))
    assert torch.equal(d1, d2), f"{label}: dqkv changes when the bias-gradient partials are requested"
    sums = d1.float().view(B * T // 32, 32, 3 * C).sum(1).double()
    cerr = float((cs.double() - sums).norm() / sums.norm())
    print(f"EDGE {label} colsum: rel err {cerr:.3e}")
    assert cerr < 1e-5, cerr


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("seed", [A.SEED_LO, A.SEED_HI], ids=["seed_lo", "seed_hi"])
def test_dropout_mask_exact_forward(seed, f32):
    """Every keep decision of the forward, exactly: with q = k = 0 each P is 1 / (q + 1), and with v[key] the unit vector
    of key % 64, out[q, d] (q + 1) (1 - p) is the NUMBER of kept keys <= q of residue class d (at most 16 at T = 1024, far
    above bf16 resolution). It must equal the count from the restated mask for every query and class of B*H = 4 heads.
    Fails if one keep decision anywhere is flipped: a wrong half for q & 16, a (q, q ^ 16) pair hashed at the wrong
    query, bh or key offset, the default multiplier used for a seed with a high word."""
    B, T, H, p = 2, 1024, 2, 0.1
    qkv = torch.zeros(B, T, 3, H, D)
    key = torch.arange(T)
    qkv[:, key, 2, :, key % 64] = 1.0
    out, _ = _forward(_act(qkv.view(B * T, 3 * H * D), f32), B, T, H, p, seed)
    torch.cuda.synchronize()
    out = A.unmerge(out.cpu().double(), B, T, H).reshape(B * H, T, D)
    counts = torch.round(out * (key + 1).double()[None, :, None] * (1.0 - p)).long()
    causal = torch.tril(torch.ones(T, T, dtype=torch.bool))
    for bh in range(B * H):  # one head's mask at a time: 2^20 elements
        keep = A.keep_mask(seed, bh, T, p) & causal
        want = keep.view(T, T // 64, 64).sum(1)
        wrong = (counts[bh] != want).nonzero()
        assert wrong.numel() == 0, f"head {bh}: {wrong.shape[0]} (query, class) counts differ, first {wrong[0].tolist()}"


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_dropout_mask_exact_backward(f32):
    """The kept keys of single queries as the dK/dV pass regenerates them: dO one-hot at (q0, column 0) and v = 1 make
    dv[key, 0] = P[q0, key] keep / (1 - p), non-zero exactly on the kept keys <= q0. Eight queries over two launches,
    one per head of B*H = 4 at T = 1024: both values of q & 16, waves 0-3, the first and the last workgroup, bh > 0.
    Fails if the backward's index arithmetic (query-major tiles, 4 queries per lane group) disagrees with the restated
    mask at any of them."""
    B, T, H, p, seed = 2, 1024, 2, 0.1, A.SEED_HI
    C = H * D
    g = torch.Generator().manual_seed(3)
    qkv = (torch.randn(B, T, 3, H, D, generator=g) * 0.1).bfloat16().float()
    qkv[:, :, 2] = 1.0
    qd = _act(qkv.view(B * T, 3 * C), f32)
    out, lse = _forward(qd, B, T, H, p, seed)
    for queries in ((5, 1023, 1000, 83), (1007, 48, 530, 777)):
        dO = torch.zeros(B, H, T, D)
        for bh, q0 in enumerate(queries):
            dO[bh // H, bh % H, q0, 0] = 1.0
        dqkv = _backward(qd, out, lse, _act(A.merge(dO), f32), B, T, H, p, seed)
        torch.cuda.synchronize()
        dv = A.split(dqkv.cpu().float(), B, T, H)[2].reshape(B * H, T, D)
        for bh, q0 in enumerate(queries):
            want = A.keep_mask(seed, bh, T, p, q=q0)[0] & (torch.arange(T) <= q0)
            assert torch.equal(dv[bh, :, 0] != 0, want), f"head {bh}, query {q0}: kept keys differ"


def _guarded(shape, dtype, n_tail=4096):
    """An output buffer: `shape` elements of NaN followed, in the same allocation, by n_tail sentinel elements."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + n_tail,), 3.0, dtype=dtype, device=dev)
    buf[:n] = float("nan")
    return buf[:n].view(shape), buf[n:]


def _nan_tailed(t):
    """t on the device, followed in its allocation by NaN (as test_kernels_gpu._tail)."""
    buf = torch.full((t.numel() + 4096,), float("nan"), dtype=t.dtype, device=dev)
    out = buf[:t.numel()].view(t.shape)
    out.copy_(t)
    return out


@pytest.mark.parametrize("B,H", [(1, 3), (3, 5)])
@pytest.mark.parametrize("T", [192, 320])
def test_partial_workgroups_write_nothing_else(T, B, H):
    """T = 192 / 320: full workgroups of 128 queries (fwd, dQ) or keys (dK/dV) followed by one whose last two waves
    hold nothing; those waves load clamped rows and must store nothing, at B*H = 3 and 15 (heads spread unevenly over the
    XCDs). Every output is NaN-filled and followed by 4096 sentinels in the same allocation, every input by NaN.
    Fails if an invalid wave stores (a sentinel after out / lse / delta / dqkv / colsum changes: rows past B*T land
    there), if a valid row is left unwritten (a NaN remains), or if a NaN past an input reaches an output."""
    C = H * D
    for p in (0.0, 0.1):
        c = A.case("plain", B, T, H)
        qd, dod = _nan_tailed(c["qkv"]), _nan_tailed(A.merge(c["dO"]).bfloat16())
        (out, out_t), (lse, lse_t) = _guarded((B * T, C), torch.bfloat16), _guarded((B * H, T), torch.float32)
        (delta, delta_t), (dqkv, dqkv_t) = _guarded((B * H, T), torch.float32), _guarded((B * T, 3 * C), torch.bfloat16)
        cs, cs_t = _guarded((B * T // 32, 3 * C), torch.float32)
        L().attn_fwd(qd, out, lse, B, T, H, D, p, A.SEED_HI)
        L().attn_bwd(qd, out, dod, lse, delta, dqkv, B, T, H, D, p, A.SEED_HI, colsum=cs)
        torch.cuda.synchronize()
        for name, body, tail in (("out", out, out_t), ("lse", lse, lse_t), ("delta", delta, delta_t),
                                 ("dqkv", dqkv, dqkv_t), ("colsum", cs, cs_t)):
            assert bool((tail == 3.0).all()), f"p={p}: {name}: written past its end"
            assert bool(torch.isfinite(body).all()), f"p={p}: {name}: an element was not written (or is not finite)"


def test_attention_rejects_bad_arguments():
    """T = 96 (not a multiple of 64), head_dim = 32 and the fused bias-gradient partials on the fp32 path are refused
    before any launch, forward and backward, both families. The buffers are sized for the next valid shape (T = 128,
    head_dim 64), so a missing check could not write out of bounds either. Fails if a guard is dropped: the kernels
    would run a shape they index wrongly."""
    KernelError = L().KernelError
    B, H, T = 1, 1, 128
    for dtype in (torch.bfloat16, torch.float32):
        qd = torch.zeros(B * T, 3 * H * D, dtype=dtype, device=dev)
        out, dod, dqkv = torch.zeros(B * T, H * D, dtype=dtype, device=dev), torch.zeros(B * T, H * D, dtype=dtype, device=dev), torch.zeros_like(qd)
        lse, delta = torch.zeros(B * H, T, device=dev), torch.zeros(B * H, T, device=dev)
        for Tb, Db in ((96, 64), (128, 32)):
            with pytest.raises(KernelError):
                L().attn_fwd(qd, out, lse, B, Tb, H, Db)
            with pytest.raises(KernelError):
                L().attn_bwd(qd, out, dod, lse, delta, dqkv, B, Tb, H, Db)
        if dtype == torch.float32:
            with pytest.raises(KernelError):
                L().attn_bwd(qd, out, dod, lse, delta, dqkv, B, T, H, D, colsum=torch.zeros(B * T // 32, 3 * H * D, device=dev))
    torch.cuda.synchronize()
