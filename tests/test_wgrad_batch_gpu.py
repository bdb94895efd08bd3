"""gpt2mi_gemm_wgrad_batch (ABI v24.3) and the deferred weight-gradient mode of the engine on the MI355X.

Kernel: 13 problems mixing the five tile shapes (1, 2, 3, 3 and 4 tiles: one and several row / column tiles, GM groups
that are full and not) over 256 tokens (two K-tile pairs, the shortest pipeline) and 640 (an even count that is no
multiple of four); every C against A.float().t() @ B.float() at the project's wgrad bound (rel_err < 1e-5), writing
and accumulating, with alpha and a device alpha; body problems bitwise against gpt2mi_gemm_wgrad(splits = 1), tail
problems bitwise against gpt2mi_gemm_wgrad_grouped; guard columns after every C; one problem and the maximum count.
Engine: 3 layers at GPT-2 124M widths, B = 4, T = 256 (324 tiles: body and tail both live), deferred against the four
launches at the bounds of test_grouped_weight_gradients_match_the_four_launches."""
import pytest
import torch

pytestmark = pytest.mark.gpu

dev = "cuda"
SHAPES = [(256, 256), (512, 256), (256, 768), (768, 256), (512, 512)]
PROBLEMS = [SHAPES[i % 5] for i in range(13)]
GUARD = 8  # columns after each C row that no kernel may touch
SENTINEL = -77.0


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


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


_cache = {}


def operands(K):
    """Per token count, once: the 13 problems' bf16 operands on the device, their fp32 references A^T B (CPU) and
    the initial C values."""
    if K not in _cache:
        g = torch.Generator().manual_seed(1000 + K)
        ops = []
        for m, n in PROBLEMS:
            A = (torch.randn(K, m, generator=g) * 0.1).to(torch.bfloat16)
            B = torch.randn(K, n, generator=g).to(torch.bfloat16)
            C0 = torch.randn(m, n, generator=g)
            ops.append((A.to(dev), B.to(dev), C0, A.float().t() @ B.float()))
        _cache[K] = ops
    return _cache[K]


def guarded(C0):
    """C0 [m][n] in a [m][n + GUARD] device buffer whose extra columns hold the sentinel."""
    m, n = C0.shape
    buf = torch.full((m, n + GUARD), SENTINEL, device=dev)
    buf[:, :n] = C0.to(dev)
    return buf


def table(count):
    return torch.empty(max(L().gemm_wgrad_batch_scratch(count), 16), dtype=torch.uint8, device=dev)


@pytest.mark.parametrize("K", [256, 640])
@pytest.mark.parametrize("acc,alpha,use_dev", [(False, 1.0, False), (True, 1.0, False), (True, 0.5, False),
                                               (False, 0.5, True)])
def test_batch_vs_fp32_reference_and_guards(K, acc, alpha, use_dev):
    ops = operands(K)
    ad = torch.tensor([0.75], device=dev) if use_dev else None
    scale = alpha * (0.75 if use_dev else 1.0)
    bufs = [guarded(o[2]) for o in ops]
    probs = [(m, n, o[0], m, o[1], n, buf, n + GUARD) for (m, n), o, buf in zip(PROBLEMS, ops, bufs)]
    L().gemm_wgrad_batch(probs, K, accumulate=acc, alpha=alpha, alpha_dev=ad, table=table(len(probs)))
    torch.cuda.synchronize()
    for (m, n), o, buf in zip(PROBLEMS, ops, bufs):
        out = buf.cpu()
        ref = scale * o[3] + (o[2] if acc else 0)
        e = rel_err(out[:, :n], ref)
        print(f"K={K} {m}x{n} acc={acc} alpha={scale}: rel_err {e:.2e}")
        assert e < 1e-5, (m, n, e)
        assert torch.all(out[:, n:] == SENTINEL), (m, n, "guard columns written")


def hand_plan(K):
    # body: the first 8 problems; tail: the last 5 (two grouped launches: 4 + 1) at 2 splits
    return list(range(8)), list(range(8, 13)), 2


def planned(K):
    # _lib.wgrad_batch_plan for a toy device of 10 CUs: 32 tiles = 3 rounds + 2, so a body and a one-problem tail
    return L().wgrad_batch_plan(PROBLEMS, K, cus=10)


@pytest.mark.parametrize("K", [256, 640])
@pytest.mark.parametrize("plan_of", [hand_plan, planned])
@pytest.mark.parametrize("acc", [False, True])
def test_planned_body_and_tail_bits(K, plan_of, acc):
    """The body's outputs bitwise equal to gemm_wgrad(splits = 1) of each problem, the tail's to gemm_wgrad_grouped of
    each problem at the plan's split; every problem formed exactly once; alpha and a device alpha."""
    ops = operands(K)
    body, tail, split = plan_of(K)
    assert sorted(body + tail) == list(range(13)) and body and tail
    ad = torch.tensor([0.75], device=dev)
    ws = torch.empty(split * sum(m * n for m, n in PROBLEMS), device=dev)
    Cs = [o[2].to(dev) for o in ops]
    probs = [(m, n, o[0], m, o[1], n, c) for (m, n), o, c in zip(PROBLEMS, ops, Cs)]
    L().gemm_wgrad_planned(probs, K, (body, tail, split), accumulate=acc, alpha=0.5, alpha_dev=ad, table=table(len(body)),
                           workspace=ws)
    torch.cuda.synchronize()
    for i, ((m, n), o) in enumerate(zip(PROBLEMS, ops)):
        ref = o[2].to(dev)
        if i in body:
            L().gemm_wgrad(m, n, K, o[0], m, o[1], n, ref, n, accumulate=acc, alpha=0.5, alpha_dev=ad, workspace=ws,
                           splits=1)
        else:
            L().gemm_wgrad_grouped([(m, n, o[0], m, o[1], n, ref)], K, accumulate=acc, alpha=0.5, alpha_dev=ad,
                                   workspace=ws, splits=split)
        torch.cuda.synchronize()
        assert torch.equal(Cs[i], ref), (i, m, n, "body" if i in body else "tail", (Cs[i] - ref).abs().max().item())
        e = rel_err(Cs[i].cpu(), 0.375 * o[3] + (o[2] if acc else 0))
        assert e < 1e-5, (i, m, n, e)


def test_count_one_and_maximum():
    """One problem; and gemm_wgrad_batch_max() problems (256 tiles-of-one over shared operands, each its own C with
    its own alpha-free result), all equal to the single-problem launch's bits; one more problem is refused."""
    K = 256
    A, B, C0, ref = operands(K)[0]
    one = torch.empty(256, 256, device=dev)
    L().gemm_wgrad_batch([(256, 256, A, 256, B, 256, one)], K, accumulate=False, table=table(1))
    single = torch.empty(256, 256, device=dev)
    L().gemm_wgrad(256, 256, K, A, 256, B, 256, single, 256, accumulate=False, splits=1)
    torch.cuda.synchronize()
    assert torch.equal(one, single)
    assert rel_err(one.cpu(), ref) < 1e-5
    nmax = L().gemm_wgrad_batch_max()
    assert nmax >= 4 * 36
    out = torch.full((nmax, 256, 256), float("nan"), device=dev)
    probs = [(256, 256, A, 256, B, 256, out[i]) for i in range(nmax)]
    L().gemm_wgrad_batch(probs, K, accumulate=False, table=table(nmax))
    torch.cuda.synchronize()
    assert torch.equal(out, single.expand(nmax, 256, 256))
    with pytest.raises(L().KernelError):
        L().gemm_wgrad_batch(probs + probs[:1], K, accumulate=False, table=table(nmax))
    with pytest.raises(L().KernelError):  # a table scratch that is too small is refused, not overrun
        L().gemm_wgrad_batch(probs, K, accumulate=False, table=table(nmax - 1))


# ---- the engine's deferred mode --------------------------------------------------------------------------------------
WGT = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")


@pytest.fixture(scope="module")
def small_model():
    from gpt_2_distributed_amd.model import GPT2, GPT2Config
    torch.manual_seed(5)
    m = GPT2(GPT2Config(n_layer=3, n_positions=256, resid_pdrop=0.1, attn_pdrop=0.1)).to(dev)
    g = torch.Generator().manual_seed(67)
    t = torch.randint(0, 50257, (8, 257), generator=g).to(dev)
    return m, t[:, :-1].contiguous(), t[:, 1:].contiguous()


def backward(m, x, y, seeds, scale=1.0):
    losses = []
    for (xb, yb), seed in zip(zip(x, y), seeds):
        m.engine().base_seed = seed
        m.engine()._step_seed = 0
        with torch.autocast("cuda", dtype=torch.bfloat16):
            _, loss = m(xb, labels=yb)
        (loss * scale).backward()
        losses.append(loss.item())
    return losses


def compare(m, a, b):
    blocks = {f"transformer.h.{l}.{n}" for l in range(3) for n in WGT}
    for n, sl in m.layout.slots.items():
        e = rel_err(a[sl.offset:sl.offset + sl.numel], b[sl.offset:sl.offset + sl.numel])
        print(f"{n}: {e:.2e}")
        assert e < (1e-5 if n in blocks else 1e-6), (n, e)


def run_mode(m, x, y, seeds, defer, group, scale=1.0):
    eng = m.engine()
    eng.DEFER_WGRADS, eng.GROUP_WGRADS = defer, group
    try:
        m.zero_grad(set_to_none=True)  # lazy: the weight-gradient GEMMs of the first backward write their slots
        losses = backward(m, x, y, seeds, scale)
        torch.cuda.synchronize()
        return losses, eng.grad.clone()
    finally:
        del eng.DEFER_WGRADS, eng.GROUP_WGRADS  # back to the class defaults


def test_engine_plan_has_body_and_tail(small_model):
    m, x, _ = small_model
    eng = m.engine()
    M = 4 * 256
    assert eng._wgrad_mode(torch.bfloat16, M) == "deferred"
    body, tail, split = L().wgrad_batch_plan([(768, 3072), (3072, 768), (768, 768), (2304, 768)] * 3, M)
    assert body and tail and 1 <= split <= 4


def test_deferred_matches_the_four_launches(small_model):
    """One batch (B = 4), dropout 0.1 with fixed seeds: equal loss, block weight gradients within 1e-5, every other
    gradient within 1e-6 (relative norm)."""
    m, x, y = small_model
    la, ga = run_mode(m, [x[:4]], [y[:4]], [11], defer=True, group=True)
    lb, gb = run_mode(m, [x[:4]], [y[:4]], [11], defer=False, group=False)
    assert la == lb
    compare(m, ga, gb)


def test_deferred_accumulates_micro_batches(small_model):
    """Two accumulated micro-batches after a lazy zero_grad: the first deferred launch writes the slots, the second
    accumulates into them."""
    m, x, y = small_model
    xs, ys = [x[:4], x[4:]], [y[:4], y[4:]]
    la, ga = run_mode(m, xs, ys, [21, 22], defer=True, group=True, scale=0.5)
    lb, gb = run_mode(m, xs, ys, [21, 22], defer=False, group=False, scale=0.5)
    assert la == lb
    compare(m, ga, gb)


def test_deferred_then_pairs_on_one_engine(small_model):
    """A training step in the deferred mode (backward + AdamW), then, the weights put back, a backward with deferral
    off on the same engine, against that backward on an engine that never deferred: the same mode on the same weights
    and seeds, so the same loss and gradients within the bounds above (they differ only by fp32 atomic order) unless
    something stale is read from the per-block buffers or the shared scratch."""
    m, x, y = small_model
    state = {k: v.clone() for k, v in m.state_dict().items()}
    lb, gb = run_mode(m, [x[4:]], [y[4:]], [32], defer=False, group=True)
    opt = m.configure_optimizers()
    run_mode(m, [x[:4]], [y[:4]], [31], defer=True, group=True)
    opt.step()
    m.load_state_dict(state)
    la, ga = run_mode(m, [x[4:]], [y[4:]], [32], defer=False, group=True)
    assert la == lb
    compare(m, ga, gb)
