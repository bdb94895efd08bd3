"""The beam-search kernels on the MI355X (csrc/beam.hip): gpt2mi_beam_select against generation.beam_select and
gpt2mi_beam_reorder against torch indexing on copies, both bit for bit, with everything around what they may write
compared against the input."""
import numpy as np
import pytest
import torch

from gpt_2_distributed_amd import _lib as K
from gpt_2_distributed_amd.generation import beam_select

pytestmark = pytest.mark.gpu

dev = "cuda"
PAD = 4  # sentinel elements on either side of every output buffer
EOS = 7
VOCAB = 60


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---- select -----------------------------------------------------------------------------------------------------------
def top_rows(rng, n, W, with_eos):
    """n rows of W (id, logprob) pairs in the sampler's order: logprobs descending, distinct ids; eos among them or not."""
    ids = np.stack([rng.permutation([t for t in range(VOCAB) if t != EOS])[:W] for _ in range(n)]).astype(np.int32)
    lps = -np.sort(rng.uniform(0.05, 6.0, size=(n, W)).astype(np.float32), axis=1)
    if with_eos:
        for r in range(n):
            ids[r, rng.integers(W)] = EOS
    return ids, lps


def group_state(kind, rng, W):
    """One group's (cum, done, ids, lps), built to reach a branch of the rule."""
    ids, lps = top_rows(rng, W, W, with_eos=kind in ("eos_inside", "done"))
    cum = -rng.uniform(0.5, 30.0, size=W).astype(np.float32)
    done = np.zeros(W, np.uint8)
    if kind == "first_step":  # forks of one prefill: identical rows, only beam 0 may expand
        ids[:], lps[:] = ids[0], lps[0]
        cum[:] = -np.inf
        cum[0] = 0.0
    elif kind == "tie_across" and W > 1:  # two beams with identical rows and identical cum, the best of the group
        cum[0] = np.float32(-0.25)
        ids[W - 1], lps[W - 1], cum[W - 1] = ids[0], lps[0], cum[0]
    elif kind == "tie_within" and W > 1:  # the two best one ulp apart under a large |cum|: one score
        cum[0] = np.float32(-4096.0)
        cum[1:] = np.float32(-5000.0) - np.arange(W - 1, dtype=np.float32)
        lps[0, 1] = np.nextafter(lps[0, 0], np.float32(-10.0))
        assert lps[0, 0] != lps[0, 1] and cum[0] + lps[0, 0] == cum[0] + lps[0, 1]
        lps[0] = -np.sort(-lps[0])
    elif kind == "done":  # finished beams among live ones, one of them the best
        done[::2] = 1
        cum[0] = np.float32(-0.01)
    return cum, done, ids, lps


KINDS = ("random", "first_step", "tie_across", "tie_within", "done", "eos_inside")


@pytest.mark.parametrize("G, W", [(1, 1), (1, 2), (3, 5), (8, 8), (3, 20), (1, 20)])
def test_select_equals_the_rule(G, W):
    R = G * W
    rng = np.random.default_rng(100 * G + W)
    sent = dict(tok=-77, parent=-78, cum=-12345.0, done=0xAB)
    for variant in range(len(KINDS)):
        parts = [group_state(KINDS[(g + variant) % len(KINDS)], rng, W) for g in range(G)]
        cum, done, ids, lps = (np.concatenate([p[i] for p in parts]) for i in range(4))
        for eos in (-1, EOS):
            want = beam_select(cum, done, ids, lps, eos, W)
            d = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
            out = dict(tok=torch.full((R + 2 * PAD,), sent["tok"], dtype=torch.int64, device=dev),
                       parent=torch.full((R + 2 * PAD,), sent["parent"], dtype=torch.int32, device=dev),
                       cum=torch.full((R + 2 * PAD,), sent["cum"], dtype=torch.float32, device=dev),
                       done=torch.full((R + 2 * PAD,), sent["done"], dtype=torch.uint8, device=dev))
            K.beam_select(d(ids), d(lps), d(cum), d(done), G, W, eos, *(out[n][PAD:PAD + R] for n in
                                                                        ("tok", "parent", "cum", "done")))
            where = f"G={G} W={W} variant={variant} eos={eos}"
            for name, ref in zip(("tok", "parent", "cum", "done"), want):
                got = out[name].cpu()
                assert bool((got[:PAD] == sent[name]).all()) and bool((got[PAD + R:] == sent[name]).all()), (where, name)
                got = got[PAD:PAD + R].numpy()
                assert got.tobytes() == ref.tobytes(), (where, name, got, ref)
            # in place: the state buffers as their own outputs
            cum_d, done_d = d(cum), d(done)
            tok2, par2 = torch.empty(R, dtype=torch.int64, device=dev), torch.empty(R, dtype=torch.int32, device=dev)
            K.beam_select(d(ids), d(lps), cum_d, done_d, G, W, eos, tok2, par2, cum_d, done_d)
            assert cum_d.cpu().numpy().tobytes() == want[2].tobytes() and done_d.cpu().numpy().tobytes() == want[3].tobytes()
            assert tok2.cpu().numpy().tobytes() == want[0].tobytes() and par2.cpu().numpy().tobytes() == want[1].tobytes()


def test_select_scenarios_reach_the_ties():
    """The tie inputs do what they are built for: the rule's result on them differs from a rule that breaks ties by
    token id, so a kernel with the wrong tie order fails the comparison above."""
    rng = np.random.default_rng(5)
    cum, done, ids, lps = group_state("tie_within", rng, 5)
    ids[0, 0], ids[0, 1] = 50, 2  # the lower rank holds the larger id
    tok = beam_select(cum, done, ids, lps, -1, 5)[0]
    assert tok[0] == 50 and tok[1] == 2
    cum, done, ids, lps = group_state("tie_across", rng, 5)
    parent = beam_select(cum, done, ids, lps, -1, 5)[1].tolist()
    s = np.float32(cum[0] + lps[0, 0])
    first = [j for j in range(5) if np.float32(cum[j] + lps[j, 0]) == s]
    assert first[:2] == [0, 4] and parent.index(0) < parent.index(4)


# ---- reorder ----------------------------------------------------------------------------------------------------------
L, H, TCAP = 2, 3, 96
WINDOWS = [(5, 70), (33, 34), (40, 40)]
MAPS = {  # name: (B, G, W, parent)
    "identity": (4, 1, 4, [0, 1, 2, 3]),
    "swap": (4, 1, 4, [1, 0, 2, 3]),
    "cycle3": (4, 1, 4, [1, 2, 0, 3]),
    "one_parent": (4, 1, 4, [2, 2, 2, 2]),
    "two_groups": (12, 2, 4, [1, 0, 3, 2, 6, 6, 4, 5]),  # rows 8 .. 11: a group left out of the call
}


def make_cache(B, fp8, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (L, B, H, TCAP, 64)
    if fp8:
        kc, vc = (torch.randint(0, 256, shape, dtype=torch.uint8, generator=g) for _ in range(2))
        ks, vs = (torch.randn(L, B, H, TCAP, generator=g) for _ in range(2))
        return [t.to(dev) for t in (kc, vc, ks, vs)]
    kc, vc = (torch.randint(-32768, 32767, shape, dtype=torch.int16, generator=g).view(torch.bfloat16) for _ in range(2))
    return [kc.to(dev), vc.to(dev), None, None]


def raw(t):
    return t if t.dtype in (torch.uint8, torch.int64) else t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: f"{w[0]}-{w[1]}")
@pytest.mark.parametrize("name", sorted(MAPS))
def test_reorder_equals_index_select(name, window, fp8):
    B, G, W, parent = MAPS[name]
    R = G * W
    other = WINDOWS[0] if window == WINDOWS[1] else WINDOWS[1]
    lo = [window[0]] * W + [other[0]] * (R - W)
    hi = [window[1]] * W + [other[1]] * (R - W)
    tensors = make_cache(B, fp8, seed=17 + len(name))
    seq = torch.randint(0, 50000, (B, TCAP), generator=torch.Generator().manual_seed(3)).to(dev)
    before = [None if t is None else t.clone() for t in tensors + [seq]]
    want = [None if t is None else t.clone() for t in before]
    par_t = torch.tensor(parent, device=dev)
    for t, src in zip(want, before):
        if t is None:
            continue
        for g in range(G):  # positions [lo, hi) of the group's rows from their parents' rows of the untouched copy
            rows, a, b = slice(g * W, g * W + W), lo[g * W], hi[g * W]
            dim = 0 if t is want[-1] else 1
            picked = src.index_select(dim, par_t[rows])
            if dim == 0:
                t[rows, a:b] = picked[:, a:b]
            else:
                t[:, rows, :, a:b] = picked[:, :, :, a:b]
    nbytes = K.beam_reorder_workspace(K.KV_FP8 if fp8 else K.KV_BF16, L, H, R, max(h - l for l, h in zip(lo, hi)))
    ws = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device=dev)
    K.beam_reorder(tensors[0], tensors[1], par_t.to(torch.int32), G, W, lo, hi, ws[:nbytes], seq=seq,
                   kscale=tensors[2], vscale=tensors[3])
    for what, got, ref, src in zip(("kcache", "vcache", "kscale", "vscale", "seq"), tensors + [seq], want, before):
        if got is None:
            continue
        assert torch.equal(raw(got), raw(ref)), (name, window, what)
        if name == "identity" or window[0] == window[1] and R == W:
            assert torch.equal(raw(got), raw(src)), (name, window, what, "nothing may be written")
    assert bool((ws[nbytes:] == 0x5A).all())  # the staging buffer ends where the query says
    if name != "identity" and window == WINDOWS[0]:  # the case does move something
        assert not torch.equal(raw(tensors[0]), raw(before[0])) and not torch.equal(seq, before[-1])
