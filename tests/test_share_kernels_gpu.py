"""gpt2mi_attn_decode_shared / _fp8 on the MI355X: a shared read of a prompt's keys and values gives the bits of the
unshared kernel.

Every case builds random caches in which the members of a group are identical below shared_len and different above
it, runs gpt2mi_attn_decode_ragged (or its fp8 sibling) on one copy and the shared entry on another, and compares `out`
and the caches with torch.equal: the shared wave does attn_row's arithmetic per (row, range), so no tolerance is needed.
The poison cases are the bandwidth claim in testable form: the shared part of every member but the lowest is never read."""
import pytest
import torch

from gpt_2_distributed_amd import _lib as K
from gpt_2_distributed_amd.generation import kv_quantize

pytestmark = pytest.mark.gpu

dev = "cuda"
FORMATS = ("bf16", "fp8")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def groups_of(B, group, length):
    return {g: [b for b in range(B) if group[b] == g] for g in set(group) if length[g] > 0}


def make_case(fp8, B, H, Tcap, group, length, seed):
    """qkv [B, 3C] and the caches [B, H, Tcap, 64] (bf16, or codes + scales): random, then every member of a group
    made a copy of its lowest row below the group's shared length."""
    gen = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, 3 * H * 64, generator=gen).to(torch.bfloat16).to(dev)
    kc = torch.randn(B, H, Tcap, 64, generator=gen).to(torch.bfloat16)
    vc = torch.randn(B, H, Tcap, 64, generator=gen).to(torch.bfloat16)
    if fp8:  # rows of different magnitudes, so that the scales differ from key to key
        mag = torch.exp2(torch.randint(-3, 4, (2, B, H, Tcap, 1), generator=gen).float())
        (kc, ks), (vc, vs) = kv_quantize(kc.float() * mag[0]), kv_quantize(vc.float() * mag[1])
        case = dict(kc=kc, vc=vc, ks=ks, vs=vs)
    else:
        case = dict(kc=kc, vc=vc)
    for g, rows in groups_of(B, group, length).items():
        for t in case.values():
            t[rows, :, :length[g]] = t[g, :, :length[g]]
    return qkv, {n: t.to(dev).contiguous() for n, t in case.items()}


def run(fp8, qkv, cache, B, H, Tcap, pos, group=None, length=None, shared=True):
    """out [B, C] and the caches after the call, on clones; shared = False: the v23 entry."""
    c = {n: t.clone() for n, t in cache.items()}
    out = torch.full((B, H * 64), float("nan"), dtype=torch.bfloat16, device=dev)
    ws = torch.full((K.attn_decode_workspace(B, H, Tcap),), float("nan"), dtype=torch.float32, device=dev)
    if shared:
        K.attn_decode_shared(qkv, c["kc"], c["vc"], out, ws, B, H, 64, Tcap, pos, group, length,
                             kscale=c.get("ks"), vscale=c.get("vs"))
    elif fp8:
        K.attn_decode_fp8_ragged(qkv, c["kc"], c["vc"], c["ks"], c["vs"], out, ws, B, H, 64, Tcap, pos)
    else:
        K.attn_decode_ragged(qkv, c["kc"], c["vc"], out, ws, B, H, 64, Tcap, pos)
    torch.cuda.synchronize()
    return out, c


def poison(fp8, cache, rows, lo, hi):
    """NaN at positions [lo[b], hi[b]) of the rows (bf16 values, or the fp8 scales) of a copy of the caches."""
    c = {n: t.clone() for n, t in cache.items()}
    for b in rows:
        for n in (("ks", "vs") if fp8 else ("kc", "vc")):
            c[n][b, :, lo[b]:hi[b]] = float("nan")
    return c


def same(a, b):
    return all(torch.equal(a[n].view(torch.uint8) if a[n].dtype != torch.float32 else a[n].view(torch.int32),
                           b[n].view(torch.uint8) if b[n].dtype != torch.float32 else b[n].view(torch.int32)) for n in a)


def check(fp8, B, H, Tcap, pos, group, length, seed=0):
    qkv, cache = make_case(fp8, B, H, Tcap, group, length, seed)
    ref, ref_c = run(fp8, qkv, cache, B, H, Tcap, pos, shared=False)
    out, out_c = run(fp8, qkv, cache, B, H, Tcap, pos, group, length)
    assert bool(torch.isfinite(ref.float()).all())
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    assert same(out_c, ref_c)
    # the cache holds the new key and value at pos for every row and is otherwise untouched
    C = H * 64
    for b in range(B):
        before = {n: t[b].clone() for n, t in cache.items()}
        k, v = (qkv[b, C:2 * C].view(H, 64), qkv[b, 2 * C:].view(H, 64))
        if fp8:
            (kq, ksc), (vq, vsc) = kv_quantize(k), kv_quantize(v)
            new = dict(kc=kq, vc=vq, ks=ksc, vs=vsc)
        else:
            new = dict(kc=k, vc=v)
        for n in before:
            before[n][:, pos[b]] = new[n]
        assert same({n: t[b] for n, t in out_c.items()}, before), b
    # poison: the shared ranges of every member but the lowest, and everything above each row's position
    members = [b for rows in groups_of(B, group, length).values() for b in rows[1:]]
    full = [32 * (length[b] // 32) for b in range(B)]
    bad = poison(fp8, cache, members, [0] * B, full)
    bad = poison(fp8, bad, range(B), [p + 1 for p in pos], [Tcap] * B)
    got, _ = run(fp8, qkv, bad, B, H, Tcap, pos, group, length)
    assert bool(torch.isfinite(got.float()).all())
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    return ref


# B = 5, rows {0, 2, 3} one group, rows 1 and 4 alone (H = 2, Tcap = 160)
GROUP5 = [0, 1, 0, 0, 4]
LENGTHS = (70, 64, 32, 31)  # two full ranges and a straddling one; exact multiples; nothing shareable


def positions(n):
    return sorted({n, 95, 96, 130})  # the first step after a fork; a range boundary above the shared part; 130


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n", LENGTHS)
def test_group_of_three_among_five(fmt, n):
    length = [n if GROUP5[b] == 0 else 0 for b in range(5)]
    for p in positions(n):
        pos = [p, max(p - 7, 0), p, p, 3]  # the rows alone sit elsewhere
        check(fmt == "fp8", 5, 2, 160, pos, GROUP5, length, seed=n + p)
    # members at different positions above the shared part
    check(fmt == "fp8", 5, 2, 160, [n, 140, 96, 131, 0], GROUP5, length, seed=n)


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_poison_bites_without_the_map(fmt):
    """The poison test proves something: the unshared entry on the poisoned cache does read those lines."""
    fp8 = fmt == "fp8"
    length = [70, 0, 70, 70, 0]
    pos = [100] * 5
    qkv, cache = make_case(fp8, 5, 2, 160, GROUP5, length, 1)
    bad = poison(fp8, cache, [2, 3], [0] * 5, [64] * 5)
    out, _ = run(fp8, qkv, bad, 5, 2, 160, pos, shared=False)
    assert not bool(torch.isfinite(out[[2, 3]].float()).any()) and bool(torch.isfinite(out[[0, 1, 4]].float()).all())
    out, _ = run(fp8, qkv, bad, 5, 2, 160, pos, None, None)  # the shared entry without a map is the unshared one
    assert not bool(torch.isfinite(out[[2, 3]].float()).any())


@pytest.mark.parametrize("fmt", FORMATS)
def test_two_groups_with_different_lengths(fmt):
    group, length = [0, 1, 0, 1, 1, 5], [40, 96, 40, 96, 96, 0]
    for pos in ([40, 96, 41, 97, 130, 17], [130] * 6):
        check(fmt == "fp8", 6, 2, 160, pos, group, length, seed=pos[0])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("members", [64, 37])
def test_more_members_than_a_chunk(fmt, members):
    """B = 64, H = 1, Tcap = 96: one group of 64, and one of 37 (no multiple of a chunk size) whose members are every
    row but the 27 odd ones from 11 on; the rest are alone."""
    B = 64
    alone = set(range(11, 64, 2)[:B - members])
    group = [b if b in alone else 0 for b in range(B)]
    length = [0 if b in alone else 64 for b in range(B)]
    assert sum(g == 0 for g in group) == members
    pos = [64 + (b % 3) * 15 if b not in alone else 5 + b for b in range(B)]
    check(fmt == "fp8", B, 1, 96, pos, group, length, seed=members)
