#!/usr/bin/env python
"""A/B of library builds (same C ABI) on the GPT-2 124M weight-gradient shapes (K = 65536 tokens): every
library in argv is loaded side by side with ctypes, outputs are compared bitwise against the first, and
the wgrad GEMM (gpt2mi_gemm_wgrad, the split-K choice of _lib.wgrad_splits) is timed in interleaved rounds.

    python tools/lib_ab.py libA.so libB.so ...
"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpt_2_distributed_amd import _lib as K  # noqa: E402
from gpt_2_distributed_amd.generation import kv_quantize  # noqa: E402

dev = "cuda"


def bind(path, _n=[0]):
    # a private copy per argument, so the same library can be listed twice with different settings
    import shutil
    import tempfile
    _n[0] += 1
    cp = os.path.join(tempfile.mkdtemp(), f"lib{_n[0]}.so")
    shutil.copy(path, cp)
    lib = ctypes.CDLL(cp)
    for name, args in K._SIGS.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = K._RESTYPES.get(name, ctypes.c_int)
    return lib


def _sched(lib):
    return getattr(lib, "sched", 0)


def main():
    libs = [bind(p) for p in sys.argv[1:]]
    # LIB_AB_IMPLS=0,2: the GEMM sched argument per library (the same .so may be listed twice; low bytes 0, 1, 2, 6)
    impls = [int(v) for v in os.environ.get("LIB_AB_IMPLS", "").split(",") if v]
    for lib, impl in zip(libs, impls):
        lib.sched = impl
    if os.environ.get("LIB_AB_OP") == "decode":
        return decode_mode(libs, torch.cuda.current_stream().cuda_stream)
    Mt, C, Vp = 65536, 768, 50432
    shapes = {"lm_head wgrad": (Vp, C), "qkv wgrad": (3 * C, C), "fc1 wgrad": (4 * C, C), "fc2 wgrad": (C, 4 * C),
              "proj wgrad": (C, C)}
    g = torch.Generator(device=dev).manual_seed(0)
    st = torch.cuda.current_stream().cuda_stream
    data = {}
    for name, (m, n) in shapes.items():
        A = (torch.randn(Mt, m, device=dev, generator=g) * 0.1).to(torch.bfloat16)
        B = (torch.randn(Mt, n, device=dev, generator=g)).to(torch.bfloat16)
        sp = K.wgrad_splits(m, n, Mt)
        ws = torch.empty(max(sp * m * n, 4), device=dev)
        data[name] = (m, n, A, B, sp, ws)
    if os.environ.get("LIB_AB_OP") == "gemm":
        return gemm_mode(libs, g, st)
    if os.environ.get("LIB_AB_OP") == "attn":
        return attn_mode(libs, g, st)
    if os.environ.get("LIB_AB_OP") == "adamw":
        return adamw_mode(libs, g, st)
    if os.environ.get("LIB_AB_OP") == "xent":
        return xent_mode(libs, g, st)
    if os.environ.get("LIB_AB_OP") == "embed":
        return embed_mode(libs, g, st)
    outs = {}
    for i, lib in enumerate(libs):
        for name, (m, n, A, B, sp, ws) in data.items():
            Cm = torch.zeros(m, n, device=dev)
            rc = lib.gpt2mi_gemm_wgrad(m, n, Mt, A.data_ptr(), m, B.data_ptr(), n, Cm.data_ptr(), n, 0, 1.0, None,
                                       ws.data_ptr(), ws.numel(), sp, _sched(lib), st)
            assert rc == 0, (i, name, rc)
            outs[(i, name)] = Cm
    torch.cuda.synchronize()
    for name in shapes:
        for i in range(1, len(libs)):
            if not torch.equal(outs[(0, name)], outs[(i, name)]):
                d = (outs[(0, name)] - outs[(i, name)]).abs().max().item()
                print(f"MISMATCH lib{i} {name}: max diff {d}")
    times = {k: [] for k in outs}
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    for _ in range(5):
        for name, (m, n, A, B, sp, ws) in data.items():
            for i, lib in enumerate(libs):
                Cm = outs[(i, name)]
                fn = lambda: lib.gpt2mi_gemm_wgrad(m, n, Mt, A.data_ptr(), m, B.data_ptr(), n, Cm.data_ptr(), n, 1,  # noqa
                                                   1.0, None, ws.data_ptr(), ws.numel(), sp, _sched(lib), st)
                fn()
                s, e = ev(), ev()
                s.record()
                for _r in range(5):
                    fn()
                e.record()
                torch.cuda.synchronize()
                times[(i, name)].append(s.elapsed_time(e) / 5)
    for name, (m, n, *_r) in data.items():
        line = f"{name:14s}"
        for i in range(len(libs)):
            t = sorted(times[(i, name)])[2]
            line += f"  lib{i}: {t * 1e3:8.1f} us {2 * m * n * Mt / t / 1e9:6.0f} TF"
        print(line, flush=True)


def gemm_mode(libs, g, st):
    """LIB_AB_OP=gemm: forward / dgrad layouts (gpt2mi_gemm, BF16 epilogue) on the lm_head and K=768 shapes."""
    Mt, C, Vp = 65536, 768, 50432
    # name: (layout, N, K, epilogue); the fused-epilogue shapes run as in the step (bias, p = 0.1)
    shapes = {"lm_head fwd": (0, Vp, C, K.EPI_BF16), "lm_head dgrad": (1, C, Vp, K.EPI_BF16),
              "qkv fwd": (0, 3 * C, C, K.EPI_BF16), "fc1 dgrad": (1, C, 4 * C, K.EPI_BF16),
              "fc1 gelu": (0, 4 * C, C, K.EPI_GELU), "fc2dg gelubwd": (0, 4 * C, C, K.EPI_GELU_BWD),
              "proj resid": (0, C, C, K.EPI_RESID), "fc2 resid": (0, C, 4 * C, K.EPI_RESID),
              # the fc1 shape with cheaper epilogues: prices the GELU math and the dropout hash of "fc1 gelu"
              "fc1shape bf16": (0, 4 * C, C, K.EPI_BF16), "fc1shape gelu nodrop": (0, 4 * C, C, K.EPI_GELU)}
    if os.environ.get("GEMM_AB_SHAPES"):
        shapes = {k: v for k, v in shapes.items() if any(t in k for t in os.environ["GEMM_AB_SHAPES"].split(","))}
    data = {}
    for name, (lay, n, k, epi) in shapes.items():
        A = (torch.randn(Mt, k, device=dev, generator=g) * 0.1).to(torch.bfloat16)
        B = (torch.randn(n, k, device=dev, generator=g) if lay == 0 else
             torch.randn(k, n, device=dev, generator=g)).to(torch.bfloat16)
        out = torch.empty(Mt, n, dtype=torch.float32 if epi == K.EPI_RESID else torch.bfloat16, device=dev)
        bias = torch.randn(n, device=dev, generator=g) if epi != K.EPI_BF16 else None
        resid = torch.randn(Mt, n, device=dev, generator=g) if epi == K.EPI_RESID else None
        aux = torch.randn(Mt, n, device=dev, generator=g).to(torch.bfloat16) if epi in (K.EPI_GELU, K.EPI_GELU_BWD) else None
        data[name] = (lay, n, k, A, B, out, epi, bias, resid, aux)
    # outputs of every library vs the first: C bitwise, the fused bias grad (atomics: any order) to 1e-5
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    for name, (lay, n, k, A, B, out, epi, bias, resid, aux) in data.items():
        ref = None
        for i, lib in enumerate(libs):
            o = torch.empty_like(out)
            db = torch.zeros(n, device=dev) if epi == K.EPI_GELU_BWD else None
            pd = 0.1 if epi in (K.EPI_GELU, K.EPI_RESID) and "nodrop" not in name else 0.0
            a2 = aux.clone() if aux is not None else None
            assert lib.gpt2mi_gemm(lay, epi, Mt, n, k, A.data_ptr(), k, B.data_ptr(), k if lay == 0 else n, o.data_ptr(),
                                   n, ptr(bias), ptr(resid), ptr(a2), n if aux is not None else 0, 1.0, None, 0, 1, pd,
                                   5, ptr(db), _sched(lib), st) == 0
            torch.cuda.synchronize()
            if ref is None:
                ref = (o, a2, db)
                continue
            if not torch.equal(o, ref[0]) or (a2 is not None and not torch.equal(a2, ref[1])):
                print(f"MISMATCH lib{i} {name}", flush=True)
            if db is not None and not torch.allclose(db, ref[2], rtol=1e-4, atol=1e-4 * ref[2].abs().max().item()):
                print(f"MISMATCH lib{i} {name} dbias: {(db - ref[2]).abs().max().item()}", flush=True)
    times = {(i, n): [] for i in range(len(libs)) for n in shapes}
    # LIB_AB_STAGGER="0;8000;6000,4": GPT2MI_PP_STAGGER per library ("<ns>[,<groups>]", read per call)
    stag = [v for v in os.environ.get("LIB_AB_STAGGER", "").split(";") if v]
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    dbs = {name: torch.zeros(v[1], device=dev) for name, v in data.items() if v[6] == K.EPI_GELU_BWD}
    # LIB_AB_HOG=<blocks>: every timed batch runs beside tools/ab/libhog.so's CU hog (that many CUs held for 3 ms on a
    # side stream, as RCCL kernels hold them in a data-parallel step)
    hog_blocks = int(os.environ.get("LIB_AB_HOG", "0"))
    if hog_blocks:
        hog = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ab", "libhog.so"))
        hog.hog.argtypes = [ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p]
        side = torch.cuda.Stream()
    for _ in range(5):
        for name, (lay, n, k, A, B, out, epi, bias, resid, aux) in data.items():
            ldb = k if lay == 0 else n
            pd = 0.1 if epi in (K.EPI_GELU, K.EPI_RESID) and "nodrop" not in name else 0.0
            for i, lib in enumerate(libs):
                if stag:
                    os.environ["GPT2MI_PP_STAGGER"] = stag[i]
                fn = lambda: lib.gpt2mi_gemm(lay, epi, Mt, n, k, A.data_ptr(), k, B.data_ptr(), ldb,  # noqa: E731
                                             out.data_ptr(), n, ptr(bias), ptr(resid), ptr(aux), n if aux is not None else 0,
                                             1.0, None, 0, 1, pd, 5, ptr(dbs.get(name)), _sched(lib), st)
                assert fn() == 0
                s, e = ev(), ev()
                if hog_blocks:
                    torch.cuda.synchronize()
                    assert hog.hog(hog_blocks, 3_000_000, side.cuda_stream) == 0
                s.record()
                for _r in range(5):
                    fn()
                e.record()
                torch.cuda.synchronize()
                times[(i, name)].append(s.elapsed_time(e) / 5)
    for name, (lay, n, k, *_r) in data.items():
        line = f"{name:15s}"
        for i in range(len(libs)):
            t = sorted(times[(i, name)])[2]
            line += f"  lib{i}: {t * 1e3:8.1f} us {2 * n * k * Mt / t / 1e9:6.0f} TF"
        print(line, flush=True)


def attn_mode(libs, g, st):
    """LIB_AB_OP=attn: attention forward / backward at cfg 2 (B=64, T=1024, H=12, D=64, dropout 0.1); outputs
    compared bitwise against the first library."""
    B, T, H, D = 64, 1024, 12, 64
    C = H * D
    pd = float(os.environ.get("LIB_AB_PDROP", "0.1"))
    qkv = (torch.randn(B * T, 3 * C, device=dev, generator=g) * 0.5).to(torch.bfloat16)
    dout = (torch.randn(B * T, C, device=dev, generator=g) * 0.1).to(torch.bfloat16)
    res = []
    for lib in libs:
        out = torch.empty(B * T, C, dtype=torch.bfloat16, device=dev)
        lse = torch.empty(B * H * T, device=dev)
        delta = torch.empty(B * H * T, device=dev)
        dqkv = torch.empty(B * T, 3 * C, dtype=torch.bfloat16, device=dev)
        res.append((out, lse, delta, dqkv))
    fwd = lambda lib, r: lib.gpt2mi_attn_fwd(qkv.data_ptr(), r[0].data_ptr(), r[1].data_ptr(), B, T, H, D, pd,  # noqa
                                              7, st)
    bwd = lambda lib, r: lib.gpt2mi_attn_bwd(qkv.data_ptr(), r[0].data_ptr(), dout.data_ptr(), r[1].data_ptr(),  # noqa
                                              r[2].data_ptr(), r[3].data_ptr(), None, B, T, H, D, pd, 7, st)
    for lib, r in zip(libs, res):
        assert fwd(lib, r) == 0 and bwd(lib, r) == 0
    torch.cuda.synchronize()
    for i in range(1, len(libs)):
        for k, name in enumerate(("out", "lse", "delta", "dqkv")):
            if not torch.equal(res[0][k], res[i][k]):
                print(f"MISMATCH lib{i} {name}")
    times = {(i, n): [] for i in range(len(libs)) for n in ("fwd", "bwd")}
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    for _ in range(5):
        for i, (lib, r) in enumerate(zip(libs, res)):
            for n, fn in (("fwd", fwd), ("bwd", bwd)):
                s, e = ev(), ev()
                s.record()
                for _r in range(10):
                    fn(lib, r)
                e.record()
                torch.cuda.synchronize()
                times[(i, n)].append(s.elapsed_time(e) / 10)
    for n in ("fwd", "bwd"):
        line = f"attn {n:10s}"
        for i in range(len(libs)):
            line += f"  lib{i}: {sorted(times[(i, n)])[2] * 1e3:8.1f} us"
        print(line, flush=True)



def adamw_mode(libs, g, st):
    """LIB_AB_OP=adamw: the fused AdamW over the 124M arena (with the bf16 shadow and the grad-norm partials);
    parameters / moments / shadow compared bitwise against the first library after one step."""
    n = 124_475_904
    p0 = torch.randn(n, device=dev, generator=g)
    gr = torch.randn(n, device=dev, generator=g) * 1e-3
    res = []
    for lib in libs:
        p, m, v = p0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        pb = torch.empty(n, dtype=torch.bfloat16, device=dev)
        part = torch.empty(4096, device=dev)
        gn = torch.empty(1, device=dev)
        res.append((p, m, v, pb, part, gn))
    step = lambda lib, r: lib.gpt2mi_adamw(r[0].data_ptr(), gr.data_ptr(), r[1].data_ptr(), r[2].data_ptr(),  # noqa
                                           r[3].data_ptr(), n, 1e-4, 0.1, 0.9, 0.95, 1e-8, 1, 1.0, r[4].data_ptr(),
                                           r[5].data_ptr(), st)
    for lib, r in zip(libs, res):
        assert step(lib, r) == 0
    torch.cuda.synchronize()
    for i in range(1, len(libs)):
        for k, name in enumerate(("p", "m", "v", "shadow")):
            if not torch.equal(res[0][k], res[i][k]):
                print(f"MISMATCH lib{i} {name}")
        print(f"grad norm lib0 {res[0][5].item():.7g} lib{i} {res[i][5].item():.7g}")
    times = {i: [] for i in range(len(libs))}
    for _ in range(5):
        for i, (lib, r) in enumerate(zip(libs, res)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _r in range(5):
                step(lib, r)
            e.record()
            torch.cuda.synchronize()
            times[i].append(s.elapsed_time(e) / 5)
    print("adamw " + "  ".join(f"lib{i}: {sorted(t)[2] * 1e3:8.1f} us" for i, t in times.items()), flush=True)


def xent_mode(libs, g, st):
    """LIB_AB_OP=xent: the register-resident cross-entropy (loss rows, lse, bf16 dlogits) at cfg 2's head
    (65536 rows of 50257 logits, row stride 50304); outputs compared bitwise against the first library."""
    M, V, ld = 65536, 50257, 50304
    logits = (torch.randn(M, ld, device=dev, generator=g) * 2).to(torch.bfloat16)
    labels = torch.randint(0, V, (M,), device=dev, generator=g)
    labels[::97] = -100
    res = []
    for lib in libs:
        res.append((torch.empty(M, device=dev), torch.empty(M, device=dev), torch.empty_like(logits),
                    torch.empty(1, device=dev), torch.empty(1, device=dev)))
    run = lambda lib, r: lib.gpt2mi_xent_fwd(logits.data_ptr(), ld, labels.data_ptr(), r[0].data_ptr(),  # noqa
                                             r[1].data_ptr(), r[2].data_ptr(), ld, M, V, -100, r[3].data_ptr(),
                                             r[4].data_ptr(), st)
    for lib, r in zip(libs, res):
        assert run(lib, r) == 0
    torch.cuda.synchronize()
    for i in range(1, len(libs)):
        for k, name in enumerate(("loss_rows", "lse", "dlogits", "loss")):
            if not torch.equal(res[0][k], res[i][k]):
                print(f"MISMATCH lib{i} {name}")
    times = {i: [] for i in range(len(libs))}
    for _ in range(5):
        for i, (lib, r) in enumerate(zip(libs, res)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _r in range(5):
                run(lib, r)
            e.record()
            torch.cuda.synchronize()
            times[i].append(s.elapsed_time(e) / 5)
    gb = 2 * 2 * M * ld / 1e9
    print("xent " + "  ".join(f"lib{i}: {sorted(t)[2] * 1e3:8.1f} us {gb / sorted(t)[2]:5.2f} TB/s"
                              for i, t in times.items()), flush=True)


def decode_mode(libs, st):
    """LIB_AB_OP=decode: the decode entries with a scalar position (gpt2mi_attn_decode, gpt2mi_embed_decode,
    gpt2mi_sample greedy and at temperature 0.8 / top_k 50 / top_p 0.95, gpt2mi_decode_step on a random-weight plan) and
    their _ragged forms at equal and at mixed positions; gpt2mi_attn_extend and gpt2mi_decode_extend over row maps, and
    gpt2mi_sample_penalized with neutral and non-neutral values. The cache entries over both formats: gpt2mi_kv_store
    and gpt2mi_kv_store_fp8, gpt2mi_attn_decode_fp8_ragged, gpt2mi_attn_extend_fp8, and gpt2mi_attn_decode_shared[_fp8]
    over share maps.
    Small shapes (B = 4 or 5, H = 2, Tcap = 70, positions 0 / 31 / 32 / 69,
    V = 509 and 50257) and GPT-2 124M's widths at B = 1, 8, 64 with pos = 575 in a 1024-position cache. Every library
    gets clones of the same seeded inputs; every output (out, the whole workspace, both caches and their scales, x, tok,
    seq, probs_out, logits) is compared
    bitwise against the first library's; each row is timed in interleaved rounds (HIP events around back-to-back
    launches, the median round). A row whose symbol a library lacks is skipped for that library, and says so."""
    g = torch.Generator(device=dev).manual_seed(0)
    bf = torch.bfloat16
    rn = lambda *s, scale=1.0, dt=torch.float32: (torch.randn(*s, device=dev, generator=g) * scale).to(dt)  # noqa: E731
    ints = lambda v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    stats = {"rows": 0, "mismatches": 0, "skipped": 0}

    def row(label, symbol, make, call, rounds=5, reps=20):
        """make() -> a fresh state (dict of tensors, clones of the shared inputs); call(lib, state) -> rc."""
        have = [i for i, lib in enumerate(libs) if hasattr(lib, symbol)]
        for i in set(range(len(libs))) - set(have):
            print(f"{label:44s} SKIPPED for lib{i}: no {symbol}", flush=True)
            stats["skipped"] += 1
        if not have or have[0] != 0:
            return
        states = {i: make() for i in have}
        for i in have:
            rc = call(libs[i], states[i])
            assert rc == 0, (label, i, rc, libs[i].gpt2mi_last_error())
        torch.cuda.synchronize()
        bad = [f"lib{i} {k}" for i in have[1:] for k, v in states[i].items() if not torch.equal(v, states[0][k])]
        stats["rows"] += 1
        stats["mismatches"] += len(bad)
        times = {i: [] for i in have}
        for _ in range(rounds):
            for i in have:
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _r in range(reps):
                    call(libs[i], states[i])
                e.record()
                torch.cuda.synchronize()
                times[i].append(s.elapsed_time(e) / reps)
        verdict = "MISMATCH " + ", ".join(bad) if bad else f"bitwise equal ({', '.join(states[0])})"
        print(f"{label:44s} " + "  ".join(f"lib{i}: {sorted(t)[rounds // 2] * 1e3:8.1f} us" for i, t in times.items()) +
              f"  {verdict}", flush=True)

    def variants(B, positions, mixed):
        """(label suffix, scalar position or None, position list) of a case: scalar and _ragged at each equal position,
        _ragged at the mixed ones."""
        out = []
        for p in positions:
            out += [(f"pos={p}", p, [p] * B), (f"ragged pos={p}", None, [p] * B)]
        return out + [("ragged mixed", None, mixed)]

    def cache(B, H, Tcap, fp8, shares=()):
        """A random cache of B streams as a function that clones it: kcache / vcache [B][H][Tcap][64] in bf16, or with fp8
        their codes and kscale / vscale [B][H][Tcap] (generation.kv_quantize of random rows). `shares`: (rows, length)
        groups whose rows hold a copy of the lowest one's first `length` positions."""
        src = dict(kcache=rn(B, H, Tcap, 64, dt=bf), vcache=rn(B, H, Tcap, 64, dt=bf))
        if fp8:
            (kc, ks), (vc, vs) = (kv_quantize(t) for t in src.values())
            src = dict(kcache=kc, vcache=vc, kscale=ks, vscale=vs)
        for rows, n in shares:
            for t in src.values():
                t[rows, :, :n] = t[rows[0], :, :n]
        return lambda: {k: v.clone() for k, v in src.items()}

    # the cache of a state as an entry takes it: kcache, vcache and, over fp8, kscale, vscale
    cache_args = lambda s: [s[k].data_ptr() for k in ("kcache", "vcache", "kscale", "vscale") if k in s]  # noqa: E731
    fp8_tag = lambda fp8: "_fp8" if fp8 else ""  # noqa: E731

    def kv_store(B, H, Tcap, T_src, n, t0):
        """gpt2mi_kv_store and gpt2mi_kv_store_fp8 of the first n of T_src rows per sequence to positions t0..: one thread
        per 8 values, B n 16 H of them. The label says how many and how many of them the last block of 256 holds: at H = 12
        the count is a multiple of 256 whenever B n is one of 4, so the small row and B = 1 are the partial last blocks."""
        qkv = rn(B * T_src, 3 * 64 * H, dt=bf)
        threads = B * n * 16 * H
        for fp8 in (False, True):
            row(f"kv_store{fp8_tag(fp8)} B={B} H={H} Tcap={Tcap} n={n} t0={t0} threads={threads} "
                f"(last block {threads % 256 or 256})",
                "gpt2mi_kv_store" + fp8_tag(fp8), cache(B, H, Tcap, fp8),
                lambda lib, s, fp8=fp8: getattr(lib, "gpt2mi_kv_store" + fp8_tag(fp8))(
                    qkv.data_ptr(), *cache_args(s), B, T_src, n, t0, H, 64, Tcap, st))

    def attn(B, H, Tcap, vs, fp8=False, shared=()):
        """The variants `vs` of gpt2mi_attn_decode[_ragged] (fp8: gpt2mi_attn_decode_fp8_ragged, which has no scalar form),
        then gpt2mi_attn_decode_shared[_fp8] over each case of `shared`: (label, pos, share_group, share_len)."""
        C = 64 * H
        qkv = rn(B, 3 * C, dt=bf)
        ws_n = libs[0].gpt2mi_attn_decode_workspace(B, H, Tcap)
        state = lambda c: dict(out=torch.zeros(B, C, dtype=bf, device=dev), ws=torch.zeros(ws_n, device=dev), **c())  # noqa
        own = cache(B, H, Tcap, fp8)
        for name, p, plist in vs:
            if fp8 and p is not None:
                continue
            sym = "gpt2mi_attn_decode" + fp8_tag(fp8) + ("" if p is not None else "_ragged")
            arg = p if p is not None else ints(plist)
            row(f"attn_decode{fp8_tag(fp8)} B={B} H={H} Tcap={Tcap} {name}", sym, lambda: state(own),
                lambda lib, s, sym=sym, arg=arg: getattr(lib, sym)(
                    qkv.data_ptr(), *cache_args(s), s["out"].data_ptr(), s["ws"].data_ptr(), ws_n, B, H, 64, Tcap, arg,
                    st))
        for name, pos, group, length in shared:
            sym = "gpt2mi_attn_decode_shared" + fp8_tag(fp8)
            groups = [([b for b in range(B) if group[b] == g], length[g]) for g in sorted(set(group)) if length[g]]
            row(f"attn_decode_shared{fp8_tag(fp8)} B={B} H={H} Tcap={Tcap} {name}", sym,
                lambda c=cache(B, H, Tcap, fp8, groups): state(c),
                lambda lib, s, sym=sym, pa=ints(pos), ga=ints(group), la=ints(length): getattr(lib, sym)(
                    qkv.data_ptr(), *cache_args(s), s["out"].data_ptr(), s["ws"].data_ptr(), ws_n, B, H, 64, Tcap, pa,
                    ga, la, st))

    def attn_extend(B, H, Tcap, maps, fp8=False):
        """gpt2mi_attn_extend (fp8: gpt2mi_attn_extend_fp8) over each row map (label, seq, pos): R rows of B sequences."""
        C = 64 * H
        sym = "gpt2mi_attn_extend" + fp8_tag(fp8)
        for name, seq, pos in maps:
            R = len(seq)
            qkv = rn(R, 3 * C, dt=bf)
            ws_n = libs[0].gpt2mi_attn_decode_workspace(R, H, Tcap)
            make = lambda R=R, ws_n=ws_n, c=cache(B, H, Tcap, fp8): dict(  # noqa: E731
                out=torch.zeros(R, C, dtype=bf, device=dev), ws=torch.zeros(ws_n, device=dev), **c())
            row(f"attn_extend{fp8_tag(fp8)} B={B} H={H} Tcap={Tcap} {name}", sym, make,
                lambda lib, s, R=R, qkv=qkv, ws_n=ws_n, sa=ints(seq), pa=ints(pos): getattr(lib, sym)(
                    qkv.data_ptr(), *cache_args(s), s["out"].data_ptr(), s["ws"].data_ptr(), ws_n, R, B, H, 64, Tcap, sa,
                    pa, st))

    def embed(B, C, V, Tcap, vs):
        tok = torch.randint(0, V, (B,), device=dev, generator=g)
        wte, wpe = rn(V, C), rn(Tcap, C)
        make = lambda: dict(x=torch.zeros(B, C, device=dev))  # noqa: E731
        for name, p, plist in vs:
            sym = "gpt2mi_embed_decode" + ("" if p is not None else "_ragged")
            arg = p if p is not None else ints(plist)
            row(f"embed_decode B={B} C={C} {name}", sym, make,
                lambda lib, s, sym=sym, arg=arg: getattr(lib, sym)(tok.data_ptr(), wte.data_ptr(), wpe.data_ptr(),
                                                                   s["x"].data_ptr(), B, C, arg, st))

    def sample(B, V, ldl, Tcap, vs):
        logits = rn(B, ldl, scale=3.0)
        make = lambda: dict(tok=torch.zeros(B, dtype=torch.int64, device=dev),  # noqa: E731
                            seq=torch.zeros(B, Tcap, dtype=torch.int64, device=dev),
                            probs_out=torch.zeros(B, V, device=dev))
        for mode, (t, k, tp) in {"greedy": (0.0, 0, 1.0), "t0.8 k50 p0.95": (0.8, 50, 0.95)}.items():
            for name, p, plist in vs:
                def call(lib, s, p=p, arr=ints(plist), t=t, k=k, tp=tp):
                    a = (logits.data_ptr(), ldl, B, V, t, k, tp, 7)
                    z = (-1, None, s["tok"].data_ptr(), s["seq"].data_ptr(), Tcap, s["probs_out"].data_ptr(), st)
                    if p is not None:
                        return lib.gpt2mi_sample(*a, p, *z)
                    return lib.gpt2mi_sample_ragged(*a, arr, None, *z)  # (row_id NULL: the row number)
                row(f"sample {mode} B={B} V={V} {name}", "gpt2mi_sample" + ("" if p is not None else "_ragged"), make, call)

    def sample_penalized(B, V, ldl, T):
        """gpt2mi_sample_penalized at position T - 1 over a random history of T - 1 tokens (seq is the history and takes
        the token), with neutral values (the plain kernels, logits_out a copy) and with (1.3, 0.5, 0.25)."""
        logits = rn(B, ldl, scale=3.0)
        hist = torch.randint(0, V, (B, T), device=dev, generator=g)
        pos, starts = ints([T - 1] * B), ints([(17 * b) % T for b in range(B)])
        pens = {}  # id(state) -> its gpt2mi_penalties, kept alive with it

        def make(vals):
            s = dict(tok=torch.zeros(B, dtype=torch.int64, device=dev), seq=hist.clone(),
                     probs_out=torch.zeros(B, V, device=dev), logits_out=torch.zeros(B, V, device=dev))
            pens[id(s)] = K.Penalties(*vals, s["seq"].data_ptr(), T, B, None, ctypes.cast(starts, ctypes.c_void_p))
            return s
        for mode, (t, k, tp) in {"greedy": (0.0, 0, 1.0), "t0.8 k50 p0.95": (0.8, 50, 0.95)}.items():
            for name, vals in {"neutral": (1.0, 0.0, 0.0), "rp1.3 pp0.5 fp0.25": (1.3, 0.5, 0.25)}.items():
                row(f"sample_penalized {mode} B={B} V={V} {name}", "gpt2mi_sample_penalized",
                    lambda vals=vals: make(vals),
                    lambda lib, s, t=t, k=k, tp=tp: lib.gpt2mi_sample_penalized(
                        logits.data_ptr(), ldl, B, V, t, k, tp, 7, pos, None, -1, None, s["tok"].data_ptr(),
                        s["seq"].data_ptr(), T, s["probs_out"].data_ptr(), ctypes.byref(pens[id(s)]),
                        s["logits_out"].data_ptr(), st))
                pens.clear()

    def step(B, C, H, L, V, Vp, Tcap, vs, reps, extends=()):
        """gpt2mi_decode_step on random weights (shared by the libraries) with each library's own buffers and caches;
        then gpt2mi_decode_extend over each row map of `extends` (label, seq, pos) on the same plan, its buffers and
        plan->rows sized for the map's rows."""
        w = dict(wte=rn(Vp, C, scale=0.02), wpe=rn(Tcap, C, scale=0.02), lnf_w=1 + rn(C, scale=0.1), lnf_b=rn(C, scale=0.1))
        w["wte"][V:] = 0
        w["wte_bf16"] = w["wte"].to(bf)
        lw = []
        for _ in range(L):
            d = {n: (1 if n.endswith("_w") else 0) + rn(C, scale=0.1) for n in ("ln1_w", "ln1_b", "ln2_w", "ln2_b")}
            for n, (o, i) in dict(qkv=(3 * C, C), proj=(C, C), fc1=(4 * C, C), fc2=(C, 4 * C)).items():
                d[n + "_w"], d[n + "_b"] = rn(o, i, scale=0.02, dt=bf), rn(o, scale=0.02)
            lw.append(d)
        tok = torch.randint(0, V, (B,), device=dev, generator=g)
        kc0, vc0 = rn(L, B, H, Tcap, 64, dt=bf), rn(L, B, H, Tcap, 64, dt=bf)
        plans = {}  # id(state) -> (plan, layers): ctypes structures of a state, kept alive with it

        def make(M=B):
            aws = libs[0].gpt2mi_attn_decode_workspace(M, H, Tcap)
            gws = max(libs[0].gpt2mi_gemm_skinny_workspace(M, n, k)
                      for n, k in ((3 * C, C), (C, C), (4 * C, C), (C, 4 * C), (Vp, C)))
            z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
            s = dict(logits=z(M, Vp), kcache=kc0.clone(), vcache=vc0.clone(), x=z(M, C), xmid=z(M, C), ln=z(M, C, dt=bf),
                     qkv=z(M, 3 * C, dt=bf), ao=z(M, C, dt=bf), h=z(M, 4 * C, dt=bf), mean=z(M), rstd=z(M),
                     attn_ws=z(max(aws, 1)), gemm_ws=z(max(gws, 1)))
            layers = (K.DecodeLayer * L)()
            for l, Y in enumerate(layers):
                for n, t in lw[l].items():
                    setattr(Y, n, t.data_ptr())
                Y.kcache, Y.vcache = s["kcache"][l].data_ptr(), s["vcache"][l].data_ptr()
            P = K.DecodePlan()
            P.B, P.C, P.H, P.L, P.Vp, P.Tcap, P.eps = B, C, H, L, Vp, Tcap, 1e-5
            for n, t in w.items():
                setattr(P, n, t.data_ptr())
            P.layers = ctypes.cast(layers, ctypes.POINTER(K.DecodeLayer))
            for n in ("x", "xmid", "ln", "qkv", "ao", "h", "mean", "rstd", "attn_ws", "gemm_ws", "logits"):
                setattr(P, n, s[n].data_ptr())
            P.attn_ws_floats, P.gemm_ws_floats = s["attn_ws"].numel(), s["gemm_ws"].numel()
            P.rows = 0 if M == B else M
            plans[id(s)] = (P, layers)
            return s
        for name, p, plist in vs:
            sym = "gpt2mi_decode_step" + ("" if p is not None else "_ragged")
            arg = p if p is not None else ints(plist)
            row(f"decode_step B={B} C={C} L={L} Vp={Vp} {name}", sym, make,
                lambda lib, s, sym=sym, arg=arg: getattr(lib, sym)(ctypes.byref(plans[id(s)][0]), tok.data_ptr(), arg, st),
                reps=reps)
            plans.clear()
        for name, seq, pos in extends:
            R = len(seq)
            xtok = torch.randint(0, V, (R,), device=dev, generator=g)
            row(f"decode_extend B={B} C={C} L={L} Vp={Vp} {name}", "gpt2mi_decode_extend", lambda R=R: make(R),
                lambda lib, s, R=R, xtok=xtok, sa=ints(seq), pa=ints(pos): lib.gpt2mi_decode_extend(
                    ctypes.byref(plans[id(s)][0]), R, xtok.data_ptr(), sa, pa, st), reps=reps)
            plans.clear()

    # the row maps of tests/test_extend_kernels_gpu.py (three runs; one sequence absent), and R rows of one sequence
    maps = [("three-runs", [0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2], [30, 31, 32, 33, 0, 1, 2, 66, 67, 68, 69]),
            ("one-absent", [0, 0, 0, 0, 2, 2, 2, 2], [30, 31, 32, 33, 66, 67, 68, 69])]
    one_run = lambda R: (f"R={R} one run to pos=575", [0] * R, list(range(576 - R, 576)))  # noqa: E731
    small = variants(4, (0, 31, 32, 69), [0, 31, 32, 69])
    # a group of three among five rows at a shared length of one and of two whole ranges (tests/test_share_kernels_gpu.py)
    share5 = [(f"3 of 5 share {n}", pos, [0, 1, 0, 3, 0], [n, 0, n, 0, n])
              for n, pos in ((32, [32, 31, 45, 0, 69]), (64, [64, 31, 66, 0, 69]))]
    kv_store(5, 2, 70, 7, 3, 30)
    for fp8 in (False, True):
        attn(4, 2, 70, small, fp8)
        attn(5, 2, 70, (), fp8, share5)
        attn_extend(3, 2, 70, maps, fp8)
    embed(4, 128, 509, 70, small)
    for V, ldl in ((509, 512), (50257, 50432)):
        sample(4, V, ldl, 70, small)
        sample_penalized(4, V, ldl, 70)
    step(4, 128, 2, 2, 509, 512, 70, small, reps=5, extends=maps)
    for fp8 in (False, True):
        attn_extend(1, 12, 1024, [one_run(8)], fp8)
    for B in (1, 8, 64):
        big = variants(B, (575,), [575 - (37 * b) % 576 for b in range(B)])
        # groups of four rows over a prompt of 512 (a row alone at B = 1), each row somewhere in the 64 positions behind it
        n = 512 if B >= 4 else 0
        share = [(f"groups of 4 share {n}", [575 - (37 * b) % 64 for b in range(B)], [b - b % 4 for b in range(B)], [n] * B)]
        kv_store(B, 12, 1024, 64, 37, 5)
        for fp8 in (False, True):
            attn(B, 12, 1024, big, fp8, share)
        embed(B, 768, 50257, 1024, big)
        sample(B, 50257, 50432, 1024, big)
        step(B, 768, 12, 12, 50257, 50432, 1024, big, reps=5,
             extends=[one_run(R) for R in (5, 8, 16)] if B == 1 else ())
    print(f"decode A/B: {stats['rows']} rows compared against lib0, {stats['mismatches']} mismatching outputs, "
          f"{stats['skipped']} skipped", flush=True)
    if stats["mismatches"]:
        raise SystemExit(1)


def embed_mode(libs, g, st):
    """LIB_AB_OP=embed: the embedding backward at cfg 2 (B=64, T=1024, C=768, dropout 0.1): dwpe compared bitwise
    against the first library, dwte (fp32 atomics, any order) to 1e-5."""
    B, T, C, V = 64, 1024, 768, 50257
    idx = torch.randint(0, V, (B * T,), device=dev, generator=g)
    dres = torch.randn(B * T, C, device=dev, generator=g)
    res = [(torch.zeros(V, C, device=dev), torch.zeros(T, C, device=dev)) for _ in libs]
    run = lambda lib, r: lib.gpt2mi_embed_bwd(idx.data_ptr(), dres.data_ptr(), r[0].data_ptr(), r[1].data_ptr(),  # noqa
                                              B, T, T, C, 0.1, 77, st)
    for lib, r in zip(libs, res):
        assert run(lib, r) == 0
    torch.cuda.synchronize()
    for i in range(1, len(libs)):
        if not torch.equal(res[0][1], res[i][1]):
            print(f"MISMATCH lib{i} dwpe")
        if not torch.allclose(res[0][0], res[i][0], rtol=1e-5, atol=1e-6):
            print(f"MISMATCH lib{i} dwte {(res[0][0] - res[i][0]).abs().max().item()}")
    times = {i: [] for i in range(len(libs))}
    for _ in range(5):
        for i, (lib, r) in enumerate(zip(libs, res)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _r in range(5):
                run(lib, r)
            e.record()
            torch.cuda.synchronize()
            times[i].append(s.elapsed_time(e) / 5)
    print("embed_bwd " + "  ".join(f"lib{i}: {sorted(t)[2] * 1e3:8.1f} us" for i, t in times.items()), flush=True)


if __name__ == "__main__":
    main()
