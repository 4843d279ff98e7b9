"""Launch census of the GEMM launchers: launch_gemm_variant, launch_gemm_f8w, the two GEMM scans and
launch_qkv_attention, one call per case through the diagnostic entries (and two store searches) under
the profile hooks, against a recorded table.

The profile hooks aggregate per kernel name the launch count and the flops and bytes each launcher
computes ON THE HOST from its arguments, so the three numbers pin the profile name a launcher picks
for an (operand type, epilogue) pair and the bytes per element it books for the output, the residual,
the e4m3 copy and split weights.  They do not see grids, persistence or the tile walk: those are
pinned on the CPU by tests/test_gemm_plan.py.  Shapes are the smallest that still reach each branch of
the launchers: M in {1, 64, 300}, N in {128, 256, 768}, K in {64, 128, 256, 768}; every variant with
every epilogue it carries (the five timing-only variants of the diagnostic library at one shape, plain
and with split weights, where they fall back to pipe), split weights (variant | 0x100), the
persistent kernels forced through the variant argument (or SR_GEMM_TILE where the entry takes no
variant), statistics strides 1 and 2, the split-K workspace one byte short and exact, K5c at 4 and 12
heads, and one fp16 and one fp8 store search at B = 200 (the GEMM scans).

The expected table, tests/golden/gemm_launch_census.json, was recorded by
tests/golden/gen_gemm_census.py on the commit BEFORE the launchers were rewritten over
csrc/sr_gemm_plan.h (the rows of the timing-only variants later, with that commit's libraries); this
test never regenerates it.  launches compare exactly, flops and bytes to a relative 1e-12 (the same
host arithmetic on the same shapes).
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_launch_census.json")

SHAPES = ((1, 128, 64), (64, 256, 128), (300, 768, 256), (300, 256, 768), (64, 768, 768))
FOLD_SHAPES = ((1, 256, 256), (64, 768, 256), (300, 256, 768))
VARIANTS = {"auto": -1, "small": 0, "big": 1, "pipe": 4, "persist": 5, "pp": 8}
TILES = (None, "pipe_persist", "pp")   # SR_GEMM_TILE for the entries without a variant argument

# name -> (entry, arguments)
CASES = {}
for _v, _vi in VARIANTS.items():
    for _e in range(5):
        for _s in SHAPES:
            CASES["gemm_%s_e%d_%dx%dx%d" % ((_v, _e) + _s)] = ("gemm", (_vi, _e) + _s)
        if _vi >= 0:
            for _s in ((300, 256, 256), (64, 768, 768)):
                CASES["gemm_%s_split_e%d_%dx%dx%d" % ((_v, _e) + _s)] = ("gemm", (_vi | 0x100, _e) + _s)
# the timing-only variants of the diagnostic library (wrong results by design, EPI_BIAS_F16 kernels
# whatever the epilogue): one shape with two big tiles; with split weights they fall back to pipe
TIMING_VARIANTS = {"noload": 6, "noepi": 7, "p_noepi": 9, "p_mathonly": 10, "p_storeonly": 11}
for _v, _vi in TIMING_VARIANTS.items():
    for _e in range(5):
        CASES["gemm_%s_e%d_300x256x256" % (_v, _e)] = ("gemm", (_vi, _e, 300, 256, 256))
    CASES["gemm_%s_split_e0_300x256x256" % _v] = ("gemm", (_vi | 0x100, 0, 300, 256, 256))
for _e in range(5):
    # (M, N, K, workspace bytes): 6 tiles x 2 chunks exactly, one byte short, a single chunk
    for _s in ((64, 768, 768, 786432), (64, 768, 768, 786431), (64, 768, 64, 786432), (300, 256, 256, 1 << 20)):
        CASES["chunked_e%d_%dx%dx%d_ws%d" % ((_e,) + _s)] = ("chunked", (0, _e) + _s)
    CASES["chunked_split_e%d" % _e] = ("chunked", (0x100, _e, 64, 768, 1536, 1 << 20))
for _t in TILES:
    for _s in FOLD_SHAPES:
        _n = "%s_%dx%dx%d" % ((_t or "auto",) + _s)
        CASES["stats_" + _n] = ("stats", (_t,) + _s)
        CASES["lnr_stats_" + _n] = ("lnr_stats", (_t,) + _s)
        for _l in (0, 1):
            CASES["stats_y8_lnr%d_%s" % (_l, _n)] = ("stats_y8", (_t, _l) + _s)
        for _f8 in (0, 1):
            CASES["ffn1_f8%d_%s" % (_f8, _n)] = ("ffn1", (_t, _f8) + _s)
            for _e in (5, 7, 8, 12, 13):
                for _ld in ((1, 2) if _e in (5, 8, 13) else (1,)):
                    CASES["fold_f8%d_e%d_ld%d_%s" % (_f8, _e, _ld, _n)] = ("fold", (_t, _f8, _e, _ld) + _s)
for _e in (0, 5):
    for _b, _h in ((2, 4), (3, 4), (2, 12)):
        CASES["qkv_attention_e%d_b%d_h%d" % (_e, _b, _h)] = ("qkv", (_e, _b, _h))
CASES["store_search_fp16_b200"] = ("store", ("fp16",))
CASES["store_search_fp8_b200"] = ("store", ("fp8",))


def _profile(lib_call, read):
    """Run lib_call() with the profile hooks of the product and the diagnostic library on (they are
    two libraries with a profile table each) and return the merged {kernel: launches, flops, bytes}."""
    from super_rag_amd import _native as N
    libs = (N.load(), N.load_diag())
    for lib in libs:
        N.check(lib.sr_profile_enable(1))
    try:
        lib_call()
    finally:
        for lib in libs:
            N.check(lib.sr_profile_enable(0))
    out = {}
    for lib in libs:
        for k, v in read(lib).items():
            o = out.setdefault(k, {"launches": 0, "flops": 0.0, "bytes": 0.0})
            for f in o:
                o[f] += v[f]
    return dict(sorted(out.items()))


def _read(lib):
    import ctypes
    from super_rag_amd import _native as N
    buf = (N.KernelStatC * 256)()
    n = ctypes.c_int32(0)
    N.check(lib.sr_profile_read(buf, 256, ctypes.byref(n)))
    return {buf[i].name.decode(): {"launches": int(buf[i].launches), "flops": float(buf[i].flops),
                                   "bytes": float(buf[i].bytes)} for i in range(n.value)}


def run_case(name, setenv, delenv):
    """One call of the case's entry under the profile hooks -> {kernel: {launches, flops, bytes}}.
    setenv(k, v) / delenv(k) change the environment (monkeypatch's in the test)."""
    import torch
    from super_rag_amd import _native as N
    entry, a = CASES[name]
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    f16 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float16)
    f32 = lambda *s: torch.ones(*s, device=dev, dtype=torch.float32)
    u8 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.uint8)
    p = lambda t: t.data_ptr() if t is not None else None
    delenv("SR_GEMM_TILE")
    if entry in ("stats", "lnr_stats", "stats_y8", "ffn1", "fold") and a[0]:
        setenv("SR_GEMM_TILE", a[0])
    keep = []

    if entry in ("gemm", "chunked"):
        variant, epi, M, N_, K = a[:5]
        x_k = K // 2 if variant >= 0 and variant & 0x100 else K
        X, W, b = f16(M, x_k), f16(N_, K), f32(N_)
        R = f32(M, N_) if epi == 2 else f16(M, N_) if epi == 4 else None
        Y = torch.zeros(M, N_, device=dev, dtype=torch.float32 if epi in (2, 3) else torch.float16)
        if entry == "gemm":
            call = lambda: N.call_diag("sr_diag_gemm", variant, epi, p(X), x_k, p(W), p(b), p(R), N_ if R is not None else 0,
                                       p(Y), N_, M, N_, K, 0, st)
        else:
            ws = u8(a[5])
            call = lambda: N.call_diag("sr_diag_gemm_chunked", variant, epi, p(X), x_k, p(W), p(b), p(R),
                                       N_ if R is not None else 0, p(Y), N_, M, N_, K, p(ws), a[5], 0, st)
    elif entry in ("stats", "lnr_stats", "stats_y8"):
        lnr = entry == "lnr_stats" or (entry == "stats_y8" and a[1])
        M, N_, K = a[-3:]
        X, W, b, R, Y = f16(M, K), f16(N_, K), f32(N_), f16(M, N_), f16(M, N_)
        mr, gamma, so, y8 = f32(M, 2), f32(N_), f32(M, N_ // 128, 2), u8(M, N_)
        if entry == "stats":
            call = lambda: N.call_diag("sr_diag_gemm_stats", p(X), K, p(W), p(b), p(R), N_, p(Y), N_, M, N_, K,
                                       p(so), 0, st)
        elif entry == "lnr_stats":
            call = lambda: N.call_diag("sr_diag_gemm_lnr_stats", p(X), K, p(W), p(b), p(R), N_, p(mr), p(gamma),
                                       p(Y), N_, M, N_, K, p(so), 0, st)
        else:
            call = lambda: N.call_diag("sr_diag_gemm_stats_y8", int(lnr), p(X), K, p(W), p(b), p(R), N_,
                                       p(mr) if lnr else None, p(gamma) if lnr else None, p(Y), N_, p(y8),
                                       M, N_, K, p(so), 0, st)
    elif entry == "ffn1":
        f8 = a[1]
        M, N_, K = a[-3:]
        X = u8(M, K) if f8 else f16(M, K)
        W = u8(N_, K) if f8 else f16(N_, K)
        wexp, b, cs, mr = torch.full((N_,), 127, device=dev, dtype=torch.uint8), f32(N_), f32(N_), f32(M, 2)
        Y = u8(M, N_) if f8 else f16(M, N_)
        call = lambda: N.call_diag("sr_diag_ffn1", 0, f8, p(X), K, p(W), p(wexp), p(b), p(cs), p(mr), p(Y), N_,
                                   M, N_, K, 0, st)
    elif entry == "fold":
        f8, epi, ld = a[1:4]
        M, N_, K = a[-3:]
        lnf, lnr, stats = epi == 5, epi in (8, 13), epi != 5
        xl, rl = (ld if lnf else 1), (ld if lnr else 1)
        X = u8(M * xl, K) if f8 else f16(M * xl, K)
        W = u8(N_, K) if f8 else f16(N_, K)
        wexp, b, cs, gamma = torch.full((N_,), 127, device=dev, dtype=torch.uint8), f32(N_), f32(N_), f32(N_)
        R, mr, Y, y8, so = f16(M * rl, N_), f32(M * ld, 2), f16(M, N_), u8(M, N_), f32(M, N_ // 128, 2)
        call = lambda: N.call_diag("sr_diag_gemm_fold", f8, epi, p(X), K * xl, p(W), p(wexp) if f8 else None, p(b),
                                   p(cs) if lnf else None, p(R) if stats else None, N_ * rl if stats else 0,
                                   p(mr) if (lnf or lnr) else None, ld, p(gamma) if lnr else None, p(Y), N_,
                                   p(y8) if epi in (12, 13) else None, p(so) if stats else None, M, N_, K, 0, st)
    elif entry == "qkv":
        epi, B, H = a
        d, S = 64 * H, 128
        X, W, b = f16(B * S, d), f16(3 * d, d), f32(3 * d)
        cs, mr = f32(3 * d), f32(B * S, 2)
        mask = torch.ones(B, S, device=dev, dtype=torch.int32)
        ctx = f16(B * S, d)
        call = lambda: N.call_diag("sr_diag_qkv_attention", epi, p(X), d, p(W), p(b), p(cs) if epi == 5 else None,
                                   p(mr) if epi == 5 else None, p(mask), p(ctx), B, S, d, H, 0, st)
    else:
        from super_rag_amd.store import NativeStore, NativeStoreSet
        rng = np.random.default_rng(5)
        store = NativeStore(128, device=0) if a[0] == "fp16" else NativeStoreSet(128, [0], dtype="fp8")
        keep.append(store)
        store.add(rng.standard_normal((20000, 128)).astype(np.float32))
        q = rng.standard_normal((200, 128)).astype(np.float32)
        call = lambda: store.search(q, 10)
    try:
        out = _profile(call, _read)
        torch.cuda.synchronize()
    finally:
        for s in keep:
            s.close()
        delenv("SR_GEMM_TILE")
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_lists_every_case(golden):
    assert sorted(golden) == sorted(CASES)


def test_gemm_launch_census(golden, monkeypatch):
    """Every case in one test (each is one tiny launch; the whole table takes a few seconds)."""
    bad = []
    for name in CASES:
        got = run_case(name, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
        want = golden[name]
        if sorted(got) != sorted(want):
            bad.append((name, "kernels", sorted(got), sorted(want)))
            continue
        for k, w in want.items():
            g = got[k]
            if g["launches"] != w["launches"]:
                bad.append((name, k, "launches", g, w))
            for f in ("flops", "bytes"):
                if abs(g[f] - w[f]) > 1e-12 * abs(w[f]):
                    bad.append((name, k, f, g, w))
    assert not bad, "%d mismatches, first: %r" % (len(bad), bad[:5])
