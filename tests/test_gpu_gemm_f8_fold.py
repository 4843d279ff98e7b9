"""GPU: the LayerNorm-folded encoder GEMMs one kernel at a time through sr_diag_gemm_fold (the
product's launch_gemm / launch_gemm_f8w with its automatic kernel choice): the fp8 FFN2 / O-projection
/ QKV forms (e4m3 A bytes, e4m3 weights with per-row E8M0 exponents) and the strided-statistics forms
of the CLS-only last layer, per element against fp64.

Exact cases use the dyadic operands of tests/fold_ref.py (every product and epilogue term a multiple
of one quantum per output column, sums below 2^24 quanta: every fp32 evaluation order is exact), so
Y must equal fp16(ref) bit for bit and the e4m3 copy must equal e4m3(Y) byte for byte; the reference
is fp64 on the dequantised operands, computed on the device.  The span statistics follow
tests/test_gpu_gemm.py: sum within rtol 1e-6 / atol 1e-3 of the fp64 sum of the kernel's own fp16 Y,
M2 within M2_GATE of two-pass fp64 on the same Y.  The random-operand cases allow half an fp16 ulp
plus the accumulation bound K 2^-23 sum_k |x_k w_k| (fp64, from the operands).
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fold_ref as FR  # noqa: E402
from test_gpu_gemm import M2_GATE  # noqa: E402

pytestmark = pytest.mark.gpu

LNF, RES, LNR, RES_Y8, LNR_Y8 = 5, 7, 8, 12, 13          # sr::Epilogue codes
KIND = {LNF: "lnf", RES: "res", LNR: "lnr", RES_Y8: "res", LNR_Y8: "lnr"}
GUARD = 40
PERSIST_M = 171 * 256 + 77                                 # x 3 n-tiles = 516 tiles: the persistent kernels


def _dev():
    import torch
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=1)
def _case(N, K, rows, f8):
    return FR.dyadic_gemm_case(N, K, rows, seed=N + K + rows + int(f8), f8=f8, device="cuda:0")


@functools.lru_cache(maxsize=1)
def _tables():
    import torch
    lut = torch.from_numpy(FR.fp16_to_e4m3_lut()).to(_dev())
    vals = torch.from_numpy(np.nan_to_num(FR.e4m3_values(np.arange(256, dtype=np.uint8)), nan=0.0)).to(_dev())
    return lut, vals


def _e4m3_of_fp16(Y):
    import torch
    lut, _ = _tables()
    return lut[(Y.view(torch.int16).long() & 0xFFFF)]


def _spread(t, ld, poison):
    """Row m of t at row ld m of a poisoned array (the rows between are never to be read)."""
    import torch
    if ld == 1:
        return t.contiguous()
    big = torch.full((t.shape[0] * ld,) + tuple(t.shape[1:]), poison, device=t.device, dtype=t.dtype)
    big[::ld] = t
    return big


def _launch(f8, epi, X, W, wexp, bias, colsum, R, mr, gamma, M, N, K, stat_ld=1, alias=False):
    """One sr_diag_gemm_fold launch on M logical rows (tensors hold the logical rows; the operand the
    statistics belong to and mr are spread over every stat_ld-th row of poisoned arrays).
    Returns (Y, y8, stat) with guard rows after M, all checked here."""
    import torch
    from super_rag_amd import _native as NT
    d = _dev()
    kind = KIND[epi]
    y8 = epi in (RES_Y8, LNR_Y8)
    stats = kind != "lnf"
    xp = (0x7E if f8 else 1e4)
    Xb = _spread(X, stat_ld if kind == "lnf" else 1, xp)
    lda = K * (stat_ld if kind == "lnf" else 1)
    mrb = _spread(mr, stat_ld, 1e4) if mr is not None else None
    Yall = torch.full((M + GUARD, N), 777.0, device=d, dtype=torch.float16)
    Rb, ldr = None, 0
    if stats:
        if alias:
            assert stat_ld == 1
            Yall[:M] = R
            Rb, ldr = Yall, N
        else:
            Rb = _spread(R, stat_ld if kind == "lnr" else 1, 1e4)
            ldr = N * (stat_ld if kind == "lnr" else 1)
    Y8all = torch.full((M + GUARD, N), 0x5A, device=d, dtype=torch.uint8)
    st = torch.full((M + GUARD, N // 128, 2), 777.0, device=d)
    p = lambda t: t.data_ptr() if t is not None else None
    NT.call_diag("sr_diag_gemm_fold", int(f8), epi, Xb.data_ptr(), lda, W.data_ptr(), p(wexp) if f8 else None,
                 bias.data_ptr(), p(colsum) if kind == "lnf" else None, p(Rb), ldr,
                 p(mrb) if kind != "res" else None, stat_ld, p(gamma) if kind == "lnr" else None,
                 Yall.data_ptr(), N, Y8all.data_ptr() if y8 else None, st.data_ptr() if stats else None,
                 M, N, K, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((Yall[M:] == 777.0).all()), "Y rows past M were written"
    assert bool((Y8all[M:] == 0x5A).all()), "y8 rows past M were written"
    assert bool((st[M:] == 777.0).all()), "stat_out rows past M were written"
    if not y8:
        assert bool((Y8all == 0x5A).all())
    if not stats:
        assert bool((st == 777.0).all())
    return Yall[:M], (Y8all[:M] if y8 else None), (st[:M] if stats else None)


def _check_y8_and_stats(Y, y8, st, tag):
    import torch
    M, N = Y.shape
    if y8 is not None:
        want = _e4m3_of_fp16(Y)
        assert torch.equal(y8, want), f"{tag}: {int((y8 != want).sum())} e4m3 bytes differ from e4m3(Y)"
    if st is not None:
        y = Y.double().reshape(M, N // 128, 128)
        s = st.double()
        ysum = y.sum(-1)
        m2 = ((y - y.mean(-1, keepdim=True)) ** 2).sum(-1)
        assert float(m2.min()) > 0.0
        assert bool(((s[..., 0] - ysum).abs() <= 1e-3 + 1e-6 * ysum.abs()).all()), \
            f"{tag}: span sums, max err {float((s[..., 0] - ysum).abs().max()):.3e}"
        rel = ((s[..., 1] - m2).abs() / m2).max().item()
        print(f"{tag}: max |sum err| {float((s[..., 0] - ysum).abs().max()):.2e}, max rel M2 err {rel:.2e} "
              f"(gate {M2_GATE})")
        assert rel <= M2_GATE, rel


def _operands(c, epi, M):
    kind = KIND[epi]
    return dict(colsum=c["colsum"], R=(c["R_res"][:M] if kind == "res" else c["R_lnr"][:M]) if kind != "lnf" else None,
                mr=None if kind == "res" else (c["mr_lnf"][:M] if kind == "lnf" else c["mr_lnr"][:M]),
                gamma=c["gamma"])


def _exact(f8, epi, M, N, K, stat_ld=1, alias=False):
    import torch
    c = _case(N, K, M, f8)
    o = _operands(c, epi, M)
    Y, y8, st = _launch(f8, epi, c["X"][:M], c["W"], c["wexp"], c["bias"], o["colsum"], o["R"], o["mr"],
                        o["gamma"], M, N, K, stat_ld=stat_ld, alias=alias)
    kind = KIND[epi]
    kw = {"lnf": dict(colsum=o["colsum"], mr=o["mr"]), "res": dict(R=o["R"]),
          "lnr": dict(R=o["R"], mr=o["mr"], gamma=o["gamma"])}[kind]
    ref = FR.fold_ref_t(kind, c["Xd"](slice(0, M)), c["Wd"], c["bias"], **kw)
    assert bool((ref.float().double() == ref).all())           # exact in fp32: one rounding to fp16 below
    assert float(ref.abs().max()) < 65504.0
    want = ref.float().half()
    tag = f"f8 {int(f8)} epi {epi} {M}x{N}x{K} stat_ld {stat_ld}"
    bad = Y.view(torch.int16) != want.view(torch.int16)
    if bool(bad.any()):
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} outputs differ from fp16(ref); first at "
                             f"{i}: got {float(Y[i[0], i[1]])!r}, want {float(want[i[0], i[1]])!r}")
    _check_y8_and_stats(Y, y8, st, tag)


EXACT_SHAPES = [(1, 768, 256), (13, 768, 256), (255, 768, 256), (256 + 17, 768, 384), (600, 256, 256),
                (600, 768, 3072), (PERSIST_M, 768, 256), (PERSIST_M, 768, 3072)]


@pytest.mark.parametrize("M,N,K,epi", [s + (e,) for s in EXACT_SHAPES for e in (LNR, LNR_Y8, RES, LNF)])
def test_fp8_fold_exact(M, N, K, epi):
    _exact(True, epi, M, N, K)


def test_fp8_ffn2_in_place():
    """Y aliases R (fold_ffn writes u2 over u1)."""
    _exact(True, LNR, 600, 768, 3072, alias=True)


@pytest.mark.parametrize("f8,epi,M", [(False, LNR, 300), (False, LNR_Y8, 300), (False, LNF, 300), (True, LNR, 300),
                                      (False, LNR, PERSIST_M), (False, LNR_Y8, PERSIST_M),
                                      (False, LNF, PERSIST_M)])
def test_strided_statistics_exact(f8, epi, M):
    """stat_ld = 7 with ldr = 7 N (LNR) or lda = 7 K (LNF): row m reads operand row and statistics row
    7 m of arrays whose other rows hold poison (the CLS-only last layer's launches).  At the
    persistent row count fp16 EPI_LNR16_STATS leaves the persistent kernel (its epilogue stages
    consecutive statistics), the _Y8 and LNF forms stay on it."""
    _exact(f8, epi, M, 768, 256, stat_ld=7)


@pytest.mark.parametrize("epi", [LNF, RES, LNR, RES_Y8, LNR_Y8])
def test_fp8_fold_random_operands(epi):
    import torch
    M, N, K = 600, 768, 3072
    d = _dev()
    g = torch.Generator(device=d).manual_seed(100 + epi)
    _, vals = _tables()
    finite = torch.tensor([b for b in range(256) if b not in FR.NAN_CODES], device=d, dtype=torch.uint8)
    # e4m3 bytes of normal-ish values: activations ~ N(0, 0.7), weight rows filling the e4m3 range
    u = torch.randn(M, K, device=d, generator=g) * 0.7 + 0.05
    X8 = torch.from_numpy(FR.e4m3_bytes(u.double().cpu().numpy())).to(d)
    w = torch.randn(N, K, device=d, generator=g) * 60.0
    W8 = torch.from_numpy(FR.e4m3_bytes(w.double().cpu().numpy())).to(d)
    assert bool(torch.isin(X8, finite).all()) and bool(torch.isin(W8, finite).all())
    wexp = torch.randint(114, 121, (N,), device=d, generator=g, dtype=torch.int32).to(torch.uint8)
    Xd = vals[X8.long()]
    Wd = vals[W8.long()] * torch.exp2(wexp.double() - 127.0)[:, None]
    bias = torch.randn(N, device=d, generator=g) * 0.1
    colsum = Wd.sum(1).float()
    gamma = 1.0 + torch.randn(N, device=d, generator=g) * 0.2
    R = (torch.randn(M, N, device=d, generator=g) * 0.8 + 0.3).half()
    kind = KIND[epi]
    if kind == "lnf":
        mr = torch.stack([Xd.mean(1), torch.rsqrt(Xd.var(1, unbiased=False) + 1e-5)], 1).float().contiguous()
    else:
        mr = torch.stack([R.double().mean(1), torch.rsqrt(R.double().var(1, unbiased=False) + 1e-5)], 1).float().contiguous()
    Y, y8, st = _launch(True, epi, X8, W8, wexp, bias, colsum, R, mr if kind != "res" else None, gamma, M, N, K)
    kw = {"lnf": dict(colsum=colsum, mr=mr), "res": dict(R=R), "lnr": dict(R=R, mr=mr, gamma=gamma)}[kind]
    ref = FR.fold_ref_t(kind, Xd, Wd, bias, **kw)
    acc = K * 2.0 ** -23 * (Xd.abs() @ Wd.abs().T)              # wexp is inside Wd
    if kind == "lnf":
        acc = acc * mr[:, 1:2].double()
    _, e = torch.frexp(ref.abs() + acc)
    half_ulp = 0.5 * torch.exp2((e - 11).clamp_min(-24).double())
    err = (Y.double() - ref).abs()
    ratio = (err / (half_ulp + acc)).max().item()
    print(f"epi {epi} random {M}x{N}x{K}: max err / bound {ratio:.3f}, max |err| {float(err.max()):.3e}")
    assert bool((err <= half_ulp + acc).all()), ratio
    _check_y8_and_stats(Y, y8, st, f"epi {epi} random")
