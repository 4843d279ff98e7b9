"""CPU: the references of tests/fold_ref.py against independent statements of the same things, and
the derived GELU-table error bound against an fp32 emulation of both tables (k_gemm.hip
gelu_t_tab_init / gelu_t8_tab_init and the two epilogue forms of store_tile_gelu).

The emulation lives only here: the GPU tests compare the kernels with fold_ref.two_gelu, never with
the emulation.  The last tests show that the brackets and the exact GEMM cases catch a subtly wrong
implementation: an emulation whose nearest-node index is shifted by one leaves the brackets, and an
fp64 reference that drops the last 128-byte K-step no longer equals the fp32 result.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fold_ref as FR  # noqa: E402

F = np.float32


# ---- e4m3 ------------------------------------------------------------------------------------------
def _probe_points():
    pos = FR.e4m3_values(np.arange(0x7F, dtype=np.uint8))
    mids = (pos[:-1] + pos[1:]) / 2.0
    # (the fp32 neighbours of the midpoints: torch converts fp64 through fp32)
    near = np.concatenate([np.nextafter(mids.astype(F), F(np.inf)), np.nextafter(mids.astype(F), F(-np.inf))])
    near = near.astype(np.float64)
    v = np.concatenate([pos, mids, near, [448.0, 449.0, 464.0, 480.0, 1e4, 2.0 ** -10, 2.0 ** -11]])
    return np.concatenate([v, -v])


def test_e4m3_all_codes_and_midpoints():
    import torch
    import mv_fp8_ref as MV
    codes = np.arange(256, dtype=np.uint8)
    vals = FR.e4m3_values(codes)
    tv = torch.from_numpy(codes).view(torch.float8_e4m3fn).double().numpy()
    finite = ~np.isnan(vals)
    assert finite.sum() == 254 and np.isnan(tv[~finite]).all()
    assert np.array_equal(vals[finite], tv[finite]) and np.array_equal(vals[finite], MV.E4M3[finite])
    back = FR.e4m3_bytes(vals[finite])
    assert np.array_equal(back, codes[finite])                  # every code (and the sign of -0) round-trips
    v = _probe_points()
    got = FR.e4m3_bytes(v)
    assert np.array_equal(got, MV.e4m3_rne(v))
    sat = np.clip(v, -448.0, 448.0)
    tq = torch.from_numpy(sat).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(got, tq)
    assert not np.isin(got, FR.NAN_CODES).any()
    lut = FR.fp16_to_e4m3_lut()
    h = np.array([0.0, -0.0, 1.0, 448.0, 464.0, 65504.0, -65504.0, 2.0 ** -24], np.float16)
    assert np.array_equal(lut[h.view(np.uint16)], FR.e4m3_bytes(h.astype(np.float64)))


# ---- quantize_rows_ref ---------------------------------------------------------------------------
def test_quantize_rows_ref_matches_the_oracle_and_the_definition():
    import torch
    from oracle import encoder_ref as ER
    W = FR.quantize_case_rows(256)
    b, wexp = FR.quantize_rows_ref(W)
    Wd = W.astype(np.float64)
    amax = np.abs(Wd).max(1)
    e = 127 - wexp.astype(np.int64)
    nz = amax > 0
    assert np.all(e[~nz] == 0)
    unclamped = nz & (np.abs(e) < 127)
    assert np.all(np.ldexp(amax[nz], e[nz].astype(np.int32)) <= 448.0)
    assert np.all(np.ldexp(amax[unclamped], (e[unclamped] + 1).astype(np.int32)) > 448.0)
    assert not np.isin(b, FR.NAN_CODES).any()
    # by value against the oracle's restatement (torch fp32: rows whose scaled values stay normal)
    ok = nz & (amax >= 2.0 ** -14)
    want = ER.fp8_rows(torch.from_numpy(W[ok].astype(np.float32))).double().numpy()
    assert np.array_equal(FR.dequant_rows(b[ok], wexp[ok]), want)


# ---- fp32 emulation of the two GELU tables -------------------------------------------------------
XMAXF = float(F(5.6568542494923802))


def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def emulate_e4m3_form(x, shift=0):
    """min(x T8[nearest node], 448) in fp32 (before the e4m3 conversion); shift: a wrong index."""
    x = np.asarray(x, F)
    h = 2.0 * XMAXF / 4096.0
    tab = FR._erfc(-(-XMAXF + np.arange(4097) * h) * 0.70710678118654752).astype(F)
    scale = F(F(4096.0) / F(F(2.0) * F(XMAXF)))
    z = np.clip(_fma32(x, scale, F(0.5 * 4096 + 0.5)), F(0.0), F(4096.0))
    idx = np.clip(z.astype(np.int64) + shift, 0, 4096)
    return np.minimum((x * tab[idx]).astype(F), F(448.0))


def emulate_fp16_form(x):
    """x (T[i] + frac dT[i]) in fp32 (before the fp16 conversion)."""
    x = np.asarray(x, F)
    h = float(F(F(2.0) * F(XMAXF) / F(1024.0)))
    x0 = -XMAXF + np.arange(1025) * h
    t0 = FR._erfc(-x0 * 0.70710678118654752).astype(F)
    t1 = FR._erfc(-(x0 + h) * 0.70710678118654752).astype(F)
    t1[-1] = t0[-1]
    dt = (t1 - t0).astype(F)
    inv = F(F(1.0) / F(F(2.0) * F(XMAXF)))
    az = (np.clip(_fma32(x, inv, F(0.5)), F(0.0), F(1.0)) * F(1024.0)).astype(F)
    i = np.floor(az).astype(np.int64)
    fr = (az - i.astype(F)).astype(F)
    return (x * _fma32(fr, dt[i], t0[i])).astype(F)


def sweep_points():
    x = np.linspace(-8.0, 8.0, 262144).astype(F)
    extra = np.array([6, -6, 50, -50, 224, -224, 1000, -1000, 5.65, -5.65, 5.66, -5.66, 223.9, 225], F)
    return np.concatenate([x, extra])


@pytest.fixture(scope="module")
def sweep():
    x = sweep_points()
    xd = x.astype(np.float64)
    return x, xd, FR.two_gelu(xd)


@pytest.mark.parametrize("form", ["e4m3", "fp16"])
def test_gelu_slack_bounds_the_fp32_emulation(sweep, form):
    x, xd, ref = sweep
    emu = (emulate_e4m3_form(x) if form == "e4m3" else emulate_fp16_form(x)).astype(np.float64)
    want = np.minimum(ref, 448.0) if form == "e4m3" else ref
    err = np.abs(emu - want)
    slack = FR.gelu_slack(xd, form)
    ratio = err / slack
    print(f"{form}: max err / slack {np.nanmax(ratio):.4f} at x = {x[np.nanargmax(ratio)]}")
    assert np.all(err <= slack)
    # the bound is tight, not generous: somewhere the emulation uses most of it
    assert np.nanmax(ratio) > 0.5


def test_slack_magnitudes_match_the_kernel_comments():
    # k_gemm.hip: |T error| <= 7.4e-6 (interpolated), <= 1.1e-3 (nearest)
    x = np.linspace(-5.0, 5.0, 20001)
    x = x[np.abs(x) > 0.5]
    rounding = 2.0 ** -21 * FR.T(x)                            # the fp32 roundings' share, per |x|
    assert (FR.gelu_slack(x, "fp16") / np.abs(x) - rounding).max() <= 7.5e-6
    assert (FR.gelu_slack(x, "e4m3") / np.abs(x) - rounding).max() <= 1.11e-3


def test_e4m3_bracket_is_nearly_a_byte(sweep):
    x, xd, ref = sweep
    lo, hi = FR.bracket(ref, FR.gelu_slack(xd, "e4m3"), FR.rnd_e4m3)
    same = np.mean(lo == hi)
    print(f"e4m3 bracket ends equal on {100 * same:.2f} % of the sweep")
    assert same >= 0.95
    got = FR.rnd_e4m3(emulate_e4m3_form(x).astype(np.float64))
    assert np.all((lo <= got) & (got <= hi))
    lo16, hi16 = FR.bracket(ref, FR.gelu_slack(xd, "fp16"), FR.rnd_fp16)
    got16 = FR.rnd_fp16(emulate_fp16_form(x).astype(np.float64))
    assert np.all((lo16 <= got16) & (got16 <= hi16))


@pytest.mark.parametrize("shift", [-1, 1])
def test_brackets_catch_a_node_index_off_by_one(sweep, shift):
    x, xd, ref = sweep
    lo, hi = FR.bracket(ref, FR.gelu_slack(xd, "e4m3"), FR.rnd_e4m3)
    got = FR.rnd_e4m3(emulate_e4m3_form(x, shift=shift).astype(np.float64))
    bad = int(np.sum((got < lo) | (got > hi)))
    print(f"nearest-node index shifted by {shift}: {bad} of {x.size} sweep points leave their bracket")
    assert bad >= 100


# ---- dyadic GEMM operands ------------------------------------------------------------------------
@pytest.mark.parametrize("f8", [True, False])
def test_dyadic_case_is_exact_in_fp32_and_catches_a_dropped_k_step(f8):
    import torch
    M, N, K = 37, 256, 384
    c = FR.dyadic_gemm_case(N, K, M, seed=5, f8=f8)
    Xd, Wd = c["Xd"](), c["Wd"]
    if f8:
        assert np.array_equal(FR.e4m3_values(c["X"].numpy()), Xd.numpy())
        assert np.array_equal(FR.dequant_rows(c["W"].numpy(), c["wexp"].numpy()), Wd.numpy())
        assert set(np.unique(c["wexp"].numpy())) >= {95, 127, 135}
        assert not c["W"].numpy()[0].astype(bool).any() and c["wexp"][0] == 127    # the zero row
    else:
        assert torch.equal(c["X"].double(), Xd) and torch.equal(c["W"].double(), Wd)
    for epi, kw in (("lnf", dict(colsum=c["colsum"], mr=c["mr_lnf"])),
                    ("res", dict(R=c["R_res"])),
                    ("lnr", dict(R=c["R_lnr"], mr=c["mr_lnr"], gamma=c["gamma"]))):
        ref = FR.fold_ref_t(epi, Xd, Wd, c["bias"], **kw)
        assert torch.equal(ref.float().double(), ref)              # representable: nothing to round
        # an fp32 evaluation in another order (k descending, the epilogue term first) is identical
        k32 = {k: (v.float() if v.dtype != torch.float32 else v) for k, v in kw.items()}
        acc = torch.zeros(M, N)
        for k0 in range(K - 64, -1, -64):
            acc = acc + Xd[:, k0:k0 + 64].float() @ Wd[:, k0:k0 + 64].float().T
        if epi == "lnf":
            got = k32["mr"][:, 1:2] * (acc - k32["mr"][:, 0:1] * k32["colsum"][None]) + c["bias"][None]
        elif epi == "res":
            got = (k32["R"] + c["bias"][None]) + acc
        else:
            got = ((k32["R"] - k32["mr"][:, 0:1]) * k32["mr"][:, 1:2]) * k32["gamma"][None] + c["bias"][None] + acc
        assert torch.equal(got.double(), ref), epi
        # a reference without the last 128-byte K-step differs in fp16 on most outputs
        step = 128 if f8 else 64
        short = FR.fold_ref_t(epi, Xd[:, :K - step], Wd[:, :K - step], c["bias"], **kw)
        differ = (short.half() != ref.half()).float().mean().item()
        print(f"f8 {f8} {epi}: dropping the last K-step changes {100 * differ:.1f} % of the fp16 outputs")
        assert differ > 0.25
    y = FR.fold_ref_t("lnr", Xd, Wd, c["bias"], R=c["R_lnr"], mr=c["mr_lnr"], gamma=c["gamma"])
    assert float(y.abs().max()) < 65504.0
    span = y.half().double().reshape(M, N // 128, 128)
    assert float(((span - span.mean(-1, keepdim=True)) ** 2).sum(-1).min()) > 0.0   # no span with M2 = 0
    ratio = (c["R_lnr"].double().mean(1).abs() / c["R_lnr"].double().std(1)).max().item()
    assert ratio >= 100.0
