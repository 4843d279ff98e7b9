"""CPU: the rounding model of the fp32-residual embedders (oracle/encoder_ref.py fp16_operands)
against the fp64 oracle, on the inputs the shipped-mode GPU tests of tests/test_gpu_encoder.py use
(tests/embed_cases.py).

Two conditions on the INPUTS, checked on the reference alone:
  * embed(fp64 weights, fp16_operands=True) vs embed(fp64 weights) <= 7e-4 relative: the chosen
    weights and shapes are ones the rounding design (fp16 tables, GEMM operands, q / k / v and
    softmax probabilities; fp32 accumulation, residual stream and LayerNorm) passes with room under
    the device's 1e-3 bar, so a device result near 1e-3 on them points at a kernel;
  * the fp32 oracle vs the fp64 oracle <= 1e-5: either is a reference far below the bar.
If a seed breaks the first, the seed or the style changes, not the cap.
"""
import numpy as np
import pytest
import torch

import embed_cases as EC
from oracle import encoder_ref as R


def _groups():
    seen = []
    for c in EC.CASES + (EC.BIG,):
        for style in c.styles:
            if (c.model, style) not in seen:
                seen.append((c.model, style))
    return seen


def _inputs(case):
    if case is EC.BIG:           # the three compared sequences only
        ids, mask = EC.batch(case)
        rows = list(EC.BIG_ROWS)
        return ids[rows], mask[rows]
    return EC.batch(case)


def test_outlier_style_is_test_style_at_all_but_three_dims():
    from super_rag_amd.encoder import random_weights
    spec = EC.spec_of("bge-small-en")
    a, b = random_weights(spec, 3, "test"), random_weights(spec, 3, "outlier")
    last = f"encoder.layer.{spec.layers - 1}.output.LayerNorm."
    dims = None
    for k in a:
        if "LayerNorm" not in k or k.startswith(last):
            np.testing.assert_array_equal(a[k], b[k])
            continue
        d = np.flatnonzero(a[k] != b[k])
        assert d.size == 3 and (dims is None or np.array_equal(d, dims)), k
        dims = d
        if k.endswith("weight"):
            np.testing.assert_allclose(b[k][d], 20.0 * a[k][d], rtol=1e-6)
        else:
            np.testing.assert_allclose(np.abs(b[k][d]), np.abs(a[k][d]) + 1.0, rtol=1e-6)
            assert np.array_equal(np.sign(b[k][d]), np.where(a[k][d] < 0, -1.0, 1.0))


@pytest.mark.parametrize("model,style", _groups())
def test_rounding_model_within_cap_on_gpu_test_inputs(model, style):
    spec = EC.spec_of(model)
    cfg = EC.ref_cfg(spec)
    w = EC.weights(model, style)
    w64 = EC.torch_weights(w, torch.float64)
    for case in EC.CASES + (EC.BIG,):
        if case.model != model or style not in case.styles:
            continue
        ids, mask = _inputs(case)
        with torch.no_grad():
            h64 = R.encode_hidden(cfg, w64, ids, mask)
            h16 = R.encode_hidden(cfg, w64, ids, mask, fp16_operands=True)
            h32 = R.encode_hidden(cfg, w, ids, mask)
        assert h64.dtype == torch.float64 and h16.dtype == torch.float64 and h32.dtype == torch.float32
        for pool in case.pools:
            ref = R.pool_hidden(h64, mask, pool)
            e16 = EC.rel(R.pool_hidden(h16, mask, pool), ref).max()
            e32 = EC.rel(R.pool_hidden(h32, mask, pool).astype(np.float64), ref).max()
            print(f"{case.name} {style} {pool}: fp16-operand model vs fp64 {e16:.2e}, "
                  f"fp32 oracle vs fp64 {e32:.2e}")
            assert e16 <= EC.REF_CAP, (case.name, style, pool, e16)
            assert e32 <= EC.FP32_CAP, (case.name, style, pool, e32)
            assert e16 > 10 * e32      # the restatement does round: not the plain oracle again
