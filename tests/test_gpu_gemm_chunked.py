"""GPU parity of the K-chunked / split-K form of the 128 x 128 GEMM (k_gemm.hip KCHUNK: the form
every embedder GEMM below the persistent threshold runs) against an fp64 reference of the same op,
through sr_diag_gemm_chunked of the diagnostic library, which lends the chunk workspace the way
Encoder::forward's lin() does (sr_diag_gemm never does, so tests/test_gpu_gemm.py cannot reach it).

Host formula of launch_gemm_variant (restated in _plan; every case asserts the values it names, and
checks on the device that the workspace was / was not written, so a retune of the host heuristic
cannot silently empty a case):

    tiles  = (N / 128) ceil(M / 128)
    nchunk = ceil((K / 64) / 6)
    split  iff nchunk >= 2, tiles <= 128 and nchunk tiles 64 KiB <= ws_bytes
    cpg    = ceil(nchunk / min(nchunk, ceil(512 / tiles)))     chunks per workgroup
    groups = ceil(nchunk / cpg)                                blockIdx.y

Per case:
  1. |y - ref| <= 2e-3 max(1, max|ref|) with ref = epi(X W^T + b (+ R)) in fp64 (the band of
     tests/test_gpu_gemm.py).  With X ~ 0.5 N(0, 1) and W ~ 0.02 N(0, 1) one K-step (64 products)
     contributes about sqrt(64) 0.5 0.02 = 0.08 per output, 10x the band at these shapes: a dropped,
     doubled or misplaced K-step or chunk cannot pass.
  2. Split-weight cases (K = 2 x_k, the activation column wraps at K-step x_k / 64) use
     W2 = [A | Bm] of two INDEPENDENT fp16 matrices and expect X (A + Bm)^T: a wrap at the wrong
     K-step multiplies part of Bm by the wrong X columns and moves the outputs by ~0.08 per K-step.
     (A true hi / lo pair could not show it: its lo half moves the result by ~2e-5.  One true
     hi / lo case keeps the assertions of test_gemm_split_weights_match_fp32_weights.)
  3. Where the call splits, the same call with a workspace too small to split (64 KiB: non-null,
     below nchunk tiles 64 KiB) returns byte-identical Y: the design's claim that an embedding
     never depends on the batch it was coalesced into (k_gemm.hip, comment above KCHUNK).
  4. Guard bands: the NaN rows of Y past M are untouched; the workspace past
     nchunk tiles 16384 floats keeps its fill, all of it when the call does not split, and the
     partial tiles before that bound are all written when it does.
"""
import pytest

pytestmark = pytest.mark.gpu

MiB = 1 << 20
KCHUNK, SPLIT_MAX_TILES, TILE_BYTES = 6, 128, 65536


def _cdiv(a, b):
    return -(-a // b)


def _plan(M, N, K, ws_bytes):
    """(tiles, nchunk, cpg, groups) of launch_gemm_variant's 128 x 128 branch; cpg 0 = not split."""
    tiles = (N // 128) * _cdiv(M, 128)
    nchunk = _cdiv(K // 64, KCHUNK)
    if nchunk >= 2 and tiles <= SPLIT_MAX_TILES and nchunk * tiles * TILE_BYTES <= ws_bytes:
        cpg = _cdiv(nchunk, min(nchunk, _cdiv(512, tiles)))
        return tiles, nchunk, cpg, _cdiv(nchunk, cpg)
    return tiles, nchunk, 0, 1


def _epilogue(torch, ref, epi, R):
    if epi == 1:
        return torch.nn.functional.gelu(ref)
    if epi in (2, 4):
        return ref + R.double()
    if epi == 3:
        return torch.tanh(ref)
    return ref


def _call(torch, epi, X, W, b, R, M, N, K, split_w, ws, ws_bytes):
    """One sr_diag_gemm_chunked call into a fresh NaN-guarded Y; returns (Y[:M], guard rows)."""
    from super_rag_amd import _native as NT
    Yall = torch.full((M + 32, N), float("nan"), device=X.device,
                      dtype=torch.float32 if epi in (2, 3) else torch.float16)
    Y = Yall[:M]
    NT.call_diag("sr_diag_gemm_chunked", 0x100 if split_w else 0, epi, X.data_ptr(), X.stride(0),
                 W.data_ptr(), b.data_ptr(), R.data_ptr() if R is not None else None,
                 R.stride(0) if R is not None else 0, Y.data_ptr(), Y.stride(0), M, N, K,
                 ws.data_ptr(), ws_bytes, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return Y, Yall[M:]


def _operands(torch, epi, M, N, K, split_w, seed):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    x_k = K // 2 if split_w else K
    X = (torch.randn(M, x_k, device=dev, generator=g) * 0.5).half()
    W = (torch.randn(N, K, device=dev, generator=g) * 0.02).half()   # split: [A | Bm], independent
    b = torch.randn(N, device=dev, generator=g) * 0.1
    R = None
    if epi == 2:
        R = torch.randn(M, N, device=dev, generator=g)
    elif epi == 4:
        R = torch.randn(M, N, device=dev, generator=g).half()
    return X, W, b, R


def _check(epi, M, N, K, split_w, ws_bytes, want, seed):
    """Run one case; returns (max |err|, band).  want = the (tiles, nchunk, cpg, groups) the case
    claims to exercise."""
    import torch
    plan = _plan(M, N, K, ws_bytes)
    assert plan == want, f"host formula gives {plan}, the case names {want}"
    tiles, nchunk, cpg, groups = plan
    X, W, b, R = _operands(torch, epi, M, N, K, split_w, seed)
    ws = torch.full((ws_bytes // 4,), float("nan"), device=X.device)
    Y, guard = _call(torch, epi, X, W, b, R, M, N, K, split_w, ws, ws_bytes)
    assert torch.isnan(guard).all().item(), "rows past M were written"
    used = nchunk * tiles * (TILE_BYTES // 4) if cpg else 0
    assert torch.isnan(ws[used:]).all().item(), "workspace written past the partial tiles"
    assert not torch.isnan(ws[:used]).any().item(), "a partial tile of a split call was not written"
    x_k = K // 2 if split_w else K
    Weff = W.double() if not split_w else W[:, :x_k].double() + W[:, x_k:].double()
    ref = _epilogue(torch, X.double() @ Weff.T + b.double(), epi, R)
    err = (Y.double() - ref).abs().max().item()
    tol = 2e-3 * max(1.0, ref.abs().max().item())
    if cpg:   # the unsplit chunked sums of the same call: bit-identical
        small = 65536
        assert small < nchunk * tiles * TILE_BYTES
        ws.fill_(float("nan"))
        Y1, guard1 = _call(torch, epi, X, W, b, R, M, N, K, split_w, ws, small)
        assert torch.isnan(guard1).all().item(), "rows past M were written (unsplit)"
        assert torch.isnan(ws).all().item(), "the unsplit call wrote to the workspace"
        assert torch.equal(Y1, Y), (f"split-K differs from the unsplit chunked sums in "
                                    f"{int((Y1 != Y).sum().item())} outputs")
    return err, tol


# name: (M, N, K, split weights, ws_bytes, (tiles, nchunk, cpg, groups), epilogues)
EMB = (0, 1, 2)            # the embedders' three: bias, bias + GELU, bias + fp32 residual
ALL = (0, 1, 2, 3, 4)
CASES = {
    # N % 256 != 0 (bge-small's 384 / 1152 can never leave this kernel); M ragged inside one tile
    "small_n_split": (77, 384, 1536, False, 64 * MiB, (3, 4, 1, 4), EMB),
    "small_n_one_chunk": (300, 1152, 384, False, 64 * MiB, (27, 1, 0, 1), EMB),
    # several chunks per workgroup (bge-base FFN2 at 49-85 coalesced queries); ragged last m-tile
    "cpg2": (1998, 768, 3072, False, 64 * MiB, (96, 8, 2, 4), ALL),
    # the edge of the split: 128 tiles split, 136 do not
    "edge_split": (2048, 1024, 3072, False, 64 * MiB, (128, 8, 2, 4), EMB),
    "edge_unsplit": (2049, 1024, 3072, False, 64 * MiB, (136, 8, 0, 1), EMB),
    # 16 chunks in 6 groups of 3: the last group holds one chunk; x_k = 3072: wrap at step 48
    "ragged_group": (1998, 768, 6144, True, 128 * MiB, (96, 16, 3, 6), ALL),
    # the same shape with the workspace of the encoder (96 MiB needed): unsplit chunked sums
    "ws_fall_through": (1998, 768, 6144, True, 64 * MiB, (96, 16, 0, 1), EMB),
    # 32 K-steps = chunks 6,6,6,6,6,2; x_k = 1024: the wrap at step 16 lies inside chunk 12..17
    "wrap_in_chunk": (600, 1024, 2048, True, 64 * MiB, (40, 6, 1, 6), EMB),
    # bge-m3 FFN2: 128 K-steps = 21 chunks of 6 + one of 2; wrap at step 64 inside chunk 60..65
    "m3_ffn2": (600, 1024, 8192, True, 64 * MiB, (40, 22, 2, 11), EMB),
    # two K-steps, one chunk
    "k128": (130, 256, 128, False, 64 * MiB, (4, 1, 0, 1), EMB),
}


def _params():
    for name, case in CASES.items():
        for epi in case[-1]:
            yield pytest.param(name, epi, id=f"{name}-epi{epi}")


@pytest.mark.parametrize("name,epi", list(_params()))
def test_chunked_gemm_against_fp64(name, epi):
    M, N, K, split_w, ws_bytes, want, _ = CASES[name]
    if name == "ragged_group":
        assert want[1] - (want[3] - 1) * want[2] == 1      # the last group holds one chunk
    if name in ("wrap_in_chunk", "m3_ffn2"):
        wrap = K // 2 // 64                                # inside a chunk, and a ragged last chunk
        assert wrap % KCHUNK != 0 and (K // 64) % KCHUNK == 2
    if name == "ws_fall_through":
        assert want[1] * want[0] * TILE_BYTES == 96 * MiB > ws_bytes
    err, tol = _check(epi, M, N, K, split_w, ws_bytes, want, seed=M + K + epi)
    print(f"{name} epi{epi} {M}x{N}x{K} (tiles, nchunk, cpg, groups) {want}: max|err| {err:.3e}, "
          f"band {tol:.1e}")
    assert err <= tol, f"{name} epi{epi} {M}x{N}x{K}: max|err| {err:.3e} > {tol:.1e}"


def test_chunked_gemm_true_hi_lo_weights():
    """W2 = [fp16(W) | fp16(W - fp16(W))] at the wrap-in-chunk shape, fp32-residual epilogue, split
    over K: X W^T with the fp32 weights (the assertions of
    test_gemm_split_weights_match_fp32_weights), and bit-identical unsplit."""
    import torch
    dev = torch.device("cuda", 0)
    M, N, K, epi = 600, 1024, 1024, 2
    ws_bytes = 64 * MiB
    assert _plan(M, N, 2 * K, ws_bytes) == (40, 6, 1, 6)
    g = torch.Generator(device=dev).manual_seed(5)
    X = (torch.randn(M, K, device=dev, generator=g) * 0.5).half()
    W = torch.randn(N, K, device=dev, generator=g) * 0.02
    hi = W.half()
    lo = (W - hi.float()).half()
    W2 = torch.cat([hi, lo], 1).contiguous()
    b = torch.randn(N, device=dev, generator=g) * 0.1
    R = torch.randn(M, N, device=dev, generator=g)
    ws = torch.full((ws_bytes // 4,), float("nan"), device=dev)
    Y, guard = _call(torch, epi, X, W2, b, R, M, N, 2 * K, True, ws, ws_bytes)
    assert torch.isnan(guard).all().item()
    assert not torch.isnan(ws[:6 * 40 * 16384]).any().item()      # it did split
    Y1, _ = _call(torch, epi, X, W2, b, R, M, N, 2 * K, True, ws, 65536)
    assert torch.equal(Y1, Y)
    ref = X.double() @ W.double().T + b.double() + R.double()
    ref_h = X.double() @ hi.double().T + b.double() + R.double()   # what unsplit fp16 weights give
    err = (Y.double() - ref).abs().max().item()
    err_h = (ref_h - ref).abs().max().item()
    out_round = 2 ** -23 * ref.abs().max().item()
    print(f"true hi/lo 600x1024x2048 epi2: max|err| {err:.3e}, fp16 weights alone {err_h:.3e}")
    assert err <= out_round + 2e-5, f"{err:.3e}"
    assert err < 0.1 * err_h, (err, err_h)
