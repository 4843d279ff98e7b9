"""Host references for the attention kernels (numpy fp64; no GPU needed to import):

selector cases   operands for which softmax is exactly one-hot, so ctx must equal one V row bit for bit
uniform cases    every score 0, so ctx is the mean of the live V rows
attention_bound  fp64 reference + derived per-element bound for random operands (K5 family, K5c)
fold_case / fold_ref   the same three for cls_attn_fold (z' as an fp16 hi + lo pair)
emu_*            fp32 / fp16 numpy emulations of the kernels' documented rounding points, with the
                 mutations tests/test_attn_ref.py counts

Selector cases.  Keys are +-1 codes (the Hadamard rows and their negatives while they last, seeded
random codes beyond), K_j = ck code[j]; query t is c code[a_t] (+ (c/2) code[b_t]: a decoy when key
a_t is masked and b_t is live; a key mask shifted by one index then selects another row).  selector_check
computes, in fp64 from the fp16 operands, every query's scores in log2 units (nats x log2 e for the
fold kernel), the winner among the live keys and its gap to the runner-up, and asserts gap >= 160.
Why 160: exp2 of anything below -150 is 0 in fp32 with or without denormals (the smallest denormal
is 2^-149), so every other weight is exactly 0, the online-softmax rescale of whatever was
accumulated before the winner's block is exactly 0 (or multiplies zeros), l == 1 and ctx == V[winner]
as stored in fp16.  The ten units between 150 and 160 cover the kernels' own fp32 rounding of the
scores: the selector dot products are integers below 2^24 (exact), the scale multiply is off by
2^-24 relative of a score below 2^15, i.e. < 2^-9; the fold cases assert that twice their fp32 score
error bound (below: winner and runner-up) stays under those ten units.  This is a condition on the inputs, checked on the CPU: not a tolerance.

Dyadic operands of K5c.  X rows are signed one-hot patterns repeated (with a per-block sign) in every
64-column block; W, bias, colsum are multiples of 2^-3 .. 2^-6, mu of 2^-6, rstd in {1/2, 1, 2}: every
product and epilogue term is a multiple of 2^-10 and every sum of magnitudes is below 2^14, far
under 2^24 quanta, so Q, K, V are exact in fp32 in any order and round to fp16 once (asserted).

Derived bound for random operands (nothing fitted to a run).  Q*, K*, V* are the fp64 values of the
epilogue on the fp16 operands; the kernel holds fp16 roundings of fp32 values:
  dQ = acc + 2^-11 (|Q*| + acc) + 2^-25,   acc = K 2^-23 rstd sum|x w| + 2^-22 (rstd (sum|x w| + |mu c|) + |b|)
(K-term: fp32 accumulation in any order; second: the epilogue's FMAs; 2^-11: fp16 rounding; 2^-25:
fp16 subnormals), likewise dK, dV; all zero for the kernels that read qkv.  Scores in nats:
  E_s(t, j) = scale [ dQ_t.|K_j| + |Q_t|.dK_j + dQ_t.dK_j ] + (d_h + 4) 2^-24 scale (|Q_t|+dQ_t).(|K_j|+dK_j)
(operand errors; fp32 dot product, scale multiply, subtraction of the row maximum), E_t = max over
live j.  A score error e changes a weight by the factor exp(e) and the softmax ratio, to first order,
by sum_j p_j e_j (v_j - ctx): at most 2 E_t sum p |v|.  With P rounded to fp16 (2^-11; below 2^-14
absolute 2^-25), the hardware exp2 within one ulp (eps_exp = 2^-23: the GCN / CDNA ISA documents give
V_EXP_F32 one ulp of accuracy), the fp32 accumulation of P.V and of l and the 1 / l multiply
((S + 4) 2^-24), and the output rounded to fp16:
  |ctx_e - ref_e| <= sum_j p_j |v_je| (2 E_t + 2^-11 + eps_exp + (S + 4) 2^-24) + sum_j p_j dV_je
                     + 2^-25 sum_{live j} |v_je| + half an fp16 ulp at |ref_e| + (all of the former).
Fold kernel: v_j = rstd_j (u_j - mu_j), score_j = rstd_j (w.u_j - mu_j sum w) / 8 with w, u fp16 (exact):
  E_s(h, j) = rstd_j / 8 [ D 2^-23 (|w_h|.|u_j| + |mu_j| sum|w_h|) + 2^-22 (|w_h.u_j| + |mu_j alpha_h|) ] + 2^-23 |s_j|,
__expf(x) = exp2(x log2 e) adds |x| 2^-23 to eps_exp per weight; p' = p rstd / l (3 x 2^-24); z' is
the difference of two separately accumulated sums, sum p' u and sig = sum p' mu, each off by
(S + 8) 2^-24 of its magnitudes (and 2^-22 of sum p'|u| in the single-read form, whose p' is an fp16
hi + lo pair); the output pair keeps z' to 2^-22 relative + 2^-24:
  |z'_e - ref_e| <= sum_j p_j |v_je| (2 E_h + eps_j) + |ref_e| sum_j p_j eps_j
                    + ((S + 8) 2^-24 [+ 2^-22]) sum_j p'_j (|u_je| + |mu_j|) + 2^-22 |ref_e| + 2^-24.
Uniform cases: every p = 1 exactly, sum V exact in fp32 (dyadic), so only 1 / l and one multiply
round (2^-22 relative covers both): fp16(ref) exactly when n_live is a power of two, else the fp16
rounding of something in ref (1 +- 2^-22) (uniform_bracket).
"""
import functools
import math

import numpy as np

LOG2E = 1.4426950408889634
GAP_MIN = 160.0
EPS_EXP = 2.0 ** -23
U16 = 2.0 ** -11


def f16(x):
    return np.asarray(x, np.float64).astype(np.float16)


def r16(x):
    """fp64 -> fp16 (one rounding, nearest even) -> fp64."""
    return f16(x).astype(np.float64)


def half_ulp16(a):
    a = np.maximum(np.abs(a), 2.0 ** -14)
    return np.ldexp(1.0, np.floor(np.log2(a)).astype(np.int32) - 11)


def hadamard(n):
    H = np.array([[1.0]])
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    assert H.shape[0] == n
    return H


def codes(n, dh, seed):
    """n distinct +-1 codes of dh dimensions: Hadamard rows then their negatives (pairwise dot <= 0;
    code[i + dh] = -code[i]) while n <= 2 dh, seeded random codes beyond.  The gap (dh - the largest
    dot product of two different codes) is asserted positive; selector_check asserts what follows."""
    if n <= 2 * dh:
        H = hadamard(dh)
        C = np.concatenate([H, -H])[:n]
    else:
        C = np.random.default_rng(seed).choice([-1.0, 1.0], (n, dh))
    D = C @ C.T
    np.fill_diagonal(D, -dh)
    assert n == 1 or dh - D.max() >= 1, "codes: two keys share a code"
    return C


# pattern ids of the key masks: 0 holes (key 0 live), 1 ragged prefix, 2 fully masked, 3 length 1,
# 4 full, 5 holes with key 0 masked and the last key live
def pattern_masks(pat_ids, S, seed):
    rng = np.random.default_rng(seed)
    out = []
    for p in pat_ids:
        m = np.zeros(S, bool)
        if p == 0:
            m = rng.random(S) < 0.6
            m[0] = True
        elif p == 1:
            m[:int(rng.integers(2, max(S, 3)))] = True
        elif p == 3:
            m[0] = True
        elif p == 4:
            m[:] = True
        elif p == 5:
            m = rng.random(S) < 0.75
            m[0], m[S - 1] = False, True
        out.append(m)
    return np.stack(out)


def v_values(B, S, heads, dh):
    """Small dyadic fp16 V rows (multiples of 2^-6 below 16), a different 64-vector for every
    (token, head) of a sequence (asserted), no two neighbouring dimensions alike."""
    b, t, h, e = np.ix_(np.arange(B), np.arange(S), np.arange(heads), np.arange(dh))
    # even dims carry the token (131 t mod the prime 2039), odd dims the head beside it
    v = (np.where(e % 2 == 0, t * 131 + e * 3 + b * 29, h * 127 + t * 3 + e * 5 + b * 29) % 2039 - 1019) / 64.0
    assert np.unique(v[0].reshape(S * heads, dh), axis=0).shape[0] == S * heads, "v_values: two rows coincide"
    assert np.all(r16(v) == v)
    return v


def selector_check(Q, K, V, masks, scale_log2, queries=None, gap_min=GAP_MIN):
    """Q, K, V [B, S, H, dh] fp64 (the values the kernel holds in fp16), masks [B, S] bool.  Every
    query row t with queries[b, t] (default: all) of a sequence with a live key must have one live
    key ahead of every other by gap_min log2 units.  Returns (expect [B, S, H, dh] = V[winner], zero
    rows for sequences without a live key; min gap; decoys = queries whose best key overall is
    masked; winner [B, H, S])."""
    B, S, H, dh = Q.shape
    expect = np.zeros_like(V)
    winner = np.full((B, H, S), -1)
    gmin, decoys = np.inf, 0
    for b in range(B):
        live = masks[b]
        if not live.any():
            continue
        sc = np.einsum("the,jhe->htj", Q[b], K[b]) * scale_log2
        raw = sc.argmax(-1)
        sc[:, :, ~live] = -np.inf
        w = sc.argmax(-1)                                             # [H, S]
        top = np.take_along_axis(sc, w[..., None], -1)[..., 0]
        np.put_along_axis(sc, w[..., None], -np.inf, -1)
        gap = top - sc.max(-1)                                        # inf with one live key
        sel = np.ones(S, bool) if queries is None else queries[b]
        assert np.all(gap[:, sel] >= gap_min), f"selector_check: gap {gap[:, sel].min():.1f} < {gap_min}"
        gmin = min(gmin, float(gap[:, sel].min()))
        decoys += int((~live[raw])[:, sel].sum())
        winner[b] = w
        for h in range(H):
            expect[b, :, h] = V[b, w[h], h]
    return expect, gmin, decoys, winner


@functools.lru_cache(maxsize=None)
def selector_qkv(S, heads, dh, pat_ids, seed, uniform=False, c=32.0, ck=32.0):
    """A selector (or uniform: K = 0) case written straight into qkv [B, S, 3 d] fp16.  Returns a dict:
    qkv, mask (int32), expect (fp16 [B, S, d]; uniform: ref fp64 and nlive), gap_min, decoys."""
    masks = pattern_masks(pat_ids, S, seed)
    B, d = len(pat_ids), heads * dh
    rng = np.random.default_rng(seed + 1)
    C = codes(S, dh, seed)
    D = C @ C.T
    scale_log2 = LOG2E / math.sqrt(dh)
    V = v_values(B, S, heads, dh)
    Q, K = np.zeros_like(V), np.zeros_like(V)
    for b in range(B):
        live = masks[b]
        li, mi = np.flatnonzero(live), np.flatnonzero(~live)
        for h in range(heads):
            kid = rng.permutation(S)                                  # key j carries code kid[j]
            K[b, :, h] = ck * C[kid]
            if li.size == 0:
                Q[b, :, h] = c * C[kid[rng.integers(0, S, S)]]
                continue
            Dk = D[np.ix_(kid, kid)]
            todo = np.arange(S)
            for _ in range(200):
                n = todo.size
                dec = (rng.random(n) < 0.25) & (mi.size > 0)
                a = np.where(dec, rng.choice(mi if mi.size else li, n), rng.choice(li, n))
                bb = rng.choice(li, n)
                sc = c * ck * (Dk[a] + 0.5 * dec[:, None] * Dk[bb]) * scale_log2
                sc[:, ~live] = -np.inf
                w = sc.argmax(-1)
                top = sc[np.arange(n), w].copy()
                sc[np.arange(n), w] = -np.inf
                ok = (w == np.where(dec, bb, a)) & (top - sc.max(-1) >= GAP_MIN + 8)
                Q[b, todo[ok], h] = c * C[kid[a[ok]]] + (0.5 * c) * dec[ok, None] * C[kid[bb[ok]]]
                todo = todo[~ok]
                if todo.size == 0:
                    break
            assert todo.size == 0, "selector_qkv: no selector query found"
    if uniform:
        K[:] = 0.0
    qkv = np.stack([Q, K, V], 2).reshape(B, S, 3 * d)
    assert np.all(r16(qkv) == qkv)
    out = dict(qkv=f16(qkv).reshape(B * S, 3 * d), mask=masks.astype(np.int32), masks=masks, B=B, S=S, d=d,
               heads=heads, dh=dh)
    if uniform:
        out["ref"], out["nlive"] = uniform_ref(V, masks), masks.sum(1)
    else:
        exp, gmin, decoys, win = selector_check(Q, K, V, masks, scale_log2)
        out.update(expect=f16(exp).reshape(B, S, d), gap_min=gmin, decoys=decoys, winner=win)
    return out


def uniform_ref(V, masks):
    """Mean of the live V rows per (sequence, head, dim), fp64 (zero without a live key): [B, 1, H, dh]."""
    n = masks.sum(1)
    s = np.einsum("bj,bjhe->bhe", masks.astype(np.float64), V)
    return (s / np.maximum(n, 1)[:, None, None])[:, None]


def uniform_bracket(ref, nlive):
    """(lo, hi) fp16 per element for a uniform case: fp16(ref) for a power-of-two n_live (lo == hi),
    else the roundings of ref (1 -+ 2^-22) -- they differ, by one ulp, only where that interval
    straddles an fp16 rounding boundary."""
    ref = np.asarray(ref, np.float64)
    n = np.asarray(nlive).reshape((-1,) + (1,) * (ref.ndim - 1))
    pow2 = (n & (n - 1)) == 0
    slack = np.where(pow2, 0.0, 2.0 ** -22) * np.abs(ref)
    return f16(ref - slack), f16(ref + slack)


# ---- K5c: the selector realised through the fused GEMM -------------------------------------------
def k5c_epilogue(acc, epi, bias, colsum, mu, rstd):
    """fp64 value of the K5c epilogue (epi 0: acc + b; 5: rstd (acc - mu c) + b); mu, rstd per row."""
    if epi == 0:
        return acc + bias[None]
    return rstd[:, None] * (acc - mu[:, None] * colsum[None]) + bias[None]


@functools.lru_cache(maxsize=None)
def k5c_case(heads, pat_ids, epi, seed, lda_pad=0, uniform=False, junk_seed=0, c=16.0, ck=16.0):
    """Selector (or uniform) operands of sr_diag_qkv_attention, S = 128, d = 64 heads.  Sequence b uses
    key-mask pattern pat_ids[b]; its masked tokens hold junk (junk_seed) in X and mr, sized so that
    Q, K, V stay finite in fp16 (an infinite V would meet its zero weight as NaN, in the unfused pair
    as well).  Returns X [B 128, lda] (gap columns poisoned), W, bias, colsum, mr, mask, expect
    [B, 128, d] fp16 (uniform: ref, nlive), check [B, 128] = the live query rows."""
    S, dh = 128, 64
    d, B, nblk = 64 * heads, len(pat_ids), heads
    lda = d + lda_pad
    upat = sorted(set(pat_ids))
    pm = dict(zip(upat, pattern_masks(tuple(upat), S, seed)))
    rng = np.random.default_rng(seed + 2)
    C = codes(128, 64, 0)
    sgn = np.where(np.arange(S) < 64, 1.0, -1.0)
    idx = np.arange(S) % 64
    lnf = epi == 5
    # per-pattern row statistics of the live tokens (dyadic): rstd in {1/2, 1, 2}, mu = im 2^-6, im != 0
    st = {p: (rng.choice([-1, 1], S) * rng.integers(1, 17, S) * 2.0 ** -6 * lnf,
              rng.choice([0.5, 1.0, 2.0], S) if lnf else np.ones(S)) for p in upat}
    bias = rng.choice([-1, 1], 3 * d) * rng.integers(1, 17, 3 * d) * 2.0 ** -6
    colsum = rng.choice([-1, 1], 3 * d) * rng.integers(1, 9, 3 * d) * 0.25 * lnf
    G = np.zeros((3, heads, 64, 64))                                   # [segment, head, dim, column]
    scale_log2 = LOG2E / 8.0
    if uniform:
        bias[d:2 * d] = 0.0
        colsum[d:2 * d] = 0.0
    e_, i_ = np.ix_(np.arange(64), np.arange(64))
    for h in range(heads):
        G[2, h] = ((i_ * 67 + e_ * 5 + h * 13) % 251 - 125) / 8.0
        kid = rng.permutation(64)
        flip = rng.integers(0, 2, 64) * 64
        kcode = np.concatenate([kid + flip, (kid + flip + 64) % 128])  # token t carries code kcode[t]
        if not uniform:
            G[1, h] = ck * C[kcode[:64]].T
        Kp = {p: r16(k5c_epilogue(sgn[:, None] * G[1, h].T[idx], epi, bias[d + 64 * h:d + 64 * h + 64],
                                  colsum[d + 64 * h:d + 64 * h + 64], *st[p])) for p in upat}
        bq, cq = bias[64 * h:64 * h + 64], colsum[64 * h:64 * h + 64]
        for i in range(64):
            for _ in range(2000):
                a, b2 = rng.integers(0, 128, 2)
                col = c * C[kcode[a]] + 0.5 * c * C[kcode[b2]]
                ok = a % 64 != b2 % 64
                for p in upat:
                    if not ok:
                        break
                    live = pm[p]
                    for t in (i, i + 64):
                        if uniform or not live[t]:
                            continue
                        q = r16(k5c_epilogue(sgn[t] * col[None], epi, bq, cq, st[p][0][t:t + 1], st[p][1][t:t + 1]))[0]
                        s = np.sort((Kp[p] @ q * scale_log2)[live])
                        if s.size > 1 and s[-1] - s[-2] < GAP_MIN + 8:
                            ok = False
                if ok:
                    break
            assert ok, "k5c_case: no selector column found"
            G[0, h, :, i] = col
    # W rows [Q; K; V] x d columns: block blk of column 64 blk + i holds rho_blk R[blk], sum_blk R = G
    rho = np.where(np.arange(nblk) % 3 == 1, -1.0, 1.0)
    R = rng.integers(-3, 4, (nblk, 3, heads, 64, 64)) * 0.25
    if uniform:
        R[:, 1] = 0.0
    R[0] = G - R[1:].sum(0)
    W = np.zeros((3 * d, d))
    for blk in range(nblk):
        W[:, 64 * blk:64 * blk + 64] = rho[blk] * R[blk].reshape(3 * d, 64)
    assert np.all(r16(W) == W)
    Xtok = np.zeros((S, d))
    for blk in range(nblk):
        Xtok[np.arange(S), 64 * blk + idx] = sgn * rho[blk]
    # exactness: every term a multiple of 2^-10 (x w: 2^-3; mu c: 2^-8; rstd (..): 2^-9; b: 2^-6), sums
    # of magnitudes far below 2^24 quanta
    mag = 2.0 * (np.abs(W).sum(1).max() + 0.25 * np.abs(colsum).max()) + np.abs(bias).max()
    assert mag < 2.0 ** 24 * 2.0 ** -10
    acc = Xtok @ W.T
    assert np.all(acc == np.rint(acc * 8) / 8)
    jr = np.random.default_rng(1000 + junk_seed)
    X = np.full((B * S, lda), 60000.0)                                  # gap columns: poison
    mr = np.zeros((B * S, 2))
    Q, K, V = (np.zeros((B, S, heads, 64)) for _ in range(3))
    masks = np.stack([pm[p] for p in pat_ids])
    wmax = np.abs(W).sum(1).max()
    jx = 2.0 ** math.floor(math.log2(65504.0 / (2.0 * (wmax + 64.0 * 2.0)) - 1.0))   # |junk x| bound
    for b, p in enumerate(pat_ids):
        live = pm[p]
        mu, rstd = st[p]
        y = k5c_epilogue(acc, epi, bias, colsum, mu, rstd)
        assert np.all(y == np.rint(y * 1024) / 1024)
        y = r16(y).reshape(S, 3, heads, 64)
        Q[b], K[b], V[b] = y[:, 0], y[:, 1], y[:, 2]
        xb = Xtok.copy()
        xb[~live] = r16(jr.uniform(-jx, jx, ((~live).sum(), d)))
        X[b * S:(b + 1) * S, :d] = xb
        mr[b * S:(b + 1) * S] = np.stack([np.where(live, mu, jr.uniform(-64.0, 64.0, S)),
                                          np.where(live, rstd, jr.uniform(0.1, 1.9, S))], 1)
    check = masks | ~masks.any(1, keepdims=True)          # live queries; every row of a fully masked sequence
    out = dict(X=f16(X), W=f16(W), bias=bias.astype(np.float32), colsum=colsum.astype(np.float32),
               mr=mr.astype(np.float32), mask=masks.astype(np.int32), masks=masks, check=check, B=B, S=S,
               d=d, heads=heads, lda=lda, epi=epi, Q=Q, K=K, V=V)
    if uniform:
        out["ref"], out["nlive"] = uniform_ref(V, masks), masks.sum(1)
    else:
        for p in upat:                                                 # live V rows all different
            for h in range(heads):
                b = pat_ids.index(p)
                assert np.unique(V[b, pm[p], h], axis=0).shape[0] == pm[p].sum()
        exp, gmin, decoys, win = selector_check(Q, K, V, masks, scale_log2, queries=masks)
        out.update(expect=f16(exp).reshape(B, S, d), gap_min=gmin, decoys=decoys, winner=win)
    return out


def k5c_random_case(heads, B, epi, seed, lda_pad=0):
    """Random operands of K5c: offset rows (|mean| 3 .. 10 standard deviations) with one outlier
    column, true fp32 row statistics and column sums (LNF), ragged / holed masks."""
    S, d = 128, 64 * heads
    rng = np.random.default_rng(seed)
    M = B * S
    sd = rng.uniform(0.05, 0.5, M) if epi == 5 else np.ones(M)           # epi 0 reads normalised rows
    off = rng.choice([-1, 1], M) * (rng.uniform(3.0, 10.0, M) * sd if epi == 5 else rng.uniform(0.3, 1.0, M))
    x = off[:, None] + sd[:, None] * rng.standard_normal((M, d))
    x[:, int(rng.integers(0, d))] += (20.0 if epi == 5 else 4.0) * sd
    X = np.full((M, d + lda_pad), 60000.0)
    X[:, :d] = r16(x)
    W = r16(rng.standard_normal((3 * d, d)) * (1.2 / math.sqrt(d)))
    bias = rng.standard_normal(3 * d).astype(np.float32) * 0.3
    xr = X[:, :d]
    mu = xr.mean(1)
    rstd = 1.0 / np.sqrt(xr.var(1) + 1e-5)
    mr = np.stack([mu, rstd], 1).astype(np.float32)
    colsum = W.sum(1).astype(np.float32)
    masks = pattern_masks(tuple([0, 1, 4, 5, 3][b % 5] for b in range(B)), S, seed)
    return dict(X=f16(X), W=f16(W), bias=bias, colsum=colsum, mr=mr, mask=masks.astype(np.int32),
                masks=masks, B=B, S=S, d=d, heads=heads, lda=d + lda_pad, epi=epi)


def k5c_qkv_exact(case):
    """(Q*, K*, V*) and (dQ, dK, dV), each [B, S, H, 64] fp64, of a K5c case (module docstring)."""
    d, heads, B, S, epi = case["d"], case["heads"], case["B"], case["S"], case["epi"]
    X = case["X"].astype(np.float64)[:, :d]
    W = case["W"].astype(np.float64)
    b = case["bias"].astype(np.float64)
    cs = case["colsum"].astype(np.float64)
    mu, rstd = case["mr"].astype(np.float64).T
    if epi == 0:
        mu, rstd, cs = np.zeros_like(mu), np.ones_like(rstd), np.zeros_like(cs)
    acc = X @ W.T
    absacc = np.abs(X) @ np.abs(W).T
    y = k5c_epilogue(acc, 5, b, cs, mu, rstd)
    T = rstd[:, None] * (absacc + np.abs(mu[:, None] * cs[None])) + np.abs(b)[None]
    a = d * 2.0 ** -23 * rstd[:, None] * absacc + 2.0 ** -22 * T
    dy = a + U16 * (np.abs(y) + a) + 2.0 ** -25
    y, dy = y.reshape(B, S, 3, heads, 64), dy.reshape(B, S, 3, heads, 64)
    return (y[:, :, 0], y[:, :, 1], y[:, :, 2]), (dy[:, :, 0], dy[:, :, 1], dy[:, :, 2])


def attention_bound(Q, K, V, masks, dh, dQ=None, dK=None, dV=None):
    """fp64 softmax(Q K^T / sqrt(dh) + mask) V and the derived bound (module docstring), [B, S, H, dh]
    each; sequences without a live key: ref 0, bound 0."""
    B, S, H, _ = Q.shape
    z = np.zeros_like(Q)
    dQ, dK, dV = (z if x is None else x for x in (dQ, dK, dV))
    scale = 1.0 / math.sqrt(dh)
    ref, bound = np.zeros_like(V), np.zeros_like(V)
    for b in range(B):
        live = masks[b]
        if not live.any():
            continue
        q, k, v = Q[b], K[b][live], V[b][live]
        dq, dk, dv = dQ[b], dK[b][live], dV[b][live]
        s = np.einsum("the,jhe->htj", q, k) * scale
        aq, ak = np.abs(q), np.abs(k)
        Es = scale * (np.einsum("the,jhe->htj", dq, ak) + np.einsum("the,jhe->htj", aq, dk) +
                      np.einsum("the,jhe->htj", dq, dk)) + \
            (dh + 4) * 2.0 ** -24 * scale * np.einsum("the,jhe->htj", aq + dq, ak + dk)
        Et = Es.max(-1)                                               # [H, S]
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        r = np.einsum("htj,jhe->the", p, v)
        pav = np.einsum("htj,jhe->the", p, np.abs(v))
        rel = 2.0 * Et.T[:, :, None] + U16 + EPS_EXP + (S + 4) * 2.0 ** -24
        bnd = pav * rel + np.einsum("htj,jhe->the", p, dv) + 2.0 ** -25 * np.abs(v).sum(0)[None]
        ref[b], bound[b] = r, bnd + half_ulp16(np.abs(r) + bnd)
    return ref, bound


# ---- cls_attn_fold ---------------------------------------------------------------------------------
def fold_ref(w, U, mu, rstd, live, single_read):
    """w [H, D], U [S, D] fp16 values, mu / rstd [S] (fp32 values), live [S] bool -> (ref z' [H, D],
    bound [H, D], E_h max score error bound in nats [H]) in fp64 (module docstring)."""
    w, U = np.asarray(w, np.float64), np.asarray(U, np.float64)[live]
    mu, rstd = np.asarray(mu, np.float64)[live], np.asarray(rstd, np.float64)[live]
    S, D = live.size, w.shape[1]
    alpha = w.sum(1)
    wu = w @ U.T                                                       # [H, n]
    s = rstd[None] * (wu - mu[None] * alpha[:, None]) * 0.125
    Es = 0.125 * rstd[None] * (D * 2.0 ** -23 * (np.abs(w) @ np.abs(U).T + np.abs(mu)[None] * np.abs(w).sum(1)[:, None]) +
                               2.0 ** -22 * (np.abs(wu) + np.abs(mu[None] * alpha[:, None]))) + 2.0 ** -23 * np.abs(s)
    Eh = Es.max(1)
    x = s - s.max(1, keepdims=True)
    p = np.exp(x)
    p /= p.sum(1, keepdims=True)
    v = rstd[:, None] * (U - mu[:, None])                              # [n, D]
    ref = p @ v
    eps = EPS_EXP + np.abs(x) * 2.0 ** -23 + 3 * 2.0 ** -24
    pp = p * rstd[None]
    cacc = (S + 8) * 2.0 ** -24 + (2.0 ** -22 if single_read else 0.0)
    bound = (p * (2.0 * Eh[:, None] + eps)) @ np.abs(v) + np.abs(ref) * (p * eps).sum(1, keepdims=True) + \
        cacc * (pp @ np.abs(U) + (pp @ np.abs(mu))[:, None]) + 2.0 ** -22 * np.abs(ref) + 2.0 ** -24
    return ref, bound, Eh


def hi_lo(z):
    """The fp16 pair of an fp32-exact z': hi = fp16(z), lo = fp16(z - hi)."""
    hi = f16(z)
    return hi, f16(np.asarray(z, np.float64) - hi.astype(np.float64))


def hi_is_nearest(hi, lo):
    """hi is an fp16 nearest to hi + lo.  Not always fp16(hi + lo): lo = fp16(z' - hi) may round up
    to exactly half an ulp of hi, and hi + lo is then a tie that nearest-even resolves either way
    (the emulation of the documented roundings does this a few times per 10^4 outputs)."""
    h, l = np.asarray(hi, np.float64), np.asarray(lo, np.float64)
    return bool(np.all(np.abs(l) <= np.abs(h + l - (h + l).astype(np.float16).astype(np.float64))))


@functools.lru_cache(maxsize=None)
def fold_selector_case(D, H, S, B, seed):
    """Selector operands of sr_diag_cls_attn_fold: every head selects a different live token (a decoy
    for about a quarter of the heads: its best token overall is masked), z' = rstd_j (u_j - mu_j)
    exactly, so the output pair is hi_lo(z').  u_j = m_j (|m_j| <= 16) + 16 code_j (tiled over D) + delta (multiples
    of 2^-4, |delta| <= 1, different per (token, dim)), w_h = code_a + code_b / 2 + 1/4, so
    alpha_h = sum w_h is D / 4 (+ code sums) and m_j alpha_h, which the kernel must subtract, is far
    above the winner's margin.  mr: mu_j = m_j + im 2^-12, rstd_j in {1/2, 1, 2}; masked tokens hold junk."""
    rng = np.random.default_rng(seed)
    C = codes(S, 64, seed) if S > 128 else codes(128, 64, 0)[rng.permutation(128)[:S]]
    masks = pattern_masks(tuple([0, 1, 5, 4, 3][b % 5] for b in range(B)), S, seed)
    rep = D // 64
    w = np.zeros((B, H, D))
    U = np.zeros((B, S, D))
    mr = np.zeros((B, S, 2))
    exp_hi = np.zeros((B, H, D), np.float16)
    exp_lo = np.zeros((B, H, D), np.float16)
    gmin, decoys, emax = np.inf, 0, 0.0
    j_, i_ = np.ix_(np.arange(S), np.arange(D))
    for b in range(B):
        live = masks[b]
        li, mi = np.flatnonzero(live), np.flatnonzero(~live)
        m = rng.integers(-16, 17, S).astype(np.float64)
        delta = ((j_ * 37 + i_ * 11 + b * 5) % 33 - 16) / 16.0
        u = m[:, None] + 16.0 * np.tile(C, (1, rep)) + delta
        assert np.all(r16(u) == u)
        mu = m + rng.integers(-2048, 2049, S) * 2.0 ** -12
        rstd = rng.choice([0.5, 1.0, 2.0], S)
        wins, free = np.zeros(H, np.int64), list(rng.permutation(li))
        for h in range(H):
            for it in range(2000):
                dec = mi.size > 0 and rng.random() < 0.25
                b2 = int(free[int(rng.integers(0, len(free)))]) if free and it < 100 else int(rng.choice(li))
                a = int(rng.choice(mi)) if dec else b2
                wh = np.tile(C[a] + (0.5 * C[b2] if dec else 0.0), rep) + 0.25
                s = rstd * (u @ wh - mu * wh.sum()) * 0.125 * LOG2E
                sl = np.sort(s[live])
                if li[s[live].argmax()] == b2 and (sl.size == 1 or sl[-1] - sl[-2] >= GAP_MIN + 8):
                    break
            else:
                raise AssertionError("fold_selector_case: no selector head found")
            w[b, h], wins[h] = wh, b2
            if b2 in free:
                free.remove(b2)                                         # a different token per head
        assert np.all(r16(w[b]) == w[b])
        # the builder's check: winner, gap (log2 units), decoys, and the kernel's fp32 score error < 1 unit
        s = rstd[None] * (w[b] @ u.T - mu[None] * w[b].sum(1)[:, None]) * 0.125 * LOG2E
        decoys += int((~live[s.argmax(1)]).sum())
        s[:, ~live] = -np.inf
        win = s.argmax(1)
        assert np.array_equal(win, wins)
        if li.size > 1:
            top2 = np.sort(s, 1)[:, -2:]
            gmin = min(gmin, float((top2[:, 1] - top2[:, 0]).min()))
        jr = np.random.default_rng(seed + 77 + b)
        u[~live] = r16(jr.uniform(-2000.0, 2000.0, ((~live).sum(), D)))
        mu_s, rstd_s = np.where(live, mu, jr.uniform(-1e3, 1e3, S)), np.where(live, rstd, jr.uniform(0.0, 50.0, S))
        U[b], mr[b] = u, np.stack([mu_s, rstd_s], 1)
        _, _, Eh = fold_ref(w[b], u, mu, rstd, live, True)
        emax = max(emax, float(Eh.max()) * LOG2E)
        z = rstd[win, None] * (u[win] - mu[win, None])
        assert np.all(z.astype(np.float32) == z)
        assert np.unique(z, axis=0).shape[0] == np.unique(win).size >= min(H, li.size) // 2
        hi, lo = hi_lo(z)
        assert np.all(hi.astype(np.float64) + lo.astype(np.float64) == z)     # the pair holds z' exactly
        exp_hi[b], exp_lo[b] = hi, lo
    assert gmin >= GAP_MIN and 2.0 * emax < 10.0, (gmin, emax)
    return dict(w=f16(w), U=f16(U).reshape(B * S, D), mr=mr.astype(np.float32), mask=masks.astype(np.int32),
                masks=masks, hi=exp_hi, lo=exp_lo, gap_min=gmin, decoys=decoys, B=B, S=S, D=D, H=H,
                lo_nonzero=int((exp_lo != 0).sum()))


def fold_random_case(D, H, S, B, seed):
    """Random offset rows (|mean| up to ~10 standard deviations), true fp32 row statistics, ragged /
    holed masks (every sequence keeps a live token), junk in masked tokens' U rows and mr."""
    rng = np.random.default_rng(seed)
    masks = pattern_masks(tuple([0, 1, 5, 4, 3][b % 5] for b in range(B)), S, seed)
    sd = rng.uniform(0.2, 1.0, (B, S))
    off = rng.uniform(-10.0, 10.0, (B, S)) * sd
    U = r16(off[..., None] + sd[..., None] * rng.standard_normal((B, S, D)))
    mu, rstd = U.mean(-1), 1.0 / np.sqrt(U.var(-1) + 1e-5)
    w = r16(rng.standard_normal((B, H, D)) * (2.5 / math.sqrt(D)) * 8.0 ** 0.5)
    U[~masks] = r16(rng.uniform(-2000.0, 2000.0, ((~masks).sum(), D)))
    mr = np.stack([np.where(masks, mu, rng.uniform(-1e3, 1e3, (B, S))),
                   np.where(masks, rstd, rng.uniform(0.0, 50.0, (B, S)))], -1)
    return dict(w=f16(w), U=f16(U).reshape(B * S, D), mr=mr.astype(np.float32), mask=masks.astype(np.int32),
                masks=masks, B=B, S=S, D=D, H=H)


def fold_case_ref(case, single_read):
    """(ref, bound) [B, H, D] of a fold case, from the fp16 / fp32 values the kernel reads."""
    B, S, D = case["B"], case["S"], case["D"]
    U = case["U"].astype(np.float64).reshape(B, S, D)
    mr = case["mr"].astype(np.float64)
    out = [fold_ref(case["w"][b].astype(np.float64), U[b], mr[b, :, 0], mr[b, :, 1], case["masks"][b], single_read)[:2]
           for b in range(B)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def kv_blockdiag_ref(wqkv, D, H):
    """numpy construction of launch_kv_blockdiag's outputs (k_encoder_misc.hip's layout comment)."""
    dh = D // H
    wk = np.zeros((H * D, D), wqkv.dtype)
    wv = np.zeros((D, 2 * H * D), wqkv.dtype)
    for h in range(H):
        ks = slice(h * dh, (h + 1) * dh)
        wk[h * D:(h + 1) * D, ks] = wqkv[D + h * dh:D + (h + 1) * dh, :].T
        for c in range(2):
            wv[ks, c * H * D + h * D:c * H * D + (h + 1) * D] = wqkv[2 * D + h * dh:2 * D + (h + 1) * dh, :]
    return wk, wv


# ---- fp32 / fp16 emulations of the documented rounding points, with mutations -----------------------
f32 = np.float32


def emu_attention(qkv, masks, heads, dh, Sq=None, mut=None):
    """qkv [B S, 3 d] fp16, masks [B, S] bool -> ctx [B, Sq, d] fp16: fp32 scores in log2 units, fp32
    exp2, P rounded to fp16, fp32 P.V and row sum of the fp16 P, one fp16 rounding of the output.
    mut: 'mask_shift' (key j reads mask j + 1), 'kv_swap', 'head_off' (K, V of head h + 1), 'scale'
    (1 / sqrt(dh / 2))."""
    B, S = masks.shape
    d = heads * dh
    Sq = S if Sq is None else Sq
    x = np.asarray(qkv).astype(f32).reshape(B, S, 3, heads, dh)
    q, k, v = x[:, :, 0], x[:, :, 1], x[:, :, 2]
    if mut == "kv_swap":
        k, v = v, k
    if mut == "head_off":
        k, v = np.roll(k, -1, 2), np.roll(v, -1, 2)
    m = np.roll(masks, -1, 1) if mut == "mask_shift" else masks
    sl2 = f32(LOG2E / math.sqrt(dh / 2 if mut == "scale" else dh))
    out = np.zeros((B, Sq, heads, dh), np.float16)
    for b in range(B):
        if not m[b].any():
            continue
        s = np.einsum("the,jhe->htj", q[b, :Sq], k[b]).astype(f32) * sl2
        s[:, :, ~m[b]] = -np.inf
        with np.errstate(over="ignore", invalid="ignore"):
            p = np.exp2(s - s.max(-1, keepdims=True)).astype(f32).astype(np.float16).astype(f32)
            o = np.einsum("htj,jhe->the", p, v[b]).astype(f32)
            l = p.sum(-1).astype(f32).T[:, :, None]
            out[b] = (o * (f32(1.0) / l)).astype(np.float16)
    return out.reshape(B, Sq, d)


def emu_k5c(case, mut=None):
    """fp32 GEMM + epilogue, fp16 Q | K | V, then emu_attention.  mut: 'last_kstep' (columns d - 64 ..
    dropped from the K-loop), 'no_mu_colsum' (the folded epilogue without -mu colsum), or an
    emu_attention mutation."""
    d, epi = case["d"], case["epi"]
    X = case["X"].astype(f32)[:, :d]
    W = case["W"].astype(f32)
    kk = d - 64 if mut == "last_kstep" else d
    acc = (X[:, :kk] @ W[:, :kk].T).astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        if epi == 5:
            mu, rstd = case["mr"][:, 0:1], case["mr"][:, 1:2]
            inner = acc if mut == "no_mu_colsum" else (acc - mu * case["colsum"][None]).astype(f32)
            y = (rstd * inner).astype(f32) + case["bias"][None]
        else:
            y = acc + case["bias"][None]
        qkv = y.astype(np.float16)
    am = mut if mut in ("mask_shift", "kv_swap", "head_off", "scale") else None
    return emu_attention(qkv, case["masks"], case["heads"], 64, mut=am)


def emu_fold(case, single_read, mut=None):
    """fp32 emulation of cls_attn_fold -> (hi, lo) [B, H, D] fp16.  mut: 'no_mu_alpha' (scores without
    -mu_j alpha_h), 'no_sig' (z' without -sig_h), 'no_lo' (lo = 0)."""
    B, S, D, H = case["B"], case["S"], case["D"], case["H"]
    U = case["U"].astype(f32).reshape(B, S, D)
    hi = np.zeros((B, H, D), np.float16)
    lo = np.zeros((B, H, D), np.float16)
    for b in range(B):
        live = case["masks"][b]
        w = case["w"][b].astype(f32)
        mu, rstd = case["mr"][b, live, 0], case["mr"][b, live, 1]
        u = U[b, live]
        alpha = w.sum(1, dtype=f32)
        acc = (w @ u.T).astype(f32)
        inner = acc if mut == "no_mu_alpha" else acc - mu[None] * alpha[:, None]
        s = (rstd[None] * inner * f32(0.125)).astype(f32)
        p = np.exp(s - s.max(1, keepdims=True)).astype(f32)
        pp = (p * (f32(1.0) / p.sum(1, keepdims=True, dtype=f32)) * rstd[None]).astype(f32)
        sig = (pp @ mu).astype(f32)
        if single_read:
            ph = pp.astype(np.float16).astype(f32)
            pl = (pp - ph).astype(np.float16).astype(f32)
            z = (ph @ u + pl @ u).astype(f32)
        else:
            z = (pp @ u).astype(f32)
        zz = z if mut == "no_sig" else (z - sig[:, None]).astype(f32)
        hi[b] = zz.astype(np.float16)
        if mut != "no_lo":
            lo[b] = (zz - hi[b].astype(f32)).astype(np.float16)
    return hi, lo


# ---- the cases the GPU tests run (tests/test_attn_ref.py checks the same ones on the CPU) -----------
K5_SHAPES = [(7, 7), (100, 100), (128, 128), (128, 97), (128, 1), (130, 130), (200, 200), (512, 512),
             (512, 481), (500, 1)]
K5_PATS = (0, 1, 2, 5, 4, 3)                # B = 6: holes, ragged, fully masked, holes, full, length 1
K5_DH32_S = [7, 100, 130]
K5C_SELECTOR = [  # (heads, pattern ids per sequence, lda pad)
    (1, (0,), 0), (1, (5, 1, 2), 8), (2, (0, 1), 8), (2, (3, 4, 2), 0), (12, (0, 1, 5), 0), (12, (5, 2), 8),
    (16, (1, 0, 4), 8), (16, (5,), 0)]
K5C_MANY = (12, tuple([0, 1, 5, 4, 3, 2][b % 6] for b in range(45)), 0)     # 276 tiles
FOLD_GEOM = [(768, 12), (1024, 16)]
FOLD_S1 = [16, 32, 48, 96, 112, 128]        # single-read form
FOLD_S2 = [16, 128, 144, 512]               # two-pass form (S <= 128 by SR_CLS_FOLD_1READ=0)
