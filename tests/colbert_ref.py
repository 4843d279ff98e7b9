"""Reference restatements for the multi-vector (ColBERT) tests, numpy fp64 unless stated:

head(h, mask, W, b)      the encoder head from given final states: v = W h + b, u = v / max(||v||,
                         1e-12), the vectors of the positions s >= 1 with mask != 0, in position order
maxsim(q, d)             (1 / Lq) sum_i max_j q_i . d_j; -inf when either side is empty
maxsim_rows(...)         the [B, K] table sr_mv_score_rows computes, with its -inf cases
combine / select         m3_rerank's weighted mean (fp32, the order multivec.combine_dev documents)
                         and its selection (score desc, row asc)
and the synthetic generators the GPU tests use (unit vectors rounded to fp16, adversarial cases).
"""
import numpy as np

F = np.float32


# -- the head ---------------------------------------------------------------------------------------------
def head_all(h, W, b):
    """h [B, S, hidden], W [dc, hidden], b [dc] -> (v, u) [B, S, dc] fp64 for every position."""
    v = np.asarray(h, np.float64) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
    n = np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-12)
    return v, v / n


def kept_positions(mask_row):
    m = np.asarray(mask_row)
    return np.nonzero((m != 0) & (np.arange(m.size) >= 1))[0]


def head(h, mask, W, b):
    """-> ([u_b fp64 [len_b, dc]], lens int32 [B])."""
    _, u = head_all(h, W, b)
    out = [u[i, kept_positions(mask[i])] for i in range(u.shape[0])]
    return out, np.asarray([o.shape[0] for o in out], np.int32)


def head_loop(h, mask, W, b):
    """head() as plain loops (the restatement's own check)."""
    B, S, d = np.shape(h)
    dc = np.shape(W)[0]
    out = []
    for i in range(B):
        rows = []
        for s in range(1, S):
            if mask[i][s] == 0:
                continue
            v = [float(b[c]) + sum(float(W[c][k]) * float(h[i][s][k]) for k in range(d)) for c in range(dc)]
            n = max(sum(x * x for x in v) ** 0.5, 1e-12)
            rows.append([x / n for x in v])
        out.append(np.asarray(rows, np.float64).reshape(len(rows), dc))
    return out


# -- MaxSim ------------------------------------------------------------------------------------------------
def maxsim(q, d):
    q = np.asarray(q, np.float64)
    d = np.asarray(d, np.float64)
    if q.shape[0] == 0 or d.shape[0] == 0:
        return -np.inf
    return float((q @ d.T).max(axis=1).sum() / q.shape[0])


def maxsim_loop(q, d):
    if len(q) == 0 or len(d) == 0:
        return -np.inf
    tot = 0.0
    for qi in q:
        best = -np.inf
        for dj in d:
            dot = 0.0
            for a, c in zip(qi, dj):
                dot += float(a) * float(c)
            best = max(best, dot)
        tot += best
    return tot / len(q)


def maxsim_rows(q_list, docs, rows, live=None):
    """docs: list of [Ld, dim] arrays (the index rows); rows [B, K]; live: optional bool [n_rows]."""
    rows = np.asarray(rows, np.int64)
    out = np.full(rows.shape, -np.inf, np.float64)
    for b in range(rows.shape[0]):
        for k in range(rows.shape[1]):
            r = int(rows[b, k])
            if r < 0 or r >= len(docs) or (live is not None and not live[r]):
                continue
            out[b, k] = maxsim(q_list[b], docs[r])
    return out


def gate(dim, lq, q, d):
    """(dim + Lq) 2^-23 max||q_i|| max||d_j||: fp16 x fp16 products are exact in fp32, so only the
    dim accumulations of a dot product and the Lq additions of the mean round."""
    nq = np.linalg.norm(np.asarray(q, np.float64), axis=-1).max() if len(q) else 0.0
    nd = np.linalg.norm(np.asarray(d, np.float64), axis=-1).max() if len(d) else 0.0
    return (dim + lq) * 2.0 ** -23 * nq * nd


# -- the combined score -----------------------------------------------------------------------------------
def combine(cos, ms, sparse=None, weights=(1, 1, 1)):
    """fp32, every operation rounded once: ((w_d cos + w_s sparse) + w_c maxsim) / (w_d + w_s + w_c);
    sparse None drops the term and its weight."""
    wd, ws, wc = (F(w) for w in weights)
    with np.errstate(invalid="ignore"):
        tot = wd * np.asarray(cos, F)
        wsum = wd
        if sparse is not None:
            tot = tot + ws * np.asarray(sparse, F)
            wsum = F(wsum + ws)
        tot = tot + wc * np.asarray(ms, F)
        wsum = F(wsum + wc)
        return (tot / wsum).astype(F)


def select(score, rows, k, extra_valid=None):
    """Top k by (score desc, row asc) among the candidates with row >= 0 and a finite score ->
    (score [B, k] fp32, rows [B, k] int64), -inf / -1 past them."""
    score = np.asarray(score, F)
    rows = np.asarray(rows, np.int64)
    B = score.shape[0]
    out_s = np.full((B, k), -np.inf, F)
    out_r = np.full((B, k), -1, np.int64)
    for b in range(B):
        ok = (rows[b] >= 0) & np.isfinite(score[b])
        if extra_valid is not None:
            ok &= extra_valid[b]
        idx = [i for i in range(rows.shape[1]) if ok[i]]
        idx.sort(key=lambda i: (-float(score[b, i]), int(rows[b, i])))
        for j, i in enumerate(idx[:k]):
            out_s[b, j] = score[b, i]
            out_r[b, j] = rows[b, i]
    return out_s, out_r


def rerank(cos, ms, sparse, rows, k, weights=(1, 1, 1)):
    valid = np.isfinite(np.asarray(cos, F)) & np.isfinite(np.asarray(ms, F))
    if sparse is not None:
        valid &= np.isfinite(np.asarray(sparse, F))
    return select(combine(cos, ms, sparse, weights), rows, k, extra_valid=valid)


# -- synthetic vectors ------------------------------------------------------------------------------------
def f16(x):
    """Round to fp16 and return the values as fp32."""
    return np.asarray(x, np.float64).astype(np.float16).astype(F)


def unit(x):
    x = np.asarray(x, np.float64)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def unit_f16(rng, n, dim):
    return f16(unit(rng.standard_normal((n, dim))))


def mixed_doc(rng, q, ld, alpha):
    """ld tokens, token j = alpha * q[(start + j) % Lq] + (1 - alpha) * noise, normalised (start
    random): with ld >= Lq every query token has its partner and MaxSim against q grows with alpha,
    from the noise level (about 0.2 to 0.4) at alpha = 0 to 1 at alpha = 1."""
    pick = q[(int(rng.integers(0, q.shape[0])) + np.arange(ld)) % q.shape[0]]
    noise = unit(rng.standard_normal((ld, q.shape[1])))
    return f16(unit(alpha * pick + (1.0 - alpha) * noise))


def all_negative_case(rng, lq, ld, dim):
    """Every q_i . d_j < 0: queries around +c, documents around -c."""
    c = unit(rng.standard_normal(dim))
    q = f16(unit(c + 0.3 * unit(rng.standard_normal((lq, dim)))))
    d = f16(unit(-c + 0.3 * unit(rng.standard_normal((ld, dim)))))
    return q, d


def tail_argmax_case(rng, lq, ld, dim):
    """Every query token's best document token lies in the last ld % 16 slots (ld % 16 != 0): the
    queries cluster around c, the body is noise, the tail sits next to c."""
    tail = ld % 16
    assert tail != 0
    c = unit(rng.standard_normal(dim))
    q = f16(unit(c + 0.3 * unit(rng.standard_normal((lq, dim)))))
    body = unit(rng.standard_normal((ld - tail, dim)))
    body = unit(body - 1.2 * (body @ c)[:, None] * c)        # pushed off c: q . body stays small
    tl = unit(c + 0.05 * unit(rng.standard_normal((tail, dim))))
    return q, f16(np.concatenate([body, tl], axis=0))


def first_last_case(rng, lq, ld, dim):
    """Query token 0's best match is document token 0, query token 1's the last one."""
    assert lq >= 2 and ld >= 2
    q = unit_f16(rng, lq, dim)
    d = unit_f16(rng, ld, dim)
    d[0] = q[0]
    d[-1] = q[1]
    return q, d
