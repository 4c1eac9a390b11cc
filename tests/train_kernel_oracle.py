"""numpy float64 / int64 restatements of every ``cotr_train_*`` computation, written from the text of include/cotr_hip.h and the
formulas in the comments of cotr_amd/csrc/train.hip and attention_train.hip - not from cotr_amd/train_ops.py, and with nothing
imported from the library.  tests/train_guard_cases.py compares the kernels with these element by element; the dropout masks are
tests/dropout_oracle.py's.  tests/test_train_guard_cpu.py pins this file against torch float64 autograd.

Conventions
* a *move* is returned in float32 with the kernel's own single roundings repeated, for a bit-for-bit comparison;
* a *sum of products* is returned as ``(value, sumabs)``: the float64 (on integer data: exact) sum and the sum of the absolute
  values of its terms, from which the caller forms the any-order bound ``(n + 2) 2^-24 sumabs`` or asserts ``sumabs < 2^24``;
* everything with a ``rsqrt``, ``exp2`` or division is returned as ``(value, scale)`` with the per-element scale of the issue's
  yardstick rule, and has a ``*_f32`` twin: the same formula in torch float32 on the CPU (the yardstick itself).
"""
import numpy as np

from tests import dropout_oracle as do

F32, F64 = np.float32, np.float64
ATT_KEYS, HEADS, HD = 512, 8, 32
LOG2E = 1.4426950408889634


def cdiv(a, b):
    return -(-a // b)


# ---- the host queries as closed forms ------------------------------------------------------------------------------------------
def ln_bwd_per(rows):
    """rows a workgroup of cotr_train_ln_bwd: at most 512 workgroups, a multiple of 4 rows each"""
    return cdiv(cdiv(rows, 512), 4) * 4


def ln_bwd_parts(rows):
    return cdiv(rows, ln_bwd_per(rows)) if rows > 0 else 0


def head_bwd_per(rows):
    return cdiv(cdiv(rows, 256), 4) * 4


def head_bwd_parts(rows):
    return cdiv(rows, head_bwd_per(rows)) if rows > 0 else 0


def colsum_per(M):
    return cdiv(M, 256)


def colsum_parts(M):
    return cdiv(M, colsum_per(M)) if M > 0 else 0


def gemm_tn_big(M, N, K):
    return N % 128 == 0 and K % 128 == 0 and N * K >= 512 * 256 and M >= 2048


def gemm_tn_splits(M, N, K):
    """the query: enough splits of M for about two workgroups a CU (512), at least 128 (64 x 64 kernel) or 256 (128 x 128) rows each"""
    tile, least = (128, 256) if gemm_tn_big(M, N, K) else (64, 128)
    tiles = (N // tile) * (K // tile)
    return max(1, min(cdiv(512, tiles), cdiv(M, least)))


def gemm_tn_plan(M, N, K):
    """-> (rows a split, partials written): the rows of a split are rounded up to a multiple of 32, so fewer partials than the query
    allows may be written"""
    if M <= 0:
        return 0, 0
    per = cdiv(cdiv(M, gemm_tn_splits(M, N, K)), 32) * 32
    return per, cdiv(M, per)


def attention_bwd_scratch(nb, nq):
    return 4 * nb * nq * 256 if nb > 0 and nq > 0 else 0


def conv_out(n, ksize, stride):
    pad = ksize // 2
    return (n + 2 * pad - ksize) // stride + 1


# ---- moves -------------------------------------------------------------------------------------------------------------------
def add_rowmod(x, x2, mod):
    rows = x.shape[0]
    idx = np.arange(rows) % mod if mod else np.arange(rows)
    return (x.astype(F32) + x2.astype(F32)[idx]).astype(F32)


def dropped(a, keep, p):
    """a * mask / (1 - p) as one float32 multiply (p == 0: untouched)"""
    a = a.astype(F32)
    if do.thresh(p) == 0:
        return a
    return np.where(keep, a * F32(do.inv_keep(p)), F32(0)).astype(F32)


def dropout_fwd(x, p, seed):
    n = x.size
    return dropped(x.reshape(-1), do.flat_mask(seed, 1, n, p)[0], p).reshape(x.shape)


def relu_drop_bwd(dy, y, p):
    inv = F32(do.inv_keep(p)) if p > 0 else F32(1)
    return np.where(y > 0, dy.astype(F32) * inv, F32(0)).astype(F32)


def transpose(src):
    """[..., R, C] -> [..., C, R]"""
    return np.ascontiguousarray(np.swapaxes(src, -1, -2))


def scale_rows(w, scale):
    return (w.astype(F32) * scale.astype(F32)[:, None]).astype(F32)


def perm_job(src_flat, Z, R, C, sz, sr, sc, scale, reverse):
    """-> [Z][C][R] float32: element (z, c, r) of the destination, src[z' sz + r sr + c sc] * scale[r] with z' = Z - 1 - z when
    the reverse-batch flag is set"""
    z = np.arange(Z)[:, None, None]
    zs = Z - 1 - z if reverse else z
    r, c = np.arange(R)[None, None, :], np.arange(C)[None, :, None]
    v = src_flat.astype(F32)[zs * sz + r * sr + c * sc]
    if scale is not None:
        v = v * scale.astype(F32)[None, None, :]
    return v.astype(F32)


def im2col_index(B, Hin, Win, Cin, ksize, stride):
    """-> (idx [M][k*k*Cin] int64 into x.reshape(-1), -1 where the tap leaves its half, Hout, Wout)"""
    pad, Hout, Wout = ksize // 2, conv_out(Hin, ksize, stride), conv_out(Win, ksize, stride)
    b, ho, side, wl, ky, kx, c = np.meshgrid(np.arange(B), np.arange(Hout), np.arange(2), np.arange(Wout), np.arange(ksize),
                                             np.arange(ksize), np.arange(Cin), indexing='ij')
    hi, wi = ho * stride - pad + ky, wl * stride - pad + kx
    inside = (hi >= 0) & (hi < Hin) & (wi >= 0) & (wi < Win)
    idx = ((b * Hin + hi) * (2 * Win) + side * Win + wi) * Cin + c
    idx = np.where(inside, idx, -1)
    return idx.reshape(B * Hout * 2 * Wout, ksize * ksize * Cin), Hout, Wout


def im2col(x, B, Hin, Win, Cin, ksize, stride):
    idx, _, _ = im2col_index(B, Hin, Win, Cin, ksize, stride)
    flat = np.concatenate([x.reshape(-1), np.zeros(1, x.dtype)])
    return flat[idx]                                                   # index -1: the appended zero


# ---- sums of products: (value, sumabs) -----------------------------------------------------------------------------------------
def col2im(dcol, B, Hin, Win, Cin, ksize, stride):
    """dx[pixel] = the sum of the dcol entries that read it -> (dx, sumabs, most terms of one element)"""
    idx, _, _ = im2col_index(B, Hin, Win, Cin, ksize, stride)
    n = B * Hin * 2 * Win * Cin
    ok = idx >= 0
    d = dcol.astype(F64)[ok]
    val = np.bincount(idx[ok], weights=d, minlength=n)
    sab = np.bincount(idx[ok], weights=np.abs(d), minlength=n)
    cnt = np.bincount(idx[ok], minlength=n)
    shape = (B, Hin, 2 * Win, Cin)
    return val.reshape(shape), sab.reshape(shape), int(cnt.max(initial=0))


def sum_parts(part):
    p = part.astype(F64)
    return p.sum(0), np.abs(p).sum(0)


def colsum(x):
    """-> out (value, sumabs), part (value, sumabs): the per-workgroup partials [parts][N]"""
    M, N = x.shape
    per, parts = colsum_per(M), colsum_parts(M)
    xx = x.astype(F64)
    pv = np.stack([xx[w * per:(w + 1) * per].sum(0) for w in range(parts)])
    pa = np.stack([np.abs(xx[w * per:(w + 1) * per]).sum(0) for w in range(parts)])
    return (xx.sum(0), np.abs(xx).sum(0)), (pv, pa)


def gemm_tn_parts(A, B, with_colsum):
    """-> (part [nsplit][N*K (+ N)], sumabs of the same shape, per): part[s] = A[rows of s]^T . B[rows of s] | column sums of A"""
    M, N = A.shape
    K = B.shape[1]
    per, nsplit = gemm_tn_plan(M, N, K)
    A64, B64 = A.astype(F64), B.astype(F64)
    vals, sabs = [], []
    for s in range(nsplit):
        a, b = A64[s * per:(s + 1) * per], B64[s * per:(s + 1) * per]
        v, sa = (a.T @ b).reshape(-1), (np.abs(a).T @ np.abs(b)).reshape(-1)
        if with_colsum:
            v, sa = np.concatenate([v, a.sum(0)]), np.concatenate([sa, np.abs(a).sum(0)])
        vals.append(v)
        sabs.append(sa)
    width = N * K + (N if with_colsum else 0)
    return np.array(vals).reshape(nsplit, width), np.array(sabs).reshape(nsplit, width), per


def gemm_tn(A, B, with_colsum):
    A64, B64 = A.astype(F64), B.astype(F64)
    v, sa = (A64.T @ B64).reshape(-1), (np.abs(A64).T @ np.abs(B64)).reshape(-1)
    if with_colsum:
        v, sa = np.concatenate([v, A64.sum(0)]), np.concatenate([sa, np.abs(A64).sum(0)])
    return v, sa


def reduce_job(dst, srcs, scale, row_len, cin, taps):
    """dst[perm(e)] += scale[e / row_len] * sum_p part[p][e] for every source (each ``[nparts][numel]``) -> (dst, sumabs)"""
    numel = dst.size
    e = np.arange(numel)
    d = e
    sc = np.ones(numel)
    if row_len:
        row, col = e // row_len, e % row_len
        if scale is not None:
            sc = scale.astype(F64)[row]
        if taps > 1:
            d = row * row_len + (col % cin) * taps + col // cin
    val, sab = dst.astype(F64).copy(), np.abs(dst.astype(F64))
    for part in srcs:
        val[d] += sc * part.astype(F64).sum(0)
        sab[d] += np.abs(sc) * np.abs(part.astype(F64)).sum(0)
    return val, sab


def head_bwd(dy, h, w2):
    """-> dh, part [parts][514], dwb [514], each (value, sumabs)"""
    rows = dy.shape[0]
    d, hh, w = dy.astype(F64), h.astype(F64), w2.astype(F64).reshape(2, 256)
    dh = (d @ w, np.abs(d) @ np.abs(w))
    per, parts = head_bwd_per(rows), head_bwd_parts(rows)

    def sums(lo, hi):
        dd, x = d[lo:hi], hh[lo:hi]
        return (np.concatenate([(dd.T @ x).reshape(-1), dd.sum(0)]), np.concatenate([(np.abs(dd).T @ np.abs(x)).reshape(-1), np.abs(dd).sum(0)]))
    ps = [sums(w_ * per, (w_ + 1) * per) for w_ in range(parts)]
    part = (np.array([p[0] for p in ps]).reshape(parts, 514), np.array([p[1] for p in ps]).reshape(parts, 514))
    return dh, part, sums(0, rows)


# ---- yardstick class: (value, scale), and the same formula in torch float32 ------------------------------------------------------
def head_fwd(x, w, b):
    """y = x . w^T + b; scale: the sum of the absolute terms"""
    x64, w64, b64 = x.astype(F64), w.astype(F64).reshape(2, 256), b.astype(F64)
    return x64 @ w64.T + b64, np.abs(x64) @ np.abs(w64).T + np.abs(b64)


def head_fwd_f32(x, w, b):
    import torch
    return (torch.from_numpy(x) @ torch.from_numpy(w).reshape(2, 256).T + torch.from_numpy(b)).numpy()


def ln_s(x, a, p, seed):
    """s = x + dropout(a) in float32, rounding for rounding (a move)"""
    rows = a.shape[0]
    s = dropped(a, do.flat_mask(seed, rows, 256, p), p)
    return s if x is None else (s + x.astype(F32)).astype(F32)


def ln_fwd(s, w, b):
    """LayerNorm over 256 channels, eps 1e-5, biased variance -> y (value, scale [rows, 1] = the row's max |y - b|),
    mean (value, scale = the row's max |s|), rstd (value, scale = rstd)"""
    s64 = s.astype(F64)
    mean = s64.mean(1, keepdims=True)
    var = ((s64 - mean) ** 2).mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + 1e-5)
    yb = (s64 - mean) * rstd * w.astype(F64)
    tiny = np.finfo(F32).tiny
    return ((yb + b.astype(F64), np.maximum(np.abs(yb).max(1, keepdims=True), tiny)),
            (mean[:, 0], np.maximum(np.abs(s64).max(1), tiny)), (rstd[:, 0], rstd[:, 0]))


def ln_fwd_f32(s, w, b):
    import torch
    st = torch.from_numpy(s)
    mean = st.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((st - mean) ** 2).mean(1, keepdim=True) + 1e-5)
    return ((st - mean) * rstd * torch.from_numpy(w) + torch.from_numpy(b)).numpy(), mean[:, 0].numpy(), rstd[:, 0].numpy()


def ln_bwd(dy, s, stats, w):
    """with xhat = (s - mean) rstd and g = dy w: ds = rstd (g - mean_c(g) - xhat mean_c(g xhat)); dgamma = sum_rows dy xhat,
    dbeta = sum_rows dy, per workgroup of ``ln_bwd_per`` rows and in total.  mean and rstd are the given ``stats``.
    -> ds (value, scale = rstd * the row's max |g| (1 + max |xhat|)^2: the sum of the absolute terms), gamma part / total
    (value, sumabs of |dy xhat|), beta part / total (value, sumabs)"""
    rows = dy.shape[0]
    d, s64, w64 = dy.astype(F64), s.astype(F64), w.astype(F64)
    mean, rstd = stats.astype(F64)[:, :1], stats.astype(F64)[:, 1:]
    xh, g = (s64 - mean) * rstd, d * w64
    ds = rstd * (g - g.mean(1, keepdims=True) - xh * (g * xh).mean(1, keepdims=True))
    scale = np.abs(rstd) * (np.abs(g) + np.abs(g).mean(1, keepdims=True) + np.abs(xh) * np.abs(g * xh).mean(1, keepdims=True))
    scale = np.maximum(scale.max(1, keepdims=True), np.finfo(F32).tiny)
    per, parts = ln_bwd_per(rows), ln_bwd_parts(rows)
    sl = [slice(w_ * per, (w_ + 1) * per) for w_ in range(parts)]
    gam = (np.array([(d[i] * xh[i]).sum(0) for i in sl]).reshape(parts, 256), np.array([np.abs(d[i] * xh[i]).sum(0) for i in sl]).reshape(parts, 256))
    bet = (np.array([d[i].sum(0) for i in sl]).reshape(parts, 256), np.array([np.abs(d[i]).sum(0) for i in sl]).reshape(parts, 256))
    return dict(ds=(ds, scale), gamma_part=gam, beta_part=bet, gamma=((d * xh).sum(0), np.abs(d * xh).sum(0)),
                beta=(d.sum(0), np.abs(d).sum(0)))


def ln_bwd_f32(dy, s, stats, w):
    import torch
    d, st, wt, stt = torch.from_numpy(dy), torch.from_numpy(s), torch.from_numpy(w), torch.from_numpy(stats)
    mean, rstd = stt[:, :1], stt[:, 1:]
    xh, g = (st - mean) * rstd, d * wt
    ds = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return ds.numpy(), (d * xh).sum(0).numpy()


def adam(p, g, m, v, lr, b1, b2, eps, bc1, bc2_sqrt, step=None):
    """m += (g - m)(1 - b1); v = v b2 + (1 - b2) g g; p -= lr / bc1 * m / (sqrt(v) / bc2_sqrt + eps), with the constants as the
    launcher rounds them to float32 (b1, b2, eps, 1 - b1 and 1 - b2 from double); ``step``: the corrections from the step count,
    bc1 = 1 - b1^t and bc2_sqrt = sqrt(1 - b2^t) with the float32 b1, b2.
    -> p, m, v as (value, scale): |update| for p; |m| + |g| and |v| + g^2 for m and v"""
    b1f, b2f, epsf = F64(F32(b1)), F64(F32(b2)), F64(F32(eps))
    omb1, omb2 = F64(F32(1.0 - b1)), F64(F32(1.0 - b2))
    if step is not None:
        bc1, bc2_sqrt = 1.0 - b1f ** F64(step), np.sqrt(1.0 - b2f ** F64(step))
    else:
        bc1, bc2_sqrt = F64(F32(bc1)), F64(F32(bc2_sqrt))
    p64, g64, m64, v64, lr64 = p.astype(F64), g.astype(F64), m.astype(F64), v.astype(F64), F64(F32(lr))
    m1 = m64 + omb1 * (g64 - m64)
    v1 = v64 * b2f + omb2 * g64 * g64
    upd = lr64 / bc1 * (m1 / (np.sqrt(v1) / bc2_sqrt + epsf))
    tiny = np.finfo(F32).tiny
    return ((p64 - upd, np.maximum(np.abs(upd), tiny)), (m1, np.maximum(np.abs(m64) + np.abs(g64), tiny)),
            (v1, np.maximum(np.abs(v64) + g64 * g64, tiny)))


def adam_f32(p, g, m, v, lr, b1, b2, eps, bc1, bc2_sqrt, step=None):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=F32))   # noqa: E731
    f = lambda a: torch.tensor(float(a), dtype=torch.float32)            # noqa: E731
    pt, gt, mt, vt = t(p), t(g), t(m), t(v)
    if step is not None:
        bc1, bc2_sqrt = 1.0 - torch.pow(f(b1), f(step)), torch.sqrt(1.0 - torch.pow(f(b2), f(step)))
    else:
        bc1, bc2_sqrt = f(bc1), f(bc2_sqrt)
    m1 = mt + f(1.0 - b1) * (gt - mt)
    v1 = vt * f(b2) + f(1.0 - b2) * gt * gt
    p1 = pt - f(lr) / bc1 * (m1 / (torch.sqrt(v1) / bc2_sqrt + f(eps)))
    return p1.numpy(), m1.numpy(), v1.numpy()


def _heads(x, nb, n):
    """[nb*n][>= 256] -> [nb][8][n][32] float64"""
    return x[:, :256].astype(F64).reshape(nb, n, HEADS, HD).transpose(0, 2, 1, 3)


def _rows(x, nb, n):
    """[nb][8][n][...] -> [nb*n][8 * ...]"""
    return np.ascontiguousarray(np.moveaxis(x, 1, 2)).reshape(nb * n, -1)


def attention_fwd(q, k, v, nb, nq, qscale, p, seed, mask_shift=0):
    """o = dropout(softmax(q k^T qscale)) v per head; lse = log2 of the sum of exp of the scaled scores
    -> o (value [nb*nq][256], scale = sum_j |p_j v_j|), lse (value [nb*nq][8], scale = max(|lse|, 1)).
    ``mask_shift``: the mask index moved by that much (what a wrong kernel would draw; the doctored-reference test)"""
    qh, kh, vh = _heads(q, nb, nq), _heads(k, nb, ATT_KEYS), _heads(v, nb, ATT_KEYS)
    s = np.einsum('bhqd,bhkd->bhqk', qh, kh) * F64(F32(qscale))
    mx = s.max(-1, keepdims=True)
    e = np.exp(s - mx)
    l = e.sum(-1, keepdims=True)
    lse = (mx + np.log(l))[..., 0] * LOG2E
    pd = e / l
    if do.thresh(p):
        keep = do.keep(seed, do.attention_index(nb, nq) + np.uint64(mask_shift), p)
        pd = np.where(keep, pd * F64(F32(do.inv_keep(p))), 0.0)
    o = np.einsum('bhqk,bhkd->bhqd', pd, vh)
    so = np.einsum('bhqk,bhkd->bhqd', pd, np.abs(vh))
    tiny = np.finfo(F32).tiny
    return (_rows(o, nb, nq), np.maximum(_rows(so, nb, nq), tiny)), (_rows(lse[..., None], nb, nq), np.maximum(np.abs(_rows(lse[..., None], nb, nq)), 1.0))


def attention_fwd_f32(q, k, v, nb, nq, qscale, p, seed):
    import torch

    def heads(x, n):
        return torch.from_numpy(np.ascontiguousarray(x[:, :256])).reshape(nb, n, HEADS, HD).permute(0, 2, 1, 3)
    s = (heads(q, nq) * float(F32(qscale))) @ heads(k, ATT_KEYS).transpose(-1, -2)
    lse = torch.logsumexp(s, -1) * float(F32(LOG2E))
    pd = torch.softmax(s, -1)
    if do.thresh(p):
        pd = torch.where(torch.from_numpy(do.attention_mask(seed, nb, nq, p)), pd * float(F32(do.inv_keep(p))), torch.zeros(()))
    o = pd @ heads(v, ATT_KEYS)
    return o.permute(0, 2, 1, 3).reshape(nb * nq, 256).numpy(), lse.permute(0, 2, 1).reshape(nb * nq, 8).numpy()


def attention_bwd(q, k, v, o, d_o, lse, nb, nq, qscale, p, seed):
    """with P = exp2(s log2e - lse) recomputed from the GIVEN lse, P~ = P mask / (1 - p), delta = rowsum(dO * O) of the GIVEN o:
    dV = P~^T dO, dP~ = dO V^T, dP = dP~ mask / (1 - p), dS = P (dP - delta), dQ = dS K qscale, dK = dS^T Q qscale
    -> delta, dq, dk, dv as (value, scale = the sum of the absolute terms)"""
    qh, kh, vh = _heads(q, nb, nq), _heads(k, nb, ATT_KEYS), _heads(v, nb, ATT_KEYS)
    oh, doh = _heads(o, nb, nq), _heads(d_o, nb, nq)
    sc = F64(F32(qscale))
    s = np.einsum('bhqd,bhkd->bhqk', qh, kh) * sc
    lse_h = lse.astype(F64).reshape(nb, nq, HEADS).transpose(0, 2, 1)[..., None]
    P = np.exp2(s * LOG2E - lse_h)
    f = 1.0
    if do.thresh(p):
        f = np.where(do.attention_mask(seed, nb, nq, p), F64(F32(do.inv_keep(p))), 0.0)
    pd = P * f
    delta, sdelta = (oh * doh).sum(-1, keepdims=True), np.abs(oh * doh).sum(-1, keepdims=True)
    dP = np.einsum('bhqd,bhkd->bhqk', doh, vh) * f
    adP = np.einsum('bhqd,bhkd->bhqk', np.abs(doh), np.abs(vh)) * f
    dS, adS = P * (dP - delta), P * (adP + sdelta)
    tiny = np.finfo(F32).tiny
    out = dict(delta=(_rows(delta, nb, nq), np.maximum(_rows(sdelta, nb, nq), tiny)))
    for name, val, sab, n in (('dq', np.einsum('bhqk,bhkd->bhqd', dS, kh) * sc, np.einsum('bhqk,bhkd->bhqd', adS, np.abs(kh)) * sc, nq),
                              ('dk', np.einsum('bhqk,bhqd->bhkd', dS, qh) * sc, np.einsum('bhqk,bhqd->bhkd', adS, np.abs(qh)) * sc, ATT_KEYS),
                              ('dv', np.einsum('bhqk,bhqd->bhkd', pd, doh), np.einsum('bhqk,bhqd->bhkd', pd, np.abs(doh)), ATT_KEYS)):
        out[name] = (_rows(val, nb, n), np.maximum(_rows(sab, nb, n), tiny))
    return out


def attention_bwd_f32(q, k, v, o, d_o, lse, nb, nq, qscale, p, seed):
    import torch

    def heads(x, n):
        return torch.from_numpy(np.ascontiguousarray(x[:, :256])).reshape(nb, n, HEADS, HD).permute(0, 2, 1, 3)

    def rows(x, n):
        return x.permute(0, 2, 1, 3).reshape(nb * n, -1).numpy()
    qh, kh, vh, oh, doh = heads(q, nq), heads(k, ATT_KEYS), heads(v, ATT_KEYS), heads(o, nq), heads(d_o, nq)
    sc = float(F32(qscale))
    s = (qh * (sc * float(F32(LOG2E)))) @ kh.transpose(-1, -2)
    P = torch.exp2(s - torch.from_numpy(np.ascontiguousarray(lse)).reshape(nb, nq, HEADS).permute(0, 2, 1)[..., None])
    f = torch.ones(())
    if do.thresh(p):
        f = torch.where(torch.from_numpy(do.attention_mask(seed, nb, nq, p)), torch.tensor(float(F32(do.inv_keep(p)))), torch.zeros(()))
    pd = P * f
    delta = (oh * doh).sum(-1, keepdim=True)
    dS = P * ((doh @ vh.transpose(-1, -2)) * f - delta)
    return dict(delta=rows(delta, nq), dq=rows((dS @ kh) * sc, nq), dk=rows((dS.transpose(-1, -2) @ qh) * sc, ATT_KEYS),
                dv=rows(pd.transpose(-1, -2) @ doh, ATT_KEYS))
