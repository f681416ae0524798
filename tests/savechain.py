"""Save-chain references for the general fused-MLP kernels (csrc/mlp.hip mlp_fwd_kernel /
mlp_bwd_kernel) in fp32, bf16 and fp16 at hidden width 32, 64 and 128 (test infrastructure, not
product code; DESIGN.md §4 "save-chain"). It generalises tests/maskmatched.py.

Every tensor a kernel stores (act[l], pre[l], hpre, stats, out, a SUM / MEAN segment's stored value,
gpre[l], din[s], the LayerNorm partials) is compared with the float64 evaluation of the SAME step from
the kernel's own previously stored operands. A step never sees an independent model's values, so ReLU
kinks never enter: the backward reference masks with act[l] > 0, as the kernel's sign bits do.

Tolerance, per element, nothing fitted to a kernel's output and no element exempt:

    |got - ref| <= (n - 1/2) * ulp_T(|ref| + d) + d

ref    the float64 value of the step (unrounded).
ulp_T  the spacing of the storage type T at that magnitude: 2^(floor(log2 x) - p + 1) with p = 8
       (bf16), 11 (fp16), 24 (fp32) significant bits, the exponent clamped at the type's smallest normal
       one (-126, -14, -126).
n      the roundings to T the kernel makes between the observable operands and the observed value
       (include/aerognn.h, csrc/common.hpp):
         n = 1  a Linear output (pre[l], hpre, out without LayerNorm), a ReLU output, round(LN(h)), a
                stored segment sum, a ReLU-masked gradient, the LayerNorm backward's gpre, din[s];
         n = 2  the non-ReLU backward act_bwd(x, round_T(dy)), rounded again on store: the inner
                rounding is 1/2 ulp_T(dy) |f'| <= 1 ulp_T(dy f');
         n = 2  round(round(LN(h)) + resid). Here the inner rounding is 1/2 ulp_T at the magnitude of
                LN(h), which is NOT bounded by a multiple of ulp_T(|ref|) when LN(h) and resid cancel.
                check_forward therefore carries it as a-priori error: d' = d + 1/2 ulp_T(|LN(h)| + d),
                then n = 1 with d'. Without cancellation that is at most the n = 2 form; with it, it is
                the bound that actually holds for the documented arithmetic.
d      an a-priori bound of the kernel's fp32 arithmetic, computed in float64 from the same operands,
       u = 2^-24:
         GEMM, inner length K (+ t further addends: bias, the projection rows), any summation order:
             d = 2 (K + 1 + t) u S,   S = |X| |W|^T + |b| (+ |P_s| + |P_d|)
         ReLU: d unchanged. Non-ReLU forward on the stored x = pre[l]: d = 8 u (|x| + |f(x)|) (erff / expf /
             tanhf to a few ulp, the cancellation of 1 + erf at negative x against |x|).
         LayerNorm of h with GEMM error d_h, M features, xh = (h - mean) rstd:
             d_y = rstd |gamma| (d_h + mean(d_h) + |xh| mean(|xh| d_h))                  first order in d_h
                   + u [(M + 1) rstd |gamma| mean|h| + (M + 9) |xh gamma| + 4 (|h| + |mean|) rstd |gamma| + 2 |y|]
             (the fp32 row sums of mean and variance, the elementwise operations).
         Stored SUM / MEAN of c member rows: d = (c + 2) u sum|x| (/ max(c, 1) for MEAN).
         LayerNorm backward from the stored g, hpre, stats (exact operands), gg = g gamma,
         c1 = mean(gg), c2 = mean(gg xh), G = (gg - c1 - xh c2) rstd:
             dxh = u (2 (|h| + |mean|) rstd + 2 |xh|)
             d_G = rstd [4 u (|gg| + |c1| + |xh c2|) + (M + 1) u (mean|gg| + |xh| mean|gg xh|)
                         + dxh |c2| + |xh| mean(|gg| dxh)]
         Backward GEMM a = G_l W_l (inner length M_l): the GEMM bound. ReLU mask: d unchanged.
         Non-ReLU: ref = a f'(x), d = d_a |f'| + |a| d_f' + 4 u |ref| with d_f' = 8 u A, A = (1 + |erf|) / 2
             + |x| pdf (gelu: 1 + erf and 1 - s cancel in fp32), s (1 + |x|) (silu), and for tanh f' = 1 - y^2 with y the STORED act[l] (the
             backward recomputes round_T(tanhf(x)), bitwise the forward's stored value), d_f' = 4 u.
         din[s] = G_0 W_0[:, cols] (+ g with din_resid): the GEMM bound + 2 u (|ref| + |g|).
         g + g2[gidx]: an fp32 add, d = u |g + g2| carried into the LayerNorm backward / gpre[last].
stats and the fp32 outputs formed by sums over rows (LayerNorm partials, agn_wgrad's dW / db) keep the
project's fp32 bars against float64 on the same stored values (check_bar): rel-L2 and max-element
<= 1e-5 for stats, <= 5e-5 for parameter gradients.

emulate_forward / emulate_backward evaluate the kernels' documented arithmetic with torch on the CPU
(fp32 accumulation, the same roundings); tests/test_savechain_cpu.py holds the checks to that and to
mutations of it, so the tolerance is tested without a GPU. Every check prints the worst ratio it saw.
"""
import math

import torch

from golden_util import max_rel, rel_l2

U = 2.0 ** -24
PBITS = {torch.float32: 24, torch.bfloat16: 8, torch.float16: 11}
EMIN = {torch.float32: -126, torch.bfloat16: -126, torch.float16: -14}
STATS_BAR, PGRAD_BAR = 1e-5, 5e-5
WORST = {}  # label -> worst ratio seen in this process (the GPU run's table in DESIGN.md)


def f64(t):
    return t.detach().cpu().double()


def ulp(x, dtype):
    """Spacing of dtype at magnitude x (float64, >= 0), clamped at the smallest normal exponent."""
    _, e = torch.frexp(x)  # x = m 2^e, m in [0.5, 1): floor(log2 x) = e - 1
    e = torch.where(x > 0, e - 1, torch.full_like(e, EMIN[dtype])).clamp_min(EMIN[dtype])
    return torch.ldexp(torch.ones_like(x), e - (PBITS[dtype] - 1))


def tolerance(ref, d, dtype, n=1):
    return (n - 0.5) * ulp(ref.abs() + d, dtype) + d


def check(name, got, ref, d, dtype, n=1, label=None):
    """Assert the tolerance on every element; prints and returns the worst |got - ref| / tolerance."""
    got = f64(got)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), name
    ratio = 0.0
    if got.numel():
        ratio = float(((got - ref).abs() / tolerance(ref, d, dtype, n)).max())
    print(f"  save-chain {name}: worst |got - ref| / tolerance {ratio:.3f} (n = {n}, {got.numel()} elements)")
    if label is not None:
        WORST[label] = max(WORST.get(label, 0.0), ratio)
    assert ratio <= 1.0, (name, ratio)
    return ratio


def check_bar(name, got, ref, bar):
    r, m = rel_l2(f64(got), ref), max_rel(f64(got), ref)
    print(f"  save-chain {name}: rel-L2 {r:.2e}, max-elem {m:.2e} (bar {bar:.0e})")
    assert r <= bar and m <= bar, (name, r, m)
    return max(r, m) / bar


# ------------------------------------------------------------------------------ float64 steps
def gemm(X, W, b=None, extra=()):
    """h = X W^T + b + sum(extra) and the GEMM bound d."""
    h, S = X @ W.T, X.abs() @ W.abs().T
    for t in ([] if b is None else [b]) + list(extra):
        h, S = h + t, S + t.abs()
    return h, 2.0 * (X.shape[1] + 1 + len(extra)) * U * S


def act_f(kind, x):
    if kind == "relu":
        return x.clamp_min(0.0)
    if kind == "gelu":
        return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if kind == "silu":
        return x * torch.sigmoid(x)
    assert kind == "tanh", kind
    return torch.tanh(x)


def act_df(kind, x, y):
    """(f'(x), A) with the fp32 error of f' bounded by 8 u A (tanh: from the stored y, 4 u)."""
    if kind == "gelu":
        cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
        pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
        return cdf + x * pdf, 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)).abs()) + x.abs() * pdf
    if kind == "silu":
        s = torch.sigmoid(x)
        return s * (1.0 + x * (1.0 - s)), s * (1.0 + x.abs())
    assert kind == "tanh", kind
    return 1.0 - y * y, torch.full_like(y, 0.5)


def layer_norm(h, d_h, gamma, beta, eps=1e-5):
    M = h.shape[1]
    mean = h.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((h - mean) ** 2).mean(1, keepdim=True) + eps)
    xh = (h - mean) * rstd
    y = xh * gamma + beta
    rg = rstd * gamma.abs()
    d = rg * (d_h + d_h.mean(1, keepdim=True) + xh.abs() * (xh.abs() * d_h).mean(1, keepdim=True))
    d = d + U * ((M + 1) * rg * h.abs().mean(1, keepdim=True) + (M + 9) * (xh * gamma).abs()
                 + 4.0 * (h.abs() + mean.abs()) * rg + 2.0 * y.abs())
    return mean[:, 0], rstd[:, 0], y, d


def layer_norm_backward(g, d_g, hpre, stats, gamma):
    M = hpre.shape[1]
    mean, rstd = stats[:, :1], stats[:, 1:2]
    xh = (hpre - mean) * rstd
    gg = g * gamma
    c1 = gg.mean(1, keepdim=True)
    c2 = (gg * xh).mean(1, keepdim=True)
    G = (gg - c1 - xh * c2) * rstd
    dxh = U * (2.0 * (hpre.abs() + mean.abs()) * rstd + 2.0 * xh.abs())
    d = rstd * (4.0 * U * (gg.abs() + c1.abs() + (xh * c2).abs())
                + (M + 1) * U * (gg.abs().mean(1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(1, keepdim=True))
                + dxh * c2.abs() + xh.abs() * (gg.abs() * dxh).mean(1, keepdim=True))
    # the error of g itself (an fp32 g + g2) through the same first-order map as the forward's
    dg = d_g * gamma.abs()
    d = d + rstd * (dg + dg.mean(1, keepdim=True) + xh.abs() * (xh.abs() * dg).mean(1, keepdim=True))
    return G, d, xh


def segment_ref(src, rowptr, mean):
    """float64 index_add of src's rows into their receivers, and the bound (c + 2) u sum|x|."""
    rp = rowptr.detach().cpu().long()
    n, cnt = rp.numel() - 1, (rp[1:] - rp[:-1])
    assert int(rp[0]) == 0 and int(rp[-1]) <= src.shape[0] and bool((cnt >= 0).all())
    recv = torch.repeat_interleave(torch.arange(n), cnt)
    rows = src[:int(rp[-1])]
    s = torch.zeros(n, src.shape[1], dtype=torch.float64).index_add_(0, recv, rows)
    sa = torch.zeros(n, src.shape[1], dtype=torch.float64).index_add_(0, recv, rows.abs())
    d = (cnt[:, None] + 2.0) * U * sa
    if mean:
        c = cnt.clamp_min(1)[:, None].double()
        s, d = s / c, d / c
    return s, d


# ------------------------------------------------------------------------------ whole chains
def check_forward(dtype, act, X, W, b, *, acts, pres=None, hpre=None, stats=None, out=None, ln=None, resid=None,
                  extra=(), tag="", label=None):
    """X: float64 [rows, K], the layer-0 operand rows as the kernel read them (stored segment values,
    gathered rows); W / b: float64 parameters (b[l] may be None); extra: float64 addends of layer 0 (the
    gathered projection rows); acts / pres / hpre / stats / out: the kernel's saves, row-major (pres
    for a non-ReLU act); ln: (gamma, beta) float64; resid: float64. Returns the worst ratio."""
    worst, prev, nlin = 0.0, X, len(W)
    for l in range(nlin - 1):
        h, d = gemm(prev, W[l], b[l], extra if l == 0 else ())
        if act == "relu":
            worst = max(worst, check(f"{tag}act[{l}]", acts[l], h.clamp_min(0.0), d, dtype, label=label))
        else:
            worst = max(worst, check(f"{tag}pre[{l}]", pres[l], h, d, dtype, label=label))
            x = f64(pres[l])
            fx = act_f(act, x)
            worst = max(worst, check(f"{tag}act[{l}]", acts[l], fx, 8.0 * U * (x.abs() + fx.abs()), dtype, label=label))
        prev = f64(acts[l])
    y, d = gemm(prev, W[-1], b[-1], extra if nlin == 1 else ())
    if ln is not None:
        if hpre is not None:
            worst = max(worst, check(f"{tag}hpre", hpre, y, d, dtype, label=label))
        mean, rstd, y, d = layer_norm(y, d, ln[0], ln[1])
        if stats is not None:
            check_bar(f"{tag}stats mean", stats[:, 0], mean, STATS_BAR)
            check_bar(f"{tag}stats rstd", stats[:, 1], rstd, STATS_BAR)
    if out is not None:
        if resid is not None:  # round(round(y) + resid): the inner rounding carried in d (module docstring)
            d = d + 0.5 * ulp(y.abs() + d, dtype) + U * (y.abs() + resid.abs())
            y = y + resid
        worst = max(worst, check(f"{tag}out", out, y, d, dtype, label=label))
    return worst


def check_backward(dtype, act, W, g, *, acts, pres=None, hpre=None, stats=None, ln_g=None, gpre, din=(), lnp=None,
                   d_g=None, tag="", label=None):
    """g: float64 upstream gradient (g + g2[gidx] formed in float64; d_g its fp32 bound or None);
    gpre: the kernel's stored pre-activation gradients, row-major; din: [(tensor, resid_flag)] in column
    order; lnp: the LayerNorm partial sums [2 M] (sum g xhat | sum g) already added over blocks in float64."""
    nlin, worst = len(W), 0.0
    d = torch.zeros_like(g) if d_g is None else d_g
    G = g
    if ln_g is not None:
        G, d, xh = layer_norm_backward(g, d, f64(hpre), f64(stats), ln_g)
        if lnp is not None:
            M = g.shape[1]
            check_bar(f"{tag}LayerNorm partials (gamma)", lnp[:M], (g * xh).sum(0), PGRAD_BAR)
            check_bar(f"{tag}LayerNorm partials (beta)", lnp[M:], g.sum(0), PGRAD_BAR)
    worst = max(worst, check(f"{tag}gpre[{nlin - 1}]", gpre[nlin - 1], G, d, dtype, label=label))
    for l in range(nlin - 1, 0, -1):
        a, d = gemm(f64(gpre[l]), W[l].T)
        if act == "relu":
            m = (f64(acts[l - 1]) > 0).double()
            worst = max(worst, check(f"{tag}gpre[{l - 1}]", gpre[l - 1], a * m, d * m, dtype, label=label))
        else:
            fp, A = act_df(act, f64(pres[l - 1]), f64(acts[l - 1]))
            ref = a * fp
            d = d * fp.abs() + a.abs() * 8.0 * U * A + 4.0 * U * ref.abs()
            worst = max(worst, check(f"{tag}gpre[{l - 1}]", gpre[l - 1], ref, d, dtype, n=2, label=label))
    G0, k0 = f64(gpre[0]), 0
    for s, (t, resid) in enumerate(din):
        k = t.shape[1]
        ref, d = gemm(G0, W[0][:, k0:k0 + k].T)
        if resid:
            d = d + 2.0 * U * (ref.abs() + g.abs()) + (0.0 if d_g is None else d_g)
            ref = ref + g
        worst = max(worst, check(f"{tag}din[{s}]", t, ref, d, dtype, label=label))
        k0 += k
    assert k0 in (0, W[0].shape[1]), (k0, W[0].shape)
    return worst


# ------------------------------------------------------------------------------ CPU emulation
def emulate_forward(dtype, act, X, W, b, ln=None, resid=None, bug=None):
    """The forward kernels' arithmetic with torch on the CPU: fp32-accumulated products of the stored
    operands, one rounding per stored value. X, W, resid: tensors of dtype; b, ln: fp32. bug (for the
    mutation checks): "k" drops layer 0's last input column, "ln" takes the LayerNorm sums as if the
    last feature were masked out. Returns dict(acts, pres, hpre, stats, out)."""
    r = {"acts": [], "pres": [], "hpre": None, "stats": None}
    prev, nlin = X, len(W)
    for l in range(nlin):
        xs, ws = prev.float(), W[l].float()
        if bug == "k" and l == 0:
            xs, ws = xs[:, :-1], ws[:, :-1]
        h = xs @ ws.T
        if b[l] is not None:
            h = h + b[l]
        if l == nlin - 1:
            break
        if act == "relu":
            prev = h.clamp_min(0.0).to(dtype)
        else:
            r["pres"].append(h.to(dtype))
            prev = act_f(act, r["pres"][-1].float()).to(dtype)
        r["acts"].append(prev)
    if ln is not None:
        r["hpre"] = h.to(dtype)
        hs = h[:, :-1] if bug == "ln" else h
        mean = hs.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((hs - mean) ** 2).mean(1, keepdim=True) + 1e-5)
        r["stats"] = torch.cat([mean, rstd], 1)
        h = (h - mean) * rstd * ln[0] + ln[1]
    r["out"] = (h.to(dtype).float() + resid.float()).to(dtype) if resid is not None else h.to(dtype)
    return r


def emulate_backward(dtype, act, W, g, fwd, ln_g=None, din_resid=False, bug=None):
    """The backward kernel's arithmetic on the forward's saves `fwd` (emulate_forward's dict):
    dict(gpre, din, lnp). bug "g": the last column of gpre[l] is dropped from each product."""
    nlin = len(W)
    A = g.float()
    r = {"gpre": [None] * nlin, "lnp": None}
    if ln_g is not None:
        mean, rstd = fwd["stats"][:, :1], fwd["stats"][:, 1:2]
        xh = (fwd["hpre"].float() - mean) * rstd
        gg = A * ln_g
        r["lnp"] = torch.cat([(A * xh).sum(0), A.sum(0)])
        A = (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True)) * rstd
    for l in range(nlin - 1, -1, -1):
        r["gpre"][l] = A.to(dtype)
        Gs, ws = r["gpre"][l].float(), W[l].float()
        if bug == "g":
            Gs, ws = Gs[:, :-1], ws[:-1]
        A = Gs @ ws
        if l == 0:
            break
        if act == "relu":
            A = A * (fwd["acts"][l - 1].float() > 0)
        else:
            x, y = fwd["pres"][l - 1].float(), fwd["acts"][l - 1].float()
            A = A.to(dtype).float() * act_df(act, x, y)[0]
    r["din"] = ((A + g.float()) if din_resid else A).to(dtype)
    return r
