"""Shared by the activation tests (tests/test_act_cpu.py, tests/test_gpu_act.py) and the goldens script
(tools/make_goldens_act.py); test infrastructure, not product code. The names of the elementwise
torch.nn.functional activations the MLP chains accept, their kinks, the fixed elementwise grid, ulp and
relative-error measures, and the choice of kink-free rows for a chain. The reference is always torch on
the CPU in float64 (F.<name> and its autograd)."""
import torch
import torch.nn.functional as F

from chainref import ref_chain

OLD = ("relu", "gelu", "silu", "tanh")
NEW = ("relu6", "hardtanh", "leaky_relu", "elu", "celu", "selu", "hardsigmoid", "hardswish", "softplus", "softsign",
       "sigmoid", "logsigmoid", "mish", "tanhshrink")
REFUSED = ("softmax", "log_softmax", "glu", "rrelu", "prelu", "threshold", "hardshrink", "softshrink")

# where the derivative (or, for the clamps, the function's slope) jumps
KINKS = {"relu": (0.0,), "relu6": (0.0, 6.0), "hardtanh": (-1.0, 1.0), "leaky_relu": (0.0,), "elu": (0.0,),
         "celu": (0.0,), "selu": (0.0,), "hardsigmoid": (-3.0, 3.0), "hardswish": (-3.0, 3.0)}
ALL_KINKS = (0.0, 1.0, -1.0, 3.0, -3.0, 6.0)

MANT = {torch.float64: 52, torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}
MIN_EXP = {torch.float64: -1022, torch.float32: -126, torch.bfloat16: -126, torch.float16: -14}
INT = {torch.float64: torch.int64, torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def tiny(dtype):
    """The smallest subnormal of dtype, as a Python float."""
    return 2.0 ** (MIN_EXP[dtype] - MANT[dtype])


def ulp(v, dtype):
    """The spacing of dtype at |v| (v float64), the subnormal spacing below the smallest normal."""
    _, e = torch.frexp(v.abs())
    e = torch.where(v == 0, torch.full_like(e, MIN_EXP[dtype]), e - 1).clamp_min(MIN_EXP[dtype])
    return torch.ldexp(torch.ones_like(v), e - MANT[dtype])


def neighbours(k, dtype):
    """[the value below k, k, the value above k] in dtype."""
    if k == 0.0:
        return [-tiny(dtype), 0.0, tiny(dtype)]
    v = torch.tensor([k], dtype=dtype)
    i = v.view(INT[dtype])
    near, far = float((i - 1).view(dtype)), float((i + 1).view(dtype))  # towards 0, away from 0
    return [near, k, far] if k > 0 else [far, k, near]


def grid(dtype, seed=20240607):
    """The fixed elementwise input: +-{0, smallest subnormal, 1e-30, 1e-4, 0.5, 1, 3, 6, 20, 88, 100, 1e4},
    every kink value with its two neighbours in dtype, and 4,096 N(0, 3) draws; (x in dtype, the index range
    of the kink points). Values are rounded to dtype (1e-30 is 0 in fp16)."""
    mags = [0.0, tiny(dtype), 1e-30, 1e-4, 0.5, 1.0, 3.0, 6.0, 20.0, 88.0, 100.0, 1e4]
    head = [s * m for m in mags for s in (1.0, -1.0)]
    kinks = [v for k in ALL_KINKS for v in neighbours(k, dtype)]
    g = torch.Generator().manual_seed(seed)
    draws = 3.0 * torch.randn(4096, generator=g, dtype=torch.float64)
    x = torch.cat([torch.tensor(head + kinks, dtype=torch.float64), draws]).to(dtype)
    return x, (len(head), len(head) + len(kinks))


def upstream(n, dtype, seed=7):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dtype)


def f64_ref(name, x, dy, y_stored=None):
    """torch's CPU float64 F.<name>(x) and dy * f'(x) by its autograd, on the values of x and dy (any
    dtype, upcast exactly). y_stored (sigmoid, tanh in 16 bits): the derivative from that output, as the
    kernels take it from the rounded output they stored."""
    xx = x.detach().double().requires_grad_(True)
    y = getattr(F, name)(xx)
    y.backward(dy.detach().double())
    gx = xx.grad
    if y_stored is not None:
        ys = y_stored.detach().double()
        gx = dy.double() * ((1.0 - ys) * ys if name == "sigmoid" else (1.0 - ys * ys))
    return y.detach(), gx


EPS64 = 2.0 ** -52


def ref_noise(name, backward, x, dy):
    """float64 only: the absolute rounding noise of torch's OWN float64 result, taken off |got - ref| before
    the relative error is formed. It is zero for every function but tanhshrink, which torch evaluates as
    x - tanh(x) (tanh(x) carries an error of eps |x|, the difference is ~ x^3 / 3: at 1e-30 torch returns 0)
    and differentiates as dy - dy (1 - tanh^2) (eps |dy| for a value of dy x^2). 4 eps |x| and 4 eps |dy|:
    the reference's noise and no more; against a reference that does not cancel (tanhshrink_exact)
    nothing is taken off."""
    if name != "tanhshrink":
        return torch.zeros_like(x)
    return 4.0 * EPS64 * (dy.abs() if backward else x.abs())


def rel_err(got, ref, noise=None):
    """|got - ref| / |ref| per element (0 where they are equal, inf where only ref is 0)."""
    d = (got.double() - ref).abs()
    if noise is not None:
        d = (d - noise).clamp_min(0.0)
    return torch.where(d == 0, torch.zeros_like(d), d / ref.abs())


def tanhshrink_exact(x, dy):
    """x - tanh(x) and dy tanh(x)^2 for float64 x, dy without cancellation: 60-digit decimal arithmetic,
    tanh = (E - 1) / (E + 1) with E = exp(2 x) from 1e-3 up (the difference loses 10 of the 60 digits at
    most there), below that the odd series to x^15 in exact rationals (next term 1e-48 of the first).
    Rounded to float64 once, at the end."""
    import decimal
    from fractions import Fraction
    ctx = decimal.Context(prec=60, Emin=-999999999, Emax=999999999)
    coef = [Fraction(1, 3), Fraction(-2, 15), Fraction(17, 315), Fraction(-62, 2835), Fraction(1382, 155925),
            Fraction(-21844, 6081075), Fraction(929569, 638512875)]
    ys, gs = [], []
    for xv, dv in zip(x.tolist(), dy.tolist()):
        if abs(xv) < 1e-3:
            xf = Fraction(xv)
            shrink = sum(c * xf ** (3 + 2 * i) for i, c in enumerate(coef))
            t = xf - shrink
            ys.append(float(shrink))
            gs.append(float(Fraction(dv) * t * t))
        else:
            X = decimal.Decimal(xv)
            E = ctx.exp(ctx.multiply(X, 2))
            t = ctx.divide(ctx.subtract(E, 1), ctx.add(E, 1))
            ys.append(float(ctx.subtract(X, t)))
            gs.append(float(ctx.multiply(decimal.Decimal(dv), ctx.multiply(t, t))))
    return torch.tensor(ys, dtype=torch.float64), torch.tensor(gs, dtype=torch.float64)


# ------------------------------------------------------------------------------ kink-free rows of a chain
def _near(sd, x, act, band):
    """Rows of x with a hidden pre-activation (float64 formula on sd, x as given) within band * std of a
    kink of act: chainref.kink_free_rows' margin, around every kink."""
    _, pres = ref_chain(sd, x, act)
    near = torch.zeros(x.shape[0], dtype=torch.bool)
    for t in pres:
        s = band * (t.std() if t.numel() > 1 else 1.0)
        for k in KINKS.get(act, ()):
            near |= ((t - k).abs() < s).any(1)
    return near


def _near_rounded(sd, x, act, dtype):
    """The same for the chain on operands rounded to a 16-bit dtype, with the margin 2 eps_T max(|kink|,
    spread) (tests/dropoutref.py kink_free_rows' 2 eps_T band): the kernels round every stored activation
    and pre-activation to dtype, so their pre-activations are about eps_T of the spread away from the
    float64 formula's, and an element that close to a kink may lie on its other side, which moves a
    gradient by percents whichever code computes it."""
    sdr = {k: v.to(dtype) for k, v in sd.items()}
    xr = x.to(dtype)
    _, pres = ref_chain(sdr, xr, act)
    near = torch.zeros(x.shape[0], dtype=torch.bool)
    for t in pres:
        s = float(t.std()) if t.numel() > 1 else 1.0
        for k in KINKS.get(act, ()):
            near |= ((t - k).abs() < 2.0 * 2.0 ** -MANT[dtype] * max(abs(k), s)).any(1)
    return near


def kink_free_select(sd, cand, act, need, band=1e-5, rounded=(torch.bfloat16, torch.float16)):
    """The first `need` rows of the candidates `cand` whose hidden pre-activations stay outside the margin
    of every kink of act, in float64 on the operands as given and on the operands rounded to each dtype of
    `rounded`. Decided by the float64 formula alone. Raises if there are fewer than `need`."""
    def near(x):
        out = _near(sd, x, act, band)
        for dt in rounded:
            out |= _near_rounded(sd, x, act, dt)
        return out

    pool = (~near(cand)).nonzero().flatten().tolist()
    keep, pool = pool[:need], pool[need:]
    # the margin is relative to the spread of the rows compared, so it must hold for the kept rows alone:
    # a row that fails among them is replaced by the next candidate, until none does
    while len(keep) == need:
        bad = near(cand[keep])
        if not bad.any():
            return cand[keep].clone()
        keep = [i for i, b in zip(keep, bad.tolist()) if not b]
        keep, pool = keep + pool[:need - len(keep)], pool[need - len(keep):]
    raise AssertionError(f"{act}: fewer than {need} kink-free rows among {cand.shape[0]} candidates")
