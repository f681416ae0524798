"""The save-chain tolerance (tests/savechain.py) checked without a GPU: the kernels' documented
arithmetic is emulated with torch on the CPU (fp32-accumulated products of the stored operands, one
rounding per stored value) for a Linear step, a ReLU and a GELU step, LayerNorm with and without a
residual and a backward step, at H in {32, 64, 128}, K in {1, 6, 17, H, 2H + 5, 3H} and 130 rows. The
emulation must sit inside the tolerance (worst ratio <= 1: the reference arithmetic alone leaves no
share of elements to exempt) and every mutation of it must fall outside:
  * one element moved by 2 ulp of the storage type (3 ulp for the one step with two roundings, the
    non-ReLU backward, whose tolerance is 3/2 ulp either side; bf16 / fp16 only: in fp32 two ulp are less than the
    GEMM bound d of any inner length here, i.e. two valid summation orders differ by more, so that
    mutation is a legal fp32 result and is asserted to PASS instead);
  * two columns swapped;
  * the last row zeroed;
  * the last valid column computed as if masked out (dropped from the product / the LayerNorm sums).
"""
import pytest
import torch

import savechain as S

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["fp32", "bf16", "fp16"]
ROWS = 130


def _ks(H):
    return [1, 6, 17, H, 2 * H + 5, 3 * H]


def _chain(dtype, H, K, nlin, out, ln, seed):
    gen = torch.Generator().manual_seed(seed)
    dims = [K] + [H] * (nlin - 1) + [out]
    X = torch.randn(ROWS, K, generator=gen).to(dtype)
    W = [(torch.randn(dims[l + 1], dims[l], generator=gen) * dims[l] ** -0.5).to(dtype) for l in range(nlin)]
    b = [0.1 * torch.randn(dims[l + 1], generator=gen) for l in range(nlin)]
    lnp = (1.0 + 0.1 * torch.randn(out, generator=gen), 0.1 * torch.randn(out, generator=gen)) if ln else None
    return X, W, b, lnp, gen


def _fwd_check(dtype, act, X, W, b, lnp, resid, r):
    return S.check_forward(dtype, act, S.f64(X), [S.f64(w) for w in W], [S.f64(v) for v in b], acts=r["acts"],
                           pres=r["pres"], hpre=r["hpre"], stats=r["stats"], out=r["out"],
                           ln=None if lnp is None else (S.f64(lnp[0]), S.f64(lnp[1])),
                           resid=None if resid is None else S.f64(resid))


def _ulp2(t, dtype, k=2):
    """The element of largest magnitude moved away from zero by k ulp of its own binade."""
    t = t.clone()
    i = int(t.abs().argmax())
    v = t.view(-1)[i].double()
    step = k * S.ulp(v.abs().reshape(1), dtype)[0]
    t.view(-1)[i] = (v + step * (1.0 if v >= 0 else -1.0)).to(dtype)
    assert t.view(-1)[i].double() != v
    return t


def _swap(t):
    t = t.clone()
    t[:, [0, -1]] = t[:, [-1, 0]]
    return t


def _zero_last_row(t):
    t = t.clone()
    t[-1] = 0
    return t


def _mutations(dtype, t, n=1):
    """(name, mutated tensor, must_fail). A value with n roundings may sit n - 1/2 ulp off, so the
    smallest move every such value must fail is 2 (n - 1/2) ulp: 2 ulp for n = 1, 3 ulp for n = 2."""
    k = 2 * n - 1 if n > 1 else 2
    out = [(f"{k} ulp", _ulp2(t, dtype, k), dtype != torch.float32), ("last row zeroed", _zero_last_row(t), True)]
    if t.shape[1] > 1:
        out.append(("columns swapped", _swap(t), True))
    return out


def _expect(check, must_fail, what):
    if must_fail:
        with pytest.raises(AssertionError):
            check()
        print(f"  mutation '{what}' rejected")
    else:
        check()


def _forward_case(dtype, act, H, K, nlin, out, ln, resid, key, seed):
    """Emulation inside the tolerance; each mutation of the tensor `key` outside."""
    X, W, b, lnp, gen = _chain(dtype, H, K, nlin, out, ln, seed)
    res = torch.randn(ROWS, out, generator=gen).to(dtype) if resid else None
    r = S.emulate_forward(dtype, act, X, W, b, lnp, res)
    worst = _fwd_check(dtype, act, X, W, b, lnp, res, r)
    assert worst <= 1.0

    def put(t):
        m = dict(r, acts=list(r["acts"]))
        if key == "out":
            m["out"] = t
        else:
            m["acts"][0] = t
        return m

    cur = r["out"] if key == "out" else r["acts"][0]
    for name, t, must_fail in _mutations(dtype, cur):
        _expect(lambda: _fwd_check(dtype, act, X, W, b, lnp, res, put(t)), must_fail, name)
    bug = "ln" if (ln and key == "out") else "k"
    if bug == "ln" or K > 1:
        rb = S.emulate_forward(dtype, act, X, W, b, lnp, res, bug=bug)
        _expect(lambda: _fwd_check(dtype, act, X, W, b, lnp, res, dict(rb, stats=r["stats"])), True,
                f"last valid column masked out ({bug})")
    return worst


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("H", [32, 64, 128])
def test_linear_step(H, dtype):
    worst = max(_forward_case(dtype, "relu", H, K, 1, H, False, False, "out", 100 + K) for K in _ks(H))
    print(f"Linear step {dtype} H = {H}: worst ratio {worst:.3f}")
    if dtype != torch.float32:
        assert worst > 0.5  # half an ulp is reached: the tolerance is not slack for the 16-bit types


@pytest.mark.parametrize("act", ["relu", "gelu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("H", [32, 64, 128])
def test_activation_step(H, dtype, act):
    worst = max(_forward_case(dtype, act, H, K, 2, H, False, False, "act", 200 + K) for K in _ks(H))
    print(f"{act} step {dtype} H = {H}: worst ratio {worst:.3f}")


@pytest.mark.parametrize("resid", [False, True], ids=["plain", "resid"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("H", [32, 64, 128])
def test_layer_norm_step(H, dtype, resid):
    worst = max(_forward_case(dtype, "relu", H, K, 1, out, True, resid, "out", 300 + K + out)
                for K in _ks(H) for out in (H, H - 7))
    print(f"LayerNorm step {dtype} H = {H} resid = {resid}: worst ratio {worst:.3f}")


@pytest.mark.parametrize("act", ["relu", "gelu", "tanh"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("H", [32, 64, 128])
def test_backward_step(H, dtype, act):
    """gpre[1] (LayerNorm backward), gpre[0] (the masked / act_bwd gradient) and din with the residual."""
    for K in _ks(H):
        X, W, b, lnp, gen = _chain(dtype, H, K, 2, H, True, 400 + K)
        g = torch.randn(ROWS, H, generator=gen).to(dtype)
        f = S.emulate_forward(dtype, act, X, W, b, lnp, None)
        W64, ln_g = [S.f64(w) for w in W], S.f64(lnp[0])
        resid = K == H

        def chk(r):
            return S.check_backward(dtype, act, W64, S.f64(g), acts=f["acts"], pres=f["pres"], hpre=f["hpre"],
                                    stats=f["stats"], ln_g=ln_g, gpre=r["gpre"], din=[(r["din"], resid)],
                                    lnp=S.f64(r["lnp"]))

        r = S.emulate_backward(dtype, act, W, g, f, lnp[0], din_resid=resid)
        worst = chk(r)
        print(f"backward step {dtype} H = {H} K = {K} {act}: worst ratio {worst:.3f}")
        assert worst <= 1.0
        for key in ("gpre0", "din"):
            n = 2 if (key == "gpre0" and act != "relu") else 1
            for name, t, must_fail in _mutations(dtype, r["gpre"][0] if key == "gpre0" else r["din"], n):
                m = dict(r, gpre=[t, r["gpre"][1]]) if key == "gpre0" else dict(r, din=t)
                if key == "gpre0":  # din follows from the stored gpre[0]: keep the pair consistent
                    m["din"] = S.emulate_backward(dtype, act, W, g, f, lnp[0], din_resid=resid)["din"]
                    _expect(lambda: S.check_backward(dtype, act, W64, S.f64(g), acts=f["acts"], pres=f["pres"],
                                                     hpre=f["hpre"], stats=f["stats"], ln_g=ln_g, gpre=m["gpre"]),
                            must_fail, f"{key} {name}")
                else:
                    _expect(lambda: chk(m), must_fail, f"{key} {name}")
        rb = S.emulate_backward(dtype, act, W, g, f, lnp[0], din_resid=resid, bug="g")
        _expect(lambda: chk(dict(rb, lnp=r["lnp"])), True, "last valid column masked out (g)")


def test_ulp():
    one = torch.tensor([1.0, 1.5, 2.0, 0.75, 0.0, 1e-44], dtype=torch.float64)
    assert S.ulp(one, torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -133, 2.0 ** -133]
    assert S.ulp(one, torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 2.0 ** -24, 2.0 ** -24]
    assert S.ulp(one, torch.float32)[:4].tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24]
    for dt in DTYPES:  # the spacing the type itself has
        x = torch.tensor([0.3, 1.0, 3.7, 100.0]).to(dt)
        nxt = torch.nextafter(x.float(), torch.tensor(float("inf"))) if dt == torch.float32 else None
        if nxt is not None:
            assert torch.equal((nxt - x).double(), S.ulp(x.double(), dt))


def test_decode_tiled_fp32_and_fp16():
    """The fp32 and fp16 AGN_TILED decoders against the layout rule of include/aerognn.h, unit by unit."""
    from maskmatched import decode_tiled
    rows = 70
    for dt, es in ((torch.float32, 4), (torch.float16, 2), (torch.bfloat16, 2)):
        U = 64 * es // 16
        per = 16 // es
        buf = torch.zeros(96 * 128, dtype=dt)
        want = torch.arange(rows * 128, dtype=torch.float32).reshape(rows, 128) % 2039
        for r in range(rows):
            for i in range(U):
                for h in range(2):
                    unit = ((r // 32) * U + i) * 64 + (r % 32) + 32 * h
                    feats = ([8 * i + 4 * h + e for e in range(4)] if es == 4 else
                             [16 * i + 4 * h + e for e in range(4)] + [16 * i + 8 + 4 * h + e for e in range(4)])
                    buf[unit * per:(unit + 1) * per] = want[r, feats].to(dt)
        got = decode_tiled(buf.reshape(96, 128), rows)
        assert got.dtype == dt and torch.equal(got.float(), want.to(dt).float())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_residual_inner_rounding(dtype):
    """Why round(round(LN(h)) + resid) carries its inner rounding in d (savechain's docstring): with
    n = 2 at the magnitude of the SUM, the documented arithmetic itself lands outside the tolerance
    wherever LN(h) and resid cancel (the inner half-ulp is taken at |LN(h)|, not at |LN(h) + resid|);
    carried as a-priori error it is inside, and no looser than n = 2 where nothing cancels."""
    H = 64
    X, W, b, lnp, gen = _chain(dtype, H, H, 1, H, True, 77)
    res = torch.randn(ROWS, H, generator=gen).to(dtype)
    r = S.emulate_forward(dtype, "relu", X, W, b, lnp, res)
    h, d = S.gemm(S.f64(X), S.f64(W[0]), S.f64(b[0]))
    _, _, y, d = S.layer_norm(h, d, S.f64(lnp[0]), S.f64(lnp[1]))
    ref, got = y + S.f64(res), S.f64(r["out"])
    literal = float(((got - ref).abs() / S.tolerance(ref, d, dtype, 2)).max())
    d1 = d + 0.5 * S.ulp(y.abs() + d, dtype)
    carried = float(((got - ref).abs() / S.tolerance(ref, d1, dtype, 1)).max())
    print(f"round(round(LN) + resid) {dtype}: n = 2 at |sum| {literal:.2f}, inner rounding carried in d {carried:.3f}")
    assert literal > 1.0 and carried <= 1.0
    calm = (y * S.f64(res) > 0)  # same sign: no cancellation
    assert bool((S.tolerance(ref, d1, dtype, 1)[calm] <= S.tolerance(ref, d, dtype, 2)[calm] * (1 + 1e-12)).all())
