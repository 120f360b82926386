"""Per-element checker for squeeze_excite (a helper module like
ops_checks.py, not collected as tests).

`check_squeeze_excite(x, w1, b1, w2, b2, act, got)` asserts a derived bound
on every element of `got` against a float64 truth `t` computed from the same
(already rounded) inputs, and returns the worst observed error over its
bound; the assertion never depends on that figure. With u = 2^-24 (one fp32
operation), u_b = 2^-8 (one rounding to bf16; 0 for fp32 tensors) and
gamma_k = k*u / (1 - k*u), all |.| applied per element and the products
being the matrix products of the op:

    ds = gamma_{HW+2} * mean|x|
    dz = |w1|.ds + gamma_{C+2} * (|w1|.(|s| + ds) + |b1|)
    dv = |w2|.dz + gamma_{Cr+2} * (|w2|.(|z| + dz) + |b2|)
    dg = dv / 6 + 3u
    |got - t| <= u_b*|t| + (1 + u_b) * |x| * (dg + u)

ds: HW - 1 adds in any order and the division (or reciprocal and product).
dz: the error of s carried through |w1|, plus a dot product of length C and
the bias add, in any order, on the perturbed s; the ReLU is 1-Lipschitz.
dv likewise over Cr. dg: the hardsigmoid is 1/6-Lipschitz with values in
[0, 1], and its own add, clamp and product cost at most 3u absolutely. The
last line is the product x * g (one u) and the rounding to the output
dtype. A gate that was rounded to bf16 on the way carries 2^-9 and breaks
this by two orders of magnitude, which is what the bound is for. No figure
here comes from a measurement."""

import torch

U = 2.0 ** -24
U_B = 2.0 ** -8


def _gamma(k):
    return k * U / (1.0 - k * U)


def truth64(x, w1, b1, w2, b2, act):
    """(s, z, g, y) of the op in float64 from the given tensors."""
    x, w1, w2 = x.double().cpu(), w1.double().cpu(), w2.double().cpu()
    s = x.mean(dim=(1, 2))
    z = s @ w1.t()
    if b1 is not None:
        z = z + b1.double().cpu()
    if act == "relu":
        z = z.clamp(min=0)
    else:
        assert act == "none", act
    v = z @ w2.t()
    if b2 is not None:
        v = v + b2.double().cpu()
    g = (v + 3).clamp(0, 6) / 6
    return s, z, g, x * g[:, None, None, :]


def check_squeeze_excite(x, w1, b1, w2, b2, act, got, what="squeeze_excite"):
    assert got.dtype == x.dtype and got.shape == x.shape, (got.dtype,
                                                           got.shape)
    assert x.dtype in (torch.bfloat16, torch.float32)
    ub = U_B if x.dtype == torch.bfloat16 else 0.0
    n, h, w, c = x.shape
    cr = w1.shape[0]
    if x.numel() == 0:
        return 0.0
    s, z, g, t = truth64(x, w1, b1, w2, b2, act)
    xa = x.double().cpu().abs()
    a1, a2 = w1.double().cpu().abs(), w2.double().cpu().abs()
    ab1 = b1.double().cpu().abs() if b1 is not None else torch.zeros(cr)
    ab2 = b2.double().cpu().abs() if b2 is not None else torch.zeros(c)
    ds = _gamma(h * w + 2) * xa.mean(dim=(1, 2))
    dz = ds @ a1.t() + _gamma(c + 2) * ((s.abs() + ds) @ a1.t() + ab1)
    dv = dz @ a2.t() + _gamma(cr + 2) * ((z.abs() + dz) @ a2.t() + ab2)
    dg = dv / 6 + 3 * U
    bound = ub * t.abs() + (1 + ub) * xa * (dg + U)[:, None, None, :]
    err = (got.double().cpu() - t).abs()
    bad = err > bound
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {err.numel()} elements over the "
            f"bound, first at {i}: got {got[i].item()!r}, truth "
            f"{t[i].item()!r}, err {err[i].item():.3e} > bound "
            f"{bound[i].item():.3e}")
    ok = bound > 0
    return (err[ok] / bound[ok]).max().item() if ok.any() else 0.0
