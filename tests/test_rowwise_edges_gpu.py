"""Row-wise HIP kernels (LayerNorm, cross-entropy, embedding forward, activation/dropout backward)
at the smallest shapes that reach every instantiation, tail and reduce path, against plain float64
torch on the CPU built from the same inputs and the same dropout mask (sparkmi.ops.rng).

Where a bound is not simply quoted from an existing test it is derived here:

* LayerNorm dgamma/dbeta: a sum of terms t_i (plus the old gradient g0) carried in fp32 has error
  <= c * (sum |t_i| + |g0|); c = 2e-6 (+ 1e-6 absolute) is what tests/test_f32_gpu.py allows fp32
  GEMM sums.  bf16: dy and the saved pre-norm sum are bf16 on both sides, the partial sums stay
  fp32, so the one bf16 error is x_hat computed from the rounded saved sum: c = 2^-7.  (The rounding
  is relative to |x|, not to |x - mean|, so the bound assumes rows whose mean is small beside their
  spread, as with the N(0, 1) inputs here.  Measured on an MI355X: at most 0.62 of the bound, at
  (1, 8) where the sum has one term; at most 0.11 of the fp32 bound.)
* Cross-entropy fp32: loss within 1e-6 * max(1, max_row |lse|) + 1e-6 (a few ulp of lse);
  gradient within 1e-6 + 2e-5 |ref| for unit-scale logits and 2e-5 + 2e-4 |ref| for logits of
  scale 30 and for a row shifted by +1e4 (ulp(lse) and the rounding of the exp2 argument grow with
  |lse| and |x - lse|).  The shifted row is taken at V = 8200: lse ~ 1e4 is stored in fp32 with up to
  half an ulp(1e4) = 4.9e-4 of rounding, which is the relative error of every softmax entry p of the
  row, so the gradient bound needs 4.9e-4 p s <= 2e-5 + 2e-4 p s (s = dloss / count = 0.7), p < 0.098;
  with N(0, 1) logits at V = 8200 no entry comes near that.
  bf16 logits: same loss bound (fp32 math on identical inputs), gradient within one bf16 ulp,
  1e-6 + 2^-7 |ref|.
* A valid row's fp32 gradient sums to s * (sum_i p_i - 1), which is s times the relative error of
  exp(-lse): checked against 1e-6 * sqrt(V) for unit-scale fp32 logits (|lse| < 32, half an ulp is
  below 1e-6).  It does not hold per construction for bf16 gradients (each entry is rounded to
  2^-9 relative on its own) nor at |lse| >= 64 (half an ulp of lse alone exceeds it), so it is
  asserted for unit-scale fp32 rows only.
* "within one bf16 ulp of float64": |got - ref| <= 2^(floor(log2 |ref|) - 7), and exactly 0 where
  the reference is 0 (dropped elements).
"""
import functools
import math
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from sparkmi import _native  # noqa: E402
from sparkmi.ops import _grad  # noqa: E402
from sparkmi.ops import planes  # noqa: E402
from sparkmi.ops import rng as R  # noqa: E402
from sparkmi.ops.embedding import embedding  # noqa: E402
from sparkmi.ops.layernorm import add_dropout_layernorm  # noqa: E402
from sparkmi.ops.loss import cross_entropy  # noqa: E402

dev = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="fp32"), pytest.param(BF16, id="bf16")]


def _scale32(p):
    """The dropout scale as the kernels receive it (a float argument)."""
    return float(torch.tensor(R.scale(p), dtype=F32))


def _within(got, ref, bound, msg):
    """|got - ref| <= bound elementwise (float64, CPU); prints the worst error / bound."""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.double()
    assert torch.isfinite(got).all(), f"{msg}: non-finite output"
    err = (got - ref).abs()
    bound = bound if torch.is_tensor(bound) else torch.full_like(ref, bound)
    bad = err > bound
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{msg}: max err {float(err.max()) if err.numel() else 0.0:.3g}, worst err/bound {worst:.3g}")
    assert not bad.any(), (f"{msg}: {int(bad.sum())} / {bad.numel()} outside the bound, max err {float(err.max()):.4g}, "
                           f"worst err/bound {worst:.3g}")


def _close(got, ref, atol, rtol, msg):
    _within(got, ref, atol + rtol * ref.double().abs(), msg)


def _bf16_ulp(ref):
    ref = ref.double()
    _, ex = torch.frexp(ref.abs())  # |ref| = m * 2^ex, m in [0.5, 1): bf16 spacing 2^(ex - 8)
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), ex - 8))


def _bits(t):
    return t.contiguous().view(torch.int16)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))  # the same inputs in every process


# ---------------------------------------------------------------------------------------------
# 1. LayerNorm
# ---------------------------------------------------------------------------------------------
LN_SHAPES = [(1, 8), (7, 96), (9, 512), (13, 520), (11, 1024), (6, 1032), (5, 1536), (5, 2048)]
LN_SEED, LN_SALT = 7, 1234


@functools.lru_cache(maxsize=None)
def _ln_case(M, D, p, has_r, bf16, tag=0):
    """Inputs (CPU, in the activation dtype) and the float64 reference; shared, never modified."""
    g = _gen("ln", M, D, p, has_r, bf16, tag)
    dt = BF16 if bf16 else F32
    c = {"M": M, "D": D, "p": p, "dt": dt}
    c["h"] = torch.randn(M, D, generator=g).to(dt)
    c["r"] = torch.randn(M, D, generator=g).to(dt) if has_r else None
    c["gamma"] = torch.randn(D, generator=g) * 0.5 + 1
    c["beta"] = torch.randn(D, generator=g) * 0.1
    c["dy"] = torch.randn(M, D, generator=g).to(dt)
    c["g0"] = torch.randn(D, generator=g)  # gamma.grad / beta.grad before the backward: non-zero
    c["b0"] = torch.randn(D, generator=g)
    x = c["h"].double()
    keep = None
    if p > 0:
        keep = R.keep_mask((M, D), p, LN_SEED, LN_SALT).double() * _scale32(p)
        x = x * keep
    if has_r:
        x = x + c["r"].double()
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + 1e-5)
    xhat = (x - mean) * rstd
    gam = c["gamma"].double()
    dy = c["dy"].double()
    gl = dy * gam
    dx = rstd * (gl - gl.mean(-1, keepdim=True) - xhat * (gl * xhat).mean(-1, keepdim=True))
    c["ref"] = {"y": xhat * gam + c["beta"].double(), "dres": dx, "dh": dx * keep if keep is not None else dx,
                "dgamma": c["g0"].double() + (dy * xhat).sum(0), "dbeta": c["b0"].double() + dy.sum(0),
                "Sg": (dy * xhat).abs().sum(0) + c["g0"].double().abs(),
                "Sb": dy.abs().sum(0) + c["b0"].double().abs()}
    return c


class _LN:
    """One LayerNorm on the GPU, forward done; backward() / results() after the backward."""

    def __init__(self, c, mark=False):
        self.c = c
        self.h = c["h"].to(dev).requires_grad_()
        if mark:
            planes.mark_grad_planes_ok(self.h)
        self.r = c["r"].to(dev).requires_grad_() if c["r"] is not None else None
        self.gamma = torch.nn.Parameter(c["gamma"].to(dev))
        self.beta = torch.nn.Parameter(c["beta"].to(dev))
        self.gamma.grad, self.beta.grad = c["g0"].to(dev), c["b0"].to(dev)
        self.cap = []
        self.h.register_hook(self.cap.append)  # the dh tensor the backward returns (carries its planes)
        self.rng = R.DropoutRNG(LN_SEED).to(dev)
        self.y = add_dropout_layernorm(self.h, self.r, self.gamma, self.beta, c["p"], self.rng, LN_SALT)
        assert self.y.dtype == c["dt"]
        self.dy = c["dy"].to(dev)

    def results(self):
        return {"y": self.y.detach(), "dh": self.cap[0], "dres": self.r.grad if self.r is not None else None,
                "dgamma": self.gamma.grad, "dbeta": self.beta.grad}


def _ln_backward(lns):
    torch.autograd.backward([l.y for l in lns], [l.dy for l in lns])
    torch.cuda.synchronize()
    assert not _grad.pending()
    return [l.results() for l in lns]


def _ln_check(c, out, what=("y", "dh", "dres", "dgamma", "dbeta")):
    ref, bf16 = c["ref"], c["dt"] == BF16
    tag = f"ln {c['M']}x{c['D']} p={c['p']} {'bf16' if bf16 else 'fp32'}"
    for k in what:
        if k == "dres" and out["dres"] is None:
            continue
        if k == "y":  # bounds of test_layernorm / test_layernorm_f32
            _close(out[k], ref[k], *((3e-2, 2e-2) if bf16 else (2e-5, 1e-5)), f"{tag} y")
        elif k in ("dh", "dres"):
            _close(out[k], ref[k], *((3e-2, 3e-2) if bf16 else (2e-5, 1e-5)), f"{tag} {k}")
        else:
            S = ref["Sg" if k == "dgamma" else "Sb"]
            _within(out[k], ref[k], (2.0 ** -7 if bf16 else 2e-6) * S + 1e-6, f"{tag} {k}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("has_r", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("M,D", LN_SHAPES)
def test_ln_edge_shapes(M, D, p, has_r, dtype):
    """Every ln_fwd / ln_bwd instantiation the backward supports, row tails (M % 8 != 0), the col < D
    tail inside a vector group, residual=None, accumulation onto non-zero gamma.grad / beta.grad;
    fp32: y's and dh's split planes are bit-equal to a split of the fp32 values (none at D % 32)."""
    c = _ln_case(M, D, p, has_r, dtype == BF16)
    ln = _LN(c)
    yp = planes.cached(ln.y)
    out, = _ln_backward([ln])
    _ln_check(c, out)
    dhp = planes.cached(out["dh"])
    if dtype == F32 and D % 32 == 0:
        assert yp is not None and dhp is not None
        for t, P, name in ((out["y"], yp, "y"), (out["dh"], dhp, "dh")):
            assert not planes.planes_only(t)
            assert P.shape == (3, M, D), name
            assert torch.equal(_bits(P), _bits(planes.split(t.detach().reshape(M, D)))), f"{name} planes"
    else:
        assert yp is None and dhp is None


@pytest.mark.parametrize("M,D", [(7, 96), (9, 512), (11, 1024), (5, 1536), (5, 2048)])
def test_ln_planes_only_matches_full(M, D):
    """With the input marked planes-ok the backward writes dh as planes only: the same planes as
    the full run bit for bit, planes.f32 rebuilds the full run's fp32 dh exactly, and the other
    outputs do not change."""
    c = _ln_case(M, D, 0.1, True, False)
    full, = _ln_backward([_LN(c)])
    only, = _ln_backward([_LN(c, mark=True)])
    assert planes.planes_only(only["dh"]) and not planes.planes_only(full["dh"])
    Pf, Po = planes.cached(full["dh"]), planes.cached(only["dh"])
    assert Pf is not None and Po is not None
    assert torch.equal(_bits(Po), _bits(Pf))
    assert torch.equal(planes.f32(only["dh"]), full["dh"])
    assert not planes.planes_only(only["dh"])
    for k in ("y", "dres", "dgamma", "dbeta"):
        assert torch.equal(only[k], full[k]), k
    _ln_check(c, only)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("defer", [False, True], ids=["immediate", "deferred"])
@pytest.mark.parametrize("M", [515, 2051, 8203])
def test_ln_reduce_paths(M, defer, dtype, monkeypatch):
    """D = 8, 8 rows per block: nb = 65 / 257 / 1026 partial rows.  Immediate fold: the 4 / 8 / 16
    row-group atomic paths of colsum2_kernel with a ragged last group; deferred fold:
    colsum2_multi_kernel, fixed order, so two runs are bitwise equal."""
    monkeypatch.setattr(_grad, "LN_DEFER", defer)
    c = _ln_case(M, 8, 0.1, True, dtype == BF16)
    out, = _ln_backward([_LN(c)])
    _ln_check(c, out)
    if defer:
        again, = _ln_backward([_LN(c)])
        for k in ("dgamma", "dbeta", "dh", "dres"):
            assert torch.equal(out[k], again[k]), k


@pytest.mark.parametrize("dtype", DTYPES)
def test_ln_deferred_mixed_widths(dtype):
    """Three LayerNorms of D = 8 / 1032 / 96 folded by one colsum2_multi launch (grid sized for the
    widest; the blocks past a narrower one's D return early)."""
    assert _grad.LN_DEFER
    cs = [_ln_case(M, D, 0.1, True, dtype == BF16) for M, D in ((13, 8), (6, 1032), (7, 96))]
    outs = _ln_backward([_LN(c) for c in cs])
    for c, o in zip(cs, outs):
        _ln_check(c, o)
    again = _ln_backward([_LN(c) for c in cs])
    for o, a in zip(outs, again):
        assert torch.equal(o["dgamma"], a["dgamma"]) and torch.equal(o["dbeta"], a["dbeta"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_ln_deferred_33_in_one_backward(dtype):
    """33 LayerNorms in one backward: _flush_ln splits the batch at 32."""
    assert _grad.LN_DEFER
    cs = [_ln_case(5, 8, 0.1, True, dtype == BF16, tag=i) for i in range(33)]
    outs = _ln_backward([_LN(c) for c in cs])
    for c, o in zip(cs, outs):
        _ln_check(c, o)
    again = _ln_backward([_LN(c) for c in cs])
    for o, a in zip(outs, again):
        assert torch.equal(o["dgamma"], a["dgamma"]) and torch.equal(o["dbeta"], a["dbeta"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_ln_width_not_multiple_of_8_raises(dtype):
    h = torch.randn(4, 100, device=dev).to(dtype)
    gamma, beta = torch.ones(100, device=dev), torch.zeros(100, device=dev)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        add_dropout_layernorm(h, h.clone(), gamma, beta)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [2056, 4096])
def test_ln_wide_rows_forward_only(D, dtype):
    """2048 < D <= 4096: ln_fwd_kernel<8> under no_grad matches float64; with a gradient required the
    call is refused in the forward (the backward has no kernel that wide), before any launch."""
    c = _ln_case(5, D, 0.1, True, dtype == BF16)
    h, r = c["h"].to(dev), c["r"].to(dev)
    gamma, beta = torch.nn.Parameter(c["gamma"].to(dev)), torch.nn.Parameter(c["beta"].to(dev))
    rng = R.DropoutRNG(LN_SEED).to(dev)
    with torch.no_grad():
        y = add_dropout_layernorm(h, r, gamma, beta, c["p"], rng, LN_SALT)
    assert not y.requires_grad
    _ln_check(c, {"y": y}, what=("y",))
    for needs in ("h", "r", "gamma"):
        hh = h.clone().requires_grad_(needs == "h")
        rr = r.clone().requires_grad_(needs == "r")
        g = gamma if needs == "gamma" else gamma.detach()
        with pytest.raises(ValueError, match="no backward kernel"):
            add_dropout_layernorm(hh, rr, g, beta.detach(), c["p"], rng, LN_SALT)
    assert gamma.grad is None and not _grad.pending()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# 2. Cross-entropy
# ---------------------------------------------------------------------------------------------
UP = 3.5  # upstream gradient: (loss * 3.5).backward()
CE_V = [2, 7, 8, 45, 255, 256, 264, 2047, 2048, 8192, 8200, 10007]


def _ce_ref(x, lab, ignore):
    xd = x.double()
    M, V = xd.shape
    lse = torch.logsumexp(xd, -1)
    valid = lab != ignore
    cnt = int(valid.sum())
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    rl = (lse - xd.gather(1, safe[:, None]).squeeze(1)) * valid
    p = torch.exp(xd - lse[:, None])
    p[torch.arange(M), safe] -= 1.0
    if cnt == 0:
        return torch.zeros((), dtype=torch.float64), torch.zeros_like(xd), lse, valid
    return rl.sum() / cnt, p * (valid.double() * UP / cnt)[:, None], lse, valid


def _ce_gpu(x, lab, ignore, mark=False):
    xg = x.to(dev).requires_grad_()
    if mark:
        planes.mark_grad_planes_ok(xg)
    cap = []
    xg.register_hook(cap.append)
    loss = cross_entropy(xg, lab.to(dev), ignore_index=ignore)
    (loss * UP).backward()
    torch.cuda.synchronize()
    return loss.detach(), cap[0]


def _ce_check(x, lab, ignore, wide, msg, zero_sum=True):
    """wide: the bound for logits of scale 30 / a shifted row; zero_sum: unit-scale fp32 rows."""
    loss, grad = _ce_gpu(x, lab, ignore)
    rl, rg, lse, valid = _ce_ref(x, lab, ignore)
    V = x.shape[1]
    _within(loss, rl, 1e-6 * max(1.0, float(lse.abs().max())) + 1e-6, f"{msg} loss")
    if x.dtype == BF16:
        _close(grad, rg, 1e-6, 2.0 ** -7, f"{msg} grad")
    elif wide:
        _close(grad, rg, 2e-5, 2e-4, f"{msg} grad")
    else:
        _close(grad, rg, 1e-6, 2e-5, f"{msg} grad")
    g = grad.detach().double().cpu()
    assert not g[~valid].any(), f"{msg}: ignored rows must have an exactly zero gradient"
    if zero_sum and x.dtype == F32 and not wide and valid.any():
        s = g[valid].sum(-1).abs().max()
        print(f"{msg}: max |row gradient sum| {float(s):.3g} (bound {1e-6 * math.sqrt(V):.3g})")
        assert float(s) <= 1e-6 * math.sqrt(V), (msg, float(s))
    return loss, grad


def _labels(M, V, ignore, g):
    """Random labels with 0, V-1 and one ignored row (ignore = 0: the label-0 rows are the ignored ones)."""
    lab = torch.randint(0, V, (M,), generator=g)
    lab[0] = 0
    if M > 1:
        lab[1] = V - 1
    if M > 2:
        lab[2] = ignore
    if M == 1:
        lab[0] = V - 1
    return lab


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", CE_V)
def test_ce_vocab_sizes(V, dtype):
    """The 16-byte path (V % 8 == 0, one or several chunks of 8192), the scalar whole-row path (V % 8),
    V smaller than a wave (lanes and waves that merge (-inf, 0)); fp32 logits of scale 1 and 30."""
    for scale in ((1.0, 30.0) if dtype == F32 else (1.0,)):
        for ignore in (0, -100):
            g = _gen("ce", V, scale, ignore)
            x = (torch.randn(5, V, generator=g) * scale).to(dtype)
            _ce_check(x, _labels(5, V, ignore, g), ignore, scale != 1.0, f"ce V={V} scale={scale} ignore={ignore}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,V", [(1, 45), (1025, 8)])
def test_ce_row_counts(M, V, dtype):
    """One row; more rows than the finalize block has threads (its loop's second trip)."""
    for ignore in (0, -100):
        g = _gen("ce rows", M, V, ignore)
        x = torch.randn(M, V, generator=g).to(dtype)
        _ce_check(x, _labels(M, V, ignore, g), ignore, False, f"ce {M}x{V} ignore={ignore}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", CE_V)
def test_ce_spike(V, dtype):
    """One logit 12 above the row's maximum at every chunk / vector / tail boundary position: a
    dropped, doubled or misplaced element changes lse and the gradient by orders of magnitude.
    Each position once with the label on the spike and once with it elsewhere."""
    pos = sorted({q for q in (0, 7, 8, 8 * (V // 8) - 1, 8 * (V // 8), V - 1, 2047, 2048, 8191, 8192) if 0 <= q < V})
    g = _gen("ce spike", V)
    x = torch.randn(2 * len(pos), V, generator=g)
    lab = torch.empty(2 * len(pos), dtype=torch.int64)
    for i, q in enumerate(pos):
        for k in (0, 1):
            row = 2 * i + k
            x[row, q] = x[row].max() + 12.0
            lab[row] = q if k == 0 else (q - 1 if q > 0 else V - 1)
    x = x.to(dtype)
    for ignore in (0, -100):
        _ce_check(x, lab, ignore, False, f"ce spike V={V} ignore={ignore}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_ce_shift_invariance(dtype):
    """A constant +1e4 on one row (see the module docstring for the choice of V = 8200)."""
    V = 8200
    g = _gen("ce shift")
    x = torch.randn(5, V, generator=g)
    x[3] += 1e4
    x = x.to(dtype)
    for ignore in (0, -100):
        _ce_check(x, _labels(5, V, ignore, g), ignore, True, f"ce shift ignore={ignore}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [45, 264])
def test_ce_all_rows_ignored(V, dtype):
    x = torch.randn(5, V, generator=_gen("ce ign", V)).to(dtype)
    loss, grad = _ce_gpu(x, torch.zeros(5, dtype=torch.int64), 0)
    assert float(loss) == 0.0
    assert torch.isfinite(grad).all() and not grad.any()


@pytest.mark.parametrize("V", [45, 264, 10007])
def test_ce_gradient_planes(V):
    """fp32: the k-padded split planes written beside the gradient (ldp > V) are bit-equal to a split
    of the fp32 gradient, padding columns zero; the planes-only run (no fp32 store) writes the same
    planes and planes.f32 rebuilds the same fp32 values."""
    g = _gen("ce planes", V)
    x = torch.randn(5, V, generator=g)
    lab = _labels(5, V, 0, g)
    _, full = _ce_gpu(x, lab, 0)
    _close(full, _ce_ref(x, lab, 0)[1], 1e-6, 2e-5, f"ce planes V={V} grad")
    P = planes.cached(full, kpad=True)
    assert P is not None and P.shape[:2] == (3, 5) and P.shape[2] == planes.r32(V) and P.shape[2] > V
    assert not planes.planes_only(full)
    assert torch.equal(_bits(P), _bits(planes.split(full.detach().reshape(5, V), kpad=True)))
    assert not P[:, :, V:].any()
    _, only = _ce_gpu(x, lab, 0, mark=True)
    assert planes.planes_only(only)
    Po = planes.cached(only, kpad=True)
    assert Po is not None and torch.equal(_bits(Po), _bits(P))
    assert torch.equal(planes.f32(only), full)


# ---------------------------------------------------------------------------------------------
# 4. act_drop_bwd / act_drop_bwd_f32, called directly
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act,p", [(0, 0.1), (1, 0.0), (1, 0.1), (2, 0.0)], ids=["id_drop", "relu", "relu_drop", "sigmoid"])
@pytest.mark.parametrize("total", [1, 3, 7, 8, 9, 2047, 16389])
def test_act_drop_bwd(total, act, p, dtype):
    """dx = dy * dact(y) * mask * scale on a flat buffer with a ragged scalar tail.  The torch fp32
    expression the fp32 kernel must equal bit for bit (one multiply, or a multiply of a multiply:
    nothing a compiler could contract):
      identity: where(keep(i), dy * scale, 0)        relu: where(y > 0, dy * scale, 0)  (scale = 1 at p = 0)
      sigmoid:  dy * (y * (1 - y))
    bf16: within one bf16 ulp of the same expression in float64."""
    C = _native.C()
    seed, salt = 11, 77
    g = _gen("adb", total, act, p)
    dy = torch.randn(total, generator=g).to(dtype)
    keep = R.keep_mask((total,), p, seed, salt) if p > 0 else torch.ones(total, dtype=torch.bool)
    if act == 1:  # the saved output of relu + dropout
        y = (torch.relu(torch.randn(total, generator=g)) * keep * _scale32(p)).to(dtype)
    elif act == 2:
        y = torch.sigmoid(torch.randn(total, generator=g)).to(dtype)
    else:
        y = None
    s32 = torch.tensor(_scale32(p), dtype=F32)

    def expr(dy, y, s):
        if act == 1:
            return torch.where(y > 0, dy * s, torch.zeros_like(dy))
        if act == 2:
            return dy * (y * (1 - y))
        return torch.where(keep, dy * s, torch.zeros_like(dy))

    rng = R.DropoutRNG(seed).to(dev)
    dyg, yg = dy.to(dev), (y.to(dev) if y is not None else None)
    dx = torch.full_like(dyg, float("nan"))
    fn = C.act_drop_bwd_f32 if dtype == F32 else C.act_drop_bwd
    fn(dyg.data_ptr(), _native.ptr(yg), dx.data_ptr(), total, act, rng.ptr(), salt, R.threshold(p), R.scale(p),
       _native.stream())
    torch.cuda.synchronize()
    if dtype == F32:
        assert torch.equal(dx.cpu(), expr(dy, y, s32))
    else:
        ref = expr(dy.double(), y.double() if y is not None else None, s32.double())
        _within(dx, ref, _bf16_ulp(ref), f"act_drop_bwd act={act} p={p} total={total}")
        assert not dx.cpu()[ref == 0].any()


# ---------------------------------------------------------------------------------------------
# 5. Embedding forward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("shape,D,V,pe_rows", [((1, 1), 8, 3, 1), ((3, 5), 96, 17, 9), ((2, 7), 520, 11, 7), ((6,), 64, 5, 8)],
                         ids=["1x1x8", "3x5x96_long_table", "2x7x520", "1d_ids"])
def test_embedding_forward(shape, D, V, pe_rows, p, dtype):
    """out = dropout(w[ids] + pe[t % S]): one token, D = 8, a positional table longer than the
    sequence, 1-D ids, the first and the last vocabulary id.  fp32: bit-equal to torch fp32
    (w[ids] + pe[:S]) * mask * scale, and at D % 32 == 0 its split planes bit-equal to a split of
    it; bf16: within one bf16 ulp of float64 from the bf16-rounded table."""
    seed, salt = 5, 99
    g = _gen("emb", shape, D, V)
    T, S = math.prod(shape), shape[-1]
    ids = torch.randint(0, V, shape, generator=g)
    flat = ids.reshape(-1)
    flat[0] = V - 1
    flat[-1] = 0 if T > 1 else V - 1
    if T > 2:
        flat[1] = 0
    w = torch.randn(V, D, generator=g)
    pe = torch.randn(pe_rows, D, generator=g)
    keep = R.keep_mask((*shape, D), p, seed, salt) if p > 0 else torch.ones(*shape, D, dtype=torch.bool)
    s32 = torch.tensor(_scale32(p), dtype=F32)
    wg = torch.nn.Parameter(w.to(dev))
    with torch.no_grad():
        out = embedding(ids.to(dev), wg, pe.to(dev), p, R.DropoutRNG(seed).to(dev), salt, out_dtype=dtype)
    torch.cuda.synchronize()
    assert out.dtype == dtype and out.shape == (*shape, D)
    if dtype == F32:
        assert torch.equal(out.cpu(), (w[ids] + pe[:S]) * keep.float() * s32)
        P = planes.cached(out)
        if D % 32 == 0:
            assert P is not None and P.shape == (3, T, D)
            assert torch.equal(_bits(P), _bits(planes.split(out.reshape(T, D))))
        else:
            assert P is None
    else:
        ref = (w.bfloat16().double()[ids] + pe.double()[:S]) * keep.double() * s32.double()
        _within(out, ref, _bf16_ulp(ref), f"emb {shape} D={D}")
        assert not out.cpu()[ref == 0].any()
