"""The non-attention training kernels on a real MI355X (csrc/rmsnorm.hip,
swiglu.hip, cross_entropy.hip, optim.hip, fp8_quant.hip, sampling.hip), each
against an fp64 torch reference of the same operation computed from the same
bf16-rounded or fp32 inputs, at the shapes where they take another path:
past every grid cap (so each grid-stride loop runs twice), odd tails,
H % 8 != 0, saturating exponentials, ignored rows, a decay boundary inside
the buffer.

How the bounds are made (E = 2^-24 is the fp32 unit roundoff):

* a bf16 output is one rounding of an fp32 value: 2^-8 * |ref| (one ulp,
  which also covers the double rounding fp64 -> fp32 -> bf16);
* fp32 arithmetic adds an absolute term built from the fp64 reference's own
  intermediate magnitudes: E per rounding of a product or sum, and for an
  fp32 sum d * E * sum|terms|, where d is the most additions a term passes
  in the kernel's reduction (n for an n-term sum of unknown order);
* the fast __expf / __logf in swiglu and cross-entropy have no derivable
  bound. Their error is measured in a natural unit (given at each constant
  below), printed by the tests, and bounded at 4x the measured maximum.

Every test prints its largest error and the largest error/bound ratio before
it asserts."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

E = 2.0 ** -24        # fp32 unit roundoff
U_BF16 = 2.0 ** -8    # one bf16 ulp, relative
# Results below the fp32 normal range (2^-126), times operand magnitudes of at
# most 2^10 in these tests, may be flushed to zero by the fast exp; 2^-100 is
# 20 orders of magnitude under any value the tests look at.
TINY = 2.0 ** -100

DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from mlx_cuda_distributed_pretraining_amd.ops import require_ext

    return require_ext()


def _ulp(dtype):
    return U_BF16 if dtype is torch.bfloat16 else 0.0


def _f32(v):
    """v as the kernel sees it: the bindings cast hyperparameters to float"""
    return float(torch.tensor(v, dtype=torch.float32))


def _check(name, got, ref, bound):
    """got within bound of the fp64 ref, elementwise; prints the figures first"""
    got = got.detach().double()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{name} has non-finite values"
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{name}: max abs err {float(err.max()) if err.numel() else 0.0:.3e}, "
          f"max err/bound {ratio:.3f}")
    bad = err > bound
    assert not bool(bad.any()), (
        f"{name}: {int(bad.sum())} of {bad.numel()} elements over the bound, "
        f"worst err/bound {ratio:.3g}")


# =============================== rmsnorm ====================================
RMS_EPS = 1e-5
# name -> (rows, H)
RMS_CASES = {
    "one_vector_3x8": (3, 8),
    "llama_width_5x2048": (5, 2048),
    "bwd_blocks_loop_1027x256": (1027, 256),   # backward cap is 1024 blocks
    "bwd_blocks_loop_2051x64": (2051, 64),     # some blocks take three rows
    "four_vectors_per_thread_7x8192": (7, 8192),
    "ragged_5x100": (5, 100),                  # H % 8 != 0: scalar path, bf16 rows
    "ragged_4x12": (4, 12),                    # not 16-byte aligned
}


def _rms_inputs(rows, H, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, H, generator=g)
    res = 0.5 * torch.randn(rows, H, generator=g)
    x[0] = 0.0
    res[0] = 0.0          # a row of all zeros: rstd = eps^-1/2, y = 0
    x[1] *= 1e4           # a row of magnitude 1e4
    w = 1.0 + 0.5 * torch.randn(H, generator=g)
    dy = torch.randn(rows, H, generator=g)
    ds = torch.randn(rows, H, generator=g)
    return [t.to(dtype).to(dev()) for t in (x, res, w, dy, ds)]


def _rms_ref(s, w, dy, dadd, dtype):
    """fp64 RMSNorm forward and backward of the stored input s, with bounds.

    A row sum in these kernels gives each thread ceil(H/256) scalar terms or
    ceil(H/2048) vectors of 8 in turn, then a 6-level wave tree and 2 levels
    over the 4 waves: a term passes at most
        d = max(ceil(H/256), 8*ceil(H/2048)) + 8
    additions, so the sum errs by at most d*E*sum|terms|.
    rstd: d*E relative on the sum of squares, halved by the inverse square
    root, and squares / mean / +eps / rsqrtf (2 ulp) add 4E:
        rel(rstd) = rr = (d/2 + 4) * E.
    y = s*rstd*w: rr, two products and the final rounding: |y| * (rr + 3E),
    plus one bf16 ulp when y is bf16.
    dx = t1 - t2*c [+ dadd], t1 = rstd*dy*w, t2 = s*rstd^3/H, c = sum(dy*w*s):
    t1 carries rr + 3 products; c is a row sum of two-product terms,
    (d+2)*E*sum|dy*w*s|; rstd^3/H carries 3rr + 4 roundings; each of the two
    additions rounds once. All of it is absolute, so a dx that cancels to
    almost nothing is still bounded by its terms.
    dw = sum over rows of dy*s*rstd (fp32, before the wrapper's cast): rows
    terms in any order, rows*E*sum|terms|, each term carrying rr + 2 products.
    """
    u = _ulp(dtype)
    s, w, dy = s.double(), w.double(), dy.double()
    rows, H = s.shape
    rstd = ((s * s).sum(-1, keepdim=True) / H + _f32(RMS_EPS)).rsqrt()
    d = max(math.ceil(H / 256), 8 * math.ceil(H / 2048)) + 8
    rr = (d / 2 + 4) * E
    y = s * rstd * w
    t = dy * w * s
    c, cabs = t.sum(-1, keepdim=True), t.abs().sum(-1, keepdim=True)
    t1 = rstd * dy * w
    t2 = s * rstd ** 3 / H
    dx = t1 - t2 * c
    acc = (t1.abs() * (rr + 4 * E)
           + t2.abs() * ((d + 2) * E * cabs + c.abs() * (3 * rr + 6 * E))
           + E * (t1.abs() + (t2 * c).abs()))
    if dadd is not None:
        dx = dx + dadd.double()
        acc = acc + E * (dx.abs() + dadd.double().abs())
    terms = dy * s * rstd
    dw = terms.sum(0)
    b_dw = terms.abs().sum(0) * (rows * E + rr + 3 * E)
    return {
        "rstd": (rstd.squeeze(-1), rstd.squeeze(-1) * rr),
        "y": (y, y.abs() * (u + (1 + u) * (rr + 3 * E))),
        "dx": (dx, u * dx.abs() + (1 + u) * acc),
        "dw": (dw, b_dw),
        "dw_cast": (dw, u * dw.abs() + (1 + u) * b_dw),
    }


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(RMS_CASES))
def test_rms_norm_fwd_bwd_vs_fp64(ext, name, dt):
    """rms_norm forward and backward (bounds: _rms_ref). The backward reads
    the kernel's own saved rstd, whose error rr is part of every bound. With
    the measured ratios below 1 a wrong element (a dropped row of the
    backward's grid-stride loop, a misread weight) is off by O(|ref|), which
    is 2^8 bounds in bf16 and over 10^4 bounds in fp32."""
    from mlx_cuda_distributed_pretraining_amd.ops.rmsnorm import rms_norm

    rows, H = RMS_CASES[name]
    dtype = DTYPES[dt]
    x, _, w, dy, _ = _rms_inputs(rows, H, dtype, seed=rows * 10007 + H)
    xl, wl = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = rms_norm(xl, wl, RMS_EPS)
    y.backward(dy)
    _, rstd_k = ext.rmsnorm_fwd(x, w, RMS_EPS)
    dx_k, dw_k = ext.rmsnorm_bwd(x, w, rstd_k, dy)
    assert y.dtype == dtype and rstd_k.dtype == torch.float32 and dw_k.dtype == torch.float32
    ref = _rms_ref(x, w, dy, None, dtype)
    _check("y", y, *ref["y"])
    _check("rstd", rstd_k, *ref["rstd"])
    _check("dx", xl.grad, *ref["dx"])
    _check("dx (binding)", dx_k, *ref["dx"])
    _check("dw fp32", dw_k, *ref["dw"])
    _check("w.grad", wl.grad, *ref["dw_cast"])


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(RMS_CASES))
def test_add_rms_norm_fwd_bwd_vs_fp64(ext, name, dt):
    """add_rms_norm: s = x + res, y = rms_norm(s), with gradients arriving on
    both outputs (ds != 0, so the residual-stream gradient has to show up in
    dx: the fp32 kernel once dropped it).

    s is one fp32 addition, rounded once more when bf16: E*|s| in fp32,
    2^-8*|s| in bf16. The kernel normalises the s it stored, so the fp64
    reference of y, rstd and the backward starts from that stored s, which
    the first check has tied to x + res."""
    from mlx_cuda_distributed_pretraining_amd.ops.rmsnorm import add_rms_norm

    rows, H = RMS_CASES[name]
    dtype = DTYPES[dt]
    x, res, w, dy, ds = _rms_inputs(rows, H, dtype, seed=rows * 10007 + H + 1)
    xl, rl, wl = (t.clone().requires_grad_(True) for t in (x, res, w))
    s, y = add_rms_norm(xl, rl, wl, RMS_EPS)
    torch.autograd.backward([s, y], [ds, dy])
    s_ref = x.double() + res.double()
    _check("s", s, s_ref, s_ref.abs() * (_ulp(dtype) or E))
    ref = _rms_ref(s.detach(), w, dy, ds, dtype)
    _check("y", y, *ref["y"])
    _check("dx", xl.grad, *ref["dx"])
    _check("dres", rl.grad, *ref["dx"])
    _check("w.grad", wl.grad, *ref["dw_cast"])

    y_k, rstd_k, s_k = ext.rmsnorm_fwd_res(x, res, w, RMS_EPS, False)
    assert torch.equal(s_k, s.detach()) and torch.equal(y_k, y.detach())
    dx_k, dw_k = ext.rmsnorm_bwd_add(s_k, w, rstd_k, dy, ds)
    _check("rstd", rstd_k, *ref["rstd"])
    _check("dx (binding)", dx_k, *ref["dx"])
    _check("dw fp32", dw_k, *ref["dw"])


def test_rms_norm_casts_an_fp32_weight_to_a_bf16_input(ext):
    """A bf16 activation with an fp32 norm weight: the kernels read the weight
    through the activation's element type, so the op hands them the weight
    rounded to bf16 and returns the weight gradient in fp32. The reference is
    the fp64 norm with that rounded weight, at the bounds of _rms_ref; reading
    the fp32 weight's bytes as bf16 instead is off by O(1)."""
    from mlx_cuda_distributed_pretraining_amd.ops.rmsnorm import add_rms_norm, rms_norm

    rows, H = 5, 264
    x, res, _, dy, ds = _rms_inputs(rows, H, torch.bfloat16, seed=77)
    g = torch.Generator().manual_seed(78)
    w32 = (1.0 + 0.5 * torch.randn(H, generator=g)).to(dev())   # not bf16 values
    wb = w32.to(torch.bfloat16)
    assert not torch.equal(wb.float(), w32)

    xl, wl = x.clone().requires_grad_(True), w32.clone().requires_grad_(True)
    y = rms_norm(xl, wl, RMS_EPS)
    y.backward(dy)
    ref = _rms_ref(x, wb, dy, None, torch.bfloat16)
    assert y.dtype == torch.bfloat16 and wl.grad.dtype == torch.float32
    _check("y", y, *ref["y"])
    _check("dx", xl.grad, *ref["dx"])
    _check("w.grad fp32", wl.grad, *ref["dw"])

    xl, rl, wl = (t.clone().requires_grad_(True) for t in (x, res, w32))
    s, y = add_rms_norm(xl, rl, wl, RMS_EPS)
    torch.autograd.backward([s, y], [ds, dy])
    ref = _rms_ref(s.detach(), wb, dy, ds, torch.bfloat16)
    assert wl.grad.dtype == torch.float32
    _check("add: y", y, *ref["y"])
    _check("add: dx", xl.grad, *ref["dx"])
    _check("add: w.grad fp32", wl.grad, *ref["dw"])


# =============================== swiglu =====================================
# name -> (rows, I)
SWIGLU_CASES = {
    "one_vector_per_row_3x8": (3, 8),
    # 1031 * 4104 / 8 = 528 903 work items, over the 2048 x 256 = 524 288 cap
    "past_grid_cap_1031x4104": (1031, 4104),
}
# gate values at which __expf saturates to 0 or inf, and the way there
SWIGLU_SAT = [0.0, -0.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0]
# Measured: the fp32 kernels' largest error in units of E*(1+|g|)*M, where M
# is the cancellation-free magnitude of the output (below) and 1+|g| is the
# argument scaling of __expf(-g) = exp2(-g*log2(e)), whose product rounding is
# relative to |g|. Measured maxima on an MI355X: out 3.111, dgate 4.690,
# dup 3.460 units (all in the 1031 x 4104 case); each bound is 4x its figure.
# A real defect (gate and up swapped, sigmoid for silu, a work item skipped)
# is O(1) relative, 10^5 of these units.
SWIGLU_FAST_K = {"out": 4 * 3.111, "dgate": 4 * 4.690, "dup": 4 * 3.460}


def _swiglu_inputs(rows, I, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    gu = 1.5 * torch.randn(rows, 2 * I, generator=g)
    sat = torch.tensor(SWIGLU_SAT)
    gu[0, :8] = sat                    # first work item
    gu[-1, I - 8:I] = sat.flip(0)      # last work item (second grid-stride pass)
    dy = torch.randn(rows, I, generator=g)
    return gu.to(dtype).to(dev()), dy.to(dtype).to(dev())


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(SWIGLU_CASES))
def test_swiglu_fwd_bwd_vs_fp64(ext, name, dt):
    """out = g*sig(g)*u, dgate = dy*u*sig*(1 + g*(1-sig)), dup = dy*g*sig
    against fp64. The error of the fast exp is bounded by SWIGLU_FAST_K[name]
    (see there) times E*(1+|g|)*M with the cancellation-free magnitudes
        M(out) = |out|, M(dup) = |dup|, M(dgate) = |dy*u|*sig*(1+|g|*(1-sig))
    (dgate itself passes through zero near g = -1.28), plus one bf16 ulp for
    bf16 outputs and TINY for results the fast exp flushes. Gates at +-88 and
    +-100 overflow and underflow __expf; everything must stay finite."""
    from mlx_cuda_distributed_pretraining_amd.ops.swiglu import swiglu

    rows, I = SWIGLU_CASES[name]
    dtype = DTYPES[dt]
    u = _ulp(dtype)
    gu, dy = _swiglu_inputs(rows, I, dtype, seed=rows + I)
    leaf = gu.clone().requires_grad_(True)
    out = swiglu(leaf)
    out.backward(dy)
    assert out.shape == (rows, I) and out.dtype == dtype

    g, up, d = gu.double()[:, :I], gu.double()[:, I:], dy.double()
    sg = torch.sigmoid(g)
    unit = E * (1 + g.abs())
    refs = {
        "out": (g * sg * up, (g * sg * up).abs(), out),
        "dgate": (d * up * sg * (1 + g * (1 - sg)),
                  (d * up).abs() * sg * (1 + g.abs() * (1 - sg)), leaf.grad[:, :I]),
        "dup": (d * g * sg, (d * g * sg).abs(), leaf.grad[:, I:]),
    }
    for key, (ref, mag, got) in refs.items():
        if dtype is torch.float32:
            need = float(((got.double() - ref).abs() / (unit * mag + TINY)).max())
            print(f"{key}: fast-exp error {need:.3f} units (bound {SWIGLU_FAST_K[key]:.3f})")
        _check(key, got, ref, u * ref.abs() + (1 + u) * (SWIGLU_FAST_K[key] * unit * mag + TINY))


# ============================ cross-entropy =================================
IGN = -100
# name -> (N, V)
CE_CASES = {
    "one_vector_5x8": (5, 8),
    "row_blocks_loop_4099x264": (4099, 264),   # forward cap is 4096 row blocks
    # 4099 * 2056 / 8 = 1 053 443 work items: over the backward's 4096 x 256 cap
    "bwd_items_loop_4099x2056": (4099, 2056),
    "wide_vocab_37x50264": (37, 50264),
}
# Measured on an MI355X, each in the unit named where it is used, and each
# bounded at 4x its figure:
#   lse (_ce_ref, unit E*(1 + A + |m| + |lse|)): 1.368 units;
#   a vocab shard's sum-exp (unit E*sum(e^z*(1+|z|))): 3.690 units;
#   a probability written by the backward (_ce_grad_ref): 1.433 units.
# A real defect (a vocab vector skipped, the max not subtracted, a row dropped
# from the sum) moves lse by 1/V..1 and the loss by one row: thousands of
# units.
CE_LSE_K = 4 * 1.368
CE_SUMEXP_K = 4 * 3.690
CE_GRAD_K = 4 * 1.433


def _ce_inputs(N, V, dtype, mult, seed, all_ignored=False):
    g = torch.Generator().manual_seed(seed)
    logits = (mult * torch.randn(N, V, generator=g)).to(dtype).to(dev())
    tg = torch.randint(0, V, (N,), generator=g)
    tg[0], tg[1] = 0, V - 1        # first and last vocab entry
    tg[2::5] = IGN
    if all_ignored:
        tg[:] = IGN
    return logits, tg.to(dev())


def _ce_ref(logits, tg):
    """fp64 lse / loss of the logits as stored, with bounds.

    lse = m + log(sum e^z), z = l - m. __expf(z) errs relative to |z| (its
    argument scaling) and __logf adds to a value of size |lse - m|, then one
    rounding of the sum m + log: measured in units of
        E * (1 + A + |m| + |lse|),   A = softmax-weighted mean |z|,
    at most CE_LSE_K of them.
    loss_sum adds the counted rows' lse - l[t] (one rounding each,
    E*(|lse|+|l[t]|)) through thread 0 of each block (ceil(N/4096) rows in
    turn), then 16 partials per thread and a 14-level tree: any term passes
    depth = ceil(N/4096) + 16 + 14 additions, depth*E*sum|row loss|."""
    l = logits.double()
    N, V = l.shape
    m = l.max(-1).values
    z = l - m[:, None]
    ez = z.exp()
    se = ez.sum(-1)
    lse = m + se.log()
    A = (ez * z.abs()).sum(-1) / se
    lse_unit = E * (1 + A + m.abs() + lse.abs())
    b_lse = CE_LSE_K * lse_unit
    mask = tg != IGN
    lt = l.gather(-1, tg.clamp_min(0)[:, None]).squeeze(-1)
    row_loss = torch.where(mask, lse - lt, torch.zeros_like(lse))
    depth = math.ceil(N / 4096) + 16 + 14
    b_loss = ((b_lse + E * (lse.abs() + lt.abs())) * mask).sum() + depth * E * row_loss.abs().sum()
    return {"l": l, "lse": lse, "lse_unit": lse_unit, "b_lse": b_lse, "mask": mask,
            "loss_sum": row_loss.sum(), "b_loss": b_loss, "ntok": int(mask.sum())}


def _ce_grad_ref(r, tg, sc, dtype, sc_rel):
    """dlogits = (e^(l - lse) - onehot) * sc on counted rows, exactly 0 on
    ignored ones. The probability p = __expf(l - lse) takes the error of the
    kernel's own fp32 lse as a relative error, and __expf's own relative to
    1 + |l - lse|: its unit is p * (lse_unit + E*(1 + |l - lse|)), measured on
    the elements off the target (there dlogits = p * sc) and bounded at
    CE_GRAD_K units. The subtraction of the one-hot and the product with sc
    round once each, sc itself carries sc_rel, and a probability under 2^-126
    is flushed to 0 (TINY). Returns (ref, bound, unit, off-target mask)."""
    u = _ulp(dtype)
    zl = r["l"] - r["lse"][:, None]
    p = zl.exp()
    onehot = torch.zeros_like(p)
    rows = torch.nonzero(r["mask"]).squeeze(-1)
    onehot[rows, tg[rows]] = 1.0
    d = (p - onehot) * sc * r["mask"][:, None]
    unit = abs(sc) * p * (r["lse_unit"][:, None] + E * (1 + zl.abs()))
    acc = (CE_GRAD_K * unit + (2 * E + sc_rel) * d.abs() + TINY) * r["mask"][:, None]
    off_target = (onehot == 0) & r["mask"][:, None]
    return d, u * d.abs() + (1 + u) * acc, unit, off_target


def _check_ce_grad(name, got, r, tg, sc, dtype, sc_rel=0.0):
    d, bound, unit, off = _ce_grad_ref(r, tg, sc, dtype, sc_rel)
    if dtype is torch.float32 and bool(off.any()):
        need = float(((got.double() - d).abs()[off] / (unit[off] + TINY)).max())
        print(f"{name}: probability error {need:.3f} units (bound {CE_GRAD_K:.3f})")
    _check(name, got, d, bound)
    assert not bool(got[~r["mask"]].any()), f"{name}: ignored rows are not exactly 0"
    # each counted row of softmax - onehot sums to 0: within the sum of its bounds
    _check(name + " row sums", got.double().sum(-1), d.sum(-1), bound.sum(-1))


@pytest.mark.parametrize("mult", [1, 30])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(CE_CASES))
def test_ce_fwd_bwd_bindings_vs_fp64(ext, name, dt, mult):
    """ext.ce_fwd (lse, loss_sum, ntok) and ext.ce_bwd (dlogits) against fp64
    (bounds: _ce_ref, _ce_grad_ref). Logits x30 have row maxima near 120,
    where exp overflows fp32 unless the maximum is subtracted first."""
    N, V = CE_CASES[name]
    dtype = DTYPES[dt]
    logits, tg = _ce_inputs(N, V, dtype, mult, seed=N + V + mult)
    loss_sum, ntok, lse = ext.ce_fwd(logits, tg, IGN)
    r = _ce_ref(logits, tg)
    assert int(ntok) == r["ntok"] > 0
    need = float(((lse.double() - r["lse"]).abs() / r["lse_unit"]).max())
    print(f"lse: fast exp/log error {need:.3f} units (bound {CE_LSE_K:.3f})")
    _check("lse", lse, r["lse"], r["b_lse"])
    _check("loss_sum", loss_sum, r["loss_sum"], r["b_loss"])

    sc = torch.tensor(0.37 / r["ntok"], dtype=torch.float32, device=dev())
    dl = ext.ce_bwd(logits, tg, lse, sc, IGN)
    assert dl.dtype == dtype
    _check_ce_grad("dlogits", dl, r, tg, float(sc), dtype)


@pytest.mark.parametrize("mult", [1, 30])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(CE_CASES))
def test_fused_cross_entropy_vs_fp64(ext, name, dt, mult):
    """fused_cross_entropy's mean loss and, through (loss * 0.25).backward(),
    its dlogits with an upstream gradient other than 1. The mean divides
    loss_sum by ntok (one rounding, E*|loss|); the backward's scale 0.25/ntok
    is one fp32 division (sc_rel = E)."""
    from mlx_cuda_distributed_pretraining_amd.ops.cross_entropy import fused_cross_entropy

    N, V = CE_CASES[name]
    dtype = DTYPES[dt]
    logits, tg = _ce_inputs(N, V, dtype, mult, seed=N + V + mult + 1)
    leaf = logits.clone().requires_grad_(True)
    loss, ntok = fused_cross_entropy(leaf, tg, IGN)
    (loss * 0.25).backward()
    r = _ce_ref(logits, tg)
    assert int(ntok) == r["ntok"] > 0
    mean = r["loss_sum"] / r["ntok"]
    _check("loss", loss, mean, r["b_loss"] / r["ntok"] + E * mean.abs())
    _check_ce_grad("dlogits", leaf.grad, r, tg, 0.25 / r["ntok"], dtype, sc_rel=E)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_cross_entropy_all_targets_ignored(ext, dt):
    """No counted row: loss_sum 0, ntok 0, a mean loss of 0 (not 0/0), dlogits
    exactly 0 everywhere, nothing NaN."""
    from mlx_cuda_distributed_pretraining_amd.ops.cross_entropy import fused_cross_entropy

    dtype = DTYPES[dt]
    logits, tg = _ce_inputs(37, 264, dtype, 1, seed=5, all_ignored=True)
    loss_sum, ntok, lse = ext.ce_fwd(logits, tg, IGN)
    assert float(loss_sum) == 0.0 and int(ntok) == 0
    assert bool(torch.isfinite(lse).all())
    leaf = logits.clone().requires_grad_(True)
    loss, ntok = fused_cross_entropy(leaf, tg, IGN)
    (loss * 0.25).backward()
    assert float(loss) == 0.0 and int(ntok) == 0
    assert not bool(leaf.grad.any()), "dlogits of ignored rows are not exactly 0"


def test_ce_vocab_parallel_shards_vs_fp64(ext):
    """ce_vp_stats and ce_vp_sumexp at N = 2051 rows (their cap is 2048 row
    blocks, so three blocks take a second row), two vocab shards combined by
    hand (the second with v0 = 136 != 0) against the fp64 full-vocab
    reference. A row maximum and a picked target logit are exact. A shard's
    sum-exp is measured in units of E * sum(e^z * (1 + |z|)), z = l - m_group
    (CE_SUMEXP_K of them at most); lse = m + log(se0 + se1) and the loss are
    then taken in fp64 from the kernels' outputs, so their bounds are the
    sum-exp bounds carried through the log: (b_se0 + b_se1) / se."""
    N, V, half = 2051, 272, 136
    logits, tg = _ce_inputs(N, V, torch.bfloat16, 3, seed=11)
    r = _ce_ref(logits, tg)
    shards = [logits[:, :half].contiguous(), logits[:, half:].contiguous()]
    ms, picked = [], []
    for v0, sh in zip((0, half), shards):
        m_k, t_k = ext.ce_vp_stats(sh, tg, v0, IGN)
        assert torch.equal(m_k.double(), sh.double().max(-1).values), f"shard max, v0={v0}"
        local = tg - v0
        inside = (tg != IGN) & (local >= 0) & (local < half)
        want = torch.where(inside, sh.double().gather(-1, local.clamp(0, half - 1)[:, None])
                           .squeeze(-1), torch.zeros(N, dtype=torch.float64, device=dev()))
        assert torch.equal(t_k.double(), want), f"picked target logit, v0={v0}"
        ms.append(m_k)
        picked.append(t_k.double())
    m = torch.maximum(ms[0], ms[1])
    se, b_se = 0.0, 0.0
    for v0, sh in zip((0, half), shards):
        se_k = ext.ce_vp_sumexp(sh, m)
        z = sh.double() - m.double()[:, None]
        unit = E * (z.exp() * (1 + z.abs())).sum(-1)
        need = float(((se_k.double() - z.exp().sum(-1)).abs() / unit).max())
        print(f"sum-exp v0={v0}: fast-exp error {need:.3f} units (bound {CE_SUMEXP_K:.3f})")
        _check(f"sum-exp v0={v0}", se_k, z.exp().sum(-1), CE_SUMEXP_K * unit)
        se = se + se_k.double()
        b_se = b_se + CE_SUMEXP_K * unit
    lse = m.double() + se.log()
    b_lse = b_se / (r["lse"] - m.double()).exp()
    _check("lse from shards", lse, r["lse"], b_lse)
    loss = torch.where(r["mask"], lse - (picked[0] + picked[1]), torch.zeros_like(lse)).sum()
    _check("loss from shards", loss, r["loss_sum"], (b_lse * r["mask"]).sum())


# ============================== optimizers ==================================
OPT_N = 2 * 1048576 + 1003      # over the 4096 x 256 cap, odd tail
OPT_BOUNDARIES = {"none": 0, "inside": OPT_N // 3, "all": OPT_N}   # N//3 % 256 != 0
OPT_CLIP = 100.0                # the gradient norms are near sqrt(N) = 1448
OPT_HP = {
    "adamw": dict(lr=1e-2, b1=0.9, b2=0.95, eps=1e-8, wd=0.1),
    "lion": dict(lr=1e-3, b1=0.9, b2=0.99, wd=0.1),
    "sgd": dict(lr=1e-2, mom=0.9, wd=0.1),
}
# relative error of the clip coefficient min(1, max/(sqrt(sumsq)+1e-6)): a term
# of grad_sumsq passes at most 8 sequential adds, an 8-level block tree, 5
# sequential partials and an 8-level tree, plus its own square: 30E <= 32E on
# sumsq, half of that through the square root, 4E for sqrt, +1e-6, the division
# and the product with the gradient.
OPT_SUMSQ_REL = 32 * E
OPT_CLIP_REL = OPT_SUMSQ_REL / 2 + 4 * E


def _opt_cases():
    cases = []
    for kind in ("adamw", "lion", "sgd", "sgd_nesterov"):
        for b in OPT_BOUNDARIES:
            for clip in (False, True):
                cases.append((kind, "bf16", "bf16", b, clip))
        for p, g in (("bf16", "fp32"), ("fp32", "bf16"), ("fp32", "fp32")):
            cases.append((kind, p, g, "inside", True))
    return cases


@pytest.fixture(scope="module")
def opt_data():
    """One set of inputs for every optimizer case: fp32 master, non-zero
    moments, three gradients; every 997th element has zero gradient and zero
    first moment (an embedding row no batch has touched)."""
    g = torch.Generator().manual_seed(1234)
    master = torch.randn(OPT_N, generator=g)
    m = 0.1 * torch.randn(OPT_N, generator=g)
    v = (0.1 * torch.randn(OPT_N, generator=g)) ** 2
    grads = [torch.randn(OPT_N, generator=g) for _ in range(3)]
    idle = torch.arange(5, OPT_N, 997)
    m[idle] = 0.0
    for gr in grads:
        gr[idle] = 0.0
    return {"master": master.to(dev()), "m": m.to(dev()), "v": v.to(dev()),
            "grads": [gr.to(dev()) for gr in grads], "idle": idle.to(dev())}


def _opt_ref(kind, hp, p, m, v, g, step, boundary, max_norm):
    """One fp64 step of csrc/optim.hip's formulas from fp32 state, with the
    bound of one fp32 evaluation. Hyperparameters are the floats the kernel
    receives; 1 - b is exact in fp32 for b in [0.5, 1]. A product or a sum
    rounds once (E of its size); the clipped gradient carries rg.
    Returns {name: (ref, bound)} and, for Lion, the undecidable-sign mask."""
    hp = {k: _f32(x) for k, x in hp.items()}
    lr, wd = hp["lr"], hp["wd"]
    cc, rg = 1.0, 0.0
    if max_norm > 0:
        cc = min(1.0, max_norm / (float(g.pow(2).sum().sqrt()) + 1e-6))
        rg = OPT_CLIP_REL
    g = g * cc
    decays = (torch.arange(p.numel(), device=p.device) < boundary) & (wd > 0)
    decay = torch.where(decays, torch.full_like(p, 1 - lr * wd), torch.ones_like(p))
    out, skip = {}, None
    if kind == "adamw":
        b1, b2, eps = hp["b1"], hp["b2"], hp["eps"]
        a1, a2 = b1 * m, (1 - b1) * g
        m2, b_m = a1 + a2, 3 * E * (a1.abs() + a2.abs()) + rg * a2.abs()
        c1, c2 = b2 * v, (1 - b2) * g * g
        v2, b_v = c1 + c2, 3 * E * (c1 + c2) + (2 * rg + 2 * E) * c2
        # bias corrections 1 - powf(b, step): powf within 2 ulp of b^step
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        r1, r2 = 2 * E * b1 ** step / bc1, 2 * E * b2 ** step / bc2
        root = (v2 / bc2).sqrt()
        denom = root + eps
        b_denom = root * (0.5 * (b_v / v2.clamp_min(1e-300) + r2) + 2 * E) + E * denom
        upd = lr * (m2 / bc1) / denom
        b_upd = lr / (bc1 * denom) * b_m + upd.abs() * (r1 + b_denom / denom + 4 * E)
        p2 = p * decay - upd
        out = {"master": (p2, 4 * E * p.abs() + E * p2.abs() + b_upd),
               "m": (m2, b_m), "v": (v2, b_v)}
    elif kind == "lion":
        b1, b2 = hp["b1"], hp["b2"]
        a1, a2 = b1 * m, (1 - b1) * g
        c = a1 + a2
        skip = c.abs() < 2.0 ** -20 * (a1.abs() + a2.abs())
        d1, d2 = b2 * m, (1 - b2) * g
        p2 = p * decay - lr * torch.sign(c)
        out = {"master": (p2, 4 * E * p.abs() + E * p2.abs() + E * lr),
               "m": (d1 + d2, 3 * E * (d1.abs() + d2.abs()) + rg * d2.abs())}
    else:
        mom = hp["mom"]
        gd = g + torch.where(decays, wd * p, torch.zeros_like(p))
        b_gd = (rg + E) * g.abs() + 2 * E * (wd * p).abs() + E * gd.abs()
        buf = mom * m + gd
        b_buf = b_gd + 2 * E * ((mom * m).abs() + gd.abs())
        if kind == "sgd_nesterov":
            upd = gd + mom * buf
            b_upd = b_gd + mom * b_buf + 2 * E * (gd.abs() + (mom * buf).abs())
        else:
            upd, b_upd = buf, b_buf
        p2 = p - lr * upd
        out = {"master": (p2, lr * b_upd + 2 * E * (p.abs() + (lr * upd).abs())),
               "m": (buf, b_buf)}
    return out, skip


@pytest.mark.parametrize("kind,pdt,gdt,boundary,clip", _opt_cases())
def test_optimizer_steps_vs_fp64(ext, opt_data, kind, pdt, gdt, boundary, clip):
    """Three consecutive AdamW / Lion / SGD steps (step counts 2, 3, 4) from
    non-zero moments over N = 2 097 152 + 1003 elements, with the decay
    boundary at 0, inside the buffer (N//3) or at N, with and without the
    folded global-norm clip, for the four (param, grad) dtype pairs.

    Each step is compared with one fp64 step (_opt_ref) taken from the fp32
    state the kernel held before it: that state is exact in fp64, so every
    step is held to the bound of a single fp32 evaluation, and since the
    state after each step is checked, so is the three-step run. Weight decay
    alone moves an element by lr*wd*|p| ~ 1e-3 relative and a wrong clip
    coefficient by a factor 14, against bounds of a few E = 6e-8.

    Lion: an element with zero gradient and zero momentum has sign 0 and must
    not move beyond its weight decay. Elements whose interpolated value is
    under 2^-20 of its two terms have no decidable sign in fp32 and are left
    out of the master comparison; they must be under 0.1 % of the buffer.
    param must be master rounded to param's dtype, bit for bit."""
    from mlx_cuda_distributed_pretraining_amd.ops import fused_optim

    hp = OPT_HP[kind.split("_")[0]]
    bnd = OPT_BOUNDARIES[boundary]
    max_norm = OPT_CLIP if clip else 0.0
    master = opt_data["master"].clone()
    param = master.to(DTYPES[pdt])
    m = opt_data["m"].clone()
    v = opt_data["v"].clone()
    idle = opt_data["idle"]
    for k in range(3):
        step = k + 2
        grad = opt_data["grads"][k].to(DTYPES[gdt])
        prev = (master.double(), m.double(), v.double())
        ss = None
        if clip:
            ss = fused_optim.grad_sumsq(grad)
            want = grad.double().pow(2).sum()
            assert abs(float(ss) - float(want)) <= OPT_SUMSQ_REL * float(want)
        if kind == "adamw":
            fused_optim.adamw_step(param, master, grad, m, v, step, hp["lr"], hp["b1"], hp["b2"],
                                   hp["eps"], hp["wd"], bnd, sumsq=ss, max_grad_norm=max_norm)
        elif kind == "lion":
            fused_optim.lion_step(param, master, grad, m, step, hp["lr"], hp["b1"], hp["b2"],
                                  hp["wd"], bnd, sumsq=ss, max_grad_norm=max_norm)
        else:
            fused_optim.sgd_step(param, master, grad, m, step, hp["lr"], hp["mom"], hp["wd"], bnd,
                                 nesterov=(kind == "sgd_nesterov"), sumsq=ss,
                                 max_grad_norm=max_norm)
        ref, skip = _opt_ref(kind, hp, *prev, grad.double(), step, bnd, max_norm)
        tag = f"step {step} "
        if skip is None:
            _check(tag + "master", master, *ref["master"])
        else:
            frac = float(skip.double().mean())
            print(f"{tag}undecidable Lion signs: {frac:.2e} of the buffer")
            assert frac < 1e-3
            keep = ~skip
            _check(tag + "master", master[keep], ref["master"][0][keep], ref["master"][1][keep])
            still = idle[idle >= bnd]      # idle and outside the decayed range
            assert torch.equal(master[still].double(), prev[0][still]), \
                "an element with zero gradient and zero momentum moved"
        _check(tag + "m", m, *ref["m"])
        if kind == "adamw":
            _check(tag + "v", v, *ref["v"])
        assert torch.equal(param, master.to(param.dtype)), "param is not master rounded"


def test_lion_zero_gradient_and_momentum_do_not_move(ext):
    """sign(0) = 0: with no gradient, no momentum and no weight decay a Lion
    step leaves master and param bit-identical (an unused embedding row once
    drifted by -lr every step)."""
    from mlx_cuda_distributed_pretraining_amd.ops import fused_optim

    n = 1003
    g = torch.Generator().manual_seed(3)
    master = torch.randn(n, generator=g).to(dev())
    param = master.bfloat16()
    before_master, before_param = master.clone(), param.clone()
    grad = torch.zeros(n, dtype=torch.bfloat16, device=dev())
    m = torch.zeros(n, device=dev())
    for step in (1, 2, 3):
        fused_optim.lion_step(param, master, grad, m, step, 1e-3, 0.9, 0.99, 0.0, n)
    assert torch.equal(master, before_master) and torch.equal(param, before_param)
    assert not bool(m.any())


# ============================= fp8 quantize =================================
def _fp8_scale_ref(amax):
    """max(amax/448, 1e-12) in fp32, as the kernels compute it"""
    return (amax.float().cpu() / 448.0).clamp_min(1e-12)


def _fp8_codes_ref(x, scale):
    """the CPU's e4m3fn rounding of x * (1/scale), 1/scale taken in fp32;
    returned dequantized so that +0 and -0 compare equal"""
    inv = torch.ones((), dtype=torch.float32) / scale.float().cpu()
    return (x.float().cpu() * inv).to(torch.float8_e4m3fn).float()


def _check_fp8(name, codes, scale, x, amax=None):
    amax = x.abs().max() if amax is None else amax
    assert codes.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32
    assert torch.equal(scale.cpu().reshape(()), _fp8_scale_ref(amax).reshape(())), \
        f"{name}: scale {float(scale)!r} vs {float(_fp8_scale_ref(amax))!r}"
    got = codes.float().cpu()
    assert not bool(got.isnan().any()), f"{name}: NaN codes"
    want = _fp8_codes_ref(x, scale)
    assert got.shape == want.shape
    diff = got != want
    print(f"{name}: {int(diff.sum())} of {diff.numel()} codes differ")
    assert torch.equal(got, want), f"{name}: {int(diff.sum())} codes differ from the reference"


def _fp8_span():
    """every bf16 significand at every exponent 2^-20 .. 2^4, both signs: after
    scaling by 448/amax the small ones land on e4m3 subnormals and on exact
    ties between two codes (round to nearest even)"""
    sig = 1.0 + torch.arange(128, dtype=torch.float32) / 128.0
    mag = (2.0 ** torch.arange(-20, 5, dtype=torch.float32))[:, None] * sig[None, :]
    return torch.cat([mag, -mag], 0)          # [50, 128]


FP8_CASES = {
    "one_vector_3x8": lambda g: torch.randn(3, 8, generator=g),
    "all_tail_1x13": lambda g: torch.randn(1, 13, generator=g),
    # n = 4 210 703 > 2048*256*8 and n % 8 = 7: both cast loops run twice
    "both_loops_2053x2051": lambda g: torch.randn(2053, 2051, generator=g),
    "all_zero_5x24": lambda g: torch.zeros(5, 24),
    "span_2e-20_to_2e4": lambda g: _fp8_span(),
}


@pytest.mark.parametrize("name", list(FP8_CASES))
def test_fp8_quantize_codes_and_scale_bit_exact(ext, name):
    """ext.fp8_quantize: scale == max(amax/448, 1e-12) in fp32 and every code
    equal to the CPU's round-to-nearest-even e4m3fn conversion of
    x * (1/scale). Both are exact operations, so the check is equality."""
    x = FP8_CASES[name](torch.Generator().manual_seed(21)).to(torch.bfloat16).to(dev())
    codes, scale = ext.fp8_quantize(x, False)
    assert codes.shape == x.shape
    _check_fp8(name, codes, scale, x)


@pytest.mark.parametrize("N,K", [(33, 65), (32, 32), (100, 7)])
def test_fp8_quantize_transposed_bit_exact(ext, N, K):
    """The transposed cast on ragged 32x32 tiles: codes [K, N] equal to the
    reference codes of x.t()."""
    x = torch.randn(N, K, generator=torch.Generator().manual_seed(N * K))
    x = x.to(torch.bfloat16).to(dev())
    codes, scale = ext.fp8_quantize(x, True)
    assert codes.shape == (K, N)
    _check_fp8(f"transposed {N}x{K}", codes, scale, x.t().contiguous())


def _fp8_producers():
    from mlx_cuda_distributed_pretraining_amd.ops.rmsnorm import add_rms_norm, rms_norm
    from mlx_cuda_distributed_pretraining_amd.ops.swiglu import swiglu

    def rms(g):
        x, _, w, _, _ = _rms_inputs(37, 520, torch.bfloat16, seed=31)
        return rms_norm(x, w, RMS_EPS, emit_amax=True)

    def add_rms(g):
        x, res, w, _, _ = _rms_inputs(37, 520, torch.bfloat16, seed=32)
        return add_rms_norm(x, res, w, RMS_EPS, emit_amax=True)[1]

    def swi(g):
        gu, _ = _swiglu_inputs(1031, 4104, torch.bfloat16, seed=33)   # 2048 partials, looping
        return swiglu(gu, emit_amax=True)

    return {"rms_norm": rms, "add_rms_norm": add_rms, "swiglu": swi}


@pytest.mark.parametrize("producer", ["rms_norm", "add_rms_norm", "swiglu"])
def test_fp8_quantize_pre_with_producer_amax(ext, producer):
    """emit_amax=True: the producer leaves per-block partial maxima of its
    fp32 results, and fp8_quantize_pre skips its own amax pass. The scale is
    max(partials)/448; the bf16 output is those fp32 results rounded, so
    max|y| <= max(partials) * (1 + 2^-8), which keeps y/scale under the 464
    where e4m3 turns to NaN; codes are bit-equal to the reference at that
    scale."""
    y = _fp8_producers()[producer](None)
    partials = y._mcdp_amax
    assert partials.dtype == torch.float32 and partials.numel() > 0
    codes, scale = ext.fp8_quantize_pre(y, partials, False)
    pmax = partials.max()
    assert float(y.abs().max()) <= float(pmax) * (1 + U_BF16)
    assert float(y.abs().max()) >= float(pmax) * (1 - U_BF16), "partials overstate max|y|"
    _check_fp8(producer, codes, scale, y, amax=pmax)


# =============================== sampling ===================================
N_DRAWS = 8192
# scipy.stats.chi2.isf(1e-6, df) for df = 3 .. 15
CHI2_ISF_1E6 = {3: 30.66, 4: 33.38, 5: 35.89, 6: 38.26, 7: 40.52, 8: 42.70, 9: 44.81,
                10: 46.86, 11: 48.87, 12: 50.83, 13: 52.75, 14: 54.64, 15: 56.49}


def _sampling_logits(kind):
    if kind == "v8":
        return torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, -0.5, 0.3, 1.2])
    if kind == "v8_minp":   # (l - max) of tokens 0, 1, 5, 6 is under log(0.1) = -2.30
        return torch.tensor([0.0, 0.5, 1.0, 3.0, 2.0, -0.5, 0.3, 1.2])
    # V = 300 > 256 threads: 12 live tokens spread over the waves, the second
    # pass of the thread loop (256, 257, 270, 299) and wave edges; the rest 12
    # nats below the lowest of them
    logits = torch.full((300,), -12.0)
    live = torch.tensor([0, 63, 64, 100, 130, 191, 192, 255, 256, 257, 270, 299])
    logits[live] = torch.linspace(0.0, 2.2, 12)
    return logits


# (logits, temperature, min_p)
SAMPLING_CASES = {
    "v8_t1.0": ("v8", 1.0, 0.0),
    "v8_t0.7": ("v8", 0.7, 0.0),
    "v300_t1.0": ("v300", 1.0, 0.0),
    "v300_t0.7": ("v300", 0.7, 0.0),
    "v8_min_p0.1": ("v8_minp", 1.0, 0.1),
}


def _chi2(counts, p):
    """Pearson chi^2 of counts against N*p; cells with an expected count under
    5 are pooled (with the next smallest cells, until the pool reaches 5)"""
    expected = (N_DRAWS * p).tolist()
    cells = sorted(zip(expected, counts.tolist()))
    pool_e = pool_c = 0.0
    while cells and (cells[0][0] < 5.0 or 0.0 < pool_e < 5.0):
        e, c = cells.pop(0)
        pool_e, pool_c = pool_e + e, pool_c + c
    if pool_e > 0.0:
        cells.append((pool_e, pool_c))
    chi2 = sum((c - e) ** 2 / e for e, c in cells)
    return chi2, len(cells) - 1


def _check_distribution(name, draws, logits, temperature, min_p):
    """draws against softmax(logits / T) (renormalised over the tokens min-p
    keeps). The bound is the chi^2 upper quantile at p = 1e-6 for the case's
    degrees of freedom; the kernel's RNG is a fixed function of the seed, so
    this is a fixed pass/fail. A sampler that ignored the temperature, or lost
    one live token, gives chi^2 in the hundreds at 8192 draws."""
    V = logits.numel()
    draws = draws.cpu()
    assert int(draws.min()) >= 0 and int(draws.max()) < V
    z = logits.double().cpu() / temperature
    p = torch.softmax(z, -1)
    if min_p > 0:
        keep = p >= min_p * p.max()
        counts = torch.bincount(draws, minlength=V)
        assert int(counts[~keep].sum()) == 0, f"{name}: drew a token under min_p * p_max"
        p = torch.where(keep, p, torch.zeros_like(p))
        p = p / p.sum()
        counts, p = counts[keep], p[keep]
    else:
        counts = torch.bincount(draws, minlength=V)
    chi2, df = _chi2(counts, p)
    print(f"{name}: chi^2 = {chi2:.2f} at df = {df} (bound {CHI2_ISF_1E6[df]})")
    assert chi2 < CHI2_ISF_1E6[df], f"{name}: chi^2 {chi2:.2f} at df {df}"


@pytest.mark.parametrize("name", list(SAMPLING_CASES))
def test_sample_token_distribution(ext, name):
    """ext.sample_token: 8192 draws with seeds 0 .. 8191 follow the softmax."""
    kind, temperature, min_p = SAMPLING_CASES[name]
    logits = _sampling_logits(kind).to(dev())
    draws = torch.stack([ext.sample_token(logits, temperature, 1.0, min_p, seed)
                         for seed in range(N_DRAWS)])
    _check_distribution(name, draws, logits, temperature, min_p)


@pytest.mark.parametrize("name", list(SAMPLING_CASES))
def test_sample_token_dev_distribution(ext, name):
    """ext.sample_token_dev: 8192 identical bf16 rows in one launch follow the
    softmax of the bf16-rounded logits, and the device position salts the
    draw: pos and pos + 1 give different tokens."""
    kind, temperature, min_p = SAMPLING_CASES[name]
    row = _sampling_logits(kind).to(torch.bfloat16).to(dev())
    logits = row[None, :].expand(N_DRAWS, -1).contiguous()
    out = [torch.empty(N_DRAWS, dtype=torch.int64, device=dev()) for _ in range(2)]
    for i, o in enumerate(out):
        pos = torch.tensor([17 + i], dtype=torch.int32, device=dev())
        ext.sample_token_dev(logits, o, temperature, min_p, 7, pos)
    assert not torch.equal(out[0], out[1]), "pos and pos + 1 drew the same tokens"
    _check_distribution(name + " pos 17", out[0], row, temperature, min_p)
    _check_distribution(name + " pos 18", out[1], row, temperature, min_p)


# ========================= host-check rejections ============================
def _all_rejected(calls):
    for i, call in enumerate(calls):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"bad call {i} was accepted")


def test_host_checks_reject_bad_rmsnorm_args(ext):
    """The rmsnorm bindings read w, res, dy and dadd through x's element type
    and index rstd by row: all of it is checked before any launch. Each bad
    tensor is at least as many bytes as the right one."""
    rows, H = 4, 64
    x, res, w, dy, ds = _rms_inputs(rows, H, torch.bfloat16, seed=1)
    y, rstd = ext.rmsnorm_fwd(x, w, RMS_EPS)
    good = ext.rmsnorm_bwd_add(x, w, rstd, dy, ds)
    _all_rejected([
        lambda: ext.rmsnorm_fwd(x, w.float(), RMS_EPS),                      # w fp32
        lambda: ext.rmsnorm_fwd(x, torch.cat([w, w]), RMS_EPS),              # w 2H long
        lambda: ext.rmsnorm_fwd(x, w.cpu(), RMS_EPS),                        # w on the host
        lambda: ext.rmsnorm_fwd_res(x, res.float(), w, RMS_EPS, False),      # res fp32
        lambda: ext.rmsnorm_bwd(x, w.float(), rstd, dy),                     # w fp32
        lambda: ext.rmsnorm_bwd(x, w, rstd.double(), dy),                    # rstd fp64
        lambda: ext.rmsnorm_bwd(x, w, torch.cat([rstd, rstd]), dy),          # rstd 2*rows
        lambda: ext.rmsnorm_bwd(x, w, rstd, dy.float()),                     # dy fp32
        lambda: ext.rmsnorm_bwd_add(x, w, rstd, dy, ds.float()),             # dadd fp32
        lambda: ext.rmsnorm_bwd_add(x, w, rstd, dy, torch.cat([ds, ds])),    # dadd 2*rows
    ])
    again = ext.rmsnorm_bwd_add(x, w, rstd, dy, ds)
    assert torch.equal(good[0], again[0]) and torch.equal(good[1], again[1])


def test_host_checks_reject_bad_swiglu_args(ext):
    """swiglu_bwd reads dy through gu's element type as [..., I] rows, and
    needs the forward's 2I % 16 == 0."""
    rows, I = 4, 16
    gu, dy = _swiglu_inputs(rows, I, torch.bfloat16, seed=2)
    good = ext.swiglu_bwd(gu, dy)
    gu24 = torch.zeros(rows, 24, dtype=torch.bfloat16, device=dev())
    _all_rejected([
        lambda: ext.swiglu_bwd(gu, dy.float()),                              # dy fp32
        lambda: ext.swiglu_bwd(gu, torch.cat([dy, dy], -1)),                 # dy [rows, 2I]
        lambda: ext.swiglu_bwd(gu, torch.cat([dy, dy], 0)),                  # dy [2*rows, I]
        lambda: ext.swiglu_bwd(gu, dy.cpu()),                                # dy on the host
        lambda: ext.swiglu_bwd(gu24, torch.zeros(rows, 12, dtype=torch.bfloat16,
                                                 device=dev())),             # 2I % 16 != 0
    ])
    assert torch.equal(good, ext.swiglu_bwd(gu, dy))


def test_host_checks_reject_bad_cross_entropy_args(ext):
    """The CE bindings index targets and lse by row and read bf16 rows as
    16-byte vectors."""
    N, V = 16, 64
    logits, tg = _ce_inputs(N, V, torch.bfloat16, 1, seed=3)
    loss_sum, ntok, lse = ext.ce_fwd(logits, tg, IGN)
    sc = torch.tensor(0.1, device=dev())
    good = ext.ce_bwd(logits, tg, lse, sc, IGN)
    m, _ = ext.ce_vp_stats(logits, tg, 0, IGN)
    l12 = torch.zeros(N, 12, dtype=torch.bfloat16, device=dev())
    tg2 = torch.cat([tg, tg])
    _all_rejected([
        lambda: ext.ce_fwd(l12, tg, IGN),                                    # bf16, V % 8 != 0
        lambda: ext.ce_fwd(logits, tg.int(), IGN),                           # targets int32
        lambda: ext.ce_fwd(logits, tg.cpu(), IGN),                           # targets on the host
        lambda: ext.ce_fwd(logits, tg2, IGN),                                # 2N targets
        lambda: ext.ce_bwd(logits, tg.cpu(), lse, sc, IGN),
        lambda: ext.ce_bwd(logits, tg2, lse, sc, IGN),
        lambda: ext.ce_bwd(logits, tg, lse.double(), sc, IGN),               # lse fp64
        lambda: ext.ce_bwd(logits, tg, torch.cat([lse, lse]), sc, IGN),      # lse 2N long
        lambda: ext.ce_vp_stats(logits, tg.cpu(), 0, IGN),
        lambda: ext.ce_vp_stats(logits, tg2, 0, IGN),
        lambda: ext.ce_vp_sumexp(logits, m.double()),                        # max fp64
        lambda: ext.ce_vp_sumexp(logits, torch.cat([m, m])),
        lambda: ext.ce_vp_sumexp(l12, m),                                    # V % 8 != 0
        lambda: ext.ce_vp_bwd(logits, tg, lse.double(), sc.reshape(1), 0, IGN),
        lambda: ext.ce_vp_bwd(logits, tg2, lse, sc.reshape(1), 0, IGN),
        lambda: ext.ce_vp_bwd(logits, tg, lse, sc.double().reshape(1), 0, IGN),   # scale fp64
    ])
    assert torch.equal(good, ext.ce_bwd(logits, tg, lse, sc, IGN))


def test_host_checks_reject_bad_optimizer_args(ext):
    """adamw_step, lion_step and sgd_step share one check: every buffer is
    indexed by param's flat index and the state is read as float."""
    n = 1003
    g = torch.Generator().manual_seed(4)
    mk = lambda: torch.randn(n, generator=g).to(dev())   # noqa: E731
    master, m, v, grad = mk(), mk(), mk().abs(), mk().bfloat16()
    param = master.bfloat16()
    ss = torch.zeros((), device=dev())
    big = torch.zeros(2 * n, device=dev())
    strided = big[::2]                                    # n elements, not contiguous

    def steps(param=param, master=master, grad=grad, m=m, v=v, ss=ss):
        return [
            lambda: ext.adamw_step(param, master, grad, m, v, ss, 1, 1e-3, 0.9, 0.95, 1e-8,
                                   0.1, n, 0.0),
            lambda: ext.lion_step(param, master, grad, m, ss, 1e-3, 0.9, 0.99, 0.1, n, 0.0),
            lambda: ext.sgd_step(param, master, grad, m, ss, 1e-3, 0.9, 0.1, n, False, 0.0),
        ]

    bad = []
    bad += steps(master=master.double())          # master fp64
    bad += steps(master=big)                      # master 2n long
    bad += steps(master=strided)                  # master not contiguous
    bad += steps(m=m.double())                    # moment fp64
    bad += steps(m=big)
    bad += steps(m=m.cpu())                       # moment on the host
    bad += steps(v=v.double())[:1]                # second moment (AdamW only)
    bad += steps(v=big)[:1]
    bad += steps(grad=grad.half())                # grad fp16
    bad += steps(grad=torch.cat([grad, grad]))    # grad 2n long
    bad += steps(param=param.half())              # param fp16
    bad += steps(ss=ss.double())                  # sumsq fp64
    bad += steps(ss=ss.cpu())                     # sumsq on the host
    _all_rejected(bad)
    # nothing ran: every buffer is as it was
    assert torch.equal(param, master.bfloat16())
    for call in steps():
        call()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(master).all())
