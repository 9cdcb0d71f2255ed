"""Final-logit soft-capping on a real MI355X: the capped cross-entropy kernels
(csrc/cross_entropy.hip: ce_cap_fwd, ce_cap_bwd, ce_vp_cap_*), the elementwise
kernels (csrc/softcap.hip) and what is built on them (ops.softcap,
ops.cross_entropy_capped, vocab_parallel_cross_entropy(softcap=c), the model's
logit_softcap, the trainer), against fp64 references computed from the logits
as stored. The method is that of tests/test_gpu_train_kernels.py and
tests/test_gpu_z_loss.py: every bound is built from the reference's own
magnitudes, every test prints its largest error / bound ratio before it
asserts.

With t = c * tanh(x / c), lse_i = logsumexp_j t_ij, p_ij = e^(t_ij - lse_i),
a = scale_ce, b = scale_z, w_i = a + b * lse_i, the backward writes
    d_ij = g_ij * f_ij,   g_ij = p_ij * w_i - a * [j = y_i],   f_ij = 1 - (t_ij / c)^2
on counted rows and exactly 0 on ignored ones.

The one new constant is SOFTCAP_K: the absolute error of the kernels' t
(softcap_val in csrc/softcap.h) in units of E * c. Measured on an MI355X
against fp64 over GRID below (test_softcap_val_error_over_the_grid prints it):
the largest figure is 3.077 units (cap 30 on logits 30 * randn; 2.914 with the
shift of -40, 2.164 at cap 1 on 30 * randn, 0.811 at cap 30 on randn); the
constant is 4 x that, the margin of the other CE constants. With delta = SOFTCAP_K * E * c:

  lse       lse is 1-Lipschitz in the sup norm of its row, so the capped lse
            errs by delta plus the plain kernel's own error on the row t,
            CE_LSE_K * lse_unit(t) (the row maximum the kernel shifts by is the
            capped raw maximum, off the maximum of its own t by 2 delta at
            most, which moves lse_unit by a term of second order).
  loss_sum  as in test_gpu_z_loss.py with that b_lse, plus delta for t_y.
  z_sum     as there with that b_lse.
  dlogits   g as in test_gpu_z_loss.py with that b_lse in w, and the exponent
            of p off by 2 delta more (t and the delta part of lse):
            |w| * p * expm1(2 delta). The factor: r = t * (1 / c) carries
            delta / c = SOFTCAP_K * E from t and two roundings, e_r =
            (SOFTCAP_K + 2) * E; f = 1 - r^2 (one fma) errs by
            b_f = 2 |r| e_r + e_r^2 + E * f; f <= 1. The product rounds once:
            acc = acc_g * (f + b_f) + |g| * b_f + E * |d|,
            and a bf16 output adds one ulp of the reference.

E, U_BF16, TINY, CE_LSE_K, CE_SUMEXP_K and CE_GRAD_K are copied from
tests/test_gpu_train_kernels.py: they were measured on an MI355X for the same
lse / exp code (units given there) and are the project's own figures."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# copied from tests/test_gpu_train_kernels.py (see the header)
E = 2.0 ** -24        # fp32 unit roundoff
U_BF16 = 2.0 ** -8    # one bf16 ulp, relative
TINY = 2.0 ** -100
CE_LSE_K = 4 * 1.368
CE_SUMEXP_K = 4 * 3.690
CE_GRAD_K = 4 * 1.433
# measured here (see the header): units of E * cap
SOFTCAP_MEASURED = 3.077
SOFTCAP_K = 4 * SOFTCAP_MEASURED

IGN = -100
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
# name -> (N, V): the shapes of tests/test_gpu_z_loss.py
CASES = {
    "one_vector_5x8": (5, 8),
    "row_blocks_loop_4099x264": (4099, 264),   # forward cap is 4096 row blocks
    "bwd_items_loop_4099x2056": (4099, 2056),  # over the backward's 4096 x 256 items
    "wide_vocab_37x50264": (37, 50264),
}
# (cap, logit multiplier): near-linear; |x / c| up to ~4; |x / c| beyond 100,
# where e^(2u) overflows fp32
REGIMES = [(30.0, 1), (30.0, 30), (1.0, 30)]
# (case, dtype, cap, multiplier, shift)
GRID = [(n, dt, c, m, 0.0) for n in CASES for dt in DTYPES for (c, m) in REGIMES]
GRID.append(("row_blocks_loop_4099x264", "fp32", 30.0, 1, -40.0))
GRID.append(("row_blocks_loop_4099x264", "bf16", 30.0, 1, -40.0))


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from mlx_cuda_distributed_pretraining_amd.ops import require_ext

    return require_ext()


def _ulp(dtype):
    return U_BF16 if dtype is torch.bfloat16 else 0.0


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _dev_scalar(v):
    return torch.tensor([v], dtype=torch.float32, device=dev())


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


def _inputs(N, V, dtype, mult, seed, shift=0.0, all_ignored=False):
    """the targets pattern of tests/test_gpu_train_kernels.py: first and last
    vocab id, every fifth row ignored"""
    g = torch.Generator().manual_seed(seed)
    logits = (mult * torch.randn(N, V, generator=g) + shift).to(dtype).to(dev())
    tg = torch.randint(0, V, (N,), generator=g)
    tg[0], tg[1] = 0, V - 1
    tg[2::5] = IGN
    if all_ignored:
        tg[:] = IGN
    return logits, tg.to(dev())


def _cap64(x, c):
    return c * torch.tanh(x.double() / c)


def _ref(logits, tg, c):
    """fp64 t / lse / loss / z of the logits as stored, with the bounds of the
    header (the forms of _ref in tests/test_gpu_z_loss.py on the row t)."""
    delta = SOFTCAP_K * E * c
    t = _cap64(logits, c)
    N, V = t.shape
    m = t.max(-1).values
    zz = t - m[:, None]
    ez = zz.exp()
    se = ez.sum(-1)
    lse = m + se.log()
    A = (ez * zz.abs()).sum(-1) / se
    lse_unit = E * (1 + A + m.abs() + lse.abs())
    b_lse = delta + CE_LSE_K * lse_unit
    mask = tg != IGN
    ty = t.gather(-1, tg.clamp_min(0)[:, None]).squeeze(-1)
    zero = torch.zeros_like(lse)
    row_loss = torch.where(mask, lse - ty, zero)
    row_z = torch.where(mask, lse * lse, zero)
    depth = math.ceil(N / 4096) + 16 + 14
    b_loss = ((b_lse + delta + E * (lse.abs() + ty.abs())) * mask).sum() \
        + depth * E * row_loss.abs().sum()
    b_z = ((2 * lse.abs() * b_lse + b_lse ** 2 + E * lse * lse) * mask).sum() \
        + depth * E * row_z.sum()
    return {"t": t, "c": c, "m": m, "lse": lse, "lse_unit": lse_unit, "b_lse": b_lse,
            "mask": mask, "ty": ty, "loss_sum": row_loss.sum(), "b_loss": b_loss,
            "z_sum": row_z.sum(), "b_z": b_z, "ntok": int(mask.sum())}


@functools.lru_cache(maxsize=None)
def _case(name, dt, c, mult, shift):
    """inputs and reference of one grid case, computed once and shared by the
    tests that use it (nobody writes to them)"""
    N, V = CASES[name]
    logits, tg = _inputs(N, V, DTYPES[dt], mult, seed=N + V + mult, shift=shift)
    return logits, tg, _ref(logits, tg, c)


def _grad_ref(r, tg, a, b, dtype, sc_rel=0.0, lse_unit=None, b_lse=None, cols=None):
    """(reference, bound) of the capped backward: see the header. lse_unit and
    b_lse default to the fused forward's; cols selects a vocab shard."""
    u = _ulp(dtype)
    c = r["c"]
    delta = SOFTCAP_K * E * c
    lse_unit = r["lse_unit"] if lse_unit is None else lse_unit
    b_lse = r["b_lse"] if b_lse is None else b_lse
    lse, mask, t = r["lse"], r["mask"][:, None], r["t"]
    zl = t - lse[:, None]
    p = zl.exp()
    onehot = torch.zeros_like(p)
    rows = torch.nonzero(r["mask"]).squeeze(-1)
    onehot[rows, tg[rows]] = 1.0
    w = (a + b * lse)[:, None]
    bl = (b * lse).abs()[:, None]
    g = p * w - a * onehot
    unit_p = p * (lse_unit[:, None] + E * (1 + zl.abs()))
    acc_g = (w.abs() * (CE_GRAD_K * unit_p + p * math.expm1(2 * delta))
             + p * (abs(b) * b_lse[:, None] + 2 * E * (abs(a) + bl))
             + 2 * E * ((p * w).abs() + abs(a) * onehot)
             + sc_rel * (p * (abs(a) + bl) + abs(a) * onehot))
    rr = (t / c).abs()
    f = 1 - rr * rr
    e_r = (SOFTCAP_K + 2) * E
    b_f = 2 * rr * e_r + e_r ** 2 + E * f
    d = g * f * mask
    acc = (acc_g * (f + b_f) + g.abs() * b_f + E * d.abs() + TINY) * mask
    bound = u * d.abs() + (1 + u) * acc
    if cols is not None:
        d, bound = d[:, cols], bound[:, cols]
    return d, bound


def _check_grad(name, got, r, tg, a, b, dtype, **kw):
    d, bound = _grad_ref(r, tg, a, b, dtype, **kw)
    _check(name, got, d, bound)
    assert not bool(got[~r["mask"]].any()), f"{name}: ignored rows are not exactly 0"


# -------------------------------- softcap_val --------------------------------
def test_softcap_val_error_over_the_grid(ext):
    """The figure behind SOFTCAP_K: |softcap_fwd(x) - c * tanh(x / c)| in units
    of E * c over every grid case (fp32 copies of the logits as stored, so the
    output is the kernel's own fp32 value). Printed per regime, then held to
    the constant; finite and |t| <= c everywhere, t(0) = 0."""
    worst = {}
    for (name, dt, c, mult, shift) in GRID:
        logits, _, r = _case(name, dt, c, mult, shift)
        y = ext.softcap_fwd(logits.float(), c)
        assert bool(torch.isfinite(y).all()) and float(y.abs().max()) <= c
        units = float((y.double() - r["t"]).abs().max()) / (E * c)
        key = (c, mult, shift)
        worst[key] = max(worst.get(key, 0.0), units)
    for key, units in worst.items():
        print(f"softcap_val, (cap, mult, shift) = {key}: {units:.3f} units of E * cap")
    top = max(worst.values())
    print(f"softcap_val: worst {top:.3f} units (SOFTCAP_MEASURED {SOFTCAP_MEASURED}, "
          f"SOFTCAP_K {SOFTCAP_K})")
    edge = torch.tensor([0.0, -0.0, 1e-30, 88.0, -88.0, 3e4, -3e4, 3e38, -3e38],
                        device=dev())
    for c in (1.0, 30.0):
        ye = ext.softcap_fwd(edge, c)
        assert float(ye[0]) == 0.0 and float(ye[1]) == 0.0
        assert bool(torch.isfinite(ye).all()) and float(ye.abs().max()) <= c
        _check(f"edge values, cap {c}", ye, _cap64(edge, c),
               torch.full((9,), SOFTCAP_K * E * c, dtype=torch.float64, device=dev()))
    assert top <= SOFTCAP_K


# --------------------------------- bindings ----------------------------------
@pytest.mark.parametrize("name,dt,c,mult,shift", GRID)
def test_ce_cap_bindings_vs_fp64(ext, name, dt, c, mult, shift):
    """ext.ce_cap_fwd (loss_sum, z_sum, ntok, lse) and ext.ce_cap_bwd against
    fp64; the backward with (a, b) both nonzero, with b = 0 and with a = 0"""
    dtype = DTYPES[dt]
    logits, tg, r = _case(name, dt, c, mult, shift)
    loss_sum, z_sum, ntok, lse = ext.ce_cap_fwd(logits, tg, IGN, c)
    assert int(ntok) == r["ntok"] > 0
    if mult == 30 and c == 1.0 and logits.numel() > 10 ** 6:
        assert float((logits.double() / c).abs().max()) > 100, "meant to be deep saturation"
    _check("lse", lse, r["lse"], r["b_lse"])
    _check("loss_sum", loss_sum, r["loss_sum"], r["b_loss"])
    _check("z_sum", z_sum, r["z_sum"], r["b_z"])

    a = _f32(0.37 / r["ntok"])
    b = _f32(2 * 0.003 / r["ntok"])
    for tag, aa, bb in (("a, b", a, b), ("b = 0", a, 0.0), ("a = 0", 0.0, b)):
        dl = ext.ce_cap_bwd(logits, tg, lse, _dev_scalar(aa), _dev_scalar(bb), IGN, c)
        assert dl.dtype == dtype
        _check_grad(f"dlogits ({tag})", dl, r, tg, aa, bb, dtype)
        if c == 30.0 and mult == 1:
            assert bool(dl.any())


@pytest.mark.parametrize("name,dt,c,mult,shift", GRID)
def test_cross_entropy_capped_vs_fp64(ext, name, dt, c, mult, shift):
    """cross_entropy_capped's two means and, through
    (0.25 * ce + 0.003 * z).backward(), its dlogits. A mean divides its sum by
    ntok (one rounding); the scales 0.25/ntok and 2*0.003/ntok are one fp32
    division each (sc_rel = E)."""
    from mlx_cuda_distributed_pretraining_amd.ops import cross_entropy_capped

    dtype = DTYPES[dt]
    logits, tg, r = _case(name, dt, c, mult, shift)
    leaf = logits.clone().requires_grad_(True)
    ce, z, ntok = cross_entropy_capped(leaf, tg, c, IGN)
    (0.25 * ce + 0.003 * z).backward()
    assert int(ntok) == r["ntok"] > 0 and not ntok.requires_grad
    ce_r, z_r = r["loss_sum"] / r["ntok"], r["z_sum"] / r["ntok"]
    _check("ce", ce, ce_r, r["b_loss"] / r["ntok"] + E * ce_r.abs())
    _check("z", z, z_r, r["b_z"] / r["ntok"] + E * z_r.abs())
    assert leaf.grad.dtype == dtype
    _check_grad("dlogits", leaf.grad, r, tg, 0.25 / r["ntok"], 2 * _f32(0.003) / r["ntok"],
                dtype, sc_rel=E)


def test_capped_sums_are_deterministic(ext):
    """loss_sum and z_sum go through per-block partials and a fixed-order
    reduction: two runs give the same bits (and so do lse and ntok)"""
    logits, tg, _ = _case("row_blocks_loop_4099x264", "bf16", 30.0, 30, 0.0)
    first = ext.ce_cap_fwd(logits, tg, IGN, 30.0)
    again = ext.ce_cap_fwd(logits, tg, IGN, 30.0)
    for x, y in zip(first, again):
        assert torch.equal(x, y)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_all_targets_ignored_and_no_rows(ext, dt):
    """No counted row: both sums and both means 0 (not 0/0), ntok 0, dlogits
    exactly 0, nothing NaN. N = 0: empty results without a launch."""
    from mlx_cuda_distributed_pretraining_amd.ops import cross_entropy_capped

    logits, tg = _inputs(37, 264, DTYPES[dt], 1, seed=5, all_ignored=True)
    loss_sum, z_sum, ntok, lse = ext.ce_cap_fwd(logits, tg, IGN, 30.0)
    assert float(loss_sum) == 0.0 and float(z_sum) == 0.0 and int(ntok) == 0
    assert bool(torch.isfinite(lse).all())
    leaf = logits.clone().requires_grad_(True)
    ce, z, ntok = cross_entropy_capped(leaf, tg, 30.0, IGN)
    (0.25 * ce + 0.003 * z).backward()
    assert float(ce.detach()) == 0.0 and float(z.detach()) == 0.0 and int(ntok) == 0
    assert bool(torch.isfinite(leaf.grad.float()).all())
    assert not bool(leaf.grad.any()), "dlogits of ignored rows are not exactly 0"

    e_l = torch.empty(0, 264, dtype=DTYPES[dt], device=dev())
    e_t = torch.empty(0, dtype=torch.long, device=dev())
    loss_sum, z_sum, ntok, lse = ext.ce_cap_fwd(e_l, e_t, IGN, 30.0)
    assert float(loss_sum) == 0.0 and float(z_sum) == 0.0 and int(ntok) == 0 and lse.numel() == 0
    dl = ext.ce_cap_bwd(e_l, e_t, lse, _dev_scalar(1.0), _dev_scalar(0.0), IGN, 30.0)
    assert dl.shape == e_l.shape
    assert ext.softcap_fwd(e_l, 30.0).shape == e_l.shape
    ext.softcap_(e_l, 30.0)
    if dt == "bf16":
        m, tgt = ext.ce_vp_cap_stats(e_l, e_t, 0, IGN, 30.0)
        assert m.numel() == 0 and ext.ce_vp_cap_sumexp(e_l, m, 30.0).numel() == 0


# -------------------------------- elementwise --------------------------------
ELEMENTWISE = [("fp32", (1, 8), 0), ("bf16", (1, 8), 0), ("fp32", (3, 50264), 0),
               ("bf16", (3, 50264), 0),
               # odd sizes on a base pointer that is not 16-byte aligned (a
               # view one element into its buffer)
               ("fp32", (7, 13), 1), ("bf16", (5, 9), 1), ("bf16", (3, 50264), 3)]


def _offset_view(shape, dtype, mult, seed, off):
    g = torch.Generator().manual_seed(seed)
    n = shape[0] * shape[1]
    buf = (mult * torch.randn(n + off, generator=g)).to(dtype).to(dev())
    x = buf[off:].view(shape)
    assert x.is_contiguous() and (x.data_ptr() % 16 != 0) == (off != 0)
    return x


@pytest.mark.parametrize("dt,shape,off", ELEMENTWISE)
@pytest.mark.parametrize("c,mult", REGIMES)
def test_elementwise_softcap_vs_fp64(ext, dt, shape, off, c, mult):
    """softcap_fwd / softcap_ / softcap_bwd and ops.softcap through autograd.
    Forward: delta, and one bf16 ulp of the reference for a bf16 output.
    Backward from the output as stored, dy * (1 - (y / c)^2): r = y * (1 / c)
    rounds twice (2E |r|, |r| <= 1), so f errs by 4E + E and the product
    rounds once: 6E |dy|, plus the bf16 ulp."""
    from mlx_cuda_distributed_pretraining_amd.ops import softcap, softcap_

    dtype = DTYPES[dt]
    u = _ulp(dtype)
    x = _offset_view(shape, dtype, mult, seed=shape[1] + mult, off=off)
    want = _cap64(x, c)
    bound = u * want.abs() + (1 + u) * SOFTCAP_K * E * c
    y = ext.softcap_fwd(x, c)
    assert y.dtype == dtype and y.shape == x.shape
    _check("softcap_fwd", y, want, bound)
    assert float(y.abs().max()) <= c

    inplace = x.clone()      # the clone is 16-byte aligned: the vector path
    softcap_(inplace, c)
    assert torch.equal(inplace, y), "in place differs from out of place"
    xv = _offset_view(shape, dtype, mult, seed=shape[1] + mult, off=off)
    assert softcap_(xv, c) is xv and torch.equal(xv, y)       # and at the offset

    dy = _offset_view(shape, dtype, 1, seed=7, off=off)
    dx = ext.softcap_bwd(dy, y, c)
    f = 1 - (y.double() / c) ** 2
    want_dx = dy.double() * f
    _check("softcap_bwd", dx, want_dx, u * want_dx.abs() + (1 + u) * 6 * E * dy.double().abs() + TINY)

    leaf = x.clone().requires_grad_(True)
    out = softcap(leaf, c)
    out.backward(dy)
    assert torch.equal(out.detach(), y) and torch.equal(leaf.grad, dx)


def test_non_contiguous_input_takes_the_composition(ext, monkeypatch):
    """A transposed view is not handed to the kernels: ops.softcap runs the
    torch composition, c * tanh(x / c) in fp32. Its bound: x / c rounds once
    (E |u| (1 - tanh^2 u) <= 0.45 E), tanh to 4 ulp at most assumed of the
    device's libm, the product once: 6 E c. Same values as the kernel path
    within the two bounds."""
    import importlib

    from mlx_cuda_distributed_pretraining_amd.ops import softcap

    softcap_mod = importlib.import_module("mlx_cuda_distributed_pretraining_amd.ops.softcap")

    c = 30.0
    base = (30 * torch.randn(64, 24, generator=torch.Generator().manual_seed(3))).to(dev())
    nc = base.t()
    assert not nc.is_contiguous()
    monkeypatch.setattr(softcap_mod._SoftcapFn, "apply",
                        lambda *a: pytest.fail("the kernel path took a strided input"))
    got = softcap(nc, c)
    monkeypatch.undo()
    want = _cap64(nc, c)
    full = lambda k: torch.full_like(want, k * E * c)
    _check("composition", got, want, full(6))
    _check("kernel on the contiguous copy", softcap(nc.contiguous(), c), want, full(SOFTCAP_K))
    with pytest.raises(RuntimeError):
        ext.softcap_fwd(nc, c)


# ------------------------------ vocab-parallel -------------------------------
VP_N, VP_V, VP_HALF = 300, 272, 136
VP_C = 6.0      # logits 3 * randn: |x / c| up to ~2


def _vp_lse_bounds(r, shards, m32):
    """_vp_lse_bounds of tests/test_gpu_z_loss.py on the capped shards: a
    shard's sum-exp errs by CE_SUMEXP_K units of E * sum(e^z * (1 + |z|)),
    z = t - m, and by the factor e^delta of its capped values; the sum of the
    shards, the log and the final addition round once each."""
    delta = SOFTCAP_K * E * r["c"]
    m = m32.double()
    b_se = 0.0
    for sh in shards:
        zz = _cap64(sh, r["c"]) - m[:, None]
        b_se = b_se + CE_SUMEXP_K * E * (zz.exp() * (1 + zz.abs())).sum(-1)
    log_se = r["lse"] - m
    b = delta + b_se / log_se.exp() + E * (1 + log_se.abs() + r["lse"].abs())
    return b, b / CE_LSE_K


def test_vocab_parallel_world1_softcap_equals_cross_entropy_capped(ext):
    """World 1: vocab_parallel_cross_entropy(softcap=c, with_z=True) and
    cross_entropy_capped on the same bf16 logits, each held to its own bound
    around the fp64 reference (the two forwards assemble lse differently): the
    means, and the gradients of 0.25 * ce + 0.003 * z. Without with_z the
    function still returns (loss, ntok)."""
    from mlx_cuda_distributed_pretraining_amd.ops import cross_entropy_capped
    from mlx_cuda_distributed_pretraining_amd.parallel.tp import vocab_parallel_cross_entropy

    logits, tg = _inputs(VP_N, VP_V, torch.bfloat16, 3, seed=12)
    r = _ref(logits, tg, VP_C)
    n = r["ntok"]
    a, b = 0.25 / n, 2 * _f32(0.003) / n
    delta = SOFTCAP_K * E * VP_C

    l1 = logits.clone().requires_grad_(True)
    ce1, z1, n1 = cross_entropy_capped(l1, tg, VP_C, IGN)
    (0.25 * ce1 + 0.003 * z1).backward()
    l2 = logits.clone().requires_grad_(True)
    out = vocab_parallel_cross_entropy(l2, tg, 0, IGN, with_z=True, softcap=VP_C)
    assert len(out) == 3
    ce2, z2, n2 = out
    (0.25 * ce2 + 0.003 * z2).backward()
    two = vocab_parallel_cross_entropy(logits, tg, 0, IGN, softcap=VP_C)
    assert len(two) == 2 and int(two[1]) == n and torch.equal(two[0], ce2.detach())
    assert int(n1) == int(n2) == n

    ce_r, z_r = r["loss_sum"] / n, r["z_sum"] / n
    _check("ce (fused)", ce1, ce_r, r["b_loss"] / n + E * ce_r.abs())
    _check("z (fused)", z1, z_r, r["b_z"] / n + E * z_r.abs())
    _check_grad("dlogits (fused)", l1.grad, r, tg, a, b, torch.bfloat16, sc_rel=E)

    b_lse, lse_unit = _vp_lse_bounds(r, [logits], _cap64(logits, VP_C).max(-1).values.float())
    mask, lse, ty = r["mask"], r["lse"], r["ty"]
    b_ce = ((b_lse + delta + E * (lse.abs() + ty.abs())) * mask).sum() \
        + VP_N * E * ((lse - ty).abs() * mask).sum()
    b_z = ((2 * lse.abs() * b_lse + b_lse ** 2 + E * lse * lse) * mask).sum() \
        + VP_N * E * (lse * lse * mask).sum()
    _check("ce (vocab-parallel)", ce2, ce_r, b_ce / n + E * ce_r.abs())
    _check("z (vocab-parallel)", z2, z_r, b_z / n + E * z_r.abs())
    _check_grad("dlogits (vocab-parallel)", l2.grad, r, tg, a, b, torch.bfloat16, sc_rel=E,
                lse_unit=lse_unit, b_lse=b_lse)
    # the cap matters here: the uncapped loss is somewhere else
    plain = vocab_parallel_cross_entropy(logits, tg, 0, IGN)
    assert abs(float(plain[0]) - float(ce_r)) > 0.05


def test_vocab_parallel_capped_two_shards_by_hand(ext):
    """Two half-vocab shards (the second with v0 = 136) driven by hand through
    ce_vp_cap_stats / ce_vp_cap_sumexp, the group lse assembled in fp32 as
    parallel/tp.py does, then ce_vp_cap_bwd per shard: m and tgt are those of
    the capped shard within delta, the lse is the full row's, and the two
    halves concatenate to ce_cap_bwd's output, each within its bound."""
    logits, tg = _inputs(VP_N, VP_V, torch.bfloat16, 3, seed=13)
    r = _ref(logits, tg, VP_C)
    delta = torch.full((VP_N,), SOFTCAP_K * E * VP_C, dtype=torch.float64, device=dev())
    shards = [logits[:, :VP_HALF].contiguous(), logits[:, VP_HALF:].contiguous()]
    stats = [ext.ce_vp_cap_stats(sh, tg, v0, IGN, VP_C) for v0, sh in zip((0, VP_HALF), shards)]
    for (m_s, _), sh in zip(stats, shards):
        _check("shard max", m_s, _cap64(sh, VP_C).max(-1).values, delta)
    _check("target value", stats[0][1] + stats[1][1], torch.where(r["mask"], r["ty"], 0 * r["ty"]),
           delta)
    m = torch.maximum(stats[0][0], stats[1][0])
    se = ext.ce_vp_cap_sumexp(shards[0], m, VP_C) + ext.ce_vp_cap_sumexp(shards[1], m, VP_C)
    lse = m + torch.log(se)
    b_lse, lse_unit = _vp_lse_bounds(r, shards, m)
    _check("group lse", lse, r["lse"], b_lse)

    a = _f32(0.37 / r["ntok"])
    b = _f32(-a / float(r["lse"][r["mask"]].median()))      # w of both signs
    halves = []
    for v0, sh in zip((0, VP_HALF), shards):
        dl = ext.ce_vp_cap_bwd(sh, tg, lse, _dev_scalar(a), _dev_scalar(b), v0, IGN, VP_C)
        assert dl.dtype == torch.bfloat16 and dl.shape == sh.shape
        d, bound = _grad_ref(r, tg, a, b, torch.bfloat16, lse_unit=lse_unit, b_lse=b_lse,
                             cols=slice(v0, v0 + VP_HALF))
        _check(f"shard dlogits, v0={v0}", dl, d, bound)
        assert not bool(dl[~r["mask"]].any())
        halves.append(dl)
    # one kernel body: from the same lse the halves are ce_cap_bwd's columns
    full = ext.ce_cap_bwd(logits, tg, lse, _dev_scalar(a), _dev_scalar(b), IGN, VP_C)
    d, bound = _grad_ref(r, tg, a, b, torch.bfloat16, lse_unit=lse_unit, b_lse=b_lse)
    _check("ce_cap_bwd from the group lse", full, d, bound)
    _check("halves against ce_cap_bwd", torch.cat(halves, -1), full.double(), 2 * bound)


# -------------------------------- host checks --------------------------------
def test_host_checks_reject_bad_capped_args(ext):
    """cap is checked on the host (finite, > 0) and the tensors as in the z
    bindings, all before any launch."""
    N, V = 16, 64
    c = 30.0
    logits, tg = _inputs(N, V, torch.bfloat16, 1, seed=3)
    loss_sum, z_sum, ntok, lse = ext.ce_cap_fwd(logits, tg, IGN, c)
    a, b = _dev_scalar(0.1), _dev_scalar(0.01)
    good = ext.ce_cap_bwd(logits, tg, lse, a, b, IGN, c)
    good_vp = ext.ce_vp_cap_bwd(logits, tg, lse, a, b, 0, IGN, c)
    m, _ = ext.ce_vp_cap_stats(logits, tg, 0, IGN, c)
    two = torch.cat([a, b])
    l12 = torch.zeros(N, 12, dtype=torch.bfloat16, device=dev())
    bad = []
    for bc in (0.0, -1.0, float("nan"), float("inf"), -float("inf"), 1e39):
        bad += [
            lambda bc=bc: ext.ce_cap_fwd(logits, tg, IGN, bc),
            lambda bc=bc: ext.ce_cap_bwd(logits, tg, lse, a, b, IGN, bc),
            lambda bc=bc: ext.ce_vp_cap_stats(logits, tg, 0, IGN, bc),
            lambda bc=bc: ext.ce_vp_cap_sumexp(logits, m, bc),
            lambda bc=bc: ext.ce_vp_cap_bwd(logits, tg, lse, a, b, 0, IGN, bc),
            lambda bc=bc: ext.softcap_fwd(logits, bc),
            lambda bc=bc: ext.softcap_(logits.clone(), bc),
            lambda bc=bc: ext.softcap_bwd(logits, logits, bc),
        ]
    bad += [
        lambda: ext.ce_cap_fwd(logits, tg.cpu(), IGN, c),                        # targets on the host
        lambda: ext.ce_cap_fwd(logits, tg.int(), IGN, c),                        # targets int32
        lambda: ext.ce_cap_fwd(logits.cpu(), tg.cpu(), IGN, c),                  # logits on the host
        lambda: ext.ce_cap_fwd(logits.half(), tg, IGN, c),                       # fp16
        lambda: ext.ce_cap_fwd(l12, tg, IGN, c),                                 # bf16, V % 8 != 0
        lambda: ext.ce_cap_fwd(logits[:, :32], tg, IGN, c),                      # strided
        lambda: ext.ce_cap_bwd(l12, tg, lse, a, b, IGN, c),
        lambda: ext.ce_cap_bwd(logits, tg.cpu(), lse, a, b, IGN, c),
        lambda: ext.ce_cap_bwd(logits, tg, lse.double(), a, b, IGN, c),          # lse fp64
        lambda: ext.ce_cap_bwd(logits, tg, torch.cat([lse, lse]), a, b, IGN, c), # lse 2N long
        lambda: ext.ce_cap_bwd(logits, tg, lse.cpu(), a, b, IGN, c),
        lambda: ext.ce_cap_bwd(logits, tg, lse, a.double(), b, IGN, c),          # scale fp64
        lambda: ext.ce_cap_bwd(logits, tg, lse, a, b.double(), IGN, c),
        lambda: ext.ce_cap_bwd(logits, tg, lse, two, b, IGN, c),                 # two elements
        lambda: ext.ce_cap_bwd(logits, tg, lse, a, two, IGN, c),
        lambda: ext.ce_cap_bwd(logits, tg, lse, a.cpu(), b, IGN, c),             # scale on the host
        lambda: ext.ce_vp_cap_stats(logits.float(), tg, 0, IGN, c),              # shard not bf16
        lambda: ext.ce_vp_cap_stats(l12, tg, 0, IGN, c),
        lambda: ext.ce_vp_cap_stats(logits, tg.int(), 0, IGN, c),
        lambda: ext.ce_vp_cap_sumexp(logits, m.double(), c),
        lambda: ext.ce_vp_cap_sumexp(logits, torch.cat([m, m]), c),
        lambda: ext.ce_vp_cap_sumexp(logits.float(), m, c),
        lambda: ext.ce_vp_cap_bwd(logits, tg.cpu(), lse, a, b, 0, IGN, c),
        lambda: ext.ce_vp_cap_bwd(logits, tg, lse.double(), a, b, 0, IGN, c),
        lambda: ext.ce_vp_cap_bwd(logits, tg, torch.cat([lse, lse]), a, b, 0, IGN, c),
        lambda: ext.ce_vp_cap_bwd(logits, tg, lse, a.double(), b, 0, IGN, c),
        lambda: ext.ce_vp_cap_bwd(logits, tg, lse, two, b, 0, IGN, c),
        lambda: ext.ce_vp_cap_bwd(logits, tg, lse, a, two, 0, IGN, c),
        lambda: ext.ce_vp_cap_bwd(logits.float(), tg, lse, a, b, 0, IGN, c),
        lambda: ext.softcap_fwd(logits.cpu(), c),
        lambda: ext.softcap_fwd(logits.half(), c),
        lambda: ext.softcap_(logits.t(), c),                                     # strided
        lambda: ext.softcap_bwd(logits, logits.float(), c),                      # dtypes differ
        lambda: ext.softcap_bwd(logits, logits[:8].contiguous(), c),             # shapes differ
    ]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    assert torch.equal(good, ext.ce_cap_bwd(logits, tg, lse, a, b, IGN, c))
    assert torch.equal(good_vp, ext.ce_vp_cap_bwd(logits, tg, lse, a, b, 0, IGN, c))


# ----------------------------------- model -----------------------------------
MODEL_CAP = 5.0


def _bf16_ulp(v):
    """the spacing of bf16 at |v| (normal range)"""
    return 2.0 ** (torch.floor(torch.log2(v.abs().float().clamp_min(2.0 ** -120))) - 7)


@functools.lru_cache(maxsize=None)
def _capped_model():
    """a tiny bf16 model with logit_softcap = 5 and a logit_scale that puts the
    standard deviation of the raw logits at 0.7 * cap, the largest near 2.5 *
    cap: a good part of the vocabulary is in the bend of tanh, and the top
    values still differ after rounding to bf16"""
    from mlx_cuda_distributed_pretraining_amd.models.llama import Model, ModelArgs

    torch.manual_seed(0)
    args = ModelArgs(hidden_size=256, intermediate_size=512, num_layers=2, num_heads=4,
                     num_kv_heads=2, head_dim=128, vocab_size=503, logit_softcap=MODEL_CAP)
    model = Model(args).to(dev(), torch.bfloat16).eval()
    x = torch.tensor([[3, 17, 41, 5, 88, 23, 9, 101, 250, 77]], device=dev())
    with torch.no_grad():
        std = float(model(x, cap_logits=False).float().std())
    model.args.logit_scale = 0.7 * MODEL_CAP / std
    return model, x


def test_model_forward_caps_every_path(ext):
    from mlx_cuda_distributed_pretraining_amd.ops import softcap

    model, x = _capped_model()
    with torch.no_grad():
        raw = model(x, cap_logits=False)
        capped = model(x)
    assert raw.dtype is torch.bfloat16
    frac = float((raw.abs() > MODEL_CAP).float().mean())
    print(f"raw logits: max |x| / cap {float(raw.abs().max()) / MODEL_CAP:.2f}, "
          f"{100 * frac:.1f}% beyond the cap")
    assert frac > 0.05 and float(raw.abs().max()) > 2 * MODEL_CAP
    want = softcap(raw, MODEL_CAP)
    assert float(capped.abs().max()) <= MODEL_CAP
    err = (capped.float() - want.float()).abs()
    print(f"model(x) vs softcap(raw): max err / ulp {float((err / _bf16_ulp(want)).max()):.3f}")
    assert bool((err <= _bf16_ulp(want)).all())
    _check("model(x) vs fp64", capped, _cap64(raw, MODEL_CAP),
           U_BF16 * _cap64(raw, MODEL_CAP).abs() + SOFTCAP_K * E * MODEL_CAP)


def test_captured_graph_decode_is_capped_and_matches_eager(ext):
    """A captured GraphDecoder greedy run of 8 tokens equals eager greedy
    generation, and the logits of every replayed step (the static tensor the
    captured step hands to its argmax) stay within the cap: the in-place
    softcap_ is part of the graph."""
    from mlx_cuda_distributed_pretraining_amd.inference.generate import generate_step
    from mlx_cuda_distributed_pretraining_amd.inference.static_decode import GraphDecoder

    model, x = _capped_model()
    prompt = x[0].tolist()
    n = 8
    oracle = list(generate_step(model, prompt, max_tokens=n))

    dec = GraphDecoder(model, batch=1, max_len=256)
    held = []
    real_pick = dec._pick
    dec._pick = lambda lg: (held.append(lg), real_pick(lg))[1]
    dec.prefill(x)
    assert float(held[-1].abs().max()) <= MODEL_CAP          # the prefill's logits
    dec.capture()
    assert dec.graph is not None
    static_logits = held[-1]                                  # of the captured step
    got, peak = [], 0.0
    for _ in range(n):
        got.append(dec.decode(1)[0].tolist()[0])
        top = float(static_logits.abs().max())
        peak = max(peak, top)
        assert top <= MODEL_CAP and bool(torch.isfinite(static_logits).all())
    print(f"captured decode: tokens {got}, largest |logit| {peak:.4f} (cap {MODEL_CAP})")
    assert peak > 0.8 * MODEL_CAP, "the cap is meant to bite on these logits"
    assert got == oracle, (got, oracle)


# ---------------------------------- trainer ----------------------------------
def test_trainer_step_goes_through_the_capped_kernels(tmp_path, monkeypatch):
    """A 2-layer bf16 trainer with logit_softcap = 5 and a vocabulary of 256:
    the step calls ce_cap_fwd and ce_cap_bwd once each through
    _FusedCECappedFn and none of the plain nodes, and reports the CE of the
    capped bf16 logits. The reference recomputes the raw logits with one more
    forward; should that forward differ from the step's by a bf16 rounding of a
    logit (U_BF16 * |x|), t moves by at most U_BF16 * |x| * (1 - tanh^2(x/c))
    <= U_BF16 * |t| (2u / sinh 2u <= 1), lse by U_BF16 * sum_j p_j |t_j| and
    the row's loss by that plus U_BF16 * |t_y|: the tolerance, next to the
    kernel's own bound."""
    from pathlib import Path

    from mlx_cuda_distributed_pretraining_amd.core.config import Config
    from mlx_cuda_distributed_pretraining_amd.core.trainer import Trainer
    from mlx_cuda_distributed_pretraining_amd.ops import cross_entropy as ce_mod

    repo = Path(__file__).resolve().parents[1]
    cfg = Config.from_yaml(repo / "configs" / "model-config-sample.yaml")
    cfg.name = "gpu-softcap"
    cfg.overwrite = True
    cfg.data.synthetic = True
    cfg.data.synthetic_vocab_size = 253
    cfg.data.tokenizer["normal_vocab_size"] = 253          # + 3 specials = 256
    cfg.model.dimensions = {"hidden_size": 256, "intermediate_size": 512, "num_layers": 2}
    cfg.model.attention = {"num_heads": 4, "num_kv_heads": 2, "head_dim": 64,
                           "max_position_embeddings": 256}
    cfg.model.misc = dict(cfg.model.misc or {}, logit_softcap=MODEL_CAP)
    cfg.data.preprocessing["max_context_size"] = 128
    cfg.training.hyperparameters.update({"batch_size": 4, "iters": 2, "learning_rate": 1e-3})
    cfg.logging.steps = {"logging_interval": 0, "checkpoint_interval": 0,
                         "validation_interval": 0}
    cfg.system.device = "cuda"
    cfg.system.precision = "bfloat16"
    t = Trainer(cfg, runs_root=str(tmp_path / "runs"))
    V = t.model_args.vocab_size
    assert V == 256 and t.device.type == "cuda" and t.param_dtype is torch.bfloat16
    assert t.model_args.logit_softcap == MODEL_CAP

    calls = []
    ext_real = ce_mod.get_ext()

    class Counting:
        def __getattr__(self, name):
            fn = getattr(ext_real, name)
            if name.startswith("ce_"):
                return lambda *a: (calls.append(name), fn(*a))[1]
            return fn

    monkeypatch.setattr(ce_mod, "get_ext", lambda: Counting())
    for node in (ce_mod._FusedCEFn, ce_mod._FusedCEWithZFn):
        monkeypatch.setattr(node, "apply",
                            lambda *a: pytest.fail("a plain loss node ran with a cap configured"))

    batch = t.data_manager.generate_batch(0).to(t.device)
    inputs, targets = batch[:, :-1], batch[:, 1:]
    t.model.train()
    with torch.no_grad():
        # a logit_scale that puts the raw logits' standard deviation at 0.7 * cap
        std = float(t.model(inputs, cap_logits=False).float().std())
        t.model.args.logit_scale = 0.7 * MODEL_CAP / std
        raw = t.model(inputs, cap_logits=False)
    assert raw.dtype is torch.bfloat16
    raw = raw.reshape(-1, V)
    tg = targets.reshape(-1)
    mask = tg != t.tokenizer.PAD_TOKEN
    n = int(mask.sum())
    tg_ref = torch.where(mask, tg, torch.full_like(tg, IGN))
    r = _ref(raw, tg_ref, MODEL_CAP)
    ce_ref = r["loss_sum"] / n
    p = (r["t"] - r["lse"][:, None]).exp()
    d_row = U_BF16 * ((p * r["t"].abs()).sum(-1) + r["ty"].abs())
    tol = float((d_row * mask).sum() / n + r["b_loss"] / n + E * ce_ref.abs())
    frac = float((raw.abs() > MODEL_CAP).float().mean())
    plain = float(torch.nn.functional.cross_entropy(raw.float()[mask], tg[mask]))

    loss, ntok = t.train_step(0)
    assert calls == ["ce_cap_fwd", "ce_cap_bwd"], calls
    assert int(ntok) == n
    got = float(loss.detach())
    print(f"loss: trainer {got:.6f}, fp64 capped {float(ce_ref):.6f}, uncapped {plain:.6f}, "
          f"tolerance {tol:.3e}; {100 * frac:.1f}% of the raw logits beyond the cap")
    assert frac > 0.02 and abs(plain - float(ce_ref)) > 10 * tol, "the cap must matter here"
    assert abs(got - float(ce_ref)) <= tol
    assert t.last_z_loss is None
