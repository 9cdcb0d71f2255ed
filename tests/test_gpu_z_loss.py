"""The z-loss cross-entropy kernels on a real MI355X (csrc/cross_entropy.hip:
ce_fwd_z, ce_bwd_z, ce_vp_bwd_z) and what is built on them
(ops.cross_entropy_with_z, vocab_parallel_cross_entropy(with_z=True), the
trainer's z_loss_coef), against an fp64 reference computed from the logits as
stored. The method is that of tests/test_gpu_train_kernels.py: every bound is
built from the reference's own magnitudes, every test prints its largest
error / bound ratio before it asserts.

With a = scale_ce, b = scale_z and w_i = a + b * lse_i the backward writes
    d_ij = p_ij * w_i - a * [j = t_i],      p_ij = e^(l_ij - lse_i),
on counted rows and exactly 0 on ignored ones. Its bound is absolute (w_i can
cancel, so nothing here is relative to |d|):
    |w_i| * CE_GRAD_K * unit_p                      the fast exp and the lse in p
  + p * (|b| * b_lse_i + 2E * (|a| + |b * lse_i|))  the kernel's lse in w, w's roundings
  + 2E * (|p * w_i| + |a| * [j = t])                product and subtraction
  + sc_rel * (p * (|a| + |b * lse_i|) + |a| * [j = t])   scales divided on the device
  + TINY,
with unit_p = p * (lse_unit + E * (1 + |l - lse|)) as in that file's
_ce_grad_ref; a bf16 output adds one ulp of the reference on top.

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

IGN = -100
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
# name -> (N, V)
CASES = {
    "one_vector_5x8": (5, 8),
    "row_blocks_loop_4099x264": (4099, 264),   # forward cap is 4096 row blocks
    # 4099 * 2056 / 8 = 1 053 443 work items: over the backward's 4096 x 256 cap
    "bwd_items_loop_4099x2056": (4099, 2056),
    "wide_vocab_37x50264": (37, 50264),
}
# (case, dtype, logit multiplier, shift): x30 puts the row maxima near 120
# (lse^2 ~ 1.4e4); the shift by -40 makes every lse negative
GRID = [(n, dt, m, 0.0) for n in CASES for dt in DTYPES for m in (1, 30)]
GRID.append(("row_blocks_loop_4099x264", "fp32", 1, -40.0))
GRID.append(("row_blocks_loop_4099x264", "bf16", 1, -40.0))


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


def _ref(logits, tg):
    """fp64 lse / loss / z of the logits as stored, with bounds. lse and
    loss_sum as in _ce_ref of tests/test_gpu_train_kernels.py. z_sum adds the
    counted rows' lse^2, squared in fp32 from the kernel's own lse:
    2|lse| b_lse + b_lse^2 for that lse, E lse^2 for the square, and the
    reduction it shares with loss_sum (thread 0 of a block adds its
    ceil(N/4096) rows in turn, then 16 partials per thread and a 14-level
    tree): depth * E * sum(lse^2), depth = ceil(N/4096) + 16 + 14."""
    l = logits.double()
    N, V = l.shape
    m = l.max(-1).values
    zz = l - m[:, None]
    ez = zz.exp()
    se = ez.sum(-1)
    lse = m + se.log()
    A = (ez * zz.abs()).sum(-1) / se
    lse_unit = E * (1 + A + m.abs() + lse.abs())
    b_lse = CE_LSE_K * lse_unit
    mask = tg != IGN
    lt = l.gather(-1, tg.clamp_min(0)[:, None]).squeeze(-1)
    zero = torch.zeros_like(lse)
    row_loss = torch.where(mask, lse - lt, zero)
    row_z = torch.where(mask, lse * lse, zero)
    depth = math.ceil(N / 4096) + 16 + 14
    b_loss = ((b_lse + E * (lse.abs() + lt.abs())) * mask).sum() + depth * E * row_loss.abs().sum()
    b_z = ((2 * lse.abs() * b_lse + b_lse ** 2 + E * lse * lse) * mask).sum() \
        + depth * E * row_z.sum()
    return {"l": l, "m": m, "lse": lse, "lse_unit": lse_unit, "b_lse": b_lse, "mask": mask,
            "loss_sum": row_loss.sum(), "b_loss": b_loss, "z_sum": row_z.sum(), "b_z": b_z,
            "ntok": int(mask.sum())}


@functools.lru_cache(maxsize=None)
def _case(name, dt, mult, shift):
    """inputs and reference of one grid case, computed once and shared by the
    tests that use it (nobody writes to them)"""
    N, V = CASES[name]
    logits, tg = _inputs(N, V, DTYPES[dt], mult, seed=N + V + mult, shift=shift)
    return logits, tg, _ref(logits, tg)


def _grad_ref(r, tg, a, b, dtype, sc_rel=0.0, lse_unit=None, b_lse=None, cols=None):
    """(reference, bound, w) of the z backward: see the header. lse_unit and
    b_lse default to the fused forward's; cols selects a vocab shard."""
    u = _ulp(dtype)
    lse_unit = r["lse_unit"] if lse_unit is None else lse_unit
    b_lse = r["b_lse"] if b_lse is None else b_lse
    lse, mask = r["lse"], r["mask"][:, None]
    zl = r["l"] - lse[:, None]
    p = zl.exp()
    onehot = torch.zeros_like(p)
    rows = torch.nonzero(r["mask"]).squeeze(-1)
    onehot[rows, tg[rows]] = 1.0
    w = (a + b * lse)[:, None]
    bl = (b * lse).abs()[:, None]
    d = (p * w - a * onehot) * mask
    unit_p = p * (lse_unit[:, None] + E * (1 + zl.abs()))
    acc = (w.abs() * CE_GRAD_K * unit_p
           + p * (abs(b) * b_lse[:, None] + 2 * E * (abs(a) + bl))
           + 2 * E * ((p * w).abs() + abs(a) * onehot)
           + sc_rel * (p * (abs(a) + bl) + abs(a) * onehot)
           + TINY) * mask
    bound = u * d.abs() + (1 + u) * acc
    if cols is not None:
        d, bound = d[:, cols], bound[:, cols]
    return d, bound, w.squeeze(-1)


def _check_grad(name, got, r, tg, a, b, dtype, **kw):
    d, bound, w = _grad_ref(r, tg, a, b, dtype, **kw)
    _check(name, got, d, bound)
    assert not bool(got[~r["mask"]].any()), f"{name}: ignored rows are not exactly 0"
    if "cols" not in kw:
        # each counted row sums to b * lse_i, within the sum of its element bounds
        want = torch.where(r["mask"], b * r["lse"], torch.zeros_like(r["lse"]))
        assert torch.allclose(d.sum(-1), want, rtol=1e-9, atol=1e-12 * (abs(a) + abs(b)))
        _check(name + " row sums", got.double().sum(-1), want, bound.sum(-1))
    return w


@pytest.mark.parametrize("name,dt,mult,shift", GRID)
def test_ce_z_bindings_vs_fp64(ext, name, dt, mult, shift):
    """ext.ce_fwd_z (loss_sum, z_sum, ntok, lse) and ext.ce_bwd_z against fp64,
    the backward twice: with a positive scale_z, and with scale_z = -a / median
    lse, which makes w_i = a + b * lse_i negative on about half of the counted
    rows and positive on the others."""
    dtype = DTYPES[dt]
    logits, tg, r = _case(name, dt, mult, shift)
    loss_sum, z_sum, ntok, lse = ext.ce_fwd_z(logits, tg, IGN)
    assert int(ntok) == r["ntok"] > 0
    if shift < 0:
        assert float(r["lse"].max()) < 0, "the shifted case is meant to have lse < 0"
    need = float(((lse.double() - r["lse"]).abs() / r["lse_unit"]).max())
    print(f"lse: fast exp/log error {need:.3f} units (bound {CE_LSE_K:.3f})")
    _check("lse", lse, r["lse"], r["b_lse"])
    _check("loss_sum", loss_sum, r["loss_sum"], r["b_loss"])
    _check("z_sum", z_sum, r["z_sum"], r["b_z"])

    a = _f32(0.37 / r["ntok"])
    b_pos = _f32(2 * 0.003 / r["ntok"])
    b_mixed = _f32(-a / float(r["lse"][r["mask"]].median()))
    for tag, b in (("b>0", b_pos), ("mixed w", b_mixed)):
        dl = ext.ce_bwd_z(logits, tg, lse, _dev_scalar(a), _dev_scalar(b), IGN)
        assert dl.dtype == dtype
        w = _check_grad(f"dlogits ({tag})", dl, r, tg, a, b, dtype)
        if tag == "mixed w":
            wc = w[r["mask"]]
            n_neg, n_pos = int((wc < 0).sum()), int((wc > 0).sum())
            print(f"mixed w: {n_neg} counted rows with w < 0, {n_pos} with w > 0")
            assert n_neg > 0 and n_pos > 0


@pytest.mark.parametrize("name,dt,mult,shift", GRID)
def test_cross_entropy_with_z_vs_fp64(ext, name, dt, mult, shift):
    """cross_entropy_with_z's two means and, through
    (0.25 * ce + 0.003 * z).backward(), its dlogits. A mean divides its sum by
    ntok (one rounding); the scales 0.25/ntok and 2*0.003/ntok are one fp32
    division each (sc_rel = E)."""
    from mlx_cuda_distributed_pretraining_amd.ops import cross_entropy_with_z

    dtype = DTYPES[dt]
    logits, tg, r = _case(name, dt, mult, shift)
    leaf = logits.clone().requires_grad_(True)
    ce, z, ntok = cross_entropy_with_z(leaf, tg, IGN)
    (0.25 * ce + 0.003 * z).backward()
    assert int(ntok) == r["ntok"] > 0
    ce_r, z_r = r["loss_sum"] / r["ntok"], r["z_sum"] / r["ntok"]
    _check("ce", ce, ce_r, r["b_loss"] / r["ntok"] + E * ce_r.abs())
    _check("z", z, z_r, r["b_z"] / r["ntok"] + E * z_r.abs())
    assert leaf.grad.dtype == dtype
    _check_grad("dlogits", leaf.grad, r, tg, 0.25 / r["ntok"], 2 * _f32(0.003) / r["ntok"],
                dtype, sc_rel=E)


@pytest.mark.parametrize("name,dt,mult,shift", [g for g in GRID if g[2] == 1])
def test_zero_scale_z_is_the_plain_path_bit_for_bit(ext, name, dt, mult, shift):
    """scale_z = 0: ce_bwd_z's dlogits equal ce_bwd's, and ce_fwd_z's loss_sum,
    lse and ntok equal ce_fwd's, bit for bit"""
    logits, tg, r = _case(name, dt, mult, shift)
    loss_p, ntok_p, lse_p = ext.ce_fwd(logits, tg, IGN)
    loss_z, z_sum, ntok_z, lse_z = ext.ce_fwd_z(logits, tg, IGN)
    assert torch.equal(loss_p, loss_z) and torch.equal(lse_p, lse_z)
    assert torch.equal(ntok_p, ntok_z)
    a = _dev_scalar(0.37 / r["ntok"])
    plain = ext.ce_bwd(logits, tg, lse_p, a, IGN)
    with_z = ext.ce_bwd_z(logits, tg, lse_p, a, _dev_scalar(0.0), IGN)
    assert torch.equal(plain, with_z)
    assert bool(plain.any())


def test_z_sum_is_deterministic(ext):
    """z_sum goes through per-block partials and a fixed-order reduction: four
    calls give the same bits (and so do loss_sum and lse)"""
    logits, tg, _ = _case("row_blocks_loop_4099x264", "bf16", 30, 0.0)
    first = ext.ce_fwd_z(logits, tg, IGN)
    for _ in range(3):
        again = ext.ce_fwd_z(logits, tg, IGN)
        for x, y in zip(first, again):
            assert torch.equal(x, y)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_all_targets_ignored(ext, dt):
    """No counted row: both sums and both means 0 (not 0/0), ntok 0, dlogits
    exactly 0, nothing NaN"""
    from mlx_cuda_distributed_pretraining_amd.ops import cross_entropy_with_z

    logits, tg = _inputs(37, 264, DTYPES[dt], 1, seed=5, all_ignored=True)
    loss_sum, z_sum, ntok, lse = ext.ce_fwd_z(logits, tg, IGN)
    assert float(loss_sum) == 0.0 and float(z_sum) == 0.0 and int(ntok) == 0
    assert bool(torch.isfinite(lse).all())
    leaf = logits.clone().requires_grad_(True)
    ce, z, ntok = cross_entropy_with_z(leaf, tg, IGN)
    (0.25 * ce + 0.003 * z).backward()
    assert float(ce.detach()) == 0.0 and float(z.detach()) == 0.0 and int(ntok) == 0
    assert bool(torch.isfinite(leaf.grad.float()).all())
    assert not bool(leaf.grad.any()), "dlogits of ignored rows are not exactly 0"


# ------------------------------ vocab-parallel -------------------------------
VP_N, VP_V, VP_HALF = 300, 272, 136


def _vp_lse_bounds(r, shards, m32):
    """error bound of lse = m + log(sum of the shards' sum-exp) taken in fp32
    from ce_vp_sumexp outputs: a shard's sum-exp errs by at most CE_SUMEXP_K
    units of E * sum(e^z * (1 + |z|)), z = l - m (tests/test_gpu_train_kernels
    .py), the sum of the shards, the log and the final addition round once
    each. Returned as (b_lse, lse_unit = b_lse / CE_LSE_K), the form _grad_ref
    takes."""
    m = m32.double()
    b_se = 0.0
    for sh in shards:
        zz = sh.double() - m[:, None]
        b_se = b_se + CE_SUMEXP_K * E * (zz.exp() * (1 + zz.abs())).sum(-1)
    log_se = r["lse"] - m
    b = b_se / log_se.exp() + E * (1 + log_se.abs() + r["lse"].abs())
    return b, b / CE_LSE_K


def test_vocab_parallel_world1_with_z_equals_cross_entropy_with_z(ext):
    """World 1: vocab_parallel_cross_entropy(with_z=True) and
    cross_entropy_with_z on the same bf16 logits. The two forwards assemble
    lse differently (ce_vp_stats / ce_vp_sumexp and torch.log against one
    kernel), so each is held to its own bound around the fp64 reference: the
    means, and the gradients of 0.25 * ce + 0.003 * z. The row sums of the
    vocab-parallel path's torch reductions take n terms in unknown order:
    n * E * sum|terms|."""
    from mlx_cuda_distributed_pretraining_amd.ops import cross_entropy_with_z
    from mlx_cuda_distributed_pretraining_amd.parallel.tp import vocab_parallel_cross_entropy

    logits, tg = _inputs(VP_N, VP_V, torch.bfloat16, 3, seed=12)
    r = _ref(logits, tg)
    n = r["ntok"]
    a, b = 0.25 / n, 2 * _f32(0.003) / n

    l1 = logits.clone().requires_grad_(True)
    ce1, z1, n1 = cross_entropy_with_z(l1, tg, IGN)
    (0.25 * ce1 + 0.003 * z1).backward()
    l2 = logits.clone().requires_grad_(True)
    out = vocab_parallel_cross_entropy(l2, tg, 0, IGN, with_z=True)
    assert len(out) == 3
    ce2, z2, n2 = out
    (0.25 * ce2 + 0.003 * z2).backward()
    plain = vocab_parallel_cross_entropy(logits, tg, 0, IGN)
    assert len(plain) == 2 and int(plain[1]) == n
    assert int(n1) == int(n2) == n

    ce_r, z_r = r["loss_sum"] / n, r["z_sum"] / n
    _check("ce (fused)", ce1, ce_r, r["b_loss"] / n + E * ce_r.abs())
    _check("z (fused)", z1, z_r, r["b_z"] / n + E * z_r.abs())
    _check_grad("dlogits (fused)", l1.grad, r, tg, a, b, torch.bfloat16, sc_rel=E)

    b_lse, lse_unit = _vp_lse_bounds(r, [logits], r["m"].float())
    mask, lse = r["mask"], r["lse"]
    lt = r["l"].gather(-1, tg.clamp_min(0)[:, None]).squeeze(-1)
    b_ce = ((b_lse + E * (lse.abs() + lt.abs())) * mask).sum() \
        + VP_N * E * ((lse - lt).abs() * mask).sum()
    b_z = ((2 * lse.abs() * b_lse + b_lse ** 2 + E * lse * lse) * mask).sum() \
        + VP_N * E * (lse * lse * mask).sum()
    _check("ce (vocab-parallel)", ce2, ce_r, b_ce / n + E * ce_r.abs())
    _check("z (vocab-parallel)", z2, z_r, b_z / n + E * z_r.abs())
    _check("plain vocab-parallel loss", plain[0], ce_r, b_ce / n + E * ce_r.abs())
    _check_grad("dlogits (vocab-parallel)", l2.grad, r, tg, a, b, torch.bfloat16, sc_rel=E,
                lse_unit=lse_unit, b_lse=b_lse)


def test_vocab_parallel_z_backward_two_shards_by_hand(ext):
    """Two half-vocab shards (the second with v0 = 136) driven by hand through
    ce_vp_stats / ce_vp_sumexp, the group lse assembled in fp32 as
    parallel/tp.py does, then ce_vp_bwd_z per shard: the two halves of the
    full-vocab z gradient, within the bounds of the header with the lse error
    of this forward (_vp_lse_bounds)."""
    logits, tg = _inputs(VP_N, VP_V, torch.bfloat16, 3, seed=13)
    r = _ref(logits, tg)
    shards = [logits[:, :VP_HALF].contiguous(), logits[:, VP_HALF:].contiguous()]
    stats = [ext.ce_vp_stats(sh, tg, v0, IGN) for v0, sh in zip((0, VP_HALF), shards)]
    m = torch.maximum(stats[0][0], stats[1][0])
    assert torch.equal(m.double(), r["m"])
    se = ext.ce_vp_sumexp(shards[0], m) + ext.ce_vp_sumexp(shards[1], m)
    lse = m + torch.log(se)
    b_lse, lse_unit = _vp_lse_bounds(r, shards, m)
    _check("group lse", lse, r["lse"], b_lse)

    a = _f32(0.37 / r["ntok"])
    b = _f32(-a / float(r["lse"][r["mask"]].median()))      # w of both signs
    for v0, sh in zip((0, VP_HALF), shards):
        dl = ext.ce_vp_bwd_z(sh, tg, lse, _dev_scalar(a), _dev_scalar(b), v0, IGN)
        assert dl.dtype == torch.bfloat16 and dl.shape == sh.shape
        d, bound, w = _grad_ref(r, tg, a, b, torch.bfloat16, lse_unit=lse_unit, b_lse=b_lse,
                                cols=slice(v0, v0 + VP_HALF))
        _check(f"shard dlogits, v0={v0}", dl, d, bound)
        assert not bool(dl[~r["mask"]].any())
        # scale_z = 0 is the plain shard backward, bit for bit
        assert torch.equal(ext.ce_vp_bwd(sh, tg, lse, _dev_scalar(a), v0, IGN),
                           ext.ce_vp_bwd_z(sh, tg, lse, _dev_scalar(a), _dev_scalar(0.0), v0, IGN))
    wc = w[r["mask"]]
    assert int((wc < 0).sum()) > 0 and int((wc > 0).sum()) > 0


# -------------------------------- host checks --------------------------------
def test_host_checks_reject_bad_z_args(ext):
    """The new bindings index targets and lse by row and read both scales as
    one float each: all of it is checked before any launch."""
    N, V = 16, 64
    logits, tg = _inputs(N, V, torch.bfloat16, 1, seed=3)
    loss_sum, z_sum, ntok, lse = ext.ce_fwd_z(logits, tg, IGN)
    a, b = _dev_scalar(0.1), _dev_scalar(0.01)
    good = ext.ce_bwd_z(logits, tg, lse, a, b, IGN)
    good_vp = ext.ce_vp_bwd_z(logits, tg, lse, a, b, 0, IGN)
    two = torch.cat([a, b])
    l12 = torch.zeros(N, 12, dtype=torch.bfloat16, device=dev())
    bad = [
        lambda: ext.ce_fwd_z(logits, tg.cpu(), IGN),                          # targets on the host
        lambda: ext.ce_fwd_z(logits, tg.int(), IGN),                          # targets int32
        lambda: ext.ce_fwd_z(l12, tg, IGN),                                   # bf16, V % 8 != 0
        lambda: ext.ce_bwd_z(logits, tg.cpu(), lse, a, b, IGN),
        lambda: ext.ce_bwd_z(logits, tg.int(), lse, a, b, IGN),
        lambda: ext.ce_bwd_z(logits, tg, lse.double(), a, b, IGN),            # lse fp64
        lambda: ext.ce_bwd_z(logits, tg, torch.cat([lse, lse]), a, b, IGN),   # lse 2N long
        lambda: ext.ce_bwd_z(logits, tg, lse, a.double(), b, IGN),            # scale fp64
        lambda: ext.ce_bwd_z(logits, tg, lse, a, b.double(), IGN),
        lambda: ext.ce_bwd_z(logits, tg, lse, two, b, IGN),                   # two elements
        lambda: ext.ce_bwd_z(logits, tg, lse, a, two, IGN),
        lambda: ext.ce_bwd_z(logits, tg, lse, a.cpu(), b, IGN),               # scale on the host
        lambda: ext.ce_vp_bwd_z(logits, tg.cpu(), lse, a, b, 0, IGN),
        lambda: ext.ce_vp_bwd_z(logits, tg.int(), lse, a, b, 0, IGN),
        lambda: ext.ce_vp_bwd_z(logits, tg, lse.double(), a, b, 0, IGN),
        lambda: ext.ce_vp_bwd_z(logits, tg, torch.cat([lse, lse]), a, b, 0, IGN),
        lambda: ext.ce_vp_bwd_z(logits, tg, lse, a.double(), b, 0, IGN),
        lambda: ext.ce_vp_bwd_z(logits, tg, lse, a, b.double(), 0, IGN),
        lambda: ext.ce_vp_bwd_z(logits, tg, lse, two, b, 0, IGN),
        lambda: ext.ce_vp_bwd_z(logits, tg, lse, a, two, 0, IGN),
        lambda: ext.ce_vp_bwd_z(logits.float(), tg, lse, a, b, 0, IGN),       # shard not bf16
    ]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    assert torch.equal(good, ext.ce_bwd_z(logits, tg, lse, a, b, IGN))
    assert torch.equal(good_vp, ext.ce_vp_bwd_z(logits, tg, lse, a, b, 0, IGN))


# ---------------------------------- trainer ----------------------------------
def test_trainer_step_reports_z_loss_through_the_fused_path(tmp_path, monkeypatch):
    """A 2-layer bf16 trainer with z_loss_coef = 1e-3 and a vocabulary of 256
    (V % 8 == 0): the step goes through _FusedCEWithZFn, and trainer.last_z_loss
    is mean(lse^2) of the model's bf16 logits. The reference recomputes the
    logits with one more forward before the step; should that forward differ
    from the step's by a bf16 rounding of a logit (one ulp, U_BF16 * |l|), lse
    moves by at most U_BF16 * sum_j p_j |l_j| and z by the mean of 2|lse| times
    that, which is the tolerance, next to the kernel's own z bound."""
    from pathlib import Path

    from mlx_cuda_distributed_pretraining_amd.core.config import Config
    from mlx_cuda_distributed_pretraining_amd.core.trainer import Trainer
    from mlx_cuda_distributed_pretraining_amd.ops import cross_entropy as ce_mod

    repo = Path(__file__).resolve().parents[1]
    cfg = Config.from_yaml(repo / "configs" / "model-config-sample.yaml")
    cfg.name = "gpu-z-loss"
    cfg.overwrite = True
    cfg.data.synthetic = True
    cfg.data.synthetic_vocab_size = 253
    cfg.data.tokenizer["normal_vocab_size"] = 253          # + 3 specials = 256
    cfg.model.dimensions = {"hidden_size": 256, "intermediate_size": 512, "num_layers": 2}
    cfg.model.attention = {"num_heads": 4, "num_kv_heads": 2, "head_dim": 64,
                           "max_position_embeddings": 256}
    cfg.data.preprocessing["max_context_size"] = 128
    cfg.training.hyperparameters.update({"batch_size": 4, "iters": 2, "learning_rate": 1e-3,
                                         "z_loss_coef": 1e-3})
    cfg.logging.steps = {"logging_interval": 0, "checkpoint_interval": 0,
                         "validation_interval": 0}
    cfg.system.device = "cuda"
    cfg.system.precision = "bfloat16"
    t = Trainer(cfg, runs_root=str(tmp_path / "runs"))
    V = t.model_args.vocab_size
    assert V == 256 and t.device.type == "cuda" and t.param_dtype is torch.bfloat16

    calls = []
    real_apply = ce_mod._FusedCEWithZFn.apply
    monkeypatch.setattr(ce_mod._FusedCEWithZFn, "apply",
                        lambda *args: (calls.append(1), real_apply(*args))[1])

    batch = t.data_manager.generate_batch(0).to(t.device)
    inputs, targets = batch[:, :-1], batch[:, 1:]
    t.model.train()
    with torch.no_grad():
        logits = t.model(inputs)
    assert logits.dtype is torch.bfloat16
    logits = logits.reshape(-1, V)
    tg = targets.reshape(-1)
    mask = tg != t.tokenizer.PAD_TOKEN
    n = int(mask.sum())
    lse32 = torch.logsumexp(logits.float(), -1)
    z32 = float((lse32 * lse32 * mask).sum() / n)

    l = logits.double()
    lse = torch.logsumexp(l, -1)
    p = (l - lse[:, None]).exp()
    d_lse = U_BF16 * (p * l.abs()).sum(-1)
    tg_ref = torch.where(mask, tg, torch.full_like(tg, IGN))
    r = _ref(logits, tg_ref)
    z_ref = r["z_sum"] / n
    tol = float((2 * lse.abs() * d_lse * mask).sum() / n + r["b_z"] / n + E * z_ref.abs())

    loss, ntok = t.train_step(0)
    assert calls == [1], "the step did not go through the fused z-loss node"
    assert int(ntok) == n
    z_got = float(t.last_z_loss)
    print(f"z_loss: trainer {z_got:.6f}, fp64 {float(z_ref):.6f}, fp32 torch {z32:.6f}, "
          f"tolerance {tol:.3e}")
    assert abs(z_got - float(z_ref)) <= tol
    # the fp32 torch figure itself: V-term sums in lse (2 * V * E relative on z,
    # |lse| > 1 here) and an N-term mean
    assert float(lse.abs().min()) > 1.0
    assert abs(z_got - z32) <= tol + (2 * V + logits.shape[0] + 8) * E * abs(z32)
    assert "z_loss=" in t.format_z_loss()
    assert bool(torch.isfinite(loss))
