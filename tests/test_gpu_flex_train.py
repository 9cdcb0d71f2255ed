"""Trainable flex attention on a real MI355X: the MOD_BLOCKMASK backward
kernels (csrc/attn_bwd.hip) behind flex_attention, against the fp32
composition on the same inputs. Tolerances are the project's own
(test_attn_fwd_gpu / test_attn_bwd_gpu): forward max abs error < 3e-2, each
gradient max abs error < 0.05 * max(max|ref|, 1). Every mask here leaves at
least one live key per row (fully masked rows are out of scope for the kernel
path, see the flex_attention docstring)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from mlx_cuda_distributed_pretraining_amd.ops import require_ext

    return require_ext()


def doc_band(b, h, qi, ki):
    return (ki <= qi) & (qi - ki < 128) & (qi // 200 == ki // 200)


def head_dep(b, h, qi, ki):
    # even heads causal, odd heads a causal band plus 16 sink columns: two
    # different masks inside one GQA group
    c = ki <= qi
    return c if h % 2 == 0 else c & ((qi - ki < 96) | (ki < 16))


def checker(b, h, qi, ki):
    return (((qi // 64) + (ki // 64)) % 2 == 0) | (ki == qi)


def band70(b, h, qi, ki):
    return (ki <= qi) & (qi - ki < 70)


def causal(b, h, qi, ki):
    return ki <= qi


def rel_bias(score, b, h, qi, ki):
    return score - 0.05 * (qi - ki).abs().to(torch.float32)


def _inputs(seed, B, S, Hq, Hkv, D):
    g = torch.Generator(device="cpu").manual_seed(seed)
    mk = lambda h: torch.randn(B, S, h, D, generator=g).to(dev(), torch.bfloat16)  # noqa: E731
    q, k, v = mk(Hq), mk(Hkv), mk(Hkv)
    dy = torch.randn(B, S, Hq, D, generator=g).to(dev(), torch.bfloat16)
    return q, k, v, dy


def _check(name, got, want):
    err = (got.float() - want).abs().max().item()
    bound = 0.05 * max(want.abs().max().item(), 1.0)
    print(f"{name}: max abs err {err:.4g} (bound {bound:.4g})")
    assert math.isfinite(err) and err < bound, f"{name} err {err} >= {bound}"


def _compare(o, q, k, v, ref_o, qf, kf, vf):
    err = (o.detach().float() - ref_o.detach()).abs().max().item()
    print(f"o: max abs err {err:.4g}")
    assert math.isfinite(err) and err < 3e-2, f"forward err {err}"
    _check("dq", q.grad, qf.grad)
    _check("dk", k.grad, kf.grad)
    _check("dv", v.grad, vf.grad)


def _leaves(*ts):
    return [t.detach().float().requires_grad_(True) for t in ts]


# (mask, B, S, Hq, Hkv, D, granule codes 0/1/2 over all of gran)
CASES = {
    "doc_band": (doc_band, 2, 512, 2, 2, 64, (376, 112, 24)),
    "head_dep": (head_dep, 1, 300, 4, 2, 128, (88, 64, 48)),
    "checker": (checker, 1, 512, 2, 2, 64, (128, 0, 128)),
    "band70": (band70, 1, 200, 2, 2, 64, (28, 28, 0)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_flex_blockmask_fwd_bwd_matches_composition(ext, name):
    from mlx_cuda_distributed_pretraining_amd.ops import attention_ref
    from mlx_cuda_distributed_pretraining_amd.ops.attention import (
        CompiledBlockMask, flex_attention,
    )

    mod, B, S, Hq, Hkv, D, codes = CASES[name]
    q, k, v, dy = _inputs(11, B, S, Hq, Hkv, D)
    for t in (q, k, v):
        t.requires_grad_(True)
    bm = CompiledBlockMask(mod, B, Hq, S, S, device=dev())
    assert tuple(int((bm.gran == c).sum()) for c in (0, 1, 2)) == codes
    o = flex_attention(q, k, v, block_mask=bm)
    o.backward(dy)

    qf, kf, vf = _leaves(q, k, v)
    scale = 1.0 / math.sqrt(D)
    if name == "head_dep":
        # attention_ref cannot broadcast a head-dependent mask: one call per
        # q head on slices of the same leaves; autograd sums the GQA group
        group = Hq // Hkv
        outs = []
        for h in range(Hq):
            g = h // group
            outs.append(attention_ref(
                qf[:, :, h:h + 1], kf[:, :, g:g + 1], vf[:, :, g:g + 1], causal=False,
                scale=scale, mask_mod=lambda b, hh, qi, ki, h=h: mod(0, h, qi, ki)))
        ref = torch.cat(outs, dim=2)
    else:
        ref = attention_ref(qf, kf, vf, causal=False, scale=scale, mask_mod=mod)
    ref.backward(dy.float())
    _compare(o, q, k, v, ref, qf, kf, vf)


def test_flex_score_mod_bias_trains_on_kernel_path(ext):
    from mlx_cuda_distributed_pretraining_amd.ops import attention_ref
    from mlx_cuda_distributed_pretraining_amd.ops.attention import flex_attention

    B, S, H, D = 1, 256, 2, 64
    q, k, v, dy = _inputs(12, B, S, H, H, D)
    for t in (q, k, v):
        t.requires_grad_(True)
    assert torch.is_grad_enabled()
    o = flex_attention(q, k, v, score_mod=rel_bias, mask_mod=causal)
    assert type(o.grad_fn).__name__ == "_FlexBlockMaskFnBackward"
    o.backward(dy)
    qf, kf, vf = _leaves(q, k, v)
    ref = attention_ref(qf, kf, vf, causal=False, scale=1.0 / math.sqrt(D),
                        score_mod=rel_bias, mask_mod=causal)
    ref.backward(dy.float())
    _compare(o, q, k, v, ref, qf, kf, vf)


def test_compiled_block_mask_keeps_the_autograd_graph(ext):
    """create_block_mask(device="cuda") + flex_attention under grad used to
    cut the graph silently (no grads, no error)."""
    from mlx_cuda_distributed_pretraining_amd.ops.attention import (
        create_block_mask, flex_attention,
    )

    B, S, H, D = 1, 128, 2, 64
    q, k, v, dy = _inputs(13, B, S, H, H, D)
    for t in (q, k, v):
        t.requires_grad_(True)
    bm = create_block_mask(band70, B, H, S, S, device="cuda")
    flex_attention(q, k, v, block_mask=bm).backward(dy)
    for t in (q, k, v):
        assert t.grad is not None and bool(torch.isfinite(t.grad).all())


def test_mask_mod_under_grad_routes_to_the_kernel_function(ext):
    from mlx_cuda_distributed_pretraining_amd.ops.attention import flex_attention

    B, S, H, D = 1, 128, 2, 64
    q, k, v, _ = _inputs(14, B, S, H, H, D)
    q.requires_grad_(True)
    o = flex_attention(q, k, v, mask_mod=band70)
    assert type(o.grad_fn).__name__ == "_FlexBlockMaskFnBackward"


def test_model_set_flex_mask_matches_fused_causal_path(ext):
    """A causal mask_mod through Model.set_flex_mask vs the same weights on
    the fused causal path. Grad tolerance: that of
    test_fused_qkv_rope_attention_matches_composition (atol = rtol = 5e-2).
    Loss bound 1e-2: both losses are fp32 cross-entropy means over bf16
    logits of magnitude <~ 1 that differ by a few bf16 roundings (2^-9
    relative each), i.e. ~1e-2 per token at the very worst before the mean
    over 254 tokens averages it down."""
    from mlx_cuda_distributed_pretraining_amd.models.llama import Model, ModelArgs

    torch.manual_seed(0)
    args = ModelArgs(hidden_size=128, intermediate_size=256, num_layers=2,
                     num_heads=2, num_kv_heads=2, head_dim=64, vocab_size=256)
    model = Model(args).to(dev(), torch.bfloat16)
    x = torch.randint(0, 256, (2, 129), generator=torch.Generator().manual_seed(1)).to(dev())

    def run():
        model.zero_grad(set_to_none=True)
        logits = model(x[:, :-1])
        loss = torch.nn.functional.cross_entropy(
            logits.reshape(-1, 256).float(), x[:, 1:].reshape(-1))
        loss.backward()
        return float(loss.detach()), [l.attention.wqkv.weight.grad.float().clone()
                             for l in model.layers]

    loss0, g0 = run()
    model.set_flex_mask(causal)
    loss1, g1 = run()
    print(f"loss fused {loss0:.6f} flex {loss1:.6f}")
    assert math.isfinite(loss1) and abs(loss1 - loss0) < 1e-2
    for a, b in zip(g1, g0):
        assert torch.allclose(a, b, atol=5e-2, rtol=5e-2), (a - b).abs().max()
