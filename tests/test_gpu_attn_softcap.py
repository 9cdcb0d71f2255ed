"""Attention-logit soft-capping on a real MI355X: the capped instantiations of
the forward, dQ, split dK / dV, merged dK+dV and decode kernels
(csrc/attn_fwd.hip, csrc/attn_bwd.hip, csrc/decode.hip) behind
flash_attention(softcap=) / rope_flash_attention_qkv(softcap=) / the model's
attention.logit_softcap, against attention_ref(softcap=c) on fp32 leaves.
Tolerances are the project's own (tests/test_gpu_doc_mask.py): forward max abs
error < 3e-2, each gradient max abs error < 0.05 * max(max|ref|, 1).

Inputs are randn bf16 from a CPU generator seeded with 31, scale 1/sqrt(D).
With c = 2 the uncapped result is far outside those tolerances (forward off by
more than 1, every gradient by more than 1), so the cases fail unless the cap
is applied forward and backward."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

CAP = 2.0
MOD_NONE, MOD_CAUSAL, MOD_SLIDING_WINDOW, MOD_PREFIX_LM, MOD_ALIBI = 0, 1, 2, 3, 4


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from mlx_cuda_distributed_pretraining_amd.ops import require_ext

    return require_ext()


def _inputs(B, Sq, Skv, Hq, Hkv, D, qmult=1.0, seed=31):
    g = torch.Generator(device="cpu").manual_seed(seed)
    mk = lambda s, h: torch.randn(B, s, h, D, generator=g)  # noqa: E731
    q, k, v, dy = mk(Sq, Hq) * qmult, mk(Skv, Hkv), mk(Skv, Hkv), mk(Sq, Hq)
    return [t.to(dev(), torch.bfloat16) for t in (q, k, v, dy)]


def _leaves(*ts):
    return [t.detach().float().requires_grad_(True) for t in ts]


def _check_fwd(o, ref):
    assert bool(torch.isfinite(o).all()), "o has non-finite values"
    err = (o.detach().float() - ref.detach().float()).abs().max().item()
    print(f"o: max abs err {err:.4g} (bound 0.03)")
    assert math.isfinite(err) and err < 3e-2, f"forward err {err}"


def _check_grad(name, got, want):
    assert bool(torch.isfinite(got).all()), f"{name} has non-finite values"
    err = (got.float() - want).abs().max().item()
    bound = 0.05 * max(want.abs().max().item(), 1.0)
    print(f"{name}: max abs err {err:.4g} (bound {bound:.4g})")
    assert math.isfinite(err) and err < bound, f"{name} err {err} >= {bound}"


# name -> (B, Sq, Skv, Hq, Hkv, D, q multiplier, mask keywords)
CASES = {
    # ragged last tile; D=128 runs the merged dK+dV kernel
    "causal_d128_merged": (1, 300, 300, 2, 2, 128, 1.0, dict(causal=True)),
    # GQA, the split dK / dV pair, 128-row kv tiles, half the scores saturated
    "causal_d64_gqa_q3": (2, 512, 512, 4, 2, 64, 3.0, dict(causal=True)),
    # MQA, window not a tile multiple
    "window100_d128_mqa": (1, 512, 512, 4, 1, 128, 1.0, dict(causal=True, window=100)),
    # full attention, Sq != Skv, both ragged
    "full_192x300_d64": (1, 192, 300, 2, 1, 64, 1.0, dict(causal=False)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_capped_fwd_bwd_matches_reference(ext, name):
    from mlx_cuda_distributed_pretraining_amd.ops import attention_ref, flash_attention

    B, Sq, Skv, Hq, Hkv, D, qmult, kw = CASES[name]
    q, k, v, dy = _inputs(B, Sq, Skv, Hq, Hkv, D, qmult)
    for t in (q, k, v):
        t.requires_grad_(True)
    o = flash_attention(q, k, v, softcap=CAP, **kw)
    o.backward(dy)
    qf, kf, vf = _leaves(q, k, v)
    ref = attention_ref(qf, kf, vf, softcap=CAP, **kw)
    ref.backward(dy.float())
    with torch.no_grad():
        plain = attention_ref(qf, kf, vf, **kw)
    gap = (plain - ref).abs().max().item()
    print(f"capped vs uncapped reference: forward differs by {gap:.3g}")
    assert gap > 0.1, "the cap is meant to bite on these inputs"
    _check_fwd(o, ref)
    _check_grad("dq", q.grad, qf.grad)
    _check_grad("dk", k.grad, kf.grad)
    _check_grad("dv", v.grad, vf.grad)


def test_capped_kv_cache_shape_forward(ext):
    """5 query rows at the end of 261 keys: the causal row offset"""
    from mlx_cuda_distributed_pretraining_amd.ops import attention_ref, flash_attention

    q, k, v, _ = _inputs(1, 5, 261, 4, 2, 64)
    o = flash_attention(q, k, v, causal=True, softcap=CAP)
    ref = attention_ref(q.float(), k.float(), v.float(), causal=True, softcap=CAP)
    plain = attention_ref(q.float(), k.float(), v.float(), causal=True)
    assert (plain - ref).abs().max().item() > 0.1
    _check_fwd(o, ref)


def test_capped_merged_equals_split_bit_for_bit(ext):
    B, S, Hq, Hkv, D = 1, 300, 2, 2, 128
    q, k, v, dy = _inputs(B, S, S, Hq, Hkv, D)
    scale = 1.0 / math.sqrt(D)
    o, lse = ext.attn_cap_fwd(q, k, v, scale, MOD_CAUSAL, 0, CAP)
    merged = ext.attn_cap_bwd(q, k, v, o, dy, lse, scale, MOD_CAUSAL, 0, CAP)
    split = ext.attn_cap_bwd_split(q, k, v, o, dy, lse, scale, MOD_CAUSAL, 0, CAP)
    for name, a, b in zip(("dq", "dk", "dv"), merged, split):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, b), f"{name}: merged and split differ"
    assert float(merged[1].abs().max()) > 0 and float(merged[2].abs().max()) > 0


@pytest.mark.parametrize("shape", [(1, 300, 2, 2, 128), (2, 512, 4, 2, 64)])
def test_uncapped_path_is_unchanged(ext, shape):
    """softcap=None calls what it called before: the same bits as the direct
    attn_fwd / attn_bwd calls, o and gradients"""
    from mlx_cuda_distributed_pretraining_amd.ops import flash_attention

    B, S, Hq, Hkv, D = shape
    q, k, v, dy = _inputs(B, S, S, Hq, Hkv, D)
    for t in (q, k, v):
        t.requires_grad_(True)
    o = flash_attention(q, k, v, causal=True, softcap=None)
    o.backward(dy)
    scale = 1.0 / math.sqrt(D)
    none = torch.empty(0, dtype=torch.float32, device=dev())
    with torch.no_grad():
        o2, lse = ext.attn_fwd(q, k, v, scale, MOD_CAUSAL, 0, none)
        dq, dk, dv = ext.attn_bwd(q, k, v, o2, dy, lse, scale, MOD_CAUSAL, 0, none)
    assert torch.equal(o, o2)
    assert torch.equal(q.grad, dq) and torch.equal(k.grad, dk) and torch.equal(v.grad, dv)


def test_extreme_inputs_stay_finite_and_lse_is_bounded(ext):
    """q x 100: every score saturates at +-c. With |t| <= c, row i (i + 1 kept
    keys) has log(i + 1) - c <= lse <= log(i + 1) + c; the slack of 1e-3 is far
    above fp32 rounding and far below any real violation."""
    B, S, Hq, Hkv, D = 1, 300, 2, 2, 64
    q, k, v, dy = _inputs(B, S, S, Hq, Hkv, D, qmult=100.0)
    scale = 1.0 / math.sqrt(D)
    o, lse = ext.attn_cap_fwd(q, k, v, scale, MOD_CAUSAL, 0, CAP)
    grads = ext.attn_cap_bwd(q, k, v, o, dy, lse, scale, MOD_CAUSAL, 0, CAP)
    for name, t in zip(("o", "lse", "dq", "dk", "dv"), (o, lse, *grads)):
        assert bool(torch.isfinite(t).all()), f"{name} has non-finite values"
    logn = torch.log(torch.arange(1, S + 1, device=dev(), dtype=torch.float32)).view(1, 1, S)
    lo = float((lse - (logn - CAP)).min())
    hi = float((lse - (logn + CAP)).max())
    print(f"lse - (log n - c): min {lo:.4g}; lse - (log n + c): max {hi:.4g}")
    assert lo >= -1e-3 and hi <= 1e-3


@pytest.mark.parametrize("qk_norm", [False, True])
def test_fused_nodes_stay_one_node_and_match_the_composition(ext, qk_norm):
    from mlx_cuda_distributed_pretraining_amd.ops import attention_ref
    from mlx_cuda_distributed_pretraining_amd.ops.attention import rope_flash_attention_qkv
    from mlx_cuda_distributed_pretraining_amd.ops.qk_norm import qk_norm_rope_ref
    from mlx_cuda_distributed_pretraining_amd.ops.rope import RopeTable, apply_rope

    B, S, Hq, Hkv, D = 2, 256, 4, 2, 128
    g = torch.Generator(device="cpu").manual_seed(31)
    qkv = torch.randn(B, S, (Hq + 2 * Hkv) * D, generator=g).to(dev(), torch.bfloat16)
    dy = torch.randn(B, S, Hq, D, generator=g).to(dev(), torch.bfloat16)
    wq = (1.0 + 0.1 * torch.randn(D, generator=g)).to(dev(), torch.bfloat16)
    wk = (1.0 + 0.1 * torch.randn(D, generator=g)).to(dev(), torch.bfloat16)
    cos, sin = RopeTable(D, 10000.0).get(S, dev(), 0)
    norm_kw = dict(q_norm_weight=wq, k_norm_weight=wk) if qk_norm else {}
    qkv.requires_grad_(True)
    o = rope_flash_attention_qkv(qkv, cos, sin, Hq, Hkv, D, softcap=CAP, **norm_kw)
    want_node = "_QKNormRopeAttnQKVFnBackward" if qk_norm else "_RopeAttnQKVFnBackward"
    assert type(o.grad_fn).__name__ == want_node, type(o.grad_fn).__name__
    o.backward(dy)

    x = qkv.detach().float().requires_grad_(True)
    q, k, v = x.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    q, k, v = q.view(B, S, Hq, D), k.view(B, S, Hkv, D), v.view(B, S, Hkv, D)
    if qk_norm:
        q, k = qk_norm_rope_ref(q, k, wq.float(), wk.float(), cos, sin, 1e-5, False, 0)
    else:
        q, k = apply_rope(q, cos, sin, False, 0), apply_rope(k, cos, sin, False, 0)
    ref = attention_ref(q, k, v, causal=True, softcap=CAP)
    ref.backward(dy.float())
    with torch.no_grad():
        gap = (attention_ref(q, k, v, causal=True) - ref).abs().max().item()
    assert gap > 0.1, gap
    _check_fwd(o, ref)
    _check_grad("dqkv", qkv.grad, x.grad)


LENGTHS = (1, 255, 256, 257, 777)


@pytest.mark.parametrize("D", [64, 128])
def test_attn_decode_cap_matches_reference(ext, D):
    from mlx_cuda_distributed_pretraining_amd.ops import attention_ref

    B, Hq, Hkv, Lmax = 2, 4, 2, 1024
    g = torch.Generator(device="cpu").manual_seed(31)
    kc = torch.randn(B, Lmax, Hkv, D, generator=g).to(dev(), torch.bfloat16)
    vc = torch.randn(B, Lmax, Hkv, D, generator=g).to(dev(), torch.bfloat16)
    part = torch.empty(B, Hq, (Lmax + 255) // 256, D + 2, dtype=torch.float32, device=dev())
    scale = 1.0 / math.sqrt(D)
    for length in LENGTHS:
        q = torch.randn(B, 1, Hq, D, generator=g).to(dev(), torch.bfloat16)
        pos = torch.tensor([length - 1], dtype=torch.int32, device=dev())
        o = ext.attn_decode_cap(q, kc, vc, pos, part, scale, CAP)
        want = attention_ref(q, kc[:, :length], vc[:, :length], causal=True, softcap=CAP)
        plain = attention_ref(q, kc[:, :length], vc[:, :length], causal=True)
        err = (o.float() - want.float()).abs().max().item()
        print(f"D={D} len={length}: err {err:.4g}, capped vs uncapped "
              f"{(plain.float() - want.float()).abs().max().item():.3g}")
        assert torch.allclose(o.float(), want.float(), atol=3e-2, rtol=3e-2), (length, err)
        if length >= 255:
            assert not torch.allclose(plain.float(), want.float(), atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("D", [64, 128])
def test_attn_decode_q8_cap_matches_the_torch_mirror(ext, D):
    """the int8 cache built by the torch mirror of kv_append_q8 (per-64-element
    group scale and zero, inference/static_decode.py), dequantized for the
    reference"""
    from mlx_cuda_distributed_pretraining_amd.ops import attention_ref

    B, Hq, Hkv, Lmax = 2, 4, 2, 1024
    g = torch.Generator(device="cpu").manual_seed(31)

    def quant(t):
        x = t.float().reshape(B, Lmax, Hkv, D // 64, 64)
        lo = x.amin(-1)
        s = ((x.amax(-1) - lo) / 255.0).clamp_min(1e-8)
        codes = ((x - lo.unsqueeze(-1)) / s.unsqueeze(-1)).round().clamp(0, 255)
        deq = (codes * s.unsqueeze(-1) + lo.unsqueeze(-1)).reshape(B, Lmax, Hkv, D)
        sz = torch.stack([s, lo], dim=-1).contiguous()
        return codes.reshape(B, Lmax, Hkv, D).to(torch.uint8).contiguous(), sz, deq

    kc, ksz, kd = quant(torch.randn(B, Lmax, Hkv, D, generator=g).to(dev()))
    vc, vsz, vd = quant(torch.randn(B, Lmax, Hkv, D, generator=g).to(dev()))
    part = torch.empty(B, Hq, (Lmax + 255) // 256, D + 2, dtype=torch.float32, device=dev())
    scale = 1.0 / math.sqrt(D)
    for length in LENGTHS:
        q = torch.randn(B, 1, Hq, D, generator=g).to(dev(), torch.bfloat16)
        pos = torch.tensor([length - 1], dtype=torch.int32, device=dev())
        o = ext.attn_decode_q8_cap(q, kc, ksz.view(B, -1), vc, vsz.view(B, -1), pos, part,
                                   scale, CAP)
        want = attention_ref(q.float(), kd[:, :length], vd[:, :length], causal=True, softcap=CAP)
        plain = attention_ref(q.float(), kd[:, :length], vd[:, :length], causal=True)
        err = (o.float() - want).abs().max().item()
        print(f"q8 D={D} len={length}: err {err:.4g}")
        assert torch.allclose(o.float(), want, atol=3e-2, rtol=3e-2), (length, err)
        if length >= 255:
            assert not torch.allclose(plain, want, atol=3e-2, rtol=3e-2)


# ----------------------------------- model -----------------------------------
@functools.lru_cache(maxsize=None)
def _capped_model():
    """tiny bf16 model with attention.logit_softcap = 2; the q and k rows of
    the fused projection are scaled up so the scores reach past the cap"""
    from mlx_cuda_distributed_pretraining_amd.models.llama import Model, ModelArgs

    torch.manual_seed(0)
    args = ModelArgs(hidden_size=256, intermediate_size=512, num_layers=2, num_heads=4,
                     num_kv_heads=2, head_dim=64, vocab_size=503, attn_logit_softcap=CAP)
    model = Model(args).to(dev(), torch.bfloat16)
    with torch.no_grad():
        for layer in model.layers:
            layer.attention.wqkv.weight[: (4 + 2) * 64] *= 12.0
    return model


def test_model_training_forward_matches_the_simple_path(ext):
    from mlx_cuda_distributed_pretraining_amd.ops.cross_entropy import fused_cross_entropy

    model = _capped_model().train()
    x = torch.randint(0, 503, (2, 129), generator=torch.Generator().manual_seed(31)).to(dev())

    def run(atype, cap):
        model.args.attention_type, model.args.attn_logit_softcap = atype, cap
        model.zero_grad(set_to_none=True)
        logits = model(x[:, :-1])
        loss, _ = fused_cross_entropy(logits.reshape(-1, 503).contiguous(),
                                      x[:, 1:].reshape(-1), ignore_index=-1)
        loss.backward()
        return float(loss.detach()), {n: p.grad.float().clone()
                                      for n, p in model.named_parameters()}

    try:
        loss, grads = run("flash", CAP)
        loss_ref, grads_ref = run("simple", CAP)
        loss_plain, _ = run("simple", None)
    finally:
        model.args.attention_type, model.args.attn_logit_softcap = "flash", CAP
    print(f"loss {loss:.5f}, simple {loss_ref:.5f}, uncapped simple {loss_plain:.5f}")
    assert abs(loss_ref - loss_plain) > 0.05, "the cap is meant to matter for this model"
    assert abs(loss - loss_ref) < 3e-2
    for n, gr in grads_ref.items():
        _check_grad(n, grads[n], gr)


def test_model_static_decode_equals_eager_cached_generation(ext):
    from mlx_cuda_distributed_pretraining_amd.inference.generate import generate_step
    from mlx_cuda_distributed_pretraining_amd.inference.static_decode import GraphDecoder

    model = _capped_model().eval()
    prompt = [3, 17, 41, 5, 88, 23, 9, 101, 250, 77]
    n = 8
    oracle = list(generate_step(model, prompt, max_tokens=n))
    dec = GraphDecoder(model, batch=1, max_len=256)
    dec.prefill(torch.tensor([prompt], device=dev()))
    dec.capture()
    assert dec.graph is not None
    got = dec.decode(n)[0].tolist()
    assert got == oracle, (got, oracle)


# -------------------------------- error paths --------------------------------
def test_cap_refuses_doc_prefix_and_alibi(ext):
    from mlx_cuda_distributed_pretraining_amd.ops import flash_attention

    q, k, v, _ = _inputs(1, 64, 64, 2, 2, 64)
    doc = torch.zeros(1, 64, dtype=torch.int32, device=dev())
    for kw in (dict(doc_start=doc), dict(prefix_len=16), dict(alibi_slopes=2)):
        with pytest.raises(ValueError, match="softcap"):
            flash_attention(q, k, v, softcap=CAP, **kw)


def test_bindings_reject_a_bad_cap(ext):
    q, k, v, dy = _inputs(1, 64, 64, 2, 2, 64)
    scale = 1.0 / math.sqrt(64)
    o, lse = ext.attn_cap_fwd(q, k, v, scale, MOD_CAUSAL, 0, CAP)
    kc = torch.zeros(1, 256, 2, 64, device=dev(), dtype=torch.bfloat16)
    part = torch.empty(1, 2, 1, 66, dtype=torch.float32, device=dev())
    pos = torch.zeros(1, dtype=torch.int32, device=dev())
    kc8 = torch.zeros(1, 256, 2, 64, device=dev(), dtype=torch.uint8)
    sz = torch.zeros(1, 256 * 2 * 2, device=dev())
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        calls = [
            lambda: ext.attn_cap_fwd(q, k, v, scale, MOD_CAUSAL, 0, bad),
            lambda: ext.attn_cap_bwd(q, k, v, o, dy, lse, scale, MOD_CAUSAL, 0, bad),
            lambda: ext.attn_cap_bwd_split(q, k, v, o, dy, lse, scale, MOD_CAUSAL, 0, bad),
            lambda: ext.attn_decode_cap(q[:, :1], kc, kc, pos, part, scale, bad),
            lambda: ext.attn_decode_q8_cap(q[:, :1], kc8, sz, kc8, sz, pos, part, scale, bad),
        ]
        for i, call in enumerate(calls):
            with pytest.raises(RuntimeError, match="cap must be finite"):
                call()
    # mods without a capped instantiation are refused on the host too
    for mod in (MOD_PREFIX_LM, MOD_ALIBI):
        with pytest.raises(RuntimeError, match="soft-capping"):
            ext.attn_cap_fwd(q, k, v, scale, mod, 0, CAP)
