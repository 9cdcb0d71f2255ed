"""Document-masked attention on a real MI355X: the MOD_DOCUMENT forward and
backward kernels (csrc/attn_fwd.hip, csrc/attn_bwd.hip) behind
flash_attention / rope_flash_attention_qkv / Model.forward(doc_start=...),
against attention_ref(doc_start=...) on fp32 leaves. Tolerances are the
project's own (tests/test_gpu_flex_train.py): forward max abs error < 3e-2,
each gradient max abs error < 0.05 * max(max|ref|, 1)."""
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


def _inputs(seed, B, S, Hq, Hkv, D):
    g = torch.Generator(device="cpu").manual_seed(seed)
    mk = lambda h: torch.randn(B, S, h, D, generator=g).to(dev(), torch.bfloat16)  # noqa: E731
    q, k, v = mk(Hq), mk(Hkv), mk(Hkv)
    dy = torch.randn(B, S, Hq, D, generator=g).to(dev(), torch.bfloat16)
    return q, k, v, dy


def _doc_start(rows, S):
    """per-row boundary lists [0, a, b, ...] -> int32 [B, S] on the GPU"""
    out = torch.zeros(len(rows), S, dtype=torch.int32)
    for b, bounds in enumerate(rows):
        for lo in bounds:
            out[b, lo:] = lo
    return out.to(dev())


def _check(name, got, want):
    assert bool(torch.isfinite(got).all()), f"{name} has non-finite values"
    err = (got.float() - want).abs().max().item()
    bound = 0.05 * max(want.abs().max().item(), 1.0)
    print(f"{name}: max abs err {err:.4g} (bound {bound:.4g})")
    assert math.isfinite(err) and err < bound, f"{name} err {err} >= {bound}"


def _compare(o, q, k, v, ref_o, qf, kf, vf):
    assert bool(torch.isfinite(o).all()), "o has non-finite values"
    err = (o.detach().float() - ref_o.detach().float()).abs().max().item()
    print(f"o: max abs err {err:.4g}")
    assert math.isfinite(err) and err < 3e-2, f"forward err {err}"
    _check("dq", q.grad, qf.grad)
    _check("dk", k.grad, kf.grad)
    _check("dv", v.grad, vf.grad)


def _leaves(*ts):
    return [t.detach().float().requires_grad_(True) for t in ts]


# name -> (B, S, Hq, Hkv, D, per-row document boundaries)
CASES = {
    # unaligned boundary; a boundary inside a 256-row block (later waves start
    # on dead tiles); a one-token document; a document that is the last
    # token; row 1 is one document
    "d64_mixed": (2, 512, 4, 2, 64, [[0, 37, 300, 301, 511], [0]]),
    # tile-aligned boundaries (the mask-free test flips exactly at a tile
    # edge), ragged last tile, q_hi and kv_lo on tile boundaries
    "d128_aligned": (1, 300, 2, 2, 128, [[0, 64, 256]]),
    # MQA; kv_lo > 0 for whole q blocks, q_hi < Sq for whole kv blocks
    "d64_mqa_long": (1, 1024, 4, 1, 64, [[0, 700]]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_doc_mask_fwd_bwd_matches_reference(ext, name):
    from mlx_cuda_distributed_pretraining_amd.ops import attention_ref, flash_attention
    from mlx_cuda_distributed_pretraining_amd.ops.attention import document_bounds

    B, S, Hq, Hkv, D, rows = CASES[name]
    q, k, v, dy = _inputs(21, B, S, Hq, Hkv, D)
    for t in (q, k, v):
        t.requires_grad_(True)
    doc_start = _doc_start(rows, S)
    # doc_end through the public builder on row 0, derived inside for the rest
    if name == "d64_mixed":
        tokens = torch.ones(B, S, dtype=torch.long, device=dev())
        for b, bounds in enumerate(rows):
            tokens[b, bounds] = 0
        ds, doc_end = document_bounds(tokens, bos_id=0)
        assert torch.equal(ds, doc_start)
        o = flash_attention(q, k, v, doc_start=doc_start, doc_end=doc_end)
    else:
        o = flash_attention(q, k, v, doc_start=doc_start)
    o.backward(dy)

    qf, kf, vf = _leaves(q, k, v)
    ref = attention_ref(qf, kf, vf, causal=True, scale=1.0 / math.sqrt(D),
                        doc_start=doc_start)
    ref.backward(dy.float())
    _compare(o, q, k, v, ref, qf, kf, vf)


@pytest.mark.parametrize("shape", [(2, 512, 4, 2, 64), (1, 300, 2, 2, 128)])
def test_single_document_matches_causal_kernels(ext, shape):
    from mlx_cuda_distributed_pretraining_amd.ops import flash_attention

    B, S, Hq, Hkv, D = shape
    q, k, v, dy = _inputs(22, B, S, Hq, Hkv, D)
    for t in (q, k, v):
        t.requires_grad_(True)
    o = flash_attention(q, k, v, doc_start=torch.zeros(B, S, dtype=torch.int32, device=dev()))
    o.backward(dy)
    q2, k2, v2 = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    o2 = flash_attention(q2, k2, v2, causal=True)
    o2.backward(dy)
    # the causal kernels' own bf16 output and gradients are the reference here
    _compare(o, q, k, v, o2, q2, k2, v2)


def test_fused_qkv_path_keeps_one_node_and_matches_composition(ext):
    from mlx_cuda_distributed_pretraining_amd.ops import attention_ref
    from mlx_cuda_distributed_pretraining_amd.ops.attention import rope_flash_attention_qkv
    from mlx_cuda_distributed_pretraining_amd.ops.rope import RopeTable, apply_rope

    B, S, Hq, Hkv, D = 2, 256, 4, 2, 128
    g = torch.Generator(device="cpu").manual_seed(23)
    cos, sin = RopeTable(D, 10000.0).get(S, dev(), 0)
    qkv = torch.randn(B, S, (Hq + 2 * Hkv) * D, generator=g).to(dev(), torch.bfloat16)
    qkv.requires_grad_(True)
    do = torch.randn(B, S, Hq, D, generator=g).to(dev(), torch.bfloat16)
    doc_start = _doc_start([[0, 100, 101], [0, 192]], S)

    o = rope_flash_attention_qkv(qkv, cos, sin, Hq, Hkv, D, doc_start=doc_start)
    assert type(o.grad_fn).__name__ == "_RopeAttnQKVFnBackward"
    o.backward(do)

    qkv2 = qkv.detach().clone().requires_grad_(True)
    q, k, v = qkv2.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    qr = apply_rope(q.view(B, S, Hq, D), cos, sin, False, 0)
    kr = apply_rope(k.view(B, S, Hkv, D), cos, sin, False, 0)
    o2 = attention_ref(qr, kr, v.view(B, S, Hkv, D), causal=True, doc_start=doc_start)
    o2.backward(do)

    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(qkv.grad).all())
    assert torch.allclose(o.detach().float(), o2.detach().float(), atol=3e-2, rtol=3e-2)
    assert torch.allclose(qkv.grad.float(), qkv2.grad.float(), atol=5e-2, rtol=5e-2), \
        (qkv.grad.float() - qkv2.grad.float()).abs().max()


def test_model_doc_start_matches_flex_mask(ext):
    """A 2-layer bf16 Model run with doc_start vs the same weights through
    set_flex_mask with the equivalent batch-dependent mask_mod. Bounds: those
    of test_model_set_flex_mask_matches_fused_causal_path (loss 1e-2, wqkv
    grads atol = rtol = 5e-2)."""
    from mlx_cuda_distributed_pretraining_amd.models.llama import Model, ModelArgs

    torch.manual_seed(0)
    args = ModelArgs(hidden_size=128, intermediate_size=256, num_layers=2,
                     num_heads=2, num_kv_heads=2, head_dim=64, vocab_size=256)
    model = Model(args).to(dev(), torch.bfloat16)
    x = torch.randint(0, 256, (2, 129), generator=torch.Generator().manual_seed(1)).to(dev())
    S = 128
    doc_start = _doc_start([[0, 45], [0, 90]], S)

    def mask_mod(b, h, qi, ki):
        b = int(b)  # CompiledBlockMask evaluates one (b, h) plane at a time
        return (ki <= qi) & (ki >= doc_start[b].view(S, 1))

    def run(**kw):
        model.zero_grad(set_to_none=True)
        logits = model(x[:, :-1], **kw)
        loss = torch.nn.functional.cross_entropy(
            logits.reshape(-1, 256).float(), x[:, 1:].reshape(-1))
        loss.backward()
        grads = [l.attention.wqkv.weight.grad.float().clone() for l in model.layers]
        return float(loss.detach()), grads

    loss0, g0 = run(doc_start=doc_start)
    plain, _ = run()
    model.set_flex_mask(mask_mod)
    loss1, g1 = run()
    print(f"loss doc {loss0:.6f} flex {loss1:.6f} plain causal {plain:.6f}")
    assert math.isfinite(loss0) and abs(loss1 - loss0) < 1e-2
    for a, b in zip(g0, g1):
        assert bool(torch.isfinite(a).all())
        assert torch.allclose(a, b, atol=5e-2, rtol=5e-2), (a - b).abs().max()


def test_host_checks_reject_bad_document_tensors(ext):
    q, k, v, _ = _inputs(24, 1, 64, 2, 2, 64)
    good = torch.zeros(1, 64, dtype=torch.int32, device=dev())
    with pytest.raises(RuntimeError):
        ext.attn_fwd_doc(q, k, v, 0.125, good.long())  # not int32
    with pytest.raises(RuntimeError):
        ext.attn_fwd_doc(q, k, v, 0.125, good[:, :32].contiguous())  # not [B, S]
    with pytest.raises(RuntimeError):
        ext.attn_fwd_doc(q, k, v, 0.125, good.cpu())  # wrong device
    with pytest.raises(RuntimeError):
        ext.attn_fwd_doc(q[:, :32].contiguous(), k, v, 0.125, good[:, :32].contiguous())  # Sq != Skv
