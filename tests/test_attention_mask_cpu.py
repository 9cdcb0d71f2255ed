"""The one mask description behind flash_attention and rope_flash_attention_qkv
(ops/attention.py), on the CPU route: every mask kind against attention_ref
differentiated directly, the fused-qkv entry point against the explicit
composition, and the argument errors through both public functions."""
import pytest
import torch

from mlx_cuda_distributed_pretraining_amd.ops.attention import (
    attention_ref, flash_attention, rope_flash_attention_qkv,
)
from mlx_cuda_distributed_pretraining_amd.ops.qk_norm import qk_norm_rope
from mlx_cuda_distributed_pretraining_amd.ops.rope import RopeTable, apply_rope

B, S, Hq, Hkv, D = 2, 40, 4, 2, 16


def _doc_start(starts=(0, 9, 25)):
    out = torch.zeros(B, S, dtype=torch.int32)
    for lo in starts:
        out[:, lo:] = lo
    return out


def _kinds():
    return {
        "none": dict(causal=False),
        "causal": dict(causal=True),
        "window7": dict(causal=True, window=7),
        "prefix11": dict(causal=True, prefix_len=11),
        "alibi": dict(causal=True,
                      alibi_slopes=torch.tensor([2.0 ** (-(i + 1)) for i in range(Hq)])),
        "doc": dict(causal=True, doc_start=_doc_start()),
    }


KINDS = list(_kinds())


@pytest.mark.parametrize("kind", KINDS)
def test_flash_attention_matches_attention_ref_autograd(kind):
    kw = _kinds()[kind]
    torch.manual_seed(0)
    q = torch.randn(B, S, Hq, D, requires_grad=True)
    k = torch.randn(B, S, Hkv, D, requires_grad=True)
    v = torch.randn(B, S, Hkv, D, requires_grad=True)
    o = flash_attention(q, k, v, **kw)
    dy = torch.randn_like(o)
    o.backward(dy)

    q2, k2, v2 = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o2 = attention_ref(q2, k2, v2, **kw)
    o2.backward(dy)
    assert torch.allclose(o, o2, atol=1e-5)
    assert torch.allclose(q.grad, q2.grad, atol=1e-4)
    assert torch.allclose(k.grad, k2.grad, atol=1e-4)
    assert torch.allclose(v.grad, v2.grad, atol=1e-4)


@pytest.mark.parametrize("qk_norm", [False, True], ids=["plain", "qknorm"])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_qkv_entry_equals_explicit_composition(kind, qk_norm):
    kw = _kinds()[kind]
    torch.manual_seed(1)
    cos, sin = RopeTable(D, 10000.0).get(S, torch.device("cpu"), 0)
    qkv = torch.randn(B, S, (Hq + 2 * Hkv) * D, requires_grad=True)
    wq = (0.5 + torch.rand(D)).requires_grad_(True)
    wk = (0.5 + torch.rand(D)).requires_grad_(True)
    norm_kw = dict(q_norm_weight=wq, k_norm_weight=wk, norm_eps=1e-5) if qk_norm else {}
    o = rope_flash_attention_qkv(qkv, cos, sin, Hq, Hkv, D, **kw, **norm_kw)
    dy = torch.randn_like(o)
    o.backward(dy)

    qkv2, wq2, wk2 = (t.detach().clone().requires_grad_(True) for t in (qkv, wq, wk))
    q, k, v = qkv2.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    q, k, v = q.view(B, S, Hq, D), k.view(B, S, Hkv, D), v.view(B, S, Hkv, D)
    if qk_norm:
        q, k = qk_norm_rope(q, k, wq2, wk2, cos, sin, 1e-5, False, 0)
    else:
        q, k = apply_rope(q, cos, sin, False, 0), apply_rope(k, cos, sin, False, 0)
    o2 = flash_attention(q, k, v, **kw)
    o2.backward(dy)

    assert torch.equal(o, o2)
    assert torch.equal(qkv.grad, qkv2.grad)
    if qk_norm:
        assert torch.equal(wq.grad, wq2.grad) and torch.equal(wk.grad, wk2.grad)


def _bad_mask_args():
    ds = _doc_start()
    return {
        "doc_end_without_doc_start": dict(doc_end=ds),
        "doc_plus_window": dict(doc_start=ds, window=7),
        "doc_plus_prefix": dict(doc_start=ds, prefix_len=11),
        "doc_plus_alibi": dict(doc_start=ds, alibi_slopes=torch.ones(Hq)),
        "doc_not_causal": dict(doc_start=ds, causal=False),
        "doc_start_shape": dict(doc_start=ds[:, :-1]),
        "doc_end_shape": dict(doc_start=ds, doc_end=ds[:1]),
    }


@pytest.mark.parametrize("bad", list(_bad_mask_args()))
def test_bad_mask_arguments_raise_through_both_entry_points(bad):
    kw = _bad_mask_args()[bad]
    q, k, v = torch.randn(B, S, Hq, D), torch.randn(B, S, Hkv, D), torch.randn(B, S, Hkv, D)
    with pytest.raises(ValueError):
        flash_attention(q, k, v, **kw)
    cos, sin = RopeTable(D, 10000.0).get(S, torch.device("cpu"), 0)
    qkv = torch.randn(B, S, (Hq + 2 * Hkv) * D)
    with pytest.raises(ValueError):
        rope_flash_attention_qkv(qkv, cos, sin, Hq, Hkv, D, **kw)
    with pytest.raises(ValueError):
        rope_flash_attention_qkv(qkv, cos, sin, Hq, Hkv, D, q_norm_weight=torch.ones(D),
                                 k_norm_weight=torch.ones(D), **kw)


def test_doc_mask_rejects_sq_ne_skv():
    # only flash_attention can see Sq != Skv: the fused qkv tensor has one S
    q, k, v = torch.randn(B, S, Hq, D), torch.randn(B, S + 8, Hkv, D), torch.randn(B, S + 8, Hkv, D)
    with pytest.raises(ValueError, match="training-only"):
        flash_attention(q, k, v, doc_start=_doc_start())
