"""Attention-logit soft-capping without a GPU: attention_ref(softcap=c), the
CPU path of flash_attention / rope_flash_attention_qkv, ModelArgs and the new
config, the model's three attention paths (full forward, KV cache, static
decode's eager branch), the combinations that must raise, and the exporter."""
import math
import sys
from pathlib import Path

import pytest
import torch

from mlx_cuda_distributed_pretraining_amd.core.config import Config
from mlx_cuda_distributed_pretraining_amd.models.llama import (
    Model, ModelArgs, make_prompt_cache,
)
from mlx_cuda_distributed_pretraining_amd.ops import attention_ref, flash_attention
from mlx_cuda_distributed_pretraining_amd.ops.attention import rope_flash_attention_qkv

REPO = Path(__file__).resolve().parent.parent
CAP = 2.0


def _qkv(seed, B, Sq, Skv, Hq, Hkv, D, mult=1.0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Sq, Hq, D, generator=g) * mult
    k = torch.randn(B, Skv, Hkv, D, generator=g)
    v = torch.randn(B, Skv, Hkv, D, generator=g)
    return q, k, v


@pytest.mark.parametrize("kw", [dict(causal=True), dict(causal=False),
                                dict(causal=True, window=5)])
def test_attention_ref_softcap_equals_the_score_mod_formulation(kw):
    q, k, v = _qkv(31, 2, 9, 13, 4, 2, 16, mult=3.0)
    cap_mod = lambda s, b, h, qi, ki: CAP * torch.tanh(s / CAP)  # noqa: E731
    got, lse = attention_ref(q, k, v, softcap=CAP, return_lse=True, **kw)
    want, lse_w = attention_ref(q, k, v, score_mod=cap_mod, return_lse=True, **kw)
    assert torch.equal(got, want) and torch.equal(lse, lse_w)
    plain = attention_ref(q, k, v, **kw)
    assert (got - plain).abs().max() > 0.1, "the cap must matter on these scores"
    # |t| <= c bounds the lse of a row with n kept keys by log(n) +- c
    n = torch.isfinite(lse).sum()  # every row has a kept key
    assert n == lse.numel() and float(lse.max()) <= math.log(13) + CAP + 1e-5


def test_cpu_flash_attention_softcap_gradients_match_autograd():
    q, k, v = _qkv(31, 1, 12, 12, 4, 2, 16, mult=3.0)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    dy = torch.randn(1, 12, 4, 16, generator=torch.Generator().manual_seed(5))
    flash_attention(*leaves, causal=True, softcap=CAP).backward(dy)
    ref = [t.clone().requires_grad_(True) for t in (q, k, v)]
    attention_ref(*ref, causal=True, softcap=CAP).backward(dy)
    plain = [t.clone().requires_grad_(True) for t in (q, k, v)]
    attention_ref(*plain, causal=True).backward(dy)
    for a, b, c in zip(leaves, ref, plain):
        assert torch.allclose(a.grad, b.grad, rtol=1e-5, atol=1e-6)
        assert (a.grad - c.grad).abs().max() > 1e-2


def test_cpu_fused_qkv_entry_takes_softcap():
    from mlx_cuda_distributed_pretraining_amd.ops.rope import RopeTable, apply_rope

    B, S, Hq, Hkv, D = 1, 10, 4, 2, 16
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(B, S, (Hq + 2 * Hkv) * D, generator=g) * 2.0
    cos, sin = RopeTable(D, 10000.0).get(S, qkv.device, 0)
    got = rope_flash_attention_qkv(qkv, cos, sin, Hq, Hkv, D, softcap=CAP)
    q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    q = apply_rope(q.view(B, S, Hq, D), cos, sin, False, 0)
    k = apply_rope(k.view(B, S, Hkv, D), cos, sin, False, 0)
    want = attention_ref(q, k, v.view(B, S, Hkv, D), causal=True, softcap=CAP)
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("bad", [0.0, -1.0, float("inf"), float("nan")])
def test_softcap_must_be_finite_and_positive(bad):
    q, k, v = _qkv(1, 1, 4, 4, 2, 2, 16)
    with pytest.raises(ValueError, match="softcap"):
        flash_attention(q, k, v, softcap=bad)


def test_softcap_refuses_doc_prefix_and_alibi():
    q, k, v = _qkv(1, 1, 8, 8, 2, 2, 16)
    doc = torch.zeros(1, 8, dtype=torch.int32)
    for kw in (dict(doc_start=doc), dict(prefix_len=3), dict(alibi_slopes=2)):
        with pytest.raises(ValueError, match="softcap"):
            flash_attention(q, k, v, softcap=CAP, **kw)
    cos = sin = torch.zeros(8, 8)
    with pytest.raises(ValueError, match="softcap"):
        rope_flash_attention_qkv(torch.zeros(1, 8, 6 * 16), cos, sin, 2, 2, 16,
                                 softcap=CAP, doc_start=doc)


# ----------------------------------- model -----------------------------------
def _args(**kw):
    base = dict(hidden_size=64, intermediate_size=128, num_layers=2, num_heads=4,
                num_kv_heads=2, head_dim=16, vocab_size=97)
    base.update(kw)
    return ModelArgs(**base)


def _model(**kw):
    torch.manual_seed(0)
    m = Model(_args(**kw)).eval()
    # scores well past the cap: scale the fused projection's q and k rows
    a = m.args
    with torch.no_grad():
        for layer in m.layers:
            layer.attention.wqkv.weight[: (a.num_heads + a.num_kv_heads) * a.head_dim] *= 25.0
    return m


def test_model_args_validate_the_cap():
    assert _args().attn_logit_softcap is None
    assert _args(attn_logit_softcap=0).attn_logit_softcap is None
    assert _args(attn_logit_softcap=50).attn_logit_softcap == 50.0
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="attention.logit_softcap"):
            _args(attn_logit_softcap=bad)
    with pytest.raises(ValueError, match="alibi"):
        _args(attn_logit_softcap=2.0, use_alibi=True)
    with pytest.raises(ValueError, match="prefix_len"):
        _args(attn_logit_softcap=2.0, attention_prefix_len=4)
    # off: the combinations are what they were
    assert _args(attn_logit_softcap=0, use_alibi=True).use_alibi


def test_new_config_extends_the_softcap_config():
    cfg = Config.from_yaml(str(REPO / "configs" / "model-config-400m-muon-qknorm-softcap2.yaml"))
    base = Config.from_yaml(str(REPO / "configs" / "model-config-400m-muon-qknorm-softcap.yaml"))
    assert cfg.model.attention["logit_softcap"] == 50.0
    assert "logit_softcap" not in base.model.attention
    assert {k: v for k, v in cfg.model.attention.items() if k != "logit_softcap"} == \
        base.model.attention
    assert cfg.model.misc == base.model.misc and cfg.model.dimensions == base.model.dimensions
    args = ModelArgs.from_config(cfg.model, 32000)
    assert args.attn_logit_softcap == 50.0 and args.logit_softcap == 30.0 and args.qk_norm
    assert ModelArgs.from_config(base.model, 32000).attn_logit_softcap is None


@pytest.mark.parametrize("atype", ["flash", "simple"])
def test_capped_model_differs_from_the_uncapped_one(atype):
    x = torch.randint(0, 97, (2, 11), generator=torch.Generator().manual_seed(2))
    capped, plain = _model(attn_logit_softcap=CAP, attention_type=atype), _model(
        attention_type=atype)
    for (n, a), (_, b) in zip(capped.state_dict().items(), plain.state_dict().items()):
        assert torch.equal(a, b), n
    with torch.no_grad():
        lc, lp = capped(x), plain(x)
    assert (lc - lp).abs().max() > 1e-2
    # the two attention types agree on the capped model
    with torch.no_grad():
        other = _model(attn_logit_softcap=CAP,
                       attention_type="simple" if atype == "flash" else "flash")(x)
    assert torch.allclose(lc, other, rtol=1e-4, atol=1e-5)


def test_cached_generation_equals_the_full_forward_on_a_capped_model():
    m = _model(attn_logit_softcap=CAP)
    x = torch.randint(0, 97, (1, 9), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        full = m(x)
        cache = make_prompt_cache(m)
        first = m(x[:, :5], cache=cache)
        rest = [m(x[:, i : i + 1], cache=cache) for i in range(5, 9)]
    got = torch.cat([first] + rest, dim=1)
    assert torch.allclose(got, full, rtol=1e-4, atol=1e-5)
    with torch.no_grad():
        assert (full - _model()(x)).abs().max() > 1e-2


@pytest.mark.parametrize("kv_bits", [None, 8])
def test_static_decode_eager_branch_equals_the_cached_path(kv_bits):
    from mlx_cuda_distributed_pretraining_amd.inference.generate import generate_step
    from mlx_cuda_distributed_pretraining_amd.inference.static_decode import GraphDecoder

    m = _model(attn_logit_softcap=CAP, head_dim=64, hidden_size=128)
    prompt = [1, 2, 3, 4, 5]
    dec = GraphDecoder(m, batch=1, max_len=64, kv_bits=kv_bits)
    dec.prefill(torch.tensor([prompt]))
    got = dec.decode(6)[0].tolist()
    if kv_bits is None:
        assert got == list(generate_step(m, prompt, max_tokens=6))
    # the eager branch really caps: its attention output differs from the
    # uncapped one on the same cache
    cache = dec.state.layers[0]
    attn = m.layers[0].attention
    qkv = torch.randn(1, 1, (4 + 2 * 2) * 64, generator=torch.Generator().manual_seed(9)) * 8
    pos = dec.state.pos.clone()
    o_cap = cache.attend(attn, qkv.clone())
    dec.state.pos.copy_(pos)
    attn.args.attn_logit_softcap = None
    try:
        o_raw = cache.attend(attn, qkv.clone())
    finally:
        attn.args.attn_logit_softcap = CAP
    assert (o_cap - o_raw).abs().max() > 1e-3


def test_flex_mask_and_doc_mask_raise_on_a_capped_model():
    m = _model(attn_logit_softcap=CAP)
    with pytest.raises(ValueError, match="set_flex_mask"):
        m.set_flex_mask(lambda b, h, qi, ki: ki <= qi)
    m.set_flex_mask(None)  # clearing stays allowed
    x = torch.randint(0, 97, (1, 8), generator=torch.Generator().manual_seed(4))
    doc = torch.zeros(1, 8, dtype=torch.int32)
    with pytest.raises(ValueError, match="logit_softcap"):
        m(x, doc_start=doc)
    _model().set_flex_mask(lambda b, h, qi, ki: ki <= qi)  # uncapped: as before


def test_tp_sharding_needs_no_change_for_the_cap():
    """The cap acts per score and per head, so attention over a shard of the
    heads equals the shard of attention over all of them."""
    q, k, v = _qkv(31, 1, 10, 10, 4, 2, 16, mult=3.0)
    whole = attention_ref(q, k, v, causal=True, softcap=CAP)
    for r in range(2):
        part = attention_ref(q[:, :, 2 * r : 2 * r + 2], k[:, :, r : r + 1], v[:, :, r : r + 1],
                             causal=True, softcap=CAP)
        assert torch.equal(part, whole[:, :, 2 * r : 2 * r + 2])


def test_exporter_refuses_a_model_with_capped_attention():
    sys.path.insert(0, str(REPO / "tools"))
    import convert_to_mlx_lm as conv

    cfg = Config.from_yaml(str(REPO / "configs" / "model-config-sample.yaml"))
    cfg.model.attention = dict(cfg.model.attention or {}, logit_softcap=50.0)
    args = ModelArgs.from_config(cfg.model, 259)
    assert args.attn_logit_softcap == 50.0
    with pytest.raises(NotImplementedError, match="attention.logit_softcap"):
        conv.hf_config_from(cfg, args)
    cfg.model.attention["logit_softcap"] = 0
    assert conv.hf_config_from(cfg, ModelArgs.from_config(cfg.model, 259))
