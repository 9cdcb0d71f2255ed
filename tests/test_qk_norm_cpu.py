"""QK-norm (per-head RMSNorm over head_dim on q and k before RoPE), CPU side:
model/config plumbing, the analytical backward the HIP kernel implements,
cache/static decode, checkpoint, exporter, TP guard."""
import json
import sys
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))

from mlx_cuda_distributed_pretraining_amd.core.config import Config
from mlx_cuda_distributed_pretraining_amd.models.llama import (
    Model, ModelArgs, make_prompt_cache,
)


def tiny_args(**kw):
    defaults = dict(hidden_size=64, intermediate_size=128, num_layers=2, num_heads=4,
                    num_kv_heads=2, vocab_size=101)
    defaults.update(kw)
    return ModelArgs(**defaults)


def _randomize_norms(model, seed=5):
    """QK-norm weights away from their all-ones init, so a dropped `* w` shows."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for layer in model.layers:
            for n in (layer.attention.q_norm, layer.attention.k_norm):
                n.weight.copy_(0.5 + torch.rand(n.weight.shape, generator=g))


# ---------------------------------------------------------------------------
# the math: plain-torch composition and the analytical backward
# ---------------------------------------------------------------------------
def rope_plain(x, cos, sin, traditional, offset, conj=False):
    """RoPE in x's own dtype (ops.rope.rope_ref computes in fp32).
    x: [B,S,H,D]; cos/sin: [Smax, D/2]. conj=True is the transpose (inverse)."""
    S, D = x.shape[1], x.shape[-1]
    half = D // 2
    c = cos[offset:offset + S].to(x.dtype).view(S, 1, half)
    s = sin[offset:offset + S].to(x.dtype).view(S, 1, half)
    if conj:
        s = -s
    if traditional:
        x0, x1 = x[..., 0::2], x[..., 1::2]
        return torch.stack([x0 * c - x1 * s, x0 * s + x1 * c], dim=-1).flatten(-2)
    x0, x1 = x[..., :half], x[..., half:]
    return torch.cat([x0 * c - x1 * s, x0 * s + x1 * c], dim=-1)


def qknorm_rope_plain(x, w, cos, sin, eps, traditional, offset):
    """y = RoPE_{s+offset}(x * rsqrt(mean_d x^2 + eps) * w), in x's dtype."""
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    return rope_plain(x * r * w, cos, sin, traditional, offset)


def qknorm_rope_backward_formula(g_r, x, w, cos, sin, eps, traditional, offset):
    """The backward csrc/qknorm_rope.hip implements, as plain torch:
        g  = RoPE^T(g_r)
        dx = r*g*w - x * r^3/D * sum_d(g*w*x)
        dw = sum_rows g*x*r
    Returns (dx, dw, r) with r = rstd of shape [B,S,H]."""
    D = x.shape[-1]
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    g = rope_plain(g_r, cos, sin, traditional, offset, conj=True)
    dx = r * g * w - x * r.pow(3) / D * (g * w * x).sum(-1, keepdim=True)
    dw = (g * x * r).reshape(-1, D).sum(0)
    return dx, dw, r.squeeze(-1)


@pytest.mark.parametrize("traditional", [False, True])
@pytest.mark.parametrize("offset", [0, 5])
def test_analytical_backward_matches_autograd_f64(traditional, offset):
    from mlx_cuda_distributed_pretraining_amd.ops.rope import RopeTable

    B, S, H, D = 2, 7, 3, 16
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, S, H, D, generator=g, dtype=torch.float64, requires_grad=True)
    w = (0.5 + torch.rand(D, generator=g, dtype=torch.float64)).requires_grad_(True)
    g_r = torch.randn(B, S, H, D, generator=g, dtype=torch.float64)
    cos, sin = RopeTable(D, 10000.0).get(S, torch.device("cpu"), offset)
    cos, sin = cos.double(), sin.double()
    eps = 1e-5

    y = qknorm_rope_plain(x, w, cos, sin, eps, traditional, offset)
    dx_ref, dw_ref = torch.autograd.grad(y, [x, w], g_r)
    dx, dw, _ = qknorm_rope_backward_formula(g_r, x.detach(), w.detach(), cos, sin, eps,
                                             traditional, offset)
    assert (dx - dx_ref).abs().max().item() < 1e-9
    assert (dw - dw_ref).abs().max().item() < 1e-9


@pytest.mark.parametrize("traditional", [False, True])
def test_plain_composition_is_the_ops_composition(traditional):
    """The test-local f64-capable composition and the package's fallback
    (rms_norm_ref -> apply_rope) are the same function."""
    from mlx_cuda_distributed_pretraining_amd.ops import qk_norm_rope
    from mlx_cuda_distributed_pretraining_amd.ops.rope import RopeTable

    B, S, Hq, Hkv, D = 2, 9, 4, 2, 16
    g = torch.Generator().manual_seed(12)
    qkv = torch.randn(B, S, (Hq + 2 * Hkv) * D, generator=g)
    q, k, _ = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    q, k = q.view(B, S, Hq, D), k.view(B, S, Hkv, D)
    wq, wk = 0.5 + torch.rand(D, generator=g), 0.5 + torch.rand(D, generator=g)
    cos, sin = RopeTable(D, 10000.0).get(S, torch.device("cpu"), 3)
    qo, ko = qk_norm_rope(q, k, wq, wk, cos, sin, 1e-5, traditional=traditional, offset=3)
    assert torch.allclose(qo, qknorm_rope_plain(q, wq, cos, sin, 1e-5, traditional, 3),
                          atol=1e-6)
    assert torch.allclose(ko, qknorm_rope_plain(k, wk, cos, sin, 1e-5, traditional, 3),
                          atol=1e-6)


# ---------------------------------------------------------------------------
# model / config
# ---------------------------------------------------------------------------
def test_qk_norm_model_builds_with_no_decay_norm_params():
    from mlx_cuda_distributed_pretraining_amd.optim.enhanced import (
        _is_no_decay, split_decay_groups,
    )

    m = Model(tiny_args(qk_norm=True))
    hd = m.args.head_dim
    params = dict(m.named_parameters())
    for i in range(len(m.layers)):
        for n in ("q_norm", "k_norm"):
            name = f"layers.{i}.attention.{n}.weight"
            assert name in params, name
            assert params[name].shape == (hd,)
            assert torch.equal(params[name], torch.ones(hd))
            assert _is_no_decay(name, params[name])
    _, no_decay = split_decay_groups(m.named_parameters())
    ids = {id(p) for p in no_decay}
    assert all(id(l.attention.q_norm.weight) in ids and id(l.attention.k_norm.weight) in ids
               for l in m.layers)
    logits = m(torch.randint(0, 101, (2, 16)))
    assert logits.shape == (2, 16, 101)


def test_flag_off_state_dict_keys_unchanged():
    m = Model(tiny_args(num_layers=1))
    assert sorted(m.state_dict().keys()) == sorted([
        "tok_embeddings.weight",
        "layers.0.attention.wqkv.weight",
        "layers.0.attention.wo.weight",
        "layers.0.attention_norm.weight",
        "layers.0.mlp.w_gate_up.weight",
        "layers.0.mlp.w_down.weight",
        "layers.0.mlp_norm.weight",
        "norm.weight",
    ])
    assert m.args.qk_norm is False


def test_config_flag_and_shipped_config():
    cfg = Config.from_yaml(REPO / "configs" / "model-config-400m-muon-qknorm.yaml")
    base = Config.from_yaml(REPO / "configs" / "model-config-400m-muon.yaml")
    assert ModelArgs.from_config(cfg.model, 32000).qk_norm is True
    assert ModelArgs.from_config(base.model, 32000).qk_norm is False
    # the child sets the flag and nothing else
    a, b = cfg.to_dict(), base.to_dict()
    a["model"]["attention"].pop("qk_norm")
    assert a == b


def test_qk_norm_changes_the_function_and_trains_its_weights():
    torch.manual_seed(0)
    m = Model(tiny_args(qk_norm=True))
    _randomize_norms(m)
    m.train()
    x = torch.randint(0, 101, (2, 12))
    loss = torch.nn.functional.cross_entropy(m(x).reshape(-1, 101), x.reshape(-1))
    loss.backward()
    for layer in m.layers:
        for n in (layer.attention.q_norm, layer.attention.k_norm):
            assert n.weight.grad is not None and n.weight.grad.abs().max() > 0


@pytest.mark.parametrize("atype", ["flash", "simple"])
def test_qk_norm_kv_cache_decode_matches_full_forward(atype):
    torch.manual_seed(0)
    m = Model(tiny_args(qk_norm=True, attention_type=atype))
    _randomize_norms(m)
    m.eval()
    x = torch.randint(0, 101, (1, 12))
    with torch.no_grad():
        full = m(x)
        cache = make_prompt_cache(m)
        m(x[:, :8], cache=cache)  # prefill 8, then decode 4 one at a time
        outs = [m(x[:, t:t + 1], cache=cache) for t in range(8, 12)]
        stepped = torch.cat(outs, dim=1)
    assert torch.allclose(full[:, 8:], stepped, atol=1e-4)


def test_qk_norm_flex_mask_path_matches_fused_causal():
    torch.manual_seed(0)
    m = Model(tiny_args(qk_norm=True))
    _randomize_norms(m)
    m.eval()
    x = torch.randint(0, 101, (2, 10))
    with torch.no_grad():
        want = m(x)
        m.set_flex_mask(lambda b, h, q, k: q >= k)
        got = m(x)
    assert torch.allclose(got, want, atol=1e-4)


@pytest.mark.parametrize("kv_bits", [None, 8])
def test_qk_norm_static_decode_matches_generate_step(kv_bits):
    from mlx_cuda_distributed_pretraining_amd.inference.generate import generate_step
    from mlx_cuda_distributed_pretraining_amd.inference.static_decode import GraphDecoder

    torch.manual_seed(0)
    hd = 64 if kv_bits else 16
    m = Model(ModelArgs(hidden_size=64, intermediate_size=128, num_layers=2, num_heads=4,
                        num_kv_heads=2, head_dim=hd, vocab_size=97, qk_norm=True)).eval()
    _randomize_norms(m)
    prompt = [3, 17, 41, 5, 88, 23, 9]
    n = 12
    oracle = list(generate_step(m, prompt, max_tokens=n))  # greedy default
    dec = GraphDecoder(m, batch=1, max_len=64, kv_bits=kv_bits)
    dec.prefill(torch.tensor([prompt]))
    got = dec.decode(n)[0].tolist()
    if kv_bits is None:
        assert got == oracle, (got, oracle)
    else:
        # int8 KV perturbs logits slightly (bound of test_int8_kv_cpu_reference_path)
        assert all(0 <= t < 97 for t in got)
        agree = sum(a == b for a, b in zip(got, oracle)) / n
        assert agree >= 0.6, (agree, got, oracle)


def test_qk_norm_checkpoint_roundtrip(tmp_path):
    from mlx_cuda_distributed_pretraining_amd.core.checkpoint import (
        load_checkpoint, save_checkpoint,
    )

    torch.manual_seed(0)
    m = Model(tiny_args(qk_norm=True))
    _randomize_norms(m)
    base = str(tmp_path / "step_1")
    save_checkpoint(base, m, None, {"step": 1})
    m2 = Model(tiny_args(qk_norm=True))
    load_checkpoint(base, m2, strict=True)
    for l1, l2 in zip(m.layers, m2.layers):
        assert torch.equal(l1.attention.q_norm.weight, l2.attention.q_norm.weight)
        assert torch.equal(l1.attention.k_norm.weight, l2.attention.k_norm.weight)
        assert not torch.equal(l2.attention.q_norm.weight, torch.ones(m.args.head_dim))


# ---------------------------------------------------------------------------
# exporter / TP
# ---------------------------------------------------------------------------
def test_exporter_maps_norm_weights_and_emits_qwen3():
    from convert_to_mlx_lm import fused_to_hf_state, hf_config_from

    args = tiny_args(num_layers=1, qk_norm=True, max_position_embeddings=128)
    m = Model(args)
    _randomize_norms(m)
    hf = fused_to_hf_state(m.state_dict(), args)
    attn = m.layers[0].attention
    assert torch.equal(hf["model.layers.0.self_attn.q_norm.weight"], attn.q_norm.weight)
    assert torch.equal(hf["model.layers.0.self_attn.k_norm.weight"], attn.k_norm.weight)
    cfg = hf_config_from(None, args)
    assert cfg["model_type"] == "qwen3"
    assert cfg["architectures"] == ["Qwen3ForCausalLM"]
    assert cfg["head_dim"] == args.head_dim


def test_exporter_flag_off_config_unchanged():
    from convert_to_mlx_lm import fused_to_hf_state, hf_config_from

    args = tiny_args(num_layers=1, max_position_embeddings=128)
    cfg = hf_config_from(None, args)
    want = {
        "architectures": ["LlamaForCausalLM"],
        "model_type": "llama",
        "hidden_size": 64,
        "intermediate_size": 128,
        "num_hidden_layers": 1,
        "num_attention_heads": 4,
        "num_key_value_heads": 2,
        "head_dim": 16,
        "vocab_size": 101,
        "max_position_embeddings": 128,
        "rms_norm_eps": 1e-5,
        "rope_theta": 10000.0,
        "tie_word_embeddings": True,
        "hidden_act": "silu",
        "attention_bias": False,
        "mlp_bias": False,
        "bos_token_id": 1,
        "eos_token_id": 2,
        "pad_token_id": 0,
        "torch_dtype": "bfloat16",
    }
    assert cfg == want
    assert json.dumps(cfg, indent=2) == json.dumps(want, indent=2)  # same key order too
    hf = fused_to_hf_state(Model(args).state_dict(), args)
    assert not any("q_norm" in k or "k_norm" in k for k in hf)


def test_tensor_parallel_with_qk_norm_is_refused():
    from mlx_cuda_distributed_pretraining_amd.parallel.tp import apply_tensor_parallel

    m = Model(tiny_args(qk_norm=True))
    with pytest.raises(NotImplementedError, match="qk_norm"):
        apply_tensor_parallel(m, 0, 2)
    with pytest.raises(NotImplementedError, match="qk_norm"):
        apply_tensor_parallel(m, 0, 2, sequence_parallel=True)
