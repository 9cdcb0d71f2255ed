"""Document-masked attention for packed sequences, CPU side: document_bounds,
the attention_ref oracle, packing invariance of a whole model, gradient
checkpointing, the trainer flag and the error paths."""
from pathlib import Path

import pytest
import torch

from mlx_cuda_distributed_pretraining_amd.models.llama import (
    Model, ModelArgs, make_prompt_cache,
)
from mlx_cuda_distributed_pretraining_amd.ops import attention_ref, flash_attention
from mlx_cuda_distributed_pretraining_amd.ops.attention import rope_flash_attention_qkv

REPO = Path(__file__).resolve().parents[1]
BOS, EOS = 7, 9


def _bounds(rows, **kw):
    from mlx_cuda_distributed_pretraining_amd.ops.attention import document_bounds

    tokens = torch.tensor(rows, dtype=torch.long)
    start, end = document_bounds(tokens, **kw)
    for t in (start, end):
        assert t.dtype == torch.int32 and t.device == tokens.device
        assert tuple(t.shape) == tuple(tokens.shape)
    return start.tolist(), end.tolist()


def test_document_bounds_bos_only():
    # BOS at column 0, mid-row, and at the last column
    start, end = _bounds([[BOS, 1, 2, BOS, 3, 4, 5, BOS]], bos_id=BOS)
    assert start == [[0, 0, 0, 3, 3, 3, 3, 7]]
    assert end == [[3, 3, 3, 7, 7, 7, 7, 8]]


def test_document_bounds_eos_only():
    # a document starts right after every EOS; an EOS in the last column
    # opens nothing
    start, end = _bounds([[1, 2, EOS, 3, EOS, 4, 5, EOS]], eos_id=EOS)
    assert start == [[0, 0, 0, 3, 3, 5, 5, 5]]
    assert end == [[3, 3, 3, 5, 5, 8, 8, 8]]


def test_document_bounds_bos_and_eos_pair_opens_one_document():
    start, end = _bounds([[BOS, 1, EOS, BOS, 2, 3, EOS, BOS]], bos_id=BOS, eos_id=EOS)
    assert start == [[0, 0, 0, 3, 3, 3, 3, 7]]
    assert end == [[3, 3, 3, 7, 7, 7, 7, 8]]


def test_document_bounds_adjacent_bos_one_token_document():
    start, end = _bounds([[1, BOS, BOS, 2, 3]], bos_id=BOS)
    assert start == [[0, 1, 2, 2, 2]]
    assert end == [[1, 2, 5, 5, 5]]


def test_document_bounds_no_boundary_and_per_row():
    # row 0 has no boundary at all; row 1 differs: nothing leaks across rows
    start, end = _bounds([[1, 2, 3, 4], [1, BOS, 3, 4]], bos_id=BOS, eos_id=EOS)
    assert start == [[0, 0, 0, 0], [0, 1, 1, 1]]
    assert end == [[4, 4, 4, 4], [1, 4, 4, 4]]


def _starts(bounds, S):
    """boundaries [0, a, b, ...] -> doc_start row of length S"""
    row = torch.zeros(S, dtype=torch.int32)
    for lo in bounds:
        row[lo:] = lo
    return row


def test_attention_ref_doc_start_equals_per_document_causal():
    B, S, Hq, Hkv, D = 2, 40, 4, 2, 16
    g = torch.Generator().manual_seed(0)
    q = torch.randn(B, S, Hq, D, generator=g)
    k = torch.randn(B, S, Hkv, D, generator=g)
    v = torch.randn(B, S, Hkv, D, generator=g)
    bounds = [[0, 7, 8, 31], [0, 20]]
    doc_start = torch.stack([_starts(b, S) for b in bounds])
    o = attention_ref(q, k, v, causal=True, doc_start=doc_start)
    for b, bs in enumerate(bounds):
        for lo, hi in zip(bs, bs[1:] + [S]):
            ref = attention_ref(q[b:b + 1, lo:hi], k[b:b + 1, lo:hi], v[b:b + 1, lo:hi],
                                causal=True)
            assert torch.allclose(o[b:b + 1, lo:hi], ref, atol=1e-5)
    # and it is a real restriction of the causal mask
    assert not torch.allclose(o, attention_ref(q, k, v, causal=True), atol=1e-2)


def _tiny_model(seed=0, **kw):
    torch.manual_seed(seed)
    args = ModelArgs(hidden_size=64, intermediate_size=128, num_layers=2, num_heads=4,
                     num_kv_heads=2, head_dim=16, vocab_size=97, **kw)
    return Model(args).float().eval()


PACK_BOUNDS = [0, 17, 18, 60]
PACK_S = 96


def test_model_packing_invariance():
    model = _tiny_model()
    tokens = torch.randint(0, 97, (1, PACK_S), generator=torch.Generator().manual_seed(1))
    doc_start = _starts(PACK_BOUNDS, PACK_S).view(1, PACK_S)
    with torch.no_grad():
        packed = model(tokens, doc_start=doc_start)
        plain = model(tokens)
        worst, leak = 0.0, 0.0
        for lo, hi in zip(PACK_BOUNDS, PACK_BOUNDS[1:] + [PACK_S]):
            alone = model(tokens[:, lo:hi])
            worst = max(worst, (packed[:, lo:hi] - alone).abs().max().item())
            if lo > 0:
                leak = max(leak, (plain[:, lo:hi] - alone).abs().max().item())
    print(f"packed vs alone {worst:.3g}; plain causal vs alone {leak:.3g}")
    assert worst < 1e-5
    assert leak > 1e-2


def test_model_simple_attention_type_honours_doc_start():
    model = _tiny_model(attention_type="simple")
    tokens = torch.randint(0, 97, (1, PACK_S), generator=torch.Generator().manual_seed(1))
    doc_start = _starts(PACK_BOUNDS, PACK_S).view(1, PACK_S)
    with torch.no_grad():
        packed = model(tokens, doc_start=doc_start)
        alone = model(tokens[:, 60:])
    assert (packed[:, 60:] - alone).abs().max().item() < 1e-5


def test_gradient_checkpointing_keeps_the_document_mask():
    tokens = torch.randint(0, 97, (2, 49), generator=torch.Generator().manual_seed(2))
    doc_start = torch.stack([_starts([0, 11, 30], 48), _starts([0, 25], 48)])

    def run(checkpoint):
        model = _tiny_model(seed=3).train()
        if checkpoint:
            for layer in model.layers:
                layer.enable_checkpointing()
        logits = model(tokens[:, :-1], doc_start=doc_start)
        loss = torch.nn.functional.cross_entropy(
            logits.reshape(-1, 97), tokens[:, 1:].reshape(-1))
        loss.backward()
        return loss.detach(), [p.grad.clone() for p in model.parameters()]

    loss0, g0 = run(False)
    loss1, g1 = run(True)
    assert torch.allclose(loss0, loss1, atol=1e-6)
    assert len(g0) == len(g1)
    for a, b in zip(g0, g1):
        assert torch.allclose(a, b, atol=1e-6)
    # the mask reached the model at all: a plain causal loss differs
    model = _tiny_model(seed=3).train()
    plain = torch.nn.functional.cross_entropy(
        model(tokens[:, :-1]).reshape(-1, 97), tokens[:, 1:].reshape(-1))
    assert abs(float(plain.detach()) - float(loss0)) > 1e-6


def _trainer(tmp_path, name, document_mask):
    from mlx_cuda_distributed_pretraining_amd.core.config import Config
    from mlx_cuda_distributed_pretraining_amd.core.trainer import Trainer

    cfg = Config.from_yaml(str(REPO / "configs" / "model-config-sample.yaml"))
    cfg.name = name
    cfg.model.dimensions = {"hidden_size": 32, "intermediate_size": 64, "num_layers": 2}
    cfg.model.attention = {"num_heads": 2, "num_kv_heads": None, "head_dim": None,
                           "max_position_embeddings": None}
    cfg.data.preprocessing["max_context_size"] = 32
    cfg.training.hyperparameters["batch_size"] = 2
    cfg.system.device = "cpu"
    if document_mask is not None:
        cfg.data.preprocessing["document_mask"] = document_mask
    return Trainer(cfg, runs_root=str(tmp_path / "runs"))


def test_trainer_document_mask_flag(tmp_path):
    from mlx_cuda_distributed_pretraining_amd.ops.attention import document_bounds

    on = _trainer(tmp_path, "doc-on", True)
    off = _trainer(tmp_path, "doc-off", False)
    nokey = _trainer(tmp_path, "doc-nokey", None)
    bos, eos = on.tokenizer.BOS_TOKEN, on.tokenizer.EOS_TOKEN
    batch = torch.randint(0, 200, (2, 33), generator=torch.Generator().manual_seed(4))
    batch[0, 0] = bos
    batch[0, 13] = eos
    batch[0, 14] = bos  # mid-row EOS BOS pair
    batch[1, 0] = bos
    batch[1, 20] = bos  # mid-row BOS alone
    inputs, targets = batch[:, :-1], batch[:, 1:]
    with torch.no_grad():
        loss_on, _ = on.compute_loss(inputs, targets)
        loss_off, _ = off.compute_loss(inputs, targets)
        loss_nokey, _ = nokey.compute_loss(inputs, targets)
        doc_start, doc_end = document_bounds(inputs, bos_id=bos, eos_id=eos)
        assert doc_start[0].tolist() == [0] * 14 + [14] * 18
        logits = on.model(inputs, doc_start=doc_start, doc_end=doc_end)
        manual = torch.nn.functional.cross_entropy(
            logits.reshape(-1, logits.shape[-1]).float(), targets.reshape(-1),
            ignore_index=on.tokenizer.PAD_TOKEN)
    assert torch.allclose(loss_on.float(), manual, atol=1e-5)
    # Same weights, same deterministic CPU fp32 path: without an effect of the
    # mask the two losses would be bit-identical (as the last assert shows for
    # off vs no key). One fp32 ulp at a loss of ~5.6 is 4.8e-7; ask for 20.
    assert abs(float(loss_on) - float(loss_off)) > 1e-5
    assert torch.equal(loss_off, loss_nokey)  # bit-identical: the flag off changes nothing


def _qkv(S=16, Skv=None):
    g = torch.Generator().manual_seed(5)
    q = torch.randn(1, S, 2, 16, generator=g)
    k = torch.randn(1, Skv or S, 2, 16, generator=g)
    v = torch.randn(1, Skv or S, 2, 16, generator=g)
    return q, k, v


@pytest.mark.parametrize("kw", [
    {"window": 4}, {"prefix_len": 4}, {"alibi_slopes": torch.tensor([0.5, 0.25])},
    {"causal": False},
])
def test_flash_attention_doc_start_rejects_other_masks(kw):
    q, k, v = _qkv()
    doc_start = torch.zeros(1, 16, dtype=torch.int32)
    with pytest.raises(ValueError):
        flash_attention(q, k, v, doc_start=doc_start, **kw)
    qkv = torch.cat([t.reshape(1, 16, -1) for t in (q, k, v)], dim=-1)
    cos = sin = torch.zeros(16, 8)
    with pytest.raises(ValueError):
        rope_flash_attention_qkv(qkv, cos, sin, 2, 2, 16, doc_start=doc_start, **kw)


def test_flash_attention_doc_start_rejects_sq_ne_skv():
    q, k, v = _qkv(S=8, Skv=16)
    with pytest.raises(ValueError):
        flash_attention(q, k, v, doc_start=torch.zeros(1, 8, dtype=torch.int32))


def test_flash_attention_doc_start_on_cpu_matches_ref_with_grads():
    q, k, v = _qkv(S=24)
    doc_start = _starts([0, 5, 19], 24).view(1, 24)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    o = flash_attention(*leaves, doc_start=doc_start)  # doc_end derived
    o.sum().backward()
    refs = [t.clone().requires_grad_(True) for t in (q, k, v)]
    ro = attention_ref(*refs, causal=True, doc_start=doc_start)
    ro.sum().backward()
    assert torch.allclose(o, ro, atol=1e-6)
    for a, b in zip(leaves, refs):
        assert torch.allclose(a.grad, b.grad, atol=1e-5)


def test_model_doc_start_with_cache_raises():
    model = _tiny_model()
    tokens = torch.randint(0, 97, (1, 8))
    doc_start = torch.zeros(1, 8, dtype=torch.int32)
    with pytest.raises(ValueError):
        model(tokens, cache=make_prompt_cache(model), doc_start=doc_start)
    with pytest.raises(ValueError):
        model.layers[0].attention(torch.zeros(1, 8, 64), make_prompt_cache(model)[0],
                                  doc_start)


def test_model_doc_start_with_flex_mask_raises():
    model = _tiny_model()
    model.set_flex_mask(lambda b, h, qi, ki: ki <= qi)
    tokens = torch.randint(0, 97, (1, 8))
    with pytest.raises(ValueError):
        model(tokens, doc_start=torch.zeros(1, 8, dtype=torch.int32))
