"""Trainable flex attention, the parts that need no GPU: the qrange tensor of
CompiledBlockMask (the dK/dV kernels' q loop bounds), the unchanged mask
tensors beside it, the CPU gradient route of flex_attention, and
Model.set_flex_mask."""
import pytest
import torch

from mlx_cuda_distributed_pretraining_amd.models.llama import Model, ModelArgs
from mlx_cuda_distributed_pretraining_amd.ops.attention import (
    CompiledBlockMask, attention_ref, flex_attention,
)


def doc_band(b, h, qi, ki):
    return (ki <= qi) & (qi - ki < 128) & (qi // 200 == ki // 200)


def checker(b, h, qi, ki):
    return (((qi // 64) + (ki // 64)) % 2 == 0) | (ki == qi)


def causal(b, h, qi, ki):
    return ki <= qi


def _dense(mod, Q, KV):
    return mod(0, 0, torch.arange(Q).unsqueeze(1), torch.arange(KV).unsqueeze(0)).bool()


def _cdiv(a, b):
    return (a + b - 1) // b


def dead_blocks(b, h, qi, ki):
    """q rows 256..511 and kv columns 256..511 dead: one whole 256-row q block
    and one whole 256-row kv block without a live element ([0, 0] rows of range
    and qrange); partial granules elsewhere."""
    return ~((qi // 256 == 1) | (ki // 256 == 1)) & ((qi + ki) % 3 != 0)


# (300, 300): ragged granule rows (ceil(Q/32) = 10, not a multiple of 8);
# (257, 129): a one-row second q block and a ragged kv block (ceil(KV/64) = 3,
# not a multiple of 4); (33, 520): more kv blocks than q blocks
SHAPES = [(300, 300), (512, 200), (257, 129), (33, 520)]
MODS = [doc_band, checker, dead_blocks]


@pytest.mark.parametrize("Q,KV", SHAPES)
@pytest.mark.parametrize("mod", MODS, ids=lambda m: m.__name__)
def test_qrange_matches_bruteforce(mod, Q, KV):
    B, H = 1, 2
    bm = CompiledBlockMask(mod, B, H, Q, KV, device="cpu")
    keep = _dense(mod, Q, KV)
    nkpb = _cdiv(KV, 256)
    assert bm.qrange.shape == (B, H, nkpb, 2) and bm.qrange.dtype == torch.int32
    for h in range(H):
        for kb in range(nkpb):
            cols = keep[:, kb * 256:(kb + 1) * 256]
            live = [t for t in range(_cdiv(Q, 32)) if cols[t * 32:(t + 1) * 32].any()]
            want = [live[0], live[-1] + 1] if live else [0, 0]
            assert bm.qrange[0, h, kb].tolist() == want, (h, kb)


@pytest.mark.parametrize("Q,KV", SHAPES)
@pytest.mark.parametrize("mod", MODS, ids=lambda m: m.__name__)
def test_gran_bits_range_unchanged(mod, Q, KV):
    """The forward's tensors, recomputed by brute force from the dense mask."""
    bm = CompiledBlockMask(mod, 1, 2, Q, KV, device="cpu")
    keep = _dense(mod, Q, KV)
    nq32, nkv, nqpb = _cdiv(Q, 32), _cdiv(KV, 64), _cdiv(Q, 256)
    gran = torch.zeros(nq32, nkv, dtype=torch.uint8)
    for qg in range(nq32):
        for kg in range(nkv):
            blk = keep[qg * 32:(qg + 1) * 32, kg * 64:(kg + 1) * 64]
            gran[qg, kg] = 0 if not blk.any() else (2 if blk.all() else 1)
    bits = torch.zeros(Q, _cdiv(KV, 8), dtype=torch.uint8)
    for kk in range(KV):
        bits[:, kk // 8] |= keep[:, kk].to(torch.uint8) << (kk % 8)
    rng = torch.zeros(nqpb, 2, dtype=torch.int32)
    for qb in range(nqpb):
        live = gran[qb * 8:(qb + 1) * 8].any(dim=0).nonzero().flatten()
        if live.numel():
            rng[qb, 0], rng[qb, 1] = int(live.min()), int(live.max()) + 1
    for h in range(2):
        assert torch.equal(bm.gran[0, h], gran)
        assert torch.equal(bm.bits[0, h], bits)
        assert torch.equal(bm.range[0, h], rng)


def test_flex_cpu_compiled_mask_grads_match_reference():
    torch.manual_seed(0)
    B, S, H, D = 1, 40, 2, 8

    def band(b, h, qi, ki):
        return (ki <= qi) & (qi - ki < 9)

    q, k, v = (torch.randn(B, S, H, D, requires_grad=True) for _ in range(3))
    bm = CompiledBlockMask(band, B, H, S, S, device="cpu")
    dy = torch.randn(B, S, H, D)
    flex_attention(q, k, v, block_mask=bm).backward(dy)
    q2, k2, v2 = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    attention_ref(q2, k2, v2, causal=False, mask_mod=band).backward(dy)
    for got, want in ((q, q2), (k, k2), (v, v2)):
        assert got.grad is not None
        assert torch.allclose(got.grad, want.grad, atol=1e-6)


def _loss_and_grads(model, x):
    model.zero_grad(set_to_none=True)
    logits = model(x[:, :-1])
    loss = torch.nn.functional.cross_entropy(
        logits.reshape(-1, logits.shape[-1]).float(), x[:, 1:].reshape(-1))
    loss.backward()
    return loss.detach(), {n: p.grad.clone() for n, p in model.named_parameters()}


def test_set_flex_mask_causal_matches_unmasked_model():
    torch.manual_seed(0)
    args = ModelArgs(hidden_size=32, intermediate_size=64, num_layers=2,
                     num_heads=2, num_kv_heads=2, vocab_size=67)
    model = Model(args)
    x = torch.randint(0, 67, (2, 25))
    loss0, g0 = _loss_and_grads(model, x)

    model.set_flex_mask(causal)
    assert all(l.attention.flex_mask is causal for l in model.layers)
    loss1, g1 = _loss_and_grads(model, x)
    assert abs(float(loss1) - float(loss0)) < 1e-4
    for n in g0:
        assert torch.allclose(g1[n], g0[n], atol=1e-4), n

    model.set_flex_mask(None)
    assert all(l.attention.flex_mask is None for l in model.layers)
    loss3, g3 = _loss_and_grads(model, x)
    assert torch.equal(loss3, loss0)
    for n in g0:
        assert torch.equal(g3[n], g0[n]), n
