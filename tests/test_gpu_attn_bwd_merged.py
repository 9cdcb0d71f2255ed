"""Merged dK+dV attention backward kernel (csrc/attn_bwd.hip) on a real MI355X.

Part 1: the merged path (attn_bwd, the default at D=128) against
the split dK and dV kernels (attn_bwd_split) on the same inputs — bit-identical,
since both form p and dS by the same code and accumulate in the same order.
Part 2: the merged results against the fp32 attention_ref backward, under the
criterion of test_attn_bwd_gpu.

Shapes are the smallest that reach every path of a 256-row, 8-wave kv block:
S=328 has two kv blocks, the second partial with waves that hold no valid row,
a ragged last q tile and a GQA group of 2; S=520 (group of 1) has three kv
blocks, the first spanning interior and diagonal q tiles, and odd iteration
counts (17 q tiles for the first block).
D=64 stays on the split kernels, so it has no case here.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128
# name -> (B, S, Hq, Hkv, flash-attention keywords)
CASES = {
    "none": (2, 328, 4, 2, dict(causal=False)),
    "causal": (2, 328, 4, 2, dict(causal=True)),
    "window64": (2, 328, 4, 2, dict(causal=True, window=64)),
    "prefix100": (2, 328, 4, 2, dict(causal=True, prefix_len=100)),
    "alibi": (2, 328, 4, 2, dict(causal=True, alibi=True)),
    "causal_3blocks": (1, 520, 2, 2, dict(causal=True)),
}


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    from mlx_cuda_distributed_pretraining_amd.ops import require_ext

    return require_ext()


_runs = {}


def run_case(ext, name):
    """Inputs, forward, merged / split / fp32-reference gradients of one case;
    computed once and shared by the tests (nothing below modifies them)."""
    if name in _runs:
        return _runs[name]
    from mlx_cuda_distributed_pretraining_amd.ops.attention import _Mask, attention_ref

    B, S, Hq, Hkv, kw = CASES[name]
    torch.manual_seed(0)
    mk = lambda *s: torch.randn(*s, device=dev(), dtype=torch.bfloat16)
    q, k, v = mk(B, S, Hq, D), mk(B, S, Hkv, D), mk(B, S, Hkv, D)
    causal, window, prefix_len = kw.get("causal", True), kw.get("window"), kw.get("prefix_len")
    alibi = None
    if kw.get("alibi"):
        alibi = torch.tensor([2 ** (-(i + 1)) for i in range(Hq)], device=dev())
    mask = _Mask.build(causal, window, prefix_len, alibi, None, None, B, S, S, Hq, dev())
    mod, modarg, slopes = mask.mod, mask.modarg, mask.slopes
    scale = 1.0 / math.sqrt(D)
    o, lse = ext.attn_fwd(q, k, v, scale, mod, modarg, slopes)
    dy = torch.randn_like(o)
    args = (q, k, v, o, dy, lse, scale, mod, modarg, slopes)
    merged = ext.attn_bwd(*args)
    split = ext.attn_bwd_split(*args)

    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    ref = attention_ref(qf, kf, vf, causal=causal, scale=scale, window=window,
                        prefix_len=prefix_len, alibi_slopes=alibi)
    ref.backward(dy.float())
    _runs[name] = dict(args=args, merged=merged, split=split,
                       ref=(qf.grad, kf.grad, vf.grad))
    return _runs[name]


@pytest.mark.parametrize("name", list(CASES))
def test_merged_equals_split(ext, name):
    r = run_case(ext, name)
    for label, got, want in zip(("dq", "dk", "dv"), r["merged"], r["split"]):
        assert torch.isfinite(want.float()).all(), f"{label} split path not finite ({name})"
        assert torch.equal(got, want), (
            f"{label} merged != split ({name}): "
            f"{(got.float() - want.float()).abs().max().item()} max abs diff, "
            f"{(got != want).sum().item()} elements")


@pytest.mark.parametrize("name", list(CASES))
def test_merged_matches_fp32_reference(ext, name):
    r = run_case(ext, name)
    for label, got, want in zip(("dq", "dk", "dv"), r["merged"], r["ref"]):
        err = (got.float() - want).abs().max().item()
        ref_mag = want.abs().max().item()
        assert err < 0.05 * max(ref_mag, 1.0), \
            f"{label} max err {err} (ref mag {ref_mag}) case {name}"


def test_merged_out_views_of_fused_buffer(ext):
    """attn_bwd writing dq, dk and dv as row-strided views of one fused
    [B, S, (Hq + 2 Hkv) D] buffer: same bits as the split path, and nothing
    outside the views' own columns is disturbed."""
    r = run_case(ext, "causal")
    B, S, Hq, Hkv, _ = CASES["causal"]
    dqkv = torch.zeros(B, S, (Hq + 2 * Hkv) * D, device=dev(), dtype=torch.bfloat16)
    dq_t = dqkv[..., : Hq * D].view(B, S, Hq, D)
    dk_t = dqkv[..., Hq * D: (Hq + Hkv) * D].view(B, S, Hkv, D)
    dv_t = dqkv[..., (Hq + Hkv) * D:].view(B, S, Hkv, D)
    out = ext.attn_bwd(*r["args"], dq_t, dk_t, dv_t)
    want = torch.cat([t.reshape(B, S, -1) for t in r["split"]], dim=-1)
    assert torch.equal(dqkv, want), (dqkv.float() - want.float()).abs().max().item()
    for got, view in zip(out, (dq_t, dk_t, dv_t)):
        assert got.data_ptr() == view.data_ptr()
