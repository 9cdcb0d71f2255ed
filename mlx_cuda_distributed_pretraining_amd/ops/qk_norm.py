"""Per-head QK-norm fused with RoPE.

QK-norm (OLMo-2, Qwen3, Gemma-3) is a learned RMSNorm over ``head_dim``
applied to every q and k head before the rotary embedding:

    y = RoPE_{s+offset}( x * rsqrt(mean_d x^2 + eps) * w )

The weights are ``[head_dim]`` vectors shared by all heads, one for q and one
for k. On bf16/fp32 GPU tensors with head_dim 64 or 128 this is one HIP kernel
each way (csrc/qknorm_rope.hip): the row already sits in registers for RoPE,
the reduction is a shuffle inside the 4 or 8 lanes that own it, and the only
saved state is one fp32 rstd per (token, head) — the normalized activations
are recomputed in backward. Everything else (CPU, fp16, ``MCDP_FORCE_TORCH=1``,
other head dims) runs the differentiable composition ``rms_norm_ref`` ->
``apply_rope``, which is also the numerics oracle of the tests.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from ._ext import get_ext, use_hip
from .rmsnorm import rms_norm_ref
from .rope import apply_rope

# head dims the kernels are compiled for (D/16 lanes own a row)
HIP_HEAD_DIMS = (64, 128)


def qk_norm_rope_ref(q, k, q_weight, k_weight, cos, sin, eps,
                     traditional: bool = False, offset: int = 0):
    """Differentiable torch composition (fallback path and test oracle)."""
    q = apply_rope(rms_norm_ref(q, q_weight, eps), cos, sin, traditional, offset)
    k = apply_rope(rms_norm_ref(k, k_weight, eps), cos, sin, traditional, offset)
    return q, k


def kernel_weight(w: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The norm weight as the kernels read it: x's dtype, contiguous, 16-byte
    aligned (they load it with 16-byte vector loads)."""
    w = w.detach().to(dtype).contiguous()
    return w if w.data_ptr() % 16 == 0 else w.clone()


def _bshd(t: torch.Tensor) -> torch.Tensor:
    """[B,S,H,D] with a contiguous (h,d) inner block, as the kernels take it."""
    B, S, H, D = t.shape
    ok = t.stride(3) == 1 and t.stride(2) == D and (
        B == 1 or S == 1 or t.stride(0) == S * t.stride(1))
    return t if ok else t.contiguous()


def _joint_view(q: torch.Tensor, k: torch.Tensor) -> Optional[torch.Tensor]:
    """If q and k are the adjacent head slices of one fused projection
    (``qkv.split(...)`` views), the [B,S,Hq+Hkv,D] view over both — one
    launch then covers q and k. None otherwise."""
    B, S, Hq, D = q.shape
    H = Hq + k.shape[2]
    if (q.dtype != k.dtype or k.shape[:2] != q.shape[:2]
            or q.untyped_storage().data_ptr() != k.untyped_storage().data_ptr()
            or k.storage_offset() != q.storage_offset() + Hq * D):
        return None
    for t in (q, k):
        if t.stride(3) != 1 or t.stride(2) != D:
            return None
    if S > 1:
        rs = q.stride(1)
        ok = k.stride(1) == rs and (B == 1 or (q.stride(0) == S * rs and k.stride(0) == S * rs))
    elif B > 1:
        rs = q.stride(0)
        ok = k.stride(0) == rs
    else:
        rs, ok = H * D, True
    if not ok or rs < H * D:
        return None
    return q.as_strided((B, S, H, D), (S * rs, rs, D, 1), q.storage_offset())


class _QKNormRopeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, q_weight, k_weight, cos, sin, eps, traditional, offset):
        ext = get_ext()
        Hq = q.shape[2]
        wq = kernel_weight(q_weight, q.dtype)
        wk = kernel_weight(k_weight, k.dtype)
        x = _joint_view(q, k)
        if x is not None:
            y, rstd = ext.qknorm_rope_fwd(x, Hq, wq, wk, cos, sin, traditional, offset, eps)
            qo, ko = y[:, :, :Hq], y[:, :, Hq:]
            rq, rk = rstd[:, :, :Hq].contiguous(), rstd[:, :, Hq:].contiguous()
        else:
            q, k = _bshd(q), _bshd(k)
            qo, rq = ext.qknorm_rope_fwd(q, Hq, wq, wq, cos, sin, traditional, offset, eps)
            ko, rk = ext.qknorm_rope_fwd(k, 0, wk, wk, cos, sin, traditional, offset, eps)
        ctx.save_for_backward(q, k, rq, rk, wq, wk, cos, sin)
        ctx.meta = (traditional, offset, q_weight.dtype, k_weight.dtype)
        return qo, ko

    @staticmethod
    def backward(ctx, gq, gk):
        q, k, rq, rk, wq, wk, cos, sin = ctx.saved_tensors
        traditional, offset, qw_dtype, kw_dtype = ctx.meta
        ext = get_ext()
        B, S, Hq, D = q.shape
        Hkv = k.shape[2]
        # dq | dk side by side, so a split-backward over a fused projection
        # finds them adjacent
        dx = torch.empty(B, S, Hq + Hkv, D, dtype=q.dtype, device=q.device)
        dq, dk = dx[:, :, :Hq], dx[:, :, Hq:]
        dwq = ext.qknorm_rope_bwd(_bshd(gq), _bshd(q), rq, Hq, wq, wq, cos, sin,
                                  traditional, offset, dq)[0]
        dwk = ext.qknorm_rope_bwd(_bshd(gk), _bshd(k), rk, 0, wk, wk, cos, sin,
                                  traditional, offset, dk)[1]
        return dq, dk, dwq.to(qw_dtype), dwk.to(kw_dtype), None, None, None, None, None


def qk_norm_rope(
    q: torch.Tensor,
    k: torch.Tensor,
    q_weight: torch.Tensor,
    k_weight: torch.Tensor,
    cos: torch.Tensor,
    sin: torch.Tensor,
    eps: float,
    traditional: bool = False,
    offset: int = 0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """q: [B,S,Hq,D], k: [B,S,Hkv,D] -> (q', k'), each head RMS-normalized over
    D with its ``[D]`` weight, then rotated at positions ``offset .. offset+S-1``.
    Gradients flow to q, k and both weights."""
    D = q.shape[-1]
    if D in HIP_HEAD_DIMS and k.shape[-1] == D and use_hip(q, k, q_weight, k_weight):
        return _QKNormRopeFn.apply(q, k, q_weight, k_weight, cos, sin, float(eps),
                                   bool(traditional), int(offset))
    return qk_norm_rope_ref(q, k, q_weight, k_weight, cos, sin, eps, traditional, offset)
