"""Soft-capping, ``y = cap * tanh(x / cap)`` (Gemma-2's final-logit cap).

The training loss does not go through here: ``cross_entropy_capped``
(ops/cross_entropy.py) caps inside the cross-entropy kernels. These are for
the paths that need the capped logits as a tensor: ``Model.forward`` for
generation, and ``softcap_`` in place for the static decoder, whose captured
graph must not allocate.

On a GPU, for contiguous bf16 / fp32 input, ``softcap`` is one autograd node
over the HIP kernels of csrc/softcap.hip; the backward is taken from the saved
*output*, ``dx = dy * (1 - (y / cap)^2)``, so the input is free to die.
Elsewhere (CPU, other dtypes, non-contiguous input) the torch composition
runs, in fp64 for fp64 input and with fp32 math otherwise.
"""
from __future__ import annotations

import math

import torch

from ._ext import get_ext, use_hip


def check_cap(cap) -> float:
    cap = float(cap)
    if not (math.isfinite(cap) and cap > 0.0):
        raise ValueError(f"softcap: cap must be finite and > 0, got {cap}")
    return cap


def _softcap_torch(x: torch.Tensor, cap: float) -> torch.Tensor:
    if x.dtype == torch.float64:
        return cap * torch.tanh(x / cap)
    return (cap * torch.tanh(x.float() / cap)).to(x.dtype)


class _SoftcapFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, cap: float):
        y = get_ext().softcap_fwd(x, cap)
        ctx.save_for_backward(y)
        ctx.cap = cap
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return get_ext().softcap_bwd(dy.contiguous(), y, ctx.cap), None


def softcap(x: torch.Tensor, cap: float) -> torch.Tensor:
    """``cap * tanh(x / cap)``, differentiable, same shape and dtype as ``x``."""
    cap = check_cap(cap)
    if use_hip(x) and x.is_contiguous():
        return _SoftcapFn.apply(x, cap)
    return _softcap_torch(x, cap)


def softcap_(x: torch.Tensor, cap: float) -> torch.Tensor:
    """``softcap`` written into ``x``; no autograd. On the HIP path it
    allocates nothing and does not synchronise."""
    cap = check_cap(cap)
    with torch.no_grad():
        if use_hip(x) and x.is_contiguous():
            get_ext().softcap_(x, cap)
        else:
            x.copy_(_softcap_torch(x, cap))
    return x
