"""Fused cross-entropy over the vocabulary with pad masking.

Replaces the reference's ``cross_entropy + pad-mask + token-count`` Python
composition (/root/reference/core/training.py:1222-1234). The HIP kernel
(csrc/cross_entropy.hip) does one pass per row: online max + sum-exp over
the 32k vocab in fp32, never materializing an fp32 copy of the logits;
backward writes bf16 dlogits = (softmax - onehot) * scale directly.

Returns (loss_mean_over_tokens, ntokens).

``cross_entropy_with_z`` adds the auxiliary z-loss (PaLM, OLMo-2): beside the
mean CE it returns ``z = mean(lse_i^2)`` over the counted rows, where ``lse``
is the log-partition the forward kernel holds anyway. The caller optimises
``ce + coef * z``; with upstream gradients g_ce and g_z of the two means the
one backward kernel writes
``dlogits = p * (a + b * lse) - a * onehot``, a = g_ce / ntok, b = 2 g_z / ntok,
so z-loss costs one multiply-add per element and no further pass over the
logits (``ce_fwd_z`` / ``ce_bwd_z``; the plain ``ce_fwd`` / ``ce_bwd`` stay as
they were and ``fused_cross_entropy`` still runs them).

``cross_entropy_capped`` is that loss of the soft-capped logits
``cap * tanh(logits / cap)``, capped inside the kernels (``ce_cap_fwd`` /
``ce_cap_bwd``).
"""
from __future__ import annotations

from typing import Tuple

import torch

from ._ext import get_ext, use_hip
from .softcap import check_cap


def cross_entropy_ref(
    logits: torch.Tensor, targets: torch.Tensor, ignore_index: int
) -> Tuple[torch.Tensor, torch.Tensor]:
    lf = logits.float()
    mask = targets != ignore_index
    ntok = mask.sum()
    safe_targets = targets.masked_fill(~mask, 0)
    lse = torch.logsumexp(lf, dim=-1)
    picked = lf.gather(-1, safe_targets.unsqueeze(-1)).squeeze(-1)
    loss = ((lse - picked) * mask).sum() / ntok.clamp(min=1)
    return loss, ntok


class _FusedCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits: torch.Tensor, targets: torch.Tensor, ignore_index: int):
        n, v = logits.shape
        if use_hip(logits) and logits.shape[-1] % 8 == 0:  # kernel needs V%8==0
            ext = get_ext()
            loss_sum, ntok, lse = ext.ce_fwd(logits.contiguous(), targets.contiguous(), ignore_index)
            ctx.save_for_backward(logits, targets, lse, ntok)
            ctx.ignore_index = ignore_index
            ctx.hip = True
            ntok_f = ntok.clamp(min=1)
            return loss_sum / ntok_f, ntok
        lf = logits.float()
        mask = targets != ignore_index
        ntok = mask.sum()
        safe_targets = targets.masked_fill(~mask, 0)
        lse = torch.logsumexp(lf, dim=-1)
        picked = lf.gather(-1, safe_targets.unsqueeze(-1)).squeeze(-1)
        loss = ((lse - picked) * mask).sum() / ntok.clamp(min=1)
        ctx.save_for_backward(logits, targets, lse, ntok)
        ctx.ignore_index = ignore_index
        ctx.hip = False
        return loss, ntok

    @staticmethod
    def backward(ctx, dloss, _dntok):
        logits, targets, lse, ntok = ctx.saved_tensors
        scale = dloss / ntok.clamp(min=1).to(dloss.dtype)
        if ctx.hip:
            ext = get_ext()
            dlogits = ext.ce_bwd(
                logits.contiguous(), targets.contiguous(), lse, scale, ctx.ignore_index
            )
            return dlogits, None, None
        mask = (targets != ctx.ignore_index).unsqueeze(-1)
        safe_targets = targets.masked_fill(~mask.squeeze(-1), 0)
        p = torch.softmax(logits.float(), dim=-1)
        p.scatter_add_(
            -1,
            safe_targets.unsqueeze(-1),
            -torch.ones_like(safe_targets, dtype=p.dtype).unsqueeze(-1),
        )
        dlogits = (p * mask * scale).to(logits.dtype)
        return dlogits, None, None


def fused_cross_entropy(
    logits: torch.Tensor, targets: torch.Tensor, ignore_index: int = -100
) -> Tuple[torch.Tensor, torch.Tensor]:
    """logits: [N, V] (any leading shape flattened by caller), targets: [N].

    Returns (mean loss over non-ignored tokens, ntokens tensor)."""
    return _FusedCEFn.apply(logits, targets, ignore_index)


class _FusedCEWithZFn(torch.autograd.Function):
    """(ce_mean, z_mean, ntok) from ce_fwd_z; the backward takes both upstream
    gradients into one ce_bwd_z launch, its two scales built on the device."""

    @staticmethod
    def forward(ctx, logits: torch.Tensor, targets: torch.Tensor, ignore_index: int):
        ext = get_ext()
        loss_sum, z_sum, ntok, lse = ext.ce_fwd_z(
            logits.contiguous(), targets.contiguous(), ignore_index)
        ctx.save_for_backward(logits, targets, lse, ntok)
        ctx.ignore_index = ignore_index
        ctx.mark_non_differentiable(ntok)
        ntok_f = ntok.clamp(min=1)
        return loss_sum / ntok_f, z_sum / ntok_f, ntok

    @staticmethod
    def backward(ctx, g_ce, g_z, _dntok):
        logits, targets, lse, ntok = ctx.saved_tensors
        ntok_f = ntok.clamp(min=1).float()
        scale_ce = (g_ce.float() / ntok_f).reshape(1)
        scale_z = (2.0 * g_z.float() / ntok_f).reshape(1)
        dlogits = get_ext().ce_bwd_z(
            logits.contiguous(), targets.contiguous(), lse, scale_ce, scale_z,
            ctx.ignore_index)
        return dlogits, None, None


def cross_entropy_with_z(
    logits: torch.Tensor, targets: torch.Tensor, ignore_index: int = -100
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """logits: [N, V], targets: [N]. Returns (ce_mean, z_mean, ntok) over the
    rows whose target is not ``ignore_index``: ce as ``fused_cross_entropy``,
    z = mean(lse^2). Both means are differentiable and are 0 when no row
    counts. The HIP path is chosen as in ``fused_cross_entropy``; elsewhere
    (CPU, other dtypes, V % 8 != 0) a torch composition runs, in fp64 for fp64
    logits and in fp32 otherwise."""
    if use_hip(logits) and logits.shape[-1] % 8 == 0:  # kernel needs V%8==0
        return _FusedCEWithZFn.apply(logits, targets, ignore_index)
    lf = logits if logits.dtype == torch.float64 else logits.float()
    mask = targets != ignore_index
    ntok = mask.sum()
    safe_targets = targets.masked_fill(~mask, 0)
    lse = torch.logsumexp(lf, dim=-1)
    picked = lf.gather(-1, safe_targets.unsqueeze(-1)).squeeze(-1)
    denom = ntok.clamp(min=1)
    ce = ((lse - picked) * mask).sum() / denom
    z = (lse * lse * mask).sum() / denom
    return ce, z, ntok


class _FusedCECappedFn(torch.autograd.Function):
    """_FusedCEWithZFn over the capped kernels: ce_cap_fwd / ce_cap_bwd cap
    every logit in registers, so neither the capped [N, V] tensor nor a saved
    copy for tanh's backward exists."""

    @staticmethod
    def forward(ctx, logits: torch.Tensor, targets: torch.Tensor, cap: float,
                ignore_index: int):
        ext = get_ext()
        loss_sum, z_sum, ntok, lse = ext.ce_cap_fwd(
            logits.contiguous(), targets.contiguous(), ignore_index, cap)
        ctx.save_for_backward(logits, targets, lse, ntok)
        ctx.ignore_index = ignore_index
        ctx.cap = cap
        ctx.mark_non_differentiable(ntok)
        ntok_f = ntok.clamp(min=1)
        return loss_sum / ntok_f, z_sum / ntok_f, ntok

    @staticmethod
    def backward(ctx, g_ce, g_z, _dntok):
        logits, targets, lse, ntok = ctx.saved_tensors
        ntok_f = ntok.clamp(min=1).float()
        scale_ce = (g_ce.float() / ntok_f).reshape(1)
        scale_z = (2.0 * g_z.float() / ntok_f).reshape(1)
        dlogits = get_ext().ce_cap_bwd(
            logits.contiguous(), targets.contiguous(), lse, scale_ce, scale_z,
            ctx.ignore_index, ctx.cap)
        return dlogits, None, None, None


def cross_entropy_capped(
    logits: torch.Tensor, targets: torch.Tensor, cap: float, ignore_index: int = -100
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``cross_entropy_with_z`` of the soft-capped logits
    ``t = cap * tanh(logits / cap)`` (final-logit soft-capping, Gemma-2):
    (ce_mean, z_mean, ntok) with lse, and so z, those of the capped rows. The
    gradient reaches the raw logits: ``(p * (a + b * lse) - a * onehot) *
    (1 - (t / cap)^2)`` with a and b as in ``cross_entropy_with_z``. The HIP
    path (same rule as ``fused_cross_entropy``) caps inside ``ce_cap_fwd`` /
    ``ce_cap_bwd`` and moves the bytes of the plain loss; elsewhere the torch
    composition runs on ``softcap(logits)``, in fp64 for fp64 logits and in
    fp32 otherwise."""
    cap = check_cap(cap)
    if use_hip(logits) and logits.shape[-1] % 8 == 0:  # kernel needs V%8==0
        return _FusedCECappedFn.apply(logits, targets, cap, ignore_index)
    lf = logits if logits.dtype == torch.float64 else logits.float()
    return cross_entropy_with_z(cap * torch.tanh(lf / cap), targets, ignore_index)
