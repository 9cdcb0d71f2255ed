"""RMSNorm with fp32 accumulation.

Replaces the reference's Python-composed RMSNorm
(/root/reference/models/llama.py:44-56) with a CDNA4 HIP kernel
(csrc/rmsnorm.hip): one workgroup per row block, wave shuffle reductions,
bf16x8 vectorized loads, fp32 math.
"""
from __future__ import annotations

import torch

from ._ext import get_ext, use_hip


def _w_like(weight: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """The kernels read the weight through x's element type: hand them one of
    x's dtype (an fp32 norm weight under a bf16 activation is cast here; the
    returned dw is cast back to the weight's dtype by the caller)."""
    return (weight if weight.dtype == x.dtype else weight.to(x.dtype)).contiguous()


def rms_norm_ref(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    """Pure-torch reference (fp32 accumulation, same contract as the kernel)."""
    xf = x.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * rstd * weight.float()).to(x.dtype)


class _RMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor, eps: float,
                emit_amax: bool = False):
        if use_hip(x, weight):
            ext = get_ext()
            if emit_amax:
                y, rstd, amax = ext.rmsnorm_fwd_res(
                    x.contiguous(), x.new_empty(0), _w_like(weight, x), eps, True
                )
                y._mcdp_amax = amax  # fp8 quantizer skips its amax pass
            else:
                y, rstd = ext.rmsnorm_fwd(x.contiguous(), _w_like(weight, x), eps)
            ctx.save_for_backward(x, weight, rstd)
            ctx.eps = eps
            ctx.hip = True
            return y
        # CPU reference path
        xf = x.float()
        rstd = torch.rsqrt(xf.pow(2).mean(-1) + eps)
        y = (xf * rstd.unsqueeze(-1) * weight.float()).to(x.dtype)
        ctx.save_for_backward(x, weight, rstd)
        ctx.eps = eps
        ctx.hip = False
        return y

    @staticmethod
    def backward(ctx, dy: torch.Tensor):
        x, weight, rstd = ctx.saved_tensors
        if ctx.hip:
            ext = get_ext()
            dx, dw = ext.rmsnorm_bwd(
                x.contiguous(), _w_like(weight, x), rstd, dy.contiguous()
            )
            return dx, dw.to(weight.dtype), None, None
        xf = x.float()
        dyf = dy.float()
        wf = weight.float()
        r = rstd.unsqueeze(-1)
        xhat = xf * r
        dw = (dyf * xhat).reshape(-1, x.shape[-1]).sum(0)
        # dx = r * (dy*w - xhat * mean(dy*w*xhat))
        dyw = dyf * wf
        dx = r * (dyw - xhat * (dyw * xhat).mean(-1, keepdim=True))
        return dx.to(x.dtype), dw.to(weight.dtype), None, None


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5,
             emit_amax: bool = False) -> torch.Tensor:
    return _RMSNormFn.apply(x, weight, eps, emit_amax)


class RMSNorm(torch.nn.Module):
    def __init__(self, hidden_size: int, eps: float = 1e-5, dtype=None):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(hidden_size, dtype=dtype))
        self.eps = eps
        # set by the model when the fp8 path consumes this norm's output
        self.emit_amax = False

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return rms_norm(x, self.weight, self.eps, self.emit_amax)

    def extra_repr(self) -> str:
        return f"{self.weight.shape[0]}, eps={self.eps}"


class _AddRMSNormFn(torch.autograd.Function):
    """Fused residual: s = x + res; y = rmsnorm(s) * w in ONE kernel each way
    (csrc/rmsnorm.hip HAS_RES / HAS_DADD) — the separate residual-add kernels
    and their HBM round trips disappear. Returns (s, y); s is the residual
    stream the next sublayer adds onto."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, res: torch.Tensor, weight: torch.Tensor, eps: float,
                emit_amax: bool = False):
        if use_hip(x, res, weight):
            ext = get_ext()
            out = ext.rmsnorm_fwd_res(
                x.contiguous(), res.contiguous(), _w_like(weight, x), eps, emit_amax
            )
            y, rstd, s = out[0], out[1], out[2]
            if emit_amax:
                y._mcdp_amax = out[3]
            ctx.save_for_backward(s, weight, rstd)
            ctx.hip = True
            return s, y
        s = x + res
        sf = s.float()
        rstd = torch.rsqrt(sf.pow(2).mean(-1) + eps)
        y = (sf * rstd.unsqueeze(-1) * weight.float()).to(x.dtype)
        ctx.save_for_backward(s, weight, rstd)
        ctx.hip = False
        return s, y

    @staticmethod
    def backward(ctx, ds: torch.Tensor, dy: torch.Tensor):
        s, weight, rstd = ctx.saved_tensors
        if ctx.hip:
            ext = get_ext()
            dadd = ds.contiguous() if ds is not None else s.new_empty(0)
            dx, dw = ext.rmsnorm_bwd_add(
                s.contiguous(), _w_like(weight, s), rstd, dy.contiguous(), dadd
            )
            # s = x + res: both inputs get the same gradient tensor
            return dx, dx, dw.to(weight.dtype), None, None
        sf = s.float()
        dyf = dy.float()
        wf = weight.float()
        r = rstd.unsqueeze(-1)
        xhat = sf * r
        dw = (dyf * xhat).reshape(-1, s.shape[-1]).sum(0)
        dyw = dyf * wf
        dx = (r * (dyw - xhat * (dyw * xhat).mean(-1, keepdim=True))).to(s.dtype)
        if ds is not None:
            dx = dx + ds
        return dx, dx, dw.to(weight.dtype), None, None


def add_rms_norm(x: torch.Tensor, res: torch.Tensor, weight: torch.Tensor,
                 eps: float = 1e-5, emit_amax: bool = False):
    """(s, y) with s = x + res and y = rms_norm(s) * weight, fused."""
    return _AddRMSNormFn.apply(x, res, weight, eps, emit_amax)
