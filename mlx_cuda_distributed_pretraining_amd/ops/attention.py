"""Attention ops: flash (tiled, online-softmax) + flex (block-sparse/score-mod).

Replaces the reference's three Python attention modules
(/root/reference/models/attention/{flash,flex,simple}_attention.py — all of
which materialize S×S scores; the "flash" one says so at flash_attention.py:100)
with a real tiled FlashAttention-2 fwd/bwd HIP kernel (csrc/attn_fwd.hip,
csrc/attn_bwd.hip): MFMA bf16 tiles, LDS-staged K/V with XOR swizzle, online
softmax, causal/sliding-window block skip, GQA without materializing repeated
K/V. FlexAttention's score/mask mods become kernel template variants
(MOD_* codes below) instead of per-element Python callbacks.

Tensor layout: BSHD — q [B, S, Hq, D], k/v [B, S, Hkv, D]; Hq % Hkv == 0.
(BSHD is what the QKV projection GEMM produces; keeping it end-to-end means
zero transpose copies on the hot path.)
"""
from __future__ import annotations

import math
from typing import Callable, NamedTuple, Optional

import torch

from ._ext import get_ext, use_hip

# Mask/score-mod variant codes understood by the kernels.
MOD_NONE = 0  # full (bidirectional) attention
MOD_CAUSAL = 1
MOD_SLIDING_WINDOW = 2  # causal AND (q - kv) < window
MOD_PREFIX_LM = 3  # bidirectional over [0, prefix) then causal
MOD_ALIBI = 4  # causal + alibi slope * (kv - q)


def _mods_to_code(causal: bool, window: Optional[int], prefix_len: Optional[int], alibi: bool):
    if alibi:
        return MOD_ALIBI
    if window is not None:
        return MOD_SLIDING_WINDOW
    if prefix_len is not None:
        return MOD_PREFIX_LM
    return MOD_CAUSAL if causal else MOD_NONE


def attention_ref(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    causal: bool = True,
    scale: Optional[float] = None,
    window: Optional[int] = None,
    prefix_len: Optional[int] = None,
    alibi_slopes: Optional[torch.Tensor] = None,
    score_mod: Optional[Callable] = None,
    mask_mod: Optional[Callable] = None,
    return_lse: bool = False,
    doc_start: Optional[torch.Tensor] = None,
    softcap: Optional[float] = None,
):
    """fp32 reference composition (used on CPU and as the test oracle).

    q: [B, S, Hq, D]; k, v: [B, Skv, Hkv, D] (BSHD).
    doc_start: optional int [B, S] document lower bounds (``document_bounds``):
    row (b, s) additionally keeps only keys at positions >= doc_start[b, s].
    It needs S == Skv and is combined with the other masks by AND.
    score_mod(scores[B,H,S,S], b_idx, h_idx, q_idx, kv_idx) -> scores, applied
    to the scaled scores (FlexAttention semantics, vectorized over the full
    score tensor). mask_mod(b, h, q_idx, kv_idx) -> bool keep-mask. Index
    tensors arrive BROADCASTABLE (q [S,1] x kv [1,Skv]); write mods as plain
    expressions over them.
    softcap: attention-logit soft-capping, ``c * tanh(scores / c)`` on the
    scaled scores, before ALiBi / ``score_mod`` / masking (see
    ``flash_attention``).
    """
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    rep = Hq // Hkv
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    qf = q.float().transpose(1, 2)  # BHSD internally
    kf = k.float().transpose(1, 2)
    vf = v.float().transpose(1, 2)
    if rep > 1:
        kf = kf.repeat_interleave(rep, dim=1)
        vf = vf.repeat_interleave(rep, dim=1)
    scores = torch.einsum("bhsd,bhtd->bhst", qf, kf) * scale
    if softcap is not None:
        scores = softcap * torch.tanh(scores / softcap)

    Skv = k.shape[1]
    # Absolute query positions: with a KV cache, the S query rows sit at the
    # END of the Skv keys (decode: S=1 at position Skv-1).
    q_idx = (torch.arange(S, device=q.device) + (Skv - S)).view(S, 1)
    kv_idx = torch.arange(Skv, device=q.device).view(1, Skv)
    keep = torch.ones(S, Skv, dtype=torch.bool, device=q.device)
    if causal or window is not None or prefix_len is not None:
        causal_keep = kv_idx <= q_idx
        if prefix_len is not None:
            keep = causal_keep | (kv_idx < prefix_len)
        elif window is not None:
            keep = causal_keep & (q_idx - kv_idx < window)
        elif causal:
            keep = causal_keep
    if alibi_slopes is not None:
        bias = alibi_slopes.float().view(1, Hq, 1, 1) * (kv_idx - q_idx).float().view(1, 1, S, Skv)
        scores = scores + bias
        keep = keep & (kv_idx <= q_idx)
    # mods receive broadcastable index tensors (q [S,1], kv [1,Skv]) so a
    # plain expression like (ki <= qi) evaluates as the outer grid — the same
    # convention CompiledBlockMask compiles with (vectorized FlexAttention
    # semantics).
    if score_mod is not None:
        b_idx = torch.arange(B, device=q.device).view(B, 1, 1, 1)
        h_idx = torch.arange(Hq, device=q.device).view(1, Hq, 1, 1)
        scores = score_mod(scores, b_idx, h_idx, q_idx.view(1, 1, S, 1),
                           kv_idx.view(1, 1, 1, Skv))
    if mask_mod is not None:
        b_idx = torch.arange(B, device=q.device)
        h_idx = torch.arange(Hq, device=q.device)
        keep = keep & mask_mod(b_idx, h_idx, q_idx, kv_idx)
    keep = keep.view(1, 1, S, Skv)
    if doc_start is not None:
        if S != Skv or tuple(doc_start.shape) != (B, S):
            raise ValueError(
                f"doc_start must be [B, S] = [{B}, {S}] with Sq == Skv, got "
                f"{tuple(doc_start.shape)} (Skv = {Skv})")
        # batch-dependent: the keep mask becomes [B, 1, S, Skv]
        keep = keep & (kv_idx.view(1, 1, 1, Skv) >= doc_start.view(B, 1, S, 1))
    scores = scores.masked_fill(~keep, float("-inf"))
    lse = torch.logsumexp(scores, dim=-1)
    p = torch.softmax(scores, dim=-1)
    # rows with no valid keys produce NaN from softmax over all -inf; zero them
    p = torch.nan_to_num(p, nan=0.0)
    o = torch.einsum("bhst,bhtd->bhsd", p, vf).transpose(1, 2)  # back to BSHD
    if return_lse:
        return o.to(q.dtype).contiguous(), lse
    return o.to(q.dtype).contiguous()


def _doc_end_from_starts(is_start: torch.Tensor) -> torch.Tensor:
    """is_start bool [B, S] -> int32 [B, S]: the next start after each column
    (S when there is none), i.e. one past the column's document."""
    B, S = is_start.shape
    idx = torch.arange(S, device=is_start.device).expand(B, S)
    nxt = torch.where(is_start, idx, torch.full_like(idx, S))
    # suffix minimum = flip-cummin; column s wants the minimum over t > s
    sfx = torch.cummin(nxt.flip(1), dim=1).values.flip(1)
    end = torch.cat([sfx[:, 1:], torch.full_like(idx[:, :1], S)], dim=1)
    return end.to(torch.int32).contiguous()


def document_bounds(tokens: torch.Tensor, bos_id: Optional[int] = None,
                    eos_id: Optional[int] = None):
    """Document bounds of packed token rows, for document-masked attention.

    tokens: int [B, S]. A document starts at column 0, at every ``bos_id`` and
    right after every ``eos_id`` (an ``EOS BOS`` pair therefore opens one
    document, not two). Returns ``(doc_start, doc_end)``, both int32 [B, S] on
    the tokens' device: the first position of each column's document and one
    past its last. Both are non-decreasing along S and
    ``doc_start[b, s] <= s < doc_end[b, s]``. A few vectorised ops, no host
    sync, no Python loop over B or S.
    """
    if tokens.dim() != 2:
        raise ValueError(f"document_bounds wants [B, S] tokens, got {tuple(tokens.shape)}")
    B, S = tokens.shape
    is_start = torch.zeros(B, S, dtype=torch.bool, device=tokens.device)
    is_start[:, :1] = True
    if bos_id is not None:
        is_start |= tokens == bos_id
    if eos_id is not None:
        is_start[:, 1:] |= tokens[:, :-1] == eos_id
    idx = torch.arange(S, device=tokens.device).expand(B, S)
    start = torch.cummax(torch.where(is_start, idx, torch.zeros_like(idx)), dim=1).values
    return start.to(torch.int32).contiguous(), _doc_end_from_starts(is_start)


class _Mask(NamedTuple):
    """The mask of one flash-attention call, in the form the kernels and the
    reference take it. ``build`` is the one place that checks and normalises
    the public keywords; ``fwd`` / ``bwd`` are the one place that picks the
    mod-code or the document binding."""

    causal: bool
    window: Optional[int]
    prefix_len: Optional[int]
    slopes: torch.Tensor  # f32 ALiBi slopes [Hq]; empty = no ALiBi
    doc_start: Optional[torch.Tensor]  # int32 contiguous [B, S], or None
    doc_end: Optional[torch.Tensor]  # likewise; set whenever doc_start is
    softcap: Optional[float] = None  # attention-logit soft-cap c, or None

    @classmethod
    def build(cls, causal, window, prefix_len, alibi_slopes, doc_start, doc_end,
              B: int, Sq: int, Skv: int, Hq: int, device, softcap=None) -> "_Mask":
        if softcap is not None:
            softcap = float(softcap)
            if not (math.isfinite(softcap) and softcap > 0):
                raise ValueError(f"softcap must be finite and > 0 (or None), got {softcap}")
            # capped kernels exist for none / causal / sliding window only; the
            # fp32 composition would be a silent O(S^2) fallback in a training run
            if doc_start is not None or prefix_len is not None or alibi_slopes is not None:
                raise ValueError("softcap cannot be combined with doc_start, prefix_len or "
                                 "ALiBi: there are no capped kernels for those masks")
        if alibi_slopes is not None and not isinstance(alibi_slopes, torch.Tensor):
            # an int head count builds the standard 2^(-8(i+1)/H) slopes —
            # matches the reference's loose API
            alibi_slopes = torch.tensor([2 ** (-8.0 * (i + 1) / Hq) for i in range(Hq)],
                                        dtype=torch.float32, device=device)
        if doc_start is None:
            if doc_end is not None:
                raise ValueError("doc_end needs doc_start")
        else:
            if window is not None or prefix_len is not None or alibi_slopes is not None:
                raise ValueError("document mask (doc_start) cannot be combined with "
                                 "window, prefix_len or ALiBi")
            if not causal:
                raise ValueError("document mask (doc_start) is causal: causal=False is not "
                                 "supported")
            if Sq != Skv:
                raise ValueError(f"document mask (doc_start) is training-only: Sq ({Sq}) != "
                                 f"Skv ({Skv})")
            # int32, contiguous, [B, S], on ``device``; doc_end derived from
            # doc_start when omitted (column s opens a document exactly when
            # doc_start[b, s] == s)
            for name, t in (("doc_start", doc_start), ("doc_end", doc_end)):
                if t is not None and tuple(t.shape) != (B, Sq):
                    raise ValueError(f"{name} must be [B, S] = [{B}, {Sq}], got {tuple(t.shape)}")
            doc_start = doc_start.to(device=device, dtype=torch.int32).contiguous()
            if doc_end is None:
                idx = torch.arange(Sq, device=device, dtype=torch.int32)
                doc_end = _doc_end_from_starts(doc_start == idx)
            else:
                doc_end = doc_end.to(device=device, dtype=torch.int32).contiguous()
        slopes = (alibi_slopes.float().contiguous() if alibi_slopes is not None
                  else torch.empty(0, dtype=torch.float32, device=device))
        return cls(causal, window, prefix_len, slopes, doc_start, doc_end, softcap)

    @property
    def mod(self) -> int:
        return _mods_to_code(self.causal, self.window, self.prefix_len, self.slopes.numel() > 0)

    @property
    def modarg(self) -> int:
        return int(self.window if self.window is not None
                   else (self.prefix_len if self.prefix_len is not None else 0))

    def save(self, ctx, *tensors):
        """ctx.save_for_backward of a node's own tensors followed by the
        mask's; ``load`` undoes it."""
        ctx.save_for_backward(*tensors, *self[3:6])
        ctx.mask_meta = (*self[:3], self.softcap)

    @classmethod
    def load(cls, ctx):
        *tensors, slopes, doc_start, doc_end = ctx.saved_tensors
        *meta, softcap = ctx.mask_meta
        return cls(*meta, slopes, doc_start, doc_end, softcap), tensors

    def ref(self, q, k, v, scale, return_lse=False):
        return attention_ref(q, k, v, causal=self.causal, scale=scale, window=self.window,
                             prefix_len=self.prefix_len,
                             alibi_slopes=self.slopes if self.slopes.numel() else None,
                             return_lse=return_lse, doc_start=self.doc_start,
                             softcap=self.softcap)

    def fwd(self, ext, q, k, v, scale):
        if self.softcap is not None:
            return ext.attn_cap_fwd(q, k, v, scale, self.mod, self.modarg, self.softcap)
        if self.doc_start is not None:
            return ext.attn_fwd_doc(q, k, v, scale, self.doc_start)
        return ext.attn_fwd(q, k, v, scale, self.mod, self.modarg, self.slopes)

    def bwd(self, ext, q, k, v, o, do, lse, scale, dq=None, dk=None, dv=None):
        """dq/dk/dv: out views to write in place; None or empty = allocate."""
        if self.softcap is not None:
            return ext.attn_cap_bwd(q, k, v, o, do, lse, scale, self.mod, self.modarg,
                                    self.softcap, dq, dk, dv)
        if self.doc_start is not None:
            return ext.attn_bwd_doc(q, k, v, o, do, lse, scale, self.doc_start, self.doc_end,
                                    dq, dk, dv)
        return ext.attn_bwd(q, k, v, o, do, lse, scale, self.mod, self.modarg, self.slopes,
                            dq, dk, dv)


class _FlashAttnFn(torch.autograd.Function):
    """Kernels on bf16 GPU inputs, the fp32 composition otherwise (mask checks:
    _Mask.build)."""

    @staticmethod
    def forward(ctx, q, k, v, scale, mask):
        scale = scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])
        hip = use_hip(q, k, v, dtypes=(torch.bfloat16,))
        if hip:
            o, lse = mask.fwd(get_ext(), q, k, v, scale)
        else:
            o, lse = mask.ref(q, k, v, scale, return_lse=True)
        mask.save(ctx, q, k, v, o, lse)
        ctx.meta = (scale, hip)
        return o

    @staticmethod
    def backward(ctx, do):
        mask, (q, k, v, o, lse) = _Mask.load(ctx)
        scale, hip = ctx.meta
        if hip:
            return (*mask.bwd(get_ext(), q, k, v, o, do, lse, scale), None, None)
        # CPU reference backward: recompute with autograd in fp32
        with torch.enable_grad():
            qf = q.detach().float().requires_grad_(True)
            kf = k.detach().float().requires_grad_(True)
            vf = v.detach().float().requires_grad_(True)
            grads = torch.autograd.grad(mask.ref(qf, kf, vf, scale), [qf, kf, vf], do.float())
        return grads[0].to(q.dtype), grads[1].to(k.dtype), grads[2].to(v.dtype), None, None


def flash_attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    causal: bool = True,
    scale: Optional[float] = None,
    window: Optional[int] = None,
    prefix_len: Optional[int] = None,
    alibi_slopes: Optional[torch.Tensor] = None,
    doc_start: Optional[torch.Tensor] = None,
    doc_end: Optional[torch.Tensor] = None,
    softcap: Optional[float] = None,
) -> torch.Tensor:
    """Tiled attention, BSHD layout: [B,S,Hq,D] x [B,S,Hkv,D] -> [B,S,Hq,D]
    (q.shape[2] is the HEAD count — an int ``alibi_slopes`` relies on that).

    Document mask (packed sequences)
    --------------------------------
    ``doc_start`` / ``doc_end`` (int [B, S], from ``document_bounds``) keep
    every token inside its own document: row (b, s) attends to keys in
    ``[doc_start[b, s], s]``. The mask is the same for all heads, costs two
    int32 rows per sequence instead of S^2 bits per head, and is rebuilt per
    batch with a few device ops. On bf16 GPU inputs it runs the MOD_DOCUMENT
    kernels forward and backward (csrc/attn_fwd.hip, csrc/attn_bwd.hip), which
    skip the kv tiles in front of a q block's first document and the q tiles
    past a kv block's last one, so it does no more work than causal. CPU and
    other dtypes run ``attention_ref(doc_start=...)``.

      * ``doc_end`` is derived from ``doc_start`` when omitted.
      * Training only: it needs Sq == Skv and ``causal=True``, and cannot be
        combined with ``window``, ``prefix_len`` or ALiBi (``ValueError``).
      * Both tensors must be well-formed (non-decreasing,
        ``doc_start <= s < doc_end``); the kernels clamp what they use as an
        address or loop bound, so a bad tensor gives wrong numbers, not a
        fault.
      * RoPE needs no per-document position reset: scores depend on
        q_pos - k_pos only.

    Attention-logit soft-capping
    ----------------------------
    ``softcap=c`` (finite, > 0) bounds the scores: with ``x = scale * q.k``,
    ``t = c * tanh(x / c)``, ``P = softmax(t)`` over the kept keys and the
    saved log-sum-exp is that of ``t`` (Gemma-2 uses c = 50). The cap comes
    after ``scale`` and before masking. The backward multiplies the score
    gradient by ``1 - (t / c)^2``. On bf16 GPU inputs it runs the capped
    instantiations of the same kernels (``attn_cap_fwd`` / ``attn_cap_bwd``:
    one exp and one reciprocal more per score, nothing kept across a tile);
    CPU and other dtypes run ``attention_ref(softcap=c)``.

      * Masks: full, causal and sliding window. With ``doc_start``,
        ``prefix_len`` or ALiBi it raises ``ValueError``: those masks have no
        capped kernels yet, and a silent O(S^2) fallback in a training run is
        worse than an error.
      * It needs ``scale > 0``.
      * ``softcap=None`` calls exactly the uncapped kernels.
    """
    B, Sq, Hq, _ = q.shape
    mask = _Mask.build(causal, window, prefix_len, alibi_slopes, doc_start, doc_end,
                       B, Sq, k.shape[1], Hq, q.device, softcap)
    return _FlashAttnFn.apply(q, k, v, scale, mask)


class _RopeAttnQKVFn(torch.autograd.Function):
    """Fused qkv-slice -> RoPE(q,k) -> flash attention, HIP path only.

    Takes the FUSED [B, S, (Hq+2*Hkv)*D] projection output directly so the
    backward can write dQ/dK/dV straight into ONE dqkv buffer (strided out
    views for attn_bwd / rope_fwd_out) — eliminating autograd's
    split-backward torch.cat over the three grads (a full extra read+write
    of the qkv-grad per layer, the CatArrayBatchedCopy kernel in profiles)."""

    @staticmethod
    def forward(ctx, qkv, cos, sin, Hq, Hkv, D, traditional, scale, mask):
        B, S, _ = qkv.shape
        scale = scale if scale is not None else 1.0 / math.sqrt(D)
        q = qkv[..., : Hq * D].view(B, S, Hq, D)
        k = qkv[..., Hq * D : (Hq + Hkv) * D].view(B, S, Hkv, D)
        v = qkv[..., (Hq + Hkv) * D :].view(B, S, Hkv, D)
        ext = get_ext()
        qr = ext.rope_fwd(q, cos, sin, traditional, 0, False)
        kr = ext.rope_fwd(k, cos, sin, traditional, 0, False)
        o, lse = mask.fwd(ext, qr, kr, v, scale)
        mask.save(ctx, qkv, qr, kr, o, lse, cos, sin)
        ctx.meta = (Hq, Hkv, D, traditional, scale)
        return o

    @staticmethod
    def backward(ctx, do):
        mask, (qkv, qr, kr, o, lse, cos, sin) = _Mask.load(ctx)
        Hq, Hkv, D, traditional, scale = ctx.meta
        B, S, _ = qkv.shape
        ext = get_ext()
        v = qkv[..., (Hq + Hkv) * D :].view(B, S, Hkv, D)
        dqkv = torch.empty_like(qkv)
        dq_t = dqkv[..., : Hq * D].view(B, S, Hq, D)
        dk_t = dqkv[..., Hq * D : (Hq + Hkv) * D].view(B, S, Hkv, D)
        dv_t = dqkv[..., (Hq + Hkv) * D :].view(B, S, Hkv, D)
        none = torch.empty(0, dtype=qkv.dtype, device=qkv.device)
        dq_r, dk_r, _ = mask.bwd(ext, qr, kr, v, o, do, lse, scale, none, none.clone(), dv_t)
        ext.rope_fwd_out(dq_r, cos, sin, traditional, 0, True, dq_t)
        ext.rope_fwd_out(dk_r, cos, sin, traditional, 0, True, dk_t)
        return (dqkv,) + (None,) * 8


class _QKNormRopeAttnQKVFn(torch.autograd.Function):
    """_RopeAttnQKVFn with per-head QK-norm: fused qkv -> RMSNorm(q,k heads) ->
    RoPE -> flash attention, HIP path only.

    Forward: ONE qknorm_rope_fwd launch covers the q and k heads (they are
    adjacent in a token row; h < Hq picks the q weight) and replaces the two
    RoPE launches; the attention kernels run unchanged on its output. Backward:
    the attention backward writes dV into the dqkv buffer and the rotated
    dQ/dK side by side into one scratch tensor, then ONE qknorm_rope_bwd launch
    un-rotates, applies the norm backward from the saved qkv and the fp32 rstd,
    writes the dq|dk slices of dqkv and returns both weight gradients."""

    @staticmethod
    def forward(ctx, qkv, q_w, k_w, cos, sin, Hq, Hkv, D, eps, traditional, scale, mask):
        B, S, _ = qkv.shape
        scale = scale if scale is not None else 1.0 / math.sqrt(D)
        x = qkv[..., : (Hq + Hkv) * D].view(B, S, Hq + Hkv, D)
        v = qkv[..., (Hq + Hkv) * D :].view(B, S, Hkv, D)
        from .qk_norm import kernel_weight

        ext = get_ext()
        wq = kernel_weight(q_w, qkv.dtype)
        wk = kernel_weight(k_w, qkv.dtype)
        y, rstd = ext.qknorm_rope_fwd(x, Hq, wq, wk, cos, sin, traditional, 0, eps)
        qr, kr = y[:, :, :Hq], y[:, :, Hq:]
        o, lse = mask.fwd(ext, qr, kr, v, scale)
        mask.save(ctx, qkv, y, rstd, wq, wk, o, lse, cos, sin)
        ctx.meta = (Hq, Hkv, D, traditional, scale, q_w.dtype, k_w.dtype)
        return o

    @staticmethod
    def backward(ctx, do):
        mask, (qkv, y, rstd, wq, wk, o, lse, cos, sin) = _Mask.load(ctx)
        Hq, Hkv, D, traditional, scale, qw_dtype, kw_dtype = ctx.meta
        B, S, _ = qkv.shape
        ext = get_ext()
        x = qkv[..., : (Hq + Hkv) * D].view(B, S, Hq + Hkv, D)
        v = qkv[..., (Hq + Hkv) * D :].view(B, S, Hkv, D)
        qr, kr = y[:, :, :Hq], y[:, :, Hq:]
        dqkv = torch.empty_like(qkv)
        dqk_t = dqkv[..., : (Hq + Hkv) * D].view(B, S, Hq + Hkv, D)
        dv_t = dqkv[..., (Hq + Hkv) * D :].view(B, S, Hkv, D)
        g_r = torch.empty_like(y)  # rotated dq | dk
        dq_r, dk_r = g_r[:, :, :Hq], g_r[:, :, Hq:]
        mask.bwd(ext, qr, kr, v, o, do, lse, scale, dq_r, dk_r, dv_t)
        dw = ext.qknorm_rope_bwd(g_r, x, rstd, Hq, wq, wk, cos, sin, traditional, 0, dqk_t)
        return (dqkv, dw[0].to(qw_dtype), dw[1].to(kw_dtype)) + (None,) * 9


def rope_flash_attention_qkv(
    qkv: torch.Tensor,
    cos: torch.Tensor,
    sin: torch.Tensor,
    n_heads: int,
    n_kv_heads: int,
    head_dim: int,
    traditional: bool = False,
    causal: bool = True,
    scale: Optional[float] = None,
    window: Optional[int] = None,
    prefix_len: Optional[int] = None,
    alibi_slopes: Optional[torch.Tensor] = None,
    doc_start: Optional[torch.Tensor] = None,
    doc_end: Optional[torch.Tensor] = None,
    q_norm_weight: Optional[torch.Tensor] = None,
    k_norm_weight: Optional[torch.Tensor] = None,
    norm_eps: float = 1e-5,
    softcap: Optional[float] = None,
) -> torch.Tensor:
    """qkv: [B, S, (Hq+2*Hkv)*D] fused projection output -> o [B, S, Hq, D].

    HIP fast path (one fused autograd node, no grad cat); CPU falls back to
    the differentiable composition of the same ops. ``doc_start`` /
    ``doc_end``: packed-sequence document mask, see ``flash_attention``.

    ``q_norm_weight`` / ``k_norm_weight`` (``[head_dim]``, both or neither):
    per-head QK-norm before RoPE, see ``ops.qk_norm``. With both ``None`` the
    path is the plain RoPE + attention one.

    ``softcap``: attention-logit soft-capping, see ``flash_attention``; the
    fused nodes stay one autograd node each and call the capped kernels."""
    from .qk_norm import HIP_HEAD_DIMS, qk_norm_rope
    from .rope import apply_rope

    B, S, _ = qkv.shape
    Hq, Hkv, D = n_heads, n_kv_heads, head_dim
    mask = _Mask.build(causal, window, prefix_len, alibi_slopes, doc_start, doc_end,
                       B, S, S, Hq, qkv.device, softcap)
    if (q_norm_weight is None) != (k_norm_weight is None):
        raise ValueError("QK-norm needs both q_norm_weight and k_norm_weight")
    qk_norm = q_norm_weight is not None
    if (not qk_norm or D in HIP_HEAD_DIMS) and use_hip(qkv, dtypes=(torch.bfloat16,)):
        if qk_norm:
            return _QKNormRopeAttnQKVFn.apply(
                qkv, q_norm_weight, k_norm_weight, cos, sin, Hq, Hkv, D, float(norm_eps),
                traditional, scale, mask)
        return _RopeAttnQKVFn.apply(qkv, cos, sin, Hq, Hkv, D, traditional, scale, mask)
    q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    q, k = q.view(B, S, Hq, D), k.view(B, S, Hkv, D)
    if qk_norm:
        q, k = qk_norm_rope(q, k, q_norm_weight, k_norm_weight, cos, sin, norm_eps,
                            traditional, 0)
    else:
        q = apply_rope(q, cos, sin, traditional, 0)
        k = apply_rope(k, cos, sin, traditional, 0)
    return _FlashAttnFn.apply(q, k, v.view(B, S, Hkv, D), scale, mask)


def flex_attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    score_mod: Optional[Callable] = None,
    mask_mod: Optional[Callable] = None,
    block_mask=None,
    scale: Optional[float] = None,
) -> torch.Tensor:
    """Programmable attention (FlexAttention parity,
    /root/reference/models/attention/flex_attention.py:414-562).

    Named patterns route to the kernel (causal / sliding_window / prefix_lm /
    alibi via ``block_mask.pattern``). An arbitrary ``mask_mod`` on bf16 GPU
    inputs (or a ``CompiledBlockMask``) is compiled to device mask tensors
    and runs the MFMA kernels forward AND backward (MOD_BLOCKMASK in
    csrc/attn_fwd.hip / csrc/attn_bwd.hip), so it trains; an additive
    ``score_mod`` rides along as a precomputed bias. Everything else — CPU,
    other dtypes, a non-additive ``score_mod``, or a ``score_mod`` whose bias
    itself requires grad — runs the fp32 reference composition, which keeps
    correct gradients but materializes S x S scores.

    Limits of the trainable kernel path:
      * Every query row needs at least one live key. A fully masked row is
        0 * (1/0) in the forward kernel's epilogue and poisons that row's
        gradients; the reference composition zeroes such rows instead.
      * ``score_mod`` is evaluated ONCE into a bf16 [B, H, S, KV] bias that
        is kept for the backward: O(S^2) memory, and the bias (e.g. a
        learned table) gets no gradient on this path.
      * The mask tensors are laid out for the kernels' 256-row blocks
        (8 waves per block, forward and backward).
    """
    if isinstance(block_mask, CompiledBlockMask):
        return _flex_blockmask(q, k, v, block_mask, score_mod, scale)
    if block_mask is not None and score_mod is None and mask_mod is None:
        p = block_mask
        return flash_attention(
            q, k, v,
            causal=p.pattern in ("causal", "sliding_window", "alibi"),
            scale=scale,
            window=p.window if p.pattern == "sliding_window" else None,
            prefix_len=p.prefix_len if p.pattern == "prefix_lm" else None,
            alibi_slopes=getattr(p, "alibi_slopes", None),
        )
    if score_mod is None and mask_mod is None:
        return flash_attention(q, k, v, causal=True, scale=scale)
    if mask_mod is not None and q.is_cuda and q.dtype == torch.bfloat16:
        bm = CompiledBlockMask(mask_mod, q.shape[0], q.shape[2], q.shape[1],
                               k.shape[1], device=q.device)
        return _flex_blockmask(q, k, v, bm, score_mod, scale)
    return attention_ref(q, k, v, causal=False, scale=scale, score_mod=score_mod, mask_mod=mask_mod)


class _FlexBlockMaskFn(torch.autograd.Function):
    """attn_fwd_blockmask / attn_bwd_blockmask as one autograd node. ``bias``
    is the score_mod bias evaluated once by the caller (empty = none); it is
    saved for the backward, never recomputed, and gets no gradient."""

    @staticmethod
    def forward(ctx, q, k, v, bias, bm, scale):
        from ._ext import require_ext

        o, lse = require_ext().attn_fwd_blockmask(q, k, v, scale, bm.gran, bm.bits,
                                                  bm.range, bias)
        ctx.save_for_backward(q, k, v, o, lse, bias)
        ctx.bm, ctx.scale = bm, scale
        return o

    @staticmethod
    def backward(ctx, do):
        from ._ext import require_ext

        q, k, v, o, lse, bias = ctx.saved_tensors
        bm = ctx.bm
        dq, dk, dv = require_ext().attn_bwd_blockmask(
            q, k, v, o, do, lse, ctx.scale, bm.gran, bm.bits, bm.range, bm.qrange, bias)
        return dq, dk, dv, None, None, None


def _flex_blockmask(q, k, v, bm: "CompiledBlockMask", score_mod, scale):
    """Kernel-path flex: compiled mask tensors + (optional) a precomputed
    additive bias tensor for score_mod (evaluated vectorized once; the
    kernel adds it pre-softmax). With grads it runs as _FlexBlockMaskFn
    (HIP forward + backward); what the kernels cannot differentiate falls
    back to the fp32 composition."""
    from ._ext import require_ext

    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v))
    if needs_grad and not use_hip(q, k, v, dtypes=(torch.bfloat16,)):
        # CPU / non-bf16 training: the composition differentiates itself
        return attention_ref(q, k, v, causal=False, scale=scale, score_mod=score_mod,
                             mask_mod=bm._mask_mod)
    bias = torch.empty(0, dtype=torch.bfloat16, device=q.device)
    if score_mod is not None:
        B, S, H, D = q.shape
        KV = k.shape[1]
        qi = torch.arange(S, device=q.device).view(1, 1, S, 1)
        ki = torch.arange(KV, device=q.device).view(1, 1, 1, KV)
        bi = torch.arange(B, device=q.device).view(B, 1, 1, 1)
        hi = torch.arange(H, device=q.device).view(1, H, 1, 1)
        # the kernel consumes score_mod as an ADDITIVE bias (f(s) = s + f(0));
        # probe additivity on a small slice and fall back to the fp32
        # composition for non-additive mods (e.g. multiplicative scaling)
        sp, kp = min(S, 8), min(KV, 8)
        probe0 = torch.zeros(B, H, sp, kp, device=q.device)
        f0 = score_mod(probe0, bi, hi, qi[:, :, :sp], ki[:, :, :, :kp]).float()
        f1 = score_mod(probe0 + 1.0, bi, hi, qi[:, :, :sp], ki[:, :, :, :kp]).float()
        if not torch.allclose(f1 - f0, torch.ones_like(f0), atol=1e-4):
            return attention_ref(q, k, v, causal=False, scale=scale,
                                 score_mod=score_mod,
                                 mask_mod=getattr(bm, "_mask_mod", None))
        zero = torch.zeros(B, H, S, KV, device=q.device)
        bias = score_mod(zero, bi, hi, qi, ki)
        if needs_grad and bias.requires_grad:
            # the bias depends on a trainable tensor (e.g. a learned table):
            # the kernels give it no gradient, the composition does
            return attention_ref(q, k, v, causal=False, scale=scale,
                                 score_mod=score_mod,
                                 mask_mod=getattr(bm, "_mask_mod", None))
        bias = bias.detach().to(torch.bfloat16)
    if needs_grad:
        return _FlexBlockMaskFn.apply(q, k, v, bias, bm, float(scale))
    o, _ = require_ext().attn_fwd_blockmask(q, k, v, float(scale), bm.gran,
                                            bm.bits, bm.range, bias)
    return o


class BlockMask:
    """Named block-sparsity pattern (device-side block mask precompute lives in
    the kernel's block-skip logic; this object carries the pattern).

    Parity surface: create_block_mask
    (/root/reference/models/attention/flex_attention.py:356-411)."""

    def __init__(
        self,
        pattern: str = "causal",
        window: Optional[int] = None,
        prefix_len: Optional[int] = None,
        alibi_slopes: Optional[torch.Tensor] = None,
        block_size: int = 128,
    ):
        assert pattern in ("causal", "full", "sliding_window", "prefix_lm", "alibi")
        self.pattern = pattern
        self.window = window
        self.prefix_len = prefix_len
        self.alibi_slopes = alibi_slopes
        self.block_size = block_size


def _live_span(live: torch.Tensor) -> torch.Tensor:
    """bool [..., n] -> int32 [..., 2]: first / last+1 True index along the last
    dim, [0, 0] where there is none. Tensor ops only, no host sync."""
    n = live.shape[-1]
    idx = torch.arange(n, device=live.device)
    last = torch.where(live, idx + 1, 0).amax(-1)
    first = torch.where(live, idx, n).amin(-1) * (last > 0)
    return torch.stack([first, last], dim=-1).to(torch.int32)


class CompiledBlockMask:
    """An arbitrary ``mask_mod`` compiled into device tensors that drive the
    K1 kernel's block-skip / per-element-bit machinery (VERDICT r1 #5;
    parity: /root/reference/models/attention/flex_attention.py:356-411 —
    the reference SAMPLED block midpoints and then materialized full S x S
    scores anyway; here the mask is exact and only live kv-tile ranges are
    visited).

    Tensors (uint8/int32, tiny vs S^2 fp32):
      gran  [B,H,ceil(Q/32),ceil(KV/64)]  0 = granule fully masked,
                                          1 = partial (per-element bits),
                                          2 = fully live (mask-free path)
      bits  [B,H,Q,ceil(KV/8)]            packed keep bits
      range [B,H,ceil(Q/256),2]           first / last+1 live kv tile per
                                          256-row kernel block
      qrange [B,H,ceil(KV/256),2]         first / last+1 live 32-row q tile
                                          per 256-row kv block (backward:
                                          the dK/dV kernels' q loop bounds)
    """

    KVB = 64
    QPB = 256

    def __init__(self, mask_mod: Callable, B: int, H: int, Q_LEN: int, KV_LEN: int,
                 device="cuda"):
        self.B, self.H, self.Q_LEN, self.KV_LEN = B, H, Q_LEN, KV_LEN
        self._mask_mod = mask_mod  # kept for the non-additive score_mod fallback
        pad = torch.nn.functional.pad
        idx = lambda n: torch.arange(n, device=device)
        qi, ki = idx(Q_LEN), idx(KV_LEN)
        nq32 = (Q_LEN + 31) // 32
        nkv = (KV_LEN + self.KVB - 1) // self.KVB
        nqpb = (Q_LEN + self.QPB - 1) // self.QPB
        nkpb = (KV_LEN + self.QPB - 1) // self.QPB  # the backward's kv blocks
        self.gran = torch.zeros(B, H, nq32, nkv, dtype=torch.uint8, device=device)
        self.bits = torch.zeros(B, H, Q_LEN, (KV_LEN + 7) // 8, dtype=torch.uint8,
                                device=device)
        weights = (1 << torch.arange(8, device=device, dtype=torch.int32)).to(torch.uint8)
        # IN-RANGE elements per granule (the last granule row / column is ragged)
        in_range = ((Q_LEN - 32 * idx(nq32)).clamp(max=32).unsqueeze(1)
                    * (KV_LEN - self.KVB * idx(nkv)).clamp(max=self.KVB))
        for b in range(B):
            for h in range(H):
                keep = mask_mod(b, h, qi.unsqueeze(1), ki.unsqueeze(0))
                keep = keep.to(torch.bool).expand(Q_LEN, KV_LEN)  # [Q, KV], exact
                # zero-pad to whole 32-row / 64-col granules
                kp = pad(keep, (0, nkv * self.KVB - KV_LEN, 0, nq32 * 32 - Q_LEN))
                packed = (kp[:Q_LEN].reshape(Q_LEN, -1, 8).to(torch.uint8) *
                          weights).sum(-1).to(torch.uint8)
                self.bits[b, h] = packed[:, : (KV_LEN + 7) // 8]
                # granule codes; "full" requires every IN-RANGE element live
                live = kp.reshape(nq32, 32, nkv, self.KVB).sum(dim=(1, 3))
                self.gran[b, h] = (live > 0).to(torch.uint8) + (live == in_range).to(torch.uint8)
        any_live = self.gran > 0
        # per 256-row block: first/last live kv tile. Pad the granule rows to
        # whole blocks of 8 first — a reshape(nqpb, -1) misassigns rows
        # whenever ceil(Q/32) is not a multiple of 8 (caught by
        # tests/test_attention_cpu.py::..._bruteforce at Q=300).
        rows = pad(any_live, (0, 0, 0, nqpb * 8 - nq32)).reshape(B, H, nqpb, 8, nkv)
        self.range = _live_span(rows.any(dim=3))
        # transpose of range for the dK/dV kernels: per 256-row kv block
        # (4 granule columns), first/last+1 live 32-row q tile
        cols = pad(any_live, (0, nkpb * 4 - nkv)).reshape(B, H, nq32, nkpb, 4)
        self.qrange = _live_span(cols.any(dim=4).transpose(2, 3))


def create_block_mask(
    mask_mod: Optional[Callable] = None,
    B: int = 1,
    H: int = 1,
    Q_LEN: int = 0,
    KV_LEN: int = 0,
    pattern: str = "causal",
    device=None,
    **kwargs,
) -> BlockMask:
    """Named patterns return a pattern BlockMask (kernel block-skip handles
    them natively); an arbitrary ``mask_mod`` callable with a CUDA device is
    compiled to a CompiledBlockMask driving the kernel (else it stays a
    python callable for the fp32 reference path)."""
    if mask_mod is not None and Q_LEN and KV_LEN and device is not None             and torch.device(device).type == "cuda":
        return CompiledBlockMask(mask_mod, B, H, Q_LEN, KV_LEN, device=device)
    return BlockMask(pattern=pattern, **kwargs)
