"""Tensor parallelism (TP) over RCCL/xGMI.

The reference exposes ``system.model_parallel`` config flags but its
``setup_model_parallelism`` logs "placeholder - not fully implemented yet"
(/root/reference/core/training.py:119-120, :1178-1193). This module makes
those flags real, the MI355X way: head-parallel attention and
intermediate-parallel MLP with ONE all-reduce per sublayer (Megatron f/g
pattern) — on an 8-GPU MI355X node the all-reduces ride point-to-point xGMI.

Mechanics
---------
- ``copy_to_tp`` ("f"): identity forward, all-reduce backward. Placed where a
  REPLICATED activation enters a column-parallel projection, so the
  replicated upstream modules (embeddings, norms) see the FULL gradient and
  stay bit-identical across ranks.
- ``reduce_from_tp`` ("g"): all-reduce forward, identity backward. Placed
  after the row-parallel projection whose rank-local output is a partial sum.
- ``apply_tensor_parallel(model, rank, world)`` shards an already-built (and
  broadcast) model IN PLACE:
    * ``wqkv``     rows -> local q heads + local kv heads (column-parallel),
    * ``wo``       columns -> local head outputs (row-parallel),
    * ``w_gate_up`` rows -> local gate slice + local up slice,
    * ``w_down``   columns -> the same local intermediate slice,
    * embeddings / norms / lm head stay replicated.
  Sharded parameters get ``p._tp_sharded = True`` so the gradient-norm
  reduction can count replicated params once (parallel/dist.py consumers).

Scope (round 1, all CPU-verified EXACT against single-process runs —
tests/test_tp_cpu.py; the collective pattern is backend-agnostic):
  * DPxTP meshes via ``init_tp_mesh`` (TP groups = adjacent ranks for xGMI
    locality; DP groups stride across replicas; gradient all-reduce rides
    the DP group only),
  * sequence parallelism (``gather_sp``/``scatter_sp``: S-sharded
    inter-sublayer activations),
  * expert parallelism for MoE (``_shard_experts``: replicated activations,
    sharded experts, router grads group-summed),
  * vocab-parallel lm head + CE (``vocab_parallel_cross_entropy`` /
    ``vp_embedding`` for tied models — no [B,S,V] logits replica),
  * per-shard TP checkpointing (trainer) + merge tool
    (tools/merge_tp_checkpoint.py).
"""
from __future__ import annotations

import torch
import torch.distributed as dist

# the TP process group (None = the default/world group). Set by
# init_tp_mesh() when TP degree < world size (DPxTP mesh).
_TP_GROUP = None


def set_tp_group(group) -> None:
    global _TP_GROUP
    _TP_GROUP = group


def _world() -> int:
    if not dist.is_initialized():
        return 1
    return dist.get_world_size(_TP_GROUP) if _TP_GROUP is not None else dist.get_world_size()


def tp_group():
    return _TP_GROUP


def init_tp_mesh(rank: int, world: int, tp: int):
    """Build the DPxTP mesh: TP groups are ADJACENT ranks (xGMI locality:
    the tp-degree peers of one model replica sit on one node's ring), DP
    groups stride across replicas. Returns (tp_rank, dp_rank, tp_pg, dp_pg).
    Every rank must call this (dist.new_group is collective)."""
    if world % tp:
        raise ValueError(f"world {world} not divisible by TP degree {tp}")
    dp = world // tp
    tp_pg = dp_pg = None
    if tp > 1 and tp < world:
        for d in range(dp):
            ranks = list(range(d * tp, (d + 1) * tp))
            g = dist.new_group(ranks)
            if rank in ranks:
                tp_pg = g
        for t in range(tp):
            ranks = list(range(t, world, tp))
            g = dist.new_group(ranks)
            if rank in ranks:
                dp_pg = g
        set_tp_group(tp_pg)
    return rank % tp, rank // tp, tp_pg, dp_pg


class _CopyToTP(torch.autograd.Function):
    """f: identity forward / all-reduce backward."""

    @staticmethod
    def forward(ctx, x: torch.Tensor) -> torch.Tensor:
        return x

    @staticmethod
    def backward(ctx, grad: torch.Tensor) -> torch.Tensor:
        if _world() > 1:
            grad = grad.contiguous()
            dist.all_reduce(grad, group=_TP_GROUP)
        return grad


class _ReduceFromTP(torch.autograd.Function):
    """g: all-reduce forward / identity backward."""

    @staticmethod
    def forward(ctx, x: torch.Tensor) -> torch.Tensor:
        if _world() > 1:
            x = x.contiguous()
            dist.all_reduce(x, group=_TP_GROUP)
        return x

    @staticmethod
    def backward(ctx, grad: torch.Tensor) -> torch.Tensor:
        return grad


def copy_to_tp(x: torch.Tensor) -> torch.Tensor:
    return _CopyToTP.apply(x)


def reduce_from_tp(x: torch.Tensor) -> torch.Tensor:
    return _ReduceFromTP.apply(x)


# ---- sequence parallelism (SP) on top of TP ----------------------------
# Between sublayers the activation stream is sharded on the SEQUENCE dim
# (norms + residual adds run on S/tp rows per rank); entering a
# column-parallel projection it is all-gathered (bwd: reduce-scatter of the
# per-rank partial grads), and the row-parallel output is reduce-scattered
# (bwd: all-gather). Same total comm volume as the f/g all-reduces, but the
# replicated norm/residual work and their activation memory shrink by tp.
# reduce-scatter is composed as all-reduce + local slice so the SAME code
# runs on gloo (CPU tests) and RCCL; a fused reduce_scatter_tensor fast
# path is a ROADMAP item.


def _sp_slice(x: torch.Tensor, rank: int, world: int) -> torch.Tensor:
    S = x.shape[1]
    loc = S // world
    return x[:, rank * loc:(rank + 1) * loc].contiguous()


def _sp_rank_world():
    if not dist.is_initialized():
        return 0, 1
    if _TP_GROUP is not None:
        return dist.get_rank(_TP_GROUP), dist.get_world_size(_TP_GROUP)
    return dist.get_rank(), dist.get_world_size()


def _all_gather_seq(x: torch.Tensor) -> torch.Tensor:
    _, world = _sp_rank_world()
    parts = [torch.empty_like(x) for _ in range(world)]
    dist.all_gather(parts, x.contiguous(), group=_TP_GROUP)
    return torch.cat(parts, dim=1)


def _reduce_scatter_seq(x: torch.Tensor) -> torch.Tensor:
    rank, world = _sp_rank_world()
    x = x.contiguous()
    # RCCL path: a real reduce_scatter moves 1/world the bytes of
    # all-reduce+slice (ROADMAP r1 #13). gloo has no reduce_scatter_tensor,
    # and the S dim must split evenly — fall back otherwise (identical
    # semantics, CPU tests run the fallback).
    backend = dist.get_backend(_TP_GROUP) if _TP_GROUP is not None else dist.get_backend()
    if str(backend) == "nccl" and x.shape[1] % world == 0:
        xt = x.movedim(1, 0).contiguous()  # scatter dim first
        out = torch.empty_like(xt[: xt.shape[0] // world])
        dist.reduce_scatter_tensor(out, xt, group=_TP_GROUP)
        return out.movedim(0, 1).contiguous()
    dist.all_reduce(x, group=_TP_GROUP)
    return _sp_slice(x, rank, world)


class _GatherSP(torch.autograd.Function):
    """S-sharded -> full: all-gather fwd, reduce-scatter bwd."""

    @staticmethod
    def forward(ctx, x: torch.Tensor) -> torch.Tensor:
        if _world() == 1:
            return x
        return _all_gather_seq(x)

    @staticmethod
    def backward(ctx, grad: torch.Tensor) -> torch.Tensor:
        if _world() == 1:
            return grad
        return _reduce_scatter_seq(grad)


class _ScatterSP(torch.autograd.Function):
    """partial-sum full -> S-sharded reduced: reduce-scatter fwd, all-gather bwd."""

    @staticmethod
    def forward(ctx, x: torch.Tensor) -> torch.Tensor:
        if _world() == 1:
            return x
        return _reduce_scatter_seq(x)

    @staticmethod
    def backward(ctx, grad: torch.Tensor) -> torch.Tensor:
        if _world() == 1:
            return grad
        return _all_gather_seq(grad)


def gather_sp(x: torch.Tensor) -> torch.Tensor:
    return _GatherSP.apply(x)


def scatter_sp(x: torch.Tensor) -> torch.Tensor:
    return _ScatterSP.apply(x)


def sp_allreduce_replicated_grads(model) -> None:
    """Under SP the replicated params (embeddings, norms, lm head) see only
    their local S-rows in backward: sum their grads over the TP group before
    the optimizer so the replicas move identically."""
    if _world() == 1:
        return
    for p in model.parameters():
        if p.grad is not None and not getattr(p, "_tp_sharded", False):
            dist.all_reduce(p.grad, group=_TP_GROUP)


def _shard_rows(weight: torch.nn.Parameter, row_idx: torch.Tensor) -> torch.nn.Parameter:
    p = torch.nn.Parameter(weight.detach()[row_idx].contiguous(),
                           requires_grad=weight.requires_grad)
    p._tp_sharded = True
    return p


def _shard_cols(weight: torch.nn.Parameter, lo: int, hi: int) -> torch.nn.Parameter:
    p = torch.nn.Parameter(weight.detach()[:, lo:hi].contiguous(),
                           requires_grad=weight.requires_grad)
    p._tp_sharded = True
    return p


def _localize_row_bias(linear: torch.nn.Linear, rank: int) -> None:
    if linear.bias is None:
        return
    if rank == 0:
        linear.bias._tp_sharded = True  # rank-local: clip reduces it over TP
    else:
        with torch.no_grad():
            linear.bias.zero_()
        linear.bias.requires_grad_(False)


def vp_embedding(tokens: torch.Tensor, weight: torch.Tensor, v0: int) -> torch.Tensor:
    """Embedding lookup over a VOCAB-SHARDED weight ([V/tp, H], this rank
    owning ids [v0, v0 + V/tp)): masked local lookup, zeros elsewhere, then
    the group sum assembles the full embedding on every rank. Backward is
    exact: each rank's weight shard receives grads only for its own ids
    (reduce_from_tp is identity in backward)."""
    lv = weight.shape[0]
    local = tokens - v0
    in_shard = (local >= 0) & (local < lv)
    safe = local.clamp(0, lv - 1)
    emb = torch.nn.functional.embedding(safe, weight)
    emb = emb * in_shard.unsqueeze(-1).to(emb.dtype)
    return reduce_from_tp(emb)


def _vp_group_lse(logits_local, targets, v0, ignore_index, cap=0.0):
    """The kernel passes and the two group reductions of the vocab-parallel
    forward: (mask, ntok, lse of the full row, target logit), all [N]. With a
    cap, all of the soft-capped row (ce_vp_cap_*)."""
    from ..ops._ext import require_ext

    ext = require_ext()
    mask = targets != ignore_index
    ntok = mask.sum()
    if cap:
        m, tgt_local = ext.ce_vp_cap_stats(logits_local, targets, v0, ignore_index, cap)
    else:
        m, tgt_local = ext.ce_vp_stats(logits_local, targets, v0, ignore_index)
    if _world() > 1:
        dist.all_reduce(m, op=dist.ReduceOp.MAX, group=_TP_GROUP)
    if cap:
        se_local = ext.ce_vp_cap_sumexp(logits_local, m, cap)
    else:
        se_local = ext.ce_vp_sumexp(logits_local, m)
    both = torch.stack([se_local, tgt_local])
    if _world() > 1:
        dist.all_reduce(both, group=_TP_GROUP)
    se, tgt = both[0], both[1]
    lse = m + torch.log(se)
    return mask, ntok, lse, tgt


class _VPCrossEntropyHIP(torch.autograd.Function):
    """Kernel-backed vocab-parallel CE (csrc/cross_entropy.hip ce_vp_*):
    two fused streaming passes over the bf16 shard (local max + target pick,
    then group-shifted sum-exp) with the two cross-rank reductions batched
    into one MAX and one SUM all-reduce; backward is one kernel writing the
    shard's softmax-minus-onehot gradient. The [N, V/tp] fp32 logits copy
    of the torch composition is never materialized (ROADMAP r1 #15)."""

    @staticmethod
    def forward(ctx, logits_local, targets, v0, ignore_index):
        mask, ntok, lse, tgt = _vp_group_lse(logits_local, targets, v0, ignore_index)
        loss_rows = torch.where(mask, lse - tgt, torch.zeros_like(lse))
        ntok_f = ntok.clamp(min=1).float()
        loss = loss_rows.sum() / ntok_f
        ctx.save_for_backward(logits_local, targets, lse, ntok_f)
        ctx.v0 = v0
        ctx.ignore_index = ignore_index
        return loss, ntok

    @staticmethod
    def backward(ctx, gloss, _gntok):
        from ..ops._ext import require_ext

        logits_local, targets, lse, ntok_f = ctx.saved_tensors
        scale = (gloss.float() / ntok_f).reshape(1)
        dl = require_ext().ce_vp_bwd(logits_local, targets, lse, scale.contiguous(),
                                     ctx.v0, ctx.ignore_index)
        return dl, None, None, None


class _VPCrossEntropyZHIP(torch.autograd.Function):
    """_VPCrossEntropyHIP with the auxiliary z-loss: the same forward passes
    (z = mean lse^2 comes from the group lse vector they assemble), and one
    ce_vp_bwd_z launch that takes the upstream gradients of both means."""

    @staticmethod
    def forward(ctx, logits_local, targets, v0, ignore_index):
        mask, ntok, lse, tgt = _vp_group_lse(logits_local, targets, v0, ignore_index)
        zero = torch.zeros_like(lse)
        ntok_f = ntok.clamp(min=1).float()
        loss = torch.where(mask, lse - tgt, zero).sum() / ntok_f
        z = torch.where(mask, lse * lse, zero).sum() / ntok_f
        ctx.save_for_backward(logits_local, targets, lse, ntok_f)
        ctx.v0 = v0
        ctx.ignore_index = ignore_index
        ctx.mark_non_differentiable(ntok)
        return loss, z, ntok

    @staticmethod
    def backward(ctx, gloss, gz, _gntok):
        from ..ops._ext import require_ext

        logits_local, targets, lse, ntok_f = ctx.saved_tensors
        scale_ce = (gloss.float() / ntok_f).reshape(1)
        scale_z = (2.0 * gz.float() / ntok_f).reshape(1)
        dl = require_ext().ce_vp_bwd_z(logits_local, targets, lse, scale_ce, scale_z,
                                       ctx.v0, ctx.ignore_index)
        return dl, None, None, None


class _VPCrossEntropyCapHIP(torch.autograd.Function):
    """_VPCrossEntropyZHIP of the soft-capped logits cap * tanh(l / cap): the
    ce_vp_cap_* kernels cap the shard in registers. There is one capped
    variant, so z is always computed (a zero upstream gradient of z leaves
    the pure capped CE)."""

    @staticmethod
    def forward(ctx, logits_local, targets, v0, ignore_index, cap):
        mask, ntok, lse, tgt = _vp_group_lse(logits_local, targets, v0, ignore_index, cap)
        zero = torch.zeros_like(lse)
        ntok_f = ntok.clamp(min=1).float()
        loss = torch.where(mask, lse - tgt, zero).sum() / ntok_f
        z = torch.where(mask, lse * lse, zero).sum() / ntok_f
        ctx.save_for_backward(logits_local, targets, lse, ntok_f)
        ctx.v0 = v0
        ctx.ignore_index = ignore_index
        ctx.cap = cap
        ctx.mark_non_differentiable(ntok)
        return loss, z, ntok

    @staticmethod
    def backward(ctx, gloss, gz, _gntok):
        from ..ops._ext import require_ext

        logits_local, targets, lse, ntok_f = ctx.saved_tensors
        scale_ce = (gloss.float() / ntok_f).reshape(1)
        scale_z = (2.0 * gz.float() / ntok_f).reshape(1)
        dl = require_ext().ce_vp_cap_bwd(logits_local, targets, lse, scale_ce, scale_z,
                                         ctx.v0, ctx.ignore_index, ctx.cap)
        return dl, None, None, None, None


def vocab_parallel_cross_entropy(logits_local: torch.Tensor, targets: torch.Tensor,
                                 v0: int, ignore_index: int = -100, with_z: bool = False,
                                 softcap: float = 0.0):
    """Cross entropy over VOCAB-SHARDED logits ([N, V/tp] on each rank,
    this rank owning vocab ids [v0, v0 + V/tp)). Returns (mean_loss, ntok)
    — numerically the full-vocab CE, but the [N, V] logits replica never
    exists. ``with_z=True`` returns (mean_loss, z, ntok), z being the mean of
    lse^2 over the counted rows (the auxiliary z-loss; ops/cross_entropy.py).
    ``softcap = c > 0`` takes the loss of the soft-capped logits
    c * tanh(l / c) (ops.cross_entropy_capped): in the ce_vp_cap_* kernels on
    the HIP path, on the capped shard in the torch composition.
    Composition keeps autograd exact: the logsumexp shift uses a
    DETACHED group max (lse is shift-invariant), and the cross-rank sums go
    through reduce_from_tp (sum forward / identity backward), so each
    rank's backward produces exactly its shard of the softmax-minus-onehot
    gradient."""
    if softcap:
        from ..ops.softcap import check_cap

        softcap = check_cap(softcap)
    if (logits_local.is_cuda and logits_local.dtype == torch.bfloat16
            and logits_local.is_contiguous() and logits_local.shape[1] % 8 == 0):
        if softcap:
            loss, z, ntok = _VPCrossEntropyCapHIP.apply(
                logits_local, targets.contiguous(), int(v0), int(ignore_index), softcap)
            return (loss, z, ntok) if with_z else (loss, ntok)
        if with_z:
            return _VPCrossEntropyZHIP.apply(logits_local, targets.contiguous(), int(v0),
                                             int(ignore_index))
        return _VPCrossEntropyHIP.apply(logits_local, targets.contiguous(), int(v0),
                                        int(ignore_index))
    lf = logits_local.float()
    if softcap:
        lf = softcap * torch.tanh(lf / softcap)
    n, v_loc = lf.shape
    mask = targets != ignore_index
    ntok = mask.sum()

    with torch.no_grad():
        m = lf.max(dim=-1).values
        if _world() > 1:
            m = m.contiguous()
            dist.all_reduce(m, op=dist.ReduceOp.MAX, group=_TP_GROUP)
    se_local = torch.exp(lf - m.unsqueeze(-1)).sum(-1, keepdim=False)
    se = reduce_from_tp(se_local.unsqueeze(0)).squeeze(0)
    lse = m + torch.log(se)

    t_local = targets.clamp(min=0) - v0
    in_shard = mask & (t_local >= 0) & (t_local < v_loc)
    safe = t_local.clamp(0, v_loc - 1)
    picked = lf.gather(-1, safe.unsqueeze(-1)).squeeze(-1)
    tgt_local = torch.where(in_shard, picked, torch.zeros_like(picked))
    tgt = reduce_from_tp(tgt_local.unsqueeze(0)).squeeze(0)

    loss_rows = torch.where(mask, lse - tgt, torch.zeros_like(lse))
    loss = loss_rows.sum() / ntok.clamp(min=1).float()
    if with_z:
        z = torch.where(mask, lse * lse, torch.zeros_like(lse)).sum() / ntok.clamp(min=1).float()
        return loss, z, ntok
    return loss, ntok


def _shard_experts(moe, rank: int, world: int, sequence_parallel: bool) -> None:
    """Expert parallelism for MoE layers inside the model-parallel group:
    experts are sharded across ranks while activations stay replicated, so
    routing needs NO all-to-all — each rank computes its local experts'
    contributions for every token and the row-parallel g all-reduce sums
    them (capacity-bound token dispatch with a real all-to-all is the
    bandwidth-optimal follow-up, ROADMAP).

    The ROUTER stays replicated but its gradient is PARTIAL per rank (each
    rank only backprops its local experts' gate terms) -> the trainer sums
    router grads over the group (ep_allreduce_router_grads). The aux
    load-balance loss is computed identically on every rank, so MoE.forward
    pre-divides it by the EP degree to survive that sum unscaled.

    Under sequence parallelism the MoE gathers the S-shard first
    (gather_sp) and scatters the reduced output back (scatter_sp) — exact,
    at the cost of momentarily holding the full activation for the MoE
    block (token-level dispatch without the gather is the all-to-all
    follow-up, ROADMAP)."""
    E = moe.num_experts
    if E % world:
        raise ValueError(f"EP degree {world} must divide num_local_experts={E}")
    le = E // world
    moe.w_gate_up = torch.nn.Parameter(
        moe.w_gate_up.detach()[rank * le:(rank + 1) * le].contiguous())
    moe.w_down = torch.nn.Parameter(
        moe.w_down.detach()[rank * le:(rank + 1) * le].contiguous())
    moe.w_gate_up._tp_sharded = True
    moe.w_down._tp_sharded = True
    moe.router.weight._ep_router = True  # grads summed over the group
    moe._ep_rank, moe._ep_world = rank, world
    moe._tp = True
    # SP: the block hands the MLP an S-SHARD; MoE gathers it (all-gather fwd
    # / reduce-scatter bwd), runs the replicated-activation EP body, and
    # reduce-scatters the partial-sum output back to the shard.
    moe._sp = sequence_parallel


def ep_allreduce_router_grads(model) -> None:
    """Sum the (partial) router gradients of EP MoE layers over the TP
    group after backward — see _shard_experts."""
    if _world() == 1:
        return
    for p in model.parameters():
        if p.grad is not None and getattr(p, "_ep_router", False):
            dist.all_reduce(p.grad, group=_TP_GROUP)


def apply_tensor_parallel(model, rank: int, world: int,
                          sequence_parallel: bool = False) -> None:
    """Shard a fully-initialized (broadcast) Llama ``Model`` in place.
    sequence_parallel: activations between sublayers are S-sharded during
    TRAINING forward (gather_sp/scatter_sp replace the f/g all-reduces)."""
    if world <= 1:
        return
    args = model.args
    if getattr(args, "qk_norm", False):
        raise NotImplementedError(
            "tensor/sequence parallelism with qk_norm is not supported yet: the "
            "[head_dim] q_norm/k_norm weights are replicated while the heads are "
            "sharded, so every rank holds a partial gradient that needs an "
            "all-reduce over the TP group (ROADMAP) - train qk_norm models with "
            "data parallelism"
        )
    if args.num_heads % world or args.num_kv_heads % world:
        raise ValueError(
            f"TP degree {world} must divide num_heads={args.num_heads} and "
            f"num_kv_heads={args.num_kv_heads}"
        )
    if args.intermediate_size % world:
        raise ValueError(f"TP degree {world} must divide intermediate_size")
    hd = args.head_dim
    hq, hkv = args.num_heads, args.num_kv_heads
    lq, lkv = hq // world, hkv // world
    inter = args.intermediate_size
    li = inter // world

    for layer in model.layers:
        attn = layer.attention
        # wqkv rows: [q(hq*hd) | k(hkv*hd) | v(hkv*hd)] -> local sections
        dev = attn.wqkv.weight.device
        q_rows = torch.arange(rank * lq * hd, (rank + 1) * lq * hd, device=dev)
        k_rows = hq * hd + torch.arange(rank * lkv * hd, (rank + 1) * lkv * hd, device=dev)
        v_rows = (hq + hkv) * hd + torch.arange(rank * lkv * hd, (rank + 1) * lkv * hd,
                                                device=dev)
        rows = torch.cat([q_rows, k_rows, v_rows])
        attn.wqkv.weight = _shard_rows(attn.wqkv.weight, rows)
        if attn.wqkv.bias is not None:
            attn.wqkv.bias = _shard_rows(attn.wqkv.bias, rows)
        attn.wo.weight = _shard_cols(attn.wo.weight, rank * lq * hd, (rank + 1) * lq * hd)
        # row-parallel bias: FULL bias on tp-rank 0, zero + FROZEN elsewhere.
        # (1/tp-scaling on every rank is wrong under optimizers: each rank
        # applies a full-magnitude update, so the summed bias moves at tp x
        # the learning rate — and Adam's scale-invariance defeats
        # grad-rescaling tricks.) Rank 0's bias is flagged _tp_sharded so the
        # clip norm reduces it across the TP group consistently.
        _localize_row_bias(attn.wo, rank)
        attn.n_heads, attn.n_kv_heads = lq, lkv
        attn.wqkv.out_features = (lq + 2 * lkv) * hd
        attn.wo.in_features = lq * hd
        if attn.alibi_slopes is not None:
            attn.alibi_slopes = attn.alibi_slopes[rank * lq:(rank + 1) * lq].contiguous()
        attn._tp = True

        mlp = layer.mlp
        if hasattr(mlp, "num_experts"):  # MoE: expert parallelism
            _shard_experts(mlp, rank, world, sequence_parallel)
            continue
        g_rows = torch.arange(rank * li, (rank + 1) * li, device=dev)
        u_rows = inter + g_rows
        mlp.w_gate_up.weight = _shard_rows(mlp.w_gate_up.weight, torch.cat([g_rows, u_rows]))
        mlp.w_down.weight = _shard_cols(mlp.w_down.weight, rank * li, (rank + 1) * li)
        if mlp.w_gate_up.bias is not None:
            mlp.w_gate_up.bias = _shard_rows(mlp.w_gate_up.bias, torch.cat([g_rows, u_rows]))
        _localize_row_bias(mlp.w_down, rank)
        mlp.w_gate_up.out_features = 2 * li
        mlp.w_down.in_features = li
        mlp._tp = True
        attn._sp = mlp._sp = sequence_parallel

    # vocab-parallel lm head (V % tp == 0, non-SP): the [B,S,V] logits
    # replica never materializes — the trainer computes
    # vocab_parallel_cross_entropy on the shard (Megatron-style).
    # Tied models shard the EMBEDDING weight (shared with the head); the
    # lookup becomes masked-local + group sum (vp_embedding).
    model._vp_vocab0 = -1
    if not sequence_parallel and args.vocab_size % world == 0:
        V = args.vocab_size
        lv = V // world
        rows = None  # torch.arange built per tensor for device correctness
        if hasattr(model, "output"):
            w = model.output.weight
            model.output.weight = _shard_rows(
                w, torch.arange(rank * lv, (rank + 1) * lv, device=w.device))
            model.output.out_features = lv
            model._vp_vocab0 = rank * lv
        elif args.tie_word_embeddings:
            w = model.tok_embeddings.weight
            model.tok_embeddings.weight = _shard_rows(
                w, torch.arange(rank * lv, (rank + 1) * lv, device=w.device))
            model.tok_embeddings.num_embeddings = lv
            model._vp_vocab0 = rank * lv
    model._tp_world = world
    model._sp_world = world if sequence_parallel else 1
