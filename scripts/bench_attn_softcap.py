#!/usr/bin/env python3
"""Attention-logit soft-capping: the capped attention kernels against the
uncapped ones and against the fp32 composition with a tanh score_mod.

Causal attention at the 1B shape (B = 4, S = 2048, 16 q heads over 8 kv heads,
D = 128, bf16), forward alone and forward + backward:
  plain    flash_attention(causal=True)              -> attn_fwd, attn_bwd
           (attention without a cap: the baseline)
  capped   flash_attention(causal=True, softcap=c)   -> attn_cap_fwd, attn_cap_bwd:
           c * tanh(score / c) taken in registers, one exp and one reciprocal
           more per score
  flex     flex_attention(score_mod=tanh cap, mask_mod=causal): what a model
           without the capped kernels has to run. A non-additive score_mod
           takes the fp32 composition (ops.attention_ref): S x S scores per
           head in memory, forward and backward through autograd.

The variants run in ONE process and alternate: each round times a window of
`--iters` calls of each in turn, with device events around the window and a
synchronise on both sides, after a warm-up of all. The per-call time of every
window is kept, so the spread over the rounds is visible next to the
differences between the variants.

FLOPs per call, from the shapes: causal attention does half of the 4 * B * Hq
* S^2 * D multiply-adds' flops in the forward (QK^T and PV) and 2.5 times that
in the backward; the TFLOP/s printed for plain and capped use these figures.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--S", type=int, default=2048)
    ap.add_argument("--Hq", type=int, default=16)
    ap.add_argument("--Hkv", type=int, default=8)
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--cap", type=float, default=50.0)
    ap.add_argument("--mult", type=float, default=3.0,
                    help="q is mult * randn: scores of standard deviation mult")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10, help="calls per timed window")
    ap.add_argument("--flex-iters", dest="flex_iters", type=int, default=2,
                    help="calls per timed window of the fp32 composition")
    ap.add_argument("--rounds", type=int, default=10, help="windows per variant")
    a = ap.parse_args()

    import torch

    sys.path.insert(0, str(ROOT))
    from mlx_cuda_distributed_pretraining_amd.ops import (
        flash_attention, flex_attention, require_ext,
    )

    assert torch.cuda.is_available(), "bench_attn_softcap needs a GPU"
    require_ext()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    q, k, v = (torch.randn(a.B, a.S, h, a.D, device=dev).mul_(m).to(torch.bfloat16)
               .requires_grad_(True)
               for h, m in ((a.Hq, a.mult), (a.Hkv, 1.0), (a.Hkv, 1.0)))
    dy = torch.randn(a.B, a.S, a.Hq, a.D, device=dev, dtype=torch.bfloat16)
    c = a.cap
    cap_mod = lambda s, b, h, qi, ki: c * torch.tanh(s / c)  # noqa: E731
    causal = lambda b, h, qi, ki: ki <= qi  # noqa: E731

    def forward(name):
        if name == "plain":
            return flash_attention(q, k, v, causal=True)
        if name == "capped":
            return flash_attention(q, k, v, causal=True, softcap=c)
        # the composition flex_attention ends in for a non-additive score_mod,
        # called directly: its per-call mask compile is left out of the timing
        from mlx_cuda_distributed_pretraining_amd.ops import attention_ref

        return attention_ref(q, k, v, causal=False, score_mod=cap_mod, mask_mod=causal)

    def fwd(name):
        with torch.no_grad():
            forward(name)

    def fwd_bwd(name):
        q.grad = k.grad = v.grad = None
        forward(name).backward(dy)

    # the composition behind flex_attention is what `flex` times: check once
    # that this score_mod really lands there (no kernel path for it)
    with torch.no_grad():
        o_flex = flex_attention(q, k, v, score_mod=cap_mod, mask_mod=causal)
        o_cap = forward("capped")
        err = float((o_flex.float() - o_cap.float()).abs().max())
    assert err < 3e-2, f"capped kernels and the flex composition disagree: {err}"

    names = ("plain", "capped", "flex")
    iters = {"plain": a.iters, "capped": a.iters, "flex": a.flex_iters}
    ms = {(n, what): [] for n in names for what in ("fwd", "fwd_bwd")}
    for what, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
        for n in names:
            for _ in range(a.warmup if n != "flex" else 1):
                fn(n)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for n in names:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(iters[n]):
                    fn(n)
                e1.record()
                torch.cuda.synchronize()
                ms[(n, what)].append(e0.elapsed_time(e1) / iters[n])

    fwd_flops = 0.5 * 4.0 * a.B * a.Hq * a.S * a.S * a.D
    flops = {"fwd": fwd_flops, "fwd_bwd": 3.5 * fwd_flops}
    out = {"shape": [a.B, a.S, a.Hq, a.Hkv, a.D], "dtype": "bf16", "cap": c, "mult": a.mult,
           "iters": iters, "rounds": a.rounds, "flex_vs_capped_max_abs_diff": err}
    for (n, what), t in ms.items():
        med = statistics.median(t)
        out[f"{n}_{what}"] = {"ms_median": med, "ms_min": min(t), "ms_max": max(t),
                              "spread_pct": 100.0 * (max(t) - min(t)) / med,
                              "tflops": flops[what] / (med * 1e-3) / 1e12,
                              "ms_windows": [round(x, 4) for x in t]}
    for what in ("fwd", "fwd_bwd"):
        out[f"capped_over_plain_{what}"] = (out[f"capped_{what}"]["ms_median"]
                                            / out[f"plain_{what}"]["ms_median"])
        out[f"flex_over_capped_{what}"] = (out[f"flex_{what}"]["ms_median"]
                                           / out[f"capped_{what}"]["ms_median"])
    print(json.dumps(out), flush=True)
    for what in ("fwd", "fwd_bwd"):
        for n in names:
            r = out[f"{n}_{what}"]
            print(f"{what:7s} {n:6s}: {r['ms_median']:.3f} ms (windows {r['ms_min']:.3f} - "
                  f"{r['ms_max']:.3f}, spread {r['spread_pct']:.2f}%), {r['tflops']:.0f} TFLOP/s")
        print(f"{what:7s} capped / plain = {out[f'capped_over_plain_{what}']:.4f}, "
              f"flex / capped = {out[f'flex_over_capped_{what}']:.2f}")


if __name__ == "__main__":
    main()
