#!/usr/bin/env python3
"""Cross-entropy of soft-capped logits: fused in the CE kernels against the
plain loss and against the unfused composition.

Forward + backward of the loss op alone at the 1B shape (N = 16 x 2048 rows,
V = 32000, bf16 logits), every fifth row ignored:
  plain    ops.fused_cross_entropy on the raw logits -> ce_fwd, ce_bwd
           (the loss without a cap: the baseline)
  capped   ops.cross_entropy_capped -> ce_cap_fwd, ce_cap_bwd: the cap
           t = c * tanh(x / c) is taken in registers
  unfused  ops.fused_cross_entropy(ops.softcap(x)) through autograd: the
           softcap_fwd / softcap_bwd kernels around the plain loss

The variants run in ONE process and alternate: each round times a window of
`--iters` forward+backward calls of each in turn, with device events around
the window and a synchronise on both sides, after a warm-up of all. The
per-call time of every window is kept, so the spread over the rounds is
visible next to the differences between the variants.

Bytes the algorithm must move per call, from the shapes: the forward reads the
logits twice (max pass, sum-exp pass), the backward reads them once and writes
dlogits once: 4 * N * V * itemsize, for plain and capped alike. The unfused
composition adds softcap's forward (read x, write y) and backward (read dy
and y, write dx): 9 of those units where the others move 4. The HBM fraction
printed for every variant uses the 4-unit figure: it is the rate at which the
variant gets the job of the fused loss done.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
HBM_PEAK = 8.0e12  # bytes/s, MI355X HBM3E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=16 * 2048)
    ap.add_argument("--V", type=int, default=32000)
    ap.add_argument("--cap", type=float, default=30.0)
    ap.add_argument("--mult", type=float, default=10.0,
                    help="logits are mult * randn: 10 with cap 30 puts |x / c| up to ~1.7")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=12, help="windows per variant")
    a = ap.parse_args()

    import torch

    sys.path.insert(0, str(ROOT))
    from mlx_cuda_distributed_pretraining_amd.ops import (
        cross_entropy_capped, fused_cross_entropy, require_ext, softcap,
    )

    assert torch.cuda.is_available(), "bench_softcap needs a GPU"
    require_ext()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    N, V = a.N, a.V
    leaf = (a.mult * torch.randn(N, V, device=dev)).to(torch.bfloat16).requires_grad_(True)
    tg = torch.randint(0, V, (N,), device=dev)
    tg[2::5] = -100

    def plain():
        leaf.grad = None
        loss, _ = fused_cross_entropy(leaf, tg, -100)
        loss.backward()

    def capped():
        leaf.grad = None
        ce, _z, _ = cross_entropy_capped(leaf, tg, a.cap, -100)
        ce.backward()

    def unfused():
        leaf.grad = None
        loss, _ = fused_cross_entropy(softcap(leaf, a.cap), tg, -100)
        loss.backward()

    variants = {"plain": plain, "capped": capped, "unfused": unfused}
    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()

    ms = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.iters)

    nbytes = 4 * N * V * leaf.element_size()
    out = {"shape": [N, V], "dtype": "bf16", "cap": a.cap, "mult": a.mult,
           "bytes_per_call": nbytes, "iters": a.iters, "rounds": a.rounds}
    for name, t in ms.items():
        med = statistics.median(t)
        out[name] = {"ms_median": med, "ms_min": min(t), "ms_max": max(t),
                     "spread_pct": 100.0 * (max(t) - min(t)) / med,
                     "bytes_per_s": nbytes / (med * 1e-3),
                     "hbm_fraction": nbytes / (med * 1e-3) / HBM_PEAK,
                     "ms_windows": [round(x, 4) for x in t]}
    out["capped_over_plain"] = out["capped"]["ms_median"] / out["plain"]["ms_median"]
    out["unfused_over_capped"] = out["unfused"]["ms_median"] / out["capped"]["ms_median"]
    print(json.dumps(out), flush=True)
    for name in variants:
        r = out[name]
        print(f"{name:7s}: {r['ms_median']:.3f} ms fwd+bwd (windows {r['ms_min']:.3f} - "
              f"{r['ms_max']:.3f}, spread {r['spread_pct']:.2f}%), "
              f"{r['bytes_per_s'] / 1e12:.2f} TB/s, {r['hbm_fraction'] * 100:.0f}% of HBM peak")
    print(f"capped / plain = {out['capped_over_plain']:.4f}, "
          f"unfused / capped = {out['unfused_over_capped']:.4f}")


if __name__ == "__main__":
    main()
