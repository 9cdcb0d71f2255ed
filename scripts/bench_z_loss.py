#!/usr/bin/env python3
"""Cross-entropy with the auxiliary z-loss against the plain fused CE.

Forward + backward of the loss op alone at the 1B shape (N = 16 x 2048 rows,
V = 32000, bf16 logits), every fifth row ignored:
  plain   ops.fused_cross_entropy      -> ce_fwd, ce_bwd (the default path)
  z       ops.cross_entropy_with_z     -> ce_fwd_z, ce_bwd_z, backward through
          ce + coef * z

Both variants run in ONE process and alternate: each round times a window of
`--iters` forward+backward calls of plain, then of z, with device events
around the window and a synchronise on both sides, after a warm-up of both.
The per-call time of every window is kept, so the spread over the rounds is
visible next to the difference between the variants.

Bytes the algorithm must move per call, from the shapes: the forward reads the
logits twice (max pass, sum-exp pass), the backward reads them once and writes
dlogits once: 4 * N * V * itemsize (the [N] targets / lse vectors are under
0.1% of that and are not counted). Both variants move the same bytes.
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
    ap.add_argument("--coef", type=float, default=1e-4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=12, help="windows per variant")
    a = ap.parse_args()

    import torch

    sys.path.insert(0, str(ROOT))
    from mlx_cuda_distributed_pretraining_amd.ops import (
        cross_entropy_with_z, fused_cross_entropy, require_ext,
    )

    assert torch.cuda.is_available(), "bench_z_loss needs a GPU"
    require_ext()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    N, V = a.N, a.V
    leaf = torch.randn(N, V, device=dev, dtype=torch.bfloat16).requires_grad_(True)
    tg = torch.randint(0, V, (N,), device=dev)
    tg[2::5] = -100

    def plain():
        leaf.grad = None
        loss, _ = fused_cross_entropy(leaf, tg, -100)
        loss.backward()

    def with_z():
        leaf.grad = None
        ce, z, _ = cross_entropy_with_z(leaf, tg, -100)
        (ce + a.coef * z).backward()

    variants = {"plain": plain, "z": with_z}
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
    out = {"shape": [N, V], "dtype": "bf16", "bytes_per_call": nbytes,
           "iters": a.iters, "rounds": a.rounds}
    for name, t in ms.items():
        med = statistics.median(t)
        out[name] = {"ms_median": med, "ms_min": min(t), "ms_max": max(t),
                     "spread_pct": 100.0 * (max(t) - min(t)) / med,
                     "bytes_per_s": nbytes / (med * 1e-3),
                     "hbm_fraction": nbytes / (med * 1e-3) / HBM_PEAK,
                     "ms_windows": [round(x, 4) for x in t]}
    out["z_over_plain"] = out["z"]["ms_median"] / out["plain"]["ms_median"]
    print(json.dumps(out), flush=True)
    for name in variants:
        r = out[name]
        print(f"{name:5s}: {r['ms_median']:.3f} ms fwd+bwd (windows {r['ms_min']:.3f} - "
              f"{r['ms_max']:.3f}, spread {r['spread_pct']:.2f}%), "
              f"{r['bytes_per_s'] / 1e12:.2f} TB/s, {r['hbm_fraction'] * 100:.0f}% of HBM peak")
    print(f"z / plain = {out['z_over_plain']:.4f}")


if __name__ == "__main__":
    main()
