#!/usr/bin/env python3
"""Per-head QK-norm + RoPE: the fused kernels against the unfused composition.

At the 1B shape (B x S x (Hq+Hkv) x D of configs/model-config-1b.yaml: 16 q
heads over 8 kv heads, D = 128, S = 2048, batch 16) on the q|k slice of one
fused QKV projection:
  fused      ops.qk_norm_rope -> ONE qknorm_rope_fwd launch forward, one
             qknorm_rope_bwd launch per tensor backward (csrc/qknorm_rope.hip)
  fused-2    the same again: the run-to-run spread
  unfused    existing kernels only: rms_norm on the q and k views (a gather to
             contiguous rows, then rmsnorm_fwd_kernel with one 256-thread
             workgroup per head_dim row), then rope_fwd, twice each; backward
             through the same ops' own backward kernels
  joint-bwd  the single-launch backward the fused attention node uses
             (qknorm_rope_bwd on the joint q|k view, dx into a strided slice)

Forward and forward+backward are timed separately (CUDA events, median over
repeats); backward = the difference. For the fused kernels the bytes the
algorithm must move (x in, y out, rstd; g and x in, dx out, rstd) over the
kernel time give the achieved HBM bandwidth, reported against the 8.0 TB/s
peak. Each variant runs in its own child process under its own `timeout`; the
first failing child ends the run.
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
VARIANTS = ("fused", "unfused", "fused-2", "joint-bwd")
HBM_PEAK = 8.0e12  # bytes/s, MI355X HBM3E


def timed(fn, warmup, repeats):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def child(a):
    import torch

    sys.path.insert(0, str(ROOT))
    from mlx_cuda_distributed_pretraining_amd.ops import (
        apply_rope, qk_norm_rope, require_ext, rms_norm,
    )
    from mlx_cuda_distributed_pretraining_amd.ops.rope import RopeTable

    assert torch.cuda.is_available(), "bench_qk_norm needs a GPU"
    ext = require_ext()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, S, Hq, Hkv, D = a.B, a.S, a.Hq, a.Hkv, a.D
    H = Hq + Hkv
    qkv = torch.randn(B, S, (Hq + 2 * Hkv) * D, device=dev, dtype=torch.bfloat16,
                      requires_grad=True)
    wq = (0.5 + torch.rand(D, device=dev)).to(torch.bfloat16).requires_grad_(True)
    wk = (0.5 + torch.rand(D, device=dev)).to(torch.bfloat16).requires_grad_(True)
    gq = torch.randn(B, S, Hq, D, device=dev, dtype=torch.bfloat16)
    gk = torch.randn(B, S, Hkv, D, device=dev, dtype=torch.bfloat16)
    cos, sin = RopeTable(D, 10000.0).get(S, dev, 0)
    eps = 1e-5

    def views():
        q, k, _ = qkv.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
        return q.view(B, S, Hq, D), k.view(B, S, Hkv, D)

    n_el = B * S * H * D
    rows = B * S * H
    out = {"variant": a.variant, "shape": [B, S, Hq, Hkv, D]}

    if a.variant == "joint-bwd":
        x = qkv.detach()[..., : H * D].view(B, S, H, D)
        g_r = torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16)
        dqkv = torch.empty_like(qkv)
        dx = dqkv[..., : H * D].view(B, S, H, D)
        wq_, wk_ = wq.detach(), wk.detach()
        _, rstd = ext.qknorm_rope_fwd(x, Hq, wq_, wk_, cos, sin, False, 0, eps)
        med, lo, hi = timed(lambda: ext.qknorm_rope_bwd(g_r, x, rstd, Hq, wq_, wk_, cos, sin,
                                                        False, 0, dx), a.warmup, a.repeats)
        nbytes = 3 * n_el * 2 + rows * 4
        out.update(bwd_ms_median=med, bwd_ms_min=lo, bwd_ms_max=hi, bwd_bytes=nbytes,
                   bwd_hbm_fraction=nbytes / (med * 1e-3) / HBM_PEAK)
        print(json.dumps(out), flush=True)
        return

    if a.variant.startswith("fused"):
        def fwd():
            q, k = views()
            return qk_norm_rope(q, k, wq, wk, cos, sin, eps)
    else:
        def fwd():
            q, k = views()
            return (apply_rope(rms_norm(q, wq, eps), cos, sin, False, 0),
                    apply_rope(rms_norm(k, wk, eps), cos, sin, False, 0))

    def fwd_only():
        with torch.no_grad():
            fwd()

    def fwd_bwd():
        qkv.grad = wq.grad = wk.grad = None
        qo, ko = fwd()
        torch.autograd.backward([qo, ko], [gq, gk])

    f_med, f_lo, f_hi = timed(fwd_only, a.warmup, a.repeats)
    fb_med, fb_lo, fb_hi = timed(fwd_bwd, a.warmup, a.repeats)
    out.update(fwd_ms_median=f_med, fwd_ms_min=f_lo, fwd_ms_max=f_hi,
               fwd_bwd_ms_median=fb_med, fwd_bwd_ms_min=fb_lo, fwd_bwd_ms_max=fb_hi,
               bwd_ms_median=fb_med - f_med)
    if a.variant.startswith("fused"):
        nbytes = 2 * n_el * 2 + rows * 4  # x in, y out, rstd out
        out.update(fwd_bytes=nbytes, fwd_hbm_fraction=nbytes / (f_med * 1e-3) / HBM_PEAK)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=VARIANTS)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--S", type=int, default=2048)
    ap.add_argument("--Hq", type=int, default=16)
    ap.add_argument("--Hkv", type=int, default=8)
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--timeout", type=int, default=180, help="seconds per variant")
    a = ap.parse_args()
    if a.variant:
        return child(a)
    res = {}
    for var in VARIANTS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, __file__,
               "--variant", var]
        for name in ("B", "S", "Hq", "Hkv", "D", "warmup", "repeats"):
            cmd += [f"--{name}", str(getattr(a, name))]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.exit(f"variant {var} failed with exit status {p.returncode}; stopping")
        res[var] = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps(res[var]), flush=True)
    f, u, f2, j = (res[v] for v in VARIANTS)
    print(f"fwd: fused {f['fwd_ms_median']:.3f} ms (again {f2['fwd_ms_median']:.3f}, "
          f"{f['fwd_hbm_fraction'] * 100:.0f}% of HBM peak) vs unfused "
          f"{u['fwd_ms_median']:.3f} ms ({u['fwd_ms_median'] / f['fwd_ms_median']:.2f}x) | "
          f"fwd+bwd: fused {f['fwd_bwd_ms_median']:.3f} ms (again "
          f"{f2['fwd_bwd_ms_median']:.3f}) vs unfused {u['fwd_bwd_ms_median']:.3f} ms "
          f"({u['fwd_bwd_ms_median'] / f['fwd_bwd_ms_median']:.2f}x) | joint bwd launch "
          f"{j['bwd_ms_median']:.3f} ms ({j['bwd_hbm_fraction'] * 100:.0f}% of HBM peak)")


if __name__ == "__main__":
    main()
