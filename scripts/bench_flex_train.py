#!/usr/bin/env python3
"""Trainable flex attention: forward+backward time and peak memory.

Three variants at the 1B attention shape (reduced batch) with the doc_band
mask (causal, 128-token band, 200-token documents; ~6% of S^2 kept at 2048):
  kernel   flex_attention(block_mask=CompiledBlockMask) — MOD_BLOCKMASK HIP
           kernels forward and backward (the mask is compiled once, outside
           the timed loop; its build time is reported separately)
  ref      attention_ref(mask_mod=...) under grad — what the same
           flex_attention(mask_mod=...) call ran before the kernels had a
           backward (fp32 composition, O(S^2) memory)
  causal   flash_attention(causal=True) — the dense-causal yardstick

Each variant runs in its own child process under its own `timeout`; the
first failing child ends the run. CUDA-event timing, median over repeats.
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
VARIANTS = ("kernel", "ref", "causal")


def doc_band(b, h, qi, ki):
    return (ki <= qi) & (qi - ki < 128) & (qi // 200 == ki // 200)


def child(a):
    import torch

    sys.path.insert(0, str(ROOT))
    from mlx_cuda_distributed_pretraining_amd.ops.attention import (
        CompiledBlockMask, attention_ref, flash_attention, flex_attention,
    )

    assert torch.cuda.is_available(), "bench_flex_train needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    q, k, v = (torch.randn(a.B, a.S, h, a.D, device=dev, dtype=torch.bfloat16,
                           requires_grad=True) for h in (a.Hq, a.Hkv, a.Hkv))
    dy = torch.randn(a.B, a.S, a.Hq, a.D, device=dev, dtype=torch.bfloat16)
    extra = {}
    if a.variant == "kernel":
        t0 = time.perf_counter()
        bm = CompiledBlockMask(doc_band, a.B, a.Hq, a.S, a.S, device=dev)
        torch.cuda.synchronize()
        extra["mask_build_ms"] = (time.perf_counter() - t0) * 1e3
        # doc_band is the same for every (b, h): count one plane's keep bits
        keep = (bm.bits[0, 0].to(torch.int32).unsqueeze(-1) >> torch.arange(8, device=dev)) & 1
        extra["kept_fraction"] = float(keep.sum()) / (a.S * a.S)
        del keep
        fn = lambda: flex_attention(q, k, v, block_mask=bm)  # noqa: E731
    elif a.variant == "ref":
        fn = lambda: attention_ref(q, k, v, causal=False, mask_mod=doc_band)  # noqa: E731
    else:
        fn = lambda: flash_attention(q, k, v, causal=True)  # noqa: E731

    def step():
        q.grad = k.grad = v.grad = None
        fn().backward(dy)

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    times = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    print(json.dumps({
        "variant": a.variant, "fwd_bwd_ms_median": statistics.median(times),
        "fwd_bwd_ms_min": min(times), "fwd_bwd_ms_max": max(times),
        "peak_mem_mib": torch.cuda.max_memory_allocated() / 2**20,
        "peak_over_inputs_mib": (torch.cuda.max_memory_allocated() - base) / 2**20,
        "shape": [a.B, a.S, a.Hq, a.Hkv, a.D], **extra,
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=VARIANTS)
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--S", type=int, default=2048)
    ap.add_argument("--Hq", type=int, default=16)
    ap.add_argument("--Hkv", type=int, default=16)
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per variant")
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
    kt, rt, ct = (res[x]["fwd_bwd_ms_median"] for x in VARIANTS)
    print(f"kernel {kt:.2f} ms / {res['kernel']['peak_mem_mib']:.0f} MiB peak | "
          f"fp32 ref {rt:.2f} ms / {res['ref']['peak_mem_mib']:.0f} MiB peak "
          f"({rt / kt:.1f}x slower) | dense causal {ct:.2f} ms "
          f"(kernel/causal = {kt / ct:.2f}, kept fraction "
          f"{res['kernel']['kept_fraction']:.3f})")


if __name__ == "__main__":
    main()
