#!/usr/bin/env python3
"""Document-masked attention for packed sequences: forward+backward time.

Variants at the 1B attention shape (S = 2048, D = 128, 16 q heads over 8 kv
heads as in configs/model-config-1b.yaml, reduced batch):
  causal      flash_attention(causal=True) — the yardstick, unchanged kernels
  causal-2    the same again: the run-to-run spread of the yardstick
  doc-single  flash_attention(doc_start=zeros) — one document per row, so the
              same mask as causal: the pure overhead of MOD_DOCUMENT
  doc-packed  flash_attention(doc_start=...) with seeded random document
              lengths (exponential, mean --mean-len tokens, at least 1); the
              kept fraction of S^2 is reported (causal keeps ~0.5)
  blockmask   the same packed mask through flex_attention(block_mask=
              CompiledBlockMask(...)); the per-batch mask build time is
              reported separately (it is outside the timed loop)

Each variant runs in its own child process under its own `timeout`; the
first failing child ends the run. CUDA-event timing, median over repeats.
"""
import argparse
import json
import random
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
VARIANTS = ("causal", "causal-2", "doc-single", "doc-packed", "blockmask")


def packed_doc_start(B, S, mean_len, seed):
    """seeded exponential document lengths -> int32 [B, S] doc_start (CPU)"""
    import torch

    rng = random.Random(seed)
    out = torch.zeros(B, S, dtype=torch.int32)
    lens = []
    for b in range(B):
        pos = 0
        while pos < S:
            n = min(max(1, int(round(rng.expovariate(1.0 / mean_len)))), S - pos)
            out[b, pos:pos + n] = pos
            lens.append(n)
            pos += n
    return out, lens


def child(a):
    import torch

    sys.path.insert(0, str(ROOT))
    from mlx_cuda_distributed_pretraining_amd.ops.attention import (
        CompiledBlockMask, flash_attention, flex_attention,
    )

    assert torch.cuda.is_available(), "bench_doc_mask needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    q, k, v = (torch.randn(a.B, a.S, h, a.D, device=dev, dtype=torch.bfloat16,
                           requires_grad=True) for h in (a.Hq, a.Hkv, a.Hkv))
    dy = torch.randn(a.B, a.S, a.Hq, a.D, device=dev, dtype=torch.bfloat16)
    extra = {}
    if a.variant in ("doc-packed", "blockmask"):
        ds_cpu, lens = packed_doc_start(a.B, a.S, a.mean_len, a.seed)
        doc_start = ds_cpu.to(dev)
        idx = torch.arange(a.S).view(1, a.S)
        extra["kept_fraction"] = float((idx - ds_cpu + 1).sum()) / (a.B * a.S * a.S)
        extra["documents"] = len(lens)
        extra["mean_doc_len"] = sum(lens) / len(lens)
    if a.variant.startswith("causal"):
        fn = lambda: flash_attention(q, k, v, causal=True)  # noqa: E731
    elif a.variant == "doc-single":
        zeros = torch.zeros(a.B, a.S, dtype=torch.int32, device=dev)
        full = torch.full((a.B, a.S), a.S, dtype=torch.int32, device=dev)
        fn = lambda: flash_attention(q, k, v, doc_start=zeros, doc_end=full)  # noqa: E731
    elif a.variant == "doc-packed":
        from mlx_cuda_distributed_pretraining_amd.ops.attention import document_bounds

        # both tensors through the public builder, as the trainer does: a
        # token row with a BOS (id 0) wherever a document starts
        ds2, doc_end = document_bounds((ds_cpu != idx).long().to(dev), bos_id=0)
        assert torch.equal(ds2, doc_start)
        fn = lambda: flash_attention(q, k, v, doc_start=doc_start, doc_end=doc_end)  # noqa: E731
    else:
        def mask_mod(b, h, qi, ki):
            return (ki <= qi) & (ki >= doc_start[int(b)].view(a.S, 1))

        t0 = time.perf_counter()
        bm = CompiledBlockMask(mask_mod, a.B, a.Hq, a.S, a.S, device=dev)
        torch.cuda.synchronize()
        extra["mask_build_ms"] = (time.perf_counter() - t0) * 1e3
        fn = lambda: flex_attention(q, k, v, block_mask=bm)  # noqa: E731

    def step():
        q.grad = k.grad = v.grad = None
        fn().backward(dy)

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
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
        "shape": [a.B, a.S, a.Hq, a.Hkv, a.D], **extra,
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=VARIANTS)
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--S", type=int, default=2048)
    ap.add_argument("--Hq", type=int, default=16)
    ap.add_argument("--Hkv", type=int, default=8)
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--mean-len", dest="mean_len", type=int, default=256,
                    help="mean document length of the packed variants")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=180, help="seconds per variant")
    a = ap.parse_args()
    if a.variant:
        return child(a)
    res = {}
    for var in VARIANTS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, __file__,
               "--variant", var]
        for name in ("B", "S", "Hq", "Hkv", "D", "seed", "warmup", "repeats"):
            cmd += [f"--{name}", str(getattr(a, name))]
        cmd += ["--mean-len", str(a.mean_len)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.exit(f"variant {var} failed with exit status {p.returncode}; stopping")
        res[var] = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps(res[var]), flush=True)
    t = {x: res[x]["fwd_bwd_ms_median"] for x in VARIANTS}
    c = t["causal"]
    print(f"causal {c:.3f} ms (again {t['causal-2']:.3f}, spread "
          f"{abs(t['causal-2'] - c) / c * 100:.1f}%) | doc-single {t['doc-single']:.3f} ms "
          f"({t['doc-single'] / c:.3f}x) | doc-packed {t['doc-packed']:.3f} ms "
          f"({t['doc-packed'] / c:.3f}x, kept {res['doc-packed']['kept_fraction']:.3f}, "
          f"mean doc {res['doc-packed']['mean_doc_len']:.0f}) | blockmask "
          f"{t['blockmask']:.3f} ms ({t['blockmask'] / c:.3f}x) + "
          f"{res['blockmask']['mask_build_ms']:.0f} ms mask build per batch")


if __name__ == "__main__":
    main()
