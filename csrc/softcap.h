// Final-logit soft-capping, t = c * tanh(x / c): the one definition that the
// capped cross-entropy kernels (cross_entropy.hip) and the elementwise kernels
// (softcap.hip) share, so a backward's p = e^(t - lse) is taken from the same
// t as the forward's lse.
#pragma once

#include "common.h"

// tanh(|u|) = (1 - q) / (1 + q) with q = e^(-2|u|) in [0, 1]: one v_exp_f32
// and one v_rcp_f32 (the only transcendental instructions; tanhf is a
// branching polynomial / exp routine several times as long) and no branch. q only
// ever underflows: past |u| ~ 44 it is 0 and the value is exactly 1, where
// the (e^u - e^-u) / (e^u + e^-u) and 1 - 2 / (e^2u + 1) forms run into
// inf / inf or need a range test. At u = 0, q = 1 and the value is exactly 0.
// The min keeps |t| <= c should the reciprocal of 1 + q round up.
//
// Error, absolute: q carries the 1 ulp of v_exp_f32 and |2u| * E of its
// argument (q * |2u| <= 1/e), d tanh / dq = -2 / (1 + q)^2 is at most 2 in
// size, the reciprocal is 1 ulp, and the two products, x * (1 / c) and
// c * tanh round once each (|u| * (1 - tanh^2 u) < 0.45). Measured on an
// MI355X against fp64 over the grid of tests/test_gpu_softcap.py: at most
// 3.08 units of E * c, E = 2^-24; the tests allow SOFTCAP_K = 4 x that.
__device__ __forceinline__ float softcap_tanh_abs(float u) {
  const float q = __expf(-2.f * fabsf(u));
  return fminf((1.f - q) * __builtin_amdgcn_rcpf(1.f + q), 1.f);
}

// inv_c = 1.f / c, divided once per thread by the caller
__device__ __forceinline__ float softcap_val(float x, float c, float inv_c) {
  return copysignf(c * softcap_tanh_abs(x * inv_c), x);
}

// d t / d x = 1 - (t / c)^2, from the capped value
__device__ __forceinline__ float softcap_dfac(float t, float inv_c) {
  const float r = t * inv_c;
  return fmaf(-r, r, 1.f);
}

// Attention-logit soft-capping (attn_fwd.hip, attn_bwd.hip, decode.hip): the
// kernels hold scores as raw q.k accumulators and exponentiate in base 2, so
// the cap travels pre-folded, computed once on the host:
//   t * log2(e) = softcap_val(acc, c2, sic)   with x = scale * acc
//   d t / d x   = softcap_dfac(t * log2(e), inv_c2)
// scale > 0, so acc carries the sign of x. One by-value kernel argument of
// the capped instantiations only (the trailing pack, as in cross_entropy.hip);
// it is wave-uniform and stays in SGPRs.
struct AttnCap {
  float c2;      // c * log2(e)
  float sic;     // scale / c
  float inv_c2;  // 1 / (c * log2(e))
};
inline AttnCap make_attn_cap(double cap, double scale) {
  constexpr double LOG2E_D = 1.4426950408889634;
  return {(float)(cap * LOG2E_D), (float)(scale / cap), (float)(1.0 / (cap * LOG2E_D))};
}
// the trailing cap argument of a CAP kernel; the others pass nothing
__device__ __forceinline__ AttnCap attn_cap_arg() { return {0.f, 0.f, 0.f}; }
__device__ __forceinline__ AttnCap attn_cap_arg(AttnCap c) { return c; }
