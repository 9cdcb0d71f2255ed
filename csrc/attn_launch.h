// Host side of the tiled attention kernels, shared by attn_fwd.hip and
// attn_bwd.hip: argument validation, the [B,S,H,D] view rules, and the two
// run-time -> compile-time switches (head dim, mod code). Every entry point
// validates through here, so they all reject the same bad inputs; `who` is the
// entry point's name for the error text.
#pragma once
#include <torch/extension.h>
#include <cmath>
#include <type_traits>
#include "attn_common.h"
#include "softcap.h"

// Everything the attention kernels take, in one plain struct. It is filled by
// the checks below and unpacked at the one launch site of each kernel; the
// kernels keep individual __restrict__ parameters (pointers inside a by-value
// struct lose __restrict__, and these kernels sit at 233-256 VGPRs).
struct AttnArgs {
  const __hip_bfloat16 *q, *k, *v;
  const float* slopes = nullptr;  // MOD_ALIBI only: f32 [Hq]
  int B, Sq, Skv, Hq, Hkv, D;
  float scale;
  int modarg = 0;
  double cap = 0.;  // attention-logit soft-cap of the attn_cap_* entry points
  long q_rs, k_rs, v_rs;  // row strides of the [B,S,H,D] views (elements)
  // MOD_BLOCKMASK only (layouts: attn_fwd.hip); qrange is backward-only
  const unsigned char *gran = nullptr, *bits = nullptr;
  const int *range = nullptr, *qrange = nullptr;
  const __hip_bfloat16* bias = nullptr;
  // MOD_DOCUMENT only: int32 [B,S]; doc_end is backward-only
  const int *doc_start = nullptr, *doc_end = nullptr;
  // forward outputs / backward inputs
  __hip_bfloat16* o = nullptr;
  float* lse = nullptr;
  // backward only
  const __hip_bfloat16* dout = nullptr;
  __hip_bfloat16 *dq = nullptr, *dk = nullptr, *dv = nullptr;
  long do_rs = 0, dq_rs = 0, dk_rs = 0, dv_rs = 0;
};

inline const __hip_bfloat16* bf16_in(const at::Tensor& t) {
  return reinterpret_cast<const __hip_bfloat16*>(t.data_ptr());
}
inline __hip_bfloat16* bf16_out(const at::Tensor& t) {
  return reinterpret_cast<__hip_bfloat16*>(t.data_ptr());
}

// [B,S,H,D] views whose (h,d) inner block is contiguous are accepted as they
// are (e.g. slices of the fused QKV projection); anything else is materialized.
// Element (b,s,h,d) then sits at (b*S+s)*stride(1) + h*D + d.
inline bool bshd_inner_ok(const at::Tensor& t) {
  return t.stride(3) == 1 && t.stride(2) == t.size(3) &&
         t.stride(0) == t.size(1) * t.stride(1);
}
inline long bshd_row_stride(at::Tensor& t) {
  if (!bshd_inner_ok(t)) t = t.contiguous();
  return t.stride(1);
}

// f(std::integral_constant<int, D>) for the two compiled head dims
template <class F>
void with_head_dim(int D, F&& f) {
  if (D == 64) f(std::integral_constant<int, 64>{});
  else f(std::integral_constant<int, 128>{});
}

// f(std::integral_constant<int, MOD>) for the five run-time mod codes
template <class F>
void with_mod(const char* who, long mod, F&& f) {
  switch (mod) {
    case MOD_NONE: f(std::integral_constant<int, MOD_NONE>{}); break;
    case MOD_CAUSAL: f(std::integral_constant<int, MOD_CAUSAL>{}); break;
    case MOD_SLIDING_WINDOW: f(std::integral_constant<int, MOD_SLIDING_WINDOW>{}); break;
    case MOD_PREFIX_LM: f(std::integral_constant<int, MOD_PREFIX_LM>{}); break;
    case MOD_ALIBI: f(std::integral_constant<int, MOD_ALIBI>{}); break;
    default: TORCH_CHECK(false, who, ": unknown mod ", mod);
  }
}

// the three mod codes that have capped instantiations
template <class F>
void with_cap_mod(const char* who, long mod, F&& f) {
  switch (mod) {
    case MOD_NONE: f(std::integral_constant<int, MOD_NONE>{}); break;
    case MOD_CAUSAL: f(std::integral_constant<int, MOD_CAUSAL>{}); break;
    case MOD_SLIDING_WINDOW: f(std::integral_constant<int, MOD_SLIDING_WINDOW>{}); break;
    default:
      TORCH_CHECK(false, who, ": soft-capping is built for mod none, causal and sliding "
                  "window, got mod ", mod);
  }
}

// the soft-cap of the attn_cap_* entry points: finite and > 0, with a scale
// > 0 (the kernels take the sign of a capped score from the raw q.k)
inline void check_cap(const char* who, AttnArgs& a, double cap) {
  TORCH_CHECK(std::isfinite(cap) && cap > 0., who, ": cap must be finite and > 0, got ", cap);
  TORCH_CHECK(std::isfinite(a.scale) && a.scale > 0.f, who, ": soft-capping needs scale > 0, got ",
              a.scale);
  a.cap = cap;
}

inline bool shape_is(const at::Tensor& t, long a, long b, long c, long d) {
  return t.dim() == 4 && t.size(0) == a && t.size(1) == b && t.size(2) == c && t.size(3) == d;
}

// q/k/v of every entry point: bf16 [B,S,H,D] on one GPU, GQA-compatible head
// counts, head dim 64 or 128. Fills the dims, row strides and pointers.
inline AttnArgs check_qkv(const char* who, at::Tensor& q, at::Tensor& k, at::Tensor& v,
                          double scale) {
  TORCH_CHECK(q.is_cuda() && k.device() == q.device() && v.device() == q.device(),
              who, ": q/k/v must be on one GPU");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16 && k.scalar_type() == at::kBFloat16 &&
              v.scalar_type() == at::kBFloat16, who, ": bf16 only");
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.sizes() == k.sizes() &&
              k.size(0) == q.size(0) && k.size(3) == q.size(3),
              who, ": q/k/v must be [B,S,H,D] with one B and D, v shaped like k");
  AttnArgs a;
  a.B = q.size(0), a.Sq = q.size(1), a.Hq = q.size(2), a.D = q.size(3);
  a.Skv = k.size(1), a.Hkv = k.size(2);
  TORCH_CHECK(a.Hkv > 0 && a.Hq % a.Hkv == 0, who, ": GQA requires Hq % Hkv == 0");
  TORCH_CHECK(a.D == 64 || a.D == 128, who, ": head_dim must be 64 or 128, got ", a.D);
  a.q_rs = bshd_row_stride(q), a.k_rs = bshd_row_stride(k), a.v_rs = bshd_row_stride(v);
  a.q = bf16_in(q), a.k = bf16_in(k), a.v = bf16_in(v);
  a.scale = (float)scale;
  return a;
}

// the backward's o / dout / lse: shaped like q (lse f32 with B*Hq*Sq elements),
// on q's GPU; o and lse are made contiguous, dout keeps a row-strided view
inline void check_o_dout_lse(const char* who, AttnArgs& a, const at::Tensor& q, at::Tensor& o,
                             at::Tensor& dout, at::Tensor& lse) {
  TORCH_CHECK(o.device() == q.device() && dout.device() == q.device() &&
              lse.device() == q.device(), who, ": o/dout/lse must be on q's GPU");
  TORCH_CHECK(o.scalar_type() == at::kBFloat16 && dout.scalar_type() == at::kBFloat16,
              who, ": bf16 only");
  TORCH_CHECK(o.sizes() == q.sizes() && dout.sizes() == q.sizes(),
              who, ": o and dout must be shaped like q");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.numel() == (long)a.B * a.Hq * a.Sq,
              who, ": lse must be f32 [B,H,S]");
  a.do_rs = bshd_row_stride(dout);
  o = o.contiguous();
  lse = lse.contiguous();
  a.o = bf16_out(o), a.dout = bf16_in(dout), a.lse = lse.data_ptr<float>();
}

// An output of the backward: empty -> allocated here; otherwise a bf16
// [B,S,H,D] view on q's GPU with a contiguous (h,d) inner block (a slice of a
// fused dQKV grad buffer). Returns its row stride.
inline long check_out_view(const char* who, at::Tensor& t, const at::Tensor& q, int S, int H) {
  if (!t.defined() || t.numel() == 0) {
    t = at::empty({q.size(0), S, H, q.size(3)}, q.options());
  } else {
    TORCH_CHECK(t.device() == q.device() && t.scalar_type() == at::kBFloat16 &&
                    shape_is(t, q.size(0), S, H, q.size(3)) && bshd_inner_ok(t),
                who, ": bad out view");
  }
  return t.stride(1);
}

// MOD_ALIBI dereferences slopes[hq] for every q head; no other mod reads it
inline void check_slopes(const char* who, AttnArgs& a, long mod, const at::Tensor& slopes,
                         const at::Tensor& q) {
  if (mod != MOD_ALIBI) return;
  TORCH_CHECK(slopes.scalar_type() == at::kFloat && slopes.device() == q.device() &&
                  slopes.is_contiguous() && slopes.numel() == a.Hq,
              who, ": ALiBi slopes must be contiguous f32 [Hq] on q's device");
  a.slopes = slopes.data_ptr<float>();
}

// The compiled block mask (ops/attention.py CompiledBlockMask): granule codes,
// packed keep bits, per-q-block live kv ranges and the optional score bias.
inline void check_blockmask(const char* who, AttnArgs& a, const at::Tensor& q, at::Tensor& gran,
                            at::Tensor& bits, at::Tensor& range, at::Tensor& bias) {
  TORCH_CHECK(gran.scalar_type() == at::kByte && bits.scalar_type() == at::kByte &&
              range.scalar_type() == at::kInt, who, ": blockmask tensor dtypes");
  TORCH_CHECK(gran.device() == q.device() && bits.device() == q.device() &&
              range.device() == q.device(), who, ": blockmask tensors must be on q's GPU");
  TORCH_CHECK(shape_is(gran, a.B, a.Hq, cdiv(a.Sq, 32), cdiv(a.Skv, 64)),
              who, ": gran shape mismatch");
  TORCH_CHECK(shape_is(bits, a.B, a.Hq, a.Sq, cdiv(a.Skv, 8)), who, ": bits shape mismatch");
  TORCH_CHECK(shape_is(range, a.B, a.Hq, cdiv(a.Sq, 256), 2), who, ": range shape mismatch");
  gran = gran.contiguous();
  bits = bits.contiguous();
  range = range.contiguous();
  a.gran = gran.data_ptr<unsigned char>();
  a.bits = bits.data_ptr<unsigned char>();
  a.range = range.data_ptr<int>();
  if (bias.numel() > 0) {
    TORCH_CHECK(bias.device() == q.device() && bias.scalar_type() == at::kBFloat16 &&
                shape_is(bias, a.B, a.Hq, a.Sq, a.Skv), who, ": bias must be bf16 [B,H,Sq,Skv]");
    bias = bias.contiguous();
    a.bias = bf16_in(bias);
  }
}

// doc_start / doc_end of the document mask (training only: Sq == Skv)
inline const int* check_doc(const char* who, const AttnArgs& a, const at::Tensor& q,
                            const at::Tensor& t, const char* name) {
  TORCH_CHECK(a.Sq == a.Skv, who, ": document mask is training-only (Sq == Skv), got ",
              a.Sq, " vs ", a.Skv);
  TORCH_CHECK(t.scalar_type() == at::kInt && t.is_contiguous() && t.dim() == 2 &&
              t.size(0) == a.B && t.size(1) == a.Sq && t.device() == q.device(),
              who, ": ", name, " must be contiguous int32 [B,S] on q's device");
  return t.data_ptr<int>();
}
