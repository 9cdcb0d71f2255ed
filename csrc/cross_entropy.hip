// Fused cross-entropy over the vocab with pad masking (kernel K6).
// Replaces /root/reference/core/training.py:1222-1234. One workgroup per row;
// two passes (max, then sum-exp) over the bf16 logits with fp32 accumulation —
// the fp32 logits are never materialized. Backward writes
// dlogits = (softmax - onehot) * scale in one streaming pass.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPException.h>
#include "common.h"
#include "softcap.h"

namespace {

// the trailing cap argument of a CAP kernel; the others pass nothing
__device__ __forceinline__ float cap_arg() { return 0.f; }
__device__ __forceinline__ float cap_arg(float c) { return c; }

// the logit as the loss sees it: capped when CAP, as stored otherwise
template <bool CAP>
__device__ __forceinline__ float capped(float x, float c, float inv_c) {
  if constexpr (CAP) return softcap_val(x, c, inv_c);
  return x;
}

// Z adds the auxiliary z-loss sum: lse^2 over the counted rows, squared in
// fp32 from the lse that is stored, into a second partial per block that goes
// through the same fixed-order reduction as the loss. Without Z the kernel is
// the plain forward, instruction for instruction.
//
// CAP: the row is the capped one, t = c * tanh(x / c) (softcap_val), and the
// cap travels as one trailing float argument (cap...), which the other
// instantiations do not have at all: their argument block is what it was.
// tanh is monotonic, so the max pass stays on the raw logits and only the row
// maximum is capped; the sum-exp pass caps every element in registers.
template <typename T, int BLOCK, bool Z, bool CAP, typename... Cap>
__global__ void ce_fwd_kernel(const T* __restrict__ logits, const long* __restrict__ targets,
                              float* __restrict__ loss_partials, float* __restrict__ z_partials,
                              long* __restrict__ ntok, float* __restrict__ lse_out, long rows,
                              int V, long ignore_index, Cap... cap) {
  static_assert(sizeof...(Cap) == (CAP ? 1 : 0) && (Z || !CAP), "CAP takes (float cap), with Z");
  __shared__ float scratch[BLOCK / WAVE];
  [[maybe_unused]] const float c = cap_arg(cap...);
  [[maybe_unused]] const float inv_c = CAP ? 1.f / c : 0.f;
  // thread 0 adds this block's rows in row order; reduce_partials_kernel then
  // adds the per-block partials in a fixed order, so the loss is the same
  // every run (the integer token count is order-independent as an atomic)
  float block_loss = 0.f;
  float block_z = 0.f;
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const T* lr = logits + row * (long)V;
    // pass 1: max
    float m = -INFINITY;
    if constexpr (sizeof(T) == 2) {
      const int VV = V / 8;
      const uint4* lv = reinterpret_cast<const uint4*>(lr);
      for (int i = threadIdx.x; i < VV; i += BLOCK) {
        U4 u; u.u = lv[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) m = fmaxf(m, bf16_bits_to_f32(u.s[j]));
      }
      for (int i = VV * 8 + threadIdx.x; i < V; i += BLOCK) m = fmaxf(m, to_f32(lr[i]));
    } else {
      for (int i = threadIdx.x; i < V; i += BLOCK) m = fmaxf(m, to_f32(lr[i]));
    }
    m = block_reduce_max<BLOCK>(m, scratch);
    if constexpr (CAP) m = softcap_val(m, c, inv_c);
    // pass 2: sum exp
    float s = 0.f;
    if constexpr (sizeof(T) == 2) {
      const int VV = V / 8;
      const uint4* lv = reinterpret_cast<const uint4*>(lr);
      for (int i = threadIdx.x; i < VV; i += BLOCK) {
        U4 u; u.u = lv[i];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          s += __expf(capped<CAP>(bf16_bits_to_f32(u.s[j]), c, inv_c) - m);
      }
      for (int i = VV * 8 + threadIdx.x; i < V; i += BLOCK)
        s += __expf(capped<CAP>(to_f32(lr[i]), c, inv_c) - m);
    } else {
      for (int i = threadIdx.x; i < V; i += BLOCK)
        s += __expf(capped<CAP>(to_f32(lr[i]), c, inv_c) - m);
    }
    s = block_reduce_sum<BLOCK>(s, scratch);
    const float lse = m + __logf(s);
    if (threadIdx.x == 0) {
      lse_out[row] = lse;
      const long t = targets[row];
      if (t != ignore_index) {
        block_loss += lse - capped<CAP>(to_f32(lr[t]), c, inv_c);
        if constexpr (Z) block_z += lse * lse;
        atomicAdd(reinterpret_cast<unsigned long long*>(ntok), 1ull);
      }
    }
  }
  if (threadIdx.x == 0) {
    loss_partials[blockIdx.x] = block_loss;
    if constexpr (Z) z_partials[blockIdx.x] = block_z;
  }
}

// Z: with a = *scale and b = *scale_z the row also carries the z-loss term,
// dlogits = (p - onehot) * a + p * (b * lse). The CE part is the plain
// kernel's own expression and the z part is added to it in one fma, so b = 0
// gives the plain kernel's bits.
// CAP: p is taken from the capped logit t and the chain rule's
// 1 - (t / c)^2 multiplies the result; lse is the capped row's.
template <typename T, bool Z, bool CAP, typename... Cap>
__global__ void ce_bwd_kernel(const T* __restrict__ logits, const long* __restrict__ targets,
                              const float* __restrict__ lse, const float* __restrict__ scale,
                              const float* __restrict__ scale_z, T* __restrict__ dlogits,
                              long rows, int V, long ignore_index, Cap... cap) {
  static_assert(sizeof...(Cap) == (CAP ? 1 : 0) && (Z || !CAP), "CAP takes (float cap), with Z");
  [[maybe_unused]] const float c = cap_arg(cap...);
  [[maybe_unused]] const float inv_c = CAP ? 1.f / c : 0.f;
  const float sc = *scale;
  float sz = 0.f;
  if constexpr (Z) sz = *scale_z;
  const int VV = V / 8;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < rows * (long)VV;
       idx += gridDim.x * (long)blockDim.x) {
    const long row = idx / VV;
    const int col = (int)(idx % VV) * 8;
    const long t = targets[row];
    const float l = lse[row];
    const T* lr = logits + row * (long)V + col;
    T* dr = dlogits + row * (long)V + col;
    if (t == ignore_index) {
#pragma unroll
      for (int j = 0; j < 8; ++j) from_f32(&dr[j], 0.f);
      continue;
    }
    const float zl = sz * l;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float x = capped<CAP>(to_f32(lr[j]), c, inv_c);
      float p = __expf(x - l);
      if constexpr (CAP) {
        const float pz = p * zl;
        if (col + j == (int)t) p -= 1.f;
        from_f32(&dr[j], fmaf(p, sc, pz) * softcap_dfac(x, inv_c));
      } else if constexpr (Z) {
        const float pz = p * zl;
        if (col + j == (int)t) p -= 1.f;
        from_f32(&dr[j], fmaf(p, sc, pz));
      } else {
        if (col + j == (int)t) p -= 1.f;
        from_f32(&dr[j], p * sc);
      }
    }
  }
}

// ---- vocab-parallel CE (TP lm-head shards; parallel/tp.py) ----
// Pass 1: per-row local max + the target logit if it lives in this shard.
// CAP: both of the capped shard (the max is capped once, tanh being monotonic).
template <int BLOCK, bool CAP, typename... Cap>
__global__ void ce_vp_stats_kernel(const __hip_bfloat16* __restrict__ logits,
                                   const long* __restrict__ targets,
                                   float* __restrict__ m_out, float* __restrict__ tgt_out,
                                   long rows, int V, long v0, long ignore_index,
                                   Cap... cap) {
  static_assert(sizeof...(Cap) == (CAP ? 1 : 0), "CAP takes (float cap)");
  __shared__ float scratch[BLOCK / WAVE];
  [[maybe_unused]] const float c = cap_arg(cap...);
  [[maybe_unused]] const float inv_c = CAP ? 1.f / c : 0.f;
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const __hip_bfloat16* lr = logits + row * (long)V;
    float m = -INFINITY;
    const int VV = V / 8;
    const uint4* lv = reinterpret_cast<const uint4*>(lr);
    for (int i = threadIdx.x; i < VV; i += BLOCK) {
      U4 u; u.u = lv[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) m = fmaxf(m, bf16_bits_to_f32(u.s[j]));
    }
    for (int i = VV * 8 + threadIdx.x; i < V; i += BLOCK) m = fmaxf(m, to_f32(lr[i]));
    m = block_reduce_max<BLOCK>(m, scratch);
    if (threadIdx.x == 0) {
      m_out[row] = capped<CAP>(m, c, inv_c);
      const long t = targets[row];
      const long tl = t - v0;
      tgt_out[row] = (t != ignore_index && tl >= 0 && tl < V)
                         ? capped<CAP>(to_f32(lr[tl]), c, inv_c) : 0.f;
    }
  }
}

// Pass 2 (after the group max all-reduce): sum exp(l - m_group); CAP: of the
// capped l.
template <int BLOCK, bool CAP, typename... Cap>
__global__ void ce_vp_sumexp_kernel(const __hip_bfloat16* __restrict__ logits,
                                    const float* __restrict__ m_group,
                                    float* __restrict__ se_out, long rows, int V,
                                    Cap... cap) {
  static_assert(sizeof...(Cap) == (CAP ? 1 : 0), "CAP takes (float cap)");
  __shared__ float scratch[BLOCK / WAVE];
  [[maybe_unused]] const float c = cap_arg(cap...);
  [[maybe_unused]] const float inv_c = CAP ? 1.f / c : 0.f;
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const __hip_bfloat16* lr = logits + row * (long)V;
    const float m = m_group[row];
    float s = 0.f;
    const int VV = V / 8;
    const uint4* lv = reinterpret_cast<const uint4*>(lr);
    for (int i = threadIdx.x; i < VV; i += BLOCK) {
      U4 u; u.u = lv[i];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        s += __expf(capped<CAP>(bf16_bits_to_f32(u.s[j]), c, inv_c) - m);
    }
    for (int i = VV * 8 + threadIdx.x; i < V; i += BLOCK)
      s += __expf(capped<CAP>(to_f32(lr[i]), c, inv_c) - m);
    s = block_reduce_sum<BLOCK>(s, scratch);
    if (threadIdx.x == 0) se_out[row] = s;
  }
}

// Backward: dlogits = (exp(l - lse_group) - onehot(t - v0)) * (*scale), rows
// with ignored targets get 0 (scale = upstream_grad / ntok, device scalar).
// Z adds p * (*scale_z * lse_group), CAP caps, both as in ce_bwd_kernel.
template <bool Z, bool CAP, typename... Cap>
__global__ void ce_vp_bwd_kernel(const __hip_bfloat16* __restrict__ logits,
                                 const long* __restrict__ targets,
                                 const float* __restrict__ lse,
                                 const float* __restrict__ scale,
                                 const float* __restrict__ scale_z,
                                 __hip_bfloat16* __restrict__ dlogits,
                                 long rows, int V, long v0, long ignore_index,
                                 Cap... cap) {
  static_assert(sizeof...(Cap) == (CAP ? 1 : 0) && (Z || !CAP), "CAP takes (float cap), with Z");
  [[maybe_unused]] const float c = cap_arg(cap...);
  [[maybe_unused]] const float inv_c = CAP ? 1.f / c : 0.f;
  const float sc = *scale;
  float sz = 0.f;
  if constexpr (Z) sz = *scale_z;
  const int VV = V / 8;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < rows * (long)VV;
       idx += gridDim.x * (long)blockDim.x) {
    const long row = idx / VV;
    const int col = (int)(idx % VV) * 8;
    const long t = targets[row];
    const float l = lse[row];
    const __hip_bfloat16* lr = logits + row * (long)V + col;
    __hip_bfloat16* dr = dlogits + row * (long)V + col;
    if (t == ignore_index) {
#pragma unroll
      for (int j = 0; j < 8; ++j) from_f32(&dr[j], 0.f);
      continue;
    }
    const long tl = t - v0;
    const float zl = sz * l;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float x = capped<CAP>(to_f32(lr[j]), c, inv_c);
      float p = __expf(x - l);
      if constexpr (CAP) {
        const float pz = p * zl;
        if (col + j == (int)tl) p -= 1.f;
        from_f32(&dr[j], fmaf(p, sc, pz) * softcap_dfac(x, inv_c));
      } else if constexpr (Z) {
        const float pz = p * zl;
        if (col + j == (int)tl) p -= 1.f;
        from_f32(&dr[j], fmaf(p, sc, pz));
      } else {
        if (col + j == (int)tl) p -= 1.f;
        from_f32(&dr[j], p * sc);
      }
    }
  }
}

// logits [rows, V] contiguous on the GPU; targets int64 [rows] beside them.
// bf16 rows are read as 16-byte vectors, so V % 8 == 0 keeps every row aligned.
void check_logits_targets(const at::Tensor& logits, const at::Tensor& targets, const char* who) {
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2,
              who, ": logits must be a contiguous 2-D GPU tensor");
  TORCH_CHECK(targets.device() == logits.device() && targets.scalar_type() == at::kLong &&
                  targets.is_contiguous() && targets.dim() == 1 &&
                  targets.size(0) == logits.size(0),
              who, ": targets must be int64 [rows] on the logits' device");
}

void check_row_f32(const at::Tensor& t, const at::Tensor& logits, const char* who,
                   const char* name) {
  TORCH_CHECK(t.device() == logits.device() && t.scalar_type() == at::kFloat &&
                  t.is_contiguous() && t.dim() == 1 && t.size(0) == logits.size(0),
              who, ": ", name, " must be fp32 [rows] on the logits' device");
}

void check_scale(const at::Tensor& scale, const at::Tensor& logits, const char* who) {
  TORCH_CHECK(scale.device() == logits.device() && scale.numel() == 1, who,
              ": scale must be one element on the logits' device");
}

void check_vp_logits(const at::Tensor& logits, const char* who) {
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2 &&
                  logits.scalar_type() == at::kBFloat16,
              who, ": logits must be a contiguous 2-D bf16 GPU tensor");
  TORCH_CHECK(logits.size(1) % 8 == 0, "ce_vp: vocab shard must be a multiple of 8");
}

// the two scales of the z backward are read as float by the kernel
void check_scale_f32(const at::Tensor& scale, const at::Tensor& logits, const char* who,
                     const char* name) {
  TORCH_CHECK(scale.device() == logits.device() && scale.numel() == 1 &&
                  scale.scalar_type() == at::kFloat,
              who, ": ", name, " must be one fp32 element on the logits' device");
}

// the soft cap c of t = c * tanh(x / c), as the kernels take it
float check_cap(double cap, const char* who) {
  const float c = (float)cap;
  TORCH_CHECK(std::isfinite(cap) && std::isfinite(c) && c > 0.f, who,
              ": cap must be finite and > 0, got ", cap);
  return c;
}

// {loss_sum, ntok, lse}, and z_sum after loss_sum when Z; CAP (always with Z)
// runs the capped kernel with cap
template <bool Z, bool CAP = false>
std::vector<at::Tensor> ce_fwd_impl(const at::Tensor& logits, const at::Tensor& targets,
                                    long ignore_index, const char* who, float cap = 0.f) {
  check_logits_targets(logits, targets, who);
  const long rows = logits.size(0);
  const int V = logits.size(1);
  TORCH_CHECK(logits.scalar_type() != at::kBFloat16 || V % 8 == 0,
              who, ": bf16 vocab must be a multiple of 8");
  auto loss_sum = at::zeros({}, logits.options().dtype(at::kFloat));
  at::Tensor z_sum, z_partials;
  if constexpr (Z) z_sum = at::zeros({}, logits.options().dtype(at::kFloat));
  auto ntok = at::zeros({}, logits.options().dtype(at::kLong));
  auto lse = at::empty({rows}, logits.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentHIPStream();
  constexpr int BLOCK = 256;
  const long grid = std::min<long>(rows, 4096);
  auto partials = at::empty({grid}, logits.options().dtype(at::kFloat));
  if constexpr (Z) z_partials = at::empty({grid}, logits.options().dtype(at::kFloat));
  if (rows == 0) {  // an empty grid is a launch error
    if constexpr (Z) return {loss_sum, z_sum, ntok, lse};
    return {loss_sum, ntok, lse};
  }
  AT_DISPATCH_FLOATING_TYPES_AND2(at::kBFloat16, at::kHalf, logits.scalar_type(), "ce_fwd", [&] {
    using T = std::conditional_t<std::is_same_v<scalar_t, at::BFloat16>, __hip_bfloat16, float>;
    if constexpr (std::is_same_v<scalar_t, at::BFloat16> || std::is_same_v<scalar_t, float>) {
      if constexpr (CAP) {
        ce_fwd_kernel<T, BLOCK, Z, true><<<grid, BLOCK, 0, stream>>>(
            reinterpret_cast<const T*>(logits.data_ptr()), targets.data_ptr<long>(),
            partials.data_ptr<float>(), z_partials.data_ptr<float>(),
            ntok.data_ptr<long>(), lse.data_ptr<float>(), rows, V, ignore_index, cap);
      } else {
        ce_fwd_kernel<T, BLOCK, Z, false><<<grid, BLOCK, 0, stream>>>(
            reinterpret_cast<const T*>(logits.data_ptr()), targets.data_ptr<long>(),
            partials.data_ptr<float>(), Z ? z_partials.data_ptr<float>() : nullptr,
            ntok.data_ptr<long>(), lse.data_ptr<float>(), rows, V, ignore_index);
      }
      C10_HIP_KERNEL_LAUNCH_CHECK();
    } else {
      TORCH_CHECK(false, "ce: unsupported dtype");
    }
  });
  reduce_partials_kernel<256><<<1, 256, 0, stream>>>(
      partials.data_ptr<float>(), (int)grid, loss_sum.data_ptr<float>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  if constexpr (Z) {
    reduce_partials_kernel<256><<<1, 256, 0, stream>>>(
        z_partials.data_ptr<float>(), (int)grid, z_sum.data_ptr<float>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
    return {loss_sum, z_sum, ntok, lse};
  }
  return {loss_sum, ntok, lse};
}

// the arguments are checked by the callers; scale_z is read only when Z
template <bool Z, bool CAP = false>
at::Tensor ce_bwd_impl(const at::Tensor& logits, const at::Tensor& targets,
                       const at::Tensor& lse, const float* scale, const float* scale_z,
                       long ignore_index, const char* who, float cap = 0.f) {
  const long rows = logits.size(0);
  const int V = logits.size(1);
  TORCH_CHECK(V % 8 == 0, who, ": vocab must be a multiple of 8");
  auto dlogits = at::empty_like(logits);
  if (logits.numel() == 0) return dlogits;
  auto stream = at::cuda::getCurrentHIPStream();
  const int block = 256;
  const long grid = std::min<long>(cdiv(rows * (V / 8), block), 4096);
  AT_DISPATCH_FLOATING_TYPES_AND2(at::kBFloat16, at::kHalf, logits.scalar_type(), "ce_bwd", [&] {
    using T = std::conditional_t<std::is_same_v<scalar_t, at::BFloat16>, __hip_bfloat16, float>;
    if constexpr (std::is_same_v<scalar_t, at::BFloat16> || std::is_same_v<scalar_t, float>) {
      if constexpr (CAP) {
        ce_bwd_kernel<T, Z, true><<<grid, block, 0, stream>>>(
            reinterpret_cast<const T*>(logits.data_ptr()), targets.data_ptr<long>(),
            lse.data_ptr<float>(), scale, scale_z,
            reinterpret_cast<T*>(dlogits.data_ptr()), rows, V, ignore_index, cap);
      } else {
        ce_bwd_kernel<T, Z, false><<<grid, block, 0, stream>>>(
            reinterpret_cast<const T*>(logits.data_ptr()), targets.data_ptr<long>(),
            lse.data_ptr<float>(), scale, scale_z,
            reinterpret_cast<T*>(dlogits.data_ptr()), rows, V, ignore_index);
      }
      C10_HIP_KERNEL_LAUNCH_CHECK();
    } else {
      TORCH_CHECK(false, "ce: unsupported dtype");
    }
  });
  return dlogits;
}

template <bool Z, bool CAP = false>
at::Tensor ce_vp_bwd_impl(const at::Tensor& logits, const at::Tensor& targets,
                          const at::Tensor& lse, const float* scale, const float* scale_z,
                          long v0, long ignore_index, float cap = 0.f) {
  const long rows = logits.size(0);
  const int V = logits.size(1);
  auto dl = at::empty_like(logits);
  if (logits.numel() == 0) return dl;
  auto stream = at::cuda::getCurrentHIPStream();
  const long work = rows * (V / 8);
  const int grid = (int)std::min<long>((work + 255) / 256, 4096);
  if constexpr (CAP) {
    ce_vp_bwd_kernel<Z, true><<<grid, 256, 0, stream>>>(
        reinterpret_cast<const __hip_bfloat16*>(logits.data_ptr()),
        targets.data_ptr<long>(), lse.data_ptr<float>(), scale, scale_z,
        reinterpret_cast<__hip_bfloat16*>(dl.data_ptr()), rows, V, v0, ignore_index, cap);
  } else {
    ce_vp_bwd_kernel<Z, false><<<grid, 256, 0, stream>>>(
        reinterpret_cast<const __hip_bfloat16*>(logits.data_ptr()),
        targets.data_ptr<long>(), lse.data_ptr<float>(), scale, scale_z,
        reinterpret_cast<__hip_bfloat16*>(dl.data_ptr()), rows, V, v0, ignore_index);
  }
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return dl;
}

}  // namespace

std::vector<at::Tensor> ce_fwd(at::Tensor logits, at::Tensor targets, long ignore_index) {
  return ce_fwd_impl<false>(logits, targets, ignore_index, "ce_fwd");
}

// (loss_sum, z_sum, ntok, lse): z_sum = sum of lse^2 over the counted rows
std::vector<at::Tensor> ce_fwd_z(at::Tensor logits, at::Tensor targets, long ignore_index) {
  return ce_fwd_impl<true>(logits, targets, ignore_index, "ce_fwd_z");
}

at::Tensor ce_bwd(at::Tensor logits, at::Tensor targets, at::Tensor lse, at::Tensor scale,
                  long ignore_index) {
  check_logits_targets(logits, targets, "ce_bwd");
  check_row_f32(lse, logits, "ce_bwd", "lse");
  check_scale(scale, logits, "ce_bwd");
  auto scale_f = scale.to(at::kFloat);
  return ce_bwd_impl<false>(logits, targets, lse, scale_f.data_ptr<float>(), nullptr,
                            ignore_index, "ce_bwd");
}

// dlogits = p * (a + b * lse) - a * onehot with a = *scale_ce (g_ce / ntok) and
// b = *scale_z (2 * g_z / ntok), both fp32 device scalars
at::Tensor ce_bwd_z(at::Tensor logits, at::Tensor targets, at::Tensor lse, at::Tensor scale_ce,
                    at::Tensor scale_z, long ignore_index) {
  check_logits_targets(logits, targets, "ce_bwd_z");
  check_row_f32(lse, logits, "ce_bwd_z", "lse");
  check_scale_f32(scale_ce, logits, "ce_bwd_z", "scale_ce");
  check_scale_f32(scale_z, logits, "ce_bwd_z", "scale_z");
  return ce_bwd_impl<true>(logits, targets, lse, scale_ce.data_ptr<float>(),
                           scale_z.data_ptr<float>(), ignore_index, "ce_bwd_z");
}

namespace {

template <bool CAP>
std::vector<at::Tensor> ce_vp_stats_impl(const at::Tensor& logits, const at::Tensor& targets,
                                         long v0, long ignore_index, const char* who,
                                         float cap = 0.f) {
  check_vp_logits(logits, who);
  check_logits_targets(logits, targets, who);
  const long rows = logits.size(0);
  const int V = logits.size(1);
  auto m = at::empty({rows}, logits.options().dtype(at::kFloat));
  auto tgt = at::empty({rows}, logits.options().dtype(at::kFloat));
  if (rows == 0) return {m, tgt};
  auto stream = at::cuda::getCurrentHIPStream();
  const int grid = (int)std::min<long>(rows, 2048);
  if constexpr (CAP) {
    ce_vp_stats_kernel<256, true><<<grid, 256, 0, stream>>>(
        reinterpret_cast<const __hip_bfloat16*>(logits.data_ptr()),
        targets.data_ptr<long>(), m.data_ptr<float>(), tgt.data_ptr<float>(),
        rows, V, v0, ignore_index, cap);
  } else {
    ce_vp_stats_kernel<256, false><<<grid, 256, 0, stream>>>(
        reinterpret_cast<const __hip_bfloat16*>(logits.data_ptr()),
        targets.data_ptr<long>(), m.data_ptr<float>(), tgt.data_ptr<float>(),
        rows, V, v0, ignore_index);
  }
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {m, tgt};
}

template <bool CAP>
at::Tensor ce_vp_sumexp_impl(const at::Tensor& logits, const at::Tensor& m_group,
                             const char* who, float cap = 0.f) {
  check_vp_logits(logits, who);
  check_row_f32(m_group, logits, who, "m_group");
  const long rows = logits.size(0);
  const int V = logits.size(1);
  auto se = at::empty({rows}, logits.options().dtype(at::kFloat));
  if (rows == 0) return se;
  auto stream = at::cuda::getCurrentHIPStream();
  const int grid = (int)std::min<long>(rows, 2048);
  if constexpr (CAP) {
    ce_vp_sumexp_kernel<256, true><<<grid, 256, 0, stream>>>(
        reinterpret_cast<const __hip_bfloat16*>(logits.data_ptr()),
        m_group.data_ptr<float>(), se.data_ptr<float>(), rows, V, cap);
  } else {
    ce_vp_sumexp_kernel<256, false><<<grid, 256, 0, stream>>>(
        reinterpret_cast<const __hip_bfloat16*>(logits.data_ptr()),
        m_group.data_ptr<float>(), se.data_ptr<float>(), rows, V);
  }
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return se;
}

}  // namespace

std::vector<at::Tensor> ce_vp_stats(at::Tensor logits, at::Tensor targets, long v0,
                                    long ignore_index) {
  return ce_vp_stats_impl<false>(logits, targets, v0, ignore_index, "ce_vp_stats");
}

at::Tensor ce_vp_sumexp(at::Tensor logits, at::Tensor m_group) {
  return ce_vp_sumexp_impl<false>(logits, m_group, "ce_vp_sumexp");
}

at::Tensor ce_vp_bwd(at::Tensor logits, at::Tensor targets, at::Tensor lse,
                     at::Tensor scale, long v0, long ignore_index) {
  check_vp_logits(logits, "ce_vp_bwd");
  check_logits_targets(logits, targets, "ce_vp_bwd");
  check_row_f32(lse, logits, "ce_vp_bwd", "lse");
  check_scale(scale, logits, "ce_vp_bwd");
  TORCH_CHECK(scale.scalar_type() == at::kFloat, "ce_vp_bwd: scale must be fp32");
  return ce_vp_bwd_impl<false>(logits, targets, lse, scale.data_ptr<float>(), nullptr, v0,
                               ignore_index);
}

// the shard's part of the z backward (ce_bwd_z), lse being the group's
at::Tensor ce_vp_bwd_z(at::Tensor logits, at::Tensor targets, at::Tensor lse,
                       at::Tensor scale_ce, at::Tensor scale_z, long v0, long ignore_index) {
  check_vp_logits(logits, "ce_vp_bwd_z");
  check_logits_targets(logits, targets, "ce_vp_bwd_z");
  check_row_f32(lse, logits, "ce_vp_bwd_z", "lse");
  check_scale_f32(scale_ce, logits, "ce_vp_bwd_z", "scale_ce");
  check_scale_f32(scale_z, logits, "ce_vp_bwd_z", "scale_z");
  return ce_vp_bwd_impl<true>(logits, targets, lse, scale_ce.data_ptr<float>(),
                              scale_z.data_ptr<float>(), v0, ignore_index);
}

// ---- final-logit soft-capping: the loss of t = cap * tanh(logits / cap) ----
// One capped variant per kernel, always with the z terms (scale_z = 0 gives
// the pure capped CE). lse, and the m / tgt / se of the shard passes, are those
// of the capped row.

// (loss_sum, z_sum, ntok, lse) as ce_fwd_z
std::vector<at::Tensor> ce_cap_fwd(at::Tensor logits, at::Tensor targets, long ignore_index,
                                   double cap) {
  const float c = check_cap(cap, "ce_cap_fwd");
  return ce_fwd_impl<true, true>(logits, targets, ignore_index, "ce_cap_fwd", c);
}

// dlogits = (p * (a + b * lse) - a * onehot) * (1 - (t / cap)^2), a and b as in ce_bwd_z
at::Tensor ce_cap_bwd(at::Tensor logits, at::Tensor targets, at::Tensor lse, at::Tensor scale_ce,
                      at::Tensor scale_z, long ignore_index, double cap) {
  const float c = check_cap(cap, "ce_cap_bwd");
  check_logits_targets(logits, targets, "ce_cap_bwd");
  check_row_f32(lse, logits, "ce_cap_bwd", "lse");
  check_scale_f32(scale_ce, logits, "ce_cap_bwd", "scale_ce");
  check_scale_f32(scale_z, logits, "ce_cap_bwd", "scale_z");
  return ce_bwd_impl<true, true>(logits, targets, lse, scale_ce.data_ptr<float>(),
                                 scale_z.data_ptr<float>(), ignore_index, "ce_cap_bwd", c);
}

std::vector<at::Tensor> ce_vp_cap_stats(at::Tensor logits, at::Tensor targets, long v0,
                                        long ignore_index, double cap) {
  const float c = check_cap(cap, "ce_vp_cap_stats");
  return ce_vp_stats_impl<true>(logits, targets, v0, ignore_index, "ce_vp_cap_stats", c);
}

at::Tensor ce_vp_cap_sumexp(at::Tensor logits, at::Tensor m_group, double cap) {
  const float c = check_cap(cap, "ce_vp_cap_sumexp");
  return ce_vp_sumexp_impl<true>(logits, m_group, "ce_vp_cap_sumexp", c);
}

at::Tensor ce_vp_cap_bwd(at::Tensor logits, at::Tensor targets, at::Tensor lse,
                         at::Tensor scale_ce, at::Tensor scale_z, long v0, long ignore_index,
                         double cap) {
  const float c = check_cap(cap, "ce_vp_cap_bwd");
  check_vp_logits(logits, "ce_vp_cap_bwd");
  check_logits_targets(logits, targets, "ce_vp_cap_bwd");
  check_row_f32(lse, logits, "ce_vp_cap_bwd", "lse");
  check_scale_f32(scale_ce, logits, "ce_vp_cap_bwd", "scale_ce");
  check_scale_f32(scale_z, logits, "ce_vp_cap_bwd", "scale_z");
  return ce_vp_bwd_impl<true, true>(logits, targets, lse, scale_ce.data_ptr<float>(),
                                    scale_z.data_ptr<float>(), v0, ignore_index, c);
}
