// Elementwise soft-capping y = c * tanh(x / c) for the paths that need the
// capped logits as a tensor (generation, the static decoder's in-place
// epilogue) and its backward from the saved output, dx = dy * (1 - (y / c)^2).
// The training loss never runs these: it caps inside the cross-entropy kernels
// (cross_entropy.hip), with the same softcap_val.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPException.h>
#include <cmath>
#include <cstdint>
#include "common.h"
#include "softcap.h"

namespace {

__device__ __forceinline__ float ld_f32(const __hip_bfloat16* p) { return to_f32(*p); }
__device__ __forceinline__ float ld_f32(const float* p) { return *p; }

// One flat pass over n elements. `head` elements come before the first
// 16-byte boundary that the buffers share (the host passes head = n when they
// do not share one, which leaves everything to the scalar loop); from there
// whole 16-byte vectors, then the scalar tail. BWD: a = dy, b = y, and
// out = a * (1 - (b / c)^2); else out = softcap_val(a) and b is not read.
// In place (out == a) is fine: an element is read and written by one thread.
template <typename T, bool BWD>
__global__ void softcap_kernel(const T* a, const T* b, T* out, long n, long head, float c) {
  constexpr int VEC = 16 / sizeof(T);
  const float inv_c = 1.f / c;
  const long nvec = (n - head) / VEC;
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const long stride = gridDim.x * (long)blockDim.x;
  for (long i = tid; i < nvec; i += stride) {
    const long k = head + i * VEC;
    U4 ua, ub, uo;
    ua.u = *reinterpret_cast<const uint4*>(a + k);
    if constexpr (BWD) ub.u = *reinterpret_cast<const uint4*>(b + k);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float va, vb = 0.f;
      if constexpr (sizeof(T) == 2) {
        va = bf16_bits_to_f32(ua.s[j]);
        if constexpr (BWD) vb = bf16_bits_to_f32(ub.s[j]);
      } else {
        va = ua.f[j];
        if constexpr (BWD) vb = ub.f[j];
      }
      const float r = BWD ? va * softcap_dfac(vb, inv_c) : softcap_val(va, c, inv_c);
      if constexpr (sizeof(T) == 2) uo.s[j] = f32_to_bf16_bits(r);
      else uo.f[j] = r;
    }
    *reinterpret_cast<uint4*>(out + k) = uo.u;
  }
  const long tail0 = head + nvec * VEC;
  const long nscalar = head + (n - tail0);
  for (long i = tid; i < nscalar; i += stride) {
    const long k = i < head ? i : tail0 + (i - head);
    const float va = ld_f32(a + k);
    const float r = BWD ? va * softcap_dfac(ld_f32(b + k), inv_c) : softcap_val(va, c, inv_c);
    from_f32(out + k, r);
  }
}

float check_softcap_cap(double cap, const char* who) {
  const float c = (float)cap;
  TORCH_CHECK(std::isfinite(cap) && std::isfinite(c) && c > 0.f, who,
              ": cap must be finite and > 0, got ", cap);
  return c;
}

void check_softcap_tensor(const at::Tensor& x, const char* who, const char* name) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() &&
                  (x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kFloat),
              who, ": ", name, " must be a contiguous bf16 or fp32 GPU tensor");
}

// elements before the 16-byte boundary common to all the pointers, n if none
long shared_head(std::initializer_list<const void*> ptrs, long n, long itemsize) {
  const uintptr_t off = reinterpret_cast<uintptr_t>(*ptrs.begin()) & 15;
  for (const void* p : ptrs)
    if ((reinterpret_cast<uintptr_t>(p) & 15) != off) return n;
  return std::min<long>(n, (long)((16 - off) & 15) / itemsize);
}

template <bool BWD>
void softcap_launch(const at::Tensor& a, const at::Tensor* b, at::Tensor& out, float c) {
  const long n = a.numel();
  if (n == 0) return;  // an empty grid is a launch error
  auto stream = at::cuda::getCurrentHIPStream();
  const long isz = a.element_size();
  const void* pb = BWD ? b->data_ptr() : a.data_ptr();
  const long head = shared_head({a.data_ptr(), pb, out.data_ptr()}, n, isz);
  const long nvec = (n - head) / (16 / isz);
  const long items = std::max<long>(nvec, n - nvec * (16 / isz));
  const int grid = (int)std::min<long>(cdiv(items, 256), 4096);
  if (a.scalar_type() == at::kBFloat16) {
    using T = __hip_bfloat16;
    softcap_kernel<T, BWD><<<grid, 256, 0, stream>>>(
        reinterpret_cast<const T*>(a.data_ptr()), reinterpret_cast<const T*>(pb),
        reinterpret_cast<T*>(out.data_ptr()), n, head, c);
  } else {
    softcap_kernel<float, BWD><<<grid, 256, 0, stream>>>(
        a.data_ptr<float>(), reinterpret_cast<const float*>(pb), out.data_ptr<float>(), n,
        head, c);
  }
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

}  // namespace

at::Tensor softcap_fwd(at::Tensor x, double cap) {
  const float c = check_softcap_cap(cap, "softcap_fwd");
  check_softcap_tensor(x, "softcap_fwd", "x");
  auto y = at::empty_like(x);
  softcap_launch<false>(x, nullptr, y, c);
  return y;
}

// in place: no allocation and no host sync, so it can sit in a captured graph
void softcap_(at::Tensor x, double cap) {
  const float c = check_softcap_cap(cap, "softcap_");
  check_softcap_tensor(x, "softcap_", "x");
  softcap_launch<false>(x, nullptr, x, c);
}

// dx = dy * (1 - (y / cap)^2) from the saved output y
at::Tensor softcap_bwd(at::Tensor dy, at::Tensor y, double cap) {
  const float c = check_softcap_cap(cap, "softcap_bwd");
  check_softcap_tensor(dy, "softcap_bwd", "dy");
  check_softcap_tensor(y, "softcap_bwd", "y");
  TORCH_CHECK(dy.scalar_type() == y.scalar_type() && dy.sizes() == y.sizes() &&
                  dy.device() == y.device(),
              "softcap_bwd: dy and y must agree in dtype, shape and device");
  auto dx = at::empty_like(y);
  softcap_launch<true>(dy, &y, dx, c);
  return dx;
}
