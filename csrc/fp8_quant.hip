// Fused e4m3 quantization for the fp8 GEMM path (ops/fp8.py).
// The torch-composed quantize ((x.float()/s).clamp().to(fp8)) costs ~5 full
// passes with fp32 intermediates (~0.42 ms for a 32768x2048 bf16 tensor —
// 40% of the GEMM it feeds); these kernels do it in 2 passes:
//   amax : block partials -> one atomicMax on monotonic float bits
//   cast : bf16 -> e4m3 with v_cvt_pk_fp8_f32, scale read from DEVICE
//          memory (no host sync; feeds _scaled_mm's device scale tensor)
// gfx950's v_cvt_pk_fp8_f32 emits OCP e4m3fn (not the MI300X fnuz variant)
// with saturation — exactly torch.float8_e4m3fn.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPException.h>
#include "common.h"

namespace {

constexpr float E4M3_MAX = 448.f;

// non-negative floats compare like their bit patterns
__global__ void amax_kernel(const __hip_bfloat16* __restrict__ x, long n,
                            unsigned* __restrict__ amax_bits) {
  __shared__ float scratch[256 / WAVE];
  float m = 0.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n / 8;
       i += gridDim.x * (long)blockDim.x) {
    U4 u;
    u.u = reinterpret_cast<const uint4*>(x)[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(bf16_bits_to_f32(u.s[j])));
  }
  for (long i = (n / 8) * 8 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * (long)blockDim.x)
    m = fmaxf(m, fabsf(to_f32(x[i])));
  m = block_reduce_max<256>(m, scratch);
  if (threadIdx.x == 0) {
    union { float f; unsigned u; } c;
    c.f = m;
    atomicMax(amax_bits, c.u);
  }
}

// write the fp32 dequant scale (amax/448, clamped) for _scaled_mm
__global__ void scale_from_amax_kernel(const unsigned* __restrict__ amax_bits,
                                       float* __restrict__ scale) {
  union { float f; unsigned u; } c;
  c.u = *amax_bits;
  *scale = fmaxf(c.f / E4M3_MAX, 1e-12f);
}

// reduce a producer's per-block partial-max array -> scale (one tiny block)
__global__ void scale_from_partials_kernel(const float* __restrict__ partials, long n,
                                           float* __restrict__ scale) {
  __shared__ float scratch[256 / WAVE];
  float m = 0.f;
  for (long i = threadIdx.x; i < n; i += 256) m = fmaxf(m, partials[i]);
  m = block_reduce_max<256>(m, scratch);
  if (threadIdx.x == 0) *scale = fmaxf(m / E4M3_MAX, 1e-12f);
}

// cast with the INVERSE scale read from device memory. 8 elems/thread.
__global__ void cast_e4m3_kernel(const __hip_bfloat16* __restrict__ x,
                                 unsigned char* __restrict__ y, long n,
                                 const float* __restrict__ scale) {
  const float inv = 1.f / *scale;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n / 8;
       i += gridDim.x * (long)blockDim.x) {
    U4 u;
    u.u = reinterpret_cast<const uint4*>(x)[i];
    unsigned lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf16_bits_to_f32(u.s[0]) * inv,
                                         bf16_bits_to_f32(u.s[1]) * inv, lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf16_bits_to_f32(u.s[2]) * inv,
                                         bf16_bits_to_f32(u.s[3]) * inv, lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf16_bits_to_f32(u.s[4]) * inv,
                                         bf16_bits_to_f32(u.s[5]) * inv, hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf16_bits_to_f32(u.s[6]) * inv,
                                         bf16_bits_to_f32(u.s[7]) * inv, hi, true);
    reinterpret_cast<uint2*>(y)[i] = uint2{lo, hi};
  }
  const float* s = scale;  // tail
  for (long i = (n / 8) * 8 + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * (long)blockDim.x) {
    unsigned v = 0;
    v = __builtin_amdgcn_cvt_pk_fp8_f32(to_f32(x[i]) * (1.f / *s), 0.f, v, false);
    y[i] = (unsigned char)(v & 0xff);
  }
}

// transposed cast: y[k][n] = quant(x[n][k]); x [N, K] bf16 -> y [K, N] e4m3.
// 32x32 LDS tile staging keeps both sides coalesced.
__global__ void cast_e4m3_t_kernel(const __hip_bfloat16* __restrict__ x,
                                   unsigned char* __restrict__ y,
                                   int N, int K, const float* __restrict__ scale) {
  __shared__ float tile[32][33];
  const float inv = 1.f / *scale;
  const int n0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
  const int tx = threadIdx.x % 32, ty = threadIdx.x / 32;  // block 256 = 32x8
  for (int r = ty; r < 32; r += 8) {
    const int n = n0 + r, k = k0 + tx;
    tile[r][tx] = (n < N && k < K) ? to_f32(x[(long)n * K + k]) * inv : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int k = k0 + r, n = n0 + tx;
    if (k < K && n < N) {
      unsigned v = 0;
      v = __builtin_amdgcn_cvt_pk_fp8_f32(tile[tx][r], 0.f, v, false);
      y[(long)k * N + n] = (unsigned char)(v & 0xff);
    }
  }
}

}  // namespace

// amax_in numel()==0 -> run the amax pass; otherwise amax_in is a PRODUCER
// kernel's per-block partial-max float array (rmsnorm / swiglu emit one) and
// the extra full read of x is skipped — the tiny reduce replaces it.
std::vector<at::Tensor> fp8_quantize_pre(at::Tensor x, at::Tensor amax_in, bool transpose) {
  // x: bf16 [.., K] (2D for transpose). Returns (codes float8_e4m3fn, scale f32[1]).
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16);
  auto xc = x.contiguous();
  const long n = xc.numel();
  auto stream = at::cuda::getCurrentHIPStream();
  const bool have_amax = amax_in.numel() > 0;
  auto scale = at::empty({}, x.options().dtype(at::kFloat));
  const long grid = std::min<long>(cdiv(n, 256 * 8), 2048);
  auto* xp = reinterpret_cast<const __hip_bfloat16*>(xc.data_ptr());
  if (n == 0) {  // nothing to cast: an empty grid is a launch error
    TORCH_CHECK(!transpose || x.dim() == 2, "fp8_quantize transpose: 2D only");
    auto y0 = transpose ? at::empty({x.size(1), x.size(0)}, xc.options().dtype(at::kFloat8_e4m3fn))
                        : at::empty_like(xc, xc.options().dtype(at::kFloat8_e4m3fn));
    return {y0, at::full({}, 1e-12f, x.options().dtype(at::kFloat))};
  }
  if (have_amax) {
    TORCH_CHECK(amax_in.scalar_type() == at::kFloat && amax_in.device() == x.device() &&
                    amax_in.is_contiguous(),
                "fp8_quantize_pre: amax partials must be contiguous fp32 on x's device");
    scale_from_partials_kernel<<<1, 256, 0, stream>>>(
        amax_in.data_ptr<float>(), amax_in.numel(), scale.data_ptr<float>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  } else {
    auto amax_bits = at::zeros({1}, x.options().dtype(at::kInt));
    amax_kernel<<<grid, 256, 0, stream>>>(
        xp, n, reinterpret_cast<unsigned*>(amax_bits.data_ptr<int>()));
    C10_HIP_KERNEL_LAUNCH_CHECK();
    scale_from_amax_kernel<<<1, 1, 0, stream>>>(
        reinterpret_cast<unsigned*>(amax_bits.data_ptr<int>()), scale.data_ptr<float>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  at::Tensor y;
  if (!transpose) {
    y = at::empty_like(xc, xc.options().dtype(at::kFloat8_e4m3fn));
    cast_e4m3_kernel<<<grid, 256, 0, stream>>>(
        xp, reinterpret_cast<unsigned char*>(y.data_ptr()), n, scale.data_ptr<float>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  } else {
    TORCH_CHECK(x.dim() == 2, "fp8_quantize transpose: 2D only");
    const int N = x.size(0), K = x.size(1);
    y = at::empty({K, N}, xc.options().dtype(at::kFloat8_e4m3fn));
    dim3 g(cdiv(N, 32), cdiv(K, 32));
    cast_e4m3_t_kernel<<<g, 256, 0, stream>>>(
        xp, reinterpret_cast<unsigned char*>(y.data_ptr()), N, K, scale.data_ptr<float>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return {y, scale};
}

std::vector<at::Tensor> fp8_quantize(at::Tensor x, bool transpose) {
  return fp8_quantize_pre(x, at::empty({0}, x.options().dtype(at::kFloat)), transpose);
}
