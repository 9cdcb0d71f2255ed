// Fused per-head QK-norm + RoPE (forward, backward, static-decode variant).
//
//   y = RoPE_{s+offset}( x * rsqrt(mean_d x^2 + eps) * w )
//
// applied to every q and k head of a [B,S,H,D] view (H = Hq + Hkv heads that
// sit next to each other in the fused QKV projection; h < Hq takes w_q, the
// rest w_k). Same thread mapping as rope_kernel: one thread owns 8 rotation
// pairs (16 elements), so a row is LPR = D/16 ADJACENT lanes (4 at D=64, 8 at
// D=128) and the reductions over head_dim are __shfl_xor butterflies inside
// that lane group — no LDS, no block reduction, x read once and y written
// once. Built from rmsnorm_fwd_kernel + rope_kernel the same math is four
// launches and two more HBM round trips over a QKV-sized tensor each way.
//
// Lane-group invariant: total_groups = rows*LPR, the block size and therefore
// the grid stride are all multiples of LPR and LPR divides 64, so the LPR
// lanes of a row sit in one wave, enter and leave the grid-stride loop
// together, and the shuffles only ever read active lanes. The same fact keeps
// a thread on the same head_dim columns for every row it visits, which is
// what lets the backward accumulate dw in registers.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

namespace {

constexpr int QKNR_BLOCK = 256;
constexpr long QKNR_MAX_GRID = 2048;

// ---- 8-element (16 B bf16 / 32 B f32) vector load/store --------------------
template <typename T>
__device__ __forceinline__ void load8(const T* __restrict__ p, float (&v)[8]) {
  if constexpr (sizeof(T) == 2) {
    U4 u;
    u.u = *reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = bf16_bits_to_f32(u.s[j]);
  } else {
    *reinterpret_cast<float4*>(v) = *reinterpret_cast<const float4*>(p);
    *reinterpret_cast<float4*>(v + 4) = *reinterpret_cast<const float4*>(p + 4);
  }
}

template <typename T>
__device__ __forceinline__ void store8(T* __restrict__ p, const float (&v)[8]) {
  if constexpr (sizeof(T) == 2) {
    U4 u;
#pragma unroll
    for (int j = 0; j < 8; ++j) u.s[j] = f32_to_bf16_bits(v[j]);
    *reinterpret_cast<uint4*>(p) = u.u;
  } else {
    *reinterpret_cast<float4*>(p) = *reinterpret_cast<const float4*>(v);
    *reinterpret_cast<float4*>(p + 4) = *reinterpret_cast<const float4*>(v + 4);
  }
}

// The 8 rotation pairs (a[j], b[j]) a thread owns in a row of D elements:
// neox pairs (d0+j, D/2+d0+j); traditional pairs (2(d0+j), 2(d0+j)+1), i.e. 16
// contiguous elements.
template <typename T, bool TRAD>
__device__ __forceinline__ void load_pairs(const T* __restrict__ row, int d0, int half,
                                           float (&a)[8], float (&b)[8]) {
  if constexpr (TRAD) {
    float e0[8], e1[8];
    load8(row + 2 * d0, e0);
    load8(row + 2 * d0 + 8, e1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] = e0[2 * j], b[j] = e0[2 * j + 1];
      a[j + 4] = e1[2 * j], b[j + 4] = e1[2 * j + 1];
    }
  } else {
    load8(row + d0, a);
    load8(row + half + d0, b);
  }
}

template <typename T, bool TRAD>
__device__ __forceinline__ void store_pairs(T* __restrict__ row, int d0, int half,
                                            const float (&a)[8], const float (&b)[8]) {
  if constexpr (TRAD) {
    float e0[8], e1[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      e0[2 * j] = a[j], e0[2 * j + 1] = b[j];
      e1[2 * j] = a[j + 4], e1[2 * j + 1] = b[j + 4];
    }
    store8(row + 2 * d0, e0);
    store8(row + 2 * d0 + 8, e1);
  } else {
    store8(row + d0, a);
    store8(row + half + d0, b);
  }
}

// Sum over the LPR lanes of a row. a + b == b + a bit for bit, so after every
// butterfly step both partners hold the same value: all lanes of the group end
// with the identical sum.
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) v += __shfl_xor(v, m, WAVE);
  return v;
}

// Normalize-and-rotate one row's 8 pairs in place; returns rstd. The forward
// and the decode kernel both call this, and every rounding step is spelled out
// (no contraction left to the compiler), so the two are bit-identical at the
// same position.
template <int D>
__device__ __forceinline__ float qknorm_rope_row(float (&a)[8], float (&b)[8],
                                                 const float (&wa)[8], const float (&wb)[8],
                                                 const float (&c)[8], const float (&s)[8],
                                                 float eps) {
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    ss = __fmaf_rn(a[j], a[j], ss);
    ss = __fmaf_rn(b[j], b[j], ss);
  }
  ss = group_sum<D / 16>(ss);
  const float r = rsqrtf(__fmaf_rn(ss, 1.0f / D, eps));
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float na = __fmul_rn(__fmul_rn(a[j], r), wa[j]);
    const float nb = __fmul_rn(__fmul_rn(b[j], r), wb[j]);
    a[j] = __fmaf_rn(na, c[j], -__fmul_rn(nb, s[j]));
    b[j] = __fmaf_rn(na, s[j], __fmul_rn(nb, c[j]));
  }
  return r;
}

// ---------------- forward ----------------
// x: row-strided [B,S,H,D] view, y: row-strided [B,S,H,D], rstd: [B,S,H] f32.
template <typename T, int D, bool TRAD>
__global__ void __launch_bounds__(QKNR_BLOCK) qknorm_rope_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                       float* __restrict__ rstd,
                                       const T* __restrict__ wq, const T* __restrict__ wk,
                                       const float* __restrict__ cost,
                                       const float* __restrict__ sint,
                                       long total_groups, int S, int H, int Hq, int offset,
                                       float eps, long x_row_stride, long y_row_stride) {
  constexpr int LPR = D / 16, half = D / 2;
  for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < total_groups;
       g += gridDim.x * (long)blockDim.x) {
    const int gi = (int)(g & (LPR - 1));
    const unsigned row = (unsigned)(g / LPR);  // (b*S + s)*H + h < 2^31 (host check)
    const unsigned tok = row / (unsigned)H;    // b*S + s
    const int h = (int)(row - tok * (unsigned)H);
    const int s = (int)(tok % (unsigned)S);
    const int d0 = gi * 8;
    float a[8], b[8], wa[8], wb[8], c[8], sn[8];
    load_pairs<T, TRAD>(x + (long)tok * x_row_stride + (long)h * D, d0, half, a, b);
    load_pairs<T, TRAD>(h < Hq ? wq : wk, d0, half, wa, wb);
    load8(cost + (long)(s + offset) * half + d0, c);
    load8(sint + (long)(s + offset) * half + d0, sn);
    const float r = qknorm_rope_row<D>(a, b, wa, wb, c, sn, eps);
    store_pairs<T, TRAD>(y + (long)tok * y_row_stride + (long)h * D, d0, half, a, b);
    if (gi == 0) rstd[row] = r;
  }
}

// ---------------- decode ----------------
// In place on [B,1,H,D] (batch stride x_b_stride) at the position held in
// device memory, so a captured graph stays position-independent.
template <typename T, int D, bool TRAD>
__global__ void __launch_bounds__(QKNR_BLOCK) qknorm_rope_decode_kernel(T* __restrict__ x,
                                          const T* __restrict__ wq, const T* __restrict__ wk,
                                          const float* __restrict__ cost,
                                          const float* __restrict__ sint,
                                          const int* __restrict__ pos,
                                          int total_groups, int H, int Hq, float eps,
                                          long x_b_stride) {
  constexpr int LPR = D / 16, half = D / 2;
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total_groups) return;  // total_groups % LPR == 0: whole lane groups leave
  const int gi = g & (LPR - 1);
  const int row = g / LPR;  // b*H + h
  const int bi = row / H;
  const int h = row - bi * H;
  const int d0 = gi * 8;
  const int p = *pos;
  T* xr = x + (long)bi * x_b_stride + (long)h * D;
  float a[8], b[8], wa[8], wb[8], c[8], sn[8];
  load_pairs<T, TRAD>(xr, d0, half, a, b);
  load_pairs<T, TRAD>(h < Hq ? wq : wk, d0, half, wa, wb);
  load8(cost + (long)p * half + d0, c);
  load8(sint + (long)p * half + d0, sn);
  qknorm_rope_row<D>(a, b, wa, wb, c, sn, eps);
  store_pairs<T, TRAD>(xr, d0, half, a, b);
}

// ---------------- backward ----------------
// g = RoPE^T(g_r);  dx = r*g*w - x * r^3/D * sum_d(g*w*x);  dw[d] = sum_rows g*x*r.
// The normalized activations are recomputed from the saved pre-norm x and rstd.
// dw: a thread stays on the same 16 columns for the whole grid-stride loop, so
// it accumulates them in registers (q rows and k rows apart); lanes with the
// same columns are then added in a fixed butterfly order, the 4 waves in wave
// order through LDS, and each block stores its partial [2, D] — the host sums
// the partials. No atomics: dw is bit-identical from run to run.
template <typename T, int D, bool TRAD>
__global__ void __launch_bounds__(QKNR_BLOCK) qknorm_rope_bwd_kernel(const T* __restrict__ gr, const T* __restrict__ x,
                                       const float* __restrict__ rstd,
                                       const T* __restrict__ wq, const T* __restrict__ wk,
                                       const float* __restrict__ cost,
                                       const float* __restrict__ sint,
                                       T* __restrict__ dx, float* __restrict__ dw_partial,
                                       long total_groups, int S, int H, int Hq, int offset,
                                       long g_row_stride, long x_row_stride,
                                       long dx_row_stride) {
  constexpr int LPR = D / 16, half = D / 2, NW = QKNR_BLOCK / WAVE;
  __shared__ float wave_dw[NW][2][D];
  const int gi = threadIdx.x & (LPR - 1);  // == g & (LPR-1) on every trip
  const int d0 = gi * 8;
  float dwq_a[8], dwq_b[8], dwk_a[8], dwk_b[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) dwq_a[j] = dwq_b[j] = dwk_a[j] = dwk_b[j] = 0.f;

  for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < total_groups;
       g += gridDim.x * (long)blockDim.x) {
    const unsigned row = (unsigned)(g / LPR);
    const unsigned tok = row / (unsigned)H;
    const int h = (int)(row - tok * (unsigned)H);
    const int s = (int)(tok % (unsigned)S);
    const bool isq = h < Hq;
    float ga[8], gb[8], xa[8], xb[8], wa[8], wb[8], c[8], sn[8];
    load_pairs<T, TRAD>(gr + (long)tok * g_row_stride + (long)h * D, d0, half, ga, gb);
    load_pairs<T, TRAD>(x + (long)tok * x_row_stride + (long)h * D, d0, half, xa, xb);
    load_pairs<T, TRAD>(isq ? wq : wk, d0, half, wa, wb);
    load8(cost + (long)(s + offset) * half + d0, c);
    load8(sint + (long)(s + offset) * half + d0, sn);
    const float r = rstd[row];
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // inverse rotation
      const float ua = ga[j] * c[j] + gb[j] * sn[j];
      const float ub = gb[j] * c[j] - ga[j] * sn[j];
      ga[j] = ua, gb[j] = ub;
      dot += ua * wa[j] * xa[j] + ub * wb[j] * xb[j];
    }
    dot = group_sum<LPR>(dot);
    const float kk = r * r * r * dot * (1.0f / D);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float ta = ga[j] * xa[j] * r, tb = gb[j] * xb[j] * r;
      dwq_a[j] += isq ? ta : 0.f;
      dwq_b[j] += isq ? tb : 0.f;
      dwk_a[j] += isq ? 0.f : ta;
      dwk_b[j] += isq ? 0.f : tb;
      ga[j] = r * ga[j] * wa[j] - xa[j] * kk;
      gb[j] = r * gb[j] * wb[j] - xb[j] * kk;
    }
    store_pairs<T, TRAD>(dx + (long)tok * dx_row_stride + (long)h * D, d0, half, ga, gb);
  }

  // all 64 lanes are back together here; lanes gi, gi+LPR, ... share columns
  const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
#pragma unroll
    for (int m = LPR; m < WAVE; m <<= 1) {
      dwq_a[j] += __shfl_xor(dwq_a[j], m, WAVE);
      dwq_b[j] += __shfl_xor(dwq_b[j], m, WAVE);
      dwk_a[j] += __shfl_xor(dwk_a[j], m, WAVE);
      dwk_b[j] += __shfl_xor(dwk_b[j], m, WAVE);
    }
  }
  if (lane < LPR) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // column of pair element a[j] / b[j] in the weight vector
      const int ca = TRAD ? 2 * (d0 + j) : d0 + j;
      const int cb = TRAD ? 2 * (d0 + j) + 1 : half + d0 + j;
      wave_dw[wid][0][ca] = dwq_a[j];
      wave_dw[wid][0][cb] = dwq_b[j];
      wave_dw[wid][1][ca] = dwk_a[j];
      wave_dw[wid][1][cb] = dwk_b[j];
    }
  }
  __syncthreads();
  float* out = dw_partial + (long)blockIdx.x * 2 * D;
  for (int i = threadIdx.x; i < 2 * D; i += QKNR_BLOCK) {
    float acc = (&wave_dw[0][0][0])[i];
#pragma unroll
    for (int w = 1; w < NW; ++w) acc += (&wave_dw[w][0][0])[i];
    out[i] = acc;
  }
}

// ---------------- host side ----------------
struct QknrView {
  int B, S, H, D;
  long rows;
};

// Element (b,s,h,d) of an accepted view sits at (b*S+s)*row_stride + h*D + d.
// Strides of size-1 dims carry no information, so they are not looked at.
bool bshd_view_ok(const at::Tensor& t) {
  if (t.dim() != 4 || t.stride(3) != 1 || t.stride(2) != t.size(3)) return false;
  return t.size(0) == 1 || t.size(1) == 1 || t.stride(0) == t.size(1) * t.stride(1);
}

long bshd_row_stride(const at::Tensor& t) {
  if (t.size(1) > 1) return t.stride(1);
  return t.size(0) > 1 ? t.stride(0) : t.size(2) * t.size(3);
}

// 16-byte vector accesses: base pointer and row stride must keep every
// 8-element chunk aligned.
bool vec_ok(const at::Tensor& t) {
  const long esz = t.element_size();
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0 &&
         (bshd_row_stride(t) * esz) % 16 == 0;
}

QknrView check_x(const char* who, const at::Tensor& x, long Hq, const at::Tensor& wq,
                 const at::Tensor& wk, const at::Tensor& cost, const at::Tensor& sint) {
  TORCH_CHECK(x.is_cuda() && bshd_view_ok(x), who,
              ": x must be a [B,S,H,D] GPU view with a contiguous (h,d) inner block");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kFloat, who,
              ": bf16 or fp32 only");
  QknrView v{(int)x.size(0), (int)x.size(1), (int)x.size(2), (int)x.size(3), 0};
  v.rows = (long)v.B * v.S * v.H;
  TORCH_CHECK(v.D == 64 || v.D == 128, who, ": head_dim must be 64 or 128, got ", v.D);
  TORCH_CHECK(v.rows > 0 && v.rows < (1L << 31), who, ": B*S*H out of range");
  TORCH_CHECK(Hq >= 0 && Hq <= v.H, who, ": Hq must be in [0, H]");
  for (const at::Tensor* w : {&wq, &wk})
    TORCH_CHECK(w->device() == x.device() && w->scalar_type() == x.scalar_type() &&
                    w->is_contiguous() && w->numel() == v.D &&
                    reinterpret_cast<uintptr_t>(w->data_ptr()) % 16 == 0,
                who, ": norm weights must be contiguous [D] tensors of x's dtype on x's device");
  for (const at::Tensor* t : {&cost, &sint})
    TORCH_CHECK(t->device() == x.device() && t->scalar_type() == at::kFloat &&
                    t->is_contiguous() && t->dim() == 2 && t->size(1) == v.D / 2 &&
                    reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                who, ": cos/sin must be contiguous f32 [Smax, D/2] tables on x's device");
  TORCH_CHECK(vec_ok(x), who, ": x is not 16-byte aligned");
  return v;
}

// Calls f(T tag, D tag, TRAD tag) for the (dtype, head_dim, pairing) at hand.
template <typename F>
void qknr_dispatch(const at::Tensor& x, int D, bool traditional, F&& f) {
  auto with_d = [&](auto ttag) {
    auto with_trad = [&](auto dtag) {
      if (traditional) f(ttag, dtag, std::true_type{});
      else f(ttag, dtag, std::false_type{});
    };
    if (D == 64) with_trad(std::integral_constant<int, 64>{});
    else with_trad(std::integral_constant<int, 128>{});
  };
  if (x.scalar_type() == at::kBFloat16) with_d((__hip_bfloat16*)nullptr);
  else with_d((float*)nullptr);
}

int qknr_grid(long total_groups) {
  return (int)std::min<long>((total_groups + QKNR_BLOCK - 1) / QKNR_BLOCK, QKNR_MAX_GRID);
}

}  // namespace

// x: [B,S,H,D] row-strided view whose first Hq heads are q heads and the rest
// k heads. Returns {y [B,S,H,D] contiguous, rstd [B,S,H] f32}.
std::vector<at::Tensor> qknorm_rope_fwd(at::Tensor x, long Hq, at::Tensor wq, at::Tensor wk,
                                        at::Tensor cost, at::Tensor sint, bool traditional,
                                        long offset, double eps) {
  const QknrView v = check_x("qknorm_rope_fwd", x, Hq, wq, wk, cost, sint);
  TORCH_CHECK(offset >= 0 && cost.size(0) >= v.S + offset && sint.size(0) >= v.S + offset,
              "qknorm_rope_fwd: rope table too small");
  auto y = at::empty({v.B, v.S, v.H, v.D}, x.options());
  auto rstd = at::empty({v.B, v.S, v.H}, x.options().dtype(at::kFloat));
  const long total_groups = v.rows * (v.D / 16);
  auto stream = at::cuda::getCurrentHIPStream();
  qknr_dispatch(x, v.D, traditional, [&](auto ttag, auto dtag, auto trad) {
    using T = std::remove_pointer_t<decltype(ttag)>;
    qknorm_rope_fwd_kernel<T, decltype(dtag)::value, decltype(trad)::value>
        <<<qknr_grid(total_groups), QKNR_BLOCK, 0, stream>>>(
            reinterpret_cast<const T*>(x.data_ptr()), reinterpret_cast<T*>(y.data_ptr()),
            rstd.data_ptr<float>(), reinterpret_cast<const T*>(wq.data_ptr()),
            reinterpret_cast<const T*>(wk.data_ptr()), cost.data_ptr<float>(),
            sint.data_ptr<float>(), total_groups, v.S, v.H, (int)Hq, (int)offset, (float)eps,
            bshd_row_stride(x), bshd_row_stride(y));
  });
  return {y, rstd};
}

// g_r: gradient w.r.t. the rotated output, x: the saved pre-norm view, dx: the
// [B,S,H,D] row-strided view to write (a slice of the fused dQKV buffer).
// Returns dw [2, D] f32: row 0 = dw_q, row 1 = dw_k.
at::Tensor qknorm_rope_bwd(at::Tensor g_r, at::Tensor x, at::Tensor rstd, long Hq,
                           at::Tensor wq, at::Tensor wk, at::Tensor cost, at::Tensor sint,
                           bool traditional, long offset, at::Tensor dx) {
  const char* who = "qknorm_rope_bwd";
  const QknrView v = check_x(who, x, Hq, wq, wk, cost, sint);
  TORCH_CHECK(offset >= 0 && cost.size(0) >= v.S + offset && sint.size(0) >= v.S + offset,
              who, ": rope table too small");
  for (const at::Tensor* t : {&g_r, &dx})
    TORCH_CHECK(t->device() == x.device() && t->scalar_type() == x.scalar_type() &&
                    t->sizes() == x.sizes() && bshd_view_ok(*t) && vec_ok(*t),
                who, ": g_r and dx must be [B,S,H,D] views like x (contiguous (h,d) inner "
                     "block, 16-byte aligned)");
  TORCH_CHECK(rstd.device() == x.device() && rstd.scalar_type() == at::kFloat &&
                  rstd.is_contiguous() && rstd.numel() == v.rows,
              who, ": rstd must be contiguous f32 [B,S,H]");
  const long total_groups = v.rows * (v.D / 16);
  const int grid = qknr_grid(total_groups);
  auto dw_partial = at::empty({grid, 2, v.D}, x.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentHIPStream();
  qknr_dispatch(x, v.D, traditional, [&](auto ttag, auto dtag, auto trad) {
    using T = std::remove_pointer_t<decltype(ttag)>;
    qknorm_rope_bwd_kernel<T, decltype(dtag)::value, decltype(trad)::value>
        <<<grid, QKNR_BLOCK, 0, stream>>>(
            reinterpret_cast<const T*>(g_r.data_ptr()), reinterpret_cast<const T*>(x.data_ptr()),
            rstd.data_ptr<float>(), reinterpret_cast<const T*>(wq.data_ptr()),
            reinterpret_cast<const T*>(wk.data_ptr()), cost.data_ptr<float>(),
            sint.data_ptr<float>(), reinterpret_cast<T*>(dx.data_ptr()),
            dw_partial.data_ptr<float>(), total_groups, v.S, v.H, (int)Hq, (int)offset,
            bshd_row_stride(g_r), bshd_row_stride(x), bshd_row_stride(dx));
  });
  return dw_partial.sum(0);
}

// In place on x [B,1,H,D] (batch-strided view) at the device position `pos`.
void qknorm_rope_decode_(at::Tensor x, long Hq, at::Tensor wq, at::Tensor wk, at::Tensor cost,
                         at::Tensor sint, bool traditional, at::Tensor pos, double eps) {
  const char* who = "qknorm_rope_decode_";
  TORCH_CHECK(x.dim() == 4 && x.size(1) == 1, who, ": x must be [B,1,H,D]");
  const QknrView v = check_x(who, x, Hq, wq, wk, cost, sint);
  TORCH_CHECK(pos.device() == x.device() && pos.scalar_type() == at::kInt && pos.numel() == 1,
              who, ": pos must be a device int32 scalar");
  TORCH_CHECK(v.rows < (1L << 24), who, ": B*H out of range");
  const int total_groups = (int)(v.rows * (v.D / 16));
  auto stream = at::cuda::getCurrentHIPStream();
  qknr_dispatch(x, v.D, traditional, [&](auto ttag, auto dtag, auto trad) {
    using T = std::remove_pointer_t<decltype(ttag)>;
    qknorm_rope_decode_kernel<T, decltype(dtag)::value, decltype(trad)::value>
        <<<(total_groups + QKNR_BLOCK - 1) / QKNR_BLOCK, QKNR_BLOCK, 0, stream>>>(
            reinterpret_cast<T*>(x.data_ptr()), reinterpret_cast<const T*>(wq.data_ptr()),
            reinterpret_cast<const T*>(wk.data_ptr()), cost.data_ptr<float>(),
            sint.data_ptr<float>(), pos.data_ptr<int>(), total_groups, v.H, (int)Hq, (float)eps,
            bshd_row_stride(x));
  });
}
