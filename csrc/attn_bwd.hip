// Tiled FlashAttention-2 backward (kernel K1 bwd).
//
// Deterministic design (no atomics):
//   preprocess  : Drow[b,h,s] = sum_d dO*O  (vectorized 16B loads, 4 rows/wave)
//   dQ kernel   : block per q-tile; recomputes P from (Q,K,lse); accumulates
//                 dQ = (P∘(dP−Drow))·scale @ K in registers
//   dK+dV kernel: block per kv-tile; loops the GQA group's q heads ONCE and
//                 accumulates both dK = dS^T @ Q and dV = P^T @ dO
//                 (attn_bwd_dkdv_kernel: D=128, 8 waves/block, every mod but
//                 blockmask). The two 32x128 fp32 accumulators are 128 VGPRs;
//                 it fits the 256-VGPR budget because the K and V fragments
//                 live in a wave-private LDS image instead of 64 registers.
//   dK kernel / dV kernel (attn_bwd_dkv_kernel): the split pair the merged
//                 kernel replaced — each streams the same Q and dO tiles and
//                 recomputes the same S and P. Still the path for D=64 (both
//                 fit registers there at 2-3 waves/SIMD, not ported), for
//                 the blockmask entry point (not ported: its bits / bias
//                 addressing wants registers the merged kernel does not have
//                 to spare without a re-tune) and under
//                 MCDP_ATTN_BWD_SPLIT=1; attn_bwd_split always runs
//                 it. Both paths share bwd_p_ds_tile, and their dK and dV
//                 are bit-identical (tests/test_gpu_attn_bwd_merged.py).
//   Every entry point goes through run_bwd (bottom of the file): preprocess,
//   dQ, then the merged kernel or the split pair — one launch site per kernel.
//
// Same gfx950 structure as the forward (attn_fwd.hip): 8 waves/block sharing
// every staged tile, DOUBLE-BUFFERED tiles with one barrier per iteration,
// T14 register-prefetch of the next tile under the MFMA clusters, base-2
// exponentials with log2(e) folded into the scale, mask-free fast path on
// interior causal tiles, s_setprio around MFMAs, MFMA layout +
// acc_to_afrag transform from attn_common.h.
//
// The bwd-specific layout trick: ALL images are row-major with the s_tr
// swizzle (attn_common.h), conflict-free for BOTH read shapes — b128 row
// reads AND the k-strided B-fragment gathers, which use gfx950's
// ds_read_b64_tr_b16 hardware transpose-read (tr16_frag). No transposed
// LDS copies are staged anywhere in the backward.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "attn_launch.h"

namespace {

// kv tile per dQ iteration: 64 rows staged per barrier at D=128 (two 32-row
// sub-tiles -> 48 MFMAs/barrier), 128 rows at D=64 (four sub-tiles, 96
// MFMAs/barrier at 166 VGPR) — the dQ kernel overrides this per D.
constexpr int KVB_FILE = 64;
constexpr float LOG2E = 1.4426950408889634f;

// MCDP_ATTN_BWD_SPLIT=1: run the split dK and dV kernels where the merged
// dK+dV kernel is the default (D=128, every mod but blockmask).
inline bool bwd_split() {
  static bool split = []() {
    const char* e = getenv("MCDP_ATTN_BWD_SPLIT");
    return e != nullptr && atoi(e) != 0;
  }();
  return split;
}

// ---------------- preprocess: Drow = rowsum(dO * O) ----------------
// 4 rows per wave: 16 lanes x 8 elements cover a D=128 row in one uint4 load.
__global__ void bwd_preprocess_kernel(const __hip_bfloat16* __restrict__ dout,
                                      const __hip_bfloat16* __restrict__ o,
                                      float* __restrict__ drow,
                                      long rows, int D, long do_rs, int Hq) {
  const int lpr = D / 8;                  // lanes needed per row (16 at D=128)
  const int rpw = WAVE / lpr;             // rows per wave (4 at D=128)
  const int lane = threadIdx.x % WAVE;
  const long row = (blockIdx.x * (long)(256 / WAVE) + threadIdx.x / WAVE) * rpw
                   + lane / lpr;
  if (row >= rows) return;
  const long bs = row / Hq;
  const int h = (int)(row % Hq);
  const int d0 = (lane % lpr) * 8;
  Bf16x8U du, ou;
  *reinterpret_cast<uint4*>(du.s) =
      *reinterpret_cast<const uint4*>(dout + bs * do_rs + (long)h * D + d0);
  *reinterpret_cast<uint4*>(ou.s) =
      *reinterpret_cast<const uint4*>(o + row * D + d0);
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) acc += to_f32(du.h[j]) * to_f32(ou.h[j]);
  // segmented reduce within the lpr-lane group
  for (int off = lpr / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if (lane % lpr == 0) drow[row] = acc;
}

// q-range of kv-tile blocks per mod (in q-row space)
template <int MOD>
__device__ __forceinline__ void q_range_for_kv(int kv0, int kpb, int q_off, int Sq,
                                               int modarg, int& q_lo, int& q_hi) {
  q_lo = 0;
  q_hi = Sq;
  if constexpr (MOD == MOD_CAUSAL || MOD == MOD_ALIBI) {
    q_lo = max(0, kv0 - q_off) & ~31;
  } else if constexpr (MOD == MOD_SLIDING_WINDOW) {
    q_lo = max(0, kv0 - q_off) & ~31;
    q_hi = min(Sq, kv0 + kpb - 1 + modarg - q_off + 1);
  } else if constexpr (MOD == MOD_PREFIX_LM) {
    if (kv0 >= modarg) q_lo = max(0, kv0 - q_off) & ~31;
  }
}

// MOD_DOCUMENT set-up of a kv-tile block: causal q_lo, and the block's last k
// row has the largest end (an ill-formed end in front of q_lo leaves an empty
// range: straight to store). Then this lane's end and the wave's smallest /
// largest one (its first / last k row's; wave-uniform loads) for the
// mask-free test and the per-wave dead-tile skip.
__device__ __forceinline__ void doc_range_for_kv(
    const int* __restrict__ doc_end, int b, int Sq, int Skv, int kvb0, int kpb, int kv0w,
    int krow, bool k_valid, int& q_lo, int& q_hi, int& dend, int& dend_wmin, int& dend_wmax,
    int& kv0u) {
  const int* de = doc_end + (long)b * Skv;
  q_lo = kvb0 & ~31;
  q_hi = max(q_lo, doc_clamp(de[min(kvb0 + kpb - 1, Skv - 1)], Sq));
  kv0u = __builtin_amdgcn_readfirstlane(kv0w);  // the wave's first k row, in an SGPR
  dend = de[k_valid ? krow : 0];
  dend_wmin = de[min(kv0u, Skv - 1)];
  dend_wmax = de[min(kv0u + 31, Skv - 1)];
}

// Attention-logit soft-capping (softcap.h), the one per-element body of the
// capped dQ loop and the capped bwd_p_ds_tile: p comes from the capped score
// t, p = 2^(t * log2e - lse2) with the forward's lse of the capped scores.
// dS = p * (dP - Drow) is then the gradient with respect to t, and the chain
// rule puts dfac = d t / d x = 1 - (t / c)^2 in front of `scale`.
__device__ __forceinline__ float cap_p(float acc, float lse2, const AttnCap& cp, float& dfac) {
  const float t2 = softcap_val(acc, cp.c2, cp.sic);
  dfac = softcap_dfac(t2, cp.inv_c2);
  return __builtin_amdgcn_exp2f(t2 - lse2);
}

// ---------------- dQ kernel (block per q-tile of QPB rows) ----------------
// CAP: the capped instantiations (MOD_NONE / MOD_CAUSAL / MOD_SLIDING_WINDOW)
// take one trailing AttnCap argument; the others do not have it at all.
template <int D, int MOD, bool CAP = false, typename... Cap>
__global__ __launch_bounds__(8 * WAVE) void attn_bwd_dq_kernel(
    const __hip_bfloat16* __restrict__ q, const __hip_bfloat16* __restrict__ k,
    const __hip_bfloat16* __restrict__ v, const __hip_bfloat16* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ drow,
    __hip_bfloat16* __restrict__ dq, const float* __restrict__ slopes,
    int B, int Sq, int Skv, int Hq, int Hkv, float scale, int modarg,
    long q_rs, long k_rs, long v_rs, long do_rs, long dq_rs,
    // MOD_BLOCKMASK only: the forward's device mask tensors (attn_fwd.hip)
    //   mb_gran  uint8 [B,H,ceil(Sq/32),ceil(Skv/64)] 0=masked 1=bits 2=full
    //   mb_bits  uint8 [B,H,Sq,ceil(Skv/8)] per-element keep bits
    //   mb_range int32 [B,H,ceil(Sq/256),2] first/last+1 live 64-row kv tile
    //   bias     bf16  [B,H,Sq,Skv] optional additive score bias (score_mod)
    const unsigned char* __restrict__ mb_gran = nullptr,
    const unsigned char* __restrict__ mb_bits = nullptr,
    const int* __restrict__ mb_range = nullptr,
    const __hip_bfloat16* __restrict__ bias = nullptr,
    // MOD_DOCUMENT only: doc_start int32 [B,Sq] (see attn_fwd.hip)
    const int* __restrict__ doc_start = nullptr, Cap... cap) {
  static_assert(sizeof...(Cap) == (CAP ? 1 : 0), "CAP takes (AttnCap cap)");
  static_assert(!CAP || MOD == MOD_NONE || MOD == MOD_CAUSAL || MOD == MOD_SLIDING_WINDOW,
                "capped instantiations: none, causal, sliding window");
  [[maybe_unused]] const AttnCap cp = attn_cap_arg(cap...);
  // waves per block (NW=4 measured 2.4x slower at D=128: 139 vs 331 TF); the
  // blockmask tensors are laid out for the resulting 256-row q blocks
  constexpr int NW = 8;
  constexpr int TPB = NW * WAVE;
  constexpr int QPB = 32 * NW;
  constexpr int DBLK = D / 16;
  constexpr int DCOL = D / 32;
  // D=64: 128-row kv tiles double the MFMAs per barrier at halved per-tile
  // register cost (mirrors the fwd D=64 KVB bump)
  constexpr int KVB = (D == 64) ? 128 : KVB_FILE;
  // K rm + V rm only: the dQ-accumulate B-fragments (K, k-strided) are read
  // straight from the row-major K image with ds_read_b64_tr_b16 (tr16_frag),
  // so no transposed K image is staged.
  constexpr int TILE = KVB * D * 2;

  __shared__ __align__(16) __hip_bfloat16 smem[2 * TILE];

  const TileMap tmap = tile_map();
  const int b = tmap.batch, hq = tmap.head, qtile = tmap.tile;
  const int hkv = hq / (Hq / Hkv);
  const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
  const int lq = lane & 31, hi = lane >> 5;
  const int q0w = qtile * QPB + wave * 32;
  const int qrow = q0w + lq;
  const bool q_valid = qrow < Sq;
  const int q_off = Skv - Sq;
  const int q_pos = qrow + q_off;
  const float scale2 = scale * LOG2E;
  const float slope2 = (MOD == MOD_ALIBI) ? slopes[hq] * LOG2E : 0.f;

  // Q and dO fragments (B-operand layout: lane holds row q=lq, 8 d values)
  bf16x8 qf[DBLK], dof[DBLK];
  {
    const long row0 = (long)b * Sq + (q_valid ? qrow : 0);
    const long hd = (long)hq * D + hi * 8;
#pragma unroll
    for (int dblk = 0; dblk < DBLK; ++dblk) {
      Bf16x8U uq, ud;
      *reinterpret_cast<uint4*>(uq.s) =
          q_valid ? *reinterpret_cast<const uint4*>(q + row0 * q_rs + hd + dblk * 16) : uint4{0, 0, 0, 0};
      *reinterpret_cast<uint4*>(ud.s) =
          q_valid ? *reinterpret_cast<const uint4*>(dout + row0 * do_rs + hd + dblk * 16) : uint4{0, 0, 0, 0};
      qf[dblk] = uq.v;
      dof[dblk] = ud.v;
    }
  }
  const float Lq2 = (q_valid ? lse[((long)b * Hq + hq) * Sq + qrow] : INFINITY) * LOG2E;
  const float Dq = q_valid ? drow[((long)b * Sq + qrow) * Hq + hq] : 0.f;
  // document mask: this lane's lower bound, and the wave's smallest / largest
  // one (its first / last row's; wave-uniform loads) for the per-wave dead
  // sub-tile skip and the mask-free test
  [[maybe_unused]] int dstart = 0, dstart_wmin = 0, dstart_wmax = 0, q0u = q0w;
  if constexpr (MOD == MOD_DOCUMENT) {
    const int* ds = doc_start + (long)b * Sq;
    q0u = __builtin_amdgcn_readfirstlane(q0w);  // the wave's first row, in an SGPR
    dstart = ds[q_valid ? qrow : 0];
    dstart_wmin = ds[min(q0u, Sq - 1)];
    dstart_wmax = ds[min(q0u + 31, Sq - 1)];
  }

  // kv range (same as forward)
  const int blk_qpos_lo = qtile * QPB + q_off;
  const int blk_qpos_hi = blk_qpos_lo + QPB - 1;
  int kv_lo = 0, kv_hi = Skv;
  if constexpr (MOD == MOD_CAUSAL || MOD == MOD_ALIBI) {
    kv_hi = min(Skv, blk_qpos_hi + 1);
  } else if constexpr (MOD == MOD_SLIDING_WINDOW) {
    kv_hi = min(Skv, blk_qpos_hi + 1);
    kv_lo = max(0, blk_qpos_lo - modarg + 1) & ~(KVB - 1);
  } else if constexpr (MOD == MOD_PREFIX_LM) {
    kv_hi = min(Skv, max(blk_qpos_hi + 1, modarg));
  } else if constexpr (MOD == MOD_BLOCKMASK) {
    // live 64-row kv tiles of this 256-row q block; kv_lo rounds down to this
    // kernel's own tile (128 rows at D=64) — the extra granule is code 0
    const int nqpb = (Sq + QPB - 1) / QPB;
    const int* r = mb_range + (((long)b * Hq + hq) * nqpb + qtile) * 2;
    kv_lo = (r[0] * 64) & ~(KVB - 1);
    kv_hi = min(Skv, r[1] * 64);
    if (kv_hi <= kv_lo) kv_hi = kv_lo;  // fully-masked row block: loop skips
  } else if constexpr (MOD == MOD_DOCUMENT) {
    // the block's first row has the smallest start; kv_lo rounds down to this
    // kernel's own tile (128 rows at D=64)
    kv_hi = min(Skv, blk_qpos_hi + 1);
    kv_lo = doc_clamp(doc_start[(long)b * Sq + qtile * QPB], Skv) & ~(KVB - 1);
  }
  // blockmask: this wave's 32-row granule row and the (b, head) planes of
  // bits / bias — all block- or wave-uniform, so they live in SGPRs. The
  // per-lane row offsets are formed inside the masked path (below): D=128
  // has no VGPRs to spare for row pointers that live across the MFMA loop.
  const unsigned char* gran_row = nullptr;
  const unsigned char* bits_bh = nullptr;
  const __hip_bfloat16* bias_bh = nullptr;
  [[maybe_unused]] const int kvb8 = (Skv + 7) / 8;
  if constexpr (MOD == MOD_BLOCKMASK) {
    const int nq32 = (Sq + 31) / 32;
    const long bh = (long)b * Hq + hq;
    gran_row = mb_gran + (bh * nq32 + min(q0w / 32, nq32 - 1)) * (long)((Skv + 63) / 64);
    bits_bh = mb_bits + bh * Sq * (long)kvb8;
    if (bias != nullptr) bias_bh = bias + bh * Sq * (long)Skv;
  }

  // T14 staging: chunks of (2 kv rows x 8 d); K and V both write row-major.
  constexpr int CH_TOT = (KVB / 2) * (D / 8);  // chunks per tile
  constexpr int NCH = (CH_TOT + TPB - 1) / TPB;
  uint4 kreg[NCH][2], vreg[NCH][2];

  auto stage_load = [&](int kv0) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int u = tid + c * TPB;
      const int row = (u / (D / 8)) * 2;
      const int d0 = (u % (D / 8)) * 8;
      if (row >= KVB) continue;
      const bool ok0 = kv0 + row < Skv;
      const bool ok1 = kv0 + row + 1 < Skv;
      const long kb = ((long)b * Skv + kv0 + row) * k_rs + (long)hkv * D + d0;
      const long vb = ((long)b * Skv + kv0 + row) * v_rs + (long)hkv * D + d0;
      kreg[c][0] = ok0 ? *reinterpret_cast<const uint4*>(k + kb) : uint4{0, 0, 0, 0};
      kreg[c][1] = ok1 ? *reinterpret_cast<const uint4*>(k + kb + k_rs) : uint4{0, 0, 0, 0};
      vreg[c][0] = ok0 ? *reinterpret_cast<const uint4*>(v + vb) : uint4{0, 0, 0, 0};
      vreg[c][1] = ok1 ? *reinterpret_cast<const uint4*>(v + vb + v_rs) : uint4{0, 0, 0, 0};
    }
  };
  auto stage_write = [&](int bufsel) {
    __hip_bfloat16* k_lds = smem + bufsel * TILE;
    __hip_bfloat16* v_lds = k_lds + KVB * D;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int u = tid + c * TPB;
      const int row = (u / (D / 8)) * 2;
      const int d0 = (u % (D / 8)) * 8;
      if (row >= KVB) continue;
      *reinterpret_cast<uint4*>(k_lds + rm_swz<D>(row, d0)) = kreg[c][0];
      *reinterpret_cast<uint4*>(k_lds + rm_swz<D>(row + 1, d0)) = kreg[c][1];
      *reinterpret_cast<uint4*>(v_lds + rm_swz<D>(row, d0)) = vreg[c][0];
      *reinterpret_cast<uint4*>(v_lds + rm_swz<D>(row + 1, d0)) = vreg[c][1];
    }
  };

  float dq_acc[DCOL][16];
#pragma unroll
  for (int dc = 0; dc < DCOL; ++dc)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq_acc[dc][r] = 0.f;

  stage_load(kv_lo);
  stage_write(0);
  __syncthreads();

  int buf = 0;
  for (int kv0 = kv_lo; kv0 < kv_hi; kv0 += KVB) {
    const bool has_next = kv0 + KVB < kv_hi;
    if (has_next) stage_load(kv0 + KVB);

    // 32-row sub-tiles of the staged kv tile (s_tr only uses low row bits,
    // so each sub-image at rows 32h.. is the same layout at a +32h*D offset)
#pragma unroll
    for (int hf = 0; hf < KVB / 32; ++hf) {
      const int kvh = kv0 + hf * 32;
      if (kvh >= kv_hi) break;  // block-uniform (kv_hi is block-level)
      // blockmask: this wave's code for the 64-column granule holding the
      // sub-tile. Code 0 skips the wave's compute only — no barrier lives
      // inside this loop, so the block stays in step.
      [[maybe_unused]] int gcode = 2;
      if constexpr (MOD == MOD_BLOCKMASK) {
        gcode = (q0w < Sq) ? __builtin_amdgcn_readfirstlane((int)gran_row[kvh >> 6]) : 0;
        if (gcode == 0) continue;
      }
      // document: sub-tiles wholly above the wave's diagonal or wholly in
      // front of its first row's document are dead for the whole wave — the
      // same compute-only skip (wave-uniform: all operands are SGPRs)
      if constexpr (MOD == MOD_DOCUMENT) {
        if (kvh > q0u + 31 || kvh + 31 < dstart_wmin) continue;
      }
      const __hip_bfloat16* k_lds = smem + buf * TILE + hf * 32 * D;
      const __hip_bfloat16* v_lds = k_lds + KVB * D;

      // S^T = mfma(K, Q); dP^T = mfma(V, dO) — both (r=k_local, c=q_local)
      f32x16 st = {}, dpt = {};
      // capped, D=128: opaque copies of the lane id (here and before the dQ
      // accumulate), as in the merged dK+dV kernel. The swizzled LDS offsets
      // are then re-formed per sub-tile instead of living across the cap
      // arithmetic: 226 VGPRs and no scratch, against 256 + 32 B without.
      int lane_s = lane;
      if constexpr (CAP && D == 128) asm volatile("" : "+v"(lane_s));
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int dblk = 0; dblk < DBLK; ++dblk) {
        const int off = rm_swz<D>(lane_s & 31, dblk * 16 + (lane_s >> 5) * 8);
        Bf16x8U kf, vf;
        *reinterpret_cast<uint4*>(kf.s) = *reinterpret_cast<const uint4*>(k_lds + off);
        *reinterpret_cast<uint4*>(vf.s) = *reinterpret_cast<const uint4*>(v_lds + off);
        st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf.v, qf[dblk], st, 0, 0, 0);
        dpt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf.v, dof[dblk], dpt, 0, 0, 0);
      }
      __builtin_amdgcn_s_setprio(0);

      // interior half-tiles: every k row kept for every q row of this wave
      // (wave-uniform branch)
      bool full = kvh + 32 <= Skv;
      if constexpr (MOD == MOD_CAUSAL) {
        full = full && (kvh + 31 <= q0w + q_off);
      } else if constexpr (MOD == MOD_SLIDING_WINDOW) {
        full = full && (kvh + 31 <= q0w + q_off) &&
               ((q0w + 31 + q_off) - kvh < modarg);
      } else if constexpr (MOD == MOD_PREFIX_LM) {
        full = full && ((kvh + 31 <= q0w + q_off) || (kvh + 32 <= modarg));
      } else if constexpr (MOD == MOD_ALIBI) {
        full = false;
      } else if constexpr (MOD == MOD_DOCUMENT) {
        // the wave's last row has its largest start
        full = full && (kvh + 31 <= q0u) && (kvh >= dstart_wmax);
      } else if constexpr (MOD == MOD_BLOCKMASK) {
        // code 2 counts out-of-range elements as live, hence the Sq bound;
        // a bias is per element, so it rules the mask-free path out
        full = full && gcode == 2 && bias == nullptr && (q0w + 31 < Sq);
      }

      float ds[16];
      if constexpr (CAP) {
        if (full) {
#pragma unroll
          for (int reg = 0; reg < 16; ++reg) {
            float dfac;
            const float p = cap_p(st[reg], Lq2, cp, dfac);
            ds[reg] = p * (dpt[reg] - Dq) * dfac * scale;
          }
        } else {
#pragma unroll
          for (int reg = 0; reg < 16; ++reg) {
            const int k_pos = kvh + acc_row(reg, hi);
            const bool keep = q_valid && attn_keep<MOD>(q_pos, k_pos, Skv, modarg);
            // the mask rides on the lse operand (p = 2^-inf = 0, every other
            // factor is finite): a select on ds instead keeps st and dpt of
            // both sub-tiles live and spills at D=128
            float dfac;
            const float p = cap_p(st[reg], keep ? Lq2 : INFINITY, cp, dfac);
            ds[reg] = p * (dpt[reg] - Dq) * dfac * scale;
          }
        }
      } else if (full) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const float p = __builtin_amdgcn_exp2f(st[reg] * scale2 - Lq2);
          ds[reg] = p * (dpt[reg] - Dq) * scale;
        }
      } else if constexpr (MOD == MOD_BLOCKMASK) {
        // this lane's 32 keep bits for the sub-tile, read once into a
        // register (bit i = k row kvh+i; rows past Skv read as masked)
        int qr = q_valid ? qrow : 0;
        // opaque copy: keeps the row-offset multiplies here instead of
        // hoisted out of the kv loop into long-lived registers
        asm volatile("" : "+v"(qr));
        const unsigned char* bits_row = bits_bh + (long)qr * kvb8 + (kvh >> 3);
        unsigned kbits = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (kvh + 8 * j < Skv) kbits |= (unsigned)bits_row[j] << (8 * j);
        const __hip_bfloat16* bias_row =
            (bias != nullptr) ? bias_bh + (long)qr * Skv + kvh : nullptr;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int kr = acc_row(reg, hi);
          const bool keep = q_valid && kvh + kr < Skv && ((kbits >> kr) & 1);
          float s2 = st[reg] * scale2;
          if (bias_row != nullptr && keep) s2 += __bfloat162float(bias_row[kr]) * LOG2E;
          const float p = keep ? __builtin_amdgcn_exp2f(s2 - Lq2) : 0.f;
          ds[reg] = p * (dpt[reg] - Dq) * scale;
        }
      } else {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int k_pos = kvh + acc_row(reg, hi);
          bool keep;
          if constexpr (MOD == MOD_DOCUMENT)
            keep = q_valid && k_pos < Skv && k_pos <= q_pos && k_pos >= dstart;
          else
            keep = q_valid && attn_keep<MOD>(q_pos, k_pos, Skv, modarg);
          float s2 = st[reg] * scale2;
          if constexpr (MOD == MOD_ALIBI) s2 += slope2 * (k_pos - q_pos);
          const float p = keep ? __builtin_amdgcn_exp2f(s2 - Lq2) : 0.f;
          ds[reg] = p * (dpt[reg] - Dq) * scale;
        }
      }

      bf16x8 da0, da1;
      acc_to_afrag(ds, da0, da1);  // -> dS[32q x 16k] A-fragments
      int lane_t = lane;
      if constexpr (CAP && D == 128) asm volatile("" : "+v"(lane_t));
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int dc = 0; dc < DCOL; ++dc) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = dq_acc[dc][r];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          // B = K[16k x 32d]: tr_read from the row-major K image
          bf16x8 kb = tr16_frag<D>(k_lds, ks * 16 + (lane_t >> 5) * 8, dc * 32, lane_t);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ks == 0 ? da0 : da1, kb, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) dq_acc[dc][r] = acc[r];
      }
      __builtin_amdgcn_s_setprio(0);
    }

    // write tile t+1 LAST: the whole iteration hides the global-load flight
    // (buf^1 was last read before the previous barrier)
    if (has_next) stage_write(buf ^ 1);

    __syncthreads();
    buf ^= 1;
  }

  // store dq: element (r=q_local, c=d_local)
  int dl = lane & 31, hi_st = hi;
  if constexpr (MOD == MOD_BLOCKMASK) {
    // lane id re-derived here: at D=128 the kernel sits on the 256-VGPR
    // limit and a lane index kept live across the kv loop spilled
    const int l = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    dl = l & 31;
    hi_st = l >> 5;
  }
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int r = acc_row(reg, hi_st);
    const int q_r = q0w + r;
    if (q_r >= Sq) continue;
    __hip_bfloat16* dqr = dq + ((long)b * Sq + q_r) * dq_rs + (long)hq * D + dl;
#pragma unroll
    for (int dc = 0; dc < DCOL; ++dc) dqr[dc * 32] = __float2bfloat16(dq_acc[dc][reg]);
  }
}

// ---------------- P / dS of one 32x32 (q, k) tile, kv-row-major kernels ------
// The one per-element body of the split dK / dV kernels and of the merged
// dK+dV kernel, so all three form p and dS by the same arithmetic (the merged
// results are required to be bit-identical to the split ones).
//   s_acc / dp_acc : S and dP accumulators, element (r=q_local, c=k_local)
//   Ls / Ds        : LDS stats of the tile's 32 q rows (lse*log2e, Drow)
//   full           : wave-uniform, every element of the tile is kept
//   pv  <- p                        (WANT_P)
//   dsv <- p * (dP - Drow) * scale  (WANT_DS)
// CAP (one trailing AttnCap argument): p and dS of the capped scores (cap_p)
//   dsv <- p * (dP - Drow) * (1 - (t / c)^2) * scale
template <int MOD, bool WANT_P, bool WANT_DS, bool CAP = false, typename... Cap>
__device__ __forceinline__ void bwd_p_ds_tile(
    const f32x16& s_acc, const f32x16& dp_acc, const float* Ls, const float* Ds,
    bool full, int hi, int q0, int q_off, int krow, bool k_valid, int Sq, int Skv,
    int modarg, float scale, float scale2, float slope2,
    // MOD_DOCUMENT: this lane's doc end; MOD_BLOCKMASK: bits / bias planes and
    // the (b, q head) plane index
    int dend, const unsigned char* mb_bits, const __hip_bfloat16* bias, long bh, int kvb8,
    float (&pv)[16], float (&dsv)[16], Cap... cap) {
  static_assert(sizeof...(Cap) == (CAP ? 1 : 0), "CAP takes (AttnCap cap)");
  if constexpr (CAP) {
    const AttnCap cp = attn_cap_arg(cap...);
    if (full) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int qr = acc_row(reg, hi);
        float dfac;
        const float p = cap_p(s_acc[reg], Ls[qr], cp, dfac);
        if constexpr (WANT_P) pv[reg] = p;
        if constexpr (WANT_DS) dsv[reg] = p * (dp_acc[reg] - Ds[qr]) * dfac * scale;
      }
    } else {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int qr = acc_row(reg, hi);
        const int q_r = q0 + qr;
        const bool keep =
            k_valid && q_r < Sq && attn_keep<MOD>(q_r + q_off, krow, Skv, modarg);
        float dfac;
        const float p = cap_p(s_acc[reg], Ls[qr], cp, dfac);
        if constexpr (WANT_P) pv[reg] = keep ? p : 0.f;
        if constexpr (WANT_DS) dsv[reg] = keep ? p * (dp_acc[reg] - Ds[qr]) * dfac * scale : 0.f;
      }
    }
  } else if (full) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int qr = acc_row(reg, hi);
      const float p = __builtin_amdgcn_exp2f(s_acc[reg] * scale2 - Ls[qr]);
      if constexpr (WANT_P) pv[reg] = p;
      if constexpr (WANT_DS) dsv[reg] = p * (dp_acc[reg] - Ds[qr]) * scale;
    }
  } else {
    // blockmask: the lane holds ONE k column and 16 q rows, so its
    // keep bits sit in 16 different bits rows (partial granules only)
    [[maybe_unused]] const unsigned char* bits_h = nullptr;
    [[maybe_unused]] const __hip_bfloat16* bias_h = nullptr;
    if constexpr (MOD == MOD_BLOCKMASK) {
      bits_h = mb_bits + bh * Sq * (long)kvb8 + (krow >> 3);
      if (bias != nullptr) bias_h = bias + bh * Sq * (long)Skv + krow;
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int qr = acc_row(reg, hi);
      const int q_r = q0 + qr;
      const int q_pos = q_r + q_off;
      const int k_pos = krow;
      bool keep;
      if constexpr (MOD == MOD_BLOCKMASK) {
        keep = k_valid && q_r < Sq;
        if (keep) keep = (bits_h[(long)q_r * kvb8] >> (krow & 7)) & 1;
      } else if constexpr (MOD == MOD_DOCUMENT) {
        keep = q_r < Sq && k_valid && q_r >= krow && q_r < dend;
      } else {
        keep = k_valid && q_r < Sq && attn_keep<MOD>(q_pos, k_pos, Skv, modarg);
      }
      float s2 = s_acc[reg] * scale2;
      if constexpr (MOD == MOD_ALIBI) s2 += slope2 * (k_pos - q_pos);
      if constexpr (MOD == MOD_BLOCKMASK) {
        if (bias != nullptr && keep)
          s2 += __bfloat162float(bias_h[(long)q_r * Skv]) * LOG2E;
      }
      const float p = keep ? __builtin_amdgcn_exp2f(s2 - Ls[qr]) : 0.f;
      if constexpr (WANT_P) pv[reg] = p;
      if constexpr (WANT_DS) dsv[reg] = p * (dp_acc[reg] - Ds[qr]) * scale;
    }
  }
}

// ---------------- dK / dV kernels (block per kv-tile, loop GQA group) -------
// The split pair: the path for D=64, the blockmask entry point and
// MCDP_ATTN_BWD_SPLIT=1; everything else runs the merged kernel below.
// WANT_DK: true -> dK (needs dP: V frags + dO rm); false -> dV (needs dO^T).
// CAP: capped scores (bwd_p_ds_tile), one trailing AttnCap argument.
template <int D, int MOD, bool WANT_DK, bool CAP = false, typename... Cap>
__global__ __launch_bounds__(8 * WAVE) void attn_bwd_dkv_kernel(
    const __hip_bfloat16* __restrict__ q, const __hip_bfloat16* __restrict__ k,
    const __hip_bfloat16* __restrict__ v, const __hip_bfloat16* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ drow,
    __hip_bfloat16* __restrict__ dkv_out, const float* __restrict__ slopes,
    int B, int Sq, int Skv, int Hq, int Hkv, float scale, int modarg,
    long q_rs, long k_rs, long v_rs, long do_rs, long dkv_rs,
    // MOD_BLOCKMASK only: mb_gran / mb_bits / bias as in the dQ kernel
    // (indexed by the q head), plus the transpose of the forward's range:
    //   mb_qrange int32 [B,H,ceil(Skv/256),2] first/last+1 live 32-row q tile
    const unsigned char* __restrict__ mb_gran = nullptr,
    const unsigned char* __restrict__ mb_bits = nullptr,
    const int* __restrict__ mb_qrange = nullptr,
    const __hip_bfloat16* __restrict__ bias = nullptr,
    // MOD_DOCUMENT only: doc_end int32 [B,Skv], one past the last position of
    // each row's document (non-decreasing along s; same for every head)
    const int* __restrict__ doc_end = nullptr, Cap... cap) {
  static_assert(sizeof...(Cap) == (CAP ? 1 : 0), "CAP takes (AttnCap cap)");
  static_assert(!CAP || MOD == MOD_NONE || MOD == MOD_CAUSAL || MOD == MOD_SLIDING_WINDOW,
                "capped instantiations: none, causal, sliding window");
  constexpr int NW = 8;  // waves per block (NW=4 measured 2.4x slower at D=128)
  constexpr int TPB = NW * WAVE;
  constexpr int KPB = 32 * NW;
  constexpr int DBLK = D / 16;
  constexpr int DCOL = D / 32;
  // q-tile images: Q rm + dO rm, TWO (GQA head, q tile) iterations staged per
  // barrier (sub-tiles s=0,1 at +s*32*D inside each 64-row tensor region).
  // The accumulate B-fragments (Q for dK, dO for dV — k-strided) are
  // tr16_frag reads from the row-major images, so no transposed copy is
  // staged.
  constexpr int TILE = 2 * 64 * D;

  __shared__ __align__(16) __hip_bfloat16 smem[2 * TILE];
  __shared__ float stats_lds[2][2][64];  // [buf][L|D][s*32 + qrow]

  const TileMap tmap = tile_map();
  const int b = tmap.batch, hkv = tmap.head, kvtile = tmap.tile;
  const int group = Hq / Hkv;
  const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
  const int lk = lane & 31, hi = lane >> 5;
  const int kv0w = kvtile * KPB + wave * 32;
  const int krow = kv0w + lk;
  const bool k_valid = krow < Skv;
  const int q_off = Skv - Sq;
  const float scale2 = scale * LOG2E;

  // K (and V for dK) fragments: lane holds row k=lk, 8 d values
  bf16x8 kf[DBLK], vf[WANT_DK ? DBLK : 1];
  {
    const long kr0 = (long)b * Skv + (k_valid ? krow : 0);
    const long khd = (long)hkv * D + hi * 8;
#pragma unroll
    for (int dblk = 0; dblk < DBLK; ++dblk) {
      Bf16x8U ku;
      *reinterpret_cast<uint4*>(ku.s) =
          k_valid ? *reinterpret_cast<const uint4*>(k + kr0 * k_rs + khd + dblk * 16) : uint4{0, 0, 0, 0};
      kf[dblk] = ku.v;
      if constexpr (WANT_DK) {
        Bf16x8U vu;
        *reinterpret_cast<uint4*>(vu.s) =
            k_valid ? *reinterpret_cast<const uint4*>(v + kr0 * v_rs + khd + dblk * 16) : uint4{0, 0, 0, 0};
        vf[dblk] = vu.v;
      }
    }
  }

  float acc_out[DCOL][16];
#pragma unroll
  for (int dc = 0; dc < DCOL; ++dc)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc_out[dc][r] = 0.f;

  int q_lo, q_hi;
  // document mask: this lane's doc end, the wave's smallest / largest one and
  // its first k row in an SGPR (doc_range_for_kv)
  [[maybe_unused]] int dend = 0, dend_wmin = 0, dend_wmax = 0, kv0u = kv0w;
  if constexpr (MOD == MOD_BLOCKMASK) {
    // union of the live q-tile ranges over this kv head's GQA group, so the
    // flat (head, q tile) iteration below stays uniform; heads with nothing
    // live in part of it skip per wave on granule code 0
    const int nkpb = (Skv + KPB - 1) / KPB;
    int t_lo = 0x7fffffff, t_hi = 0;
    for (int g = 0; g < group; ++g) {
      const int* r = mb_qrange + (((long)b * Hq + hkv * group + g) * nkpb + kvtile) * 2;
      if (r[1] > r[0]) {
        t_lo = min(t_lo, r[0]);
        t_hi = max(t_hi, r[1]);
      }
    }
    q_lo = (t_hi > 0) ? t_lo * 32 : 0;
    q_hi = (t_hi > 0) ? min(Sq, t_hi * 32) : 0;  // empty: straight to store
  } else if constexpr (MOD == MOD_DOCUMENT) {
    doc_range_for_kv(doc_end, b, Sq, Skv, kvtile * KPB, KPB, kv0w, krow, k_valid, q_lo, q_hi,
                     dend, dend_wmin, dend_wmax, kv0u);
  } else {
    q_range_for_kv<MOD>(kvtile * KPB, KPB, q_off, Sq, modarg, q_lo, q_hi);
  }
  // blockmask per-wave constants: granule column of this wave's 32 k rows
  // (inside one 64-column granule), this lane's byte/bit in a bits row
  [[maybe_unused]] const int nq32 = (Sq + 31) / 32;
  [[maybe_unused]] const int nkvt = (Skv + 63) / 64;
  [[maybe_unused]] const int kvb8 = (Skv + 7) / 8;

  // sub-tiles per barrier: dV runs two (32 MFMAs/barrier, 220-238 VGPR);
  // dK holds V fragments too and spills at NP=2, so it stays at one.
  // dK at NP=2 re-checked in round 2 (post-NU staging): 256 VGPR with 7
  // spills + 32 B scratch AND occupancy halves (2 blocks/CU -> 1) — stays 1.
  constexpr int NP = WANT_DK ? ((D == 64) ? 2 : 1) : 2;  // dK fits NP=2 at D=64

  // T14 staging of two 32-row q tiles: threads 0..255 own Q chunks
  // (2 rows x 8 d), threads 256..511 own dO chunks; each thread carries one
  // chunk pair per sub-tile.
  constexpr int CH_TOT = (32 / 2) * (D / 8);  // 256 chunks per tensor-tile
  // chunk units per thread: 1 (Q half / dO half split across the 512
  // threads; D=64 leaves the upper 256 idle) — each unit decides Q-vs-dO by
  // its global index
  constexpr int NU = (2 * CH_TOT + TPB - 1) / TPB;
  uint4 sreg[NU][2];  // ONE sub-tile's chunk pairs at a time (split-half
                      // staging: load s -> compute s-1 -> write s)
  // the sub-tile's lse / Drow ride the same pipeline in lanes 0-31 of wave 0:
  // loaded next to the tile, stored to LDS with it, so their latency hides
  // under the compute like the tile's instead of sitting before the barrier
  float st_l = 0.f, st_d = 0.f;

  auto stage_load = [&](int hq_, int q0) {
    if (tid < 32) {
      const int qr = q0 + tid;
      st_l = (qr < Sq) ? lse[((long)b * Hq + hq_) * Sq + qr] : INFINITY;
      st_d = (qr < Sq) ? drow[((long)b * Sq + qr) * Hq + hq_] : 0.f;
    }
#pragma unroll
    for (int cu = 0; cu < NU; ++cu) {
      const int u0 = tid + cu * TPB;
      if (u0 >= 2 * CH_TOT) continue;
      const bool isq = u0 < CH_TOT;
      const int u = isq ? u0 : u0 - CH_TOT;
      const int row = (u / (D / 8)) * 2;
      const int d0 = (u % (D / 8)) * 8;
      const __hip_bfloat16* src = isq ? q : dout;
      const long rs_ = isq ? q_rs : do_rs;
      const bool ok0 = q0 + row < Sq;
      const bool ok1 = q0 + row + 1 < Sq;
      const long base = ((long)b * Sq + q0 + row) * rs_ + (long)hq_ * D + d0;
      sreg[cu][0] = ok0 ? *reinterpret_cast<const uint4*>(src + base) : uint4{0, 0, 0, 0};
      sreg[cu][1] = ok1 ? *reinterpret_cast<const uint4*>(src + base + rs_) : uint4{0, 0, 0, 0};
    }
  };
  auto stage_write = [&](int bufsel, int s) {
    __hip_bfloat16* q_lds = smem + bufsel * TILE;
    __hip_bfloat16* do_lds = q_lds + 64 * D;
#pragma unroll
    for (int cu = 0; cu < NU; ++cu) {
      const int u0 = tid + cu * TPB;
      if (u0 >= 2 * CH_TOT) continue;
      const bool isq = u0 < CH_TOT;
      const int u = isq ? u0 : u0 - CH_TOT;
      const int row = (u / (D / 8)) * 2;
      const int d0 = (u % (D / 8)) * 8;
      __hip_bfloat16* dst = (isq ? q_lds : do_lds) + s * 32 * D;
      *reinterpret_cast<uint4*>(dst + rm_swz<D>(row, d0)) = sreg[cu][0];
      *reinterpret_cast<uint4*>(dst + rm_swz<D>(row + 1, d0)) = sreg[cu][1];
    }
    if (tid < 32) {
      stats_lds[bufsel][0][s * 32 + tid] = st_l * LOG2E;
      stats_lds[bufsel][1][s * 32 + tid] = st_d;
    }
  };

  // iterate (GQA head, q tile) pairs with a flat prefetch pipeline
  const int ntiles = (q_hi - q_lo + 31) / 32;
  const int total_iters = group * ntiles;
  if (total_iters == 0) goto store;

  {
    auto iter_to = [&](int it, int& hq_, int& q0) {
      hq_ = hkv * group + it / ntiles;
      q0 = q_lo + (it % ntiles) * 32;
    };
    int hq0_, q00;
    iter_to(0, hq0_, q00);
    stage_load(hq0_, q00);
    stage_write(0, 0);
    if (NP == 2 && total_iters > 1) {
      int hq1_, q01;
      iter_to(1, hq1_, q01);
      stage_load(hq1_, q01);
      stage_write(0, 1);
    }
    __syncthreads();

    int buf = 0;
    for (int it0 = 0; it0 < total_iters; it0 += NP) {
      const int npair = min(NP, total_iters - it0);
      const bool has_next = it0 + NP < total_iters;
      const int nleft = total_iters - it0 - NP;  // sub-tiles in the next pair

      // split-half staging: next pair's half h loads during THIS pair's
      // half h compute and is written to buf^1 right after it (buf^1 was
      // last read before the previous barrier, so the write is race-free)
      if (has_next) {
        int nhq, nq0;
        iter_to(it0 + NP, nhq, nq0);
        stage_load(nhq, nq0);
      }

#pragma unroll
      for (int s = 0; s < NP; ++s) {
        if (s >= npair) break;  // block-uniform
        int hq_, q0;
        iter_to(it0 + s, hq_, q0);
        const float slope2 = (MOD == MOD_ALIBI) ? slopes[hq_] * LOG2E : 0.f;
        const __hip_bfloat16* q_lds = smem + buf * TILE + s * 32 * D;
        const __hip_bfloat16* do_lds = smem + buf * TILE + 64 * D + s * 32 * D;

        // blockmask: the wave's 32 k rows lie inside one 64-column granule;
        // the code is per q head. Code 0 skips the wave's compute only — the
        // staging epilogue and the barrier below still run.
        [[maybe_unused]] int gcode = 2;
        if constexpr (MOD == MOD_BLOCKMASK) {
          const long gi = (((long)b * Hq + hq_) * nq32 + (q0 >> 5)) * (long)nkvt + (kv0w >> 6);
          gcode = (kv0w < Skv) ? __builtin_amdgcn_readfirstlane((int)mb_gran[gi]) : 0;
        }
        // document: a q tile wholly above the wave's first k row, or wholly
        // past its last k row's document, is dead for the whole wave — same
        // compute-only skip (all operands are SGPRs)
        if constexpr (MOD == MOD_DOCUMENT) {
          gcode = (kv0u < Skv && q0 + 31 >= kv0u && q0 < dend_wmax) ? 1 : 0;
        }
        if ((MOD != MOD_BLOCKMASK && MOD != MOD_DOCUMENT) || gcode != 0) {
          // S = mfma(Q, K^T): A=Q rm frags from LDS, B = register kf.
          // element (r=q_local, c=k_local)
          f32x16 s_acc = {}, dp_acc = {};
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int dblk = 0; dblk < DBLK; ++dblk) {
            const int off = rm_swz<D>(lk, dblk * 16 + hi * 8);
            Bf16x8U qa;
            *reinterpret_cast<uint4*>(qa.s) = *reinterpret_cast<const uint4*>(q_lds + off);
            s_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa.v, kf[dblk], s_acc, 0, 0, 0);
            if constexpr (WANT_DK) {
              Bf16x8U da;
              *reinterpret_cast<uint4*>(da.s) = *reinterpret_cast<const uint4*>(do_lds + off);
              dp_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da.v, vf[dblk], dp_acc, 0, 0, 0);
            }
          }
          __builtin_amdgcn_s_setprio(0);

          // interior (q tile entirely below this wave's k rows): mask-free
          bool full = q0 + 31 < Sq;
          if constexpr (MOD == MOD_CAUSAL) {
            full = full && (q0 + q_off >= kv0w + 31);
          } else if constexpr (MOD == MOD_SLIDING_WINDOW) {
            full = full && (q0 + q_off >= kv0w + 31) &&
                   ((q0 + 31 + q_off) - kv0w < modarg);
          } else if constexpr (MOD == MOD_PREFIX_LM) {
            // second clause wave-uniform: whole wave's k rows inside the prefix
            full = full && ((q0 + q_off >= kv0w + 31) || (kv0w + 31 < modarg));
          } else if constexpr (MOD == MOD_DOCUMENT) {
            // the wave's first k row has its smallest end
            full = full && (q0 >= kv0u + 31) && (q0 + 31 < dend_wmin);
          } else if constexpr (MOD == MOD_BLOCKMASK) {
            // code 2 counts out-of-range elements as live, hence the bounds;
            // a bias is per element, so it rules the mask-free path out
            full = full && gcode == 2 && bias == nullptr && (kv0w + 31 < Skv);
          } else {
            full = false;  // MOD_NONE boundary Sq checks + ALIBI slope
          }

          // dS (dK) or P (dV) of the tile; the other array stays unused
          float pv[16], pv_unused[16];
          bwd_p_ds_tile<MOD, !WANT_DK, WANT_DK, CAP>(
              s_acc, dp_acc, &stats_lds[buf][0][s * 32], &stats_lds[buf][1][s * 32], full, hi,
              q0, q_off, krow, k_valid, Sq, Skv, modarg, scale, scale2, slope2, dend, mb_bits,
              bias, (long)b * Hq + hq_, kvb8, WANT_DK ? pv_unused : pv, WANT_DK ? pv : pv_unused,
              cap...);

          // transform: acc holds M[r=q][c=k]; A-frags of M^T = dS^T (dK) / P^T (dV)
          bf16x8 a0, a1;
          acc_to_afrag(pv, a0, a1);
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int dc = 0; dc < DCOL; ++dc) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = acc_out[dc][r];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
              // B = X[16q x 32d] (X = Q for dK, dO for dV): tr_read from rm image
              bf16x8 xb = tr16_frag<D>(WANT_DK ? q_lds : do_lds, ks * 16 + hi * 8,
                                       dc * 32, lane);
              acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ks == 0 ? a0 : a1, xb, acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) acc_out[dc][r] = acc[r];
          }
          __builtin_amdgcn_s_setprio(0);
        }

        // split-half staging epilogue: write the half that loaded during
        // this half's compute, then start the next half's load
        if (has_next) {
          if (s == 0) {
            stage_write(buf ^ 1, 0);
            if (NP == 2 && nleft > 1) {
              int nhq, nq0;
              iter_to(it0 + NP + 1, nhq, nq0);
              stage_load(nhq, nq0);
            }
          } else if (nleft > 1) {
            stage_write(buf ^ 1, 1);
          }
        }
      }

      __syncthreads();
      buf ^= 1;
    }
  }

store:
  // store: element (r=k_local, c=d_local)
  {
    const int dl = lane & 31;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int r = acc_row(reg, hi);
      const int k_r = kv0w + r;
      if (k_r >= Skv) continue;
      __hip_bfloat16* out = dkv_out + ((long)b * Skv + k_r) * dkv_rs + (long)hkv * D + dl;
#pragma unroll
      for (int dc = 0; dc < DCOL; ++dc) out[dc * 32] = __float2bfloat16(acc_out[dc][reg]);
    }
  }
}

// ---------------- merged dK + dV kernel (block per kv-tile) -----------------
// One pass over the (GQA head, q tile) sequence of the split kernels, in the
// same order, with BOTH 32x128 fp32 accumulators per wave (128 VGPRs): Q and
// dO are staged once, S and P are formed once, one barrier per q tile.
// What makes it fit 256 VGPRs: the K and V fragments (64 registers in the
// split dK kernel) live in a wave-private LDS image instead, written once in
// the prologue in fragment order [dblk][lane] x 16 B — no other wave reads a
// wave's 32 rows, so no swizzle is needed and each ds_read_b128 is one
// contiguous 1 KB. The last K dblk stays in 4 registers, which is what keeps
// the static LDS under the 160 KB limit:
//   Q/dO tiles 2 x 16 KB + K image 8 x 7 KB + V image 8 x 8 KB + stats 512 B.
// p and dS come from bwd_p_ds_tile and each accumulator sees its MFMAs in
// the split kernels' order, so dK and dV are bit-identical to theirs.
// CAP: capped scores (bwd_p_ds_tile), one trailing AttnCap argument.
template <int D, int MOD, bool CAP = false, typename... Cap>
__global__ __launch_bounds__(8 * WAVE) void attn_bwd_dkdv_kernel(
    const __hip_bfloat16* __restrict__ q, const __hip_bfloat16* __restrict__ k,
    const __hip_bfloat16* __restrict__ v, const __hip_bfloat16* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ drow,
    __hip_bfloat16* __restrict__ dk_out, __hip_bfloat16* __restrict__ dv_out,
    const float* __restrict__ slopes,
    int B, int Sq, int Skv, int Hq, int Hkv, float scale, int modarg,
    long q_rs, long k_rs, long v_rs, long do_rs, long dk_rs, long dv_rs,
    // MOD_DOCUMENT only: doc_end int32 [B,Skv], as in the split kernels
    const int* __restrict__ doc_end = nullptr, Cap... cap) {
  static_assert(sizeof...(Cap) == (CAP ? 1 : 0), "CAP takes (AttnCap cap)");
  static_assert(!CAP || MOD == MOD_NONE || MOD == MOD_CAUSAL || MOD == MOD_SLIDING_WINDOW,
                "capped instantiations: none, causal, sliding window");
  static_assert(D == 128, "merged dK+dV kernel is built for D=128");
  static_assert(MOD != MOD_BLOCKMASK, "blockmask stays on the split kernels");
  constexpr int NW = 8;
  constexpr int TPB = NW * WAVE;
  constexpr int KPB = 32 * NW;
  constexpr int DBLK = D / 16;
  constexpr int DCOL = D / 32;
  constexpr int TILE = 2 * 32 * D;         // one 32-row Q tile + one 32-row dO tile
  constexpr int FRAG = WAVE * 8;           // elements of one [lane] x 16 B fragment block
  constexpr int KIMG = (DBLK - 1) * FRAG;  // per-wave K image (last dblk in registers)
  constexpr int WIMG = KIMG + DBLK * FRAG; // per-wave K image + V image

  __shared__ __align__(16) __hip_bfloat16 smem[2 * TILE + NW * WIMG];
  __shared__ float stats_lds[2][2][32];  // [buf][L|D][qrow]
  static_assert(sizeof(smem) + sizeof(stats_lds) <= 160 * 1024, "LDS budget");

  const TileMap tmap = tile_map();
  const int b = tmap.batch, hkv = tmap.head, kvtile = tmap.tile;
  const int group = Hq / Hkv;
  const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
  const int lk = lane & 31, hi = lane >> 5;
  const int kv0w = kvtile * KPB + wave * 32;
  const int krow = kv0w + lk;
  const bool k_valid = krow < Skv;
  const int q_off = Skv - Sq;
  const float scale2 = scale * LOG2E;

  // K / V fragments (lane holds row k=lk, 8 d values; rows past Skv are
  // zeros) -> this wave's image. Only this wave reads it back, and the first
  // barrier below sits between these writes and the first read anyway.
  __hip_bfloat16* const kimg = smem + 2 * TILE + wave * WIMG + lane * 8;
  __hip_bfloat16* const vimg = kimg + KIMG;
  bf16x8 kf_last;
  {
    const long kr0 = (long)b * Skv + (k_valid ? krow : 0);
    const long khd = (long)hkv * D + hi * 8;
#pragma unroll
    for (int dblk = 0; dblk < DBLK; ++dblk) {
      Bf16x8U ku, vu;
      *reinterpret_cast<uint4*>(ku.s) =
          k_valid ? *reinterpret_cast<const uint4*>(k + kr0 * k_rs + khd + dblk * 16) : uint4{0, 0, 0, 0};
      *reinterpret_cast<uint4*>(vu.s) =
          k_valid ? *reinterpret_cast<const uint4*>(v + kr0 * v_rs + khd + dblk * 16) : uint4{0, 0, 0, 0};
      if (dblk < DBLK - 1)
        *reinterpret_cast<uint4*>(kimg + dblk * FRAG) = *reinterpret_cast<uint4*>(ku.s);
      else
        kf_last = ku.v;
      *reinterpret_cast<uint4*>(vimg + dblk * FRAG) = *reinterpret_cast<uint4*>(vu.s);
    }
  }

  float dk_acc[DCOL][16], dv_acc[DCOL][16];
#pragma unroll
  for (int dc = 0; dc < DCOL; ++dc)
#pragma unroll
    for (int r = 0; r < 16; ++r) dk_acc[dc][r] = dv_acc[dc][r] = 0.f;

  int q_lo, q_hi;
  // document mask, as in the split kernels (doc_range_for_kv)
  [[maybe_unused]] int dend = 0, dend_wmin = 0, dend_wmax = 0, kv0u = kv0w;
  if constexpr (MOD == MOD_DOCUMENT) {
    doc_range_for_kv(doc_end, b, Sq, Skv, kvtile * KPB, KPB, kv0w, krow, k_valid, q_lo, q_hi,
                     dend, dend_wmin, dend_wmax, kv0u);
  } else {
    q_range_for_kv<MOD>(kvtile * KPB, KPB, q_off, Sq, modarg, q_lo, q_hi);
  }

  // T14 staging of one 32-row q tile: threads 0..255 own Q chunks (2 rows x
  // 8 d), threads 256..511 own dO chunks; lanes 0-31 of wave 0 carry the
  // tile's lse / Drow through the same load -> write pipeline.
  constexpr int CH_TOT = (32 / 2) * (D / 8);  // 256 chunks per tensor-tile
  static_assert(2 * CH_TOT == TPB, "one chunk pair per thread");
  uint4 sreg[2];
  float st_l = 0.f, st_d = 0.f;
  // waves 0-3 stage Q, waves 4-7 dO: wave-uniform, so the source pointer and
  // row stride stay in SGPRs
  const bool isq = __builtin_amdgcn_readfirstlane(wave) < NW / 2;
  const int su = isq ? tid : tid - CH_TOT;
  const int srow = (su / (D / 8)) * 2;
  const int sd0 = (su % (D / 8)) * 8;

  auto stage_load = [&](int hq_, int q0) {
    if (tid < 32) {
      const int qr = q0 + tid;
      st_l = (qr < Sq) ? lse[((long)b * Hq + hq_) * Sq + qr] : INFINITY;
      st_d = (qr < Sq) ? drow[((long)b * Sq + qr) * Hq + hq_] : 0.f;
    }
    const __hip_bfloat16* src = isq ? q : dout;
    const long rs_ = isq ? q_rs : do_rs;
    const bool ok0 = q0 + srow < Sq;
    const bool ok1 = q0 + srow + 1 < Sq;
    const long base = ((long)b * Sq + q0 + srow) * rs_ + (long)hq_ * D + sd0;
    sreg[0] = ok0 ? *reinterpret_cast<const uint4*>(src + base) : uint4{0, 0, 0, 0};
    sreg[1] = ok1 ? *reinterpret_cast<const uint4*>(src + base + rs_) : uint4{0, 0, 0, 0};
  };
  auto stage_write = [&](int bufsel) {
    __hip_bfloat16* dst = smem + bufsel * TILE + (isq ? 0 : 32 * D);
    *reinterpret_cast<uint4*>(dst + rm_swz<D>(srow, sd0)) = sreg[0];
    *reinterpret_cast<uint4*>(dst + rm_swz<D>(srow + 1, sd0)) = sreg[1];
    if (tid < 32) {
      stats_lds[bufsel][0][tid] = st_l * LOG2E;
      stats_lds[bufsel][1][tid] = st_d;
    }
  };

  // iterate (GQA head, q tile) pairs with a flat prefetch pipeline
  const int ntiles = (q_hi - q_lo + 31) / 32;
  const int total_iters = group * ntiles;
  if (total_iters == 0) goto store;

  {
    auto iter_to = [&](int it, int& hq_, int& q0) {
      hq_ = hkv * group + it / ntiles;
      q0 = q_lo + (it % ntiles) * 32;
    };
    int hq0_, q00;
    iter_to(0, hq0_, q00);
    stage_load(hq0_, q00);
    stage_write(0);
    __syncthreads();

    // this wave's compute for one (GQA head, q tile) staged in buffer buf
    auto tile_compute = [&](int hq_, int q0, int buf) {
      const float slope2 = (MOD == MOD_ALIBI) ? slopes[hq_] * LOG2E : 0.f;
      const __hip_bfloat16* q_lds = smem + buf * TILE;
      const __hip_bfloat16* do_lds = q_lds + 32 * D;

      // S = mfma(Q, K^T), dP = mfma(dO, V^T): A = Q / dO rm frags, B = K / V
      // frags from the wave's image; element (r=q_local, c=k_local)
      f32x16 s_acc = {}, dp_acc = {};
      // opaque copies of the lane id (here and before the accumulates): the
      // swizzled LDS offsets derived from them are re-formed per iteration
      // (a few VALU ops) instead of being hoisted out of the loop into ~16
      // registers that would be live across the P / dS phase, where the
      // kernel sits on the 256-VGPR limit
      int lane_s = lane;
      asm volatile("" : "+v"(lane_s));
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int dblk = 0; dblk < DBLK; ++dblk) {
        const int off = rm_swz<D>(lane_s & 31, dblk * 16 + (lane_s >> 5) * 8);
        Bf16x8U qa, da, kb, vb;
        *reinterpret_cast<uint4*>(qa.s) = *reinterpret_cast<const uint4*>(q_lds + off);
        if (dblk < DBLK - 1)
          *reinterpret_cast<uint4*>(kb.s) = *reinterpret_cast<const uint4*>(kimg + dblk * FRAG);
        else
          kb.v = kf_last;
        *reinterpret_cast<uint4*>(da.s) = *reinterpret_cast<const uint4*>(do_lds + off);
        *reinterpret_cast<uint4*>(vb.s) = *reinterpret_cast<const uint4*>(vimg + dblk * FRAG);
        s_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa.v, kb.v, s_acc, 0, 0, 0);
        dp_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da.v, vb.v, dp_acc, 0, 0, 0);
      }
      __builtin_amdgcn_s_setprio(0);

      // interior (q tile entirely below this wave's k rows): mask-free
      bool full = q0 + 31 < Sq;
      if constexpr (MOD == MOD_CAUSAL) {
        full = full && (q0 + q_off >= kv0w + 31);
      } else if constexpr (MOD == MOD_SLIDING_WINDOW) {
        full = full && (q0 + q_off >= kv0w + 31) &&
               ((q0 + 31 + q_off) - kv0w < modarg);
      } else if constexpr (MOD == MOD_PREFIX_LM) {
        full = full && ((q0 + q_off >= kv0w + 31) || (kv0w + 31 < modarg));
      } else if constexpr (MOD == MOD_DOCUMENT) {
        // the wave's first k row has its smallest end
        full = full && (q0 >= kv0u + 31) && (q0 + 31 < dend_wmin);
      } else {
        full = false;  // MOD_NONE boundary Sq checks + ALIBI slope
      }

      float pv[16], dsv[16];
      bwd_p_ds_tile<MOD, true, true, CAP>(
          s_acc, dp_acc, &stats_lds[buf][0][0], &stats_lds[buf][1][0], full, hi, q0, q_off,
          krow, k_valid, Sq, Skv, modarg, scale, scale2, slope2, dend, nullptr, nullptr, 0, 0,
          pv, dsv, cap...);

      // dV += P^T . dO first: the packed P fragments die before dK starts
      int lane_t = lane;
      {
        bf16x8 a0, a1;
        acc_to_afrag(pv, a0, a1);
        asm volatile("" : "+v"(lane_t));
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int dc = 0; dc < DCOL; ++dc) {
          f32x16 acc;
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = dv_acc[dc][r];
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            bf16x8 xb = tr16_frag<D>(do_lds, ks * 16 + (lane_t >> 5) * 8, dc * 32, lane_t);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ks == 0 ? a0 : a1, xb, acc, 0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) dv_acc[dc][r] = acc[r];
        }
        __builtin_amdgcn_s_setprio(0);
      }
      // dK += dS^T . Q
      {
        bf16x8 a0, a1;
        acc_to_afrag(dsv, a0, a1);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int dc = 0; dc < DCOL; ++dc) {
          f32x16 acc;
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = dk_acc[dc][r];
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            bf16x8 xb = tr16_frag<D>(q_lds, ks * 16 + (lane_t >> 5) * 8, dc * 32, lane_t);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ks == 0 ? a0 : a1, xb, acc, 0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) dk_acc[dc][r] = acc[r];
        }
        __builtin_amdgcn_s_setprio(0);
      }
    };

    int buf = 0;
    for (int it = 0; it < total_iters; ++it) {
      const bool has_next = it + 1 < total_iters;
      // the next tile loads during this tile's compute and is written to
      // buf^1 after it (buf^1 was last read before the previous barrier)
      if (has_next) {
        int nhq, nq0;
        iter_to(it + 1, nhq, nq0);
        stage_load(nhq, nq0);
      }
      int hq_, q0;
      iter_to(it, hq_, q0);
      // document: a q tile wholly above the wave's first k row, or wholly
      // past its last k row's document, is dead for the whole wave — skip
      // the compute only (all operands are SGPRs), staging and barrier run
      bool live = true;
      if constexpr (MOD == MOD_DOCUMENT)
        live = kv0u < Skv && q0 + 31 >= kv0u && q0 < dend_wmax;
      if (live) tile_compute(hq_, q0, buf);

      if (has_next) stage_write(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  }

store:
  // store: element (r=k_local, c=d_local)
  {
    const int dl = lane & 31;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int r = acc_row(reg, hi);
      const int k_r = kv0w + r;
      if (k_r >= Skv) continue;
      const long o = (long)hkv * D + dl;
      __hip_bfloat16* outk = dk_out + ((long)b * Skv + k_r) * dk_rs + o;
      __hip_bfloat16* outv = dv_out + ((long)b * Skv + k_r) * dv_rs + o;
#pragma unroll
      for (int dc = 0; dc < DCOL; ++dc) {
        outk[dc * 32] = __float2bfloat16(dk_acc[dc][reg]);
        outv[dc * 32] = __float2bfloat16(dv_acc[dc][reg]);
      }
    }
  }
}

// The one backward launch sequence: Drow, dQ, then dK and dV. 8 waves per
// block of 256 q rows (dQ) / 256 kv rows (dK, dV).
// CAP: the capped instantiations, with make_attn_cap(a.cap, a.scale) as their
// trailing argument; the others are launched exactly as before.
template <int MOD, bool CAP = false>
void run_bwd(const AttnArgs& a, const at::Tensor& q, bool force_split) {
  auto drow_t = at::empty({(long)a.B * a.Sq * a.Hq}, q.options().dtype(at::kFloat));
  const float* drow = drow_t.data_ptr<float>();
  auto stream = at::cuda::getCurrentHIPStream();
  {  // preprocess: 4 rows per wave at D=128 (vectorized 16 B loads)
    const long rows = (long)a.B * a.Sq * a.Hq;
    const int rpw = WAVE / (a.D / 8);
    const long grid = cdiv(rows, (long)(256 / WAVE) * rpw);
    bwd_preprocess_kernel<<<grid, 256, 0, stream>>>(a.dout, a.o, drow_t.data_ptr<float>(), rows,
                                                    a.D, a.do_rs, a.Hq);
  }
  constexpr int BLK = 8 * 32;
  const dim3 gq(cdiv(a.Sq, BLK), a.Hq, a.B), gkv(cdiv(a.Skv, BLK), a.Hkv, a.B), block(8 * WAVE);
  const bool split = force_split || bwd_split();
  // launch(cap...) with the cap argument when CAP, with nothing otherwise
  auto with_cap = [&](auto&& launch) {
    if constexpr (CAP) launch(make_attn_cap(a.cap, a.scale));
    else launch();
  };
  with_head_dim(a.D, [&](auto dtag) {
    constexpr int D = decltype(dtag)::value;
    with_cap([&](auto... cap) {
      attn_bwd_dq_kernel<D, MOD, CAP><<<gq, block, 0, stream>>>(
          a.q, a.k, a.v, a.dout, a.lse, drow, a.dq, a.slopes, a.B, a.Sq, a.Skv, a.Hq, a.Hkv,
          a.scale, a.modarg, a.q_rs, a.k_rs, a.v_rs, a.do_rs, a.dq_rs,
          a.gran, a.bits, a.range, a.bias, a.doc_start, cap...);
    });
    // merged dK+dV at D=128 (D=64 and blockmask keep the split pair)
    if constexpr (D == 128 && MOD != MOD_BLOCKMASK) {
      if (!split) {
        with_cap([&](auto... cap) {
          attn_bwd_dkdv_kernel<D, MOD, CAP><<<gkv, block, 0, stream>>>(
              a.q, a.k, a.v, a.dout, a.lse, drow, a.dk, a.dv, a.slopes, a.B, a.Sq, a.Skv, a.Hq,
              a.Hkv, a.scale, a.modarg, a.q_rs, a.k_rs, a.v_rs, a.do_rs, a.dk_rs, a.dv_rs,
              a.doc_end, cap...);
        });
        return;
      }
    }
    auto dkv = [&](auto want_dk, __hip_bfloat16* out, long out_rs) {
      with_cap([&](auto... cap) {
        attn_bwd_dkv_kernel<D, MOD, decltype(want_dk)::value, CAP><<<gkv, block, 0, stream>>>(
            a.q, a.k, a.v, a.dout, a.lse, drow, out, a.slopes, a.B, a.Sq, a.Skv, a.Hq, a.Hkv,
            a.scale, a.modarg, a.q_rs, a.k_rs, a.v_rs, a.do_rs, out_rs,
            a.gran, a.bits, a.qrange, a.bias, a.doc_end, cap...);
      });
    };
    dkv(std::true_type{}, a.dk, a.dk_rs);
    dkv(std::false_type{}, a.dv, a.dv_rs);
  });
}

// Checks shared by every entry point. dq/dk/dv may be empty (allocated here)
// or pre-allocated row-strided views (slices of a fused dQKV grad buffer).
AttnArgs bwd_args(const char* who, at::Tensor& q, at::Tensor& k, at::Tensor& v, at::Tensor& o,
                  at::Tensor& dout, at::Tensor& lse, double scale, at::Tensor& dq,
                  at::Tensor& dk, at::Tensor& dv) {
  AttnArgs a = check_qkv(who, q, k, v, scale);
  check_o_dout_lse(who, a, q, o, dout, lse);
  a.dq_rs = check_out_view(who, dq, q, a.Sq, a.Hq);
  a.dk_rs = check_out_view(who, dk, q, a.Skv, a.Hkv);
  a.dv_rs = check_out_view(who, dv, q, a.Skv, a.Hkv);
  a.dq = bf16_out(dq), a.dk = bf16_out(dk), a.dv = bf16_out(dv);
  return a;
}

std::vector<at::Tensor> attn_bwd_impl(const char* who, at::Tensor q, at::Tensor k, at::Tensor v,
                                      at::Tensor o, at::Tensor dout, at::Tensor lse,
                                      double scale, long mod, long modarg, at::Tensor slopes,
                                      at::Tensor dq, at::Tensor dk, at::Tensor dv,
                                      bool force_split) {
  AttnArgs a = bwd_args(who, q, k, v, o, dout, lse, scale, dq, dk, dv);
  check_slopes(who, a, mod, slopes, q);
  a.modarg = (int)modarg;
  with_mod(who, mod, [&](auto mtag) { run_bwd<decltype(mtag)::value>(a, q, force_split); });
  return {dq, dk, dv};
}

}  // namespace

// dq/dk/dv: absent or empty -> allocated here; else row-strided out views
// (slices of a fused dQKV grad buffer) that the kernels write in place.
using OptTensor = c10::optional<at::Tensor>;

std::vector<at::Tensor> attn_bwd(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
                                 at::Tensor dout, at::Tensor lse, double scale, long mod,
                                 long modarg, at::Tensor slopes,
                                 OptTensor dq, OptTensor dk, OptTensor dv) {
  return attn_bwd_impl("attn_bwd", q, k, v, o, dout, lse, scale, mod, modarg, slopes,
                       dq.value_or(at::Tensor()), dk.value_or(at::Tensor()),
                       dv.value_or(at::Tensor()), false);
}

// attn_bwd on the split dK / dV kernels whatever the default is, so a test
// can compare the two paths inside one process.
std::vector<at::Tensor> attn_bwd_split(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
                                       at::Tensor dout, at::Tensor lse, double scale, long mod,
                                       long modarg, at::Tensor slopes) {
  return attn_bwd_impl("attn_bwd_split", q, k, v, o, dout, lse, scale, mod, modarg, slopes,
                       {}, {}, {}, true);
}

// Backward of attn_cap_fwd: o and lse are those of the capped scores.
// attn_cap_bwd takes dq/dk/dv like attn_bwd; attn_cap_bwd_split always runs the
// split dK / dV kernels.
std::vector<at::Tensor> attn_cap_bwd_impl(const char* who, at::Tensor q, at::Tensor k,
                                          at::Tensor v, at::Tensor o, at::Tensor dout,
                                          at::Tensor lse, double scale, long mod, long modarg,
                                          double cap, at::Tensor dq, at::Tensor dk, at::Tensor dv,
                                          bool force_split) {
  AttnArgs a = bwd_args(who, q, k, v, o, dout, lse, scale, dq, dk, dv);
  check_cap(who, a, cap);
  a.modarg = (int)modarg;
  with_cap_mod(who, mod, [&](auto mtag) {
    run_bwd<decltype(mtag)::value, true>(a, q, force_split);
  });
  return {dq, dk, dv};
}

std::vector<at::Tensor> attn_cap_bwd(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
                                     at::Tensor dout, at::Tensor lse, double scale, long mod,
                                     long modarg, double cap,
                                     OptTensor dq, OptTensor dk, OptTensor dv) {
  return attn_cap_bwd_impl("attn_cap_bwd", q, k, v, o, dout, lse, scale, mod, modarg, cap,
                           dq.value_or(at::Tensor()), dk.value_or(at::Tensor()),
                           dv.value_or(at::Tensor()), false);
}

std::vector<at::Tensor> attn_cap_bwd_split(at::Tensor q, at::Tensor k, at::Tensor v,
                                           at::Tensor o, at::Tensor dout, at::Tensor lse,
                                           double scale, long mod, long modarg, double cap) {
  return attn_cap_bwd_impl("attn_cap_bwd_split", q, k, v, o, dout, lse, scale, mod, modarg, cap,
                           {}, {}, {}, true);
}

// Backward of attn_fwd_blockmask (trainable flex attention): same device mask
// tensors as the forward plus qrange, the per-kv-block transpose of range.
// bias (may be empty) gets no gradient.
std::vector<at::Tensor> attn_bwd_blockmask(at::Tensor q, at::Tensor k, at::Tensor v,
                                           at::Tensor o, at::Tensor dout, at::Tensor lse,
                                           double scale, at::Tensor gran, at::Tensor bits,
                                           at::Tensor range, at::Tensor qrange,
                                           at::Tensor bias) {
  const char* who = "attn_bwd_blockmask";
  at::Tensor dq, dk, dv;
  AttnArgs a = bwd_args(who, q, k, v, o, dout, lse, scale, dq, dk, dv);
  check_blockmask(who, a, q, gran, bits, range, bias);
  TORCH_CHECK(qrange.scalar_type() == at::kInt && qrange.device() == q.device() &&
              shape_is(qrange, a.B, a.Hq, cdiv(a.Skv, 256), 2),
              who, ": qrange must be int32 [B,H,ceil(Skv/256),2] on q's GPU");
  qrange = qrange.contiguous();
  a.qrange = qrange.data_ptr<int>();
  run_bwd<MOD_BLOCKMASK>(a, q, false);
  return {dq, dk, dv};
}

// Backward of attn_fwd_doc (document-masked packed sequences). doc_start /
// doc_end are int32 [B, S]; dq/dk/dv as in attn_bwd.
std::vector<at::Tensor> attn_bwd_doc(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
                                     at::Tensor dout, at::Tensor lse, double scale,
                                     at::Tensor doc_start, at::Tensor doc_end,
                                     OptTensor dq_, OptTensor dk_, OptTensor dv_) {
  const char* who = "attn_bwd_doc";
  at::Tensor dq = dq_.value_or(at::Tensor()), dk = dk_.value_or(at::Tensor()),
             dv = dv_.value_or(at::Tensor());
  AttnArgs a = bwd_args(who, q, k, v, o, dout, lse, scale, dq, dk, dv);
  a.doc_start = check_doc(who, a, q, doc_start, "doc_start");
  a.doc_end = check_doc(who, a, q, doc_end, "doc_end");
  run_bwd<MOD_DOCUMENT>(a, q, false);
  return {dq, dk, dv};
}
