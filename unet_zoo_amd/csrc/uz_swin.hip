// Swin-UNet V2 specific kernels for gfx950 (MI355X)  (reference: unet_zoo/models/swin_unet_v2.py):
//   * patch extraction for PatchEmbed's Conv2d(k = s = patch)                           (:548-556)
//   * LayerNorm forward / backward over the channel dimension of a token tensor [P][C], with the
//     reference's token permutations folded into the addressing — PatchMerging's 2x2 gather+concat
//     (:315-332), PatchExpand / FinalPatchExpand_X4's 'b h w (p1 p2 c) -> b (h p1) (w p2) c'
//     (:352-362, :375-387) — and the block tail `shortcut + drop_path(norm1(.))` (:264-267) fused in
//   * LayerNorm with the 1x1 segmentation head fused behind it
// Window attention and its position-bias MLP are in uz_winattn.hip.  The Linear layers around these run on the
// LDS-DMA GEMM (uz_gemm_dma.hip) and the weight-gradient kernels.  Everything here is bandwidth / latency bound.
#include "uz_common.h"

namespace {

template <typename T> __device__ __forceinline__ void store_f(T* p, const float* f) {
  Vec16<T> v;
#pragma unroll
  for (int i = 0; i < ElemTraits<T>::VEC; ++i) v.v[i] = (T)f[i];
  st16(p, v);
}

// ---------------------------------------------------------------------------------------------
// patches: out[p = (b, i, j)][k = (kh*ps + kw)*C + c] = x[b][c][i*ps + kh][j*ps + kw], zero for k >= ps*ps*C
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ x, int N, int C, int H, int W, int ps,
                                                       int Kpad, T* __restrict__ out) {
  const int Ho = H / ps, Wo = W / ps, K = ps * ps * C;
  const long long total = (long long)N * Ho * Wo * Kpad;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(idx % Kpad);
    const long long p = idx / Kpad;
    float v = 0.f;
    if (k < K) {
      const int c = k % C, tap = k / C, kh = tap / ps, kw = tap - kh * ps;
      const int j = (int)(p % Wo);
      const long long t = p / Wo;
      const int i = (int)(t % Ho), b = (int)(t / Ho);
      v = x[(((size_t)b * C + c) * H + i * ps + kh) * W + j * ps + kw];
    }
    out[idx] = (T)v;
  }
}

// ---------------------------------------------------------------------------------------------
// LayerNorm.  Output token t (grid Ho x Wo, C channels); its input row is assembled by `mode`:
//   0 plain     : x[t][c]
//   1 merge 2x2 : Ho = H/2; channel segment s = c / (C/4) comes from input token (2i + (s&1), 2j + (s>>1)),
//                 channels c - s*C/4 (torch.cat([x0, x1, x2, x3], -1) of PatchMerging)
//   2 expand r  : Ho = H*r; output token (h*r + p1, w*r + p2) reads input token (h, w), channels
//                 (p1*r + p2)*C + c
// y = [res +] [sb[image] *] (xhat * gamma + beta); mean and rstd per token are kept for the backward.
// One wave per token, lanes stride over the 16-byte channel chunks (at most MAXIT per lane).
// ---------------------------------------------------------------------------------------------
struct FastDiv {
  unsigned m;
  int s;
};

struct LnArgs {
  const void* x;
  void* y;            // fwd: output; bwd: unused
  const void* res;    // fwd: optional residual (same layout as y)
  const void* g;      // bwd: gradient of y
  void* dx;           // bwd: gradient of x (mapped like x)
  const float* gamma;
  const float* beta;
  const float* sb;    // optional per-image factor of the normalised branch (stochastic depth)
  float* stats;       // [P_out][2] mean, rstd
  float* partial;     // bwd: [gridDim.x][2][C] sums of g*xhat (dgamma) and g (dbeta)
  int N, Ho, Wo, C, ldx, ldy, ldr, ldg, lddx, mode, r;
  float eps;
  int act;                // 1: GELU applied to the result (ACT instantiations)
  FastDiv fWo, fHo, fr;   // token index -> (image, row, column) and the expand sub-position without v_rcp sequences
  int Hin, Win;           // grid of x: (Ho, Wo) plain, (2 Ho, 2 Wo) merge, (Ho / r, Wo / r) expand
};

constexpr int LN_MAXIT = 8;     // 16-byte chunks per lane: C <= 64 * 8 * 4 = 2048 in fp32
constexpr int LN_MAXC = 2048;   // MixFFN_skip of MISSFormer's 512-channel stage: LayerNorm(4 * 512)

// Unsigned division by a launch constant (n < 2^31): q = umulhi(n, m) >> s with m = ceil(2^(32+s) / d),
// exact for every 31-bit n (Granlund & Montgomery); d = 1 is m = 0.  A runtime integer division costs ~25
// VALU instructions; the token -> (image, row, column[, sub-position]) decomposition needs four of them per
// token and lane and dominated the instruction count of these bandwidth kernels.
__device__ __forceinline__ int fdiv(int n, const FastDiv f) {
  return f.m == 0 ? n : (int)(__umulhi((unsigned)n, f.m) >> f.s);
}

// where token t of the normalised map reads x: pixel `pix` of x's grid, first channel `coff`
struct TokPos {
  int img, pix, coff;
};
__device__ __forceinline__ TokPos ln_tok(const LnArgs& a, int t) {
  TokPos p;
  const int tt = fdiv(t, a.fWo), ow = t - tt * a.Wo;
  p.img = fdiv(tt, a.fHo);
  const int oh = tt - p.img * a.Ho;
  p.coff = 0;
  if (a.mode == 0) {
    p.pix = t;
  } else if (a.mode == 1) {
    p.pix = (p.img * a.Hin + 2 * oh) * a.Win + 2 * ow;
  } else {
    const int h = fdiv(oh, a.fr), p1 = oh - h * a.r, w = fdiv(ow, a.fr), p2 = ow - w * a.r;
    p.pix = (p.img * a.Hin + h) * a.Win + w;
    p.coff = (p1 * a.r + p2) * a.C;
  }
  return p;
}
// per-lane constants of channel chunk c0: merge mode takes segment s = c0 / (C/4) from the pixel at
// (+ (s & 1) rows, + (s >> 1) columns), channels c0 - s C/4
__device__ __forceinline__ void ln_chunk(const LnArgs& a, int c0, int* dpix, int* cch) {
  *dpix = 0;
  *cch = c0;
  if (a.mode == 1) {
    const int Cq = a.C >> 2, sg = c0 / Cq;
    *dpix = (sg & 1) * a.Win + (sg >> 1);
    *cch = c0 - sg * Cq;
  }
}
__device__ __forceinline__ size_t ln_off(const TokPos& p, int dpix, int cch, int ld) {
  return (size_t)(p.pix + dpix) * ld + p.coff + cch;
}

// sum over the LPT consecutive lanes that share a token (LPT a power of two <= 64)
__device__ __forceinline__ float group_sum(float v, int lpt) {
  for (int o = lpt >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// LPT = min(64, pow2 >= C/VEC) lanes per token, 64/LPT tokens per wave, 4 waves per workgroup: a
// 96-channel bf16 token (12 chunks) occupies 16 lanes, not a whole wave.  A lane carries MAXIT chunks of
// each of U tokens; all their loads are issued before the first reduction and stay packed (16 bytes = 4
// registers) until they are used, so that a wave keeps U * MAXIT * 16 (x2 with a residual / in the
// backward) bytes per lane in flight at a register count that still admits 4+ waves per SIMD: with one
// token per pass and the register budget of MAXIT = 6 the kernel ran at 1 - 1.5 TB/s, bound by latency.
template <typename T> __device__ __forceinline__ void unpack_f(const uint4& r, float* f);
template <> __device__ __forceinline__ void unpack_f<float>(const uint4& r, float* f) {
  f[0] = __uint_as_float(r.x); f[1] = __uint_as_float(r.y); f[2] = __uint_as_float(r.z); f[3] = __uint_as_float(r.w);
}
template <> __device__ __forceinline__ void unpack_f<bf16_t>(const uint4& r, float* f) {
  const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f[2 * k] = __uint_as_float(w[k] << 16);
    f[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
  }
}
// keeps a packed load packed: the optimiser otherwise converts every loaded chunk to fp32 as soon as it lands
// (twice the registers), which costs the occupancy that the loads in flight were meant to buy
__device__ __forceinline__ void pin(uint4& r) { asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(r.z), "+v"(r.w)); }

// GELU (erf form, nn.GELU(): MixFFN_skip's act(norm1(.)), missformer.py:206) and its derivative.  erf by
// Abramowitz-Stegun 7.1.26 (|error| < 1.5e-7, below fp32 resolution of the products it enters): one v_exp, one
// v_rcp and five FMAs; its e^(-z^2/2) is also the density the derivative needs.  libdevice's erff costs ~3x that
// and made the fused LayerNorm kernels ALU-bound.
__device__ __forceinline__ void ln_gelu_parts(float z, float* cdf, float* pdf) {
  const float x = fabsf(z) * 0.70710678118654752f;
  const float t = __builtin_amdgcn_rcpf(1.f + 0.3275911f * x);
  const float e = __expf(-x * x);
  const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
  const float er = copysignf(1.f - poly * e, z);
  *cdf = 0.5f * (1.f + er);
  *pdf = 0.3989422804014327f * e;
}
__device__ __forceinline__ float ln_gelu(float z) {
  float c, p;
  ln_gelu_parts(z, &c, &p);
  return z * c;
}
__device__ __forceinline__ float ln_dgelu(float z) {
  float c, p;
  ln_gelu_parts(z, &c, &p);
  return c + z * p;
}

template <typename T, bool BWD, int MAXIT, int U, bool ACT>
__global__ __launch_bounds__(256) void layernorm_kernel(const LnArgs a, int lpt) {
  constexpr int VEC = ElemTraits<T>::VEC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane & (lpt - 1), grp = lane / lpt, tpw = 64 / lpt;
  const int CC = a.C / VEC;
  const int P = a.N * a.Ho * a.Wo;
  const T* __restrict__ x = static_cast<const T*>(a.x);
  const T* __restrict__ second = static_cast<const T*>(BWD ? a.g : a.res);   // g, or the optional residual
  const int ld2 = BWD ? a.ldg : a.ldr;
  float gam[MAXIT][VEC], bet[MAXIT][VEC], ag[MAXIT][VEC], ab[MAXIT][VEC];
  int dpix[MAXIT], cch[MAXIT];
  // Every load of this kernel is UNCONDITIONAL: an out-of-range lane reads a valid dummy address and its value is replaced
  // by a select.  Loads inside `if (in range)` blocks made hipcc 7.2 close every block with s_waitcnt vmcnt(0): the three
  // chunks of a token (and the 48 gamma / beta words before them) arrived one memory round trip after the other, which
  // is what a launch on a 1.5 MB tensor spent its 10 us on (tools/ln_bench.py under rocprofv3: see DESIGN 3b).
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int cc = sub + lpt * it;
    ln_chunk(a, cc * VEC, &dpix[it], &cch[it]);
    const bool in = cc < CC;
    const int c0 = in ? cc * VEC : 0;
#pragma unroll
    for (int e = 0; e < VEC; e += 4) {
      const float4 gq = *reinterpret_cast<const float4*>(a.gamma + c0 + e);
      const float4 bq = (!BWD || ACT) ? *reinterpret_cast<const float4*>(a.beta + c0 + e) : make_float4(0.f, 0.f, 0.f, 0.f);
      gam[it][e] = in ? gq.x : 0.f, gam[it][e + 1] = in ? gq.y : 0.f, gam[it][e + 2] = in ? gq.z : 0.f, gam[it][e + 3] = in ? gq.w : 0.f;
      bet[it][e] = in ? bq.x : 0.f, bet[it][e + 1] = in ? bq.y : 0.f, bet[it][e + 2] = in ? bq.z : 0.f, bet[it][e + 3] = in ? bq.w : 0.f;
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) ag[it][e] = ab[it][e] = 0.f;
  }
  const float invC = 1.f / (float)a.C;
  const int tpb = 4 * tpw * U;  // tokens per workgroup pass
  for (int t0 = blockIdx.x * tpb; t0 < P; t0 += gridDim.x * tpb) {
    int t[U];
    TokPos pos[U];
    bool tok[U];    // whole lane groups go idle together; shuffles below stay inside a group
    uint4 xr[U][MAXIT], sr[U][MAXIT];
    float mean[U], rstd[U], fsc[U];
    const bool has2 = BWD || second != nullptr;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      t[u] = t0 + (u * 4 + wave) * tpw + grp;
      tok[u] = t[u] < P;
      const int tc = tok[u] ? t[u] : 0;
      pos[u] = ln_tok(a, tc);
#pragma unroll
      for (int it = 0; it < MAXIT; ++it) {
        const int cc = sub + lpt * it;
        const bool ok = cc < CC && tok[u], ok2 = ok && has2;
        const T* px = ok ? x + ln_off(pos[u], dpix[it], cch[it], a.ldx) : x;
        const T* ps = ok2 ? second + (size_t)tc * ld2 + cc * VEC : x;
        const uint4 rx = *reinterpret_cast<const uint4*>(px), rs = *reinterpret_cast<const uint4*>(ps);
        xr[u][it].x = ok ? rx.x : 0u, xr[u][it].y = ok ? rx.y : 0u, xr[u][it].z = ok ? rx.z : 0u, xr[u][it].w = ok ? rx.w : 0u;
        sr[u][it].x = ok2 ? rs.x : 0u, sr[u][it].y = ok2 ? rs.y : 0u, sr[u][it].z = ok2 ? rs.z : 0u, sr[u][it].w = ok2 ? rs.w : 0u;
      }
      if constexpr (BWD) {
        const float2 ms = *reinterpret_cast<const float2*>(a.stats + (size_t)tc * 2);
        mean[u] = tok[u] ? ms.x : 0.f;
        rstd[u] = tok[u] ? ms.y : 0.f;
      }
      // the per-image factor (stochastic depth) with the operands, not after the reductions
      const float* pf = a.sb != nullptr ? a.sb + pos[u].img : a.gamma;
      const float fv = *pf;
      fsc[u] = a.sb != nullptr ? fv : 1.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int it = 0; it < MAXIT; ++it) {
        pin(xr[u][it]);
        pin(sr[u][it]);
      }
    if constexpr (!BWD) {
      T* __restrict__ y = static_cast<T*>(a.y);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        __builtin_amdgcn_sched_barrier(0);   // one token at a time: the packed loads stay packed until here
        float v[MAXIT][VEC];
        float s = 0.f;
#pragma unroll
        for (int it = 0; it < MAXIT; ++it) {
          unpack_f<T>(xr[u][it], v[it]);
#pragma unroll
          for (int e = 0; e < VEC; ++e) s += v[it][e];
        }
        const float mu = group_sum(s, lpt) * invC;
        float q = 0.f;
#pragma unroll
        for (int it = 0; it < MAXIT; ++it)
          if (sub + lpt * it < CC) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              const float d = v[it][e] - mu;
              q += d * d;
            }
          }
        const float rs = rsqrtf(group_sum(q, lpt) * invC + a.eps);
        const float f = fsc[u];
#pragma unroll
        for (int it = 0; it < MAXIT; ++it) {
          const int cc = sub + lpt * it;
          if (cc < CC && tok[u]) {
            float o[VEC], rv[VEC];
            unpack_f<T>(sr[u][it], rv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              o[e] = f * ((v[it][e] - mu) * rs * gam[it][e] + bet[it][e]);
              if (second != nullptr) o[e] += rv[e];
              if constexpr (ACT) o[e] = ln_gelu(o[e]);
            }
            store_f(y + (size_t)t[u] * a.ldy + cc * VEC, o);
          }
        }
        // (after the outputs: the block's join waits for the stores in front of it)
        if (sub == 0 && tok[u]) *reinterpret_cast<float2*>(a.stats + (size_t)t[u] * 2) = make_float2(mu, rs);
      }
    } else {
      T* __restrict__ dx = static_cast<T*>(a.dx);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        __builtin_amdgcn_sched_barrier(0);   // one token at a time: the packed loads stay packed until here
        const float f = fsc[u];
        float xh[MAXIT][VEC], gv[MAXIT][VEC];
        float s1 = 0.f, s2 = 0.f;  // sum of g*gamma, sum of g*gamma*xhat
#pragma unroll
        for (int it = 0; it < MAXIT; ++it) {
          unpack_f<T>(xr[u][it], xh[it]);
          unpack_f<T>(sr[u][it], gv[it]);
          if (sub + lpt * it < CC && tok[u]) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              gv[it][e] *= f;
              xh[it][e] = (xh[it][e] - mean[u]) * rstd[u];
              if constexpr (ACT) gv[it][e] *= ln_dgelu(xh[it][e] * gam[it][e] + bet[it][e]);
              ag[it][e] += gv[it][e] * xh[it][e];
              ab[it][e] += gv[it][e];
              const float gg = gv[it][e] * gam[it][e];
              s1 += gg;
              s2 += gg * xh[it][e];
            }
          }
        }
        s1 = group_sum(s1, lpt) * invC;
        s2 = group_sum(s2, lpt) * invC;
#pragma unroll
        for (int it = 0; it < MAXIT; ++it) {
          const int cc = sub + lpt * it;
          if (cc < CC && tok[u]) {
            float o[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] = rstd[u] * (gv[it][e] * gam[it][e] - s1 - xh[it][e] * s2);
            store_f(dx + ln_off(pos[u], dpix[it], cch[it], a.lddx), o);
          }
        }
      }
    }
  }
  if constexpr (BWD) {
    // one partial row per workgroup: the 4 * tpw lane groups are summed through LDS in a fixed order
    extern __shared__ float red[];  // [4 * tpw][2][C]
    const int gidx = wave * tpw + grp, ngrp = 4 * tpw;
    float* mine = red + (size_t)gidx * 2 * a.C;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int cc = sub + lpt * it;
      if (cc < CC) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          mine[cc * VEC + e] = ag[it][e];
          mine[a.C + cc * VEC + e] = ab[it][e];
        }
      }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 2 * a.C; c += 256) {
      float t = 0.f;
      for (int k = 0; k < ngrp; ++k) t += red[(size_t)k * 2 * a.C + c];
      a.partial[(size_t)blockIdx.x * 2 * a.C + c] = t;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// LayerNorm + 1x1 head: logits[img][k][oh][ow] = b[k] + sum_c w[k][c] LN(x)[token][c], the tail of
// swin_unet_v2 (FinalPatchExpand_X4's norm, :385, followed by the 1x1 `output` convolution, :690 / :753).
// At B=16 256x256 the normalised tensor is 201 MB: written by the LayerNorm, read by the head, written
// again as its gradient and read back by the LayerNorm backward.  Fused, the forward reads x once and the
// backward reads x and writes dx.  With wg[k][c] = w[k][c] gamma[c]:
//   logit_k = rstd * sum_c wg_kc (x_c - mean) + (sum_c w_kc beta_c + b_k)
//   d x     = rstd * (gg - mean_c(gg) - xhat mean_c(gg xhat)),   gg_c = sum_k dlogit_k wg_kc
// and all four parameter gradients follow from S_kc = sum_t dlogit_tk xhat_tc and D_k = sum_t dlogit_tk:
//   d gamma_c = sum_k w_kc S_kc   d beta_c = sum_k w_kc D_k   d w_kc = gamma_c S_kc + beta_c D_k   d b_k = D_k
// so a lane carries wg and S only (not gamma, beta, w and four accumulators).  Partial rows [K*C + K] per
// workgroup, finished by ln_head_finalize_kernel.  KT = 1 with three chunks per lane, or up to 4 classes with one.
// ---------------------------------------------------------------------------------------------
struct LnHeadArgs {
  LnArgs ln;            // x, dx, gamma, beta, stats, partial, N, Ho, Wo, C, ldx, lddx, mode, r, eps
  const float* w;       // [K][C]
  const float* b;       // [K] or null
  float* logits;        // fwd out  (N, K, Ho, Wo)
  const float* dlogits; // bwd in   (N, K, Ho, Wo)
  int K;
};

template <typename T, bool BWD, int KT, int MAXIT, int U>
__global__ __launch_bounds__(256) void ln_head_kernel(const LnHeadArgs h, int lpt) {
  constexpr int VEC = ElemTraits<T>::VEC;
  const LnArgs& a = h.ln;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane & (lpt - 1), grp = lane / lpt, tpw = 64 / lpt;
  const int CC = a.C / VEC, K = h.K;
  const int P = a.N * a.Ho * a.Wo, HW = a.Ho * a.Wo;
  const T* __restrict__ x = static_cast<const T*>(a.x);
  float wg[KT][MAXIT][VEC], S[KT][MAXIT][VEC], D[KT], cst[KT], swg[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    float c0 = 0.f, c1 = 0.f;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int cc = sub + lpt * it;
      const bool in = cc < CC && k < K;
      // unconditional 16-byte loads (chunk 0 of class 0 for a lane out of range, then a select): as `in ? w[...] : 0` these
      // were 3 x 8 x 3 dword loads, each waited for before the next was issued (see layernorm_kernel)
      const int co = in ? cc * VEC : 0;
      const size_t wo = in ? (size_t)k * a.C + cc * VEC : 0;
#pragma unroll
      for (int e = 0; e < VEC; e += 4) {
        const float4 wq = *reinterpret_cast<const float4*>(h.w + wo + e);
        const float4 gq = *reinterpret_cast<const float4*>(a.gamma + co + e);
        const float4 bq = *reinterpret_cast<const float4*>(a.beta + co + e);
        const float wv[4] = {wq.x, wq.y, wq.z, wq.w}, gv[4] = {gq.x, gq.y, gq.z, gq.w}, bv[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          wg[k][it][e + q] = in ? wv[q] * gv[q] : 0.f;
          S[k][it][e + q] = 0.f;
          c0 += in ? wv[q] * bv[q] : 0.f;
          c1 += wg[k][it][e + q];
        }
      }
    }
    const float bk = h.b != nullptr ? h.b[k < K ? k : 0] : 0.f;
    cst[k] = group_sum(c0, lpt) + ((h.b != nullptr && k < K) ? bk : 0.f);
    swg[k] = group_sum(c1, lpt);
    D[k] = 0.f;
  }
  (void)swg;
  const float invC = 1.f / (float)a.C;
  const int tpb = 4 * tpw * U;
  for (int t0 = blockIdx.x * tpb; t0 < P; t0 += gridDim.x * tpb) {
    int t[U], rem[U];   // rem: the token's pixel inside its image (logits are NCHW planes)
    TokPos pos[U];
    bool tok[U];
    uint4 xr[U][MAXIT];
    float dl[U][KT], mean[U], rstd[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      t[u] = t0 + (u * 4 + wave) * tpw + grp;
      tok[u] = t[u] < P;
      const int tc = tok[u] ? t[u] : 0;
      pos[u] = ln_tok(a, tc);
      rem[u] = tc - pos[u].img * HW;
      // unconditional loads (a dummy address for lanes out of range, then a select): see layernorm_kernel
#pragma unroll
      for (int it = 0; it < MAXIT; ++it) {
        const int cc = sub + lpt * it;
        const bool ok = cc < CC && tok[u];
        const uint4 rx = *reinterpret_cast<const uint4*>(ok ? x + ln_off(pos[u], 0, cc * VEC, a.ldx) : x);
        xr[u][it].x = ok ? rx.x : 0u, xr[u][it].y = ok ? rx.y : 0u, xr[u][it].z = ok ? rx.z : 0u, xr[u][it].w = ok ? rx.w : 0u;
      }
      if constexpr (BWD) {
        const float2 ms = *reinterpret_cast<const float2*>(a.stats + (size_t)tc * 2);
        mean[u] = tok[u] ? ms.x : 0.f;
        rstd[u] = tok[u] ? ms.y : 0.f;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          const bool okk = tok[u] && k < K;
          const float dv = h.dlogits[okk ? ((size_t)pos[u].img * K + k) * HW + rem[u] : 0];
          dl[u][k] = okk ? dv : 0.f;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int it = 0; it < MAXIT; ++it) pin(xr[u][it]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      __builtin_amdgcn_sched_barrier(0);
      float v[MAXIT][VEC];
#pragma unroll
      for (int it = 0; it < MAXIT; ++it) unpack_f<T>(xr[u][it], v[it]);
      if constexpr (!BWD) {
        float s = 0.f;
#pragma unroll
        for (int it = 0; it < MAXIT; ++it)
#pragma unroll
          for (int e = 0; e < VEC; ++e) s += v[it][e];
        const float mu = group_sum(s, lpt) * invC;
        float q = 0.f, lk[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) lk[k] = 0.f;
#pragma unroll
        for (int it = 0; it < MAXIT; ++it)
          if (sub + lpt * it < CC) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              const float d = v[it][e] - mu;
              q = fmaf(d, d, q);
#pragma unroll
              for (int k = 0; k < KT; ++k) lk[k] = fmaf(d, wg[k][it][e], lk[k]);
            }
          }
        const float rs = rsqrtf(group_sum(q, lpt) * invC + a.eps);
        if (sub == 0 && tok[u]) {
          a.stats[(size_t)t[u] * 2] = mu;
          a.stats[(size_t)t[u] * 2 + 1] = rs;
        }
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          const float tot = group_sum(lk[k], lpt);
          if (sub == 0 && tok[u] && k < K) h.logits[((size_t)pos[u].img * K + k) * HW + rem[u]] = fmaf(rs, tot, cst[k]);
        }
      } else {
        T* __restrict__ dx = static_cast<T*>(a.dx);
        float gg[MAXIT][VEC];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int it = 0; it < MAXIT; ++it) {
          const bool in = sub + lpt * it < CC && tok[u];
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            const float xh = in ? (v[it][e] - mean[u]) * rstd[u] : 0.f;
            v[it][e] = xh;
            float g = 0.f;
#pragma unroll
            for (int k = 0; k < KT; ++k) {
              g = fmaf(dl[u][k], wg[k][it][e], g);
              S[k][it][e] = fmaf(dl[u][k], xh, S[k][it][e]);
            }
            gg[it][e] = g;
            s1 += g;
            s2 = fmaf(g, xh, s2);
          }
        }
#pragma unroll
        for (int k = 0; k < KT; ++k) D[k] += dl[u][k];
        s1 = group_sum(s1, lpt) * invC;
        s2 = group_sum(s2, lpt) * invC;
#pragma unroll
        for (int it = 0; it < MAXIT; ++it) {
          const int cc = sub + lpt * it;
          if (cc < CC && tok[u]) {
            float o[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] = rstd[u] * (gg[it][e] - s1 - v[it][e] * s2);
            store_f(dx + ln_off(pos[u], 0, cc * VEC, a.lddx), o);
          }
        }
      }
    }
  }
  if constexpr (BWD) {
    // one partial row per workgroup: [S (K*C) | D (K)]
    extern __shared__ float red[];  // [4 * tpw][K * C + K]
    const int gidx = wave * tpw + grp, ngrp = 4 * tpw;
    const int n = K * a.C + K;
    float* mine = red + (size_t)gidx * n;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int cc = sub + lpt * it;
      if (cc < CC) {
#pragma unroll
        for (int e = 0; e < VEC; ++e)
#pragma unroll
          for (int k = 0; k < KT; ++k)
            if (k < K) mine[k * a.C + cc * VEC + e] = S[k][it][e];
      }
    }
    if (sub == 0) {
#pragma unroll
      for (int k = 0; k < KT; ++k)
        if (k < K) mine[K * a.C + k] = D[k];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < n; c += 256) {
      float t = 0.f;
      for (int k = 0; k < ngrp; ++k) t += red[(size_t)k * n + c];
      a.partial[(size_t)blockIdx.x * n + c] = t;
    }
  }
}

// grid (C / 8), 1024 threads = 8 channels x 128 row groups (the rows are many -- one per workgroup of the main
// kernel -- and the columns few); sums the rows (in double, fixed order) and forms the four gradients from S
// and D (see the head comment)
__global__ __launch_bounds__(1024) void ln_head_finalize_kernel(const float* __restrict__ partial, int rows, int C, int K,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const float* __restrict__ w, float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta, float* __restrict__ dw,
                                                                float* __restrict__ db) {
  __shared__ double sh[128][9];
  __shared__ double sD[4];
  const int el = threadIdx.x & 7, g = threadIdx.x >> 3;
  const int c = blockIdx.x * 8 + el, n = K * C + K;
  double Skc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k <= K; ++k) {   // k == K: the D columns (el < K)
    const int col = k < K ? k * C + c : K * C + el;
    const bool in = k < K ? c < C : el < K;
    double s = 0.0;
    // eight rows per trip, unconditional loads (row 0 / column 0 out of range, dropped below), added in the same order as one row
    // per trip: this loop was rows / 128 dependent round trips per pass
    for (int r = g; r < rows; r += 8 * 128) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = partial[(size_t)(r + u * 128 < rows ? r + u * 128 : 0) * n + (in ? col : 0)];
#pragma unroll
      for (int u = 0; u < 8; ++u) asm volatile("" : "+v"(v[u]));
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (in && r + u * 128 < rows) s += (double)v[u];
    }
    __syncthreads();
    sh[g][el] = s;
    __syncthreads();
    if (g == 0) {
      double t = 0.0;
      for (int r = 0; r < 128; ++r) t += sh[r][el];
      if (k < K) Skc[k] = t;
      else if (el < K) sD[el] = t;
    }
  }
  __syncthreads();
  if (g == 0 && c < C) {
    double dg = 0.0, dbt = 0.0;
    for (int k = 0; k < K; ++k) {
      const double wv = (double)w[(size_t)k * C + c];
      dg += wv * Skc[k];
      dbt += wv * sD[k];
      dw[(size_t)k * C + c] = (float)((double)gamma[c] * Skc[k] + (double)beta[c] * sD[k]);
    }
    dgamma[c] = (float)dg;
    dbeta[c] = (float)dbt;
  }
  if (blockIdx.x == 0 && g == 0 && el < K && db != nullptr) db[el] = (float)sD[el];
}

inline int grid_cap(long long units, int per_block, int per_cu) {
  long long g = (units + per_block - 1) / per_block;
  const long long cap = (long long)UZ_NUM_CU * per_cu;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// see fdiv(): m = ceil(2^(32+s) / d), d = 1 -> m = 0
static FastDiv make_fastdiv(int d) {
  FastDiv f{0u, 0};
  if (d <= 1) return f;
  int S = 0;
  while ((1LL << S) < d) ++S;   // ceil(log2 d) >= 1
  f.s = S - 1;
  f.m = (unsigned)(((1ULL << (31 + S)) + (unsigned long long)d - 1) / (unsigned long long)d);
  return f;
}
static void ln_geometry(const uz_ln_desc* d, LnArgs* a) {
  a->fWo = make_fastdiv(d->Wo);
  a->fHo = make_fastdiv(d->Ho);
  a->fr = make_fastdiv(d->mode == 2 ? d->r : 1);
  a->Hin = d->mode == 1 ? 2 * d->Ho : d->mode == 2 ? d->Ho / d->r : d->Ho;
  a->Win = d->mode == 1 ? 2 * d->Wo : d->mode == 2 ? d->Wo / d->r : d->Wo;
}

int ln_lpt(const uz_ln_desc* d) {
  int cc = d->C / (d->dtype == UZ_BF16 ? 8 : 4);
  if (!(uz_tune_flags() & 0x100000)) cc = (cc + 2) / 3;   // three chunks per lane (see ln_unroll)
  int l = 1;
  while (l < cc && l < 64) l <<= 1;
  return l;
}

int ln_check(const char* fn, const uz_ln_desc* d) {
  UZ_REQUIRE(d != nullptr, "%s: null descriptor", fn);
  UZ_REQUIRE(d->dtype == UZ_F32 || d->dtype == UZ_BF16, "%s: bad dtype", fn);
  const int vec = d->dtype == UZ_BF16 ? 8 : 4;
  UZ_REQUIRE(d->N > 0 && d->Ho > 0 && d->Wo > 0 && d->C > 0 && d->C % vec == 0, "%s: bad shape", fn);
  UZ_REQUIRE(d->C / vec <= 64 * LN_MAXIT && d->C <= LN_MAXC, "%s: C=%d too large (max %d)", fn, d->C, LN_MAXC);
  // dynamic LDS of the backward: 4 * (64 / lanes-per-token) groups x 2 x C floats
  UZ_REQUIRE((long long)4 * (64 / ln_lpt(d)) * 2 * d->C * 4 <= 64 * 1024, "%s: C=%d: partial-row staging exceeds 64 KiB", fn, d->C);
  UZ_REQUIRE(d->mode >= 0 && d->mode <= 2, "%s: bad mode %d", fn, d->mode);
  if (d->mode == 1) UZ_REQUIRE(d->C % (4 * vec) == 0 && d->ldx % vec == 0 && d->ldx >= d->C / 4, "%s: merge needs C %% %d == 0", fn, 4 * vec);
  if (d->mode == 2) UZ_REQUIRE(d->r >= 1 && d->Ho % d->r == 0 && d->Wo % d->r == 0 && d->ldx >= d->r * d->r * d->C, "%s: bad expand factor", fn);
  if (d->mode == 0) UZ_REQUIRE(d->ldx >= d->C, "%s: bad ldx", fn);
  UZ_REQUIRE(d->ldx % vec == 0, "%s: ldx must be a multiple of %d", fn, vec);
  UZ_REQUIRE((long long)d->N * d->Ho * d->Wo < (1LL << 31), "%s: too many tokens", fn);
  return UZ_OK;
}

// chunks per lane and tokens per lane group and pass of the instantiation that serves d
int ln_its(const uz_ln_desc* d) {
  const int vec = d->dtype == UZ_BF16 ? 8 : 4, lpt = ln_lpt(d);
  return (d->C / vec + lpt - 1) / lpt;
}
// tokens per lane group and pass.  Measured on the 1M-token expand LayerNorm of swin_unet_v2 (201 MB in, 201 MB
// out, three chunks per lane): forward U = 1 / 2 -> 101 / 119 us, backward 200 / 185 us; U = 4 spills.
int ln_unroll(const uz_ln_desc* d, bool bwd) {
  const int its = ln_its(d);
  const int u = (int)((uz_tune_flags() >> 16) & 15);
  if (u == 1 || u == 2 || u == 4 || (u == 8 && its == 1)) return its > 3 ? 1 : u;
  if (its > 3) return 1;
  if (its > 1) return bwd ? 2 : 1;
  return 4;
}

int ln_grid(const uz_ln_desc* d, bool bwd) {
  const int tpb = 4 * (64 / ln_lpt(d)) * ln_unroll(d, bwd);
  return grid_cap((long long)d->N * d->Ho * d->Wo, tpb, 8);
}

template <bool BWD>
void ln_launch(const uz_ln_desc* d, dim3 grid, dim3 block, size_t shm, hipStream_t st, const LnArgs& a, int lpt) {
  const int its = ln_its(d), u = ln_unroll(d, BWD);
#define UZ_LN(T, I, U)                                                                                   \
  do {                                                                                                   \
    if (a.act) hipLaunchKernelGGL((layernorm_kernel<T, BWD, I, U, true>), grid, block, shm, st, a, lpt); \
    else hipLaunchKernelGGL((layernorm_kernel<T, BWD, I, U, false>), grid, block, shm, st, a, lpt);      \
  } while (0)
#define UZ_LN_U(T, I) \
  do { if (u == 1) UZ_LN(T, I, 1); else if (u == 4) UZ_LN(T, I, 4); else UZ_LN(T, I, 2); } while (0)
  if (d->dtype == UZ_BF16) {
    if (its == 1) { if (u == 8) UZ_LN(bf16_t, 1, 8); else UZ_LN_U(bf16_t, 1); }
    else if (its == 2) UZ_LN_U(bf16_t, 2);
    else if (its == 3) UZ_LN_U(bf16_t, 3);
    else if (its <= 6) UZ_LN(bf16_t, 6, 1);
    else UZ_LN(bf16_t, 8, 1);
  } else {
    if (its == 1) { if (u == 8) UZ_LN(float, 1, 8); else UZ_LN_U(float, 1); }
    else if (its == 2) UZ_LN_U(float, 2);
    else if (its == 3) UZ_LN_U(float, 3);
    else if (its <= 6) UZ_LN(float, 6, 1);
    else UZ_LN(float, 8, 1);
  }
#undef UZ_LN_U
#undef UZ_LN
}

}  // namespace

extern "C" int uz_patchify(int dtype, const float* x_nchw, int N, int C, int H, int W, int patch, int Kpad,
                           void* out, void* stream) {
  UZ_REQUIRE(dtype == UZ_F32 || dtype == UZ_BF16, "uz_patchify: bad dtype");
  UZ_REQUIRE(x_nchw && out && N > 0 && C > 0 && patch > 0 && H % patch == 0 && W % patch == 0, "uz_patchify: bad shape");
  UZ_REQUIRE(Kpad >= patch * patch * C, "uz_patchify: Kpad too small");
  const long long total = (long long)N * (H / patch) * (W / patch) * Kpad;
  const dim3 grid(grid_cap(total, 256, 16)), block(256);
  if (dtype == UZ_BF16) hipLaunchKernelGGL((patchify_kernel<bf16_t>), grid, block, 0, (hipStream_t)stream, x_nchw, N, C, H, W, patch, Kpad, (bf16_t*)out);
  else hipLaunchKernelGGL((patchify_kernel<float>), grid, block, 0, (hipStream_t)stream, x_nchw, N, C, H, W, patch, Kpad, (float*)out);
  UZ_LAUNCH_CHECK("uz_patchify");
  return UZ_OK;
}

extern "C" int uz_layernorm_fwd(const uz_ln_desc* d, const void* x, const float* gamma, const float* beta,
                                const void* res, const float* image_scale, void* y, float* stats, void* stream) {
  const int rc = ln_check("uz_layernorm_fwd", d);
  if (rc != UZ_OK) return rc;
  const int vec = d->dtype == UZ_BF16 ? 8 : 4;
  UZ_REQUIRE(x && gamma && beta && y && stats, "uz_layernorm_fwd: null pointer");
  UZ_REQUIRE((((uintptr_t)gamma | (uintptr_t)beta) & 15) == 0 && ((uintptr_t)stats & 7) == 0,
             "uz_layernorm_fwd: gamma / beta must be 16-byte aligned, stats 8-byte aligned");
  UZ_REQUIRE(d->ldy % vec == 0 && d->ldy >= d->C, "uz_layernorm_fwd: bad ldy");
  if (res) UZ_REQUIRE(d->ldr % vec == 0 && d->ldr >= d->C, "uz_layernorm_fwd: bad ldr");
  LnArgs a{};
  a.x = x; a.y = y; a.res = res; a.gamma = gamma; a.beta = beta; a.sb = image_scale; a.stats = stats;
  a.N = d->N; a.Ho = d->Ho; a.Wo = d->Wo; a.C = d->C; a.ldx = d->ldx; a.ldy = d->ldy; a.ldr = d->ldr;
  a.mode = d->mode; a.r = d->r; a.eps = d->eps; a.act = d->act;
  UZ_REQUIRE(d->act == 0 || (d->act == 1 && !res && !image_scale), "uz_layernorm_fwd: act = %d (GELU = 1 takes no residual / image scale)", d->act);
  ln_geometry(d, &a);
  const dim3 grid(ln_grid(d, false)), block(256);
  const int lpt = ln_lpt(d);
  ln_launch<false>(d, grid, block, 0, (hipStream_t)stream, a, lpt);
  UZ_LAUNCH_CHECK("uz_layernorm_fwd");
  return UZ_OK;
}

extern "C" int uz_layernorm_bwd_rows(const uz_ln_desc* d) {
  const int rc = ln_check("uz_layernorm_bwd_rows", d);
  if (rc != UZ_OK) return rc;
  return ln_grid(d, true);
}

static int ln_bwd_common(const char* fn, const uz_ln_desc* d, const void* x, const float* gamma, const float* beta,
                         const float* stats, const void* g, const float* image_scale, void* dx, float* partial,
                         void* stream) {
  const int rc = ln_check(fn, d);
  if (rc != UZ_OK) return rc;
  const int vec = d->dtype == UZ_BF16 ? 8 : 4;
  UZ_REQUIRE(x && gamma && stats && g && dx && partial, "%s: null pointer", fn);
  UZ_REQUIRE((((uintptr_t)gamma | (uintptr_t)beta) & 15) == 0 && ((uintptr_t)stats & 7) == 0,
             "%s: gamma / beta must be 16-byte aligned, stats 8-byte aligned", fn);
  UZ_REQUIRE(d->ldg % vec == 0 && d->ldg >= d->C && d->lddx % vec == 0, "%s: bad ldg / lddx", fn);
  LnArgs a{};
  a.x = x; a.g = g; a.dx = dx; a.gamma = gamma; a.beta = beta; a.sb = image_scale; a.stats = const_cast<float*>(stats);
  a.partial = partial;
  a.N = d->N; a.Ho = d->Ho; a.Wo = d->Wo; a.C = d->C; a.ldx = d->ldx; a.ldg = d->ldg; a.lddx = d->lddx;
  a.mode = d->mode; a.r = d->r; a.eps = d->eps; a.act = d->act;
  ln_geometry(d, &a);
  const dim3 grid(ln_grid(d, true)), block(256);
  const int lpt = ln_lpt(d);
  const size_t shm = (size_t)4 * (64 / lpt) * 2 * d->C * sizeof(float);
  ln_launch<true>(d, grid, block, shm, (hipStream_t)stream, a, lpt);
  UZ_LAUNCH_CHECK(fn);
  return UZ_OK;
}

extern "C" int uz_layernorm_bwd(const uz_ln_desc* d, const void* x, const float* gamma, const float* stats,
                                const void* g, const float* image_scale, void* dx, float* partial, void* stream) {
  UZ_REQUIRE(d && d->act == 0, "uz_layernorm_bwd: an activation needs beta: call uz_layernorm_act_bwd");
  return ln_bwd_common("uz_layernorm_bwd", d, x, gamma, nullptr, stats, g, image_scale, dx, partial, stream);
}

extern "C" int uz_layernorm_act_bwd(const uz_ln_desc* d, const void* x, const float* gamma, const float* beta,
                                    const float* stats, const void* g, void* dx, float* partial, void* stream) {
  UZ_REQUIRE(d && d->act == 1 && beta, "uz_layernorm_act_bwd: act must be 1 (GELU) and beta given");
  return ln_bwd_common("uz_layernorm_act_bwd", d, x, gamma, beta, stats, g, nullptr, dx, partial, stream);
}

// ---- LayerNorm + 1x1 head --------------------------------------------------------------------------
constexpr int LNH_MAXK = 4;

// lanes per token: one class -> three chunks per lane (the layout the plain kernel measures fastest with);
// more classes -> one chunk per lane, so that wg and S of all classes stay in registers
static int ln_head_its(int K) { return K == 1 ? 3 : 1; }
static int ln_head_lpt(const uz_ln_desc* d, int K) {
  const int its = ln_head_its(K);
  const int cc = (d->C / (d->dtype == UZ_BF16 ? 8 : 4) + its - 1) / its;
  int l = 1;
  while (l < cc && l < 64) l <<= 1;
  return l;
}
static int ln_head_check(const char* fn, const uz_ln_desc* d, int K) {
  const int rc = ln_check(fn, d);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(K >= 1 && K <= LNH_MAXK, "%s: K=%d classes (max %d)", fn, K, LNH_MAXK);
  const int vec = d->dtype == UZ_BF16 ? 8 : 4;
  UZ_REQUIRE(d->C / vec <= 64 * ln_head_its(K), "%s: C=%d too wide for %d classes", fn, d->C, K);
  const long long shm = (long long)4 * (64 / ln_head_lpt(d, K)) * (K * d->C + K) * 4;
  UZ_REQUIRE(shm <= 64 * 1024, "%s: partial-row staging exceeds 64 KiB", fn);
  return UZ_OK;
}
static int ln_head_unroll(bool bwd, int K) { return (K == 1 && !bwd) ? 1 : 2; }
static int ln_head_grid(const uz_ln_desc* d, int K, bool bwd) {
  return grid_cap((long long)d->N * d->Ho * d->Wo, 4 * (64 / ln_head_lpt(d, K)) * ln_head_unroll(bwd, K), 8);
}
static void ln_head_args(const uz_ln_desc* d, LnHeadArgs* h) {
  LnArgs& a = h->ln;
  a.N = d->N; a.Ho = d->Ho; a.Wo = d->Wo; a.C = d->C; a.ldx = d->ldx; a.lddx = d->lddx;
  a.mode = d->mode; a.r = d->r; a.eps = d->eps;
  ln_geometry(d, &a);
}
template <bool BWD>
static void ln_head_launch(const uz_ln_desc* d, const LnHeadArgs& h, size_t shm, hipStream_t st) {
  const dim3 grid(ln_head_grid(d, h.K, BWD)), block(256);
  const int lpt = ln_head_lpt(d, h.K);
#define UZ_LNH(T) \
  do { \
    if (h.K == 1) hipLaunchKernelGGL((ln_head_kernel<T, BWD, 1, 3, (BWD ? 2 : 1)>), grid, block, shm, st, h, lpt); \
    else hipLaunchKernelGGL((ln_head_kernel<T, BWD, 4, 1, 2>), grid, block, shm, st, h, lpt); \
  } while (0)
  if (d->dtype == UZ_BF16) UZ_LNH(bf16_t);
  else UZ_LNH(float);
#undef UZ_LNH
}

extern "C" int uz_ln_head_fwd(const uz_ln_desc* d, const void* x, const float* gamma, const float* beta,
                              const float* w, const float* b, int K, float* logits, float* stats, void* stream) {
  const int rc = ln_head_check("uz_ln_head_fwd", d, K);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(x && gamma && beta && w && logits && stats, "uz_ln_head_fwd: null pointer");
  UZ_REQUIRE((((uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)w) & 15) == 0 && ((uintptr_t)stats & 7) == 0,
             "uz_ln_head_fwd: gamma / beta / w must be 16-byte aligned, stats 8-byte aligned");
  LnHeadArgs h{};
  ln_head_args(d, &h);
  h.ln.x = x; h.ln.gamma = gamma; h.ln.beta = beta; h.ln.stats = stats;
  h.w = w; h.b = b; h.logits = logits; h.K = K;
  ln_head_launch<false>(d, h, 0, (hipStream_t)stream);
  UZ_LAUNCH_CHECK("uz_ln_head_fwd");
  return UZ_OK;
}

extern "C" long long uz_ln_head_bwd_workspace_bytes(const uz_ln_desc* d, int K) {
  const int rc = ln_head_check("uz_ln_head_bwd_workspace_bytes", d, K);
  if (rc != UZ_OK) return rc;
  return (long long)ln_head_grid(d, K, true) * (K * d->C + K) * (long long)sizeof(float);
}

extern "C" int uz_ln_head_bwd(const uz_ln_desc* d, const void* x, const float* gamma, const float* beta,
                              const float* w, int K, const float* stats, const float* dlogits, void* dx,
                              float* dgamma, float* dbeta, float* dw, float* db, float* workspace, void* stream) {
  const int rc = ln_head_check("uz_ln_head_bwd", d, K);
  if (rc != UZ_OK) return rc;
  const int vec = d->dtype == UZ_BF16 ? 8 : 4;
  UZ_REQUIRE(x && gamma && beta && w && stats && dlogits && dx && dgamma && dbeta && dw && workspace,
             "uz_ln_head_bwd: null pointer");
  UZ_REQUIRE((((uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)w) & 15) == 0 && ((uintptr_t)stats & 7) == 0,
             "uz_ln_head_bwd: gamma / beta / w must be 16-byte aligned, stats 8-byte aligned");
  UZ_REQUIRE(d->lddx % vec == 0, "uz_ln_head_bwd: bad lddx");
  LnHeadArgs h{};
  ln_head_args(d, &h);
  h.ln.x = x; h.ln.gamma = gamma; h.ln.beta = beta; h.ln.stats = const_cast<float*>(stats);
  h.ln.dx = dx; h.ln.partial = workspace;
  h.w = w; h.dlogits = dlogits; h.K = K;
  const size_t shm = (size_t)4 * (64 / ln_head_lpt(d, K)) * (K * d->C + K) * sizeof(float);
  ln_head_launch<true>(d, h, shm, (hipStream_t)stream);
  UZ_LAUNCH_CHECK("uz_ln_head_bwd");
  hipLaunchKernelGGL(ln_head_finalize_kernel, dim3(uz_cdiv(d->C, 8)), dim3(1024), 0, (hipStream_t)stream,
                     (const float*)workspace, ln_head_grid(d, K, true), d->C, K, gamma, beta, w, dgamma, dbeta, dw, db);
  UZ_LAUNCH_CHECK("uz_ln_head_bwd (finalize)");
  return UZ_OK;
}
