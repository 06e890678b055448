// Window attention for windows of 65 .. 256 tokens (window_size 9 .. 16), gfx950 (MI355X).
// Reference: unet_zoo/models/swin_unet_v2.py:127-159 (cosine attention, per-entry temperature tau clipped at 0.01,
// continuous position bias, shifted-window mask, softmax, @v) with roll / window_partition / window_reverse
// (:30-56, :246-262) folded into the addressing (win_token()), as in uz_swin.hip.
//
// The kernels of uz_swin.hip hold a whole window in one 64-row tile; here a window is walked in 32 x 32 tiles of
// the score matrix, flash-style.  One 256-thread workgroup per (window, head), resident for the launch (it walks
// its share of the windows); wave w owns the 32-token tiles w, w + 4, ... of the OUTPUT index and walks the tiles
// of the summed index, so no partial result ever crosses a wave:
//   forward      column = query i (lane & 31), rows = keys:  S^T = K Q^T, running (max, sum), O^T += V^T P^T
//   backward 1   column = query i, rows = keys:     S^T, dP^T = V dO^T, dS -> d(bias) / d(tau), dQ^T += K^T W1^T
//   backward 2   column = key j,   rows = queries:  S = Q K^T, dP = dO V^T,     dV^T += dO^T P, dK^T += Q^T W1
// (the backward recomputes S in both passes from the forward's row log-sum-exp).  All products run on the matrix
// cores: v_mfma_f32_32x32x16_bf16 for bf16, v_mfma_f32_32x32x2_f32 for fp32 (the parity path: fp32 products and
// sums, same code).  An accumulator lane owns ONE column and 16 rows 8 (e >> 2) + 4 (lane >> 5) + (e & 3) of the
// tile, so the softmax and the element math run on registers; the second product of each pass takes those
// registers as its B fragment (the accumulator's row order is used as the K order of both operands) and its A
// fragment from a transposed tile X^T[32 d][tokens] in LDS.  Row-major fragments (16 head-dim values of one token)
// come straight from global memory: 32 (bf16) / 64 (fp32) contiguous bytes per lane.
// N need not be a multiple of 32: loads are issued unconditionally on clamped indices and selected afterwards
// (DESIGN 3h), padded keys get exp = 0, padded queries write nothing, the padded columns of the LDS tiles are zero.
// d(bias) / d(tau): a workgroup adds the dS of its windows into ITS row of `partial` in global memory (each
// element is owned by one lane for the whole launch: plain read-modify-write in window order, no atomics; the
// first window stores).  256 x 256 fp32 sums per head do not fit LDS or registers.
#include "uz_common.h"

namespace {

constexpr int WD = 32;             // head dimension
constexpr int WN = UZ_WIDE_MAXN;   // tokens per window at most
constexpr int WTS = 260;           // row stride of the transposed LDS tiles [32 d][WN tokens] in elements: rows stay
                                   // 8-byte (bf16) / 16-byte (fp32) aligned and 32 rows spread over the banks
constexpr float NEG = -1e30f;      // "minus infinity" that stays finite under subtraction

__device__ __forceinline__ float rcp_(float x) { return __builtin_amdgcn_rcpf(x); }

template <typename T> __device__ __forceinline__ void load32(const T* p, float* f) {  // 32 values of one token's head
  constexpr int VEC = ElemTraits<T>::VEC;
#pragma unroll
  for (int c = 0; c < WD / VEC; ++c) {
    const Vec16<T> v = ld16(p + c * VEC);
#pragma unroll
    for (int e = 0; e < VEC; ++e) f[c * VEC + e] = (float)v.v[e];
  }
}

// Row-major fragment: head-dim values d = 16 (lane >> 5) + {0 .. 15} of the token of row / column (lane & 31).
// A and B fragments share the form, so the K order (bf16: 16 lh + 8 s + e for instruction s; fp32: 16 lh + t for
// instruction t) is the same on both sides of a product.
template <typename T> struct Frag;
template <> struct Frag<bf16_t> {
  bf16x8 v[2];
};
template <> struct Frag<float> {
  float v[16];
};
__device__ __forceinline__ Frag<bf16_t> load_frag(const bf16_t* p) {
  Frag<bf16_t> f;
  f.v[0] = *reinterpret_cast<const bf16x8*>(p);
  f.v[1] = *reinterpret_cast<const bf16x8*>(p + 8);
  return f;
}
__device__ __forceinline__ Frag<float> load_frag(const float* p) {
  Frag<float> f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float4 v = *reinterpret_cast<const float4*>(p + 4 * c);
    f.v[4 * c] = v.x;
    f.v[4 * c + 1] = v.y;
    f.v[4 * c + 2] = v.z;
    f.v[4 * c + 3] = v.w;
  }
  return f;
}
__device__ __forceinline__ float sumsq(const Frag<bf16_t>& f) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = (float)f.v[c][e];
      s = fmaf(x, x, s);
    }
  return s;
}
__device__ __forceinline__ float sumsq(const Frag<float>& f) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) s = fmaf(f.v[e], f.v[e], s);
  return s;
}
// c[row of a][row of b] += a . b over the head dimension
__device__ __forceinline__ void mma_rows(const Frag<bf16_t>& a, const Frag<bf16_t>& b, f32x16& c) {
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v[0], b.v[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v[1], b.v[1], c, 0, 0, 0);
}
__device__ __forceinline__ void mma_rows(const Frag<float>& a, const Frag<float>& b, f32x16& c) {
#pragma unroll
  for (int t = 0; t < 16; ++t) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[t], b.v[t], c, 0, 0, 0);
}
// c[d][column] += sum over the tile's 32 tokens of XT[d][token] * p(token, column), p = the lane's 16 values in
// accumulator order.  xt = XT + (lane & 31) * WTS + 32 * tile + 4 * (lane >> 5).
__device__ __forceinline__ void mma_t(const bf16_t* xt, const float* p, f32x16& c) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const bf16x4 lo4 = *reinterpret_cast<const bf16x4*>(xt + 16 * s), hi4 = *reinterpret_cast<const bf16x4*>(xt + 16 * s + 8);
    const bf16x8 af = __builtin_shufflevector(lo4, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
    bf16x8 bf;
#pragma unroll
    for (int e = 0; e < 8; ++e) bf[e] = (bf16_t)p[8 * s + e];
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, c, 0, 0, 0);
  }
}
__device__ __forceinline__ void mma_t(const float* xt, const float* p, f32x16& c) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 a4 = *reinterpret_cast<const float4*>(xt + 8 * g);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, p[4 * g], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, p[4 * g + 1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, p[4 * g + 2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, p[4 * g + 3], c, 0, 0, 0);
  }
}
// the value the second product multiplies: the softmax sum is taken over what is actually multiplied
__device__ __forceinline__ float as_operand(bf16_t, float p) { return (float)(bf16_t)p; }
__device__ __forceinline__ float as_operand(float, float p) { return p; }

// four consecutive head-dim values of one token row (8 / 16 bytes)
__device__ __forceinline__ void store4(bf16_t* p, const float* f) {
  bf16x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = (bf16_t)f[e];
  *reinterpret_cast<bf16x4*>(p) = v;
}
__device__ __forceinline__ void store4(float* p, const float* f) {
  *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
}

__device__ __forceinline__ int acc_row(int r, int lh) { return 8 * (r >> 2) + 4 * lh + (r & 3); }

// ---------------------------------------------------------------------------------------------
// Forward
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256, UZ_WIDE_SLOTS_FWD) void winattn_wide_fwd_kernel(const AttnArgs a) {
  __shared__ __attribute__((aligned(16))) T sVT[WD * WTS];
  __shared__ float sKn[WN];
  __shared__ int sTok[WN], sCnt[WN];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, l31 = lane & 31, lh = lane >> 5, h = blockIdx.y;
  const int N = a.ws * a.ws, NT = (N + 31) >> 5;
  const int nWin = a.B * (a.H / a.ws) * (a.W / a.ws);
  const T* __restrict__ qkv = static_cast<const T*>(a.qkv);
  T* __restrict__ out = static_cast<T*>(a.out);
  for (int win = blockIdx.x; win < nWin; win += gridDim.x) {
    __syncthreads();   // the previous window's readers are done
    {  // thread = token: key norm, region id, token row and the V^T column (zero for padding)
      const bool in = tid < N;
      const WinTok me = win_token(a, win, in ? tid : 0);
      const T* row = qkv + (size_t)me.tok * a.ldq + h * WD;
      float kk[WD], vv[WD];
      load32(row + a.C, kk);
      load32(row + 2 * a.C, vv);
      float k2 = 0.f;
#pragma unroll
      for (int e = 0; e < WD; ++e) k2 = fmaf(kk[e], kk[e], k2);
      sKn[tid] = in ? sqrtf(k2) : 1.f;
      sTok[tid] = me.tok;
      sCnt[tid] = in ? me.cnt : -1;
#pragma unroll
      for (int e = 0; e < WD; ++e) sVT[e * WTS + tid] = in ? (T)vv[e] : (T)0.f;
    }
    __syncthreads();
    for (int qt = w; qt < NT; qt += 4) {
      const int iq = 32 * qt + l31;
      const bool qin = iq < N;
      const int iqc = qin ? iq : 0;
      const int tokq = sTok[iq], cntq = sCnt[iq];
      const Frag<T> qf = load_frag(qkv + (size_t)tokq * a.ldq + h * WD + 16 * lh);
      float q2 = sumsq(qf);
      q2 += __shfl_xor(q2, 32);
      const float qn = a.scale * sqrtf(q2);
      const float* __restrict__ taur = a.tau + ((size_t)h * a.Nt + iqc) * a.Nt;
      const float* __restrict__ biasr = a.bias + ((size_t)h * N + iqc) * N;
      float m = NEG, l = 0.f;
      f32x16 o;
#pragma unroll
      for (int r = 0; r < 16; ++r) o[r] = 0.f;
      for (int kt = 0; kt < NT; ++kt) {
        const int tokk = sTok[32 * kt + l31];
        const Frag<T> kf = load_frag(qkv + (size_t)tokk * a.ldq + a.C + h * WD + 16 * lh);
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
        mma_rows(kf, qf, st);
        float sv[16], tv[16], bv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = 32 * kt + acc_row(r, lh), jc = j < N ? j : 0;
          tv[r] = taur[jc];
          bv[r] = biasr[jc];
        }
        float tmax = NEG;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = 32 * kt + acc_row(r, lh);
          float s = st[r] * a.scale * rcp_(fmaxf(qn * sKn[j], 1e-6f)) * rcp_(fmaxf(tv[r], 0.01f)) + bv[r];
          if (sCnt[j] != cntq) s -= 100.f;
          s = j < N ? s : NEG;
          sv[r] = s;
          tmax = fmaxf(tmax, s);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float mn = fmaxf(m, tmax), corr = __expf(m - mn);
        float p[16], lp = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          p[r] = as_operand(T(), __expf(sv[r] - mn));
          lp += p[r];
          o[r] *= corr;
        }
        l = fmaf(l, corr, lp);
        m = mn;
        mma_t(sVT + l31 * WTS + 32 * kt + 4 * lh, p, o);
      }
      l += __shfl_xor(l, 32);
      if (qin) {
        const float inv = 1.f / l;
        T* orow = out + (size_t)tokq * a.ldo + h * WD + 4 * lh;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          float v4[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v4[e] = o[4 * q4 + e] * inv;
          store4(orow + 8 * q4, v4);
        }
        if (lh == 0) a.lse[((size_t)win * a.heads + h) * N + iq] = m + __logf(l);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Backward
// ---------------------------------------------------------------------------------------------
// one (query, key) element: the score, P, dS and what the products take from it.  The 1e-6 clamp of the cosine's
// denominator is followed pair by pair (no gradient through the norms where it holds), d(tau) is 0 below 0.01.
struct Elem {
  float p, ds, w1, nrm, dtau;
};
__device__ __forceinline__ Elem attn_elem(float u_raw, float dp, float scale, float qn, float kn, float other_n, float tv,
                                          float bias, bool masked, bool valid, float lse, float Di) {
  const float nn = qn * kn;
  const bool clamped = nn <= 1e-6f;
  const float rden = rcp_(clamped ? 1e-6f : nn);
  const float ti = rcp_(fmaxf(tv, 0.01f));
  const float u = u_raw * scale, c = u * rden;
  float s = c * ti + bias;
  if (masked) s -= 100.f;
  Elem e;
  e.p = valid ? __expf(s - lse) : 0.f;
  e.ds = e.p * (dp - Di);
  e.dtau = tv >= 0.01f ? -e.ds * c * ti * ti : 0.f;
  const float dc = e.ds * ti;
  e.w1 = dc * rden;
  e.nrm = clamped ? 0.f : dc * u * other_n * rden * rden;   // times 1 / (own norm): the norm term of dq / dk
  return e;
}

template <typename T>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? UZ_WIDE_SLOTS_BWD_BF16 : UZ_WIDE_SLOTS_BWD_F32))
void winattn_wide_bwd_kernel(const AttnArgs a) {
  __shared__ __attribute__((aligned(16))) T sKT[WD * WTS], sQT[WD * WTS], sGT[WD * WTS];
  __shared__ float sKn[WN], sQn[WN], sLse[WN], sDi[WN];
  __shared__ int sTok[WN], sCnt[WN];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, l31 = lane & 31, lh = lane >> 5, h = blockIdx.y;
  const int N = a.ws * a.ws, NT = (N + 31) >> 5;
  const int nWin = a.B * (a.H / a.ws) * (a.W / a.ws);
  const T* __restrict__ qkv = static_cast<const T*>(a.qkv);
  const T* __restrict__ out = static_cast<const T*>(a.out);
  const T* __restrict__ dout = static_cast<const T*>(a.dout);
  T* __restrict__ dqkv = static_cast<T*>(a.dqkv);
  float* __restrict__ part_b = a.partial + ((size_t)blockIdx.x * 2 * a.heads + h) * N * N;   // [row][2][heads][N][N]
  float* __restrict__ part_t = part_b + (size_t)a.heads * N * N;
  for (int win = blockIdx.x; win < nWin; win += gridDim.x) {
    const bool first = win == (int)blockIdx.x;
    __syncthreads();   // the previous window's readers are done
    {  // thread = token: norms, lse, D = dO . O, region id, token row, the K^T / Q^T / dO^T columns (zero for padding)
      const bool in = tid < N;
      const WinTok me = win_token(a, win, in ? tid : 0);
      const T* row = qkv + (size_t)me.tok * a.ldq + h * WD;
      float qq[WD], kk[WD], gg[WD], oo[WD];
      load32(row, qq);
      load32(row + a.C, kk);
      load32(dout + (size_t)me.tok * a.lddo + h * WD, gg);
      load32(out + (size_t)me.tok * a.ldo + h * WD, oo);
      const float lse = a.lse[((size_t)win * a.heads + h) * N + (in ? tid : 0)];
      float q2 = 0.f, k2 = 0.f, Di = 0.f;
#pragma unroll
      for (int e = 0; e < WD; ++e) {
        q2 = fmaf(qq[e], qq[e], q2);
        k2 = fmaf(kk[e], kk[e], k2);
        Di = fmaf(gg[e], oo[e], Di);
      }
      sQn[tid] = in ? a.scale * sqrtf(q2) : 1.f;
      sKn[tid] = in ? sqrtf(k2) : 1.f;
      sLse[tid] = in ? lse : 0.f;
      sDi[tid] = in ? Di : 0.f;
      sTok[tid] = me.tok;
      sCnt[tid] = in ? me.cnt : -1;
#pragma unroll
      for (int e = 0; e < WD; ++e) {
        sQT[e * WTS + tid] = in ? (T)qq[e] : (T)0.f;
        sKT[e * WTS + tid] = in ? (T)kk[e] : (T)0.f;
        sGT[e * WTS + tid] = in ? (T)gg[e] : (T)0.f;
      }
    }
    __syncthreads();
    // ---- pass 1: column = query, rows = keys -> d(bias), d(tau), dq
    for (int qt = w; qt < NT; qt += 4) {
      const int iq = 32 * qt + l31;
      const bool qin = iq < N;
      const int iqc = qin ? iq : 0;
      const int tokq = sTok[iq], cntq = sCnt[iq];
      const Frag<T> qf = load_frag(qkv + (size_t)tokq * a.ldq + h * WD + 16 * lh);
      const Frag<T> gf = load_frag(dout + (size_t)tokq * a.lddo + h * WD + 16 * lh);
      const float qn = sQn[iq], lse = sLse[iq], Di = sDi[iq];
      const float* __restrict__ taur = a.tau + ((size_t)h * a.Nt + iqc) * a.Nt;
      const float* __restrict__ biasr = a.bias + ((size_t)h * N + iqc) * N;
      float* __restrict__ pbr = part_b + (size_t)iqc * N;
      float* __restrict__ ptr = part_t + (size_t)iqc * N;
      f32x16 dq;
#pragma unroll
      for (int r = 0; r < 16; ++r) dq[r] = 0.f;
      float bs = 0.f;
      for (int kt = 0; kt < NT; ++kt) {
        const int tokk = sTok[32 * kt + l31];
        const T* krow = qkv + (size_t)tokk * a.ldq + a.C + h * WD + 16 * lh;
        const Frag<T> kf = load_frag(krow), vf = load_frag(krow + a.C);
        f32x16 st, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = dp[r] = 0.f;
        mma_rows(kf, qf, st);
        mma_rows(vf, gf, dp);
        float tv[16], bv[16], ob[16], ot[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = 32 * kt + acc_row(r, lh), jc = j < N ? j : 0;
          tv[r] = taur[jc];
          bv[r] = biasr[jc];
          ob[r] = pbr[jc];
          ot[r] = ptr[jc];
        }
        float w1[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = 32 * kt + acc_row(r, lh);
          const bool ok = qin && j < N;
          const float kn = sKn[j];
          const Elem e = attn_elem(st[r], dp[r], a.scale, qn, kn, kn, tv[r], bv[r], sCnt[j] != cntq, ok, lse, Di);
          w1[r] = e.w1;
          bs += e.nrm;
          if (ok) {
            pbr[j] = (first ? 0.f : ob[r]) + e.ds;
            ptr[j] = (first ? 0.f : ot[r]) + e.dtau;
          }
        }
        mma_t(sKT + l31 * WTS + 32 * kt + 4 * lh, w1, dq);
      }
      bs += __shfl_xor(bs, 32);
      bs *= rcp_(qn);
      if (qin) {
        T* drow = dqkv + (size_t)tokq * a.lddq + h * WD + 4 * lh;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          float v4[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float qs = a.scale * (float)sQT[(8 * q4 + 4 * lh + e) * WTS + iq];
            v4[e] = a.scale * (dq[4 * q4 + e] - bs * qs);
          }
          store4(drow + 8 * q4, v4);
        }
      }
    }
    // ---- pass 2: column = key, rows = queries -> dk, dv
    for (int kt = w; kt < NT; kt += 4) {
      const int jk = 32 * kt + l31;
      const bool kin = jk < N;
      const int jkc = kin ? jk : 0;
      const int tokk = sTok[jk], cntk = sCnt[jk];
      const T* krow = qkv + (size_t)tokk * a.ldq + a.C + h * WD + 16 * lh;
      const Frag<T> kf = load_frag(krow), vf = load_frag(krow + a.C);
      const float kn = sKn[jk];
      const float* __restrict__ tauc = a.tau + (size_t)h * a.Nt * a.Nt + jkc;
      const float* __restrict__ biasc = a.bias + (size_t)h * N * N + jkc;
      f32x16 dk, dv;
#pragma unroll
      for (int r = 0; r < 16; ++r) dk[r] = dv[r] = 0.f;
      float bsk = 0.f;
      for (int qt = 0; qt < NT; ++qt) {
        const int tokr = sTok[32 * qt + l31];
        const Frag<T> qf = load_frag(qkv + (size_t)tokr * a.ldq + h * WD + 16 * lh);
        const Frag<T> gf = load_frag(dout + (size_t)tokr * a.lddo + h * WD + 16 * lh);
        f32x16 st, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = dp[r] = 0.f;
        mma_rows(qf, kf, st);
        mma_rows(gf, vf, dp);
        float tv[16], bv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = 32 * qt + acc_row(r, lh), ic = i < N ? i : 0;
          tv[r] = tauc[(size_t)ic * a.Nt];
          bv[r] = biasc[(size_t)ic * N];
        }
        float pp[16], w1[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = 32 * qt + acc_row(r, lh);
          const bool ok = kin && i < N;
          const float qn = sQn[i];
          const Elem e = attn_elem(st[r], dp[r], a.scale, qn, kn, qn, tv[r], bv[r], sCnt[i] != cntk, ok, sLse[i], sDi[i]);
          pp[r] = e.p;
          w1[r] = e.w1;
          bsk += e.nrm;
        }
        mma_t(sGT + l31 * WTS + 32 * qt + 4 * lh, pp, dv);
        mma_t(sQT + l31 * WTS + 32 * qt + 4 * lh, w1, dk);
      }
      bsk += __shfl_xor(bsk, 32);
      bsk *= rcp_(kn);
      if (kin) {
        T* drow = dqkv + (size_t)tokk * a.lddq + a.C + h * WD + 4 * lh;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          float k4[4], v4[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            k4[e] = a.scale * dk[4 * q4 + e] - bsk * (float)sKT[(8 * q4 + 4 * lh + e) * WTS + jk];
            v4[e] = dv[4 * q4 + e];
          }
          store4(drow + 8 * q4, k4);
          store4(drow + a.C + 8 * q4, v4);
        }
      }
    }
  }
}

}  // namespace

int uz_winattn_wide_fwd_launch(int dtype, const AttnArgs& a, int grid_x, hipStream_t s) {
  const dim3 grid(grid_x, a.heads), block(256);
  if (dtype == UZ_BF16) hipLaunchKernelGGL((winattn_wide_fwd_kernel<bf16_t>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((winattn_wide_fwd_kernel<float>), grid, block, 0, s, a);
  UZ_LAUNCH_CHECK("uz_winattn_fwd (wide)");
  return UZ_OK;
}

int uz_winattn_wide_bwd_launch(int dtype, const AttnArgs& a, int grid_x, hipStream_t s) {
  const dim3 grid(grid_x, a.heads), block(256);
  if (dtype == UZ_BF16) hipLaunchKernelGGL((winattn_wide_bwd_kernel<bf16_t>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((winattn_wide_bwd_kernel<float>), grid, block, 0, s, a);
  UZ_LAUNCH_CHECK("uz_winattn_bwd (wide)");
  return UZ_OK;
}
