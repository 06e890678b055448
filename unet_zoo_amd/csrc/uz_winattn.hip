// Swin-UNet V2 window attention for gfx950 (MI355X)  (reference: unet_zoo/models/swin_unet_v2.py):
//   * window attention core, forward / backward                                          (:127-159):
//     cosine attention with learned per-entry temperature tau (clipped at 0.01), additive continuous
//     position bias, shifted-window mask computed from the region ids (:214-236), softmax, @v.
//     window_partition / torch.roll / window_reverse (:30-56, :246-262) are index arithmetic here
//     (win_token()): a (window, head) workgroup reads q, k, v of its tokens from the [P][3C] qkv tensor
//     and writes the head's output back to the SAME token rows.
//   * the continuous position bias MLP (cpb) that produces the additive bias                (:121-125)
// Two kernel families, chosen by attn_plan(): windows of up to 64 tokens (window_size <= 8) sit in one
// 64-row tile -- plain fp32 VALU code for fp32 (one thread per query in the forward and the first
// backward phase, per key in the second), matrix-core kernels for bf16; windows of 65 .. 256 tokens
// (window_size 9 .. 16) are walked in 32 x 32 tiles on the matrix cores in both dtypes.  All are
// flash-style: the forward keeps only the row log-sum-exp, the backward recomputes P.  Workgroups stay
// resident and walk their share of the windows, so every grid is sized by the kernel's slots constant
// (tests/test_winattn_resources.py holds those to the compiled kernels' registers and LDS).
// The Linear layers around these run on the LDS-DMA GEMM (uz_gemm_dma.hip) and the weight-gradient kernels.
#include "uz_common.h"

// The kernels' one argument.  Used by this file only; it sits outside the unnamed namespace because its name is part of
// the kernels' symbols.
struct AttnArgs {
  const void* qkv;    // [P][3C]: per token [3][heads][32]
  void* out;          // [P][C]   (bwd: the forward output, read)
  float* lse;         // [B*nW][heads][N] row log-sum-exp
  const float* tau;   // [heads][Nt][Nt] (Nt = window_size^2 of the parameter, N <= Nt used)
  const float* bias;  // [heads][N][N]
  const void* dout;   // bwd: gradient of out [P][C]
  void* dqkv;         // bwd: gradient of qkv [P][3C]
  float* partial;     // bwd: [gridDim.x][2][heads][N][N] sums of dS (dbias) and d(tau)
  int B, H, W, C, heads, ws, shift, Nt;
  int ldq, ldo, lddo, lddq;
  float scale;
  int flags;          // ablation build only (UZ_KFLAGS)
};

namespace {

struct WinTok {
  int tok;   // row of the token tensor
  int cnt;   // region id of the shifted-window mask
};
__device__ __forceinline__ WinTok win_token(const AttnArgs& a, int win, int i) {
  const int nwx = a.W / a.ws, nwy = a.H / a.ws, nW = nwx * nwy;
  const int b = win / nW, wi = win - b * nW, wy = wi / nwx, wx = wi - wy * nwx;
  const int iy = i / a.ws, ix = i - iy * a.ws;
  const int hs = wy * a.ws + iy, wsx = wx * a.ws + ix;  // coordinates in the rolled image
  int h = hs + a.shift, w = wsx + a.shift;
  if (h >= a.H) h -= a.H;
  if (w >= a.W) w -= a.W;
  WinTok t;
  t.tok = (b * a.H + h) * a.W + w;
  const int hid = hs < a.H - a.ws ? 0 : (hs < a.H - a.shift ? 1 : 2);
  const int wid = wsx < a.W - a.ws ? 0 : (wsx < a.W - a.shift ? 1 : 2);
  t.cnt = a.shift > 0 ? hid * 3 + wid : 0;
  return t;
}

// Resident workgroups per CU of each kernel.  Workgroups stay resident for the whole launch, so the grids are sized by
// these (attn_plan()); tests/test_winattn_resources.py reads them from this file and holds them to the registers and
// the LDS of the compiled kernels.
constexpr int ATTN_SLOTS_FWD = 2;           // winattn_fwd_kernel<float>
constexpr int ATTN_SLOTS_FWD_MFMA2 = 3;     // winattn_fwd_mfma2_kernel
constexpr int ATTN_SLOTS_BWD = 1;           // winattn_bwd_kernel<float>
constexpr int ATTN_SLOTS_BWD_MFMA = 2;      // winattn_bwd_mfma_kernel
constexpr int UZ_WIDE_SLOTS_FWD = 2;        // winattn_wide_fwd_kernel<T>
constexpr int UZ_WIDE_SLOTS_BWD_BF16 = 2;   // winattn_wide_bwd_kernel<bf16_t>
constexpr int UZ_WIDE_SLOTS_BWD_F32 = 1;    // winattn_wide_bwd_kernel<float>
constexpr int UZ_WIDE_MAXN = 256;           // tokens per window at most (16 x 16)
constexpr long long UZ_WIDE_PARTIAL_BYTES = 64LL << 20;   // cap of one wide backward launch's d(bias) / d(tau) partial rows

template <typename T> __device__ __forceinline__ void load_f(const T* p, float* f) {
  const Vec16<T> v = ld16(p);
#pragma unroll
  for (int i = 0; i < ElemTraits<T>::VEC; ++i) f[i] = (float)v.v[i];
}
template <typename T> __device__ __forceinline__ void store_f(T* p, const float* f) {
  Vec16<T> v;
#pragma unroll
  for (int i = 0; i < ElemTraits<T>::VEC; ++i) v.v[i] = (T)f[i];
  st16(p, v);
}

// ---------------------------------------------------------------------------------------------
// Windows of up to 64 tokens (window_size <= 8): the whole window in one 64-row tile.
// ---------------------------------------------------------------------------------------------
constexpr int AD = 32;       // head dimension (embed_dim 96 / 3 heads, doubled together: always 32)
constexpr int AN = 64;       // max tokens per window of the one-tile kernels (window_size <= 8; wider: the tile-walking kernels)
constexpr int ARS = AD + 4;  // LDS row stride of the [token][32] tiles: rows stay 16-byte aligned, so a row
                             // (read by all lanes at once = broadcast) costs 8 ds_read_b128, not 32 ds_read_b32
constexpr int ANS = AN + 1;  // LDS row stride of the [N][N] matrices
constexpr int AJ = AN / 4;   // keys (forward, backward phase A) per wave: the four waves split the other index

__device__ __forceinline__ void lds_row(const float* row, float* f) {  // 32 floats, 16-byte aligned
#pragma unroll
  for (int c = 0; c < AD / 4; ++c) {
    const float4 v = reinterpret_cast<const float4*>(row)[c];
    f[4 * c] = v.x;
    f[4 * c + 1] = v.y;
    f[4 * c + 2] = v.z;
    f[4 * c + 3] = v.w;
  }
}
__device__ __forceinline__ float rcp(float x) { return __builtin_amdgcn_rcpf(x); }  // v_rcp_f32, 1 ulp

// 32-wide fp32 vector helpers written on float pairs so that they compile to v_pk_fma_f32 / v_pk_mul_f32
// (two fp32 operations per lane and instruction): the attention kernels are VALU-bound
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
__device__ __forceinline__ float dot32(const float* a, const float* b) {
  f32x2 acc = {0.f, 0.f};
#pragma unroll
  for (int e = 0; e < AD; e += 2) {
    const f32x2 x = {a[e], a[e + 1]}, y = {b[e], b[e + 1]};
    acc = __builtin_elementwise_fma(x, y, acc);
  }
  return acc.x + acc.y;
}
__device__ __forceinline__ void axpy32(float w, const float* x, float* y) {  // y += w * x
  const f32x2 ws = {w, w};
#pragma unroll
  for (int e = 0; e < AD; e += 2) {
    const f32x2 xv = {x[e], x[e + 1]}, yv = {y[e], y[e + 1]};
    const f32x2 r = __builtin_elementwise_fma(ws, xv, yv);
    y[e] = r.x;
    y[e + 1] = r.y;
  }
}
__device__ __forceinline__ void scale_axpy32(float c, float w, const float* x, float* y) {  // y = c * y + w * x
  const f32x2 cs = {c, c}, ws = {w, w};
#pragma unroll
  for (int e = 0; e < AD; e += 2) {
    const f32x2 xv = {x[e], x[e + 1]}, yv = {y[e], y[e + 1]};
    const f32x2 r = __builtin_elementwise_fma(ws, xv, cs * yv);
    y[e] = r.x;
    y[e + 1] = r.y;
  }
}

template <typename T> __device__ __forceinline__ void load_head(const T* p, float* f) {  // 32 values
  constexpr int VEC = ElemTraits<T>::VEC;
#pragma unroll
  for (int c = 0; c < AD / VEC; ++c) load_f(p + c * VEC, f + c * VEC);
}

template <typename T> __device__ __forceinline__ void store8(T* p, const float* f) {  // 8 consecutive values
  constexpr int VEC = ElemTraits<T>::VEC;
#pragma unroll
  for (int c = 0; c < 8 / VEC; ++c) store_f(p + c * VEC, f + c * VEC);
}

// Forward: one 256-thread workgroup (one wave per SIMD) per (window, head); lane = query i, the four
// waves split the key range, each with its own running (max, sum, output); the partial states are
// merged through LDS in a fixed order.
template <typename T>
__global__ __launch_bounds__(256) void winattn_fwd_kernel(const AttnArgs a) {
  constexpr int PS = AD + 3;  // partial row: 32 outputs, max, sum (+1 pad)
  __shared__ float sK[AN * ARS], sV[AN * ARS], sKn[AN], sPart[4 * AN * PS];
  __shared__ int sCnt[AN];
  const int tid = threadIdx.x, w = tid >> 6, i = tid & 63, h = blockIdx.y;
  const int N = a.ws * a.ws;
  const int jc = (N + 3) >> 2, lo = w * jc, hi = min(N, lo + jc);
  const int nWin = a.B * (a.H / a.ws) * (a.W / a.ws);
  const T* __restrict__ qkv = static_cast<const T*>(a.qkv);
  T* __restrict__ out = static_cast<T*>(a.out);
  // 1/clip(tau) and bias of this thread's (query, key range): fixed for the head, kept in registers
  float ti[AJ], bi[AJ];
#pragma unroll
  for (int jj = 0; jj < AJ; ++jj) {
    const int j = lo + jj;
    const bool ok = i < N && j < hi;
    ti[jj] = ok ? 1.f / fmaxf(a.tau[((size_t)h * a.Nt + i) * a.Nt + j], 0.01f) : 0.f;
    bi[jj] = ok ? a.bias[((size_t)h * N + i) * N + j] : 0.f;
  }
  for (int win = blockIdx.x; win < nWin; win += gridDim.x) {
    __syncthreads();  // previous window's readers are done
    float q[AD];
    float qn = 0.f;
    WinTok me = {0, 0};
    if (i < N) {
      me = win_token(a, win, i);
      const T* row = qkv + (size_t)me.tok * a.ldq + h * AD;
      load_head(row, q);
#pragma unroll
      for (int e = 0; e < AD; ++e) {
        q[e] *= a.scale;
        qn += q[e] * q[e];
      }
      qn = sqrtf(qn);
      if (w == 0) {
        float kv[AD];
        load_head(row + a.C, kv);
        float kn = 0.f;
#pragma unroll
        for (int e = 0; e < AD; ++e) {
          kn += kv[e] * kv[e];
          sK[i * ARS + e] = kv[e];
        }
        sKn[i] = sqrtf(kn);
        sCnt[i] = me.cnt;
      } else if (w == 1) {
        float kv[AD];
        load_head(row + 2 * a.C, kv);
#pragma unroll
        for (int e = 0; e < AD; ++e) sV[i * ARS + e] = kv[e];
      }
    }
    __syncthreads();
    {
      float m = -INFINITY, l = 0.f, o[AD];
#pragma unroll
      for (int e = 0; e < AD; ++e) o[e] = 0.f;
      if (i < N) {
#pragma unroll
        for (int jj = 0; jj < AJ; ++jj) {
          const int j = lo + jj;
          if (j < hi) {
            float row[AD];
            lds_row(sK + j * ARS, row);
            const float u = dot32(q, row);
            float s = u * rcp(fmaxf(qn * sKn[j], 1e-6f)) * ti[jj] + bi[jj];
            if (sCnt[j] != me.cnt) s -= 100.f;
            const float mn = fmaxf(m, s);
            const float corr = __expf(m - mn), p = __expf(s - mn);
            l = l * corr + p;
            lds_row(sV + j * ARS, row);
            scale_axpy32(corr, p, row, o);
            m = mn;
          }
        }
      }
      float* pr = sPart + (w * AN + i) * PS;
#pragma unroll
      for (int e = 0; e < AD; ++e) pr[e] = o[e];
      pr[AD] = m;
      pr[AD + 1] = l;
    }
    __syncthreads();
    if (i < N) {  // merge the four partial states; wave w writes output components [8w, 8w + 8)
      float m = -INFINITY;
#pragma unroll
      for (int k = 0; k < 4; ++k) m = fmaxf(m, sPart[(k * AN + i) * PS + AD]);
      float l = 0.f, o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float* pr = sPart + (k * AN + i) * PS;
        const float f = pr[AD + 1] > 0.f ? __expf(pr[AD] - m) : 0.f;  // a wave with an empty key range has l = 0
        l = fmaf(pr[AD + 1], f, l);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = fmaf(pr[8 * w + e], f, o[e]);
      }
      const float inv = 1.f / l;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] *= inv;
      store8(out + (size_t)me.tok * a.ldo + h * AD + 8 * w, o);
      if (w == 0) a.lse[((size_t)win * a.heads + h) * N + i] = m + __logf(l);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// bf16 on the matrix cores, windows of up to 64 tokens.  Common to the forward and the backward below:
//   S^T = K Q^T   v_mfma_f32_32x32x16_bf16, K rows / Q rows straight from global memory as the A / B
//                 fragments (16 bytes of one token's head slice per lane) -> accumulator column = query
//                 (lane & 31), rows = keys: a lane owns, for ITS query, 16 keys per 32-key tile, so the
//                 softmax runs over registers, no LDS round trip;
//   O^T = V^T P^T the exponentials are packed to bf16 in registers and are directly the B fragment (the
//                 accumulator's key order 32kt + 16s + 8(e>>2) + 4(lane>>5) + (e&3) is used as the K order
//                 of both operands); V^T comes from an LDS tile [32 d][64 keys].
// ---------------------------------------------------------------------------------------------
constexpr int VTS = 72;  // V^T row stride in bf16 elements (144 B: 8-byte aligned rows, spreads banks)

// ---------------------------------------------------------------------------------------------
// bf16 backward on the matrix cores.
// Pass 1 (accumulator column = query i, rows = keys): U^T = K Q^T and dP^T = V dO^T by MFMA, then per
// element P, dS, d(bias) / d(tau) sums (registers, kept over the wave's windows) and W1 = dS/(tau den);
// dQ^T = K^T W1^T with the bf16-packed W1 registers as the B fragment.  Pass 2 (column = key j, rows =
// queries): U = Q K^T, dP = dO V^T, the same element math, dV^T = dO^T P and dK^T = Q^T W1.  The
// transposed operands (K^T, dO^T, Q^T: [32 d][64 tokens]) are per-wave LDS tiles.
// (A first version with one wave per (window, head) needed 128 running-sum registers per lane, spilled and
// was slower than the VALU kernel; see the block decomposition inside the kernel.)
// ---------------------------------------------------------------------------------------------
// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for vmcnt(0): every global load in flight (the
// next window's prefetch) and every global store (the window's results, acknowledged ~1 us after issue) -- four such drains
// per window were more than half of the attention kernels' wave time (SQ_WAIT_ANY / SQ_WAVE_CYCLES = 0.55).  The kernels
// below exchange data between waves through LDS only.
// Contract of every call site (round-4 review): (1) nothing a wave wrote to GLOBAL memory is read by another wave of the
// workgroup afterwards -- results leave through each wave's own stores, the prefetch loads land in registers of the wave that
// issued them -- so no vmcnt wait is owed; (2) every call sits in workgroup-uniform control flow (the window loop's trip count
// and the pass structure depend on blockIdx and kernel arguments only), as s_barrier requires; `asm volatile` with a memory
// clobber is not moved across other memory accesses or into a branch by the compiler.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ bf16x8 pack8(const float* f) {
  bf16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (bf16_t)f[e];
  return v;
}
// A fragment of a transposed tile XT[d][token]: row d = l31, the 8 K-slots = tokens 32 t + 16 s + 4 lh + {0..3}, + 8
__device__ __forceinline__ bf16x8 tfrag(const bf16_t* xt, int l31, int lh, int t, int s2) {
  const bf16_t* p = xt + l31 * VTS + 32 * t + 16 * s2 + 4 * lh;
  const bf16x4 lo4 = *reinterpret_cast<const bf16x4*>(p), hi4 = *reinterpret_cast<const bf16x4*>(p + 8);
  return __builtin_shufflevector(lo4, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
}

__global__ __launch_bounds__(256, 2) void winattn_bwd_mfma_kernel(const AttnArgs a) {
  // One workgroup per (window, head); wave w owns the 32 x 32 block (query tile qt = w >> 1, key tile kt = w & 1)
  // of the score matrix, so a lane carries 16 + 16 running sums instead of 128 and the element code exists once.
  // The element pass runs with column = query (everything per query is the lane's own); it leaves P and
  // W = dC / (|q||k|) of its block in LDS as bf16 [key][query], which is the B operand of the dk / dv products,
  // so there is no second element pass.  The projection terms of the two normalisations come from the products
  // themselves: with A_i = sum_j W_ij k_j, sum_j dC_ij c_ij = q_i . A_i (likewise for k), a 32-term dot in
  // the epilogue instead of six operations per score element.  The reference clamps the norm product at 1e-6
  // (swin_unet_v2.py:137-139): a clamped pair keeps u / 1e-6 and has NO projection term.  Round 5 follows that to the
  // letter: a wave whose queries could reach the clamp against this key tile (|scale q| * min |k| < 1e-6, a test of one
  // multiply per window) takes a slow path that sums W_ij u_ij over its clamped pairs -- per query in a register, per key
  // by shuffles into sCorrK -- and the epilogues subtract those sums from q_i . A_i / k_j . B_j.  (Rounds 1-4 kept the
  // projection term for 0 < |q||k| <= 1e-6 and were exact for zero rows only.)
  // Partial dq (over kt) and dk / dv (over qt) of the two waves that share a tile meet in LDS.
  __shared__ __attribute__((aligned(16))) bf16_t sKT[AD * VTS], sGT[AD * VTS], sQT[AD * VTS];
  __shared__ __attribute__((aligned(16))) bf16_t sPW[2 * AN * VTS];   // P, W [key][query]; later the dk / dv hand-over
  __shared__ float sRedQ[2][64 * 17];   // dq hand-over of the kt = 1 waves, [lane][16] (+1 pad)
  __shared__ __attribute__((aligned(16))) float sRk[AN];   // 1 / |k_j|
  __shared__ __attribute__((aligned(16))) int sCnt[AN];
  __shared__ float sRkMax[2];        // per key tile: max 1 / |k_j| over its non-zero keys
  __shared__ float sCorrK[2][AN];    // [query tile][key]: sum over the tile's CLAMPED pairs of W_ij u_ij (zero in the fast path)
  // 1 / clip(tau) (negated where the clip is active) and the bias of this head in LANE ORDER: a lane's 16 score elements are
  // the same (query, key) pairs in every window, [table][g4][thread] holds its four values of key group g4 as one 16-byte
  // read that is conflict-free across the wave (the [query][key] table it replaces cost 32 ds_read_b32 per window, each
  // waited for where it was used)
  __shared__ float4 sTabL[2][4][256];
  static_assert(2 * 2 * 64 * 17 * sizeof(float) <= sizeof(bf16_t) * 2 * AN * VTS, "dk / dv hand-over must fit in sPW");
  bf16_t* sP = sPW;
  bf16_t* sW = sPW + AN * VTS;
  float* sRedK = reinterpret_cast<float*>(sPW);   // [2 key tiles][2 (dk, dv)][64 * 17]
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, l31 = lane & 31, lh = lane >> 5, h = blockIdx.y;
  const int qt = w >> 1, kt = w & 1;
  const int N = a.ws * a.ws;
  const int nWin = a.B * (a.H / a.ws) * (a.W / a.ws);
  const bool masked = a.shift > 0;
  const bf16_t* __restrict__ qkv = static_cast<const bf16_t*>(a.qkv);
  const bf16_t* __restrict__ out = static_cast<const bf16_t*>(a.out);
  const bf16_t* __restrict__ dout = static_cast<const bf16_t*>(a.dout);
  bf16_t* __restrict__ dqkv = static_cast<bf16_t*>(a.dqkv);
  const int iq = 32 * qt + l31, jk = 32 * kt + l31;   // this lane's query (column role) / key (column role)
  // running sums over this workgroup's windows of dS (-> d bias) and dS * c (-> d tau) for
  // (query 32 qt + l31, key 32 kt + 4 lh + (r & 3) + 8 (r >> 2))
  f32x2 accb2[8], acct2[8];   // element pairs (r, r + 1)
#pragma unroll
  for (int r = 0; r < 8; ++r) accb2[r] = acct2[r] = (f32x2){0.f, 0.f};
  // the two tables: coalesced rows from global memory into a [query][key] staging tile (the P / W area), then each lane
  // gathers its own 16 entries into the lane-order table
  float* stage = reinterpret_cast<float*>(sPW);   // [AN][ANS] floats
  static_assert(AN * ANS * sizeof(float) <= sizeof(bf16_t) * 2 * AN * VTS, "the staging tile must fit in sPW");
  {
    // all 32 loads of a thread in flight at once (as a loop of load -> divide -> store they were 16 serialized memory round
    // trips, 8 us of a kernel that spends 4 us per window)
    float tv[16], bv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int e = tid + 256 * i, r = e >> 6, c = e & 63;
      const bool in = r < N && c < N && !(UZ_KFLAGS(a) & 0x10000);
      // (unconditional loads -- entry (0, 0) for a lane outside the window -- then a select: under `in ? ... :` every load
      // was waited for before the next was issued, the "16 serialized round trips" again)
      tv[i] = a.tau[in ? ((size_t)h * a.Nt + r) * a.Nt + c : 0];
      bv[i] = a.bias[in ? ((size_t)h * N + r) * N + c : 0];
    }
    // (the loaded values are made opaque before the selects: a value that is only used when `in` holds is otherwise turned back
    // into a load under a branch)
#pragma unroll
    for (int i = 0; i < 16; ++i) asm volatile("" : "+v"(tv[i]), "+v"(bv[i]));
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int e = tid + 256 * i, r = e >> 6, c = e & 63;
      const bool in = r < N && c < N && !(UZ_KFLAGS(a) & 0x10000);
      tv[i] = in ? tv[i] : 1.f;
      bv[i] = in ? bv[i] : ((r < N && c < N) ? 0.f : -1e30f);   // padding: exp() = 0, no test
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int e = tid + 256 * i, r = e >> 6, c = e & 63;
        const float inv = 1.f / fmaxf(tv[i], 0.01f);
        stage[r * ANS + c] = t == 0 ? (tv[i] >= 0.01f ? inv : -inv) : bv[i];   // negated where the clip is active
      }
      __syncthreads();
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const float* sp = stage + iq * ANS + 32 * kt + 8 * g4 + 4 * lh;
        sTabL[t][g4][tid] = make_float4(sp[0], sp[1], sp[2], sp[3]);
      }
      __syncthreads();
    }
  }

  // A window's q, dO, O, k, v fragments are fetched one window ahead: the loads are issued right after the
  // score products have consumed the current ones and land during the element pass.
  WinTok ntq = {0, -1}, ntk = {0, -1};
  bf16x8 nq[2], ng[2], no[2], nk[2], nv[2];
  float nlse = 0.f;
  // (The forward kernel's fetch is unconditional, DESIGN 3h.  Here that form measured SLOWER -- 52.8 -> 58.9 us on the 64 x 64
  // token map -- the loop's top then waits with the previous window's dq / dk / dv stores behind the prefetched loads; the
  // conditional form waits for its loads right here, before those stores are issued, and the second resident workgroup of the
  // CU covers the round trip.)
  auto fetch = [&](int win) {
    ntq = {0, -1};
    ntk = {0, -1};
    nlse = 0.f;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int e = 0; e < 8; ++e) nq[ks][e] = ng[ks][e] = no[ks][e] = nk[ks][e] = nv[ks][e] = (bf16_t)0.f;
    if (iq < N) {
      ntq = win_token(a, win, iq);
      const bf16_t* row = qkv + (size_t)ntq.tok * a.ldq + h * AD + 8 * lh;
      const bf16_t* grow = dout + (size_t)ntq.tok * a.lddo + h * AD + 8 * lh;
      const bf16_t* orow = out + (size_t)ntq.tok * a.ldo + h * AD + 8 * lh;
      nlse = a.lse[((size_t)win * a.heads + h) * N + iq];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        nq[ks] = *reinterpret_cast<const bf16x8*>(row + 16 * ks);
        ng[ks] = *reinterpret_cast<const bf16x8*>(grow + 16 * ks);
        no[ks] = *reinterpret_cast<const bf16x8*>(orow + 16 * ks);
      }
    }
    if (jk < N) {
      ntk = win_token(a, win, jk);
      const bf16_t* row = qkv + (size_t)ntk.tok * a.ldq + a.C + h * AD + 8 * lh;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        nk[ks] = *reinterpret_cast<const bf16x8*>(row + 16 * ks);
        nv[ks] = *reinterpret_cast<const bf16x8*>(row + a.C + 16 * ks);
      }
    }
  };
  if ((int)blockIdx.x < nWin) fetch(blockIdx.x);

  for (int win = blockIdx.x; win < nWin; win += gridDim.x) {
    if (UZ_KFLAGS(a) & 0x40000) break;
    lds_barrier();   // previous window: every reader of the tiles / hand-over areas is done (and sTab has landed)
    const WinTok tq = ntq, tkk = ntk;
    bf16x8 qf[2], gf[2], kf[2], vf[2];
    float rq = 0.f, Di = 0.f;
    const float lse = nlse;
    {
      float q2 = 0.f, k2 = 0.f;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        qf[ks] = nq[ks];
        gf[ks] = ng[ks];
        kf[ks] = nk[ks];
        vf[ks] = nv[ks];
        // |q|^2, |k|^2 and dO . O on bf16 pairs (v_dot2c_f32_bf16: fp32 products and sums), 12 instructions instead of ~130
        const bf16x2* qp = reinterpret_cast<const bf16x2*>(&qf[ks]);
        const bf16x2* kp = reinterpret_cast<const bf16x2*>(&kf[ks]);
        const bf16x2* gp = reinterpret_cast<const bf16x2*>(&gf[ks]);
        const bf16x2* op = reinterpret_cast<const bf16x2*>(&no[ks]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          q2 = __builtin_amdgcn_fdot2_f32_bf16(qp[e], qp[e], q2, false);
          k2 = __builtin_amdgcn_fdot2_f32_bf16(kp[e], kp[e], k2, false);
          Di = __builtin_amdgcn_fdot2_f32_bf16(gp[e], op[e], Di, false);
        }
      }
      q2 += __shfl_xor(q2, 32);
      Di += __shfl_xor(Di, 32);
      k2 += __shfl_xor(k2, 32);
      rq = rcp(a.scale * sqrtf(q2));   // inf for a zero row: the product below is clamped
      if (kt == 0) {   // the two waves of a query tile hold the same q / dO: one of them publishes
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int d = 16 * ks + 8 * lh + e;
            sGT[d * VTS + iq] = gf[ks][e];
            sQT[d * VTS + iq] = qf[ks][e];
          }
      }
      if (lh == 0) sCorrK[qt][jk] = 0.f;   // this wave's own region; filled by its slow path only
      if (qt == 0) {
        if (lh == 0) {
          sRk[jk] = rcp(sqrtf(k2));
          sCnt[jk] = tkk.cnt;
        }
        float rkm = k2 > 0.f ? rcp(sqrtf(k2)) : 0.f;   // zero keys (padding, dead rows) cannot contribute: u = 0
#pragma unroll
        for (int m = 1; m < 32; m <<= 1) rkm = fmaxf(rkm, __shfl_xor(rkm, m));
        if (lane == 0) sRkMax[kt] = rkm;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int e = 0; e < 8; ++e) sKT[(16 * ks + 8 * lh + e) * VTS + jk] = kf[ks][e];
      }
    }
    lds_barrier();

    // ---------------- element pass: column = query iq, rows = keys of tile kt
    f32x16 dq, dk, dv;
    float corrQ_keep = 0.f;
    {
      f32x16 ut, dt;
#pragma unroll
      for (int r = 0; r < 16; ++r) ut[r] = dt[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        ut = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], ut, 0, 0, 0);
        dt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[ks], gf[ks], dt, 0, 0, 0);
      }
      if (win + (int)gridDim.x < nWin) fetch(win + gridDim.x);
      float w1[16];
      // could any pair of this wave fall under the clamp?  1 / (|scale q_i| |k_j|) > 1e6 for the smallest non-zero |k| of the tile
      float corrQ = 0.f;
      const bool slow = __ballot(rq < INFINITY && rq * sRkMax[kt] > 1e6f) != 0;
      bf16_t* pcol = sP + (32 * kt + 4 * lh) * VTS + iq;
      bf16_t* wcol = sW + (32 * kt + 4 * lh) * VTS + iq;
      // per key group of four: 1 / |k|, the two table entries (and, under the shifted-window mask, the region ids) in one
      // 16-byte read each -- own data of the lane, so the 16 elements are independent chains; the arithmetic runs on float
      // pairs (v_pk_mul / v_pk_fma / v_pk_add_f32: two elements per instruction)
      const f32x2 sc2 = {a.scale, a.scale}, rq2 = {rq, rq}, nlse2 = {-lse, -lse}, nDi2 = {-Di, -Di};
      const f32x2 l2e2 = {1.44269504088896341f, 1.44269504088896341f};
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const float4 v = *reinterpret_cast<const float4*>(&sRk[32 * kt + 8 * g4 + 4 * lh]);
        const float4 t = sTabL[0][g4][tid], b = sTabL[1][g4][tid];
        float4 pn = make_float4(0.f, 0.f, 0.f, 0.f);
        if (masked) {
          const int4 c4 = *reinterpret_cast<const int4*>(&sCnt[32 * kt + 8 * g4 + 4 * lh]);
          pn.x = c4.x != tq.cnt ? -100.f : 0.f;
          pn.y = c4.y != tq.cnt ? -100.f : 0.f;
          pn.z = c4.z != tq.cnt ? -100.f : 0.f;
          pn.w = c4.w != tq.cnt ? -100.f : 0.f;
        }
#pragma unroll
        for (int hp = 0; hp < 2; ++hp) {
          const int r = 4 * g4 + 2 * hp, jr = 2 * hp + 8 * g4;   // jr: key row inside the tile, less 4 * lh
          const f32x2 rk2 = hp ? (f32x2){v.z, v.w} : (f32x2){v.x, v.y};
          const f32x2 ti2 = hp ? (f32x2){fabsf(t.z), fabsf(t.w)} : (f32x2){fabsf(t.x), fabsf(t.y)};
          const f32x2 bi2 = hp ? (f32x2){b.z, b.w} : (f32x2){b.x, b.y};
          const f32x2 pn2 = hp ? (f32x2){pn.z, pn.w} : (f32x2){pn.x, pn.y};
          const f32x2 ut2 = {ut[r], ut[r + 1]}, dt2 = {dt[r], dt[r + 1]};
          f32x2 rden = rq2 * rk2;                                  // 1 / max(|scale q||k|, 1e-6)
          const bool cx = slow && rden.x > 1e6f, cy = slow && rden.y > 1e6f;
          rden.x = fminf(rden.x, 1e6f);
          rden.y = fminf(rden.y, 1e6f);
          const f32x2 c = (ut2 * sc2) * rden;
          f32x2 sv = __builtin_elementwise_fma(c, ti2, bi2);
          if (masked) sv += pn2;
          const f32x2 ea = (sv + nlse2) * l2e2;
          const f32x2 pp = {__builtin_amdgcn_exp2f(ea.x), __builtin_amdgcn_exp2f(ea.y)};
          const f32x2 ds = pp * (dt2 + nDi2);
          accb2[r >> 1] += ds;
          acct2[r >> 1] = __builtin_elementwise_fma(ds, c, acct2[r >> 1]);
          const f32x2 ww = (ds * ti2) * rden;
          if (slow) {   // wave-uniform; W_ij u_ij of the clamped pairs: per query here, per key across the 32 query lanes
            float ex = cx ? ww.x * ut2.x : 0.f, ey = cy ? ww.y * ut2.y : 0.f;
            corrQ += ex + ey;
#pragma unroll
            for (int m = 1; m < 32; m <<= 1) {
              ex += __shfl_xor(ex, m);
              ey += __shfl_xor(ey, m);
            }
            if (l31 == 0) {
              sCorrK[qt][32 * kt + 4 * lh + jr] = ex;
              sCorrK[qt][32 * kt + 4 * lh + jr + 1] = ey;
            }
          }
          w1[r] = ww.x;
          w1[r + 1] = ww.y;
          pcol[jr * VTS] = (bf16_t)pp.x;
          pcol[(jr + 1) * VTS] = (bf16_t)pp.y;
          wcol[jr * VTS] = (bf16_t)ww.x;
          wcol[(jr + 1) * VTS] = (bf16_t)ww.y;
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) dq[r] = dk[r] = dv[r] = 0.f;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
        dq = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tfrag(sKT, l31, lh, kt, s2), pack8(w1 + 8 * s2), dq, 0, 0, 0);
      // dv, dk partials of (key tile kt) over (query tile qt): the B operand is this wave's own P / W block
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        dv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tfrag(sGT, l31, lh, qt, s2), tfrag(sP + 32 * kt * VTS, l31, lh, qt, s2), dv, 0, 0, 0);
        dk = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tfrag(sQT, l31, lh, qt, s2), tfrag(sW + 32 * kt * VTS, l31, lh, qt, s2), dk, 0, 0, 0);
      }
      if (kt == 1) {   // hand the dq partial to the kt = 0 wave of this query tile
        float* red = &sRedQ[qt][lane * 17];
#pragma unroll
        for (int r = 0; r < 16; ++r) red[r] = dq[r];
        red[16] = corrQ;
      }
      corrQ_keep = corrQ;
    }
    lds_barrier();   // dq partials visible; every wave is done with P / W
    if (kt == 0 && iq < N) {
      // dq_i = scale * (A_i - (q_i . A_i) / |q_i|^2 q_i), A_i = sum_j W_ij k_j
      const float* r1 = &sRedQ[qt][lane * 17];
      bf16_t* drow = dqkv + (size_t)tq.tok * a.lddq + h * AD + 4 * lh;
      float qv[16], dot = 0.f, q2 = 0.f;
      // q_i from the transposed LDS tile, not from global memory again: a load here waits behind the next window's prefetch
      // and in front of this window's stores (vmcnt is in order), a full memory round trip per window and epilogue
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * q4 + e;
          qv[r] = (float)sQT[(4 * lh + 8 * q4 + e) * VTS + iq];
          dq[r] += r1[r];
          dot = fmaf(qv[r], dq[r], dot);
          q2 = fmaf(qv[r], qv[r], q2);
        }
      }
      dot += __shfl_xor(dot, 32);
      q2 += __shfl_xor(q2, 32);
      float cq = corrQ_keep + r1[16];          // the clamped pairs of both key tiles ...
      cq += __shfl_xor(cq, 32);                // ... and both halves of the rows: they have no projection term
      const float pr = (dot - cq) * rcp(fmaxf(q2, 1e-30f));
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        bf16x4 o4;
#pragma unroll
        for (int e = 0; e < 4; ++e) o4[e] = (bf16_t)(a.scale * (dq[4 * q4 + e] - pr * qv[4 * q4 + e]));
        *reinterpret_cast<bf16x4*>(drow + 8 * q4) = o4;
      }
    }
    if (qt == 1) {     // hand the dk / dv partials to the qt = 0 wave of this key tile
      float* red = sRedK + (kt * 2 + 0) * 64 * 17 + lane * 17;
      float* red2 = sRedK + (kt * 2 + 1) * 64 * 17 + lane * 17;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        red[r] = dk[r];
        red2[r] = dv[r];
      }
    }
    lds_barrier();
    if (qt == 0 && jk < N) {
      // dk_j = B_j - (k_j . B_j) / |k_j|^2 k_j, B_j = scale * sum_i W_ij q_i
      const float* k1 = sRedK + (kt * 2 + 0) * 64 * 17 + lane * 17;
      const float* v1 = sRedK + (kt * 2 + 1) * 64 * 17 + lane * 17;
      bf16_t* drow = dqkv + (size_t)tkk.tok * a.lddq + a.C + h * AD + 4 * lh;
      float kv[16], dot = 0.f, k2 = 0.f;
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * q4 + e;
          kv[r] = (float)sKT[(4 * lh + 8 * q4 + e) * VTS + jk];
          dk[r] = a.scale * (dk[r] + k1[r]);
          dot = fmaf(kv[r], dk[r], dot);
          k2 = fmaf(kv[r], kv[r], k2);
        }
      }
      dot += __shfl_xor(dot, 32);
      k2 += __shfl_xor(k2, 32);
      dot -= a.scale * (sCorrK[0][jk] + sCorrK[1][jk]);   // clamped pairs (both query tiles): no projection term
      const float pr = dot * rcp(fmaxf(k2, 1e-30f));
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        bf16x4 o4, o5;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o4[e] = (bf16_t)(dk[4 * q4 + e] - pr * kv[4 * q4 + e]);
          o5[e] = (bf16_t)(dv[4 * q4 + e] + v1[4 * q4 + e]);
        }
        *reinterpret_cast<bf16x4*>(drow + 8 * q4) = o4;
        *reinterpret_cast<bf16x4*>(drow + a.C + 8 * q4) = o5;
      }
    }
  }
  // The sums leave through the staging tile as whole rows (a lane's own 16 elements are 4-byte pieces of 32 different rows:
  // written directly they were 2048 partial-sector writes per wave and table)
  float* part = a.partial + ((size_t)blockIdx.x * 2 * a.heads + h) * N * N;   // [row][2][heads][N][N]
  const size_t tau_off = (size_t)a.heads * N * N;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    __syncthreads();   // the last window's readers of sPW (t = 0) / the row stores of t = 0 are done
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const float tis = reinterpret_cast<const float*>(&sTabL[0][r >> 2][tid])[r & 3];
      // d/dtau of c / clip(tau, 0.01): -sum(dS c) / tau^2 where the clip is not active, else 0
      stage[iq * ANS + j] = t == 0 ? accb2[r >> 1][r & 1] : (tis > 0.f ? -acct2[r >> 1][r & 1] * tis * tis : 0.f);
    }
    __syncthreads();
    for (int r = w; r < N; r += 4)
      if (lane < N && !(UZ_KFLAGS(a) & 0x20000)) part[(t ? tau_off : 0) + r * N + lane] = stage[r * ANS + lane];
  }
}

// bf16 forward, block-per-wave form (the decomposition of winattn_bwd_mfma_kernel): one workgroup per
// (window, head), wave w owns the 32 x 32 score block (query tile qt = w >> 1, key tile kt = w & 1) with
// column = query.  The two waves of a query tile exchange their row maxima, then their row sums and partial
// P V products, through LDS.  Three workgroups fit a CU (a first version with one wave per (window, head) fit one).
__global__ __launch_bounds__(256) void winattn_fwd_mfma2_kernel(const AttnArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t sVT[AD * VTS];
  __shared__ float sRedO[2][64 * 17];   // P V hand-over of the kt = 1 waves, [lane][16] (+1 pad)
  __shared__ float sM[2][AN], sL[2][AN];
  __shared__ __attribute__((aligned(16))) float sRk[AN];
  __shared__ __attribute__((aligned(16))) int sCnt[AN];
  // 1 / clip(tau) and bias of this head (padding: bias = -1e30) in lane order, as in winattn_bwd_mfma_kernel: [table][key group
  // of four][thread] -> the lane's own four values in one conflict-free 16-byte read
  __shared__ float4 sTabL[2][4][256];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, l31 = lane & 31, lh = lane >> 5, h = blockIdx.y;
  const int qt = w >> 1, kt = w & 1;
  const int N = a.ws * a.ws;
  const int nWin = a.B * (a.H / a.ws) * (a.W / a.ws);
  const bool masked = a.shift > 0;
  const bf16_t* __restrict__ qkv = static_cast<const bf16_t*>(a.qkv);
  bf16_t* __restrict__ out = static_cast<bf16_t*>(a.out);
  const int iq = 32 * qt + l31, jk = 32 * kt + l31;   // this lane's query (column role) / key (column role)
  {
    // coalesced rows from global memory (all 32 loads of a thread in flight at once) into a [query][key] staging tile -- the
    // P V hand-over area, not yet in use --, then each lane gathers its own 16 entries
    float* stage = &sRedO[0][0];   // 32 query rows at a time
    static_assert(32 * ANS <= 2 * 64 * 17, "half the staging tile must fit in sRedO");
    float tv[16], bv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int e = tid + 256 * i, r = e >> 6, c = e & 63;
      const bool in = r < N && c < N;
      // unconditional loads (entry (0, 0) for a lane outside the window, then a select): as `in ? table[...] : pad` every
      // load was waited for before the next was issued
      tv[i] = a.tau[in ? ((size_t)h * a.Nt + r) * a.Nt + c : 0];
      bv[i] = a.bias[in ? ((size_t)h * N + r) * N + c : 0];
    }
    // (the loaded values are made opaque before the selects: a value that is only used when `in` holds is otherwise turned back
    // into a load under a branch)
#pragma unroll
    for (int i = 0; i < 16; ++i) asm volatile("" : "+v"(tv[i]), "+v"(bv[i]));
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int e = tid + 256 * i, r = e >> 6, c = e & 63;
      const bool in = r < N && c < N;
      tv[i] = in ? tv[i] : 1.f;
      bv[i] = in ? bv[i] : -1e30f;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int i = 8 * half; i < 8 * half + 8; ++i) {   // rows 32 half .. 32 half + 31
          const int e = tid + 256 * i, r = (e >> 6) - 32 * half, c = e & 63;
          stage[r * ANS + c] = t == 0 ? 1.f / fmaxf(tv[i], 0.01f) : bv[i];
        }
        __syncthreads();
        if (qt == half) {
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            const float* sp = stage + l31 * ANS + 32 * kt + 8 * g4 + 4 * lh;
            sTabL[t][g4][tid] = make_float4(sp[0], sp[1], sp[2], sp[3]);
          }
        }
        __syncthreads();
      }
    }
  }

  WinTok ntq = {0, -1}, ntk = {0, -1};
  bf16x8 nq[2], nk[2], nv[2];
  // The next window's operands, requested while this one is computed.  UNCONDITIONAL loads: a lane beyond the window (7 x 7
  // windows) reads token 0 of its window and is zeroed by a select -- as loads under `if (iq < N)` each group was closed by
  // s_waitcnt vmcnt(0) (hipcc 7.2) and the prefetch waited for its own data in the middle of the current window.
  auto fetch = [&](int win) {
    const bool qin = iq < N, kin = jk < N;
    const WinTok tq0 = win_token(a, win, qin ? iq : 0), tk0 = win_token(a, win, kin ? jk : 0);
    const bf16_t* rowq = qkv + (size_t)tq0.tok * a.ldq + h * AD + 8 * lh;
    const bf16_t* rowk = qkv + (size_t)tk0.tok * a.ldq + a.C + h * AD + 8 * lh;
    // the RAW loaded registers are kept; lanes beyond the window are zeroed where the registers are consumed, one window
    // later (a select here would wait for the data at once)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      nq[ks] = *reinterpret_cast<const bf16x8*>(rowq + 16 * ks);
      nk[ks] = *reinterpret_cast<const bf16x8*>(rowk + 16 * ks);
      nv[ks] = *reinterpret_cast<const bf16x8*>(rowk + a.C + 16 * ks);
    }
    ntq = qin ? tq0 : WinTok{0, -1};
    ntk = kin ? tk0 : WinTok{0, -1};
  };
  const bool qin = iq < N, kin = jk < N;
  bf16x8 zero8;
#pragma unroll
  for (int e = 0; e < 8; ++e) zero8[e] = (bf16_t)0.f;
  if ((int)blockIdx.x < nWin) fetch(blockIdx.x);

  for (int win = blockIdx.x; win < nWin; win += gridDim.x) {
    lds_barrier();   // previous window's readers are done (and sTab has landed)
    const WinTok tq = ntq, tkk = ntk;
    bf16x8 qf[2], kf[2];
    float rq;
    {
      float q2 = 0.f, k2 = 0.f;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        qf[ks] = qin ? nq[ks] : zero8;
        kf[ks] = kin ? nk[ks] : zero8;
        const bf16x2* qp = reinterpret_cast<const bf16x2*>(&qf[ks]);
        const bf16x2* kp = reinterpret_cast<const bf16x2*>(&kf[ks]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {   // v_dot2c_f32_bf16
          q2 = __builtin_amdgcn_fdot2_f32_bf16(qp[e], qp[e], q2, false);
          k2 = __builtin_amdgcn_fdot2_f32_bf16(kp[e], kp[e], k2, false);
        }
      }
      q2 += __shfl_xor(q2, 32);
      k2 += __shfl_xor(k2, 32);
      rq = rcp(a.scale * sqrtf(q2));   // inf for a zero row: the product below is clamped
      if (qt == 0) {
        if (lh == 0) {
          sRk[jk] = rcp(sqrtf(k2));
          sCnt[jk] = tkk.cnt;
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int e = 0; e < 8; ++e) sVT[(16 * ks + 8 * lh + e) * VTS + jk] = kin ? nv[ks][e] : (bf16_t)0.f;
      }
    }
    lds_barrier();
    f32x16 ut;
#pragma unroll
    for (int r = 0; r < 16; ++r) ut[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) ut = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], ut, 0, 0, 0);
    {   // (unconditionally: the last window of a workgroup fetches itself again rather than putting the loads under a branch)
      const int nxt = win + (int)gridDim.x;
      fetch(nxt < nWin ? nxt : win);
    }
    float sv[16], mx = -3.0e38f;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {   // key group of four: one 16-byte read per operand, 16 independent element chains
      const float4 kq = *reinterpret_cast<const float4*>(&sRk[32 * kt + 8 * g4 + 4 * lh]);
      const float4 t = sTabL[0][g4][tid], b = sTabL[1][g4][tid];
      const float rk4[4] = {kq.x, kq.y, kq.z, kq.w}, ti4[4] = {t.x, t.y, t.z, t.w}, bi4[4] = {b.x, b.y, b.z, b.w};
      float pen4[4] = {0.f, 0.f, 0.f, 0.f};
      if (masked) {
        const int4 c4 = *reinterpret_cast<const int4*>(&sCnt[32 * kt + 8 * g4 + 4 * lh]);
        pen4[0] = c4.x != tq.cnt ? -100.f : 0.f;
        pen4[1] = c4.y != tq.cnt ? -100.f : 0.f;
        pen4[2] = c4.z != tq.cnt ? -100.f : 0.f;
        pen4[3] = c4.w != tq.cnt ? -100.f : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * g4 + e;
        const float rden = fminf(rq * rk4[e], 1e6f);      // 1 / max(|scale q||k|, 1e-6)
        const float v = fmaf(ut[r] * a.scale * rden, ti4[e], bi4[e]) + pen4[e];
        sv[r] = v;
        mx = fmaxf(mx, v);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    if (lh == 0) sM[kt][iq] = mx;
    lds_barrier();
    const float m = fmaxf(sM[0][iq], sM[1][iq]);
    float ls = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      sv[r] = __expf(sv[r] - m);
      ls += sv[r];
    }
    ls += __shfl_xor(ls, 32);
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
      o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tfrag(sVT, l31, lh, kt, s2), pack8(sv + 8 * s2), o, 0, 0, 0);
    if (kt == 1) {
      float* red = &sRedO[qt][lane * 17];
#pragma unroll
      for (int r = 0; r < 16; ++r) red[r] = o[r];
      if (lh == 0) sL[qt][l31] = ls;
    }
    lds_barrier();
    if (kt == 0 && iq < N) {
      const float* r1 = &sRedO[qt][lane * 17];
      const float l = ls + sL[qt][l31];
      const float inv = rcp(l);
      bf16_t* orow = out + (size_t)tq.tok * a.ldo + h * AD + 4 * lh;
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        bf16x4 o4;
#pragma unroll
        for (int e = 0; e < 4; ++e) o4[e] = (bf16_t)((o[4 * q4 + e] + r1[4 * q4 + e]) * inv);
        *reinterpret_cast<bf16x4*>(orow + 8 * q4) = o4;
      }
      if (lh == 0) a.lse[((size_t)win * a.heads + h) * N + iq] = m + __logf(l);
    }
  }
}

// Backward: one 256-thread workgroup (one wave per SIMD) per (window, head).  Phase A: lane = query i, the
// four waves split the key range; phase B: lane = key j, the waves split the query range; per-wave
// partial sums of dq / dk / dv meet in LDS and are added in a fixed order.  dS-derived sums for d(bias)
// and d(tau) accumulate over the workgroup's windows in LDS (wave w owns its key columns).
template <typename T>
__global__ __launch_bounds__(256) void winattn_bwd_kernel(const AttnArgs a) {
  constexpr int TILE = AN * ARS, MAT = AN * ANS;
  __shared__ float smem[2 * TILE + 2 * MAT + 4 * TILE + 2 * MAT + 3 * AN];
  __shared__ int sCnt[AN];
  float* const sK = smem;                 // phase A: K rows; phase B: Q rows
  float* const sV = smem + TILE;          // phase A: V rows; phase B: dO rows
  float* const sP = smem + 2 * TILE;
  float* const sDC = sP + MAT;
  float* const sRA = sDC + MAT;           // [4][AN][ARS]: per-wave partial (dq vector part, scalar part)
  float* const sDB = sRA + 4 * TILE;
  float* const sDT = sDB + MAT;
  float* const sKn = sDT + MAT;
  float* const sQn = sKn + AN;
  float* const sPB = smem;                // [4][AN][ANS] partial (dk, dv, scalar), aliases sK .. sRA after phase B
  static_assert(4 * MAT <= 2 * TILE + 2 * MAT + 4 * TILE, "phase B partials must fit the aliased region");
  const int tid = threadIdx.x, w = tid >> 6, i = tid & 63, h = blockIdx.y;
  const int N = a.ws * a.ws;
  const int jc = (N + 3) >> 2, lo = w * jc, hi = min(N, lo + jc);
  const int nWin = a.B * (a.H / a.ws) * (a.W / a.ws);
  const T* __restrict__ qkv = static_cast<const T*>(a.qkv);
  const T* __restrict__ out = static_cast<const T*>(a.out);
  const T* __restrict__ dout = static_cast<const T*>(a.dout);
  T* __restrict__ dqkv = static_cast<T*>(a.dqkv);
  for (int e = tid; e < MAT; e += 256) sDB[e] = sDT[e] = 0.f;
  for (int win = blockIdx.x; win < nWin; win += gridDim.x) {
    __syncthreads();
    float q[AD], kk[AD], go[AD];
    float qn = 0.f, kn = 0.f, Di = 0.f, rqn = 0.f, rkn = 0.f;
    WinTok me = {0, 0};
    if (i < N) {
      me = win_token(a, win, i);
      const T* row = qkv + (size_t)me.tok * a.ldq + h * AD;
      float t[AD];
      load_head(row, q);
      load_head(row + a.C, kk);
      load_head(dout + (size_t)me.tok * a.lddo + h * AD, go);
      load_head(out + (size_t)me.tok * a.ldo + h * AD, t);
#pragma unroll
      for (int e = 0; e < AD; ++e) {
        q[e] *= a.scale;
        qn += q[e] * q[e];
        kn += kk[e] * kk[e];
        Di = fmaf(go[e], t[e], Di);
      }
      qn = sqrtf(qn);
      kn = sqrtf(kn);
      rqn = rcp(qn);
      rkn = rcp(kn);
      if (w == 0) {
        load_head(row + 2 * a.C, t);
#pragma unroll
        for (int e = 0; e < AD; ++e) {
          sK[i * ARS + e] = kk[e];
          sV[i * ARS + e] = t[e];
        }
        sKn[i] = kn;
        sQn[i] = qn;
        sCnt[i] = me.cnt;
      }
    }
    __syncthreads();
    {  // ---- phase A: query i, keys [lo, hi)
      float av[AD], bs = 0.f;
#pragma unroll
      for (int e = 0; e < AD; ++e) av[e] = 0.f;
      if (i < N) {
        const float lse = a.lse[((size_t)win * a.heads + h) * N + i];
        for (int j = lo; j < hi; ++j) {
          float krow[AD], vrow[AD];
          lds_row(sK + j * ARS, krow);
          lds_row(sV + j * ARS, vrow);
          const float u = dot32(q, krow), dp = dot32(go, vrow);
          const float nn = qn * sKn[j];
          const bool clamped = nn <= 1e-6f;
          const float den = clamped ? 1e-6f : nn;
          const float tv = a.tau[((size_t)h * a.Nt + i) * a.Nt + j];
          const float ti = rcp(fmaxf(tv, 0.01f));
          const float rden = rcp(den);
          const float c = u * rden;
          float s = c * ti + a.bias[((size_t)h * N + i) * N + j];
          if (sCnt[j] != me.cnt) s -= 100.f;
          const float p = __expf(s - lse);
          const float ds = p * (dp - Di);
          sP[i * ANS + j] = p;
          sDB[i * ANS + j] += ds;
          if (tv >= 0.01f) sDT[i * ANS + j] -= ds * c * ti * ti;
          const float dc = ds * ti;
          sDC[i * ANS + j] = dc;
          const float w1 = dc * rden;
          axpy32(w1, krow, av);
          if (!clamped) bs += dc * u * sKn[j] * rden * rden * rqn;  // d(den)/d(qs_i) = kn_j * qs_i / n_i
        }
      }
      float* ra = sRA + (w * AN + i) * ARS;
#pragma unroll
      for (int e = 0; e < AD; ++e) ra[e] = av[e];
      ra[AD] = bs;
    }
    __syncthreads();
    if (i < N) {  // dq: wave w finishes components [8w, 8w + 8) of query i; wave 0 re-stages Q and dO
      float tot[8], bt = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) tot[e] = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float* ra = sRA + (k * AN + i) * ARS;
        bt += ra[AD];
#pragma unroll
        for (int e = 0; e < 8; ++e) tot[e] += ra[8 * w + e];
      }
      float dq[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float qe = 0.f;  // q[8 w + e] without dynamic register indexing
#pragma unroll
        for (int k = 0; k < 4; ++k) qe = (w == k) ? q[8 * k + e] : qe;
        dq[e] = a.scale * (tot[e] - bt * qe);
      }
      store8(dqkv + (size_t)me.tok * a.lddq + h * AD + 8 * w, dq);
      if (w == 0) {
#pragma unroll
        for (int e = 0; e < AD; ++e) {
          sK[i * ARS + e] = q[e];
          sV[i * ARS + e] = go[e];
        }
      }
    }
    __syncthreads();
    float dk[AD], dv[AD], bsk = 0.f;
#pragma unroll
    for (int e = 0; e < AD; ++e) dk[e] = dv[e] = 0.f;
    if (i < N) {  // ---- phase B: key j = i, queries [lo, hi)
      const int j = i;
      for (int r = lo; r < hi; ++r) {
        const float p = sP[r * ANS + j], dc = sDC[r * ANS + j];
        float qrow[AD], grow[AD];
        lds_row(sK + r * ARS, qrow);
        lds_row(sV + r * ARS, grow);
        const float u = dot32(qrow, kk);
        axpy32(p, grow, dv);
        const float nn = sQn[r] * kn;
        const bool clamped = nn <= 1e-6f;
        const float den = clamped ? 1e-6f : nn;
        const float rden = rcp(den);
        const float w1 = dc * rden;
        axpy32(w1, qrow, dk);
        if (!clamped) bsk += dc * u * sQn[r] * rden * rden * rkn;
      }
    }
    __syncthreads();  // everyone is done with sP / sDC / the Q, dO tiles: the partials may overwrite them
    {
      float* pb = sPB + (w * AN + i) * ANS;
#pragma unroll
      for (int e = 0; e < AD; ++e) {
        pb[e] = dk[e];
        pb[AD + e] = dv[e];
      }
      pb[2 * AD] = bsk;
    }
    __syncthreads();
    if (i < N) {  // waves 0, 1: halves of dk; waves 2, 3: halves of dv
      float tot[16], bt = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) tot[e] = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float* pb = sPB + (k * AN + i) * ANS;
        bt += pb[2 * AD];
#pragma unroll
        for (int e = 0; e < 16; ++e) tot[e] += pb[16 * w + e];
      }
      if (w < 2) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float ke = (w == 0) ? kk[e] : kk[16 + e];
          tot[e] -= bt * ke;
        }
      }
      T* row = dqkv + (size_t)me.tok * a.lddq + h * AD + (w < 2 ? a.C + 16 * w : 2 * a.C + 16 * (w - 2));
      store8(row, tot);
      store8(row + 8, tot + 8);
    }
  }
  __syncthreads();
  float* part = a.partial + ((size_t)blockIdx.x * 2 * a.heads + h) * N * N;   // [row][2][heads][N][N]
  const size_t tau_off = (size_t)a.heads * N * N;
  for (int e = tid; e < N * N; e += 256) {
    const int r = e / N, c = e - r * N;
    part[e] = sDB[r * ANS + c];
    part[tau_off + e] = sDT[r * ANS + c];
  }
}
// (Measured and rejected: keeping the tau / bias values and the d(bias) / d(tau) sums of a lane's 16 keys in
// registers with the key loop fully unrolled — 15 % slower, the unrolled body no longer fits the
// instruction cache; recomputing P in phase B to halve LDS and double the occupancy — 26 % slower.)

// ---------------------------------------------------------------------------------------------
// Windows of 65 .. 256 tokens (window_size 9 .. 16).
// The kernels above hold a whole window in one 64-row tile; here a window is walked in 32 x 32 tiles of
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
// ---------------------------------------------------------------------------------------------
constexpr int WD = 32;             // head dimension
constexpr int WN = UZ_WIDE_MAXN;   // tokens per window at most
constexpr int WTS = 260;           // row stride of the transposed LDS tiles [32 d][WN tokens] in elements: rows stay
                                   // 8-byte (bf16) / 16-byte (fp32) aligned and 32 rows spread over the banks
constexpr float NEG = -1e30f;      // "minus infinity" that stays finite under subtraction

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
          float s = st[r] * a.scale * rcp(fmaxf(qn * sKn[j], 1e-6f)) * rcp(fmaxf(tv[r], 0.01f)) + bv[r];
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
  const float rden = rcp(clamped ? 1e-6f : nn);
  const float ti = rcp(fmaxf(tv, 0.01f));
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
      bs *= rcp(qn);
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
      bsk *= rcp(kn);
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

// ---------------------------------------------------------------------------------------------
// Continuous position bias: bias[h][r] = b2[h] + sum_k w2[h][k] relu(w1[k][0] x0(r) + w1[k][1] x1(r) + b1[k])
// over the R = N*N log-spaced offsets (get_continuous_relative_position_bias, swin_unet_v2.py:121-125 with
// Mlp_Relu :58-72).  A function of parameters only; hidden = 256, heads <= 32, any R (4096 at window 8, 65 536 at window 16).
// ---------------------------------------------------------------------------------------------
constexpr int CPB_MAXH = 32;
constexpr int CPB_MAXHID = 512;

// grid (R / 256, heads): one thread per (offset r, head h); fc1 and this head's fc2 row sit in LDS
__global__ __launch_bounds__(256) void cpb_fwd_kernel(const float* __restrict__ idx, const float* __restrict__ w1,
                                                      const float* __restrict__ b1, const float* __restrict__ w2,
                                                      const float* __restrict__ b2, int R, int hidden, int heads,
                                                      float* __restrict__ bias) {
  __shared__ float4 sW[CPB_MAXHID];  // (w1[k][0], w1[k][1], b1[k], w2[h][k])
  const int h = blockIdx.y;
  for (int k = threadIdx.x; k < hidden; k += 256)
    sW[k] = make_float4(w1[2 * k], w1[2 * k + 1], b1[k], w2[h * hidden + k]);
  __syncthreads();
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const float x0 = idx[2 * r], x1 = idx[2 * r + 1];
  float acc = b2[h];
#pragma unroll 8
  for (int k = 0; k < hidden; ++k) {
    const float4 wv = sW[k];
    acc = fmaf(wv.w, fmaxf(fmaf(wv.x, x0, fmaf(wv.y, x1, wv.z)), 0.f), acc);
  }
  bias[(size_t)h * R + r] = acc;
}

// one 1024-thread workgroup per hidden unit (the kernel is bound by the latency of the few G / idx loads each
// thread issues, so the rows are spread over 16 waves).  Sums over the R rows in a fixed order: per-thread
// strided sums, xor-shuffle within a wave, then the sixteen waves in order.
constexpr int CPB_KB = 1;
constexpr int CPB_NW = 16;

__global__ __launch_bounds__(1024) void cpb_bwd_kernel(const float* __restrict__ idx, const float* __restrict__ w1,
                                                      const float* __restrict__ b1, const float* __restrict__ w2,
                                                      const float* __restrict__ G, int R, int hidden, int heads,
                                                      float* __restrict__ dw1, float* __restrict__ db1,
                                                      float* __restrict__ dw2, float* __restrict__ db2) {
  __shared__ float red[CPB_NW][CPB_KB * (CPB_MAXH + 3) + CPB_MAXH];
  const int k0 = blockIdx.x * CPB_KB, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  float wa[CPB_KB], wb[CPB_KB], bk[CPB_KB];
#pragma unroll
  for (int q = 0; q < CPB_KB; ++q) {
    const int k = min(k0 + q, hidden - 1);
    wa[q] = w1[2 * k];
    wb[q] = w1[2 * k + 1];
    bk[q] = b1[k];
  }
  float a2[CPB_KB][CPB_MAXH], g2[CPB_MAXH], a10[CPB_KB], a11[CPB_KB], ab[CPB_KB];
#pragma unroll
  for (int q = 0; q < CPB_KB; ++q) {
    a10[q] = a11[q] = ab[q] = 0.f;
#pragma unroll
    for (int h = 0; h < CPB_MAXH; ++h) a2[q][h] = 0.f;
  }
#pragma unroll
  for (int h = 0; h < CPB_MAXH; ++h) g2[h] = 0.f;
  for (int r = t; r < R; r += 64 * CPB_NW) {
    const float x0 = idx[2 * r], x1 = idx[2 * r + 1];
    float pre[CPB_KB], hv[CPB_KB], gs[CPB_KB];
#pragma unroll
    for (int q = 0; q < CPB_KB; ++q) {
      pre[q] = fmaf(wa[q], x0, fmaf(wb[q], x1, bk[q]));
      hv[q] = fmaxf(pre[q], 0.f);
      gs[q] = 0.f;
    }
#pragma unroll
    for (int h = 0; h < CPB_MAXH; ++h)
      if (h < heads) {
        const float g = G[(size_t)h * R + r];
        g2[h] += g;
#pragma unroll
        for (int q = 0; q < CPB_KB; ++q) {
          gs[q] = fmaf(g, w2[h * hidden + min(k0 + q, hidden - 1)], gs[q]);
          a2[q][h] = fmaf(g, hv[q], a2[q][h]);
        }
      }
#pragma unroll
    for (int q = 0; q < CPB_KB; ++q) {
      const float dl = pre[q] > 0.f ? gs[q] : 0.f;
      a10[q] = fmaf(dl, x0, a10[q]);
      a11[q] = fmaf(dl, x1, a11[q]);
      ab[q] += dl;
    }
  }
  auto wsum = [](float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
  };
  constexpr int PERK = CPB_MAXH + 3;
#pragma unroll
  for (int q = 0; q < CPB_KB; ++q) {
    const float s0 = wsum(a10[q]), s1 = wsum(a11[q]), s2 = wsum(ab[q]);
    if (lane == 0) {
      red[wv][q * PERK] = s0;
      red[wv][q * PERK + 1] = s1;
      red[wv][q * PERK + 2] = s2;
    }
#pragma unroll
    for (int h = 0; h < CPB_MAXH; ++h)
      if (h < heads) {
        const float v = wsum(a2[q][h]);
        if (lane == 0) red[wv][q * PERK + 3 + h] = v;
      }
  }
  if (blockIdx.x == 0) {
#pragma unroll
    for (int h = 0; h < CPB_MAXH; ++h)
      if (h < heads) {
        const float v = wsum(g2[h]);
        if (lane == 0) red[wv][CPB_KB * PERK + h] = v;
      }
  }
  __syncthreads();
  if (t < CPB_KB * PERK + CPB_MAXH) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < CPB_NW; ++k) v += red[k][t];
    if (t < CPB_KB * PERK) {
      const int q = t / PERK, e = t - q * PERK, k = k0 + q;
      if (k < hidden) {
        if (e == 0) dw1[2 * k] = v;
        else if (e == 1) dw1[2 * k + 1] = v;
        else if (e == 2) db1[k] = v;
        else if (e - 3 < heads) dw2[(e - 3) * hidden + k] = v;
      }
    } else if (blockIdx.x == 0 && t - CPB_KB * PERK < heads) {
      db2[t - CPB_KB * PERK] = v;
    }
  }
}

// ---- all position-bias MLPs of a model in one launch ------------------------------------------------
// The MLPs are tiny (R <= 4096 offsets up to window 8, 65 536 at window 16; 256 hidden units, <= 32 heads) and a function of parameters only, so
// a model's 14 of them are evaluated together at the start of the forward and differentiated together at the
// end of the backward: 2 + 1 launches instead of 28, and the backward reads each G once (cpb_bwd_kernel above
// re-reads it per hidden unit: 22 us per module, bound by L2).
constexpr int CPB_MAXB = 24;     // modules per launch (the descriptor array travels in the kernel arguments)
constexpr int CPB_ROWS = 128;    // offsets per workgroup of the batched backward
struct CpbBatch {
  uz_cpb_item it[CPB_MAXB];
  long long off[CPB_MAXB];       // float offset of the module's partial sums in the workspace
};

__global__ __launch_bounds__(256) void cpb_fwd_batched_kernel(const CpbBatch b) {
  __shared__ float4 sW[CPB_MAXHID];  // (w1[k][0], w1[k][1], b1[k], w2[h][k])
  const uz_cpb_item& m = b.it[blockIdx.z];
  const int h = blockIdx.y, R = m.R, hidden = m.hidden;
  if (h >= m.heads || (int)(blockIdx.x * 256) >= R) return;   // whole workgroups
  for (int k = threadIdx.x; k < hidden; k += 256)
    sW[k] = make_float4(m.w1[2 * k], m.w1[2 * k + 1], m.b1[k], m.w2[h * hidden + k]);
  __syncthreads();
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  const float x0 = m.idx[2 * r], x1 = m.idx[2 * r + 1];
  float acc = m.b2[h];
#pragma unroll 8
  for (int k = 0; k < hidden; ++k) {
    const float4 wv = sW[k];
    acc = fmaf(wv.w, fmaxf(fmaf(wv.x, x0, fmaf(wv.y, x1, wv.z)), 0.f), acc);
  }
  m.bias[(size_t)h * R + r] = acc;
}

// grid (row blocks, modules), 512 threads: thread = hidden unit k (512 / hidden groups split the block's rows).
// Partial sums per (row block, group): [(heads + 3)][hidden] = d w2[h][k] (heads), d w1[k][0], d w1[k][1], d b1[k];
// per row block: [heads] sums of G (d b2).  cpb_bwd_finalize_kernel adds them in a fixed order.
__global__ __launch_bounds__(512) void cpb_bwd_batched_kernel(const CpbBatch b, float* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float sG[CPB_ROWS][CPB_MAXH];
  __shared__ float sX[CPB_ROWS][2];
  const uz_cpb_item& m = b.it[blockIdx.y];
  const int R = m.R, hidden = m.hidden, heads = m.heads, tid = threadIdx.x;
  const int r0 = blockIdx.x * CPB_ROWS;
  if (r0 >= R) return;
  const int hp = (heads + 3) & ~3;
  for (int e = tid; e < CPB_ROWS * hp; e += 512) {
    const int h = e / CPB_ROWS, r = e - h * CPB_ROWS;
    sG[r][h] = (h < heads && r0 + r < R) ? m.G[(size_t)h * R + r0 + r] : 0.f;
  }
  for (int e = tid; e < CPB_ROWS; e += 512) {
    const bool in = r0 + e < R;
    sX[e][0] = in ? m.idx[2 * (r0 + e)] : 0.f;
    sX[e][1] = in ? m.idx[2 * (r0 + e) + 1] : 0.f;
  }
  __syncthreads();
  const int nsub = 512 / hidden, RB = (R + CPB_ROWS - 1) / CPB_ROWS;
  const int nmain = (heads + 3) * hidden;
  float* main_ws = ws + b.off[blockIdx.y];
  if (tid < heads) {   // d b2 partial of this row block
    float t = 0.f;
    for (int r = 0; r < CPB_ROWS; ++r) t += sG[r][tid];
    main_ws[(size_t)RB * nsub * nmain + (size_t)blockIdx.x * heads + tid] = t;
  }
  const int sub = tid / hidden, k = tid - sub * hidden;
  if (sub >= nsub) return;
  const int rows_per = CPB_ROWS / nsub + (CPB_ROWS % nsub != 0);
  const int rb = sub * rows_per, re = min(rb + rows_per, CPB_ROWS);
  const float wa = m.w1[2 * k], wb = m.w1[2 * k + 1], bk = m.b1[k];
  float w2c[CPB_MAXH], a2[CPB_MAXH];
#pragma unroll
  for (int h = 0; h < CPB_MAXH; ++h) {
    w2c[h] = h < heads ? m.w2[h * hidden + k] : 0.f;
    a2[h] = 0.f;
  }
  float a10 = 0.f, a11 = 0.f, ab = 0.f;
  for (int r = rb; r < re; ++r) {
    const float x0 = sX[r][0], x1 = sX[r][1];
    const float pre = fmaf(wa, x0, fmaf(wb, x1, bk));
    const float hv = fmaxf(pre, 0.f);
    float gs = 0.f;
#pragma unroll
    for (int h4 = 0; h4 < CPB_MAXH / 4; ++h4)
      if (4 * h4 < hp) {
        const float4 g = *reinterpret_cast<const float4*>(&sG[r][4 * h4]);
        gs = fmaf(g.x, w2c[4 * h4], gs);
        gs = fmaf(g.y, w2c[4 * h4 + 1], gs);
        gs = fmaf(g.z, w2c[4 * h4 + 2], gs);
        gs = fmaf(g.w, w2c[4 * h4 + 3], gs);
        a2[4 * h4] = fmaf(g.x, hv, a2[4 * h4]);
        a2[4 * h4 + 1] = fmaf(g.y, hv, a2[4 * h4 + 1]);
        a2[4 * h4 + 2] = fmaf(g.z, hv, a2[4 * h4 + 2]);
        a2[4 * h4 + 3] = fmaf(g.w, hv, a2[4 * h4 + 3]);
      }
    const float dl = pre > 0.f ? gs : 0.f;
    a10 = fmaf(dl, x0, a10);
    a11 = fmaf(dl, x1, a11);
    ab += dl;
  }
  float* row = main_ws + ((size_t)blockIdx.x * nsub + sub) * nmain;
#pragma unroll
  for (int h = 0; h < CPB_MAXH; ++h)
    if (h < heads) row[h * hidden + k] = a2[h];
  row[heads * hidden + k] = a10;
  row[(heads + 1) * hidden + k] = a11;
  row[(heads + 2) * hidden + k] = ab;
}

__global__ __launch_bounds__(256) void cpb_bwd_finalize_kernel(const CpbBatch b, const float* __restrict__ ws) {
  const uz_cpb_item& m = b.it[blockIdx.y];
  const int hidden = m.hidden, heads = m.heads;
  const int nsub = 512 / hidden, RB = (m.R + CPB_ROWS - 1) / CPB_ROWS, rows = RB * nsub;
  const int nmain = (heads + 3) * hidden;
  const float* main_ws = ws + b.off[blockIdx.y];
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < nmain) {
    float t = 0.f;
    for (int r = 0; r < rows; r += 8) {   // eight rows per trip, unconditional loads, same order of additions
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = main_ws[(size_t)(r + u < rows ? r + u : 0) * nmain + e];
#pragma unroll
      for (int u = 0; u < 8; ++u) asm volatile("" : "+v"(v[u]));
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (r + u < rows) t += v[u];
    }
    const int j = e / hidden, k = e - j * hidden;
    if (j < heads) m.dw2[j * hidden + k] = t;
    else if (j == heads) m.dw1[2 * k] = t;
    else if (j == heads + 1) m.dw1[2 * k + 1] = t;
    else m.db1[k] = t;
  } else if (e - nmain < heads) {
    const float* tail = main_ws + (size_t)rows * nmain;
    float t = 0.f;
    for (int r = 0; r < RB; ++r) t += tail[(size_t)r * heads + (e - nmain)];
    m.db2[e - nmain] = t;
  }
}

}  // namespace

static int attn_check(const char* fn, const uz_winattn_desc* d) {
  UZ_REQUIRE(d != nullptr, "%s: null descriptor", fn);
  UZ_REQUIRE(d->dtype == UZ_F32 || d->dtype == UZ_BF16, "%s: bad dtype", fn);
  UZ_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->heads > 0 && d->C == d->heads * AD,
             "%s: needs head_dim 32 (C=%d, heads=%d)", fn, d->C, d->heads);
  UZ_REQUIRE(d->ws >= 1 && d->ws * d->ws <= UZ_WIDE_MAXN && d->H % d->ws == 0 && d->W % d->ws == 0,
             "%s: window %d does not tile %dx%d (or exceeds 16x16)", fn, d->ws, d->H, d->W);
  UZ_REQUIRE(d->shift >= 0 && d->shift < d->ws && d->Nt >= d->ws * d->ws, "%s: bad shift / tau size", fn);
  const int vec = d->dtype == UZ_BF16 ? 8 : 4;
  UZ_REQUIRE(d->ldq % vec == 0 && d->ldq >= 3 * d->C && d->ldo % vec == 0 && d->ldo >= d->C, "%s: bad strides", fn);
  UZ_REQUIRE((long long)d->B * d->H * d->W < (1LL << 31), "%s: too many tokens", fn);
  return UZ_OK;
}

// Workgroups of the window-attention kernels stay resident for the whole launch (each walks its share of the
// windows of one head), so the grid must FIT: one workgroup more than the chip holds doubles the run time.
// slots = resident workgroups per CU of the kernel; windows are dealt evenly (per-workgroup count first).
static int attn_grid_x(const uz_winattn_desc* d, int slots_per_cu) {
  const long long units_x = (long long)d->B * (d->H / d->ws) * (d->W / d->ws);
  const char* e = uz_ablate_env("UZ_ATTN_GX");   // measurement hook (tools/attn_bench.py)
  if (e && atoi(e) > 0) return (int)(atoi(e) < units_x ? atoi(e) : units_x);
  long long cap = (long long)UZ_NUM_CU * slots_per_cu / d->heads;
  if (cap < 1) cap = 1;
  const long long per = (units_x + cap - 1) / cap;
  const long long g = (units_x + per - 1) / per;
  return (int)(g < 1 ? 1 : g);
}

// The kernel a descriptor runs on, per direction, and its grid: windows of more than AN tokens on the tile-walking
// kernels, narrower ones on the matrix-core kernels in bf16 and on the scalar kernels in fp32.  A function of the
// descriptor and the CU reserve only.
struct AttnPlan {
  void (*kernel)(const AttnArgs);
  int slots, grid_x;
};
static AttnPlan attn_plan(const uz_winattn_desc* d, bool bwd) {
  const bool bf16 = d->dtype == UZ_BF16, wide = d->ws * d->ws > AN;
  AttnPlan p;
  if (wide && bf16)
    p = bwd ? AttnPlan{winattn_wide_bwd_kernel<bf16_t>, UZ_WIDE_SLOTS_BWD_BF16}
            : AttnPlan{winattn_wide_fwd_kernel<bf16_t>, UZ_WIDE_SLOTS_FWD};
  else if (wide)
    p = bwd ? AttnPlan{winattn_wide_bwd_kernel<float>, UZ_WIDE_SLOTS_BWD_F32}
            : AttnPlan{winattn_wide_fwd_kernel<float>, UZ_WIDE_SLOTS_FWD};
  else if (bf16)
    p = bwd ? AttnPlan{winattn_bwd_mfma_kernel, ATTN_SLOTS_BWD_MFMA} : AttnPlan{winattn_fwd_mfma2_kernel, ATTN_SLOTS_FWD_MFMA2};
  else
    p = bwd ? AttnPlan{winattn_bwd_kernel<float>, ATTN_SLOTS_BWD} : AttnPlan{winattn_fwd_kernel<float>, ATTN_SLOTS_FWD};
  p.grid_x = attn_grid_x(d, p.slots);
  if (wide && bwd) {
    // d(bias) / d(tau) rows are [2][heads][N][N] fp32 each (1.5 MiB at N = 256, 3 heads): the grid -- one row per
    // workgroup column -- is capped so that the launch's partial buffer stays within UZ_WIDE_PARTIAL_BYTES
    const long long N = (long long)d->ws * d->ws, row_bytes = 2LL * d->heads * N * N * (long long)sizeof(float);
    const long long cap = UZ_WIDE_PARTIAL_BYTES / row_bytes;
    if (p.grid_x > cap) p.grid_x = (int)(cap < 1 ? 1 : cap);
  }
  return p;
}

static AttnArgs attn_args(const uz_winattn_desc* d, const void* qkv, const float* tau, const float* bias, const void* out,
                          const float* lse) {
  AttnArgs a{};
  a.qkv = qkv; a.out = const_cast<void*>(out); a.lse = const_cast<float*>(lse); a.tau = tau; a.bias = bias;
  a.B = d->B; a.H = d->H; a.W = d->W; a.C = d->C; a.heads = d->heads; a.ws = d->ws; a.shift = d->shift; a.Nt = d->Nt;
  a.ldq = d->ldq; a.ldo = d->ldo; a.scale = d->scale; a.flags = uz_tune_flags();
  return a;
}

extern "C" int uz_winattn_fwd(const uz_winattn_desc* d, const void* qkv, const float* tau, const float* bias,
                              void* out, float* lse, void* stream) {
  const int rc = attn_check("uz_winattn_fwd", d);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(qkv && tau && bias && out && lse, "uz_winattn_fwd: null pointer");
  const AttnArgs a = attn_args(d, qkv, tau, bias, out, lse);
  const AttnPlan p = attn_plan(d, false);
  hipLaunchKernelGGL(p.kernel, dim3(p.grid_x, d->heads), dim3(256), 0, (hipStream_t)stream, a);
  UZ_LAUNCH_CHECK("uz_winattn_fwd");
  return UZ_OK;
}

extern "C" int uz_winattn_bwd_rows(const uz_winattn_desc* d) {
  const int rc = attn_check("uz_winattn_bwd_rows", d);
  if (rc != UZ_OK) return rc;
  return attn_plan(d, true).grid_x;
}

extern "C" int uz_winattn_bwd(const uz_winattn_desc* d, const void* qkv, const float* tau, const float* bias,
                              const void* out, const float* lse, const void* dout, int lddo, void* dqkv, int lddq,
                              float* partial, void* stream) {
  const int rc = attn_check("uz_winattn_bwd", d);
  if (rc != UZ_OK) return rc;
  const int vec = d->dtype == UZ_BF16 ? 8 : 4;
  UZ_REQUIRE(qkv && tau && bias && out && lse && dout && dqkv && partial, "uz_winattn_bwd: null pointer");
  UZ_REQUIRE(lddo % vec == 0 && lddo >= d->C && lddq % vec == 0 && lddq >= 3 * d->C, "uz_winattn_bwd: bad strides");
  AttnArgs a = attn_args(d, qkv, tau, bias, out, lse);
  a.dout = dout; a.dqkv = dqkv; a.partial = partial; a.lddo = lddo; a.lddq = lddq;
  const AttnPlan p = attn_plan(d, true);
  hipLaunchKernelGGL(p.kernel, dim3(p.grid_x, d->heads), dim3(256), 0, (hipStream_t)stream, a);
  UZ_LAUNCH_CHECK("uz_winattn_bwd");
  return UZ_OK;
}


static int cpb_check(const char* fn, int R, int hidden, int heads) {
  UZ_REQUIRE(R > 0 && hidden > 0 && hidden <= CPB_MAXHID && heads > 0 && heads <= CPB_MAXH,
             "%s: bad shape (heads <= %d, hidden <= %d)", fn, CPB_MAXH, CPB_MAXHID);
  return UZ_OK;
}

extern "C" int uz_cpb_fwd(const float* idx, const float* w1, const float* b1, const float* w2, const float* b2, int R,
                          int hidden, int heads, float* bias, void* stream) {
  const int rc = cpb_check("uz_cpb_fwd", R, hidden, heads);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(idx && w1 && b1 && w2 && b2 && bias, "uz_cpb_fwd: null pointer");
  hipLaunchKernelGGL(cpb_fwd_kernel, dim3(uz_cdiv(R, 256), heads), dim3(256), 0, (hipStream_t)stream, idx, w1, b1, w2,
                     b2, R, hidden, heads, bias);
  UZ_LAUNCH_CHECK("uz_cpb_fwd");
  return UZ_OK;
}

extern "C" int uz_cpb_bwd(const float* idx, const float* w1, const float* b1, const float* w2, const float* G, int R,
                          int hidden, int heads, float* dw1, float* db1, float* dw2, float* db2, void* stream) {
  const int rc = cpb_check("uz_cpb_bwd", R, hidden, heads);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(idx && w1 && b1 && w2 && G && dw1 && db1 && dw2 && db2, "uz_cpb_bwd: null pointer");
  hipLaunchKernelGGL(cpb_bwd_kernel, dim3(uz_cdiv(hidden, CPB_KB)), dim3(64 * CPB_NW), 0, (hipStream_t)stream, idx, w1, b1, w2, G,
                     R, hidden, heads, dw1, db1, dw2, db2);
  UZ_LAUNCH_CHECK("uz_cpb_bwd");
  return UZ_OK;
}

static long long cpb_item_ws_floats(const uz_cpb_item* m) {
  const long long nsub = 512 / m->hidden, RB = (m->R + CPB_ROWS - 1) / CPB_ROWS;
  return RB * nsub * (long long)(m->heads + 3) * m->hidden + RB * m->heads;
}

static int cpb_batch_check(const char* fn, const uz_cpb_item* items, int n, bool bwd) {
  UZ_REQUIRE(items != nullptr && n > 0, "%s: empty batch", fn);
  for (int i = 0; i < n; ++i) {
    const uz_cpb_item* m = items + i;
    const int rc = cpb_check(fn, m->R, m->hidden, m->heads);
    if (rc != UZ_OK) return rc;
    UZ_REQUIRE(m->idx && m->w1 && m->b1 && m->w2, "%s: item %d: null pointer", fn, i);
    if (bwd) UZ_REQUIRE(m->G && m->dw1 && m->db1 && m->dw2 && m->db2, "%s: item %d: null gradient pointer", fn, i);
    else UZ_REQUIRE(m->b2 && m->bias, "%s: item %d: null pointer", fn, i);
  }
  return UZ_OK;
}

extern "C" int uz_cpb_fwd_batched(const uz_cpb_item* items, int n, void* stream) {
  const int rc = cpb_batch_check("uz_cpb_fwd_batched", items, n, false);
  if (rc != UZ_OK) return rc;
  for (int i0 = 0; i0 < n; i0 += CPB_MAXB) {
    const int nb = n - i0 < CPB_MAXB ? n - i0 : CPB_MAXB;
    CpbBatch b{};
    int rmax = 0, hmax = 0;
    for (int i = 0; i < nb; ++i) {
      b.it[i] = items[i0 + i];
      rmax = items[i0 + i].R > rmax ? items[i0 + i].R : rmax;
      hmax = items[i0 + i].heads > hmax ? items[i0 + i].heads : hmax;
    }
    hipLaunchKernelGGL(cpb_fwd_batched_kernel, dim3(uz_cdiv(rmax, 256), hmax, nb), dim3(256), 0, (hipStream_t)stream, b);
    UZ_LAUNCH_CHECK("uz_cpb_fwd_batched");
  }
  return UZ_OK;
}

extern "C" long long uz_cpb_bwd_batched_workspace_bytes(const uz_cpb_item* items, int n) {
  UZ_REQUIRE(items != nullptr && n > 0, "uz_cpb_bwd_batched_workspace_bytes: empty batch");
  long long tot = 0;
  for (int i = 0; i < n; ++i) {
    const int rc = cpb_check("uz_cpb_bwd_batched_workspace_bytes", items[i].R, items[i].hidden, items[i].heads);
    if (rc != UZ_OK) return rc;
    tot += cpb_item_ws_floats(items + i);
  }
  return tot * (long long)sizeof(float);
}

extern "C" int uz_cpb_bwd_batched(const uz_cpb_item* items, int n, float* workspace, void* stream) {
  const int rc = cpb_batch_check("uz_cpb_bwd_batched", items, n, true);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(workspace != nullptr, "uz_cpb_bwd_batched: null workspace");
  long long off = 0;
  for (int i0 = 0; i0 < n; i0 += CPB_MAXB) {
    const int nb = n - i0 < CPB_MAXB ? n - i0 : CPB_MAXB;
    CpbBatch b{};
    int rmax = 0, omax = 0;
    for (int i = 0; i < nb; ++i) {
      const uz_cpb_item& m = items[i0 + i];
      b.it[i] = m;
      b.off[i] = off;
      off += cpb_item_ws_floats(&m);
      rmax = m.R > rmax ? m.R : rmax;
      const int outs = (m.heads + 3) * m.hidden + m.heads;
      omax = outs > omax ? outs : omax;
    }
    hipLaunchKernelGGL(cpb_bwd_batched_kernel, dim3(uz_cdiv(rmax, CPB_ROWS), nb), dim3(512), 0, (hipStream_t)stream, b, workspace);
    UZ_LAUNCH_CHECK("uz_cpb_bwd_batched");
    hipLaunchKernelGGL(cpb_bwd_finalize_kernel, dim3(uz_cdiv(omax, 256), nb), dim3(256), 0, (hipStream_t)stream, b,
                       (const float*)workspace);
    UZ_LAUNCH_CHECK("uz_cpb_bwd_batched (finalize)");
  }
  return UZ_OK;
}