// k x k convolution with k in {1, 5} (stride 1, zero padding k/2) for gfx950 (MI355X), NHWC: forward / input gradient
// and weight gradient on the MFMA matrix cores, plus the BatchNorm + ELU element passes of VNet.
//
// Stands in for nn.Conv2d(C, C, kernel_size=5, padding=2) of the reference's LUConv / InputTransition /
// OutputTransition (unet_zoo/models/vnet.py:31, :47, :120), for its two gradients under autograd, and for
// ContBatchNorm2d -> ELU with the residual sums and Dropout2d masks around them (vnet.py:35, :65, :82-85, :102-114).
//
// Forward / input gradient: implicit GEMM with a FLAT reduction index, C[M = pixels][N] = A[M][K = 25 * Cin] * B[N][K]^T.
//   uz_conv_igemm walks (tap, 128-byte channel slab) pairs, so a 32-channel bf16 layer would fill half of every slab with
//   zeros; here a 128-byte K-step is cut out of the flat index k = tap * Cin + c, so it may span two taps (Cin = 32, bf16)
//   or a quarter of one (Cin = 256): no padding for any Cin that is a multiple of 16 bytes.  The rest is the generic
//   kernel's shape: 128-pixel x BN tile, 4 waves, register-staged global -> LDS double buffer with XOR-swizzled 16-byte
//   chunks, persistent over M so the BatchNorm partial sums leave a block once as one deterministic row.
//   The input gradient is the same kernel on the flipped, transposed weights (UZ_PACK_CONV_DGRAD).
// Weight gradient: out[i][j][tap] = sum_p L[p][i] * R[p + tap][j]; one (channel tile, tap, pixel range) per workgroup,
//   pixel-major LDS tiles read with ds_read_b64_tr_b16 (bf16) / ds_read_b32 (fp32) as uz_wgrad.hip does, but the four
//   waves split the PIXELS of a K-step instead of the tile, so a 32 x 32 tile (VNet's 32-channel layers, and the
//   num_classes-wide output layer padded to 8) keeps all four busy; they meet in LDS in a fixed order.  Pixel ranges write
//   their own fp32 slabs, a second kernel sums them in a fixed order into the (Cout, Cin, 5, 5) layout: deterministic.
#include "uz_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------- forward / dgrad
struct C5Args {
  const void* x;
  const void* w;
  void* y;
  const float* bias;
  float* stats;
  int M, H, W, Cin, ldx, Nout, ldy, K, ks, tiles_m;
};

template <typename T> struct Mma5;
template <> struct Mma5<bf16_t> {
  static __device__ __forceinline__ void run(const Vec16<bf16_t>& a, const Vec16<bf16_t>& b, f32x16& c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&a), *reinterpret_cast<const bf16x8*>(&b), c,
                                                0, 0, 0);
  }
};
template <> struct Mma5<float> {
  // the K order inside a 128-byte slab is permuted identically for A and B: the dot product is unchanged
  static __device__ __forceinline__ void run(const Vec16<float>& a, const Vec16<float>& b, f32x16& c) {
#pragma unroll
    for (int t = 0; t < 4; ++t) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[t], b.v[t], c, 0, 0, 0);
  }
};

template <typename T, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256, 2) void conv5_kernel(const C5Args a) {
  constexpr int VEC = ElemTraits<T>::VEC;
  constexpr int BK = 8 * VEC;  // elements per 128-byte K-step
  constexpr int AR = BM / 32, BR = BN / 32;
  constexpr int WTM = BM / WM, WTN = BN / WN, TM = WTM / 32, TN = WTN / 32;
  static_assert(WM * WN == 4, "4 waves per block");
  static_assert(TM >= 1 && TN >= 1, "wave tile");
  constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE = A_BYTES + B_BYTES;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int lc = tid & 7, lr = tid >> 3;
  const int l31 = lane & 31, lh = lane >> 5;
  const int n0 = blockIdx.y * BN;
  const T* __restrict__ xg = static_cast<const T*>(a.x);
  const T* __restrict__ wg = static_cast<const T*>(a.w);
  T* __restrict__ yg = static_cast<T*>(a.y);

  const T* bptr[BR];
  bool bval[BR];
#pragma unroll
  for (int i = 0; i < BR; ++i) {
    const int n = n0 + lr + 32 * i;
    bval[i] = n < a.Nout;
    bptr[i] = wg + (size_t)(bval[i] ? n : 0) * a.K;
  }

  float s1[TN], s2[TN];
#pragma unroll
  for (int i = 0; i < TN; ++i) s1[i] = s2[i] = 0.f;

  const int nk = (a.K + BK - 1) / BK;
  const int HW = a.H * a.W;
  const int rad = a.ks >> 1;
  const int st_sw = ((lr >> 1) & 7);   // store-side swizzle (row = lr + 32 i)
  const int ld_sw = ((l31 >> 1) & 7);  // read-side swizzle (row = 32 j + l31)

  for (int tile = blockIdx.x; tile < a.tiles_m; tile += gridDim.x) {
    const int m0 = tile * BM;
    int rh[AR], rw[AR], rpix[AR];
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const int m = m0 + lr + 32 * i;
      const bool ok = m < a.M;
      const int mm = ok ? m : 0;
      const int img = mm / HW;
      const int rem = mm - img * HW;
      const int h = rem / a.W;
      rh[i] = ok ? h : -(1 << 28);
      rw[i] = rem - h * a.W;
      rpix[i] = mm;
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // every load of a K-step is issued unconditionally from a clamped (always valid) address, the zero for a
    // tap outside the image / a row outside the tile is selected afterwards -- a load under a branch is waited for where
    // the branch ends, one memory round trip per row
    f32x4 ra[AR], rb[BR];

    auto load_step = [&](int kb) {
      const int kk = kb * BK + lc * VEC;   // this thread's 16-byte chunk of the flat reduction index
      const bool kok = kk < a.K;
      const int tap = (kok ? kk : 0) / a.Cin;
      const int c = (kok ? kk : 0) - tap * a.Cin;
      const int ty = tap / a.ks;
      const int dy = ty - rad, dx = tap - ty * a.ks - rad;
      bool aok[AR];
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        const int hh = rh[i] + dy, ww = rw[i] + dx;
        aok[i] = kok && (unsigned)hh < (unsigned)a.H && (unsigned)ww < (unsigned)a.W;
        const size_t off = (size_t)(aok[i] ? rpix[i] + dy * a.W + dx : 0) * (size_t)a.ldx + c;
        ra[i] = *reinterpret_cast<const f32x4*>(xg + off);
      }
#pragma unroll
      for (int i = 0; i < BR; ++i) rb[i] = *reinterpret_cast<const f32x4*>(bptr[i] + (kok ? kk : 0));
#pragma unroll
      for (int i = 0; i < AR; ++i) asm volatile("" : "+v"(ra[i]));
#pragma unroll
      for (int i = 0; i < BR; ++i) asm volatile("" : "+v"(rb[i]));
      const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < AR; ++i) ra[i] = aok[i] ? ra[i] : z4;
#pragma unroll
      for (int i = 0; i < BR; ++i) rb[i] = (bval[i] && kok) ? rb[i] : z4;
    };
    auto store_step = [&](int buf) {
      char* sA = smem + buf * STAGE;
      char* sB = sA + A_BYTES;
#pragma unroll
      for (int i = 0; i < AR; ++i) *reinterpret_cast<f32x4*>(sA + (lr + 32 * i) * 128 + ((lc ^ st_sw) << 4)) = ra[i];
#pragma unroll
      for (int i = 0; i < BR; ++i) *reinterpret_cast<f32x4*>(sB + (lr + 32 * i) * 128 + ((lc ^ st_sw) << 4)) = rb[i];
    };

    load_step(0);
    store_step(0);
    __syncthreads();
    for (int kb = 0; kb < nk; ++kb) {
      const bool more = kb + 1 < nk;
      if (more) load_step(kb + 1);
      const char* sA = smem + (kb & 1) * STAGE;
      const char* sB = sA + A_BYTES;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int chunk = ((2 * q + lh) ^ ld_sw) << 4;
        Vec16<T> af[TM], bf[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const Vec16<T>*>(sA + (wm * WTM + i * 32 + l31) * 128 + chunk);
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const Vec16<T>*>(sB + (wn * WTN + j * 32 + l31) * 128 + chunk);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) Mma5<T>::run(af[i], bf[j], acc[i][j]);
      }
      if (more) store_step((kb + 1) & 1);
      __syncthreads();
    }

    // epilogue: bias, store, per-channel statistics of the stored value
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + wn * WTN + j * 32 + l31;
      const bool nok = n < a.Nout;
      const float bv = (a.bias != nullptr && nok) ? a.bias[n] : 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (m < a.M && nok) {
            const T tv = (T)(acc[i][j][r] + bv);
            yg[(size_t)m * a.ldy + n] = tv;
            const float fv = (float)tv;
            s1[j] += fv;
            s2[j] += fv * fv;
          }
        }
      }
    }
  }

  if (a.stats != nullptr) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      s1[j] += __shfl_xor(s1[j], 32);
      s2[j] += __shfl_xor(s2[j], 32);
    }
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);  // [WM][BN][2]
    if (lh == 0) {
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = wn * WTN + j * 32 + l31;
        red[(wm * BN + col) * 2 + 0] = s1[j];
        red[(wm * BN + col) * 2 + 1] = s2[j];
      }
    }
    __syncthreads();
    if (tid < BN) {
      float t1 = 0.f, t2 = 0.f;
#pragma unroll
      for (int k = 0; k < WM; ++k) {
        t1 += red[(k * BN + tid) * 2 + 0];
        t2 += red[(k * BN + tid) * 2 + 1];
      }
      const int n = n0 + tid;
      if (n < a.Nout) {
        a.stats[((size_t)blockIdx.x * 2 + 0) * a.Nout + n] = t1;
        a.stats[((size_t)blockIdx.x * 2 + 1) * a.Nout + n] = t2;
      }
    }
  }
}

struct C5Plan {
  int bn, tiles_m, tiles_n, grid_m;
};

int c5_plan(const uz_conv5x5_desc* d, C5Plan* p) {
  UZ_REQUIRE(d != nullptr, "uz_conv5x5: null descriptor");
  UZ_REQUIRE(d->dtype == UZ_F32 || d->dtype == UZ_BF16, "uz_conv5x5: bad dtype %d", d->dtype);
  const int vec = d->dtype == UZ_BF16 ? 8 : 4;
  UZ_REQUIRE(d->ksize == 5 || d->ksize == 1, "uz_conv5x5: kernel size %d is not supported (5, or 1 for a pointwise layer)",
             d->ksize);
  UZ_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Nout > 0, "uz_conv5x5: non-positive shape");
  UZ_REQUIRE(d->Cin % vec == 0 && d->Cin <= 512, "uz_conv5x5: Cin=%d must be a multiple of %d, at most 512", d->Cin, vec);
  UZ_REQUIRE(d->Nout <= 512, "uz_conv5x5: Nout=%d, at most 512 output channels", d->Nout);
  UZ_REQUIRE(d->ldx % vec == 0 && d->ldx >= d->Cin, "uz_conv5x5: bad ldx=%d (Cin=%d)", d->ldx, d->Cin);
  UZ_REQUIRE(d->ldy >= d->Nout, "uz_conv5x5: bad ldy=%d (Nout=%d)", d->ldy, d->Nout);
  const long long M = (long long)d->N * d->H * d->W;
  UZ_REQUIRE(M < (1LL << 31) && M * (long long)(d->ldx > d->ldy ? d->ldx : d->ldy) < (1LL << 40), "uz_conv5x5: tensor too large");
  p->bn = d->Nout <= 32 ? 32 : (d->Nout <= 64 ? 64 : 128);
  p->tiles_m = uz_cdiv(M, 128);
  p->tiles_n = uz_cdiv(d->Nout, p->bn);
  int cap = (2 * UZ_NUM_CU_HW) / p->tiles_n;   // the hardware's CU count: the number of statistics rows is fixed per shape
  if (cap < 1) cap = 1;
  p->grid_m = p->tiles_m < cap ? p->tiles_m : cap;
  return UZ_OK;
}

template <typename T> int c5_launch(const C5Plan& p, const C5Args& a, hipStream_t s) {
  dim3 grid(p.grid_m, p.tiles_n), block(256);
  if (p.bn == 32) {
    hipLaunchKernelGGL((conv5_kernel<T, 128, 32, 4, 1>), grid, block, 0, s, a);
  } else if (p.bn == 64) {
    hipLaunchKernelGGL((conv5_kernel<T, 128, 64, 2, 2>), grid, block, 0, s, a);
  } else {
    hipLaunchKernelGGL((conv5_kernel<T, 128, 128, 2, 2>), grid, block, 0, s, a);
  }
  UZ_LAUNCH_CHECK("uz_conv5x5");
  return UZ_OK;
}

// ---------------------------------------------------------------------------------------------------- weight gradient
struct W5Args {
  const void* L;
  const void* R;
  float* slab;
  int P, H, W, Ci, ldl, Cj, ldr, ks, ntaps, chunk, tiles_j;
};

template <typename T> struct W5Cfg;
template <> struct W5Cfg<bf16_t> {
  static constexpr int BKP = 64;  // pixels per K-step
  static constexpr int PAD = 64;  // bytes of row padding: the four pixel rows of a transposed read land on distinct banks
};
template <> struct W5Cfg<float> {
  static constexpr int BKP = 32;
  static constexpr int PAD = 0;
};

template <typename T, int B>
__global__ __launch_bounds__(256, 2) void wgrad5_kernel(const W5Args a) {
  constexpr int VEC = ElemTraits<T>::VEC;
  constexpr int BKP = W5Cfg<T>::BKP;
  constexpr int CPR = B / VEC;      // 16-byte chunks per pixel row
  constexpr int RPP = 256 / CPR;    // pixel rows per pass
  constexpr int NP = BKP / RPP;
  static_assert(NP >= 1, "tile too wide for BKP");
  constexpr int RS = B * (int)sizeof(T) + W5Cfg<T>::PAD;
  constexpr int T_BYTES = BKP * RS, STAGE = 2 * T_BYTES;
  constexpr int TT = B / 32;        // 32 x 32 MFMA tiles per edge; every wave owns the whole B x B tile
  constexpr int RED_BYTES = 3 * TT * TT * 16 * 64 * (int)sizeof(float);
  constexpr int SMEM = 2 * STAGE > RED_BYTES ? 2 * STAGE : RED_BYTES;
  __shared__ __attribute__((aligned(16))) char smem[SMEM];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int ti0 = (blockIdx.x / a.tiles_j) * B, tj0 = (blockIdx.x % a.tiles_j) * B;
  const int tap = blockIdx.y;
  const int pbeg = blockIdx.z * a.chunk;
  const int pend = (pbeg + a.chunk < a.P) ? pbeg + a.chunk : a.P;
  const T* __restrict__ Lg = static_cast<const T*>(a.L);
  const T* __restrict__ Rg = static_cast<const T*>(a.R);

  const int rad = a.ks >> 1;
  const int ty = tap / a.ks;
  const int dy = ty - rad, dx = tap - ty * a.ks - rad;

  const int lcc = tid % CPR, lrr = tid / CPR;
  const bool cokI = ti0 + lcc * VEC < a.Ci;
  const bool cokJ = tj0 + lcc * VEC < a.Cj;
  int rh[NP], rw[NP];
  const int HW = a.H * a.W;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int p = pbeg + lrr + RPP * i;
    const int rem = p % HW;
    rh[i] = rem / a.W;
    rw[i] = rem - rh[i] * a.W;
  }

  f32x16 acc[TT][TT];
#pragma unroll
  for (int i = 0; i < TT; ++i)
#pragma unroll
    for (int j = 0; j < TT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  f32x4 rl[NP], rr[NP];   // loads unconditional from clamped addresses, zeros selected afterwards
  int pk = pbeg;  // first pixel of the K-step being loaded

  auto load_step = [&]() {
    bool okl[NP], okr[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int p = pk + lrr + RPP * i;
      const bool in = p < pend;
      okl[i] = in && cokI;
      rl[i] = *reinterpret_cast<const f32x4*>(Lg + (okl[i] ? (size_t)p * a.ldl + ti0 + lcc * VEC : (size_t)0));
      const int hh = rh[i] + dy, ww = rw[i] + dx;
      okr[i] = in && cokJ && (unsigned)hh < (unsigned)a.H && (unsigned)ww < (unsigned)a.W;
      rr[i] = *reinterpret_cast<const f32x4*>(Rg + (okr[i] ? (size_t)(p + dy * a.W + dx) * a.ldr + tj0 + lcc * VEC : (size_t)0));
      // this row's coordinates at the next K-step
      rw[i] += BKP;
      while (rw[i] >= a.W) {
        rw[i] -= a.W;
        if (++rh[i] == a.H) rh[i] = 0;
      }
    }
    pk += BKP;
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NP; ++i) asm volatile("" : "+v"(rl[i]), "+v"(rr[i]));
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      rl[i] = okl[i] ? rl[i] : z4;
      rr[i] = okr[i] ? rr[i] : z4;
    }
  };
  auto store_step = [&](int buf) {
    char* sL = smem + buf * STAGE;
    char* sR = sL + T_BYTES;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      *reinterpret_cast<f32x4*>(sL + (lrr + RPP * i) * RS + lcc * 16) = rl[i];
      *reinterpret_cast<f32x4*>(sR + (lrr + RPP * i) * RS + lcc * 16) = rr[i];
    }
  };

  const int nk = (pend - pbeg + BKP - 1) / BKP;
  if (nk > 0) {
    load_step();
    store_step(0);
  }
  __syncthreads();
  for (int kb = 0; kb < nk; ++kb) {
    const bool more = kb + 1 < nk;
    if (more) load_step();
    const char* sL = smem + (kb & 1) * STAGE;
    const char* sR = sL + T_BYTES;
    if constexpr (sizeof(T) == 2) {
      // wave w owns pixels 16 w .. 16 w + 15 of the step; lane -> (16-lane group g, row q, column quad p4) of the
      // transposed 4 x 16 block read
      const int g = lane >> 4, q = (lane & 15) >> 2, p4 = lane & 3;
      const int krow = 16 * wave + 8 * (g >> 1) + q;
      const int ccol = 16 * (g & 1) + 4 * p4;
      typedef __attribute__((address_space(3))) bf16x4* lds_bf16x4_ptr;
      bf16x8 af[TT], bfr[TT];
#pragma unroll
      for (int i = 0; i < TT; ++i) {
        const char* p0 = sL + krow * RS + (i * 32 + ccol) * 2;
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(p0));
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(p0 + 4 * RS));
        af[i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int j = 0; j < TT; ++j) {
        const char* p0 = sR + krow * RS + (j * 32 + ccol) * 2;
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(p0));
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(p0 + 4 * RS));
        bfr[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int i = 0; i < TT; ++i)
#pragma unroll
        for (int j = 0; j < TT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    } else {
      // wave w owns pixels 8 w .. 8 w + 7 of the step
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = 8 * wave + 2 * s + lh;
        float af[TT], bfr[TT];
#pragma unroll
        for (int i = 0; i < TT; ++i) af[i] = *reinterpret_cast<const float*>(sL + k * RS + (i * 32 + l31) * 4);
#pragma unroll
        for (int j = 0; j < TT; ++j) bfr[j] = *reinterpret_cast<const float*>(sR + k * RS + (j * 32 + l31) * 4);
#pragma unroll
        for (int i = 0; i < TT; ++i)
#pragma unroll
          for (int j = 0; j < TT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bfr[j], acc[i][j], 0, 0, 0);
      }
    }
    if (more) store_step((kb + 1) & 1);
    __syncthreads();
  }

  // the four waves' partial tiles meet in LDS: waves 1..3 park theirs, wave 0 adds them in that order
  float* red = reinterpret_cast<float*>(smem);
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < TT; ++i)
#pragma unroll
      for (int j = 0; j < TT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[((((wave - 1) * TT + i) * TT + j) * 16 + r) * 64 + lane] = acc[i][j][r];
  }
  __syncthreads();
  if (wave != 0) return;
  // partial slab [split][tap][Ci][Cj]: lanes 0..31 write 32 consecutive j (128 contiguous bytes)
  float* slab = a.slab + ((size_t)blockIdx.z * a.ntaps + tap) * (size_t)a.Ci * a.Cj;
#pragma unroll
  for (int i = 0; i < TT; ++i) {
#pragma unroll
    for (int j = 0; j < TT; ++j) {
      const int cj = tj0 + j * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = acc[i][j][r];
#pragma unroll
        for (int w = 0; w < 3; ++w) v += red[(((w * TT + i) * TT + j) * 16 + r) * 64 + lane];
        const int ci = ti0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (ci < a.Ci && cj < a.Cj) slab[(size_t)ci * a.Cj + cj] = v;
      }
    }
  }
}

// out[(i * CjOut + j) * ntaps + t] = sum_z slab[z][t][i][j] for i < CiOut, j < CjOut (channels beyond them are the zero
// padding of a thin layer); splits added in ascending order
__global__ __launch_bounds__(256) void wgrad5_reduce_kernel(const float* __restrict__ slab, int split, int ntaps, int Ci, int Cj,
                                                           int CiOut, int CjOut, float* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const int t = blockIdx.y;
  if (e >= (long long)CiOut * CjOut) return;
  const int i = (int)(e / CjOut), j = (int)(e - (long long)i * CjOut);
  const size_t CiCj = (size_t)Ci * Cj;
  const float* src = slab + (size_t)t * CiCj + (size_t)i * Cj + j;
  float v = 0.f;
  for (int z = 0; z < split; ++z) v += src[(size_t)z * ntaps * CiCj];
  out[e * ntaps + t] = v;
}

struct W5Plan {
  int b, tiles_i, tiles_j, split, chunk, ntaps;
};

int w5_plan(const uz_wgrad5x5_desc* d, W5Plan* p) {
  UZ_REQUIRE(d != nullptr, "uz_wgrad5x5: null descriptor");
  UZ_REQUIRE(d->dtype == UZ_F32 || d->dtype == UZ_BF16, "uz_wgrad5x5: bad dtype %d", d->dtype);
  const int vec = d->dtype == UZ_BF16 ? 8 : 4;
  const int bkp = d->dtype == UZ_BF16 ? 64 : 32;
  UZ_REQUIRE(d->ksize == 5 || d->ksize == 1, "uz_wgrad5x5: kernel size %d is not supported (5, or 1 for a pointwise layer)",
             d->ksize);
  UZ_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Ci > 0 && d->Cj > 0, "uz_wgrad5x5: non-positive shape");
  UZ_REQUIRE(d->Ci % vec == 0 && d->Cj % vec == 0 && d->Ci <= 512 && d->Cj <= 512,
             "uz_wgrad5x5: channels (%d, %d) must be multiples of %d, at most 512", d->Ci, d->Cj, vec);
  UZ_REQUIRE(d->ldl % vec == 0 && d->ldr % vec == 0 && d->ldl >= d->Ci && d->ldr >= d->Cj, "uz_wgrad5x5: bad leading dimension");
  UZ_REQUIRE(d->CiOut > 0 && d->CiOut <= d->Ci && d->CjOut > 0 && d->CjOut <= d->Cj,
             "uz_wgrad5x5: result channels (%d, %d) outside the operands' (%d, %d)", d->CiOut, d->CjOut, d->Ci, d->Cj);
  const long long P = (long long)d->N * d->H * d->W;
  UZ_REQUIRE(P < (1LL << 31) - (1 << 20), "uz_wgrad5x5: too large");
  p->ntaps = d->ksize * d->ksize;
  p->b = (d->Ci <= 32 && d->Cj <= 32) ? 32 : 64;
  p->tiles_i = uz_cdiv(d->Ci, p->b);
  p->tiles_j = uz_cdiv(d->Cj, p->b);
  const long long base = (long long)p->tiles_i * p->tiles_j * p->ntaps;
  // sized by the hardware's CU count, not by uz_set_cu_reserve(): the number of pixel ranges is the number of slabs and
  // with it the order of the final sums -- a gradient must not change in its last bits with the reserve.  These are
  // ordinary grids of short workgroups (no one-workgroup-per-CU persistence), so a collective on another stream finds
  // free CUs as workgroups retire; the reserve is for the persistent 160 KB kernels.
  long long split = (4LL * UZ_NUM_CU_HW + base - 1) / base;
  long long max_split = P / (4LL * bkp) > 0 ? P / (4LL * bkp) : 1;
  if (max_split > 64) max_split = 64;
  if (split > max_split) split = max_split;
  if (split < 1) split = 1;
  long long chunk = (P + split - 1) / split;
  chunk = ((chunk + bkp - 1) / bkp) * bkp;
  split = (P + chunk - 1) / chunk;
  p->split = (int)split;
  p->chunk = (int)chunk;
  return UZ_OK;
}

template <typename T> int w5_launch(const W5Plan& p, const W5Args& a, hipStream_t s) {
  dim3 grid(p.tiles_i * p.tiles_j, p.ntaps, p.split), block(256);
  if (p.b == 32) {
    hipLaunchKernelGGL((wgrad5_kernel<T, 32>), grid, block, 0, s, a);
  } else {
    hipLaunchKernelGGL((wgrad5_kernel<T, 64>), grid, block, 0, s, a);
  }
  UZ_LAUNCH_CHECK("uz_wgrad5x5");
  return UZ_OK;
}

// ---------------------------------------------------------------------------------------------------- BatchNorm + ELU
// V channels per thread: a 16-byte vector where the channel count and every leading dimension allow it, else one element
// (the num_classes-wide output layer)
template <typename T, int V> __device__ __forceinline__ void ldv(const T* p, float* o) {
  if constexpr (V == 1) {
    o[0] = (float)p[0];
  } else {
    const Vec16<T> v = ld16(p);
#pragma unroll
    for (int i = 0; i < V; ++i) o[i] = (float)v.v[i];
  }
}
template <typename T, int V> __device__ __forceinline__ void stv(T* p, const float* o) {
  if constexpr (V == 1) {
    p[0] = (T)o[0];
  } else {
    Vec16<T> v;
#pragma unroll
    for (int i = 0; i < V; ++i) v.v[i] = (T)o[i];
    st16(p, v);
  }
}
__device__ __forceinline__ float elu1(float x) { return x > 0.f ? x : expm1f(x); }

struct BeArgs {
  const void* x;      // raw convolution output
  const void* res;    // nullable
  void* out;
  void* out2;         // nullable: out * mask2[n][c]
  const float *scale, *shift, *mask2;
  int ldx, ldres, ldo, ldo2, C, HW, flags;
  long long P;
};

template <typename T, int V> __global__ __launch_bounds__(256) void bn_elu_apply_kernel(const BeArgs a) {
  const int CC = a.C / V;
  const long long total = a.P * CC;
  const T* __restrict__ xg = static_cast<const T*>(a.x);
  const T* __restrict__ rg = static_cast<const T*>(a.res);
  T* __restrict__ og = static_cast<T*>(a.out);
  T* __restrict__ o2g = static_cast<T*>(a.out2);
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long p = idx / CC;
    const int c0 = (int)(idx - p * CC) * V;
    float v[V], sc[V], sh[V], r[V];
    ldv<T, V>(xg + (size_t)p * a.ldx + c0, v);
    ldv<float, V == 1 ? 1 : 4>(a.scale + c0, sc);
    ldv<float, V == 1 ? 1 : 4>(a.shift + c0, sh);
    if constexpr (V == 8) {
      ldv<float, 4>(a.scale + c0 + 4, sc + 4);
      ldv<float, 4>(a.shift + c0 + 4, sh + 4);
    }
    // unconditional: without a residual the load re-reads x's own line and the value is not used
    ldv<T, V>((rg != nullptr ? rg : xg) + (size_t)p * (rg != nullptr ? a.ldres : a.ldx) + c0, r);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      float t = fmaf(v[i], sc[i], sh[i]);
      if (a.flags & 1) t = elu1(t);
      if (rg != nullptr) t = (float)(T)t + r[i];   // the sum of two stored tensors, as torch.add of them gives it
      if (a.flags & 2) t = elu1(t);
      v[i] = (float)(T)t;
    }
    stv<T, V>(og + (size_t)p * a.ldo + c0, v);
    if (o2g != nullptr) {
      const float* mk = a.mask2 + (size_t)(p / a.HW) * a.C + c0;
#pragma unroll
      for (int i = 0; i < V; ++i) v[i] *= mk[i];
      stv<T, V>(o2g + (size_t)p * a.ldo2 + c0, v);
    }
  }
}

struct BbArgs {
  const void* x;      // raw convolution output
  const void* out;    // stored result of the forward pass (read when act2 is ELU)
  const void *g0, *g1, *g2;   // gradients of out (g0; g1 nullable) and of out2 (g2 nullable, times mask2)
  const float *scale, *shift, *mean, *invstd, *mask2;
  float* partials;    // reduce: [rows][2][C]
  const double* sums; // apply: totals [2][C]
  void* dx;
  void* gres;         // nullable: gradient of the residual input
  int ldx, ldo, ldg0, ldg1, ldg2, lddx, ldgres, C, HW, flags;
  // every source is loaded unconditionally.  An absent one (g1, g2 / mask2, out) points at a tensor that IS
  // there (g0, scale, x) and enters with weight 0 / stride 0 / an unused factor, so no load sits under a branch.
  float w1, w2;
  int mask_rows;      // 1: mask2 is (N, C); 0: the stand-in row
  long long P;
  double count;
};

// the gradient at the BatchNorm's output, and (gz) at the residual input
template <typename T, int V>
__device__ __forceinline__ void bn_elu_grad(const BbArgs& a, long long p, int c0, const float* sc, const float* sh, float* xv,
                                            float* gb, float* gz) {
  ldv<T, V>(static_cast<const T*>(a.x) + (size_t)p * a.ldx + c0, xv);
  float t1[V], t2[V], o[V], mk[V];
  ldv<T, V>(static_cast<const T*>(a.g0) + (size_t)p * a.ldg0 + c0, gz);
  ldv<T, V>(static_cast<const T*>(a.g1) + (size_t)p * a.ldg1 + c0, t1);
  ldv<T, V>(static_cast<const T*>(a.g2) + (size_t)p * a.ldg2 + c0, t2);
  ldv<T, V>(static_cast<const T*>(a.out) + (size_t)p * a.ldo + c0, o);
  const float* mp = a.mask2 + (size_t)(p / a.HW) * a.C * a.mask_rows + c0;
#pragma unroll
  for (int i = 0; i < V; ++i) mk[i] = mp[i];
  const bool act2 = (a.flags & 2) != 0;
#pragma unroll
  for (int i = 0; i < V; ++i) {
    gz[i] = fmaf(a.w2 * t2[i], mk[i], fmaf(a.w1, t1[i], gz[i]));
    // ELU'(z) from the stored result y: 1 where y > 0, else y + 1
    gz[i] *= (act2 && !(o[i] > 0.f)) ? o[i] + 1.f : 1.f;
  }
#pragma unroll
  for (int i = 0; i < V; ++i) {
    gb[i] = gz[i];
    if (a.flags & 1) {
      const float t = fmaf(xv[i], sc[i], sh[i]);
      gb[i] *= t > 0.f ? 1.f : __expf(t);
    }
  }
}

// block (bx channel chunks, by pixel lanes); grid (gx pixel groups, gy chunk groups); one partial row per blockIdx.x
template <typename T, int V> __global__ __launch_bounds__(256) void bn_elu_bwd_reduce_kernel(const BbArgs a) {
  __shared__ float red[256 * 2 * V];
  const int CC = a.C / V;
  const int cc = blockIdx.y * blockDim.x + threadIdx.x;
  const bool cok = cc < CC;
  const int c0 = (cok ? cc : 0) * V;
  float sc[V], sh[V], mu[V], is[V], s1[V], s2[V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    sc[i] = a.scale[c0 + i];
    sh[i] = a.shift[c0 + i];
    mu[i] = a.mean[c0 + i];
    is[i] = a.invstd[c0 + i];
    s1[i] = s2[i] = 0.f;
  }
  const long long stride = (long long)gridDim.x * blockDim.y;
  for (long long p = (long long)blockIdx.x * blockDim.y + threadIdx.y; p < a.P && cok; p += stride) {
    float xv[V], gb[V], gz[V];
    bn_elu_grad<T, V>(a, p, c0, sc, sh, xv, gb, gz);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      s1[i] += gb[i];
      s2[i] = fmaf(gb[i], (xv[i] - mu[i]) * is[i], s2[i]);
    }
  }
  float* mine = red + ((size_t)threadIdx.y * blockDim.x + threadIdx.x) * (2 * V);
#pragma unroll
  for (int i = 0; i < V; ++i) {
    mine[i] = s1[i];
    mine[V + i] = s2[i];
  }
  __syncthreads();
  for (int e = threadIdx.y; e < 2 * V; e += blockDim.y) {
    float t = 0.f;
    for (int r = 0; r < (int)blockDim.y; ++r) t += red[((size_t)r * blockDim.x + threadIdx.x) * (2 * V) + e];
    if (cok) a.partials[((size_t)blockIdx.x * 2 + e / V) * a.C + c0 + (e % V)] = t;
  }
}

template <typename T, int V> __global__ __launch_bounds__(256) void bn_elu_bwd_apply_kernel(const BbArgs a) {
  const int CC = a.C / V;
  const long long total = a.P * CC;
  const float inv = (float)(1.0 / a.count);
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long p = idx / CC;
    const int c0 = (int)(idx - p * CC) * V;
    float sc[V], sh[V], xv[V], gb[V], gz[V], o[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      sc[i] = a.scale[c0 + i];
      sh[i] = a.shift[c0 + i];
    }
    bn_elu_grad<T, V>(a, p, c0, sc, sh, xv, gb, gz);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float m1 = (float)a.sums[c0 + i] * inv, m2 = (float)a.sums[a.C + c0 + i] * inv;
      const float xh = (xv[i] - a.mean[c0 + i]) * a.invstd[c0 + i];
      o[i] = sc[i] * (gb[i] - m1 - xh * m2);
    }
    stv<T, V>(static_cast<T*>(a.dx) + (size_t)p * a.lddx + c0, o);
    if (a.gres != nullptr) stv<T, V>(static_cast<T*>(a.gres) + (size_t)p * a.ldgres + c0, gz);
  }
}

int be_vec(int dtype, int C, const int* lds, int n) {
  const int vec = dtype == UZ_BF16 ? 8 : 4;
  if (C % vec != 0) return 1;
  for (int i = 0; i < n; ++i)
    if (lds[i] % vec != 0) return 1;
  return vec;
}

// the vector path reads and writes 16 bytes at a time: every tensor it touches has to start on a 16-byte boundary
bool be_aligned(const void* const* ptrs, int n) {
  for (int i = 0; i < n; ++i)
    if (ptrs[i] != nullptr && ((uintptr_t)ptrs[i] & 15) != 0) return false;
  return true;
}

void be_reduce_shape(int CC, long long P, dim3* grid, dim3* block) {
  int bx = 1;
  while (bx < CC && bx < 64) bx <<= 1;
  const int by = 256 / bx;
  const int gy = (CC + bx - 1) / bx;
  long long gx = (P + (long long)by * 8 - 1) / ((long long)by * 8);
  long long cap = 2LL * UZ_NUM_CU_HW / gy;   // the hardware's CU count: the partial rows fix the order of dgamma / dbeta's sums
  if (cap < 1) cap = 1;
  if (gx > cap) gx = cap;
  if (gx < 1) gx = 1;
  *grid = dim3((unsigned)gx, (unsigned)gy);
  *block = dim3((unsigned)bx, (unsigned)by);
}

int be_grid(long long total) {
  long long g = (total + 255) / 256;
  const long long cap = 8LL * UZ_NUM_CU_HW;
  if (g > cap) g = cap;
  return g < 1 ? 1 : (int)g;
}

int bb_check(const uz_bn_elu_bwd_desc* d, const char* who) {
  UZ_REQUIRE(d != nullptr, "%s: null descriptor", who);
  UZ_REQUIRE(d->dtype == UZ_F32 || d->dtype == UZ_BF16, "%s: bad dtype %d", who, d->dtype);
  UZ_REQUIRE(d->N > 0 && d->HW > 0 && d->C > 0, "%s: non-positive shape", who);
  UZ_REQUIRE((long long)d->N * d->HW < (1LL << 31), "%s: too large", who);
  UZ_REQUIRE((d->flags & ~3) == 0, "%s: bad flags %d", who, d->flags);
  UZ_REQUIRE(d->ldx >= d->C && d->ldg0 >= d->C && d->lddx >= d->C, "%s: bad leading dimension", who);
  return UZ_OK;
}

int bb_vec(const uz_bn_elu_bwd_desc* d) {
  const int lds[7] = {d->ldx, d->ldo, d->ldg0, d->ldg1, d->ldg2, d->lddx, d->ldgres};
  return be_vec(d->dtype, d->C, lds, 7);
}

BbArgs bb_args(const uz_bn_elu_bwd_desc* d, const void* x, const void* out, const void* g0, const void* g1, const void* g2,
               const float* mask2, const float* scale, const float* shift, const float* mean, const float* invstd) {
  BbArgs a;
  const bool act2 = (d->flags & 2) != 0;
  a.x = x, a.g0 = g0;
  a.out = act2 ? out : x, a.ldo = act2 ? d->ldo : d->ldx;
  a.g1 = g1 ? g1 : g0, a.ldg1 = g1 ? d->ldg1 : d->ldg0, a.w1 = g1 ? 1.f : 0.f;
  a.g2 = g2 ? g2 : g0, a.ldg2 = g2 ? d->ldg2 : d->ldg0, a.w2 = g2 ? 1.f : 0.f;
  a.mask2 = g2 ? mask2 : scale, a.mask_rows = g2 ? 1 : 0;
  a.scale = scale, a.shift = shift, a.mean = mean, a.invstd = invstd;
  a.partials = nullptr, a.sums = nullptr, a.dx = nullptr, a.gres = nullptr;
  a.ldx = d->ldx, a.ldg0 = d->ldg0, a.lddx = d->lddx, a.ldgres = d->ldgres;
  a.C = d->C, a.HW = d->HW, a.flags = d->flags;
  a.P = (long long)d->N * d->HW;
  a.count = (double)a.P;
  return a;
}

}  // namespace

extern "C" int uz_conv5x5_grid_m(const uz_conv5x5_desc* d) {
  C5Plan p;
  const int rc = c5_plan(d, &p);
  return rc != UZ_OK ? rc : p.grid_m;
}

extern "C" int uz_conv5x5(const uz_conv5x5_desc* d, const void* x, const void* w_packed, const float* bias, void* y, float* stats,
                          void* stream) {
  C5Plan p;
  const int rc = c5_plan(d, &p);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(x && w_packed && y, "uz_conv5x5: null pointer");
  UZ_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)w_packed & 15) == 0, "uz_conv5x5: x / w must be 16-byte aligned");
  C5Args a;
  a.x = x, a.w = w_packed, a.y = y, a.bias = bias, a.stats = stats;
  a.M = d->N * d->H * d->W, a.H = d->H, a.W = d->W, a.Cin = d->Cin, a.ldx = d->ldx, a.Nout = d->Nout, a.ldy = d->ldy;
  a.ks = d->ksize, a.K = d->ksize * d->ksize * d->Cin, a.tiles_m = p.tiles_m;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return d->dtype == UZ_BF16 ? c5_launch<bf16_t>(p, a, s) : c5_launch<float>(p, a, s);
}

extern "C" long long uz_wgrad5x5_workspace_bytes(const uz_wgrad5x5_desc* d) {
  W5Plan p;
  const int rc = w5_plan(d, &p);
  if (rc != UZ_OK) return rc;
  return (long long)p.split * p.ntaps * d->Ci * d->Cj * (long long)sizeof(float);
}

extern "C" int uz_wgrad5x5(const uz_wgrad5x5_desc* d, const void* L, const void* R, float* out, void* workspace, void* stream) {
  W5Plan p;
  const int rc = w5_plan(d, &p);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(L && R && out && workspace, "uz_wgrad5x5: null pointer");
  UZ_REQUIRE(((uintptr_t)L & 15) == 0 && ((uintptr_t)R & 15) == 0, "uz_wgrad5x5: L / R must be 16-byte aligned");
  W5Args a;
  a.L = L, a.R = R, a.slab = static_cast<float*>(workspace);
  a.P = d->N * d->H * d->W, a.H = d->H, a.W = d->W, a.Ci = d->Ci, a.ldl = d->ldl, a.Cj = d->Cj, a.ldr = d->ldr;
  a.ks = d->ksize, a.ntaps = p.ntaps, a.chunk = p.chunk, a.tiles_j = p.tiles_j;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc2 = d->dtype == UZ_BF16 ? w5_launch<bf16_t>(p, a, s) : w5_launch<float>(p, a, s);
  if (rc2 != UZ_OK) return rc2;
  const long long n = (long long)d->CiOut * d->CjOut;
  hipLaunchKernelGGL(wgrad5_reduce_kernel, dim3((unsigned)((n + 255) / 256), p.ntaps), dim3(256), 0, s,
                     static_cast<const float*>(workspace), p.split, p.ntaps, d->Ci, d->Cj, d->CiOut, d->CjOut, out);
  UZ_LAUNCH_CHECK("uz_wgrad5x5(reduce)");
  return UZ_OK;
}

extern "C" int uz_bn_elu_apply(int dtype, const void* x, int ldx, const float* scale, const float* shift, int N, int HW, int C,
                               const void* res, int ldres, void* out, int ldo, void* out2, int ldo2, const float* mask2,
                               int flags, void* stream) {
  UZ_REQUIRE(dtype == UZ_F32 || dtype == UZ_BF16, "uz_bn_elu_apply: bad dtype %d", dtype);
  UZ_REQUIRE(N > 0 && HW > 0 && C > 0 && (long long)N * HW < (1LL << 31), "uz_bn_elu_apply: bad shape");
  UZ_REQUIRE((flags & ~3) == 0, "uz_bn_elu_apply: bad flags %d", flags);
  UZ_REQUIRE(x && scale && shift && out, "uz_bn_elu_apply: null pointer");
  UZ_REQUIRE(ldx >= C && ldo >= C && (res == nullptr || ldres >= C) && (out2 == nullptr || (ldo2 >= C && mask2 != nullptr)),
             "uz_bn_elu_apply: bad leading dimension / missing mask");
  const int lds[4] = {ldx, res ? ldres : 0, ldo, out2 ? ldo2 : 0};
  const int V = be_vec(dtype, C, lds, 4);
  const void* const ptrs[6] = {x, res, out, out2, scale, shift};
  UZ_REQUIRE(V == 1 || be_aligned(ptrs, 6), "uz_bn_elu_apply: tensors read as 16-byte vectors must be 16-byte aligned");
  BeArgs a;
  a.x = x, a.res = res, a.out = out, a.out2 = out2, a.scale = scale, a.shift = shift, a.mask2 = mask2;
  a.ldx = ldx, a.ldres = ldres, a.ldo = ldo, a.ldo2 = ldo2, a.C = C, a.HW = HW, a.flags = flags;
  a.P = (long long)N * HW;
  const dim3 grid(be_grid(a.P * (C / V))), block(256);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == UZ_BF16) {
    if (V == 8) hipLaunchKernelGGL((bn_elu_apply_kernel<bf16_t, 8>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((bn_elu_apply_kernel<bf16_t, 1>), grid, block, 0, s, a);
  } else {
    if (V == 4) hipLaunchKernelGGL((bn_elu_apply_kernel<float, 4>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((bn_elu_apply_kernel<float, 1>), grid, block, 0, s, a);
  }
  UZ_LAUNCH_CHECK("uz_bn_elu_apply");
  return UZ_OK;
}

extern "C" int uz_bn_elu_bwd_rows(const uz_bn_elu_bwd_desc* d) {
  const int rc = bb_check(d, "uz_bn_elu_bwd_rows");
  if (rc != UZ_OK) return rc;
  dim3 grid, block;
  be_reduce_shape(d->C / bb_vec(d), (long long)d->N * d->HW, &grid, &block);
  return (int)grid.x;
}

extern "C" int uz_bn_elu_bwd_reduce(const uz_bn_elu_bwd_desc* d, const void* x, const void* out, const void* g0, const void* g1,
                                    const void* g2, const float* mask2, const float* scale, const float* shift,
                                    const float* mean, const float* invstd, float* partials, void* stream) {
  const int rc = bb_check(d, "uz_bn_elu_bwd_reduce");
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(x && g0 && scale && shift && mean && invstd && partials, "uz_bn_elu_bwd_reduce: null pointer");
  UZ_REQUIRE((g2 == nullptr || mask2 != nullptr) && (!(d->flags & 2) || out != nullptr), "uz_bn_elu_bwd_reduce: missing mask / out");
  UZ_REQUIRE((!(d->flags & 2) || d->ldo >= d->C) && (g1 == nullptr || d->ldg1 >= d->C) && (g2 == nullptr || d->ldg2 >= d->C),
             "uz_bn_elu_bwd_reduce: bad leading dimension of out / g1 / g2");
  {
    const void* const ptrs[5] = {x, (d->flags & 2) ? out : nullptr, g0, g1, g2};
    UZ_REQUIRE(bb_vec(d) == 1 || be_aligned(ptrs, 5), "uz_bn_elu_bwd_reduce: tensors read as 16-byte vectors must be 16-byte aligned");
  }
  BbArgs a = bb_args(d, x, out, g0, g1, g2, mask2, scale, shift, mean, invstd);
  a.partials = partials;
  const int V = bb_vec(d);
  dim3 grid, block;
  be_reduce_shape(d->C / V, a.P, &grid, &block);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d->dtype == UZ_BF16) {
    if (V == 8) hipLaunchKernelGGL((bn_elu_bwd_reduce_kernel<bf16_t, 8>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((bn_elu_bwd_reduce_kernel<bf16_t, 1>), grid, block, 0, s, a);
  } else {
    if (V == 4) hipLaunchKernelGGL((bn_elu_bwd_reduce_kernel<float, 4>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((bn_elu_bwd_reduce_kernel<float, 1>), grid, block, 0, s, a);
  }
  UZ_LAUNCH_CHECK("uz_bn_elu_bwd_reduce");
  return UZ_OK;
}

extern "C" int uz_bn_elu_bwd_apply(const uz_bn_elu_bwd_desc* d, const void* x, const void* out, const void* g0, const void* g1,
                                   const void* g2, const float* mask2, const float* scale, const float* shift,
                                   const float* mean, const float* invstd, const double* sums, void* dx, void* gres,
                                   void* stream) {
  const int rc = bb_check(d, "uz_bn_elu_bwd_apply");
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(x && g0 && scale && shift && mean && invstd && sums && dx, "uz_bn_elu_bwd_apply: null pointer");
  UZ_REQUIRE((g2 == nullptr || mask2 != nullptr) && (!(d->flags & 2) || out != nullptr), "uz_bn_elu_bwd_apply: missing mask / out");
  UZ_REQUIRE(gres == nullptr || d->ldgres >= d->C, "uz_bn_elu_bwd_apply: bad ldgres");
  UZ_REQUIRE((!(d->flags & 2) || d->ldo >= d->C) && (g1 == nullptr || d->ldg1 >= d->C) && (g2 == nullptr || d->ldg2 >= d->C),
             "uz_bn_elu_bwd_apply: bad leading dimension of out / g1 / g2");
  {
    const void* const ptrs[7] = {x, (d->flags & 2) ? out : nullptr, g0, g1, g2, dx, gres};
    UZ_REQUIRE(bb_vec(d) == 1 || be_aligned(ptrs, 7), "uz_bn_elu_bwd_apply: tensors read as 16-byte vectors must be 16-byte aligned");
  }
  BbArgs a = bb_args(d, x, out, g0, g1, g2, mask2, scale, shift, mean, invstd);
  a.sums = sums, a.dx = dx, a.gres = gres;
  const int V = bb_vec(d);
  const dim3 grid(be_grid(a.P * (d->C / V))), block(256);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d->dtype == UZ_BF16) {
    if (V == 8) hipLaunchKernelGGL((bn_elu_bwd_apply_kernel<bf16_t, 8>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((bn_elu_bwd_apply_kernel<bf16_t, 1>), grid, block, 0, s, a);
  } else {
    if (V == 4) hipLaunchKernelGGL((bn_elu_bwd_apply_kernel<float, 4>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((bn_elu_bwd_apply_kernel<float, 1>), grid, block, 0, s, a);
  }
  UZ_LAUNCH_CHECK("uz_bn_elu_bwd_apply");
  return UZ_OK;
}
