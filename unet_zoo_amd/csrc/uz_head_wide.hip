// Wide 1x1 head: K = 1..32 logits as a skinny matrix product on the fp32-input MFMA.
//   uz_head_wide_fwd   out[n][k][hw] = b[k] + sum_c x[p][c] w[k][c]         (N, K, HW) fp32 planes
//   uz_head_wide_bwd   dx[p][c] = sum_k g[n][k][hw] w[k][c]  (stored as T, nullable)
//                      dw[k][c] = sum_p g x,  db[k] = sum_p g                per-workgroup partial rows + a finalize launch
// One arithmetic rule for both dtypes and the three products: exact fp32 products, fp32 accumulation
// (v_mfma_f32_16x16x4_f32); bf16 activations are widened in registers, w and g are never rounded.  This is the arithmetic
// class of the narrow head (uz_outconv_*, fp32 FMA on fp32 weights): only the order of the additions differs.
//
// v_mfma_f32_16x16x4_f32: lane l gives A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; it receives
// D[row = 4 (l >> 4) + r][col = l & 15] in register r.  The reduction index is free as long as A and B agree:
//   forward   rows = classes, cols = pixels; lane quarter q = l >> 4 owns the channels [q S, (q + 1) S), S = C / 4 rounded up
//             to 8, so a lane fetches its pixel's share with 16-byte loads; channels past C are zero on both operands
//   dx        rows = channels, cols = pixels; quarter q owns the classes [q KP / 4, (q + 1) KP / 4), KP = 16 or 32
//   dw        rows = classes, cols = channels; the reduction runs over the pixels of the tile, both operands from LDS
// Workgroups are persistent and walk pixel tiles; the grid is sized from UZ_NUM_CU_HW, never from the CU reserve, so the
// order of the additions (the partial rows of dw / db) does not follow uz_set_cu_reserve.  No float atomics anywhere.
#include "uz_common.h"

namespace {

constexpr int HD_THREADS = 256;
constexpr int HD_TILE = 256;        // forward: pixels per workgroup and trip, 64 per wave = four MFMA column blocks
constexpr int HD_MAXK = 32, HD_MAXC = 512;
constexpr int HD_WG_PER_CU = 2;
constexpr int HD_G_BYTES = HD_MAXK * (HD_TILE + 4) * 4;   // backward: the logit gradients of a tile [KP][TP + 4] fp32
constexpr int HD_X_BYTES = 36864;                         // backward: the activations of a tile [TP][C * sizeof(T) + 16]
constexpr int HD_FIN_GROUPS = 32;

__host__ __device__ inline int hd_span(int C) { return ((C + 3) / 4 + 7) / 8 * 8; }   // channels of one lane quarter
// backward: pixels per tile (a power of two, 16..256) so that the tile's activations fit HD_X_BYTES
__host__ __device__ inline int hd_bwd_tile(int C, int esize) {
  int tp = HD_TILE;
  while (tp * (C * esize + 16) > HD_X_BYTES) tp >>= 1;
  return tp;
}
// backward: the four waves are PG pixel groups x 4 / PG channel groups of at most eight 16-channel blocks
__host__ __device__ inline int hd_bwd_pg(int C) {
  const int nblk = (C + 15) / 16;
  return nblk <= 8 ? 4 : nblk <= 16 ? 2 : 1;
}

__device__ __forceinline__ f32x4 hd_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// LDS traffic inside one wave (the staging tile of the forward): the LDS executes a wave's instructions in order, the fences
// keep the compiler from moving them
__device__ __forceinline__ void hd_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// eight consecutive channels of one pixel as loaded: one 16-byte vector of bf16, two of fp32
template <typename T> struct Raw8 {
  Vec16<T> v[8 / ElemTraits<T>::VEC];
};
// UNCONDITIONAL loads from a clamped address; hd_get() selects the zero afterwards
template <typename T> __device__ __forceinline__ Raw8<T> hd_ld8(const T* row, int ch0, int C) {
  constexpr int VEC = ElemTraits<T>::VEC;
  Raw8<T> r;
#pragma unroll
  for (int h = 0; h < 8 / VEC; ++h) {
    const int c = ch0 + h * VEC;
    r.v[h] = ld16(row + (c < C ? c : 0));
  }
  return r;
}
template <typename T> __device__ __forceinline__ float hd_get(const Raw8<T>& r, int e, bool okp, int ch0, int C) {
  constexpr int VEC = ElemTraits<T>::VEC;
  const float v = (float)r.v[e / VEC].v[e % VEC];
  return (okp && ch0 + e / VEC * VEC < C) ? v : 0.f;   // C % VEC == 0: a vector is inside C or outside
}

// NVR: 8-channel vectors per lane quarter whose weights stay in registers (1, 2: C <= 64); 0: any span, weights in an LDS copy
// laid out [quarter][step / 4][class][4] so that a lane reads four steps of its class with one 16-byte read
template <typename T, int KB, int NVR>
__global__ __launch_bounds__(HD_THREADS) void head_wide_fwd_kernel(const T* __restrict__ x, int ldx, int N, int HW, int C,
                                                                   const float* __restrict__ w, const float* __restrict__ b,
                                                                   int K, float* __restrict__ out) {
  constexpr bool WL = NVR == 0;
  constexpr int KP = KB * 16;
  __shared__ float stage[4][16][64];   // per wave: 16 classes x 64 pixels, columns xor-swizzled by the class quarter
  __shared__ __attribute__((aligned(16))) float wl[WL ? KP * 4 * (HD_MAXC / 4) : 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, j = lane & 15;
  const unsigned P = (unsigned)N * (unsigned)HW;   // < 2^31 (checked on the host)
  const int S = hd_span(C), nv = S / 8;
  const unsigned tiles = (P + HD_TILE - 1) / HD_TILE;

  float wr[KB][WL ? 1 : NVR * 8];
  if constexpr (WL) {
    for (int e = threadIdx.x; e < KP * 4 * S; e += HD_THREADS) {
      const int k = e / (4 * S), r = e - k * 4 * S, qq = r / S, s = r - qq * S;
      const bool ok = k < K && r < C;   // channel qq S + s = r
      const float v = w[ok ? k * C + r : 0];
      wl[((qq * (S / 4) + (s >> 2)) * KP + k) * 4 + (s & 3)] = ok ? v : 0.f;
    }
    __syncthreads();
  } else {
#pragma unroll
    for (int cb = 0; cb < KB; ++cb)
#pragma unroll
      for (int s = 0; s < NVR * 8; ++s) {
        const int k = cb * 16 + j, c = q * S + s;
        const bool ok = k < K && c < C;
        const float v = w[ok ? k * C + c : 0];
        wr[cb][s] = ok ? v : 0.f;
      }
  }
  float bias[KB][4];
#pragma unroll
  for (int cb = 0; cb < KB; ++cb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = cb * 16 + 4 * q + r;
      const float v = b[k < K ? k : 0];
      bias[cb][r] = k < K ? v : 0.f;
    }

  for (unsigned tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const unsigned pw = tile * HD_TILE + wave * 64;   // the wave's 64 consecutive pixels
    f32x4 acc[4][KB];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int cb = 0; cb < KB; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[u][cb][r] = bias[cb][r];
    bool okp[4];
    const T* row[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned p = pw + u * 16 + j;
      okp[u] = p < P;
      row[u] = x + (size_t)(okp[u] ? p : 0u) * ldx;
    }
    if constexpr (!WL) {
      Raw8<T> xr[4][NVR];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < NVR; ++v) xr[u][v] = hd_ld8(row[u], q * S + v * 8, C);
#pragma unroll
      for (int v = 0; v < NVR; ++v)
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float bx = hd_get(xr[u][v], e, okp[u], q * S + v * 8, C);
#pragma unroll
            for (int cb = 0; cb < KB; ++cb) acc[u][cb] = hd_mfma(wr[cb][v * 8 + e], bx, acc[u][cb]);
          }
    } else {
      Raw8<T> cur[4], nxt[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) cur[u] = hd_ld8(row[u], q * S, C);
      for (int v = 0; v < nv; ++v) {
        const int vn = v + 1 < nv ? v + 1 : v;   // the next vector is fetched before this one is multiplied
#pragma unroll
        for (int u = 0; u < 4; ++u) nxt[u] = hd_ld8(row[u], q * S + vn * 8, C);
        f32x4 wv[KB][2];
#pragma unroll
        for (int cb = 0; cb < KB; ++cb)
#pragma unroll
          for (int h = 0; h < 2; ++h)
            wv[cb][h] = *reinterpret_cast<const f32x4*>(&wl[((q * (S / 4) + v * 2 + h) * KP + cb * 16 + j) * 4]);
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float bx = hd_get(cur[u], e, okp[u], q * S + v * 8, C);
#pragma unroll
            for (int cb = 0; cb < KB; ++cb) acc[u][cb] = hd_mfma(wv[cb][e >> 2][e & 3], bx, acc[u][cb]);
          }
#pragma unroll
        for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
      }
    }
    // the accumulator holds 16 pixels x 4 classes per lane quarter; through the wave's LDS tile every class plane is
    // written in one run of 64 consecutive pixels (a tile may straddle images: image and offset per pixel)
    const unsigned p = pw + lane;
    const bool okl = p < P;
    const unsigned pc = okl ? p : 0u;
    const unsigned img = pc / (unsigned)HW, hw = pc - img * (unsigned)HW;
    float* obase = out + (size_t)img * K * HW + hw;
#pragma unroll
    for (int cb = 0; cb < KB; ++cb) {
      hd_wave_sync();
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) stage[wave][4 * q + r][(u * 16 + j) ^ (q << 4)] = acc[u][cb][r];
      hd_wave_sync();
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) {
        const int k = cb * 16 + kk;
        if (k < K) {
          const float v = stage[wave][kk][lane ^ (((kk >> 2) & 3) << 4)];
          if (okl) obase[(size_t)k * HW] = v;
        }
      }
    }
  }
}

__device__ __forceinline__ void hd_store4(float* p, const f32x4& v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ void hd_store4(bf16_t* p, const f32x4& v) {
  bf16x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = (bf16_t)v[i];
  *reinterpret_cast<bf16x4*>(p) = o;
}

// partial[blockIdx.x][k][C + 1]: this workgroup's sums of g x (C values) and of g (1 value), the narrow kernel's scheme
template <typename T, int KB>
__global__ __launch_bounds__(HD_THREADS) void head_wide_bwd_kernel(const T* __restrict__ x, int ldx, int N, int HW, int C,
                                                                   const float* __restrict__ w, int K,
                                                                   const float* __restrict__ g, T* __restrict__ dx, int lddx,
                                                                   float* __restrict__ partial) {
  constexpr int VEC = ElemTraits<T>::VEC;
  constexpr int KP = KB * 16, KQ = KP / 4, KW = KP / 4;   // KQ classes per lane quarter (dx); KW classes per wave (g load)
  __shared__ __attribute__((aligned(16))) char smem[HD_G_BYTES + HD_X_BYTES];
  float* gs = reinterpret_cast<float*>(smem);   // [KP][TP + 4]
  char* xs = smem + HD_G_BYTES;                 // [TP][C * sizeof(T) + 16]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, j = lane & 15;
  const unsigned P = (unsigned)N * (unsigned)HW;   // < 2^31 (checked on the host)
  const int TP = hd_bwd_tile(C, (int)sizeof(T)), GS = TP + 4, XROW = C * (int)sizeof(T) + 16;
  const int PG = hd_bwd_pg(C), pg = wave % PG, cg = wave / PG, TPG = TP / PG;
  const int nblk = (C + 15) / 16, nvec = C / VEC;
  const unsigned tiles = (P + TP - 1) / TP;

  f32x4 acc[KB][8];
#pragma unroll
  for (int cb = 0; cb < KB; ++cb)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[cb][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbacc[KW];
#pragma unroll
  for (int kk = 0; kk < KW; ++kk) dbacc[kk] = 0.f;

  for (unsigned tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const unsigned t0 = tile * TP;
    __syncthreads();   // the tile before has been read
    // -- the tile's logit gradients: wave `wave` fetches the classes kk * 4 + wave, a lane one pixel of a 64-pixel run
    for (int c0 = 0; c0 < TP; c0 += 64) {
      const int px = c0 + lane;
      const unsigned p = t0 + px;
      const bool okp = px < TP && p < P;
      const unsigned pc = okp ? p : 0u;
      const unsigned img = pc / (unsigned)HW, hw = pc - img * (unsigned)HW;
      const float* gb = g + (size_t)img * K * HW + hw;
      float gv[KW];
#pragma unroll
      for (int kk = 0; kk < KW; ++kk) {
        const int k = kk * 4 + wave;
        gv[kk] = gb[(size_t)(k < K ? k : 0) * HW];
      }
#pragma unroll
      for (int kk = 0; kk < KW; ++kk) {
        const int k = kk * 4 + wave;
        const float v = (okp && k < K) ? gv[kk] : 0.f;
        dbacc[kk] += v;
        if (px < TP) gs[k * GS + px] = v;
      }
    }
    // -- the tile's activations, 16-byte vectors, four per thread in flight
    const int total = TP * nvec;
    for (int i0 = 0; i0 < total; i0 += 4 * HD_THREADS) {
      Vec16<T> r[4];
      int pxs[4], vvs[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int idx = i0 + u * HD_THREADS + (int)threadIdx.x;
        const bool in = idx < total;
        const int px = in ? idx / nvec : 0, vv = in ? idx - px * nvec : 0;
        const unsigned p = t0 + px;
        const bool ok = in && p < P;
        r[u] = ld16(x + (size_t)(ok ? p : 0u) * ldx + (ok ? vv * VEC : 0));
        if (!ok) r[u] = zero16<T>();
        pxs[u] = in ? px : -1;
        vvs[u] = vv;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (pxs[u] >= 0) *reinterpret_cast<Vec16<T>*>(xs + pxs[u] * XROW + vvs[u] * 16) = r[u];
    }
    __syncthreads();
    // -- dx: rows = channels, cols = pixels, the reduction over the classes; a lane ends with four consecutive channels
    if (dx != nullptr) {
      for (int m = 0; m < nblk; ++m) {
        float aw[KQ];
        const int ca = m * 16 + j;
#pragma unroll
        for (int s = 0; s < KQ; ++s) {
          const int k = q * KQ + s;
          const bool ok = k < K && ca < C;
          const float v = w[ok ? k * C + ca : 0];
          aw[s] = ok ? v : 0.f;
        }
        for (int st = wave; st < TP / 16; st += 4) {
          f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < KQ; ++s) d = hd_mfma(aw[s], gs[(q * KQ + s) * GS + st * 16 + j], d);
          const unsigned p = t0 + st * 16 + j;
          const int c0 = m * 16 + 4 * q;
          if (p < P && c0 < C) hd_store4(dx + (size_t)p * lddx + c0, d);
        }
      }
    }
    // -- dw: rows = classes, cols = channels, the reduction over this wave's pixels of the tile
    for (int t = 0; t < TPG / 4; ++t) {
      const int px = pg * TPG + 4 * t + q;
      float ga[KB];
#pragma unroll
      for (int cb = 0; cb < KB; ++cb) ga[cb] = gs[(cb * 16 + j) * GS + px];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int mb = cg * 8 + i;
        if (mb < nblk) {
          const int ch = mb * 16 + j;
          const float xv = (float)*reinterpret_cast<const T*>(xs + px * XROW + (ch < C ? ch : 0) * (int)sizeof(T));
          const float bx = ch < C ? xv : 0.f;
#pragma unroll
          for (int cb = 0; cb < KB; ++cb) acc[cb][i] = hd_mfma(ga[cb], bx, acc[cb][i]);
        }
      }
    }
  }
  // -- the waves' accumulators meet in LDS; the pixel groups are added in index order
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);   // [wave][KB][8][16 classes][16 channels]
#pragma unroll
  for (int cb = 0; cb < KB; ++cb)
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(((wave * KB + cb) * 8 + i) * 16 + 4 * q + r) * 16 + j] = acc[cb][i][r];
  __syncthreads();
  float* prow = partial + (size_t)blockIdx.x * K * (C + 1);
  for (int e = threadIdx.x; e < K * C; e += HD_THREADS) {
    const int k = e / C, c = e - k * C;
    const int cb = k >> 4, mb = c >> 4, cgi = mb >> 3, i = mb & 7;
    float s = 0.f;
    for (int pgi = 0; pgi < PG; ++pgi) s += red[((((cgi * PG + pgi) * KB + cb) * 8 + i) * 16 + (k & 15)) * 16 + (c & 15)];
    prow[k * (C + 1) + c] = s;
  }
#pragma unroll
  for (int kk = 0; kk < KW; ++kk) {
    float v = dbacc[kk];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int k = kk * 4 + wave;
    if (lane == 0 && k < K) prow[k * (C + 1) + C] = v;
  }
}

// dw[k][c] = sum_rows partial[row][k][c], db[k] = sum_rows partial[row][k][C]: eight elements per workgroup, 32 threads
// per element; thread g adds its contiguous share of the rows in index order, then thread 0 the 32 shares in index order
__global__ __launch_bounds__(HD_THREADS) void head_wide_finalize_kernel(const float* __restrict__ partial, int rows, int K, int C,
                                                                        float* __restrict__ dw, float* __restrict__ db) {
  __shared__ double sh[HD_FIN_GROUPS][8];
  const int el = threadIdx.x & 7, gi = threadIdx.x >> 3;
  const int ne = K * (C + 1);
  const int e = blockIdx.x * 8 + el;
  const bool in = e < ne;
  const int per = (rows + HD_FIN_GROUPS - 1) / HD_FIN_GROUPS;
  const int r0 = gi * per, r1 = min(rows, r0 + per);
  const float* base = partial + (in ? e : 0);
  double s = 0.0;
  for (int r = r0; r < r1; r += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = base[(size_t)(r + u < r1 ? r + u : 0) * ne];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (r + u < r1) s += (double)v[u];
  }
  sh[gi][el] = s;
  __syncthreads();
  if (gi == 0 && in) {
    double t = 0.0;
    for (int i = 0; i < HD_FIN_GROUPS; ++i) t += sh[i][el];
    const int k = e / (C + 1), c = e - k * (C + 1);
    if (c < C) dw[k * C + c] = (float)t;
    else db[k] = (float)t;
  }
}

int hd_esize(int dtype) { return dtype == UZ_BF16 ? 2 : 4; }
int hd_supported(int dtype, int C, int K) {
  if (dtype != UZ_BF16 && dtype != UZ_F32) return 0;
  const int vec = dtype == UZ_BF16 ? 8 : 4;
  return C > 0 && C % vec == 0 && C <= HD_MAXC && K >= 1 && K <= HD_MAXK;
}
// the grids come from the hardware's CU count, not from uz_num_cu(): the partial rows, and with them the order of the
// additions, must not follow uz_set_cu_reserve
int hd_fwd_grid(long long P) { return (int)min((P + HD_TILE - 1) / HD_TILE, (long long)UZ_NUM_CU_HW * HD_WG_PER_CU); }
int hd_bwd_grid(int dtype, long long P, int C) {
  const int tp = hd_bwd_tile(C, hd_esize(dtype));
  return (int)min((P + tp - 1) / tp, (long long)UZ_NUM_CU_HW * HD_WG_PER_CU);
}

template <typename T, int KB>
void hd_launch_fwd(int grid, hipStream_t s, const void* x, int ldx, int N, int HW, int C, const float* w, const float* b, int K,
                   float* out) {
  const int nv = hd_span(C) / 8;
  if (nv == 1)
    hipLaunchKernelGGL((head_wide_fwd_kernel<T, KB, 1>), dim3(grid), dim3(HD_THREADS), 0, s, (const T*)x, ldx, N, HW, C, w, b, K, out);
  else if (nv == 2)
    hipLaunchKernelGGL((head_wide_fwd_kernel<T, KB, 2>), dim3(grid), dim3(HD_THREADS), 0, s, (const T*)x, ldx, N, HW, C, w, b, K, out);
  else
    hipLaunchKernelGGL((head_wide_fwd_kernel<T, KB, 0>), dim3(grid), dim3(HD_THREADS), 0, s, (const T*)x, ldx, N, HW, C, w, b, K, out);
}

}  // namespace

extern "C" int uz_head_wide_supported(int dtype, int C, int K) { return hd_supported(dtype, C, K); }

extern "C" int uz_head_wide_grid(int dtype, int N, int HW, int C, int K) {
  UZ_REQUIRE(hd_supported(dtype, C, K), "uz_head_wide_grid: dtype=%d C=%d K=%d unsupported (C <= %d, K <= %d)", dtype, C, K,
             HD_MAXC, HD_MAXK);
  UZ_REQUIRE(N > 0 && HW > 0 && (long long)N * HW < (1LL << 31), "uz_head_wide_grid: bad shape");
  return hd_fwd_grid((long long)N * HW);
}

extern "C" int uz_head_wide_fwd(int dtype, const void* x, int ldx, int N, int HW, int C, const float* w, const float* b, int K,
                                float* out, void* stream) {
  UZ_REQUIRE(dtype == UZ_F32 || dtype == UZ_BF16, "uz_head_wide_fwd: bad dtype");
  const int vec = dtype == UZ_BF16 ? 8 : 4;
  UZ_REQUIRE(K >= 1 && K <= HD_MAXK, "uz_head_wide_fwd: K=%d (max %d)", K, HD_MAXK);
  UZ_REQUIRE(C > 0 && C % vec == 0 && C <= HD_MAXC, "uz_head_wide_fwd: C=%d unsupported (a multiple of %d, max %d)", C, vec, HD_MAXC);
  UZ_REQUIRE(x && w && b && out, "uz_head_wide_fwd: null pointer");
  UZ_REQUIRE(ldx >= C && ldx % vec == 0, "uz_head_wide_fwd: ldx=%d (>= C=%d, a multiple of %d)", ldx, C, vec);
  UZ_REQUIRE(N > 0 && HW > 0 && (long long)N * HW < (1LL << 31), "uz_head_wide_fwd: bad shape (N * HW < 2^31)");
  UZ_REQUIRE(((uintptr_t)x & 15) == 0, "uz_head_wide_fwd: x is not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int grid = hd_fwd_grid((long long)N * HW);
  if (dtype == UZ_BF16) {
    if (K > 16) hd_launch_fwd<bf16_t, 2>(grid, s, x, ldx, N, HW, C, w, b, K, out);
    else hd_launch_fwd<bf16_t, 1>(grid, s, x, ldx, N, HW, C, w, b, K, out);
  } else {
    if (K > 16) hd_launch_fwd<float, 2>(grid, s, x, ldx, N, HW, C, w, b, K, out);
    else hd_launch_fwd<float, 1>(grid, s, x, ldx, N, HW, C, w, b, K, out);
  }
  UZ_LAUNCH_CHECK("uz_head_wide_fwd");
  return UZ_OK;
}

extern "C" long long uz_head_wide_bwd_workspace_bytes(int dtype, int N, int HW, int C, int K) {
  UZ_REQUIRE(hd_supported(dtype, C, K), "uz_head_wide_bwd_workspace_bytes: dtype=%d C=%d K=%d unsupported (C <= %d, K <= %d)",
             dtype, C, K, HD_MAXC, HD_MAXK);
  UZ_REQUIRE(N > 0 && HW > 0 && (long long)N * HW < (1LL << 31), "uz_head_wide_bwd_workspace_bytes: bad shape");
  return (long long)hd_bwd_grid(dtype, (long long)N * HW, C) * K * (C + 1) * (long long)sizeof(float);
}

extern "C" int uz_head_wide_bwd(int dtype, const void* x, int ldx, int N, int HW, int C, const float* w, int K, const float* g,
                                void* dx, int lddx, float* dw, float* db, void* workspace, void* stream) {
  UZ_REQUIRE(dtype == UZ_F32 || dtype == UZ_BF16, "uz_head_wide_bwd: bad dtype");
  const int vec = dtype == UZ_BF16 ? 8 : 4;
  UZ_REQUIRE(K >= 1 && K <= HD_MAXK, "uz_head_wide_bwd: K=%d (max %d)", K, HD_MAXK);
  UZ_REQUIRE(C > 0 && C % vec == 0 && C <= HD_MAXC, "uz_head_wide_bwd: C=%d unsupported (a multiple of %d, max %d)", C, vec, HD_MAXC);
  UZ_REQUIRE(x && w && g && dw && db && workspace, "uz_head_wide_bwd: null pointer");
  UZ_REQUIRE(ldx >= C && ldx % vec == 0, "uz_head_wide_bwd: ldx=%d (>= C=%d, a multiple of %d)", ldx, C, vec);
  UZ_REQUIRE(N > 0 && HW > 0 && (long long)N * HW < (1LL << 31), "uz_head_wide_bwd: bad shape (N * HW < 2^31)");
  UZ_REQUIRE(((uintptr_t)x & 15) == 0, "uz_head_wide_bwd: x is not 16-byte aligned");
  if (dx) UZ_REQUIRE(lddx >= C && lddx % vec == 0 && ((uintptr_t)dx & 15) == 0, "uz_head_wide_bwd: bad lddx=%d or dx alignment", lddx);
  hipStream_t s = (hipStream_t)stream;
  const int grid = hd_bwd_grid(dtype, (long long)N * HW, C);
  float* part = (float*)workspace;
  if (dtype == UZ_BF16) {
    if (K > 16)
      hipLaunchKernelGGL((head_wide_bwd_kernel<bf16_t, 2>), dim3(grid), dim3(HD_THREADS), 0, s, (const bf16_t*)x, ldx, N, HW, C, w, K, g, (bf16_t*)dx, lddx, part);
    else
      hipLaunchKernelGGL((head_wide_bwd_kernel<bf16_t, 1>), dim3(grid), dim3(HD_THREADS), 0, s, (const bf16_t*)x, ldx, N, HW, C, w, K, g, (bf16_t*)dx, lddx, part);
  } else {
    if (K > 16)
      hipLaunchKernelGGL((head_wide_bwd_kernel<float, 2>), dim3(grid), dim3(HD_THREADS), 0, s, (const float*)x, ldx, N, HW, C, w, K, g, (float*)dx, lddx, part);
    else
      hipLaunchKernelGGL((head_wide_bwd_kernel<float, 1>), dim3(grid), dim3(HD_THREADS), 0, s, (const float*)x, ldx, N, HW, C, w, K, g, (float*)dx, lddx, part);
  }
  UZ_LAUNCH_CHECK("uz_head_wide_bwd");
  const int ne = K * (C + 1);
  hipLaunchKernelGGL(head_wide_finalize_kernel, dim3(uz_cdiv(ne, 8)), dim3(HD_THREADS), 0, s, part, grid, K, C, dw, db);
  UZ_LAUNCH_CHECK("uz_head_wide_bwd(finalize)");
  return UZ_OK;
}
