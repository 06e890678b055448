// MISSFormer / MiT blocks for gfx950 (reference unet_zoo/models/missformer.py):
//   * spatial-reduction attention  softmax(q k^T * scale) v  with head_dim D (multiples of 8 up to 128), N queries against NK << N reduced
//     keys per image (EfficientSelfAtten :21-39, M_EfficientSelfAtten :113-128): forward, dQ and dK/dV kernels on
//     v_mfma_f32_32x32x16_bf16 (bf16) and a scalar fp32 path for the fp32 run mode;
//   * depthwise 3x3 convolution of MixFFN_skip (DWConv :168-177, "dwconv(fc1) + fc1" :205) forward / input
//     gradient / weight gradient;
//   * exact GELU (nn.GELU(), :196) forward / backward;
//   * space-to-depth (the Conv2d(dim, dim, r, r) of the spatial reduction becomes a GEMM over r*r*C columns);
//   * im2col of the NCHW fp32 network input for OverlapPatchEmbeddings' 7x7 stride-4 convolution (:238-250).
#include <math.h>
#include <stdint.h>

#include "uz_common.h"

namespace {

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

inline int grid_cap(long long units, int per_block, int waves = 16) {
  long long g = (units + per_block - 1) / per_block;
  const long long cap = (long long)UZ_NUM_CU * waves;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// ---------------------------------------------------------------------------------------------
// GELU (erf form): y = x * Phi(x);  backward dx = g * (Phi(x) + x * phi(x))
// ---------------------------------------------------------------------------------------------
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void gelu_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ g, int ldg,
                                                   T* __restrict__ y, int ldy, long long P, int C) {
  constexpr int VEC = ElemTraits<T>::VEC;
  const int CC = C / VEC;
  const long long total = P * CC;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int c0 = (int)(idx % CC) * VEC;
    const long long p = idx / CC;
    float v[VEC], r[VEC];
    load_f(x + (size_t)p * ldx + c0, v);
    if constexpr (BWD) {
      float gv[VEC];
      load_f(g + (size_t)p * ldg + c0, gv);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float cdf = 0.5f * (1.f + erff(v[i] * 0.70710678118654752f));
        const float pdf = 0.3989422804014327f * __expf(-0.5f * v[i] * v[i]);
        r[i] = gv[i] * (cdf + v[i] * pdf);
      }
    } else {
#pragma unroll
      for (int i = 0; i < VEC; ++i) r[i] = 0.5f * v[i] * (1.f + erff(v[i] * 0.70710678118654752f));
    }
    store_f(y + (size_t)p * ldy + c0, r);
  }
}

// ---------------------------------------------------------------------------------------------
// Depthwise 3x3, padding 1, NHWC.  wt is tap-major [9][C] fp32 (the host transposes the (C,1,3,3) parameter).
//   flags bit 0: add the centre input (the "+ fc1_out" of MixFFN_skip, or "+ g" in its gradient)
//   flags bit 1: flipped taps (gradient with respect to the input)
// One thread: 8 consecutive output pixels of a row x one 16-byte channel chunk; the 3 x 10 input vectors it
// needs are each loaded once.
// ---------------------------------------------------------------------------------------------
#ifndef DW_SW
#define DW_SW 6    // pixels per thread; measured on the missformer step (SW, waves/SIMD): (8,1) 2.24 ms, (8,2) 2.03, (6,2) 1.86, (4,3) 4.2 (spills)
#define DW_OCC 2
#endif
template <typename T>
__global__ __launch_bounds__(256, DW_OCC) void dwconv3x3_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ wt,
                                                        const float* __restrict__ bias, T* __restrict__ y, int ldy,
                                                        int N, int H, int W, int C, int flags) {
  constexpr int VEC = ElemTraits<T>::VEC;
  constexpr int SW = DW_SW;
  const int CC = C / VEC, WS = (W + SW - 1) / SW;
  const long long total = (long long)N * H * WS * CC;
  const bool skip = flags & 1, flip = flags & 2;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int c0 = (int)(idx % CC) * VEC;
    long long u = idx / CC;
    const int ws = (int)(u % WS);
    u /= WS;
    const int h = (int)(u % H), n = (int)(u / H);
    float wr[9][VEC];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float* wp = wt + (size_t)(flip ? 8 - t : t) * C + c0;
#pragma unroll
      for (int i = 0; i < VEC; ++i) wr[t][i] = wp[i];
    }
    float bv[VEC], acc[SW][VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) bv[i] = 0.f;
    if (bias != nullptr) {
#pragma unroll
      for (int i = 0; i < VEC; i += 4) *reinterpret_cast<f32x4*>(bv + i) = *reinterpret_cast<const f32x4*>(bias + c0 + i);
    }
#pragma unroll
    for (int o = 0; o < SW; ++o)
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[o][i] = bv[i];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      __builtin_amdgcn_sched_barrier(0);   // one row's loads in flight at a time (three rows at once cost 320 VGPRs)
      const int hh = h + dy - 1;
      const bool rok = (unsigned)hh < (unsigned)H;
      const T* row = x + ((size_t)n * H + (rok ? hh : h)) * W * ldx + c0;
      // all ten loads of the row are issued before the first use: addresses are clamped into the row and the
      // out-of-range vectors zeroed afterwards (a branch per load would serialise their latencies)
      Vec16<T> raw[SW + 2];
#pragma unroll
      for (int j = 0; j < SW + 2; ++j) {
        const int ww = ws * SW - 1 + j;
        raw[j] = ld16(row + (size_t)min(max(ww, 0), W - 1) * ldx);
      }
#pragma unroll
      for (int j = 0; j < SW + 2; ++j) {
        const int ww = ws * SW - 1 + j;
        const bool ok = rok && (unsigned)ww < (unsigned)W;
        __builtin_amdgcn_sched_barrier(0);   // convert one packed vector at a time (all ten at once: +80 VGPRs)
        float v[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) v[i] = ok ? (float)raw[j].v[i] : 0.f;
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) {
          const int o = j - tx;   // output pixel ws*SW + o reads input column (ws*SW + o) + tx - 1
          if (o < 0 || o >= SW) continue;
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[o][i] = fmaf(wr[dy * 3 + tx][i], v[i], acc[o][i]);
          if (skip && dy == 1 && tx == 1) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[o][i] += v[i];
          }
        }
      }
    }
#pragma unroll
    for (int o = 0; o < SW; ++o) {
      const int w = ws * SW + o;
      if (w < W) store_f(y + (((size_t)n * H + h) * W + w) * ldy + c0, acc[o]);
    }
  }
}

// Weight / bias gradient of the depthwise convolution: part[row][10][C], taps 0..8 then the bias; a
// workgroup is (channel chunks) x (pixel segments of 32 along a row); segments are summed in LDS in a
// fixed order, rows by uz_sum_rows_f32.
#ifndef DWG_SEG_PX
#define DWG_SEG_PX 32
#endif
constexpr int DWG_SEG = DWG_SEG_PX;
template <typename T>
__global__ __launch_bounds__(256) void dwconv3x3_wgrad_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ g,
                                                              int ldg, float* __restrict__ part, int N, int H, int W,
                                                              int C, int ccb, int pr) {
  constexpr int VEC = ElemTraits<T>::VEC;
  extern __shared__ float red[];   // [pr][ccb][10][VEC]
  const int CC = C / VEC, WS = (W + DWG_SEG - 1) / DWG_SEG;
  const int lc = threadIdx.x % ccb, ls = threadIdx.x / ccb;
  const int cc = blockIdx.y * ccb + lc;
  const long long seg = (long long)blockIdx.x * pr + ls, nseg = (long long)N * H * WS;
  float acc[10][VEC];
#pragma unroll
  for (int t = 0; t < 10; ++t)
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[t][i] = 0.f;
  if (cc < CC && seg < nseg && ls < pr) {
    const int c0 = cc * VEC;
    const int ws = (int)(seg % WS);
    const long long u = seg / WS;
    const int h = (int)(u % H), n = (int)(u / H);
    const int w0 = ws * DWG_SEG, w1 = min(W, w0 + DWG_SEG);
    // sliding 3x3 window: columns a = w-1, b = w, c = w+1 of rows h-1, h, h+1; every step loads one new
    // column (3 vectors) and one gradient vector instead of nine inputs
    const T* xr[3];
    bool rv[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int hh = h + r - 1;
      rv[r] = (unsigned)hh < (unsigned)H;
      xr[r] = x + ((size_t)n * H + (rv[r] ? hh : h)) * W * ldx + c0;
    }
    auto column = [&](float (&col)[3][VEC], int ww) {   // clamped address + select: the three loads issue together
      const bool cok = (unsigned)ww < (unsigned)W;
      const size_t off = (size_t)min(max(ww, 0), W - 1) * ldx;
      Vec16<T> raw[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) raw[r] = ld16(xr[r] + off);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int i = 0; i < VEC; ++i) col[r][i] = (rv[r] && cok) ? (float)raw[r].v[i] : 0.f;
    };
    const T* gr = g + ((size_t)n * H + h) * W * ldg + c0;
    // (loading column w+2 and the next gradient one pixel ahead of their use was measured slower: 1.56 vs 1.45 ms
    // per missformer step, 217 vs 182 VGPRs)
    auto pixel = [&](const float (&a)[3][VEC], const float (&b)[3][VEC], float (&c)[3][VEC], int w) {
      column(c, w + 1);
      float gv[VEC];
      load_f(gr + (size_t)w * ldg, gv);
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[9][i] += gv[i];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          acc[3 * r + 0][i] = fmaf(gv[i], a[r][i], acc[3 * r + 0][i]);
          acc[3 * r + 1][i] = fmaf(gv[i], b[r][i], acc[3 * r + 1][i]);
          acc[3 * r + 2][i] = fmaf(gv[i], c[r][i], acc[3 * r + 2][i]);
        }
    };
    float A[3][VEC], B[3][VEC], Cc[3][VEC];
    column(A, w0 - 1);
    column(B, w0);
    for (int w = w0; w < w1; w += 3) {
      pixel(A, B, Cc, w);
      if (w + 1 < w1) pixel(B, Cc, A, w + 1);
      if (w + 2 < w1) pixel(Cc, A, B, w + 2);
    }
  }
  if (ls < pr) {
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
      for (int i = 0; i < VEC; ++i) red[((ls * ccb + lc) * 10 + t) * VEC + i] = acc[t][i];
  }
  __syncthreads();
  if (ls == 0 && cc < CC) {
    for (int s = 1; s < pr; ++s)
#pragma unroll
      for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[t][i] += red[((s * ccb + lc) * 10 + t) * VEC + i];
    float* o = part + (size_t)blockIdx.x * 10 * C + cc * VEC;
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
      for (int i = 0; i < VEC; ++i) o[(size_t)t * C + i] = acc[t][i];
  }
}

// ---------------------------------------------------------------------------------------------
// space-to-depth: d[n, ho, wo, (ty*r + tx)*C + c] = s[n, ho*r + ty, wo*r + tx, c] over the H x W fine map, Ho = H / r,
// Wo = W / r (floor: a Conv2d(C, C', r, r) drops the bottom / right border when r does not divide the map).  Inverse:
// the same index map with source and destination exchanged, and zeros written to the dropped border.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void space_to_depth_kernel(const T* __restrict__ src, int lds_, T* __restrict__ dst,
                                                             int ldd, int N, int H, int W, int C, int r, int inverse) {
  constexpr int VEC = ElemTraits<T>::VEC;
  const int CC = C / VEC, Ho = H / r, Wo = W / r;
  const long long total = (long long)N * H * W * CC;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int c0 = (int)(idx % CC) * VEC;
    long long u = idx / CC;
    const int w = (int)(u % W);
    u /= W;
    const int h = (int)(u % H), n = (int)(u / H);
    const bool kept = h < Ho * r && w < Wo * r;
    const size_t fine = ((size_t)n * H + h) * W + w;
    const size_t coarse = ((size_t)n * Ho + (kept ? h / r : 0)) * Wo + (kept ? w / r : 0);
    const int tap = (h % r) * r + (w % r);
    if (inverse) {
      const Vec16<T> v = ld16(src + coarse * lds_ + (size_t)(kept ? tap : 0) * C + c0);
      Vec16<T> z;
#pragma unroll
      for (int i = 0; i < VEC; ++i) z.v[i] = kept ? v.v[i] : (T)0.f;
      st16(dst + fine * ldd + c0, z);
    } else if (kept) {
      st16(dst + coarse * ldd + (size_t)tap * C + c0, ld16(src + fine * lds_ + c0));
    }
  }
}

// im2col of the NCHW fp32 input for a k x k convolution with stride s and zero padding p:
// out[(n, ho, wo)][(kh*k + kw)*C + c], columns >= k*k*C are zero.
template <typename T>
__global__ __launch_bounds__(256) void im2col_nchw_kernel(const float* __restrict__ x, int N, int C, int H, int W, int k,
                                                          int s, int p, int Ho, int Wo, int Kpad, T* __restrict__ out) {
  const int K = k * k * C;
  const long long total = (long long)N * Ho * Wo * Kpad;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int kk = (int)(idx % Kpad);
    const long long pix = idx / Kpad;
    float v = 0.f;
    if (kk < K) {
      const int c = kk % C, tap = kk / C, kh = tap / k, kw = tap - kh * k;
      const int j = (int)(pix % Wo);
      const long long t = pix / Wo;
      const int i = (int)(t % Ho), b = (int)(t / Ho);
      const int hh = i * s + kh - p, ww = j * s + kw - p;
      if ((unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W) v = x[(((size_t)b * C + c) * H + hh) * W + ww];
    }
    out[idx] = (T)v;
  }
}

// out[i] = T(sum_r part[r][i])  (fixed order)
template <typename T>
__global__ __launch_bounds__(256) void sum_parts_kernel(const float* __restrict__ part, int rows, long long n,
                                                        T* __restrict__ out) {
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n;
       i += (long long)gridDim.x * blockDim.x * 4) {
    f32x4 s = *reinterpret_cast<const f32x4*>(part + i);
    for (int r = 1; r < rows; ++r) s += *reinterpret_cast<const f32x4*>(part + (size_t)r * n + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) out[i + e] = (T)s[e];
  }
}

// ---------------------------------------------------------------------------------------------
// Spatial-reduction attention.  q [B][N][ldq], head h = columns h*D .. h*D+D-1 (D = head_dim, a multiple of 8 in
// [8, 128]); keys and values are rows of the kv tensor: key j of image b is row ((j / kps) * B + b) * kps + j % kps
// (kps = NK for one [B][NK] block; the bridge's keys are four blocks of kps rows, one per scale, each stored
// [B][kps]).  lse is kept in log2 units of the scaled scores: p = exp2(s * scale * log2(e) - lse).
// The kernels are templated on T = ceil(D / 32), the number of 32-wide d tiles; D itself is a run-time mask.  Columns
// [D, 32T) are zero in the LDS tiles and in the operand registers, so QK^T contracts over D padded to 16 and the padded
// rows of PV / dV^T / dK^T are computed and never stored.  T = 2, D = 64 runs MISSFormer's arithmetic unchanged.
// ---------------------------------------------------------------------------------------------
struct SraArgs {
  const void *q, *k, *v, *o, *go;   // go: gradient of o (backward)
  void *out, *dq;                   // forward output / dQ
  float *lse, *delta, *ws;          // [B][heads][N] each; ws: dK/dV partials [chunk][kv rows][ldws]
  int B, N, NK, heads, kps, D;
  int ldq, ldk, ldv, ldo, ldgo, lddq, ldws;
  int qc;                            // queries per chunk of the dK/dV kernel
  long long ws_chunk;                // floats per chunk of ws
  float scale;
};

constexpr int SD_MIN = 8, SD_MAX = 128;   // supported head dims: multiples of 8 in [SD_MIN, SD_MAX]

// Shapes per T.  TS: LDS row stride in bf16 elements, 32T + 8 = 64T + 16 bytes = 4T + 1 sixteen-byte bank quads -- odd,
// so the 16-byte row reads of 16 lanes (16 consecutive rows) hit 16 distinct quads (T = 2: 72 elements, 144 B).
template <int T> struct SraShape {
  static constexpr int TS = 32 * T + 8;
  static constexpr int NS = 2 * T;                  // 16-wide contraction slices of QK^T
  static constexpr int CPR = 4 * T;                 // 16-byte chunks per staged row
  static constexpr int CPT = (CPR + 7) / 8;         // ... per staging thread (eight threads per row)
};

__device__ __forceinline__ size_t kv_row(const SraArgs& a, int b, int j) {
  return ((size_t)(j / a.kps) * a.B + b) * a.kps + j % a.kps;
}

typedef short s16x4 __attribute__((ext_vector_type(4)));

// A operand (32 rows d = col0 + l31, 16 contraction indices) of v_mfma_f32_32x32x16_bf16 read TRANSPOSED from a
// row-major [row = contraction index][TS] LDS tile: contraction slots 8*lh + {0..3} are tile rows row0 + {0..3},
// slots 8*lh + {4..7} rows row0 + 8 + {0..3} (row0 already holds the lane half's offset 4*lh) - the order in which
// the 32x32 accumulator of the previous product holds its rows, so that accumulator feeds the B operand as is.
// ds_read_b64_tr_b16: a group of 16 lanes reads a 4-row x 16-column block; lane 4q+p supplies the address of row q,
// columns 4p..4p+3 and lane i receives column i of the four rows.
template <int TS>
__device__ __forceinline__ bf16x8 tr_operand(const bf16_t* tile, int row0, int col0, int lane) {
  const int i = lane & 15, cb = col0 + 16 * ((lane >> 4) & 1);
  const bf16_t* p = tile + (row0 + (i >> 2)) * TS + cb + 4 * (i & 3);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)p);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(p + 8 * TS));
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  const s16x8 both = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, both);
}

template <int TS>
__device__ __forceinline__ bf16x8 row_operand(const bf16_t* tile, int row, int s, int lh) {
  return *reinterpret_cast<const bf16x8*>(tile + row * TS + 16 * s + 8 * lh);
}

__device__ __forceinline__ uint4 ld_u4(const bf16_t* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ uint4 sel_u4(bool ok, const uint4& v) { return ok ? v : make_uint4(0, 0, 0, 0); }

// B operand rows of this lane's query / key straight from global memory: NS slices of 16, zero beyond `valid` and
// beyond column D.  rowp is a valid row either way; every load issues (clamped column) and the mask is a select.
template <int NS>
__device__ __forceinline__ void load_b_operand(const bf16_t* rowp, bool valid, int lh, int D, bf16x8* f) {
  uint4 raw[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) raw[s] = ld_u4(rowp + min(16 * s + 8 * lh, D - 8));
#pragma unroll
  for (int s = 0; s < NS; ++s) asm volatile("" : "+v"(raw[s].x), "+v"(raw[s].y), "+v"(raw[s].z), "+v"(raw[s].w));
#pragma unroll
  for (int s = 0; s < NS; ++s) f[s] = __builtin_bit_cast(bf16x8, sel_u4(valid && 16 * s + 8 * lh < D, raw[s]));
}

// 32 rows of a key / query block into an LDS tile: raw 16-byte chunks fetched with clamped addresses (fetch_rows), the
// mask applied where they are stored (stage_rows); columns [D, 32T) are written as zeros.
template <int T>
__device__ __forceinline__ void fetch_rows(const bf16_t* rowp, int D, int sch, uint4* r) {
#pragma unroll
  for (int i = 0; i < SraShape<T>::CPT; ++i) r[i] = ld_u4(rowp + min(8 * (sch + 8 * i), D - 8));
}
template <int T>
__device__ __forceinline__ void stage_rows(bf16_t* tile, int srow, int sch, bool row_ok, int D, const uint4* r) {
#pragma unroll
  for (int i = 0; i < SraShape<T>::CPT; ++i) {
    const int ch = sch + 8 * i;
    if (ch < SraShape<T>::CPR)
      *reinterpret_cast<uint4*>(tile + srow * SraShape<T>::TS + 8 * ch) = sel_u4(row_ok && 8 * ch < D, r[i]);
  }
}

__device__ __forceinline__ f32x16 zero_acc() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

// store transposed accumulators (rows d of T 32-row tiles, column = this lane's token) as token-major bf16, d < D
template <int T>
__device__ __forceinline__ void store_t_tiles(bf16_t* rowp, int lh, int D, const f32x16* t, float mul) {
#pragma unroll
  for (int dt = 0; dt < T; ++dt)
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const int col = 32 * dt + 8 * q4 + 4 * lh;
      if (col >= D) continue;
      bf16x4 o4;
#pragma unroll
      for (int e = 0; e < 4; ++e) o4[e] = (bf16_t)(t[dt][4 * q4 + e] * mul);
      *reinterpret_cast<bf16x4*>(rowp + col) = o4;
    }
}

template <int T>
__global__ __launch_bounds__(256) void sra_fwd_mfma_kernel(const SraArgs a) {
  using S = SraShape<T>;
  constexpr int TS = S::TS, NS = S::NS;
  __shared__ __attribute__((aligned(16))) bf16_t sK[32 * TS];
  __shared__ __attribute__((aligned(16))) bf16_t sV[32 * TS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const int b = blockIdx.z, h = blockIdx.y, D = a.D;
  const int qi = blockIdx.x * 128 + 32 * w + l31;
  const bf16_t* Q = (const bf16_t*)a.q;
  const bf16_t* K = (const bf16_t*)a.k;
  const bf16_t* V = (const bf16_t*)a.v;
  bf16x8 qf[NS];
  load_b_operand<NS>(Q + ((size_t)b * a.N + min(qi, a.N - 1)) * a.ldq + h * D, qi < a.N, lh, D, qf);
  const int srow = tid >> 3, sch = tid & 7;
  uint4 rk[S::CPT], rv[S::CPT];
  auto fetch = [&](int kb) {
    const size_t row = kv_row(a, b, min(kb * 32 + srow, a.NK - 1));
    fetch_rows<T>(K + row * a.ldk + h * D, D, sch, rk);
    fetch_rows<T>(V + row * a.ldv + h * D, D, sch, rv);
  };
  f32x16 o[T];
#pragma unroll
  for (int t = 0; t < T; ++t) o[t] = zero_acc();
  float m = -INFINITY, l = 0.f;
  const float c = a.scale * 1.4426950408889634f;
  const int nkb = (a.NK + 31) / 32;
  fetch(0);
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();
    const bool kin = kb * 32 + srow < a.NK;
    stage_rows<T>(sK, srow, sch, kin, D, rk);
    stage_rows<T>(sV, srow, sch, kin, D, rv);
    __syncthreads();
    fetch(min(kb + 1, nkb - 1));   // the last block fetches itself again
    f32x16 st = zero_acc();
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if (16 * s < D) st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_operand<TS>(sK, l31, s, lh), qf[s], st, 0, 0, 0);
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const float sv = key < a.NK ? st[r] * c : -INFINITY;
      st[r] = sv;
      mx = fmaxf(mx, sv);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx);   // finite: every block holds at least one real key
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    m = mn;
    l *= alpha;
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
      for (int t = 0; t < T; ++t) o[t][r] *= alpha;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      bf16x8 pf;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bf16_t pb = (bf16_t)__builtin_amdgcn_exp2f(st[8 * s2 + e] - m);
        l += (float)pb;   // normalise by what is actually multiplied
        pf[e] = pb;
      }
#pragma unroll
      for (int t = 0; t < T; ++t)
        o[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_operand<TS>(sV, 16 * s2 + 4 * lh, 32 * t, lane), pf, o[t], 0, 0, 0);
    }
  }
  l += __shfl_xor(l, 32);
  if (qi < a.N) {
    store_t_tiles<T>((bf16_t*)a.out + ((size_t)b * a.N + qi) * a.ldo + h * D, lh, D, o, 1.f / l);
    if (lh == 0) a.lse[((size_t)b * a.heads + h) * a.N + qi] = m + __log2f(l);
  }
}

// dQ (and delta = rowsum(dO * O), kept for the dK/dV kernel): the forward's loop with dP^T = V dO^T,
// dS^T = P^T (dP^T - delta) * scale and dQ^T += K^T dS^T.
template <int T>
__global__ __launch_bounds__(256) void sra_bwd_dq_mfma_kernel(const SraArgs a) {
  using S = SraShape<T>;
  constexpr int TS = S::TS, NS = S::NS;
  __shared__ __attribute__((aligned(16))) bf16_t sK[32 * TS];
  __shared__ __attribute__((aligned(16))) bf16_t sV[32 * TS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const int b = blockIdx.z, h = blockIdx.y, D = a.D;
  const int qi = blockIdx.x * 128 + 32 * w + l31;
  const bool qv = qi < a.N;
  const size_t qrow = (size_t)b * a.N + min(qi, a.N - 1);
  const bf16_t* K = (const bf16_t*)a.k;
  const bf16_t* V = (const bf16_t*)a.v;
  bf16x8 qf[NS], gf[NS], of[NS];
  load_b_operand<NS>((const bf16_t*)a.q + qrow * a.ldq + h * D, qv, lh, D, qf);
  load_b_operand<NS>((const bf16_t*)a.go + qrow * a.ldgo + h * D, qv, lh, D, gf);
  load_b_operand<NS>((const bf16_t*)a.o + qrow * a.ldo + h * D, qv, lh, D, of);
  float delta = 0.f;
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) delta = fmaf((float)gf[s][e], (float)of[s][e], delta);
  delta += __shfl_xor(delta, 32);
  const size_t li = ((size_t)b * a.heads + h) * a.N + min(qi, a.N - 1);
  const float lse = qv ? a.lse[li] : INFINITY;
  if (qv && lh == 0) a.delta[li] = delta;
  const int srow = tid >> 3, sch = tid & 7;
  uint4 rk[S::CPT], rv[S::CPT];
  auto fetch = [&](int kb) {
    const size_t row = kv_row(a, b, min(kb * 32 + srow, a.NK - 1));
    fetch_rows<T>(K + row * a.ldk + h * D, D, sch, rk);
    fetch_rows<T>(V + row * a.ldv + h * D, D, sch, rv);
  };
  f32x16 dq[T];
#pragma unroll
  for (int t = 0; t < T; ++t) dq[t] = zero_acc();
  const float c = a.scale * 1.4426950408889634f;
  const int nkb = (a.NK + 31) / 32;
  fetch(0);
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();
    const bool kin = kb * 32 + srow < a.NK;
    stage_rows<T>(sK, srow, sch, kin, D, rk);
    stage_rows<T>(sV, srow, sch, kin, D, rv);
    __syncthreads();
    fetch(min(kb + 1, nkb - 1));
    f32x16 st = zero_acc(), dp = zero_acc();
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (16 * s >= D) continue;
      st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_operand<TS>(sK, l31, s, lh), qf[s], st, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_operand<TS>(sV, l31, s, lh), gf[s], dp, 0, 0, 0);
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      bf16x8 df;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int r = 8 * s2 + e;
        const int key = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float p = key < a.NK ? __builtin_amdgcn_exp2f(st[r] * c - lse) : 0.f;
        df[e] = (bf16_t)(p * (dp[r] - delta) * a.scale);
      }
#pragma unroll
      for (int t = 0; t < T; ++t)
        dq[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_operand<TS>(sK, 16 * s2 + 4 * lh, 32 * t, lane), df, dq[t], 0, 0, 0);
    }
  }
  if (qv) store_t_tiles<T>((bf16_t*)a.dq + qrow * a.lddq + h * D, lh, D, dq, 1.f);
}

// dK / dV: a wave owns 32 keys (its K and V rows are the B operands for the whole loop) and walks the
// queries of its chunk in blocks of 32 staged in LDS: S = Q K^T and dP = dO V^T with the query as the
// accumulator row, dV^T += dO^T P, dK^T += Q^T dS.  Partials per chunk go to ws, summed by sum_parts_kernel.
template <int T>
__global__ __launch_bounds__(256) void sra_bwd_dkv_mfma_kernel(const SraArgs a) {
  using S = SraShape<T>;
  constexpr int TS = S::TS, NS = S::NS;
  __shared__ __attribute__((aligned(16))) bf16_t sQ[32 * TS];
  __shared__ __attribute__((aligned(16))) bf16_t sG[32 * TS];
  __shared__ float sL[32], sD[32];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const int kgroups = (a.NK + 127) / 128;
  const int b = blockIdx.z, h = blockIdx.y / kgroups, kg = blockIdx.y % kgroups, D = a.D;
  const int kj = kg * 128 + 32 * w + l31;
  const bool kvalid = kj < a.NK;
  const size_t krow = kv_row(a, b, min(kj, a.NK - 1));
  bf16x8 kf[NS], vf[NS];
  load_b_operand<NS>((const bf16_t*)a.k + krow * a.ldk + h * D, kvalid, lh, D, kf);
  load_b_operand<NS>((const bf16_t*)a.v + krow * a.ldv + h * D, kvalid, lh, D, vf);
  const bf16_t* Q = (const bf16_t*)a.q;
  const bf16_t* G = (const bf16_t*)a.go;
  const int q_begin = blockIdx.x * a.qc, q_end = min(a.N, q_begin + a.qc);
  const int srow = tid >> 3, sch = tid & 7;
  uint4 rq[S::CPT], rg[S::CPT];
  float rl, rd;
  auto fetch = [&](int q0) {
    const size_t row = (size_t)b * a.N + min(q0 + srow, q_end - 1);
    fetch_rows<T>(Q + row * a.ldq + h * D, D, sch, rq);
    fetch_rows<T>(G + row * a.ldgo + h * D, D, sch, rg);
    const size_t li = ((size_t)b * a.heads + h) * a.N + min(q0 + (tid & 31), q_end - 1);
    rl = a.lse[li];
    rd = a.delta[li];
  };
  f32x16 dk[T], dv[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    dk[t] = zero_acc();
    dv[t] = zero_acc();
  }
  const float c = a.scale * 1.4426950408889634f;
  const int q_last = q_begin + ((q_end - q_begin - 1) / 32) * 32;
  fetch(q_begin);
  for (int q0 = q_begin; q0 < q_end; q0 += 32) {
    __syncthreads();
    const bool qin = q0 + srow < q_end;
    stage_rows<T>(sQ, srow, sch, qin, D, rq);
    stage_rows<T>(sG, srow, sch, qin, D, rg);
    if (tid < 32) {
      const bool in = q0 + tid < q_end;
      sL[tid] = in ? rl : INFINITY;   // padded query: p = exp2(-inf) = 0
      sD[tid] = in ? rd : 0.f;
    }
    __syncthreads();
    fetch(min(q0 + 32, q_last));
    f32x16 st = zero_acc(), dp = zero_acc();
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (16 * s >= D) continue;
      st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_operand<TS>(sQ, l31, s, lh), kf[s], st, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_operand<TS>(sG, l31, s, lh), vf[s], dp, 0, 0, 0);
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      bf16x8 pf, df;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int r = 8 * s2 + e;
        const int qq = (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float p = kvalid ? __builtin_amdgcn_exp2f(st[r] * c - sL[qq]) : 0.f;
        pf[e] = (bf16_t)p;
        df[e] = (bf16_t)(p * (dp[r] - sD[qq]) * a.scale);
      }
#pragma unroll
      for (int t = 0; t < T; ++t)
        dv[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_operand<TS>(sG, 16 * s2 + 4 * lh, 32 * t, lane), pf, dv[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < T; ++t)
        dk[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_operand<TS>(sQ, 16 * s2 + 4 * lh, 32 * t, lane), df, dk[t], 0, 0, 0);
    }
  }
  if (kvalid) {
    // ws row = the kv row, columns [0, C) dK and [C, 2C) dV with C = heads * D
    float* o = a.ws + (size_t)blockIdx.x * a.ws_chunk + krow * a.ldws + h * D + 4 * lh;
    const int C = a.heads * D;
#pragma unroll
    for (int dt = 0; dt < T; ++dt)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        if (32 * dt + 8 * q4 + 4 * lh >= D) continue;
        f32x4 k4, v4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          k4[e] = dk[dt][4 * q4 + e];
          v4[e] = dv[dt][4 * q4 + e];
        }
        *reinterpret_cast<f32x4*>(o + 32 * dt + 8 * q4) = k4;
        *reinterpret_cast<f32x4*>(o + C + 32 * dt + 8 * q4) = v4;
      }
  }
}

// ---- fp32 run mode: scalar kernels, one query (forward, dQ) or one key (dK/dV) per TPQ threads -------------------
// A thread holds DH = 32T / TPQ of the padded head dims; for T > 2 two neighbouring lanes share a token and add their
// partial dot products with one shuffle (T <= 2: one thread per token, the head dims in order, as before).
constexpr int SF_KB = 32;   // keys (or queries) staged per block
template <int T> struct SraF32 {
  static constexpr int DP = 32 * T;
  static constexpr int TPQ = T > 2 ? 2 : 1;
  static constexpr int DH = DP / TPQ;
};
template <int TPQ> __device__ __forceinline__ float pair_sum(float x) {
  if constexpr (TPQ == 2) return x + __shfl_xor(x, 1);
  return x;
}

// rows [r0, r0 + SF_KB) of a [row][DP] fp32 LDS tile from two token tensors, 16 bytes per load; rows >= nrows and
// columns >= D are zero
template <int DP, int NT, typename RowFn>
__device__ __forceinline__ void stage_f32(float (*s0)[DP], float (*s1)[DP], const float* p0, int ld0, const float* p1,
                                          int ld1, int nrows, int D, RowFn rowof) {
  for (int i = threadIdx.x; i < SF_KB * DP / 4; i += NT) {
    const int j = i / (DP / 4), d = 4 * (i % (DP / 4));
    const size_t row = rowof(min(j, nrows - 1));
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(p0 + row * ld0 + min(d, D - 4));
    const f32x4 v1 = *reinterpret_cast<const f32x4*>(p1 + row * ld1 + min(d, D - 4));
    const bool ok = j < nrows && d < D;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(&s0[j][d]) = ok ? v0 : z;
    *reinterpret_cast<f32x4*>(&s1[j][d]) = ok ? v1 : z;
  }
}

// this thread's DH head dims [d0, d0 + DH) of a token row, zero from column D on (clamped 16-byte loads + select)
template <int DH>
__device__ __forceinline__ void load_row_f32(const float* rowp, int d0, int D, float mul, float* r) {
#pragma unroll
  for (int c = 0; c < DH; c += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(rowp + min(d0 + c, D - 4));
    const bool in = d0 + c < D;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[c + e] = in ? v[e] * mul : 0.f;
  }
}

template <int T>
__global__ __launch_bounds__(128) void sra_fwd_f32_kernel(const SraArgs a) {
  using F = SraF32<T>;
  constexpr int DP = F::DP, TPQ = F::TPQ, DH = F::DH;
  __shared__ float sK[SF_KB][DP], sV[SF_KB][DP];
  const int b = blockIdx.z, h = blockIdx.y, D = a.D;
  const int qi = blockIdx.x * (128 / TPQ) + threadIdx.x / TPQ, d0 = (threadIdx.x % TPQ) * DH;
  const bool qv = qi < a.N;
  const float* qp = (const float*)a.q + ((size_t)b * a.N + min(qi, a.N - 1)) * a.ldq + h * D;
  float q[DH], o[DH];
  load_row_f32<DH>(qp, d0, D, a.scale, q);
#pragma unroll
  for (int d = 0; d < DH; ++d) o[d] = 0.f;
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < a.NK; k0 += SF_KB) {
    __syncthreads();
    stage_f32<DP, 128>(sK, sV, (const float*)a.k + h * D, a.ldk, (const float*)a.v + h * D, a.ldv, a.NK - k0, D,
                       [&](int j) { return kv_row(a, b, k0 + j); });
    __syncthreads();
    const int nk = min(SF_KB, a.NK - k0);
    for (int j = 0; j < nk; ++j) {
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < DH; ++d) s = fmaf(q[d], sK[j][d0 + d], s);
      s = pair_sum<TPQ>(s);
      const float mn = fmaxf(m, s);
      const float alpha = __expf(m - mn), p = __expf(s - mn);
      m = mn;
      l = l * alpha + p;
#pragma unroll
      for (int d = 0; d < DH; ++d) o[d] = fmaf(o[d], alpha, p * sV[j][d0 + d]);
    }
  }
  if (qv) {
    float* op = (float*)a.out + ((size_t)b * a.N + qi) * a.ldo + h * D;
    const float inv = 1.f / l;
#pragma unroll
    for (int d = 0; d < DH; ++d)
      if (d0 + d < D) op[d0 + d] = o[d] * inv;
    if (d0 == 0) a.lse[((size_t)b * a.heads + h) * a.N + qi] = (m + __logf(l)) * 1.4426950408889634f;
  }
}

template <int T>
__global__ __launch_bounds__(128) void sra_bwd_dq_f32_kernel(const SraArgs a) {
  using F = SraF32<T>;
  constexpr int DP = F::DP, TPQ = F::TPQ, DH = F::DH;
  __shared__ float sK[SF_KB][DP], sV[SF_KB][DP];
  const int b = blockIdx.z, h = blockIdx.y, D = a.D;
  const int qi = blockIdx.x * (128 / TPQ) + threadIdx.x / TPQ, d0 = (threadIdx.x % TPQ) * DH;
  const bool qv = qi < a.N;
  const size_t qrow = (size_t)b * a.N + min(qi, a.N - 1);
  const float* qp = (const float*)a.q + qrow * a.ldq + h * D;
  const float* gp = (const float*)a.go + qrow * a.ldgo + h * D;
  const float* op = (const float*)a.o + qrow * a.ldo + h * D;
  float q[DH], g[DH], dq[DH];
  load_row_f32<DH>(qp, d0, D, 1.f, q);
  load_row_f32<DH>(gp, d0, D, 1.f, g);
  float delta = 0.f;
#pragma unroll
  for (int c = 0; c < DH; c += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(op + min(d0 + c, D - 4));
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      dq[c + e] = 0.f;
      delta = fmaf(g[c + e], d0 + c < D ? v[e] : 0.f, delta);
    }
  }
  delta = pair_sum<TPQ>(delta);
  const size_t li = ((size_t)b * a.heads + h) * a.N + min(qi, a.N - 1);
  const float lse = a.lse[li] * 0.6931471805599453f;
  if (qv && d0 == 0) a.delta[li] = delta;
  for (int k0 = 0; k0 < a.NK; k0 += SF_KB) {
    __syncthreads();
    stage_f32<DP, 128>(sK, sV, (const float*)a.k + h * D, a.ldk, (const float*)a.v + h * D, a.ldv, a.NK - k0, D,
                       [&](int j) { return kv_row(a, b, k0 + j); });
    __syncthreads();
    const int nk = min(SF_KB, a.NK - k0);
    for (int j = 0; j < nk; ++j) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < DH; ++d) {
        s = fmaf(q[d], sK[j][d0 + d], s);
        dp = fmaf(g[d], sV[j][d0 + d], dp);
      }
      s = pair_sum<TPQ>(s);
      dp = pair_sum<TPQ>(dp);
      const float ds = __expf(s * a.scale - lse) * (dp - delta) * a.scale;
#pragma unroll
      for (int d = 0; d < DH; ++d) dq[d] = fmaf(ds, sK[j][d0 + d], dq[d]);
    }
  }
  if (qv) {
    float* dp_ = (float*)a.dq + qrow * a.lddq + h * D;
#pragma unroll
    for (int d = 0; d < DH; ++d)
      if (d0 + d < D) dp_[d0 + d] = dq[d];
  }
}

// keys per workgroup of the fp32 dK/dV kernel (64 threads)
inline int sra_f32_kpb(int D) { return D > 64 ? 32 : 64; }

// one key per TPQ threads; blockIdx.x = query chunk; PASS 0: dV, PASS 1: dK (each keeps k and one accumulator row)
template <int T, int PASS>
__global__ __launch_bounds__(64) void sra_bwd_dkv_f32_kernel(const SraArgs a) {
  using F = SraF32<T>;
  constexpr int DP = F::DP, TPQ = F::TPQ, DH = F::DH, KPB = 64 / TPQ;
  __shared__ float sQ[SF_KB][DP], sG[SF_KB][DP], sL[SF_KB], sD[SF_KB];
  const int kgroups = (a.NK + KPB - 1) / KPB, D = a.D;
  const int b = blockIdx.z, h = blockIdx.y / kgroups, kj = (blockIdx.y % kgroups) * KPB + threadIdx.x / TPQ;
  const int d0 = (threadIdx.x % TPQ) * DH;
  const bool kvalid = kj < a.NK;
  const size_t krow = kv_row(a, b, min(kj, a.NK - 1));
  const float* kp = (const float*)a.k + krow * a.ldk + h * D;
  const float* vp = (const float*)a.v + krow * a.ldv + h * D;
  float k[DH], v[DH], acc[DH];
  load_row_f32<DH>(kp, d0, D, 1.f, k);
  if (PASS) load_row_f32<DH>(vp, d0, D, 1.f, v);
#pragma unroll
  for (int d = 0; d < DH; ++d) {
    if (!PASS) v[d] = 0.f;
    acc[d] = 0.f;
  }
  const int q_begin = blockIdx.x * a.qc, q_end = min(a.N, q_begin + a.qc);
  for (int q0 = q_begin; q0 < q_end; q0 += SF_KB) {
    __syncthreads();
    const int nq = min(SF_KB, q_end - q0);
    stage_f32<DP, 64>(sQ, sG, (const float*)a.q + h * D, a.ldq, (const float*)a.go + h * D, a.ldgo, nq, D,
                      [&](int j) { return (size_t)b * a.N + q0 + j; });
    if (threadIdx.x < SF_KB && threadIdx.x < nq) {
      const size_t li = ((size_t)b * a.heads + h) * a.N + q0 + threadIdx.x;
      sL[threadIdx.x] = a.lse[li] * 0.6931471805599453f;
      sD[threadIdx.x] = a.delta[li];
    }
    __syncthreads();
    for (int j = 0; j < nq; ++j) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < DH; ++d) {
        s = fmaf(sQ[j][d0 + d], k[d], s);
        if (PASS) dp = fmaf(sG[j][d0 + d], v[d], dp);
      }
      s = pair_sum<TPQ>(s);
      if (PASS) dp = pair_sum<TPQ>(dp);
      const float p = __expf(s * a.scale - sL[j]);
      if (PASS) {
        const float ds = p * (dp - sD[j]) * a.scale;
#pragma unroll
        for (int d = 0; d < DH; ++d) acc[d] = fmaf(ds, sQ[j][d0 + d], acc[d]);
      } else {
#pragma unroll
        for (int d = 0; d < DH; ++d) acc[d] = fmaf(p, sG[j][d0 + d], acc[d]);
      }
    }
  }
  if (kvalid) {
    float* o = a.ws + (size_t)blockIdx.x * a.ws_chunk + krow * a.ldws + h * D + (PASS ? 0 : a.heads * D);
#pragma unroll
    for (int d = 0; d < DH; ++d)
      if (d0 + d < D) o[d0 + d] = acc[d];
  }
}

int sra_check(const char* fn, const uz_sra_desc* d) {
  UZ_REQUIRE(d != nullptr, "%s: null descriptor", fn);
  UZ_REQUIRE(d->dtype == UZ_F32 || d->dtype == UZ_BF16, "%s: bad dtype", fn);
  const int vec = d->dtype == UZ_BF16 ? 8 : 4;
  UZ_REQUIRE(d->head_dim >= SD_MIN && d->head_dim <= SD_MAX && d->head_dim % 8 == 0,
             "%s: head_dim %d unsupported (the kernels take multiples of 8 from %d to %d)", fn, d->head_dim, SD_MIN, SD_MAX);
  const int kpb = sra_f32_kpb(d->head_dim);
  UZ_REQUIRE(d->B > 0 && d->N > 0 && d->NK > 0 && d->heads > 0 && d->B <= 65535 && d->heads * ((d->NK + kpb - 1) / kpb) <= 65535,
             "%s: bad shape B=%d N=%d NK=%d heads=%d", fn, d->B, d->N, d->NK, d->heads);
  UZ_REQUIRE(d->kps > 0 && d->NK % d->kps == 0, "%s: NK=%d is not a multiple of the segment length %d", fn, d->NK, d->kps);
  const int C = d->heads * d->head_dim;
  UZ_REQUIRE(d->ldq >= C && d->ldk >= C && d->ldv >= C && d->ldo >= C && d->ldq % vec == 0 && d->ldk % vec == 0 &&
                 d->ldv % vec == 0 && d->ldo % vec == 0, "%s: bad leading dimensions", fn);
  UZ_REQUIRE((long long)d->B * d->N < (1LL << 31) && (long long)d->B * d->NK < (1LL << 31), "%s: too many rows", fn);
  return UZ_OK;
}

void sra_fill(const uz_sra_desc* d, SraArgs* a) {
  a->B = d->B; a->N = d->N; a->NK = d->NK; a->heads = d->heads; a->kps = d->kps; a->D = d->head_dim;
  a->ldq = d->ldq; a->ldk = d->ldk; a->ldv = d->ldv; a->ldo = d->ldo;
  a->scale = d->scale;
}

// query chunks of the dK/dV kernel: enough workgroups to fill the chip, chunks of at least 64 queries
void sra_chunks(const uz_sra_desc* d, int* qc, int* nchunks) {
  const int per = d->dtype == UZ_BF16 ? 128 : sra_f32_kpb(d->head_dim);
  const long long base = (long long)d->B * d->heads * ((d->NK + per - 1) / per);
  const int nqb = (d->N + 31) / 32;
  long long want = (4LL * UZ_NUM_CU + base - 1) / base;
  if (want < 1) want = 1;
  if (want > (nqb + 1) / 2) want = (nqb + 1) / 2;
  if (want < 1) want = 1;
  const int blocks = (int)((nqb + want - 1) / want);
  *qc = blocks * 32;
  *nchunks = (d->N + *qc - 1) / *qc;
}

// floats of the delta vector, rounded so the partial tiles that follow stay 64-byte aligned
long long sra_delta_floats(const uz_sra_desc* d) { return (((long long)d->B * d->heads * d->N + 15) / 16) * 16; }

template <int T> void sra_launch_fwd(const uz_sra_desc* d, const SraArgs& a, hipStream_t s) {
  if (d->dtype == UZ_BF16) {
    hipLaunchKernelGGL(sra_fwd_mfma_kernel<T>, dim3((d->N + 127) / 128, d->heads, d->B), dim3(256), 0, s, a);
  } else {
    constexpr int qpb = 128 / SraF32<T>::TPQ;
    hipLaunchKernelGGL(sra_fwd_f32_kernel<T>, dim3((d->N + qpb - 1) / qpb, d->heads, d->B), dim3(128), 0, s, a);
  }
}

template <int T> int sra_launch_bwd(const uz_sra_desc* d, const SraArgs& a, int nchunks, void* dkv, hipStream_t s) {
  if (d->dtype == UZ_BF16) {
    hipLaunchKernelGGL(sra_bwd_dq_mfma_kernel<T>, dim3((d->N + 127) / 128, d->heads, d->B), dim3(256), 0, s, a);
    UZ_LAUNCH_CHECK("uz_sra_bwd(dq)");
    hipLaunchKernelGGL(sra_bwd_dkv_mfma_kernel<T>, dim3(nchunks, d->heads * ((d->NK + 127) / 128), d->B), dim3(256), 0, s, a);
    UZ_LAUNCH_CHECK("uz_sra_bwd(dkv)");
    hipLaunchKernelGGL((sum_parts_kernel<bf16_t>), dim3(grid_cap(a.ws_chunk / 4, 256)), dim3(256), 0, s, a.ws, nchunks, a.ws_chunk, (bf16_t*)dkv);
  } else {
    constexpr int qpb = 128 / SraF32<T>::TPQ, kpb = 64 / SraF32<T>::TPQ;
    hipLaunchKernelGGL(sra_bwd_dq_f32_kernel<T>, dim3((d->N + qpb - 1) / qpb, d->heads, d->B), dim3(128), 0, s, a);
    UZ_LAUNCH_CHECK("uz_sra_bwd(dq)");
    const dim3 gk(nchunks, d->heads * ((d->NK + kpb - 1) / kpb), d->B);
    hipLaunchKernelGGL((sra_bwd_dkv_f32_kernel<T, 0>), gk, dim3(64), 0, s, a);
    hipLaunchKernelGGL((sra_bwd_dkv_f32_kernel<T, 1>), gk, dim3(64), 0, s, a);
    UZ_LAUNCH_CHECK("uz_sra_bwd(dkv)");
    hipLaunchKernelGGL((sum_parts_kernel<float>), dim3(grid_cap(a.ws_chunk / 4, 256)), dim3(256), 0, s, a.ws, nchunks, a.ws_chunk, (float*)dkv);
  }
  UZ_LAUNCH_CHECK("uz_sra_bwd(sum)");
  return UZ_OK;
}

}  // namespace

extern "C" int uz_gelu_fwd(int dtype, const void* x, int ldx, void* y, int ldy, long long P, int C, void* stream) {
  UZ_REQUIRE(dtype == UZ_F32 || dtype == UZ_BF16, "uz_gelu_fwd: bad dtype");
  const int vec = dtype == UZ_BF16 ? 8 : 4;
  UZ_REQUIRE(x && y && P > 0 && C > 0 && C % vec == 0 && ldx % vec == 0 && ldy % vec == 0 && ldx >= C && ldy >= C, "uz_gelu_fwd: bad shape");
  const dim3 grid(grid_cap(P * (C / vec), 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == UZ_BF16) hipLaunchKernelGGL((gelu_kernel<bf16_t, false>), grid, block, 0, s, (const bf16_t*)x, ldx, (const bf16_t*)nullptr, 0, (bf16_t*)y, ldy, P, C);
  else hipLaunchKernelGGL((gelu_kernel<float, false>), grid, block, 0, s, (const float*)x, ldx, (const float*)nullptr, 0, (float*)y, ldy, P, C);
  UZ_LAUNCH_CHECK("uz_gelu_fwd");
  return UZ_OK;
}

extern "C" int uz_gelu_bwd(int dtype, const void* x, int ldx, const void* g, int ldg, void* dx, int lddx, long long P,
                           int C, void* stream) {
  UZ_REQUIRE(dtype == UZ_F32 || dtype == UZ_BF16, "uz_gelu_bwd: bad dtype");
  const int vec = dtype == UZ_BF16 ? 8 : 4;
  UZ_REQUIRE(x && g && dx && P > 0 && C > 0 && C % vec == 0 && ldx % vec == 0 && ldg % vec == 0 && lddx % vec == 0 &&
                 ldx >= C && ldg >= C && lddx >= C, "uz_gelu_bwd: bad shape");
  const dim3 grid(grid_cap(P * (C / vec), 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == UZ_BF16) hipLaunchKernelGGL((gelu_kernel<bf16_t, true>), grid, block, 0, s, (const bf16_t*)x, ldx, (const bf16_t*)g, ldg, (bf16_t*)dx, lddx, P, C);
  else hipLaunchKernelGGL((gelu_kernel<float, true>), grid, block, 0, s, (const float*)x, ldx, (const float*)g, ldg, (float*)dx, lddx, P, C);
  UZ_LAUNCH_CHECK("uz_gelu_bwd");
  return UZ_OK;
}

extern "C" int uz_dwconv3x3(int dtype, const void* x, int ldx, const float* w_taps, const float* bias, void* y, int ldy,
                            int N, int H, int W, int C, int flags, void* stream) {
  UZ_REQUIRE(dtype == UZ_F32 || dtype == UZ_BF16, "uz_dwconv3x3: bad dtype");
  const int vec = dtype == UZ_BF16 ? 8 : 4;
  UZ_REQUIRE(x && w_taps && y && N > 0 && H > 0 && W > 0 && C > 0 && C % vec == 0, "uz_dwconv3x3: bad shape");
  UZ_REQUIRE(ldx % vec == 0 && ldy % vec == 0 && ldx >= C && ldy >= C && (flags & ~3) == 0, "uz_dwconv3x3: bad strides / flags");
  const long long total = (long long)N * H * ((W + DW_SW - 1) / DW_SW) * (C / vec);
  const dim3 grid(grid_cap(total, 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == UZ_BF16) hipLaunchKernelGGL((dwconv3x3_kernel<bf16_t>), grid, block, 0, s, (const bf16_t*)x, ldx, w_taps, bias, (bf16_t*)y, ldy, N, H, W, C, flags);
  else hipLaunchKernelGGL((dwconv3x3_kernel<float>), grid, block, 0, s, (const float*)x, ldx, w_taps, bias, (float*)y, ldy, N, H, W, C, flags);
  UZ_LAUNCH_CHECK("uz_dwconv3x3");
  return UZ_OK;
}

static void dwg_geometry(int dtype, int N, int H, int W, int C, int* ccb, int* pr, int* gx, int* gy) {
  const int CC = C / (dtype == UZ_BF16 ? 8 : 4);
  const int threads = dtype == UZ_BF16 ? 128 : 256;   // 40 KB of staging either way
  *ccb = CC < threads ? CC : threads;
  *pr = threads / *ccb;
  if (*pr > 8) *pr = 8;
  const long long nseg = (long long)N * H * ((W + DWG_SEG - 1) / DWG_SEG);
  *gx = (int)((nseg + *pr - 1) / *pr);
  *gy = (CC + *ccb - 1) / *ccb;
}

extern "C" int uz_dwconv3x3_wgrad_rows(int dtype, int N, int H, int W, int C) {
  int ccb, pr, gx, gy;
  if ((dtype != UZ_F32 && dtype != UZ_BF16) || N <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
  dwg_geometry(dtype, N, H, W, C, &ccb, &pr, &gx, &gy);
  return gx;
}

extern "C" int uz_dwconv3x3_wgrad(int dtype, const void* x, int ldx, const void* g, int ldg, float* part, int N, int H,
                                  int W, int C, void* stream) {
  UZ_REQUIRE(dtype == UZ_F32 || dtype == UZ_BF16, "uz_dwconv3x3_wgrad: bad dtype");
  const int vec = dtype == UZ_BF16 ? 8 : 4;
  UZ_REQUIRE(x && g && part && N > 0 && H > 0 && W > 0 && C > 0 && C % vec == 0, "uz_dwconv3x3_wgrad: bad shape");
  UZ_REQUIRE(ldx % vec == 0 && ldg % vec == 0 && ldx >= C && ldg >= C, "uz_dwconv3x3_wgrad: bad strides");
  int ccb, pr, gx, gy;
  dwg_geometry(dtype, N, H, W, C, &ccb, &pr, &gx, &gy);
  const size_t shm = (size_t)pr * ccb * 10 * vec * sizeof(float);
  UZ_REQUIRE(shm <= 64 * 1024, "uz_dwconv3x3_wgrad: staging exceeds 64 KiB");
  const dim3 grid(gx, gy), block(ccb * pr);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == UZ_BF16) hipLaunchKernelGGL((dwconv3x3_wgrad_kernel<bf16_t>), grid, block, shm, s, (const bf16_t*)x, ldx, (const bf16_t*)g, ldg, part, N, H, W, C, ccb, pr);
  else hipLaunchKernelGGL((dwconv3x3_wgrad_kernel<float>), grid, block, shm, s, (const float*)x, ldx, (const float*)g, ldg, part, N, H, W, C, ccb, pr);
  UZ_LAUNCH_CHECK("uz_dwconv3x3_wgrad");
  return UZ_OK;
}

extern "C" int uz_space_to_depth_crop(int dtype, const void* src, int lds_, void* dst, int ldd, int N, int H, int W,
                                      int C, int r, int inverse, void* stream) {
  UZ_REQUIRE(dtype == UZ_F32 || dtype == UZ_BF16, "uz_space_to_depth: bad dtype");
  const int vec = dtype == UZ_BF16 ? 8 : 4;
  UZ_REQUIRE(src && dst && N > 0 && r > 0 && H >= r && W >= r && C > 0 && C % vec == 0, "uz_space_to_depth: bad shape");
  const int lfine = inverse ? ldd : lds_, lcoarse = inverse ? lds_ : ldd;
  UZ_REQUIRE(lfine % vec == 0 && lcoarse % vec == 0 && lfine >= C && lcoarse >= r * r * C, "uz_space_to_depth: bad strides");
  const long long total = (long long)N * H * W * (C / vec);
  const dim3 grid(grid_cap(total, 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == UZ_BF16) hipLaunchKernelGGL((space_to_depth_kernel<bf16_t>), grid, block, 0, s, (const bf16_t*)src, lds_, (bf16_t*)dst, ldd, N, H, W, C, r, inverse);
  else hipLaunchKernelGGL((space_to_depth_kernel<float>), grid, block, 0, s, (const float*)src, lds_, (float*)dst, ldd, N, H, W, C, r, inverse);
  UZ_LAUNCH_CHECK("uz_space_to_depth");
  return UZ_OK;
}

extern "C" int uz_space_to_depth(int dtype, const void* src, int lds_, void* dst, int ldd, int N, int Ho, int Wo, int C,
                                 int r, int inverse, void* stream) {
  UZ_REQUIRE(Ho > 0 && Wo > 0 && r > 0, "uz_space_to_depth: bad shape");
  return uz_space_to_depth_crop(dtype, src, lds_, dst, ldd, N, Ho * r, Wo * r, C, r, inverse, stream);
}

extern "C" int uz_im2col_nchw(int dtype, const float* x_nchw, int N, int C, int H, int W, int k, int stride, int pad,
                              int Kpad, void* out, void* stream) {
  UZ_REQUIRE(dtype == UZ_F32 || dtype == UZ_BF16, "uz_im2col_nchw: bad dtype");
  UZ_REQUIRE(x_nchw && out && N > 0 && C > 0 && H > 0 && W > 0 && k > 0 && stride > 0 && pad >= 0, "uz_im2col_nchw: bad shape");
  UZ_REQUIRE(H + 2 * pad >= k && W + 2 * pad >= k && Kpad >= k * k * C, "uz_im2col_nchw: bad kernel / Kpad");
  const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  const long long total = (long long)N * Ho * Wo * Kpad;
  const dim3 grid(grid_cap(total, 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == UZ_BF16) hipLaunchKernelGGL((im2col_nchw_kernel<bf16_t>), grid, block, 0, s, x_nchw, N, C, H, W, k, stride, pad, Ho, Wo, Kpad, (bf16_t*)out);
  else hipLaunchKernelGGL((im2col_nchw_kernel<float>), grid, block, 0, s, x_nchw, N, C, H, W, k, stride, pad, Ho, Wo, Kpad, (float*)out);
  UZ_LAUNCH_CHECK("uz_im2col_nchw");
  return UZ_OK;
}

extern "C" int uz_sra_fwd(const uz_sra_desc* d, const void* q, const void* k, const void* v, void* out, float* lse,
                          void* stream) {
  const int rc = sra_check("uz_sra_fwd", d);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(q && k && v && out && lse, "uz_sra_fwd: null pointer");
  SraArgs a{};
  sra_fill(d, &a);
  a.q = q; a.k = k; a.v = v; a.out = out; a.lse = lse;
  hipStream_t s = (hipStream_t)stream;
  switch ((d->head_dim + 31) / 32) {
    case 1: sra_launch_fwd<1>(d, a, s); break;
    case 2: sra_launch_fwd<2>(d, a, s); break;
    case 3: sra_launch_fwd<3>(d, a, s); break;
    default: sra_launch_fwd<4>(d, a, s); break;
  }
  UZ_LAUNCH_CHECK("uz_sra_fwd");
  return UZ_OK;
}

extern "C" long long uz_sra_bwd_workspace_bytes(const uz_sra_desc* d) {
  if (sra_check("uz_sra_bwd_workspace_bytes", d) != UZ_OK) return -1;
  int qc, nchunks;
  sra_chunks(d, &qc, &nchunks);
  // delta [B][heads][N] + partial dK/dV [chunks][kv rows][2C]
  return (sra_delta_floats(d) + (long long)nchunks * d->B * d->NK * 2 * d->heads * d->head_dim) * 4;
}

extern "C" int uz_sra_bwd(const uz_sra_desc* d, const void* q, const void* k, const void* v, const void* o,
                          const float* lse, const void* go, int ldgo, void* dq, int lddq, void* dkv, int lddkv,
                          void* workspace, void* stream) {
  const int rc = sra_check("uz_sra_bwd", d);
  if (rc != UZ_OK) return rc;
  const int vec = d->dtype == UZ_BF16 ? 8 : 4, C = d->heads * d->head_dim;
  UZ_REQUIRE(q && k && v && o && lse && go && dq && dkv && workspace, "uz_sra_bwd: null pointer");
  UZ_REQUIRE(ldgo >= C && lddq >= C && ldgo % vec == 0 && lddq % vec == 0, "uz_sra_bwd: bad gradient strides");
  UZ_REQUIRE(lddkv == 2 * C, "uz_sra_bwd: dkv must be a dense [B * NK][2 * heads * head_dim] tensor (lddkv = %d)", lddkv);
  SraArgs a{};
  sra_fill(d, &a);
  a.q = q; a.k = k; a.v = v; a.o = o; a.go = go; a.dq = dq; a.lse = const_cast<float*>(lse);
  a.ldgo = ldgo; a.lddq = lddq; a.ldws = 2 * C;
  int nchunks;
  sra_chunks(d, &a.qc, &nchunks);
  a.delta = (float*)workspace;
  a.ws = a.delta + sra_delta_floats(d);
  a.ws_chunk = (long long)d->B * d->NK * 2 * C;
  hipStream_t s = (hipStream_t)stream;
  switch ((d->head_dim + 31) / 32) {
    case 1: return sra_launch_bwd<1>(d, a, nchunks, dkv, s);
    case 2: return sra_launch_bwd<2>(d, a, nchunks, dkv, s);
    case 3: return sra_launch_bwd<3>(d, a, nchunks, dkv, s);
    default: return sra_launch_bwd<4>(d, a, nchunks, dkv, s);
  }
}
