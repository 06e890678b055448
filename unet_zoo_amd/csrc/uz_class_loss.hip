// Softmax cross-entropy + soft Dice of several output maps in three launches, whatever the number of maps: partial sums,
// one finalize workgroup, gradient (include/unetzoo_hip.h) -- the multi-class counterpart of uz_region_loss.hip.
// The maps travel by value in the kernel arguments: no table upload, capturable in a hipGraph.  Fixed summation order, no
// atomics, no memset; the workspace is written before it is read in every call.
#include <float.h>
#include "uz_common.h"

namespace {

constexpr int CL_THREADS = 256;
constexpr int CL_RUN = 4;             // pixels of a run: one 16-byte load per class plane ...
// ... and ONE (4-byte loads, a wave still reads 256 contiguous bytes per plane) above 16 classes: four pixels of 32 classes
// are 128 registers of logits beside 96 of sums, and the kernels then spill or run one wave per SIMD
constexpr int cl_run_of(int k) { return k > 16 ? 1 : 4; }
template <int KB> constexpr int cl_run_v = cl_run_of(KB);
// the logits of a run, one class: a vector value, so that the 16-byte load fills it and the 16-byte store takes it as it is
template <int KB> using ClVec = float __attribute__((ext_vector_type(cl_run_of(KB))));
constexpr int CL_MAX_ROWS = 512;      // workgroup rows of one map (all its images) ...
constexpr int CL_MAX_RUNS = 64;       // ... unless a lane would then walk more runs than this (10-bit counters, float sums)
constexpr int CL_FIN_THREADS = 1024;
constexpr int CL_HEAD = 4;            // sum CE terms, sum w_y, valid pixels, labels out of range
constexpr int CL_PER = 5;             // per class: I = sum p [y == c], S = sum p (or p^2), T, TP, P

// Waves per SIMD the register allocation of a class bucket is held to.  __launch_bounds__(256) alone lets the scheduler
// spend all 256 registers (and accumulation registers beyond them) on hoisting every table read and comparison of a pass
// over the classes to its top, which at K >= 16 costs the occupancy the loads need.
constexpr int cl_waves_of(int kb, bool grad) { return kb <= 4 ? 6 : kb <= 9 ? (grad ? 3 : 4) : 2; }

struct ClItems {
  uz_class_item it[UZ_CLASS_MAX_ITEMS];
};

struct ClGeo {
  long long HW, nruns;   // pixels of an image, runs of four (the last may be short)
  int N, K, rows, iters; // workgroup rows per image, runs per lane
  int ignore_index;
  int square;
  float one_m_eps, eps_k;   // 1 - label_smoothing, label_smoothing / K
};

// workgroup -> (map, image, row): blockIdx.x = (item * N + n) * rows + row
__device__ __forceinline__ void cl_where(int N, int rows, int* pair, int* item, int* n, int* row) {
  *pair = (int)blockIdx.x / rows;
  *row = (int)blockIdx.x - *pair * rows;
  *item = *pair / N;
  *n = *pair - *item * N;
}

// Per-class constants of a workgroup live in LDS, not in registers: K weights (and, for the gradient, K coefficient pairs)
// held as wave-uniform values overflow the scalar registers.  tab4[c] = (w_c, u_c, v_c, b_c); classes >= K weigh nothing and
// have b_c = -inf, which added to their (dummy) logits keeps them out of the maximum and makes their exp 0; b_c = 0 otherwise.
// Returns sum_c w_c (fixed order).
template <int KB>
__device__ __forceinline__ float cl_table(float4 (&tab4)[KB], const float* __restrict__ cw, const float* __restrict__ cf, int K) {
  if ((int)threadIdx.x < KB) {
    const int c = threadIdx.x, cc = c < K ? c : 0;
    float w = 1.f, u = 0.f, v = 0.f;
    if (cw != nullptr) w = cw[cc];
    if (cf != nullptr) {
      u = cf[2 + 2 * cc];
      v = cf[3 + 2 * cc];
    }
    tab4[c] = make_float4(c < K ? w : 0.f, u, v, c < K ? 0.f : -INFINITY);
  }
  __syncthreads();
  float wsum = 0.f;
  for (int c = 0; c < KB; ++c) wsum += tab4[c].x;
  return wsum;
}
// An index 0 the compiler cannot see through: a table read at [cl_zero() + c] stays inside the pass over the classes that
// wrote it down -- one broadcast LDS read per class and run -- instead of K (or 3 K) values hoisted into registers.
__device__ __forceinline__ int cl_zero() {
  int z = 0;
  asm volatile("" : "+v"(z));
  return z;
}
// ... and one that exists only once `after` does (the last result of the pass before): the reads of a pass cannot be moved
// in front of the pass before it, where 4 K registers would hold them
__device__ __forceinline__ int cl_zero_after(float after) {
  int z = 0;
  asm volatile("" : "+v"(z) : "v"(after));
  return z;
}

// All loads of one run, unconditional: a lane out of range reads run 0 / pixel 0, a class >= K reads plane K - 1;
// the selects come after every load is issued.  VEC: one 16-byte load per plane; else the same four pixels one by one.
// pm = which of the four pixels exist.
template <int KB, bool VEC>
__device__ __forceinline__ void cl_load(const float* __restrict__ x, const int* __restrict__ y, const ClGeo& g, long long run,
                                        ClVec<KB> (&xv)[KB], int (&yv)[cl_run_v<KB>], bool (&pm)[cl_run_v<KB>]) {
  const bool in = run < g.nruns;
  if (VEC) {
    constexpr int RUN = cl_run_v<KB>;
    typedef float fvec __attribute__((ext_vector_type(RUN)));   // one 16-byte load, not split (K > 16: one float)
    typedef int ivec __attribute__((ext_vector_type(RUN)));
    const long long r = in ? run : 0;
    long long step = g.HW / RUN;                                 // vectors between two class planes
    int kk = g.K;                                                // (compared with K afresh: K lane masks `c < K` kept as
    asm volatile("" : "+s"(kk));                                 // loop invariants spill just the same)
    asm volatile("" : "+s"(step));                               // walked plane by plane: K plane offsets kept as loop
    const fvec* __restrict__ xp = reinterpret_cast<const fvec*>(x) + r;   // invariants are 2 K scalar registers, which spill
#pragma unroll
    for (int c = 0; c < KB; ++c) {
      xv[c] = *xp;
      xp += c + 1 < kk ? step : 0;                              // a class >= K reads the last plane again
    }
    const ivec l = reinterpret_cast<const ivec*>(y)[r];
#pragma unroll
    for (int j = 0; j < RUN; ++j) {
      yv[j] = l[j];
      pm[j] = in;
    }
  } else {
    long long q[cl_run_v<KB>];
#pragma unroll
    for (int j = 0; j < cl_run_v<KB>; ++j) {
      pm[j] = run * cl_run_v<KB> + j < g.HW;   // implies run < nruns
      q[j] = pm[j] ? run * cl_run_v<KB> + j : 0;
    }
    long long step = g.HW;
    int kk = g.K;
    asm volatile("" : "+s"(step));
    asm volatile("" : "+s"(kk));
    const float* __restrict__ xp = x;
#pragma unroll
    for (int c = 0; c < KB; ++c) {
#pragma unroll
      for (int j = 0; j < cl_run_v<KB>; ++j) xv[c][j] = xp[q[j]];
      xp += c + 1 < kk ? step : 0;
    }
#pragma unroll
    for (int j = 0; j < cl_run_v<KB>; ++j) yv[j] = y[q[j]];
  }
}

// The softmax of a run's four pixels in place: x[c][j] <- exp(x[c][j] - max_j); what the loss and the gradient share.
template <int RUN>
struct ClPix {
  float inv[RUN];    // 1 / sum exp, 0 at a pixel that is not valid: every p_c is then 0
  float lse[RUN];    // log sum exp(x - max)
  float zy[RUN];     // x_y - max
  float wy[RUN];     // w_y, 0 at a pixel that is not valid
  float swz[RUN];    // sum_c w_c (x_c - max)
  int pred[RUN];     // argmax (the lowest index among equals), -1 at a pixel that is not valid
  int yy[RUN];       // the label, -1 at a pixel that is not valid
  bool valid[RUN], oor[RUN];
};

template <int KB>
__device__ __forceinline__ void cl_softmax(ClVec<KB> (&xv)[KB], const int (&yv)[cl_run_v<KB>], const bool (&pm)[cl_run_v<KB>], const ClGeo& g,
                                           const float4 (&tab4)[KB], ClPix<cl_run_v<KB>>& r) {
  float m[cl_run_v<KB>], sum[cl_run_v<KB>];
  const int z0 = cl_zero();
#pragma unroll
  for (int j = 0; j < cl_run_v<KB>; ++j) {
    const bool inr = yv[j] >= 0 && yv[j] < g.K, ign = yv[j] == g.ignore_index;
    r.valid[j] = pm[j] && inr && !ign;
    r.oor[j] = pm[j] && !inr && !ign;
    r.yy[j] = r.valid[j] ? yv[j] : -1;
    m[j] = xv[0][j];
    r.pred[j] = 0;
    sum[j] = 0.f;
    r.zy[j] = 0.f;
    r.wy[j] = 0.f;
    r.swz[j] = 0.f;
  }
#pragma unroll
  for (int c = 1; c < KB; ++c) {
    const float bc = tab4[z0 + c].w;
#pragma unroll
    for (int j = 0; j < cl_run_v<KB>; ++j) {
      xv[c][j] += bc;
      const bool up = xv[c][j] > m[j];
      m[j] = up ? xv[c][j] : m[j];
      r.pred[j] = up ? c : r.pred[j];
    }
  }
  const int z1 = cl_zero_after(m[0]);
#pragma unroll
  for (int c = 0; c < KB; ++c) {
    const float wc = tab4[z1 + c].x;
#pragma unroll
    for (int j = 0; j < cl_run_v<KB>; ++j) {
      const float z = xv[c][j] - m[j];
      const float e = __expf(z);   // z <= 0: the absolute error of exp2(z log2 e) stays below 2e-7
      sum[j] += e;
      const bool is = r.yy[j] == c;
      r.zy[j] = is ? z : r.zy[j];
      r.wy[j] = is ? wc : r.wy[j];
      r.swz[j] = fmaf(wc, fmaxf(z, -FLT_MAX), r.swz[j]);   // a class >= K: 0 * -FLT_MAX, not 0 * -inf
      xv[c][j] = e;
    }
  }
#pragma unroll
  for (int j = 0; j < cl_run_v<KB>; ++j) {
    r.inv[j] = r.valid[j] ? 1.f / sum[j] : 0.f;
    r.lse[j] = logf(sum[j]);
    r.pred[j] = r.valid[j] ? r.pred[j] : -1;
  }
}

// The same labels behind an empty asm: the comparisons y == c of one pass over the classes are then not kept (K x 4 lane
// masks in scalar registers, which spill) for the next pass but formed again, one v_cmp each.
template <int RUN>
__device__ __forceinline__ void cl_opaque(const int (&a)[RUN], int (&b)[RUN]) {
#pragma unroll
  for (int j = 0; j < RUN; ++j) {
    b[j] = a[j];
    asm volatile("" : "+v"(b[j]));
  }
}

// part[blockIdx.x][CL_HEAD + CL_PER * K] (doubles)
template <int KB, bool VEC>
__global__ __launch_bounds__(CL_THREADS) __attribute__((amdgpu_waves_per_eu(cl_waves_of(KB, false)))) void class_partial_kernel(const ClItems tab, const ClGeo g, const int* __restrict__ labels,
                                                                   const float* __restrict__ cw, double* __restrict__ part) {
  int pair, item, n, row;
  cl_where(g.N, g.rows, &pair, &item, &n, &row);
  const float* __restrict__ x = tab.it[item].logits + (size_t)n * g.K * g.HW;
  const int* __restrict__ y = labels + (size_t)n * g.HW;
  __shared__ float4 tab4[KB];
  const float wsum = cl_table<KB>(tab4, cw, nullptr, g.K);
  double ce = 0.0, wacc = 0.0;
  float S[KB], I[KB];
  unsigned cnt[KB];        // T | P << 10 | TP << 20: at most 4 * CL_MAX_RUNS = 256 pixels per lane
  unsigned head = 0;       // valid | out of range << 16
#pragma unroll
  for (int c = 0; c < KB; ++c) {
    S[c] = 0.f;
    I[c] = 0.f;
    cnt[c] = 0u;
  }
  for (int it = 0; it < g.iters; ++it) {
    const long long run = ((long long)it * g.rows + row) * CL_THREADS + threadIdx.x;
    ClVec<KB> xv[KB];
    int yv[cl_run_v<KB>];
    bool pm[cl_run_v<KB>];
    cl_load<KB, VEC>(x, y, g, run, xv, yv, pm);
    ClPix<cl_run_v<KB>> r;
    cl_softmax<KB>(xv, yv, pm, g, tab4, r);
    unsigned code_y[cl_run_v<KB>];
    int y2[cl_run_v<KB>];
    cl_opaque(r.yy, y2);
#pragma unroll
    for (int j = 0; j < cl_run_v<KB>; ++j) {
      const float term = g.one_m_eps * r.wy[j] * (r.lse[j] - r.zy[j]) + g.eps_k * (r.lse[j] * wsum - r.swz[j]);
      ce += (double)(r.valid[j] ? term : 0.f);
      wacc += (double)r.wy[j];
      head += (r.valid[j] ? 1u : 0u) + (r.oor[j] ? 1u << 16 : 0u);
      code_y[j] = 1u + (r.pred[j] == r.yy[j] ? 1u << 20 : 0u);
    }
#pragma unroll
    for (int c = 0; c < KB; ++c) {
#pragma unroll
      for (int j = 0; j < cl_run_v<KB>; ++j) {
        const float p = xv[c][j] * r.inv[j];
        S[c] += g.square ? p * p : p;
        const bool is = y2[j] == c;
        I[c] += is ? p : 0.f;
        cnt[c] += (is ? code_y[j] : 0u) + (r.pred[j] == c ? 1u << 10 : 0u);
      }
      }
  }
  // a lane's sums become doubles here; fixed trees from here on
  __shared__ double red[CL_THREADS / 64][CL_HEAD + CL_PER * KB];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  {
    double a = ce, b = wacc;
    long long h = (long long)(head & 0xffffu) | (long long)(head >> 16) << 32;
    for (int o = 32; o > 0; o >>= 1) {
      a += __shfl_down(a, o);
      b += __shfl_down(b, o);
      h += __shfl_down(h, o);
    }
    if (lane == 0) {
      red[wv][0] = a;
      red[wv][1] = b;
      red[wv][2] = (double)(h & 0xffffffffLL);
      red[wv][3] = (double)(h >> 32);
    }
  }
#pragma unroll
  for (int c = 0; c < KB; ++c) {
    if (c < g.K) {   // uniform
      double a = (double)I[c], b = (double)S[c];
      long long k = (long long)(cnt[c] & 1023u) | (long long)((cnt[c] >> 10) & 1023u) << 21 | (long long)(cnt[c] >> 20) << 42;
      for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o);
        b += __shfl_down(b, o);
        k += __shfl_down(k, o);
      }
      if (lane == 0) {
        double* r = &red[wv][CL_HEAD + CL_PER * c];
        r[0] = a;
        r[1] = b;
        r[2] = (double)(k & 0x1fffffLL);           // T
        r[3] = (double)(k >> 42);                  // TP
        r[4] = (double)((k >> 21) & 0x1fffffLL);   // P
      }
    }
    __builtin_amdgcn_sched_barrier(0);   // one class after the other: interleaved, the trees of all classes are live at once
  }
  __syncthreads();
  const int cols = CL_HEAD + CL_PER * g.K;
  if ((int)threadIdx.x < cols) {
    double v = 0.0;
    for (int q = 0; q < CL_THREADS / 64; ++q) v += red[q][threadIdx.x];
    part[(size_t)blockIdx.x * cols + threadIdx.x] = v;
  }
}

// One workgroup.  (1) tot[pair][col] = the pair's rows added in row order; (2) per (map, group, class) the Dice term and
// the coefficients, per map the cross-entropy, of the metric map the counts -- every thread adds its shares in a fixed
// order and a fixed tree over the workgroup totals them.  coef[pair] = (weight w_ce / W, 0, then (u_c, v_c) per class).
__global__ __launch_bounds__(CL_FIN_THREADS) void class_finalize_kernel(const ClItems tab, const uz_class_desc d, int rows,
                                                                        const double* __restrict__ part, double* __restrict__ tot,
                                                                        float* __restrict__ coef, float* __restrict__ out,
                                                                        long long* __restrict__ counts) {
  __shared__ double red[CL_FIN_THREADS / 64][3];
  const int K = d.K, N = d.N, cols = CL_HEAD + CL_PER * K, cs = 2 * K + 2;
  const long long ncol = (long long)d.n_items * N * cols;
  for (long long j = threadIdx.x; j < ncol; j += CL_FIN_THREADS) {
    const long long pair = j / cols;
    const int col = (int)(j - pair * cols);
    const double* __restrict__ p = part + (size_t)pair * rows * cols + col;
    double s = 0.0;
    int r = 0;
    for (; r + 7 < rows; r += 8) {   // eight loads in flight, added in row order
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(r + u) * cols];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; r < rows; ++r) s += p[(size_t)r * cols];
    tot[j] = s;
  }
  __syncthreads();   // tot is read below by other threads of this workgroup
  const bool batch = d.reduce == UZ_CLASS_REDUCE_BATCH;
  const int G = batch ? 1 : N, c0 = d.include_background ? 0 : 1, nC = K - c0;
  const double sm = (double)d.smooth;
  double acc[3] = {0.0, 0.0, 0.0};   // loss; of the metric map: sum of the class Dice values, number of classes counted
  const long long jobs = (long long)d.n_items * G * K;
  for (long long j = threadIdx.x; j < jobs; j += CL_FIN_THREADS) {
    const int item = (int)(j / ((long long)G * K));
    const int rem = (int)(j - (long long)item * G * K);
    const int gi = rem / K, c = rem - gi * K;
    const int n0 = batch ? 0 : gi, n1 = batch ? N : gi + 1;
    double I = 0.0, S = 0.0, T = 0.0;
    for (int n = n0; n < n1; ++n) {
      const double* __restrict__ r = tot + ((size_t)item * N + n) * cols + CL_HEAD + CL_PER * c;
      I += r[0];
      S += r[1];
      T += r[2];
    }
    float u = 0.f, v = 0.f;
    if (c >= c0) {
      const double scale = (double)tab.it[item].weight * (double)d.w_dice / ((double)G * (double)nC);
      const double den = S + T + sm, num = 2.0 * I + sm;
      acc[0] += scale * ((S + T - 2.0 * I) / den);   // 1 - num / den without the cancellation
      u = (float)(-2.0 * scale / den);
      v = (float)(scale * num / (den * den));
    }
    for (int n = n0; n < n1; ++n) {
      float* __restrict__ cf = coef + ((size_t)item * N + n) * cs + 2 + 2 * c;
      cf[0] = u;
      cf[1] = v;
    }
  }
  for (int item = threadIdx.x; item < d.n_items; item += CL_FIN_THREADS) {
    double num = 0.0, W = 0.0;
    for (int n = 0; n < N; ++n) {
      const double* __restrict__ r = tot + ((size_t)item * N + n) * cols;
      num += r[0];
      W += r[1];
    }
    const double wc = (double)tab.it[item].weight * (double)d.w_ce;
    const bool any = W > 0.0;                  // no valid pixel: CE = 0 with zero gradient
    if (any) acc[0] += wc * (num / W);
    const float cew = any ? (float)(wc / W) : 0.f;
    for (int n = 0; n < N; ++n) {
      float* __restrict__ cf = coef + ((size_t)item * N + n) * cs;
      cf[0] = cew;
      cf[1] = 0.f;
    }
  }
  for (int c = threadIdx.x; c < K; c += CL_FIN_THREADS) {
    double T = 0.0, TP = 0.0, P = 0.0, valid = 0.0, oor = 0.0;
    for (int n = 0; n < N; ++n) {
      const double* __restrict__ r = tot + ((size_t)d.metric_item * N + n) * cols;
      T += r[CL_HEAD + CL_PER * c + 2];
      TP += r[CL_HEAD + CL_PER * c + 3];
      P += r[CL_HEAD + CL_PER * c + 4];
      valid += r[2];
      oor += r[3];
    }
    if (c >= c0 && P + T > 0.0) {
      acc[1] += 2.0 * TP / (P + T);
      acc[2] += 1.0;
    }
    if (counts != nullptr) {
      counts[3 * c + 0] = (long long)TP;
      counts[3 * c + 1] = (long long)P;
      counts[3 * c + 2] = (long long)T;
      if (c == 0) {
        counts[3 * K + 0] = (long long)valid;
        counts[3 * K + 1] = (long long)N * d.HW - (long long)valid - (long long)oor;
        counts[3 * K + 2] = (long long)oor;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double v = acc[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double v[3] = {0.0, 0.0, 0.0};
    for (int q = 0; q < CL_FIN_THREADS / 64; ++q)
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] += red[q][k];
    out[0] = (float)v[0];
    out[1] = v[2] == 0.0 ? 1.f : (float)(v[1] / v[2]);
  }
}

template <int KB, bool VEC>
__global__ __launch_bounds__(CL_THREADS) __attribute__((amdgpu_waves_per_eu(cl_waves_of(KB, true)))) void class_grad_kernel(const ClItems tab, const ClGeo g, const int* __restrict__ labels,
                                                                const float* __restrict__ cw, const float* __restrict__ coef) {
  int pair, item, n, row;
  cl_where(g.N, g.rows, &pair, &item, &n, &row);
  float* __restrict__ dl = tab.it[item].dlogits;
  if (dl == nullptr) return;   // the whole workgroup: a map without a gradient
  dl += (size_t)n * g.K * g.HW;
  const float* __restrict__ x = tab.it[item].logits + (size_t)n * g.K * g.HW;
  const int* __restrict__ y = labels + (size_t)n * g.HW;
  __shared__ float4 tab4[KB];
  const float* __restrict__ cf = coef + (size_t)pair * (2 * g.K + 2);
  const float cew = cf[0];
  const float wsum = cl_table<KB>(tab4, cw, cf, g.K);
  for (int it = 0; it < g.iters; ++it) {
    const long long run = ((long long)it * g.rows + row) * CL_THREADS + threadIdx.x;
    ClVec<KB> xv[KB];
    int yv[cl_run_v<KB>];
    bool pm[cl_run_v<KB>];
    cl_load<KB, VEC>(x, y, g, run, xv, yv, pm);
    ClPix<cl_run_v<KB>> r;
    cl_softmax<KB>(xv, yv, pm, g, tab4, r);
    // g_c = d(loss)/d(p_c) = u_c [y == c] + v_c (square: 2 p_c v_c); dlogits_k = p_k (g_k - sum_c p_c g_c) + CE part
    const float sq2 = g.square ? 2.f : 0.f, sq1 = g.square ? 0.f : 1.f;   // d S / d p = 2 p (square) or 1, without a lane mask
    float dot[cl_run_v<KB>], A[cl_run_v<KB>];
    int y2[cl_run_v<KB>], y3[cl_run_v<KB>];
    cl_opaque(r.yy, y2);
    cl_opaque(r.yy, y3);
    const int z2 = cl_zero_after(r.inv[0]);
#pragma unroll
    for (int j = 0; j < cl_run_v<KB>; ++j) {
      dot[j] = 0.f;
      A[j] = g.one_m_eps * r.wy[j] + g.eps_k * wsum;   // sum_c a_c
    }
#pragma unroll
    for (int c = 0; c < KB; ++c) {
      const float4 t4 = tab4[z2 + c];
      const float cu = t4.y, cv = t4.z;
#pragma unroll
      for (int j = 0; j < cl_run_v<KB>; ++j) {
        const float p = xv[c][j] * r.inv[j];
        const float gc = (y2[j] == c ? cu : 0.f) + cv * fmaf(sq2, p, sq1);
        dot[j] = fmaf(p, gc, dot[j]);
        xv[c][j] = p;
      }
      }
    const int z3 = cl_zero_after(dot[0]);
#pragma unroll
    for (int c = 0; c < KB; ++c) {
      const float4 t4 = tab4[z3 + c];
      const float wc = t4.x, cu = t4.y, cv = t4.z;
#pragma unroll
      for (int j = 0; j < cl_run_v<KB>; ++j) {
        const float p = xv[c][j];
        const bool is = y3[j] == c;
        const float gc = (is ? cu : 0.f) + cv * fmaf(sq2, p, sq1);
        const float a = wc * ((is ? g.one_m_eps : 0.f) + g.eps_k);
        const float v = p * (gc - dot[j]) + cew * (p * A[j] - a);
        xv[c][j] = y3[j] >= 0 ? v : 0.f;   // exactly 0 at a pixel that is not valid (yy = -1)
      }
      }
    // the results exist here, whatever lanes store them: left alone, the compiler sinks each pixel's whole computation into
    // the conditional store blocks below and keeps every table value alive across all of them
#pragma unroll
    for (int c = 0; c < KB; ++c) {
      if constexpr (cl_run_v<KB> == 1) {
        float t = xv[c][0];
        asm volatile("" : "+v"(t));
        xv[c][0] = t;
      } else {
        asm volatile("" : "+v"(xv[c]));
      }
    }
    long long step = VEC ? g.HW / cl_run_v<KB> : g.HW;
    int kk = g.K;
    asm volatile("" : "+s"(step));
    asm volatile("" : "+s"(kk));
    if (VEC) {
      if (run < g.nruns) {
        typedef float fvec __attribute__((ext_vector_type(cl_run_v<KB>)));
        fvec* __restrict__ dp = reinterpret_cast<fvec*>(dl) + run;
#pragma unroll
        for (int c = 0; c < KB; ++c)
          if (c < kk) {
            *dp = xv[c];
            dp += step;
          }
      }
    } else {
#pragma unroll
      for (int j = 0; j < cl_run_v<KB>; ++j)
        if (pm[j]) {
          float* __restrict__ dp = dl + run * cl_run_v<KB> + j;
#pragma unroll
          for (int c = 0; c < KB; ++c)
            if (c < kk) {
              *dp = xv[c][j];
              dp += step;
            }
        }
    }
  }
}

struct ClPlan {
  ClGeo g;
  int pairs;   // n_items * N
  int cols;    // doubles of a row
};

int cl_plan(const char* fn, const uz_class_desc* d, ClPlan* p) {
  UZ_REQUIRE(d != nullptr, "%s: null descriptor", fn);
  UZ_REQUIRE(d->n_items >= 1 && d->n_items <= UZ_CLASS_MAX_ITEMS, "%s: n_items = %d outside [1, %d]", fn, d->n_items,
             UZ_CLASS_MAX_ITEMS);
  UZ_REQUIRE(d->K >= 2 && d->K <= UZ_CLASS_MAX_K, "%s: K = %d outside [2, %d]", fn, d->K, UZ_CLASS_MAX_K);
  UZ_REQUIRE(d->N > 0 && d->HW > 0, "%s: N = %d, HW = %lld", fn, d->N, d->HW);
  UZ_REQUIRE(d->N <= (1 << 20), "%s: N = %d above 2^20", fn, d->N);
  UZ_REQUIRE(d->metric_item >= 0 && d->metric_item < d->n_items, "%s: metric_item = %d outside [0, %d)", fn, d->metric_item,
             d->n_items);
  // written so that a NaN is refused too
  UZ_REQUIRE(d->smooth > 0.f && d->smooth < INFINITY, "%s: smooth must be positive", fn);
  UZ_REQUIRE(d->label_smoothing >= 0.f && d->label_smoothing < 1.f, "%s: label_smoothing must be in [0, 1)", fn);
  UZ_REQUIRE(d->w_ce >= 0.f && d->w_ce < INFINITY && d->w_dice >= 0.f && d->w_dice < INFINITY,
             "%s: w_ce and w_dice must be >= 0", fn);
  UZ_REQUIRE(d->w_ce > 0.f || d->w_dice > 0.f, "%s: w_ce and w_dice are both zero", fn);
  UZ_REQUIRE(d->reduce == UZ_CLASS_REDUCE_BATCH || d->reduce == UZ_CLASS_REDUCE_IMAGE, "%s: reduce = %d is neither batch nor image",
             fn, d->reduce);
  ClGeo& g = p->g;
  g.HW = d->HW;
  const int run = cl_run_of(d->K <= 2 ? 2 : d->K <= 4 ? 4 : d->K <= 9 ? 9 : d->K <= 16 ? 16 : 32);   // the bucket's, as uz_class_loss picks it
  g.nruns = (d->HW + run - 1) / run;
  g.N = d->N;
  g.K = d->K;
  long long rows = (g.nruns + CL_THREADS - 1) / CL_THREADS;   // one run per lane ...
  const long long cap = CL_MAX_ROWS / d->N > 0 ? CL_MAX_ROWS / d->N : 1;   // ... until the map has CL_MAX_ROWS rows (per map, so
  if (rows > cap) rows = cap;                                             // that its rows do not depend on the other maps)
  const long long need = (g.nruns + (long long)CL_THREADS * CL_MAX_RUNS - 1) / ((long long)CL_THREADS * CL_MAX_RUNS);
  if (rows < need) rows = need;                                           // a lane walks at most CL_MAX_RUNS runs
  p->pairs = d->n_items * d->N;
  UZ_REQUIRE((long long)p->pairs * rows < (1LL << 30), "%s: %d images of %lld pixels are too many", fn, p->pairs, d->HW);
  g.rows = (int)rows;
  g.iters = (int)((g.nruns + rows * CL_THREADS - 1) / (rows * CL_THREADS));
  g.ignore_index = d->ignore_index;
  g.square = d->square != 0;
  g.one_m_eps = 1.f - d->label_smoothing;
  g.eps_k = d->label_smoothing / (float)d->K;
  p->cols = CL_HEAD + CL_PER * d->K;
  return UZ_OK;
}

// rows | totals (doubles), then the coefficients (floats)
long long cl_doubles(const ClPlan& p) { return (long long)p.pairs * (p.g.rows + 1) * p.cols; }

template <int KB, bool VEC>
int cl_launch(const ClPlan& p, const uz_class_desc* d, const ClItems& tab, const int* labels, const float* cw, float* out2,
              long long* counts, void* workspace, bool grad, hipStream_t s) {
  double* part = (double*)workspace;
  double* tot = part + (size_t)p.pairs * p.g.rows * p.cols;
  float* coef = (float*)(part + cl_doubles(p));
  const dim3 grid((unsigned)(p.pairs * p.g.rows));
  hipLaunchKernelGGL((class_partial_kernel<KB, VEC>), grid, dim3(CL_THREADS), 0, s, tab, p.g, labels, cw, part);
  UZ_LAUNCH_CHECK("uz_class_loss(partial)");
  hipLaunchKernelGGL(class_finalize_kernel, dim3(1), dim3(CL_FIN_THREADS), 0, s, tab, *d, p.g.rows, (const double*)part, tot, coef,
                     out2, counts);
  UZ_LAUNCH_CHECK("uz_class_loss(finalize)");
  if (!grad) return UZ_OK;   // evaluation: no gradient launch
  hipLaunchKernelGGL((class_grad_kernel<KB, VEC>), grid, dim3(CL_THREADS), 0, s, tab, p.g, labels, cw, (const float*)coef);
  UZ_LAUNCH_CHECK("uz_class_loss(grad)");
  return UZ_OK;
}

template <int KB>
int cl_launch_vec(bool vec, const ClPlan& p, const uz_class_desc* d, const ClItems& tab, const int* labels, const float* cw,
                  float* out2, long long* counts, void* workspace, bool grad, hipStream_t s) {
  return vec ? cl_launch<KB, true>(p, d, tab, labels, cw, out2, counts, workspace, grad, s)
             : cl_launch<KB, false>(p, d, tab, labels, cw, out2, counts, workspace, grad, s);
}

}  // namespace

extern "C" long long uz_class_loss_workspace_bytes(const uz_class_desc* d) {
  ClPlan p;
  if (cl_plan("uz_class_loss_workspace_bytes", d, &p) != UZ_OK) return -1;
  const long long bytes = cl_doubles(p) * (long long)sizeof(double) + (long long)p.pairs * (2 * d->K + 2) * (long long)sizeof(float);
  return uz_align16(bytes);
}

extern "C" int uz_class_loss(const uz_class_desc* d, const uz_class_item* items, const int* labels, const float* class_weight,
                             float* out2, long long* counts, void* workspace, void* stream) {
  ClPlan p;
  const int rc = cl_plan("uz_class_loss", d, &p);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(items != nullptr && labels != nullptr && out2 != nullptr && workspace != nullptr,
             "uz_class_loss: null items / labels / out2 / workspace");
  UZ_REQUIRE(((uintptr_t)workspace & 15) == 0, "uz_class_loss: the workspace must be 16-byte aligned");
  ClItems tab;
  bool vec = d->HW % 4 == 0 && ((uintptr_t)labels & 15) == 0, grad = false;
  for (int i = 0; i < d->n_items; ++i) {
    const uz_class_item& it = items[i];
    UZ_REQUIRE(it.logits != nullptr, "uz_class_loss: item %d has null logits", i);
    UZ_REQUIRE(it.weight >= 0.f && it.weight < INFINITY, "uz_class_loss: item %d has a negative weight", i);
    if ((((uintptr_t)it.logits | (uintptr_t)it.dlogits) & 15) != 0) vec = false;
    grad = grad || it.dlogits != nullptr;
    tab.it[i] = it;
  }
  for (int i = d->n_items; i < UZ_CLASS_MAX_ITEMS; ++i) tab.it[i] = tab.it[0];
  hipStream_t s = (hipStream_t)stream;
  // the classes live in registers: the smallest compile-time bound that holds K
  if (d->K <= 2) return cl_launch_vec<2>(vec, p, d, tab, labels, class_weight, out2, counts, workspace, grad, s);
  if (d->K <= 4) return cl_launch_vec<4>(vec, p, d, tab, labels, class_weight, out2, counts, workspace, grad, s);
  if (d->K <= 9) return cl_launch_vec<9>(vec, p, d, tab, labels, class_weight, out2, counts, workspace, grad, s);
  if (d->K <= 16) return cl_launch_vec<16>(vec, p, d, tab, labels, class_weight, out2, counts, workspace, grad, s);
  return cl_launch_vec<32>(vec, p, d, tab, labels, class_weight, out2, counts, workspace, grad, s);
}
