// The scheduled step tail (gfx950): clip_grad_norm_ + AdamW as uz_clip_adamw (uz_eltwise.hip) computes them, with the
// learning rate, the step counter and the EMA decay held ON THE DEVICE -- a per-step schedule (warm-up, cosine, polynomial,
// step decay) needs no host work and no new capture --, an optional averaged copy of the weights updated in the same
// streaming pass, and an optional accumulated gradient read beside the fresh one.
//
// uz_tail_step is three launches, as uz_clip_adamw:
//   1. tail_sqnorm_kernel<ACC>   per-workgroup float64 sums of squares of the effective gradient (fixed order);
//   2. tail_prepare_kernel<SCHED> one workgroup: norm, clip coefficient, t += 1, bias corrections; its thread 0 evaluates the
//                                schedule in double from t and the base rate, rounds it ONCE to float, forms the EMA decay;
//   3. tail_apply_kernel<ACC, EMA>  one pass over p, g, (acc), m, v, (ema): 28 bytes per parameter, + 4 with acc, + 8 with ema.
// ACC / EMA are template parameters: a run-time `if (ema)` around the loads would close them with a wait where the branch ends.
// The AdamW arithmetic is adamw_apply_kernel's, expression for expression: with a constant schedule and neither acc nor ema
// the three buffers come out bit-identical to uz_clip_adamw's (tests/test_steptail_gpu.py).
#include "uz_common.h"
#include <math.h>

namespace {

constexpr int TAIL_ROWS = 1024;   // uz_clip_adamw's ADAMW_ROWS: the same partial rows, the same order of the sums

// the gradient a step consumes: g, or the mean of the k micro-batch gradients (acc holds the first k - 1)
template <bool ACC> __device__ __forceinline__ float eff(float g, float a, float inv_k) { return ACC ? (g + a) * inv_k : g; }

template <bool ACC>
__global__ __launch_bounds__(256) void tail_sqnorm_kernel(const float* __restrict__ g, const float* __restrict__ acc, float inv_k,
                                                          long long n, double* __restrict__ partial) {
  __shared__ double red[256];
  double s = 0.0;
  const long long n4 = n >> 2;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  const float4* a4 = reinterpret_cast<const float4*>(acc);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float4 v = g4[i];
    if (ACC) {
      const float4 a = a4[i];
      v.x = eff<true>(v.x, a.x, inv_k);
      v.y = eff<true>(v.y, a.y, inv_k);
      v.z = eff<true>(v.z, a.z, inv_k);
      v.w = eff<true>(v.w, a.w, inv_k);
    }
    s += (double)(v.x * v.x + v.y * v.y) + (double)(v.z * v.z + v.w * v.w);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long long i = (n4 << 2) + threadIdx.x;
    const float v = eff<ACC>(g[i], ACC ? acc[i] : 0.f, inv_k);
    s += (double)v * v;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// the schedule at step t (0-based index of the step being taken) for the base rate L, in double.  SCHED is a template
// parameter: an instance holds the arithmetic of its own form only (a constant schedule: none beyond the warm-up's division)
template <int SCHED> __device__ __forceinline__ double tail_schedule(const uz_tail_desc& d, double t, double L) {
  const double W = d.warmup_steps, lo = d.min_lr;
  if (t < W) return L * ((double)d.warmup_start + (1.0 - (double)d.warmup_start) * t / W);
  if (SCHED == UZ_SCHED_CONSTANT) return L;
  if (SCHED == UZ_SCHED_STEP) {
    const double lr = L * pow((double)d.gamma, floor((t - W) / (double)d.every));
    return lr > lo ? lr : lo;
  }
  double u = (t - W) / ((double)d.total_steps - W);
  u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
  if (SCHED == UZ_SCHED_COSINE) return lo + (L - lo) * 0.5 * (1.0 + cospi(u));   // cos(pi u) without the argument reduction
  return lo + (L - lo) * pow(1.0 - u, (double)d.power);   // UZ_SCHED_POLY
}

template <int SCHED>
__global__ __launch_bounds__(256) void tail_prepare_kernel(const double* __restrict__ partial, int rows, uz_tail_desc d,
                                                           int has_ema, float* __restrict__ state) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < rows; i += 256) s += partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(red[0]);
    float coef = 1.f;
    if (d.max_norm > 0.f) {
      coef = d.max_norm / (norm + 1e-6f);   // torch: clamp(max_norm / (total_norm + 1e-6), max=1)
      if (coef > 1.f) coef = 1.f;
    }
    const float t0 = state[0];
    const float t = t0 + 1.f;
    float decay = 0.f;
    if (has_ema) {
      decay = d.ema_decay;
      if (d.ema_warmup) {
        const float w = (float)((1.0 + (double)t0) / (10.0 + (double)t0));
        if (w < decay) decay = w;
      }
    }
    state[0] = t;
    state[2] = (float)tail_schedule<SCHED>(d, (double)t0, (double)state[1]);
    state[3] = decay;
    state[4] = coef;
    state[5] = norm;
    state[6] = 1.f - powf(d.beta1, t);
    state[7] = 1.f - powf(d.beta2, t);
  }
}

template <bool ACC, bool EMA>
__global__ __launch_bounds__(256) void tail_apply_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         const float* __restrict__ acc, float* __restrict__ m,
                                                         float* __restrict__ v, float* __restrict__ ema, long long n,
                                                         float beta1, float beta2, float eps, float wd, float inv_k,
                                                         const float* __restrict__ state) {
  const float lr = state[2], coef = state[4], bc1 = state[6], bc2 = state[7];
  const float omd = 1.f - state[3];
  const float step_size = lr / bc1, rs2 = rsqrtf(bc2), decay = 1.f - lr * wd;
  auto upd = [&](float& pv, float gv, float& mv, float& vv) {
    gv *= coef;
    pv *= decay;                                   // decoupled weight decay
    mv = beta1 * mv + (1.f - beta1) * gv;          // torch: exp_avg.lerp_(grad, 1 - beta1)
    vv = beta2 * vv + (1.f - beta2) * gv * gv;
    pv -= step_size * mv / (sqrtf(vv) * rs2 + eps);
  };
  auto avg = [&](float& ev, float pv) { ev += omd * (pv - ev); };
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float4 pv = reinterpret_cast<float4*>(p)[i], mv = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 ev;
    if (ACC) {
      const float4 a = reinterpret_cast<const float4*>(acc)[i];
      gv.x = eff<true>(gv.x, a.x, inv_k);
      gv.y = eff<true>(gv.y, a.y, inv_k);
      gv.z = eff<true>(gv.z, a.z, inv_k);
      gv.w = eff<true>(gv.w, a.w, inv_k);
    }
    if (EMA) ev = reinterpret_cast<float4*>(ema)[i];
    upd(pv.x, gv.x, mv.x, vv.x);
    upd(pv.y, gv.y, mv.y, vv.y);
    upd(pv.z, gv.z, mv.z, vv.z);
    upd(pv.w, gv.w, mv.w, vv.w);
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
    if (EMA) {
      avg(ev.x, pv.x);
      avg(ev.y, pv.y);
      avg(ev.z, pv.z);
      avg(ev.w, pv.w);
      reinterpret_cast<float4*>(ema)[i] = ev;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long long i = (n4 << 2) + threadIdx.x;
    upd(p[i], eff<ACC>(g[i], ACC ? acc[i] : 0.f, inv_k), m[i], v[i]);
    if (EMA) avg(ema[i], p[i]);
  }
}

// acc = FIRST ? g : acc + g   (FIRST never reads acc: whatever it held is gone)
template <bool FIRST>
__global__ __launch_bounds__(256) void tail_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, long long n) {
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float4 gv = reinterpret_cast<const float4*>(g)[i];
    if (!FIRST) {
      const float4 a = reinterpret_cast<float4*>(acc)[i];
      gv.x += a.x;
      gv.y += a.y;
      gv.z += a.z;
      gv.w += a.w;
    }
    reinterpret_cast<float4*>(acc)[i] = gv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long long i = (n4 << 2) + threadIdx.x;
    acc[i] = FIRST ? g[i] : acc[i] + g[i];
  }
}

// a and b are distinct buffers (checked on the host): no __restrict__ promise is needed, none is made
__global__ __launch_bounds__(256) void tail_swap_kernel(float* a, float* b, long long n) {
  const long long n4 = n >> 2;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const float4 av = reinterpret_cast<float4*>(a)[i], bv = reinterpret_cast<float4*>(b)[i];
    reinterpret_cast<float4*>(a)[i] = bv;
    reinterpret_cast<float4*>(b)[i] = av;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long long i = (n4 << 2) + threadIdx.x;
    const float av = a[i], bv = b[i];
    a[i] = bv;
    b[i] = av;
  }
}

bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

// workgroups of a streaming pass over n floats: one float4 per thread, at most UZ_NUM_CU * 8 (uz_clip_adamw's grid)
int stream_grid(long long n) {
  const long long blocks = (n / 4 + 255) / 256, cap = (long long)UZ_NUM_CU * 8;
  return (int)(blocks < cap ? (blocks < 1 ? 1 : blocks) : cap);
}

}  // namespace

extern "C" long long uz_tail_workspace_bytes(void) { return (long long)TAIL_ROWS * 8; }

extern "C" int uz_tail_step(const uz_tail_desc* d, float* p, const float* g, const float* acc, float* m, float* v, float* ema,
                            float* state, void* workspace, void* stream) {
  UZ_REQUIRE(d && p && g && m && v && state && workspace, "uz_tail_step: null pointer");
  UZ_REQUIRE(d->n > 0, "uz_tail_step: n=%lld must be positive", d->n);
  UZ_REQUIRE(aligned16(p, g, m, v) && aligned16(acc, ema, workspace), "uz_tail_step: buffers must be 16-byte aligned");
  UZ_REQUIRE(((uintptr_t)state & 3) == 0, "uz_tail_step: state must be 4-byte aligned");
  const float fin[] = {d->beta1, d->beta2, d->eps, d->weight_decay, d->max_norm, d->warmup_steps, d->warmup_start, d->total_steps,
                       d->min_lr, d->power, d->gamma, d->every, d->ema_decay};
  for (float f : fin) UZ_REQUIRE(isfinite(f), "uz_tail_step: a descriptor number is not finite");
  UZ_REQUIRE(d->sched >= UZ_SCHED_CONSTANT && d->sched <= UZ_SCHED_STEP, "uz_tail_step: sched=%d is not a UZ_SCHED_* value", d->sched);
  UZ_REQUIRE(d->warmup_steps >= 0.f, "uz_tail_step: warmup_steps=%g must be >= 0", d->warmup_steps);
  if (d->sched == UZ_SCHED_COSINE || d->sched == UZ_SCHED_POLY)
    UZ_REQUIRE(d->total_steps > d->warmup_steps, "uz_tail_step: total_steps=%g must exceed warmup_steps=%g", d->total_steps, d->warmup_steps);
  if (d->sched == UZ_SCHED_POLY) UZ_REQUIRE(d->power > 0.f, "uz_tail_step: power=%g must be positive", d->power);
  if (d->sched == UZ_SCHED_STEP)
    UZ_REQUIRE(d->every >= 1.f && d->gamma > 0.f && d->gamma <= 1.f, "uz_tail_step: every=%g must be >= 1 and gamma=%g in (0, 1]",
               d->every, d->gamma);
  UZ_REQUIRE(d->accumulate >= 1, "uz_tail_step: accumulate=%d must be >= 1", d->accumulate);
  if (ema) UZ_REQUIRE(d->ema_decay >= 0.f && d->ema_decay < 1.f, "uz_tail_step: ema_decay=%g must be in [0, 1)", d->ema_decay);
  hipStream_t s = (hipStream_t)stream;
  double* partial = static_cast<double*>(workspace);
  const long long n = d->n, blocks = (n / 4 + 255) / 256;
  const int rows = (int)(blocks < TAIL_ROWS ? (blocks < 1 ? 1 : blocks) : TAIL_ROWS);
  const int grid = stream_grid(n);
  const float inv_k = 1.f / (float)d->accumulate;
  if (acc)
    hipLaunchKernelGGL(tail_sqnorm_kernel<true>, dim3(rows), dim3(256), 0, s, g, acc, inv_k, n, partial);
  else
    hipLaunchKernelGGL(tail_sqnorm_kernel<false>, dim3(rows), dim3(256), 0, s, g, acc, inv_k, n, partial);
  UZ_LAUNCH_CHECK("uz_tail_step(norm)");
#define UZ_TAIL_PREPARE(S) \
  hipLaunchKernelGGL(tail_prepare_kernel<S>, dim3(1), dim3(256), 0, s, partial, rows, *d, ema != nullptr ? 1 : 0, state)
  switch (d->sched) {
    case UZ_SCHED_COSINE: UZ_TAIL_PREPARE(UZ_SCHED_COSINE); break;
    case UZ_SCHED_POLY: UZ_TAIL_PREPARE(UZ_SCHED_POLY); break;
    case UZ_SCHED_STEP: UZ_TAIL_PREPARE(UZ_SCHED_STEP); break;
    default: UZ_TAIL_PREPARE(UZ_SCHED_CONSTANT); break;
  }
#undef UZ_TAIL_PREPARE
  UZ_LAUNCH_CHECK("uz_tail_step(prepare)");
#define UZ_TAIL_APPLY(A, E)                                                                                              \
  hipLaunchKernelGGL((tail_apply_kernel<A, E>), dim3(grid), dim3(256), 0, s, p, g, acc, m, v, ema, n, d->beta1, d->beta2, \
                     d->eps, d->weight_decay, inv_k, state)
  if (acc && ema)
    UZ_TAIL_APPLY(true, true);
  else if (acc)
    UZ_TAIL_APPLY(true, false);
  else if (ema)
    UZ_TAIL_APPLY(false, true);
  else
    UZ_TAIL_APPLY(false, false);
#undef UZ_TAIL_APPLY
  UZ_LAUNCH_CHECK("uz_tail_step(apply)");
  return UZ_OK;
}

extern "C" int uz_tail_accumulate(float* acc, const float* g, long long n, int first, void* stream) {
  UZ_REQUIRE(acc && g && n > 0, "uz_tail_accumulate: bad args");
  UZ_REQUIRE(aligned16(acc, g), "uz_tail_accumulate: buffers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (first)
    hipLaunchKernelGGL(tail_accumulate_kernel<true>, dim3(stream_grid(n)), dim3(256), 0, s, acc, g, n);
  else
    hipLaunchKernelGGL(tail_accumulate_kernel<false>, dim3(stream_grid(n)), dim3(256), 0, s, acc, g, n);
  UZ_LAUNCH_CHECK("uz_tail_accumulate");
  return UZ_OK;
}

extern "C" int uz_tail_swap(float* a, float* b, long long n, void* stream) {
  UZ_REQUIRE(a && b && n > 0, "uz_tail_swap: bad args");
  UZ_REQUIRE(aligned16(a, b), "uz_tail_swap: buffers must be 16-byte aligned");
  UZ_REQUIRE(a + n <= b || b + n <= a, "uz_tail_swap: the buffers overlap");
  hipLaunchKernelGGL(tail_swap_kernel, dim3(stream_grid(n)), dim3(256), 0, (hipStream_t)stream, a, b, n);
  UZ_LAUNCH_CHECK("uz_tail_swap");
  return UZ_OK;
}
