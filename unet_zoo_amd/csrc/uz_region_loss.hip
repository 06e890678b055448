// BCE + region term (soft Dice / Tversky / focal Tversky) of several output maps in three launches, whatever the
// number of maps: partial sums, one finalize workgroup, gradient (include/unetzoo_hip.h).  The maps travel by
// value in the kernel arguments (as in uz_colsum.hip): no table upload, capturable in a hipGraph.  Fixed summation order,
// no atomics, no memset; the workspace is written before it is read in every call.
#include "uz_common.h"

namespace {

constexpr int RL_THREADS = 256;
constexpr int RL_UNROLL = 4;                               // 16-byte loads of x (and of t) a lane keeps in flight
constexpr int RL_CHUNK = RL_THREADS * 4 * RL_UNROLL;       // elements per workgroup row before a chunk gets a second row
constexpr int RL_MAX_ROWS = 1024;                          // rows of one map (all its chunks), as BD_MAX_ROWS
constexpr int RL_FIN_THREADS = 1024;
constexpr int RL_COLS = 6;                                 // sum bce, sum p t, sum p, sum t, sum [x > 0] t, sum [x > 0]

struct RlItems {
  uz_region_item it[UZ_REGION_MAX_ITEMS];
};

struct RlElem {
  float p, q, sp;   // sigmoid(x), p (1 - p), softplus(-x)
};
// e = exp(-|x|) serves all three: softplus(-x) = max(-x, 0) + log(1 + e) is ATen's max + log(exp(-max) + exp(-x - max))
// (one of its two exponentials is exp(0)); p = 1 / (1 + e) or e / (1 + e); p (1 - p) as written: 0 once p rounds to 1
__device__ __forceinline__ RlElem rl_elem(float x) {
  const float e = expf(-fabsf(x));
  const float inv = 1.f / (1.f + e);
  RlElem r;
  r.p = x >= 0.f ? inv : e * inv;
  r.q = r.p * (1.f - r.p);
  r.sp = fmaxf(-x, 0.f) + logf(1.f + e);
  return r;
}

__device__ __forceinline__ void rl_acc(double* s, float x, float t, float pwm1) {
  const RlElem r = rl_elem(x);
  const float pred = x > 0.f ? 1.f : 0.f;
  s[0] += (double)((1.f - t) * x + (1.f + pwm1 * t) * r.sp);
  s[1] += (double)(r.p * t);
  s[2] += (double)r.p;
  s[3] += (double)t;
  s[4] += (double)(pred * t);
  s[5] += (double)pred;
}

// workgroup -> (map, chunk, row): blockIdx.x = (item * groups + g) * rows + row; one division per workgroup
__device__ __forceinline__ void rl_where(int groups, int rows, int* pair, int* item, int* g, int* row) {
  *pair = (int)blockIdx.x / rows;
  *row = (int)blockIdx.x - *pair * rows;
  *item = *pair / groups;
  *g = *pair - *item * groups;
}

// part[blockIdx.x][6]; VEC: 16-byte loads (glen % 4 == 0, aligned pointers), else one float per load
template <bool VEC>
__global__ __launch_bounds__(RL_THREADS) void region_partial_kernel(const RlItems tab, long long glen, int groups, int rows,
                                                                    float pwm1, double* __restrict__ part) {
  int pair, item, g, row;
  rl_where(groups, rows, &pair, &item, &g, &row);
  const float* __restrict__ x = tab.it[item].logits + (size_t)g * glen;
  const float* __restrict__ t = tab.it[item].target + (size_t)g * glen;
  double s[RL_COLS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const long long stride = (long long)rows * RL_THREADS;
  long long i = (long long)row * RL_THREADS + threadIdx.x;
  if (VEC) {
    const long long nq = glen >> 2;
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
    const float4* __restrict__ t4 = reinterpret_cast<const float4*>(t);
    for (; i + (RL_UNROLL - 1) * stride < nq; i += RL_UNROLL * stride) {   // eight 16-byte loads in flight, then the arithmetic
      float4 xv[RL_UNROLL], tv[RL_UNROLL];
#pragma unroll
      for (int u = 0; u < RL_UNROLL; ++u) {
        xv[u] = x4[i + u * stride];
        tv[u] = t4[i + u * stride];
      }
#pragma unroll
      for (int u = 0; u < RL_UNROLL; ++u) {
        rl_acc(s, xv[u].x, tv[u].x, pwm1);
        rl_acc(s, xv[u].y, tv[u].y, pwm1);
        rl_acc(s, xv[u].z, tv[u].z, pwm1);
        rl_acc(s, xv[u].w, tv[u].w, pwm1);
      }
    }
    for (; i < nq; i += stride) {
      const float4 xv = x4[i], tv = t4[i];
      rl_acc(s, xv.x, tv.x, pwm1);
      rl_acc(s, xv.y, tv.y, pwm1);
      rl_acc(s, xv.z, tv.z, pwm1);
      rl_acc(s, xv.w, tv.w, pwm1);
    }
  } else {
    for (; i + (RL_UNROLL - 1) * stride < glen; i += RL_UNROLL * stride) {
      float xv[RL_UNROLL], tv[RL_UNROLL];
#pragma unroll
      for (int u = 0; u < RL_UNROLL; ++u) {
        xv[u] = x[i + u * stride];
        tv[u] = t[i + u * stride];
      }
#pragma unroll
      for (int u = 0; u < RL_UNROLL; ++u) rl_acc(s, xv[u], tv[u], pwm1);
    }
    for (; i < glen; i += stride) rl_acc(s, x[i], t[i], pwm1);
  }
  __shared__ double red[RL_THREADS / 64][RL_COLS];
#pragma unroll
  for (int k = 0; k < RL_COLS; ++k) {
    double v = s[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < RL_COLS) {
    double v = 0.0;
    for (int w = 0; w < RL_THREADS / 64; ++w) v += red[w][threadIdx.x];
    part[(size_t)blockIdx.x * RL_COLS + threadIdx.x] = v;
  }
}

// One workgroup.  `sub` lanes (a power of two <= 64) share a (map, chunk) pair: lane l adds rows l, l + sub, ... and a
// fixed tree joins them; the pair's first lane forms TI, the coefficients and the pair's share of the loss; a fixed tree
// over the workgroup totals the shares.  coef[pair] = (u_g, v_g, weight * w_bce / n, 0), u and v with the map's weight.
__global__ __launch_bounds__(RL_FIN_THREADS) void region_finalize_kernel(const RlItems tab, const uz_region_desc d, int rows,
                                                                         int sub, const double* __restrict__ part,
                                                                         float4* __restrict__ coef, float* __restrict__ out) {
  __shared__ double red[RL_FIN_THREADS / 64][4];
  const int pairs = d.n_items * d.groups;
  const int l = threadIdx.x & (sub - 1), slot = threadIdx.x / sub, slots = RL_FIN_THREADS / sub;
  const double a = (double)d.alpha, b = (double)d.beta, sm = (double)d.smooth, gam = (double)d.gamma;
  double tot[4] = {0.0, 0.0, 0.0, 0.0};   // loss, and of the metric map: sum [x > 0] t, sum [x > 0], sum t
  for (int base = 0; base < pairs; base += slots) {
    const int pair = base + slot;
    const bool valid = pair < pairs;
    const double* __restrict__ rowp = part + (size_t)(valid ? pair : 0) * rows * RL_COLS;
    double s[RL_COLS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = l; r < rows; r += sub)
#pragma unroll
      for (int k = 0; k < RL_COLS; ++k) s[k] += rowp[(size_t)r * RL_COLS + k];
#pragma unroll
    for (int k = 0; k < RL_COLS; ++k)
      for (int o = sub >> 1; o > 0; o >>= 1) s[k] += __shfl_down(s[k], o, sub);
    if (valid && l == 0) {
      const int item = pair / d.groups;
      const double w = (double)tab.it[item].weight;
      const double I = s[1], S = s[2], T = s[3];
      const double fp = a * (S - I) + b * (T - I);        // what the denominator has more than the numerator
      const double num = I + sm, den = num + fp;
      const double q = fmax(fp / den, 0.0);               // 1 - TI, without the cancellation of 1 - num / den
      double h = 1.0;                                     // q^(gamma - 1): 1 for gamma == 1, also at q == 0
      if (d.gamma != 1.f) h = pow(q, gam - 1.0);
      const double f = q * h;                             // (1 - TI)^gamma
      const double c = w * (double)d.w_region / (double)d.groups * gam * h / (den * den);
      // d(TI)/d(p_i) = t_i (den - num (1 - a - b)) / den^2 - num a / den^2, and d f / d TI = -gamma h
      coef[pair] = make_float4((float)(-c * (den - num * (1.0 - a - b))), (float)(c * num * a),
                               (float)(w * (double)d.w_bce / (double)d.n), 0.f);
      tot[0] += w * ((double)d.w_bce * s[0] / (double)d.n + (double)d.w_region * f / (double)d.groups);
      if (item == d.metric_item) {
        tot[1] += s[4];
        tot[2] += s[5];
        tot[3] += s[3];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double v = tot[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int w = 0; w < RL_FIN_THREADS / 64; ++w)
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] += red[w][k];
    out[0] = (float)v[0];
    const double uni = v[2] + v[3];
    out[1] = uni == 0.0 ? 1.f : (float)((2.0 * v[1] + 1e-7) / (uni + 1e-7));
  }
}

__device__ __forceinline__ float rl_grad(float x, float t, float4 c, float pw, float pwm1) {
  const RlElem r = rl_elem(x);
  return c.z * (r.p * (1.f + pwm1 * t) - pw * t) + (c.x * t + c.y) * r.q;
}

template <bool VEC>
__global__ __launch_bounds__(RL_THREADS) void region_grad_kernel(const RlItems tab, long long glen, int groups, int rows,
                                                                 float pw, const float4* __restrict__ coef) {
  int pair, item, g, row;
  rl_where(groups, rows, &pair, &item, &g, &row);
  float* __restrict__ dl = tab.it[item].dlogits;
  if (dl == nullptr) return;   // the whole workgroup: a map without a gradient
  dl += (size_t)g * glen;
  const float* __restrict__ x = tab.it[item].logits + (size_t)g * glen;
  const float* __restrict__ t = tab.it[item].target + (size_t)g * glen;
  const float4 c = coef[pair];
  const float pwm1 = pw - 1.f;
  const long long stride = (long long)rows * RL_THREADS;
  long long i = (long long)row * RL_THREADS + threadIdx.x;
  if (VEC) {
    const long long nq = glen >> 2;
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
    const float4* __restrict__ t4 = reinterpret_cast<const float4*>(t);
    float4* __restrict__ d4 = reinterpret_cast<float4*>(dl);
    for (; i + (RL_UNROLL - 1) * stride < nq; i += RL_UNROLL * stride) {
      float4 xv[RL_UNROLL], tv[RL_UNROLL];
#pragma unroll
      for (int u = 0; u < RL_UNROLL; ++u) {
        xv[u] = x4[i + u * stride];
        tv[u] = t4[i + u * stride];
      }
#pragma unroll
      for (int u = 0; u < RL_UNROLL; ++u)
        d4[i + u * stride] = make_float4(rl_grad(xv[u].x, tv[u].x, c, pw, pwm1), rl_grad(xv[u].y, tv[u].y, c, pw, pwm1),
                                         rl_grad(xv[u].z, tv[u].z, c, pw, pwm1), rl_grad(xv[u].w, tv[u].w, c, pw, pwm1));
    }
    for (; i < nq; i += stride) {
      const float4 xv = x4[i], tv = t4[i];
      d4[i] = make_float4(rl_grad(xv.x, tv.x, c, pw, pwm1), rl_grad(xv.y, tv.y, c, pw, pwm1),
                          rl_grad(xv.z, tv.z, c, pw, pwm1), rl_grad(xv.w, tv.w, c, pw, pwm1));
    }
  } else {
    for (; i + (RL_UNROLL - 1) * stride < glen; i += RL_UNROLL * stride) {
      float xv[RL_UNROLL], tv[RL_UNROLL];
#pragma unroll
      for (int u = 0; u < RL_UNROLL; ++u) {
        xv[u] = x[i + u * stride];
        tv[u] = t[i + u * stride];
      }
#pragma unroll
      for (int u = 0; u < RL_UNROLL; ++u) dl[i + u * stride] = rl_grad(xv[u], tv[u], c, pw, pwm1);
    }
    for (; i < glen; i += stride) dl[i] = rl_grad(x[i], t[i], c, pw, pwm1);
  }
}

struct RlPlan {
  long long glen;   // elements of one chunk
  int pairs;        // n_items * groups
  int rows;         // workgroup rows per chunk
  int sub;          // finalize lanes per (map, chunk)
};

int rl_plan(const char* fn, const uz_region_desc* d, RlPlan* p) {
  UZ_REQUIRE(d != nullptr, "%s: null descriptor", fn);
  UZ_REQUIRE(d->n_items >= 1 && d->n_items <= UZ_REGION_MAX_ITEMS, "%s: n_items = %d outside [1, %d]", fn, d->n_items,
             UZ_REGION_MAX_ITEMS);
  UZ_REQUIRE(d->n > 0, "%s: n = %lld", fn, d->n);
  UZ_REQUIRE(d->groups >= 1 && d->n % d->groups == 0, "%s: groups = %d does not divide n = %lld", fn, d->groups, d->n);
  UZ_REQUIRE(d->groups <= (1 << 24), "%s: groups = %d above 2^24", fn, d->groups);
  UZ_REQUIRE(d->metric_item >= 0 && d->metric_item < d->n_items, "%s: metric_item = %d outside [0, %d)", fn, d->metric_item,
             d->n_items);
  // written so that a NaN is refused too
  UZ_REQUIRE(d->smooth > 0.f && d->smooth < INFINITY, "%s: smooth must be positive", fn);
  UZ_REQUIRE(d->gamma >= 1.f && d->gamma < INFINITY, "%s: gamma must be >= 1", fn);
  UZ_REQUIRE(d->alpha >= 0.f && d->alpha < INFINITY && d->beta >= 0.f && d->beta < INFINITY,
             "%s: alpha and beta must be >= 0", fn);
  UZ_REQUIRE(d->w_bce >= 0.f && d->w_bce < INFINITY && d->w_region >= 0.f && d->w_region < INFINITY,
             "%s: w_bce and w_region must be >= 0", fn);
  UZ_REQUIRE(d->w_bce > 0.f || d->w_region > 0.f, "%s: w_bce and w_region are both zero", fn);
  UZ_REQUIRE(d->pos_weight > 0.f && d->pos_weight < INFINITY, "%s: pos_weight must be positive", fn);
  p->glen = d->n / d->groups;
  p->pairs = d->n_items * d->groups;
  long long rows = (p->glen + RL_CHUNK - 1) / RL_CHUNK;
  const long long cap = RL_MAX_ROWS / d->groups > 0 ? RL_MAX_ROWS / d->groups : 1;   // per map, so that a map's rows do not
  if (rows > cap) rows = cap;                                                        // depend on how many maps travel along
  p->rows = (int)rows;
  int sub = 1;
  while (sub < p->rows && sub < 64) sub <<= 1;
  p->sub = sub;
  UZ_REQUIRE((long long)p->pairs * p->rows < (1LL << 30), "%s: %d chunks are too many", fn, p->pairs);
  return UZ_OK;
}

}  // namespace

extern "C" long long uz_region_loss_workspace_bytes(const uz_region_desc* d) {
  RlPlan p;
  if (rl_plan("uz_region_loss_workspace_bytes", d, &p) != UZ_OK) return -1;
  return (long long)p.pairs * p.rows * RL_COLS * (long long)sizeof(double) + (long long)p.pairs * (long long)sizeof(float4);
}

extern "C" int uz_region_loss(const uz_region_desc* d, const uz_region_item* items, float* out2, void* workspace, void* stream) {
  RlPlan p;
  const int rc = rl_plan("uz_region_loss", d, &p);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(items != nullptr && out2 != nullptr && workspace != nullptr, "uz_region_loss: null items / out2 / workspace");
  UZ_REQUIRE(((uintptr_t)workspace & 15) == 0, "uz_region_loss: the workspace must be 16-byte aligned");
  RlItems tab;
  bool vec = p.glen % 4 == 0, grad = false;
  for (int i = 0; i < d->n_items; ++i) {
    const uz_region_item& it = items[i];
    UZ_REQUIRE(it.logits != nullptr && it.target != nullptr, "uz_region_loss: item %d has a null logits / target", i);
    UZ_REQUIRE(it.weight >= 0.f && it.weight < INFINITY, "uz_region_loss: item %d has a negative weight", i);
    if ((((uintptr_t)it.logits | (uintptr_t)it.target | (uintptr_t)it.dlogits) & 15) != 0) vec = false;
    grad = grad || it.dlogits != nullptr;
    tab.it[i] = it;
  }
  for (int i = d->n_items; i < UZ_REGION_MAX_ITEMS; ++i) tab.it[i] = tab.it[0];
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)workspace;
  float4* coef = (float4*)(part + (size_t)p.pairs * p.rows * RL_COLS);   // 48 bytes per row: stays 16-byte aligned
  const dim3 grid((unsigned)(p.pairs * p.rows));
  const float pwm1 = d->pos_weight - 1.f;
  if (vec) hipLaunchKernelGGL(region_partial_kernel<true>, grid, dim3(RL_THREADS), 0, s, tab, p.glen, d->groups, p.rows, pwm1, part);
  else hipLaunchKernelGGL(region_partial_kernel<false>, grid, dim3(RL_THREADS), 0, s, tab, p.glen, d->groups, p.rows, pwm1, part);
  UZ_LAUNCH_CHECK("uz_region_loss(partial)");
  hipLaunchKernelGGL(region_finalize_kernel, dim3(1), dim3(RL_FIN_THREADS), 0, s, tab, *d, p.rows, p.sub, (const double*)part,
                     coef, out2);
  UZ_LAUNCH_CHECK("uz_region_loss(finalize)");
  if (!grad) return UZ_OK;   // evaluation: no gradient launch
  if (vec) hipLaunchKernelGGL(region_grad_kernel<true>, grid, dim3(RL_THREADS), 0, s, tab, p.glen, d->groups, p.rows, d->pos_weight,
                              (const float4*)coef);
  else hipLaunchKernelGGL(region_grad_kernel<false>, grid, dim3(RL_THREADS), 0, s, tab, p.glen, d->groups, p.rows, d->pos_weight,
                          (const float4*)coef);
  UZ_LAUNCH_CHECK("uz_region_loss(grad)");
  return UZ_OK;
}
