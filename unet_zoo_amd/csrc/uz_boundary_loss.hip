// Boundary loss (Kervadec et al.) on the device: the exact signed squared Euclidean distance transform of the target, dense,
// and the mean of probability x signed distance map over several output maps, added to a base loss whose value and
// gradients already exist (include/unetzoo_hip.h).  M planes: every (image, channel) in the binary mode, every
// (image, class of Cset) in the class mode.
//   sd2(p) = +min over g in G of |p - g|^2 for p outside G, -min over q outside G of |p - q|^2 for p in G, 0 everywhere when
//            G is empty or the whole plane -- an INTEGER, |sd2| < 2^25 for H, W <= 4096
// Five launches, every one with a fixed grid for a descriptor:
//   rows     per (plane, row): membership and the distance along the row to the nearest pixel of the OPPOSITE membership as
//            one 16-bit value (bit 15: in G; low 15 bits: the distance, BL_NONE = the row has none), and the row's pixels in G
//            and outside G
//   planes   per plane: |G| and the first and the last row that holds a pixel of G / of its complement, from the rows' counts
//            in row order (no atomics: nothing to clear)
//   columns  per pixel (i, j) of a plane that is neither empty nor full: min over i' of g(i', j)^2 + (i - i')^2 with
//            g = 0 where (i', j) has the opposite membership, searched outwards from i until (i - i')^2 >= the best, over
//            the rows that hold a pixel of the opposite membership only
//   loss     phi from sd2 on the fly; per (workgroup, map) the float64 sum of p * phi, and dl <- base_scale dl + weight ow dB/dx
//   finalize the workgroup sums in index order, out[0] = base_scale * base_loss + weight * sum_m ow_m B_m, out[1] = B_main
#include "uz_common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int BL_THREADS = 256;
constexpr int BL_NONE = 0x7FFF;       // no pixel of the opposite membership in this row.  NEVER squared: every use selects on it first
constexpr int BL_IN = 0x8000;         // the pixel is in G
constexpr int BL_MAX_HW = 4096;
constexpr int BL_WORDS = BL_MAX_HW / 64;
constexpr int BL_STEP = 8;            // rows up and rows down of one round trip of the column search
constexpr int BL_CNT = 8;             // counters of a plane: |G|, first / last row with a pixel of G, first / last row with one outside G, spare

struct BlItems {
  uz_boundary_item it[UZ_CLASS_MAX_ITEMS];
};

struct BlGeo {
  int mode;
  int n_items;
  int N, K;          // K: channels (binary) or classes
  int first;         // class mode: the first class of Cset
  int P;             // planes per image: C (binary) or K - first
  int M;             // N * P
  int H, W, HW;
  int tiles;         // units of BL_THREADS pixels per plane
  int units;         // M * tiles: the column pass
  int ignore_index;
  int metric_item;
  float spacing;
  float inv_den;     // 1 / (N P H W)
  long long pixels;  // what the loss pass walks: N C H W elements (binary) or N H W pixels (class)
};

// A workgroup takes planes blockIdx.x, blockIdx.x + gridDim.x, ...: cnt[plane] = |G|, first / last row with a pixel of G,
// first / last row with a pixel outside G (INT_MAX / -1 when there is none)
__global__ __launch_bounds__(BL_THREADS) void boundary_planes_kernel(BlGeo geo, const int2* __restrict__ rowinfo, int* __restrict__ cnt) {
  __shared__ int red[BL_THREADS / 64][5];
  const int H = geo.H, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int plane = blockIdx.x; plane < geo.M; plane += gridDim.x) {
    int n = 0, lo_g = INT_MAX, hi_g = -1, lo_c = INT_MAX, hi_c = -1;
    for (int i = threadIdx.x; i < H; i += BL_THREADS) {
      const int2 r = rowinfo[(size_t)plane * H + i];
      n += r.x;
      lo_g = r.x ? min(lo_g, i) : lo_g;
      hi_g = r.x ? max(hi_g, i) : hi_g;
      lo_c = r.y ? min(lo_c, i) : lo_c;
      hi_c = r.y ? max(hi_c, i) : hi_c;
    }
    for (int o = 32; o > 0; o >>= 1) {
      n += __shfl_down(n, o);
      lo_g = min(lo_g, __shfl_down(lo_g, o));
      hi_g = max(hi_g, __shfl_down(hi_g, o));
      lo_c = min(lo_c, __shfl_down(lo_c, o));
      hi_c = max(hi_c, __shfl_down(hi_c, o));
    }
    if (lane == 0) {
      red[wave][0] = n, red[wave][1] = lo_g, red[wave][2] = hi_g, red[wave][3] = lo_c, red[wave][4] = hi_c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int q = 1; q < BL_THREADS / 64; ++q) {
        n += red[q][0];
        lo_g = min(lo_g, red[q][1]);
        hi_g = max(hi_g, red[q][2]);
        lo_c = min(lo_c, red[q][3]);
        hi_c = max(hi_c, red[q][4]);
      }
      int* __restrict__ c = cnt + (size_t)plane * BL_CNT;
      c[0] = n, c[1] = lo_g, c[2] = hi_g, c[3] = lo_c, c[4] = hi_c;
    }
    __syncthreads();
  }
}

// A workgroup takes (plane, row) units blockIdx.x, blockIdx.x + gridDim.x, ...: a wave's ballot is one 64-pixel word of the
// row's membership bits (and of its complement inside the picture); every pixel then finds the nearest set bit of the
// OTHER word to its left and to its right.
template <int MODE>
__global__ __launch_bounds__(BL_THREADS) void boundary_rows_kernel(BlGeo geo, const void* __restrict__ target, unsigned short* __restrict__ g,
                                                                   int2* __restrict__ rowinfo) {
  __shared__ unsigned long long bits[2][BL_WORDS];   // [0]: in G; [1]: in the picture and not in G
  __shared__ int tally[2];                           // pixels of the row in G, outside G
  const int H = geo.H, W = geo.W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunks = (W + BL_THREADS - 1) / BL_THREADS, nwords = (W + 63) / 64;
  for (int unit = blockIdx.x; unit < geo.M * H; unit += gridDim.x) {
    const int plane = unit / H, i = unit - plane * H;
    const int n = plane / geo.P, cls = geo.first + (plane - n * geo.P);
    const float* __restrict__ tf = static_cast<const float*>(target) + (size_t)plane * geo.HW + (size_t)i * W;
    const int* __restrict__ ti = static_cast<const int*>(target) + (size_t)n * geo.HW + (size_t)i * W;
    int in_n = 0, out_n = 0;                         // of this wave
    if (threadIdx.x == 0) tally[0] = tally[1] = 0;
    for (int ch = 0; ch < chunks; ++ch) {
      const int j = ch * BL_THREADS + (int)threadIdx.x;
      const bool live = j < W;
      const int jc = live ? j : W - 1;
      bool in;
      if (MODE == UZ_BOUNDARY_BINARY) {
        in = live && tf[jc] > 0.5f;
      } else {
        const int y = ti[jc];                        // cls is inside [0, K): an out-of-range label is in no G_c
        in = live && y == cls && y != geo.ignore_index;
      }
      const unsigned long long bi = __ballot(in), bo = __ballot(live && !in);
      in_n += __popcll(bi);
      out_n += __popcll(bo);
      if (lane == 0 && ch * 4 + wave < nwords) {
        bits[0][ch * 4 + wave] = bi;
        bits[1][ch * 4 + wave] = bo;
      }
    }
    __syncthreads();
    if (lane == 0) {
      if (in_n) atomicAdd(&tally[0], in_n);
      if (out_n) atomicAdd(&tally[1], out_n);
    }
    for (int j = threadIdx.x; j < W; j += BL_THREADS) {
      const int w0 = j >> 6, b = j & 63;
      const bool in = (bits[0][w0] >> b) & 1ull;
      const unsigned long long* o = bits[in ? 1 : 0];
      int dist = BL_NONE;
      unsigned long long mk = o[w0] & (~0ull >> (63 - b));            // pixels of the other membership at or left of j
      int ww = w0;
      while (mk == 0 && ww > 0) mk = o[--ww];
      if (mk) dist = j - (ww * 64 + 63 - __clzll((long long)mk));
      mk = o[w0] & (~0ull << b);                                       // at or right of j
      ww = w0;
      while (mk == 0 && ww + 1 < nwords) mk = o[++ww];
      if (mk) dist = min(dist, ww * 64 + __ffsll((unsigned long long)mk) - 1 - j);
      g[(size_t)plane * geo.HW + (size_t)i * W + j] = (unsigned short)(dist | (in ? BL_IN : 0));
    }
    __syncthreads();                                 // the words are rewritten by the next unit, the tally is complete
    if (threadIdx.x == 0) rowinfo[unit] = make_int2(tally[0], tally[1]);      // (the thread that clears the tally for the next unit)
  }
}

// min(best, d(i -+ r, j)^2 + r^2 for r = r0 .. r0 + S - 1), d = the row distance of (i -+ r, j) to the nearest pixel whose
// membership is not `mine`: 0 where that pixel is one itself, its stored distance otherwise.  2 S loads issued together,
// unconditional from clamped rows; the sentinel and the picture's edge are selected afterwards
template <int S>
__device__ __forceinline__ int bl_round(const unsigned short* __restrict__ gp, int i, int j, int H, int W, int r0, int best, int mine) {
  int gu[S], gd[S];
#pragma unroll
  for (int e = 0; e < S; ++e) {
    gu[e] = gp[(size_t)max(i - r0 - e, 0) * W + j];
    gd[e] = gp[(size_t)min(i + r0 + e, H - 1) * W + j];
  }
#pragma unroll
  for (int e = 0; e < S; ++e) {
    const int r = r0 + e;
    const int du = (gu[e] & BL_IN) != mine ? 0 : (gu[e] & BL_NONE);
    const int dd = (gd[e] & BL_IN) != mine ? 0 : (gd[e] & BL_NONE);
    const int cu = (i - r >= 0 && du != BL_NONE) ? du * du + r * r : INT_MAX;      // d <= 4095: d^2 + r^2 < 2^25
    const int cd = (i + r < H && dd != BL_NONE) ? dd * dd + r * r : INT_MAX;
    best = min(best, min(cu, cd));
  }
  return best;
}

// A workgroup takes units blockIdx.x, blockIdx.x + gridDim.x, ...; a unit is BL_THREADS consecutive pixels of one plane.
// An empty or a full plane is zeroed without a search (uniform over the unit).
__global__ __launch_bounds__(BL_THREADS) void boundary_columns_kernel(BlGeo geo, const unsigned short* __restrict__ g, const int* __restrict__ cnt,
                                                                      int* __restrict__ sd2) {
  const int H = geo.H, W = geo.W;
  for (int unit = blockIdx.x; unit < geo.units; unit += gridDim.x) {
    const int plane = unit / geo.tiles, tile = unit - plane * geo.tiles;
    const int pix = tile * BL_THREADS + (int)threadIdx.x;
    const bool live = pix < geo.HW;
    int* __restrict__ out = sd2 + (size_t)plane * geo.HW;
    const int* __restrict__ c = cnt + (size_t)plane * BL_CNT;
    const int ng = c[0];
    if (ng == 0 || ng == geo.HW) {
      if (live) out[pix] = 0;
      continue;
    }
    const unsigned short* __restrict__ gp = g + (size_t)plane * geo.HW;
    const int pc = live ? pix : geo.HW - 1;
    const int i = pc / W, j = pc - i * W;
    const int mine = gp[pc] & BL_IN;
    int best = live ? INT_MAX : 0;                   // a lane beyond the plane takes no round
    // only the rows lo .. hi hold a pixel of the other membership (the plane has both: lo <= hi): every other row would
    // answer with the sentinel, so the search starts at the nearer end of that range and ends at the farther one
    const int lo = mine ? c[3] : c[1], hi = mine ? c[4] : c[2];
    const int rmin = max(0, max(lo - i, i - hi)), rmax = max(i - lo, hi - i);
    // Several row pairs per round trip: the exit test depends on the loads.  A candidate beyond the stopping distance is
    // still a true distance to a pixel of the other membership: the minimum is the same.  The plane holds both
    // memberships, so the search ends with a hit.
    for (int r0 = rmin; r0 <= rmax && r0 * r0 < best; r0 += BL_STEP) best = bl_round<BL_STEP>(gp, i, j, H, W, r0, best, mine);
    if (live) out[pix] = mine ? -best : best;
  }
}

// phi = spacing sqrt(sd2) outside G, -spacing (sqrt(-sd2) - 1) inside, 0 at 0: edt(~G) ~G - (edt(G) - 1) G
__device__ __forceinline__ float bl_phi(int v, float sp) {
  const float r = sqrtf((float)(v < 0 ? -v : v));    // |sd2| < 2^25: exact in float
  return v > 0 ? sp * r : v < 0 ? -sp * (r - 1.f) : 0.f;
}

// The sum of a workgroup in a fixed tree -> part[blockIdx.x * n_items + item], by thread 0
__device__ __forceinline__ void bl_block_sum(double a, double* red, double* __restrict__ dst) {
  for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = 0.0;
    for (int q = 0; q < BL_THREADS / 64; ++q) v += red[q];
    *dst = v;
  }
  __syncthreads();
}

// One pass over all maps: map after map (the item table is in the kernel arguments), every workgroup its elements
// blockIdx.x * 256 + t, + gridDim.x * 256, ... -- the grid is fixed for a descriptor, and so is the order of every sum.
template <int MODE>
__global__ __launch_bounds__(BL_THREADS) void boundary_loss_kernel(const BlItems tab, const BlGeo geo, const void* __restrict__ target,
                                                                   const int* __restrict__ sd2, const float* __restrict__ scales,
                                                                   double* __restrict__ part) {
  __shared__ double red[BL_THREADS / 64];
  const float wgt = scales[0], bscale = scales[1], sp = geo.spacing;
  const long long stride = (long long)gridDim.x * BL_THREADS;
  for (int item = 0; item < geo.n_items; ++item) {
    const float* __restrict__ x = tab.it[item].logits;
    float* __restrict__ dl = tab.it[item].dlogits;
    const float coef = wgt * tab.it[item].weight * geo.inv_den;
    double acc = 0.0;
    for (long long e = (long long)blockIdx.x * BL_THREADS + threadIdx.x; e < geo.pixels; e += stride) {
      if (MODE == UZ_BOUNDARY_BINARY) {
        const float xv = x[e], phi = bl_phi(sd2[e], sp);
        const float a = expf(-fabsf(xv)), inv = 1.f / (1.f + a);
        const float p = xv >= 0.f ? inv : a * inv, q = xv >= 0.f ? a * inv : inv;      // sigmoid(x), 1 - sigmoid(x)
        acc += (double)p * (double)phi;
        if (dl != nullptr) dl[e] = bscale * dl[e] + coef * (phi * p * q);
      } else {
        const int n = (int)(e / geo.HW), pix = (int)(e - (long long)n * geo.HW);
        const int y = static_cast<const int*>(target)[e];
        const bool valid = y >= 0 && y < geo.K && y != geo.ignore_index;
        const size_t at = (size_t)n * geo.K * geo.HW + pix;
        const float* __restrict__ xp = x + at;
        const int* __restrict__ sp2 = sd2 + (size_t)n * geo.P * geo.HW + pix;
        float m = xp[0];
        for (int c = 1; c < geo.K; ++c) m = fmaxf(m, xp[(size_t)c * geo.HW]);
        float s = 0.f, dot = 0.f;
        for (int c = 0; c < geo.K; ++c) {
          const float ex = expf(xp[(size_t)c * geo.HW] - m);
          s += ex;
          if (c >= geo.first) dot = fmaf(ex, bl_phi(sp2[(size_t)(c - geo.first) * geo.HW], sp), dot);
        }
        const float inv = 1.f / s;
        dot *= inv;                                  // sum over Cset of p_c phi_c
        acc += valid ? (double)dot : 0.0;
        if (dl != nullptr) {
          float* __restrict__ dp = dl + at;
          for (int c = 0; c < geo.K; ++c) {
            const float pk = expf(xp[(size_t)c * geo.HW] - m) * inv;
            const float phit = c >= geo.first ? bl_phi(sp2[(size_t)(c - geo.first) * geo.HW], sp) : 0.f;
            const float gk = valid ? coef * (pk * (phit - dot)) : 0.f;      // exactly nothing at an ignored pixel
            dp[(size_t)c * geo.HW] = bscale * dp[(size_t)c * geo.HW] + gk;
          }
        }
      }
    }
    bl_block_sum(acc, red, part + (size_t)blockIdx.x * geo.n_items + item);
  }
}

// One workgroup: per map the workgroup sums in index order (thread t adds rows t, t + 256, ..., then a fixed tree)
__global__ __launch_bounds__(BL_THREADS) void boundary_finalize_kernel(const BlItems tab, const BlGeo geo, int nwg, const double* __restrict__ part,
                                                                       const float* __restrict__ scales, const float* __restrict__ base_loss,
                                                                       float* __restrict__ out) {
  __shared__ double red[BL_THREADS];
  double total = 0.0, metric = 0.0;                  // thread 0's
  for (int item = 0; item < geo.n_items; ++item) {
    double a = 0.0;
    for (int r = threadIdx.x; r < nwg; r += BL_THREADS) a += part[(size_t)r * geo.n_items + item];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = BL_THREADS / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const double B = red[0] * (double)geo.inv_den;
      total += (double)tab.it[item].weight * B;
      if (item == geo.metric_item) metric = B;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)((double)scales[1] * (double)base_loss[0] + (double)scales[0] * total);
    out[1] = (float)metric;
  }
}

struct BlPlan {
  BlGeo geo;
  int grid;                     // the column pass
  int rows_grid, planes_grid, loss_grid;
  long long off[4], bytes;      // g, cnt, part, rowinfo
};

int bl_plan(const uz_boundary_desc* d, const char* who, BlPlan* p) {
  UZ_REQUIRE(d != nullptr, "%s: null descriptor", who);
  UZ_REQUIRE(d->mode == UZ_BOUNDARY_BINARY || d->mode == UZ_BOUNDARY_CLASS, "%s: unknown mode %d", who, d->mode);
  UZ_REQUIRE(d->n_items >= 1 && d->n_items <= UZ_CLASS_MAX_ITEMS, "%s: n_items = %d outside [1, %d]", who, d->n_items, UZ_CLASS_MAX_ITEMS);
  UZ_REQUIRE(d->N >= 1 && d->C >= 1 && d->H >= 1 && d->W >= 1, "%s: non-positive shape", who);
  UZ_REQUIRE(d->H <= BL_MAX_HW && d->W <= BL_MAX_HW, "%s: H = %d, W = %d above %d", who, d->H, d->W, BL_MAX_HW);
  if (d->mode == UZ_BOUNDARY_CLASS) {
    UZ_REQUIRE(d->C >= 2 && d->C <= UZ_CLASS_MAX_K, "%s: K = %d outside [2, %d]", who, d->C, UZ_CLASS_MAX_K);
    UZ_REQUIRE(d->first_class >= 0 && d->first_class < d->C, "%s: first_class = %d outside [0, %d)", who, d->first_class, d->C);
  }
  UZ_REQUIRE(d->metric_item >= 0 && d->metric_item < d->n_items, "%s: metric_item = %d outside [0, %d)", who, d->metric_item, d->n_items);
  // written so that a NaN is refused too
  UZ_REQUIRE(d->spacing > 0.f && d->spacing < INFINITY, "%s: spacing must be positive and finite", who);
  UZ_REQUIRE((long long)d->N * d->C * d->H * d->W < (1LL << 31), "%s: too large (N C H W >= 2^31)", who);
  BlGeo& g = p->geo;
  const bool cls = d->mode == UZ_BOUNDARY_CLASS;
  g.mode = d->mode;
  g.n_items = d->n_items;
  g.N = d->N, g.K = d->C;
  g.first = cls ? d->first_class : 0;
  g.P = d->C - g.first;
  g.M = d->N * g.P;
  g.H = d->H, g.W = d->W, g.HW = d->H * d->W;
  g.tiles = uz_cdiv(g.HW, BL_THREADS);
  UZ_REQUIRE((long long)g.M * g.tiles < (1LL << 30), "%s: too many (plane, 256-pixel unit) items", who);
  g.units = g.M * g.tiles;
  g.ignore_index = d->ignore_index;
  g.metric_item = d->metric_item;
  g.spacing = d->spacing;
  g.inv_den = (float)(1.0 / ((double)g.M * (double)g.HW));
  g.pixels = cls ? (long long)d->N * g.HW : (long long)g.M * g.HW;
  // eight workgroups of four waves per CU of the hardware: what can be resident at once; more units than that are walked
  p->rows_grid = uz_grid_cap((long long)g.M * g.H, 8);
  p->planes_grid = uz_grid_cap(g.M, 8);
  p->grid = uz_grid_cap(g.units, 8);
  p->loss_grid = uz_grid_cap((g.pixels + BL_THREADS - 1) / BL_THREADS, 8);
  const long long sizes[4] = {2LL * g.M * g.HW, 4LL * g.M * BL_CNT, 8LL * p->loss_grid * g.n_items, 8LL * g.M * g.H};
  p->bytes = uz_carve(sizes, 4, p->off);
  return UZ_OK;
}

}  // namespace

extern "C" long long uz_boundary_workspace_bytes(const uz_boundary_desc* d) {
  BlPlan p;
  if (bl_plan(d, "uz_boundary_workspace_bytes", &p) != UZ_OK) return -1;
  return p.bytes;
}

extern "C" int uz_boundary_grid(const uz_boundary_desc* d, int* units) {
  BlPlan p;
  const int rc = bl_plan(d, "uz_boundary_grid", &p);
  if (rc != UZ_OK) return rc;
  if (units) *units = p.geo.units;
  return p.grid;
}

extern "C" int uz_boundary_loss(const uz_boundary_desc* d, const uz_boundary_item* items, const void* target, const float* scales,
                                const float* base_loss, float* out, int* sd2, void* workspace, void* stream) {
  BlPlan p;
  const int rc = bl_plan(d, "uz_boundary_loss", &p);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(items && target && scales && base_loss && out && sd2 && workspace, "uz_boundary_loss: null pointer");
  UZ_REQUIRE((((uintptr_t)target | (uintptr_t)scales | (uintptr_t)base_loss | (uintptr_t)out | (uintptr_t)sd2) & 3) == 0,
             "uz_boundary_loss: tensors must be 4-byte aligned");
  UZ_REQUIRE(((uintptr_t)workspace & 15) == 0, "uz_boundary_loss: the workspace must be 16-byte aligned");
  const BlGeo& g = p.geo;
  const long long map_bytes = 4LL * d->N * d->C * g.HW;
  // what the call writes (out, sd2, workspace, every dlogits) against everything else it touches
  UzRange in[3 + UZ_CLASS_MAX_ITEMS] = {uz_range(target, d->mode == UZ_BOUNDARY_CLASS ? 4LL * d->N * g.HW : map_bytes), uz_range(scales, 8),
                                        uz_range(base_loss, 4)};
  UzRange outr[3 + UZ_CLASS_MAX_ITEMS] = {uz_range(out, 8), uz_range(sd2, 4LL * g.M * g.HW), uz_range(workspace, p.bytes)};
  int n_in = 3, n_out = 3;
  BlItems tab;
  bool any_grad;      // the loss launch serves both: unused here
  const int irc = uz_map_items("uz_boundary_loss", items, d->n_items, map_bytes, in, &n_in, outr, &n_out, &any_grad, tab.it);
  if (irc != UZ_OK) return irc;
  UZ_REQUIRE(!uz_any_overlap(outr, n_out, in, n_in), "uz_boundary_loss: tensors overlap");
  char* base = static_cast<char*>(workspace);
  unsigned short* gw = reinterpret_cast<unsigned short*>(base + p.off[0]);
  int* cnt = reinterpret_cast<int*>(base + p.off[1]);
  double* part = reinterpret_cast<double*>(base + p.off[2]);
  int2* rowinfo = reinterpret_cast<int2*>(base + p.off[3]);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(BL_THREADS);
  const bool cls = d->mode == UZ_BOUNDARY_CLASS;

  const dim3 rgrid((unsigned)p.rows_grid);
  if (cls) hipLaunchKernelGGL((boundary_rows_kernel<UZ_BOUNDARY_CLASS>), rgrid, block, 0, s, g, target, gw, rowinfo);
  else hipLaunchKernelGGL((boundary_rows_kernel<UZ_BOUNDARY_BINARY>), rgrid, block, 0, s, g, target, gw, rowinfo);
  UZ_LAUNCH_CHECK("uz_boundary_loss(rows)");
  hipLaunchKernelGGL(boundary_planes_kernel, dim3((unsigned)p.planes_grid), block, 0, s, g, (const int2*)rowinfo, cnt);
  UZ_LAUNCH_CHECK("uz_boundary_loss(planes)");
  hipLaunchKernelGGL(boundary_columns_kernel, dim3((unsigned)p.grid), block, 0, s, g, (const unsigned short*)gw, (const int*)cnt, sd2);
  UZ_LAUNCH_CHECK("uz_boundary_loss(columns)");
  const dim3 lgrid((unsigned)p.loss_grid);
  if (cls) hipLaunchKernelGGL((boundary_loss_kernel<UZ_BOUNDARY_CLASS>), lgrid, block, 0, s, tab, g, target, (const int*)sd2, scales, part);
  else hipLaunchKernelGGL((boundary_loss_kernel<UZ_BOUNDARY_BINARY>), lgrid, block, 0, s, tab, g, target, (const int*)sd2, scales, part);
  UZ_LAUNCH_CHECK("uz_boundary_loss(loss)");
  hipLaunchKernelGGL(boundary_finalize_kernel, dim3(1), block, 0, s, tab, g, p.loss_grid, (const double*)part, scales, base_loss, out);
  UZ_LAUNCH_CHECK("uz_boundary_loss(finalize)");
  return UZ_OK;
}
