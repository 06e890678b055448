// Surface-distance metrics on the device: Hausdorff, percentile Hausdorff (HD95) and average symmetric surface distance of a
// thresholded prediction against its target, per (image, class) pair, exactly.  A = prediction, B = target.
//   S(X)   = pixels of X with a 4-neighbour outside X (outside the picture counts as outside X)
//   d2(p,S)= min over s in S of (pi - si)^2 + (pj - sj)^2          -- an INTEGER, below 2^25 for H, W <= 4096
//   D      = { d2(p, S(B)) : p in S(A) } + { d2(p, S(A)) : p in S(B) },  n = |S(A)| + |S(B)|
// Seven launches, every one with a fixed grid for a descriptor:
//   clear    the integer part of the workspace (counters, histograms)
//   codes    (prediction class, target class) of every pixel as two bytes; 255 = in no mask.  The binary mode is the class
//            mode with K = 2, first_class = 1 and every (image, channel) plane as an image of its own
//   rows     per (image, row): the surface bits of the row for every class and both masks, |X| and |S(X)| (integer atomics),
//            and g(i, j) = distance to the nearest surface pixel of row i, 16 bits, SF_NONE = the row has none
//   columns  per surface pixel (i, j) of one mask: d2 = min over i' of g_other(i', j)^2 + (i - i')^2, searched outwards from
//            i until (i - i')^2 >= the best; d2 goes to a dense int32 plane (-1: no query), into the first histogram
//            (d2 >> 12, integer atomics) and into max d2; sqrt(d2) is summed in float64 per unit in a fixed order
//   select1  per pair: the bins of the first histogram that hold ranks k and k + 1
//   level2   the low 12 bits of the d2 inside those two bins, histogrammed
//   finalize per pair: D_(k), D_(k+1), the unit sums in index order, the three values and the statistics
#include "uz_common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int SF_THREADS = 256;
constexpr int SF_NONE = 0xFFFF;       // g: no surface pixel in this row.  NEVER squared: every use selects on it first
constexpr int SF_LOW_BITS = 12;       // second histogram: the low 12 bits; first: d2 >> 12, 2^13 bins for d2 < 2^25
constexpr int SF_BINS1 = 1 << 13;
constexpr int SF_BINS2 = 1 << SF_LOW_BITS;
constexpr int SF_MAX_HW = 4096;
constexpr int SF_WORDS = SF_MAX_HW / 64;
constexpr int SF_STEP = 16;           // rows up and rows down of one round trip of the column search (8: 1 .. 4 % slower)
constexpr int SF_CNT = 8;             // counters of a pair: |A|, |B|, |S(A)|, |S(B)|, max d2, three spare

struct SfGeo {
  int mode;
  int M;        // images of the class formulation: N (class mode) or N * C (binary mode)
  int K;        // classes of an image; 2 in the binary mode
  int first;    // first class that is a pair
  int P;        // pairs per image: K - first
  int NP;       // M * P
  int H, W, HW;
  int tiles;    // units of SF_THREADS pixels per plane
  int units;    // 2 * NP * tiles: the column pass and the second histogram
  int ignore_index;
};

struct SfWs {
  unsigned short* codes;   // M * HW
  unsigned short* g;       // 2 * NP * HW, plane = pair * 2 + side
  int* d2;                 // 2 * NP * HW
  double* part;            // units
  int* nq;                 // units: 1 where the unit holds a query
  int* cnt;                // NP * SF_CNT      } cleared by every call
  int* hist1;              // NP * SF_BINS1    }
  int* hist2;              // NP * 2 * SF_BINS2}
  int* sel;                // NP * 4: bin of rank k, rank inside it, bin of rank k + 1, rank inside it (bins -1: no pair)
  long long nclear;        // ints from cnt on that a call clears
};

__global__ __launch_bounds__(SF_THREADS) void surface_clear_kernel(int4* __restrict__ p, long long n4) {
  for (long long i = (long long)blockIdx.x * SF_THREADS + threadIdx.x; i < n4; i += (long long)gridDim.x * SF_THREADS)
    p[i] = make_int4(0, 0, 0, 0);
}

// one pixel per thread and step; the K planes of a pixel are read unconditionally from a clamped pixel
template <int MODE>
__global__ __launch_bounds__(SF_THREADS) void surface_codes_kernel(SfGeo geo, const float* __restrict__ logits, const void* __restrict__ target,
                                                                   unsigned short* __restrict__ codes) {
  const long long total = (long long)geo.M * geo.HW;
  for (long long base = (long long)blockIdx.x * SF_THREADS; base < total; base += (long long)gridDim.x * SF_THREADS) {
    const long long e = base + threadIdx.x;
    const bool live = e < total;
    const long long ec = live ? e : total - 1;
    int pred, targ;
    if (MODE == UZ_SURFACE_BINARY) {
      const float x = logits[ec], t = static_cast<const float*>(target)[ec];
      pred = x > 0.f ? 1 : 0;
      targ = t > 0.5f ? 1 : 0;
    } else {
      const int m = (int)(ec / geo.HW), pix = (int)(ec - (long long)m * geo.HW);
      const float* __restrict__ x = logits + (size_t)m * geo.K * geo.HW + pix;
      const int y = static_cast<const int*>(target)[ec];
      float best = x[0];
      pred = 0;
      for (int c = 1; c < geo.K; ++c) {
        const float v = x[(size_t)c * geo.HW];
        const bool up = v > best;          // ties: the lowest index, as uz_class_loss
        best = up ? v : best;
        pred = up ? c : pred;
      }
      const bool valid = y >= 0 && y < geo.K && y != geo.ignore_index;
      targ = valid ? y : 255;
      pred = valid ? pred : 255;           // an ignored pixel belongs to neither mask of any class
    }
    if (live) codes[e] = (unsigned short)(pred | targ << 8);
  }
}

// A workgroup takes (image, row) units blockIdx.x, blockIdx.x + gridDim.x, ...: the codes of rows i - 1, i, i + 1 go to LDS
// once, then every class builds the surface bits of both masks (a wave's ballot is one 64-pixel word) and the row distances.
__global__ __launch_bounds__(SF_THREADS) void surface_rows_kernel(SfGeo geo, const unsigned short* __restrict__ codes,
                                                                  unsigned short* __restrict__ g, int* __restrict__ cnt) {
  __shared__ unsigned short row[3][SF_MAX_HW];
  __shared__ unsigned long long bits[2][SF_WORDS];
  __shared__ int tally[4];
  const int H = geo.H, W = geo.W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunks = (W + SF_THREADS - 1) / SF_THREADS, nwords = (W + 63) / 64;
  for (int unit = blockIdx.x; unit < geo.M * H; unit += gridDim.x) {
    const int m = unit / H, i = unit - m * H;
    const unsigned short* __restrict__ src = codes + (size_t)m * geo.HW;
    const int iu = i > 0 ? i - 1 : 0, id = i + 1 < H ? i + 1 : H - 1;
    for (int j = threadIdx.x; j < W; j += SF_THREADS) {
      const unsigned short a = src[(size_t)iu * W + j], b = src[(size_t)i * W + j], c = src[(size_t)id * W + j];
      row[0][j] = i > 0 ? a : (unsigned short)0xFFFF;       // outside the picture: in no mask
      row[1][j] = b;
      row[2][j] = i + 1 < H ? c : (unsigned short)0xFFFF;
    }
    if (threadIdx.x < 4) tally[threadIdx.x] = 0;
    __syncthreads();
    for (int cls = geo.first; cls < geo.K; ++cls) {
      const int pair = m * geo.P + (cls - geo.first);
      int in_n[2] = {0, 0}, sf_n[2] = {0, 0};
      for (int ch = 0; ch < chunks; ++ch) {
        const int j = ch * SF_THREADS + (int)threadIdx.x;
        const bool live = j < W;
        const int jc = live ? j : W - 1, jl = jc > 0 ? jc - 1 : 0, jr = jc + 1 < W ? jc + 1 : W - 1;
        const unsigned c0 = row[1][jc], cl = row[1][jl], cr = row[1][jr], cu = row[0][jc], cd = row[2][jc];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int sh = 8 * s;
          const bool in = live && (int)((c0 >> sh) & 255) == cls;
          const bool inner = jc > 0 && jc + 1 < W && (int)((cl >> sh) & 255) == cls && (int)((cr >> sh) & 255) == cls &&
                             (int)((cu >> sh) & 255) == cls && (int)((cd >> sh) & 255) == cls;
          const unsigned long long bi = __ballot(in), bs = __ballot(in && !inner);
          in_n[s] += __popcll(bi);
          sf_n[s] += __popcll(bs);
          if (lane == 0 && ch * 4 + wave < nwords) bits[s][ch * 4 + wave] = bs;
        }
      }
      if (lane == 0) {
        atomicAdd(&tally[0], in_n[0]);
        atomicAdd(&tally[1], in_n[1]);
        atomicAdd(&tally[2], sf_n[0]);
        atomicAdd(&tally[3], sf_n[1]);
      }
      __syncthreads();
      for (int j = threadIdx.x; j < W; j += SF_THREADS) {
        const int w0 = j >> 6, b = j & 63;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          int dist = SF_NONE;
          unsigned long long mk = bits[s][w0] & (~0ull >> (63 - b));      // surface pixels at or left of j
          int ww = w0;
          while (mk == 0 && ww > 0) mk = bits[s][--ww];
          if (mk) dist = j - (ww * 64 + 63 - __clzll((long long)mk));
          mk = bits[s][w0] & (~0ull << b);                                 // at or right of j
          ww = w0;
          while (mk == 0 && ww + 1 < nwords) mk = bits[s][++ww];
          if (mk) dist = min(dist, ww * 64 + __ffsll((unsigned long long)mk) - 1 - j);
          g[((size_t)(pair * 2 + s) * H + i) * W + j] = (unsigned short)dist;
        }
      }
      if (threadIdx.x < 4) {
        const int v = tally[threadIdx.x];
        if (v) atomicAdd(&cnt[(size_t)pair * SF_CNT + threadIdx.x], v);
        tally[threadIdx.x] = 0;
      }
      __syncthreads();
    }
  }
}

// hist[bin] += 1 for every lane with act, one atomic per distinct bin of the wave.  Called by all 64 lanes together.
__device__ __forceinline__ void sf_wave_hist(int* __restrict__ hist, int bin, bool act) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(act);
  while (todo) {
    const int leader = __ffsll(todo) - 1;
    const int b = __shfl(bin, leader);
    const unsigned long long same = __ballot(act && bin == b);
    if (lane == leader) atomicAdd(hist + b, __popcll(same));
    act = act && bin != b;
    todo &= ~same;
  }
}

// min(best, g_other(i -+ r, j)^2 + r^2 for r = r0 .. r0 + S - 1): 2 S loads issued together, unconditional from clamped rows;
// the sentinel and the picture's edge are selected afterwards
template <int S>
__device__ __forceinline__ int sf_round(const unsigned short* __restrict__ go, int i, int j, int H, int W, int r0, int best) {
  int gu[S], gd[S];
#pragma unroll
  for (int e = 0; e < S; ++e) {
    gu[e] = go[(size_t)max(i - r0 - e, 0) * W + j];
    gd[e] = go[(size_t)min(i + r0 + e, H - 1) * W + j];
  }
#pragma unroll
  for (int e = 0; e < S; ++e) {
    const int r = r0 + e;
    const int cu = (i - r >= 0 && gu[e] != SF_NONE) ? gu[e] * gu[e] + r * r : INT_MAX;      // g <= 4095: g^2 + r^2 < 2^25
    const int cd = (i + r < H && gd[e] != SF_NONE) ? gd[e] * gd[e] + r * r : INT_MAX;
    best = min(best, min(cu, cd));
  }
  return best;
}

// A workgroup takes units blockIdx.x, blockIdx.x + gridDim.x, ...; a unit is SF_THREADS consecutive pixels of one plane
// (pair, side).  The loads of a round are unconditional from clamped rows, the sentinel and the picture's edge are selected
// afterwards; a lane that is no query starts with best = 0 and takes no round.
__global__ __launch_bounds__(SF_THREADS) void surface_columns_kernel(SfGeo geo, const unsigned short* __restrict__ g, int* __restrict__ d2,
                                                                     double* __restrict__ part, int* __restrict__ nq, int* __restrict__ cnt,
                                                                     int* __restrict__ hist1) {
  __shared__ double ssum[SF_THREADS];
  __shared__ int smax[SF_THREADS];
  const int H = geo.H, W = geo.W;
  for (int unit = blockIdx.x; unit < geo.units; unit += gridDim.x) {
    const int plane = unit / geo.tiles, tile = unit - plane * geo.tiles;
    const int pair = plane >> 1;
    const unsigned short* __restrict__ gs = g + (size_t)plane * geo.HW;
    const unsigned short* __restrict__ go = g + (size_t)(plane ^ 1) * geo.HW;
    const int pix = tile * SF_THREADS + (int)threadIdx.x;
    const bool live = pix < geo.HW;
    const int pc = live ? pix : geo.HW - 1;
    const int i = pc / W, j = pc - i * W;
    // nothing to search for when the other mask is empty (uniform over the unit): the pair has no distances
    const bool query = live && gs[pc] == 0 && cnt[(size_t)pair * SF_CNT + ((plane & 1) ^ 1)] > 0;
    if (!__syncthreads_or(query)) {                  // most units of compact masks hold no surface pixel: nothing to do, and
      if (threadIdx.x == 0) {                        // the second histogram skips the unit, so its d2 are not written either
        part[unit] = 0.0;
        nq[unit] = 0;
      }
      continue;
    }
    int best = query ? INT_MAX : 0;
    const int rmax = max(i, H - 1 - i);              // beyond it both rows lie outside the picture
    // Several row pairs per round trip: the exit test depends on the loads, so one pair at a time costs one memory latency
    // per row.  A candidate beyond the stopping distance is still a true distance to a surface pixel: the minimum is the same.
    for (int r0 = 0; r0 <= rmax && r0 * r0 < best; r0 += SF_STEP) best = sf_round<SF_STEP>(go, i, j, H, W, r0, best);
    const bool hit = query && best != INT_MAX;       // no hit: the other mask is empty, the pair has no distances
    if (live) d2[(size_t)plane * geo.HW + pix] = hit ? best : -1;
    sf_wave_hist(hist1 + (size_t)pair * SF_BINS1, best >> SF_LOW_BITS, hit);
    ssum[threadIdx.x] = hit ? sqrt((double)best) : 0.0;
    smax[threadIdx.x] = hit ? best : 0;
    __syncthreads();
    for (int s = SF_THREADS / 2; s > 0; s >>= 1) {   // a fixed tree: the unit's sum does not depend on the grid
      if ((int)threadIdx.x < s) {
        ssum[threadIdx.x] += ssum[threadIdx.x + s];
        smax[threadIdx.x] = max(smax[threadIdx.x], smax[threadIdx.x + s]);
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      part[unit] = ssum[0];
      nq[unit] = 1;
      if (smax[0] > 0) atomicMax(&cnt[(size_t)pair * SF_CNT + 4], smax[0]);
    }
    __syncthreads();
  }
}

// state of a pair from |A|, |B|
__device__ __forceinline__ int sf_state(int na, int nb) { return (na == 0 ? 1 : 0) | (nb == 0 ? 2 : 0); }

// ranks k and k1 = min(k + 1, n - 1) of the n distances and the weight f of the upper one
__device__ __forceinline__ void sf_ranks(int n, double qf, int* k, int* k1, double* f) {
  const double r = (double)(n - 1) * qf;
  int kk = (int)floor(r);
  kk = kk < 0 ? 0 : kk > n - 1 ? n - 1 : kk;
  *k = kk;
  *k1 = kk + 1 < n - 1 ? kk + 1 : n - 1;
  *f = r - (double)kk;
}

// (bin, rank inside the bin) of rank k in an LDS histogram whose chunk sums (`per` bins each, chunk t = thread t's) are in
// csum, written to res[0..1] by the one thread whose chunk holds the rank.  Called by all threads; no loop waits for the
// value it has just read, so the LDS reads overlap.  The last chunk answers when the histogram holds fewer than k + 1.
__device__ __forceinline__ void sf_find(const int* h, const int* csum, int per, int k, int* res) {
  const int t = threadIdx.x;
  int excl = 0;
  for (int u = 0; u < t; ++u) excl += csum[u];
  if (excl <= k && (k < excl + csum[t] || t == SF_THREADS - 1)) {
    int b = 0, before = excl, run = excl;
    for (int e = 0; e < per - 1; ++e) {
      run += h[t * per + e];
      const bool pass = run <= k;
      b = pass ? e + 1 : b;
      before = pass ? run : before;
    }
    res[0] = t * per + b;
    res[1] = k - before;
  }
}

__global__ __launch_bounds__(SF_THREADS) void surface_select1_kernel(SfGeo geo, double qf, const int* __restrict__ cnt,
                                                                     const int* __restrict__ hist1, int* __restrict__ sel) {
  __shared__ int h[SF_BINS1];
  __shared__ int csum[SF_THREADS];
  const int pair = blockIdx.x;
  constexpr int PER = SF_BINS1 / SF_THREADS;
  const int* __restrict__ src = hist1 + (size_t)pair * SF_BINS1;
  for (int b = threadIdx.x; b < SF_BINS1; b += SF_THREADS) h[b] = src[b];
  __syncthreads();
  int s = 0;
  for (int b = 0; b < PER; ++b) s += h[threadIdx.x * PER + b];
  csum[threadIdx.x] = s;
  __syncthreads();
  const int* c = cnt + (size_t)pair * SF_CNT;
  if (sf_state(c[0], c[1]) == 0) {                   // uniform
    int k, k1;
    double f;
    sf_ranks(c[2] + c[3], qf, &k, &k1, &f);
    sf_find(h, csum, PER, k, sel + pair * 4);
    sf_find(h, csum, PER, k1, sel + pair * 4 + 2);
  } else if (threadIdx.x < 4) {
    sel[pair * 4 + threadIdx.x] = threadIdx.x & 1 ? 0 : -1;
  }
}

__global__ __launch_bounds__(SF_THREADS) void surface_level2_kernel(SfGeo geo, const int* __restrict__ d2, const int* __restrict__ nq,
                                                                    const int* __restrict__ sel, int* __restrict__ hist2) {
  for (int unit = blockIdx.x; unit < geo.units; unit += gridDim.x) {
    const int plane = unit / geo.tiles, tile = unit - plane * geo.tiles;
    const int pair = plane >> 1;
    const int bk = sel[pair * 4], bk1 = sel[pair * 4 + 2];
    if (bk < 0 || nq[unit] == 0) continue;           // uniform: the pair has no distances, or the unit no query
    const int pix = tile * SF_THREADS + (int)threadIdx.x;
    const bool live = pix < geo.HW;
    const int v = d2[(size_t)plane * geo.HW + (live ? pix : geo.HW - 1)];
    const bool hit = live && v >= 0;
    const int hi = v >> SF_LOW_BITS, lo = v & (SF_BINS2 - 1);
    int* __restrict__ h = hist2 + (size_t)pair * 2 * SF_BINS2;
    sf_wave_hist(h, lo, hit && hi == bk);
    sf_wave_hist(h + SF_BINS2, lo, hit && hi == bk1);
  }
}

__global__ __launch_bounds__(SF_THREADS) void surface_finalize_kernel(SfGeo geo, double qf, double spacing, const int* __restrict__ cnt,
                                                                      const int* __restrict__ sel, const int* __restrict__ hist2,
                                                                      const double* __restrict__ part, float* __restrict__ out,
                                                                      long long* __restrict__ stats) {
  __shared__ int h[2][SF_BINS2];
  __shared__ int csum[2][SF_THREADS];
  __shared__ double ssum[2][SF_THREADS];
  __shared__ int found[4];
  const int pair = blockIdx.x;
  constexpr int PER = SF_BINS2 / SF_THREADS;
  const int* __restrict__ src = hist2 + (size_t)pair * 2 * SF_BINS2;
  for (int b = threadIdx.x; b < 2 * SF_BINS2; b += SF_THREADS) h[b / SF_BINS2][b % SF_BINS2] = src[b];
  // the unit sums of each side: thread t adds units t, t + 256, ... in that order, then a fixed tree
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const double* __restrict__ p = part + (size_t)(pair * 2 + s) * geo.tiles;
    double a = 0.0;
    for (int t = threadIdx.x; t < geo.tiles; t += SF_THREADS) a += p[t];
    ssum[s][threadIdx.x] = a;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    int a = 0;
    for (int b = 0; b < PER; ++b) a += h[s][threadIdx.x * PER + b];
    csum[s][threadIdx.x] = a;
  }
  for (int w = SF_THREADS / 2; w > 0; w >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < w) {
      ssum[0][threadIdx.x] += ssum[0][threadIdx.x + w];
      ssum[1][threadIdx.x] += ssum[1][threadIdx.x + w];
    }
  }
  __syncthreads();
  const int* c = cnt + (size_t)pair * SF_CNT;
  const int state = sf_state(c[0], c[1]);
  if (state == 0) {                                  // uniform
    sf_find(h[0], csum[0], PER, sel[pair * 4 + 1], found);
    sf_find(h[1], csum[1], PER, sel[pair * 4 + 3], found + 2);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double hd = 0.0, hdq = 0.0, assd = 0.0;
    long long dmax = 0, dk = 0, dk1 = 0;
    if (state == 0) {
      int k, k1;
      double f;
      sf_ranks(c[2] + c[3], qf, &k, &k1, &f);
      dk = ((long long)sel[pair * 4] << SF_LOW_BITS) | found[0];
      dk1 = ((long long)sel[pair * 4 + 2] << SF_LOW_BITS) | found[2];
      dmax = c[4];
      const double lo = sqrt((double)dk), hi = sqrt((double)dk1);
      hd = spacing * sqrt((double)dmax);
      hdq = spacing * (lo + f * (hi - lo));
      assd = spacing * 0.5 * (ssum[0][0] / (double)c[2] + ssum[1][0] / (double)c[3]);
    }
    float* o = out + (size_t)pair * 4;
    o[0] = (float)hd, o[1] = (float)hdq, o[2] = (float)assd, o[3] = 0.f;
    long long* st = stats + (size_t)pair * 8;
    st[0] = c[2], st[1] = c[3], st[2] = dmax, st[3] = dk, st[4] = dk1, st[5] = state, st[6] = c[0], st[7] = c[1];
  }
}

struct SfPlan {
  SfGeo geo;
  int grid;                     // the column pass and the second histogram
  int clear_grid, codes_grid, rows_grid;
  long long off[9], bytes;      // codes, g, d2, part, nq, cnt, hist1, hist2, sel
};

int sf_plan(const uz_surface_desc* d, const char* who, SfPlan* p) {
  UZ_REQUIRE(d != nullptr, "%s: null descriptor", who);
  UZ_REQUIRE(d->mode == UZ_SURFACE_BINARY || d->mode == UZ_SURFACE_CLASS, "%s: unknown mode %d", who, d->mode);
  UZ_REQUIRE(d->N >= 1 && d->C >= 1 && d->H >= 1 && d->W >= 1, "%s: non-positive shape", who);
  UZ_REQUIRE(d->H <= SF_MAX_HW && d->W <= SF_MAX_HW, "%s: H = %d, W = %d above %d", who, d->H, d->W, SF_MAX_HW);
  if (d->mode == UZ_SURFACE_CLASS) {
    UZ_REQUIRE(d->C >= 2 && d->C <= UZ_CLASS_MAX_K, "%s: K = %d outside [2, %d]", who, d->C, UZ_CLASS_MAX_K);
    UZ_REQUIRE(d->first_class >= 0 && d->first_class < d->C, "%s: first_class = %d outside [0, %d)", who, d->first_class, d->C);
  }
  // written so that a NaN is refused too
  UZ_REQUIRE(d->q > 0.0 && d->q <= 100.0, "%s: q outside (0, 100]", who);
  UZ_REQUIRE(d->spacing > 0.0 && d->spacing < (double)INFINITY, "%s: spacing must be positive and finite", who);
  UZ_REQUIRE((long long)d->N * d->C * d->H * d->W < (1LL << 31), "%s: too large (N C H W >= 2^31)", who);
  SfGeo& g = p->geo;
  const bool cls = d->mode == UZ_SURFACE_CLASS;
  g.mode = d->mode;
  g.M = cls ? d->N : d->N * d->C;
  g.K = cls ? d->C : 2;
  g.first = cls ? d->first_class : 1;
  g.P = g.K - g.first;
  g.NP = g.M * g.P;
  g.H = d->H, g.W = d->W, g.HW = d->H * d->W;
  g.tiles = uz_cdiv(g.HW, SF_THREADS);
  UZ_REQUIRE(2LL * g.NP * g.tiles < (1LL << 30), "%s: too many (pair, 256-pixel unit) items", who);
  g.units = 2 * g.NP * g.tiles;
  g.ignore_index = d->ignore_index;
  // eight workgroups of four waves per CU of the hardware: what can be resident at once; more units than that are walked
  p->grid = uz_grid_cap(g.units, 8);
  p->codes_grid = uz_grid_cap(((long long)g.M * g.HW + SF_THREADS - 1) / SF_THREADS, 8);
  p->rows_grid = uz_grid_cap((long long)g.M * g.H, 8);
  const long long planes = 2LL * g.NP * g.HW;
  const long long sizes[9] = {2LL * g.M * g.HW, 2 * planes, 4 * planes, 8LL * g.units, 4LL * g.units, 4LL * g.NP * SF_CNT,
                              4LL * g.NP * SF_BINS1, 8LL * g.NP * SF_BINS2, 16LL * g.NP};
  p->bytes = uz_carve(sizes, 9, p->off);
  p->clear_grid = uz_grid_cap(uz_cdiv((p->off[8] - p->off[5]) / 16, SF_THREADS), 8);      // cnt, hist1, hist2 as int4
  return UZ_OK;
}

}  // namespace

extern "C" long long uz_surface_workspace_bytes(const uz_surface_desc* d) {
  SfPlan p;
  if (sf_plan(d, "uz_surface_workspace_bytes", &p) != UZ_OK) return -1;
  return p.bytes;
}

extern "C" int uz_surface_grid(const uz_surface_desc* d, int* units) {
  SfPlan p;
  const int rc = sf_plan(d, "uz_surface_grid", &p);
  if (rc != UZ_OK) return rc;
  if (units) *units = p.geo.units;
  return p.grid;
}

extern "C" int uz_surface_metrics(const uz_surface_desc* d, const float* logits, const void* target, float* out, long long* stats,
                                  void* workspace, void* stream) {
  SfPlan p;
  const int rc = sf_plan(d, "uz_surface_metrics", &p);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(logits && target && out && stats && workspace, "uz_surface_metrics: null pointer");
  UZ_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)target & 3) == 0 && ((uintptr_t)out & 3) == 0,
             "uz_surface_metrics: tensors must be 4-byte aligned");
  UZ_REQUIRE(((uintptr_t)stats & 7) == 0, "uz_surface_metrics: stats must be 8-byte aligned");
  UZ_REQUIRE(((uintptr_t)workspace & 15) == 0, "uz_surface_metrics: the workspace must be 16-byte aligned");
  const SfGeo& g = p.geo;
  const long long px = (long long)d->N * d->H * d->W;
  const UzRange r[5] = {uz_range(logits, 4LL * px * d->C), uz_range(target, d->mode == UZ_SURFACE_CLASS ? 4LL * px : 4LL * px * d->C),
                        uz_range(out, 16LL * g.NP), uz_range(stats, 64LL * g.NP), uz_range(workspace, p.bytes)};
  UZ_REQUIRE(!uz_any_overlap(r, 5, nullptr, 0), "uz_surface_metrics: tensors overlap");
  char* base = static_cast<char*>(workspace);
  SfWs ws;
  ws.codes = reinterpret_cast<unsigned short*>(base + p.off[0]);
  ws.g = reinterpret_cast<unsigned short*>(base + p.off[1]);
  ws.d2 = reinterpret_cast<int*>(base + p.off[2]);
  ws.part = reinterpret_cast<double*>(base + p.off[3]);
  ws.nq = reinterpret_cast<int*>(base + p.off[4]);
  ws.cnt = reinterpret_cast<int*>(base + p.off[5]);
  ws.hist1 = reinterpret_cast<int*>(base + p.off[6]);
  ws.hist2 = reinterpret_cast<int*>(base + p.off[7]);
  ws.sel = reinterpret_cast<int*>(base + p.off[8]);
  ws.nclear = (p.off[8] - p.off[5]) / 4;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(SF_THREADS);
  const double qf = d->q / 100.0;

  hipLaunchKernelGGL(surface_clear_kernel, dim3((unsigned)p.clear_grid), block, 0, s, reinterpret_cast<int4*>(ws.cnt), ws.nclear / 4);
  UZ_LAUNCH_CHECK("uz_surface_metrics(clear)");
  const dim3 cgrid((unsigned)p.codes_grid);
  if (d->mode == UZ_SURFACE_BINARY) hipLaunchKernelGGL((surface_codes_kernel<UZ_SURFACE_BINARY>), cgrid, block, 0, s, g, logits, target, ws.codes);
  else hipLaunchKernelGGL((surface_codes_kernel<UZ_SURFACE_CLASS>), cgrid, block, 0, s, g, logits, target, ws.codes);
  UZ_LAUNCH_CHECK("uz_surface_metrics(codes)");
  hipLaunchKernelGGL(surface_rows_kernel, dim3((unsigned)p.rows_grid), block, 0, s, g, (const unsigned short*)ws.codes, ws.g, ws.cnt);
  UZ_LAUNCH_CHECK("uz_surface_metrics(rows)");
  hipLaunchKernelGGL(surface_columns_kernel, dim3((unsigned)p.grid), block, 0, s, g, (const unsigned short*)ws.g, ws.d2, ws.part, ws.nq, ws.cnt, ws.hist1);
  UZ_LAUNCH_CHECK("uz_surface_metrics(columns)");
  hipLaunchKernelGGL(surface_select1_kernel, dim3((unsigned)g.NP), block, 0, s, g, qf, (const int*)ws.cnt, (const int*)ws.hist1, ws.sel);
  UZ_LAUNCH_CHECK("uz_surface_metrics(select1)");
  hipLaunchKernelGGL(surface_level2_kernel, dim3((unsigned)p.grid), block, 0, s, g, (const int*)ws.d2, (const int*)ws.nq, (const int*)ws.sel, ws.hist2);
  UZ_LAUNCH_CHECK("uz_surface_metrics(level2)");
  hipLaunchKernelGGL(surface_finalize_kernel, dim3((unsigned)g.NP), block, 0, s, g, qf, d->spacing, (const int*)ws.cnt, (const int*)ws.sel,
                     (const int*)ws.hist2, (const double*)ws.part, out, stats);
  UZ_LAUNCH_CHECK("uz_surface_metrics(finalize)");
  return UZ_OK;
}
