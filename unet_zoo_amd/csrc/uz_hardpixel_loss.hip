// Hard-pixel mining (top-k cross-entropy as in nnU-Net's DC_and_topk, OHEM cross-entropy as in mmseg's OHEMPixelSampler,
// focal loss: Lin et al., "Focal Loss for Dense Object Detection", ICCV 2017) on the device, added to a base loss whose
// value and gradients already exist (include/unetzoo_hip.h).  The library's exact k-th-largest selection: an
// MSB-first radix select over the bit patterns of the per-pixel losses -- counts only, nothing is moved.
//   geometry  the f of a map is one fp32 per element (binary mode, N C H W) or per pixel (class mode, N H W): P values a
//             map; a segment is the whole of them (L = P) or one image's (per_image, L = P / N), always a contiguous range:
//             S = 1 or N segments a map, GS = n_items S in the call; a unit is (segment, chunk), a chunk HP_TILE * tpr
//             consecutive elements of a segment with tpr the smallest integer that leaves at most HP_MAX_ROWS chunks
//   key       bits(f): f >= 0, so the bit pattern orders as an unsigned integer; 0xFFFFFFFF for a pixel that is in no segment
//   digit     8 bits, most significant first: 4 rounds.  A unit counts its digits in LDS integer atomics on HP_COPIES copies
//             of the 256 bins, copy = lane mod HP_COPIES: the losses of a trained network share a few exponents, so most
//             lanes of a wave hit ONE bin of the first digit -- 64 adds on one address become 4 on each of 16 addresses in 16
//             different banks, whatever the data.  Copy q of bin b lies at q * HP_PITCH + b with HP_PITCH = 257: the copies
//             of one bin fall on banks b + q, and the read-out (thread = bin, copy after copy) is a run of 256 consecutive
//             words, conflict-free; the copies are summed when the unit's row is stored
// Launches, every one with a fixed grid for a descriptor (10, whatever the data and with or without gradient buffers):
//   loss      f of every element of every map, `losses` of the main map, per unit: n (valid), c (l > -log max_prob) and
//             the first digit's 256 counts
//   pick 0    per segment: n, c, m = max(k, c), the segments of its map with n > 0; the units' rows added (integers: any
//             order gives the same), the bins scanned from the top: the first digit and the rank that remains
//   3 x (hist, pick)   hist: per unit the next digit's counts over the elements that match the prefix found so far;
//             pick as above; the last one knows tau to the bit, n_above and n_tie and writes `selection`
//   grad      per unit: the float64 sum of f over f > tau (every thread its elements in index order, then a fixed tree);
//             where a map has a gradient buffer: dl <- base_scale dl + weight ow dV/dx, p recomputed from the logits
//   finalize  per map the segments' values from the units' sums in index order, out[0] and out[1]
// No workgroup waits for another inside a launch, no float atomics, nothing to clear: every counter is a plain store.  The
// float64 sums are per UNIT, not per workgroup: a capped grid (max_workgroups) walks the same units and gives the same bits.
#include "uz_common.h"

#include <float.h>
#include <math.h>

namespace {

constexpr int HP_THREADS = 256;
constexpr int HP_WAVES = HP_THREADS / 64;
constexpr int HP_TILE = 2048;                     // elements: the smallest chunk
constexpr int HP_MAX_ROWS = 256;                  // chunks of a segment at most: what a pick adds per bin
constexpr int HP_BINS = 256;                      // 8 bits a round
constexpr int HP_DIGITS = 4;
constexpr int HP_COPIES = 16;                     // of every bin in LDS, one per lane mod 16
constexpr int HP_PITCH = HP_BINS + 1;             // words from one copy of the bins to the next: bank = (bin + copy) mod 32
constexpr int HP_LDS = HP_COPIES * HP_PITCH;
constexpr int HP_MAX_SEGS = 1 << 16;              // segments of a call: pick 0 walks the counters of a map's segments
constexpr int HP_PICK_THREADS = 1024;
constexpr int HP_PICK_GROUPS = HP_PICK_THREADS / HP_BINS;
constexpr int HP_STATE = 8;                       // ints of a segment's state
constexpr unsigned HP_NONE = 0xFFFFFFFFu;
constexpr long long HP_MAX_SEG = 1LL << 24;       // elements of one segment: (float)n is exact
constexpr long long HP_MAX_ELEMS = 1LL << 28;     // elements of all maps of a call

enum { ST_PREFIX, ST_RANK, ST_ABOVE, ST_M, ST_N, ST_TIE, ST_NSEG, ST_C };

struct HpItems {
  uz_hardpixel_item it[UZ_CLASS_MAX_ITEMS];
};

struct HpGeo {
  int mode;
  int n_items;
  int N, C, HW;
  int S;             // segments per map: N (per_image) or 1
  int GS;            // segments of the call: n_items * S
  int L;             // elements of a segment
  int chunk;         // elements of a unit: HP_TILE * tpr
  int tps;           // chunks per segment, <= HP_MAX_ROWS
  int units;         // GS * tps
  int ignore_index;
  int main_item;
  int min_kept;
  float keep;
  float thr;         // c counts l > thr = -log(max_prob); +inf: off
  float gamma;
  long long P;       // f values of a map: N C H W (binary) or N H W (class)
  long long E;       // elements of a map: N C H W
};

template <int WAVES>
__device__ __forceinline__ int hp_block_sum(int v, int* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
  for (int q = 0; q < WAVES; ++q) t += red[q];
  __syncthreads();
  return t;
}

// f = q^gamma l and df/dl = q^gamma + gamma q^(gamma - 1) p_t l with q = 1 - p_t; gamma = 0: f = l and df/dl = 1 exactly.
// p_t is exp(-l), not 1 - q: at a hard pixel (q near 1, l large) the difference would carry q's rounding times gamma l
__device__ __forceinline__ float hp_focal(float q, float l, float gamma, float* dfdl) {
  if (gamma == 0.f) {
    *dfdl = 1.f;
    return l;
  }
  const float qg1 = gamma == 1.f ? 1.f : (gamma == 2.f ? q : powf(q, gamma - 1.f));
  const float qg = qg1 * q;
  *dfdl = qg + gamma * qg1 * expf(-l) * l;
  return qg * l;
}

// Binary mode: z = -s x, l = softplus(z) = max(z, 0) + log1p(exp(-|x|)), q = 1 - p_t = sigmoid(z)
__device__ __forceinline__ float hp_binary(float x, bool b, float* q) {
  const float z = b ? -x : x;
  const float e = expf(-fabsf(x));
  *q = (z >= 0.f ? 1.f : e) / (1.f + e);
  return fmaxf(z, 0.f) + log1pf(e);
}

// Class mode: l = logsumexp_K(x) - x_y = log1p(sum_{c != top} exp(x_c - max)) + (max - x_y), both terms >= 0; the K planes
// are walked twice, nothing per class is held.  *inv = p_top, *rest = (1 - p_top) / p_top, q = 1 - p_y without a
// difference of near-equals where y is the class of the largest logit
__device__ __forceinline__ float hp_class(const float* __restrict__ xp, int K, int HW, int y, float* mx, int* top, float* rest, float* inv,
                                          float* q) {
  float m = xp[0], xy = xp[0];
  int t = 0;
  for (int c = 1; c < K; ++c) {
    const float v = xp[(size_t)c * HW];
    xy = c == y ? v : xy;
    t = v > m ? c : t;
    m = v > m ? v : m;
  }
  float r = 0.f;
  for (int c = 0; c < K; ++c) r += c == t ? 0.f : expf(xp[(size_t)c * HW] - m);
  const float i = 1.f / (1.f + r);
  *mx = m, *top = t, *rest = r, *inv = i;
  *q = y == t ? r * i : 1.f - expf(xy - m) * i;
  return fmaxf(log1pf(r) + (m - xy), 0.f);
}

// the unit's row: the copies of every bin added, bin = thread; n and c of the unit
__device__ __forceinline__ void hp_store_row(const int* h, int* __restrict__ hist, int unit) {
  int v = 0;
  for (int q = 0; q < HP_COPIES; ++q) v += h[q * HP_PITCH + threadIdx.x];
  hist[(size_t)unit * HP_BINS + threadIdx.x] = v;
}

__device__ __forceinline__ void hp_clear(int* h) {
  for (int q = threadIdx.x; q < HP_LDS; q += HP_THREADS) h[q] = 0;
}

__global__ __launch_bounds__(HP_THREADS) void hardpixel_loss_binary_kernel(const HpItems tab, const HpGeo geo, const float* __restrict__ target,
                                                                           unsigned* __restrict__ fbits, float* __restrict__ losses,
                                                                           int* __restrict__ hist, int* __restrict__ cnt) {
  __shared__ int h[HP_LDS];
  __shared__ int red[HP_WAVES];
  const int copy = (threadIdx.x & (HP_COPIES - 1)) * HP_PITCH;
  for (int unit = blockIdx.x; unit < geo.units; unit += gridDim.x) {
    const int gseg = unit / geo.tps, tile = unit - gseg * geo.tps;
    const int item = gseg / geo.S, s = gseg - item * geo.S;
    const float* __restrict__ x = tab.it[item].logits;
    hp_clear(h);
    __syncthreads();
    const int end = min(geo.L, (tile + 1) * geo.chunk);
    int n = 0, c = 0;
    for (int j = tile * geo.chunk + (int)threadIdx.x; j < end; j += HP_THREADS) {
      const size_t a = (size_t)s * geo.L + j;           // a segment is a contiguous range of the map
      float q, dfdl;
      const float l = hp_binary(x[a], target[a] > 0.5f, &q);
      const float f = hp_focal(q, l, geo.gamma, &dfdl);
      unsigned bits = __float_as_uint(f);
      bits = f >= 0.f ? bits : HP_NONE;                 // a NaN is in no segment
      fbits[(size_t)item * geo.P + a] = bits;
      if (item == geo.main_item) losses[a] = f;
      if (bits != HP_NONE) {
        atomicAdd(&h[copy + (bits >> 24)], 1);      // an integer count in LDS: the same whatever the order
        n += 1;
        c += l > geo.thr ? 1 : 0;
      }
    }
    __syncthreads();
    hp_store_row(h, hist, unit);
    n = hp_block_sum<HP_WAVES>(n, red);
    c = hp_block_sum<HP_WAVES>(c, red);
    if (threadIdx.x == 0) cnt[2 * unit] = n, cnt[2 * unit + 1] = c;
  }
}

__global__ __launch_bounds__(HP_THREADS) void hardpixel_loss_class_kernel(const HpItems tab, const HpGeo geo, const int* __restrict__ target,
                                                                          unsigned* __restrict__ fbits, float* __restrict__ losses,
                                                                          int* __restrict__ hist, int* __restrict__ cnt) {
  __shared__ int h[HP_LDS];
  __shared__ int red[HP_WAVES];
  const int copy = (threadIdx.x & (HP_COPIES - 1)) * HP_PITCH;
  const int K = geo.C;
  for (int unit = blockIdx.x; unit < geo.units; unit += gridDim.x) {
    const int gseg = unit / geo.tps, tile = unit - gseg * geo.tps;
    const int item = gseg / geo.S, s = gseg - item * geo.S;
    const float* __restrict__ x = tab.it[item].logits;
    hp_clear(h);
    __syncthreads();
    const int end = min(geo.L, (tile + 1) * geo.chunk);
    int n = 0, c = 0;
    for (int j = tile * geo.chunk + (int)threadIdx.x; j < end; j += HP_THREADS) {
      const long long px = (long long)s * geo.L + j;    // pixel of the batch
      const int img = (int)(px / geo.HW), pix = (int)(px - (long long)img * geo.HW);
      const int y = target[px];
      const bool valid = y >= 0 && y < K && y != geo.ignore_index;
      unsigned bits = HP_NONE;
      float f = 0.f;
      if (valid) {
        float mx, rest, inv, q, dfdl;
        int top;
        const float l = hp_class(x + (size_t)img * K * geo.HW + pix, K, geo.HW, y, &mx, &top, &rest, &inv, &q);
        f = hp_focal(-expm1f(-l), l, geo.gamma, &dfdl);
        bits = f >= 0.f ? __float_as_uint(f) : HP_NONE;
        if (bits != HP_NONE) {
          atomicAdd(&h[copy + (bits >> 24)], 1);
          n += 1;
          c += l > geo.thr ? 1 : 0;
        }
      }
      fbits[(size_t)item * geo.P + px] = bits;
      if (item == geo.main_item) losses[px] = f;
    }
    __syncthreads();
    hp_store_row(h, hist, unit);
    n = hp_block_sum<HP_WAVES>(n, red);
    c = hp_block_sum<HP_WAVES>(c, red);
    if (threadIdx.x == 0) cnt[2 * unit] = n, cnt[2 * unit + 1] = c;
  }
}

// Round r >= 1: the digit at `shift` of the elements whose bits above it equal the segment's prefix
__global__ __launch_bounds__(HP_THREADS) void hardpixel_hist_kernel(const HpGeo geo, int shift, const unsigned* __restrict__ fbits,
                                                                    const int* __restrict__ state, int* __restrict__ hist) {
  __shared__ int h[HP_LDS];
  const int copy = (threadIdx.x & (HP_COPIES - 1)) * HP_PITCH;
  for (int unit = blockIdx.x; unit < geo.units; unit += gridDim.x) {
    const int gseg = unit / geo.tps, tile = unit - gseg * geo.tps;
    const unsigned prefix = (unsigned)state[(size_t)gseg * HP_STATE + ST_PREFIX] >> (shift + 8);
    const bool live = state[(size_t)gseg * HP_STATE + ST_M] > 0;
    hp_clear(h);
    __syncthreads();
    const int end = live ? min(geo.L, (tile + 1) * geo.chunk) : 0;
    const unsigned* __restrict__ fb = fbits + (size_t)gseg * geo.L;      // maps, then segments: one after the other
    for (int j = tile * geo.chunk + (int)threadIdx.x; j < end; j += HP_THREADS) {
      const unsigned bits = fb[j];
      if (bits != HP_NONE && (bits >> (shift + 8)) == prefix) atomicAdd(&h[copy + ((bits >> shift) & (HP_BINS - 1))], 1);
    }
    __syncthreads();
    hp_store_row(h, hist, unit);
    __syncthreads();
  }
}

// A workgroup takes segments.  The units' rows are added per bin (group g of 256 threads the chunks g, g + 4, ...), the
// inclusive sums from the top bin down are formed, and the ONE bin d with (count above d) < rank <= (count above d) + count(d)
// fixes the digit: prefix |= d << shift, above += count above d, rank -= count above d.  Round 0 first makes the segment's
// n, c and m and counts the segments of its map that have a valid pixel; the last round writes `selection`.
__global__ __launch_bounds__(HP_PICK_THREADS) void hardpixel_pick_kernel(const HpGeo geo, int round, const int* __restrict__ hist,
                                                                         const int* __restrict__ cnt, int* __restrict__ state,
                                                                         int* __restrict__ selection) {
  __shared__ int tot[HP_PICK_GROUPS][HP_BINS];
  __shared__ int suf[2][HP_BINS];
  __shared__ int red[HP_PICK_THREADS / 64];
  const int tid = threadIdx.x, bin = tid & (HP_BINS - 1), grp = tid / HP_BINS;
  const int shift = 24 - 8 * round;
  for (int gseg = blockIdx.x; gseg < geo.GS; gseg += gridDim.x) {
    int* __restrict__ st = state + (size_t)gseg * HP_STATE;
    const int item = gseg / geo.S;
    unsigned prefix = 0;
    int rank, above = 0, m, n, c, nseg;
    if (round == 0) {
      int nn = 0, cc = 0, ne = 0;
      for (int t = tid; t < geo.tps; t += HP_PICK_THREADS) {
        nn += cnt[2 * ((size_t)gseg * geo.tps + t)];
        cc += cnt[2 * ((size_t)gseg * geo.tps + t) + 1];
      }
      for (int s = tid; s < geo.S; s += HP_PICK_THREADS) {
        int any = 0;
        for (int t = 0; t < geo.tps; ++t) any |= cnt[2 * ((size_t)(item * geo.S + s) * geo.tps + t)];
        ne += any > 0 ? 1 : 0;
      }
      n = hp_block_sum<HP_PICK_THREADS / 64>(nn, red);
      c = hp_block_sum<HP_PICK_THREADS / 64>(cc, red);
      nseg = hp_block_sum<HP_PICK_THREADS / 64>(ne, red);
      m = 0;
      if (n > 0) {
        // ceil(keep n) from the fp32 product, one rounding: keep = 0.1f of n = 1000 is 100, not 101
        int k = (int)ceilf(__fmul_rn(geo.keep, (float)n));
        k = max(k, geo.min_kept);
        k = min(max(k, 1), n);
        m = max(k, c);
      }
      rank = m;
    } else {
      prefix = (unsigned)st[ST_PREFIX];
      rank = st[ST_RANK], above = st[ST_ABOVE], m = st[ST_M], n = st[ST_N], nseg = st[ST_NSEG], c = st[ST_C];
    }
    int a = 0;
    for (int t = grp; t < geo.tps; t += HP_PICK_GROUPS) a += hist[((size_t)gseg * geo.tps + t) * HP_BINS + bin];
    tot[grp][bin] = a;
    __syncthreads();      // also: every thread has read the state that one thread rewrites below
    if (tid < HP_BINS) {
      int v = 0;
      for (int q = 0; q < HP_PICK_GROUPS; ++q) v += tot[q][bin];
      tot[0][bin] = v;
      suf[0][bin] = v;
    }
    __syncthreads();
    int cur = 0;
    for (int o = 1; o < HP_BINS; o <<= 1) {
      if (tid < HP_BINS) suf[cur ^ 1][bin] = suf[cur][bin] + (bin + o < HP_BINS ? suf[cur][bin + o] : 0);
      __syncthreads();
      cur ^= 1;
    }
    if (tid < HP_BINS) {
      const int incl = suf[cur][bin], v = tot[0][bin], excl = incl - v, total = suf[cur][0];
      const int rk = min(rank, total);
      const bool last = round == HP_DIGITS - 1;
      int* __restrict__ sel = selection + (size_t)(gseg - geo.main_item * geo.S) * 4;
      if (m > 0 && total > 0) {
        if (excl < rk && rk <= incl) {      // exactly one bin
          const unsigned p = prefix | ((unsigned)bin << shift);
          st[ST_PREFIX] = (int)p, st[ST_RANK] = rk - excl, st[ST_ABOVE] = above + excl, st[ST_M] = m, st[ST_N] = n;
          st[ST_TIE] = v, st[ST_NSEG] = nseg, st[ST_C] = c;
          if (last && item == geo.main_item) sel[0] = m, sel[1] = above + excl, sel[2] = v, sel[3] = (int)p;
        }
      } else if (tid == 0) {                // no valid pixel: the segment adds 0 and weighs nothing
        st[ST_PREFIX] = 0, st[ST_RANK] = 0, st[ST_ABOVE] = 0, st[ST_M] = 0, st[ST_N] = n, st[ST_TIE] = 0, st[ST_NSEG] = nseg, st[ST_C] = c;
        if (last && item == geo.main_item) sel[0] = 0, sel[1] = 0, sel[2] = 0, sel[3] = 0;
      }
    }
    __syncthreads();
  }
}

// the weights of a unit's segment, the map's coefficient included: f > tau weighs hi, f == tau weighs tie
struct HpWeights {
  unsigned tau;
  float hi, tie;
};

__device__ __forceinline__ HpWeights hp_weights(const int* __restrict__ st, float coef) {
  HpWeights w;
  const int m = st[ST_M], above = st[ST_ABOVE], ntie = st[ST_TIE], nseg = st[ST_NSEG];
  w.tau = (unsigned)st[ST_PREFIX];
  w.hi = w.tie = 0.f;
  if (m > 0) {
    const double share = (double)coef / ((double)m * (double)nseg);
    w.hi = (float)share;
    w.tie = (float)(share * (double)(m - above) / (double)ntie);
  }
  return w;
}

__device__ __forceinline__ void hp_store_part(double acc, double* dred, double* __restrict__ part, int unit) {
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
  if ((threadIdx.x & 63) == 0) dred[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = 0.0;
    for (int q = 0; q < HP_WAVES; ++q) v += dred[q];
    part[unit] = v;
  }
  __syncthreads();
}

// dV/dx = w df/dl (-s q) at a kept element
__global__ __launch_bounds__(HP_THREADS) void hardpixel_grad_binary_kernel(const HpItems tab, const HpGeo geo, const float* __restrict__ target,
                                                                           const unsigned* __restrict__ fbits, const int* __restrict__ state,
                                                                           const float* __restrict__ scales, double* __restrict__ part) {
  __shared__ double dred[HP_WAVES];
  const float wgt = scales[0], bscale = scales[1];
  for (int unit = blockIdx.x; unit < geo.units; unit += gridDim.x) {
    const int gseg = unit / geo.tps, tile = unit - gseg * geo.tps;
    const int item = gseg / geo.S, s = gseg - item * geo.S;
    const float* __restrict__ x = tab.it[item].logits;
    float* __restrict__ dl = tab.it[item].dlogits;
    const HpWeights w = hp_weights(state + (size_t)gseg * HP_STATE, wgt * tab.it[item].weight);
    const int end = min(geo.L, (tile + 1) * geo.chunk);
    double acc = 0.0;
    for (int j = tile * geo.chunk + (int)threadIdx.x; j < end; j += HP_THREADS) {
      const size_t a = (size_t)s * geo.L + j;
      const unsigned bits = fbits[(size_t)item * geo.P + a];
      const bool valid = bits != HP_NONE;
      if (valid && bits > w.tau) acc += (double)__uint_as_float(bits);
      if (dl == nullptr) continue;
      const float wt = !valid ? 0.f : (bits > w.tau ? w.hi : (bits == w.tau ? w.tie : 0.f));
      if (wt != 0.f) {
        const bool b = target[a] > 0.5f;
        float q, dfdl;
        const float l = hp_binary(x[a], b, &q);
        hp_focal(q, l, geo.gamma, &dfdl);
        const float g = wt * dfdl * (b ? -q : q);
        dl[a] = bscale * dl[a] + g;
      } else if (bscale != 1.f) {
        dl[a] = bscale * dl[a];
      }
    }
    hp_store_part(acc, dred, part, unit);
  }
}

// dV/dx_c = w df/dl (p_c - [c == y]) at a kept pixel; the K planes are walked three times, nothing per class is held
__global__ __launch_bounds__(HP_THREADS) void hardpixel_grad_class_kernel(const HpItems tab, const HpGeo geo, const int* __restrict__ target,
                                                                          const unsigned* __restrict__ fbits, const int* __restrict__ state,
                                                                          const float* __restrict__ scales, double* __restrict__ part) {
  __shared__ double dred[HP_WAVES];
  const float wgt = scales[0], bscale = scales[1];
  const int K = geo.C;
  for (int unit = blockIdx.x; unit < geo.units; unit += gridDim.x) {
    const int gseg = unit / geo.tps, tile = unit - gseg * geo.tps;
    const int item = gseg / geo.S, s = gseg - item * geo.S;
    const float* __restrict__ x = tab.it[item].logits;
    float* __restrict__ dl = tab.it[item].dlogits;
    const HpWeights w = hp_weights(state + (size_t)gseg * HP_STATE, wgt * tab.it[item].weight);
    const int end = min(geo.L, (tile + 1) * geo.chunk);
    double acc = 0.0;
    for (int j = tile * geo.chunk + (int)threadIdx.x; j < end; j += HP_THREADS) {
      const long long px = (long long)s * geo.L + j;
      const unsigned bits = fbits[(size_t)item * geo.P + px];
      const bool valid = bits != HP_NONE;
      if (valid && bits > w.tau) acc += (double)__uint_as_float(bits);
      if (dl == nullptr) continue;
      const int img = (int)(px / geo.HW), pix = (int)(px - (long long)img * geo.HW);
      const size_t at = (size_t)img * K * geo.HW + pix;
      float* __restrict__ dp = dl + at;
      const float wt = !valid ? 0.f : (bits > w.tau ? w.hi : (bits == w.tau ? w.tie : 0.f));
      if (wt != 0.f) {
        const float* __restrict__ xp = x + at;
        const int y = target[px];
        float mx, rest, inv, q, dfdl;
        int top;
        const float l = hp_class(xp, K, geo.HW, y, &mx, &top, &rest, &inv, &q);
        hp_focal(q, l, geo.gamma, &dfdl);
        const float g = wt * dfdl;
        for (int c = 0; c < K; ++c) {
          const float p = c == top ? inv : expf(xp[(size_t)c * geo.HW] - mx) * inv;
          dp[(size_t)c * geo.HW] = bscale * dp[(size_t)c * geo.HW] + g * (c == y ? -q : p);
        }
      } else if (bscale != 1.f) {               // exactly nothing of the term at a pixel that is not kept or in no segment
        for (int c = 0; c < K; ++c) dp[(size_t)c * geo.HW] = bscale * dp[(size_t)c * geo.HW];
      }
    }
    hp_store_part(acc, dred, part, unit);
  }
}

// One workgroup: per map, thread t takes the segments t, t + 256, ...: a segment's units in index order, then
// V_seg = (sum_{f > tau} f + (m - n_above) tau) / m; the threads' sums by a fixed tree, over the segments with n > 0
__global__ __launch_bounds__(HP_THREADS) void hardpixel_finalize_kernel(const HpItems tab, const HpGeo geo, const double* __restrict__ part,
                                                                        const int* __restrict__ state, const float* __restrict__ scales,
                                                                        const float* __restrict__ base_loss, float* __restrict__ out) {
  __shared__ double red[HP_THREADS];
  double total = 0.0, metric = 0.0;                  // thread 0's
  for (int item = 0; item < geo.n_items; ++item) {
    double a = 0.0;
    for (int s = threadIdx.x; s < geo.S; s += HP_THREADS) {
      const int gseg = item * geo.S + s;
      const int* __restrict__ st = state + (size_t)gseg * HP_STATE;
      const int m = st[ST_M];
      if (m > 0) {
        double sum = 0.0;
        for (int t = 0; t < geo.tps; ++t) sum += part[(size_t)gseg * geo.tps + t];
        a += (sum + (double)(m - st[ST_ABOVE]) * (double)__uint_as_float((unsigned)st[ST_PREFIX])) / (double)m;
      }
    }
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = HP_THREADS / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const int nseg = state[(size_t)item * geo.S * HP_STATE + ST_NSEG];
      const double V = nseg > 0 ? red[0] / (double)nseg : 0.0;
      total += (double)tab.it[item].weight * V;
      if (item == geo.main_item) metric = V;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)((double)scales[1] * (double)base_loss[0] + (double)scales[0] * total);
    out[1] = (float)metric;
  }
}

enum { HP_F, HP_HIST, HP_CNT, HP_STATE_BUF, HP_PART, HP_NBUF };

struct HpPlan {
  HpGeo geo;
  int grid;                     // the passes over (segment, chunk) units
  int pick_grid;
  long long off[HP_NBUF], bytes;
};

int hp_plan(const uz_hardpixel_desc* d, const char* who, HpPlan* p) {
  UZ_REQUIRE(d != nullptr, "%s: null descriptor", who);
  UZ_REQUIRE(d->mode == UZ_HARDPIXEL_BINARY || d->mode == UZ_HARDPIXEL_CLASS, "%s: unknown mode %d", who, d->mode);
  UZ_REQUIRE(d->n_items >= 1 && d->n_items <= UZ_CLASS_MAX_ITEMS, "%s: n_items = %d outside [1, %d]", who, d->n_items, UZ_CLASS_MAX_ITEMS);
  UZ_REQUIRE(d->N >= 1 && d->C >= 1 && d->H >= 1 && d->W >= 1, "%s: non-positive shape", who);
  const bool cls = d->mode == UZ_HARDPIXEL_CLASS;
  if (cls) UZ_REQUIRE(d->C >= 2 && d->C <= UZ_CLASS_MAX_K, "%s: K = %d outside [2, %d]", who, d->C, UZ_CLASS_MAX_K);
  UZ_REQUIRE(d->main_item >= 0 && d->main_item < d->n_items, "%s: main_item = %d outside [0, %d)", who, d->main_item, d->n_items);
  UZ_REQUIRE(d->keep > 0.f && d->keep <= 1.f, "%s: keep = %g outside (0, 1]", who, (double)d->keep);
  UZ_REQUIRE(d->min_kept >= 0, "%s: min_kept = %d is negative", who, d->min_kept);
  UZ_REQUIRE(d->max_prob == 0.f || (d->max_prob > 0.f && d->max_prob < 1.f), "%s: max_prob = %g, must be 0 (off) or in (0, 1)", who,
             (double)d->max_prob);
  UZ_REQUIRE(d->gamma == 0.f || (d->gamma >= 1.f && d->gamma < INFINITY), "%s: gamma = %g, must be 0 or a finite value >= 1", who,
             (double)d->gamma);
  UZ_REQUIRE(d->max_workgroups >= 0, "%s: max_workgroups = %d is negative", who, d->max_workgroups);
  const long long HW = (long long)d->H * d->W, pixels = HW * d->N, E = pixels * d->C;
  const long long P = cls ? pixels : E;
  const long long L = d->per_image ? P / d->N : P;
  UZ_REQUIRE(L <= HP_MAX_SEG, "%s: a segment of %lld elements, at most %lld", who, L, HP_MAX_SEG);
  UZ_REQUIRE(E * d->n_items <= HP_MAX_ELEMS, "%s: %lld elements in %d maps, at most %lld", who, E * d->n_items, d->n_items, HP_MAX_ELEMS);
  HpGeo& g = p->geo;
  g.mode = d->mode;
  g.n_items = d->n_items;
  g.N = d->N, g.C = d->C, g.HW = (int)HW;
  g.S = d->per_image ? d->N : 1;
  UZ_REQUIRE((long long)d->n_items * g.S <= HP_MAX_SEGS, "%s: %lld segments in the call, at most %d", who, (long long)d->n_items * g.S,
             HP_MAX_SEGS);
  g.GS = d->n_items * g.S;
  g.L = (int)L;
  const int tiles = uz_cdiv(L, HP_TILE);
  g.chunk = HP_TILE * uz_cdiv(tiles, HP_MAX_ROWS);
  g.tps = uz_cdiv(L, g.chunk);
  g.units = g.GS * g.tps;                 // at most 2^28 / 2048 full tiles and one ragged unit per segment (<= 2^16)
  g.ignore_index = d->ignore_index;
  g.main_item = d->main_item;
  g.min_kept = d->min_kept;
  g.keep = d->keep;
  g.thr = d->max_prob > 0.f ? (float)(-log((double)d->max_prob)) : INFINITY;
  g.gamma = d->gamma;
  g.P = P;
  g.E = E;
  // eight workgroups of four waves per CU of the hardware: what can be resident at once; more units than that are walked
  int grid = uz_grid_cap(g.units, 8);
  int pick_grid = uz_grid_cap(g.GS, 2);
  if (d->max_workgroups > 0 && grid > d->max_workgroups) grid = d->max_workgroups;
  if (d->max_workgroups > 0 && pick_grid > d->max_workgroups) pick_grid = d->max_workgroups;
  p->grid = grid;
  p->pick_grid = pick_grid;
  const long long sizes[HP_NBUF] = {4 * P * d->n_items, 4LL * g.units * HP_BINS, 8LL * g.units, 4LL * HP_STATE * g.GS, 8LL * g.units};
  p->bytes = uz_carve(sizes, HP_NBUF, p->off);
  return UZ_OK;
}

}  // namespace

extern "C" long long uz_hardpixel_workspace_bytes(const uz_hardpixel_desc* d) {
  HpPlan p;
  if (hp_plan(d, "uz_hardpixel_workspace_bytes", &p) != UZ_OK) return -1;
  return p.bytes;
}

extern "C" int uz_hardpixel_grid(const uz_hardpixel_desc* d, int* units) {
  HpPlan p;
  const int rc = hp_plan(d, "uz_hardpixel_grid", &p);
  if (rc != UZ_OK) return rc;
  if (units) *units = p.geo.units;
  return p.grid;
}

extern "C" int uz_hardpixel_loss(const uz_hardpixel_desc* d, const uz_hardpixel_item* items, const void* target, const float* scales,
                                 const float* base_loss, float* out, float* losses, int* selection, void* workspace, void* stream) {
  HpPlan p;
  const int rc = hp_plan(d, "uz_hardpixel_loss", &p);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(items && target && scales && base_loss && out && losses && selection && workspace, "uz_hardpixel_loss: null pointer");
  UZ_REQUIRE((((uintptr_t)target | (uintptr_t)scales | (uintptr_t)base_loss | (uintptr_t)out | (uintptr_t)losses | (uintptr_t)selection) & 3) == 0,
             "uz_hardpixel_loss: tensors must be 4-byte aligned");
  UZ_REQUIRE(((uintptr_t)workspace & 15) == 0, "uz_hardpixel_loss: the workspace must be 16-byte aligned");
  const HpGeo& g = p.geo;
  const bool cls = d->mode == UZ_HARDPIXEL_CLASS;
  const long long map_bytes = 4LL * g.E;
  // what the call writes (out, losses, selection, workspace, every dlogits) against everything else it touches
  UzRange in[3 + UZ_CLASS_MAX_ITEMS] = {uz_range(target, 4LL * g.P), uz_range(scales, 8), uz_range(base_loss, 4)};
  UzRange outr[4 + UZ_CLASS_MAX_ITEMS] = {uz_range(out, 8), uz_range(losses, 4LL * g.P), uz_range(selection, 16LL * g.S),
                                          uz_range(workspace, p.bytes)};
  int n_in = 3, n_out = 4;
  HpItems tab;
  bool any_grad;
  const int irc = uz_map_items("uz_hardpixel_loss", items, d->n_items, map_bytes, in, &n_in, outr, &n_out, &any_grad, tab.it);
  if (irc != UZ_OK) return irc;
  UZ_REQUIRE(!uz_any_overlap(outr, n_out, in, n_in), "uz_hardpixel_loss: tensors overlap");
  char* base = static_cast<char*>(workspace);
  unsigned* fbits = reinterpret_cast<unsigned*>(base + p.off[HP_F]);
  int* hist = reinterpret_cast<int*>(base + p.off[HP_HIST]);
  int* cnt = reinterpret_cast<int*>(base + p.off[HP_CNT]);
  int* state = reinterpret_cast<int*>(base + p.off[HP_STATE_BUF]);
  double* part = reinterpret_cast<double*>(base + p.off[HP_PART]);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(HP_THREADS), grid((unsigned)p.grid), pblock(HP_PICK_THREADS), pgrid((unsigned)p.pick_grid);

  if (cls) hipLaunchKernelGGL(hardpixel_loss_class_kernel, grid, block, 0, s, tab, g, static_cast<const int*>(target), fbits, losses, hist, cnt);
  else hipLaunchKernelGGL(hardpixel_loss_binary_kernel, grid, block, 0, s, tab, g, static_cast<const float*>(target), fbits, losses, hist, cnt);
  UZ_LAUNCH_CHECK("uz_hardpixel_loss(loss)");
  for (int round = 0; round < HP_DIGITS; ++round) {
    if (round > 0) {
      hipLaunchKernelGGL(hardpixel_hist_kernel, grid, block, 0, s, g, 24 - 8 * round, (const unsigned*)fbits, (const int*)state, hist);
      UZ_LAUNCH_CHECK("uz_hardpixel_loss(hist)");
    }
    hipLaunchKernelGGL(hardpixel_pick_kernel, pgrid, pblock, 0, s, g, round, (const int*)hist, (const int*)cnt, state, selection);
    UZ_LAUNCH_CHECK("uz_hardpixel_loss(pick)");
  }
  if (cls) hipLaunchKernelGGL(hardpixel_grad_class_kernel, grid, block, 0, s, tab, g, static_cast<const int*>(target), (const unsigned*)fbits, (const int*)state, scales, part);
  else hipLaunchKernelGGL(hardpixel_grad_binary_kernel, grid, block, 0, s, tab, g, static_cast<const float*>(target), (const unsigned*)fbits, (const int*)state, scales, part);
  UZ_LAUNCH_CHECK("uz_hardpixel_loss(grad)");
  hipLaunchKernelGGL(hardpixel_finalize_kernel, dim3(1), block, 0, s, tab, g, (const double*)part, (const int*)state, scales, base_loss, out);
  UZ_LAUNCH_CHECK("uz_hardpixel_loss(finalize)");
  return UZ_OK;
}
