// Lovasz hinge / Lovasz-softmax (Berman, Triggs, Blaschko: "The Lovasz-Softmax loss", CVPR 2018) on the device, added to a base
// loss whose value and gradients already exist (include/unetzoo_hip.h).  The library's segmented stable sort.
//   geometry  `lines` pixel lines of L pixels: every image (per_image, L = H W) or the whole batch as one line (L = N H W);
//             a segment is (line, channel / class): S = lines C per map, GS = n_items S in the call; a tile is LV_TILE
//             consecutive elements of a segment, a unit one (segment, tile)
//   key       ~bits(e) for a ranked element (e > 0: the bit pattern of a positive float orders as an unsigned integer, its
//             complement descending), 0xFFFFFFFF for an unranked one: ascending keys = descending errors, unranked last
//   value     position in the segment | membership bit << 31
// Launches, every one with a fixed grid for a descriptor (19 with a gradient buffer, 18 without):
//   keys      e, key and value of every element of every map, `errors` of the main map, the members per (segment, tile)
//   segments  per (map, line): G of every segment from the tiles' counts, the present classes, the segment's share of V
//   4 x (hist, rowscan, scatter)   least-significant-digit radix sort, 8 bits a pass, between two buffers:
//       hist     per unit the 256 digit counts (LDS integer atomics: counts do not depend on arrival order)
//       rowscan  per (segment, digit) row the exclusive scan over the tiles, in place, and the row's total; a wave a row
//       scatter  per unit: offset of (digit, tile) = digits below in the segment + same digit in earlier tiles; inside the
//                tile rounds, waves and lanes are taken in index order (ballot match + a running LDS offset handed from wave
//                to wave between barriers), so equal digits keep their order: the sort is stable and has ONE result
//   bits      per unit of the SORTED segment the members
//   scan      per unit: members before the tile (earlier tiles' counts) + ballot prefix -> c, n, the Jaccard difference g from
//             the integers in float64; sum of e g by a fixed tree; g by POSITION (what the gradient reads) and `ranks`
//   grad      dl <- base_scale dl + weight ow dV/dx  (only when a map has a gradient buffer)
//   finalize  the units' sums in index order, out[0] = base_scale base_loss + weight sum_m ow_m V_m, out[1] = V_main
// No workgroup waits for another inside a launch, no float atomics, nothing to clear: every counter is a plain store.
#include "uz_common.h"

#include <math.h>

namespace {

constexpr int LV_THREADS = 256;
constexpr int LV_WAVES = LV_THREADS / 64;
constexpr int LV_ROUNDS = 4;
constexpr int LV_TILE = LV_THREADS * LV_ROUNDS;
constexpr int LV_BINS = 256;          // 8 bits a pass
constexpr int LV_PASSES = 4;          // even: the sorted segment is back in the first buffer
constexpr unsigned LV_UNRANKED = 0xFFFFFFFFu;
constexpr unsigned LV_MEMBER = 0x80000000u;
constexpr long long LV_MAX_SEG = 1LL << 22;       // elements of one segment
constexpr long long LV_MAX_ELEMS = 1LL << 28;     // elements of all maps of a call

struct LvItems {
  uz_lovasz_item it[UZ_CLASS_MAX_ITEMS];
};

struct LvGeo {
  int mode;
  int n_items;
  int N, C, HW;
  int lines;         // N (per_image) or 1
  int S;             // segments per map: lines * C
  int GS;            // segments of the call: n_items * S
  int L;             // elements of a segment: H W or N H W
  int tps;           // tiles per segment
  int units;         // GS * tps
  int punits;        // class mode, keys pass: n_items * lines * tps (a unit: one pixel tile, all classes)
  int all_classes;
  int ignore_index;
  int main_item;
  long long E;       // elements of a map: N C H W
  long long pixels;  // N H W
};

// the sum of a workgroup's integers, to every thread
__device__ __forceinline__ int lv_block_sum(int v, int* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
  for (int q = 0; q < LV_WAVES; ++q) t += red[q];
  __syncthreads();
  return t;
}

__device__ __forceinline__ unsigned lv_key(float e) { return e > 0.f ? ~__float_as_uint(e) : LV_UNRANKED; }      // a NaN is unranked

// Binary mode: e = 1 - x s with s = +1 in the target, -1 outside: x s is exact, e is one rounding
__global__ __launch_bounds__(LV_THREADS) void lovasz_keys_binary_kernel(const LvItems tab, const LvGeo geo, const float* __restrict__ target,
                                                                        unsigned* __restrict__ key, unsigned* __restrict__ val,
                                                                        int* __restrict__ tileG, float* __restrict__ errors) {
  __shared__ int red[LV_WAVES];
  for (int unit = blockIdx.x; unit < geo.units; unit += gridDim.x) {
    const int gseg = unit / geo.tps, tile = unit - gseg * geo.tps;
    const int item = gseg / geo.S, s = gseg - item * geo.S;
    const int line = s / geo.C, c = s - line * geo.C;
    const float* __restrict__ x = tab.it[item].logits;
    int mine = 0;
    for (int r = 0; r < LV_ROUNDS; ++r) {
      const int j = tile * LV_TILE + r * LV_THREADS + (int)threadIdx.x;
      if (j < geo.L) {
        const long long q = (long long)line * geo.L + j;
        const int n = (int)(q / geo.HW), pix = (int)(q - (long long)n * geo.HW);
        const size_t a = ((size_t)n * geo.C + c) * geo.HW + pix;
        const float xv = x[a];
        const bool b = target[a] > 0.5f;
        const float e = b ? 1.f - xv : 1.f + xv;
        const size_t at = (size_t)gseg * geo.L + j;
        key[at] = lv_key(e);
        val[at] = (unsigned)j | (b ? LV_MEMBER : 0u);
        if (item == geo.main_item) errors[(size_t)s * geo.L + j] = e;
        mine += b ? 1 : 0;
      }
    }
    const int total = lv_block_sum(mine, red);
    if (threadIdx.x == 0) tileG[unit] = total;
  }
}

// Class mode: p = softmax_K(x), e_c = |[y == c] - p_c|; a pixel whose label is ignore_index or outside [0, K) has e = 0 in
// every class and is no member: unranked, it sorts behind every ranked element and changes no count.  A unit is a tile of
// pixels of a line; the K planes are walked three times, nothing per class is held.
__global__ __launch_bounds__(LV_THREADS) void lovasz_keys_class_kernel(const LvItems tab, const LvGeo geo, const int* __restrict__ target,
                                                                       unsigned* __restrict__ key, unsigned* __restrict__ val,
                                                                       int* __restrict__ tileG, float* __restrict__ errors) {
  __shared__ int cnt[UZ_CLASS_MAX_K];
  const int K = geo.C;
  for (int unit = blockIdx.x; unit < geo.punits; unit += gridDim.x) {
    const int item = unit / (geo.lines * geo.tps), rem = unit - item * (geo.lines * geo.tps);
    const int line = rem / geo.tps, tile = rem - line * geo.tps;
    const float* __restrict__ x = tab.it[item].logits;
    const int seg0 = item * geo.S + line * K;
    if ((int)threadIdx.x < K) cnt[threadIdx.x] = 0;
    __syncthreads();
    for (int r = 0; r < LV_ROUNDS; ++r) {
      const int j = tile * LV_TILE + r * LV_THREADS + (int)threadIdx.x;
      if (j < geo.L) {
        const long long q = (long long)line * geo.L + j;
        const int n = (int)(q / geo.HW), pix = (int)(q - (long long)n * geo.HW);
        const int y = target[q];
        const bool valid = y >= 0 && y < K && y != geo.ignore_index;
        const float* __restrict__ xp = x + (size_t)n * K * geo.HW + pix;
        float m = xp[0];
        for (int c = 1; c < K; ++c) m = fmaxf(m, xp[(size_t)c * geo.HW]);
        float sum = 0.f;
        for (int c = 0; c < K; ++c) sum += expf(xp[(size_t)c * geo.HW] - m);
        const float inv = 1.f / sum;
        for (int c = 0; c < K; ++c) {
          const float p = expf(xp[(size_t)c * geo.HW] - m) * inv;
          const bool b = valid && y == c;
          const float e = valid ? (b ? 1.f - p : p) : 0.f;
          const size_t at = (size_t)(seg0 + c) * geo.L + j;
          key[at] = lv_key(e);
          val[at] = (unsigned)j | (b ? LV_MEMBER : 0u);
          if (item == geo.main_item) errors[(size_t)(line * K + c) * geo.L + j] = e;
        }
        if (valid) atomicAdd(&cnt[y], 1);      // an integer count in LDS: the same whatever the order
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < K) tileG[(size_t)(seg0 + (int)threadIdx.x) * geo.tps + tile] = cnt[threadIdx.x];
    __syncthreads();
  }
}

// A workgroup takes (map, line) pairs: G of its C segments from the tiles' counts, then every segment's share of V:
// 1 / (lines |P|) for a segment of P, 0 otherwise; P = the classes with G > 0 ("present") or all C
__global__ __launch_bounds__(LV_THREADS) void lovasz_segments_kernel(const LvGeo geo, const int* __restrict__ tileG, int* __restrict__ segG,
                                                                     double* __restrict__ wseg) {
  __shared__ int red[LV_WAVES];
  for (int unit = blockIdx.x; unit < geo.n_items * geo.lines; unit += gridDim.x) {
    const int seg0 = unit * geo.C;             // (item * lines + line) * C
    int present = 0;
    for (int c = 0; c < geo.C; ++c) {
      int g = 0;
      for (int t = threadIdx.x; t < geo.tps; t += LV_THREADS) g += tileG[(size_t)(seg0 + c) * geo.tps + t];
      g = lv_block_sum(g, red);
      if (threadIdx.x == 0) segG[seg0 + c] = g;
      present += g > 0 ? 1 : 0;
    }
    const int P = geo.all_classes ? geo.C : present;
    __syncthreads();                           // thread 0's stores to segG, read back by the workgroup
    for (int c = threadIdx.x; c < geo.C; c += LV_THREADS) {
      const bool in = geo.all_classes || segG[seg0 + c] > 0;
      wseg[seg0 + c] = in ? 1.0 / ((double)geo.lines * (double)P) : 0.0;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(LV_THREADS) void lovasz_hist_kernel(const LvGeo geo, int shift, const unsigned* __restrict__ key, int* __restrict__ hist) {
  __shared__ int h[LV_BINS];
  for (int unit = blockIdx.x; unit < geo.units; unit += gridDim.x) {
    const int gseg = unit / geo.tps, tile = unit - gseg * geo.tps;
    h[threadIdx.x] = 0;
    __syncthreads();
    for (int r = 0; r < LV_ROUNDS; ++r) {
      const int j = tile * LV_TILE + r * LV_THREADS + (int)threadIdx.x;
      if (j < geo.L) atomicAdd(&h[(key[(size_t)gseg * geo.L + j] >> shift) & (LV_BINS - 1)], 1);
    }
    __syncthreads();
    hist[((size_t)gseg * LV_BINS + threadIdx.x) * geo.tps + tile] = h[threadIdx.x];
    __syncthreads();
  }
}

// A WAVE takes (segment, digit) rows: the exclusive scan over the row's tiles in place, the row's total to digit_tot
__global__ __launch_bounds__(LV_THREADS) void lovasz_rowscan_kernel(const LvGeo geo, int* __restrict__ hist, int* __restrict__ digit_tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows = geo.GS * LV_BINS;
  for (int row = blockIdx.x * LV_WAVES + wave; row < rows; row += gridDim.x * LV_WAVES) {
    int* __restrict__ h = hist + (size_t)row * geo.tps;
    int carry = 0;
    for (int t0 = 0; t0 < geo.tps; t0 += 64) {     // uniform over the wave
      const int t = t0 + lane;
      const int v = t < geo.tps ? h[t] : 0;
      int incl = v;
      for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o);
        if (lane >= o) incl += u;
      }
      if (t < geo.tps) h[t] = carry + incl - v;
      carry += __shfl(incl, 63);
    }
    if (lane == 0) digit_tot[row] = carry;
  }
}

__global__ __launch_bounds__(LV_THREADS) void lovasz_scatter_kernel(const LvGeo geo, int shift, const unsigned* __restrict__ key,
                                                                    const unsigned* __restrict__ val, unsigned* __restrict__ key_out,
                                                                    unsigned* __restrict__ val_out, const int* __restrict__ hist,
                                                                    const int* __restrict__ digit_tot) {
  __shared__ int off[LV_BINS];       // where the next element of a digit goes: advanced wave after wave, round after round
  __shared__ int wsum[LV_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below_me = (1ull << lane) - 1ull;
  for (int unit = blockIdx.x; unit < geo.units; unit += gridDim.x) {
    const int gseg = unit / geo.tps, tile = unit - gseg * geo.tps;
    {                                // thread = digit: the elements of the segment with a smaller digit + this digit's in earlier tiles
      const int v = digit_tot[gseg * LV_BINS + threadIdx.x];
      int incl = v;
      for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o);
        if (lane >= o) incl += u;
      }
      if (lane == 63) wsum[wave] = incl;
      __syncthreads();
      int base = 0;
      for (int q = 0; q < wave; ++q) base += wsum[q];
      off[threadIdx.x] = base + incl - v + hist[((size_t)gseg * LV_BINS + threadIdx.x) * geo.tps + tile];
      __syncthreads();
    }
    for (int r = 0; r < LV_ROUNDS; ++r) {
      const int j = tile * LV_TILE + r * LV_THREADS + (int)threadIdx.x;
      const bool live = j < geo.L;
      const size_t at = (size_t)gseg * geo.L + (live ? j : 0);
      const unsigned k = key[at], pv = val[at];
      const int d = (int)((k >> shift) & (LV_BINS - 1));
      unsigned long long same = __ballot(live);      // the live lanes of this wave with my digit (wave64: 64 bits)
#pragma unroll
      for (int bit = 0; bit < 8; ++bit) {
        const bool mine = (d >> bit) & 1;
        const unsigned long long bb = __ballot(mine);
        same &= mine ? bb : ~bb;
      }
      const int below = __popcll(same & below_me), count = __popcll(same);
      const int leader = same ? __ffsll(same) - 1 : 0;
      int old = 0;
      for (int w = 0; w < LV_WAVES; ++w) {           // wave after wave: the order inside a digit is the index order
        if (wave == w && live && below == 0) {
          old = off[d];
          off[d] = old + count;
        }
        __syncthreads();
      }
      old = __shfl(old, leader);
      const int dest = old + below;
      if (live && (unsigned)dest < (unsigned)geo.L) {      // always inside for counts that match the keys; never a wild store
        key_out[(size_t)gseg * geo.L + dest] = k;
        val_out[(size_t)gseg * geo.L + dest] = pv;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(LV_THREADS) void lovasz_bits_kernel(const LvGeo geo, const unsigned* __restrict__ val, int* __restrict__ tileB) {
  __shared__ int red[LV_WAVES];
  for (int unit = blockIdx.x; unit < geo.units; unit += gridDim.x) {
    const int gseg = unit / geo.tps, tile = unit - gseg * geo.tps;
    int mine = 0;
    for (int r = 0; r < LV_ROUNDS; ++r) {
      const int j = tile * LV_TILE + r * LV_THREADS + (int)threadIdx.x;
      if (j < geo.L) mine += (int)(val[(size_t)gseg * geo.L + j] >> 31);
    }
    const int total = lv_block_sum(mine, red);
    if (threadIdx.x == 0) tileB[unit] = total;
  }
}

// Element `rank` of the sorted segment: c = members among ranks 0 .. rank, n = rank + 1 - c, and with G members in the segment
//   g = 1 / (G + n) for a member, (G - c) / ((G + n - 1) (G + n)) otherwise, 1 at rank 0 of a segment without a member
// -- J_rank - J_(rank-1) with J = 1 - (G - c) / (G + n), from the integers.  The unranked tail gets g = 0 and rank -1.
__global__ __launch_bounds__(LV_THREADS) void lovasz_scan_kernel(const LvGeo geo, const unsigned* __restrict__ key, const unsigned* __restrict__ val,
                                                                 const int* __restrict__ tileB, const int* __restrict__ segG,
                                                                 float* __restrict__ gw, int* __restrict__ ranks, double* __restrict__ part) {
  __shared__ int red[LV_WAVES];
  __shared__ int wcnt[LV_ROUNDS][LV_WAVES];
  __shared__ double dred[LV_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long upto_me = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
  for (int unit = blockIdx.x; unit < geo.units; unit += gridDim.x) {
    const int gseg = unit / geo.tps, tile = unit - gseg * geo.tps;
    const int item = gseg / geo.S, s = gseg - item * geo.S;
    int before = 0;                  // members in the earlier tiles of the sorted segment
    for (int t = threadIdx.x; t < tile; t += LV_THREADS) before += tileB[(size_t)gseg * geo.tps + t];
    before = lv_block_sum(before, red);
    const int G = segG[gseg];
    unsigned k[LV_ROUNDS], pv[LV_ROUNDS];
    unsigned long long members[LV_ROUNDS];
#pragma unroll
    for (int r = 0; r < LV_ROUNDS; ++r) {
      const int j = tile * LV_TILE + r * LV_THREADS + (int)threadIdx.x;
      const bool live = j < geo.L;
      const size_t at = (size_t)gseg * geo.L + (live ? j : 0);
      k[r] = key[at];
      pv[r] = val[at];
      members[r] = __ballot(live && (pv[r] >> 31));
      if (lane == 0) wcnt[r][wave] = __popcll(members[r]);
    }
    __syncthreads();
    double acc = 0.0;
    int c0 = before;                 // members before round r of this tile
#pragma unroll
    for (int r = 0; r < LV_ROUNDS; ++r) {
      int c = c0;
      for (int q = 0; q < LV_WAVES; ++q) {
        c += q < wave ? wcnt[r][q] : 0;
        c0 += wcnt[r][q];
      }
      c += __popcll(members[r] & upto_me);
      const int rank = tile * LV_TILE + r * LV_THREADS + (int)threadIdx.x;
      if (rank < geo.L) {
        const bool ranked = k[r] != LV_UNRANKED;
        const int pos = (int)(pv[r] & ~LV_MEMBER);
        float gf = 0.f;
        if (ranked) {
          const int n = rank + 1 - c;
          double g;
          if (G == 0) g = rank == 0 ? 1.0 : 0.0;
          else if (pv[r] >> 31) g = 1.0 / (double)(G + n);
          else g = (double)(G - c) / ((double)(G + n - 1) * (double)(G + n));
          acc += (double)__uint_as_float(~k[r]) * g;
          gf = (float)g;
        }
        if ((unsigned)pos < (unsigned)geo.L) {
          gw[(size_t)gseg * geo.L + pos] = gf;
          if (item == geo.main_item) ranks[(size_t)s * geo.L + pos] = ranked ? rank : -1;
        }
      }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
    if (lane == 0) dred[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      double v = 0.0;
      for (int q = 0; q < LV_WAVES; ++q) v += dred[q];
      part[unit] = v;
    }
    __syncthreads();
  }
}

// dV/dx = -s g share at a ranked element (g = 0 elsewhere); map after map, the grid is fixed for a descriptor
__global__ __launch_bounds__(LV_THREADS) void lovasz_grad_binary_kernel(const LvItems tab, const LvGeo geo, const float* __restrict__ target,
                                                                        const float* __restrict__ gw, const double* __restrict__ wseg,
                                                                        const float* __restrict__ scales) {
  const float wgt = scales[0], bscale = scales[1];
  const long long stride = (long long)gridDim.x * LV_THREADS;
  for (int item = 0; item < geo.n_items; ++item) {
    float* __restrict__ dl = tab.it[item].dlogits;
    if (dl == nullptr) continue;
    const float coef = wgt * tab.it[item].weight;
    for (long long a = (long long)blockIdx.x * LV_THREADS + threadIdx.x; a < geo.E; a += stride) {
      const int plane = (int)(a / geo.HW), pix = (int)(a - (long long)plane * geo.HW);
      const int n = plane / geo.C, c = plane - n * geo.C;
      const int line = geo.lines == 1 ? 0 : n;
      const long long j = geo.lines == 1 ? (long long)n * geo.HW + pix : pix;
      const int gseg = item * geo.S + line * geo.C + c;
      const float gs = gw[(size_t)gseg * geo.L + j] * (float)wseg[gseg];
      const float d = target[a] > 0.5f ? -gs : gs;
      dl[a] = bscale * dl[a] + coef * d;
    }
  }
}

// dV/dx_k = p_k (d_k - sum_c p_c d_c) with d_c = sign(p_c - [y == c]) g_c share_c; the K planes are walked, nothing per class
// is held
__global__ __launch_bounds__(LV_THREADS) void lovasz_grad_class_kernel(const LvItems tab, const LvGeo geo, const int* __restrict__ target,
                                                                       const float* __restrict__ gw, const double* __restrict__ wseg,
                                                                       const float* __restrict__ scales) {
  const float wgt = scales[0], bscale = scales[1];
  const int K = geo.C;
  const long long stride = (long long)gridDim.x * LV_THREADS;
  for (int item = 0; item < geo.n_items; ++item) {
    const float* __restrict__ x = tab.it[item].logits;
    float* __restrict__ dl = tab.it[item].dlogits;
    if (dl == nullptr) continue;
    const float coef = wgt * tab.it[item].weight;
    for (long long q = (long long)blockIdx.x * LV_THREADS + threadIdx.x; q < geo.pixels; q += stride) {
      const int n = (int)(q / geo.HW), pix = (int)(q - (long long)n * geo.HW);
      const int y = target[q];
      const bool valid = y >= 0 && y < K && y != geo.ignore_index;
      const int line = geo.lines == 1 ? 0 : n;
      const long long j = geo.lines == 1 ? q : pix;
      const int seg0 = item * geo.S + line * K;
      const size_t at = (size_t)n * K * geo.HW + pix;
      const float* __restrict__ xp = x + at;
      float* __restrict__ dp = dl + at;
      // d_k - sum_c p_c d_c cancels where p_k is near 1, which only the largest logit's class `top` can be: there it is taken
      // as d_top (1 - p_top) - sum_{c != top} p_c d_c with 1 - p_top = (sum_{c != top} exp) / sum, no difference of near-equals
      float m = xp[0];
      int top = 0;
      for (int c = 1; c < K; ++c) {
        const float v = xp[(size_t)c * geo.HW];
        top = v > m ? c : top;
        m = v > m ? v : m;
      }
      float rest = 0.f;
      for (int c = 0; c < K; ++c) rest += c == top ? 0.f : expf(xp[(size_t)c * geo.HW] - m);
      const float inv = 1.f / (1.f + rest);      // p_top: exp(0) = 1
      float dot_rest = 0.f, d_top = 0.f;
      for (int c = 0; c < K; ++c) {
        const float gs = gw[(size_t)(seg0 + c) * geo.L + j] * (float)wseg[seg0 + c];
        const float dc = y == c ? -gs : gs;
        if (c == top) d_top = dc;
        else dot_rest = fmaf(expf(xp[(size_t)c * geo.HW] - m) * inv, dc, dot_rest);
      }
      for (int c = 0; c < K; ++c) {
        const float p = c == top ? inv : expf(xp[(size_t)c * geo.HW] - m) * inv;
        const float gs = gw[(size_t)(seg0 + c) * geo.L + j] * (float)wseg[seg0 + c];
        const float t = c == top ? d_top * (rest * inv) - dot_rest : (y == c ? -gs : gs) - fmaf(inv, d_top, dot_rest);
        const float gk = valid ? coef * (p * t) : 0.f;      // exactly nothing at an ignored pixel
        dp[(size_t)c * geo.HW] = bscale * dp[(size_t)c * geo.HW] + gk;
      }
    }
  }
}

// One workgroup: per map the units' sums times their segment's share, in index order (thread t adds units t, t + 256, ...,
// then a fixed tree)
__global__ __launch_bounds__(LV_THREADS) void lovasz_finalize_kernel(const LvItems tab, const LvGeo geo, const double* __restrict__ part,
                                                                     const double* __restrict__ wseg, const float* __restrict__ scales,
                                                                     const float* __restrict__ base_loss, float* __restrict__ out) {
  __shared__ double red[LV_THREADS];
  const int per_item = geo.S * geo.tps;
  double total = 0.0, metric = 0.0;                  // thread 0's
  for (int item = 0; item < geo.n_items; ++item) {
    double a = 0.0;
    for (int r = threadIdx.x; r < per_item; r += LV_THREADS)
      a += wseg[item * geo.S + r / geo.tps] * part[(size_t)item * per_item + r];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = LV_THREADS / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      total += (double)tab.it[item].weight * red[0];
      if (item == geo.main_item) metric = red[0];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)((double)scales[1] * (double)base_loss[0] + (double)scales[0] * total);
    out[1] = (float)metric;
  }
}

enum { LV_KEY_A, LV_VAL_A, LV_KEY_B, LV_VAL_B, LV_HIST, LV_DTOT, LV_TILE_G, LV_TILE_B, LV_SEG_G, LV_WSEG, LV_PART, LV_NBUF };

struct LvPlan {
  LvGeo geo;
  int grid;                     // the passes over (segment, tile) units
  int keys_grid, seg_grid, row_grid, grad_grid;
  long long off[LV_NBUF], bytes;
};

int lv_plan(const uz_lovasz_desc* d, const char* who, LvPlan* p) {
  UZ_REQUIRE(d != nullptr, "%s: null descriptor", who);
  UZ_REQUIRE(d->mode == UZ_LOVASZ_BINARY || d->mode == UZ_LOVASZ_CLASS, "%s: unknown mode %d", who, d->mode);
  UZ_REQUIRE(d->n_items >= 1 && d->n_items <= UZ_CLASS_MAX_ITEMS, "%s: n_items = %d outside [1, %d]", who, d->n_items, UZ_CLASS_MAX_ITEMS);
  UZ_REQUIRE(d->N >= 1 && d->C >= 1 && d->H >= 1 && d->W >= 1, "%s: non-positive shape", who);
  UZ_REQUIRE(d->classes == UZ_LOVASZ_PRESENT || d->classes == UZ_LOVASZ_ALL, "%s: unknown classes mode %d", who, d->classes);
  const bool cls = d->mode == UZ_LOVASZ_CLASS;
  if (cls) UZ_REQUIRE(d->C >= 2 && d->C <= UZ_CLASS_MAX_K, "%s: K = %d outside [2, %d]", who, d->C, UZ_CLASS_MAX_K);
  UZ_REQUIRE(d->main_item >= 0 && d->main_item < d->n_items, "%s: main_item = %d outside [0, %d)", who, d->main_item, d->n_items);
  const long long HW = (long long)d->H * d->W, pixels = HW * d->N, E = pixels * d->C;
  const long long L = d->per_image ? HW : pixels;
  UZ_REQUIRE(L <= LV_MAX_SEG, "%s: a segment of %lld elements, at most %lld", who, L, LV_MAX_SEG);
  UZ_REQUIRE(E * d->n_items <= LV_MAX_ELEMS, "%s: %lld elements in %d maps, at most %lld", who, E * d->n_items, d->n_items, LV_MAX_ELEMS);
  LvGeo& g = p->geo;
  g.mode = d->mode;
  g.n_items = d->n_items;
  g.N = d->N, g.C = d->C, g.HW = (int)HW;
  g.lines = d->per_image ? d->N : 1;
  const long long GS = (long long)d->n_items * g.lines * d->C;
  UZ_REQUIRE(GS * LV_BINS < (1LL << 31), "%s: too many segments (%lld)", who, GS);
  g.S = g.lines * d->C;
  g.GS = (int)GS;
  g.L = (int)L;
  g.tps = uz_cdiv(L, LV_TILE);
  UZ_REQUIRE(GS * g.tps < (1LL << 30), "%s: too many (segment, tile) units", who);
  g.units = g.GS * g.tps;
  g.punits = d->n_items * g.lines * g.tps;
  g.all_classes = (!cls || d->classes == UZ_LOVASZ_ALL) ? 1 : 0;      // the binary mode has no absent channel
  g.ignore_index = d->ignore_index;
  g.main_item = d->main_item;
  g.E = E;
  g.pixels = pixels;
  // eight workgroups of four waves per CU of the hardware: what can be resident at once; more units than that are walked
  p->grid = uz_grid_cap(g.units, 8);
  p->keys_grid = uz_grid_cap(cls ? g.punits : g.units, 8);
  p->seg_grid = uz_grid_cap(d->n_items * g.lines, 8);
  p->row_grid = uz_grid_cap(uz_cdiv((long long)g.GS * LV_BINS, LV_WAVES), 8);
  p->grad_grid = uz_grid_cap(((cls ? pixels : E) + LV_THREADS - 1) / LV_THREADS, 8);
  const long long TE = E * d->n_items;
  const long long sizes[LV_NBUF] = {4 * TE, 4 * TE, 4 * TE, 4 * TE, 4LL * g.GS * LV_BINS * g.tps, 4LL * g.GS * LV_BINS,
                                    4LL * g.units, 4LL * g.units, 4LL * g.GS, 8LL * g.GS, 8LL * g.units};
  p->bytes = uz_carve(sizes, LV_NBUF, p->off);
  return UZ_OK;
}

}  // namespace

extern "C" long long uz_lovasz_workspace_bytes(const uz_lovasz_desc* d) {
  LvPlan p;
  if (lv_plan(d, "uz_lovasz_workspace_bytes", &p) != UZ_OK) return -1;
  return p.bytes;
}

extern "C" int uz_lovasz_grid(const uz_lovasz_desc* d, int* units) {
  LvPlan p;
  const int rc = lv_plan(d, "uz_lovasz_grid", &p);
  if (rc != UZ_OK) return rc;
  if (units) *units = p.geo.units;
  return p.grid;
}

extern "C" int uz_lovasz_loss(const uz_lovasz_desc* d, const uz_lovasz_item* items, const void* target, const float* scales,
                              const float* base_loss, float* out, float* errors, int* ranks, void* workspace, void* stream) {
  LvPlan p;
  const int rc = lv_plan(d, "uz_lovasz_loss", &p);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(items && target && scales && base_loss && out && errors && ranks && workspace, "uz_lovasz_loss: null pointer");
  UZ_REQUIRE((((uintptr_t)target | (uintptr_t)scales | (uintptr_t)base_loss | (uintptr_t)out | (uintptr_t)errors | (uintptr_t)ranks) & 3) == 0,
             "uz_lovasz_loss: tensors must be 4-byte aligned");
  UZ_REQUIRE(((uintptr_t)workspace & 15) == 0, "uz_lovasz_loss: the workspace must be 16-byte aligned");
  const LvGeo& g = p.geo;
  const bool cls = d->mode == UZ_LOVASZ_CLASS;
  const long long map_bytes = 4LL * g.E;
  // what the call writes (out, errors, ranks, workspace, every dlogits) against everything else it touches
  UzRange in[3 + UZ_CLASS_MAX_ITEMS] = {uz_range(target, cls ? 4LL * g.pixels : map_bytes), uz_range(scales, 8), uz_range(base_loss, 4)};
  UzRange outr[4 + UZ_CLASS_MAX_ITEMS] = {uz_range(out, 8), uz_range(errors, map_bytes), uz_range(ranks, map_bytes),
                                          uz_range(workspace, p.bytes)};
  int n_in = 3, n_out = 4;
  LvItems tab;
  bool any_grad;
  const int irc = uz_map_items("uz_lovasz_loss", items, d->n_items, map_bytes, in, &n_in, outr, &n_out, &any_grad, tab.it);
  if (irc != UZ_OK) return irc;
  UZ_REQUIRE(!uz_any_overlap(outr, n_out, in, n_in), "uz_lovasz_loss: tensors overlap");
  char* base = static_cast<char*>(workspace);
  unsigned* kv[2][2] = {{reinterpret_cast<unsigned*>(base + p.off[LV_KEY_A]), reinterpret_cast<unsigned*>(base + p.off[LV_VAL_A])},
                        {reinterpret_cast<unsigned*>(base + p.off[LV_KEY_B]), reinterpret_cast<unsigned*>(base + p.off[LV_VAL_B])}};
  int* hist = reinterpret_cast<int*>(base + p.off[LV_HIST]);
  int* dtot = reinterpret_cast<int*>(base + p.off[LV_DTOT]);
  int* tileG = reinterpret_cast<int*>(base + p.off[LV_TILE_G]);
  int* tileB = reinterpret_cast<int*>(base + p.off[LV_TILE_B]);
  int* segG = reinterpret_cast<int*>(base + p.off[LV_SEG_G]);
  double* wseg = reinterpret_cast<double*>(base + p.off[LV_WSEG]);
  double* part = reinterpret_cast<double*>(base + p.off[LV_PART]);
  float* gw = reinterpret_cast<float*>(kv[1][0]);      // g by position: the second key buffer, free once the sort is done
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(LV_THREADS), grid((unsigned)p.grid);

  if (cls) hipLaunchKernelGGL(lovasz_keys_class_kernel, dim3((unsigned)p.keys_grid), block, 0, s, tab, g, static_cast<const int*>(target), kv[0][0], kv[0][1], tileG, errors);
  else hipLaunchKernelGGL(lovasz_keys_binary_kernel, dim3((unsigned)p.keys_grid), block, 0, s, tab, g, static_cast<const float*>(target), kv[0][0], kv[0][1], tileG, errors);
  UZ_LAUNCH_CHECK("uz_lovasz_loss(keys)");
  hipLaunchKernelGGL(lovasz_segments_kernel, dim3((unsigned)p.seg_grid), block, 0, s, g, (const int*)tileG, segG, wseg);
  UZ_LAUNCH_CHECK("uz_lovasz_loss(segments)");
  for (int pass = 0; pass < LV_PASSES; ++pass) {
    unsigned* const* src = kv[pass & 1];
    unsigned* const* dst = kv[(pass & 1) ^ 1];
    hipLaunchKernelGGL(lovasz_hist_kernel, grid, block, 0, s, g, 8 * pass, (const unsigned*)src[0], hist);
    UZ_LAUNCH_CHECK("uz_lovasz_loss(hist)");
    hipLaunchKernelGGL(lovasz_rowscan_kernel, dim3((unsigned)p.row_grid), block, 0, s, g, hist, dtot);
    UZ_LAUNCH_CHECK("uz_lovasz_loss(rowscan)");
    hipLaunchKernelGGL(lovasz_scatter_kernel, grid, block, 0, s, g, 8 * pass, (const unsigned*)src[0], (const unsigned*)src[1], dst[0], dst[1],
                       (const int*)hist, (const int*)dtot);
    UZ_LAUNCH_CHECK("uz_lovasz_loss(scatter)");
  }
  hipLaunchKernelGGL(lovasz_bits_kernel, grid, block, 0, s, g, (const unsigned*)kv[0][1], tileB);
  UZ_LAUNCH_CHECK("uz_lovasz_loss(bits)");
  hipLaunchKernelGGL(lovasz_scan_kernel, grid, block, 0, s, g, (const unsigned*)kv[0][0], (const unsigned*)kv[0][1], (const int*)tileB,
                     (const int*)segG, gw, ranks, part);
  UZ_LAUNCH_CHECK("uz_lovasz_loss(scan)");
  if (any_grad) {
    const dim3 ggrid((unsigned)p.grad_grid);
    if (cls) hipLaunchKernelGGL(lovasz_grad_class_kernel, ggrid, block, 0, s, tab, g, static_cast<const int*>(target), (const float*)gw, (const double*)wseg, scales);
    else hipLaunchKernelGGL(lovasz_grad_binary_kernel, ggrid, block, 0, s, tab, g, static_cast<const float*>(target), (const float*)gw, (const double*)wseg, scales);
    UZ_LAUNCH_CHECK("uz_lovasz_loss(grad)");
  }
  hipLaunchKernelGGL(lovasz_finalize_kernel, dim3(1), block, 0, s, tab, g, (const double*)part, (const double*)wseg, scales, base_loss, out);
  UZ_LAUNCH_CHECK("uz_lovasz_loss(finalize)");
  return UZ_OK;
}
