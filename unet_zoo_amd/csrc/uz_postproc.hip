// Mask post-processing on the device: fill holes, connected components, drop small ones, keep the k largest, number the
// survivors in raster order -- per (image, plane), every result an integer that scipy.ndimage gives too.
// A plane is `x > thr` of a channel (binary mode) or `argmax_K == c` (class mode); after the first launch the binary mode is
// the class mode with K = 2, first_class = 1 and every (image, channel) an image of its own, as in uz_surface.hip.
// Launches, every one with a grid fixed by the descriptor; what needs an order is a launch of its own, no workgroup ever
// waits for another one:
//   clear     the counters of the workspace
//   codes     the class of every pixel, one byte
//  [init      the COMPLEMENT of every plane as a set, parent = first pixel of the pixel's run inside its 64-pixel word
//   merge     atomic-min union-find over the cross                                  } only with fill_holes
//   compress  parent = root; the root collects the area and whether the set touches the picture's edge
//   fill      plane = plane + the complement pixels whose set does not touch the edge]
//   init, merge (cross or square), compress   the same three on the plane itself
//   top x 8   round r: the largest (area, smallest root) key below the key of round r - 1, one 64-bit integer maximum
//   keep      mask, kept roots per unit, boxes and coordinate sums of the eight largest kept components (integer atomics)
//   scan      per plane: exclusive scan of the unit counts
//   number    every kept root takes its raster-order number
//   apply     the label plane
//   finalize  stats and comps
//  [classmap  class mode]
// During merge and compress every access to the parent plane is a relaxed atomic of agent scope (uz_postproc_core.h says why
// a stale parent is harmless); later launches read it with plain loads.  Every find / union is bounded by H * W steps and sets
// the plane's error word when the bound trips.
#include "uz_common.h"
#include "uz_postproc_core.h"

#include <limits.h>

namespace {

constexpr int PP_THREADS = 256;
constexpr int PP_MAX_HW = 4096;
constexpr int PP_EDGE = 1 << 30;          // area word of a root: the set touches the picture's edge
constexpr int PP_AREA = PP_EDGE - 1;
constexpr int PP_CNT = 8;                 // counters of a plane: found, kept, area, area kept, filled, error, two spare
constexpr int PP_ACC = 6;                 // per top component: H-1-i_min, W-1-j_min, i_max, j_max, sum i, sum j (all >= 0)

struct PpGeo {
  int mode;
  int M;        // images of the class formulation: N (class mode) or N * C (binary mode)
  int K;        // classes of an image; 2 in the binary mode
  int first;    // first class that is a plane
  int P;        // planes per image: K - first
  int NP;       // M * P
  int H, W, HW;
  int tiles;    // units of PP_THREADS pixels per plane
  int units;    // NP * tiles
  int conn, min_area, keep;
  float thr;
};

struct PpWs {
  unsigned char* codes;          // M * HW
  unsigned char* set;            // NP * HW: the set being labelled (the complement, then the plane)
  int* parent;                   // NP * HW
  int* area;                     // NP * HW: at a root, the area (| PP_EDGE); after `number`, the label of a kept root
  int* ucnt;                     // units: kept roots of the unit
  int* uoff;                     // units: kept roots of the plane before the unit
  long long* cnt;                // NP * PP_CNT           } cleared by every call
  unsigned long long* top;       // NP * 8                }
  long long* acc;                // NP * 8 * PP_ACC       }
};

__global__ __launch_bounds__(PP_THREADS) void postproc_clear_kernel(int4* __restrict__ p, long long n4) {
  for (long long i = (long long)blockIdx.x * PP_THREADS + threadIdx.x; i < n4; i += (long long)gridDim.x * PP_THREADS)
    p[i] = make_int4(0, 0, 0, 0);
}

// one pixel per thread and step; the K planes of a pixel are read unconditionally from a clamped pixel
template <int MODE>
__global__ __launch_bounds__(PP_THREADS) void postproc_codes_kernel(PpGeo geo, const float* __restrict__ x, unsigned char* __restrict__ codes) {
  const long long total = (long long)geo.M * geo.HW;
  for (long long base = (long long)blockIdx.x * PP_THREADS; base < total; base += (long long)gridDim.x * PP_THREADS) {
    const long long e = base + threadIdx.x;
    const bool live = e < total;
    const long long ec = live ? e : total - 1;
    int code;
    if (MODE == UZ_POST_BINARY) {
      code = x[ec] > geo.thr ? 1 : 0;
    } else {
      const int m = (int)(ec / geo.HW), pix = (int)(ec - (long long)m * geo.HW);
      const float* __restrict__ xp = x + (size_t)m * geo.K * geo.HW + pix;
      float best = xp[0];
      code = 0;
      for (int c = 1; c < geo.K; ++c) {
        const float v = xp[(size_t)c * geo.HW];
        const bool up = v > best;          // ties: the lowest index, as uz_class_loss and uz_surface
        best = up ? v : best;
        code = up ? c : code;
      }
    }
    if (live) codes[e] = (unsigned char)code;
  }
}

// A unit is PP_THREADS consecutive pixels of one plane; a workgroup takes units blockIdx.x, blockIdx.x + gridDim.x, ...
#define PP_UNIT_LOOP                                                        \
  for (int unit = blockIdx.x; unit < geo.units; unit += gridDim.x)
#define PP_UNIT_PIXEL                                                       \
  const int plane = unit / geo.tiles, tile = unit - plane * geo.tiles;      \
  const int pix = tile * PP_THREADS + (int)threadIdx.x;                     \
  const bool live = pix < geo.HW;                                           \
  const int pc = live ? pix : geo.HW - 1;                                   \
  const size_t pb = (size_t)plane * geo.HW

// SRC 0: the set is the plane (code == class); 1: its complement; 2: the set plane as the fill launch left it
template <int SRC>
__global__ __launch_bounds__(PP_THREADS) void postproc_init_kernel(PpGeo geo, const unsigned char* __restrict__ codes,
                                                                   unsigned char* __restrict__ set, int* __restrict__ parent,
                                                                   int* __restrict__ area) {
  const int lane = threadIdx.x & 63;
  PP_UNIT_LOOP {
    PP_UNIT_PIXEL;
    const int m = plane / geo.P, cls = geo.first + (plane - m * geo.P);
    bool in;
    if (SRC == 2) in = set[pb + pc] != 0;
    else in = ((int)codes[(size_t)m * geo.HW + pc] == cls) == (SRC == 0);
    in = in && live;
    const int j = pc % geo.W;
    const unsigned long long inb = __ballot(in), rsb = __ballot(j == 0);
    const int start = in ? pix - lane + pp_run_start(inb, rsb, lane) : pix;
    if (live) {
      if (SRC != 2) set[pb + pix] = in ? 1 : 0;
      parent[pb + pix] = start;
      area[pb + pix] = 0;
    }
  }
}

__global__ __launch_bounds__(PP_THREADS) void postproc_merge_kernel(PpGeo geo, int conn, const unsigned char* __restrict__ set,
                                                                    int* __restrict__ parent, long long* __restrict__ cnt) {
  const int W = geo.W;
  PP_UNIT_LOOP {
    PP_UNIT_PIXEL;
    const unsigned char* __restrict__ s = set + pb;
    int* __restrict__ par = parent + pb;
    const int i = pc / W, j = pc - i * W;
    // unconditional loads from clamped pixels, the picture's edge is selected afterwards
    const int iu = i > 0 ? i - 1 : 0, jl = j > 0 ? j - 1 : 0, jr = j + 1 < W ? j + 1 : W - 1;
    const unsigned char c0 = s[pc], cl = s[i * W + jl], cr = s[i * W + jr], cul = s[iu * W + jl], cu = s[iu * W + j], cur = s[iu * W + jr];
    const bool in = live && c0 != 0;
    const bool l = j > 0 && cl != 0, r = j + 1 < W && cr != 0;
    const bool u = i > 0 && cu != 0, ul = i > 0 && j > 0 && cul != 0, ur = i > 0 && j + 1 < W && cur != 0;
    const unsigned links = in ? pp_links(conn, (pc & 63) == 0, l, r, ul, u, ur) : 0u;
    int rc = 0;
    if (links & PP_LEFT) rc |= pp_union(par, pc, pc - 1, geo.HW);
    if (links & PP_UP) rc |= pp_union(par, pc, pc - W, geo.HW);
    if (links & PP_UPLEFT) rc |= pp_union(par, pc, pc - W - 1, geo.HW);
    if (links & PP_UPRIGHT) rc |= pp_union(par, pc, pc - W + 1, geo.HW);
    if (rc != 0) atomicOr((unsigned long long*)&cnt[(size_t)plane * PP_CNT + 5], 1ull);
  }
}

// COUNT: the plane's own pass (found components and area go to the counters)
template <bool COUNT>
__global__ __launch_bounds__(PP_THREADS) void postproc_compress_kernel(PpGeo geo, const unsigned char* __restrict__ set,
                                                                       int* __restrict__ parent, int* __restrict__ area,
                                                                       long long* __restrict__ cnt) {
  const int H = geo.H, W = geo.W;
  const int lane = threadIdx.x & 63;
  PP_UNIT_LOOP {
    PP_UNIT_PIXEL;
    int* __restrict__ par = parent + pb;
    const bool in = live && set[pb + pc] != 0;
    int root = in ? pp_find(par, pc, geo.HW) : pc;
    const bool bad = root == PP_NONE;
    root = bad ? pc : root;
    // an atomic store: others may be walking through this pixel; the root is an ancestor, so whichever value they see works
    if (in) __hip_atomic_store(par + pc, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int i = pc / W, j = pc - i * W;
    const bool edge = i == 0 || j == 0 || i == H - 1 || j == W - 1;
    // one integer atomic per distinct root of the wave
    unsigned long long todo = __ballot(in);
    bool act = in;
    while (todo) {
      const int leader = __ffsll(todo) - 1;
      const int b = __shfl(root, leader);
      const unsigned long long same = __ballot(act && root == b);
      const unsigned long long onedge = __ballot(act && root == b && edge);
      if (lane == leader) {
        atomicAdd(area + pb + b, __popcll(same));
        if (onedge) atomicOr(area + pb + b, PP_EDGE);
      }
      act = act && root != b;
      todo &= ~same;
    }
    const int nbad = __syncthreads_count(bad);
    if (COUNT) {
      const int nin = __syncthreads_count(in), nroot = __syncthreads_count(in && root == pc);
      if (threadIdx.x == 0) {
        if (nroot) atomicAdd((unsigned long long*)&cnt[(size_t)plane * PP_CNT + 0], (unsigned long long)nroot);
        if (nin) atomicAdd((unsigned long long*)&cnt[(size_t)plane * PP_CNT + 2], (unsigned long long)nin);
      }
    }
    if (threadIdx.x == 0 && nbad) atomicOr((unsigned long long*)&cnt[(size_t)plane * PP_CNT + 5], 2ull);
  }
}

// set (the complement) -> set (the plane with its holes filled): plain loads, the labelling of the complement is finished
__global__ __launch_bounds__(PP_THREADS) void postproc_fill_kernel(PpGeo geo, unsigned char* __restrict__ set, const int* __restrict__ parent,
                                                                   const int* __restrict__ area, long long* __restrict__ cnt) {
  PP_UNIT_LOOP {
    PP_UNIT_PIXEL;
    const bool comp = set[pb + pc] != 0;
    const int root = parent[pb + pc];                    // a pixel outside the set is its own parent
    const bool open = (area[pb + root] & PP_EDGE) != 0;
    const bool hole = live && comp && !open;
    if (live) set[pb + pix] = (!comp || hole) ? 1 : 0;
    const int nh = __syncthreads_count(hole);
    if (threadIdx.x == 0 && nh) atomicAdd((unsigned long long*)&cnt[(size_t)plane * PP_CNT + 4], (unsigned long long)nh);
  }
}

__global__ __launch_bounds__(PP_THREADS) void postproc_top_kernel(PpGeo geo, int round, const unsigned char* __restrict__ set,
                                                                  const int* __restrict__ parent, const int* __restrict__ area,
                                                                  unsigned long long* __restrict__ top) {
  __shared__ unsigned long long best;
  PP_UNIT_LOOP {
    PP_UNIT_PIXEL;
    if (threadIdx.x == 0) best = 0ull;
    __syncthreads();
    const unsigned long long prev = round > 0 ? top[(size_t)plane * 8 + round - 1] : ~0ull;
    const bool root = live && set[pb + pc] != 0 && parent[pb + pc] == pc;
    const int a = area[pb + pc] & PP_AREA;
    const unsigned long long key = pp_key(a, pc);
    if (root && a >= geo.min_area && key < prev) atomicMax(&best, key);
    __syncthreads();
    if (threadIdx.x == 0 && best != 0ull) atomicMax(top + (size_t)plane * 8 + round, best);
    __syncthreads();
  }
}

__global__ __launch_bounds__(PP_THREADS) void postproc_keep_kernel(PpGeo geo, const unsigned char* __restrict__ set, const int* __restrict__ parent,
                                                                   const int* __restrict__ area, const unsigned long long* __restrict__ top,
                                                                   unsigned char* __restrict__ mask, int* __restrict__ ucnt,
                                                                   long long* __restrict__ cnt, long long* __restrict__ acc) {
  __shared__ unsigned long long tk[8];
  __shared__ int sa[8][PP_ACC];
  const int H = geo.H, W = geo.W;
  PP_UNIT_LOOP {
    PP_UNIT_PIXEL;
    if (threadIdx.x < 8) tk[threadIdx.x] = top[(size_t)plane * 8 + threadIdx.x];
    if (threadIdx.x < 8 * PP_ACC) sa[threadIdx.x / PP_ACC][threadIdx.x % PP_ACC] = 0;
    __syncthreads();
    const bool in = live && set[pb + pc] != 0;
    const int root = parent[pb + pc];
    const int a = area[pb + root] & PP_AREA;
    const unsigned long long key = pp_key(a, root);
    // with fewer than `keep` candidates the key of round keep - 1 is 0: every candidate stays
    const bool kept = in && a >= geo.min_area && (geo.keep == 0 || key >= tk[geo.keep - 1]);
    if (live) mask[pb + pix] = kept ? 1 : 0;
    const int nrec = geo.keep == 0 ? 8 : geo.keep;
    int rec = -1;
#pragma unroll
    for (int r = 0; r < 8; ++r) rec = (kept && r < nrec && key == tk[r]) ? r : rec;
    if (rec >= 0) {
      const int i = pc / W, j = pc - i * W;
      atomicMax(&sa[rec][0], H - 1 - i);
      atomicMax(&sa[rec][1], W - 1 - j);
      atomicMax(&sa[rec][2], i);
      atomicMax(&sa[rec][3], j);
      atomicAdd(&sa[rec][4], i);          // 256 pixels of coordinates below 4096: far from 2^31
      atomicAdd(&sa[rec][5], j);
    }
    const int nk = __syncthreads_count(kept), nr = __syncthreads_count(kept && root == pc);
    const int any = __syncthreads_or(rec >= 0);
    if (threadIdx.x == 0) {
      ucnt[unit] = nr;
      if (nk) atomicAdd((unsigned long long*)&cnt[(size_t)plane * PP_CNT + 3], (unsigned long long)nk);
    }
    if (any && threadIdx.x < 8 * PP_ACC) {
      const int r = threadIdx.x / PP_ACC, f = threadIdx.x % PP_ACC;
      const int v = sa[r][f];
      long long* dst = acc + ((size_t)plane * 8 + r) * PP_ACC + f;
      if (v > 0) {
        if (f < 4) atomicMax(dst, (long long)v);
        else atomicAdd((unsigned long long*)dst, (unsigned long long)v);
      }
    }
    __syncthreads();
  }
}

// one workgroup per plane: uoff = exclusive scan of ucnt over the plane's units, the total = components kept
__global__ __launch_bounds__(PP_THREADS) void postproc_scan_kernel(PpGeo geo, const int* __restrict__ ucnt, int* __restrict__ uoff,
                                                                   long long* __restrict__ cnt) {
  __shared__ int part[PP_THREADS];
  for (int plane = blockIdx.x; plane < geo.NP; plane += gridDim.x) {
    const int per = (geo.tiles + PP_THREADS - 1) / PP_THREADS;
    const int t0 = min((int)threadIdx.x * per, geo.tiles), t1 = min(t0 + per, geo.tiles);
    const int* __restrict__ c = ucnt + (size_t)plane * geo.tiles;
    int s = 0;
    for (int t = t0; t < t1; ++t) s += c[t];
    part[threadIdx.x] = s;
    __syncthreads();
    int before = 0;
    for (int u = 0; u < (int)threadIdx.x; ++u) before += part[u];
    for (int t = t0; t < t1; ++t) {
      uoff[(size_t)plane * geo.tiles + t] = before;
      before += c[t];
    }
    if (threadIdx.x == PP_THREADS - 1) cnt[(size_t)plane * PP_CNT + 1] = before;
    __syncthreads();
  }
}

// a kept root's number: kept roots of the plane before its unit + kept roots of the unit before it + 1 (raster order)
__global__ __launch_bounds__(PP_THREADS) void postproc_number_kernel(PpGeo geo, const unsigned char* __restrict__ mask, const int* __restrict__ parent,
                                                                     const int* __restrict__ uoff, int* __restrict__ area) {
  __shared__ int wsum[PP_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  PP_UNIT_LOOP {
    PP_UNIT_PIXEL;
    const bool root = live && mask[pb + pc] != 0 && parent[pb + pc] == pc;
    const unsigned long long b = __ballot(root);
    if (lane == 0) wsum[wave] = __popcll(b);
    __syncthreads();
    int before = uoff[unit] + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) before += wsum[w];
    if (root) area[pb + pix] = before + 1;
    __syncthreads();
  }
}

__global__ __launch_bounds__(PP_THREADS) void postproc_apply_kernel(PpGeo geo, const unsigned char* __restrict__ mask, const int* __restrict__ parent,
                                                                    const int* __restrict__ area, int* __restrict__ labels) {
  PP_UNIT_LOOP {
    PP_UNIT_PIXEL;
    const int lab = area[pb + parent[pb + pc]];
    const bool on = mask[pb + pc] != 0;
    if (live && labels) labels[pb + pix] = on ? lab : 0;
  }
}

__global__ __launch_bounds__(PP_THREADS) void postproc_finalize_kernel(PpGeo geo, const long long* __restrict__ cnt,
                                                                       const unsigned long long* __restrict__ top,
                                                                       const long long* __restrict__ acc, long long* __restrict__ stats,
                                                                       long long* __restrict__ comps) {
  const int plane = blockIdx.x * PP_THREADS + threadIdx.x;
  if (plane >= geo.NP) return;
  const long long* c = cnt + (size_t)plane * PP_CNT;
  const unsigned long long* t = top + (size_t)plane * 8;
  long long* st = stats + (size_t)plane * 8;
  st[0] = c[0], st[1] = c[1], st[2] = c[2], st[3] = c[3], st[4] = c[4];
  st[5] = pp_key_area(t[0]);
  st[6] = c[5], st[7] = 0;
  const int nrec = geo.keep == 0 ? 8 : geo.keep;
  for (int r = 0; r < 8; ++r) {
    long long* o = comps + ((size_t)plane * 8 + r) * 8;
    const long long* a = acc + ((size_t)plane * 8 + r) * PP_ACC;
    const bool used = r < nrec && t[r] != 0ull;
    o[0] = used ? pp_key_area(t[r]) : 0;
    o[1] = used ? geo.H - 1 - a[0] : 0;
    o[2] = used ? geo.W - 1 - a[1] : 0;
    o[3] = used ? a[2] : 0;
    o[4] = used ? a[3] : 0;
    o[5] = used ? a[4] : 0;
    o[6] = used ? a[5] : 0;
    o[7] = used ? pp_key_root(t[r]) : 0;
  }
}

// the argmax class where its plane kept the pixel, else the lowest class whose final plane holds it (a filled hole), else 0
__global__ __launch_bounds__(PP_THREADS) void postproc_classmap_kernel(PpGeo geo, const unsigned char* __restrict__ codes,
                                                                       const unsigned char* __restrict__ mask, unsigned char* __restrict__ cmap) {
  const long long total = (long long)geo.M * geo.HW;
  for (long long base = (long long)blockIdx.x * PP_THREADS; base < total; base += (long long)gridDim.x * PP_THREADS) {
    const long long e = base + threadIdx.x;
    const bool live = e < total;
    const long long ec = live ? e : total - 1;
    const int m = (int)(ec / geo.HW), pix = (int)(ec - (long long)m * geo.HW);
    const int code = codes[ec];
    const unsigned char* __restrict__ mk = mask + (size_t)m * geo.P * geo.HW + pix;
    int lowest = 0;
    bool own = false;
    for (int p = geo.P - 1; p >= 0; --p) {
      const bool on = mk[(size_t)p * geo.HW] != 0;
      lowest = on ? geo.first + p : lowest;
      own = own || (on && geo.first + p == code);
    }
    if (live && cmap) cmap[e] = (unsigned char)(own ? code : lowest);
  }
}

struct PpPlan {
  PpGeo geo;
  int grid;                     // the per-unit launches
  int clear_grid, codes_grid, scan_grid, fin_grid;
  long long off[9], bytes;      // codes, set, parent, area, ucnt, uoff, cnt, top, acc
};

int pp_plan(const uz_postproc_desc* d, const char* who, PpPlan* p) {
  UZ_REQUIRE(d != nullptr, "%s: null descriptor", who);
  UZ_REQUIRE(d->mode == UZ_POST_BINARY || d->mode == UZ_POST_CLASS, "%s: unknown mode %d", who, d->mode);
  UZ_REQUIRE(d->N >= 1 && d->C >= 1 && d->H >= 1 && d->W >= 1, "%s: non-positive shape", who);
  UZ_REQUIRE(d->H <= PP_MAX_HW && d->W <= PP_MAX_HW, "%s: H = %d, W = %d above %d", who, d->H, d->W, PP_MAX_HW);
  if (d->mode == UZ_POST_CLASS) {
    UZ_REQUIRE(d->C >= 2 && d->C <= UZ_CLASS_MAX_K, "%s: K = %d outside [2, %d]", who, d->C, UZ_CLASS_MAX_K);
    UZ_REQUIRE(d->first_class >= 0 && d->first_class < d->C, "%s: first_class = %d outside [0, %d)", who, d->first_class, d->C);
  }
  UZ_REQUIRE(d->connectivity == 1 || d->connectivity == 2, "%s: connectivity = %d, must be 1 or 2", who, d->connectivity);
  UZ_REQUIRE(d->fill_holes == 0 || d->fill_holes == 1, "%s: fill_holes = %d, must be 0 or 1", who, d->fill_holes);
  UZ_REQUIRE(d->min_area >= 0, "%s: min_area = %d is negative", who, d->min_area);
  UZ_REQUIRE(d->keep_largest >= 0 && d->keep_largest <= UZ_POST_MAX_KEEP, "%s: keep_largest = %d outside [0, %d]", who, d->keep_largest,
             UZ_POST_MAX_KEEP);
  UZ_REQUIRE(d->thr == d->thr, "%s: thr is not a number", who);
  UZ_REQUIRE((long long)d->N * d->C * d->H * d->W < (1LL << 31), "%s: too large (N C H W >= 2^31)", who);
  PpGeo& g = p->geo;
  const bool cls = d->mode == UZ_POST_CLASS;
  g.mode = d->mode;
  g.M = cls ? d->N : d->N * d->C;
  g.K = cls ? d->C : 2;
  g.first = cls ? d->first_class : 1;
  g.P = g.K - g.first;
  g.NP = g.M * g.P;
  g.H = d->H, g.W = d->W, g.HW = d->H * d->W;
  g.tiles = uz_cdiv(g.HW, PP_THREADS);
  g.units = g.NP * g.tiles;          // below 2^31 / 256 + N P
  g.conn = d->connectivity, g.min_area = d->min_area, g.keep = d->keep_largest;
  g.thr = d->thr;
  // eight workgroups of four waves per CU of the hardware: what can be resident at once; more units than that are walked
  p->grid = uz_grid_cap(g.units, 8);
  p->codes_grid = uz_grid_cap(((long long)g.M * g.HW + PP_THREADS - 1) / PP_THREADS, 8);
  p->scan_grid = uz_grid_cap(g.NP, 8);
  p->fin_grid = uz_cdiv(g.NP, PP_THREADS);
  const long long px = (long long)g.NP * g.HW;
  const long long sizes[9] = {(long long)g.M * g.HW, px, 4 * px, 4 * px, 4LL * g.units, 4LL * g.units, 8LL * g.NP * PP_CNT, 8LL * g.NP * 8,
                              8LL * g.NP * 8 * PP_ACC};
  p->bytes = uz_carve(sizes, 9, p->off);
  p->clear_grid = uz_grid_cap(uz_cdiv((p->bytes - p->off[6]) / 16, PP_THREADS), 8);      // cnt, top, acc as int4
  return UZ_OK;
}

}  // namespace

extern "C" long long uz_postproc_workspace_bytes(const uz_postproc_desc* d) {
  PpPlan p;
  if (pp_plan(d, "uz_postproc_workspace_bytes", &p) != UZ_OK) return -1;
  return p.bytes;
}

extern "C" int uz_postproc_grid(const uz_postproc_desc* d, int* units) {
  PpPlan p;
  const int rc = pp_plan(d, "uz_postproc_grid", &p);
  if (rc != UZ_OK) return rc;
  if (units) *units = p.geo.units;
  return p.grid;
}

extern "C" int uz_postproc(const uz_postproc_desc* d, const float* x, unsigned char* mask, int* labels, unsigned char* class_map,
                           long long* stats, long long* comps, void* workspace, void* stream) {
  PpPlan p;
  const int rc = pp_plan(d, "uz_postproc", &p);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(x && mask && stats && comps && workspace, "uz_postproc: null pointer");
  UZ_REQUIRE(class_map == nullptr || d->mode == UZ_POST_CLASS, "uz_postproc: class_map belongs to the class mode");
  UZ_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)labels & 3) == 0, "uz_postproc: x and labels must be 4-byte aligned");
  UZ_REQUIRE(((uintptr_t)stats & 7) == 0 && ((uintptr_t)comps & 7) == 0, "uz_postproc: stats and comps must be 8-byte aligned");
  UZ_REQUIRE(((uintptr_t)workspace & 15) == 0, "uz_postproc: the workspace must be 16-byte aligned");
  const PpGeo& g = p.geo;
  const long long px = (long long)g.NP * g.HW;
  const UzRange r[7] = {uz_range(x, 4LL * d->N * d->C * g.HW), uz_range(mask, px), uz_range(labels, 4 * px),
                        uz_range(class_map, (long long)g.M * g.HW), uz_range(stats, 64LL * g.NP), uz_range(comps, 512LL * g.NP),
                        uz_range(workspace, p.bytes)};
  UZ_REQUIRE(!uz_any_overlap(r, 7, nullptr, 0), "uz_postproc: tensors overlap");
  char* base = static_cast<char*>(workspace);
  PpWs ws;
  ws.codes = reinterpret_cast<unsigned char*>(base + p.off[0]);
  ws.set = reinterpret_cast<unsigned char*>(base + p.off[1]);
  ws.parent = reinterpret_cast<int*>(base + p.off[2]);
  ws.area = reinterpret_cast<int*>(base + p.off[3]);
  ws.ucnt = reinterpret_cast<int*>(base + p.off[4]);
  ws.uoff = reinterpret_cast<int*>(base + p.off[5]);
  ws.cnt = reinterpret_cast<long long*>(base + p.off[6]);
  ws.top = reinterpret_cast<unsigned long long*>(base + p.off[7]);
  ws.acc = reinterpret_cast<long long*>(base + p.off[8]);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(PP_THREADS), ugrid((unsigned)p.grid), cgrid((unsigned)p.codes_grid);

  hipLaunchKernelGGL(postproc_clear_kernel, dim3((unsigned)p.clear_grid), block, 0, s, reinterpret_cast<int4*>(ws.cnt),
                     (p.bytes - p.off[6]) / 16);
  UZ_LAUNCH_CHECK("uz_postproc(clear)");
  if (d->mode == UZ_POST_BINARY) hipLaunchKernelGGL((postproc_codes_kernel<UZ_POST_BINARY>), cgrid, block, 0, s, g, x, ws.codes);
  else hipLaunchKernelGGL((postproc_codes_kernel<UZ_POST_CLASS>), cgrid, block, 0, s, g, x, ws.codes);
  UZ_LAUNCH_CHECK("uz_postproc(codes)");
  if (d->fill_holes) {
    hipLaunchKernelGGL((postproc_init_kernel<1>), ugrid, block, 0, s, g, (const unsigned char*)ws.codes, ws.set, ws.parent, ws.area);
    UZ_LAUNCH_CHECK("uz_postproc(init, complement)");
    hipLaunchKernelGGL(postproc_merge_kernel, ugrid, block, 0, s, g, 1, (const unsigned char*)ws.set, ws.parent, ws.cnt);
    UZ_LAUNCH_CHECK("uz_postproc(merge, complement)");
    hipLaunchKernelGGL((postproc_compress_kernel<false>), ugrid, block, 0, s, g, (const unsigned char*)ws.set, ws.parent, ws.area, ws.cnt);
    UZ_LAUNCH_CHECK("uz_postproc(compress, complement)");
    hipLaunchKernelGGL(postproc_fill_kernel, ugrid, block, 0, s, g, ws.set, (const int*)ws.parent, (const int*)ws.area, ws.cnt);
    UZ_LAUNCH_CHECK("uz_postproc(fill)");
    hipLaunchKernelGGL((postproc_init_kernel<2>), ugrid, block, 0, s, g, (const unsigned char*)ws.codes, ws.set, ws.parent, ws.area);
  } else {
    hipLaunchKernelGGL((postproc_init_kernel<0>), ugrid, block, 0, s, g, (const unsigned char*)ws.codes, ws.set, ws.parent, ws.area);
  }
  UZ_LAUNCH_CHECK("uz_postproc(init)");
  hipLaunchKernelGGL(postproc_merge_kernel, ugrid, block, 0, s, g, g.conn, (const unsigned char*)ws.set, ws.parent, ws.cnt);
  UZ_LAUNCH_CHECK("uz_postproc(merge)");
  hipLaunchKernelGGL((postproc_compress_kernel<true>), ugrid, block, 0, s, g, (const unsigned char*)ws.set, ws.parent, ws.area, ws.cnt);
  UZ_LAUNCH_CHECK("uz_postproc(compress)");
  for (int round = 0; round < 8; ++round) {
    hipLaunchKernelGGL(postproc_top_kernel, ugrid, block, 0, s, g, round, (const unsigned char*)ws.set, (const int*)ws.parent,
                       (const int*)ws.area, ws.top);
    UZ_LAUNCH_CHECK("uz_postproc(top)");
  }
  hipLaunchKernelGGL(postproc_keep_kernel, ugrid, block, 0, s, g, (const unsigned char*)ws.set, (const int*)ws.parent, (const int*)ws.area,
                     (const unsigned long long*)ws.top, mask, ws.ucnt, ws.cnt, ws.acc);
  UZ_LAUNCH_CHECK("uz_postproc(keep)");
  hipLaunchKernelGGL(postproc_scan_kernel, dim3((unsigned)p.scan_grid), block, 0, s, g, (const int*)ws.ucnt, ws.uoff, ws.cnt);
  UZ_LAUNCH_CHECK("uz_postproc(scan)");
  // launched whether or not the optional outputs are asked for: the launches of a call depend on the descriptor alone
  hipLaunchKernelGGL(postproc_number_kernel, ugrid, block, 0, s, g, (const unsigned char*)mask, (const int*)ws.parent, (const int*)ws.uoff,
                     ws.area);
  UZ_LAUNCH_CHECK("uz_postproc(number)");
  hipLaunchKernelGGL(postproc_apply_kernel, ugrid, block, 0, s, g, (const unsigned char*)mask, (const int*)ws.parent, (const int*)ws.area,
                     labels);
  UZ_LAUNCH_CHECK("uz_postproc(apply)");
  hipLaunchKernelGGL(postproc_finalize_kernel, dim3((unsigned)p.fin_grid), block, 0, s, g, (const long long*)ws.cnt,
                     (const unsigned long long*)ws.top, (const long long*)ws.acc, stats, comps);
  UZ_LAUNCH_CHECK("uz_postproc(finalize)");
  if (d->mode == UZ_POST_CLASS) {
    hipLaunchKernelGGL(postproc_classmap_kernel, cgrid, block, 0, s, g, (const unsigned char*)ws.codes, (const unsigned char*)mask, class_map);
    UZ_LAUNCH_CHECK("uz_postproc(classmap)");
  }
  return UZ_OK;
}
