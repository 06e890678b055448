// Confusion counts on the device: TP / FP / FN / TN and the score histograms of a thresholded binary prediction, or the K x K
// confusion matrix of an argmax prediction, per image, and the overlap scores derived from them.  Every count is
// an integer: exact, independent of the order of arrival and of the grid.
// Three launches, every one with a fixed grid for a descriptor:
//   clear    the int32 workspace (counts, histograms)
//   count    a workgroup takes one contiguous run of (plane, tile) units; a tile is CF_TILE consecutive pixels of a plane (binary:
//            an (image, channel) plane; class: an image, whose K logit planes are read per pixel).  Loads are unconditional from
//            a clamped address, 16 bytes per lane where the plane size and the bases allow it.  Counts go to a
//            histogram in LDS, aggregated per wave first: ballots for TP / FP / FN / TN and the two end bins (a trained model
//            puts nearly every pixel there), one add per distinct bin of the wave for the rest.  When the run leaves a plane,
//            and at its end, the non-zero bins are added to the workspace with integer atomics.
//   finalize per plane (binary) or image (class): the counts as int64 and the scores, one float64 division each
#include "uz_common.h"

#include <math.h>

namespace {

constexpr int CF_THREADS = 256;
constexpr int CF_PER = 4;                          // pixels per thread and tile
constexpr int CF_TILE = CF_THREADS * CF_PER;
constexpr int CF_MIN_BINS = 16, CF_MAX_BINS = 1024;
constexpr int CF_MAX_HW = 4096;
constexpr int CF_MAX_K = UZ_CLASS_MAX_K;

struct CfGeo {
  int mode;
  int M;        // planes of the counting pass: N * C (binary) or N (class)
  int K;        // classes; 2 in the binary mode
  int first;    // first class that is a pair
  int P;        // pairs per image
  int HW;
  int tiles;    // units per plane
  int units;    // M * tiles
  int B;        // bins (binary), 0 otherwise
  int ignore_index;
};

__global__ __launch_bounds__(CF_THREADS) void confusion_clear_kernel(int4* __restrict__ p, long long n4) {
  for (long long i = (long long)blockIdx.x * CF_THREADS + threadIdx.x; i < n4; i += (long long)gridDim.x * CF_THREADS)
    p[i] = make_int4(0, 0, 0, 0);
}

// hist[bin] += 1 for every lane with act, one atomic per distinct bin of the wave.  Called by all 64 lanes together.
__device__ __forceinline__ void cf_wave_hist(int* __restrict__ hist, int bin, bool act) {
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

// the CF_PER values of this thread in tile `tile` of a plane of HW floats / ints: one 16-byte load (VEC: HW % 4 == 0 and the
// plane 16-byte aligned, so a quad is live or dead as a whole) or CF_PER coalesced 4-byte loads; always from a clamped address
template <bool VEC, typename T>
__device__ __forceinline__ void cf_load(const T* __restrict__ plane, int HW, int tile, T (&v)[CF_PER]) {
  if (VEC) {
    const int q = tile * CF_THREADS + (int)threadIdx.x, qn = HW >> 2;
    const int4 r = reinterpret_cast<const int4*>(plane)[q < qn ? q : qn - 1];
    static_assert(sizeof(T) == 4, "four bytes per element");
    v[0] = __builtin_bit_cast(T, r.x), v[1] = __builtin_bit_cast(T, r.y), v[2] = __builtin_bit_cast(T, r.z), v[3] = __builtin_bit_cast(T, r.w);
  } else {
#pragma unroll
    for (int e = 0; e < CF_PER; ++e) {
      const int pix = tile * CF_TILE + e * CF_THREADS + (int)threadIdx.x;
      v[e] = plane[pix < HW ? pix : HW - 1];
    }
  }
}
template <bool VEC>
__device__ __forceinline__ bool cf_live(int HW, int tile, int e) {
  return VEC ? (tile * CF_THREADS + (int)threadIdx.x) * 4 < HW : tile * CF_TILE + e * CF_THREADS + (int)threadIdx.x < HW;
}

// the run of units of this workgroup: [u0, u1), contiguous, so that a run crosses as few planes as can be
__device__ __forceinline__ void cf_run(int units, int* u0, int* u1) {
  *u0 = (int)((long long)blockIdx.x * units / gridDim.x);
  *u1 = (int)((long long)(blockIdx.x + 1) * units / gridDim.x);
}

// add the non-zero bins h[0 .. n) of the workgroup to dst and zero them.  Called by all threads, after a barrier.
__device__ __forceinline__ void cf_flush(int* __restrict__ h, int n, int* __restrict__ dst) {
  for (int i = threadIdx.x; i < n; i += CF_THREADS) {
    const int v = h[i];
    if (v) {
      atomicAdd(dst + i, v);
      h[i] = 0;
    }
  }
}

// Binary mode.  LDS: hist[2][B] (s = the target's side), the edges beside it, and the four counts.  acc[] are the wave's own
// sums since the last flush, the same in every lane: TP, FP, FN, TN, then bin 0 and bin B - 1 of the negatives and positives.
template <bool VEC>
__global__ __launch_bounds__(CF_THREADS) void confusion_binary_kernel(CfGeo geo, const float* __restrict__ logits, const float* __restrict__ target,
                                                                      const float* __restrict__ edges, int* __restrict__ wcnt,
                                                                      int* __restrict__ whist) {
  __shared__ int h[2 * CF_MAX_BINS];
  __shared__ float edge[CF_MAX_BINS];
  __shared__ int cnt[4];
  const int B = geo.B, lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < B - 1; i += CF_THREADS) edge[i] = edges[i];
  for (int i = threadIdx.x; i < 2 * B; i += CF_THREADS) h[i] = 0;
  if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
  __syncthreads();
  int u0, u1;
  cf_run(geo.units, &u0, &u1);
  int acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int cur = u0 / geo.tiles;
  for (int u = u0; u <= u1; ++u) {                     // u == u1: the flush at the end of the run
    const int plane = u < u1 ? u / geo.tiles : -1;
    if (plane != cur && u > u0) {                      // uniform over the workgroup
      if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (acc[e]) atomicAdd(&cnt[e], acc[e]);
        if (acc[4]) atomicAdd(&h[0], acc[4]);
        if (acc[5]) atomicAdd(&h[B - 1], acc[5]);
        if (acc[6]) atomicAdd(&h[B], acc[6]);
        if (acc[7]) atomicAdd(&h[2 * B - 1], acc[7]);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = 0;
      __syncthreads();
      cf_flush(h, 2 * B, whist + (size_t)cur * 2 * B);
      if (threadIdx.x < 4 && cnt[threadIdx.x]) {
        atomicAdd(wcnt + (size_t)cur * 4 + threadIdx.x, cnt[threadIdx.x]);
        cnt[threadIdx.x] = 0;
      }
      __syncthreads();
    }
    if (u == u1) break;
    cur = plane;
    const int tile = u - plane * geo.tiles;
    float x[CF_PER], t[CF_PER];
    cf_load<VEC>(logits + (size_t)plane * geo.HW, geo.HW, tile, x);
    cf_load<VEC>(target + (size_t)plane * geo.HW, geo.HW, tile, t);
#pragma unroll
    for (int e = 0; e < CF_PER; ++e) {
      const bool live = cf_live<VEC>(geo.HW, tile, e);
      int bin = 0;                                     // the number of edges <= x: B - 1 ascending edges, B a power of two
      for (int step = B >> 1; step > 0; step >>= 1) bin += x[e] >= edge[bin + step - 1] ? step : 0;      // NaN: never, bin 0
      const unsigned long long bl = __ballot(live), bp = __ballot(live && x[e] > 0.f), bt = __ballot(live && t[e] > 0.5f);
      const unsigned long long b0 = __ballot(live && bin == 0), b1 = __ballot(live && bin == B - 1);
      acc[0] += __popcll(bp & bt);
      acc[1] += __popcll(bp & ~bt);
      acc[2] += __popcll(bt & ~bp);
      acc[3] += __popcll(bl & ~bp & ~bt);
      acc[4] += __popcll(b0 & ~bt);
      acc[5] += __popcll(b1 & ~bt);
      acc[6] += __popcll(b0 & bt);
      acc[7] += __popcll(b1 & bt);
      cf_wave_hist(h, (t[e] > 0.5f ? B : 0) + bin, live && bin != 0 && bin != B - 1);
    }
  }
}

// Class mode.  LDS: the K x K matrix of the image, row = label, column = prediction.
template <bool VEC>
__global__ __launch_bounds__(CF_THREADS) void confusion_class_kernel(CfGeo geo, const float* __restrict__ logits, const int* __restrict__ target,
                                                                     int* __restrict__ wmat) {
  __shared__ int h[CF_MAX_K * CF_MAX_K];
  const int K = geo.K, KK = K * K;
  for (int i = threadIdx.x; i < KK; i += CF_THREADS) h[i] = 0;
  __syncthreads();
  int u0, u1;
  cf_run(geo.units, &u0, &u1);
  int cur = u0 / geo.tiles;
  for (int u = u0; u <= u1; ++u) {
    const int img = u < u1 ? u / geo.tiles : -1;
    if (img != cur && u > u0) {                        // uniform over the workgroup
      __syncthreads();
      cf_flush(h, KK, wmat + (size_t)cur * KK);
      __syncthreads();
    }
    if (u == u1) break;
    cur = img;
    const int tile = u - img * geo.tiles;
    const float* __restrict__ x = logits + (size_t)img * K * geo.HW;
    int y[CF_PER], pred[CF_PER];
    float best[CF_PER];
    cf_load<VEC>(target + (size_t)img * geo.HW, geo.HW, tile, y);
    cf_load<VEC>(x, geo.HW, tile, best);
#pragma unroll
    for (int e = 0; e < CF_PER; ++e) pred[e] = 0;
    for (int c = 1; c < K; ++c) {
      float v[CF_PER];
      cf_load<VEC>(x + (size_t)c * geo.HW, geo.HW, tile, v);
#pragma unroll
      for (int e = 0; e < CF_PER; ++e) {
        const bool up = v[e] > best[e];                // ties: the lowest index, as uz_class_loss
        best[e] = up ? v[e] : best[e];
        pred[e] = up ? c : pred[e];
      }
    }
#pragma unroll
    for (int e = 0; e < CF_PER; ++e) {
      const bool valid = cf_live<VEC>(geo.HW, tile, e) && y[e] >= 0 && y[e] < K && y[e] != geo.ignore_index;
      cf_wave_hist(h, valid ? y[e] * K + pred[e] : 0, valid);
    }
  }
}

// state of a pair from |prediction| and |target|
__device__ __forceinline__ int cf_state(long long na, long long nb) { return (na == 0 ? 1 : 0) | (nb == 0 ? 2 : 0); }
__device__ __forceinline__ float cf_ratio(long long num, long long den) { return den > 0 ? (float)((double)num / (double)den) : 0.f; }

__device__ __forceinline__ void cf_scores(long long tp, long long fp, long long fn, long long tn, float* __restrict__ o) {
  const int state = cf_state(tp + fp, tp + fn);
  o[0] = state == 3 ? 1.f : cf_ratio(2 * tp, 2 * tp + fp + fn);
  o[1] = state == 3 ? 1.f : cf_ratio(tp, tp + fp + fn);
  o[2] = cf_ratio(tp, tp + fp);
  o[3] = cf_ratio(tp, tp + fn);
  o[4] = cf_ratio(tn, tn + fp);
  o[5] = (float)state;
  o[6] = 0.f;
  o[7] = 0.f;
}

// one workgroup per plane: P = C, so the plane is the pair
__global__ __launch_bounds__(CF_THREADS) void confusion_finalize_binary_kernel(CfGeo geo, const int* __restrict__ wcnt, const int* __restrict__ whist,
                                                                               long long* __restrict__ counts, long long* __restrict__ hist,
                                                                               float* __restrict__ out) {
  const int plane = blockIdx.x, n = 2 * geo.B;
  for (int i = threadIdx.x; i < n; i += CF_THREADS) hist[(size_t)plane * n + i] = whist[(size_t)plane * n + i];
  if (threadIdx.x == 0) {
    const int* c = wcnt + (size_t)plane * 4;
    long long* d = counts + (size_t)plane * 4;
    d[0] = c[0], d[1] = c[1], d[2] = c[2], d[3] = c[3];
    cf_scores(c[0], c[1], c[2], c[3], out + (size_t)plane * 8);
  }
}

// one workgroup per image
__global__ __launch_bounds__(CF_THREADS) void confusion_finalize_class_kernel(CfGeo geo, const int* __restrict__ wmat, long long* __restrict__ counts,
                                                                              float* __restrict__ out) {
  __shared__ int m[CF_MAX_K * CF_MAX_K];
  const int img = blockIdx.x, K = geo.K, KK = K * K;
  for (int i = threadIdx.x; i < KK; i += CF_THREADS) {
    const int v = wmat[(size_t)img * KK + i];
    m[i] = v;
    counts[(size_t)img * KK + i] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < geo.P) {
    const int c = geo.first + (int)threadIdx.x;
    long long total = 0, row = 0, col = 0;
    for (int i = 0; i < KK; ++i) total += m[i];
    for (int j = 0; j < K; ++j) {
      row += m[c * K + j];
      col += m[j * K + c];
    }
    const long long tp = m[c * K + c], fp = col - tp, fn = row - tp;
    cf_scores(tp, fp, fn, total - tp - fp - fn, out + ((size_t)img * geo.P + threadIdx.x) * 8);
  }
}

struct CfPlan {
  CfGeo geo;
  int grid;                  // the counting pass
  int clear_grid;
  long long off_hist;        // binary: bytes from the counts to the histograms
  long long bytes;
};

int cf_plan(const uz_confusion_desc* d, const char* who, CfPlan* p) {
  UZ_REQUIRE(d != nullptr, "%s: null descriptor", who);
  UZ_REQUIRE(d->mode == UZ_CONFUSION_BINARY || d->mode == UZ_CONFUSION_CLASS, "%s: unknown mode %d", who, d->mode);
  UZ_REQUIRE(d->N >= 1 && d->C >= 1 && d->H >= 1 && d->W >= 1, "%s: non-positive shape (N, C, H, W must be >= 1)", who);
  UZ_REQUIRE(d->H <= CF_MAX_HW && d->W <= CF_MAX_HW, "%s: H = %d, W = %d above %d", who, d->H, d->W, CF_MAX_HW);
  const bool cls = d->mode == UZ_CONFUSION_CLASS;
  if (cls) {
    UZ_REQUIRE(d->C >= 2 && d->C <= CF_MAX_K, "%s: K = %d outside [2, %d]", who, d->C, CF_MAX_K);
    UZ_REQUIRE(d->first_class >= 0 && d->first_class < d->C, "%s: first_class = %d outside [0, %d)", who, d->first_class, d->C);
    UZ_REQUIRE(d->bins == 0, "%s: bins = %d, must be 0 in the class mode", who, d->bins);
  } else {
    UZ_REQUIRE(d->bins >= CF_MIN_BINS && d->bins <= CF_MAX_BINS && (d->bins & (d->bins - 1)) == 0,
               "%s: bins = %d, must be a power of two in [%d, %d]", who, d->bins, CF_MIN_BINS, CF_MAX_BINS);
  }
  UZ_REQUIRE(d->max_workgroups >= 0, "%s: max_workgroups = %d is negative", who, d->max_workgroups);
  UZ_REQUIRE((long long)d->N * d->C * d->H * d->W < (1LL << 31), "%s: too large (N C H W >= 2^31)", who);
  CfGeo& g = p->geo;
  g.mode = d->mode;
  g.M = cls ? d->N : d->N * d->C;
  g.K = cls ? d->C : 2;
  g.first = cls ? d->first_class : 1;
  g.P = cls ? g.K - g.first : d->C;
  g.HW = d->H * d->W;
  g.tiles = uz_cdiv(g.HW, CF_TILE);
  g.units = g.M * g.tiles;                 // below 2^31 / 1024 + M
  g.B = cls ? 0 : d->bins;
  g.ignore_index = d->ignore_index;
  // eight workgroups of four waves per CU of the hardware: what can be resident at once; more units than that are walked
  int grid = uz_grid_cap(g.units, 8);
  if (d->max_workgroups > 0 && grid > d->max_workgroups) grid = d->max_workgroups;
  p->grid = grid;
  if (cls) {
    p->off_hist = 0;
    p->bytes = uz_align16(4LL * g.M * g.K * g.K);
  } else {
    p->off_hist = uz_align16(16LL * g.M);
    p->bytes = p->off_hist + uz_align16(8LL * g.M * g.B);
  }
  p->clear_grid = uz_grid_cap(uz_cdiv(p->bytes / 16, CF_THREADS), 8);
  return UZ_OK;
}

}  // namespace

extern "C" long long uz_confusion_workspace_bytes(const uz_confusion_desc* d) {
  CfPlan p;
  if (cf_plan(d, "uz_confusion_workspace_bytes", &p) != UZ_OK) return -1;
  return p.bytes;
}

extern "C" int uz_confusion_grid(const uz_confusion_desc* d, int* units) {
  CfPlan p;
  const int rc = cf_plan(d, "uz_confusion_grid", &p);
  if (rc != UZ_OK) return rc;
  if (units) *units = p.geo.units;
  return p.grid;
}

extern "C" int uz_confusion_metrics(const uz_confusion_desc* d, const float* logits, const void* target, const float* edges, long long* counts,
                                    long long* hist, float* out, void* workspace, void* stream) {
  CfPlan p;
  const int rc = cf_plan(d, "uz_confusion_metrics", &p);
  if (rc != UZ_OK) return rc;
  const CfGeo& g = p.geo;
  const bool cls = d->mode == UZ_CONFUSION_CLASS;
  UZ_REQUIRE(logits && target && counts && out && workspace, "uz_confusion_metrics: null pointer");
  if (!cls) {
    UZ_REQUIRE(edges != nullptr, "uz_confusion_metrics: null edges in the binary mode");
    UZ_REQUIRE(hist != nullptr, "uz_confusion_metrics: null hist in the binary mode");
  }
  UZ_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)target & 3) == 0 && ((uintptr_t)out & 3) == 0 && (cls || ((uintptr_t)edges & 3) == 0),
             "uz_confusion_metrics: tensors must be 4-byte aligned");
  UZ_REQUIRE(((uintptr_t)counts & 7) == 0 && (cls || ((uintptr_t)hist & 7) == 0), "uz_confusion_metrics: counts and hist must be 8-byte aligned");
  UZ_REQUIRE(((uintptr_t)workspace & 15) == 0, "uz_confusion_metrics: the workspace must be 16-byte aligned");
  const long long px = (long long)d->N * d->H * d->W;
  const UzRange r[7] = {uz_range(logits, 4LL * px * d->C), uz_range(target, cls ? 4LL * px : 4LL * px * d->C),
                        uz_range(counts, cls ? 8LL * g.M * g.K * g.K : 32LL * g.M), uz_range(out, 32LL * d->N * g.P),
                        uz_range(workspace, p.bytes), uz_range(edges, 4LL * (g.B - 1)), uz_range(hist, 16LL * g.M * g.B)};
  UZ_REQUIRE(!uz_any_overlap(r, 7, nullptr, 0), "uz_confusion_metrics: tensors overlap");      // class mode: B = 0, edges and hist are empty
  int* wcnt = static_cast<int*>(workspace);
  int* whist = reinterpret_cast<int*>(static_cast<char*>(workspace) + p.off_hist);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(CF_THREADS);
  // the 16-byte path: every plane starts on a 16-byte boundary and holds whole quads
  const bool vec = g.HW % 4 == 0 && ((uintptr_t)logits & 15) == 0 && ((uintptr_t)target & 15) == 0;

  hipLaunchKernelGGL(confusion_clear_kernel, dim3((unsigned)p.clear_grid), block, 0, s, reinterpret_cast<int4*>(workspace), p.bytes / 16);
  UZ_LAUNCH_CHECK("uz_confusion_metrics(clear)");
  if (cls) {
    const int* y = static_cast<const int*>(target);
    if (vec) hipLaunchKernelGGL((confusion_class_kernel<true>), dim3((unsigned)p.grid), block, 0, s, g, logits, y, wcnt);
    else hipLaunchKernelGGL((confusion_class_kernel<false>), dim3((unsigned)p.grid), block, 0, s, g, logits, y, wcnt);
    UZ_LAUNCH_CHECK("uz_confusion_metrics(count)");
    hipLaunchKernelGGL(confusion_finalize_class_kernel, dim3((unsigned)g.M), block, 0, s, g, (const int*)wcnt, counts, out);
  } else {
    const float* t = static_cast<const float*>(target);
    if (vec) hipLaunchKernelGGL((confusion_binary_kernel<true>), dim3((unsigned)p.grid), block, 0, s, g, logits, t, edges, wcnt, whist);
    else hipLaunchKernelGGL((confusion_binary_kernel<false>), dim3((unsigned)p.grid), block, 0, s, g, logits, t, edges, wcnt, whist);
    UZ_LAUNCH_CHECK("uz_confusion_metrics(count)");
    hipLaunchKernelGGL(confusion_finalize_binary_kernel, dim3((unsigned)g.M), block, 0, s, g, (const int*)wcnt, (const int*)whist, counts, hist, out);
  }
  UZ_LAUNCH_CHECK("uz_confusion_metrics(finalize)");
  return UZ_OK;
}
