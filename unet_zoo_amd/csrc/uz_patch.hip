// Patch training from a pool of pictures that stays on the device: where the foreground is (once per pool), which patches
// to take (per step, from uniform draws) and the patches themselves.
//   uz_patch_index: mask -> index [M][P][H + 1] int32, the exclusive prefix over rows of each plane's per-row foreground count
//   uz_patch_draw : (B, 8) uniforms -> coords (B, 4) int32 [m, y0, x0, plane or -1], one wavefront per patch
//   uz_patch_cut  : coords -> image_out (B, C, h, w) fp32 and mask_out, plain copies (uint8 pictures: v * scale[c] + shift[c])
// Foreground plane p: an fp32 mask's channel p above 0.5, or label == p + 1.  The k-th foreground pixel of a plane in
// row-major order is found without a list of pixels: the row by a binary search of the index, the column by a ballot /
// popcount walk of that row in 64-pixel chunks.
#include "uz_common.h"

#include <math.h>

namespace {

constexpr int PATCH_THREADS = 256;
constexpr int PATCH_PX = 4;   // consecutive output pixels of one row per thread: one 16-byte store per plane
enum { MK_NONE = 0, MK_F32 = 1, MK_I32 = 2 };

// ---- index -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool patch_fg(int mask_kind, const void* row, int x, int p) {
  if (mask_kind == MK_F32) return static_cast<const float*>(row)[x] > 0.5f;
  return static_cast<const int*>(row)[x] == p + 1;
}

// row `y` of plane (m, p): channel p of an fp32 mask, the label map itself otherwise
__device__ __forceinline__ const void* patch_mask_row(int mask_kind, const void* mask, int Cm, int H, int W, int m, int p, int y) {
  if (mask_kind == MK_F32) return static_cast<const float*>(mask) + (((size_t)m * Cm + p) * H + y) * W;
  return static_cast<const int*>(mask) + ((size_t)m * H + y) * W;
}

// one wave per row of a plane: index[(m, p)][y] <- the row's foreground count (patch_scan_kernel turns them into the prefix)
__global__ __launch_bounds__(PATCH_THREADS) void patch_count_kernel(int mask_kind, int Cm, int P, int H, int W, long long rows,
                                                                    const void* __restrict__ mask, int* __restrict__ index) {
  const int lane = threadIdx.x & (UZ_WAVE - 1);
  const long long r = (long long)blockIdx.x * (PATCH_THREADS / UZ_WAVE) + threadIdx.x / UZ_WAVE;   // (m * P + p) * H + y
  if (r >= rows) return;   // a whole wave
  const long long mp = r / H;
  const int y = (int)(r - mp * H), m = (int)(mp / P), p = (int)(mp - (long long)m * P);
  const void* row = patch_mask_row(mask_kind, mask, Cm, H, W, m, p, y);
  int n = 0;
  for (int c0 = 0; c0 < W; c0 += UZ_WAVE) {
    const int x = c0 + lane;
    const bool fg = patch_fg(mask_kind, row, min(x, W - 1), p);   // the load is unconditional from a clamped address
    n += __popcll(__ballot(fg && x < W));
  }
  if (lane == 0) index[mp * (H + 1) + y] = n;
}

// one wave per plane: the H counts -> their exclusive prefix in place, entry H <- the plane's total
__global__ __launch_bounds__(UZ_WAVE) void patch_scan_kernel(int H, int* __restrict__ index) {
  const int lane = threadIdx.x;
  int* idx = index + (size_t)blockIdx.x * (H + 1);
  int base = 0;
  for (int y0 = 0; y0 < H; y0 += UZ_WAVE) {
    const int y = y0 + lane;
    const int n = y < H ? idx[y] : 0;
    int s = n;   // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < UZ_WAVE; d <<= 1) {
      const int t = __shfl_up(s, d);
      if (lane >= d) s += t;
    }
    if (y < H) idx[y] = base + s - n;
    base += __shfl(s, UZ_WAVE - 1);
  }
  if (lane == 0) idx[H] = base;
}

// ---- draw ------------------------------------------------------------------------------------------------------------------
struct PatchDraw {
  int M, H, W, mask_kind, Cm, P, h, w, use_indices;
  float pos, jitter;
};

// min(n - 1, floor(u * n)) with ONE float64 product: the restatement (tests/patch_ref.py) forms the same number.  (The lower
// clamp changes nothing for u in [0, 1); it keeps a draw that is not a uniform from naming something outside the pool.)
__device__ __forceinline__ int patch_pick(float u, int n) {
  const int k = (int)floor((double)u * (double)n);
  return max(0, min(n - 1, k));
}

// where in the patch the chosen pixel lands: min(n - 1, floor((0.5 + (u - 0.5) * jitter) * n)), every operation rounded on its
// own (no fused multiply-add: the restatement has none)
__device__ __forceinline__ int patch_anchor(float u, float jitter, int n) {
#pragma clang fp contract(off)
  const double t = ((double)u - 0.5) * (double)jitter;
  const double f = (0.5 + t) * (double)n;
  return max(0, min(n - 1, (int)floor(f)));
}

// one wave per patch; every lane carries the same scalars, the row walk is the only place where the lanes differ
__global__ __launch_bounds__(UZ_WAVE) void patch_draw_kernel(PatchDraw a, const float* __restrict__ u, const int* __restrict__ indices,
                                                              const int* __restrict__ index, const void* __restrict__ mask,
                                                              int* __restrict__ coords) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* ub = u + (size_t)b * 8;
  const float u0 = ub[0], u1 = ub[1], u2 = ub[2], u3 = ub[3], u4 = ub[4], u5 = ub[5];
  int* out = coords + (size_t)b * 4;
  int m;
  if (a.use_indices) {
    m = indices[b];
    if (m < 0 || m >= a.M) {   // uniform: the patch is cut as zeros, nothing of the pool is read for it
      if (lane == 0) out[0] = -1, out[1] = 0, out[2] = 0, out[3] = -1;
      return;
    }
  } else {
    m = patch_pick(u0, a.M);
  }
  int y0 = patch_pick(u4, a.H - a.h + 1), x0 = patch_pick(u5, a.W - a.w + 1), plane = -1;
  if (a.P > 0 && u1 < a.pos) {
    const int* idx_m = index + (size_t)m * a.P * (a.H + 1);
    int present = 0;   // bit p: plane p of this picture is not empty
    for (int p = 0; p < a.P; ++p) present |= (idx_m[(size_t)p * (a.H + 1) + a.H] > 0) << p;
    if (present) {
      int k = patch_pick(u2, __popc(present));
      int bits = present;
      for (; k > 0; --k) bits &= bits - 1;   // drop the k lowest set bits
      plane = __ffs(bits) - 1;
      const int* idx = idx_m + (size_t)plane * (a.H + 1);
      const int rank = patch_pick(u3, idx[a.H]);
      int lo = 0, hi = a.H - 1;   // the last row whose prefix is <= rank: it holds the pixel (its count is then > 0)
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (idx[mid] <= rank) lo = mid;
        else hi = mid - 1;
      }
      const int py = lo;
      int rem = rank - idx[py], px = 0;
      const void* row = patch_mask_row(a.mask_kind, mask, a.Cm, a.H, a.W, m, plane, py);
      for (int c0 = 0; c0 < a.W; c0 += UZ_WAVE) {
        const int x = c0 + lane;
        const bool fg = patch_fg(a.mask_kind, row, min(x, a.W - 1), plane) && x < a.W;
        const unsigned long long set = __ballot(fg);
        const int n = __popcll(set);
        if (rem < n) {   // uniform: the rem-th set bit is the lane whose bit is set with rem set bits below it
          const unsigned long long below = set & ((1ull << lane) - 1ull);
          const unsigned long long hit = __ballot(fg && __popcll(below) == rem);
          px = c0 + __ffsll((long long)hit) - 1;
          break;
        }
        rem -= n;
      }
      px = min(max(px, 0), a.W - 1);   // an index that does not belong to this mask finds no lane: still inside the picture
      const int ry = patch_anchor(u4, a.jitter, a.h), rx = patch_anchor(u5, a.jitter, a.w);
      y0 = min(max(py - ry, 0), a.H - a.h);
      x0 = min(max(px - rx, 0), a.W - a.w);
    }
  }
  if (lane == 0) out[0] = m, out[1] = y0, out[2] = x0, out[3] = plane;
}

// ---- cut -------------------------------------------------------------------------------------------------------------------
struct PatchShape {
  int M, H, W, B, h, w, Wq;   // Wq: runs of PATCH_PX pixels per patch row
  int ups;                    // units (PATCH_THREADS runs) per patch
  int units;                  // B * ups
  int Cm;
  int vec;                    // 16-byte stores: w % 4 == 0 and every output 16-byte aligned
};

template <typename T> __device__ __forceinline__ T patch_ld(const T* base, unsigned byte_off) {
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byte_off);
}

// four floats of one output row: one dwordx4 store, or the pixels inside the row one by one
__device__ __forceinline__ void patch_store4(float* __restrict__ row, int j0, int w, bool vec, bool live, const float (&v)[PATCH_PX]) {
  if (!live) return;
  if (vec) {
    *reinterpret_cast<float4*>(row + j0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < PATCH_PX; ++e)
      if (j0 + e < w) row[j0 + e] = v[e];
  }
}

// A workgroup takes units blockIdx.x, blockIdx.x + gridDim.x, ...; a unit is PATCH_THREADS runs of one patch, so the patch's
// coordinates are uniform over the workgroup (scalar loads).  Every load is unconditional from a clamped address and the zero
// of a patch without a picture (m = -1) is selected afterwards; a lane beyond the patch's last run computes run 0
// again and stores nothing.  The coordinates are clamped into the pool whatever they hold: nothing is read out of range.
template <int C, typename PIX, int MK>
__global__ __launch_bounds__(PATCH_THREADS) void patch_cut_kernel(PatchShape sh, const PIX* __restrict__ image, const void* __restrict__ mask,
                                                                   const int* __restrict__ coords, const float* __restrict__ norm,
                                                                   float* __restrict__ image_out, void* __restrict__ mask_out) {
  const int h = sh.h, w = sh.w;
  const size_t plane = (size_t)sh.H * sh.W, oplane = (size_t)h * w;
  for (int unit = blockIdx.x; unit < sh.units; unit += gridDim.x) {
    const int b = unit / sh.ups;
    const int* cb = coords + (size_t)b * 4;
    const int m_raw = cb[0];
    const bool have = m_raw >= 0 && m_raw < sh.M;
    const int m = have ? m_raw : 0;
    const int y0 = min(max(cb[1], 0), sh.H - h), x0 = min(max(cb[2], 0), sh.W - w);
    int item = (unit - b * sh.ups) * PATCH_THREADS + (int)threadIdx.x;
    const bool live = item < h * sh.Wq;
    item = live ? item : 0;
    const int i = item / sh.Wq, j0 = (item - i * sh.Wq) * PATCH_PX;
    unsigned off[PATCH_PX];   // element offsets inside a plane (H W < 2^30)
#pragma unroll
    for (int e = 0; e < PATCH_PX; ++e) off[e] = (unsigned)((y0 + i) * sh.W + x0 + min(j0 + e, w - 1));

    // every channel's run, and the first mask plane's, in flight together
    PIX t[C][PATCH_PX];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      const PIX* src = image + ((size_t)m * C + ch) * plane;
#pragma unroll
      for (int e = 0; e < PATCH_PX; ++e) t[ch][e] = patch_ld(src, (unsigned)sizeof(PIX) * off[e]);
    }
    float mf[PATCH_PX];
    int mi[PATCH_PX];
    if (MK == MK_F32) {
      const float* src = static_cast<const float*>(mask) + (size_t)m * sh.Cm * plane;
#pragma unroll
      for (int e = 0; e < PATCH_PX; ++e) mf[e] = patch_ld(src, 4u * off[e]);
    } else if (MK == MK_I32) {
      const int* src = static_cast<const int*>(mask) + (size_t)m * plane;
#pragma unroll
      for (int e = 0; e < PATCH_PX; ++e) mi[e] = patch_ld(src, 4u * off[e]);
    }
    // the values become opaque only here, after the last load is issued
    float tf[C][PATCH_PX];
#pragma unroll
    for (int ch = 0; ch < C; ++ch)
#pragma unroll
      for (int e = 0; e < PATCH_PX; ++e) {
        tf[ch][e] = (float)t[ch][e];   // exact for uint8, the value itself for fp32
        asm volatile("" : "+v"(tf[ch][e]));
      }
    if (MK == MK_F32) {
#pragma unroll
      for (int e = 0; e < PATCH_PX; ++e) asm volatile("" : "+v"(mf[e]));
    } else if (MK == MK_I32) {
#pragma unroll
      for (int e = 0; e < PATCH_PX; ++e) asm volatile("" : "+v"(mi[e]));
    }

    const size_t row = (size_t)i * w;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      float o[PATCH_PX];
      if (sizeof(PIX) == 1) {
        const float scale = norm ? norm[ch] : 1.f, shift = norm ? norm[C + ch] : 0.f;
#pragma unroll
        for (int e = 0; e < PATCH_PX; ++e) o[e] = have ? fmaf(tf[ch][e], scale, shift) : 0.f;
      } else {
#pragma unroll
        for (int e = 0; e < PATCH_PX; ++e) o[e] = have ? tf[ch][e] : 0.f;
      }
      patch_store4(image_out + ((size_t)b * C + ch) * oplane + row, j0, w, sh.vec, live, o);
    }
    if (MK == MK_I32) {
      int* dst = static_cast<int*>(mask_out) + (size_t)b * oplane + row;
      float o[PATCH_PX];
#pragma unroll
      for (int e = 0; e < PATCH_PX; ++e) o[e] = __int_as_float(have ? mi[e] : 0);   // moved as bits
      patch_store4(reinterpret_cast<float*>(dst), j0, w, sh.vec, live, o);
    } else if (MK == MK_F32) {
      const float* src = static_cast<const float*>(mask) + (size_t)m * sh.Cm * plane;
      float* dst = static_cast<float*>(mask_out) + (size_t)b * sh.Cm * oplane + row;
      for (int cm = 0;;) {
        float o[PATCH_PX];
#pragma unroll
        for (int e = 0; e < PATCH_PX; ++e) o[e] = have ? mf[e] : 0.f;
        patch_store4(dst + (size_t)cm * oplane, j0, w, sh.vec, live, o);
        if (++cm >= sh.Cm) break;
#pragma unroll
        for (int e = 0; e < PATCH_PX; ++e) mf[e] = patch_ld(src + (size_t)cm * plane, 4u * off[e]);
#pragma unroll
        for (int e = 0; e < PATCH_PX; ++e) asm volatile("" : "+v"(mf[e]));
      }
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
int patch_check(const uz_patch_desc* d, const char* who) {
  UZ_REQUIRE(d != nullptr, "%s: null descriptor", who);
  UZ_REQUIRE(d->M > 0 && d->H > 0 && d->W > 0, "%s: non-positive pool shape (M, H, W = %d, %d, %d)", who, d->M, d->H, d->W);
  UZ_REQUIRE(d->C >= 1 && d->C <= 4, "%s: C = %d outside 1..4", who, d->C);
  UZ_REQUIRE(d->image_kind == UZ_PATCH_IMAGE_F32 || d->image_kind == UZ_PATCH_IMAGE_U8, "%s: bad image_kind %d", who, d->image_kind);
  UZ_REQUIRE(d->mask_kind >= UZ_PATCH_MASK_NONE && d->mask_kind <= UZ_PATCH_MASK_I32, "%s: bad mask_kind %d", who, d->mask_kind);
  UZ_REQUIRE(d->mask_kind != UZ_PATCH_MASK_F32 || (d->Cm >= 1 && d->Cm <= 8), "%s: Cm = %d outside 1..8", who, d->Cm);
  UZ_REQUIRE(d->mask_kind != UZ_PATCH_MASK_F32 || d->P == d->Cm, "%s: P = %d, an fp32 mask has P = Cm = %d planes", who, d->P, d->Cm);
  UZ_REQUIRE(d->mask_kind != UZ_PATCH_MASK_I32 || (d->P >= 1 && d->P <= 8), "%s: P = %d outside 1..8 (num_classes - 1)", who, d->P);
  UZ_REQUIRE(d->mask_kind != UZ_PATCH_MASK_NONE || d->P == 0, "%s: P = %d without a mask", who, d->P);
  UZ_REQUIRE(d->B >= 1, "%s: B = %d, a batch has at least one patch", who, d->B);
  UZ_REQUIRE(d->h >= 1 && d->w >= 1, "%s: non-positive window (h, w = %d, %d)", who, d->h, d->w);
  UZ_REQUIRE(d->h <= d->H && d->w <= d->W, "%s: the window %d x %d is larger than the picture %d x %d (pad upstream)", who, d->h, d->w,
             d->H, d->W);
  UZ_REQUIRE(d->pos >= 0.f && d->pos <= 1.f, "%s: pos is a probability in [0, 1]", who);
  UZ_REQUIRE(d->jitter >= 0.f && d->jitter <= 1.f, "%s: jitter outside [0, 1]", who);
  UZ_REQUIRE((long long)d->H * d->W < (1LL << 30), "%s: too large (H W >= 2^30)", who);
  UZ_REQUIRE((long long)d->M * (d->P > 0 ? d->P : 1) * ((long long)d->H + 1) < (1LL << 31), "%s: too large (M P (H + 1) >= 2^31)", who);
  const int cmax = d->mask_kind == UZ_PATCH_MASK_F32 && d->Cm > d->C ? d->Cm : d->C;
  UZ_REQUIRE((long long)d->B * cmax * d->h * d->w < (1LL << 31), "%s: too large (B max(C, Cm) h w >= 2^31)", who);
  return UZ_OK;
}

long long patch_index_bytes(const uz_patch_desc* d) { return 4LL * d->M * d->P * ((long long)d->H + 1); }
long long patch_mask_bytes(const uz_patch_desc* d) {
  const long long px = (long long)d->M * d->H * d->W;
  return d->mask_kind == UZ_PATCH_MASK_NONE ? 0 : 4LL * px * (d->mask_kind == UZ_PATCH_MASK_F32 ? d->Cm : 1);
}

struct PatchPlan {
  PatchShape sh;
  int grid;
};

int patch_plan(const uz_patch_desc* d, const char* who, PatchPlan* p) {
  const int rc = patch_check(d, who);
  if (rc != UZ_OK) return rc;
  PatchShape& s = p->sh;
  s.M = d->M, s.H = d->H, s.W = d->W, s.B = d->B, s.h = d->h, s.w = d->w;
  s.Wq = (d->w + PATCH_PX - 1) / PATCH_PX;
  s.ups = uz_cdiv((long long)d->h * s.Wq, PATCH_THREADS);
  s.units = d->B * s.ups;
  s.Cm = d->mask_kind == UZ_PATCH_MASK_F32 ? d->Cm : 1;
  s.vec = 0;
  // eight workgroups of four waves per CU of the hardware: what can be resident at once; more units than that are walked
  p->grid = uz_grid_cap(s.units, 8);
  return UZ_OK;
}

template <int C, typename PIX>
void patch_launch(int mk, const PatchPlan& p, hipStream_t s, const void* image, const void* mask, const int* coords, const float* norm,
                  float* image_out, void* mask_out) {
  const dim3 grid(p.grid), block(PATCH_THREADS);
  const PIX* img = static_cast<const PIX*>(image);
  if (mk == MK_F32) hipLaunchKernelGGL((patch_cut_kernel<C, PIX, MK_F32>), grid, block, 0, s, p.sh, img, mask, coords, norm, image_out, mask_out);
  else if (mk == MK_I32) hipLaunchKernelGGL((patch_cut_kernel<C, PIX, MK_I32>), grid, block, 0, s, p.sh, img, mask, coords, norm, image_out, mask_out);
  else hipLaunchKernelGGL((patch_cut_kernel<C, PIX, MK_NONE>), grid, block, 0, s, p.sh, img, mask, coords, norm, image_out, mask_out);
}

template <typename PIX>
void patch_launch_c(int C, int mk, const PatchPlan& p, hipStream_t s, const void* image, const void* mask, const int* coords,
                    const float* norm, float* image_out, void* mask_out) {
  switch (C) {
    case 1: patch_launch<1, PIX>(mk, p, s, image, mask, coords, norm, image_out, mask_out); break;
    case 2: patch_launch<2, PIX>(mk, p, s, image, mask, coords, norm, image_out, mask_out); break;
    case 3: patch_launch<3, PIX>(mk, p, s, image, mask, coords, norm, image_out, mask_out); break;
    default: patch_launch<4, PIX>(mk, p, s, image, mask, coords, norm, image_out, mask_out); break;
  }
}

}  // namespace

extern "C" long long uz_patch_index_bytes(const uz_patch_desc* d) {
  const int rc = patch_check(d, "uz_patch_index_bytes");
  if (rc != UZ_OK) return rc;
  return patch_index_bytes(d);
}

extern "C" int uz_patch_index(const uz_patch_desc* d, const void* mask, int* index, void* stream) {
  const int rc = patch_check(d, "uz_patch_index");
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(d->mask_kind != UZ_PATCH_MASK_NONE, "uz_patch_index: mask_kind none has no foreground planes to index");
  UZ_REQUIRE(mask && index, "uz_patch_index: null pointer");
  UZ_REQUIRE(((uintptr_t)mask & 3) == 0 && ((uintptr_t)index & 3) == 0, "uz_patch_index: tensors must be 4-byte aligned");
  UZ_REQUIRE(!uz_overlap(uz_range(mask, patch_mask_bytes(d)), uz_range(index, patch_index_bytes(d))),
             "uz_patch_index: mask and index overlap");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long rows = (long long)d->M * d->P * d->H;   // < 2^31 (patch_check)
  const int wpb = PATCH_THREADS / UZ_WAVE;
  hipLaunchKernelGGL(patch_count_kernel, dim3((unsigned)((rows + wpb - 1) / wpb)), dim3(PATCH_THREADS), 0, s, d->mask_kind, d->Cm, d->P,
                     d->H, d->W, rows, mask, index);
  hipLaunchKernelGGL(patch_scan_kernel, dim3((unsigned)(d->M * d->P)), dim3(UZ_WAVE), 0, s, d->H, index);
  UZ_LAUNCH_CHECK("uz_patch_index");
  return UZ_OK;
}

extern "C" int uz_patch_draw(const uz_patch_desc* d, const float* u, const int* indices, const int* index, const void* mask, int* coords,
                             void* stream) {
  const int rc = patch_check(d, "uz_patch_draw");
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(u && coords, "uz_patch_draw: null pointer");
  UZ_REQUIRE(d->use_indices == 0 || d->use_indices == 1, "uz_patch_draw: use_indices = %d is not 0 or 1", d->use_indices);
  UZ_REQUIRE((d->use_indices != 0) == (indices != nullptr),
             "uz_patch_draw: indices does not match use_indices = %d (null pointer, or a pointer that would not be read)", d->use_indices);
  UZ_REQUIRE(d->mask_kind == UZ_PATCH_MASK_NONE ? (!mask && !index) : (mask && index),
             "uz_patch_draw: mask / index do not match mask_kind %d (null pointer, or a pointer without a mask)", d->mask_kind);
  UZ_REQUIRE(((uintptr_t)u & 3) == 0 && ((uintptr_t)indices & 3) == 0 && ((uintptr_t)index & 3) == 0 && ((uintptr_t)mask & 3) == 0 &&
                 ((uintptr_t)coords & 3) == 0,
             "uz_patch_draw: tensors must be 4-byte aligned");
  const UzRange out = uz_range(coords, 16LL * d->B);
  const UzRange in[4] = {uz_range(u, 32LL * d->B), uz_range(indices, 4LL * d->B), uz_range(index, patch_index_bytes(d)),
                         uz_range(mask, patch_mask_bytes(d))};
  UZ_REQUIRE(!uz_any_overlap(&out, 1, in, 4), "uz_patch_draw: coords overlap an input");
  PatchDraw a;
  a.M = d->M, a.H = d->H, a.W = d->W, a.mask_kind = d->mask_kind, a.Cm = d->Cm, a.P = d->P, a.h = d->h, a.w = d->w;
  a.use_indices = d->use_indices, a.pos = d->pos, a.jitter = d->jitter;
  hipLaunchKernelGGL(patch_draw_kernel, dim3((unsigned)d->B), dim3(UZ_WAVE), 0, static_cast<hipStream_t>(stream), a, u, indices, index,
                     mask, coords);
  UZ_LAUNCH_CHECK("uz_patch_draw");
  return UZ_OK;
}

extern "C" int uz_patch_cut_grid(const uz_patch_desc* d, int* units) {
  PatchPlan p;
  const int rc = patch_plan(d, "uz_patch_cut_grid", &p);
  if (rc != UZ_OK) return rc;
  if (units) *units = p.sh.units;
  return p.grid;
}

extern "C" int uz_patch_cut(const uz_patch_desc* d, const void* image, const void* mask, const int* coords, const float* norm,
                            float* image_out, void* mask_out, void* stream) {
  PatchPlan p;
  const int rc = patch_plan(d, "uz_patch_cut", &p);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(image && coords && image_out, "uz_patch_cut: null pointer");
  UZ_REQUIRE(d->mask_kind == UZ_PATCH_MASK_NONE ? (!mask && !mask_out) : (mask && mask_out),
             "uz_patch_cut: mask / mask_out do not match mask_kind %d (null pointer, or a pointer without a mask)", d->mask_kind);
  UZ_REQUIRE(d->image_kind == UZ_PATCH_IMAGE_U8 || !norm, "uz_patch_cut: norm goes with uint8 pictures only (image_kind %d)", d->image_kind);
  const int esz = d->image_kind == UZ_PATCH_IMAGE_U8 ? 1 : 4;
  UZ_REQUIRE(((uintptr_t)image & (esz - 1)) == 0 && ((uintptr_t)mask & 3) == 0 && ((uintptr_t)coords & 3) == 0 && ((uintptr_t)norm & 3) == 0 &&
                 ((uintptr_t)image_out & 3) == 0 && ((uintptr_t)mask_out & 3) == 0,
             "uz_patch_cut: tensors must be 4-byte aligned");
  const long long opx = (long long)d->B * d->h * d->w;
  const long long ombytes = d->mask_kind == UZ_PATCH_MASK_NONE ? 0 : 4LL * opx * p.sh.Cm;
  const UzRange in[4] = {uz_range(image, (long long)esz * d->M * d->C * d->H * d->W), uz_range(mask, patch_mask_bytes(d)),
                         uz_range(coords, 16LL * d->B), uz_range(norm, 8LL * d->C)};
  const UzRange out[2] = {uz_range(image_out, 4LL * opx * d->C), uz_range(mask_out, ombytes)};
  UZ_REQUIRE(!uz_any_overlap(&out[0], 1, in, 4) && !uz_any_overlap(&out[1], 1, in, 4), "uz_patch_cut: an output overlaps an input");
  UZ_REQUIRE(!uz_any_overlap(out, 2, nullptr, 0), "uz_patch_cut: the two outputs overlap");
  p.sh.vec = d->w % 4 == 0 && ((uintptr_t)image_out & 15) == 0 && ((uintptr_t)mask_out & 15) == 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d->image_kind == UZ_PATCH_IMAGE_U8) patch_launch_c<unsigned char>(d->C, d->mask_kind, p, s, image, mask, coords, norm, image_out, mask_out);
  else patch_launch_c<float>(d->C, d->mask_kind, p, s, image, mask, coords, norm, image_out, mask_out);
  UZ_LAUNCH_CHECK("uz_patch_cut");
  return UZ_OK;
}
