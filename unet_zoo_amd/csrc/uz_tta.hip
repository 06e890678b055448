// Flip test-time augmentation around a model, and the plain decision without post-processing.
//   uz_flip_views   the V flipped copies of an input batch, one launch
//   uz_tta_merge    prob = mean over the views of sigmoid (binary) or softmax over K (class) of the views' logits, each read
//                   through its inverse flip; fp32 arithmetic, the views summed in view order: no atomics, bit-reproducible
//   uz_mask_decide  mask / class_map of `x > thr` or argmax_K without any component step
// A view is a bit of {identity, hflip (along W), vflip (along H), hvflip}; the view order is the bit order.  A flip is its own
// inverse, so both directions are the same index map.
#include "uz_common.h"

namespace {

constexpr int TT_THREADS = 256;

struct TtViews {
  const void* src[4];
  void* dst[4];
  int fw[4], fh[4];   // flip along W / along H
  int V;
};

int tt_views(int bits, TtViews* v) {
  v->V = 0;
  for (int b = 0; b < 4; ++b)
    if (bits >> b & 1) {
      v->fw[v->V] = (b & 1) ? 1 : 0;    // hflip = 1, hvflip = 3
      v->fh[v->V] = (b & 2) ? 1 : 0;    // vflip = 2, hvflip = 3
      ++v->V;
    }
  for (int k = v->V; k < 4; ++k) v->fw[k] = v->fh[k] = 0, v->src[k] = nullptr, v->dst[k] = nullptr;
  return v->V;
}

__device__ __forceinline__ float tt_ld(const float* p, size_t i) { return p[i]; }
__device__ __forceinline__ float tt_ld(const bf16_t* p, size_t i) { return (float)p[i]; }

// one element of x per thread and step: V stores
__global__ __launch_bounds__(TT_THREADS) void tta_flip_kernel(TtViews vw, const float* __restrict__ x, long long total, int H, int W) {
  for (long long e = (long long)blockIdx.x * TT_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * TT_THREADS) {
    const float v = x[e];
    const int w = (int)(e % W), h = (int)(e / W % H);
    const long long row0 = e - w - (long long)h * W;      // the plane's first element
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < vw.V) {
        const int hh = vw.fh[k] ? H - 1 - h : h, ww = vw.fw[k] ? W - 1 - w : w;
        static_cast<float*>(vw.dst[k])[row0 + (long long)hh * W + ww] = v;
      }
  }
}

// one pixel of one image per thread and step
template <typename T, int MODE>
__global__ __launch_bounds__(TT_THREADS) void tta_merge_kernel(TtViews vw, float* __restrict__ prob, int N, int C, int H, int W) {
  const int HW = H * W;
  const long long total = MODE == UZ_POST_CLASS ? (long long)N * HW : (long long)N * C * HW;
  const float inv_scale = (float)vw.V;
  for (long long e = (long long)blockIdx.x * TT_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * TT_THREADS) {
    const int pix = (int)(e % HW);
    const long long img = e / HW;                          // image (class mode) or (image, channel) plane (binary mode)
    const int h = pix / W, w = pix - h * W;
    size_t at[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int hh = vw.fh[k] ? H - 1 - h : h, ww = vw.fw[k] ? W - 1 - w : w;
      at[k] = (size_t)img * (MODE == UZ_POST_CLASS ? (size_t)C * HW : (size_t)HW) + (size_t)hh * W + ww;
    }
    if (MODE == UZ_POST_BINARY) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < vw.V) acc += 1.f / (1.f + expf(-tt_ld(static_cast<const T*>(vw.src[k]), at[k])));
      prob[e] = acc / inv_scale;
    } else {
      float mx[4], den[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        mx[k] = 0.f, den[k] = 1.f;
        if (k < vw.V) {
          const T* __restrict__ s = static_cast<const T*>(vw.src[k]);
          float m = tt_ld(s, at[k]);
          for (int c = 1; c < C; ++c) m = fmaxf(m, tt_ld(s, at[k] + (size_t)c * HW));
          float d = 0.f;
          for (int c = 0; c < C; ++c) d += expf(tt_ld(s, at[k] + (size_t)c * HW) - m);
          mx[k] = m, den[k] = d;
        }
      }
      for (int c = 0; c < C; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < vw.V) acc += expf(tt_ld(static_cast<const T*>(vw.src[k]), at[k] + (size_t)c * HW) - mx[k]) / den[k];
        prob[(size_t)img * C * HW + (size_t)c * HW + pix] = acc / inv_scale;
      }
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(TT_THREADS) void tta_decide_kernel(const float* __restrict__ x, unsigned char* __restrict__ mask,
                                                                unsigned char* __restrict__ cmap, int N, int C, int HW, int first, float thr) {
  const long long total = MODE == UZ_POST_CLASS ? (long long)N * HW : (long long)N * C * HW;
  for (long long e = (long long)blockIdx.x * TT_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * TT_THREADS) {
    if (MODE == UZ_POST_BINARY) {
      mask[e] = x[e] > thr ? 1 : 0;
    } else {
      const long long n = e / HW;
      const int pix = (int)(e - n * HW);
      const float* __restrict__ xp = x + (size_t)n * C * HW + pix;
      float best = xp[0];
      int code = 0;
      for (int c = 1; c < C; ++c) {
        const float v = xp[(size_t)c * HW];
        const bool up = v > best;          // ties: the lowest index
        best = up ? v : best;
        code = up ? c : code;
      }
      for (int c = first; c < C; ++c) mask[((size_t)n * (C - first) + (c - first)) * HW + pix] = c == code ? 1 : 0;
      if (cmap) cmap[e] = (unsigned char)code;
    }
  }
}

int tt_check(const uz_tta_desc* d, const char* who) {
  UZ_REQUIRE(d != nullptr, "%s: null descriptor", who);
  UZ_REQUIRE(d->mode == UZ_POST_BINARY || d->mode == UZ_POST_CLASS, "%s: unknown mode %d", who, d->mode);
  UZ_REQUIRE(d->N >= 1 && d->C >= 1 && d->H >= 1 && d->W >= 1, "%s: non-positive shape", who);
  if (d->mode == UZ_POST_CLASS) UZ_REQUIRE(d->C >= 2 && d->C <= UZ_CLASS_MAX_K, "%s: K = %d outside [2, %d]", who, d->C, UZ_CLASS_MAX_K);
  UZ_REQUIRE(d->views >= 1 && d->views <= 15, "%s: views = %d is no non-empty subset of the four flips", who, d->views);
  UZ_REQUIRE(d->dtype == UZ_F32 || d->dtype == UZ_BF16, "%s: unknown dtype %d", who, d->dtype);
  UZ_REQUIRE((long long)d->N * d->C * d->H * d->W < (1LL << 31), "%s: too large (N C H W >= 2^31)", who);
  return UZ_OK;
}

unsigned tt_grid(long long total) { return (unsigned)uz_grid_cap((total + TT_THREADS - 1) / TT_THREADS, 8); }

}  // namespace

extern "C" int uz_tta_num_views(int views) {
  TtViews v;
  return (views >= 1 && views <= 15) ? tt_views(views, &v) : -1;
}

extern "C" int uz_flip_views(const uz_tta_desc* d, const float* x, float* const* out, void* stream) {
  const int rc = tt_check(d, "uz_flip_views");
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(x && out, "uz_flip_views: null pointer");
  TtViews v;
  tt_views(d->views, &v);
  const long long total = (long long)d->N * d->C * d->H * d->W;
  for (int k = 0; k < v.V; ++k) {
    UZ_REQUIRE(out[k] != nullptr && ((uintptr_t)out[k] & 3) == 0, "uz_flip_views: view %d is null or misaligned", k);
    const UzRange view = uz_range(out[k], 4 * total);
    UZ_REQUIRE(!uz_overlap(view, uz_range(x, 4 * total)), "uz_flip_views: view %d overlaps the input", k);
    for (int j = 0; j < k; ++j) UZ_REQUIRE(!uz_overlap(view, uz_range(out[j], 4 * total)), "uz_flip_views: views %d and %d overlap", j, k);
    v.dst[k] = out[k];
  }
  hipLaunchKernelGGL(tta_flip_kernel, dim3(tt_grid(total)), dim3(TT_THREADS), 0, static_cast<hipStream_t>(stream), v, x, total, d->H, d->W);
  UZ_LAUNCH_CHECK("uz_flip_views");
  return UZ_OK;
}

extern "C" int uz_tta_merge(const uz_tta_desc* d, const void* const* logits, float* prob, void* stream) {
  const int rc = tt_check(d, "uz_tta_merge");
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(logits && prob, "uz_tta_merge: null pointer");
  TtViews v;
  tt_views(d->views, &v);
  const long long total = (long long)d->N * d->C * d->H * d->W, esz = d->dtype == UZ_F32 ? 4 : 2;
  for (int k = 0; k < v.V; ++k) {
    UZ_REQUIRE(logits[k] != nullptr && ((uintptr_t)logits[k] & (esz - 1)) == 0, "uz_tta_merge: view %d is null or misaligned", k);
    UZ_REQUIRE(!uz_overlap(uz_range(logits[k], esz * total), uz_range(prob, 4 * total)), "uz_tta_merge: view %d overlaps prob", k);
    v.src[k] = logits[k];
  }
  const bool cls = d->mode == UZ_POST_CLASS;
  const long long items = cls ? (long long)d->N * d->H * d->W : total;
  const dim3 grid(tt_grid(items)), block(TT_THREADS);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d->dtype == UZ_F32) {
    if (cls) hipLaunchKernelGGL((tta_merge_kernel<float, UZ_POST_CLASS>), grid, block, 0, s, v, prob, d->N, d->C, d->H, d->W);
    else hipLaunchKernelGGL((tta_merge_kernel<float, UZ_POST_BINARY>), grid, block, 0, s, v, prob, d->N, d->C, d->H, d->W);
  } else {
    if (cls) hipLaunchKernelGGL((tta_merge_kernel<bf16_t, UZ_POST_CLASS>), grid, block, 0, s, v, prob, d->N, d->C, d->H, d->W);
    else hipLaunchKernelGGL((tta_merge_kernel<bf16_t, UZ_POST_BINARY>), grid, block, 0, s, v, prob, d->N, d->C, d->H, d->W);
  }
  UZ_LAUNCH_CHECK("uz_tta_merge");
  return UZ_OK;
}

extern "C" int uz_mask_decide(const uz_tta_desc* d, const float* x, float thr, int first_class, unsigned char* mask, unsigned char* class_map,
                              void* stream) {
  const int rc = tt_check(d, "uz_mask_decide");
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(x && mask, "uz_mask_decide: null pointer");
  UZ_REQUIRE(thr == thr, "uz_mask_decide: thr is not a number");
  const bool cls = d->mode == UZ_POST_CLASS;
  UZ_REQUIRE(class_map == nullptr || cls, "uz_mask_decide: class_map belongs to the class mode");
  if (cls) UZ_REQUIRE(first_class >= 0 && first_class < d->C, "uz_mask_decide: first_class = %d outside [0, %d)", first_class, d->C);
  const int HW = d->H * d->W;
  const long long items = cls ? (long long)d->N * HW : (long long)d->N * d->C * HW;
  const dim3 grid(tt_grid(items)), block(TT_THREADS);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (cls) hipLaunchKernelGGL((tta_decide_kernel<UZ_POST_CLASS>), grid, block, 0, s, x, mask, class_map, d->N, d->C, HW, first_class, thr);
  else hipLaunchKernelGGL((tta_decide_kernel<UZ_POST_BINARY>), grid, block, 0, s, x, mask, class_map, d->N, d->C, HW, 0, thr);
  UZ_LAUNCH_CHECK("uz_mask_decide");
  return UZ_OK;
}
