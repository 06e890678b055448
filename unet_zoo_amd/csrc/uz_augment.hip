// Training-time augmentation on the device: a per-sample affine warp (flips, rotation, scaling, translation), an optional
// smooth displacement grid and an intensity jitter, applied to the picture and its mask in ONE launch.
//   uz_augment_params: (N, 8) uniforms -> (N, 16) per-sample parameters (the inverse map and the jitter), one tiny launch
//   uz_augment_apply : picture (bilinear, fill outside, then contrast * v + brightness) and mask / labels (nearest, fill outside)
// Coordinates: output pixel (i, j) has u = j + 0.5 - W/2, v = i + 0.5 - H/2 and reads the source at
//   sx = a u + b v + ox + Dx(i, j),  sy = c u + d v + oy + Dy(i, j)        (pixel-index coordinates: sx = 3 IS column 3)
// D = the (2, G, G) displacement grid of the sample interpolated bilinearly with align_corners = True.
#include "uz_common.h"

#include <math.h>

namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_PX = 4;   // consecutive output pixels of one row per thread: one 16-byte store per plane
// A unit is AUG_THREADS consecutive runs of a sample in row-major order: a wave writes 1 KB of one output row.  (Measured
// against 16-row x 64-pixel tiles with a wave on a 16 x 16 patch, which keeps the SOURCE footprint of a load compact under a
// rotation: 27.0 .. 27.3 us against 19.6 .. 20.7 us at 16 x 3 x 256 x 256 on one GPU, alternating -- the stores in 64-byte
// pieces cost more than the gathers gain; profiles/augment_256_b16.txt.)

struct AugRanges {
  float p_hflip, p_vflip, rotate, scale_min, scale_max, translate, brightness, contrast;
};

__global__ void augment_params_kernel(AugRanges r, int N, int H, int W, const float* __restrict__ u, float* __restrict__ params) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  double q[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) q[k] = (double)u[(size_t)n * 8 + k];
  // the arithmetic is float64 and rounded once: the map's entries are then the float32 neighbours of the exact ones
  const double fx = u[(size_t)n * 8 + 0] < r.p_hflip ? -1.0 : 1.0;
  const double fy = u[(size_t)n * 8 + 1] < r.p_vflip ? -1.0 : 1.0;
  const double theta = (2.0 * q[2] - 1.0) * (double)r.rotate * (M_PI / 180.0);
  const double s = (double)r.scale_min + q[3] * ((double)r.scale_max - (double)r.scale_min);
  const double tx = (2.0 * q[4] - 1.0) * (double)r.translate * (double)W;
  const double ty = (2.0 * q[5] - 1.0) * (double)r.translate * (double)H;
  const double cs = cos(theta), sn = sin(theta);
  float* p = params + (size_t)n * 16;
  p[0] = (float)(cs * fx / s);
  p[1] = (float)(sn * fy / s);
  p[2] = (float)(0.5 * W + tx - 0.5);
  p[3] = (float)(-sn * fx / s);
  p[4] = (float)(cs * fy / s);
  p[5] = (float)(0.5 * H + ty - 0.5);
  p[6] = (float)(1.0 + (2.0 * q[7] - 1.0) * (double)r.contrast);
  p[7] = (float)((2.0 * q[6] - 1.0) * (double)r.brightness);
#pragma unroll
  for (int k = 8; k < 16; ++k) p[k] = 0.f;
}

enum { MK_NONE = 0, MK_F32 = 1, MK_I32 = 2 };

struct AugShape {
  int N, H, W, Wq;   // Wq: runs of AUG_PX pixels per row
  int ups;           // units (AUG_THREADS runs) per sample
  int units;         // N * ups
  int Cm, G;
  int vec;           // 16-byte stores: W % 4 == 0 and every output 16-byte aligned
  float gsx, gsy;    // (G - 1) / (W - 1), (G - 1) / (H - 1)
  float image_fill, mask_fill;
  int label_fill;
};

// base[byte_off / 4] with a 32-bit unsigned byte offset: the load takes the plane's base from scalar registers and the offset
// from one vector register.  A signed element index costs a 64-bit shift-add per load (85 in the 3-channel kernel, 22 more
// registers); the time is the same within the run-to-run spread (18 .. 22 us either way), the leaner form is kept.
template <typename T> __device__ __forceinline__ T aug_ld(const T* base, unsigned byte_off) {
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byte_off);
}

// four floats of one output row: one dwordx4 store, or the pixels inside the row one by one
__device__ __forceinline__ void aug_store4(float* __restrict__ row, int j0, int W, bool vec, bool live, const float (&v)[AUG_PX]) {
  if (!live) return;
  if (vec) {
    *reinterpret_cast<float4*>(row + j0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < AUG_PX; ++e)
      if (j0 + e < W) row[j0 + e] = v[e];
  }
}

// A workgroup takes units blockIdx.x, blockIdx.x + gridDim.x, ...; a unit is AUG_THREADS runs of one sample, so the sample's
// parameters are uniform over the workgroup (scalar loads).  Every load is unconditional from a clamped address and the fill
// is selected afterwards; a lane beyond the sample's last run computes run 0 again and stores nothing.
template <int C, int MK>
__global__ __launch_bounds__(AUG_THREADS) void augment_apply_kernel(
    AugShape sh, const float* __restrict__ image, const void* __restrict__ mask, const float* __restrict__ params,
    const float* __restrict__ disp, float* __restrict__ image_out, void* __restrict__ mask_out) {
  const int H = sh.H, W = sh.W;
  const size_t plane = (size_t)H * W;
  for (int unit = blockIdx.x; unit < sh.units; unit += gridDim.x) {
    const int n = unit / sh.ups;
    const float* pp = params + (size_t)n * 16;
    const float a = pp[0], b = pp[1], ox = pp[2], c = pp[3], d = pp[4], oy = pp[5], contrast = pp[6], brightness = pp[7];
    int item = (unit - n * sh.ups) * AUG_THREADS + (int)threadIdx.x;
    const bool live = item < H * sh.Wq;
    item = live ? item : 0;
    const int i = item / sh.Wq, j0 = (item - i * sh.Wq) * AUG_PX;
    const float v = (float)i + 0.5f - 0.5f * (float)H;

    float dx[AUG_PX], dy[AUG_PX];
#pragma unroll
    for (int e = 0; e < AUG_PX; ++e) dx[e] = dy[e] = 0.f;
    if (sh.G > 0) {   // uniform; the taps need these values, so the wait that closes the block is the one they need anyway
      const int G = sh.G;
      const float* gx_plane = disp + (size_t)n * 2 * G * G;
      const float* gy_plane = gx_plane + G * G;
      const float gy = (float)i * sh.gsy;
      const int y0 = min((int)gy, G - 2);
      const float ty = gy - (float)y0;
      float t[AUG_PX][2][4];
      float tx[AUG_PX];
#pragma unroll
      for (int e = 0; e < AUG_PX; ++e) {
        const float gx = (float)min(j0 + e, W - 1) * sh.gsx;
        const int x0 = min((int)gx, G - 2);
        tx[e] = gx - (float)x0;
        const int o = y0 * G + x0;
        t[e][0][0] = gx_plane[o], t[e][0][1] = gx_plane[o + 1], t[e][0][2] = gx_plane[o + G], t[e][0][3] = gx_plane[o + G + 1];
        t[e][1][0] = gy_plane[o], t[e][1][1] = gy_plane[o + 1], t[e][1][2] = gy_plane[o + G], t[e][1][3] = gy_plane[o + G + 1];
      }
#pragma unroll
      for (int e = 0; e < AUG_PX; ++e) {
        const float wx1 = tx[e], wx0 = 1.f - tx[e];
        dx[e] = (1.f - ty) * (wx0 * t[e][0][0] + wx1 * t[e][0][1]) + ty * (wx0 * t[e][0][2] + wx1 * t[e][0][3]);
        dy[e] = (1.f - ty) * (wx0 * t[e][1][0] + wx1 * t[e][1][1]) + ty * (wx0 * t[e][1][2] + wx1 * t[e][1][3]);
      }
    }

    // source coordinates, tap offsets inside a plane (clamped) and which taps lie inside the picture
    float fx[AUG_PX], fy[AUG_PX];
    unsigned o00[AUG_PX], o01[AUG_PX], o10[AUG_PX], o11[AUG_PX], om[AUG_PX];   // byte offsets inside a plane (H W < 2^30)
    int in[AUG_PX];   // bit 0..3: tap 00, 01, 10, 11 inside the picture; bit 4: the nearest pixel inside (bits, not lane masks: 20 masks spill the SGPRs)
#pragma unroll
    for (int e = 0; e < AUG_PX; ++e) {
      const float u = (float)(j0 + e) + 0.5f - 0.5f * (float)W;
      const float sx = fmaf(a, u, fmaf(b, v, ox)) + dx[e];
      const float sy = fmaf(c, u, fmaf(d, v, oy)) + dy[e];
      // far outside is outside: the clamp keeps the float -> int conversion in range and changes no tap of the picture
      const float sxc = fminf(fmaxf(sx, -2.f), (float)W + 1.f), syc = fminf(fmaxf(sy, -2.f), (float)H + 1.f);
      const float flx = floorf(sxc), fly = floorf(syc);
      fx[e] = sxc - flx, fy[e] = syc - fly;
      const int x0 = (int)flx, y0 = (int)fly;
      const int inx0 = x0 >= 0 && x0 < W, inx1 = x0 + 1 >= 0 && x0 + 1 < W;
      const int iny0 = y0 >= 0 && y0 < H, iny1 = y0 + 1 >= 0 && y0 + 1 < H;
      const int xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1);
      const int ya = min(max(y0, 0), H - 1), yb = min(max(y0 + 1, 0), H - 1);
      o00[e] = 4u * (unsigned)(ya * W + xa), o01[e] = 4u * (unsigned)(ya * W + xb);
      o10[e] = 4u * (unsigned)(yb * W + xa), o11[e] = 4u * (unsigned)(yb * W + xb);
      const int xm = (int)floorf(sxc + 0.5f), ym = (int)floorf(syc + 0.5f);
      in[e] = (inx0 & iny0) | (inx1 & iny0) << 1 | (inx0 & iny1) << 2 | (inx1 & iny1) << 3 | (xm >= 0 && xm < W && ym >= 0 && ym < H) << 4;
      om[e] = 4u * (unsigned)(min(max(ym, 0), H - 1) * W + min(max(xm, 0), W - 1));
    }

    // every tap of every channel, and the first mask plane, in flight together
    float t[C][AUG_PX][4];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      const float* src = image + ((size_t)n * C + ch) * plane;
#pragma unroll
      for (int e = 0; e < AUG_PX; ++e)
        t[ch][e][0] = aug_ld(src, o00[e]), t[ch][e][1] = aug_ld(src, o01[e]), t[ch][e][2] = aug_ld(src, o10[e]), t[ch][e][3] = aug_ld(src, o11[e]);
    }
    float mf[AUG_PX];
    int mi[AUG_PX];
    if (MK == MK_F32) {
      const float* src = static_cast<const float*>(mask) + (size_t)n * sh.Cm * plane;
#pragma unroll
      for (int e = 0; e < AUG_PX; ++e) mf[e] = aug_ld(src, om[e]);
    } else if (MK == MK_I32) {
      const int* src = static_cast<const int*>(mask) + (size_t)n * plane;
#pragma unroll
      for (int e = 0; e < AUG_PX; ++e) mi[e] = aug_ld(src, om[e]);
    }
    // the values become opaque only here, after the last load is issued: a select next to its load turns into a branch around
    // it, and the block is closed by a wait
#pragma unroll
    for (int ch = 0; ch < C; ++ch)
#pragma unroll
      for (int e = 0; e < AUG_PX; ++e)
#pragma unroll
        for (int k = 0; k < 4; ++k) asm volatile("" : "+v"(t[ch][e][k]));
    if (MK == MK_F32) {
#pragma unroll
      for (int e = 0; e < AUG_PX; ++e) asm volatile("" : "+v"(mf[e]));
    } else if (MK == MK_I32) {
#pragma unroll
      for (int e = 0; e < AUG_PX; ++e) asm volatile("" : "+v"(mi[e]));
    }

    const size_t row = (size_t)i * W;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      float o[AUG_PX];
#pragma unroll
      for (int e = 0; e < AUG_PX; ++e) {
        const float fill = sh.image_fill;
        const float v00 = in[e] & 1 ? t[ch][e][0] : fill, v01 = in[e] & 2 ? t[ch][e][1] : fill;
        const float v10 = in[e] & 4 ? t[ch][e][2] : fill, v11 = in[e] & 8 ? t[ch][e][3] : fill;
        const float wx1 = fx[e], wx0 = 1.f - fx[e];
        const float val = (1.f - fy[e]) * (wx0 * v00 + wx1 * v01) + fy[e] * (wx0 * v10 + wx1 * v11);
        o[e] = contrast * val + brightness;
      }
      aug_store4(image_out + ((size_t)n * C + ch) * plane + row, j0, W, sh.vec, live, o);
    }
    if (MK == MK_I32) {
      int* dst = static_cast<int*>(mask_out) + (size_t)n * plane + row;
      float o[AUG_PX];
#pragma unroll
      for (int e = 0; e < AUG_PX; ++e) o[e] = __int_as_float(in[e] & 16 ? mi[e] : sh.label_fill);   // moved as bits
      aug_store4(reinterpret_cast<float*>(dst), j0, W, sh.vec, live, o);
    } else if (MK == MK_F32) {
      const float* src = static_cast<const float*>(mask) + (size_t)n * sh.Cm * plane;
      float* dst = static_cast<float*>(mask_out) + (size_t)n * sh.Cm * plane + row;
      for (int cm = 0;;) {
        float o[AUG_PX];
#pragma unroll
        for (int e = 0; e < AUG_PX; ++e) o[e] = in[e] & 16 ? mf[e] : sh.mask_fill;
        aug_store4(dst + (size_t)cm * plane, j0, W, sh.vec, live, o);
        if (++cm >= sh.Cm) break;
#pragma unroll
        for (int e = 0; e < AUG_PX; ++e) mf[e] = aug_ld(src + (size_t)cm * plane, om[e]);
#pragma unroll
        for (int e = 0; e < AUG_PX; ++e) asm volatile("" : "+v"(mf[e]));
      }
    }
  }
}

int aug_check_ranges(const uz_augment_desc* d, const char* who) {
  UZ_REQUIRE(d != nullptr, "%s: null descriptor", who);
  UZ_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0, "%s: non-positive shape", who);
  UZ_REQUIRE(d->p_hflip >= 0.f && d->p_hflip <= 1.f && d->p_vflip >= 0.f && d->p_vflip <= 1.f, "%s: flip probability outside [0, 1]", who);
  UZ_REQUIRE(d->scale_min > 0.f && d->scale_min <= d->scale_max && isfinite(d->scale_max), "%s: scale needs 0 < min <= max", who);
  UZ_REQUIRE(d->rotate >= 0.f && d->translate >= 0.f && d->brightness >= 0.f && d->contrast >= 0.f && isfinite(d->rotate) &&
                 isfinite(d->translate) && isfinite(d->brightness) && isfinite(d->contrast),
             "%s: negative or non-finite range", who);
  return UZ_OK;
}

struct AugPlan {
  AugShape sh;
  int grid;
};

int aug_plan(const uz_augment_desc* d, const char* who, AugPlan* p) {
  UZ_REQUIRE(d != nullptr, "%s: null descriptor", who);
  UZ_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0, "%s: non-positive shape", who);
  UZ_REQUIRE(d->C >= 1 && d->C <= 4, "%s: C = %d outside 1..4", who, d->C);
  UZ_REQUIRE(d->mask_kind >= UZ_AUGMENT_MASK_NONE && d->mask_kind <= UZ_AUGMENT_MASK_I32, "%s: bad mask_kind %d", who, d->mask_kind);
  UZ_REQUIRE(d->mask_kind != UZ_AUGMENT_MASK_F32 || (d->Cm >= 1 && d->Cm <= 8), "%s: Cm = %d outside 1..8", who, d->Cm);
  UZ_REQUIRE(d->G == 0 || (d->G >= 2 && d->G <= 16), "%s: G = %d outside 2..16 (0: no displacement grid)", who, d->G);
  UZ_REQUIRE(d->G == 0 || (d->H >= 2 && d->W >= 2), "%s: a displacement grid needs H, W >= 2", who);
  UZ_REQUIRE(isfinite(d->image_fill) && isfinite(d->mask_fill), "%s: non-finite fill", who);
  const int cmax = d->mask_kind == UZ_AUGMENT_MASK_F32 && d->Cm > d->C ? d->Cm : d->C;
  UZ_REQUIRE((long long)d->N * cmax * d->H * d->W < (1LL << 31), "%s: too large (N max(C, Cm) H W >= 2^31)", who);
  UZ_REQUIRE((long long)d->H * d->W < (1LL << 30), "%s: too large (H W >= 2^30)", who);
  AugShape& s = p->sh;
  s.N = d->N, s.H = d->H, s.W = d->W;
  s.Wq = (d->W + AUG_PX - 1) / AUG_PX;
  s.ups = uz_cdiv((long long)d->H * s.Wq, AUG_THREADS);
  s.units = d->N * s.ups;
  s.Cm = d->mask_kind == UZ_AUGMENT_MASK_F32 ? d->Cm : 1;
  s.G = d->G;
  s.vec = 0;
  s.gsx = d->G ? (float)((double)(d->G - 1) / (double)(d->W - 1)) : 0.f;
  s.gsy = d->G ? (float)((double)(d->G - 1) / (double)(d->H - 1)) : 0.f;
  s.image_fill = d->image_fill, s.mask_fill = d->mask_fill, s.label_fill = d->label_fill;
  // eight workgroups of four waves per CU of the hardware: what can be resident at once; more units than that are walked
  p->grid = uz_grid_cap(s.units, 8);
  return UZ_OK;
}

template <int C>
void aug_launch(int mk, const AugPlan& p, hipStream_t s, const float* image, const void* mask, const float* params, const float* disp,
                float* image_out, void* mask_out) {
  const dim3 grid(p.grid), block(AUG_THREADS);
  if (mk == MK_F32) hipLaunchKernelGGL((augment_apply_kernel<C, MK_F32>), grid, block, 0, s, p.sh, image, mask, params, disp, image_out, mask_out);
  else if (mk == MK_I32) hipLaunchKernelGGL((augment_apply_kernel<C, MK_I32>), grid, block, 0, s, p.sh, image, mask, params, disp, image_out, mask_out);
  else hipLaunchKernelGGL((augment_apply_kernel<C, MK_NONE>), grid, block, 0, s, p.sh, image, mask, params, disp, image_out, mask_out);
}

}  // namespace

extern "C" int uz_augment_params(const uz_augment_desc* d, const float* u, float* params, void* stream) {
  const int rc = aug_check_ranges(d, "uz_augment_params");
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(u && params, "uz_augment_params: null pointer");
  UZ_REQUIRE(!uz_overlap(uz_range(u, 32LL * d->N), uz_range(params, 64LL * d->N)), "uz_augment_params: u and params overlap");
  AugRanges r;
  r.p_hflip = d->p_hflip, r.p_vflip = d->p_vflip, r.rotate = d->rotate, r.scale_min = d->scale_min, r.scale_max = d->scale_max;
  r.translate = d->translate, r.brightness = d->brightness, r.contrast = d->contrast;
  hipLaunchKernelGGL(augment_params_kernel, dim3((unsigned)((d->N + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream), r, d->N,
                     d->H, d->W, u, params);
  UZ_LAUNCH_CHECK("uz_augment_params");
  return UZ_OK;
}

extern "C" int uz_augment_grid(const uz_augment_desc* d, int* units) {
  AugPlan p;
  const int rc = aug_plan(d, "uz_augment_grid", &p);
  if (rc != UZ_OK) return rc;
  if (units) *units = p.sh.units;
  return p.grid;
}

extern "C" int uz_augment_apply(const uz_augment_desc* d, const float* image, const void* mask, const float* params, const float* disp,
                                float* image_out, void* mask_out, void* stream) {
  AugPlan p;
  const int rc = aug_plan(d, "uz_augment_apply", &p);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(image && params && image_out, "uz_augment_apply: null pointer");
  UZ_REQUIRE(d->mask_kind == UZ_AUGMENT_MASK_NONE ? (!mask && !mask_out) : (mask && mask_out),
             "uz_augment_apply: mask / mask_out do not match mask_kind %d (null pointer, or a pointer without a mask)", d->mask_kind);
  UZ_REQUIRE((d->G > 0) == (disp != nullptr), "uz_augment_apply: the displacement grid does not match G = %d (null pointer, or a pointer with G = 0)", d->G);
  const long long px = (long long)d->N * d->H * d->W;
  const long long mbytes = d->mask_kind == UZ_AUGMENT_MASK_NONE ? 0 : 4LL * px * p.sh.Cm;
  const UzRange in[4] = {uz_range(image, 4LL * px * d->C), uz_range(mask, mbytes), uz_range(params, 64LL * d->N),
                         uz_range(disp, 8LL * d->N * d->G * d->G)};
  const UzRange out[2] = {uz_range(image_out, 4LL * px * d->C), uz_range(mask_out, mbytes)};
  UZ_REQUIRE(!uz_any_overlap(&out[0], 1, in, 4) && !uz_any_overlap(&out[1], 1, in, 4),
             "uz_augment_apply: an output overlaps an input (the warp cannot run in place)");
  UZ_REQUIRE(!uz_any_overlap(out, 2, nullptr, 0), "uz_augment_apply: the two outputs overlap");
  UZ_REQUIRE(((uintptr_t)image & 3) == 0 && ((uintptr_t)mask & 3) == 0 && ((uintptr_t)params & 3) == 0 && ((uintptr_t)disp & 3) == 0 &&
                 ((uintptr_t)image_out & 3) == 0 && ((uintptr_t)mask_out & 3) == 0,
             "uz_augment_apply: tensors must be 4-byte aligned");
  p.sh.vec = d->W % 4 == 0 && ((uintptr_t)image_out & 15) == 0 && ((uintptr_t)mask_out & 15) == 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (d->C) {
    case 1: aug_launch<1>(d->mask_kind, p, s, image, mask, params, disp, image_out, mask_out); break;
    case 2: aug_launch<2>(d->mask_kind, p, s, image, mask, params, disp, image_out, mask_out); break;
    case 3: aug_launch<3>(d->mask_kind, p, s, image, mask, params, disp, image_out, mask_out); break;
    default: aug_launch<4>(d->mask_kind, p, s, image, mask, params, disp, image_out, mask_out); break;
  }
  UZ_LAUNCH_CHECK("uz_augment_apply");
  return UZ_OK;
}
