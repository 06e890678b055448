// Sliding-window inference around a model.
//   uz_tile_plan    the tile starts along one axis (MONAI's rule), pure host code: Python calls it and never restates it
//   uz_tile_gather  the tiles [t0, t0 + tn) of an image batch as one contiguous batch, zero or reflect padding, one launch
//   uz_tile_blend   prob = sum_k w_k p_k / sum_k w_k over the tiles that cover a pixel, in tile order; one thread owns a pixel:
//                   fp32 products and sums, one IEEE division, no atomics, bit-reproducible
// Along an axis the image lies on a canvas of max(size, window) pixels at offset floor((window - size) / 2) when it is smaller
// than the window.  The start tables travel in the kernel arguments; they are strictly ascending, so the tiles that cover a
// canvas pixel along an axis are a run [first, first + count) of the table.
#include "uz_common.h"

namespace {

constexpr int TL_THREADS = 256;
static_assert(TL_THREADS == UZ_TILE_MAX_AXIS, "a workgroup stages one table entry per thread");

struct TlTabs {
  int ys[UZ_TILE_MAX_AXIS], xs[UZ_TILE_MAX_AXIS];
};

__device__ __forceinline__ int tl_src(int i, int size, int reflect) {
  // canvas pixel minus the image's offset -> the image pixel, or -1 for a zero
  if (i >= 0 && i < size) return i;
  if (!reflect) return -1;
  return i < 0 ? -i : 2 * (size - 1) - i;            // pad < size: one reflection lands inside
}

// one element of the tile batch per thread and step
__global__ __launch_bounds__(TL_THREADS) void tile_gather_kernel(TlTabs tab, const float* __restrict__ x, float* __restrict__ out, long long total,
                                                                 int C, int H, int W, int th, int tw, int ny, int nx, int oy, int ox, int t0,
                                                                 int reflect) {
  __shared__ int sy[UZ_TILE_MAX_AXIS], sx[UZ_TILE_MAX_AXIS];
  sy[threadIdx.x] = tab.ys[threadIdx.x], sx[threadIdx.x] = tab.xs[threadIdx.x];      // (loads from the argument segment: no scratch copy)
  __syncthreads();
  for (long long e = (long long)blockIdx.x * TL_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * TL_THREADS) {
    const int xx = (int)(e % tw), yy = (int)(e / tw % th);
    const long long plane = e / ((long long)tw * th);
    const int c = (int)(plane % C), t = t0 + (int)(plane / C);
    const int ix = t % nx, iy = t / nx % ny, n = t / (nx * ny);
    const int h = tl_src(sy[iy] + yy - oy, H, reflect), w = tl_src(sx[ix] + xx - ox, W, reflect);
    const bool in = h >= 0 && w >= 0;
    const float v = x[in ? (((size_t)n * C + c) * H + h) * W + w : 0];
    out[e] = in ? v : 0.f;
  }
}

// one pixel of the output per thread and step.  KY x KX slots: slot (a, b) is the tile (first_y + a, first_x + b); a slot past
// the run reads the run's first tile (a valid address) and adds nothing.  All KY KX loads are issued before the arithmetic.
template <int KY, int KX>
__global__ __launch_bounds__(TL_THREADS) void tile_blend_kernel(TlTabs tab, const float* __restrict__ tiles, const float* __restrict__ gh,
                                                                const float* __restrict__ gw, float* __restrict__ out, long long total, int C,
                                                                int H, int W, int th, int tw, int ny, int nx, int oy, int ox) {
  __shared__ int sy[UZ_TILE_MAX_AXIS], sx[UZ_TILE_MAX_AXIS];
  sy[threadIdx.x] = tab.ys[threadIdx.x], sx[threadIdx.x] = tab.xs[threadIdx.x];
  __syncthreads();
  for (long long e = (long long)blockIdx.x * TL_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * TL_THREADS) {
    const int x = (int)(e % W), y = (int)(e / W % H);
    const long long plane = e / ((long long)W * H);
    const int c = (int)(plane % C), n = (int)(plane / C);
    const int cy = y + oy, cx = x + ox;               // on the canvas
    int fy = 0, ly = 0, fx = 0, lx = 0;               // tiles wholly before the pixel / starting at or before it
    for (int i = 0; i < ny; ++i) fy += sy[i] + th <= cy, ly += sy[i] <= cy;
    for (int i = 0; i < nx; ++i) fx += sx[i] + tw <= cx, lx += sx[i] <= cx;
    const int ky = ly - fy, kx = lx - fx;             // >= 1 each: the host checked that the tables leave no gap
    int py[KY], px[KX];                               // the pixel's place in the tile of a slot
    size_t rowat[KY], colat[KX];                      // tile t = (n ny + iy) nx + ix starts at t C th tw
    float wy[KY], wx[KX];
#pragma unroll
    for (int a = 0; a < KY; ++a) {
      const int iy = a < ky ? fy + a : fy;
      py[a] = cy - sy[iy];
      rowat[a] = ((((size_t)n * ny + iy) * nx * C + c) * th + py[a]) * tw;
    }
#pragma unroll
    for (int b = 0; b < KX; ++b) {
      const int ix = b < kx ? fx + b : fx;
      px[b] = cx - sx[ix];
      colat[b] = (size_t)ix * C * th * tw + px[b];
    }
    float p[KY][KX];
#pragma unroll
    for (int a = 0; a < KY; ++a)
#pragma unroll
      for (int b = 0; b < KX; ++b) p[a][b] = tiles[rowat[a] + colat[b]];
#pragma unroll
    for (int a = 0; a < KY; ++a) wy[a] = gh[py[a]];
#pragma unroll
    for (int b = 0; b < KX; ++b) wx[b] = gw[px[b]];
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int a = 0; a < KY; ++a)
#pragma unroll
      for (int b = 0; b < KX; ++b) {
        const bool on = a < ky && b < kx;
        const float w = fmaxf(__fmul_rn(wy[a], wx[b]), 1e-3f);
        num = __fadd_rn(num, on ? __fmul_rn(w, p[a][b]) : 0.f);     // + 0 changes nothing: the sum is the covering tiles' alone
        den = __fadd_rn(den, on ? w : 0.f);
      }
    out[e] = __fdiv_rn(num, den);
  }
}

typedef void (*TlBlendFn)(TlTabs, const float*, const float*, const float*, float*, long long, int, int, int, int, int, int, int, int, int);

template <int KY>
TlBlendFn tl_blend_x(int kx) {
  return kx <= 1 ? tile_blend_kernel<KY, 1> : kx <= 2 ? tile_blend_kernel<KY, 2> : kx <= 4 ? tile_blend_kernel<KY, 4> : tile_blend_kernel<KY, 8>;
}

TlBlendFn tl_blend(int ky, int kx) {
  return ky <= 1 ? tl_blend_x<1>(kx) : ky <= 2 ? tl_blend_x<2>(kx) : ky <= 4 ? tl_blend_x<4>(kx) : tl_blend_x<8>(kx);
}

unsigned tl_grid(long long total) { return (unsigned)uz_grid_cap((total + TL_THREADS - 1) / TL_THREADS, 8); }

// the start table of one axis: strictly ascending from 0 to D - window, no gap; *cover = the most tiles over one pixel
int tl_axis(const char* who, const char* axis, const int* starts, int n, int size, int window, int* cover) {
  UZ_REQUIRE(n >= 1 && n <= UZ_TILE_MAX_AXIS, "%s: %d tiles along %s outside [1, %d]", who, n, axis, UZ_TILE_MAX_AXIS);
  const int D = size > window ? size : window;
  UZ_REQUIRE(starts[0] == 0 && starts[n - 1] == D - window, "%s: the starts along %s do not run from 0 to %d", who, axis, D - window);
  for (int i = 1; i < n; ++i)
    UZ_REQUIRE(starts[i] > starts[i - 1] && starts[i] - starts[i - 1] <= window, "%s: the starts along %s are not ascending or leave a gap at %d",
               who, axis, i);
  int most = 1;
  for (int i = 0; i < n; ++i) {
    int j = i;
    while (j + 1 < n && starts[j + 1] - starts[i] < window) ++j;      // the pixel starts[j] lies in the tiles i .. j
    most = j - i + 1 > most ? j - i + 1 : most;
  }
  UZ_REQUIRE(most <= UZ_TILE_MAX_COVER, "%s: %d tiles cover one pixel along %s, at most %d", who, most, axis, UZ_TILE_MAX_COVER);
  *cover = most;
  return UZ_OK;
}

int tl_shape(const char* who, int N, int C, int H, int W, int th, int tw) {
  UZ_REQUIRE(N >= 1 && C >= 1 && H >= 1 && W >= 1, "%s: non-positive shape", who);
  UZ_REQUIRE(th >= 1 && tw >= 1, "%s: non-positive window", who);
  UZ_REQUIRE((long long)N * C * H * W < (1LL << 31), "%s: too large (N C H W >= 2^31)", who);
  return UZ_OK;
}

void tl_tabs(TlTabs* t, const int* ys, int ny, const int* xs, int nx) {
  for (int i = 0; i < UZ_TILE_MAX_AXIS; ++i) t->ys[i] = i < ny ? ys[i] : 0, t->xs[i] = i < nx ? xs[i] : 0;
}

}  // namespace

extern "C" int uz_tile_plan(int size, int window, double overlap, int* starts, int cap) {
  UZ_REQUIRE(size >= 1 && window >= 1, "uz_tile_plan: size = %d and window = %d must be positive", size, window);
  UZ_REQUIRE(overlap >= 0.0 && overlap <= 0.75, "uz_tile_plan: overlap = %g outside [0, 0.75]", overlap);     // (a NaN fails both)
  UZ_REQUIRE(starts != nullptr, "uz_tile_plan: null pointer");
  const long long D = size > window ? size : window;
  int step = (int)(window * (1.0 - overlap));
  step = step < 1 ? 1 : step;
  const long long n = D == window ? 1 : (D - window + step - 1) / step + 1;
  UZ_REQUIRE(n <= UZ_TILE_MAX_AXIS && n <= cap, "uz_tile_plan: %lld tiles along an axis, at most %d (and room for %d)", n, UZ_TILE_MAX_AXIS, cap);
  for (long long i = 0; i < n; ++i) starts[i] = (int)(i * step < D - window ? i * step : D - window);
  return (int)n;
}

extern "C" int uz_tile_gather(const uz_tile_gather_desc* d, const int* ys, const int* xs, const float* x, float* out, void* stream) {
  const char* who = "uz_tile_gather";
  UZ_REQUIRE(d != nullptr, "%s: null descriptor", who);
  int rc = tl_shape(who, d->N, d->C, d->H, d->W, d->th, d->tw);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(d->pad_mode == UZ_TILE_PAD_ZERO || d->pad_mode == UZ_TILE_PAD_REFLECT, "%s: unknown pad_mode %d", who, d->pad_mode);
  UZ_REQUIRE(ys && xs && x && out, "%s: null pointer", who);
  int cover;
  if ((rc = tl_axis(who, "H", ys, d->ny, d->H, d->th, &cover)) != UZ_OK) return rc;
  if ((rc = tl_axis(who, "W", xs, d->nx, d->W, d->tw, &cover)) != UZ_OK) return rc;
  const long long T = (long long)d->N * d->ny * d->nx;
  UZ_REQUIRE(d->t0 >= 0 && d->tn >= 1 && (long long)d->t0 + d->tn <= T, "%s: tiles [%d, %d + %d) outside the list of %lld", who, d->t0, d->t0, d->tn, T);
  const long long total = (long long)d->tn * d->C * d->th * d->tw, nx_ = (long long)d->N * d->C * d->H * d->W;
  UZ_REQUIRE(total < (1LL << 31), "%s: too large (tn C th tw >= 2^31)", who);
  const int py = d->th > d->H ? d->th - d->H : 0, px = d->tw > d->W ? d->tw - d->W : 0;     // the whole padding of an axis
  const int oy = py / 2, ox = px / 2;
  if (d->pad_mode == UZ_TILE_PAD_REFLECT)
    UZ_REQUIRE(py - oy < d->H && px - ox < d->W, "%s: reflect needs pad < size, got pads (%d, %d) on a %d x %d image", who, py - oy, px - ox, d->H, d->W);
  UZ_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)out & 3) == 0, "%s: a tensor is not 4-byte aligned", who);
  UZ_REQUIRE(!uz_overlap(uz_range(x, 4 * nx_), uz_range(out, 4 * total)), "%s: the output overlaps the input", who);
  TlTabs tab;
  tl_tabs(&tab, ys, d->ny, xs, d->nx);
  hipLaunchKernelGGL(tile_gather_kernel, dim3(tl_grid(total)), dim3(TL_THREADS), 0, static_cast<hipStream_t>(stream), tab, x, out, total, d->C, d->H,
                     d->W, d->th, d->tw, d->ny, d->nx, oy, ox, d->t0, d->pad_mode == UZ_TILE_PAD_REFLECT ? 1 : 0);
  UZ_LAUNCH_CHECK(who);
  return UZ_OK;
}

extern "C" int uz_tile_blend(const uz_tile_blend_desc* d, const int* ys, const int* xs, const float* tiles, const float* gh, const float* gw,
                             float* out, void* stream) {
  const char* who = "uz_tile_blend";
  UZ_REQUIRE(d != nullptr, "%s: null descriptor", who);
  int rc = tl_shape(who, d->N, d->C, d->H, d->W, d->th, d->tw);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(ys && xs && tiles && gh && gw && out, "%s: null pointer", who);
  int ky, kx;
  if ((rc = tl_axis(who, "H", ys, d->ny, d->H, d->th, &ky)) != UZ_OK) return rc;
  if ((rc = tl_axis(who, "W", xs, d->nx, d->W, d->tw, &kx)) != UZ_OK) return rc;
  const long long total = (long long)d->N * d->C * d->H * d->W, nt = (long long)d->N * d->ny * d->nx * d->C * d->th * d->tw;
  UZ_REQUIRE(nt < (1LL << 31), "%s: too large (T C th tw >= 2^31)", who);
  UZ_REQUIRE((((uintptr_t)tiles | (uintptr_t)gh | (uintptr_t)gw | (uintptr_t)out) & 3) == 0, "%s: a tensor is not 4-byte aligned", who);
  const UzRange outr = uz_range(out, 4 * total), in[3] = {uz_range(tiles, 4 * nt), uz_range(gh, 4LL * d->th), uz_range(gw, 4LL * d->tw)};
  UZ_REQUIRE(!uz_any_overlap(&outr, 1, in, 3), "%s: the output overlaps an input", who);
  const int oy = d->th > d->H ? (d->th - d->H) / 2 : 0, ox = d->tw > d->W ? (d->tw - d->W) / 2 : 0;
  TlTabs tab;
  tl_tabs(&tab, ys, d->ny, xs, d->nx);
  TlBlendFn fn = tl_blend(ky, kx);
  hipLaunchKernelGGL(fn, dim3(tl_grid(total)), dim3(TL_THREADS), 0, static_cast<hipStream_t>(stream), tab, tiles, gh, gw, out, total, d->C, d->H, d->W,
                     d->th, d->tw, d->ny, d->nx, oy, ox);
  UZ_LAUNCH_CHECK(who);
  return UZ_OK;
}
