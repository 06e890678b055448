/* Plain-C restatement (host pointers, one thread) of the two entries that form a gradient instead of reading it:
 *   uz_bn_relu_bwd_apply_head  -> uz_bn_relu_bwd_apply_head_ref
 *   uz_conv3x3_first_wgrad_bn  -> uz_conv3x3_first_wgrad_bn_ref
 * bf16 tensors as uint16 bit patterns.  Compiled by the tests that use it (tests/fold_ref.py); build with -ffp-contract=off:
 * every fused multiply-add of the statement is written as fmaf(). */
#include <math.h>
#include <stdint.h>
#include <string.h>

static float bf2f(uint16_t b) {
  uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

static uint16_t f2bf(float f) { /* round to nearest even (finite inputs) */
  uint32_t u;
  memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

/* dy of the BatchNorm + ReLU backward apply pass for one element */
static float bn_bwd_elem(float y, float g, float sc, float sh, float mu, float is, float k0, float k1) {
  const float pre = fmaf(y, sc, sh);
  const float dz = pre > 0.f ? g : 0.f;
  const float xh = (y - mu) * is;
  return sc * ((dz - k0) - xh * k1);
}

int uz_bn_relu_bwd_apply_head_ref(int N, int H, int W, int C, int ldy, int lddy, const uint16_t* y, const float* scale,
                                  const float* shift, const float* mean, const float* invstd, const float* g_nchw,
                                  const float* w, int Kout, const double* sums, double count, uint16_t* dy) {
  const int HW = H * W;
  const double inv = 1.0 / count;
  for (int n = 0; n < N; ++n)
    for (int hw = 0; hw < HW; ++hw) {
      const long long p = (long long)n * HW + hw;
      for (int c = 0; c < C; ++c) {
        float d = 0.f;
        for (int k = 0; k < Kout; ++k) d = fmaf(g_nchw[((long long)n * Kout + k) * HW + hw], w[k * C + c], d);
        const float gv = bf2f(f2bf(d)); /* the gradient as the head would have stored it */
        const float k0 = (float)(sums[c] * inv), k1 = (float)(sums[C + c] * inv);
        dy[p * lddy + c] = f2bf(bn_bwd_elem(bf2f(y[p * ldy + c]), gv, scale[c], shift[c], mean[c], invstd[c], k0, k1));
      }
    }
  return 0;
}

int uz_conv3x3_first_wgrad_bn_ref(const float* x, int N, int C, int H, int W, const uint16_t* g, int ldg, const uint16_t* y,
                                  int ldy, const float* scale, const float* shift, const float* mean, const float* invstd,
                                  const double* sums, double count, int Cout, float* dw) {
  const double inv = 1.0 / count;
  for (int co = 0; co < Cout; ++co) {
    const float k0 = (float)(sums[co] * inv), k1 = (float)(sums[Cout + co] * inv);
    for (int c = 0; c < C; ++c)
      for (int ty = 0; ty < 3; ++ty)
        for (int tx = 0; tx < 3; ++tx) {
          double acc = 0.0;
          for (int n = 0; n < N; ++n)
            for (int h = 0; h < H; ++h)
              for (int ww = 0; ww < W; ++ww) {
                const int ih = h + ty - 1, iw = ww + tx - 1;
                if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;
                const long long p = ((long long)n * H + h) * W + ww;
                const float d = bf2f(f2bf(bn_bwd_elem(bf2f(y[p * ldy + co]), bf2f(g[p * ldg + co]), scale[co], shift[co],
                                                      mean[co], invstd[co], k0, k1)));
                const float xv = bf2f(f2bf(x[(((long long)n * C + c) * H + ih) * W + iw]));
                acc += (double)d * (double)xv;
              }
          dw[((co * C + c) * 3 + ty) * 3 + tx] = (float)acc;
        }
  }
  return 0;
}
