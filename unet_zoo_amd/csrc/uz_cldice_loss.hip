// clDice (Shit et al.: "clDice -- a novel topology-preserving loss function for tubular structure segmentation", CVPR 2021) on
// the device, added to a base loss whose value and gradients already exist (include/unetzoo_hip.h).
// For a plane a (H, W), every window clipped to the picture:
//   erode(a)  = min(v, h), v the minimum of the vertical 3-window (up, centre, down), h of the horizontal one (left, centre,
//               right);   dilate(a) = the maximum of the 3 x 3 window;   open(a) = dilate(erode(a))
//   skel_k(a) : S = relu(a - open(a)); then k times: a <- erode(a), d = relu(a - open(a)), S <- S + relu(d - S d)
// i.e. with a_0 = a, a_(j+1) = erode(a_j), d_j = relu(a_j - dilate(a_(j+1))): S_0 = d_0, S_j = S_(j-1) + relu(d_j - S_(j-1) d_j).
// skel_k at a pixel depends on a within Chebyshev distance R = k + 2.  Per segment, with s = smooth:
//   Tprec = (sum skel(p) t + s) / (sum skel(p) + s),  Tsens = (sum skel(t) p + s) / (sum skel(t) + s),
//   cl = 1 - 2 Tprec Tsens / (Tprec + Tsens);   V = the mean of cl over the segments
// Subgradients are torch's: relu'(0) = 0; dilate routes to the first maximum in row-major window order; v to the first minimum
// top to bottom, h left to right; min(v, h) to the smaller one, half to each on v == h.
//
// Launches, every one with a fixed grid for a descriptor (6 with a gradient buffer, 4 without):
//   prob      p = sigmoid(x) or the masked softmax of every map -> workspace (and `probs` of the main map); class mode: the
//             target planes t_c = (y == c) of the valid pixels
//   tskel     per (plane, tile): skel(t), once for all maps -> `target_skeleton`
//   forward   per (map, plane, tile) unit: the tile of p with a halo of R in LDS, all k + 1 rounds there; the unit's float64
//             sums of skel(p) t, skel(p), skel(t) p, skel(t); `skeleton` of the main map
//   sums      one workgroup, a wave a segment: the units' sums in index order, cl, V, dV/dA, dV/dB, dV/dC; out[0], out[1]
//   backward  per unit: a halo of 2 R.  Round j = k .. 0: a_0 .. a_(j+1) and S_(j-1) are formed again from p (two rolling
//             images; nothing of the forward is kept, which is what lets k = 10 fit), q_j = dV/d(a_j - open) at every pixel,
//             then in GATHER form: every pixel of a_(j+1) collects -q_j from the 3 x 3 windows whose first maximum it is, and
//             every pixel of a_j collects d/da_(j+1) from the (at most five) erosions that chose it.  The choices are 10-bit
//             codes in a 16-bit LDS image.  No LDS float atomics.  + dV/dC skel(t); dV/dp of the tile interior -> workspace
//   grad      dl <- base_scale dl + weight ow dV/dp dp/dx  (sigmoid' or the softmax coupling)
// No workgroup waits for another inside a launch, no float atomics, nothing to clear: every buffer is fully written by plain
// stores before it is read.  The k + 1 intermediate images never reach global memory.
#include "uz_common.h"

#include <math.h>

namespace {

constexpr int CD_TH = UZ_CLDICE_TILE_H, CD_TW = UZ_CLDICE_TILE_W;
constexpr int CD_THREADS = 1024;      // tile kernels: one workgroup per CU at k = 10 (LDS), 16 waves to hide the LDS latency
constexpr int CD_WAVES = CD_THREADS / 64;
constexpr int CD_PT = 256;            // the streaming passes and the sums
constexpr long long CD_MAX_ELEMS = 1LL << 28;

struct CdItems {
  uz_cldice_item it[UZ_CLASS_MAX_ITEMS];
};

struct CdGeo {
  int mode, n_items;
  int N, C, H, W, HW;
  int c0, Cp;          // first plane that counts, planes that count per image
  int NP;              // N * Cp
  int per_image, nseg; // segments per map
  int k;               // iterations
  int tx, tiles;       // tiles across, tiles per plane
  int tunits;          // NP * tiles: the target's units
  int units;           // n_items * tunits
  int ignore_index, main_item;
  double smooth;
  long long E, pixels; // N C H W, N H W
};

// ------------------------------------------------------------------------------------------------- the morphology on an LDS image
// A region is RH x RW pixels at picture offset (oy, ox); a pixel outside the picture is never read or written, which is what
// clips the windows to the picture.  They are clipped to the region too, so that no index leaves it; the passes below never
// need a pixel that this second clipping has touched (CdRect).
struct CdPix {
  bool in, up, dn, lf, rt;
};

template <int RH, int RW>
__device__ __forceinline__ CdPix cd_pix(int ry, int rx, int oy, int ox, int H, int W) {
  const int gy = oy + ry, gx = ox + rx;
  CdPix p;
  p.in = gy >= 0 && gy < H && gx >= 0 && gx < W;
  p.up = ry > 0 && gy > 0;
  p.dn = ry < RH - 1 && gy < H - 1;
  p.lf = rx > 0 && gx > 0;
  p.rt = rx < RW - 1 && gx < W - 1;
  return p;
}

// The region without a margin of m pixels on every side: what one pass works on.  An operation reads its input one pixel
// further out than it writes, so the passes of a round shrink towards the tile and no pixel is computed that nothing needs.
template <int RH, int RW>
struct CdRect {
  int m, w, n;
  float inv;
  __device__ explicit CdRect(int margin) : m(margin), w(RW - 2 * margin), n((RH - 2 * margin) * (RW - 2 * margin)), inv(1.f / (float)(RW - 2 * margin)) {}
  // pixel idx of the rectangle in row-major order -> its index in the region (idx < 2^13: the float quotient is off by one at most)
  __device__ __forceinline__ int at(int idx, int& ry, int& rx) const {
    int q = (int)((float)idx * inv), r = idx - q * w;
    if (r < 0) --q, r += w;
    else if (r >= w) ++q, r -= w;
    ry = m + q, rx = m + r;
    return ry * RW + rx;
  }
};

// code bits: 0-3 the dilation's first maximum (row-major index in the 3 x 3 window), 4-5 v's choice (0 up, 1 centre, 2 down),
// 6-7 h's (0 left, 1 centre, 2 right), 8-9: 0 v < h, 1 v == h, 2 v > h
template <int RH, int RW, bool CODE>
__device__ __forceinline__ void cd_erode(const float* A, float* B, unsigned short* code, int m, int oy, int ox, int H, int W) {
  const CdRect<RH, RW> rc(m);
  for (int idx = threadIdx.x; idx < rc.n; idx += CD_THREADS) {
    int ry, rx;
    const int i = rc.at(idx, ry, rx);
    const CdPix p = cd_pix<RH, RW>(ry, rx, oy, ox, H, W);
    if (!p.in) continue;
    const float c = A[i];
    if (!CODE && p.up && p.dn && p.lf && p.rt) {      // all five inside the picture, the choices not wanted: the plain minimum
      B[i] = fminf(fminf(fminf(A[i - RW], A[i + RW]), fminf(A[i - 1], A[i + 1])), c);
      continue;
    }
    const float u = A[p.up ? i - RW : i], d = A[p.dn ? i + RW : i], l = A[p.lf ? i - 1 : i], r = A[p.rt ? i + 1 : i];
    float v = c, h = c;
    int va = 1, ha = 1;
    if (p.up && u <= c) v = u, va = 0;      // the first minimum top to bottom
    if (p.dn && d < v) v = d, va = 2;
    if (p.lf && l <= c) h = l, ha = 0;      // ... left to right
    if (p.rt && r < h) h = r, ha = 2;
    B[i] = fminf(v, h);
    if (CODE) code[i] = (unsigned short)((va << 4) | (ha << 6) | ((v < h ? 0 : (v == h ? 1 : 2)) << 8));
  }
}

template <int RW>
__device__ __forceinline__ float cd_dilate(const float* B, int i, const CdPix& p, int& idx) {
  float best = 0.f;
  if (p.up && p.dn && p.lf && p.rt) {      // the whole window inside the picture: nine reads at fixed offsets
    best = B[i - RW - 1];
    idx = 0;
#pragma unroll
    for (int w = 1; w < 9; ++w) {
      const float val = B[i + (w / 3 - 1) * RW + (w % 3 - 1)];
      if (val > best) best = val, idx = w;
    }
    return best;
  }
  idx = -1;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
    const bool oky = dy < 0 ? p.up : (dy > 0 ? p.dn : true);
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const bool ok = oky && (dx < 0 ? p.lf : (dx > 0 ? p.rt : true));
      const float val = B[ok ? i + dy * RW + dx : i];
      if (ok && (idx < 0 || val > best)) best = val, idx = (dy + 1) * 3 + dx + 1;      // the first maximum in row-major order
    }
  }
  return best;
}

// the maximum alone
template <int RW>
__device__ __forceinline__ float cd_dilate_max(const float* B, int i, const CdPix& p) {
  if (p.up && p.dn && p.lf && p.rt) {
    const float r0 = fmaxf(fmaxf(B[i - RW - 1], B[i - RW]), B[i - RW + 1]);
    const float r1 = fmaxf(fmaxf(B[i - 1], B[i]), B[i + 1]);
    const float r2 = fmaxf(fmaxf(B[i + RW - 1], B[i + RW]), B[i + RW + 1]);
    return fmaxf(fmaxf(r0, r1), r2);
  }
  int idx;
  return cd_dilate<RW>(B, i, p, idx);
}

// S_i from a_i (A) and a_(i+1) (B) at every pixel of the region less a margin of m; S holds S_(i-1)
template <int RH, int RW>
__device__ __forceinline__ void cd_skel_step(const float* A, const float* B, float* S, int round, int m, int oy, int ox, int H, int W) {
  const CdRect<RH, RW> rc(m);
  for (int idx = threadIdx.x; idx < rc.n; idx += CD_THREADS) {
    int ry, rx;
    const int i = rc.at(idx, ry, rx);
    const CdPix p = cd_pix<RH, RW>(ry, rx, oy, ox, H, W);
    if (!p.in) continue;
    const float d = fmaxf(A[i] - cd_dilate_max<RW>(B, i, p), 0.f);
    if (round == 0) {
      S[i] = d;
    } else {
      const float s = S[i];
      S[i] = s + fmaxf(d - s * d, 0.f);
    }
  }
}

// the plane's region -> LDS; the address is clamped and the value selected, no load under a branch
template <int RH, int RW>
__device__ __forceinline__ void cd_load(const float* __restrict__ plane, float* A, int m, int oy, int ox, int H, int W) {
  const CdRect<RH, RW> rc(m);
  for (int idx = threadIdx.x; idx < rc.n; idx += CD_THREADS) {
    int ry, rx;
    const int i = rc.at(idx, ry, rx);
    const int gy = oy + ry, gx = ox + rx;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    const float v = plane[in ? (size_t)gy * W + gx : 0];
    A[i] = in ? v : 0.f;
  }
}

// the sum of a workgroup's doubles in a fixed order, to thread 0
__device__ __forceinline__ double cd_block_sum(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int q = 0; q < CD_WAVES; ++q) t += red[q];
  __syncthreads();
  return t;
}

constexpr int cd_halo(int kmax) { return kmax + 2; }

// ------------------------------------------------------------------------------------------------------------- forward tiles
// TARGET: the planes are the target's, skel(t) -> tskel, no sums.  Otherwise a unit is (map, plane, tile).
template <int KMAX, bool TARGET>
__global__ __launch_bounds__(CD_THREADS) void cldice_forward_kernel(const CdGeo geo, const float* __restrict__ prob, const float* __restrict__ tplanes,
                                                                    float* __restrict__ tskel, float* __restrict__ skeleton,
                                                                    double* __restrict__ part) {
  constexpr int HALO = cd_halo(KMAX), RH = CD_TH + 2 * HALO, RW = CD_TW + 2 * HALO;
  __shared__ float img[3][RH * RW];
  __shared__ double red[CD_WAVES];
  const int H = geo.H, W = geo.W;
  const int total = TARGET ? geo.tunits : geo.units;
  for (int unit = blockIdx.x; unit < total; unit += gridDim.x) {
    const int item = unit / geo.tunits, rem = unit - item * geo.tunits;
    const int pl = rem / geo.tiles, tile = rem - pl * geo.tiles;
    const int n = pl / geo.Cp, c = geo.c0 + (pl - n * geo.Cp);
    const int ty = tile / geo.tx, tcol = tile - ty * geo.tx;
    const int oy = ty * CD_TH - HALO, ox = tcol * CD_TW - HALO;
    const size_t plane_at = ((size_t)n * geo.C + c) * geo.HW;
    const float* __restrict__ src = TARGET ? tplanes + plane_at : prob + (size_t)item * geo.E + plane_at;
    float *A = img[0], *B = img[1], *S = img[2];
    // S is wanted on the tile: a_(i+1) one pixel further out, a_i on a halo of k + 2 - i, p on R = k + 2
    const int m0 = HALO - (geo.k + 2);
    cd_load<RH, RW>(src, A, m0, oy, ox, H, W);
    __syncthreads();
    for (int i = 0; i <= geo.k; ++i) {
      cd_erode<RH, RW, false>(A, B, nullptr, m0 + i + 1, oy, ox, H, W);
      __syncthreads();
      cd_skel_step<RH, RW>(A, B, S, i, HALO, oy, ox, H, W);
      __syncthreads();
      float* t = A;
      A = B, B = t;
    }
    double sa = 0.0, sb = 0.0, sc = 0.0, sd = 0.0;
    const CdRect<RH, RW> inner(HALO);
    for (int idx = threadIdx.x; idx < inner.n; idx += CD_THREADS) {
      int ry, rx;
      const int i = inner.at(idx, ry, rx);
      const int gy = oy + ry, gx = ox + rx;
      if (gy >= H || gx >= W) continue;
      const size_t at = plane_at + (size_t)gy * W + gx;
      const float s = S[i];
      if (TARGET) {
        tskel[at] = s;
      } else {
        const float t = tplanes[at], ts = tskel[at], p = src[(size_t)gy * W + gx];
        sa += (double)s * (double)t;
        sb += (double)s;
        sc += (double)ts * (double)p;
        sd += (double)ts;
        if (item == geo.main_item) skeleton[at] = s;
      }
    }
    if (!TARGET) {
      sa = cd_block_sum(sa, red);
      sb = cd_block_sum(sb, red);
      sc = cd_block_sum(sc, red);
      sd = cd_block_sum(sd, red);
      if (threadIdx.x == 0) {
        double* o = part + (size_t)unit * 4;
        o[0] = sa, o[1] = sb, o[2] = sc, o[3] = sd;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------ backward tiles
template <int KMAX>
__global__ __launch_bounds__(CD_THREADS) void cldice_backward_kernel(const CdItems tab, const CdGeo geo, const float* __restrict__ prob,
                                                                     const float* __restrict__ tplanes, const float* __restrict__ tskel,
                                                                     const double* __restrict__ coef, float* __restrict__ dprob) {
  constexpr int HALO = 2 * cd_halo(KMAX), RH = CD_TH + 2 * HALO, RW = CD_TW + 2 * HALO, RN = RH * RW;
  __shared__ float img[5][RN];
  __shared__ unsigned short code[RN];
  const int H = geo.H, W = geo.W;
  for (int unit = blockIdx.x; unit < geo.units; unit += gridDim.x) {
    const int item = unit / geo.tunits, rem = unit - item * geo.tunits;
    if (tab.it[item].dlogits == nullptr) continue;      // uniform over the workgroup
    const int pl = rem / geo.tiles, tile = rem - pl * geo.tiles;
    const int n = pl / geo.Cp, cc = pl - n * geo.Cp, c = geo.c0 + cc;
    const int ty = tile / geo.tx, tcol = tile - ty * geo.tx;
    const int oy = ty * CD_TH - HALO, ox = tcol * CD_TW - HALO;
    const size_t plane_at = ((size_t)n * geo.C + c) * geo.HW;
    const float* __restrict__ src = prob + (size_t)item * geo.E + plane_at;
    const int seg = item * geo.nseg + (geo.per_image ? pl : cc);
    const float cA = (float)coef[seg * 3 + 0], cB = (float)coef[seg * 3 + 1], cC = (float)coef[seg * 3 + 2];
    float *A = img[0], *B = img[1], *GA = img[2];       // the two rolling images a_i, a_(i+1) and d/da_(j+1)
    float* const SQ = img[3];                           // S_(j-1), then q_j
    float* const G = img[4];                            // dV/dS_j
    for (int i = threadIdx.x; i < RN; i += CD_THREADS) {
      const int ry = i / RW, rx = i - ry * RW;
      const int gy = oy + ry, gx = ox + rx;
      const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
      const float t = tplanes[plane_at + (in ? (size_t)gy * W + gx : 0)];
      G[i] = in ? cA * t + cB : 0.f;                    // dV/dskel(p) = dV/dA t + dV/dB
      GA[i] = 0.f;
    }
    __syncthreads();
    for (int j = geo.k; j >= 0; --j) {
      // halos of round j, in pixels around the tile: d/da_j on j, d/da_(j+1) on j + 1, q_j and S_(j-1) on j + 2, a_(j+1) on
      // j + 3, a_i on 2 j + 4 - i, p on 2 j + 4 (<= 2 R)
      const int mp = HALO - (2 * j + 4), mq = HALO - (j + 2);
      cd_load<RH, RW>(src, A, mp, oy, ox, H, W);
      __syncthreads();
      for (int i = 0; i < j; ++i) {                     // a_0 .. a_j and S_(j-1) again
        cd_erode<RH, RW, false>(A, B, nullptr, mp + i + 1, oy, ox, H, W);
        __syncthreads();
        cd_skel_step<RH, RW>(A, B, SQ, i, mq, oy, ox, H, W);
        __syncthreads();
        float* t = A;
        A = B, B = t;
      }
      cd_erode<RH, RW, true>(A, B, code, mp + j + 1, oy, ox, H, W);      // A = a_j, B = a_(j+1), with the erosion's choices
      __syncthreads();
      const CdRect<RH, RW> rq(mq), rd(mq + 1), re(mq + 2);
      for (int ix = threadIdx.x; ix < rq.n; ix += CD_THREADS) {
        int ry, rx;
        const int i = rq.at(ix, ry, rx);
        const CdPix p = cd_pix<RH, RW>(ry, rx, oy, ox, H, W);
        if (!p.in) continue;
        int idx;
        const float raw = A[i] - cd_dilate<RW>(B, i, p, idx);
        const float d = fmaxf(raw, 0.f), g = G[i];
        float gd = g;                                   // j = 0: S_0 = d_0
        if (j > 0) {
          const float s = SQ[i];
          const bool m = d - s * d > 0.f;
          gd = m ? g - g * s : 0.f;                     // dV/dd_j
          G[i] = m ? g - g * d : g;                     // dV/dS_(j-1)
        }
        SQ[i] = raw > 0.f ? gd : 0.f;                   // q_j: relu'(0) = 0
        code[i] = (unsigned short)(code[i] | idx);
      }
      __syncthreads();
      // d/da_(j+1) += dilate^T(-q_j): from the windows (centres y around x) whose first maximum is x
      for (int ix = threadIdx.x; ix < rd.n; ix += CD_THREADS) {
        int ry, rx;
        const int i = rd.at(ix, ry, rx);
        const CdPix p = cd_pix<RH, RW>(ry, rx, oy, ox, H, W);
        if (!p.in) continue;
        float acc = GA[i];
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
          const bool oky = dy < 0 ? p.up : (dy > 0 ? p.dn : true);
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const bool ok = oky && (dx < 0 ? p.lf : (dx > 0 ? p.rt : true));
            const int y = ok ? i + dy * RW + dx : i;
            const bool hit = ok && (code[y] & 15) == (1 - dy) * 3 + (1 - dx);
            const float q = SQ[y];
            acc -= hit ? q : 0.f;
          }
        }
        GA[i] = acc;
      }
      __syncthreads();
      // d/da_j = q_j + erode^T(d/da_(j+1)): from the erosions (centres y = x and its four neighbours) that chose x
      for (int ix = threadIdx.x; ix < re.n; ix += CD_THREADS) {
        int ry, rx;
        const int i = re.at(ix, ry, rx);
        const CdPix p = cd_pix<RH, RW>(ry, rx, oy, ox, H, W);
        if (!p.in) continue;
        float acc = SQ[i];
        {
          const int cd = code[i];
          const int cmp = (cd >> 8) & 3;
          const float wv = cmp == 0 ? 1.f : (cmp == 1 ? 0.5f : 0.f), g = GA[i];
          if (((cd >> 4) & 3) == 1) acc += wv * g;
          if (((cd >> 6) & 3) == 1) acc += (1.f - wv) * g;
        }
        {                                               // the pixel below: x is its `up`
          const int y = p.dn ? i + RW : i, cd = code[y], cmp = (cd >> 8) & 3;
          const float wv = cmp == 0 ? 1.f : (cmp == 1 ? 0.5f : 0.f), g = GA[y];
          if (p.dn && ((cd >> 4) & 3) == 0) acc += wv * g;
        }
        {                                               // above: x is its `down`
          const int y = p.up ? i - RW : i, cd = code[y], cmp = (cd >> 8) & 3;
          const float wv = cmp == 0 ? 1.f : (cmp == 1 ? 0.5f : 0.f), g = GA[y];
          if (p.up && ((cd >> 4) & 3) == 2) acc += wv * g;
        }
        {                                               // to the right: x is its `left`
          const int y = p.rt ? i + 1 : i, cd = code[y], cmp = (cd >> 8) & 3;
          const float wh = cmp == 2 ? 1.f : (cmp == 1 ? 0.5f : 0.f), g = GA[y];
          if (p.rt && ((cd >> 6) & 3) == 0) acc += wh * g;
        }
        {                                               // to the left: x is its `right`
          const int y = p.lf ? i - 1 : i, cd = code[y], cmp = (cd >> 8) & 3;
          const float wh = cmp == 2 ? 1.f : (cmp == 1 ? 0.5f : 0.f), g = GA[y];
          if (p.lf && ((cd >> 6) & 3) == 2) acc += wh * g;
        }
        B[i] = acc;                                     // a_(j+1) is done with
      }
      __syncthreads();
      float* t = GA;                                    // d/da_j where a_(j+1) was; the old gradient image rolls next
      GA = B, B = t;
    }
    float* const dst = dprob + (size_t)item * geo.E + plane_at;
    const CdRect<RH, RW> inner(HALO);
    for (int ix = threadIdx.x; ix < inner.n; ix += CD_THREADS) {
      int ry, rx;
      const int i = inner.at(ix, ry, rx);
      const int gy = oy + ry, gx = ox + rx;
      if (gy >= H || gx >= W) continue;
      const size_t at = (size_t)gy * W + gx;
      dst[at] = GA[i] + cC * tskel[plane_at + at];      // + the direct term dV/dC skel(t)
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------- the streaming passes
__device__ __forceinline__ float cd_sigmoid(float x) {
  const float e = expf(-fabsf(x));
  return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

__global__ __launch_bounds__(CD_PT) void cldice_prob_binary_kernel(const CdItems tab, const CdGeo geo, float* __restrict__ prob, float* __restrict__ probs) {
  const long long stride = (long long)gridDim.x * CD_PT;
  for (int item = 0; item < geo.n_items; ++item) {
    const float* __restrict__ x = tab.it[item].logits;
    float* __restrict__ o = prob + (size_t)item * geo.E;
    for (long long a = (long long)blockIdx.x * CD_PT + threadIdx.x; a < geo.E; a += stride) {
      const float p = cd_sigmoid(x[a]);
      o[a] = p;
      if (item == geo.main_item) probs[a] = p;
    }
  }
}

// p = softmax_K(x), t_c = (y == c); a pixel whose label is ignore_index or outside [0, K): p_c = t_c = 0 in every plane
__global__ __launch_bounds__(CD_PT) void cldice_prob_class_kernel(const CdItems tab, const CdGeo geo, const int* __restrict__ target,
                                                                   float* __restrict__ prob, float* __restrict__ probs, float* __restrict__ tplanes) {
  const int K = geo.C;
  const long long stride = (long long)gridDim.x * CD_PT;
  for (int item = 0; item < geo.n_items; ++item) {
    const float* __restrict__ x = tab.it[item].logits;
    float* __restrict__ o = prob + (size_t)item * geo.E;
    for (long long q = (long long)blockIdx.x * CD_PT + threadIdx.x; q < geo.pixels; q += stride) {
      const int n = (int)(q / geo.HW), pix = (int)(q - (long long)n * geo.HW);
      const int y = target[q];
      const bool valid = y >= 0 && y < K && y != geo.ignore_index;
      const size_t at = (size_t)n * K * geo.HW + pix;
      const float* __restrict__ xp = x + at;
      float m = xp[0];
      for (int c = 1; c < K; ++c) m = fmaxf(m, xp[(size_t)c * geo.HW]);
      float sum = 0.f;
      for (int c = 0; c < K; ++c) sum += expf(xp[(size_t)c * geo.HW] - m);
      const float inv = 1.f / sum;
      for (int c = 0; c < K; ++c) {
        const float p = valid ? expf(xp[(size_t)c * geo.HW] - m) * inv : 0.f;
        o[at + (size_t)c * geo.HW] = p;
        if (item == geo.main_item) probs[at + (size_t)c * geo.HW] = p;
        if (item == 0) tplanes[at + (size_t)c * geo.HW] = valid && y == c ? 1.f : 0.f;
      }
    }
  }
}

// One workgroup.  A WAVE takes (map, segment) pairs: the units' four sums in index order (lane l adds units l, l + 64, ...,
// then a fixed tree), cl and the coefficients dV/dA, dV/dB, dV/dC with A = sum skel(p) t, B = sum skel(p), C = sum skel(t) p.
// Then thread 0: V of every map, out[0], out[1].
__global__ __launch_bounds__(CD_PT) void cldice_sums_kernel(const CdItems tab, const CdGeo geo, const double* __restrict__ part, double* __restrict__ coef,
                                                            double* __restrict__ clv, const float* __restrict__ scales,
                                                            const float* __restrict__ base_loss, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per_seg = geo.per_image ? geo.tiles : geo.N * geo.tiles;
  const int pairs = geo.n_items * geo.nseg;
  for (int pr = wave; pr < pairs; pr += CD_PT / 64) {
    const int item = pr / geo.nseg, seg = pr - item * geo.nseg;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int u = lane; u < per_seg; u += 64) {
      int pl, tile;
      if (geo.per_image) {
        pl = seg, tile = u;
      } else {
        const int n = u / geo.tiles;
        tile = u - n * geo.tiles, pl = n * geo.Cp + seg;
      }
      const double* __restrict__ o = part + ((size_t)item * geo.tunits + (size_t)pl * geo.tiles + tile) * 4;
      s[0] += o[0], s[1] += o[1], s[2] += o[2], s[3] += o[3];
    }
    for (int e = 0; e < 4; ++e)
      for (int o = 32; o > 0; o >>= 1) s[e] += __shfl_down(s[e], o);
    if (lane == 0) {
      const double sm = geo.smooth, inv_seg = 1.0 / (double)geo.nseg;
      const double tp = (s[0] + sm) / (s[1] + sm), ts = (s[2] + sm) / (s[3] + sm), den = tp + ts;
      clv[pr] = 1.0 - 2.0 * tp * ts / den;
      const double dtp = -2.0 * ts * ts / (den * den), dts = -2.0 * tp * tp / (den * den);      // d cl / d Tprec, d Tsens
      coef[pr * 3 + 0] = inv_seg * dtp / (s[1] + sm);
      coef[pr * 3 + 1] = -inv_seg * dtp * (s[0] + sm) / ((s[1] + sm) * (s[1] + sm));
      coef[pr * 3 + 2] = inv_seg * dts / (s[3] + sm);
    }
  }
  __syncthreads();      // the lanes' stores to clv, read back by thread 0
  if (threadIdx.x == 0) {
    double total = 0.0, metric = 0.0;
    for (int item = 0; item < geo.n_items; ++item) {
      double v = 0.0;
      for (int seg = 0; seg < geo.nseg; ++seg) v += clv[item * geo.nseg + seg];
      v /= (double)geo.nseg;
      total += (double)tab.it[item].weight * v;
      if (item == geo.main_item) metric = v;
    }
    out[0] = (float)((double)scales[1] * (double)base_loss[0] + (double)scales[0] * total);
    out[1] = (float)metric;
  }
}

// dV/dx = dV/dp p (1 - p)
__global__ __launch_bounds__(CD_PT) void cldice_grad_binary_kernel(const CdItems tab, const CdGeo geo, const float* __restrict__ prob,
                                                                   const float* __restrict__ dprob, const float* __restrict__ scales) {
  const float wgt = scales[0], bscale = scales[1];
  const long long stride = (long long)gridDim.x * CD_PT;
  for (int item = 0; item < geo.n_items; ++item) {
    float* __restrict__ dl = tab.it[item].dlogits;
    if (dl == nullptr) continue;
    const float coef = wgt * tab.it[item].weight;
    const float* __restrict__ pp = prob + (size_t)item * geo.E;
    const float* __restrict__ dp = dprob + (size_t)item * geo.E;
    for (long long a = (long long)blockIdx.x * CD_PT + threadIdx.x; a < geo.E; a += stride) {
      const float p = pp[a];
      dl[a] = bscale * dl[a] + coef * (dp[a] * (p * (1.f - p)));
    }
  }
}

// dV/dx_k = p_k (g_k - sum_c p_c g_c), g_c = dV/dp_c (0 for an excluded class); exactly nothing at an ignored pixel
__global__ __launch_bounds__(CD_PT) void cldice_grad_class_kernel(const CdItems tab, const CdGeo geo, const int* __restrict__ target,
                                                                  const float* __restrict__ prob, const float* __restrict__ dprob,
                                                                  const float* __restrict__ scales) {
  const float wgt = scales[0], bscale = scales[1];
  const int K = geo.C;
  const long long stride = (long long)gridDim.x * CD_PT;
  for (int item = 0; item < geo.n_items; ++item) {
    float* __restrict__ dl = tab.it[item].dlogits;
    if (dl == nullptr) continue;
    const float coef = wgt * tab.it[item].weight;
    for (long long q = (long long)blockIdx.x * CD_PT + threadIdx.x; q < geo.pixels; q += stride) {
      const int n = (int)(q / geo.HW), pix = (int)(q - (long long)n * geo.HW);
      const int y = target[q];
      const bool valid = y >= 0 && y < K && y != geo.ignore_index;
      const size_t at = (size_t)item * geo.E + (size_t)n * K * geo.HW + pix;
      const float* __restrict__ pp = prob + at;
      const float* __restrict__ gp = dprob + at;
      float* __restrict__ dp = dl + (size_t)n * K * geo.HW + pix;
      float dot = 0.f;
      for (int c = geo.c0; c < K; ++c) dot = fmaf(pp[(size_t)c * geo.HW], gp[(size_t)c * geo.HW], dot);
      for (int c = 0; c < K; ++c) {
        const float g = c >= geo.c0 ? gp[(size_t)(c >= geo.c0 ? c : geo.c0) * geo.HW] : 0.f;
        const float gk = valid ? coef * (pp[(size_t)c * geo.HW] * (g - dot)) : 0.f;
        dp[(size_t)c * geo.HW] = bscale * dp[(size_t)c * geo.HW] + gk;
      }
    }
  }
}

// --------------------------------------------------------------------------------------------------------------------- host
enum { CD_PROB, CD_TPL, CD_DPROB, CD_PART, CD_COEF, CD_CL, CD_NBUF };

struct CdPlan {
  CdGeo geo;
  int grid, tgrid, stream_grid;
  long long off[CD_NBUF], bytes;
};

int cd_plan(const uz_cldice_desc* d, const char* who, CdPlan* p) {
  UZ_REQUIRE(d != nullptr, "%s: null descriptor", who);
  UZ_REQUIRE(d->mode == UZ_CLDICE_BINARY || d->mode == UZ_CLDICE_CLASS, "%s: unknown mode %d", who, d->mode);
  UZ_REQUIRE(d->n_items >= 1 && d->n_items <= UZ_CLASS_MAX_ITEMS, "%s: n_items = %d outside [1, %d]", who, d->n_items, UZ_CLASS_MAX_ITEMS);
  UZ_REQUIRE(d->N >= 1 && d->C >= 1 && d->H >= 1 && d->W >= 1, "%s: non-positive shape", who);
  const bool cls = d->mode == UZ_CLDICE_CLASS;
  if (cls) UZ_REQUIRE(d->C >= 2 && d->C <= UZ_CLASS_MAX_K, "%s: K = %d outside [2, %d]", who, d->C, UZ_CLASS_MAX_K);
  UZ_REQUIRE(d->main_item >= 0 && d->main_item < d->n_items, "%s: main_item = %d outside [0, %d)", who, d->main_item, d->n_items);
  UZ_REQUIRE(d->iterations >= 1 && d->iterations <= UZ_CLDICE_MAX_ITERATIONS, "%s: iterations = %d outside [1, %d]", who, d->iterations,
             UZ_CLDICE_MAX_ITERATIONS);
  UZ_REQUIRE(d->smooth > 0.f && d->smooth < INFINITY, "%s: smooth must be finite and positive", who);
  const long long HW = (long long)d->H * d->W, pixels = HW * d->N, E = pixels * d->C;
  UZ_REQUIRE(E * d->n_items <= CD_MAX_ELEMS, "%s: %lld elements in %d maps, at most %lld", who, E * d->n_items, d->n_items, CD_MAX_ELEMS);
  CdGeo& g = p->geo;
  g.mode = d->mode;
  g.n_items = d->n_items;
  g.N = d->N, g.C = d->C, g.H = d->H, g.W = d->W, g.HW = (int)HW;
  g.c0 = (cls && !d->include_background) ? 1 : 0;
  g.Cp = d->C - g.c0;
  g.NP = d->N * g.Cp;
  g.per_image = d->per_image ? 1 : 0;
  g.nseg = g.per_image ? g.NP : g.Cp;
  g.k = d->iterations;
  g.tx = uz_cdiv(d->W, CD_TW);
  g.tiles = g.tx * uz_cdiv(d->H, CD_TH);
  const long long tunits = (long long)g.NP * g.tiles, units = tunits * d->n_items;
  UZ_REQUIRE(units < (1LL << 28), "%s: too many (map, plane, tile) units", who);
  g.tunits = (int)tunits;
  g.units = (int)units;
  g.ignore_index = d->ignore_index;
  g.main_item = d->main_item;
  g.smooth = (double)d->smooth;
  g.E = E;
  g.pixels = pixels;
  // four workgroups per CU of the hardware; more units than that are walked
  p->grid = uz_grid_cap(g.units, 4);
  p->tgrid = uz_grid_cap(g.tunits, 4);
  p->stream_grid = uz_grid_cap(((cls ? pixels : E) + CD_PT - 1) / CD_PT, 8);
  const long long pairs = (long long)d->n_items * g.nseg;
  const long long sizes[CD_NBUF] = {4 * E * d->n_items, cls ? 4 * E : 0, 4 * E * d->n_items, 32LL * g.units, 24 * pairs, 8 * pairs};
  p->bytes = uz_carve(sizes, CD_NBUF, p->off);
  return UZ_OK;
}

template <int KMAX>
void cd_tiles(const CdPlan& p, const float* prob, const float* tpl, float* tskel, float* skeleton, double* part,
              hipStream_t s) {
  const dim3 block(CD_THREADS);
  hipLaunchKernelGGL((cldice_forward_kernel<KMAX, true>), dim3((unsigned)p.tgrid), block, 0, s, p.geo, prob, tpl, tskel, skeleton, part);
  hipLaunchKernelGGL((cldice_forward_kernel<KMAX, false>), dim3((unsigned)p.grid), block, 0, s, p.geo, prob, tpl, tskel, skeleton, part);
}

template <int KMAX>
void cd_back(const CdPlan& p, const CdItems& tab, const float* prob, const float* tpl, const float* tskel, const double* coef, float* dprob,
             hipStream_t s) {
  hipLaunchKernelGGL((cldice_backward_kernel<KMAX>), dim3((unsigned)p.grid), dim3(CD_THREADS), 0, s, tab, p.geo, prob, tpl, tskel, coef, dprob);
}

}  // namespace

extern "C" long long uz_cldice_workspace_bytes(const uz_cldice_desc* d) {
  CdPlan p;
  if (cd_plan(d, "uz_cldice_workspace_bytes", &p) != UZ_OK) return -1;
  return p.bytes;
}

extern "C" int uz_cldice_grid(const uz_cldice_desc* d, int* units) {
  CdPlan p;
  const int rc = cd_plan(d, "uz_cldice_grid", &p);
  if (rc != UZ_OK) return rc;
  if (units) *units = p.geo.units;
  return p.grid;
}

extern "C" int uz_cldice_loss(const uz_cldice_desc* d, const uz_cldice_item* items, const void* target, const float* scales,
                              const float* base_loss, float* out, float* probs, float* skeleton, float* target_skeleton, void* workspace,
                              void* stream) {
  CdPlan p;
  const int rc = cd_plan(d, "uz_cldice_loss", &p);
  if (rc != UZ_OK) return rc;
  UZ_REQUIRE(items && target && scales && base_loss && out && probs && skeleton && target_skeleton && workspace, "uz_cldice_loss: null pointer");
  UZ_REQUIRE((((uintptr_t)target | (uintptr_t)scales | (uintptr_t)base_loss | (uintptr_t)out | (uintptr_t)probs | (uintptr_t)skeleton |
               (uintptr_t)target_skeleton) & 3) == 0,
             "uz_cldice_loss: tensors must be 4-byte aligned");
  UZ_REQUIRE(((uintptr_t)workspace & 15) == 0, "uz_cldice_loss: the workspace must be 16-byte aligned");
  const CdGeo& g = p.geo;
  const bool cls = d->mode == UZ_CLDICE_CLASS;
  const long long map_bytes = 4LL * g.E;
  // what the call writes (out, the three plane outputs, workspace, every dlogits) against everything else it touches
  UzRange in[3 + UZ_CLASS_MAX_ITEMS] = {uz_range(target, cls ? 4LL * g.pixels : map_bytes), uz_range(scales, 8), uz_range(base_loss, 4)};
  UzRange outr[5 + UZ_CLASS_MAX_ITEMS] = {uz_range(out, 8), uz_range(probs, map_bytes), uz_range(skeleton, map_bytes),
                                          uz_range(target_skeleton, map_bytes), uz_range(workspace, p.bytes)};
  int n_in = 3, n_out = 5;
  CdItems tab;
  bool any_grad;
  const int irc = uz_map_items("uz_cldice_loss", items, d->n_items, map_bytes, in, &n_in, outr, &n_out, &any_grad, tab.it);
  if (irc != UZ_OK) return irc;
  UZ_REQUIRE(!uz_any_overlap(outr, n_out, in, n_in), "uz_cldice_loss: tensors overlap");
  char* base = static_cast<char*>(workspace);
  float* prob = reinterpret_cast<float*>(base + p.off[CD_PROB]);
  float* tplw = reinterpret_cast<float*>(base + p.off[CD_TPL]);
  float* dprob = reinterpret_cast<float*>(base + p.off[CD_DPROB]);
  double* part = reinterpret_cast<double*>(base + p.off[CD_PART]);
  double* coef = reinterpret_cast<double*>(base + p.off[CD_COEF]);
  double* clv = reinterpret_cast<double*>(base + p.off[CD_CL]);
  const float* tpl = cls ? tplw : static_cast<const float*>(target);      // the target's planes
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 sblock(CD_PT), sgrid((unsigned)p.stream_grid);

  if (cls) hipLaunchKernelGGL(cldice_prob_class_kernel, sgrid, sblock, 0, s, tab, g, static_cast<const int*>(target), prob, probs, tplw);
  else hipLaunchKernelGGL(cldice_prob_binary_kernel, sgrid, sblock, 0, s, tab, g, prob, probs);
  UZ_LAUNCH_CHECK("uz_cldice_loss(prob)");
  // the kernels' LDS images are sized for the largest k of their instance: the smallest instance that holds k
  if (g.k <= 3) cd_tiles<3>(p, prob, tpl, target_skeleton, skeleton, part, s);
  else if (g.k <= 6) cd_tiles<6>(p, prob, tpl, target_skeleton, skeleton, part, s);
  else cd_tiles<UZ_CLDICE_MAX_ITERATIONS>(p, prob, tpl, target_skeleton, skeleton, part, s);
  UZ_LAUNCH_CHECK("uz_cldice_loss(forward)");
  hipLaunchKernelGGL(cldice_sums_kernel, dim3(1), sblock, 0, s, tab, g, (const double*)part, coef, clv, scales, base_loss, out);
  UZ_LAUNCH_CHECK("uz_cldice_loss(sums)");
  if (any_grad) {
    if (g.k <= 3) cd_back<3>(p, tab, prob, tpl, target_skeleton, coef, dprob, s);
    else if (g.k <= 6) cd_back<6>(p, tab, prob, tpl, target_skeleton, coef, dprob, s);
    else cd_back<UZ_CLDICE_MAX_ITERATIONS>(p, tab, prob, tpl, target_skeleton, coef, dprob, s);
    UZ_LAUNCH_CHECK("uz_cldice_loss(backward)");
    if (cls) hipLaunchKernelGGL(cldice_grad_class_kernel, sgrid, sblock, 0, s, tab, g, static_cast<const int*>(target), (const float*)prob, (const float*)dprob, scales);
    else hipLaunchKernelGGL(cldice_grad_binary_kernel, sgrid, sblock, 0, s, tab, g, (const float*)prob, (const float*)dprob, scales);
    UZ_LAUNCH_CHECK("uz_cldice_loss(grad)");
  }
  return UZ_OK;
}
