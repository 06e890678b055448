/*
 * unetzoo_hip.h — C ABI of libunetzoo_hip.so, the MI355X (gfx950) kernel library behind the
 * unet_zoo encoder/decoder hot path.
 *
 * The reference (irfanfadhullah/unet_zoo) has no FFI: every primitive below replaces an ATen op
 * that the reference reaches through torch.nn.  Each entry point cites
 * the reference call site it stands in for.  Conventions:
 *   - plain pointers + ints, no torch types, no allocation inside, no exceptions;
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (caller passes torch's current stream);
 *   - activations are NHWC ("pixel-major"): element (pixel p, channel c) of a tensor lives at
 *     base[p * ld + c]; `ld` (elements) lets a tensor be a channel slice of a wider buffer, which
 *     is how skip-concats are never materialised (reference: torch.cat, common_layers.py:115);
 *   - dtype: UZ_F32 = IEEE fp32 storage + exact-fp32 MFMA (parity mode),
 *            UZ_BF16 = bf16 storage + bf16 MFMA with fp32 accumulate (throughput mode);
 *   - return 0 on success, otherwise a negative UZ_E* code or a positive hipError_t;
 *     uz_last_error_string() describes the last failure on the calling thread.
 * All functions are re-entrant.  Process-global mutable state: the thread-local error string and ONE process-wide
 * setting, uz_set_cu_reserve() (an atomic the plans read when they size their grids; set it before planning or capturing).
 */
#ifndef UNETZOO_HIP_H
#define UNETZOO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UZ_ABI_VERSION 1

enum { UZ_F32 = 0, UZ_BF16 = 1 };

enum {
  UZ_OK = 0,
  UZ_EINVAL = -1,   /* bad shape / alignment / unsupported combination */
  UZ_ENOTIMPL = -2
};

/* tap geometry of an implicit-GEMM convolution */
enum {
  UZ_TAPS_CONV = 0,     /* ntaps = 1 (1x1) or 9 (3x3, dilation `dil`, zero padding `dil`) */
  UZ_TAPS_GATHER2X2 = 1, /* ntaps = 4: input pixel (2h+a, 2w+b), tap = 2a+b (ConvTranspose k2s2 dgrad) */
  UZ_TAPS_CONV_UP2 = 2,  /* 3x3 taps on the nearest-neighbour x2 upsampling of the input: the input tensor
                            lives at (H/2, W/2) and pixel (h, w) reads (h>>1, w>>1)
                            (nn.Upsample(scale_factor=2) + Conv2d, common_layers.py:69-72) */
  UZ_TAPS_CONV_S2 = 3    /* ntaps = 9: Conv2d(k3, stride 2, padding 1): output pixel (h, w) reads input pixel
                            (2h + ty - 1, 2w + tx - 1) of the (Hin, Win) grid, H = ceil(Hin / 2); zero outside
                            (ResidualConv, common_layers.py:188).  uz_conv_igemm: forward; uz_wgrad: weight gradient
                            (L = dy at (H, W), R = x at (Hr, Wr) = (Hin, Win)) */
};
enum {
  UZ_STORE_PLAIN = 0,    /* y[p*ldy + n] */
  UZ_STORE_SHUFFLE2X2 = 1 /* n = (2a+b)*Co + co  ->  y[pix(2h+a,2w+b)*ldy + co] (ConvTranspose k2s2 fwd) */
};

int uz_abi_version(void);
const char* uz_last_error_string(void);
/* Measurement hook (bench.py's per-launch profile, tools/): between uz_profile_arm(e0, e1) and uz_profile_disarm() the
 * kernel launches made by THIS thread through the library record the two hipEvent_t handles at the kernels' own begin
 * and end timestamps (first launch: both; later launches: the end event only), so hipEventElapsedTime(e0, e1) is the
 * duration from the first kernel's begin to the last kernel's end -- what a kernel trace reports, without the dispatch
 * latency that events recorded around a launch include.  Not to be armed during stream capture.  uz_profile_disarm()
 * returns the number of launches seen. */
int uz_profile_arm(void* start_event, void* stop_event);
int uz_profile_disarm(void);
/* 1 when the library was built with -DUZ_ABLATE (the measurement build of tools/kbench.py, whose kernels honour the
 * UZ_TUNE / UZ_ATTN_GX / UZ_WG_SPLIT environment switches), 0 for the shipped build, which never reads the
 * environment.  bench.py refuses to time an ablation build. */
int uz_build_ablate(void);
/* sha256 (hex) of the kernel sources the library was built from (csrc/Makefile: $(HASHED), concatenated in that order):
 * lets a test tell a stale build -- the library is a build artefact outside the repository's history. */
const char* uz_source_hash(void);
/* Hold `n` of the 256 CUs back from the library's persistent grids (0 <= n <= 128; default 0): the convolution, GEMM and
 * weight-gradient kernels run one 160 KB workgroup per CU, so a collective launched beside the backward (RCCL all-reduce
 * of a finished gradient span; reference seam unet_zoo/utils/multi_gpu.py:20-31) finds no CU to start on
 * until a kernel boundary.  With a reserve every plan sizes its grid -- and its statistics / slab partition, so call it
 * BEFORE querying *_grid_m / *_workspace_bytes -- for 256 - n CUs.  Process-wide; results stay equal up to the fp32
 * order of the per-workgroup partial sums.  uz_get_cu_reserve() returns the current value. */
/* Measurement: the shader clock this device holds under a dense bf16 MFMA stream (the quantity that sets every
 * MFMA-bound kernel's time and differs between devices -- MI355X_MICROARCH.md "DVFS give-back").  `workgroups` blocks of
 * 512 threads issue 8 * iters v_mfma_f32_16x16x32_bf16 per wave on random operands; block b writes
 * out_pairs[2 b] = shader cycles (s_memtime), out_pairs[2 b + 1] = 100 MHz ticks (s_memrealtime) of its loop
 * (uint64, device memory).  clock [GHz] = cycles / ticks / 10.  bench.py reports the median after a settling run. */
int uz_clock_probe(int iters, void* out_pairs, int workgroups, void* stream);
int uz_set_cu_reserve(int n);
int uz_get_cu_reserve(void);

/* ---------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution on the matrix cores.
 *   y[p, n] = bias[n] + sum_{tap, c} x[pix(p, tap), c] * w[n, tap*Cin + c]
 * Replaces: nn.Conv2d k3 p1 (common_layers.py:28,31,47,52,71; u2net.py:10 with dilation),
 *           nn.Conv2d k1 (attention_unet.py:11,18,25), their input-gradients (autograd, a19),
 *           nn.ConvTranspose2d k2 s2 forward and input-gradient (common_layers.py:104).
 * Optionally emits per-channel partial sums (sum, sum of squares) of the stored value for the
 * train-mode BatchNorm that follows (common_layers.py:29,32): stats_partial[g][0][n], [g][1][n]
 * for g < *grid_m as returned by uz_conv_igemm_grid_m(); reduced by uz_bn_finalize().
 * Requirements: Cin % (16/sizeof(T)*8) == 0 (bf16: 64, fp32: 32), K = ntaps*Cin,
 *               x, w, y 16-byte aligned, ldx % (16/sizeof(T)) == 0.
 * ------------------------------------------------------------------------------------------- */
typedef struct uz_conv_desc {
  int dtype;
  int N, H, W;     /* output pixel grid */
  int Hin, Win;    /* input pixel grid (== H, W for UZ_TAPS_CONV; 2H..2H+1, 2W..2W+1 for GATHER2X2) */
  int Cin, ldx;    /* channels per tap, input pixel stride */
  int Nout, ldy;   /* GEMM N (rows of w), output pixel stride */
  int ntaps, taps_mode, dil;
  int store_mode, Co; /* Co: channels per sub-pixel for UZ_STORE_SHUFFLE2X2 (Nout = 4*Co) */
  int Hout, Wout;     /* UZ_STORE_SHUFFLE2X2: pixel grid of the destination, 2H..2H+1 x 2W..2W+1 (0 = 2H, 2W).
                       * The 2H x 2W result lands at its top-left; UpSample_UNet's F.pad of an odd skip size
                       * (common_layers.py:110-113) leaves the last row / column to the caller (zeros). */
} uz_conv_desc;

int uz_conv_igemm_grid_m(const uz_conv_desc* d); /* number of stats partial rows; <0 on error */
/* Name of the kernel family the library's own plan picks for this descriptor (what uz_conv_igemm_ws() will launch;
 * `with_workspace` != 0: called with a workspace), e.g. "conv3x3_pp512_bf16", "conv3x3_pp256_bf16", "conv3x3_direct_bf16_bn128",
 * "conv3x3_direct_bf16_bn64_resident", "conv3x3_res64_bf16", "gemm_dma_bf16", "igemm_f32_128x64_tapsplit"; a "_up2"
 * suffix marks the nearest-upsampled input.  Measurement code (bench.py's per-family roofline) labels launches with
 * it instead of mirroring the plan.  Writes at most cap - 1 characters + NUL, returns the full length, < 0 on error. */
int uz_conv_igemm_kernel_name(const uz_conv_desc* d, int with_workspace, char* buf, int cap);
int uz_conv_igemm(const uz_conv_desc* d, const void* x, const void* w_packed, const float* bias,
                  void* y, float* stats_partial, void* stream);
/* y = conv(x) + bias + res: the same with an (M, ldres) tensor of the run dtype added in the epilogue (the result is
 * rounded to the run dtype before the addition, as a separate add of the stored tensor would): the residual sums
 * x + proj(.), tx + fc2(.) of a transformer block (missformer.py:266-267) and, in the backward, the sum of a tensor's
 * gradients when the last contribution is an input-gradient GEMM.  Problems of the LDS-DMA GEMM (1x1 / Linear, the
 * gather modes) with UZ_STORE_PLAIN; others: UZ_ENOTIMPL. */
int uz_conv_igemm_res(const uz_conv_desc* d, const void* x, const void* w_packed, const float* bias,
                      const void* res, int ldres, void* y, void* stream);
/* The same with the workspace of uz_conv_igemm_workspace_bytes() (may be NULL): products with few tiles and a long K loop
 * (Linear layers on the 8 x 8 / 16 x 16 token maps) then run split over K -- fp32 partial tiles, a fixed-order reduce pass
 * that adds bias and residual -- as uz_conv_igemm_ws does for the form without a residual. */
int uz_conv_igemm_res_ws(const uz_conv_desc* d, const void* x, const void* w_packed, const float* bias,
                         const void* res, int ldres, void* y, void* workspace, void* stream);
/* Same with a scratch buffer: small-M 3x3 problems on the generic kernel (u2net's dilated layers at
 * <= 32x32 maps, u2net.py:196-201) split their nine taps across workgroups into fp32 partial tiles in
 * `workspace` and finish with a fixed-order reduce + bias + statistics pass.  workspace_bytes() == 0:
 * identical to uz_conv_igemm (workspace may be NULL).  The statistics rows of THIS entry point are
 * counted by uz_conv_igemm_ws_grid_m().  The same entry serves the split-K form of the direct bf16 3x3 kernel: the
 * 16 x 16 / 32 x 32 bottleneck maps of a 256 x 256 input have 32 ... 128 tiles of 16 ... 32 channel slabs x nine taps, so
 * with a workspace the slabs of a tile are dealt to 2 ... 8 workgroups (fp32 partial tiles, the same reduce pass;
 * uz_conv_igemm_kernel_name(d, 1) then ends in "_splitk").  The split is sized by the hardware's CU count. */
long long uz_conv_igemm_workspace_bytes(const uz_conv_desc* d);
int uz_conv_igemm_ws_grid_m(const uz_conv_desc* d);
int uz_conv_igemm_ws(const uz_conv_desc* d, const void* x, const void* w_packed, const float* bias,
                     void* y, float* stats_partial, void* workspace, void* stream);
/* Input-gradient convolution with the first pass of the BatchNorm backward fused into its epilogue.
 * y = conv(x, w) is the gradient of an activation a = relu(bn(bn_y)) (common_layers.py:28-33: the Conv -> BN -> ReLU
 * whose output feeds only this convolution's forward).  Instead of the statistics of y the kernel writes, per
 * workgroup row of `partial` ([uz_conv_igemm_grid_m()][2][Nout], the layout of uz_bn_relu_bwd_reduce's
 * workspace), sum(dz) and sum(dz * xhat) over its pixels with dz = y * [scale * bn_y + shift > 0] (y as stored,
 * i.e. rounded to the tensor dtype) and xhat = (bn_y - mean) * invstd: uz_bn_bwd_finalize() then stands in for
 * uz_bn_relu_bwd_reduce() and the activation gradient is not read a second time.  bf16 problems of the direct 3x3
 * kernels whose epilogue is staged through LDS and of the LDS-DMA GEMM with UZ_STORE_PLAIN (the 2x2-gather input
 * gradient of ConvTranspose2d k2 s2, common_layers.py:104: the decoder blocks' last BatchNorm)
 * (uz_conv_igemm_bnred_supported() == 1); others: UZ_ENOTIMPL. */
int uz_conv_igemm_bnred_supported(const uz_conv_desc* d);
int uz_conv_igemm_bnred(const uz_conv_desc* d, const void* x, const void* w_packed, void* y, const void* bn_y,
                        int ld_bny, const float* scale, const float* shift, const float* mean, const float* invstd,
                        float* partial, void* stream);

/* Convolution that reads its input THROUGH the BatchNorm + ReLU in front of it (round 5): x holds the raw output of the
 * preceding convolution, the kernel computes y = conv(a, w) + bias with a = relu(x * in_scale[c] + in_shift[c]) formed
 * inside LDS on the halo patch (fp32 fma, rounded to the tensor dtype exactly as uz_bn_relu_apply would store it; zero
 * padding stays zero), so the normalised activation of a DoubleConv's first half (common_layers.py:28-33: Conv -> BN ->
 * ReLU -> Conv) is never written to or read from HBM.  Statistics rows as uz_conv_igemm (uz_conv_igemm_grid_m() rows).
 * bf16 3x3 problems of the direct ping-pong kernel whose LDS image leaves room for the channel table
 * (uz_conv_igemm_xf_supported() == 1); others: UZ_ENOTIMPL -- the caller then materialises the activation. */
int uz_conv_igemm_xf_supported(const uz_conv_desc* d);
int uz_conv_igemm_xf(const uz_conv_desc* d, const void* x, const float* in_scale, const float* in_shift,
                     const void* w_packed, const float* bias, void* y, float* stats_partial, void* stream);

/* Convolution with the eval-mode BatchNorm [+ ReLU] behind it formed in the epilogue: out_scale / out_shift are the constant
 * vectors of uz_bn_eval_scale(), known before the launch.  Per output element, from the fp32 accumulator:
 *   v = acc + bias[co];  a = fmaf(v, out_scale[co], out_shift[co]);  if (relu) a = max(a, 0);  y[p * ldy + co] = T(a)
 * -- uz_bn_relu_apply's expression on the UNROUNDED fp32 value, rounded once to the run dtype (fp32: bit-identical to
 * uz_conv_igemm + uz_bn_relu_apply; bf16: one rounding instead of two).  The raw convolution output is neither written nor
 * read back and no statistics rows are written.  ldy may exceed Nout (one half of a concat buffer): only [0, Nout) of a
 * pixel is touched.  Problems with UZ_STORE_PLAIN and UZ_TAPS_CONV / UZ_TAPS_CONV_UP2 that uz_conv_igemm plans on the direct
 * 3x3 kernels with a workgroup- or wave-wide staged epilogue (conv3x3_pp*, conv3x3_direct_*, both dtypes) or on the generic
 * kernel (igemm_*), without a split plan (uz_conv_igemm_bnact_supported() == 1); the split-K / tap-split plans, the
 * weights-in-registers kernel (conv3x3_res64_*), the LDS-DMA GEMM, the gather modes and the shuffle store: UZ_ENOTIMPL, no
 * launch -- the caller then runs uz_conv_igemm + uz_bn_relu_apply.  The refusal follows the PLAN of the descriptor, not how
 * the call is made: a problem that uz_conv_igemm_ws would split over a workspace is refused although the unsplit form of
 * the same kernel exists (it is the slower route for those shapes).  out_scale / out_shift: 16-byte aligned. */
int uz_conv_igemm_bnact_supported(const uz_conv_desc* d);
int uz_conv_igemm_bnact(const uz_conv_desc* d, const void* x, const void* w_packed, const float* bias,
                        const float* out_scale, const float* out_shift, int relu, void* y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Weight gradient (reduction over pixels), fp32 output in the reference's parameter layout.
 *   out[i, j, tap] (+)= sum_p L[p, i] * R[pix(p, tap), j]
 * conv k3/k1:  L = dy (i = c_out), R = x (j = c_in)   -> out is OIHW        (nn.Conv2d.weight)
 * convT k2s2:  L = x  (i = c_in),  R = dy (j = c_out) -> out is (Cin,Cout,2,2) (ConvTranspose2d.weight)
 * Replaces the weight-gradient half of autograd for the call sites above.
 * Two kernels: the pixel range is split over uz_wgrad_split() workgroup slices that each write an
 * fp32 partial slab into `workspace` (uz_wgrad_workspace_bytes() bytes, no initialisation
 * needed); a second kernel adds the slabs in fixed order and transposes into `out`
 * (deterministic, no atomics).
 * ------------------------------------------------------------------------------------------- */
typedef struct uz_wgrad_desc {
  int dtype;
  int N, H, W;     /* pixel grid of L */
  int Hr, Wr;      /* pixel grid of R */
  int Ci, ldl;     /* channels / pixel stride of L */
  int Cj, ldr;     /* channels / pixel stride of R */
  int ntaps, taps_mode, dil;
} uz_wgrad_desc;

int uz_wgrad_split(const uz_wgrad_desc* d);
long long uz_wgrad_workspace_bytes(const uz_wgrad_desc* d); /* <0 on error */
int uz_wgrad(const uz_wgrad_desc* d, const void* L, const void* R, float* out, void* workspace,
             void* stream);
/* The kernel family the library's plan launches for this descriptor, written to buf (labels of per-kernel measurements;
 * e.g. "wgrad9_bf16_128x64_rowwalk": nine taps per workgroup, uz_wgrad9.hip).  Returns the length, <0 on error. */
int uz_wgrad_kernel_name(const uz_wgrad_desc* d, char* buf, int cap);
/* The weight gradient of a convolution whose input was read through the BatchNorm + ReLU in front of it (uz_conv_igemm_xf):
 * R holds the RAW output of the preceding convolution; the kernel's loader waves form relu(R * r_scale[c] + r_shift[c]),
 * rounded to the tensor dtype as uz_bn_relu_apply would store it, inside the LDS ring (zero padding stays zero), so the
 * normalised activation of a DoubleConv's first half (common_layers.py:28-33) is not needed in the backward either.
 * Nine-tap bf16 problems of the row-walk kernel (uz_wgrad_xf_supported() == 1); others: UZ_ENOTIMPL.  phase: 0 = uz_wgrad's
 * two launches, 1 / 2 = as uz_wgrad_phase.  Workspace: uz_wgrad_workspace_bytes(). */
int uz_wgrad_xf_supported(const uz_wgrad_desc* d);
int uz_wgrad_xf(const uz_wgrad_desc* d, const void* L, const void* R, const float* r_scale, const float* r_shift,
                float* out, void* workspace, void* stream, int phase);
/* uz_wgrad in two calls, for per-kernel measurements (bench.py brackets each with its own event pair): phase 1 = the main
 * kernel (partial slabs into the workspace), phase 2 = the fixed-order slab reduction into `out`.  uz_wgrad == 1 then 2. */
int uz_wgrad_phase(const uz_wgrad_desc* d, const void* L, const void* R, float* out, void* workspace, void* stream,
                   int phase);
/* n independent problems, each exactly uz_wgrad(&items[i].desc, L, R, out, ...), issued together: the one-tap (nn.Linear)
 * problems of the bf16 run mode share launches -- one per tile shape and 24 problems, plus one reduction per 64 -- with the
 * pixel split planned for the whole set; every other problem runs through uz_wgrad.  The weight gradients of a model's
 * Linear layers (swin_unet_v2.py:205-240, missformer.py:148-214) are not needed before the optimizer step, so the host
 * defers them to the end of the backward pass.  Deterministic for a given set of items: each problem's pixel split -- and so
 * the order of its fp32 additions -- is a function of the set, not of timing.  A problem that is not split writes straight
 * into `out`.  Workspace: uz_wgrad_multi_workspace_bytes(), 256-byte aligned. */
typedef struct {
  uz_wgrad_desc desc;
  const void* L;
  const void* R;
  float* out;
} uz_wgrad_item;
long long uz_wgrad_multi_workspace_bytes(const uz_wgrad_item* items, int n); /* <0 on error */
int uz_wgrad_multi(const uz_wgrad_item* items, int n, void* workspace, void* stream);
/* `batch` independent one-tap problems of the shape `d` in one launch pair: problem b reads L + b * lb, R + b * rb
 * (strides in elements, multiples of 16 bytes) and writes out + b * ob floats -- the per-image products of the token
 * attention that contract over the rows of both operands (dV_b = A_b^T dO_b, dK_b = dS_b^T Q_b,
 * unet_transformer.py:133-136; the channel Gram matrix x_b^T x_b of transatt_unet.py:93-101).  The pixel split is
 * planned for the whole batch. */
long long uz_wgrad_batched_workspace_bytes(const uz_wgrad_desc* d, int batch);
int uz_wgrad_batched(const uz_wgrad_desc* d, int batch, const void* L, long long lb, const void* R, long long rb,
                     float* out, long long ob, void* workspace, void* stream);
/* The same with a second batch level: batch * batch2 problems, problem (b, h) reads L + b * lb + h * lb2, R + b * rb +
 * h * rb2 and writes out + (b * batch2 + h) * ob (the scores Q_h^T K_h of every (image, head), uctransnet.py:160-168). */
int uz_wgrad_batched2(const uz_wgrad_desc* d, int batch, int batch2, const void* L, long long lb, long long lb2, const void* R,
                      long long rb, long long rb2, float* out, long long ob, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The network's first convolution as direct kernels (bf16 run mode; uz_conv_first.hip): nn.Conv2d(C <= 3, Cout in {32, 64},
 * k3, p1) on the fp32 NCHW input image (reference: the first layer of every UNet-family model, common_layers.py:28 reached
 * from unet.py:15; attention_unet.py:11; u2net.py:30) -- no im2col buffer.
 *   fwd:   y[p][co] (bf16 NHWC, pixel stride ldy) = bias[co] + sum_{c,ty,tx} w[co][c][ty][tx] x[n][c][h+ty-1][w+tx-1], x and w
 *          rounded to bf16 (what the im2col path stored), fp32 accumulation, one rounding; stats (nullable):
 *          uz_conv3x3_first_rows(N, H, W) partial rows [row][2][Cout] of sum / sum of squares of the STORED values
 *          (uz_bn_finalize reads them).
 *   wgrad: dw[co][c][ty][tx] (fp32, the parameter's own layout) = sum_p dy[p][co] x[n][c][h+ty-1][w+tx-1]; workspace of
 *          uz_conv3x3_first_wgrad_workspace_bytes() for the workgroups' partial slabs (fixed-order reduction).
 * ------------------------------------------------------------------------------------------- */
int uz_conv3x3_first_supported(int dtype, int C, int Cout);
int uz_conv3x3_first_rows(int N, int H, int W);
int uz_conv3x3_first_fwd(int dtype, const float* x, int N, int C, int H, int W, const float* w, const float* bias, int Cout,
                         void* y, int ldy, float* stats, void* stream);
/* uz_conv3x3_first_fwd with the eval-mode BatchNorm [+ ReLU] in the epilogue (the semantics of uz_conv_igemm_bnact); no
 * statistics. */
int uz_conv3x3_first_fwd_bnact(int dtype, const float* x, int N, int C, int H, int W, const float* w, const float* bias,
                               int Cout, const float* out_scale, const float* out_shift, int relu, void* y, int ldy,
                               void* stream);
long long uz_conv3x3_first_wgrad_workspace_bytes(int N, int H, int W, int Cout);
int uz_conv3x3_first_wgrad(int dtype, const float* x, int N, int C, int H, int W, const void* dy, int lddy, int Cout, float* dw,
                           void* workspace, void* stream);
/* uz_conv3x3_first_wgrad reading its dy THROUGH the BatchNorm + ReLU backward of the layer (training, no pool, no residual):
 * the image needs no input gradient, so the weight gradient is the only reader of that dy and forms it where it fills its
 * tile, from the gradient g of the activation and the raw convolution output y (both bf16 NHWC), the four BatchNorm vectors
 * and the totals sums[2][C] of uz_bn_bwd_finalize, with the expressions of uz_bn_relu_bwd_apply, rounded to bf16:
 *   k0 = (float)(sums[0][c] / count), k1 = (float)(sums[1][c] / count), dz = fma(y, scale, shift) > 0 ? g : 0,
 *   dy = bf16(scale * (dz - k0 - (y - mean) * invstd * k1)).
 * Same workspace and reduction: dw is bitwise that of uz_bn_relu_bwd_apply + uz_conv3x3_first_wgrad. */
int uz_conv3x3_first_wgrad_bn(int dtype, const float* x, int N, int C, int H, int W, const void* g, int ldg, const void* y,
                              int ldy, const float* scale, const float* shift, const float* mean, const float* invstd,
                              const double* sums, double count, int Cout, float* dw, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Weight re-packing: fp32 master parameters in the reference layout -> kernel layout in run dtype.
 *   UZ_PACK_CONV_FWD : w[Co][Ci][T] (OIHW)     -> dst[Co][t*Ci + ci]
 *   UZ_PACK_CONV_DGRAD: w[Co][Ci][T]           -> dst[Ci][(T-1-t)*Co + co]   (flipped taps)
 *   UZ_PACK_CONVT_FWD : w[Ci][Co][4]           -> dst[t*Co + co][ci]
 *   UZ_PACK_CONVT_DGRAD: w[Ci][Co][4]          -> dst[ci][t*Co + co]
 *   UZ_PACK_IM2COL    : w[Co][Ci][T], K=T*Ci   -> dst[Co][Kpad], k = t*Ci + ci, zero padded
 *   UZ_PACK_VEC_REPEAT: v[Co] (Ci = 1)         -> dst[t*Co + c] = v[c], t < T, dst stays FP32 whatever `dtype` (the bias of
 *                       nn.ConvTranspose2d k2 s2 for each of the four sub-pixels of the pixel-shuffle store,
 *                       common_layers.py:104; batched form only: a model's four repeats ride in the weights' launch)
 * ------------------------------------------------------------------------------------------- */
enum { UZ_PACK_CONV_FWD = 0, UZ_PACK_CONV_DGRAD = 1, UZ_PACK_CONVT_FWD = 2, UZ_PACK_CONVT_DGRAD = 3,
       UZ_PACK_IM2COL = 4, UZ_PACK_VEC_REPEAT = 5 };
int uz_pack_weights(int dtype, int mode, const float* w, int Co, int Ci, int T, int Kpad, void* dst,
                    void* stream);
/* The same for a whole model in one launch: `items_device` is a device array of n_items entries
 * sorted by `begin` = number of destination elements of all earlier entries; total_elements = sum. */
typedef struct uz_pack_item {
  const float* src;
  void* dst;
  long long begin;
  int mode, Co, Ci, T, Kpad;
  int pad_;
} uz_pack_item;
int uz_pack_weights_batched(int dtype, const uz_pack_item* items_device, int n_items,
                            long long total_elements, void* stream);
/* 3x3 convolution weights (Co, Ci multiples of 32): forward AND input-gradient layouts from one
 * coalesced read of the OIHW tensor; either destination may be NULL. */
typedef struct uz_pack3x3_item {
  const float* src;
  void* dst_fwd;    /* [Co][t*Ci + ci]        (UZ_PACK_CONV_FWD)   */
  void* dst_dgrad;  /* [Ci][(8-t)*Co + co]    (UZ_PACK_CONV_DGRAD) */
  int Co, Ci;
  int tile_begin;   /* number of 32x32 (co, ci) tiles of all earlier items */
  int pad_;
} uz_pack3x3_item;
int uz_pack_conv3x3_batched(int dtype, const uz_pack3x3_item* items_device, int n_items, int total_tiles,
                            void* stream);

/* im2col of a small-channel NCHW fp32 input (the network input, unet.py:31 first conv):
 *   dst[p][t*C + c] = x[n, c, h+dy, w+dx] (zero padded), dst row length Kpad, k >= 9C zero. */
int uz_im2col3x3_nchw(int dtype, const float* x_nchw, int N, int C, int H, int W, int Kpad, void* dst,
                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * BatchNorm2d (train): finalize statistics.  nn.BatchNorm2d, common_layers.py:29,32.
 *   mean = S1/count, var = S2/count - mean^2 (biased), invstd = 1/sqrt(var+eps)
 *   scale = gamma*invstd, shift = beta - mean*scale
 *   running_mean = (1-m)*rm + m*mean ; running_var = (1-m)*rv + m*var*count/(count-1)
 * stats_partial as written by uz_conv_igemm ([grid_m][2][C]).
 * ------------------------------------------------------------------------------------------- */
int uz_bn_finalize(const float* stats_partial, int grid_m, int C, double count, const float* gamma,
                   const float* beta, float eps, float momentum, float* running_mean,
                   float* running_var, float* scale, float* shift, float* mean, float* invstd,
                   void* stream);
/* eval mode: scale/shift from running statistics (SURVEY §2.3 "BatchNorm2d (eval)") */
int uz_bn_eval_scale(int C, const float* gamma, const float* beta, const float* running_mean,
                     const float* running_var, float eps, float* scale, float* shift, void* stream);

/* act = relu(scale*y + shift) written to `act` (ld = lda), and optionally its MaxPool2d(2,2)
 * (floor mode; common_layers.py:90) to `pooled`.  BN-apply + ReLU + pool in one pass. */
int uz_bn_relu_apply(int dtype, const void* y, int ldy, const float* scale, const float* shift,
                     int N, int H, int W, int C, void* act, int lda, void* pooled, int ldp,
                     void* stream);
/* Same with a residual: act = relu(scale*y + shift) + res, pooled = MaxPool2d(2,2)(act).
 * Replaces the RSU block tail `hx1d + hxin` (u2net.py:74,119,157,188,213) and the stage pools
 * (u2net.py:221-229).  res == NULL is uz_bn_relu_apply. */
int uz_bn_relu_add_apply(int dtype, const void* y, int ldy, const float* scale, const float* shift,
                         int N, int H, int W, int C, const void* res, int ldr, void* act, int lda,
                         void* pooled, int ldp, int pool_ceil, void* stream);
/* uz_bn_finalize + uz_bn_relu_add_apply in ONE launch (training forward of Conv -> BatchNorm -> ReLU, common_layers.py:28-33):
 * the first workgroups of the element pass sum the `rows` partial rows (same order as uz_bn_finalize: the same bits), write
 * vec = [scale | shift | mean | invstd] (4 C floats) and the running statistics, and release a flag the other workgroups wait
 * for before they read scale / shift.  *flag must be 0 at launch (one int per call, the caller clears its flag arena once per
 * step) and is left at the number of finalizing workgroups.  Where the grid is smaller than the finalize (a few pixels, many
 * channels) the two launches are issued instead and the flag is not touched. */
int uz_bn_relu_add_apply_fin(int dtype, const void* y, int ldy, const float* stats_partial, int rows, double count,
                             const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                             float* running_var, float* vec, int* flag, int N, int H, int W, int C, const void* res, int ldr,
                             void* act, int lda, void* pooled, int ldp, int pool_ceil, void* stream);
/* pool_ceil bit 0 = 1: pooled is (N, ceil(H/2), ceil(W/2), C), border windows clipped (ceil_mode=True, u2net.py:30);
 * bit 0 = 0: pooled is (N, H/2, W/2, C), an odd last row / column is not pooled (MaxPool2d default); bit 1: BatchNorm without
 * the ReLU; bit 2: the pass walks the tensor from its end (see uz_bnbwd_desc.pool_ceil; identical output). */

/* Backward of (BN train -> ReLU [-> MaxPool2d(2,2)]) in two passes.
 * The gradient arriving at the activation is
 *     g = g0[p] + g1[p] + (p is the first max of its 2x2 window ? gpool[window] : 0)
 * (any of g0/g1/gpool may be NULL).  Pass 1 (uz_bn_relu_bwd_reduce) writes one partial row per
 * workgroup into `workspace` (uz_bn_relu_bwd_workspace_bytes() bytes), then a finalize kernel
 * sums the rows in fixed order into sums[0][c] = sum g*mask, sums[1][c] = sum g*mask*xhat
 * (double) and dbeta = sums[0], dgamma = sums[1] (fp32; may be NULL).  Pass 2 writes
 *     dy = scale * (g*mask - sums0/count - xhat*sums1/count). */
typedef struct uz_bnbwd_desc {
  int dtype;
  int N, H, W, C;
  int ldy, ldg0, ldg1, ldgp, lddy;
  int pool_ceil; /* bit 0: geometry of gpool: 1 = (ceil(H/2), ceil(W/2)) with clipped border windows, 0 = (H/2, W/2);
                  * bit 1: the forward was BatchNorm WITHOUT ReLU (uz_bn_relu_add_apply with the same bit); with unit
                  * scale and zero shift that pair is a stand-alone MaxPool2d(2) of an arbitrary tensor
                  * (unet_transformer.py:151);
                  * bit 2: walk the tensors from their END (same values; the part the producing kernel wrote last is what
                  * the 256 MB Infinity Cache still holds -- a pass after a convolution runs 15 % faster that way; the
                  * partial rows of pass 1 then belong to other pixel groups, so the fp32 totals differ in the last bits
                  * between the two walks, each walk being deterministic) */
} uz_bnbwd_desc;
/* Statistics of a BatchNorm whose input is not a convolution output (pre-activation blocks, `ResidualConv`,
 * common_layers.py:186-187): per-channel sum and sum of squares of x (P pixels, C channels, row stride ld) as
 * partial rows [uz_colstats_rows()][2][C], the layout uz_bn_finalize() reads. */
int uz_colstats_rows(int dtype, int P, int C);
int uz_colstats(int dtype, const void* x, int ld, int P, int C, float* partial, void* stream);
long long uz_bn_relu_bwd_workspace_bytes(const uz_bnbwd_desc* d, int has_pool_grad);
int uz_bn_relu_bwd_reduce(const uz_bnbwd_desc* d, const void* y, const float* scale,
                          const float* shift, const float* mean, const float* invstd, const void* g0,
                          const void* g1, const void* gpool, void* workspace, double* sums,
                          float* dgamma, float* dbeta, void* stream);
int uz_bn_relu_bwd_apply(const uz_bnbwd_desc* d, const void* y, const float* scale,
                         const float* shift, const float* mean, const float* invstd, const void* g0,
                         const void* g1, const void* gpool, const double* sums, double count,
                         void* dy, void* stream);
/* Pass 1 alone: the partial rows [rows][2][C] into `workspace`, rows = uz_bn_relu_bwd_workspace_bytes() / (8 C); and
 * uz_bn_bwd_finalize + uz_bn_relu_bwd_apply in ONE launch over such rows (from uz_bn_relu_bwd_reduce_rows, uz_conv_igemm_bnred
 * or uz_outconv_bwd_bnred): the flag protocol of uz_bn_relu_add_apply_fin; sums / dgamma / dbeta are written as by
 * uz_bn_bwd_finalize (same order of additions). */
int uz_bn_relu_bwd_reduce_rows(const uz_bnbwd_desc* d, const void* y, const float* scale, const float* shift,
                               const float* mean, const float* invstd, const void* g0, const void* g1, const void* gpool,
                               void* workspace, void* stream);
int uz_bn_relu_bwd_apply_fin(const uz_bnbwd_desc* d, const void* y, const float* scale, const float* shift,
                             const float* mean, const float* invstd, const void* g0, const void* g1, const void* gpool,
                             const float* partial, int rows, double* sums, float* dgamma, float* dbeta, int* flag,
                             double count, void* dy, void* stream);
/* The finalize half of uz_bn_relu_bwd_reduce() alone: sums[2][C] (double), dbeta = sums[0], dgamma = sums[1] from
 * `rows` partial rows [rows][2][C] written by uz_conv_igemm_bnred(). */
int uz_bn_bwd_finalize(const float* partial, int rows, int C, double* sums, float* dgamma, float* dbeta, void* stream);
/* uz_bn_relu_bwd_apply for the block in front of the 1x1 head when its gradient was never written down (bf16, ReLU, no pool;
 * uz_outconv_bwd_bnred with dx == NULL): the gradient of pixel p, channel c is formed from the logit gradients g (fp32 NKHW)
 * and the head's weights w[Kout][C] as the head would have stored it -- d = 0; d = fmaf(g[n][k][hw], w[k][c], d) for
 * ascending k; bf16(d) -- and enters the expressions of the apply pass unchanged: same dy, bit for bit, as the two launches.
 * d->pool_ceil: bit 2 (walk from the end) only; ldg0 / ldg1 / ldgp unused. */
int uz_bn_relu_bwd_apply_head_supported(int dtype, int C, int Kout);
int uz_bn_relu_bwd_apply_head(const uz_bnbwd_desc* d, const void* y, const float* scale, const float* shift, const float* mean,
                              const float* invstd, const float* g_nchw, const float* w, int Kout, const double* sums,
                              double count, void* dy, void* stream);

/* 1x1 convolution with few outputs (OutConv, common_layers.py:125), NCHW fp32 logits.
 *   out[n, k, h, w] = b[k] + sum_c x[p, c] * w[k, c],  k < Kout <= 8 */
int uz_outconv_fwd(int dtype, const void* x, int ldx, int N, int HW, int C, const float* w,
                   const float* b, int Kout, float* out_nchw, void* stream);
/* uz_outconv_fwd on the RAW output y of the convolution in front, read through that layer's BatchNorm + ReLU (bf16):
 *   x[p, c] = bf16(max(fma(y[p, c], scale[c], shift[c]), 0))   -- the value uz_bn_relu_apply() would have stored --
 * so the normalised activation of the last decoder block (DoubleConv's second half, common_layers.py:31-33, feeding OutConv,
 * :125) is never written down; its backward is uz_outconv_bwd_bnred(x = NULL). */
int uz_outconv_fwd_xf(int dtype, const void* y, int ldy, int N, int HW, int C, const float* scale, const float* shift,
                      const float* w, const float* b, int Kout, float* out_nchw, void* stream);
/* dx[p,c] = sum_k g[n,k,hw] * w[k,c];  dw[k,c] = sum_p g*x;  db[k] = sum_p g.
 * Two kernels (per-workgroup partial rows in `workspace`, then a fixed-order sum): deterministic. */
long long uz_outconv_bwd_workspace_bytes(int dtype, int N, int HW, int C, int Kout);
int uz_outconv_bwd(int dtype, const void* x, int ldx, int N, int HW, int C, const float* w, int Kout,
                   const float* g_nchw, void* dx, int lddx, float* dw, float* db, void* workspace,
                   void* stream);
/* uz_outconv_bwd with the first pass of a BatchNorm backward in the same pass over the pixels (bf16): x = relu(bn(bn_y))
 * feeds only this head, so the gradient dx it writes is the whole gradient of that activation; bn_partial receives
 * [uz_outconv_bwd_rows()][2][C] partial rows for uz_bn_bwd_finalize() (see uz_conv_igemm_bnred).  x == NULL: the
 * activation was never written down (uz_outconv_fwd_xf); the kernel forms it from bn_y, scale, shift (ldx unused).
 * dx == NULL: the gradient is not stored (its reader forms it: uz_bn_relu_bwd_apply_head); dw, db and the rows as before. */
int uz_outconv_bwd_rows(int dtype, int N, int HW, int C);
int uz_outconv_bwd_bnred(int dtype, const void* x, int ldx, int N, int HW, int C, const float* w, int Kout,
                         const float* g_nchw, void* dx, int lddx, float* dw, float* db, void* workspace,
                         const void* bn_y, int ld_bny, const float* scale, const float* shift, const float* mean,
                         const float* invstd, float* bn_partial, void* stream);

/* The wide 1x1 head (uz_head_wide.hip): the same three products for K = 1..32 classes as a skinny matrix product on the
 * fp32-input MFMA -- exact fp32 products, fp32 accumulation for bf16 and fp32 activations alike (bf16 is widened in registers;
 * w and g are never rounded), i.e. the arithmetic class of uz_outconv_* in another order of additions.
 *   x: NHWC, P = N * HW pixels, C channels, row stride ldx >= C, 16-byte aligned rows;  w: (K, C) fp32;  b: (K) fp32;
 *   out, g: (N, K, HW) fp32 planes;  dx: T with row stride lddx, NULL = not wanted;  dw: (K, C);  db: (K).
 * uz_head_wide_supported: 1 for bf16 / fp32, C % VEC == 0 (8 / 4), C <= 512, 1 <= K <= 32.
 * uz_head_wide_grid: the workgroups of the forward's walk over 256-pixel tiles.  It is sized from the hardware's CU count,
 * never from uz_set_cu_reserve(), and so is the backward's (workspace bytes / (4 K (C + 1)) partial rows): the order of the
 * additions is a function of the shape alone, the results are bit-identical from call to call (no atomics).
 * UZ_EINVAL with a message before any launch: N * HW >= 2^31, a null required pointer, ldx < C, K or C out of range. */
int uz_head_wide_supported(int dtype, int C, int K);
int uz_head_wide_grid(int dtype, int N, int HW, int C, int K);
int uz_head_wide_fwd(int dtype, const void* x, int ldx, int N, int HW, int C, const float* w, const float* b, int K,
                     float* out, void* stream);
long long uz_head_wide_bwd_workspace_bytes(int dtype, int N, int HW, int C, int K);
int uz_head_wide_bwd(int dtype, const void* x, int ldx, int N, int HW, int C, const float* w, int K, const float* g,
                     void* dx, int lddx, float* dw, float* db, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Additive attention gate (AttentionBlock.forward, attention_unet.py:34-40), everything except the
 * two 1x1 convolutions W_g / W_x (those are uz_conv_igemm with statistics):
 *   q[p]   = b_psi + sum_c relu(bn_g(g1raw) + bn_x(x1raw))[p,c] * w_psi[c]      uz_attn_psi_fwd
 *   out    = x * sigmoid(bn_q(q))                                               uz_attn_gate_fwd
 * and the backward chain (see uz_attn.hip).  vec_* are the [4][channels] (scale, shift, mean,
 * invstd) rows produced by uz_bn_finalize; partial buffers hold uz_attn_grid() rows.
 * ------------------------------------------------------------------------------------------- */
int uz_attn_grid(int dtype, int P, int channels);
int uz_attn_psi_fwd(int dtype, const void* g1raw, int ldg, const void* x1raw, int ldx, const float* vec_g,
                    const float* vec_x, const float* wpsi, const float* bpsi /* device, may be NULL */,
                    int P, int F, float* q, float* partial /* [grid(F)][2] */, void* stream);
int uz_attn_gate_fwd(int dtype, const void* x, int ldx, const float* q, const float* vec_q, int P, int C,
                     void* out, int ldo, void* stream);
int uz_attn_bwd_psi(int dtype, const void* dout, int ldd, const void* x, int ldx, const float* q,
                    const float* vec_q, int P, int C, void* dx_direct, int lddx, float* dz,
                    float* partial /* [grid(C)][2] */, void* stream);
int uz_attn_bwd_reduce(int dtype, const void* g1raw, int ldg, const void* x1raw, int ldx, const float* q,
                       const float* dz, const float* wpsi, const float* vec_g, const float* vec_x,
                       const float* vec_q, const double* a01, int P, int F,
                       float* partial /* [grid(F)][4F+1] */, void* stream);
int uz_attn_bwd_apply(int dtype, const void* g1raw, int ldg, const void* x1raw, int ldx, const float* q,
                      const float* dz, const float* wpsi, const float* vec_g, const float* vec_x,
                      const float* vec_q, const double* a01, const double* totals, int P, int F,
                      void* dg1raw, int lddg, void* dx1raw, int lddx, void* stream);
/* out[e] (double) = sum over rows of partial[row][e] */
int uz_sum_rows(const float* partial, int rows, int n, double* out, void* stream);
/* the same sums (accumulated in double) rounded to fp32 and written where they are wanted: elements
 * [0, n0) to out0, [n0, n) to out1 (NULL when n0 == n) -- e.g. the two halves of uz_layernorm_bwd()'s
 * rows straight into the gradient tensors of weight and bias */
int uz_sum_rows_f32(const float* partial, int rows, int n, float* out0, int n0, float* out1, void* stream);
/* ... of the first n columns of rows that are ld >= n floats apart (a column window of wider partial rows) */
int uz_sum_rows_f32_ld(const float* partial, int ld, int rows, int n, float* out0, int n0, float* out1,
                       void* stream);
/* backward of nearest x2 upsampling: dx[coarse pixel] = sum of its 2x2 fine pixels (H, W coarse) */
int uz_sum2x2(int dtype, const void* du, int ldu, int N, int H, int W, int C, void* dx, int lddx,
              void* stream);

/* ---------------------------------------------------------------------------------------------
 * U^2-Net pieces (reference: unet_zoo/models/u2net.py).
 * ------------------------------------------------------------------------------------------- */
/* F.interpolate(mode='bilinear', align_corners=False, size=(Ho, Wo)) (u2net.py:19-22).
 * Element (n, h, w, c) of x lives at x[n*x_img_stride + (h*Wi + w)*ldx + c] (strides in elements),
 * likewise y: NHWC activations (ld = channel count of the holding buffer) and NCHW 1-channel logit
 * planes (ld = 1, C = 1) go through the same entry point. */
int uz_bilinear_fwd(int dtype, const void* x, int ldx, long long x_img_stride, int N, int Hi, int Wi,
                    int C, void* y, int ldy, long long y_img_stride, int Ho, int Wo, void* stream);
/* its backward: g at (Ho, Wo) -> dx at (Hi, Wi), overwritten (gather form, deterministic) */
int uz_bilinear_bwd(int dtype, const void* g, int ldg, long long g_img_stride, int N, int Hi, int Wi,
                    int C, void* dx, int lddx, long long dx_img_stride, int Ho, int Wo, void* stream);
/* the same pair with the align_corners switch of F.interpolate / nn.Upsample (align_corners != 0:
 * nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True), nested_unet.py:32) */
int uz_resize_bilinear_fwd(int dtype, const void* x, int ldx, long long x_img_stride, int N, int Hi, int Wi,
                           int C, void* y, int ldy, long long y_img_stride, int Ho, int Wo, int align_corners,
                           void* stream);
int uz_resize_bilinear_bwd(int dtype, const void* g, int ldg, long long g_img_stride, int N, int Hi, int Wi,
                           int C, void* dx, int lddx, long long dx_img_stride, int Ho, int Wo, int align_corners,
                           void* stream);
/* Pixel-grid moves of NHWC tensors (row strides lds / ldd in elements, C channels):
 *   mode 0 copy (a tensor into its slot of a concat buffer: UNet++'s dense skips, nested_unet.py:80-93),
 *   mode 1 dst[h, w] = src[2h, 2w]  (Hd = ceil(Hs/2): what a stride-2 convolution keeps or reads),
 *   mode 2 dst[h, w] = (h, w even) ? src[h/2, w/2] : 0  (Hs = ceil(Hd/2): that selection's gradient). */
int uz_resample2(int dtype, const void* src, int lds, int N, int Hs, int Ws, int C, void* dst, int ldd, int Hd,
                 int Wd, int mode, void* stream);
/* out = g0 + g1 + unpool(gp): total gradient of `act` consumed directly (g0, g1 may be NULL) and through
 * MaxPool2d(2,2) (gp at (H/2, W/2), routed to the first maximum of each window as ATen does). */
int uz_pool_grad_combine(int dtype, int N, int H, int W, int C, const void* act, int lda, const void* g0,
                         int ldg0, const void* g1, int ldg1, const void* gp, int ldgp, void* out, int ldo,
                         int pool_ceil, void* stream);
/* Side head Conv2d(C, 1, 3, padding=1) (u2net.py:238-243): x NHWC, w = the (1, C, 3, 3) fp32 parameter,
 * bias 1 value or NULL, out[n*out_img_stride + h*W + w] fp32; taps_ws: N*9*H*W floats of scratch. */
int uz_sideconv3x3_fwd(int dtype, const void* x, int ldx, int N, int H, int W, int C, const float* w,
                       const float* bias, float* taps_ws, float* out, long long out_img_stride,
                       void* stream);
long long uz_sideconv3x3_bwd_workspace_bytes(int dtype, int N, int H, int W, int C);
/* g[n*g_img_stride + hw] = d(loss)/d(out); dx (NHWC, may be NULL), dw (1, C, 3, 3), db (1 value or NULL) */
int uz_sideconv3x3_bwd(int dtype, const void* x, int ldx, int N, int H, int W, int C, const float* w,
                       const float* g, long long g_img_stride, void* dx, int lddx, float* dw, float* db,
                       void* workspace, void* stream);
/* Fuse conv Conv2d(Cc, K, 1) on the NCHW fp32 concat d (N, Cc, HW) of the side maps (u2net.py:244,288) */
int uz_fuse1x1_fwd(const float* d, int N, int HW, int Cc, int K, const float* w, const float* b,
                   float* out, void* stream);
long long uz_fuse1x1_bwd_workspace_bytes(int N, int HW, int Cc, int K);
/* dcat = W^T g (+ g_extra[s] added onto channels [s*K, (s+1)*K): the gradients that arrive at the
 * side outputs themselves; host array of n_extra = Cc/K device pointers, entries may be NULL; n_extra
 * may be 0), dw (K, Cc), db (K).  g == NULL: only the extras flow, dw = db = 0. */
int uz_fuse1x1_bwd(const float* d, int N, int HW, int Cc, int K, const float* w, const float* g,
                   const float* const* g_extra, int n_extra, float* dcat, float* dw, float* db,
                   void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Swin-UNet V2 pieces (reference: unet_zoo/models/swin_unet_v2.py).  Tokens are NHWC activations:
 * row = (image, h, w) on the token grid, C channels.  nn.Linear runs on uz_conv_igemm (ntaps = 1).
 * ------------------------------------------------------------------------------------------- */
/* PatchEmbed's Conv2d(kernel = stride = patch) input (swin_unet_v2.py:548-556):
 * out[(b,i,j)][(kh*patch + kw)*C + c] = x[b][c][i*patch+kh][j*patch+kw], zero up to Kpad. */
int uz_patchify(int dtype, const float* x_nchw, int N, int C, int H, int W, int patch, int Kpad,
                void* out, void* stream);

/* nn.LayerNorm over C of an (N, Ho, Wo, C) token tensor.  mode selects how an output token's input
 * row is addressed (the reference's permutations, never materialised):
 *   UZ_LN_PLAIN   x[token][c]
 *   UZ_LN_MERGE   PatchMerging (:315-332): input grid (2Ho, 2Wo) with C/4 channels; channel segment
 *                 s = c/(C/4) of output token (i, j) is input token (2i + (s&1), 2j + (s>>1))
 *   UZ_LN_EXPAND  PatchExpand / FinalPatchExpand_X4 (:352-362, :375-387): input grid (Ho/r, Wo/r) with
 *                 r*r*C channels; output token (h*r+p1, w*r+p2) reads channels (p1*r+p2)*C + c
 * y = [res +] [image_scale[image] *] LN(x): the block tail shortcut + drop_path(norm1(.)) (:264-267).
 * stats: (P_out, 2) fp32 mean / rstd, kept for the backward. */
enum { UZ_LN_PLAIN = 0, UZ_LN_MERGE = 1, UZ_LN_EXPAND = 2 };
typedef struct uz_ln_desc {
  int dtype, N, Ho, Wo, C;
  int ldx, ldy, ldr, ldg, lddx; /* row strides (elements) of x, y, res, g (grad of y), dx */
  int mode, r;
  float eps;
  int act; /* 0: none; 1: exact GELU applied to the result (MixFFN_skip's act(norm1(.)), missformer.py:206;
              no residual / image scale; backward through uz_layernorm_act_bwd) */
} uz_ln_desc;
/* (every entry of this family: gamma / beta are read with 16-byte loads, stats -- (mean, rstd) pairs -- with 8-byte accesses:
 * 16- / 8-byte aligned pointers) */
int uz_layernorm_fwd(const uz_ln_desc* d, const void* x, const float* gamma, const float* beta,
                     const void* res, const float* image_scale, void* y, float* stats, void* stream);
int uz_layernorm_bwd_rows(const uz_ln_desc* d); /* rows of `partial`; <0 on error */
/* dx (addressed like x; every input element is written exactly once) and per-workgroup partial rows
 * partial[row][2][C] = sums of g*xhat (-> dgamma) and g (-> dbeta), g already scaled by image_scale;
 * add the rows with uz_sum_rows().  The residual branch's gradient is g itself. */
int uz_layernorm_bwd(const uz_ln_desc* d, const void* x, const float* gamma, const float* stats,
                     const void* g, const float* image_scale, void* dx, float* partial, void* stream);
/* the same for act = 1: g is the gradient of GELU(LayerNorm(x)); beta rebuilds the pre-activation */
int uz_layernorm_act_bwd(const uz_ln_desc* d, const void* x, const float* gamma, const float* beta,
                         const float* stats, const void* g, void* dx, float* partial, void* stream);
/* LayerNorm followed by a 1x1 head (FinalPatchExpand_X4's norm + the `output` convolution of swin_unet_v2,
 * swin_unet_v2.py:385, :690, :753) without materialising the normalised tensor: logits (N, K, Ho, Wo) fp32 =
 * b[k] + sum_c w[k][c] LN(x)[token][c] with x addressed as in uz_layernorm_fwd (d->ldy / ldr / ldg unused),
 * K <= 4 (K = 1: C <= 192 sixteen-byte chunks, else 64).  Backward from dlogits: dx with x's addressing (lddx)
 * and the gradients of gamma, beta (C), w (K, C), b (K; may be NULL), overwritten. */
int uz_ln_head_fwd(const uz_ln_desc* d, const void* x, const float* gamma, const float* beta, const float* w,
                   const float* b /* or NULL */, int K, float* logits, float* stats, void* stream);
long long uz_ln_head_bwd_workspace_bytes(const uz_ln_desc* d, int K);
int uz_ln_head_bwd(const uz_ln_desc* d, const void* x, const float* gamma, const float* beta, const float* w,
                   int K, const float* stats, const float* dlogits, void* dx, float* dgamma, float* dbeta,
                   float* dw, float* db /* or NULL */, float* workspace, void* stream);

/* WindowAttention core (:127-159) with window_partition / roll / window_reverse (:30-56, :246-262)
 * as index arithmetic: qkv (P, 3C) = [3][heads][32] per token, out (P, C).  For window tokens i, j
 *   S_ij = (scale q_i . k_j) / max(|scale q_i| |k_j|, 1e-6) / max(tau[h][i][j], 0.01) + bias[h][i][j]
 *          (- 100 when the shifted-window region ids differ, :214-236);  out_i = softmax_j(S) v
 * tau: (heads, Nt, Nt) parameter (Nt >= ws*ws), bias: (heads, ws*ws, ws*ws) fp32 = cpb MLP output.
 * lse: (B*nW, heads, ws*ws) row log-sum-exp kept for the backward.  head_dim must be 32, ws <= 16: windows of up to 64
 * tokens (ws <= 8) hold the window in one tile, windows of 65 .. 256 tokens (ws 9 .. 16) walk it in 32 x 32 tiles of
 * the score matrix (both in uz_winattn.hip); ws > 16 fails ("exceeds 16x16"). */
typedef struct uz_winattn_desc {
  int dtype, B, H, W, C, heads, ws, shift, Nt;
  int ldq, ldo;
  float scale;
} uz_winattn_desc;
int uz_winattn_fwd(const uz_winattn_desc* d, const void* qkv, const float* tau, const float* bias,
                   void* out, float* lse, void* stream);
/* Continuous position bias (:121-125, Mlp_Relu :58-72): bias[h][r] = fc2(relu(fc1(idx[r]))) over the
 * R = N*N log-spaced offsets idx (R, 2) (any R: 65 536 at ws 16); w1 (hidden, 2), b1 (hidden), w2 (heads, hidden), b2 (heads), fp32.
 * Backward from G = d bias (heads, R): gradients of the four parameter tensors, overwritten. */
int uz_cpb_fwd(const float* idx, const float* w1, const float* b1, const float* w2, const float* b2, int R,
               int hidden, int heads, float* bias, void* stream);
int uz_cpb_bwd(const float* idx, const float* w1, const float* b1, const float* w2, const float* G, int R,
               int hidden, int heads, float* dw1, float* db1, float* dw2, float* db2, void* stream);
/* All position-bias MLPs of a model in one launch each way (they depend on parameters only: forward at the
 * start of the step, backward once every d bias is known).  Forward reads idx, w1, b1, w2, b2 and writes
 * bias; backward reads idx, w1, b1, w2, G and overwrites dw1, db1, dw2, db2 (unused pointers may be NULL). */
typedef struct {
  const float* idx;      /* (R, 2) */
  const float* w1;       /* (hidden, 2) */
  const float* b1;       /* (hidden) */
  const float* w2;       /* (heads, hidden) */
  const float* b2;       /* (heads) */
  int R, hidden, heads, reserved;
  float* bias;           /* forward out (heads, R) */
  const float* G;        /* backward in (heads, R) */
  float* dw1;
  float* db1;
  float* dw2;
  float* db2;
} uz_cpb_item;
int uz_cpb_fwd_batched(const uz_cpb_item* items, int n, void* stream);
long long uz_cpb_bwd_batched_workspace_bytes(const uz_cpb_item* items, int n);
int uz_cpb_bwd_batched(const uz_cpb_item* items, int n, float* workspace, void* stream);
/* rows of `partial`; <0 on error.  A function of the descriptor and the CU reserve only.  For windows of more than 64
 * tokens the rows (1.5 MiB each at ws 16 with 3 heads) are capped so that the buffer stays within 64 MiB. */
int uz_winattn_bwd_rows(const uz_winattn_desc* d);
/* dqkv (P, 3C) fully written; partial[row][2][heads][N][N]: sums over the row's windows of dS (-> d bias)
 * and of d tau (zero where tau < 0.01), every element written (no zero-fill needed); add the rows with uz_sum_rows() /
 * uz_sum_rows_f32(). */
int uz_winattn_bwd(const uz_winattn_desc* d, const void* qkv, const float* tau, const float* bias,
                   const void* out, const float* lse, const void* dout, int lddo, void* dqkv, int lddq,
                   float* partial, void* stream);

/* out[c] = sum_p x[p*ld + c] (fp32; out zeroed by caller). ConvTranspose2d bias gradient. */
int uz_colsum(int dtype, const void* x, int ld, int P, int C, float* out, void* stream);
/* Deterministic form (per-workgroup partial rows in `workspace`, fixed-order finalize; `out` is
 * overwritten, no zeroing needed): nn.Linear / PatchEmbed bias gradients (swin_unet_v2.py:120,123,546). */
long long uz_colsum_workspace_bytes(int dtype, int P, int C);
int uz_colsum_ws(int dtype, const void* x, int ld, int P, int C, float* out, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Step tail: torch.nn.utils.clip_grad_norm_(params, max_norm) followed by torch.optim.AdamW.step()
 * (unet_zoo/utils/training_loop.py:119-121) over FLAT fp32 buffers p, g, m (exp_avg), v (exp_avg_sq) of n
 * elements.  The clipped gradient is consumed, not written back.  `step` is a device scalar (float),
 * incremented by this call; max_norm <= 0 disables clipping.  After the call workspace holds, at byte
 * offset 8192, four floats: clip coefficient, 1-beta1^t, 1-beta2^t, total gradient norm.
 * ------------------------------------------------------------------------------------------- */
long long uz_clip_adamw_workspace_bytes(void);
int uz_clip_adamw(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, float max_norm, float* step, void* workspace,
                  void* stream);

/* ---------------------------------------------------------------------------------------------
 * The scheduled step tail: the arithmetic of uz_clip_adamw with the learning rate, the step counter and the EMA decay
 * held on the device, an optional averaged copy of the weights and an optional accumulated gradient.  uz_steptail.hip
 * Three launches: per-workgroup float64 sums of squares of the effective gradient; one workgroup that forms the norm, the
 * clip coefficient, t + 1, the bias corrections, the rate and the EMA decay into `state`; one streaming pass over p, g, (acc),
 * m, v, (ema).  With sched = UZ_SCHED_CONSTANT, warmup_steps = 0 and acc = ema = NULL, p, m and v come out bit-identical to
 * uz_clip_adamw's for the rate state[1].
 * Effective gradient: g when acc is NULL, else (g + acc) * (1.f / accumulate), the mean of `accumulate` micro-batch gradients
 *   of which acc holds the sum of all but the last (uz_tail_accumulate).  The norm, the clipping and AdamW all see this mean.
 * Schedule, closed-form in t = state[0] BEFORE the call (the 0-based index of the step being taken), evaluated in double and
 *   rounded once to float; L = state[1], W = warmup_steps, T = total_steps, u = clamp((t - W) / (T - W), 0, 1):
 *     t < W (every form)  lr = L * (warmup_start + (1 - warmup_start) * t / W)
 *     UZ_SCHED_CONSTANT   lr = L
 *     UZ_SCHED_COSINE     lr = min_lr + (L - min_lr) * 0.5 * (1 + cos(pi * u))
 *     UZ_SCHED_POLY       lr = min_lr + (L - min_lr) * (1 - u)^power
 *     UZ_SCHED_STEP       lr = max(min_lr, L * gamma^floor((t - W) / every))
 * EMA (ema != NULL), after the AdamW update of an element: e += (1 - d) * (p_new - e), d = ema_decay, or with ema_warmup
 *   d = min(ema_decay, (1 + t) / (10 + t)).
 * state: 8 device floats.  [0] optimizer steps done (advanced by the call); [1] the base rate, written by the host (the call
 *   only reads it); the call writes [2] the rate it used, [3] the EMA decay it used (0 without ema), [4] the clip
 *   coefficient, [5] the gradient norm before clipping, [6] 1 - beta1^t, [7] 1 - beta2^t.
 * All flat buffers hold n floats and are 16-byte aligned, as is the workspace of uz_tail_workspace_bytes() bytes.
 * UZ_EINVAL before any launch: a null or misaligned pointer, n <= 0, a number that is not finite, an unknown sched,
 *   warmup_steps < 0, total_steps <= warmup_steps (cosine, poly), power <= 0 (poly), every < 1 or gamma outside (0, 1] (step),
 *   accumulate < 1, ema_decay outside [0, 1) with ema.
 * ------------------------------------------------------------------------------------------- */
enum { UZ_SCHED_CONSTANT = 0, UZ_SCHED_COSINE = 1, UZ_SCHED_POLY = 2, UZ_SCHED_STEP = 3 };
typedef struct uz_tail_desc {
  long long n;            /* elements of every flat buffer */
  float beta1, beta2, eps, weight_decay, max_norm;   /* as uz_clip_adamw; max_norm <= 0: no clipping */
  int   sched;            /* UZ_SCHED_* */
  float warmup_steps, warmup_start, total_steps, min_lr, power, gamma, every;
  float ema_decay;        /* used when ema != NULL */
  int   ema_warmup;       /* 1: d_t = min(ema_decay, (1 + t) / (10 + t)) */
  int   accumulate;       /* k >= 1: the gradient is (g + acc) / k when acc != NULL, else g */
} uz_tail_desc;
long long uz_tail_workspace_bytes(void);
int uz_tail_step(const uz_tail_desc* d, float* p, const float* g, const float* acc /* nullable */, float* m, float* v,
                 float* ema /* nullable */, float* state, void* workspace, void* stream);
/* acc = first ? g : acc + g over n floats (one launch); with first != 0 the previous contents of acc are not read */
int uz_tail_accumulate(float* acc, const float* g, long long n, int first, void* stream);
/* the CONTENTS of a and b exchanged (one launch); the buffers must not overlap */
int uz_tail_swap(float* a, float* b, long long n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * MISSFormer / MiT blocks (unet_zoo/models/missformer.py).  uz_mit.hip
 * ------------------------------------------------------------------------------------------- */
/* nn.GELU() (erf form) of MixFFN_skip (missformer.py:196,206) on a (P, C) token tensor */
int uz_gelu_fwd(int dtype, const void* x, int ldx, void* y, int ldy, long long P, int C, void* stream);
int uz_gelu_bwd(int dtype, const void* x, int ldx, const void* g, int ldg, void* dx, int lddx, long long P,
                int C, void* stream);
/* DWConv: Conv2d(C, C, 3, 1, 1, groups=C) on NHWC tokens (missformer.py:168-177).  w_taps = the (C,1,3,3)
 * parameter transposed to [9][C] fp32.  flags bit 0: y += x (the "dwconv(fc1) + fc1" of MixFFN_skip :205),
 * bit 1: flipped taps (the gradient with respect to the input; bias NULL). */
int uz_dwconv3x3(int dtype, const void* x, int ldx, const float* w_taps, const float* bias, void* y, int ldy,
                 int N, int H, int W, int C, int flags, void* stream);
/* partial sums part[rows][10][C] (taps 0..8, then the bias) of d(loss)/d(w_taps), d(loss)/d(bias); rows from
 * uz_dwconv3x3_wgrad_rows(); reduce over rows with uz_sum_rows_f32. */
int uz_dwconv3x3_wgrad_rows(int dtype, int N, int H, int W, int C);
int uz_dwconv3x3_wgrad(int dtype, const void* x, int ldx, const void* g, int ldg, float* part, int N, int H,
                       int W, int C, void* stream);
/* dst[n, ho, wo, (ty*r + tx)*C + c] = src[n, ho*r + ty, wo*r + tx, c]: the input of a Conv2d(C, C', r, r)
 * (EfficientSelfAtten.sr, missformer.py:17-18,26-27) as GEMM rows; inverse != 0 scatters such rows back. */
int uz_space_to_depth(int dtype, const void* src, int lds, void* dst, int ldd, int N, int Ho, int Wo, int C, int r,
                      int inverse, void* stream);
/* the same over an H x W fine map with Ho = H / r, Wo = W / r rounded down (Conv2d drops the bottom / right border when
 * r does not divide the map, unext.py Attention.sr); inverse != 0 also writes zeros to that border. */
int uz_space_to_depth_crop(int dtype, const void* src, int lds, void* dst, int ldd, int N, int H, int W, int C, int r,
                           int inverse, void* stream);
/* im2col of the NCHW fp32 input for OverlapPatchEmbeddings' Conv2d(3, 64, 7, 4, 3) (missformer.py:242,312):
 * out[(n, ho, wo)][(kh*k + kw)*C + c] in the run dtype, zero beyond k*k*C up to Kpad. */
int uz_im2col_nchw(int dtype, const float* x_nchw, int N, int C, int H, int W, int k, int stride, int pad, int Kpad,
                   void* out, void* stream);
/* softmax(q k^T * scale) v per (image, head), head_dim D a multiple of 8 in [8, 128] (missformer.py:21-39, :113-128;
 * unext.py Attention).  q / out: (B*N, ld) token tensors, head h in columns [D*h, D*h+D).  Key j of image b is row
 * ((j / kps) * B + b) * kps + j % kps of k / v (kps = NK: one [B][NK] block; the bridge attends to four
 * blocks of kps rows, missformer.py:81-100).  lse: B*heads*N floats kept for the backward: log2 of the sum of
 * exp(scaled scores), i.e. logsumexp / ln 2. */
typedef struct uz_sra_desc {
  int dtype, B, N, NK, heads, head_dim, kps;
  int ldq, ldk, ldv, ldo;
  float scale;
} uz_sra_desc;
int uz_sra_fwd(const uz_sra_desc* d, const void* q, const void* k, const void* v, void* out, float* lse,
               void* stream);
long long uz_sra_bwd_workspace_bytes(const uz_sra_desc* d);
/* go = d(loss)/d(out); dq like q; dkv: dense (B*NK, 2*heads*D) rows laid out like the kv tensor, dK in the
 * first heads*D columns and dV in the rest (k = kv, v = kv + heads*D, ldk = ldv = 2*heads*D). */
int uz_sra_bwd(const uz_sra_desc* d, const void* q, const void* k, const void* v, const void* o, const float* lse,
               const void* go, int ldgo, void* dq, int lddq, void* dkv, int lddkv, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Loss and metric of the training step on the device.  uz_loss.hip
 * out2[0] = BCEWithLogitsLoss(logits, target) with mean reduction (scripts/train.py:135, training_loop.py:113-119),
 * out2[1] = dice_coefficient(logits, target) of the thresholded prediction (utils/metrics.py:7-24: sigmoid > 0.5,
 * epsilon 1e-7, 1.0 for an empty union); dlogits (may be NULL) = d(loss)/d(logits) = (sigmoid(x) - t) / n.
 * n fp32 elements each; two launches, fixed summation order, no host synchronisation (the reference reads
 * loss.item() / dc.item() every step, training_loop.py:123-124). */
long long uz_bce_dice_workspace_bytes(long long n);
int uz_bce_dice(const float* logits, const float* target, long long n, float* dlogits, float* out2, void* workspace,
                void* stream);

/* ---------------------------------------------------------------------------------------------
 * BCE + a region term (soft Dice / Tversky / focal Tversky) over several output maps at once.  uz_region_loss.hip
 * Per map (logits x, target t, n fp32 elements each, p = sigmoid(x)); the flattened map is cut into `groups` contiguous
 * chunks of n / groups elements (1: the batch, N: per image, N * K: per channel):
 *   BCE    = mean_i [ (1 - t_i) x_i + (1 + (pos_weight - 1) t_i) softplus(-x_i) ]         (ATen's stable form)
 *   TI_g   = (I_g + s) / (I_g + alpha (S_g - I_g) + beta (T_g - I_g) + s),   I = sum p t, S = sum p, T = sum t over chunk g
 *   region = mean_g (1 - TI_g)^gamma                  (1 - TI_g formed as (alpha (S - I) + beta (T - I)) / denominator;
 *                                                       gamma == 1 takes no power)
 *   out2[0] = sum_m items[m].weight * (w_bce * BCE_m + w_region * region_m)
 *   out2[1] = the thresholded Dice METRIC of map `metric_item`, exactly as uz_bce_dice defines it
 *   items[m].dlogits (nullable) = d(out2[0]) / d(items[m].logits)
 * alpha = beta = 0.5, s = s' / 2 is the soft Dice (2 I + s') / (S + T + s').
 * `items` is a HOST array of n_items <= UZ_REGION_MAX_ITEMS entries, copied into the kernel arguments as
 * uz_colsum_batched does with its items: no table upload, so a call can be captured into a hipGraph whatever tensors it
 * names, and the host sees whether any gradient is asked for.  All maps of a call share n, groups and the target's layout.
 * Launches, whatever n_items is: (1) one row of six doubles per workgroup (sum bce, sum p t, sum p, sum t, sum [x > 0] t,
 * sum [x > 0]), every workgroup inside one chunk of one map; (2) one workgroup totals the rows in a fixed order, forms
 * TI_g, the loss, the Dice and per chunk the coefficients (u_g, v_g) of d(loss)/d(p_i) = u_g t_i + v_g; (3) the gradient
 *   dlogits_i = weight * [ w_bce / n * (p_i (1 + (pos_weight - 1) t_i) - pos_weight t_i) + (u_g t_i + v_g) p_i (1 - p_i) ]
 * -- not launched when every dlogits is NULL.  No atomics, no memset, no host read; the workspace is written before it is
 * read in every call; two calls on the same inputs give the same bits.  16-byte loads when n / groups is a multiple of 4
 * and every pointer is 16-byte aligned, scalar loads otherwise (chosen here, on the host).
 * UZ_EINVAL before any launch: null descriptor / items / out2 / workspace / logits / target, n <= 0, groups < 1 or not
 * dividing n, n_items outside [1, UZ_REGION_MAX_ITEMS], metric_item outside [0, n_items), smooth <= 0, gamma < 1,
 * alpha / beta / w_bce / w_region / an item's weight negative, w_bce = w_region = 0, pos_weight <= 0, a workspace that
 * is not 16-byte aligned. */
#define UZ_REGION_MAX_ITEMS 64
typedef struct uz_region_item {
  const float* logits;
  const float* target;
  float* dlogits; /* nullable */
  float weight;
} uz_region_item;
typedef struct uz_region_desc {
  int n_items;
  long long n; /* elements per map */
  int groups;  /* per map; divides n */
  float w_bce, w_region, alpha, beta, smooth, gamma, pos_weight;
  int metric_item;
} uz_region_desc;
long long uz_region_loss_workspace_bytes(const uz_region_desc* d); /* < 0: refused */
int uz_region_loss(const uz_region_desc* d, const uz_region_item* items, float* out2 /* loss, dice */, void* workspace,
                   void* stream);

/* ---------------------------------------------------------------------------------------------
 * Softmax cross-entropy + soft Dice over several output maps at once: the multi-class counterpart of
 * uz_region_loss.  uz_class_loss.hip
 * Per map: logits x (N, K, HW) fp32, contiguous; the labels y (N, HW) int32 are shared by all maps.  A pixel is VALID
 * when y != ignore_index and 0 <= y < K; a label outside [0, K) that is not ignore_index is treated as ignored and
 * counted (counts, below).  p = softmax_K(x), w = class_weight (NULL: ones), e = label_smoothing:
 *   a_c(i) = (1 - e) w_c [c == y_i] + (e / K) w_c
 *   CE     = sum_valid sum_c a_c(i) (-log p_c(i)) / sum_valid w_{y_i}          (F.cross_entropy with mean reduction;
 *                                                                               0 with zero gradient when no pixel is valid)
 *   I, S, T = sum p_c [y == c], sum p_c (square: sum p_c^2), sum [y == c]       over the valid pixels of group g
 *   dice   = mean_{g, c in C} (1 - (2 I + smooth) / (S + T + smooth))          formed as (S + T - 2 I) / denominator
 *            g: the batch (reduce = UZ_CLASS_REDUCE_BATCH) or each image (UZ_CLASS_REDUCE_IMAGE);
 *            C: all classes, or 1 .. K-1 when include_background == 0
 *   out2[0] = sum_m items[m].weight * (w_ce * CE_m + w_dice * dice_m)
 *   out2[1] = of map `metric_item`, prediction argmax_K x (ties: the lowest index), over the valid pixels of the batch:
 *             mean over the classes of C with P_c + T_c > 0 of 2 TP_c / (P_c + T_c); 1 when no class remains
 *   counts (nullable): K + 1 rows of 3 -- TP_c, P_c, T_c per class of that map, then (valid, ignored, out of range)
 *   items[m].dlogits (nullable) = d(out2[0]) / d(items[m].logits); exactly 0 at pixels that are not valid
 * Launches, whatever n_items is: (1) one row of 4 + 5 K doubles per workgroup (sum CE terms, sum w_y, valid, out of
 * range; per class I, S, T, TP, P), every workgroup inside one image of one map, one lane per run of four pixels
 * walking the K planes; (2) one workgroup totals the rows in a fixed order and writes out2, counts and per (map, image)
 * the factor weight w_ce / W and per class the coefficients (u, v) of d(loss)/d(p_c) = u [y == c] + v (square: 2 p_c v);
 * (3) the gradient dlogits_k = p_k (g_k - sum_c p_c g_c) + weight w_ce (p_k sum_c a_c - a_k) / W, the softmax
 * recomputed -- not launched when every dlogits is NULL.  No atomics, no memset, no host read; the workspace is written
 * before it is read in every call; two calls on the same inputs give the same bits.  16-byte loads when HW is a
 * multiple of 4 and every pointer is 16-byte aligned, scalar loads of the same runs otherwise: the same numbers.  Above
 * 16 classes a lane takes one pixel at a time (4-byte loads on both paths): four pixels of 32 classes do not fit the
 * registers.
 * `items` is a HOST array copied into the kernel arguments (as uz_region_loss's).
 * UZ_EINVAL before any launch: null descriptor / items / labels / out2 / workspace / logits, K outside
 * [2, UZ_CLASS_MAX_K], n_items outside [1, UZ_CLASS_MAX_ITEMS], N or HW <= 0, smooth <= 0, label_smoothing outside
 * [0, 1), w_ce / w_dice / an item's weight negative, w_ce = w_dice = 0, reduce not one of the two, metric_item outside
 * [0, n_items), a workspace that is not 16-byte aligned. */
#define UZ_CLASS_MAX_ITEMS 16
#define UZ_CLASS_MAX_K 32
#define UZ_CLASS_REDUCE_BATCH 0
#define UZ_CLASS_REDUCE_IMAGE 1
/* one output map of a composed loss (uz_class_loss, uz_boundary_loss, uz_lovasz_loss, uz_cldice_loss, uz_hardpixel_loss): the five
 * item names are one type */
typedef struct uz_map_item {
  const float* logits;
  float* dlogits; /* nullable; in: the base loss's gradient where there is one, out: the combined one */
  float weight;
} uz_map_item;
typedef uz_map_item uz_class_item;
typedef struct uz_class_desc {
  int n_items;
  int N, K;
  long long HW;
  float w_ce, w_dice, smooth, label_smoothing;
  int ignore_index;
  int reduce;             /* UZ_CLASS_REDUCE_* */
  int include_background; /* 0: the Dice term and the metric leave class 0 out */
  int square;             /* S = sum p^2 */
  int metric_item;
} uz_class_desc;
long long uz_class_loss_workspace_bytes(const uz_class_desc* d); /* < 0: refused */
int uz_class_loss(const uz_class_desc* d, const uz_class_item* items, const int* labels,
                  const float* class_weight /* K floats on the device, nullable */, float* out2 /* loss, dice */,
                  long long* counts /* (K + 1) x 3, nullable */, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Bias gradients of a whole backward pass (or phase) in two launches.  uz_colsum.hip
 * out_i[c] = sum_p x_i[p*ld + c] (fp32) for n tensors of the run dtype: what `uz_colsum_ws` computes for one
 * nn.Linear / Conv2d bias (db = sum over tokens of the output gradient), for all of them at once; `items` is a
 * HOST array, copied into the kernel arguments (80 tensors per launch pair).  Deterministic. */
typedef struct uz_colsum_item {
  const void* x; /* (P, ld) rows, C <= ld columns used */
  float* out;    /* C floats */
  int P, C, ld, reserved;
} uz_colsum_item;
/* uz_sum_rows_f32 for n partial buffers at once (the parameter gradients that kernels leave as per-workgroup rows:
 * LayerNorm dgamma | dbeta, depthwise weight gradients): out0[e] / out1[e - n0] = sum_r partial[r*n + e]. */
typedef struct uz_sum_rows_item {
  const float* partial;
  float* out0;
  float* out1; /* may be NULL when n0 == n */
  int rows, n, n0, reserved;
} uz_sum_rows_item;
int uz_sum_rows_f32_batched(const uz_sum_rows_item* items, int n, void* stream);
long long uz_colsum_batched_workspace_bytes(int dtype, const uz_colsum_item* items, int n);
int uz_colsum_batched(int dtype, const uz_colsum_item* items, int n, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Residual sums with ReLU: out = relu(a + b) (b may be NULL) and its gradient dx = g * [out > 0], which both
 * summands receive.  Replaces `x = x + temp; x = F.relu(x)` of Multiresblock.forward and `x = x + shortcut;
 * x = F.relu(x)` of Respath.forward (unet_zoo/models/multiresunet.py:79-80, 127-129, 133-135).
 * ------------------------------------------------------------------------------------------- */
int uz_add_relu(int dtype, const void* a, int lda, const void* b, int ldb, void* out, int ldo, long long P, int C,
                void* stream);
int uz_relu_bwd(int dtype, const void* out, int ldo, const void* g, int ldg, void* dx, int lddx, long long P, int C,
                void* stream);

/* ---------------------------------------------------------------------------------------------
 * Input pipeline on the GPU (BoneDataset.__getitem__, unet_zoo/data/datasets.py:40-59):
 *   transforms.Resize((512, 512)) on a PIL image = Pillow's antialiased two-pass BILINEAR resample of 8-bit pixels in
 *   22-bit fixed point (Pillow src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc,
 *   ImagingResampleHorizontal_8bpc / Vertical_8bpc), then ToTensor (p / 255) and Normalize((v - mean) / std) for the
 *   image, `> 0.5` for the mask.  Bit-exact with Pillow + torch on the CPU.
 * uz_pil_resample_h_u8: dst[h][x][c] (uint8, HWC) for x < Wout from src (H, Win, C) uint8; `bounds` = Wout pairs
 *   (first tap, tap count), `kk` = Wout rows of `ksize` fixed-point coefficients (device pointers, built on the host).
 * uz_pil_resample_v_f32: the vertical pass over (Hin, W, C) uint8 fused with the conversion: mode 0 writes
 *   out[c][y][x] = (p / 255 - mean[c]) / std[c] (fp32, CHW), mode 1 (C = 1) out = (p / 255 > 0.5).  mean / std: HOST
 *   pointers to C floats.
 * ------------------------------------------------------------------------------------------- */
int uz_pil_resample_h_u8(const void* src, int H, int Win, int C, const int* bounds, const int* kk, int ksize, int Wout,
                         void* dst, void* stream);
int uz_pil_resample_v_f32(const void* src, int Hin, int W, int C, const int* bounds, const int* kk, int ksize, int Hout,
                          const float* mean_host, const float* std_host, int mode, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense token attention (U-Transformer's MultiHeadSelfAttention / MultiHeadCrossAttention,
 * unet_zoo/models/unet_transformer.py:126-137, :190-213; TransAttUNet's PAM_Module and ScaledDotProductAttention,
 * unet_zoo/models/transatt_unet.py:41-49, :91-107): torch.bmm + nn.Softmax on (b, tokens, tokens) matrices.
 *
 * uz_gemm_nt: y_b[m][n] = sum_k x_b[m][k] * w_b[n][k] (+ bias[n]) (+ res_b[m][n]) for b < batch -- the LDS-DMA GEMM of
 *   uz_conv_igemm's 1x1 path with a matrix index on the grid.  Strides (ldx, ldw, ldy, ldres: rows; xb, wb, yb, resb:
 *   matrices; 0 = one operand shared by the batch) in ELEMENTS, all multiples of 16 bytes; one matrix < 2 GB.
 *   Replaces torch.bmm(Q, K^T), torch.bmm(A, V) and the MultiHeadDense products x @ W (:24-27) and their gradients
 *   with respect to the left operand; the gradients that contract over the ROWS of both operands (dV = A^T dO,
 *   dK = dS^T Q, dW = X^T dQ) are uz_wgrad with ntaps = 1.
 * uz_softmax_fwd: s_b <- softmax(scale * s_b) in place over axis 0 (every COLUMN sums to one: nn.Softmax(dim=1) of a
 *   (b, rows, cols) tensor, unet_transformer.py:123; three streaming launches: column statistics per 512-row slice,
 *   their combination, the elementwise apply -- `workspace` of uz_softmax_workspace_bytes()) or axis 1 (rows; at most
 *   2048 bf16 / 1024 fp32 columns; no workspace).
 * uz_softmax_bwd: g_b <- a_b * (g_b - dot) * scale in place, a = the softmax output, dot = sum of a * g along the
 *   normalised axis.  Axis 0: `dot` is a (batch, cols) fp32 buffer, computed by a first pass unless dot_given != 0
 *   (attention knows it more cheaply: sum_q A[q][k] dA[q][k] = dV[k] . V[k]); axis 1: computed in registers.
 * uz_adaptive_avgpool_fwd / _bwd: F.adaptive_avg_pool2d on NHWC maps (:196-198) and its gradient (accumulate != 0: added
 *   to dx).  uz_rowdot_f32: out[r] = sum_c a[r][c] * b[r][c] (a fp32, b run dtype).  uz_cast_rows: dst = (run dtype) src
 *   row by row (accumulate != 0: dst += src): the fp32 results of uz_wgrad back into activations.
 * ------------------------------------------------------------------------------------------- */
typedef struct uz_gemm_desc {
  int dtype, batch, M, N, K;
  int ldx, ldw, ldy, ldres;
  long long xb, wb, yb, resb;
  /* optional second batch level (0 / 1: none): batch * batch2 matrices, matrix (b, h) at + b * xb + h * xb2 ... --
   * UCTransNet's heads, which sit side by side in the channels of one token map (uctransnet.py:140-158) */
  int batch2;
  long long xb2, wb2, yb2, resb2;
} uz_gemm_desc;
int uz_gemm_nt(const uz_gemm_desc* d, const void* x, const void* w, const float* bias, const void* res, void* y,
               void* stream);
long long uz_softmax_workspace_bytes(int batch, int rows, int cols, int axis);   /* axis 0: partial column statistics */
int uz_softmax_fwd(int dtype, void* s, int ld, long long sb, int batch, int rows, int cols, int axis, float scale,
                   void* workspace, void* stream);
int uz_softmax_bwd(int dtype, const void* a, void* g, int ld, long long sb, int batch, int rows, int cols, int axis,
                   float scale, float* dot, int dot_given, void* stream);
int uz_adaptive_avgpool_fwd(int dtype, const void* x, int ldx, int N, int Hi, int Wi, int C, void* y, int ldy, int Ho,
                            int Wo, void* stream);
int uz_adaptive_avgpool_bwd(int dtype, const void* g, int ldg, int N, int Hi, int Wi, int C, void* dx, int lddx, int Ho,
                            int Wo, int accumulate, void* stream);
int uz_rowdot_f32(int dtype, const float* a, int lda, const void* b, int ldb, long long rows, int C, float* out,
                  void* stream);
int uz_cast_rows(int dtype, const float* src, int lds, void* dst, int ldd, long long rows, int C, int accumulate,
                 void* stream);
/* out[p][c] = x[p][c] + map[p % HW][c], map fp32 (HW, C): `x + self.pe(x)` (unet_transformer.py:128-129, :181-185), the
 * learned embeddings of transatt_unet.py:144-145 and swin_unet_v2.py:714-715, broadcast over the batch. */
int uz_add_map(int dtype, const void* x, int ldx, const float* map, void* out, int ldo, long long P, int HW, int C,
               void* stream);

/* nn.Dropout(p) in training mode (uctransnet.py:54, :222-223; swin_unet_v2.py:158, :716): out = x * [u >= p] / (1 - p) with
 * u the caller's uniform draw (P x C fp32, contiguous; torch.rand: the generator stays torch's, a seed reproduces a run).
 * The backward is the same call on the gradient with the same u. */
int uz_dropout(int dtype, const void* x, int ldx, const float* u, float p, void* out, int ldo, long long P, int C,
               void* stream);

/* The gate of UCTransNet's CCA (uctransnet.py:417-427): with s[n][c] = sigmoid(...) > 0 per (image, channel),
 *   mode 2 (forward):  out = relu(x * s)
 *   mode 0 (backward): out = g * [x > 0] * x            -- its per-image column sums are d(loss)/d(s)
 *   mode 1 (backward): out = g * [x > 0] * s + a[n][c]   -- a: the gradient reaching x through the global average behind s
 * x, g, out: (N * HW, C) activations; s, a: (N, C) fp32. */
int uz_chanscale_relu(int dtype, int mode, const void* g, int ldg, const void* x, int ldx, const float* s, const float* a,
                      int N, int HW, int C, void* out, int ldo, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Channel-wise cross attention of UCTransNet (Attention_org.forward, unet_zoo/models/uctransnet.py:160-216): the part
 * between the matrix products.  `scores` fp32 (B, H, C, KV) = Q^T K per (image, head) (uz_wgrad_batched); per plane:
 * x = scale * scores, InstanceNorm2d (mean / biased variance over the (C, KV) plane, eps, no affine; :176), softmax over KV
 * (:177).  fwd writes pcat[b][c][h * KV + kv] = P / H and its transpose pcat_t[b][h * KV + kv][c] in the run dtype: the
 * context product over K = H * KV with V (B, tokens, H * KV) then is `context_layer.mean(dim=3)` of all heads (:195-199) in
 * one uz_gemm_nt.  bwd takes d(loss)/d(pcat) (fp32, (B, C, H * KV)) and writes d(loss)/d(scores) as ds[b][h][c][kv] and
 * ds_t[b][h][kv][c] (run dtype), recomputing the statistics and probabilities from `scores`.  KV <= 1024.
 * ------------------------------------------------------------------------------------------- */
int uz_chanattn_probs_fwd(int dtype, const float* scores, int B, int H, int C, int KV, float scale, float eps, void* pcat,
                          void* pcat_t, void* stream);
int uz_chanattn_probs_bwd(int dtype, const float* scores, const float* dpc, int B, int H, int C, int KV, float scale,
                          float eps, void* ds, void* ds_t, void* stream);

/* ---------------------------------------------------------------------------------------------
 * VNet (unet_zoo/models/vnet.py): k x k convolution with k = 5 (zero padding 2) or k = 1, stride 1, NHWC, and the
 * BatchNorm + ELU element passes around it (uz_conv5x5.hip).
 *
 * uz_conv5x5: y[p][n] = sum_{tap, c} x[p + tap][c] * w[n][tap * Cin + c] + bias[n]  (forward: UZ_PACK_CONV_FWD weights;
 * input gradient: the gradient as x and UZ_PACK_CONV_DGRAD weights).  Cin a multiple of 16 bytes and <= 512, Nout <= 512 of
 * any value (the num_classes-wide output layer); everything else is refused with UZ_EINVAL before any launch.
 * stats (nullable): BatchNorm partial rows [uz_conv5x5_grid_m()][2][Nout] of the stored values, as uz_conv_igemm leaves them.
 * ------------------------------------------------------------------------------------------- */
typedef struct uz_conv5x5_desc {
  int dtype;
  int N, H, W;
  int Cin, ldx;
  int Nout, ldy;
  int ksize;   /* 5 or 1 */
} uz_conv5x5_desc;
int uz_conv5x5_grid_m(const uz_conv5x5_desc* d);
int uz_conv5x5(const uz_conv5x5_desc* d, const void* x, const void* w_packed, const float* bias, void* y, float* stats,
               void* stream);
/* out[i][j][tap] = sum_p L[p][i] * R[p + tap][j] for i < CiOut, j < CjOut: fp32, the (Cout, Cin, k, k) parameter layout with
 * L = the output gradient and R = the layer input.  Ci, Cj: the operands' channel counts (multiples of 16 bytes, <= 512;
 * a thin layer's operand is zero-padded to that), CiOut <= Ci, CjOut <= Cj: the parameter's.  Deterministic: per-range
 * slabs in the workspace, summed in a fixed order. */
typedef struct uz_wgrad5x5_desc {
  int dtype;
  int N, H, W;
  int Ci, ldl;
  int Cj, ldr;
  int ksize;   /* 5 or 1 */
  int CiOut, CjOut;
} uz_wgrad5x5_desc;
long long uz_wgrad5x5_workspace_bytes(const uz_wgrad5x5_desc* d);
int uz_wgrad5x5(const uz_wgrad5x5_desc* d, const void* L, const void* R, float* out, void* workspace, void* stream);

/* ContBatchNorm2d -> ELU with VNet's residual sums and Dropout2d masks (vnet.py:35, :65, :82-85, :102-114):
 *   out  = act2( act1( x * scale + shift ) + res ),  act = ELU(alpha = 1) or identity: flags bit 0 = act1, bit 1 = act2
 *   out2 = out * mask2[n][c]      (nullable: the Dropout2d'ed copy, e.g. straight into its half of a concat buffer;
 *                                  mask2 fp32 (N, C) holding 0 or 1 / (1 - p))
 * Any C; 16-byte vectors where C and every leading dimension allow them, and then every tensor must start on a 16-byte
 * boundary (UZ_EINVAL otherwise; the same holds for the two backward passes). */
int uz_bn_elu_apply(int dtype, const void* x, int ldx, const float* scale, const float* shift, int N, int HW, int C,
                    const void* res, int ldres, void* out, int ldo, void* out2, int ldo2, const float* mask2, int flags,
                    void* stream);
/* Its backward, two passes as uz_bn_relu_bwd_*: G = g0 [+ g1] [+ g2 * mask2] is the gradient of `out` (g2: that of out2);
 * no pre-activation tensor is kept: ELU'(z) = 1 where the stored result y > 0, else y + 1 (act2, from `out`), and act1's
 * factor is recomputed from x.  reduce: partial rows [uz_bn_elu_bwd_rows()][2][C] of (sum dbn, sum dbn * xhat), which
 * uz_bn_bwd_finalize() totals; apply: dx (gradient of x, batch statistics) and gres (nullable: gradient of res). */
typedef struct uz_bn_elu_bwd_desc {
  int dtype;
  int N, HW, C;
  int ldx, ldo, ldg0, ldg1, ldg2, lddx, ldgres;
  int flags;
} uz_bn_elu_bwd_desc;
int uz_bn_elu_bwd_rows(const uz_bn_elu_bwd_desc* d);
int uz_bn_elu_bwd_reduce(const uz_bn_elu_bwd_desc* d, const void* x, const void* out, const void* g0, const void* g1,
                         const void* g2, const float* mask2, const float* scale, const float* shift, const float* mean,
                         const float* invstd, float* partials, void* stream);
int uz_bn_elu_bwd_apply(const uz_bn_elu_bwd_desc* d, const void* x, const void* out, const void* g0, const void* g1,
                        const void* g2, const float* mask2, const float* scale, const float* shift, const float* mean,
                        const float* invstd, const double* sums, void* dx, void* gres, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training-time augmentation on the device: flips, rotation, scaling, translation, an optional smooth displacement
 * grid and an intensity jitter, for the picture and its mask together.  uz_augment.hip
 * uz_augment_params (one tiny launch): u (N, 8) fp32 uniforms in [0, 1) -> params (N, 16) fp32 per sample,
 *   [a, b, ox, c, d, oy, contrast, brightness, 0 ...]:
 *   fx = u0 < p_hflip ? -1 : 1, fy = u1 < p_vflip ? -1 : 1, theta = (2 u2 - 1) rotate (degrees),
 *   s = scale_min + u3 (scale_max - scale_min), tx = (2 u4 - 1) translate W, ty = (2 u5 - 1) translate H,
 *   brightness = (2 u6 - 1) brightness_range, contrast = 1 + (2 u7 - 1) contrast_range;
 *   the inverse map M = (1 / s) R(-theta) diag(fx, fy): a = cos fx / s, b = sin fy / s, c = -sin fx / s, d = cos fy / s,
 *   ox = W / 2 + tx - 0.5, oy = H / 2 + ty - 0.5.  Formed in float64, rounded once.
 * uz_augment_apply (one launch): image (N, C, H, W) fp32, C in 1..4; mask (mask_kind) none, fp32 (N, Cm, H, W) with Cm in
 *   1..8, or int32 (N, H, W); disp (nullable, G = 0) the displacement grid (N, 2, G, G) fp32 in pixels (x then y), G in
 *   2..16.  Output pixel (i, j), u = j + 0.5 - W / 2, v = i + 0.5 - H / 2, reads the source at
 *     sx = a u + b v + ox + Dx(i, j),  sy = c u + d v + oy + Dy(i, j)         (pixel indices: sx = 3 is column 3)
 *   D = the grid interpolated bilinearly at (j (G - 1) / (W - 1), i (G - 1) / (H - 1))  (align_corners = True).
 *   image_out = contrast * B + brightness, B = bilinear over the four taps around (floor sx, floor sy), a tap outside the
 *   picture contributing image_fill; mask_out = the mask at (floor(sx + 0.5), floor(sy + 0.5)), mask_fill / label_fill
 *   outside, no jitter.  The outputs have the inputs' shapes and must not overlap any input or each other.
 * A thread owns four consecutive pixels of one row for every plane: 16-byte stores when W % 4 == 0 and the outputs are
 * 16-byte aligned, 4-byte stores of the same values otherwise.  uz_augment_grid() returns the number of workgroups of the
 * launch and (units, nullable) the units they share out (a unit: 256 consecutive runs of four pixels of one sample):
 * units > workgroups means workgroups walk.
 * UZ_EINVAL before any launch: null descriptor / pointer, a mask or grid pointer that does not match mask_kind / G,
 * N, H, W <= 0, C outside 1..4, Cm outside 1..8, G outside {0, 2..16} (or H, W < 2 with a grid), non-finite fills,
 * N max(C, Cm) H W >= 2^31, H W >= 2^30, overlapping or misaligned (4 bytes) tensors; uz_augment_params: probabilities outside [0, 1], scale not
 * 0 < min <= max, a negative or non-finite range. */
#define UZ_AUGMENT_MASK_NONE 0
#define UZ_AUGMENT_MASK_F32 1
#define UZ_AUGMENT_MASK_I32 2
typedef struct uz_augment_desc {
  int N, C, H, W;
  int mask_kind; /* UZ_AUGMENT_MASK_* */
  int Cm;        /* channels of an fp32 mask */
  int G;         /* 0: no displacement grid */
  float p_hflip, p_vflip, rotate, scale_min, scale_max, translate, brightness, contrast;
  float image_fill, mask_fill;
  int label_fill;
} uz_augment_desc;
int uz_augment_params(const uz_augment_desc* d, const float* u, float* params, void* stream);
int uz_augment_grid(const uz_augment_desc* d, int* units /* nullable */);
int uz_augment_apply(const uz_augment_desc* d, const float* image, const void* mask, const float* params, const float* disp,
                     float* image_out, void* mask_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Patch training from a pool of pictures that stays on the device: foreground-aware patch coordinates from uniform draws,
 * and the patches.  uz_patch.hip
 * Pool: image (M, C, H, W) fp32 or uint8 (image_kind), C in 1..4; mask (mask_kind) none, fp32 (M, Cm, H, W) with Cm in 1..8, or
 *   int32 class indices (M, H, W).  Foreground planes, P of them: an fp32 mask has P = Cm, plane c is mask[m, c] > 0.5; labels
 *   have P = num_classes - 1 <= 8, plane p is label == p + 1 (class 0, an ignore index and every other value are background);
 *   no mask: P = 0.  A batch is B patches of h x w pixels, h <= H and w <= W.
 * uz_patch_index (two launches, once per pool): index [M][P][H + 1] int32 (uz_patch_index_bytes), entry y of plane (m, p) the
 *   number of foreground pixels in its rows 0..y-1, entry H the plane's total.  A wave counts a row by ballot + popcount over
 *   64-pixel chunks, a second kernel scans the H counts of each plane: plain stores, no atomics, no memset.
 * uz_patch_draw (one launch, one wavefront per patch): u (B, 8) fp32 uniforms in [0, 1) -> coords (B, 4) int32
 *   [m, y0, x0, plane or -1].  pick(u, n) = min(n - 1, (int)floor((double)u * n)), one float64 product.
 *   m = indices[b] with use_indices (a value outside 0..M-1: coords = [-1, 0, 0, -1], the patch is cut as zeros), else pick(u0, M).
 *   Foreground mode, if u1 < pos (float32) and picture m has a non-empty plane: plane = the pick(u2, n_present)-th non-empty
 *   plane in ascending order; (py, px) = its pick(u3, count)-th foreground pixel in row-major order (the row by a binary search
 *   of the index, the column by a ballot / popcount walk of the row); the pixel lands at patch row
 *   ry = min(h - 1, floor((0.5 + (u4 - 0.5) * jitter) * h)) in float64, every operation rounded (column: u5, w), so jitter 0
 *   centres it and jitter 1 places it uniformly; y0 = clamp(py - ry, 0, H - h), x0 = clamp(px - rx, 0, W - w).
 *   Random mode otherwise: y0 = pick(u4, H - h + 1), x0 = pick(u5, W - w + 1), plane = -1.  u6, u7 are reserved (not read).
 *   A float32 uniform carries 24 bits: a plane with more than 2^24 foreground pixels is sampled on a 2^24-point lattice of
 *   ranks (likewise a pool of more than 2^24 pictures or offsets).
 * uz_patch_cut (one launch): image_out (B, C, h, w) fp32 and mask_out (B, Cm, h, w) fp32 or (B, h, w) int32, the window at
 *   (y0, x0) of picture m.  fp32 pictures and both mask kinds are copied exactly; uint8 pictures become
 *   fmaf((float)v, scale[c], shift[c]) with norm = [scale[0..C), shift[0..C)] fp32 on the device (NULL: scale 1, shift 0; fp32
 *   pictures take no norm).  m outside 0..M-1 gives zeros; y0, x0 are clamped into the picture, nothing is read out of range.
 *   A thread owns four consecutive pixels of one patch row for every plane: 16-byte stores when w % 4 == 0 and the outputs
 *   are 16-byte aligned, 4-byte stores otherwise; loads are 4-byte / 1-byte (x0 is arbitrary).  uz_patch_cut_grid() returns the
 *   number of workgroups and (units, nullable) the units they share out (a unit: 256 consecutive runs of four pixels of one
 *   patch): units > workgroups means workgroups walk.
 * UZ_EINVAL before any launch: null descriptor / pointer; a mask, index, indices or norm pointer that does not match
 * mask_kind / use_indices / image_kind; M, H, W, B, h, w <= 0, C outside 1..4, Cm outside 1..8, P not Cm (fp32 mask), outside
 * 1..8 (labels) or not 0 (no mask); h > H or w > W (pad upstream); pos or jitter outside [0, 1] or not finite; H W >= 2^30,
 * M P (H + 1) >= 2^31, B max(C, Cm) h w >= 2^31; misaligned (4 bytes; uint8 pictures: none) or overlapping tensors. */
#define UZ_PATCH_IMAGE_F32 0
#define UZ_PATCH_IMAGE_U8 1
#define UZ_PATCH_MASK_NONE 0
#define UZ_PATCH_MASK_F32 1
#define UZ_PATCH_MASK_I32 2
typedef struct uz_patch_desc {
  int M, C, H, W;
  int image_kind;  /* UZ_PATCH_IMAGE_* */
  int mask_kind;   /* UZ_PATCH_MASK_* */
  int Cm;          /* channels of an fp32 mask */
  int P;           /* foreground planes */
  int B, h, w;     /* patches per batch and their size */
  int use_indices; /* 1: the source pictures come from `indices` */
  float pos;       /* probability of foreground mode */
  float jitter;    /* 0: the chosen pixel at the patch centre .. 1: anywhere in the patch */
} uz_patch_desc;
long long uz_patch_index_bytes(const uz_patch_desc* d);
int uz_patch_index(const uz_patch_desc* d, const void* mask, int* index, void* stream);
int uz_patch_draw(const uz_patch_desc* d, const float* u, const int* indices /* nullable */, const int* index, const void* mask,
                  int* coords, void* stream);
int uz_patch_cut_grid(const uz_patch_desc* d, int* units /* nullable */);
int uz_patch_cut(const uz_patch_desc* d, const void* image, const void* mask, const int* coords, const float* norm /* nullable */,
                 float* image_out, void* mask_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Surface-distance metrics of a thresholded prediction A against its target B, per (image, class) pair, exact: Hausdorff,
 * percentile Hausdorff (HD95) and average symmetric surface distance as medpy's hd / hd95 / assd compute them in 2D with
 * connectivity 1.  uz_surface.hip
 *   S(X)  = the pixels of X with a 4-neighbour outside X; outside the picture counts as outside X
 *   d2(p, S) = min over s in S of (pi - si)^2 + (pj - sj)^2, an integer
 *   D     = { d2(p, S(B)) : p in S(A) } + { d2(p, S(A)) : p in S(B) } as a multiset, n = |S(A)| + |S(B)|
 *   hd    = spacing sqrt(max D)
 *   hdq   = spacing (lo + f (hi - lo)),  r = (n - 1) (q / 100), k = floor(r), f = r - k, lo = sqrt(D_(k)),
 *           hi = sqrt(D_(min(k + 1, n - 1))), D_(k) the k-th smallest (from 0): numpy.percentile(sqrt(D), q), linear
 *   assd  = spacing / 2 (mean of sqrt over the first part of D + mean of sqrt over the second)
 *   state = 0 both masks non-empty, 1 A empty, 2 B empty, 3 both empty; with a state other than 0 the three values and the
 *           three d2 statistics are 0
 * The order statistics are exact (integer histograms of d2); sqrt, the interpolation and the sums are float64, the sums in
 * a fixed order, and every value is rounded to float32 once.
 * UZ_SURFACE_BINARY: logits and target (N, C, H, W) fp32; A = logits > 0, B = target > 0.5, every channel a pair: P = C.
 * UZ_SURFACE_CLASS : logits (N, C, H, W) fp32 with C = K classes, target (N, H, W) int32 labels; A = (argmax_K == c), ties
 *   to the lowest index, B = (label == c), for c = first_class .. K - 1: P = K - first_class.  A pixel whose label is
 *   ignore_index or outside [0, K) belongs to no mask of any class.
 * out (N, P, 4) fp32 = hd, hdq, assd, 0;  stats (N, P, 8) int64 = |S(A)|, |S(B)|, max d2, D_(k), D_(k+1), state, |A|, |B|.
 * One call is SEVEN launches whatever the shape (clear, codes, rows, columns, select1, level2, finalize), no allocation, no
 * memset, no host synchronisation; the workspace (uz_surface_workspace_bytes, 16-byte aligned) is cleared by the first
 * launch.  uz_surface_grid() returns the workgroups of the widest launch (the column pass) and (units, nullable) the units
 * they share out (a unit: 256 consecutive pixels of one mask of one pair): units > workgroups means workgroups walk.
 * UZ_EINVAL before any launch: null descriptor / pointer, unknown mode, N, C, H or W < 1, H or W > 4096, in the class mode
 * K outside [2, UZ_CLASS_MAX_K] or first_class outside [0, K), q outside (0, 100], spacing not positive and finite,
 * N C H W >= 2^31, tensors misaligned (4 bytes; stats 8, workspace 16) or overlapping. */
#define UZ_SURFACE_BINARY 0
#define UZ_SURFACE_CLASS 1
typedef struct uz_surface_desc {
  int mode;         /* UZ_SURFACE_* */
  int N, C, H, W;   /* C: channels (binary) or classes K (class mode) */
  int first_class;  /* class mode: the first class that is a pair (1 leaves the background out) */
  int ignore_index; /* class mode */
  int reserved;
  double q;         /* percentile of hdq, 0 < q <= 100 */
  double spacing;   /* isotropic pixel spacing */
} uz_surface_desc;
long long uz_surface_workspace_bytes(const uz_surface_desc* d); /* < 0: refused */
int uz_surface_grid(const uz_surface_desc* d, int* units /* nullable */);
int uz_surface_metrics(const uz_surface_desc* d, const float* logits, const void* target, float* out, long long* stats,
                       void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Confusion counts of a thresholded prediction against its target, per (image, class) pair, and the overlap scores derived
 * from them; in the binary mode also the score histograms that ROC / PR curves are summed from.  Everything counted is an
 * integer: exact, independent of the order of arrival and of the grid, summable over a pass.  uz_confusion.hip
 * UZ_CONFUSION_BINARY: logits and target (N, C, H, W) fp32; every (image, channel) plane is a pair: P = C.
 *   prediction x > 0, target t > 0.5 (the thresholds of uz_bce_dice and uz_surface): x = 0 is negative, t = 0.5 is negative,
 *   a NaN logit is negative.
 *   counts (N, P, 4) int64 = TP, FP, FN, TN
 *   hist   (N, P, 2, B) int64: hist[n, p, s, b] = pixels with (t > 0.5) == s and bin(x) == b, where
 *          bin(x) = the number of edges e_k with x >= e_k   -- numpy.searchsorted(edges, x, side="right"); NaN: bin 0
 *   edges  B - 1 floats ON THE DEVICE, strictly ascending and finite, IN LOGIT SPACE: the kernel compares floats against the
 *          table and evaluates no sigmoid.  Their contents are the caller's responsibility (a host check would read device
 *          memory); a table that is not ascending gives a histogram that means nothing, never an access out of bounds.
 * UZ_CONFUSION_CLASS : logits (N, C, H, W) fp32 with C = K classes, target (N, H, W) int32 labels; prediction argmax_K, ties
 *   to the lowest index (as uz_class_loss and uz_surface).  A pixel whose label is ignore_index or outside [0, K) is counted
 *   nowhere.
 *   counts (N, K, K) int64: counts[n, t, p] = pixels with label t and prediction p
 *   hist and edges are not used (NULL), bins = 0.  Pairs are the classes first_class .. K - 1: P = K - first_class, with
 *   TP = counts[c, c], FP = column sum - TP, FN = row sum - TP, TN = valid pixels - TP - FP - FN.
 * out (N, P, 8) fp32 = dice, iou, precision, recall, specificity, state, 0, 0 per pair:
 *   dice = 2 TP / (2 TP + FP + FN), iou = TP / (TP + FP + FN), precision = TP / (TP + FP), recall = TP / (TP + FN),
 *   specificity = TN / (TN + FP); every score is ONE float64 division of integers, rounded to float32 once; a score whose
 *   denominator is 0 is 0, except dice = iou = 1 in state 3
 *   state = 0 both masks non-empty, 1 the prediction empty, 2 the target empty, 3 both empty (as uz_surface)
 * One call is THREE launches whatever the shape (clear, count, finalize), no allocation, no memset, no host
 * synchronisation; the workspace (uz_confusion_workspace_bytes, 16-byte aligned, int32 counters: a plane has at most 2^24
 * pixels) is cleared by the first launch.  The counting pass gives every workgroup one contiguous run of (plane, tile) units
 * (a tile: 1024 consecutive pixels of a plane, in the class mode of an image), counts into a histogram in LDS and adds its
 * non-zero bins to the workspace with integer atomics when the run leaves a plane and at its end.  uz_confusion_grid()
 * returns the workgroups of the counting pass and (units, nullable) the units they share out: units > workgroups means
 * workgroups walk.  max_workgroups > 0 caps the grid.
 * UZ_EINVAL before any launch: null descriptor / pointer (edges and hist: binary mode only), unknown mode, N, C, H or W < 1,
 * H or W > 4096, N C H W >= 2^31, in the class mode K outside [2, UZ_CLASS_MAX_K], first_class outside [0, K) or bins != 0,
 * in the binary mode bins not a power of two in [16, 1024], max_workgroups < 0, tensors misaligned (4 bytes; counts and hist
 * 8, workspace 16) or overlapping. */
#define UZ_CONFUSION_BINARY 0
#define UZ_CONFUSION_CLASS 1
typedef struct uz_confusion_desc {
  int mode;           /* UZ_CONFUSION_* */
  int N, C, H, W;     /* C: channels (binary) or classes K (class mode) */
  int first_class;    /* class mode: the first class that is a pair (1 leaves the background out) */
  int ignore_index;   /* class mode */
  int bins;           /* binary mode: B, a power of two in [16, 1024]; class mode: 0 */
  int max_workgroups; /* 0: the plan's own grid; > 0: cap it (CU sharing; lets a small shape walk) */
  int reserved[3];
} uz_confusion_desc;
long long uz_confusion_workspace_bytes(const uz_confusion_desc* d); /* < 0: refused */
int uz_confusion_grid(const uz_confusion_desc* d, int* units /* nullable */);
int uz_confusion_metrics(const uz_confusion_desc* d, const float* logits, const void* target, const float* edges /* binary: B - 1 */,
                         long long* counts, long long* hist /* binary */, float* out, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Boundary loss (Kervadec et al., "Boundary loss for highly unbalanced segmentation") on top of a base loss whose value
 * and gradients exist already: the exact signed Euclidean distance transform of the target, dense, and the mean of
 * probability x signed distance over several output maps.  uz_boundary_loss.hip
 * Per plane with target mask G on H x W, sd2 is an INTEGER:
 *   sd2(p) = +min over g in G of |p - g|^2 for p outside G, -min over q outside G of |p - q|^2 for p in G, and 0
 *            everywhere when G is empty or the whole plane.  Pixels outside the picture do not exist.
 *   phi(p) = spacing sqrt(sd2) where sd2 > 0, -spacing (sqrt(-sd2) - 1) where sd2 < 0, 0 where sd2 = 0
 *            -- edt(~G) ~G - (edt(G) - 1) G of scipy.ndimage.distance_transform_edt
 * UZ_BOUNDARY_BINARY: logits and target (N, C, H, W) fp32; G = target > 0.5, every (image, channel) a plane: M = N C;
 *   p = sigmoid(x);  B = sum p phi / (N C H W);  dB/dx = phi p (1 - p) / (N C H W).
 * UZ_BOUNDARY_CLASS : logits (N, C, H, W) fp32 with C = K classes, target (N, H, W) int32 labels y; G_c = (y == c) for
 *   c in Cset = first_class .. K - 1: M = N (K - first_class), plane n * (K - first_class) + (c - first_class).  A pixel
 *   whose label is ignore_index or outside [0, K) is in no G_c (for the transform it is complement), adds nothing to the sum
 *   and has zero gradient.  p = softmax_K(x);  B = sum over valid pixels and Cset of p_c phi_c / (N |Cset| H W);
 *   dB/dx_k = p_k (phit_k - sum_c p_c phit_c) / (N |Cset| H W) with phit_c = phi_c in Cset, 0 otherwise.
 * scales = {weight, base_scale}, two floats ON THE DEVICE, and base_loss, one float on the device, are read by the kernels:
 *   out[0] = base_scale * base_loss + weight * sum_m items[m].weight * B_m;   out[1] = B of map metric_item
 *   items[m].dlogits (nullable) holds d(base_loss)/d(logits) on entry and is rewritten in place:
 *   dl <- base_scale * dl + weight * items[m].weight * dB/dx
 * sd2 (M, H, W) int32 is an OUTPUT of the call, computed once and shared by all maps; phi is formed from it on the fly.
 * One call is FIVE launches whatever n_items is (rows, planes, columns, loss, finalize), no allocation, no memset, no host
 * read; float64 sums in a fixed order: two calls on the same inputs give the same bits.  `items` is a HOST array copied
 * into the kernel arguments.  uz_boundary_grid() returns the workgroups of the column pass and (units, nullable) the units
 * they share out (a unit: 256 consecutive pixels of one plane): units > workgroups means workgroups walk.
 * UZ_EINVAL before any launch: null descriptor / pointer (dlogits may be null), unknown mode, n_items outside
 * [1, UZ_CLASS_MAX_ITEMS], N, C, H or W < 1, H or W > 4096, in the class mode K outside [2, UZ_CLASS_MAX_K] or first_class
 * outside [0, K), metric_item outside [0, n_items), spacing not positive and finite, N C H W >= 2^31, 2^30 or more units,
 * an item's weight negative, tensors misaligned (4 bytes; workspace 16), or a written buffer (out, sd2, workspace, dlogits)
 * overlapping any other buffer of the call. */
#define UZ_BOUNDARY_BINARY 0
#define UZ_BOUNDARY_CLASS 1
typedef uz_map_item uz_boundary_item;
typedef struct uz_boundary_desc {
  int mode; /* UZ_BOUNDARY_* */
  int n_items;
  int N, C, H, W;   /* C: channels (binary) or classes K (class mode) */
  int first_class;  /* class mode: the first class of Cset (1 leaves the background out) */
  int ignore_index; /* class mode */
  int metric_item;
  float spacing; /* isotropic pixel spacing */
} uz_boundary_desc;
long long uz_boundary_workspace_bytes(const uz_boundary_desc* d); /* < 0: refused */
int uz_boundary_grid(const uz_boundary_desc* d, int* units /* nullable */);
int uz_boundary_loss(const uz_boundary_desc* d, const uz_boundary_item* items, const void* target,
                     const float* scales /* device: weight, base_scale */, const float* base_loss /* device */,
                     float* out /* 2 */, int* sd2 /* M * H * W, an output */, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Lovasz hinge / Lovasz-softmax (Berman, Triggs, Blaschko, "The Lovasz-Softmax loss", CVPR 2018) on top of a base loss whose
 * value and gradients exist already: a segmented STABLE sort of the pixel errors and a scan over the sorted membership
 * bits.  uz_lovasz_loss.hip
 * A segment is a list of (error e, membership bit b).  The elements with e > 0 are ranked 0, 1, ... by descending e, ties by
 * ascending position; an element with e <= 0 has rank -1, adds nothing and has zero gradient.  With G members (b = 1) in
 * the whole segment, c members among ranks 0 .. r and n = r + 1 - c, the element at rank r weighs
 *   g = 1 / (G + n) if b = 1,  (G - c) / ((G + n - 1) (G + n)) if b = 0,  1 at rank 0 of a segment with G = 0
 * (the difference J_r - J_(r-1) of J_r = 1 - (G - c) / (G + n)), and the segment's value is L = sum over ranks of e g.
 * UZ_LOVASZ_BINARY: logits and target (N, C, H, W) fp32; b = target > 0.5, s = +1 where b else -1, e = 1 - x s in fp32.
 *   per_image: a segment per (image, channel) in row-major pixel order, S = N C of length H W; otherwise a segment per
 *   channel over the batch in image-major order, S = C of length N H W.  V = mean of L over the S segments;
 *   dV/dx = -s g / S at a ranked pixel.
 * UZ_LOVASZ_CLASS : logits (N, C, H, W) fp32 with C = K classes, target (N, H, W) int32 labels y; p = softmax_K(x), for
 *   class c: b = (y == c), e = |b - p_c|.  A pixel whose label is ignore_index or outside [0, K) is in no segment (e = 0,
 *   rank -1, no member, zero gradient on all K logits).  per_image: a segment per (image, class), segment n K + c;
 *   otherwise per class over the batch.  With P_l the classes that have a member in line l (an image, or the batch), or all
 *   K with UZ_LOVASZ_ALL:  V = (1 / lines) sum_l (1 / |P_l|) sum_{c in P_l} L_{l,c}; a line with empty P_l adds 0.
 *   dV/dx_k = p_k (d_k - sum_c p_c d_c) with d_c = sign(p_c - b) g / (lines |P_l|) at a ranked element, 0 otherwise.
 * scales = {weight, base_scale}, two floats ON THE DEVICE, and base_loss, one float on the device, are read by the kernels:
 *   out[0] = base_scale * base_loss + weight * sum_m items[m].weight * V_m;   out[1] = V of map main_item
 *   items[m].dlogits (nullable) holds d(base_loss)/d(logits) on entry and is rewritten in place:
 *   dl <- base_scale * dl + weight * items[m].weight * dV/dx
 * errors (S, length) fp32 and ranks (S, length) int32 are OUTPUTS of the call, of map main_item.  Every map is sorted on its
 * own, all of them in the same launches: the workspace grows linearly with n_items (16 bytes per element of every map for
 * the two key / value buffers, plus about 1 byte per element for the digit counts).
 * One call is 18 launches, 19 when a map has a gradient buffer, whatever n_items and the data are: keys, segments, 4 x (hist,
 * rowscan, scatter) of a least-significant-digit radix sort with 8-bit digits, bits, scan, [grad,] finalize.  No
 * allocation, no memset, no host read, no float atomics, no waiting between workgroups; float64 sums in a fixed order and
 * a scatter whose positions do not depend on arrival order: two calls on the same inputs give the same bits, `ranks`
 * included.  `items` is a HOST array copied into the kernel arguments.  uz_lovasz_grid() returns the workgroups of the passes
 * over (segment, tile) units and (units, nullable) the units they share out (a unit: 1024 consecutive elements of one
 * segment): units > workgroups means workgroups walk.
 * UZ_EINVAL before any launch: null descriptor / pointer (dlogits may be null), unknown mode or classes mode, n_items outside
 * [1, UZ_CLASS_MAX_ITEMS], N, C, H or W < 1, in the class mode K outside [2, UZ_CLASS_MAX_K], main_item outside
 * [0, n_items), a segment longer than 2^22, more than 2^28 elements in all maps, an item's weight negative, tensors
 * misaligned (4 bytes; workspace 16), or a written buffer (out, errors, ranks, workspace, dlogits) overlapping any other
 * buffer of the call. */
#define UZ_LOVASZ_BINARY 0
#define UZ_LOVASZ_CLASS 1
#define UZ_LOVASZ_PRESENT 0
#define UZ_LOVASZ_ALL 1
typedef uz_map_item uz_lovasz_item;
typedef struct uz_lovasz_desc {
  int mode; /* UZ_LOVASZ_BINARY / UZ_LOVASZ_CLASS */
  int n_items;
  int N, C, H, W;   /* C: channels (binary) or classes K (class mode) */
  int per_image;    /* 0: one segment per channel / class over the whole batch */
  int classes;      /* class mode: UZ_LOVASZ_PRESENT / UZ_LOVASZ_ALL */
  int ignore_index; /* class mode */
  int main_item;
} uz_lovasz_desc;
long long uz_lovasz_workspace_bytes(const uz_lovasz_desc* d); /* < 0: refused */
int uz_lovasz_grid(const uz_lovasz_desc* d, int* units /* nullable */);
int uz_lovasz_loss(const uz_lovasz_desc* d, const uz_lovasz_item* items, const void* target,
                   const float* scales /* device: weight, base_scale */, const float* base_loss /* device */,
                   float* out /* 2 */, float* errors /* S * length, an output */, int* ranks /* S * length, an output */,
                   void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * clDice (Shit et al., "clDice -- a novel topology-preserving loss function for tubular structure segmentation", CVPR 2021)
 * on top of a base loss whose value and gradients exist already: the soft skeleton as a stencil held in LDS.
 * uz_cldice_loss.hip
 * For a plane a (H, W), every window clipped to the picture:
 *   erode(a) = min(v, h): v the minimum of the vertical 3-window (up, centre, down), h of the horizontal one (left, centre,
 *   right);  dilate(a) = the maximum of the 3 x 3 window;  open(a) = dilate(erode(a));
 *   skel_k(a): S = relu(a - open(a)); then k times: a <- erode(a), d = relu(a - open(a)), S <- S + relu(d - S d).
 * skel_k(a) at a pixel depends on a within Chebyshev distance R = k + 2; k = iterations.  For one segment, with prediction
 * plane(s) p, target plane(s) t and s = smooth > 0:
 *   Tprec = (sum skel(p) t + s) / (sum skel(p) + s),  Tsens = (sum skel(t) p + s) / (sum skel(t) + s),
 *   cl = 1 - 2 Tprec Tsens / (Tprec + Tsens);   V = the mean of cl over the segments.
 * UZ_CLDICE_BINARY: logits and target (N, C, H, W) fp32; p = sigmoid(x) in fp32, t the target as given (soft values in
 *   [0, 1] allowed; skel(t) gets no gradient).  per_image = 0: a segment per channel over the batch; 1: per (image, channel).
 * UZ_CLDICE_CLASS : logits (N, C, H, W) fp32 with C = K classes, target (N, H, W) int32 labels y; p = softmax_K(x),
 *   t_c = (y == c); the classes are 1 .. K-1, or 0 .. K-1 with include_background.  A pixel whose label is ignore_index or
 *   outside [0, K) has p_c = t_c = 0 in every plane before the skeleton, whatever gradient reaches it is dropped: its K
 *   logits get exactly zero.  dV/dx_k = p_k (g_k - sum_c p_c g_c) with g_c = dV/dp_c, 0 for an excluded class.
 * Subgradients are torch's: relu'(0) = 0; dilate routes to the first maximum in row-major window order; v to the first
 * minimum top to bottom, h left to right; min(v, h) to the smaller one, half to each on v == h.
 * scales = {weight, base_scale} and base_loss are ON THE DEVICE, as for uz_lovasz_loss:
 *   out[0] = base_scale * base_loss + weight * sum_m items[m].weight * V_m;   out[1] = V of map main_item
 *   items[m].dlogits (nullable): dl <- base_scale * dl + weight * items[m].weight * dV/dx, in place.
 * probs and skeleton (N, C, H, W) fp32 are OUTPUTS, p and skel(p) of map main_item (an excluded class's skeleton plane is
 * not written); target_skeleton (N, C, H, W) fp32 is skel(t), computed once per call for all maps.
 * One call is 4 launches, 6 when a map has a gradient buffer, whatever n_items and the data are: prob, target skeleton,
 * forward tiles, sums (+ out), [backward tiles, grad].  A tile is UZ_CLDICE_TILE_H x UZ_CLDICE_TILE_W pixels of one plane
 * with a halo of R (forward) or 2 R (backward, which forms the forward again); a unit is (map, plane, tile).  No allocation,
 * no memset, no host read, no float atomics, no waiting between workgroups; float64 sums in a fixed order: two calls on the
 * same inputs give the same bits.  The k + 1 intermediate images of a map stay in LDS.  The workspace holds p and dV/dp of
 * every map (8 bytes per element) plus, in the class mode, the target's planes.  uz_cldice_grid() returns the workgroups of
 * the tile passes and (units, nullable) the units they share out: units > workgroups means workgroups walk.
 * UZ_EINVAL before any launch: the cases of uz_lovasz_loss (no segment limit), iterations outside
 * [1, UZ_CLDICE_MAX_ITERATIONS], smooth not finite or not positive. */
#define UZ_CLDICE_BINARY 0
#define UZ_CLDICE_CLASS 1
#define UZ_CLDICE_MAX_ITERATIONS 10
#define UZ_CLDICE_TILE_H 32
#define UZ_CLDICE_TILE_W 32
typedef uz_map_item uz_cldice_item;
typedef struct uz_cldice_desc {
  int mode; /* UZ_CLDICE_BINARY / UZ_CLDICE_CLASS */
  int n_items;
  int N, C, H, W;         /* C: channels (binary) or classes K (class mode) */
  int per_image;          /* 0: one segment per channel / class over the whole batch */
  int include_background; /* class mode: class 0 counts too */
  int ignore_index;       /* class mode */
  int iterations;         /* k */
  float smooth;
  int main_item;
} uz_cldice_desc;
long long uz_cldice_workspace_bytes(const uz_cldice_desc* d); /* < 0: refused */
int uz_cldice_grid(const uz_cldice_desc* d, int* units /* nullable */);
int uz_cldice_loss(const uz_cldice_desc* d, const uz_cldice_item* items, const void* target,
                   const float* scales /* device: weight, base_scale */, const float* base_loss /* device */,
                   float* out /* 2 */, float* probs /* N C H W, an output */, float* skeleton /* N C H W, an output */,
                   float* target_skeleton /* N C H W, an output */, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Hard-pixel mining -- top-k cross-entropy (nnU-Net's DC_and_topk), OHEM cross-entropy (keep the pixels whose true-class
 * probability is below max_prob, and min_kept at least) and focal loss (Lin et al., ICCV 2017) -- on top of a base loss
 * whose value and gradients exist already: an exact k-th-largest selection per segment, an MSB-first radix select over the
 * bit patterns of the per-pixel losses.  uz_hardpixel_loss.hip
 * A segment is a list of valid pixels, each with a plain loss l >= 0 and a true-class probability p_t = exp(-l).
 * UZ_HARDPIXEL_CLASS : logits (N, C, H, W) fp32 with C = K classes, target (N, H, W) int32 labels y;
 *   l = logsumexp_K(x) - x_y in fp32 with the maximum subtracted.  A pixel whose label is ignore_index or outside [0, K) is
 *   in no segment and gets zero gradient on all K logits.  No class weights and no label smoothing enter: the base's.
 * UZ_HARDPIXEL_BINARY: logits and target (N, C, H, W) fp32; b = target > 0.5, s = +1 where b else -1, l = softplus(-s x);
 *   every element is valid.
 * Focal modulation: f = (1 - p_t)^gamma l with gamma = 0 or gamma >= 1 (in (0, 1) the factor (1 - p_t)^(gamma - 1) of the
 *   derivative is unbounded at p_t -> 1).  f increases with l, so selecting on f and on l keep the same pixels.
 *   df/dl = (1 - p_t)^gamma + gamma (1 - p_t)^(gamma - 1) p_t l, exactly 1 at gamma = 0;
 *   dl/dx_c = p_c - [c == y] (class), dl/dx = -s (1 - p_t) (binary).
 * Segments: per_image = 0: one per output map over the whole batch; 1: one per image (binary: all C channels of the image).
 * Kept count of a segment with n valid pixels: k = clamp(max(min_kept, ceil(keep n)), 1, n), the product keep n taken in
 *   fp32 (one rounding: keep = 0.1f of n = 1000 is 100); with max_prob > 0, c = #{p_t < max_prob} counted on the plain
 *   l > -log(max_prob) (the threshold rounded to fp32), otherwise c = 0; m = max(k, c).  n = 0: the segment adds 0 and has
 *   zero gradient.
 * Value: tau = the m-th largest f of the segment, n_above = #{f > tau}, n_tie = #{f == tau};
 *   V_seg = (sum_{f > tau} f + (m - n_above) tau) / m;   V = the mean of V_seg over the segments of the map with n > 0.
 * Gradient: a pixel with f > tau weighs 1 / m, one with f == tau weighs (m - n_above) / (n_tie m), every other 0: a
 *   subgradient of the top-m sum that does not depend on position or arrival order; without ties torch.topk's gradient.
 * scales = {weight, base_scale} and base_loss are ON THE DEVICE, as for uz_lovasz_loss:
 *   out[0] = base_scale * base_loss + weight * sum_m items[m].weight * V_m;   out[1] = V of map main_item
 *   items[m].dlogits (nullable): dl <- base_scale * dl + weight * items[m].weight * dV/dx, in place.
 * losses is the f of map main_item in the map's own layout ((N, C, H, W) binary, (N, H, W) class; 0 at a pixel in no
 * segment), selection (segments, 4) int32 of map main_item: m, n_above, n_tie and the bit pattern of tau; both OUTPUTS.
 * One call is 10 launches whatever n_items, the data and the gradient buffers are: loss (with the first digit's counts),
 * pick, 3 x (hist, pick) with 8-bit digits, grad (which also forms the float64 sums of the kept f per unit), finalize.  A
 * unit is (segment, chunk), a chunk 2048 t consecutive elements of a segment with t the smallest integer that leaves at
 * most 256 chunks a segment.  No allocation, no memset, no host read, no float atomics, no waiting between workgroups;
 * integer counts and float64 sums per unit in a fixed order: two calls on the same inputs give the same bits, and so does a
 * call with max_workgroups set.  The workspace: 4 bytes per element of every map's f, and per unit 1024 bytes of digit
 * counts + 8 bytes of n and c + 8 bytes of sum, and 32 bytes per segment, each of the five buffers on a 16-byte boundary.
 * uz_hardpixel_grid returns the workgroups of the passes over units and (units, nullable) the units they share out:
 * units > workgroups means workgroups walk.
 * UZ_EINVAL before any launch: the cases of uz_lovasz_loss (a segment longer than 2^24 here), more than 2^16 segments in
 * the call (n_items N with per_image), keep outside (0, 1],
 * min_kept < 0, max_prob outside {0} U (0, 1), gamma negative, not finite or in (0, 1), max_workgroups < 0. */
#define UZ_HARDPIXEL_BINARY 0
#define UZ_HARDPIXEL_CLASS 1
typedef uz_map_item uz_hardpixel_item;
typedef struct uz_hardpixel_desc {
  int mode; /* UZ_HARDPIXEL_BINARY / UZ_HARDPIXEL_CLASS */
  int n_items;
  int N, C, H, W;     /* C: channels (binary) or classes K (class mode) */
  int per_image;      /* 0: one segment per map over the whole batch */
  int ignore_index;   /* class mode */
  int main_item;
  float keep;         /* (0, 1] */
  int min_kept;       /* >= 0 */
  float max_prob;     /* 0 = off, else in (0, 1) */
  float gamma;        /* 0 or >= 1 */
  int max_workgroups; /* 0: the plan's own grid; > 0: cap it, as in uz_confusion_desc */
} uz_hardpixel_desc;
long long uz_hardpixel_workspace_bytes(const uz_hardpixel_desc* d); /* < 0: refused */
int uz_hardpixel_grid(const uz_hardpixel_desc* d, int* units /* nullable */);
int uz_hardpixel_loss(const uz_hardpixel_desc* d, const uz_hardpixel_item* items, const void* target,
                      const float* scales /* device: weight, base_scale */, const float* base_loss /* device */,
                      float* out /* 2 */, float* losses /* an output */, int* selection /* segments * 4, an output */,
                      void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mask post-processing, per (image, plane), every result an integer that scipy.ndimage gives too.  uz_postproc.hip
 * UZ_POST_BINARY: x (N, C, H, W) fp32; plane = x > thr, every channel a plane: P = C.  Logits with thr = 0 or
 *   probabilities with thr = 0.5.
 * UZ_POST_CLASS : x (N, C, H, W) fp32 with C = K classes; plane c = (argmax_K == c), ties to the lowest index, for
 *   c = first_class .. K - 1: P = K - first_class.
 * Per plane, in this order:
 *   1. fill_holes: add every pixel of the complement that is not 4-connected, within the complement, to a pixel on the
 *      picture's edge (scipy.ndimage.binary_fill_holes, default structure: the cross whatever `connectivity` is)
 *   2. components with connectivity 1 (cross) or 2 (3 x 3 square); a component's root is its smallest index i W + j
 *   3. drop the components with area < min_area
 *   4. keep_largest = k > 0: keep the k components of largest area, ties to the smaller root
 * mask   (N, P, H, W) u8   the surviving pixels, 0 / 1
 * labels (N, P, H, W) i32  the survivors numbered 1 .. n in raster order of their roots = scipy.ndimage.label(mask)[0]
 * class_map (N, H, W) u8   class mode: the argmax class where its plane kept the pixel, else the lowest class whose final
 *                          plane holds it (a filled hole), else 0
 * stats  (N, P, 8) i64     components after step 1, components kept, area after step 1, area kept, pixels added by step 1,
 *                          the largest area among the components of at least min_area, error word, 0
 * comps  (N, P, 8, 8) i64  the eight (keep_largest, if smaller) largest kept components in the order of step 4, each
 *                          area, i_min, j_min, i_max, j_max, sum i, sum j, root; unused records are zero
 * labels and class_map may be null.  The error word is non-zero when a bounded find / union loop ran out (H W steps, a true
 * bound: a bug, never a property of the input); the results of that plane are then undefined.
 * The launches of a call depend on the descriptor alone: 18 (+ 4 with fill_holes, + 1 in the class mode); no allocation,
 * no memset, no host synchronisation; the workspace (uz_postproc_workspace_bytes, 16-byte aligned) is cleared by the first
 * launch.  No workgroup waits for another inside a launch.  uz_postproc_grid() returns the workgroups of the per-unit
 * launches and (units, nullable) the units they share out (a unit: 256 consecutive pixels of a plane).
 * UZ_EINVAL before any launch: null descriptor / pointer, unknown mode, N, C, H or W < 1, H or W > 4096, in the class mode
 * K outside [2, UZ_CLASS_MAX_K] or first_class outside [0, K), connectivity not 1 or 2, fill_holes not 0 or 1, min_area < 0,
 * keep_largest outside [0, UZ_POST_MAX_KEEP], thr NaN, N C H W >= 2^31, class_map in the binary mode, tensors misaligned
 * (x, labels 4 bytes; stats, comps 8; workspace 16) or overlapping. */
#define UZ_POST_BINARY 0
#define UZ_POST_CLASS 1
#define UZ_POST_MAX_KEEP 8
typedef struct uz_postproc_desc {
  int mode;         /* UZ_POST_* */
  int N, C, H, W;   /* C: channels (binary) or classes K (class mode) */
  int first_class;  /* class mode: the first class that is a plane (1 leaves the background out) */
  int connectivity; /* 1 | 2 */
  int fill_holes;   /* 0 | 1 */
  int min_area;     /* >= 0 */
  int keep_largest; /* 0 .. UZ_POST_MAX_KEEP; 0 = all */
  float thr;        /* binary mode */
  int reserved;
} uz_postproc_desc;
long long uz_postproc_workspace_bytes(const uz_postproc_desc* d); /* < 0: refused */
int uz_postproc_grid(const uz_postproc_desc* d, int* units /* nullable */);
int uz_postproc(const uz_postproc_desc* d, const float* x, unsigned char* mask, int* labels /* nullable */,
                unsigned char* class_map /* nullable */, long long* stats, long long* comps, void* workspace, void* stream);

/* Flip test-time augmentation.  uz_tta.hip.  views: a non-empty bit set of 1 identity, 2 hflip (along W), 4 vflip (along H),
 * 8 hvflip; V = its bit count, the view order is the bit order.
 * uz_flip_views: out[v] (N, C, H, W) fp32 = view v of x; `out` is a HOST array of V device pointers.  One launch.
 * uz_tta_merge : prob (N, C, H, W) fp32 = mean over the views of sigmoid (UZ_POST_BINARY) or softmax over the C = K classes
 *   (UZ_POST_CLASS) of logits[v] (N, C, H, W, `dtype` UZ_F32 or UZ_BF16; a HOST array of V device pointers), each read through
 *   its inverse flip.  fp32 arithmetic, the views added in view order, then divided by V: no atomics, bit-reproducible.  One
 *   launch.  With views = 1 it is the plain sigmoid / softmax.
 * uz_mask_decide: the decision without any component step: mask (N, P, H, W) u8 = x > thr per channel (binary) or the
 *   one-hot planes of argmax_K for the classes from first_class on (class mode, ties to the lowest index), class_map
 *   (N, H, W) u8 = argmax_K (class mode, nullable).  `views` and `dtype` of the descriptor must be valid and are not used. */
typedef struct uz_tta_desc {
  int mode;         /* UZ_POST_* */
  int N, C, H, W;
  int views;        /* bit set, 1 .. 15 */
  int dtype;        /* of the logits of uz_tta_merge */
  int reserved;
} uz_tta_desc;
int uz_tta_num_views(int views); /* V, or < 0 */
int uz_flip_views(const uz_tta_desc* d, const float* x, float* const* out, void* stream);
int uz_tta_merge(const uz_tta_desc* d, const void* const* logits, float* prob, void* stream);
int uz_mask_decide(const uz_tta_desc* d, const float* x, float thr, int first_class, unsigned char* mask,
                   unsigned char* class_map /* nullable */, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sliding-window inference: cutting overlapping windows and blending their probabilities.  uz_tile.hip
 * Along one axis an image of `size` pixels lies on a canvas of D = max(size, window) pixels, at offset
 * floor((window - size) / 2) when it is smaller than the window (else 0).  uz_tile_plan() writes the tile starts on that
 * canvas by the rule of MONAI's sliding_window_inference: step s = max(int(window (1 - overlap)), 1), n = 1 if D == window
 * else ceil((D - window) / s) + 1 tiles, start_i = min(i s, D - window): the last tile is shifted back, none sticks out.
 * It returns n, or -1: size or window < 1, overlap outside [0, 0.75] or NaN, starts null, n > cap or n > UZ_TILE_MAX_AXIS.
 * Pure host code.
 * Tile t of the list is (n ny + iy) nx + ix; ys[ny] / xs[nx] are HOST tables of starts (copied into the kernel arguments),
 * strictly ascending from 0 to D - window with no gap wider than the window.
 * uz_tile_gather: out (tn, C, th, tw) fp32 = the tiles [t0, t0 + tn) of x (N, C, H, W) fp32, an exact copy; canvas pixels
 *   outside the image are 0 (UZ_TILE_PAD_ZERO) or the image mirrored without repeating its edge (UZ_TILE_PAD_REFLECT, the
 *   indexing of torch.nn.functional.pad(mode="reflect"); needs pad < size).  One launch.
 * uz_tile_blend : out (N, C, H, W) fp32 = sum_k w_k p_k / sum_k w_k over the tiles of `tiles` (N ny nx, C, th, tw) fp32
 *   that cover the pixel, in tile order (iy ascending, then ix ascending), w = fmaxf(gh[y'] gw[x'], 1e-3f) at the pixel's
 *   place (y', x') in that tile; gh[th], gw[tw] fp32 DEVICE tables.  One thread owns a pixel: no atomics, fp32 products, sums
 *   and one IEEE division, bit-reproducible.  Only the H x W image region of the canvas is written.  One launch.
 * UZ_EINVAL before any launch: null descriptor / pointer, N, C, H, W, th or tw < 1, ny or nx outside [1, UZ_TILE_MAX_AXIS],
 * a start table that breaks the rule above, more than UZ_TILE_MAX_COVER tiles over one pixel along an axis, unknown pad_mode,
 * reflect with pad >= size, [t0, t0 + tn) outside the list, N C H W, T C th tw or tn C th tw >= 2^31, tensors misaligned
 * (4 bytes) or output overlapping an input. */
#define UZ_TILE_MAX_AXIS 256
#define UZ_TILE_MAX_COVER 8
#define UZ_TILE_PAD_ZERO 0
#define UZ_TILE_PAD_REFLECT 1
typedef struct uz_tile_gather_desc {
  int N, C, H, W;   /* the image batch */
  int th, tw;       /* the window */
  int ny, nx;       /* tiles along H / W */
  int pad_mode;     /* UZ_TILE_PAD_* */
  int t0, tn;       /* the tiles [t0, t0 + tn) of the list of N ny nx */
  int reserved;
} uz_tile_gather_desc;
typedef struct uz_tile_blend_desc {
  int N, C, H, W;   /* the blended output */
  int th, tw;       /* the window */
  int ny, nx;       /* tiles along H / W */
} uz_tile_blend_desc;
int uz_tile_plan(int size, int window, double overlap, int* starts, int cap); /* n, or -1 */
int uz_tile_gather(const uz_tile_gather_desc* d, const int* ys, const int* xs, const float* x, float* out, void* stream);
int uz_tile_blend(const uz_tile_blend_desc* d, const int* ys, const int* xs, const float* tiles, const float* gh,
                  const float* gw, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNETZOO_HIP_H */
