/* vf_hip.h — C ABI of the MI355X (gfx950) backend for the context-encoder GAN hot path.
 *
 * The reference (MKimiSH/video-filler, Lua/Torch7) has no FFI of its own: its compute boundary is
 * Torch7's nn.Module / nn.Criterion object protocol plus ONE backend-swap hook, util.cudnn(net)
 * (util.lua:108-131, called at train.lua:245-258 / train_vid_weighted.lua:330-347).  Each entry point
 * below is what a Torch7-side module class bound through LuaJIT ffi.cdef would call in place of the
 * THNN / THCUNN / cudnn native it replaces; the replaced native and the reference call site are cited
 * per function.  INTEGRATION.md shows the ffi.cdef + nn.Module stubs.
 *
 * Conventions
 *  - every function returns 0 on success, non-zero on error; vf_last_error() gives the message
 *    (Torch7 natives raise THError -> Lua error(); the binding turns non-zero into error()).
 *  - all tensor pointers are DEVICE pointers to fp32 unless stated; nothing is allocated or freed
 *    by the library except through vf_malloc / vf_free; the caller owns every buffer.
 *  - all work is enqueued on the context's stream; no call synchronises the host except
 *    vf_stream_synchronize and vf_memcpy_d2h.
 *  - activations are NHWC ("channels-last": logical B x C x H x W as the reference indexes it,
 *    physical [B][H][W][C]).  Convolution weights are the reference tensors in channels-last too:
 *      nn.SpatialConvolution      logical [Cout][Cin][kH][kW]  physical [Cout][kH][kW][Cin]
 *      nn.SpatialFullConvolution  logical [Cin][Cout][kH][kW]  physical [Cin][kH][kW][Cout]
 *    vf_nchw_to_nhwc / vf_nhwc_to_nchw convert reference-layout buffers at the boundary.
 *  - convolutions: any square kernel / stride / padding is accepted.  The matrix-core kernels serve k = 4 with
 *    (stride, pad) in {(2,1), (1,0)} on power-of-two maps — the shapes of the reference's main nets
 *    (train.lua:89-146,183-196; fineSize 64 / 128 / 256) — everything else runs on the general kernels of
 *    vf_conv_generic.hip behind the same entry points (see "Shapes" below; vf_conv_is_fast tells which).
 */
#ifndef VF_HIP_H
#define VF_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct vf_ctx vf_ctx;

/* activation codes for fused epilogues and vf_act_* */
enum { VF_ACT_NONE = 0, VF_ACT_LRELU = 1, VF_ACT_RELU = 2, VF_ACT_TANH = 3, VF_ACT_SIGMOID = 4 };

/* ---- context / memory / errors ------------------------------------------------------------ */
const char* vf_last_error(void);
int vf_version(void);
/* cutorch.setDevice(opt.gpu) (train.lua:249).  stream = hipStream_t or NULL for the null stream. */
int vf_ctx_create(vf_ctx** out, int device, void* stream);
int vf_ctx_destroy(vf_ctx* ctx);
/* How the conv / full-conv passes of this context form their products (inputs, outputs and accumulators are fp32 in
 * every mode; activations, weights, BatchNorm, criteria and Adam stay fp32 in HBM):
 *   3 (default): fp32-grade on the bf16 matrix pipe — every fp32 operand element is split EXACTLY into three bf16 planes
 *      (x = hi + mid + lo: 3 x 8 bits = the 24-bit significand) on its way into LDS and the six largest cross terms run
 *      on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; the three dropped terms are below 2^-24 of a product, i.e.
 *      one fp32 rounding.  Passes the fp32 parity tolerances unchanged (tests/test_gpu_bf16.py and the whole -m gpu
 *      suite); 1.1-1.4x faster than mode 0 because the bf16 pipe is 16x the f32 one.
 *      Outside the normal range mode 3 is NOT mode 0 (tests/test_gpu_bf16.py covers normals 1e-18 .. 1e18 only):
 *        - a +-inf operand element gives NaN in every output it reaches (the split forms inf - inf), where modes 0 / 1 give
 *          +-inf; NaN operands give NaN in all modes;
 *        - operand elements below ~2^-110 in magnitude lose their low planes (the residuals are bf16 subnormals, which the
 *          matrix pipe flushes): such an element is carried with 8-16 significant bits instead of 24, and fp32 subnormal
 *          operands are treated as zero.  Products that small are far below fp32's own rounding of any sum they join.
 *      Training never produces either (activations and weights of the reference nets are O(1e-3 .. 1e2)); a host that can
 *      feed infinities and needs IEEE behaviour for them selects mode 0.
 *   0: native fp32 operands, v_mfma_f32_32x32x2_f32 (an fmaf chain, bit for bit).
 *   1: operands ROUNDED to bf16 (round-to-nearest-even), one product term — opt-in, ~2^-9 relative operand rounding. */
int vf_ctx_set_mfma_mode(vf_ctx* ctx, int mode);
int vf_ctx_set_stream(vf_ctx* ctx, void* stream);
/* scratch for split-K slabs and reduction partials; caller-owned, >= vf_workspace_bytes_hint(). */
int vf_ctx_set_workspace(vf_ctx* ctx, void* ptr, size_t bytes);
size_t vf_workspace_bytes_hint(void);
int vf_stream_synchronize(vf_ctx* ctx);
int vf_malloc(void** out, size_t bytes);
int vf_free(void* ptr);
int vf_memcpy_h2d(vf_ctx* ctx, void* dst, const void* src, size_t bytes);
int vf_memcpy_d2h(vf_ctx* ctx, void* dst, const void* src, size_t bytes); /* synchronises */
int vf_zero(vf_ctx* ctx, void* ptr, size_t bytes);                       /* Tensor:zero() */
/* bias zeroing sweep `m.bias:zero()` over every *Convolution* module (train.lua:279-280):
 * zero nseg segments base[offs[i] .. offs[i]+lens[i]) ; offs/lens are DEVICE int64 arrays. */
int vf_zero_segments(vf_ctx* ctx, float* base, const int64_t* offs, const int64_t* lens, int nseg);
int vf_nchw_to_nhwc(vf_ctx* ctx, const float* src, float* dst, int B, int C, int H, int W);
int vf_nhwc_to_nchw(vf_ctx* ctx, const float* src, float* dst, int B, int C, int H, int W);

/* ---- nn.SpatialConvolution (THNN SpatialConvolutionMM / cudnn.SpatialConvolution) ----------
 * Shapes.  The matrix-core kernels (vf_conv.hip, vf_pgemm.hip) serve the reference's main nets: kernel 4x4 with
 * stride 2 pad 1 on maps whose H and W are POWERS OF TWO (pixel coordinates are split with shifts and masks), and the
 * 4x4 stride 1 pad 0 bottleneck pair on a 4x4 / 1x1 map (train.lua:89-146,183-199).  Every other geometry — the option
 * branches' 5x5 / 1x1 convolutions, or 4x4 stride 2 on a map that is not a power of two — is served by the general
 * kernels of vf_conv_generic.hip through the same entry points: same results to the fp32 tolerances, native fp32
 * arithmetic whatever the context's product mode, and several times slower (they are not on the training hot path:
 * fineSize is 64 / 128 / 256 in every recipe of the reference).  vf_conv_is_fast reports which path a geometry takes. */
/* updateOutput.  y[B][Ho][Wo][Cout] = act(conv(x[B][H][W][Cin], w) + bias).  bias may be NULL.
 * act/slope fuse a following in-place nn.LeakyReLU / nn.ReLU / nn.Tanh / nn.Sigmoid (train.lua:90,196). */
int vf_conv_is_fast(int H, int W, int k, int stride, int pad);
int vf_conv2d_fwd(vf_ctx* ctx, const float* x, const float* w, const float* bias, float* y, int B, int H,
                  int W, int Cin, int Cout, int k, int stride, int pad, int act, float slope);
/* updateGradInput.  gx[B][H][W][Cin] from gy[B][Ho][Wo][Cout]. */
int vf_conv2d_bwd_data(vf_ctx* ctx, const float* gy, const float* w, float* gx, int B, int H, int W,
                       int Cin, int Cout, int k, int stride, int pad);
/* accGradParameters(scale = 1).  gw = beta*gw + dW ; gb = beta*gb + db (gb may be NULL).
 * beta = 1 is Torch's accumulate; beta = 0 overwrites (saves the gradParameters:zero() pass). */
/* updateGradInput of a conv whose INPUT is the in-place activated output of the module before it (train.lua:89-91:
 * conv -> LeakyReLU(0.2, true) -> conv): gx = (W^T * gy) .* act'(x_act), i.e. this conv's updateGradInput and the
 * nn.LeakyReLU:updateGradInput pass over the same tensor in one epilogue.  x_act is this conv's own input. */
int vf_conv2d_bwd_data_act(vf_ctx* ctx, const float* gy, const float* w, float* gx, const float* x_act, int act,
                           float slope, int B, int H, int W, int Cin, int Cout, int k, int stride, int pad);
int vf_conv2d_bwd_weight(vf_ctx* ctx, const float* x, const float* gy, float* gw, float* gb, int B, int H,
                         int W, int Cin, int Cout, int k, int stride, int pad, float beta);

/* ---- nn.SpatialFullConvolution (THNN SpatialFullConvolution; train.lua:134-146) ------------- */
/* x[B][H][W][Cin] -> y[B][Ho][Wo][Cout], Ho = (H-1)*stride - 2*pad + k. */
int vf_deconv2d_fwd(vf_ctx* ctx, const float* x, const float* w, const float* bias, float* y, int B, int H,
                    int W, int Cin, int Cout, int k, int stride, int pad, int act, float slope);
int vf_deconv2d_bwd_data(vf_ctx* ctx, const float* gy, const float* w, float* gx, int B, int H, int W,
                         int Cin, int Cout, int k, int stride, int pad);
int vf_deconv2d_bwd_weight(vf_ctx* ctx, const float* x, const float* gy, float* gw, float* gb, int B, int H,
                           int W, int Cin, int Cout, int k, int stride, int pad, float beta);

/* ---- the same passes from PRE-SPLIT operands (vf_pgemm.hip) ----------------------------------
 * The default product mode forms every fp32 product from three bf16 planes per operand (x = hi + mid + lo, exact: see
 * vf_ctx_set_mfma_mode).  The entry points above split their fp32 operands inside the GEMM, in every pass that reads
 * them; these take operands split ONCE by whoever produced them — `planes` = bf16 [3][n], plane q at q * n elements:
 *   vf_planes_split    any fp32 tensor of n elements (n % 4 == 0)
 *   vf_weight_planes   a conv / full-conv weight, physical [d0][16][d1]: native planes [3][d0][16][d1] and (optional)
 *                      transposed planes [3][d1][16][d0] — the data-gradient / full-conv forward passes walk the transpose
 *   vf_bn_train_fwd_pre / vf_bn_bwd_pre write the planes of their output beside it (y_planes / gx_planes, may be NULL)
 * and compute bit for bit the six-term products of mode 3 (another summation order over K: same parity tolerances).
 * 4x4, stride 2, pad 1 only, channel counts of the gathered operand % 32 == 0, output channels >= 32 and % 4 == 0, more
 * than 64 GEMM rows (vf_pconv_supported says; everything else stays with the entry points above).
 *   vf_pconv_gather    conv forward (ap = x planes [B][H][W][Cin], wp = native planes of w [Cout][16][Cin]) and full-conv
 *                      data-gradient (ap = gy planes, wp = native planes of the full-conv weight [Cin_full][16][Cout_full])
 *   vf_pconv_scatter   conv data-gradient (ap = gy planes on the LOW-res grid H x W, wp = transposed planes [Cin][16][Cout];
 *                      dmask/dact/dslope as vf_conv2d_bwd_data_act) and full-conv forward (ap = x planes, wp = transposed
 *                      planes of the full-conv weight [Cout_full][16][Cin_full], bias, act); output is 2H x 2W
 * Both honour a pending vf_bn_fuse_next_* attachment like the entry points above. */
int vf_planes_split(vf_ctx* ctx, const float* x, void* planes, int64_t n);
/* vf_conv2d_fwd that also leaves the planes of y (in its epilogue for the 3-channel image-side layers, train.lua:89,183) */
int vf_conv2d_fwd_planes(vf_ctx* ctx, const float* x, const float* w, const float* bias, float* y, void* y_planes, int B,
                         int H, int W, int Cin, int Cout, int k, int stride, int pad, int act, float slope);
int vf_weight_planes(vf_ctx* ctx, const float* w, void* planes_native, void* planes_transposed, int d0, int d1);
/* the same for n weights in one launch: desc_dev = device array of n records {const float* w; void* native; void* transposed;
 * int d0, d1, gx = ceil(d0/32), gz = ceil(d1/32), blk_off (first block of the record: running sum of gx*16*gz), pad;} (48 bytes
 * each); blocks = the total.  A net refreshes its weight planes once per parameter update (optim.adam, train.lua:421-424). */
int vf_weight_planes_multi(vf_ctx* ctx, const void* desc_dev, int n, int blocks);
int vf_pconv_supported(int B, int H, int W, int Cin, int Cout, int k, int stride, int pad, int transposed);
/* The planes path in the bf16-operand mode (vf_ctx_set_mfma_mode 1): `planes` is then ONE plane, bf16 [1][n], the operand rounded
 * to nearest-even by its producer — every producer above (vf_planes_split, vf_weight_planes[_multi], the y_planes / gx_planes
 * of the BatchNorm entries, vf_conv2d_fwd_planes) writes that form when the context is in mode 1 — and the GEMMs issue one MFMA
 * per product instead of six (k_pconv_dma<.., NPL = 1>, k_pwgrad_group<.., NPL = 1>).  Served shapes are narrower (whole
 * 64-channel K steps, whole 64 x 64 tiles): vf_pconv_supported_in_mode(1, ...); mode 3 = vf_pconv_supported; mode 0: never.
 * Results equal the in-kernel-rounding kernels' (same products, another summation order). */
int vf_pconv_supported_in_mode(int mfma_mode, int B, int H, int W, int Cin, int Cout, int k, int stride, int pad, int transposed);
/* Which kernel serves a planes pass is a tiling decision of the library (kernel map).  Two of the choices can be switched
 * per process, for same-box A/B runs and for the tests that compare the kernels bit for bit: gather_patch (0 / 1: k_pconv_patch_g for
 * the gather passes on whole 128-row tiles; default 1, env VF_PG_GPATCH) and scatter_patch (0 off, 1 auto, 2 / 4 parity classes per
 * block of k_pconv_patch_tr; default 1, env VF_PG_PATCH).  A negative value leaves a setting as it is.  Results do not depend on it:
 * every choice forms the same six-term products in the same K order per output element. */
int vf_pconv_set_routing(int gather_patch, int scatter_patch);
int vf_pconv_gather(vf_ctx* ctx, const void* ap, const void* wp, const float* bias, float* y, int B, int H, int W, int Cin,
                    int Cout, int act, float slope);
int vf_pconv_scatter(vf_ctx* ctx, const void* ap, const void* wp, const float* bias, float* y, int B, int H, int W, int Cin,
                     int Cout, int act, float slope, const float* dmask, int dact, float dslope);
/* accGradParameters with the planes of BOTH operands at hand (x_planes: bf16 [3][B*H*W*Cin], gy_planes: bf16 [3][B*Ho*Wo*Cout],
 * the layout vf_planes_split writes; x and gy themselves are still needed: bias gradient, shapes the planes kernel does not
 * take).  The weight gradient runs on k_pwgrad_group — both operands DMA-staged as [pixel][channel] tiles, fragments by the
 * transposing LDS read — when the product mode is 3, stride 2 pad 1, the low-resolution operand has a multiple of 128
 * channels (or exactly 64: the kernel's 64-row tile form), the gathered one a multiple of 64 and the pixel count is a multiple of 32; otherwise exactly
 * vf_conv2d_bwd_weight / vf_deconv2d_bwd_weight.  Same six-term products, another summation order over pixels. */
int vf_conv2d_bwd_weight_planes(vf_ctx* ctx, const float* x, const float* gy, const void* x_planes, const void* gy_planes, float* gw,
                                float* gb, int B, int H, int W, int Cin, int Cout, int k, int stride, int pad, float beta);
int vf_deconv2d_bwd_weight_planes(vf_ctx* ctx, const float* x, const float* gy, const void* x_planes, const void* gy_planes,
                                  float* gw, float* gb, int B, int H, int W, int Cin, int Cout, int k, int stride, int pad,
                                  float beta);

/* ---- nn.SpatialBatchNormalization (THNN/THCUNN BatchNormalization; train.lua:92) ------------ */
/* Training forward in two phases so a data-parallel caller can all-reduce `sums` in between:
 *   vf_bn_stats     : sums[0..C) = sum(x - shift), sums[C..2C) = sum((x - shift)^2)  (DOUBLE), shift = running_mean
 *   vf_bn_finalize  : mean/invstd from sums over n_total rows; updates running stats (momentum, unbiased var)
 *   vf_bn_apply     : y = act((x - mean) * invstd * gamma + beta)     (y may alias x)
 * vf_bn_train_fwd runs the three back to back.  npix = B*H*W rows of C channels. */
int vf_bn_stats(vf_ctx* ctx, const float* x, const float* shift, double* sums, int64_t npix, int C);
int vf_bn_finalize(vf_ctx* ctx, const double* sums, float* running_mean, float* running_var, float* save_mean,
                   float* save_invstd, int64_t n_total, int C, float momentum, float eps);
int vf_bn_apply(vf_ctx* ctx, const float* x, float* y, const float* gamma, const float* beta, const float* mean,
                const float* invstd, int64_t npix, int C, int act, float slope);
int vf_bn_train_fwd(vf_ctx* ctx, const float* x, float* y, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float* save_mean, float* save_invstd, double* sums,
                    int64_t npix, int C, float momentum, float eps, int act, float slope);
/* evaluate() mode (test_vid.lua:48): running statistics. */
int vf_bn_eval_fwd(vf_ctx* ctx, const float* x, float* y, const float* gamma, const float* beta,
                   const float* running_mean, const float* running_var, int64_t npix, int C, float eps, int act,
                   float slope);
/* Backward, also two-phase: vf_bn_bwd_stats gives sums[0..C) = sum(g), sums[C..2C) = sum(g*(x-mean)) with
 * g = gy masked by the fused activation's derivative (y_act = the activated output; NULL when act = NONE);
 * vf_bn_bwd_apply writes gx (may be NULL) and ggamma/gbeta (may be NULL) = pbeta*old + new. */
int vf_bn_bwd_stats(vf_ctx* ctx, const float* x, const float* y_act, const float* gy, const float* save_mean,
                    double* sums, int64_t npix, int C, int act, float slope);
int vf_bn_bwd_apply(vf_ctx* ctx, const float* x, const float* y_act, const float* gy, float* gx, float* ggamma,
                    float* gbeta, const float* gamma, const float* save_mean, const float* save_invstd,
                    const double* sums, int64_t npix, int64_t n_total, int C, int act, float slope, float pbeta);
int vf_bn_bwd(vf_ctx* ctx, const float* x, const float* y_act, const float* gy, float* gx, float* ggamma,
              float* gbeta, const float* gamma, const float* save_mean, const float* save_invstd, double* sums,
              int64_t npix, int C, int act, float slope, float pbeta);
/* The same two calls over a batch that is the concatenation of `groups` independent batches of npix_per_group pixels
 * each (netD's real and fake passes of one closure run as one tensor, train.lua:300-349): statistics, running-average
 * updates and backward sums are per group, in group order — exactly what `groups` separate calls would compute, in one
 * launch per stage.  save_mean / save_invstd are [groups][C], sums is [groups][2C]; gamma/beta gradients accumulate the
 * groups' contributions in order (pbeta applies to the first). */
int vf_bn_train_fwd_groups(vf_ctx* ctx, const float* x, float* y, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float* save_mean, float* save_invstd,
                           double* sums, int64_t npix_per_group, int C, int groups, float momentum, float eps,
                           int act, float slope);
int vf_bn_bwd_groups(vf_ctx* ctx, const float* x, const float* y_act, const float* gy, float* gx, float* ggamma,
                     float* gbeta, const float* gamma, const float* save_mean, const float* save_invstd,
                     double* sums, int64_t npix_per_group, int C, int groups, int act, float slope, float pbeta);

/* BatchNorm statistics as a by-product of the convolution that produces the tensor (train.lua:91-92: every BatchNorm of the
 * nets follows a convolution).  vf_bn_fuse_next_fwd / _bwd attach a request to the context; the NEXT vf_conv2d_fwd /
 * vf_deconv2d_fwd (fwd) or vf_conv2d_bwd_data / vf_deconv2d_bwd_data (bwd) on it leaves per-tile partial sums in `part`
 * ([groups][rows][2][C] doubles, rows <= part_rows_cap / groups) from its epilogue (or from its split-K combine), and
 * vf_bn_fuse_result says how many rows per group it wrote — 0 when that launch could not (thin or generic shapes, tiles
 * that straddle a batch group): the caller then runs the plain vf_bn_train_fwd / vf_bn_bwd.
 *   fwd: sums of (v - shift), (v - shift)^2 of the conv output v, shift = running_mean[C]  -> vf_bn_train_fwd_pre
 *   bwd: the data-gradient pass stores its output ALREADY MASKED by the derivative of the activation fused behind the
 *        BatchNorm (act, y_act = the activated BatchNorm output; nn.LeakyReLU / nn.ReLU:updateGradInput) and sums
 *        g and g * (x - save_mean), x = the BatchNorm's input                                   -> vf_bn_bwd_pre
 * The _pre calls are vf_bn_train_fwd_groups / vf_bn_bwd_groups without their statistics pass (g_masked: no activation);
 * y_planes / gx_planes (may be NULL): the three bf16 planes of the output, [3][groups * npix_per_group * C], written beside
 * it for a vf_pconv_* consumer. */
int vf_bn_train_fwd_planes(vf_ctx* ctx, const float* x, float* y, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float* save_mean, float* save_invstd, double* sums,
                           int64_t npix_per_group, int C, int groups, float momentum, float eps, int act, float slope,
                           void* y_planes);      /* vf_bn_train_fwd_groups + the planes of y */
int vf_bn_bwd_planes(vf_ctx* ctx, const float* x, const float* y_act, const float* gy, float* gx, float* ggamma,
                     float* gbeta, const float* gamma, const float* save_mean, const float* save_invstd, double* sums,
                     int64_t npix_per_group, int C, int groups, int act, float slope, float pbeta,
                     void* gx_planes);           /* vf_bn_bwd_groups + the planes of gx */
int vf_bn_fuse_next_fwd(vf_ctx* ctx, const float* shift, double* part, int part_rows_cap, int groups);
int vf_bn_fuse_next_bwd(vf_ctx* ctx, const float* x, const float* y_act, int act, float slope, const float* save_mean,
                        double* part, int part_rows_cap, int groups);
int vf_bn_fuse_result(vf_ctx* ctx, int* rows_per_group);
int vf_bn_train_fwd_pre(vf_ctx* ctx, const double* part, int rows_per_group, const float* x, float* y, const float* gamma,
                        const float* beta, float* running_mean, float* running_var, float* save_mean, float* save_invstd,
                        double* sums, int64_t npix_per_group, int C, int groups, float momentum, float eps, int act,
                        float slope, void* y_planes);
int vf_bn_bwd_pre(vf_ctx* ctx, const double* part, int rows_per_group, const float* x, const float* g_masked, float* gx,
                  float* ggamma, float* gbeta, const float* gamma, const float* save_mean, const float* save_invstd,
                  double* sums, int64_t npix_per_group, int C, int groups, float pbeta, void* gx_planes);

/* ---- pointwise modules, criteria, Adam, layout (vf_core.hip): common rules ------------------------------------------
 * n <= 0 (an empty tensor; for vf_gdl_* H = W = 1, for the transposes B*C*H*W = 0, for vf_zero_segments nseg <= 0): the call
 *   returns 0, launches nothing over its operands and writes nothing — not the output, not the loss slot.  (vf_adam_step still
 *   advances t_dev: it is vf_adam_prep + vf_adam_apply.)
 * alignment: the pointwise modules and vf_mse_fwd read 16 bytes at a time when every operand is 16-byte aligned; otherwise they
 *   take a scalar route for n <= 65536 (sub-batch views of small tensors) and refuse larger n.  vf_recon_grad_mix takes its
 *   scalar kernel for any n when an operand is not 16-byte aligned or n % 4 != 0.  vf_adam_* refuse unaligned operands.
 *   Every float operand must be 4-byte aligned. */
/* ---- pointwise modules (nn.LeakyReLU / ReLU / Tanh / Sigmoid; train.lua:90,146,196) --------- */
int vf_act_fwd(vf_ctx* ctx, const float* x, float* y, int64_t n, int act, float slope); /* y may alias x */
/* gx = gy * act'(.) evaluated from the ACTIVATED output y (in-place semantics); gx may alias gy */
int vf_act_bwd(vf_ctx* ctx, const float* y, const float* gy, float* gx, int64_t n, int act, float slope);
/* y = a*x + b*y  (Tensor:mul / :add(alpha, src), train.lua:382) */
int vf_axpby(vf_ctx* ctx, float a, const float* x, float b, float* y, int64_t n);
/* y = y .* x  (Tensor:cmul, train_vid_weighted.lua:497) */
int vf_cmul(vf_ctx* ctx, const float* x, float* y, int64_t n);
/* y = a*y + b   (input_mask:mul(1-lambda):add(lambda), train_vid_weighted.lua:494) */
int vf_scale_shift(vf_ctx* ctx, float* y, float a, float b, int64_t n);
/* out = mask != 0 ? fake : real   (maskedSelect + maskedCopy, train_vid_weighted.lua:430-432) */
int vf_masked_compose(vf_ctx* ctx, float* out, const float* real, const float* fake, const float* mask,
                      int64_t n);

/* ---- criteria: loss scalars are written to DEVICE doubles (no host sync) -------------------- */
/* nn.BCECriterion (eps 1e-12, sizeAverage; train.lua:204).  target = constant label (label:fill). */
int vf_bce_fwd(vf_ctx* ctx, const float* x, float label, int n, double* loss);
int vf_bce_bwd(vf_ctx* ctx, const float* x, float label, float* gx, int n);
/* criterion:forward and criterion:backward of the same scores in ONE launch, for one group of n scores or for two consecutive
 * groups with their own labels (netD's real and fake halves, train.lua:331-349): loss0 / loss1 get the group means, gx the
 * gradient of all groups * n scores.  Element for element vf_bce_fwd + vf_bce_bwd. */
int vf_bce_fwd_bwd(vf_ctx* ctx, const float* x, float label0, float label1, int n_per_group, int groups, double* loss0,
                   double* loss1, float* gx);
/* nn.MSECriterion (train.lua:207).  loss = mean((x-t)^2); gx = (2/n)(x-t). */
int vf_mse_fwd(vf_ctx* ctx, const float* x, const float* t, int64_t n, double* loss);
int vf_mse_bwd(vf_ctx* ctx, const float* x, const float* t, float* gx, int64_t n);
/* Fused generator reconstruction gradient (train_vid_weighted.lua:489-503,523-528 / train.lua:377-399):
 *   loss  = mean((x-t)^2)
 *   df_dg = alpha*df_dg + (2/n)(x-t) * wgt,   wgt = c0 + c1*mask[i]            (mask != NULL)
 *                                             wgt = inside band ? c0 : c0 + c1  (mask == NULL, band > 0:
 *                                                   rows/cols [band, HW-band) of an HW x HW image are "inside")
 * n = B*HW*HW*C elements, NHWC.  The band form is for SQUARE maps only (the call takes one HW for rows and columns and refuses
 * an n that is not a multiple of HW*HW*C); the mask form and band = 0 take any n, HW and C are then unused. */
int vf_recon_grad_mix(vf_ctx* ctx, float* df_dg, const float* x, const float* t, const float* mask, float alpha,
                      float c0, float c1, int band, int HW, int C, int64_t n, double* loss);
/* nn.GDLCriterion(1):forward (gdl_criterion.lua:38-45) incl. the flattened-pairing quirk. */
int vf_gdl_fwd(vf_ctx* ctx, const float* yhat, const float* y, int B, int H, int W, int C, double* loss);
/* updateGradInput (gdl_criterion.lua:47-53): gyhat = d loss / d yhat, same shapes.  No driver of the reference calls it
 * (train_vid_weighted.lua:523-528 adds the forward VALUE to the loss and uses the MSE gradient); provided so that
 * nn.GDLCriterion is a complete nn.Criterion.  Derivative convention of THNN Abs / AbsCriterion: +1 at 0. */
int vf_gdl_bwd(vf_ctx* ctx, const float* yhat, const float* y, float* gyhat, int B, int H, int W, int C);
/* nn.MaskedMSECriterion(w) (MaskedMSECriterion.lua:29-41); mask is uint8 0/1. */
int vf_masked_mse_fwd(vf_ctx* ctx, const float* x, const float* xhat, const uint8_t* mask, float w, int64_t n,
                      double* loss);
int vf_masked_mse_bwd(vf_ctx* ctx, const float* x, const float* xhat, const uint8_t* mask, float w, float* gx,
                      int64_t n);

/* ---- optim.adam (train.lua:421-424) -------------------------------------------------------- */
/* One fused pass over the flat parameter vector (28 B/param).  t_dev points to TWO DEVICE int32 words:
 * t_dev[0] = state.t (the call increments it first), t_dev[1] = scratch for the fp32 step size
 * lr*sqrt(1-beta2^t)/(1-beta1^t), computed on the device in double so a captured graph replays correctly.
 * Hyper-parameters are doubles, as Lua numbers are. */
int vf_adam_step(vf_ctx* ctx, float* x, const float* g, float* m, float* v, int64_t n, double lr, double beta1,
                 double beta2, double eps, int32_t* t_dev);
/* The two halves of vf_adam_step, so that one update can be applied range by range (and on more than one stream):
 * vf_adam_prep advances the step count and derives the step size ONCE (t_dev[0] += 1, t_dev[1] = bits of
 * lr*sqrt(1-beta2^t)/(1-beta1^t)); vf_adam_apply updates x[0..n) (any 16-byte aligned sub-range of the flat
 * vectors) with that step size.  prep + apply over the whole vector == vf_adam_step. */
int vf_adam_prep(vf_ctx* ctx, double lr, double beta1, double beta2, int32_t* t_dev);
int vf_adam_apply(vf_ctx* ctx, float* x, const float* g, float* m, float* v, int64_t n, double beta1, double beta2,
                  double eps, const int32_t* t_dev);
/* the same pass over several element ranges of the flat vectors in ONE launch (offsets / lengths in floats, multiples of 4, at most 8
 * ranges; host arrays): the generator's vector around the slices vf_net_adam_fused takes */
int vf_adam_apply_ranges(vf_ctx* ctx, float* x, const float* g, float* m, float* v, const int64_t* offsets, const int64_t* lengths,
                         int nranges, double beta1, double beta2, double eps, const int32_t* t_dev);
/* optim.adam applied inside the weight-gradient kernel of a bottleneck layer (train.lua:104 conv nef*8 -> nBottleneck on a 4x4
 * map, :134 full-conv nBottleneck -> ngf*8 onto one; THNN accGradParameters with K = batch):
 *   g[n][col] = sum_{k < K} U[k][n] * V[k][col]        U = [K][Nu] (the 1x1-map side), V = [K][Ncols] (the 4x4-map side, Ncols = 16*C)
 * is formed in the accumulators and consumed there: x, m, v = [Nu][Ncols] slices of the flat parameter vector and of the optimiser
 * state are read and written once — 24 B per weight where accGradParameters + vf_adam_apply move 32 (those two tensors are 92 % of
 * train.lua's generator).  g (may be NULL) also receives the gradient (gradParameters stays complete; 28 B).  Requires a fresh
 * gradient (zeroGradParameters before the backward pass, as both closures do) and t_dev after vf_adam_prep; element for element
 * the update of vf_adam_apply.  vf_wgrad_adam_outer_supported: 1 when the shape is the kernel's (Ncols % 128 == 0, Nu even, >= 64). */
int vf_wgrad_adam_outer_supported(int K, int Nu, int Ncols);
int vf_wgrad_adam_outer(vf_ctx* ctx, const float* U, const float* V, int K, int Nu, int Ncols, float* x, float* m, float* v,
                        float* g, double beta1, double beta2, double eps, const int32_t* t_dev);
/* the same with the batch rows gathered from several ranks (data parallel): row k lives in segment k / rows_per_seg at row
 * k % rows_per_seg of it, the segments seg_stride floats apart (U and V both); g = gscale * sum (1 / world: the mean over ranks).
 * K % rows_per_seg == 0, seg_stride % 4 == 0; U, V 8-byte aligned. */
int vf_wgrad_adam_outer_gathered(vf_ctx* ctx, const float* U, const float* V, int K, int rows_per_seg, int64_t seg_stride, int Nu,
                                 int Ncols, float* x, float* m, float* v, float* g, float gscale, double beta1, double beta2,
                                 double eps, const int32_t* t_dev);
/* the same for rows [row0, row0 + nrows) of the tensors only (row0 even, nrows even and >= 64; x, m, v, g point at row 0): the
 * data-parallel update sharded by weight rows — bit for bit what the whole-tensor call gives those rows */
int vf_wgrad_adam_outer_rows(vf_ctx* ctx, const float* U, const float* V, int K, int rows_per_seg, int64_t seg_stride, int Nu, int Ncols,
                             int row0, int nrows, float* x, float* m, float* v, float* g, float gscale, double beta1, double beta2,
                             double eps, const int32_t* t_dev);

/* ---- batch preparation and the inference tile loop (the data formats either side of the closures) ---------
 * train.lua:284-298: from the loader's batch (B x C x fs x fs planar, [-1,1]) produce the NHWC generator input with
 * the centre hole [fs/4+ov, 3fs/4-ov)^2 painted with fill[c] (DEVICE float[C]; 2*{117,104,123}/255-1 in the reference)
 * and the NHWC clone of the centre crop [fs/4, 3fs/4)^2 taken BEFORE painting. */
int vf_center_prepare(vf_ctx* ctx, const float* batch_nchw, float* ctx_nhwc, float* center_nhwc, const float* fill,
                      int B, int C, int fs, int overlapPred);
/* datavid/donkey_folder.lua:135-189 (trainHook, withMask) for ONE sample: crop the decoded clip (C x iH x iW planar,
 * [0,1]) at 0-based (w1, h1), build the mask (nblocks == 0: crop of the mask image `mask` (iH x iW), non-zero =
 * masked, :162-166; nblocks > 0: randomBlockMask's squares of side block_size at 1-based HOST coordinates tlx/tly,
 * :114-129), fill masked pixels with mask_value, mirror horizontally if flip (:178-183), map [0,1] -> [-1,1]
 * (:185-187).  Outputs are fs x fs x C NHWC: full clip, masked clip, mask as 0/1 floats. */
int vf_clip_prepare(vf_ctx* ctx, const float* clip, const float* mask, float* full, float* masked, float* maskout,
                    int C, int iH, int iW, int fs, int w1, int h1, int flip, float mask_value, int nblocks,
                    int block_size, const int* tlx, const int* tly);
/* test_vid_wholeim.lua:159-205: the padded planar clip (groups*nc x H x W; H, W multiples of fs) cut into
 * (H/fs)*(W/fs) tiles, all gathered into ONE NHWC batch — row (tile*groups + g) is fs x fs x nc — so the generator
 * runs once instead of once per tile (evaluate-mode BatchNorm makes that exact); vflip (DEVICE uint8 per tile, or
 * NULL) flips a tile vertically on the way in (:167-170) and back on the way out (:191-197). */
int vf_tiles_gather(vf_ctx* ctx, const float* full, float* tiles, int groups, int nc, int H, int W, int fs,
                    const unsigned char* vflip);
int vf_tiles_scatter(vf_ctx* ctx, const float* tiles, float* out, int groups, int nc, int H, int W, int fs,
                     const unsigned char* vflip);

/* Overlapped, blended inference windows (the rule is tests/window_blend_ref.py).  The clip is F frames of
 * nc x H x W, planar (F*nc) x H x W; a window is inputLen frames x fs x fs.  Per axis the windows start at 0, stride,
 * 2 stride, ... while they fit, and one more at n - size if the last ends before n (y, x: size fs, stride `stride`;
 * t: size inputLen, stride `stride_t`); n >= size, 1 <= stride <= size and 2 stride >= size, nothing is padded.  Window
 * (it, iy, ix) has number (it*NY + iy)*NX + ix and is batch row `number`; channel k of the row is frame origin + k / nc,
 * colour k % nc.  All three check their arguments before any launch, allocate nothing and do not synchronise.
 * vf_windows_gather: rows [w0, w0 + nw) of the window batch, NHWC nw x fs x fs x (inputLen*nc). */
int vf_windows_gather(vf_ctx* ctx, const float* frames, float* tiles, int F, int nc, int H, int W, int inputLen, int fs,
                      int stride, int stride_t, int w0, int nw);
/* Adds the net's output rows [w0, w0 + nw) (NHWC, as gathered) into the fp32 accumulator acc ((F*nc) x H x W, zeroed by
 * the caller before the first chunk): per sample, for every covering window of the chunk in ascending number,
 * acc = fadd(acc, fmul(float(w), v)) with the integer weight w = wt wy wx, w.(i) = min(i + 1, size - i, size - stride + 1).
 * No atomics; chunks issued in ascending order on one stream give the same bits whatever their size. */
int vf_windows_accumulate(vf_ctx* ctx, const float* tiles, float* acc, int F, int nc, int H, int W, int inputLen, int fs,
                          int stride, int stride_t, int w0, int nw);
/* out = fdiv(acc, float(sum of the covering weights)), the sum an integer of the geometry.  With frames (planar, [-1,1]),
 * mask (nc x H x W uint8, non-zero = hole), inpaint and full all given it also does test_vid_wholeim.lua:214-224: inpaint =
 * out inside the mask, the frame outside, and out, inpaint, full = x * 0.5 + 0.5 of out, inpaint, frames (the bits of
 * vf_masked_compose and vf_scale_shift); with all four NULL, out is the plain quotient. */
int vf_windows_finish(vf_ctx* ctx, const float* acc, const float* frames, const unsigned char* mask, float* out, float* inpaint,
                      float* full, int F, int nc, int H, int W, int inputLen, int fs, int stride, int stride_t);

/* ---- Torch7 image.scale (bilinear) and the loaders built on it (vf_image.hip) --------------------
 * Bit-identical to the float32 restatement of image.c's scaleBilinear: rows first (W -> width), then columns
 * (H -> height), one rounding per operation.  src_layout 0: float planar N x C x H x W; src_layout 1: decoded uint8
 * N x H x W x C (interleaved, as decoders return it), read as b / 255 in float (image.load(path, nc, 'float')).
 * Sides must lie in [1, 65535].
 * vf_image_scale: image.scale of N frames of one size into float planar N x C x height x width. */
int vf_image_scale(vf_ctx* ctx, const void* src, int src_layout, float* dst, int N, int C, int H, int W, int height,
                   int width);
/* The Byte path (masks): uint8 planar N x C x H x W -> uint8 planar N x C x height x width; the intermediate row pass
 * and the result are rounded through image.c's FromIntermediate (+0.5, clamp to [0, 255], truncate). */
int vf_image_scale_u8(vf_ctx* ctx, const unsigned char* src, unsigned char* dst, int N, int C, int H, int W, int height,
                      int width);
/* data/donkey_folder.lua:40-88 (trainHook of train.lua's loader) for ONE image: image.scale to height x width, crop
 * fs x fs at the 0-based corner (w1, h1) of the scaled image, mirror horizontally if flip, map [0,1] -> [-1,1]
 * (mul(2):add(-1)); out: C x fs x fs planar (one row of the B x C x fs x fs loader batch).  Only the crop's pixels
 * are evaluated; the scaled image is never stored. */
int vf_image_hook2d(vf_ctx* ctx, const void* src, int src_layout, float* out, int C, int H, int W, int height, int width,
                    int fs, int w1, int h1, int flip);
/* test_vid_wholeim.lua:109-141 (loadImages): image.scale of N frames to height x width, pixels where fill_mask (DEVICE
 * uint8 C x height x width, shared by the frames, non-zero = masked; or NULL) is set replaced by fill_value
 * (maskedFill), zero-padded bottom-right to outh x outw, then mul(2):add(-1) over the whole padded frame (padding
 * becomes -1).  out: float planar N x C x outh x outw. */
int vf_image_whole_frames(vf_ctx* ctx, const void* src, int src_layout, float* out, int N, int C, int H, int W, int height,
                          int width, int outh, int outw, const unsigned char* fill_mask, float fill_value);
/* datavid/donkey_folder.lua:148,165 on the device clip (C x iH x iW planar float) and the Byte mask (iH x iW uint8, or
 * NULL): out (DEVICE double[2]) = {sum of the fs x fs crop at 0-based (w1, h1) over all C channels, accumulated in
 * double; max of the same crop of the mask}.  One block, fixed order: deterministic. */
int vf_crop_stats(vf_ctx* ctx, const float* clip, const unsigned char* mask, int C, int iH, int iW, int fs, int w1, int h1,
                  double* out);
/* datavid/donkey_wholeim.lua:141-215 (trainHook of train_wholeim_input.lua's loader) for ONE 3-channel frame, the
 * module-global mask already scaled (:72; mask: DEVICE uint8 height x width, non-zero = masked, or NULL: all zero):
 * image.scale to height x width; maskedFill with mask_value; frame, masked frame and mask shifted up-left by
 * (crop_h-1, crop_w-1) — both 1-based draws — with ZERO bands bottom and right; all three mirrored over the full width
 * if flip; windows of fs x fs at steps floor((height-fs)/(arr_h-1)), floor((width-fs)/(arr_w-1)), rows outermost;
 * mul(2):add(-1) on the frames.  Channels-last rows of the loader batch: masked fs x fs x (3*arr_h*arr_w) (every
 * window of the masked frame), full and maskout fs x fs x 12 (windows (0,0), (0,1), (1,0), (1,1) of the frame and of
 * the mask as 0/1 floats).  sum (DEVICE double[1]): the sum of window (0,0) of the shifted, mirrored, unmasked frame
 * before the [-1,1] map (the dark test of :188-189), accumulated in double in a fixed order.  Only the windows' pixels
 * are evaluated; the scaled frame is never stored.  The geometry the reference is not defined for is an error before
 * anything is launched: steps below 2, a window loop that does not visit arr_h x arr_w windows, arrays below 2 x 2, a
 * crop beyond the scaled frame.  Uses fs doubles of the workspace. */
int vf_patch_array_prepare(vf_ctx* ctx, const void* src, int src_layout, const unsigned char* mask, float* masked, float* full,
                           float* maskout, double* sum, int H, int W, int height, int width, int fs, int arr_h, int arr_w,
                           int crop_w, int crop_h, int flip, float mask_value);

/* ---- baseline JPEG decode (vf_jpeg.hip) -------------------------------------------------------------
 * image.load of data/donkey_folder.lua and datavid/donkey_folder.lua (libjpeg's default decompression) on the device,
 * byte for byte: islow IDCT, fancy upsampling, ycc_rgb_convert.  Supported: SOF0 / SOF1, 8-bit samples, Huffman
 * coding, ONE scan (interleaved for YCbCr), 1 component or 3 in YCbCr with luma sampling 1x1, 2x1 or 2x2 and chroma
 * 1x1 (4:4:4, 4:2:2, 4:2:0), sides up to 16384, with or without restart intervals.  Everything else is unsupported.
 * vf_jpeg_inspect (host only, no GPU): parse the markers of one file.  info (int64[12]) = {width, height, components,
 * luma h, luma v, restart interval (MCUs, 0: none), scan begin, scan end (byte range of the entropy-coded data),
 * supported (0 / 1), SOF marker (0xC0 ...), restart segments, sample precision}; when not supported, reason (may be
 * NULL) receives why.  scan_walk 0 reads the headers only (cheap; whether the file is supported is known from them):
 * scan end and restart segments are then -1.  scan_walk 1 also walks the entropy-coded data for them.  Returns
 * non-zero, with vf_last_error(), for a file that is malformed: truncated headers, no SOS, a Huffman table whose code
 * counts overflow their lengths, a component listed twice in the scan; with scan_walk, also restart markers out of
 * sequence or missing, and 0xFF fill bytes inside the entropy-coded data. */
enum { VF_JPEG_OK = 0, VF_JPEG_BAD_CODE = 1, VF_JPEG_SHORT_DATA = 2 };   /* per-image status words of vf_jpeg_decode */
int vf_jpeg_inspect(const unsigned char* data, size_t len, int scan_walk, int64_t* info, char* reason, int reason_cap);
/* Sizes for one batch: the n files are data[offs[i] .. offs[i+1]) (HOST memory).  ws_bytes: the DEVICE workspace
 * vf_jpeg_decode needs; stage_bytes: its HOST staging buffer (pinned memory keeps the one upload asynchronous).  Read
 * from the headers alone, so they are upper bounds (the scan data is walked once, by vf_jpeg_decode).
 * subseq_bytes (>= 8): length of the subsequences the Huffman decoder synchronises over.  Fails, naming the image,
 * on a file that is malformed (2) or unsupported (3). */
int vf_jpeg_workspace_bytes(const unsigned char* data, const int64_t* offs, int n, int subseq_bytes, size_t* ws_bytes,
                            size_t* stage_bytes);
/* Decode the batch on the context's stream: image i becomes uint8 H x W x channels at out + out_offs[i] (DEVICE out,
 * HOST out_offs).  channels 3: RGB (a grayscale file is replicated, as image.load(path, 3)); 1: grayscale files only.
 * status (DEVICE int32[n]) receives VF_JPEG_* per image, rounds (DEVICE int32[1]) the largest number of
 * synchronisation rounds any segment needed.  The host parses and packs every file into stage (caller-owned, >=
 * stage_bytes) and enqueues one upload into ws (caller-owned DEVICE memory, >= ws_bytes); stage must stay untouched
 * until the stream reaches this call's work.  Nothing is allocated and nothing synchronises. */
int vf_jpeg_decode(vf_ctx* ctx, const unsigned char* data, const int64_t* offs, int n, int channels, int subseq_bytes,
                   const int64_t* out_offs, unsigned char* out, void* stage, size_t stage_bytes, void* ws, size_t ws_bytes,
                   int32_t* status, int32_t* rounds);

/* ---- progressive JPEG decode (vf_jpeg.hip) -----------------------------------------------------------
 * SOF2 files through the same dequantisation, IDCT, upsampling and colour conversion: for a progression that is
 * complete, libjpeg's output is its output for the baseline file of the same coefficients, so the result is byte for
 * byte libjpeg's.  The entropy decoding is jdphuff.c's.  Supported: SOF2, Huffman coding, 8-bit samples, components,
 * colour spaces, samplings, sides and quantisation tables as for the baseline decoder, restart intervals or none (DRI
 * may change between scans), up to 64 scans whose progression is ORDERLY (the first scan of every coefficient of every
 * component has Ah = 0, every later one has Ah = the Al before it, a component's DC comes before its AC) and COMPLETE
 * (every coefficient has reached Al = 0 by the end).  A file that is not orderly or not complete is unsupported, not
 * malformed (libjpeg warns and block-smooths; there is no one result to pin).  Malformed (an error naming the scan):
 * an SOS that breaks libjpeg's JERR_BAD_PROGRESSION conditions (Ss <= Se <= 63; Ss = 0 means Se = 0; Ss > 0 means one
 * component; Al <= 13; Ah = 0 or Al = Ah - 1), or that names a Huffman slot no DHT has defined (a DC refinement scan
 * needs none), and everything vf_jpeg_inspect calls malformed.  vf_jpeg_inspect itself is unchanged: to it a
 * progressive file stays unsupported.
 * vf_jpeg_scans_inspect (host only, no GPU): walk the whole file.  info (int64[12]) = {width, height, components, luma
 * h, luma v, scans, supported (0 / 1), SOF marker, sample precision, scan levels, coefficient blocks, blocks per MCU}.
 * scans (may be NULL; int64[scan_cap][16]) receives per scan {components, their places in the frame (4 entries, -1
 * beyond), Ss, Se, Ah, Al, restart interval, begin, end (byte range of its entropy-coded data), restart segments,
 * level, units (MCUs of an interleaved scan, real blocks of a single-component one), 0}.  A scan's level is one more
 * than the highest level among the earlier scans that touch the same component and an overlapping band; scans of one
 * level are independent.  A file whose headers already rule it out (CMYK, 12-bit, ...; reason as vf_jpeg_inspect) or
 * that is not SOF2 ("not progressive") reports no scans; a progression found out of order stops the walk there. */
int vf_jpeg_scans_inspect(const unsigned char* data, size_t len, int64_t* info, int64_t* scans, int scan_cap, char* reason,
                          int reason_cap);
/* Exact sizes for one batch of supported progressive files, as vf_jpeg_workspace_bytes (the files are walked);
 * subseq_bytes as there, for the first scans. */
int vf_jpeg_prog_workspace_bytes(const unsigned char* data, const int64_t* offs, int n, int subseq_bytes, size_t* ws_bytes,
                                 size_t* stage_bytes);
/* Decode the batch on the context's stream; arguments and rules as vf_jpeg_decode, so a caller can decode baseline
 * and progressive files into one output buffer with one call each.  One upload, the unstuffing launch, one launch per
 * scan level of the batch (3 for libjpeg's default scripts; never a function of n), then the baseline IDCT and colour
 * launches.  Level 0 holds every first scan (Ah = 0), one block per (image, scan, restart segment), decoded by
 * self-synchronisation over subsequences of subseq_bytes as the baseline scan is; the later levels hold the refinement
 * scans, one lane per (image, scan, restart segment) walking it in order.  rounds (DEVICE int32[1]): the largest number
 * of synchronisation rounds any first-scan segment needed; levels (HOST, may be NULL): the number of level launches. */
int vf_jpeg_prog_decode(vf_ctx* ctx, const unsigned char* data, const int64_t* offs, int n, int channels, int subseq_bytes,
                        const int64_t* out_offs, unsigned char* out, void* stage, size_t stage_bytes, void* ws, size_t ws_bytes,
                        int32_t* status, int32_t* rounds, int32_t* levels);
/* Host only, no GPU: the assembled quantised coefficients of ONE supported progressive file, from the same decode
 * functions and the same packed batch the device runs.  subseq_bytes 0: every scan is walked in order, segment by
 * segment (what the refinement lanes do); >= 8: the first scans go through the self-synchronising scheme instead, its
 * lanes run one after the other (what the first-scan blocks do).  coef (HOST int16[coef_blocks][64], coef_blocks >=
 * info[10] of vf_jpeg_scans_inspect): block m * bpm + b is block b of MCU m (MCUs in raster order; within one, the
 * components in frame order, each component's blocks in raster order, dummy blocks included), its 64 values in natural
 * (row-major) order.  status receives the worst VF_JPEG_* of any segment; corrupt data ends in a status and never reads
 * or writes outside the buffers. */
int vf_jpeg_prog_coefficients_host(const unsigned char* data, size_t len, int subseq_bytes, int16_t* coef, size_t coef_blocks,
                                   int32_t* status);

/* ---- other samplings, RGB and several scans (vf_jpeg.hip; DESIGN.md 5.2, "layouts") ----------------------------------
 * Every 8-bit Huffman-coded SOF0 / SOF1 / SOF2 file of 1 or 3 components that libjpeg decodes without comment, byte for
 * byte its output.  Sampling: factors 1..4 per component whose ratios to the frame's largest are whole numbers, at most
 * 10 blocks in the MCU of all components (a one-component file ignores its factors); every component is upsampled by
 * jdsample.c's choice for it (copy, h2v1 / h2v2 fancy above 2 samples of width, h1v2 fancy, else replication).  Colour:
 * jdapimin.c's default_decompress_parms (JFIF or Adobe transform 1: YCbCr; Adobe transform 0, or no marker and ids
 * 'R','G','B': RGB, copied; anything else YCbCr).  A sequential file may have any number of scans with Ss = 0, Se = 63,
 * Ah = Al = 0, each of 1..3 components with the DHT / DRI state at its SOS (table slots 0..3 for SOF1), every component
 * in exactly one scan: a component in two scans is malformed, one in no scan unsupported.  Progressive files follow
 * vf_jpeg_scans_inspect's rules.  Unsupported, with vf_jpeg_inspect's reasons: 4 components, arithmetic coding, 12-bit
 * samples, lossless and hierarchical files, sides above 16384.  The four entries above behave as before.
 * vf_jpeg_inspect_layouts (host only, no GPU): walk the whole file.  info (int64[20]) = {width, height, components, h
 * and v of component 0, of 1, of 2, colour (0 grey, 1 YCbCr, 2 RGB), scans, supported (0 / 1), SOF marker, sample
 * precision, scan levels, coefficient blocks, blocks per MCU, 0, 0, 0}; reason as vf_jpeg_inspect. */
int vf_jpeg_inspect_layouts(const unsigned char* data, size_t len, int64_t* info, char* reason, int reason_cap);
/* Exact sizes for one batch, as vf_jpeg_prog_workspace_bytes; fails, naming the image, on a file the inspector refuses. */
int vf_jpeg_layouts_workspace_bytes(const unsigned char* data, const int64_t* offs, int n, int subseq_bytes, size_t* ws_bytes,
                                    size_t* stage_bytes);
/* Decode the batch, sequential and progressive files mixed, on the context's stream; arguments, rules and launches as
 * vf_jpeg_prog_decode.  Every scan of every sequential file is a first scan: its restart segments join level 0's one
 * launch, a block each, and its DC differences are summed per (image, scan, restart segment, component).  Nothing is
 * allocated, nothing synchronises, and the launch count is never a function of n. */
int vf_jpeg_decode_layouts(vf_ctx* ctx, const unsigned char* data, const int64_t* offs, int n, int channels, int subseq_bytes,
                           const int64_t* out_offs, unsigned char* out, void* stage, size_t stage_bytes, void* ws, size_t ws_bytes,
                           int32_t* status, int32_t* rounds, int32_t* levels);
/* Host only, no GPU: as vf_jpeg_prog_coefficients_host for ONE file vf_jpeg_inspect_layouts supports, of either kind
 * (coef_blocks >= its info[15]); blocks no scan codes (the dummy blocks of single-component scans) are zero. */
int vf_jpeg_layouts_coefficients_host(const unsigned char* data, size_t len, int subseq_bytes, int16_t* coef, size_t coef_blocks,
                                      int32_t* status);

/* ---- PNG decode (vf_png_decode.hip) ------------------------------------------------------------------
 * image.load of a PNG file (the masks of datavid/donkey_folder.lua, test_vid_wholeim.lua:112 and
 * test_more_complex.lua:102, demo.lua:51, and the frames vf_png_encode writes) on the device: the BYTES libpng gives
 * with grey below 8 bits and palettes expanded.  Supported: colour types 0, 2, 3, 4, 6 at bit depths 1, 2, 4, 8, no
 * interlace, sides up to 16384, any number of IDAT chunks, ancillary chunks, tRNS with a palette.  Unsupported (known
 * from the headers): 16-bit samples, Adam7 (the *_full entries below take both), IDAT data above 256 MiB.
 * vf_png_inspect (host only, no GPU): walk the chunks of one file.  info (int64[12]) = {width, height, bit depth,
 * colour type, interlace, channels after expansion (1 - 4: what image.load(path) gives), IDAT bytes in total, IDAT
 * chunks, palette entries, tRNS entries, supported (0 / 1), inflated bytes expected H * (1 + ceil(W * bits / 8))};
 * when not supported, reason (may be NULL) receives why.  Returns non-zero, with vf_last_error(), for a file that is
 * malformed: a bad signature, IHDR not first or with illegal fields, no PLTE for colour type 3 or PLTE after IDAT,
 * IDAT chunks not consecutive, no IEND, a chunk running past the file, a wrong CRC on IHDR, PLTE, tRNS, IDAT or IEND
 * (other ancillary chunks are skipped unchecked), a zlib header that is not deflate with a window of at most 32 KiB,
 * no preset dictionary and a valid FCHECK. */
enum {
  VF_PNG_OK = 0, VF_PNG_BAD_CODE = 1, VF_PNG_SHORT_DATA = 2, VF_PNG_BAD_DISTANCE = 3, VF_PNG_BAD_LENGTH = 4,
  VF_PNG_BAD_FILTER = 5, VF_PNG_BAD_ADLER = 6, VF_PNG_BAD_INDEX = 7
};   /* per-image status words of vf_png_decode */
int vf_png_inspect(const unsigned char* data, size_t len, int64_t* info, char* reason, int reason_cap);
/* Sizes for one batch: the n files are data[offs[i] .. offs[i+1]) (HOST memory).  ws_bytes: the DEVICE workspace
 * vf_png_decode needs; stage_bytes: its HOST staging buffer (pinned memory keeps the one upload asynchronous).  Read
 * from the chunk headers alone (no CRC is computed).  channels: 0 (the file's own, after expansion), 1 or 3.  Fails,
 * naming the image, on a file that is malformed (2) or unsupported (3); unsupported here also: channels 1 on a colour
 * file, channels 0 on a grey or RGB file with tRNS. */
int vf_png_decode_workspace_bytes(const unsigned char* data, const int64_t* offs, int n, int channels, size_t* ws_bytes,
                                  size_t* stage_bytes);
/* Decode the batch on the context's stream: image i becomes uint8 H x W x C at out + out_offs[i] (DEVICE out, HOST
 * out_offs), C = channels, or the file's own for channels 0.  channels 3 replicates grey, takes the grey of
 * grey+alpha, drops the alpha of RGBA and gives RGB from a palette; channels 1 takes grey and grey+alpha files;
 * a palette with tRNS gives RGBA for channels 0 (alpha 255 past the end of tRNS).  status (DEVICE int32[n]) receives
 * VF_PNG_* per image.  The host checks the CRCs, concatenates each file's IDAT payloads (minus the two zlib header
 * bytes) and packs them with PLTE / tRNS and a descriptor per image into stage (caller-owned, >= stage_bytes), and
 * enqueues one upload into ws (caller-owned DEVICE memory, >= ws_bytes) and three launches; stage must stay untouched
 * until the stream reaches this call's work.  Nothing is allocated and nothing synchronises.  This is the pipeline of
 * vf_png_decode_full below under the default rule with out_kind 0: the same descriptor and kernels, a file being the
 * one-pass case; the profiling labels are pngd_inflate, pngd_unfilter, pngd_expand. */
int vf_png_decode(vf_ctx* ctx, const unsigned char* data, const int64_t* offs, int n, int channels, const int64_t* out_offs,
                  unsigned char* out, void* stage, size_t stage_bytes, void* ws, size_t ws_bytes, int32_t* status);
/* image.load(path, nc, 'float') on top of the decoded bytes: dst[i] = src[i] / 255 in float32, an IEEE division
 * (correctly rounded), n elements, DEVICE src and dst, on the context's stream. */
int vf_png_bytes_to_float(vf_ctx* ctx, const unsigned char* src, float* dst, int64_t n);
/* The full rule ("Interlaced and 16-bit files"): the three entries above keep their behaviour; these
 * also take Adam7-interlaced files and 16-bit samples (colour types 0, 2, 4, 6; big-endian; a filter unit of up to 8
 * bytes).  Adam7: the inflated stream holds up to seven sub-images, pass p = 1..7 taking the pixels (x0 + i dx,
 * y0 + j dy) with (x0, y0, dx, dy) = (0,0,8,8) (4,0,8,8) (0,4,4,8) (2,0,4,4) (0,2,2,4) (1,0,2,2) (0,1,1,2), of
 * w_p = ceil((W - x0) / dx) by h_p = ceil((H - y0) / dy) pixels; a pass with w_p or h_p zero is absent; each present
 * pass has its own row length rb_p = ceil(w_p * samples * depth / 8), filter byte per row and zeros above its first
 * row; the stream inflates to sum h_p * (1 + rb_p) bytes, else VF_PNG_BAD_LENGTH.  Decided: the uint8 result of a
 * 16-bit sample is its HIGH byte (libpng's png_set_strip_16, Pillow's result).  Recalled, not checked against Torch:
 * 'float' of a 16-bit file is sample / 65535 on the whole sample.  Still unsupported: a side above 16384, IDAT data
 * above 256 MiB, an expected inflated size of 2^31 bytes or more (the decoder's sizes are int32), and by channels what
 * vf_png_decode_workspace_bytes refuses.
 * vf_png_inspect_full (host only, no GPU): vf_png_inspect's chunk walk and malformed-file errors; info[10], info[11]
 * and reason follow the full rule; passes (int64[21], may be NULL) receives (w_p, h_p, rb_p) of the seven passes, zeros
 * for an absent one; a file without interlace is one pass, the first. */
int vf_png_inspect_full(const unsigned char* data, size_t len, int64_t* info, int64_t* passes, char* reason, int reason_cap);
/* vf_png_decode_workspace_bytes and vf_png_decode under the full rule, with one more parameter.  out_kind 0: image i
 * becomes uint8 H x W x C; 1: float32 H x W x C written by the expansion kernel, byte / 255 for files of up to 8 bits
 * (the bits of vf_png_bytes_to_float) and sample / 65535 for 16-bit files, both IEEE divisions.  out_offs counts
 * ELEMENTS of out (bytes or floats).  Files vf_png_decode takes may be in the batch and give its bytes, and a batch of
 * such files with out_kind 0 needs exactly the sizes vf_png_decode_workspace_bytes returns.  The same contract
 * otherwise: host files, one upload, three launches (inflate; unfilter, one wave per image and pass; expand; the
 * profiling labels are pngd_inflate, pngd_unfilter_full, pngd_expand_full), nothing allocated, nothing synchronised,
 * VF_PNG_* per image in status. */
int vf_png_decode_full_workspace_bytes(const unsigned char* data, const int64_t* offs, int n, int channels, int out_kind,
                                       size_t* ws_bytes, size_t* stage_bytes);
int vf_png_decode_full(vf_ctx* ctx, const unsigned char* data, const int64_t* offs, int n, int channels, int out_kind,
                       const int64_t* out_offs, void* out, void* stage, size_t stage_bytes, void* ws, size_t ws_bytes,
                       int32_t* status);

/* ---- PNG encode (vf_png.hip) ---------------------------------------------------------------------------
 * image.save of test_vid.lua:138, test_vid_wholeim.lua:229-242 and test_more_complex.lua:200-214 on the device: a batch
 * of n frames of one H x W x C in, n whole PNG files out, back to back.  8-bit samples, C = 3 (colour type 2) or 1
 * (colour type 0), no interlace, sides 1 to 16384, n up to 65535; anything else is an error naming the geometry,
 * before anything is launched.  kind 0: float n x C x H x W, every value through image.savePNG's rule
 * b = (uint8) trunc(255f * min(max(x, 0), 1)) in float32 (NaN: 0); kind 1: uint8 n x H x W x C, taken as they are.
 * Rows carry the adaptive filter libpng chooses by default (smallest sum of absolute filtered values, None, Sub, Up,
 * Average, Paeth in that order on ties); the filtered stream is deflated in independent 8 KiB chunks, one IDAT each,
 * dynamic Huffman codes over LZ77 tokens or a stored block when that is not smaller.  A file's bytes depend on its own
 * frame only, and are the same on every run.
 * vf_png_workspace_bytes (host only, no GPU): the DEVICE workspace and an upper bound on the output for the batch. */
int vf_png_workspace_bytes(int n, int H, int W, int C, size_t* ws_bytes, size_t* out_bytes);
/* Encode on the context's stream.  ws (>= ws_bytes) and out (out_cap >= the bound above) are caller-owned DEVICE memory;
 * offsets (DEVICE int64[n + 1]) receives the files' places: file i is out[offsets[i] .. offsets[i + 1]).  Nothing is
 * allocated and nothing synchronises. */
int vf_png_encode(vf_ctx* ctx, const void* src, int kind, int n, int H, int W, int C, void* ws, size_t ws_bytes,
                  unsigned char* out, size_t out_cap, int64_t* offsets);
/* vf_png_encode with a compression level.  0: vf_png_encode, byte for byte.  1 ("dense"): the same filter, chunks, IDATs,
 * Huffman construction and workspace, with a denser matcher in the deflate stage (k_png_deflate_dense; tests/png_dense_ref.py
 * is its rule): hash chains over the chunk and the 8 KiB of the same frame's stream before it, distance 1 and 64 chain
 * entries per position, the same literal pricing, one lazy step, so a back-reference may reach into the preceding chunk
 * (never into another frame).  About half the bytes of level 0 on smooth frames, several times its deflate time.  Any other
 * level is an error naming `level`, before anything is launched.  vf_png_workspace_bytes holds for both levels. */
int vf_png_encode_level(vf_ctx* ctx, const void* src, int kind, int n, int H, int W, int C, int level, void* ws, size_t ws_bytes,
                        unsigned char* out, size_t out_cap, int64_t* offsets);

/* ---- JPEG encode (vf_jpeg_enc.hip) ---------------------------------------------------------------------
 * image.save('x.jpg') / image.compressJPG, the JPEG folders the loaders read and the payload of the training scripts'
 * disp.image, on the device: a batch of n frames of one H x W x C in, n whole baseline JFIF files out, back to back,
 * byte for byte what libjpeg's default compression writes (jpeg_set_defaults, jpeg_set_quality(quality, TRUE), the fixed
 * Annex K Huffman tables, no restart intervals (vf_jpeg_encode_opts has both options), the islow DCT; Pillow's save(format="JPEG", quality, subsampling) is the
 * same).  8-bit samples, C = 3 (RGB in, YCbCr coded) or 1 (grey), sides 1 to 16384, n 1 to 65535, quality 1 to 100;
 * subsampling 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0 (luma 1x1, 2x1 or 2x2 against chroma 1x1; ignored for C = 1); anything else
 * is an error naming the argument, before anything is launched.  kind 0: float n x C x H x W, every value through
 * image.savePNG's rule (see vf_png_encode; Torch7's saveJPG clamps and truncates the same way); kind 1: uint8
 * n x H x W x C, taken as they are.  A file's bytes depend on its own frame, the quality and the sampling only, and are
 * the same on every run.
 * vf_jpeg_encode_workspace_bytes (host only, no GPU): the DEVICE workspace and an upper bound on the output for the
 * batch.  The bound: a block's code is at most 64 coefficients of 16 code bits + 11 value bits, 216 bytes; byte stuffing
 * can at most double the stream; the header is at most 624 bytes and EOI 2:
 * out_bytes = n * (2 * 216 * blocks per frame + 626), blocks counted in whole MCUs, dummies included. */
int vf_jpeg_encode_workspace_bytes(int n, int H, int W, int C, int subsampling, size_t* ws_bytes, size_t* out_bytes);
/* Encode on the context's stream.  ws (>= ws_bytes) and out (out_cap >= the bound above) are caller-owned DEVICE memory;
 * offsets (DEVICE int64[n + 1]) receives the files' places: file i is out[offsets[i] .. offsets[i + 1]).  Nine launches
 * whatever n is; nothing is allocated and nothing synchronises. */
int vf_jpeg_encode(vf_ctx* ctx, const void* src, int kind, int n, int H, int W, int C, int quality, int subsampling,
                   void* ws, size_t ws_bytes, unsigned char* out, size_t out_cap, int64_t* offsets);
/* The same with libjpeg's two save() options, byte for byte what libjpeg writes with them (Pillow's restart_marker_rows,
 * restart_marker_blocks and optimize; tests/jpeg_enc_opts_ref.py is the rule in numpy).
 * Restart intervals: restart_rows > 0 asks for an interval of that many rows of MCUs, clamped to 65535 MCUs; otherwise
 * restart_blocks is the interval in MCUs; 0 and 0: none.  A DRI segment stands between the last DHT and SOS; in front of
 * every interval but the first the stream is padded to a byte with 1-bits, RST0..RST7 in turn follows, and the DC
 * predictors start again at 0.  restart_rows and restart_blocks are 0 to 65535 each.
 * optimize = 1: every file carries Huffman tables made from its own symbol counts (jpeg_gen_optimal_table: codes of at most
 * 16 bits, no all-ones code), in the four DHT segments of the default file (two for grey), each 21 bytes + its symbols;
 * a file's header is then its own and no longer than the default one.  optimize is 0 or 1.
 * Anything else is an error naming the argument, before anything is launched.  With all three 0 the bounds and the files
 * are those of vf_jpeg_encode.  The bound: an interval adds DRI's 6 bytes and, per segment, a pad byte, its stuffing byte
 * and two marker bytes: out_bytes = n * (2 * 216 * blocks per frame + 626 [+ 4 * segments + 6]); optimised codes are at
 * most 16 bits too.  The workspace grows by 16 bytes per segment, and with optimize by the counters, the code table and
 * the DHT segments of every image. */
int vf_jpeg_encode_opts_workspace_bytes(int n, int H, int W, int C, int subsampling, int restart_rows, int restart_blocks,
                                        int optimize, size_t* ws_bytes, size_t* out_bytes);
/* As vf_jpeg_encode: ten launches with an interval alone, twelve and one memset with optimize, whatever n is; the counts,
 * the tables and the headers are made on the device; nothing is allocated and nothing synchronises. */
int vf_jpeg_encode_opts(vf_ctx* ctx, const void* src, int kind, int n, int H, int W, int C, int quality, int subsampling,
                        int restart_rows, int restart_blocks, int optimize, void* ws, size_t ws_bytes, unsigned char* out,
                        size_t out_cap, int64_t* offsets);
/* The same frames as progressive files (SOF2), byte for byte what libjpeg writes with jpeg_simple_progression (Pillow's
 * progressive=True; tests/jpeg_enc_prog_ref.py is the rule in numpy): 10 scans for C = 3 (DC of all components, Y 1-5,
 * Cr, Cb, Y 6-63, Y refined, DC refined, Cr, Cb and Y refined), 6 for C = 1, every scan but the DC refinement behind the
 * DHT segments of its own optimal tables (libjpeg forces optimize_coding here).  The arguments, limits and errors are those
 * of vf_jpeg_encode; restart intervals cannot be asked for.
 * The bound.  Over all scans a luma block's code is at most: DC 16 code bits + 11 value bits, its refinement 1 bit; an AC
 * coefficient's first scan 16 + 10 bits (63 coefficients), a refinement scan 16 + 1 sign bit or 1 correction bit per
 * coefficient (twice 63), a ZRL less than that per coefficient it covers; and in each of the four AC scans one EOBn of
 * 16 + 14 bits: 28 + 63 * 26 + 2 * 63 * 17 + 4 * 30 = 3928 bits, rounded up to 3968, 496 bytes (a chroma block has one
 * refinement scan less; a dummy has only the DC bits).  Every scan ends in at most one pad byte; byte stuffing can at
 * most double the stream; SOI to SOF2 is at most 192 bytes, a scan's header at most two DHT segments of 288 bytes and an
 * SOS of 14; EOI 2:
 * out_bytes = n * (2 * (496 * blocks per frame + scans) + 192 + scans * 590 + 2), blocks counted in whole MCUs. */
int vf_jpeg_encode_prog_workspace_bytes(int n, int H, int W, int C, int subsampling, size_t* ws_bytes, size_t* out_bytes);
/* As vf_jpeg_encode: twelve launches and two memsets whatever n and the scan count are (the kernels take the scan as a
 * grid dimension); the runs, the counts, the tables and the headers are made on the device; nothing is allocated and
 * nothing synchronises. */
int vf_jpeg_encode_prog(vf_ctx* ctx, const void* src, int kind, int n, int H, int W, int C, int quality, int subsampling,
                        void* ws, size_t ws_bytes, unsigned char* out, size_t out_cap, int64_t* offsets);

/* ---- animated GIF encode (vf_gif.hip) ------------------------------------------------------------------
 * The `convert -delay D pred_1.png ... x_result.gif` that ends test_vid.lua:140-147, test_vid_wholeim.lua:244-257 and
 * test_more_complex.lua:216-229, on the device: `clips` clips of `frames` RGB frames of one H x W in, `clips` whole
 * GIF89a files out, back to back.  Sides 1 to 16384, 1 to 65535 frames per clip, 1 to 65535 clips, delay 0 to 65535
 * centiseconds; anything else is an error naming the argument, before anything is launched.  kind 0: float
 * (clips*frames) x 3 x H x W, every value through image.savePNG's rule (see vf_png_encode); kind 1: uint8
 * (clips*frames) x H x W x 3, taken as they are.  The rule is the project's own and all-integer (tests/gif_ref.py is its
 * definition; ImageMagick's adaptive tree and dithering are not restated): a local table of 256 per frame, the frame's
 * colours in ascending order when there are at most 256 (lossless), else median cut on the 5-bit histogram with box
 * means; nearest entry per pixel, lowest index on a tie, no dithering; LZW with a Clear every 3824 pixels; loop count 0,
 * disposal 0, no transparency, no frame differencing.  A file's bytes depend on its own frames and the delay only, a
 * frame's bytes (graphic control extension to block terminator) on that frame and the delay only; the same on every run.
 * vf_gif_workspace_bytes (host only, no GPU): the DEVICE workspace and an upper bound on the output for the batch. */
int vf_gif_workspace_bytes(int clips, int frames, int H, int W, size_t* ws_bytes, size_t* out_bytes);
/* Encode on the context's stream.  ws (>= ws_bytes) and out (out_cap >= the bound above) are caller-owned DEVICE memory;
 * offsets (DEVICE int64[clips + 1]) receives the files' places: file i is out[offsets[i] .. offsets[i + 1]).  Nothing is
 * allocated and nothing synchronises. */
int vf_gif_encode(vf_ctx* ctx, const void* src, int kind, int clips, int frames, int H, int W, int delay_cs, void* ws,
                  size_t ws_bytes, unsigned char* out, size_t out_cap, int64_t* offsets);

/* ---- animated PNG encode (vf_png.hip) -----------------------------------------------------------------
 * A clip as ONE lossless file every browser plays: g clips of n frames of one H x W x C in, g whole APNG files out, back to
 * back.  tests/apng_ref.py is the definition: the file is assembled from the n PNG files vf_png_encode writes for the
 * clip's frames — signature, frame 0's IHDR, acTL (num_frames n, num_plays loop; 0 plays forever); per frame an fcTL
 * (the whole canvas at (0,0), delay / 100 s, dispose NONE, blend SOURCE) and the frame's own zlib stream, frame 0's as
 * its IDAT chunks unchanged, every later frame's as one fdAT (sequence number + the IDAT's payload) per IDAT; IEND.
 * Sequence numbers run 0, 1, 2, ... over fcTL and fdAT together.  No frame differencing, no sub-rectangles.  A file's
 * bytes depend on its own frames, delay and loop only, and are the same on every run; the file is also a valid PNG of
 * frame 0.  C, sides and kind as vf_png_encode; n and g 1 to 65535 each, n * (chunks of a frame + 1) below 2^31 (a chunk
 * is 8192 filtered bytes), delay (centiseconds) and loop 0 to 65535; anything else is an error naming the argument,
 * before anything is launched.  kind 0: float (g*n) x C x H x W; kind 1: uint8 (g*n) x H x W x C.
 * vf_apng_workspace_bytes (host only, no GPU): the DEVICE workspace and an upper bound on the output for the batch,
 * g * (n * (H * (W * C + 1) + 21 * chunks + 6 + 38) + 65). */
int vf_apng_workspace_bytes(int g, int n, int H, int W, int C, int delay, int loop, size_t* ws_bytes, size_t* out_bytes);
/* Encode on the context's stream.  ws (>= ws_bytes) and out (out_cap >= the bound above) are caller-owned DEVICE memory;
 * offsets (DEVICE int64[g + 1]) receives the files' places: file i is out[offsets[i] .. offsets[i + 1]).  Nothing is
 * allocated and nothing synchronises. */
int vf_apng_encode(vf_ctx* ctx, const void* src, int kind, int g, int n, int H, int W, int C, int delay, int loop, void* ws,
                   size_t ws_bytes, unsigned char* out, size_t out_cap, int64_t* offsets);
/* vf_apng_encode with vf_png_encode_level's compression level: the file assembled from the PNG files of that level.  Level 0
 * is vf_apng_encode; any level but 0 and 1 is an error naming `level`.  vf_apng_workspace_bytes holds for both levels. */
int vf_apng_encode_level(vf_ctx* ctx, const void* src, int kind, int g, int n, int H, int W, int C, int delay, int loop, int level,
                         void* ws, size_t ws_bytes, unsigned char* out, size_t out_cap, int64_t* offsets);

/* ---- animated PNG decode (vf_png_decode.hip, vf_apng_parse.h) -----------------------------------------
 * APNG files (the ones vf_apng_encode writes among them) and plain PNG files to the composited canvas of every frame, on
 * the device and all-integer; tests/apng_decode_ref.py is the definition.  Frames: acTL.num_frames of them, one per fcTL;
 * frame k's pixels are the zlib stream of its data chunks (the IDATs when its fcTL precedes them, else its fdATs without
 * their sequence numbers) decoded under the full PNG rule (vf_png_decode_full) as an image of the fcTL's width x height
 * with the IHDR's depth, colour type and interlace and the file's PLTE / tRNS.  A default image without an fcTL in front
 * is not a frame; a PNG without acTL is a clip of one frame.  Canvas: the IHDR's size, transparent black; blend SOURCE
 * replaces the rectangle, alpha included; dispose 0 leaves the canvas, 1 clears the rectangle to transparent black, 2
 * restores what was there before the frame (on the first frame: clears).  Output frame k is the canvas after frame k was
 * rendered: grey replicated, alpha 255 where the file has none, a pixel nothing painted (0,0,0,0); a 16-bit sample gives
 * its high byte.  Not taken (supported = 0 with the reason): blend OVER in a file that carries alpha (colour type 4 or 6,
 * or tRNS; without alpha OVER is SOURCE), tRNS on colour types 0 and 2, a side above 16384, more than 65535 frames,
 * 2 GiB or more of RGBA frames, a frame the full rule refuses.  Malformed (an error): a wrong CRC on IHDR, PLTE, tRNS,
 * IDAT, IEND, acTL, fcTL or fdAT; a second acTL or one after IDAT; num_frames 0 or not the number of fcTL chunks; a
 * sequence number missing, repeated or out of order; an fdAT before the first fcTL, shorter than 4 bytes or in the frame
 * the IDATs hold; a frame without data or with a bad zlib header; a zero-size frame or one that leaves the canvas; an
 * fcTL in front of IDAT that is not the whole canvas at (0,0), or two of them; dispose above 2, blend above 1;
 * truncation; and what vf_png_inspect calls malformed.
 * vf_apng_inspect (host only, no GPU): walk one whole file.  info (int64[12]) = {width, height, bit depth, colour type,
 * interlace, channels of the decoded frames (1, 2, 3, 4), frames, num_plays or -1 without acTL, supported, animated (an
 * acTL), the IDAT image is frame 0, palette entries}.  frames (int64[frame_cap][9], may be NULL with frame_cap 0)
 * receives per frame {x, y, w, h, delay_num, delay_den, dispose, blend, data_bytes} for the first frame_cap frames.
 * reason: why not supported.  Returns non-zero for a malformed file. */
int vf_apng_inspect(const unsigned char* data, size_t len, int64_t* info, int64_t* frames, int frame_cap, char* reason,
                    int reason_cap);
/* The calling convention of vf_gif_decode: n files back to back (file i is data[offs[i] .. offs[i + 1])), alpha 0: RGB,
 * 1: RGBA.  ws_bytes: the DEVICE workspace; stage_bytes: the HOST staging buffer.  An error naming the image for a
 * malformed (2) or unsupported (3) file.  All frames of a batch are images of one launch: 65535 frames at most. */
int vf_apng_decode_workspace_bytes(const unsigned char* data, const int64_t* offs, int n, int alpha, size_t* ws_bytes,
                                   size_t* stage_bytes);
/* Decode on the context's stream: file i's frames x H x W x (3 or 4) canvases go to out[out_offs[i] ...]; status (DEVICE
 * int32[n]) receives VF_PNG_* per file: the first of its frames' that is not 0, and then nothing of the file is written.
 * ONE upload, then four launches whatever n and the frame counts (inflate, unfilter, expand as in vf_png_decode_full with
 * a frame per image, k_apng_compose: a thread per canvas pixel).  Nothing is allocated and nothing synchronises. */
int vf_apng_decode(vf_ctx* ctx, const unsigned char* data, const int64_t* offs, int n, int alpha, const int64_t* out_offs,
                   unsigned char* out, void* stage, size_t stage_bytes, void* ws, size_t ws_bytes, int32_t* status);

/* ---- animated GIF decode (vf_gif_decode.hip) --------------------------------------------------------
 * GIF87a and GIF89a files (the ones vf_gif_encode writes among them) to the composited canvas of every frame, on the
 * device and all-integer; tests/gif_decode_ref.py is the definition.  Container: logical screen, optional global table,
 * any sequence of extensions (the graphic control extension gives disposal, transparency and delay, NETSCAPE2.0 the
 * loop count, the others are skipped), image descriptors with an optional local table and interlace flag, the trailer;
 * bytes behind the trailer are ignored.  LZW: minimum code size 2 to 8, a leading Clear optional, KwKwK, and a full
 * dictionary of 4096 entries stays as it is until a Clear comes; decoding stops once the rectangle is full.
 * Compositing is the browsers' rule: the RGBA canvas starts transparent; frame k paints its non-transparent indices as
 * (table colour, 255) and the canvas is output frame k; then disposal 2 clears the rectangle to (0,0,0,0), 3 restores
 * the canvas as it was before the frame, anything else keeps it.  RGB output is the colour planes (a transparent pixel
 * is 0,0,0), RGBA adds alpha (0 or 255).
 * vf_gif_inspect (host only, no GPU): walk one whole file.  info (int64[8]) = {width, height, frames, loop count or -1
 * without a NETSCAPE2.0 block, supported (0/1), entries of the global table or 0, version (87 or 89), sum of the frame
 * rectangles' pixels}; frames (may be NULL; int64[frame_cap][12]) receives, for the first frame_cap frames, {delay in
 * centiseconds, disposal, x, y, w, h, interlace, transparent index or -1, entries of the active table, table is local,
 * LZW minimum code size, bytes of image data}; reason receives why a parsable file is not supported (a side above
 * 16384, more than 65535 frames, decoded frames of 2 GiB or more, frame rectangles above 256 Mi pixels, a frame's data
 * above 256 MiB), else "".  Non-zero, with vf_last_error, for a malformed file: bad signature, truncation, no trailer,
 * no frame, a rectangle that leaves the screen, a frame without any colour table, a minimum code size outside 2 .. 8. */
enum {
  VF_GIF_OK = 0, VF_GIF_BAD_CODE = 1, VF_GIF_SHORT_DATA = 2, VF_GIF_BAD_INDEX = 3
};   /* per-file status words of vf_gif_decode: a code above the next free one, or a first code behind a Clear that is
      * no root; EOI or the end of the data before the rectangle is full; an index that is painted and lies at or
      * above the active table's size.  A file's word is the largest of its frames'; indices are only looked at when
      * every frame's code stream was good. */
int vf_gif_inspect(const unsigned char* data, size_t len, int64_t* info, int64_t* frames, int frame_cap, char* reason,
                   int reason_cap);
/* Host only, no GPU: ws_bytes receives the DEVICE workspace (the upload, then every frame's index plane) that
 * vf_gif_decode needs; stage_bytes: its HOST staging buffer (pinned memory keeps the one upload asynchronous).  data
 * holds the n files back to back, file i at offs[i] .. offs[i+1]; alpha 0: RGB output, 1: RGBA.  Error 2 for a malformed
 * file, 3 for an unsupported one, naming the image. */
int vf_gif_decode_workspace_bytes(const unsigned char* data, const int64_t* offs, int n, int alpha, size_t* ws_bytes,
                                  size_t* stage_bytes);
/* Decode on the context's stream: file i becomes uint8 frames_i x H_i x W_i x (3 | 4) at out + out_offs[i]; status
 * (DEVICE int32[n]) receives VF_GIF_* per file.  The host walks each file, strips the sub-block length bytes so that
 * every frame's code stream is contiguous, and packs the streams, one colour table and one descriptor per frame into
 * stage -> ONE upload; then two launches whatever n and the frame counts (k_gifd_lzw: a block per frame; k_gifd_compose:
 * a thread per canvas pixel of a file).  out, ws and status are caller-owned DEVICE memory, stage HOST memory that
 * stays untouched until the stream has passed the upload.  Nothing is allocated and nothing synchronises. */
int vf_gif_decode(vf_ctx* ctx, const unsigned char* data, const int64_t* offs, int n, int alpha, const int64_t* out_offs,
                  unsigned char* out, void* stage, size_t stage_bytes, void* ws, size_t ws_bytes, int32_t* status);

/* ---- contact sheets of the inference scripts (vf_display.hip) -----------------------------------------
 * image.toDisplayTensor(input, padding, nrow, scaleeach, min, max, symmetric, saturate) of test.lua:129, demo.lua:96 and
 * test_vid.lua:149 for the one input form they use: a packed float tensor N x C x h x w, C = 1 or 3 (src_layout 0:
 * planar; 1: NHWC, N x h x w x C).  grid: float planar C x (h+padding)*ymaps x (w+padding)*xmaps, xmaps = min(nrow, N),
 * ymaps = ceil(N / xmaps); image k (row-major, 0-based) sits in cell (k / xmaps, k % xmaps) at offset padding/2; the
 * padding and the cells past N hold the pack's maximum; then image.minmax runs over the grid — or, with scaleeach, over
 * every image before the layout (the fill is then the maximum of the scaled pack).  minmax: with neither bound given
 * saturate is dropped; min absent: -max(|tmin|, |tmax|) if symmetric, else tmin; t += (float)(-min) unless min == 0;
 * the divisor is (float)(2 max(|tmin|, |tmax|)) (max absent, symmetric), the shifted tensor's maximum (max absent), or
 * (float)((double)max - (double)min); t /= divisor unless it is 0 (IEEE float32 division); clamp to [0,1] if saturate.
 * has_min / has_max say whether min / max are given (Lua's nil otherwise).  Bit-identical to tests/display_ref.py and the
 * same on every run; inputs must be finite.  Odd or negative padding, C outside {1, 3} and grids of 2^31 elements or more
 * than 65535 cells are errors naming the argument or the shape, before anything is launched.  Two launches; the first
 * (min / max partials into the context workspace) is skipped when the extremes are not needed: both bounds given, no
 * scaleeach, and no padding or empty cell to fill.
 * vf_display_workspace_bytes (host only, no GPU): the bytes of the context workspace the call uses. */
int vf_display_workspace_bytes(int N, int C, int h, int w, int padding, int nrow, int scaleeach, int has_min, int has_max,
                               size_t* ws_bytes);
int vf_display_tensor(vf_ctx* ctx, const float* packed, int src_layout, float* grid, int N, int C, int h, int w, int padding,
                      int nrow, int scaleeach, int has_min, double min, int has_max, double max, int symmetric, int saturate);
/* test.lua:98-128 (= demo.lua:73-95) in one pass.  ctx_nhwc: the generator input B x fs x fs x C in [-1,1], hole painted
 * (vf_center_prepare); pred_nhwc: the prediction B x fs/2 x fs/2 x C.  pretty (planar 2B x C x fs x fs, [0,1]): row 2i is
 * the input mapped by add(1):mul(0.5) with the hole [fs/4+ov, 3fs/4-ov)^2 set to exactly 1 (:122-124), row 2i+1 the context
 * with pred[ov : fs/2-ov]^2 copied over the same hole (:98) and then mapped.  pasted (planar B x C x fs x fs; or NULL)
 * receives row 2i+1 alone (image_ctx of :102), pred_mapped (planar B x C x fs/2 x fs/2; or NULL) the whole prediction
 * mapped (:103).  fs % 4 != 0 or fs/2 - 2*overlapPred <= 0 is an error before anything is launched. */
int vf_center_finish(vf_ctx* ctx, const float* ctx_nhwc, const float* pred_nhwc, float* pretty, float* pasted,
                     float* pred_mapped, int B, int C, int fs, int overlapPred);

/* ---- scores of result frames (vf_metrics.hip) ----------------------------------------------------------
 * PSNR, SSIM, absolute error and flicker of N result frames `a` against N truth frames `b`, on the BYTES image.save
 * would write.  kind 0: both float N x C x H x W, every value through image.savePNG's rule (see vf_png_encode); kind 1:
 * both uint8 N x H x W x C, taken as they are.  C = 1 or 3, sides 1 to 16384, N 1 to 65535.  Only rows < vh and columns
 * < vw count (1 <= vh <= H, 1 <= vw <= W); what lies outside is never read.  mask (DEVICE uint8 H x W, non-zero = hole)
 * may be NULL.  clip != 0: the batch is one clip and the flicker term runs over it; 0: independent images, flicker 0.
 * table (DEVICE int64[N][2][VF_METRICS_COLS]) receives, per frame and region (0: every valid pixel; 1: the valid pixels
 * under the mask, all zero without one), summed over the channels, in this column order:
 *   VF_METRICS_N       samples counted
 *   VF_METRICS_SSE     sum (a - b)^2
 *   VF_METRICS_SAE     sum |a - b|
 *   VF_METRICS_SSIM_Q  sum over the windows of llrint(s * 2^30), s the window's SSIM (uniform 7 x 7, sample covariance,
 *                      K1 0.01, K2 0.03, L 255, per channel; from the integer window sums by two IEEE double divisions
 *                      and one multiplication); windows wholly inside the valid rectangle, a window
 *                      belonging to region 1 when its centre pixel does
 *   VF_METRICS_SSIM_N  windows counted
 *   VF_METRICS_FLICKER sum |(a_t - a_{t-1}) - (b_t - b_{t-1})| for frames t >= 1 of a clip, else 0
 * Every column is an integer sum: the table equals tests/metrics_ref.py exactly and is the same on every run.  One
 * memset and one launch on the context's stream, whatever N; nothing is allocated and nothing synchronises.  Bad
 * arguments are errors naming them, before anything is launched. */
enum {
  VF_METRICS_N = 0, VF_METRICS_SSE = 1, VF_METRICS_SAE = 2, VF_METRICS_SSIM_Q = 3, VF_METRICS_SSIM_N = 4,
  VF_METRICS_FLICKER = 5, VF_METRICS_COLS = 6
};
int vf_frame_metrics(vf_ctx* ctx, const void* a, const void* b, int kind, int N, int C, int H, int W, int vh, int vw,
                     const unsigned char* mask, int clip, int64_t* table);

/* ---- option branches of train.lua: noiseGen (:109-124, 319-327) and conditionAdv (:158-180) -----------------------
 * nn.JoinTable(2) over NHWC tensors: dst[p][c_dst + c] = src[p][c_src + c] for c < Ccopy, p < npix (forward: one call
 * per table element into the joined tensor; updateGradInput: one call per element out of the joined gradient).
 * The branches' convolutions (5x5 stride 2 pad 2 / 2+32; 1x1) are served by vf_conv2d_* above: any kernel size,
 * stride and padding is accepted there, the 4x4 shapes of the main nets take the matrix-core path. */
int vf_channel_copy(vf_ctx* ctx, const float* src, int Csrc, int c_src, float* dst, int Cdst, int c_dst, int Ccopy,
                    int64_t npix);
/* noise:uniform(-1,1) (normal = 0) / noise:normal(0,1) (normal = 1), train.lua:319-323.  Counter-based: element i is a
 * function of (seed, counter, i) only (splitmix64; Torch7's generator stream is not reproducible).  counter_dev, if
 * not NULL, is a DEVICE int32 read at run time (e.g. Adam's step count, so a replayed HIP graph draws fresh noise
 * every iteration); otherwise `counter` is used. */
int vf_noise_fill(vf_ctx* ctx, float* out, int64_t n, uint64_t seed, const int32_t* counter_dev, uint64_t counter,
                  int normal);

/* ---- every weight gradient of one backward walk in one launch -----------------------------------------------------
 * Between vf_wgrad_group_begin and vf_wgrad_group_end, vf_conv2d_bwd_weight / vf_deconv2d_bwd_weight calls on this
 * context are RECORDED (the 16-byte-vectorised ones; others still launch at once) and the group — one grouped GEMM
 * launch per tile family plus one grouped split-K reduce — runs at _end.  Valid because accGradParameters of a layer
 * reads only that layer's input and gradOutput, which the nn protocol keeps in the modules' buffers until the walk is
 * over; the caller must not overwrite them, nor read gradWeight, before _end.  The workspace must hold the split-K
 * slabs of all recorded layers at once (vf_workspace_bytes_hint); if it does not, the group is flushed early. */
int vf_wgrad_group_begin(vf_ctx* ctx);
int vf_wgrad_group_end(vf_ctx* ctx);
/* Drop an open group without launching anything (a host-side error cut the backward walk short): the recorded GEMMs are
 * discarded and the context is back to immediate launches.  No-op when no group is open. */
int vf_wgrad_group_abort(vf_ctx* ctx);
/* Data parallel: a walk whose weight gradients leave in two launches, both at its END (a group launched in the middle of the
 * data-gradient chain slowed the passes behind it by 20-40 %: DESIGN.md 8).  vf_wgrad_group_count: gradients recorded so far (the
 * host reads it when the walk passes the bucket boundary); vf_wgrad_group_end_partial(count): launch the first `count` recorded
 * ones — the finished bucket, whose exchange can start — and keep the group open; vf_wgrad_group_end launches the rest. */
int vf_wgrad_group_count(vf_ctx* ctx, int* count);
int vf_wgrad_group_end_partial(vf_ctx* ctx, int count);

/* ---- every conv bias gradient of one backward walk in two launches ----------------------------------------------
 * gradBias = sum over pixels of gradOutput (THNN accGradParameters) is not needed before optim.adam, and each layer's
 * gradOutput stays in its module's buffer until the walk ends, so the column sums of all layers run as ONE stage-1 and
 * ONE stage-2 launch.  desc_dev: DEVICE array of n 64-byte descriptors
 *   { const float* g; float* gb; double* part; int64 P; int32 C, cq, rows_per_block, gx, gy, blk1_off, blk2_off; float beta }
 * (g: [P][C] gradOutput, C % 4 == 0, 16-byte aligned; part: gx*C doubles of scratch; geometry from vf_bias_grad_plan;
 * blk1_off / blk2_off: running sums of gx*gy / ceil(C/4) over the layers).  gb = beta*gb + column sums. */
int vf_bias_grad_plan(int64_t P, int C, int* cq, int* rows_per_block, int* gx, int* gy);
int vf_bias_grad_multi(vf_ctx* ctx, const void* desc_dev, int n, int blocks1, int blocks2);

/* ---- data-parallel exchange over RCCL (one process per GPU) --------------------------------------------------------
 * The reference trains on one device (train.lua:42 `gpu = 1`); BASELINE's N > 1 configuration is data parallelism over
 * the same closures: the flat gradient vectors of train.lua:240-241 are averaged over ranks before each optim.adam,
 * optionally BatchNorm's sums are added over ranks (statistics of the global batch).  These entries are that exchange, so
 * a Lua / FFI host needs nothing besides this library.  RCCL is bound at run time (dlopen "librccl.so", or $VF_RCCL_LIB)
 * at the first call; the rest of the library does not depend on it.
 *
 * vf_comm_available: 0 if RCCL can be bound in this process (local, non-collective: check it on every rank and let the ranks
 *   agree BEFORE entering the collective vf_comm_init, so that a rank without RCCL does not leave the others waiting).
 * vf_comm_unique_id: rank 0 fills 128 opaque bytes; the host hands them to every rank (file, socket, MPI ...).
 * vf_comm_init: on any failure the half-built communicator is released (RCCL comm aborted, stream / events destroyed).
 * vf_comm_init: collective over all ranks, on the CURRENT device (hipSetDevice first).
 * vf_comm_allreduce_async: in place, on the communicator's own stream, ordered after the work already given to ctx's
 *   stream; ctx's stream carries on (backward kernels overlap the bucket's flight).  dtype 0 = f32, 1 = f64;
 *   op 0 = sum, 1 = average, 2 = max, 3 = min.  *ticket (0..63, reused round-robin) names it for vf_comm_wait, which makes
 *   ctx's stream wait on the DEVICE for that collective and all earlier ones (the host does not block).
 * vf_comm_allreduce_avg_async: the gradient bucket case (f32, average).
 * vf_comm_allreduce_inline: the collective on ctx's stream itself (SyncBN sums; capturable into a hipGraph with the
 *   kernels around it).  vf_comm_broadcast: root's buffer to all ranks, on ctx's stream (initial parameters).
 * vf_comm_barrier: host-blocking; both streams of every rank have drained. */
typedef struct vf_comm vf_comm;
#define VF_COMM_ID_BYTES 128
int vf_comm_available(void);
int vf_comm_unique_id(void* id128);
int vf_comm_init(vf_comm** out, const void* id128, int world, int rank);
int vf_comm_world(const vf_comm* c);
int vf_comm_rank(const vf_comm* c);
int vf_comm_allreduce_async(vf_comm* c, vf_ctx* ctx, void* buf, int64_t count, int dtype, int op, int* ticket);
int vf_comm_allreduce_avg_async(vf_comm* c, vf_ctx* ctx, float* buf, int64_t n, int* ticket);
/* the two halves of an all-reduce (buf: world * shard_count floats; rank r's shard at buf + r * shard_count), for an optimiser
 * sharded over the ranks: reduce-scatter the gradient (mean), update 1 / world of the parameters, all-gather them */
int vf_comm_reduce_scatter_avg_async(vf_comm* c, vf_ctx* ctx, float* buf, int64_t shard_count, int* ticket);
int vf_comm_allgather_async(vf_comm* c, vf_ctx* ctx, float* buf, int64_t shard_count, int* ticket);
/* rank `root`'s buf[0..count) to every rank on the exchange stream (ticketed like the collectives above): the row blocks of a tensor
 * whose rows do not split evenly over the ranks travel as one broadcast per rank (vf_net_fused_adam_row_range) */
int vf_comm_broadcast_async(vf_comm* c, vf_ctx* ctx, float* buf, int64_t count, int root, int* ticket);
int vf_comm_wait(vf_comm* c, vf_ctx* ctx, int ticket);
int vf_comm_allreduce_inline(vf_comm* c, vf_ctx* ctx, void* buf, int64_t count, int dtype, int op);
int vf_comm_broadcast(vf_comm* c, vf_ctx* ctx, void* buf, int64_t count, int dtype, int root);
int vf_comm_barrier(vf_comm* c, vf_ctx* ctx);
int vf_comm_destroy(vf_comm* c);

/* ---- per-kernel timers (the reference has three torch.Timers, train.lua:241-243; these are finer) ----
 * Between vf_prof_begin and vf_prof_end every kernel launch of the library is bracketed by HIP events on the
 * context's stream.  vf_prof_end synchronises and aggregates per kernel name; vf_prof_get reads entry i:
 * launches, total milliseconds, and the ALGORITHMIC flops / bytes the launches were asked to do. */
int vf_prof_begin(vf_ctx* ctx);
int vf_prof_end(vf_ctx* ctx);
int vf_prof_count(void);
int vf_prof_get(int i, char* name, int name_cap, int64_t* launches, double* ms, double* flops, double* bytes);

/* ---- nn.Sequential as one object: the FAST path behind the boundary (net_{create, forward, backward,
 * update_grad_input, parameters}) ---------------------------------------------------------------------------------------------
 * util.cudnn(net) (util.lua:108-131) is where the reference swaps a net onto a GPU backend; from then on its drivers only call
 * net:forward / :backward / :updateGradInput / :getParameters / :apply(bias:zero()) / :zeroGradParameters / :evaluate
 * (train.lua:245-263, 278-410; train_vid_weighted.lua:330-355, 373-537).  vf_net is that net: hand over the layer list the
 * reference builds with netG:add(...) / netD:add(...) (train.lua:87-199) and drive it with one call per Torch7 method.  It
 * executes the plan with every cross-layer shortcut of the hot path (csrc/vf_net.hip): activations in their producer's
 * epilogue, BatchNorm statistics as a by-product of the neighbouring GEMMs (vf_bn_fuse_next_* / vf_bn_*_pre), operands as bf16
 * planes handed from producer to consumer (vf_pconv_*), weight planes of the whole net refreshed in one launch per parameter
 * update, every weight gradient of a walk in one grouped launch and every conv bias gradient in two, lazy gradient zeroing,
 * netD's real + fake passes as one batch of 2B with BatchNorm per half (vf_net_set_batch_groups), backward walks cut at a
 * gradient bucket (vf_net_backward_range), SyncBN over vf_comm_*.  The benched iteration runs through exactly these calls
 * (bench.py --host cabi; video-filler_amd/cnet.py and lua/hipnn.lua's hipnn.Net are thin hosts of it).
 * Chain nets only (the table modules of train.lua's option branches stay with a module-by-module host).
 * Activations NHWC, weights channels-last; the flat parameter buffer holds {weight, bias} ({gamma, beta}) module by module,
 * segments padded to 64 floats (vf_net_param_offset).  All calls enqueue on the context's stream; buffers whose need depends on
 * the path a pass takes (planes) are allocated at first use, so run one iteration before capturing a hipGraph. */
enum { VF_L_CONV = 1, VF_L_FULLCONV = 2, VF_L_BN = 3, VF_L_ACT = 4, VF_L_VIEW = 5 };
typedef struct vf_layer_desc {
  int kind;             /* VF_L_* */
  int nin, nout;        /* conv / full-conv planes; BatchNorm: nout = channels */
  int k, stride, pad;   /* conv / full-conv */
  int act;              /* VF_L_ACT: VF_ACT_LRELU / RELU / TANH / SIGMOID */
  float slope;          /* LeakyReLU negval */
  float eps, momentum;  /* BatchNorm (0 -> 1e-5 / 0.1) */
} vf_layer_desc;
typedef struct vf_net vf_net;
int vf_net_create(vf_ctx* ctx, vf_net** out, const vf_layer_desc* layers, int nlayers, int B, int C, int H, int W);
int vf_net_destroy(vf_net* net);
/* a new input shape: activations / planes / BatchNorm scratch re-planned, parameters and running statistics kept (Torch7
 * modules resize their outputs on the fly).  Synchronises; not inside a capture. */
int vf_net_reshape(vf_net* net, int B, int C, int H, int W);
int vf_net_parameters(vf_net* net, float** params, float** grads, int64_t* count);   /* net:getParameters() */
/* host-owned flat storage (count >= vf_net_parameters' count floats each, 16-byte aligned, same layout) instead of the net's
 * own: Torch7 keeps parameters in Lua-owned tensors, whose weight / bias views all alias ONE storage after getParameters().
 * Nothing is copied.  NULL, NULL: back to the net's own buffers. */
int vf_net_bind_parameters(vf_net* net, float* params, float* grads, int64_t count);
int64_t vf_net_param_offset(const vf_net* net, int layer, int which, int64_t* length); /* which: 0 weight/gamma, 1 bias/beta; -1 if none */
int vf_net_bn_running(vf_net* net, int layer, float** running_mean, float** running_var);
int vf_net_bind_bn_running(vf_net* net, int layer, float* running_mean, float* running_var);   /* host-owned running statistics */
int vf_net_bn_saved(vf_net* net, int layer, float** save_mean, float** save_invstd);          /* [groups][C] of the last forward */
int vf_net_training(vf_net* net, int train);                                          /* net:training() / net:evaluate() */
int vf_net_zero_grad(vf_net* net);                                                    /* net:zeroGradParameters() (lazy) */
/* the conv-bias sweep of both closures (train.lua:279-280), one launch; `other` (may be NULL): the second net of the sweep */
int vf_net_zero_conv_biases(vf_net* net, vf_net* other);
int vf_net_forward(vf_net* net, const float* x, const float** y);                     /* net:forward(input) */
int vf_net_backward(vf_net* net, const float* x, const float* gy, const float** gx);  /* net:backward(input, gradOutput) */
int vf_net_update_grad_input(vf_net* net, const float* x, const float* gy, const float** gx); /* train.lua:366 */
/* vf_net_backward leaves out the first layer's gradInput (*gx = NULL): Torch7 always computes it, the drivers never read it for
 * netD's two full backward passes nor for netG's (train.lua:318,348,403) */
int vf_net_set_skip_input_grad(vf_net* net, int on);
/* The next forwards carry G concatenated, independent batches (netD's [real; fake], train.lua:331-349): BatchNorm statistics,
 * running-average updates (in group order) and backward sums per group — what G separate calls compute — while the convolutions
 * see one batch.  vf_net_update_grad_input_group: updateGradInput over group g alone (x / gy hold that group's samples; saved
 * activations and statistics are that group's): fGx's pass over the fake half. */
int vf_net_set_batch_groups(vf_net* net, int G);
int vf_net_update_grad_input_group(vf_net* net, const float* x, const float* gy, int g, int G, const float** gx);
/* Data parallel: the walk cut where a gradient bucket is complete.  The net's execution plan has vf_net_plan_size entries (an
 * absorbed activation shares its producer's); vf_net_bucket_split gives the plan index k and flat offset of the shortest tail
 * plan[k:] owning >= frac of the parameters; vf_net_backward_range(hi, lo) runs backward over entries hi-1 .. lo (hi < 0: from
 * the top; gy = what the entry above hi returned).  After the walk over [k, top) the flat gradient [offset, end) is final. */
int vf_net_plan_size(const vf_net* net);
/* 1 if the last forward left the SIGN BITS of this layer's activated output beside it (a 3-channel-input conv + (Leaky)ReLU): the
 * data-gradient pass of the conv above then reads its derivative mask from them — one broadcast word per pixel and 32 channels
 * instead of the fp32 activation.  Internal to the net object; not under an activation observer. */
int vf_net_layer_has_act_bits(const vf_net* net, int layer);
int vf_net_bucket_split(const vf_net* net, double frac, int* plan_index, int64_t* flat_offset);
int vf_net_backward_range(vf_net* net, const float* x, const float* gy, int hi, int lo, int need_input_grad, const float** gx);
/* the same cut without interrupting the data-gradient chain: vf_net_backward_split walks the WHOLE net, then launches the weight
 * and bias gradients of plan entries >= k only (flat gradient [offset, end) final: start its exchange); vf_net_backward_finish
 * launches the gradients of the entries below k.  Nothing else may record weight gradients on the context in between. */
int vf_net_backward_split(vf_net* net, const float* x, const float* gy, int k, int need_input_grad, const float** gx);
int vf_net_backward_finish(vf_net* net);
/* optim.adam fused into the bottleneck pair's weight gradients (vf_wgrad_adam_outer).  vf_net_set_fused_adam(1): backward walks
 * leave out the weight gradient of every layer the fused kernel takes and remember its operands (the module buffers, untouched
 * until the next forward); *count = the number of such layers (0: nothing to fuse — keep the plain update).  vf_net_fused_adam_range
 * names the i-th layer's weight slice of the flat vectors, which the host's own vf_adam_apply calls must leave out.
 * vf_net_adam_fused, after the backward pass and vf_adam_prep: the fused kernel per marked layer (m, v: the optimiser's flat state,
 * laid out like the parameters; keep_grad: gradParameters receives those slices too).  A marked layer whose gradient was not fresh
 * (a second backward without zeroGradParameters) was accumulated the plain way and gets vf_adam_apply on its slice. */
int vf_net_set_fused_adam(vf_net* net, int on, int* count);
int vf_net_fused_adam_range(const vf_net* net, int i, int64_t* offset, int64_t* length);
int vf_net_adam_fused(vf_net* net, float* m, float* v, double beta1, double beta2, double eps, const int32_t* t_dev, int keep_grad);
/* Data parallel with the fused update: the two weight gradients (92 % of the generator's bytes) are NOT exchanged.  Each rank packs
 * the operands they are the product of — batch x (Nu + Ncols) floats per layer, 6 MB at batchSize 64 against 262 MB of gradient —
 * into its segment of a gather buffer (vf_net_fused_adam_pack, after the backward pass; vf_net_fused_adam_pack_size floats, a
 * multiple of 4), the host all-gathers the segments (vf_comm_allgather_async), and vf_net_adam_fused_gathered forms the gradient
 * of the GLOBAL batch in the fused kernel on every rank (world * batch rows, scaled by 1 / world: the mean over ranks, the same
 * bits on every rank) and applies the update.  The rest of the flat gradient is all-reduced as before. */
int vf_net_fused_adam_pack_size(const vf_net* net, int64_t* floats);
int vf_net_fused_adam_pack(vf_net* net, float* segment);
int vf_net_adam_fused_gathered(vf_net* net, const float* all_segments, int world, int64_t seg_stride, float* m, float* v, double beta1,
                               double beta2, double eps, const int32_t* t_dev, int keep_grad);
/* ... with the update sharded by weight ROWS: this rank (row_rank of row_world) forms the global-batch gradient of its 1 / row_world of
 * every fused tensor's rows and updates them (m, v: those rows only); the host then all-gathers the updated rows of each
 * vf_net_fused_adam_range slice (equal, contiguous row blocks).  vf_net_fused_adam_rows_ok: do the row counts split that way? */
int vf_net_fused_adam_rows_ok(const vf_net* net, int row_world);
/* The row blocks: rank r of row_world owns rows [r * bs, min(Nu, (r + 1) * bs)), bs = 2 * ceil(Nu / (2 * row_world)) — equal blocks
 * where the rows split evenly, a shorter last block where they do not (every block at least 64 rows: vf_net_fused_adam_rows_ok).
 * vf_net_fused_adam_row_range: that block of fused layer i (of vf_net_set_fused_adam's count) as an element range of the flat vectors. */
int vf_net_fused_adam_row_range(const vf_net* net, int i, int row_rank, int row_world, int64_t* offset, int64_t* length);
/* Hiding the exchange of the updated rows: the host issues it on the communicator's stream right after the update (vf_comm_allgather_async
 * / vf_comm_broadcast_async) and hands the tickets to the net; the NEXT vf_net_forward runs the layers in front of the bottleneck conv
 * (train.lua:89-104; they read none of those weights) beside the transfer and waits for the tickets in front of the first layer the fused
 * update takes.  One-shot. */
int vf_net_forward_wait_fused(vf_net* net, vf_comm* comm, int ticket);
int vf_net_adam_fused_gathered_rows(vf_net* net, const float* all_segments, int world, int64_t seg_stride, float* m, float* v, double beta1,
                                    double beta2, double eps, const int32_t* t_dev, int keep_grad, int row_rank, int row_world);
/* SyncBN: BatchNorm sums all-reduced over `comm` (world ranks; statistics of the global batch).  force: take that path at world 1
 * too.  comm NULL / world 1 / force 0: device-local statistics.  world > 1 with comm NULL is refused (it would silently be local). */
int vf_net_set_sync_bn(vf_net* net, vf_comm* comm, int world, int force);
/* Weight planes (bf16 shadows of the conv weights the planes kernels read).  Unmanaged (default): refreshed at the start of every
 * forward / backward call.  Managed: the host calls vf_net_refresh_weight_planes once after each parameter update (optim.adam, a
 * checkpoint load) — one launch per net and update instead of one per call. */
int vf_net_set_weight_planes_managed(vf_net* net, int on);
int vf_net_refresh_weight_planes(vf_net* net);
/* where the planes kernels are used (process-wide; defaults 3 GFLOP per pass and 1024 GEMM rows) */
int vf_net_set_planes_gate(double min_gflop_per_pass, int min_rows);
int vf_net_layer_output(vf_net* net, int layer, const float** y);                     /* net.modules[i].output */
int vf_net_layer_grad_input(vf_net* net, int layer, const float** gx);                /* net.modules[i].gradInput */
int vf_net_layer_shape(const vf_net* net, int layer, int* B, int* C, int* H, int* W, int* Co, int* Ho, int* Wo);
/* module `layer` writes its output into the host's buffer (e.g. netG's last convolution straight into the fake half of netD's
 * [real; fake] input); NULL: the net's own buffer again */
int vf_net_bind_output(vf_net* net, int layer, float* y);
/* Observer of every (Leaky)ReLU output of a forward pass, called on the host right after the producing launch was enqueued:
 * fn(user, layer index of the activation module, device pointer, element count) -> 1 if it edited the tensor (on the context's
 * stream), 0 if not, < 0 on error.  The parity tests pin derivative choices at the kink with it; NULL: none. */
typedef int (*vf_net_act_observer)(void* user, int layer, float* y, int64_t numel);
int vf_net_set_act_observer(vf_net* net, vf_net_act_observer fn, void* user);

/* ---- roctx ranges (the reference's tracing is three torch.Timers; this is the profiler-visible counterpart) ----
 * vf_range_push / vf_range_pop / vf_mark forward to roctx when a roctx library is present (librocprofiler-sdk-roctx.so as
 * injected by rocprofv3, else libroctx64.so; $VF_ROCTX_LIB overrides) and are no-ops otherwise: `rocprofv3 --marker-trace
 * --kernel-trace` shows them beside the kernels.  vf_trace_enable(1) (or VF_ROCTX=1 in the environment) additionally puts one
 * range around every launch site of the library, named like the vf_prof_* kernel table.  vf_trace_available: 1 if bound.
 * vf_range_depth: ranges currently open (pushes minus pops). */
int vf_trace_available(void);
int vf_trace_enable(int on);
int vf_range_push(const char* name);
int vf_range_pop(void);
int vf_mark(const char* message);
int vf_range_depth(void);

#ifdef __cplusplus
}
#endif
#endif /* VF_HIP_H */
