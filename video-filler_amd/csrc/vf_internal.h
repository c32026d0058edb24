// vf_internal.h — what the .hip files of the library share among themselves: the geometry of a conv pass, and the one declaration
// of every function that one file defines and another calls (grouped by the defining file).  Included by vf_common.h.
#pragma once
struct vf_ctx; struct VfBnSt; struct VfBnRequest; struct VfConvExtras; struct VfPWGradGroup; struct VfFusedLayer; struct WgRecorder;

// One conv layer's geometry as the entry points of include/vf_hip.h take it: batch, the H x W map with Cin channels the layer
// reads (a full-conv's low-resolution side), Cout channels out, kernel size, stride, padding.
struct VfConvShape {
  int B, H, W, Cin, Cout, k, stride, pad;
  int out_h() const { return (H + 2 * pad - k) / stride + 1; }      // nn.SpatialConvolution's output map
  int out_w() const { return (W + 2 * pad - k) / stride + 1; }
  int full_out_h() const { return (H - 1) * stride - 2 * pad + k; }      // nn.SpatialFullConvolution's output map
  int full_out_w() const { return (W - 1) * stride - 2 * pad + k; }
  bool pow2_map() const { return H > 0 && (H & (H - 1)) == 0 && W > 0 && (W & (W - 1)) == 0; }
  // the two geometries of the reference's main nets: 4x4 stride 2 pad 1, and 4x4 stride 1 pad 0 (the bottleneck, the 512 -> 1 head)
  bool main_net_taps() const { return k == 4 && ((stride == 2 && pad == 1) || (stride == 1 && pad == 0)); }
  // a conv the matrix-core kernels serve (vf_conv_is_fast); vf_conv_generic.hip takes every other one
  bool matrix_core_conv() const { return main_net_taps() && (stride == 2 || (H == 4 && W == 4)) && pow2_map(); }
  // The layer run the other way round, as the shape of the pass that computes its data-gradient: a conv's is a full-conv from its
  // output map (Cout channels) back to Cin, a full-conv's is a conv from its output map back to Cin.
  VfConvShape gradient_of_conv() const { return {B, out_h(), out_w(), Cout, Cin, k, stride, pad}; }
  VfConvShape gradient_of_full() const { return {B, full_out_h(), full_out_w(), Cout, Cin, k, stride, pad}; }
};

// ---- vf_conv.hip
void vf_internal_wg_free(vf_ctx* ctx);
// The split-K combine of the GEMM hosts, plain or leaving BatchNorm statistics partials (st), and whether a shape fits the latter
int vf_internal_slab_reduce(vf_ctx* ctx, const float* slab, float* dst, const float* bias, int64_t total, int N, int ksplit, int act,
                            float slope, const float* dmask, int dact, float dslope, const VfBnSt* st, int st_groups);
bool vf_internal_slab_st_ok(int64_t total, int N, int groups, int rows_cap, int* blocks_per_group);
// The conv entry points with their extras as an argument (ex is never NULL, except where noted); the C-ABI forms wrap them
int vf_internal_conv2d_fwd(vf_ctx* ctx, const float* x, const float* w, const float* bias, float* y, const VfConvShape& s, int act,
                           float slope, VfConvExtras* ex);
int vf_internal_conv2d_bwd_data(vf_ctx* ctx, const float* gy, const float* w, float* gx, const VfConvShape& s, VfConvExtras* ex);
int vf_internal_conv2d_bwd_data_act(vf_ctx* ctx, const float* gy, const float* w, float* gx, const float* x_act, int act, float slope,
                                    const VfConvShape& s, VfConvExtras* ex);
int vf_internal_conv2d_bwd_weight(vf_ctx* ctx, const float* x, const float* gy, const void* x_planes, const void* gy_planes, float* gw,
                                  float* gb, const VfConvShape& s, float beta, const VfConvExtras* ex);      // ex may be NULL
int vf_internal_deconv2d_fwd(vf_ctx* ctx, const float* x, const float* w, const float* bias, float* y, const VfConvShape& s, int act,
                             float slope, VfConvExtras* ex);
int vf_internal_deconv2d_bwd_data(vf_ctx* ctx, const float* gy, const float* w, float* gx, const VfConvShape& s, VfConvExtras* ex);
int vf_internal_deconv2d_bwd_weight(vf_ctx* ctx, const float* x, const float* gy, const void* x_planes, const void* gy_planes, float* gw,
                                    float* gb, const VfConvShape& s, float beta);
// a BatchNorm request as vf_bn_fuse_next_fwd / _bwd form it
int vf_internal_bn_request_fwd(VfBnRequest* r, const float* shift, double* part, int part_rows_cap, int groups);
int vf_internal_bn_request_bwd(VfBnRequest* r, const float* x, const float* y_act, int act, float slope, const float* save_mean,
                               double* part, int part_rows_cap, int groups);

// ---- vf_conv_thin.hip: the 3-channel image side (vf_internal_deconv_thin_out reads s as a full-conv)
int vf_internal_conv2d_fwd_planes(vf_ctx* ctx, const float* x, const float* w, const float* bias, float* y, void* y_planes,
                                  const VfConvShape& s, int act, float slope, VfConvExtras* ex);
int vf_internal_conv_thin_fwd(vf_ctx* ctx, const float* x, const float* w, const float* bias, float* y, void* y_planes,
                              const VfConvShape& s, int act, float slope, VfConvExtras* ex);
int vf_internal_deconv_thin_out(vf_ctx* ctx, const float* x, const float* w, const float* bias, float* y, const VfConvShape& s, int act,
                                float slope);

// ---- vf_conv_generic.hip: the option branches' convolutions (5x5 stride 2 pad 2 / 34, 1x1: train.lua:109-113,158-170)
int vf_internal_gconv_fwd(vf_ctx* ctx, const float* x, const float* w, const float* bias, float* y, const VfConvShape& s, int act,
                          float slope);
int vf_internal_gconv_bwd_data(vf_ctx* ctx, const float* gy, const float* w, float* gx, const VfConvShape& s);
int vf_internal_gconv_bwd_weight(vf_ctx* ctx, const float* x, const float* gy, float* gw, float* gb, const VfConvShape& s, float beta);

// ---- vf_pgemm.hip: the planes-fed passes (4x4 stride 2 pad 1).  gather: s a conv; scatter: s a full-conv
bool vf_internal_pconv_supported(int mfma_mode, const VfConvShape& s, bool transposed);
int vf_internal_pconv_gather(vf_ctx* ctx, const void* ap, const void* wp, const float* bias, float* y, const VfConvShape& s, int act,
                             float slope, VfConvExtras* ex);
int vf_internal_pconv_scatter(vf_ctx* ctx, const void* ap, const void* wp, const float* bias, float* y, const VfConvShape& s, int act,
                              float slope, const float* dmask, int dact, float dslope, VfConvExtras* ex);
int vf_internal_pwgrad_group(vf_ctx* ctx, const VfPWGradGroup& G, int blocks, const char* name, double flops);

// ---- vf_smallm.hip: the bottleneck GEMMs at a small batch (launch_igemm)
int vf_internal_smallm_plan(int form, int M, int N, int K, size_t ws_bytes);
int vf_internal_smallm_launch(vf_ctx* ctx, int form, const float* A, const float* W, float* slab, int M, int N, int K, int ksplit);

// ---- vf_wgrad_small.hip: the bottleneck weight gradient (K = batch), alone and with optim.adam in its epilogue
int vf_internal_wgrad_smallk(vf_ctx* ctx, const float* U, const float* V, float* dW, int K, int Nu, int Ncols, float beta);
int vf_internal_adam_fused_multi(vf_ctx* ctx, const VfFusedLayer* layers, int nl, double beta1, double beta2, double eps,
                                 const int32_t* t_dev);

// ---- vf_bn.hip: gb = beta * gb + column sums of g [P][C] (a conv's bias gradient)
int vf_internal_colsum(vf_ctx* ctx, const float* g, float* gb, int64_t P, int C, float beta);
