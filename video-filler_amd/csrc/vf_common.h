// vf_common.h — shared host-side plumbing for the gfx950 backend (context, error reporting, launch checks).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/vf_hip.h"
#include "vf_internal.h"

#define VF_API extern "C" __attribute__((visibility("default")))

// BatchNorm statistics as a by-product of the GEMM that produces the tensor: the epilogue (or the split-K slab reduce) of a
// conv-like launch leaves per-tile partial sums that vf_bn_train_fwd_pre / vf_bn_bwd_pre finalize, so the tensor is not read
// again just to be summed.
struct VfBnSt {
  int mode;               // 0 none; 1 forward: s1 = sum(v - shift), s2 = sum((v - shift)^2); 2 backward: s1 = sum(g), s2 = sum(g*(x - mean)),
                          //   g = the launch's output masked by the activation derivative (the output IS stored masked)
  const float* vec;       // mode 1: [C] shift (running_mean); mode 2: [groups][C] save_mean
  const float* x;         // mode 2: the BatchNorm input at the output's index
  double* part;           // [groups][rows_per_group][2][C]
  int rows_per_group;     // partial rows each group ends up with (what the finalize kernels walk)
  int tiles_per_group;    // GEMM epilogue: row tiles per batch group; slab reduce: blocks per group
  int zpar;               // GEMM epilogue: output-parity classes sharing a row tile (1 or 4)
};
// the request for them: st carries mode, vec, x and part; the launch that takes it fills in the plan (vf_plan_bn_stats)
struct VfBnRequest {
  VfBnSt st = {};
  const float* yact = nullptr;  // mode 2: activated BatchNorm output (the derivative mask), its activation
  int act = 0;
  float slope = 0.f;
  int groups = 1, rows_cap = 0;
};

// What one conv-like pass does beyond its convolution: arguments of the internal entry points (vf_internal_conv2d_* and the
// hosts below them), so that what a launch does is visible where it is called.  A default-constructed value is a plain pass.
struct VfConvExtras {
  VfBnRequest bn;               // BatchNorm statistics of the output; bn_result_rows: rows_per_group written, 0: this pass could not
  int bn_result_rows = 0;
  // sign bits of an activated tensor (vf_net.hip).  act_bits_out: the thin-input conv forward (vf_conv_thin.hip) also writes, per
  // output pixel and 64-channel group, two words — bit j of word h = (channel 2j + h) > 0; act_bits_written says whether it did.
  // dmask_bits: the planes-fed transposed pass (vf_pgemm.hip) reads its activation-derivative mask from such bits (a broadcast
  // word per pixel) instead of the fp32 activation — 2 MB instead of 67 MB for E2's data-gradient (train.lua:90: the LeakyReLU
  // below the second conv)
  unsigned* act_bits_out = nullptr;
  int act_bits_written = 0;
  const unsigned* dmask_bits = nullptr;
  // the 512 -> 1 head passes of vf_conv.hip (k_dot_bwd_data / k_dot_bwd_weight: netD's last conv, train.lua:195-196) multiply
  // their gradOutput by the derivative of the Sigmoid fused into that conv, evaluated from the activated output — instead of a
  // pass of its own over B values in front of them
  const float* dot_act_y = nullptr;
  int dot_act = 0;
  float dot_act_slope = 0.f;
};

struct vf_ctx {
  int device;
  hipStream_t stream;
  void* ws;         // caller-owned scratch (split-K slabs, reduction partials)
  size_t ws_bytes;
  size_t ws_front;  // bytes at the front of ws currently held by an im2col / column buffer (thin-channel passes)
  int mfma_bf16;    // 0: native f32 MFMA; 1: operands rounded to bf16; 3 (default): exact three-plane bf16 split
  WgRecorder* wg;   // the weight-gradient group recorder and its open flag (vf_conv.hip: made on first use, freed by vf_internal_wg_free)
  // the public two-call protocol around a conv (module-by-module hosts): vf_bn_fuse_next_* leave a request here, the next
  // forward / data-gradient entry point takes it, unconditionally (vf_take_pending), and vf_bn_fuse_result reads what it made of it
  VfBnRequest bn_pending;
  int bn_result_rows = 0;
};

// A public forward / data-gradient entry point: moves the pending request out of the context before anything else, so that a
// refused call leaves nothing behind for an unrelated later launch, and hands it to the pass as an argument.
template <class F>
static inline int vf_take_pending(vf_ctx* ctx, F&& pass) {
  VfConvExtras ex;
  ex.bn = ctx->bn_pending;
  ctx->bn_pending.st.mode = 0;
  const int rc = pass(&ex);
  if (ex.bn.st.mode) ctx->bn_result_rows = rc ? 0 : ex.bn_result_rows;
  return rc;
}

static inline char* vf_ws_ptr(vf_ctx* c) { return (char*)c->ws + c->ws_front; }
static inline size_t vf_ws_avail(vf_ctx* c) { return c->ws_bytes > c->ws_front ? c->ws_bytes - c->ws_front : 0; }

void vf_set_error(const char* fmt, ...);

#define VF_CHECK_HIP(expr)                                                              \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess) {                                                             \
      vf_set_error("%s:%d: %s failed: %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return 1;                                                                         \
    }                                                                                   \
  } while (0)

#define VF_REQUIRE(cond, ...)      \
  do {                             \
    if (!(cond)) {                 \
      vf_set_error(__VA_ARGS__);   \
      return 2;                    \
    }                              \
  } while (0)

#define VF_LAUNCH_CHECK() VF_CHECK_HIP(hipGetLastError())

// per-launch profiling scope (active only between vf_prof_begin / vf_prof_end)
bool vf_prof_enabled();
// begin: appends a record and returns its index; end (begin false): records the stop event of record `idx` (scopes nest: an
// inner VfProf or a timed launch inside a scope appends records of its own)
int vf_prof_push(vf_ctx* ctx, const char* name, double flops, double bytes, bool begin, int idx = -1);
// roctx range around a launch site (vf_trace.hip): active with vf_trace_enable(1) / VF_ROCTX=1, free otherwise
bool vf_trace_enabled();
extern "C" int vf_range_push(const char* name);
extern "C" int vf_range_pop(void);
struct VfRange {
  bool on;
  explicit VfRange(const char* name) : on(vf_trace_enabled()) {
    if (on) vf_range_push(name);
  }
  ~VfRange() {
    if (on) vf_range_pop();
  }
};
struct VfProf {
  vf_ctx* c;
  bool on;
  VfRange range;
  int idx = -1;
  VfProf(vf_ctx* ctx, const char* name, double flops, double bytes) : c(ctx), on(vf_prof_enabled()), range(name) {
    if (on) idx = vf_prof_push(c, name, flops, bytes, true);
  }
  ~VfProf() {
    if (on) vf_prof_push(c, nullptr, 0, 0, false, idx);
  }
};

// Single-kernel launches are timed with hipExtLaunchKernelGGL's start/stop events: the elapsed time is the kernel's own
// execution (what rocprofv3's kernel trace reports), without the launch gap an event pair around the call would add.
bool vf_prof_ext(const char* name, double flops, double bytes, hipEvent_t* e0, hipEvent_t* e1);
#define VF_LAUNCH_TIMED(ctx, name, flops, bytes, kernel, grid, block, ...)                                   \
  do {                                                                                                       \
    VfRange _vr(name);                                                                                       \
    hipEvent_t _e0, _e1;                                                                                     \
    if (vf_prof_ext(name, flops, bytes, &_e0, &_e1))                                                         \
      hipExtLaunchKernelGGL(kernel, grid, block, 0, (ctx)->stream, _e0, _e1, 0, __VA_ARGS__);                \
    else                                                                                                     \
      hipLaunchKernelGGL(kernel, grid, block, 0, (ctx)->stream, __VA_ARGS__);                                \
  } while (0)

// compile-time loop: f(VfIntC<0>{}) ... f(VfIntC<N-1>{}) — the index is a constant inside the body
template <int I> struct VfIntC { static constexpr int value = I; };
template <int N, int I = 0, typename F>
__device__ __forceinline__ void vf_static_for(F&& f) {
  if constexpr (I < N) {
    f(VfIntC<I>{});
    vf_static_for<N, I + 1>(f);
  }
}

// Weight gradient from PRE-SPLIT operands (vf_pgemm.hip: k_pwgrad_group; recorded by vf_conv.hip's group recorder).
//   dW[n][tap][c] = sum_p U[p][n] * V[(b, 2 my - 1 + kh, 2 mx - 1 + kw)][c]      p = (b, my, mx) on the low-resolution grid
// Up / Vp: bf16 planes [3][pixels][channels] of the two operands (conv: U = gradOutput, V = input; full-conv: U = input,
// V = gradOutput).  out: dW, or the split-K slabs (ksplit > 1: slab s at s * Nu * 16 * Cv elements).
struct VfPWGrad {
  const void* Up;               // NULL: the fp32-fed form below
  const void* Vp;
  // fp32-fed form (the two bottleneck layers riding in the same launch: their planes do not exist, K = batch): plain matrices
  // Uf [P][Nu], Vf [P][16 * Cv]; the block splits them on their way into LDS
  const float* Uf;
  const float* Vf;
  float* out;
  unsigned u_ps, v_ps;          // plane strides in bytes
  int P, lgMh, lgMw;            // low-resolution pixels = B << (lgMh + lgMw)
  int Nu, Cv, Hv, Wv;
  int gx, gy, gz;               // column tiles (16 * Cv / 128), row tiles (Nu / 128), split-K
  int ksplit, nk;               // nk = P / 32 K steps
  float beta;                   // ksplit == 1: dW = beta * dW + sum
};
#define VF_PWG_MAX 16
struct VfPWGradGroup {
  int n;
  int blk_off[VF_PWG_MAX + 1];  // multiples of 8 (the XCD-aware tile order of a layer assumes blockIdx % 8 == local id % 8)
  VfPWGrad d[VF_PWG_MAX];
};

static inline int vf_ilog2(int v) {  // v must be a power of two
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}
static inline bool vf_is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
static inline int64_t vf_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline bool vf_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline size_t vf_up256(size_t v) { return (v + 255) & ~(size_t)255; }
// Regions of a workspace one behind the other, each starting on a 256-byte boundary: take(bytes) -> the region's offset; `at` is
// the size of everything taken so far
struct VfCarve {
  size_t at = 0;
  size_t take(size_t bytes) {
    const size_t o = at;
    at += vf_up256(bytes);
    return o;
  }
};
// What every vf_*_encode entry requires behind its plan, before any launch: a known kind of source and room for the plan's two
// bounds.  who names the entry, ch the channel count as its message writes it ("C" or "3"), batch the geometry in words.
static inline int vf_check_encode_entry(const char* who, int kind, const char* ch, const char* batch, size_t ws_bytes, size_t ws_need,
                                        size_t out_cap, size_t out_need) {
  VF_REQUIRE(kind == 0 || kind == 1, "%s: kind %d is not 0 (float N x %s x H x W) or 1 (uint8 N x H x W x %s)", who, kind, ch, ch);
  VF_REQUIRE(ws_bytes >= ws_need, "%s: the workspace holds %zu bytes, %s need %zu", who, ws_bytes, batch, ws_need);
  VF_REQUIRE(out_cap >= out_need, "%s: the output holds %zu bytes, %s may take %zu", who, out_cap, batch, out_need);
  return 0;
}
#define VF_OOB 0x80000000u   // byte offset that is always out of range of a buffer descriptor (operands are < 2 GiB)

// Descriptor tables of the one-launch-per-net kernels, built by the hosts (vf_net.hip; video-filler_amd/backend.py mirrors the
// layouts as COLSUM_DESC / WPLANES_DESC).  VfColsumDesc: every conv bias gradient of a backward walk (vf_bn.hip,
// vf_bias_grad_multi).  VfWpDesc: every weight of a net to planes (vf_pgemm.hip, vf_weight_planes_multi).
struct VfColsumDesc {
  const float* g;          // [P][C] gradOutput
  float* gb;               // [C]   gradBias:  gb = beta*gb + column sums
  double* part;            // [gx][C] scratch partials
  int64_t P;
  int C, cq, rows_per_block, gx, gy;
  int blk1_off, blk2_off;  // first block of this layer in stage 1 / stage 2
  float beta;
};
static_assert(sizeof(VfColsumDesc) == 64, "descriptor layout is shared with the host mirror");
struct VfWpDesc {
  const float* w;        // physical [d0][16][d1]
  void* nat;             // planes [3][d0][16][d1]
  void* tr;              // planes [3][d1][16][d0]
  int d0, d1;
  int gx, gz;            // 32-wide tiles over d0 and d1
  int blk_off;           // first block of this weight
  int pad;
};
static_assert(sizeof(VfWpDesc) == 48, "descriptor layout is shared with the host mirror");

// The split-K count of a GEMM launch, written once for ig_plan, wg_plan (vf_conv.hip) and pg_plan (vf_pgemm.hip): a grid below
// three quarters of `target` blocks, with at least min_nk K steps, is split into up to nk / k_per_split ranges — as many as bring
// it to the target and whose slabs (slab_bytes each) fit the workspace — and the ranges are then shaped by the caller's rule.
enum VfKRanges {
  VF_K_EVEN_OUT,      // ceil(nk / ksplit) steps per range, no empty trailing range
  VF_K_WHOLE_EQUAL    // ksplit divides nk: every tile runs the same number of steps
};
static inline int vf_split_k(int64_t blocks, int target, int nk, int min_nk, int k_per_split, size_t slab_bytes, size_t ws_avail,
                             VfKRanges rule) {
  if (!(blocks < target * 3 / 4 && nk >= min_nk)) return 1;
  int ksplit = (int)std::min<int64_t>(nk / k_per_split, vf_cdiv(target, blocks));
  while (ksplit > 1 && (size_t)ksplit * slab_bytes > ws_avail) --ksplit;
  if (rule == VF_K_WHOLE_EQUAL) {
    while (ksplit > 1 && nk % ksplit != 0) --ksplit;
    return ksplit;
  }
  if (ksplit < 1) ksplit = 1;
  const int steps = (int)vf_cdiv(nk, ksplit);
  return (int)vf_cdiv(nk, steps);
}

// The statistics plan of a GEMM launch (ig_plan's IGemm, pg_plan's PGemm; bm x . tiles in gm rows, zpar parity classes, ksplit K
// ranges), as data: st.mode 0 is "none".  With one K range per tile the epilogue leaves a partial row per row tile and parity
// class, where the batch groups are whole tiles; under split-K the slab reduce leaves them (`slab`: the combine gets &st).  A
// shape that fits neither, or no request (r NULL: an inner launch), gives mode 0.  Mode 2 stores the output masked by the
// activation derivative, what BatchNorm's backward sums: dmask / dact / dslope are the launch's mask either way.
struct VfBnStPlan {
  VfBnSt st = {};
  bool slab = false;
  const float* dmask = nullptr;
  int dact = 0;
  float dslope = 0.f;
};
template <class G>
static inline VfBnStPlan vf_plan_bn_stats(const VfBnRequest* r, const G& g, int ksplit, int bm, int gm, int zpar) {
  VfBnStPlan p;
  p.dmask = g.dmask; p.dact = g.dact; p.dslope = g.dslope;
  if (!r || !r->st.mode) return p;
  VfBnSt st = r->st;
  st.zpar = ksplit == 1 ? zpar : 1;
  if (ksplit == 1) {
    if (g.M % r->groups != 0 || (g.M / r->groups) % bm != 0 || (int64_t)(gm / r->groups) * zpar > r->rows_cap) return p;
    st.tiles_per_group = gm / r->groups;
  } else if (!vf_internal_slab_st_ok(g.out_elems, g.N, r->groups, r->rows_cap, &st.tiles_per_group)) {
    return p;
  }
  st.rows_per_group = st.tiles_per_group * st.zpar;
  p.st = st;
  if (st.mode == 2) {
    p.dmask = r->yact; p.dact = r->act; p.dslope = r->slope;
  }
  p.slab = ksplit > 1;
  return p;
}
// ... and its one writer: the launch step, once the pass is certain to launch, puts the plan into the kernel's arguments and tells
// the caller's extras what it will find
template <class G>
static inline void vf_take_bn_stats(const VfBnStPlan& p, G& g, VfConvExtras* ex) {
  g.st = p.st;
  g.dmask = p.dmask; g.dact = p.dact; g.dslope = p.dslope;
  if (p.st.mode) ex->bn_result_rows = p.st.rows_per_group;
}
// The tail of a split-K launch (kind: "igemm" or "pconv", the profiling label): the slabs are combined in a fixed order, with the
// BatchNorm partials where the plan left them to this pass
template <class G>
static inline int vf_combine_slabs(vf_ctx* ctx, const char* kind, const G& g, bool slab_st, int groups) {
  if (g.ksplit <= 1) return 0;
  char label[48];
  snprintf(label, sizeof(label), "slab_reduce_%s%s", kind, slab_st ? "_bnstats" : "");
  VfProf prof(ctx, label, 0.0, 4.0 * (double)g.out_elems * (g.ksplit + 1));
  return vf_internal_slab_reduce(ctx, g.slab, g.Y, g.bias, g.out_elems, g.N, g.ksplit, g.act, g.slope, g.dmask, g.dact, g.dslope,
                                 slab_st ? &g.st : nullptr, slab_st ? groups : 1);
}

// optim/adam.lua's element update, fp32 in the reference's operation order (one definition for k_adam and for the weight-gradient
// kernel that applies it in its epilogue, vf_wgrad_small.hip): step = lr * sqrt(1 - b2^t) / (1 - b1^t)
__device__ __forceinline__ void vf_adam_upd(float& xv, float gv, float& mv, float& vv, float b1, float omb1, float b2, float omb2,
                                            float eps, float step) {
  float mi = mv * b1;
  mi = mi + omb1 * gv;
  float vi = vv * b2;
  vi = vi + (omb2 * gv) * gv;
  float d = sqrtf(vi);
  d = d + eps;
  mv = mi;
  vv = vi;
  xv = xv - (step * mi) / d;
}

// One layer of the fused bottleneck update (vf_wgrad_small.hip k_adam_fused_wgrad; built by vf_wgrad_adam_outer* and by vf_net.hip):
//   g = gscale * sum_k U[k][:]^T V[k][:]  consumed by optim.adam on x, m, v [Nu][Ncols]; g_out (may be NULL) also receives it.
// Batch row k lives in segment k / kps at row k % kps, the segments `seg` floats apart (seg == 0: one segment, plain rows).
// Rows [row0, row0 + Nu) of a weight matrix of ldu rows (ldu == 0: all of it — row0 = 0, ldu = Nu): U's batch rows are ldu floats
// long; x, m, v, g_out point at the matrix's first row, the kernel offsets them (data parallel: every rank forms and applies ITS rows).
struct VfFusedLayer {
  const float *U, *V;
  float *x, *m, *v, *g_out;
  int K, Nu, Ncols;
  int kps;
  int64_t seg;
  float gscale;
  int row0, ldu;
};
#define VF_FUSED_MAX 4

// fused activation
__device__ __forceinline__ float vf_act_apply(float v, int act, float slope) {
  switch (act) {
    case VF_ACT_LRELU: return v > 0.f ? v : v * slope;
    case VF_ACT_RELU: return v > 0.f ? v : 0.f;
    case VF_ACT_TANH: return tanhf(v);
    case VF_ACT_SIGMOID: return 1.f / (1.f + expf(-v));
    default: return v;
  }
}
// derivative factor evaluated from the ACTIVATED value y
__device__ __forceinline__ float vf_act_grad(float y, float g, int act, float slope) {
  switch (act) {
    case VF_ACT_LRELU: return y > 0.f ? g : g * slope;
    case VF_ACT_RELU: return y > 0.f ? g : 0.f;
    case VF_ACT_TANH: return g * (1.f - y * y);
    case VF_ACT_SIGMOID: return g * (1.f - y) * y;
    default: return g;
  }
}
