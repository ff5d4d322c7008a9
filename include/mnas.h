/*
 * mnas.h -- C ABI of libmnas_hip.so: the MI355X (gfx950) kernels behind the MNASNet training hot path.
 *
 * The reference (snakers4/mnasnet-pytorch) has no FFI of its own: its hot path is
 *     ConvBlock.forward      src/models/mnasnet.py:58-62   (conv -> BatchNorm2d -> ReLU)
 *     MBConv_block.forward   src/models/mnasnet.py:131-137 (x + seq(x))
 *     loss.backward()        src/train.py:439              (autograd mirror of the above)
 * executed by PyTorch ATen.  This library is what a maintainer binds instead of ATen for that path
 * (INTEGRATION.md shows the ctypes stub).  Every entry point:
 *   - takes plain pointers + sizes (no torch types), device pointers unless stated otherwise;
 *   - launches on the HIP stream passed as `stream` (a hipStream_t cast to void*), never synchronises,
 *     never allocates or frees, keeps no pointer after returning, has no global mutable state;
 *   - returns 0 (MNAS_OK) or a non-zero hipError_t / MNAS_E* code; never throws across the ABI;
 *   - is bit-reproducible: no float atomics, every partial-sum table is reduced in a fixed order.
 *
 * Data layout in HBM
 *   activations / activation gradients : NHWC, bf16, dense, C % 8 == 0 (16-byte channel groups)
 *   network input                      : NCHW fp32 (what train.py:427 hands over), read by the stem kernel
 *   network output / its gradient      : NCHW fp32 (what classifiers.py:109 consumes)
 *   BatchNorm is never applied in place: a conv kernel writes the RAW conv output y (bias included) and
 *   per-workgroup partial (sum, sum of squares); mnas_bn_fwd_finalize turns them into a per-channel
 *   (scale, shift); every CONSUMER applies relu(scale*y+shift) while loading ("act-on-load").
 *   In backward the consumer of a gradient computes dy = c1*(g*[scale*y+shift>0]) + c2*y + c3 while
 *   loading ("dy-on-load"); c1..c3 come from mnas_bn_bwd_finalize.
 *
 * BN coefficient block ("bnbuf"): float[8][C] per ConvBlock application
 *   row 0 scale  s = gamma*invstd         row 4 c3
 *   row 1 shift  t = beta - mean*s        row 5 batch mean
 *   row 2 c1                              row 6 invstd
 *   row 3 c2                              row 7 (reserved)
 *   Frozen statistics (mnas_bn_frozen_tables): rows 5, 6 hold the running mean and 1/sqrt(running_var+eps), c1 = s, c2 = c3 = 0.
 *   Who touches which rows (tests/plan_access.py is this, per launch-list slot, and tests/test_gpu_plan_access.py holds it to the kernels):
 *     mnas_bn_fwd_finalize        writes 0, 1 and, training, 5, 6          mnas_bn_frozen_tables   writes 0..6
 *     act-on-load (scale, shift)  reads 0, 1 (two pointers)               dy-on-load (coef)       reads 0..4
 *     every BatchNorm-backward reduce, fused (red_bn) or mnas_bn_bwd_reduce (bnbuf): reads 0, 1 (the mask) and 5, 6 (xhat)
 *     mnas_bn_bwd_finalize / mnas_bwd_post: read 0, 5, 6, write 2..4; their frozen twins read 0, 5, 6 and write nothing
 *     row 7 is touched by nobody.
 *
 * Partial tables (all fp32, all fully overwritten by their producer, no memset needed; "cols" is the producer's nparts unless the
 * library picks it, in which case the host-side query named below says how many):
 *   statistics and reduce partials      float[2][C][cols]   conv / stem / tconv: cols = nparts; depthwise: mnas_dw_rows;
 *                                                           mnas_se_bwd_apply: mnas_se_bwd_apply_cols; mnas_bn_bwd_reduce: nparts
 *   weight-gradient partials            float[rows][Co][taps*Ci] (depthwise: float[rows][k*k][C]); rows = nsplit / nparts
 *                                       (depthwise: mnas_dw_rows which = 1, 3, 7)
 *   A finalize reads exactly rows x the row size it is told.  Two-level reductions (more than 256 rows) fold every 128-row chunk
 *   into the chunk's first row, in place: those rows are read and then overwritten, the other rows are only read.
 *   mnas_se_proj_finalize reads all N*kseg slabs and overwrites slab n*kseg of every image with the image's gated sum.
 *   mnas_se_bwd_reduce's scratch is float[splits][N][C] = mnas_se_scratch_bytes, written and consumed inside the call.
 */
#ifndef MNAS_H
#define MNAS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MNAS_OK 0
#define MNAS_EINVAL 10001   /* unsupported shape / argument */
#define MNAS_BN_ROWS 8

/* "act-on-load" input: value = scale ? relu(scale[c]*data+shift[c]) : data */
typedef struct MnasActIn {
    const void*  data;    /* bf16 NHWC */
    const float* scale;   /* [C] or NULL */
    const float* shift;   /* [C] or NULL */
} MnasActIn;

/* "dy-on-load" input: dy = c1*(g*[s*y+t>0]) + c2*y + c3, coef = bnbuf rows 0..4.  y == NULL && coef == NULL: g IS dy. */
typedef struct MnasGradIn {
    const void*  g;       /* bf16 NHWC: dL/d(activated output) */
    const void*  y;       /* bf16 NHWC: saved raw conv output */
    const float* coef;    /* float[5][C] */
} MnasGradIn;

int mnas_version(void);                 /* ABI version: 8 (+ the image batch transform and the photometric image ops, and + mnas_grad_sqnorm / mnas_*_step_ex, and + mnas_head_cross_entropy_soft / mnas_img_mix, and + mnas_img_aug, and + mnas_head_cross_entropy_kd, and + mnas_*_step_seg, and + mnas_img_erase / mnas_philox4x32_10, all additive: no layout or opcode changed, so still 8; round 6: + mnas_probe_copy4 / _read; 7 = round 5: + mnas_se_fc_*; 6 = struct layouts changed in rounds 2, 3, twice in round 4 -- 4 = the tiled-block forms,
                                         * 5 = squeeze-excite on load: MnasConvGemm.gate, MnasPwBwd.seg_px -- and in round 5: 6 = the opt-in
                                         * forms that lost their A/B are gone (MnasPwBwd.dy_out / red4, MnasDwBwd.src_* / g_gate / g_bias,
                                         * mnas_dw_exp_*, mnas_irb_*, mnas_gram*, mnas_se_bn_assemble); their opcode numbers stay retired) */
const char* mnas_arch(void);            /* "gfx950" */

/* ---- 1x1 / dense kxk convolution as an implicit GEMM on MFMA (bf16 in, fp32 accumulate) -------------
 * Replaces ATen conv2d forward / conv2d input-gradient for ConvBlock's groups==1 convs
 * (mnasnet.py:48-54 with kernel_size 1 or 3).
 * mode 0 (forward):  out[n,ho,wo,co] = bias[co] + sum_{kh,kw,ci} act(in)[n,ho*s+kh-p,wo*s+kw-p,ci] * W
 *                    in  = (N,Hi,Wi,Ci) read through `act`;  out = (N,Ho,Wo,Co)
 * mode 1 (dgrad):    out[n,hi,wi,ci] = resid + sum_{kh,kw,co} dy[n,(hi+p-kh)/s,(wi+p-kw)/s,co] * W
 *                    in  = dy (N,Hi,Wi,Ci) read through `grad` (Hi,Wi,Ci are the FORWARD OUTPUT dims and
 *                    channels), out = (N,Ho,Wo,Co) are the FORWARD INPUT dims/channels.
 * w: packed bf16 [Co_pad16][Kpad32], K = kh*kw*Ci ordered (tap, ci) -- see mnas_pack_weights.
 * stats (optional, forward): float[2][Co][nparts] partial (sum, sumsq) of the fp32 output, one column per
 * pixel-workgroup (channel-major so the finalize kernel reads one channel contiguously); fully overwritten
 * (no memset needed). */
typedef struct MnasConvGemm {
    int32_t mode;
    int32_t N, Hi, Wi, Ci;
    int32_t Ho, Wo, Co;
    int32_t kh, kw, stride, pad;
    int32_t nparts;          /* pixel-workgroups (grid.x); 1..4096 */
    int32_t reserved;
    MnasActIn  act;
    MnasGradIn grad;
    const void*  w;
    const float* bias;       /* [Co] or NULL */
    const void*  resid;      /* bf16 (N,Ho,Wo,Co) or NULL */
    void*        out;        /* bf16 (N,Ho,Wo,Co) */
    float*       stats;      /* or NULL */
    /* mode 1 only, optional: fuse the NEXT BatchNorm-backward reduction into this kernel's epilogue.  `out` is the
     * gradient g of some ConvBlock's activated output; red_y is that ConvBlock's saved raw output (same shape as
     * out), red_bn its bnbuf.  stats then receives float[2][Co][nparts] partial (sum dz, sum dz*xhat), exactly what
     * mnas_bn_bwd_reduce would produce from (out, red_y, red_bn). */
    const void*  red_y;
    const float* red_bn;
    /* ABI 5, mode 0, 1x1 only, optional: per-(image, input channel) multiplier float[N][Ci] applied AFTER the activation on
     * load, value = relu(scale*x+shift) * gate[n][c] -- the squeeze-excite excitation folded into the project conv's load
     * (mnas_se_gate writes the table).  Requires act.scale; supported shapes: mnas_conv_gemm_gate_ok. */
    const float* gate;
} MnasConvGemm;
int mnas_conv_gemm_gate_ok(int N, int HW, int Ci, int Co);
int mnas_conv_gemm(const MnasConvGemm* a, void* stream);
/* Pixels per tile (64 or 128) mnas_conv_gemm uses for a problem with M output pixels, Co output channels and reduction
 * length K (= kh*kw*Ci of that mode): callers size nparts in whole tiles with it (host-side, no launch). */
int mnas_conv_gemm_tile_pixels(int M, int Co, int K);
/* Preferred nparts for a launch (host-side, no launch): > 0 where the kernel sizes its own persistent grid (the 1x1
 * forward: DMA-pipelined kernel, csrc/mnas_pwf.hip), -1 = caller's choice in whole tiles (mnas_conv_gemm_tile_pixels).
 * taps = kh*kw. */
int mnas_conv_gemm_parts(int mode, int M, int Ci, int Co, int taps);
/* Same question for the dense k x k convs, which depend on the image geometry: > 0 (= N) where mnas_conv_gemm runs the
 * whole-image kernel (csrc/mnas_dimg.hip: 3x3, pad 1, output plane <= 256 pixels, N >= 32; mode 1: stride 1 and a
 * materialised dy), -1 otherwise.  mode 1 arguments as in MnasConvGemm (Hi,Wi,Ci = dy dims, Ho,Wo,Co = result dims). */
int mnas_conv_img_parts(int mode, int N, int Hi, int Wi, int Ci, int Ho, int Wo, int Co, int k, int stride, int pad);
/* Which kernel family mnas_conv_gemm runs for a launch (host-side, no launch; additive within ABI 8).  The query and the launch
 * share one dispatcher function, so the answer is what runs.  Returns MNAS_ROUTE_* or -MNAS_EINVAL for arguments mnas_conv_gemm
 * refuses before it picks a kernel (refusals of a single k_igemm instance -- LDS size, a gate on a wide tile -- still come from the
 * launch).  out (or NULL): int[4], for MNAS_ROUTE_IGEMM = {NT (16-cout tiles per workgroup), PT (64-pixel groups per tile), K
 * elements per LDS chunk (32 / 64 / 128), 1 = parity-class form of the stride-2 3x3 input gradient}, zeros otherwise. */
#define MNAS_ROUTE_PWX   0   /* csrc/mnas_pwx.hip: widening 1x1 forward, weight-stationary */
#define MNAS_ROUTE_PWS   1   /* csrc/mnas_pws.hip: long-reduction 1x1, K split over the waves */
#define MNAS_ROUTE_PWF   2   /* csrc/mnas_pwf.hip: DMA-pipelined 1x1 forward */
#define MNAS_ROUTE_PWD   3   /* csrc/mnas_pwf.hip: DMA-pipelined 1x1 input gradient over a materialised dy */
#define MNAS_ROUTE_C3R   4   /* csrc/mnas_c3r.hip: weight-heavy dense 3x3 on the 7x7 planes */
#define MNAS_ROUTE_DIMG  5   /* csrc/mnas_dimg.hip: dense 3x3, whole image per workgroup */
#define MNAS_ROUTE_C3X   6   /* csrc/mnas_c3x.hip: stride-2 3x3 forward on the large maps */
#define MNAS_ROUTE_IGEMM 7   /* csrc/mnas_gemm.hip: k_igemm, every other shape */
int mnas_conv_gemm_route(const MnasConvGemm* a, int* out);
/* Which template instance of that family runs (host-side, no launch; additive within ABI 8).  The query IS the launch function,
 * stopped where it would launch, so it also refuses what a family's own run function refuses.  Returns MNAS_ROUTE_* or
 * -MNAS_EINVAL; out (or NULL): int[8], the template arguments followed by the plan values that pick a code path, zeros beyond:
 *   MNAS_ROUTE_PWS              {NT, KSW, NW, GATE}
 *   MNAS_ROUTE_PWF, _PWD        {NT, PT, WRES (weight block resident), K chunks}
 *   MNAS_ROUTE_PWX              {TPW, KS, NW}
 *   MNAS_ROUTE_DIMG             {PXW, CG bound of the instantiation, images per pass, K chunks}
 *   MNAS_ROUTE_C3R              {NT, KSW, PTW, KQ, cout slices (grid.y)}
 *   MNAS_ROUTE_C3X              {TPW, KS}
 *   MNAS_ROUTE_IGEMM            as mnas_conv_gemm_route (refusals of a single k_igemm instance still come from the launch) */
int mnas_conv_gemm_instance(const MnasConvGemm* a, int* out);

/* ---- input gradient of the stride-2 dense 3x3 convs as a transposed convolution (csrc/mnas_tconv.hip): one GEMM per 2x2
 * output block over the four dy pixels it depends on; no per-element gather.  dy: bf16 (N,Ho,Wo,Co), MATERIALISED
 * (mnas_dy_materialize); w: mnas_pack_weights(MNAS_PACK_TCONV, Co, Ci, 3, 3); out: bf16 (N,2Ho,2Wo,Ci); optional fused
 * BatchNorm-backward reduce as in mnas_conv_gemm mode 1 (stats: float[2][Ci][nparts]).  Supported: the conv's input plane is
 * exactly 2Ho x 2Wo, 4*Co <= 256, 4*Ci <= 96 (mnas_tconv_supported); otherwise use mnas_conv_gemm(mode 1). */
typedef struct MnasTconvDgrad {
    int32_t N, Ho, Wo, Co, Ci, nparts;
    const void* dy;
    const void* w;
    void* out;
    float* stats;
    const void* red_y;
    const float* red_bn;
} MnasTconvDgrad;
int mnas_tconv_dgrad(const MnasTconvDgrad* a, void* stream);
int mnas_tconv_supported(int Ho, int Wo, int Co, int Ci);
int mnas_tconv_parts(int N, int Ho, int Wo, int Co, int Ci);     /* preferred nparts (persistent workgroups) */
/* Which kernel and template instance mnas_tconv_dgrad runs (host-side: the launch function stopped where it would launch).  Returns
 * MNAS_TCONV_* or -MNAS_EINVAL; out (or NULL): int[8] = {TPW, KSM, channel blocks} (k_tcx), {KQ0, KQ1, KQ3, channel slices}
 * (k_tcr), {NT, PT} (k_tconv), zeros beyond. */
#define MNAS_TCONV_TCX   0   /* csrc/mnas_tcx.hip: weight-stationary, the large maps */
#define MNAS_TCONV_TCR   1   /* csrc/mnas_tcx.hip: weight rows register-resident, onto the 7x7 plane */
#define MNAS_TCONV_TCONV 2   /* csrc/mnas_tconv.hip */
int mnas_tconv_dgrad_instance(const MnasTconvDgrad* a, int* out);

/* ---- weight gradient of the same convs: dW[co][tap][ci] = sum_pix dy[pix][co] * act(x)[src(pix,tap)][ci]
 * Replaces ATen conv2d weight-gradient.  x = (N,Hi,Wi,Ci) forward input, dy = (N,Ho,Wo,Co).
 * partial: float[nsplit][Co][K] (K = kh*kw*Ci), one slab per pixel split, fully overwritten;
 * reduce + relayout with mnas_wgrad_finalize. */
typedef struct MnasConvWgrad {
    int32_t N, Hi, Wi, Ci;
    int32_t Ho, Wo, Co;
    int32_t kh, kw, stride, pad;
    int32_t nsplit;
    MnasActIn  x;
    MnasGradIn dy;
    float* partial;
} MnasConvWgrad;
int mnas_conv_wgrad(const MnasConvWgrad* a, void* stream);
/* Number of (cout x k) slabs mnas_conv_wgrad splits dW[Co][taps*Ci] into (the slab shape is chosen per (Co, K)): a launch
 * runs nsplit x slabs workgroups, so callers size nsplit as (workgroup budget) / slabs. */
int mnas_conv_wgrad_slabs(int Co, int Ci, int taps);
/* Slab shape of the k_wgrad_t instance a launch runs (host-side: the launch function stopped where it would launch): 0 or
 * -MNAS_EINVAL; out (or NULL): int[2] = {CT, KT}, 32-cout x 32-k tiles per slab. */
int mnas_conv_wgrad_instance(const MnasConvWgrad* a, int* out);

/* grad[co][ci][kh][kw] (reference layout, fp32) (+)= sum_s partial[s][co][tap*Ci+ci].  Deterministic (fixed summation
 * order, no atomics).  `partial` is scratch: with more than 256 splits the first row of every 128-row chunk is
 * overwritten by the chunk's sum (two-level reduction). */
int mnas_wgrad_finalize(float* partial, int nsplit, int Co, int Ci, int taps,
                        float* grad, int accumulate, void* stream);

/* ---- fused backward of a 1x1 conv: input gradient + weight-gradient partials + (optionally) the BatchNorm-backward
 * reduce of the ConvBlock that produced x, in one sweep over the pixels.  Replaces the pair
 * mnas_conv_gemm(mode 1) + mnas_conv_wgrad for the large-pixel-count layers (autograd mirror of mnasnet.py:48-62).
 * Supported channel pairs: mnas_pw_bwd_supported(Ci, Co) != 0 (the 112^2/56^2/28^2 pointwise convs of MNASNet-1.0).
 * wpartial: float[nparts][Co][Ci], one slab per workgroup, fully overwritten -> mnas_wgrad_finalize(wpartial, nparts,
 * Co, Ci, 1, grad, ...).  red_partial (or NULL): float[2][Ci][nparts] = (sum dz, sum dz*xhat) of (gin, red_y) under
 * red_bn -- the fused BatchNorm-backward reduce of the ConvBlock whose activated output gin is the gradient of (red_y =
 * its raw output; equals x.data when x is that block's virtual activation). */
typedef struct MnasPwBwd {
    int32_t M, Ci, Co, nparts;   /* pixels, conv input / output channels, persistent workgroups (<= 65535) */
    MnasActIn  x;                /* forward input (M,Ci): raw + producer's (scale,shift), or a materialised activation */
    MnasGradIn dy;               /* g, y (M,Co) and coef[5][Co] of this ConvBlock's BatchNorm */
    const void* w;               /* MNAS_PACK_DGRAD weights */
    const void* resid;           /* bf16 (M,Ci) added to gin, or NULL */
    void*  gin;                  /* bf16 (M,Ci) */
    float* wpartial;
    float* red_partial;
    const void*  red_y;
    const float* red_bn;
    /* round 4, "RECOMP" (the EXPAND conv's backward; mnas_pw_bwd_forms bit 1): dy.y == NULL && w_fwd != NULL -- the raw forward
     * output y of dy-on-load is not read but recomputed per tile as bf16(W act(x) + b_fwd) from the staged x tile, bit-identical
     * to what mnas_conv_gemm(mode 0) stored (same MFMA, same k order).  w_fwd: MNAS_PACK_FWD [Co_pad16][Ci_pad32]; Ci <= 32. */
    const void*  w_fwd;
    const float* b_fwd;
    /* round 4: store gin MASKED, dz = gin*[s*x+t>0] under red_bn (the mask its fused reduce computes anyway), for a consumer
     * that would otherwise re-derive it per element and window column (mnas_dw_bwd g_masked).  Out-stage forms with the fused
     * reduce only (mnas_pw_bwd_forms bit 2); MNAS_EINVAL otherwise. */
    int32_t gin_masked;
    /* ABI 5: > 0 = "segment mode": workgroup b owns the contiguous pixels [b*seg_px, (b+1)*seg_px) (nparts*seg_px >= M >
     * (nparts-1)*seg_px) instead of striding over the tiles of the whole tensor, so that wpartial[b] is the weight-gradient sum
     * over a KNOWN pixel range -- with seg_px dividing H*W, a fraction of one image: what mnas_se_proj_finalize needs. */
    int32_t seg_px;
} MnasPwBwd;
int mnas_pw_bwd(const MnasPwBwd* a, void* stream);
int mnas_pw_bwd_supported(int Ci, int Co);
/* ABI 5: pixels per tile (64 / 128) and channel slices of the launch for a supported channel pair (-1 otherwise): segment mode
 * wastes ceil(seg_px / tile) * tile - seg_px pixel slots per workgroup, a caller picks seg_px with that in view. */
int mnas_pw_bwd_tile_pixels(int Ci, int Co);
int mnas_pw_bwd_slices(int Ci, int Co);
int mnas_pw_bwd_forms(int Ci, int Co);      /* bit 1: RECOMP available for this channel pair, bit 2: out-stage form (gin_masked) */
/* The k_pw_bwd instance a launch runs (host-side: the launch function stopped where it would launch): 0 or -MNAS_EINVAL; out (or
 * NULL): int[8] = {NTO, NTI per slice, PT, channel slices, OS (out-stage form), FORM (2 = RECOMP)}, zeros beyond. */
int mnas_pw_bwd_instance(const MnasPwBwd* a, int* out);

/* ---- depthwise kxk (k in {3,5}, stride 1, pad k/2), LDS-tiled direct conv on the vector ALU ----------
 * Replaces ATen conv2d fwd/bwd for ConvBlock's groups==C convs (mnasnet.py:122-125, 76-81). */
typedef struct MnasDwFwd {
    int32_t N, H, W, C, k;
    int32_t nparts;          /* upper bound on workgroups; must be >= C/64 (channel blocks) */
    MnasActIn in;
    const float* w;          /* fp32 [k*k][C] (tap-major) */
    const float* bias;       /* [C] or NULL */
    void*  out;              /* bf16 (N,Ho,Wo,C) raw output */
    float* stats;            /* float[2][C][rows] or NULL, rows = mnas_dw_rows(N,H,W,C,k,nparts,0) (stride 2: which = 4) */
    /* ABI 6: 0 / 1 = stride 1 (the LDS row-ring sweeps); 2 = the depthwise conv of SepConv(reduce=True) (mnasnet.py:73-81):
     * Ho = (H + 2*(k/2) - k)/2 + 1, plain direct kernels (csrc/mnas_dw2.hip). */
    int32_t stride, reserved;
} MnasDwFwd;
int mnas_dw_fwd(const MnasDwFwd* a, void* stream);
/* Number of partial rows/columns a depthwise launch writes for this shape and nparts (host-side, no launch).
 * which = 0: forward statistics float[2][C][rows];
 * which = 1: both tables of a phase-0 (fused) backward launch: wpartial float[rows][k*k][C], reduce float[2][C][rows];
 * which = 2: the fused-reduce table of a phase-1 (input-gradient-only) launch;
 * which = 3: wpartial of a phase-2 (weight-gradient-only) launch.  Returns < 0 for unsupported shapes.
 * which = 4 / 7: the same as 0 / 3 for the STRIDE-2 kernels (MnasDwFwd.stride / MnasDwBwd.stride == 2). */
/* Diagnostics: geometry picked for a launch form (`which` as in mnas_dw_rows).  out[7] = {channel pairs per workgroup,
 * 4-column strips per workgroup, threads, strips per image row, channel blocks, LDS bytes, rows per DMA group}. */
int mnas_dw_geometry(int N, int H, int W, int C, int k, int which, int* out);
int mnas_dw_rows(int N, int H, int W, int C, int k, int nparts, int which);

typedef struct MnasDwBwd {
    int32_t N, H, W, C, k;
    int32_t nparts;
    MnasActIn  x;            /* forward input (act-on-load) */
    MnasGradIn dy;           /* gradient of the forward output (dy-on-load) */
    const float* w;          /* fp32 [k*k][C] */
    void*  gin;              /* bf16 (N,H,W,C): dL/d act(x) */
    float* wpartial;         /* float[rows1][k*k][C], rows1 = mnas_dw_rows(...,1), fully overwritten */
    /* optional fused BatchNorm-backward reduction for the producer of x (x.data = its raw output, red_bn = its
     * bnbuf): red_partial receives float[2][C][r] (sum dz, sum dz*xhat) of (gin, x.data), r = mnas_dw_rows(...,1) for
     * phase 0 and mnas_dw_rows(...,2) for phase 1; wpartial rows: which = 1 (phase 0) / 3 (phase 2) */
    const float* red_bn;
    float* red_partial;
    int32_t phase;           /* 0: one fused sweep (input gradient + weight gradient + reduce); 1: input gradient (+reduce)
                                only; 2: weight gradient only (lets the caller put the two on different streams) */
    int32_t stride;          /* ABI 6: 0 / 1 = stride 1; 2 = SepConv(reduce=True)'s depthwise conv (N,H,W = the conv's INPUT dims): only the
                                two-launch form -- phase 1 (input gradient, no fused reduce, no g_masked), phase 2 (weight gradient,
                                wpartial float[mnas_dw_rows(...,7)][k*k][C]) */
    /* round 4: dy.g already holds dz = g*[s*y+t>0] (written by mnas_pw_bwd with gin_masked): dy-on-read skips the mask.
     * Phase 0 with the fused reduce only; results are bit-identical to the plain form on the unmasked g. */
    int32_t g_masked, reserved;
} MnasDwBwd;
int mnas_dw_bwd(const MnasDwBwd* a, void* stream);
/* grad[c][0][kh][kw] (+)= sum_{p<nparts} wpartial[p][tap][c]   (pass nparts = rows1); wpartial is scratch like above */
int mnas_dw_wgrad_finalize(float* wpartial, int nparts, int C, int k, float* grad, int accumulate,
                           void* stream);

/* ---- stem: dense 3x3 stride 2 pad 1 on the fp32 NCHW network input (mnasnet.py:179) ------------------ */
typedef struct MnasStemFwd {
    int32_t N, H, W, Ho, Wo, Co;      /* Ci == 3 */
    int32_t nparts;
    const float* x;          /* fp32 NCHW (N,3,H,W) */
    const void*  w;          /* packed bf16 [Co_pad16][32]: mnas_pack_weights(MNAS_PACK_FWD, Co, 27, 1, 1) of
                                the reference [Co][3][3][3] tensor viewed as [Co][27] (k = ci*9+kh*3+kw) */
    const float* bias;
    void*  out;              /* bf16 (N,Ho,Wo,Co) */
    float* stats;            /* float[2][Co][nparts] */
    /* optional fused input pipeline (the normalisation the reference's dataset applies on the CPU: datasets.py:474-516
     * transforms.Normalize with the mean / std of classifiers.py:91-92): the conv reads in_affine[0][c] * x + in_affine[1][c];
     * in_u8 != 0: x is a uint8 NCHW image (a quarter of the PCIe / HBM bytes).  The two fields are independent: in_u8 without
     * in_affine reads the byte values 0..255 themselves.  The staged value is bf16(fmaf(x, scale, shift)), and the zero padding
     * pads the TRANSFORMED image.  Band-kernel shapes only (Co == 32, W % 4 == 0; the weight gradient also needs Wo % 8 == 0):
     * on any other shape a launch with in_affine or in_u8 returns MNAS_EINVAL and writes nothing. */
    const float* in_affine;  /* float[2][3] (scale, shift per input plane) or NULL */
    int32_t in_u8, reserved;
} MnasStemFwd;
int mnas_stem_fwd(const MnasStemFwd* a, void* stream);
typedef struct MnasStemWgrad {
    int32_t N, H, W, Ho, Wo, Co;
    int32_t nparts;
    const float* x;
    MnasGradIn dy;
    float* partial;          /* float[nparts][Co][27], fully overwritten */
    const float* in_affine;  /* as in MnasStemFwd: the weight gradient must see the same transformed input */
    int32_t in_u8, reserved;
} MnasStemWgrad;
int mnas_stem_wgrad(const MnasStemWgrad* a, void* stream);
/* Preferred nparts (persistent workgroups) for the stem launches: which = 0 forward, 1 weight gradient; -1 = caller's choice
 * (host-side, no launch).  Co == 32, W % 4 == 0 (and Wo % 8 == 0 for the weight gradient) run as band kernels
 * (csrc/mnas_stem.hip: input rows staged once per band in LDS); other shapes use the im2col staging of the GEMM kernels. */
int mnas_stem_parts(int which, int N, int H, int W, int Co);
/* Input gradient of the stem conv = dL/d image, fp32 NCHW (N,3,H,W): ATen conv2d input gradient of ConvBlock(3, Co, 3, stride 2,
 * pad 1) with dy-on-load; w = the reference fp32 [Co][3][3][3] weight (rounded to bf16 inside, like the forward's packed copy);
 * in_affine as in MnasStemFwd (the result is the gradient w.r.t. the RAW float image: scaled by in_affine[0][c]) or NULL.
 * Not on the training path (train.py:427) -- a plain gather kernel for autograd completeness (saliency, adversarial inputs). */
int mnas_stem_dgrad(const MnasGradIn* dy, const float* w, int N, int H, int W, int Ho, int Wo, int Co, const float* in_affine,
                    float* dx, void* stream);

/* ---- BatchNorm2d bookkeeping (replaces ATen native_batch_norm / native_batch_norm_backward) ---------- */
/* partial: float[2][C][nparts] (sum, sumsq over `count` elements per channel).
 * training=1: batch stats -> bnbuf rows 0,1,5,6; running_mean/var momentum update (unbiased var),
 *             num_batches_tracked (int64 device scalar, may be NULL) += 1.
 * training=0: bnbuf rows 0,1 from the running stats; nothing else is touched (partial may be NULL). */
int mnas_bn_fwd_finalize(const float* partial, int nparts, int C, double count,
                         const float* gamma, const float* beta,
                         float* running_mean, float* running_var, int64_t* num_batches_tracked,
                         float momentum, float eps, int training, float* bnbuf, void* stream);
/* partial[0][c][p] = sum dz, partial[1][c][p] = sum dz*xhat over the rows of workgroup p, where
 * dz = g*[s*y+t>0], xhat = (y-mean)*invstd.  g,y: bf16 [rows][C]. */
int mnas_bn_bwd_reduce(const void* g, const void* y, const float* bnbuf, int64_t rows, int C,
                       int nparts, float* partial, void* stream);
/* out[rows][C] (bf16) = dy-on-load of (g, y, coef), materialised once.  mnas_conv_gemm(mode 1) and mnas_conv_wgrad accept the
 * result as a PLAIN gradient: grad.g = out, grad.y = grad.coef = NULL (no transform on load).  Used for the dense 3x3 convs,
 * whose kernels gather every dy element 2.25-10 times. */
int mnas_dy_materialize(const MnasGradIn* d, int64_t rows, int C, void* out_bf16, void* stream);
/* dgamma (+)= sum dz*xhat ; dbeta (+)= sum dz ; bnbuf rows 2..4 = c1,c2,c3 */
int mnas_bn_bwd_finalize(const float* partial, int nparts, int C, double count,
                         float* bnbuf, float* dgamma, float* dbeta, int accumulate, void* stream);

/* ---- one launch for the bookkeeping between two dependent backward kernels: mnas_bn_bwd_finalize (accumulate = 1) of the next
 * layer + up to two weight-gradient reductions (mnas_wgrad_finalize / mnas_dw_wgrad_finalize semantics, accumulate = 1).
 * level: 0 = none, 1 = whole reduction in one level (nsplit <= 256), 2 = first level of two (chunks of 128 rows folded into
 * each chunk's first row, in place), 3 = second level of the same table (call it in a LATER launch than its level 2).
 * bn_C == 0: no BatchNorm part. */
typedef struct MnasPostWgrad {
    float* partial;          /* float[nsplit][Co][taps*Ci]   (dw: float[nsplit][taps][Co]) */
    float* grad;             /* reference layout, accumulated into */
    int32_t nsplit, Co, Ci, taps, dw, level;
} MnasPostWgrad;
typedef struct MnasBwdPost {
    const float* bn_partial; /* float[2][C][nparts] */
    float* bnbuf;
    float* dgamma;
    float* dbeta;
    double count;
    int32_t bn_nparts, bn_C;
    MnasPostWgrad w1, w2;
} MnasBwdPost;
int mnas_bwd_post(const MnasBwdPost* p, void* stream);

/* ---- frozen BatchNorm statistics: training with the RUNNING buffers (model.train(); features.eval(): the fine-tuning recipe).
 * y is normalised with (running_mean, running_var), which are constants of the step, so
 *     dy = s*dz             bnbuf rows 2..4 = (s, +0, +0): the conv backward kernels run unchanged
 *     dgamma += S2, dbeta += S1, dbias += s*S1      with S1 = sum dz, S2 = sum dz*(y*invstd - running_mean*invstd)
 * (conv.bias has a gradient here: batch statistics cancel the bias, running statistics do not).  S1 / S2 are the partial tables the
 * fused reduces and mnas_bn_bwd_reduce already produce from rows 0, 1, 5, 6.
 *
 * mnas_bn_frozen_tables: the whole coefficient block of `n` ConvBlock applications in ONE launch (`descs`: DEVICE array); they
 * depend on parameters and buffers only, not on the batch.  Per channel, fp32, in the arithmetic of mnas_bn_fwd_finalize(training=0):
 *     invstd = 1/sqrtf(running_var + eps), s = gamma*invstd, t = beta - running_mean*s
 *     rows 0..6 = s, t, s, +0, +0, running_mean, invstd     (row 7 and the running buffers are not written) */
typedef struct MnasBnFrozenDesc {
    const float* gamma;
    const float* beta;
    const float* running_mean;
    const float* running_var;
    float*  bnbuf;           /* float[8][C] */
    int32_t C;
    float   eps;
} MnasBnFrozenDesc;
int mnas_bn_frozen_tables(const MnasBnFrozenDesc* descs, int n, void* stream);
/* mnas_bn_bwd_finalize under frozen statistics: dgamma (+)= S2, dbeta (+)= S1, dbias (+)= s*S1 (formed in double from the double
 * partial sums, rounded once); bnbuf (row 0 = s) is only read.  Any of the three gradient pointers may be NULL. */
int mnas_bn_bwd_finalize_frozen(const float* partial, int nparts, int C, const float* bnbuf, float* dgamma, float* dbeta,
                                float* dbias, int accumulate, void* stream);
/* mnas_bwd_post under frozen statistics: the fields of MnasBwdPost (count is not used) + dbias.  The BatchNorm blocks do the three
 * accumulations above and leave bnbuf alone; the weight-gradient tasks are those of mnas_bwd_post. */
typedef struct MnasBwdPostFrozen {
    const float* bn_partial; /* float[2][C][nparts] */
    const float* bnbuf;
    float* dgamma;
    float* dbeta;
    double count;
    int32_t bn_nparts, bn_C;
    MnasPostWgrad w1, w2;
    float* dbias;
} MnasBwdPostFrozen;
int mnas_bwd_post_frozen(const MnasBwdPostFrozen* p, void* stream);

/* ---- element-wise glue ------------------------------------------------------------------------------ */
/* out = act(a) + act(b)   (b.data may be NULL -> out = act(a)); rows x C bf16.  The MBConv_block residual
 * (mnasnet.py:133).  If out_nchw_f32 != NULL the result is ALSO/INSTEAD written as fp32 NCHW (N,C,H,W)
 * with rows = N*HW (the features output handed to AdaptiveAvgPool2d, classifiers.py:109). */
int mnas_add_act(const MnasActIn* a, const MnasActIn* b, int64_t rows, int C, void* out_bf16,
                 float* out_nchw_f32, int HW, void* stream);
/* Global average pool fused with the last BatchNorm+ReLU: out[n][c] (fp32) = mean over the HW pixels of act(a)[n][.][c]
 * (classifiers.py:49,109: AdaptiveAvgPool2d(1) on the features output, which is then never materialised), and its backward:
 * g[n][hw][c] (bf16 NHWC) = gpool[n][c] / HW. */
int mnas_pool_act(const MnasActIn* a, int N, int HW, int C, float* out, void* stream);
int mnas_pool_bwd(const float* gpool, int N, int HW, int C, void* g_bf16, void* stream);
/* bf16 NHWC <- fp32 NCHW  (incoming gradient of the features output) */
int mnas_nchw_f32_to_nhwc_bf16(const float* src, void* dst, int N, int C, int HW, void* stream);

/* ---- classifier head + loss (csrc/mnas_head.hip) -------------------------------------------------------
 * Replaces, for FineTuneModelPool.classifier (classifiers.py:56-89: nn.Sequential of Dropout / Linear / ReLU) and
 * nn.CrossEntropyLoss (train.py:277), ATen's dropout / addmm / relu / log_softmax / nll_loss forward and backward.
 * One MnasHeadLinear = the Dropout in front of a Linear + the Linear + the optional ReLU behind it, all fp32:
 *   fwd    y[N][O]  = act( (x * keep/(1-p)) W^T + b )                 act = relu if `relu`
 *   bwd_w  dw[O][I] (+)= dz^T (x * keep/(1-p)),  db[O] (+)= sum_n dz   (+= if `accumulate`)
 *   bwd_x  dx[N][I] = (dz W) * keep/(1-p) * [relu_mask > 0]            relu_mask = x when the layer in FRONT ends in a
 *                                                                      ReLU (then dx is that layer's dz), else NULL
 * keep(seed, n*I+i) is a counter-based hash (splitmix64), never stored: the three calls of one layer and step take the same
 * (drop_p, seed); drop_p == 0 (or eval mode) -> no dropout.  mnas_head_dropout_mask writes the keep bytes of a layer
 * (tests).  Unused pointers may be NULL. */
typedef struct MnasHeadLinear {
    int32_t N, I, O;
    int32_t relu;            /* fwd: ReLU after the Linear */
    int32_t accumulate;      /* bwd_w */
    float   drop_p;          /* dropout probability on the layer's input, 0 <= p < 1 */
    uint64_t seed;
    const void* x;           /* [N][I] layer input (before dropout) */
    const void* w;           /* [O][I] */
    const void* b;           /* [O] or NULL */
    void*       y;           /* [N][O] */
    const void* dz;          /* [N][O] gradient of the Linear's output (after the ReLU mask) */
    void*       dw;          /* [O][I] */
    void*       db;          /* [O] or NULL */
    void*       dx;          /* [N][I] */
    const void* relu_mask;   /* [N][I] or NULL */
} MnasHeadLinear;
int mnas_head_linear_fwd(const MnasHeadLinear* a, void* stream);
int mnas_head_linear_bwd_w(const MnasHeadLinear* a, void* stream);
int mnas_head_linear_bwd_x(const MnasHeadLinear* a, void* stream);
int mnas_head_dropout_mask(void* out_u8, int64_t n, float p, uint64_t seed, void* stream);
/* nn.CrossEntropyLoss(reduction='mean', ignore_index): logits fp32 [N][C], target int64 [N].
 * loss_rows[N] (scratch), *loss = mean over the non-ignored rows, dlogits[N][C] = dloss/dlogits (NULL: forward only).
 * A target outside [0, C) that is not ignore_index sets *bad_flag (int32, device) and poisons the loss with NaN (ATen
 * asserts on the device). */
int mnas_head_cross_entropy(const void* logits, const void* target, int N, int C, int64_t ignore_index,
                            void* loss_rows, void* loss, void* dlogits, void* bad_flag, void* stream);

/* ---- device-resident loss / top-k accuracy meters (csrc/mnas_head.hip) ------------------------------------
 * The lines that follow the step in the reference's loops -- losses.update(loss.item(), input.size(0)) (train.py:447, :575),
 * accuracy(sm(out), target, topk=(1, 5)) and the two acc meters' update(prec.item(), n) (train.py:465-468, :589-592), with
 * AverageMeter and accuracy() as defined at train.py:657-700 -- cost three host reads per batch there.  Here one MnasMeters
 * block in DEVICE memory is moved by the kernels of the step and copied to the host when the caller wants to print.
 * Every field is 8 bytes wide: the first MNAS_METERS_NUM_I64 are int64, the last MNAS_METERS_NUM_F64 double, so the block
 * is two tensors for an all-reduce.
 *
 * Correctness rule: row n is correct@k iff rank_n < k, where, with t = target[n] and z = logits,
 *     rank_n = #{j : z[n][j] > z[n][t]} + #{j < t : z[n][j] == z[n][t]}          (ties go to the lower index).
 * Rows whose target is ignore_index, outside [0, C), or whose target logit is not finite are wrong for every k and still count
 * in `samples` (the reference divides by the batch size).  k > C is clamped to C.  The counts are integers summed in a fixed
 * order: exact and identical from run to run.  The rule is evaluated on the LOGITS; the reference evaluates it on
 * softmax(out) in fp32, which is monotone up to rounding.
 *
 * loss_sum += (double)loss * (double)N, one thread, step order, product and sum rounded separately: bit for bit the Python-float
 * AverageMeter.sum fed with loss.item().  AverageMeter.avg = loss_sum / loss_samples, .val = last_loss; accuracy in percent =
 * correct[i] * 100 / samples (avg) and last_correct[i] * 100 / last_n (val). */
#define MNAS_METERS_MAX_K   4
#define MNAS_METERS_NUM_I64 14
#define MNAS_METERS_NUM_F64 3
typedef struct MnasMeters {
    /* running */
    int64_t steps;                               /* updates since the block was zeroed */
    int64_t samples;                             /* sum of N over all updates */
    int64_t loss_samples;                        /* sum of N over the updates that carried a loss (AverageMeter.count of the loss) */
    int64_t nonfinite_steps;                     /* updates whose loss was NaN / Inf */
    int64_t correct[MNAS_METERS_MAX_K];          /* rows correct@ks[i] */
    /* last update (AverageMeter.val) */
    int64_t last_n;
    int64_t last_loss_n;                         /* N of the last update that carried a loss */
    int64_t last_correct[MNAS_METERS_MAX_K];
    double  loss_sum;                            /* running: sum of (double)loss_i * N_i */
    double  last_loss;                           /* loss of the last update that carried one */
    double  last_loss_sum;                       /* last_loss * last_loss_n (what an all-reduce sums: val over ranks = sum / n) */
} MnasMeters;
/* Both calls: stream-ordered, no allocation, no host read of device memory, capturable in a hipGraph.  ks: nk (1..4) values of
 * k >= 1 in HOST memory, read at call time; correct[i] belongs to ks[i], so one block is always fed with the same ks.
 * rank_rows: int32 [N] scratch.  Zero the block (hipMemsetAsync) to reset it.
 *   mnas_head_cross_entropy_metrics : mnas_head_cross_entropy plus the update of *meters with its loss, in the same two launches
 *                                     (loss, dlogits and bad_flag are bit-identical to it)
 *   mnas_head_metrics               : logits from anywhere; loss = device fp32 scalar or NULL (then only steps, samples and the
 *                                     accuracy fields move).  No ignore_index: any target outside [0, C) is a wrong row. */
int mnas_head_cross_entropy_metrics(const void* logits, const void* target, int N, int C, int64_t ignore_index,
                                    void* loss_rows, void* loss, void* dlogits, void* bad_flag, const int* ks, int nk,
                                    void* rank_rows, MnasMeters* meters, void* stream);
int mnas_head_metrics(const void* logits, const void* target, int N, int C, const int* ks, int nk, const void* loss,
                      void* rank_rows, MnasMeters* meters, void* stream);

/* ---- soft-target cross-entropy (csrc/mnas_head.hip; additive within ABI 8, outside the launch lists): label smoothing and batch
 * mixing (Mixup / CutMix) in the loss of the step.  Every row has two labels a = target_a[n], b = target_b[n] and a weight
 * l = lam[n] on a; its target row is
 *     q = (1 - eps) (l e[a] + (1 - l) e[b]) + eps / C                          eps = label_smoothing in [0, 1]
 * and, with lse = logsumexp(z[n]),
 *     loss_rows[n]  = (1 - eps) (l (lse - z[n][a]) + (1 - l) (lse - z[n][b])) + eps (lse - mean_c z[n][c])
 *     *loss         = sum(loss_rows) / count,   dlogits[n][c] = (softmax(z[n])[c] - q[c]) / count      (NULL: forward only)
 * which is F.cross_entropy(z, a, label_smoothing=eps) and ..(z, b, ..) combined per row as l CE(a) + (1 - l) CE(b).
 * eps == 0: there is no smoothing term -- a -inf logit at a class that is no label (a masked class) leaves the row's loss finite,
 * as in mnas_head_cross_entropy; with eps > 0 such a row's loss is +inf (its gradient stays finite).
 * target_b NULL: no mixing (b = a, l = 1; lam is not read).  lam NULL: l = 1 (device fp32 [N] otherwise).
 * A row is ignored when a == ignore_index or, with mixing, b == ignore_index: it contributes 0 and is not counted; count = rows
 * not ignored, 0/0 = NaN.  A label outside [0, C), or an l that is NaN or outside [0, 1], sets *bad_flag (int32, device) and
 * poisons the loss with NaN; such a row indexes no memory.  Two launches, fixed summation order, no float atomics.
 * meters non-NULL (then ks, nk, rank_rows as for mnas_head_cross_entropy_metrics): the same launches move the block; a row is
 * ranked against the label that carries the larger weight, a when l >= 0.5, else b; ignored and refused rows are wrong for every
 * k.  label_smoothing outside [0, 1]: MNAS_EINVAL, no launch. */
int mnas_head_cross_entropy_soft(const void* logits, const void* target_a, const void* target_b, const float* lam,
                                 float label_smoothing, int N, int C, int64_t ignore_index, void* loss_rows, void* loss,
                                 void* dlogits, void* bad_flag, const int* ks, int nk, void* rank_rows, MnasMeters* meters,
                                 void* stream);

/* ---- distillation cross-entropy (csrc/mnas_head.hip; additive within ABI 8, outside the launch lists): class weights and a dense
 * teacher distribution (knowledge distillation, Hinton et al. 2015) on top of the soft-target loss above.  Labels a, b, weight l,
 * eps and the target row q are those of mnas_head_cross_entropy_soft; class_weight w (device fp32 [C], finite and >= 0; NULL: every
 * weight 1) and teacher_logits t (device fp32 [N][C]; NULL: no distillation term) are optional.  With p = softmax(z[n]):
 *     hard_n = -sum_c w[c] q[c] log p[c]
 *            = (1 - eps) (l w[a] (lse - z[a]) + (1 - l) w[b] (lse - z[b])) + eps (Wm lse - sum_c w[c] z[c] / C),   Wm = mean_c w[c]
 *     s_n    = l w[a] + (1 - l) w[b],   D = sum of s_n over the rows not ignored,   hard = sum_n hard_n / D
 * which for a plain class vector is F.cross_entropy(z, y, weight=w, label_smoothing=eps) and with w == 1 the value of
 * mnas_head_cross_entropy_soft; and with pT = softmax(t[n] / T), pS = softmax(z[n] / T), T = temperature > 0:
 *     kd_n = sum_c pT[c] (log pT[c] - log pS[c]),   kd = T^2 sum_n kd_n / N       (all N rows, ignored ones included)
 * which is T^2 F.kl_div(log_softmax(z / T), softmax(t / T), reduction='batchmean').  *loss = (1 - alpha) hard + alpha kd;
 *     dlogits[n][c] = (1 - alpha) (p[c] S_n - w[c] q[c]) / D + alpha T (pS[c] - pT[c]) / N,   S_n = sum_c w[c] q[c]   (NULL: forward only)
 * loss_rows: device fp32 [2 N], hard_n in the first half and kd_n in the second; loss_parts: device fp32 [2] = (hard, kd), or NULL.
 * Rules:
 *   - a class with pT[c] == 0 (a -inf teacher logit: a masked class) adds exactly 0 to kd_n, never 0 * inf;
 *   - a -inf student logit where pT[c] > 0 makes the row's kd_n +inf; its gradient stays finite;
 *   - alpha == 1: the hard term is left out of *loss and of dlogits (no 0 * inf; the eps == 0 precedent); loss_rows' first half and
 *     loss_parts[0] are still written;
 *   - alpha == 0 or t == NULL: the distillation term is left out, t is not read, *loss = hard (whatever alpha is when t == NULL),
 *     kd_n and loss_parts[1] are 0;
 *   - NaN logits give NaN results;
 *   - an ignored row (a or, with mixing, b == ignore_index) adds 0 to the hard term, to D and to the hard gradient; it takes part
 *     in the distillation term like any other row;
 *   - a refused row -- a label outside [0, C), an l that is NaN or outside [0, 1] -- sets *bad_flag and poisons *loss and both
 *     parts with NaN; its dlogits row is all zeros; it indexes no memory (neither z nor w);
 *   - D == 0: hard = 0/0 = NaN (every row ignored, or every counted weight 0); the hard gradient is then 0;
 *   - eps == 0: no smoothing term, as in mnas_head_cross_entropy_soft;
 *   - temperature not > 0, alpha or label_smoothing outside [0, 1] (NaN included), a NULL logits / target_a / loss_rows / loss /
 *     bad_flag, N or C < 1: MNAS_EINVAL, no launch.  The class weights are NOT checked on the device (the Python layer refuses
 *     negative and non-finite ones).
 * Two launches (one 256-lane workgroup per row, one workgroup for the two means and the meters), fixed summation order, no float
 * atomics: bit-identical from run to run; no allocation and no host read: capturable.  Any N >= 1, C >= 1.  meters as for
 * mnas_head_cross_entropy_soft (a row is ranked against its heavier label); the loss meter receives *loss.  The kernel's operation
 * order is written out above k_head_ce_kd. */
int mnas_head_cross_entropy_kd(const void* logits, const void* target_a, const void* target_b, const float* lam,
                               float label_smoothing, const float* class_weight, const void* teacher_logits, float temperature,
                               float alpha, int N, int C, int64_t ignore_index, void* loss_rows, void* loss, void* loss_parts,
                               void* dlogits, void* bad_flag, const int* ks, int nk, void* rank_rows, MnasMeters* meters,
                               void* stream);

/* ---- the multi-label branch of the step (csrc/mnas_mlabel.hip): MultiClassBCELoss (src/models/multi_class_loss.py), HardDice
 * and the per-sample macro-F1 of batch_metrics (src/utils/metric.py) as train.py:274-279, 453-463, 577-587 use them, with the three
 * AverageMeters of that branch in one MnasMultiLabelMeters block in device memory.  logits z, target t, weights w: fp32 [N][C].
 *
 * Arithmetic rule:
 *   loss element  e = max(z,0) - z*t + log1p(exp(-|z|)), times w when weights are given;  b = sum(e) / (N*C)  (row sums in fp32 in
 *                 a fixed order, the N row sums added in double, one rounding to fp32).
 *   focal         pt = exp(-b), loss = balance * (1-pt)^gamma * b -- applied to the MEAN b, not per element, as the reference does
 *                 (evaluated in double by one thread, rounded once); without focal loss = b.
 *   gradient      dlogits = s * w * (sigma(z) - t) / (N*C);  s = 1 without focal, else
 *                 s = balance * (1-pt)^(gamma-1) * ((1-pt) + gamma*pt*b)  (gamma >= 1);  sigma(z) = 1/(1+exp(-z)) for z >= 0 and
 *                 exp(z)/(1+exp(z)) for z < 0.
 *   F1            class c of a row is predicted iff z >= 0 and true iff t == 1 (batch_metrics: sigmoid < 0.5 -> 0, then > 0 -> 1, so
 *                 0.5 counts as positive).  With tp/fp/fn/tn over the row's C classes: F1_1 = 2tp/(2tp+fp+fn) if tp+fp+fn > 0,
 *                 F1_0 = 2tn/(2tn+fp+fn) if tn+fp+fn > 0; the row's F1 is the mean of those that exist (scikit-learn's macro average
 *                 over the labels present), in double.  Batch value = (sum of the rows' F1, in row order, by one thread, one
 *                 rounded double sum per row) / N: the reference's sum(list) / len(list).
 *   HardDice      predicted iff z > threshold_logit (strict; 0 for the threshold 0.5); I = #(predicted and t == 1),
 *                 U = #predicted + #(t == 1) (minus I with deduct_intersection); value = clamp(1 + log(2I/U), 0, 1) in fp32 and 0
 *                 when I == 0.
 *   A NaN logit is predicted negative under both rules (comparisons are false).  Targets other than exactly 1 are negatives for the
 *   metrics; any t enters the loss (soft labels).
 *   Deviation from the reference: both prediction rules are evaluated on the LOGIT, not on an fp32 sigmoid.  They differ only for
 *   0 < |z| < 2^-23, where the fp32 sigmoid rounds to exactly 0.5 (sigmoid(1e-9) is not > 0.5; sigmoid(-1e-9) == 0.5 counts as
 *   positive for F1).  At z == 0 both agree with the reference: F1 positive, Dice negative.
 *
 * The block follows MnasMeters: every field 8 bytes, all int64 first, then all double (an all-reduce is two tensors).  Each meter is
 * an AverageMeter: sum += val * n as one rounded double product and one rounded double sum per update, no fused multiply-add. */
#define MNAS_MLABEL_NUM_I64 16
#define MNAS_MLABEL_NUM_F64 9
typedef struct MnasMultiLabelMeters {
    /* running */
    int64_t steps;                               /* updates since the block was zeroed */
    int64_t samples;                             /* sum of N over all updates */
    int64_t nonfinite_steps;                     /* updates whose loss was NaN / Inf */
    int64_t loss_n;                              /* AverageMeter.count of the loss meter (sum of n_loss over updates with a loss) */
    int64_t dice_n;                              /* ... of the HardDice meter */
    int64_t f1_n;                                /* ... of the F1 meter */
    int64_t tp;                                  /* Dice rule: predicted and true */
    int64_t fp;                                  /* Dice rule: predicted, not true */
    int64_t fn;                                  /* Dice rule: true, not predicted */
    /* last update */
    int64_t last_n;
    int64_t last_loss_n;                         /* n_loss of the last update that carried a loss */
    int64_t last_dice_n;
    int64_t last_f1_n;
    int64_t last_tp;
    int64_t last_fp;
    int64_t last_fn;
    double  loss_sum;                            /* running: sum of val * n */
    double  dice_sum;
    double  f1_sum;
    double  last_loss;                           /* AverageMeter.val */
    double  last_dice;
    double  last_f1;
    double  last_loss_sum;                       /* val * n of the last update (what an all-reduce sums: val over ranks = sum / n) */
    double  last_dice_sum;
    double  last_f1_sum;
} MnasMultiLabelMeters;
/* All calls: stream-ordered, no allocation, no host read of device memory, no float atomics (results do not depend on the run),
 * capturable in a hipGraph.  scratch: mnas_mlabel_scratch_bytes(N) bytes of device memory, 16-byte aligned, owned by the call until
 * it has run.  Its layout after a call (24 N + 16 bytes; the tests read the row sums and s from it): double f1_rows[N] at byte 0,
 * float loss_rows[N] (the sum of each row's loss elements, mnas_mlabel_bce only) at byte 8 N, int cI[N], cP[N], cT[N] (the Dice
 * rule's counts per row) at bytes 12 N, 16 N and 20 N, and one float `scale` (focal: the gradient's factor s) at byte 24 N.
 * Zero the block (hipMemsetAsync) to reset it.  The meters' Dice threshold is 0.5 without deduct_intersection
 * (train.py:279).  n_loss / n_dice / n_f1: the weights of the three meters (train.py:447-463: N, N and the number of classes).
 *   mnas_mlabel_bce       : *loss (device fp32) and dlogits (NULL: forward only); weights NULL: none; focal != 0: the focal
 *                           transform with focus_param (>= 1) and balance_param.  meters != NULL: the same launches also update the
 *                           block (loss and dlogits are bit-identical either way).  Two launches, three with focal and dlogits.
 *   mnas_mlabel_metrics   : logits from anywhere; loss = device fp32 scalar or NULL (then the loss meter does not move).  Two launches.
 *   mnas_mlabel_hard_dice : *out (device fp32) = HardDice of one batch.  Two launches. */
int64_t mnas_mlabel_scratch_bytes(int N);
int mnas_mlabel_bce(const void* logits, const void* target, const void* weights, int N, int C, int focal, float focus_param,
                    float balance_param, void* scratch, void* loss, void* dlogits, MnasMultiLabelMeters* meters, int64_t n_loss,
                    int64_t n_dice, int64_t n_f1, void* stream);
int mnas_mlabel_metrics(const void* logits, const void* target, int N, int C, const void* loss, void* scratch,
                        MnasMultiLabelMeters* meters, int64_t n_loss, int64_t n_dice, int64_t n_f1, void* stream);
int mnas_mlabel_hard_dice(const void* logits, const void* target, int N, int C, float threshold_logit, int deduct_intersection,
                          void* scratch, void* out, void* stream);

/* ---- multi-label loss (csrc/mnas_mlabel.hip; build-defined -- the reference has plain BCE only): per-element asymmetric focal
 * loss (Ridnik et al., "Asymmetric Loss for Multi-Label Classification"; gamma+ = gamma- = gamma, m = 0 is the sigmoid focal loss
 * without its alpha term), pos_weight, binary label smoothing and mixed label rows, in mnas_mlabel_bce's two launches.
 * logits z, labels Y, weights w: fp32 [N][C] (w NULL: 1); pos_weight p: fp32 [C] (NULL: 1); partner: int64 [N] and lam: fp32 [N],
 * both or neither.
 *
 * Arithmetic rule (fp32; sp(x) = max(x,0) + log1p(exp(-|x|)); sigma = the piecewise sigmoid above, 1 - sigma its other branch --
 * exp(-|z|)/(1+exp(-|z|)) for z >= 0, 1/(1+exp(-|z|)) for z < 0 -- never a subtraction):
 *   mixed rows   y = fma(lam_n, Y[n][c], (1 - lam_n) * Y[partner_n][c])            (no partner: y = Y[n][c])
 *   smoothing    t = fma(1 - eps, y, eps/2)                                         (eps = 0: t = y, no operation)
 *   L+ = sp(-z)  F+ = exp(-(gamma+ * sp(z)))                                        (gamma+ = 0: F+ = 1, no exp)
 *   sigma_m = sigma - m;   m = 0:  F- = exp(-(gamma- * sp(-z))), L- = sp(z)         (log sigma = -sp(-z): no cancellation)
 *                          m > 0, sigma_m > 0:  F- = exp(gamma- * log(sigma_m)), L- = -log1p(-sigma_m)
 *                          m > 0, sigma_m <= 0: L- = 0, F- = 0 (gamma- = 0: 1): the element's negative part and its gradient are 0
 *                          (gamma- = 0: F- = 1, no exp)
 *   e   = fma(1 - t, F- * L-, (p t) * (F+ * L+));   the row sum adds fma(e, w, .)
 *   loss = sum(e w) / D, D = N*C (reduction MNAS_MLABEL_MEAN) or N (MNAS_MLABEL_ROWS: summed over the classes, averaged over the
 *          rows); row sums in fp32 in k_mlabel_row's fixed order, the N row sums added in double, one rounding to fp32
 *   dlogits = (w * fma(1 - t, dneg, (p t) * dpos)) * (float)(1/D)     -- the focusing weights are differentiated:
 *     dpos = -(F+ * fma(gamma+ * sigma, L+, 1 - sigma))                             (gamma+ = 0: -(1 - sigma))
 *     dneg = F- * fma(gamma- * (1 - sigma), sp(z), sigma)                           (m = 0; gamma- = 0: sigma) -- no division by 1 - sigma
 *     dneg = (sigma (1 - sigma)) * fma(gamma- * exp((gamma- - 1) * log(sigma_m)), L-, F- / (1 - sigma_m))    (m > 0, sigma > m strictly)
 *   Powers are expf / logf / log1pf only, never powf.  Each multiply that feeds an add is the fma written above; every other operation
 *   rounds on its own.
 *   With gamma+ = gamma- = 0, m = 0 and no pos_weight the element is mnas_mlabel_bce's own (e = max(z,0) - z*t + log1p(exp(-|z|)),
 *   gradient w (sigma - t) / D) on the mixed, smoothed t; with eps = 0, no partner and MNAS_MLABEL_MEAN besides, the call is
 *   mnas_mlabel_bce(focal = 0) bit for bit: loss, dlogits, scratch and meters block.
 *   Meters: a class of row n is true iff the RAW label (before mixing and smoothing) of the row's dominant image is exactly 1 --
 *   row n when lam_n >= 0.5, row partner_n otherwise; prediction rules, F1, HardDice and the block update as above.
 *   Bad rows: partner_n outside [0, N) or lam_n not in [0, 1] (NaN included).  Such a row reads no partner row (nothing is read
 *   out of bounds); its labels are NaN, so its row loss, the batch loss and its gradient row are NaN (nonfinite_steps counts the
 *   step; an optimizer's skip_nonfinite sees the gradient); the meters count it against its own labels.  Other rows' gradients
 *   do not change.
 *   Refused on the host with MNAS_EINVAL before any launch, nothing written: a NULL logits / labels / cfg / scratch / loss, N or
 *   C < 1, a scratch not 16-byte aligned, partner without lam or lam without partner, gamma+ or gamma- outside {0} u [1, 16],
 *   m outside [0, 0.5], eps outside [0, 1), any of them NaN, an unknown reduction, a non-zero reserved field, a negative meter weight.
 *   Scratch: mnas_mlabel_scratch_bytes(N), the layout above (`scale` is not written).  dlogits NULL: forward only, the same loss
 *   bits; meters NULL or not: the same loss and dlogits bits.  Two launches in every configuration: the gradient is final after
 *   the row launch.  16-byte loads and stores when C % 4 == 0 and logits, labels, weights, pos_weight and dlogits are 16-byte
 *   aligned, scalar ones otherwise. */
#define MNAS_MLABEL_MEAN 0
#define MNAS_MLABEL_ROWS 1
typedef struct MnasMlabelLoss {
    float gamma_pos, gamma_neg, margin, smoothing;
    int reduction;                               /* MNAS_MLABEL_MEAN / MNAS_MLABEL_ROWS */
    int reserved[3];                             /* 0 */
} MnasMlabelLoss;
int mnas_mlabel_loss(const void* logits, const void* labels, const void* partner /* int64[N] or NULL */,
                     const void* lam /* fp32[N], NULL iff partner is NULL */, const void* weights, const void* pos_weight,
                     int N, int C, const MnasMlabelLoss* cfg, void* scratch, void* loss, void* dlogits,
                     MnasMultiLabelMeters* meters, int64_t n_loss, int64_t n_dice, int64_t n_f1, void* stream);

/* ---- squeeze-and-excitation of the SE variant of MBConv_block (BASELINE config 4; build-defined -- the reference has no SE
 * block; csrc/mnas_se.hip, restated in oracle.se_apply).  a = the activated depthwise output (act-on-load of y2), u = the
 * excite logits fp32 [N][C] (mnas_pool_act -> mnas_head_linear_fwd x2 produce them).
 *   mnas_se_scale      : out = act(a) * sigmoid(u)[n][c]            (bf16 (N,HW,C): what the project conv then reads)
 *   mnas_se_bwd_reduce : du[n][c] = (sum_hw gs * act(a)) * s (1 - s), s = sigmoid(u)   (gs = dL/d out, bf16); scratch =
 *                        mnas_se_scratch_bytes(N, HW, C) bytes of partial sums (pixel splits, added in a fixed order)
 *   mnas_se_bwd_apply  : out = gs * sigmoid(u) + dz[n][c] / HW      (dz = dL/d(pooled a) from the MLP backward; out = dL/d act(a));
 *                        optional fused BatchNorm-backward reduce of the ConvBlock whose activated output `out` is the gradient of:
 *                        red_partial float[2][C][mnas_se_bwd_apply_cols(N,HW,C)] from (out, red_y, red_bn), as mnas_bn_bwd_reduce */
int mnas_se_scale(const MnasActIn* a, const float* u, int N, int HW, int C, void* out_bf16, void* stream);
int mnas_se_bwd_reduce(const void* gs, const MnasActIn* a, const float* u, int N, int HW, int C, float* du, float* scratch,
                       void* stream);
int64_t mnas_se_scratch_bytes(int N, int HW, int C);
int mnas_se_bwd_apply(const void* gs, const float* u, const float* dz, int N, int HW, int C, void* out_bf16,
                      const void* red_y, const float* red_bn, float* red_partial, void* stream);
int mnas_se_bwd_apply_cols(int N, int HW, int C);
/* ABI 5 -- the excitation applied ON LOAD instead of through a materialised a*s (csrc/mnas_se.hip):
 *   mnas_se_gate          : gate[n][c] = sigmoid(u[n][c]), fp32 -- the table MnasConvGemm.gate takes.
 *   mnas_se_proj_finalize : after mnas_pw_bwd of the PROJECT conv run in segment mode (MnasPwBwd.seg_px = HW / kseg, nparts =
 *                           N * kseg) on the UNGATED activation act(a): wpartial float[N*kseg][Co][Ci] holds per-image(-fraction)
 *                           sums of dy[pix][o] * act(a)[pix][c].  Writes du[n][c] = (sum_o W[o][c] * P_n[o][c]) * s (1 - s)
 *                           (= what mnas_se_bwd_reduce computes from gs = dy . W, without the pass over gs and a) and the conv's
 *                           weight gradient dW[o][c] (+)= sum_n s[n][c] * P_n[o][c].  W: the conv's fp32 MASTER weight [Co][Ci]
 *                           (gs itself was formed with the bf16-rounded weight: du differs from mnas_se_bwd_reduce's by that
 *                           rounding, <= 4e-3 relative per term, inside the gradient tolerances of tests/test_gpu_se.py).
 *                           wpartial is overwritten (scratch).  Deterministic (fixed summation order). */
int mnas_se_gate(const float* u, int N, int C, float* gate, void* stream);
int mnas_se_proj_finalize(float* wpartial, int N, int kseg, int Co, int Ci, const float* u, const float* W, float* dW,
                          int accumulate, float* du, void* stream);
/* The excitation MLP in one launch per direction (ABI 7).  z [N][E] fp32 = the pooled activation, W1 [R][E] / b1 [R] = fc1, W2 [E][R] /
 * b2 [E] = fc2 (torch.nn.Linear layouts, 4-byte alignment is enough), shapes: mnas_se_fc_supported:
 *   mnas_se_fc_fwd : hb = relu(W1 z + b1) [N][R];  u = W2 hb + b2 [N][E];  gate = sigmoid(u) [N][E] when gate != NULL
 *                    (replaces two mnas_head_linear_fwd calls and mnas_se_gate)
 *   mnas_se_fc_bwd : from du = dL/du [N][E]:  dh = (du W2) * [hb > 0] [N][R] (caller-provided scratch);  dz = dh W1 [N][E];
 *                    dW2 (+)= du^T hb, db2 (+)= sum_n du, dW1 (+)= dh^T z, db1 (+)= sum_n dh   (accumulate != 0: add to the buffers)
 *                    (replaces two mnas_head_linear_bwd_w and two mnas_head_linear_bwd_x calls; two kernels, fixed summation order) */
int mnas_se_fc_supported(int E, int R);     /* 1: the two calls below take this shape (R <= 48, E <= 1280, 64 KB of LDS); else use mnas_head_linear_* */
int mnas_se_fc_fwd(const float* z, const float* W1, const float* b1, const float* W2, const float* b2, int N, int E, int R,
                   float* hb, float* u, float* gate, void* stream);
int mnas_se_fc_bwd(const float* du, const float* z, const float* hb, const float* W1, const float* W2, int N, int E, int R,
                   float* dh, float* dz, float* dW1, float* db1, float* dW2, float* db2, int accumulate, void* stream);


/* ---- weight packing (fp32 reference layout [Co][Ci/g][kh][kw] -> kernel layouts) -------------------- */
#define MNAS_PACK_FWD   0   /* bf16 [Co_pad16][Kpad32], k = tap*Ci+ci            (mnas_conv_gemm mode 0) */
#define MNAS_PACK_DGRAD 1   /* bf16 [Ci_pad16][Kpad32], k = tap*Co+co            (mnas_conv_gemm mode 1) */
#define MNAS_PACK_DW    2   /* fp32 [k*k][C]                                      (mnas_dw_*)            */
#define MNAS_PACK_TCONV 3   /* bf16 [round16(4*Ci)][round32(4*Co)]: block matrix of a 3x3 stride-2 conv's taps by output parity
                               class (rows) and dy neighbour (columns)            (mnas_tconv_dgrad)     */
int mnas_pack_weights(const float* w, int kind, int Co, int Ci, int kh, int kw, void* dst, void* stream);
/* The same for many tensors in one launch: `descs` is a DEVICE array of n descriptors (taps = kh*kw; for MNAS_PACK_DW
 * Ci is ignored).  Used once per forward for all layers of the network. */
typedef struct MnasPackDesc {
    const float* w;
    void*   dst;
    int32_t kind, Co, Ci, taps;
} MnasPackDesc;
int mnas_pack_weights_batch(const MnasPackDesc* descs, int n, void* stream);
/* sizes in BYTES of the packed buffers */
int64_t mnas_packed_bytes(int kind, int Co, int Ci, int kh, int kw);

/* ---- fused Adam over a flat fp32 parameter/gradient buffer (train.py:219-221: Adam(lr)) -------------- */
int mnas_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);

/* The other two optimizers train.py offers (:222-228), same flat buffers and grad_scale convention:
 * torch.optim.RMSprop (centered = False; momentum_buf may be NULL when momentum == 0) and torch.optim.SGD (step = 1 initialises
 * the momentum buffer with the gradient, as torch does; momentum_buf may be NULL when momentum == 0). */
int mnas_rmsprop_step(float* p, const float* g, float* square_avg, float* momentum_buf, int64_t n, float lr, float alpha,
                      float eps, float weight_decay, float momentum, float grad_scale, void* stream);
int mnas_sgd_step(float* p, const float* g, float* momentum_buf, int64_t n, float lr, float momentum, float dampening,
                  float weight_decay, int nesterov, int step, float grad_scale, void* stream);

/* ---- global-norm gradient clipping, non-finite skip and weight EMA on the flat buffers ------------------
 * Additive: four new symbols and three new structs; no existing entry point, struct layout, opcode or kernel changes, so the ABI
 * version stays 8.
 *
 * The norm is that of the gradient the optimizer consumes, g[i] * grad_scale (the product formed in fp32), over every trainable
 * run of the flat buffer.  One deterministic launch per run leaves fp64 partial sums of squares in consecutive slots of ONE table of
 * MNAS_GRADNORM_MAX_PARTS doubles; every workgroup of every *_step_ex launch of the step then reduces the nparts used slots itself,
 * in a fixed order, so all of them derive the same bits  S = sum of the slots,  norm = (float)sqrt(S)  with no finalize launch and
 * nothing read by the host.  No atomics anywhere: the same input gives the same partials, norm and coefficient on every run and on
 * every rank of a data-parallel job. */
#define MNAS_GRADNORM_MAX_PARTS 1024
/* Device block the *_step_ex launch with update_stats != 0 moves (thread 0 of workgroup 0; zero it to reset).  32 bytes. */
typedef struct MnasGradStats {
    float   last_norm;        /* norm of the last step (0 when no norm was taken: EMA only) */
    float   last_coef;        /* clip coefficient of the last step as computed (1 when not clipping) */
    int64_t steps;            /* *_step_ex steps, skipped ones included */
    int64_t clipped_steps;    /* steps applied with coef < 1 */
    int64_t skipped_steps;    /* steps dropped by skip_nonfinite */
} MnasGradStats;
/* One run's partial sums: grid = min(256, ceil(n / 1024)) workgroups of 256 threads, a function of n only; workgroup b writes
 * partial[part_offset + b].  Every lane adds the squares of its grid-stride elements in increasing index order in fp64 (the fp32
 * product g[i] * grad_scale widened first: 1e25 squares to a finite value), then a wave-64 butterfly, then the four waves through
 * LDS in wave order.  g needs 4-byte alignment only (a run may start at any element).  *nparts_out (HOST, may be NULL) = the
 * grid; n == 0 launches nothing and reports 0.  MNAS_EINVAL, and no launch, when part_offset < 0 or part_offset + grid exceeds
 * MNAS_GRADNORM_MAX_PARTS. */
int mnas_grad_sqnorm(const float* g, int64_t n, float grad_scale, double* partial, int part_offset, int* nparts_out, void* stream);
/* HOST struct: what a *_step_ex launch does beyond its plain counterpart.
 *   coef = 1, or with 0 < max_norm < +inf:  q = max_norm / (norm + 1e-6f) in fp32, coef = q < 1 ? q : 1, a NaN q kept
 *          (torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1)); the update consumes
 *          (g[i] * grad_scale) * coef in front of the weight-decay fma -- with coef == 1 bit for bit the plain update;
 *   skip_nonfinite and a NaN / Inf norm: the launch writes nothing to p, the moments or the EMA, and the step counts as skipped;
 *          without the flag a non-finite norm propagates through coef as in torch (error_if_nonfinite = False);
 *   ema != NULL: after p[i] is written, ema[i] = fmaf(ema_decay, ema[i], (1 - ema_decay) * p[i]); ema points at the run's first
 *          element like p; ema_decay in [0, 1);
 *   update_stats: set on ONE launch of a step (the first run's).
 * nparts == 0 (no norm taken) is valid for an EMA-only step: max_norm and skip_nonfinite must then be off. */
typedef struct MnasOptExtra {
    const double*  partial;         /* the table mnas_grad_sqnorm filled; may be NULL when nparts == 0 */
    int32_t        nparts;          /* used slots, 0 .. MNAS_GRADNORM_MAX_PARTS */
    float          max_norm;        /* <= 0 or +inf: do not clip */
    int32_t        skip_nonfinite;
    float*         ema;             /* NULL: no EMA */
    float          ema_decay;
    MnasGradStats* stats;           /* DEVICE; may be NULL when update_stats == 0 */
    int32_t        update_stats;
} MnasOptExtra;
int mnas_adam_step_ex(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                      float weight_decay, int step, float grad_scale, const MnasOptExtra* extra, void* stream);
int mnas_rmsprop_step_ex(float* p, const float* g, float* square_avg, float* momentum_buf, int64_t n, float lr, float alpha,
                         float eps, float weight_decay, float momentum, float grad_scale, const MnasOptExtra* extra, void* stream);
int mnas_sgd_step_ex(float* p, const float* g, float* momentum_buf, int64_t n, float lr, float momentum, float dampening,
                     float weight_decay, int nesterov, int step, float grad_scale, const MnasOptExtra* extra, void* stream);

/* ---- parameter groups, decoupled weight decay and layer-wise trust ratios (LAMB / LARS) on the flat buffers ----------
 * Additive: three new symbols and four new structs; no existing entry point, struct layout, opcode or kernel changes, so the ABI
 * version stays 8.
 *
 * The whole flat buffer is updated by ONE call, and the update itself is one launch, whatever the number of parameter tensors
 * and groups.  Two DEVICE tables, built by the caller and uploaded only when they change, tell the kernels which tensor an
 * element belongs to:
 *   segment = one trainable parameter tensor: elements [begin, begin + n) of the flat buffers, its group, and its tiles
 *             [tile0, tile0 + ntiles) of the tile table.  A frozen tensor has no segment: nothing of it is read or written.
 *   tile    = at most MNAS_OPT_TILE consecutive elements of ONE segment: [begin, begin + n), its segment.  The tiles of a segment
 *             are consecutive in the table and in increasing element order, and the tiles cover every segment exactly once.
 * Segments (and so tiles) start at any element: 4-byte alignment only, as for mnas_grad_sqnorm.  The tables are NOT checked on the
 * device: a tile outside the buffers is an out-of-bounds access, a group index >= ngroups reads an unset group.
 * The groups are a HOST array read at every call: lr, weight_decay and the two flags travel to the kernels by value (as lr reaches
 * mnas_adam_step), so a scheduler costs no upload.  The other hyper-parameters (betas, eps, alpha, momentum, ...) are per call.
 *
 * Per element, all in fp32, fmaf exactly where the plain kernels use it;  gs = g[i] * grad_scale,  with an extra that clips:
 * gs = (g[i] * grad_scale) * coef  (MnasOptExtra above; extra NULL or not clipping: no further multiply / coef == 1):
 *   coupled decay (decoupled == 0, trust_kind == 0): bit for bit the update mnas_<kind>_step / _step_ex applies to that element
 *       with the group's lr and weight_decay;
 *   decoupled decay (decoupled != 0): p' = p * f with f = (float)(1.0 - (double)lr * (double)weight_decay) formed on the host
 *       (torch's param.mul_(1 - lr * weight_decay)), then the optimizer's update of p' from gs with weight_decay = 0: for Adam
 *       torch.optim.AdamW; the same for RMSprop and SGD;
 *   LAMB (trust_kind == MNAS_TRUST_LAMB, Adam only):  m = fmaf(b1, m, (1 - b1) * gs), v = fmaf(b2, v, (1 - b2) * gs * gs),
 *       u = (m / bc1) / (sqrtf(v) / bc2_sqrt + eps), and with weight_decay != 0  u = fmaf(weight_decay, p, u);
 *       p = p - (lr * r) * u.   Over the element's segment  w = (float)sqrt(sum (double)p^2),  un = (float)sqrt(sum (double)u^2),
 *       r = (w > 0 && un > 0) ? w / un : 1;
 *   LARS (trust_kind == MNAS_TRUST_LARS, SGD only):  gn = (float)sqrt(sum (double)gs^2),  w as above,
 *       r = (w > 0 && gn > 0) ? (trust_coef * w) / (fmaf(weight_decay, w, gn) + trust_eps) : 1;
 *       gi = (weight_decay != 0 ? fmaf(weight_decay, p, gs) : gs) * r, then momentum / dampening / nesterov and p = p - lr * gi
 *       as in mnas_sgd_step;
 *   a group with trust == 0 in a trust-ratio step: r = 1 (exactly; no norm is taken of its segments), and, if it is decoupled,
 *       p' = p * f first and weight_decay = 0 in u / gi.
 * Norms (trust_kind != 0 only): no atomics.  A read-only pass ahead of the update recomputes m, v in registers and leaves, per
 * tile, two fp64 partial sums in tile_partial[2 t], [2 t + 1]: every lane adds the squares of its elements t.begin + lane + 256 j in
 * increasing j in fp64 (the fp32 value widened first), then the wave-64 butterfly and the four waves in wave order, as in
 * mnas_grad_sqnorm.  A small finalize launch (one lane per segment) adds each segment's tile partials in tile order and writes
 * ratio[segment] once; the update launch reads it.  All of it is a function of the tables and the data only, not of the grid: the
 * same input gives the same bits on every run and on every rank.
 * extra (may be NULL) means what it means for mnas_*_step_ex, with ema pointing at the BASE of the shadow buffer and update_stats
 * honoured by the update launch alone.  With skip_nonfinite and a non-finite global norm, none of the launches writes anything but
 * the stats block: p, the moments, the EMA, tile_partial and ratio stay as they were.
 * Launches of one call: [norm pass, ratio finalize,] update; 256-thread workgroups grid-stride over the tiles, at most 2048 of
 * them.  Nothing is allocated, uploaded, read back or synchronised: the call can be captured.
 * MNAS_EINVAL, before anything is launched: a NULL segs / tiles / groups / p / g (or moment buffer the optimizer needs), nsegs
 * outside [0, MNAS_OPT_MAX_SEGS], ngroups outside [1, MNAS_OPT_MAX_GROUPS], ntiles < 0 (or < nsegs), trust_kind outside 0..2, LAMB
 * on anything but Adam, LARS on anything but SGD, any trust_kind != 0 on RMSprop, trust_kind != 0 without tile_partial / ratio, a
 * group with decoupled and trust both set, trust_eps < 0, a NaN lr / weight_decay / trust_coef / trust_eps / grad_scale, step < 1
 * (Adam, SGD), and whatever mnas_*_step_ex refuses of a non-NULL extra.  nsegs == 0 is valid and launches nothing. */
#define MNAS_OPT_TILE 4096
#define MNAS_OPT_MAX_GROUPS 32
#define MNAS_OPT_MAX_SEGS 4096
#define MNAS_TRUST_NONE 0
#define MNAS_TRUST_LAMB 1
#define MNAS_TRUST_LARS 2
typedef struct MnasOptSeg {          /* DEVICE table entry, 32 bytes */
    int64_t begin;                   /* first element inside the flat buffers */
    int64_t n;                       /* elements, >= 1 */
    int32_t group;                   /* 0 .. ngroups - 1 */
    int32_t tile0;                   /* the segment's first tile */
    int32_t ntiles;                  /* ceil(n / MNAS_OPT_TILE) */
    int32_t reserved;                /* 0 */
} MnasOptSeg;
typedef struct MnasOptTile {         /* DEVICE table entry, 16 bytes */
    int64_t begin;                   /* first element inside the flat buffers */
    int32_t n;                       /* 1 .. MNAS_OPT_TILE */
    int32_t seg;                     /* the segment the tile belongs to */
} MnasOptTile;
typedef struct MnasOptGroup {        /* HOST array entry, 16 bytes */
    float   lr;
    float   weight_decay;
    int32_t decoupled;               /* != 0: decoupled decay (not together with trust) */
    int32_t trust;                   /* != 0: the group's segments take the step's trust ratio */
} MnasOptGroup;
typedef struct MnasOptSegs {         /* HOST struct */
    const MnasOptSeg*   segs;        /* DEVICE, nsegs entries */
    const MnasOptTile*  tiles;       /* DEVICE, ntiles entries */
    const MnasOptGroup* groups;      /* HOST, ngroups entries */
    int32_t             nsegs;
    int32_t             ntiles;
    int32_t             ngroups;
    int32_t             trust_kind;  /* MNAS_TRUST_* */
    double*             tile_partial;/* DEVICE workspace, 2 * ntiles doubles; may be NULL when trust_kind == 0 */
    float*              ratio;       /* DEVICE, nsegs floats: the step's trust ratios; may be NULL when trust_kind == 0 */
    float               trust_coef;  /* LARS */
    float               trust_eps;   /* LARS, >= 0 */
} MnasOptSegs;
/* The plain entry points' arguments with p / g / the moments as the BASE of the flat buffers and without n, lr, weight_decay. */
int mnas_adam_step_seg(float* p, const float* g, float* m, float* v, float beta1, float beta2, float eps, int step,
                       float grad_scale, const MnasOptSegs* segs, const MnasOptExtra* extra, void* stream);
int mnas_rmsprop_step_seg(float* p, const float* g, float* square_avg, float* momentum_buf, float alpha, float eps, float momentum,
                          float grad_scale, const MnasOptSegs* segs, const MnasOptExtra* extra, void* stream);
int mnas_sgd_step_seg(float* p, const float* g, float* momentum_buf, float momentum, float dampening, int nesterov, int step,
                      float grad_scale, const MnasOptSegs* segs, const MnasOptExtra* extra, void* stream);

/* ---- batched launch: run a pre-built list of the calls above with ONE host->library transition ------- */
#define MNAS_OP_CONV_GEMM 1
#define MNAS_OP_CONV_WGRAD 2
#define MNAS_OP_WGRAD_FINALIZE 3
#define MNAS_OP_DW_FWD 4
#define MNAS_OP_DW_BWD 5
#define MNAS_OP_DW_WGRAD_FINALIZE 6
#define MNAS_OP_STEM_FWD 7
#define MNAS_OP_STEM_WGRAD 8
#define MNAS_OP_BN_FWD_FINALIZE 9
#define MNAS_OP_BN_BWD_REDUCE 10
#define MNAS_OP_BN_BWD_FINALIZE 11
#define MNAS_OP_ADD_ACT 12
#define MNAS_OP_NCHW_TO_NHWC 13
#define MNAS_OP_PACK_WEIGHTS 14
#define MNAS_OP_EVENT_RECORD 15    /* p[0] = event handle from mnas_event_create: hipEventRecord on the op's stream;
                                      p[1] = NULL or a HOST int*: the record is skipped while *p[1] == 0 (measurement gating) */
#define MNAS_OP_EVENT_WAIT 16      /* p[0] = event handle: hipStreamWaitEvent(op's stream, event) */
#define MNAS_OP_PW_BWD 17
#define MNAS_OP_PACK_BATCH 18
#define MNAS_OP_POOL_ACT 22
#define MNAS_OP_POOL_BWD 23
#define MNAS_OP_DY_MAT 24
#define MNAS_OP_BWD_POST 25
#define MNAS_OP_TCONV_DGRAD 26
/* 19-21, 27-29, 36: retired in ABI 6 (Gram-statistics / fused-block / affine-on-read forms; DESIGN_HISTORY.md) */
#define MNAS_OP_HEAD_LINEAR 30  /* i[5]: 0 forward, 1 weight gradient, 2 input gradient */
#define MNAS_OP_SE_SCALE 31
#define MNAS_OP_SE_BWD_REDUCE 32
#define MNAS_OP_SE_BWD_APPLY 33
#define MNAS_OP_SE_GATE 34          /* ABI 5 */
#define MNAS_OP_SE_PROJ_FIN 35      /* ABI 5 */
#define MNAS_OP_SE_FC_FWD 37        /* ABI 7: i = {N, E, R}; p = {z, W1, b1, W2, b2, hb, u, gate or NULL} */
#define MNAS_OP_STEM_DGRAD 39       /* ABI 7: i = {N, H, W, Ho, Wo, Co}; p = {g, y, coef, w fp32, in_affine or NULL, dx} */
#define MNAS_OP_SE_FC_BWD 38        /* ABI 7: i = {N, E, R, accumulate}; p = {du, z, hb, W1, W2, dh, dz, dW1, db1, dW2, db2} */
/* frozen BatchNorm statistics (ABI 8, additive) */
#define MNAS_OP_BN_FROZEN_BATCH 40          /* i = {n}; p = {descs: device array of MnasBnFrozenDesc} */
#define MNAS_OP_BWD_POST_FROZEN 41          /* the slots of MNAS_OP_BWD_POST; p[8] = dbias */
#define MNAS_OP_BN_BWD_FINALIZE_FROZEN 42   /* i = {nparts, C, accumulate}; p = {partial, bnbuf, dgamma, dbeta, dbias} */
typedef struct MnasOp {
    int32_t opcode;
    int32_t i[15];
    double  d[4];
    void*   p[16];
} MnasOp;
/* Field use per opcode is documented next to mnas_run_ops in csrc/mnas_abi.hip. Stops at the first error
 * and returns it (index of the failing op in *failed_at if non-NULL). */
int mnas_run_ops(const MnasOp* ops, int n, void* stream, int* failed_at);
/* Same, over several streams: op.i[14] selects streams[op.i[14]] (0 <= i[14] < nstreams).  Ordering between
 * streams is expressed with MNAS_OP_EVENT_RECORD / MNAS_OP_EVENT_WAIT ops.  Used to run the weight-gradient
 * kernels of a layer concurrently with the input-gradient chain (they only share read-only inputs). */
int mnas_run_ops_multi(const MnasOp* ops, int n, void* const* streams, int nstreams, int* failed_at);
/* The same launch list captured once into a hipGraph and replayed (ABI 7).  mnas_graph_create runs the list under stream capture on
 * streams[0] (nothing executes) and instantiates it; mnas_graph_launch replays it on `stream`.  Everything in the list is baked in
 * -- pointers, integers, and whether a gated EVENT_RECORD was live at capture time: re-create when the list changes. */
int mnas_graph_create(const MnasOp* ops, int n, void* const* streams, int nstreams, void** exec_out, int* failed_at);
int mnas_graph_launch(void* exec, void* stream);
int mnas_graph_destroy(void* exec);

/* ---- scratch sizes (bytes) of the partial tables the launches above write; the library never allocates.
 * kind MNAS_WS_CONV_STATS:  float[2][c][n]      (c = Co, n = nparts; also the fused-reduce tables)
 * kind MNAS_WS_CONV_WGRAD:  float[n][c][k]      (n = nsplit, c = Co, k = kh*kw*Ci)
 * kind MNAS_WS_PW_BWD:      float[n][c][k]      (n = nparts, c = Co, k = Ci)
 * kind MNAS_WS_DW_WGRAD:    float[n][k][c]      (n = mnas_dw_rows(...), k = taps, c = C) */
#define MNAS_WS_CONV_STATS 0
#define MNAS_WS_CONV_WGRAD 1
#define MNAS_WS_PW_BWD 2
#define MNAS_WS_DW_WGRAD 3
int64_t mnas_workspace_bytes(int kind, int n, int c, int k);

/* ---- HIP events on the launch stream (measurement only: bench.py brackets single kernel launches inside
 * the timed region; torch.cuda.Event cannot be recorded from inside mnas_run_ops) ------------------------ */
int mnas_event_create(void** event);
int mnas_event_destroy(void* event);
int mnas_event_record(void* event, void* stream);
int mnas_event_elapsed_ms(void* start, void* stop, float* ms);   /* non-zero if either is not complete */

/* ---- box calibration (measurement only, csrc/mnas_probe.hip): what THIS GPU sustains, taken by bench.py right before and after
 * its timed windows -- boxes of one pool differ in shader clock / power state, and a step rate means nothing without them.
 * mnas_probe_copy: dst = src as 16-byte-per-lane loads and stores (bytes % 16 == 0); rate = 2*bytes / time.
 * mnas_probe_valu: blocks x 256 threads, iters x 8 independent v_pk_fma_f32 per lane, nothing else:
 *                  flop = blocks*256*iters*8*4;  TFLOP/s / 65.536 = sustained shader clock in GHz (256 CUs x 4 SIMDs x 16 lanes). */
int mnas_probe_copy(const void* src, void* dst, int64_t bytes, void* stream);
int mnas_probe_valu(float* out, int blocks, int iters, void* stream);
/* round 6 (ABI 8): the probes a kernel of the step may be compared with -- four independent 16-byte nontemporal loads in flight
 * per lane (k_probe_copy keeps one).  mnas_probe_copy4: rate = 2*bytes / time.  mnas_probe_read: read-only stream, `sink`
 * (>= 4 * workgroups bytes) is never written; rate = bytes / time.  Both: bytes % 16384 == 0.  blocks = 0: one 16 KB trip per
 * workgroup up to 65536 workgroups, > 0: that many persistent workgroups. */
int mnas_probe_copy4(const void* src, void* dst, int64_t bytes, int blocks, void* stream);
int mnas_probe_read(const void* src, void* sink, int64_t bytes, int blocks, void* stream);
int mnas_probe_empty(int blocks, int threads, void* stream);      /* a kernel that does nothing: the cost of one launch in a stream */

/* ---- image batch transform (csrc/mnas_imgx.hip; additive within ABI 8, outside the launch lists): the geometric half of the
 * reference's PIL input pipeline (datasets.py preprocess_img: crop, Resize / RandomResizedCrop with BILINEAR, flips) on the GPU.
 * Every output image is, byte for byte,
 *     flips(window(PIL.Image.crop(src, box).resize((rw, rh), Image.BILINEAR)))
 * with src a decoded HWC uint8 image (C = 1 is replicated to RGB, C = 4 drops alpha), the window Ho x Wo at (win_top, win_left)
 * of the rh x rw resized box, and the flips applied to the window.  Output: NCHW uint8 (N, 3, Ho, Wo), contiguous -- what the
 * stem's uint8 input path reads.  Per axis the box may be downscaled at most MNAS_IMGX_MAX_DOWNSCALE times (any upscale). */
#define MNAS_IMGX_HFLIP 1
#define MNAS_IMGX_VFLIP 2
#define MNAS_IMGX_MAX_DOWNSCALE 32
#define MNAS_IMGX_MAX_DIM 65536        /* source and resized sides */
#define MNAS_IMGX_MAX_OUT 16384        /* Ho, Wo */
typedef struct MnasImgXform {          /* 64 bytes */
    int64_t src_offset;                /* byte offset of the image in `src` */
    int32_t src_h, src_w, src_c, src_stride;     /* HWC uint8, c in {1, 3, 4}, row stride in bytes */
    int32_t box_top, box_left, box_h, box_w;     /* crop box, inside the image */
    int32_t rh, rw;                    /* the box is resized to rh x rw (PIL bilinear) */
    int32_t win_top, win_left;         /* Ho x Wo window inside the resized box */
    int32_t flags;                     /* MNAS_IMGX_HFLIP | MNAS_IMGX_VFLIP */
    int32_t reserved;                  /* 0 */
} MnasImgXform;
/* Host-side validation, no launch: every item's box inside its image, its window inside the resized box, its bytes inside
 * [0, src_bytes), c in {1, 3, 4}, sizes >= 1, downscale within range, unknown flags 0; n in [0, 65535], Ho, Wo in
 * [1, MNAS_IMGX_MAX_OUT], src_bytes a positive multiple of 16.  0 or MNAS_EINVAL.  items_host: HOST pointer. */
int mnas_img_xform_check(const MnasImgXform* items_host, int n, int Ho, int Wo, int64_t src_bytes);
/* items (n descriptors), src (16-byte aligned, src_bytes % 16 == 0) and out (4-byte aligned, n*3*Ho*Wo bytes): device.
 * Run the host check on the same descriptors first; the kernel re-checks each descriptor it reads, writes nothing for one it
 * refuses, and clamps every source address into [0, src_bytes). */
int mnas_img_xform(const MnasImgXform* items, int n, int Ho, int Wo, const void* src, int64_t src_bytes, void* out_u8_nchw,
                   void* stream);

/* ---- photometric image ops (csrc/mnas_imgc.hip; additive within ABI 8, outside the launch lists): the other half of the
 * reference's input pipeline (preprocessing type 3: torchvision 0.2.x ColorJitter, RandomGrayscale) on uint8 RGB batches, byte
 * for byte what Pillow computes:
 *     BRIGHTNESS / CONTRAST / SATURATION f = ImageEnhance.*.enhance(f) = Image.blend(degenerate, img, (float)f)
 *         degenerate: 0 / the image's grey mean int(sum(L) / (H*W) + 0.5) / the pixel's grey L
 *     HUE         img.convert('HSV'), H = (H + hue_shift) mod 256, .convert('RGB')   (adjust_hue: hue_shift = int(f*255) mod 256)
 *     GRAY        (L, L, L), L = convert('L') = (19595 r + 38470 g + 7471 b + 0x8000) >> 16
 * Each item holds one image's ops, applied in order; a CONTRAST mean is taken over the image as the ops before it left it. */
#define MNAS_IMGC_BRIGHTNESS 1         /* blend with 0 */
#define MNAS_IMGC_CONTRAST   2         /* blend with the image's rounded grey mean; at most one per item */
#define MNAS_IMGC_SATURATION 3         /* blend with the pixel's grey */
#define MNAS_IMGC_HUE        4         /* RGB -> HSV, H += hue_shift mod 256, HSV -> RGB */
#define MNAS_IMGC_GRAY       5         /* (L, L, L) */
#define MNAS_IMGC_MAX_OPS    5
#define MNAS_IMGC_NCHW 0               /* (n, 3, H, W) uint8 */
#define MNAS_IMGC_NHWC 1               /* (n, H, W, 3) uint8 */
typedef struct MnasImgColor {          /* 52 bytes */
    int32_t nops;                      /* 0..MNAS_IMGC_MAX_OPS, applied in order; 0 = copy (in place: the image is not touched) */
    int32_t op[MNAS_IMGC_MAX_OPS];     /* MNAS_IMGC_BRIGHTNESS .. MNAS_IMGC_GRAY */
    float factor[MNAS_IMGC_MAX_OPS];   /* blend alpha of BRIGHTNESS / CONTRAST / SATURATION; finite and >= 0 for every k < nops */
    int32_t hue_shift;                 /* 0..255, used by HUE */
    int32_t reserved;                  /* 0 */
} MnasImgColor;
/* Host-side validation, no launch: every item's nops in [0, MAX_OPS], ops known, at most one CONTRAST, factors finite and >= 0,
 * hue_shift in [0, 255], reserved 0; n in [0, 65535], H, W in [1, MNAS_IMGX_MAX_OUT].  0 or MNAS_EINVAL.  items_host: HOST. */
int mnas_img_color_check(const MnasImgColor* items_host, int n, int H, int W);
/* Bytes of device workspace mnas_img_color needs when some item has CONTRAST (per-image partial sums); -1 for a bad shape. */
int64_t mnas_img_color_workspace_bytes(int n, int H, int W);
/* items (n descriptors), in and out (n*3*H*W bytes each, contiguous, in the given layouts) and workspace: device.  in == out
 * (in place) only with in_layout == out_layout; otherwise the two must not overlap.  workspace: mnas_img_color_workspace_bytes
 * bytes, 4-byte aligned, or null when no item has CONTRAST (the mean pass is then skipped).  Two launches when workspace is
 * given (the per-image grey sums, then the ops), one otherwise.  Run the host check first; the kernels re-check each
 * descriptor they read and write nothing for one they refuse (a CONTRAST item without a workspace included). */
int mnas_img_color(const MnasImgColor* items, int n, int H, int W, int in_layout, const void* in, int out_layout, void* out,
                   void* workspace, void* stream);

/* ---- batch mixing on uint8 images (csrc/mnas_imgm.hip; additive within ABI 8, outside the launch lists): Mixup and CutMix of
 * every image of an (n, 3, H, W) uint8 NCHW batch -- the layout the stem's uint8 input path reads -- with a partner image of the
 * same batch, so that a mixed batch stays a byte batch on the device:
 *     NONE    out = x
 *     MIXUP   out = (w x + (65536 - w) partner + 32768) >> 16 per byte, w = w16: integer arithmetic, defined byte for byte; at most
 *             0.5 away from the real-valued blend with weight w / 65536 (correct rounding)
 *     CUTMIX  out = partner inside rows [y0, y1) x columns [x0, x1) of every plane, x elsewhere
 * The weight of x that the loss needs is w16 / 65536 for MIXUP and 1 - (y1 - y0) (x1 - x0) / (H W) for CUTMIX. */
#define MNAS_IMGM_NONE   0             /* copy */
#define MNAS_IMGM_MIXUP  1             /* integer blend with the partner, w16 in [0, 65536] on x */
#define MNAS_IMGM_CUTMIX 2             /* the partner's bytes inside the box */
typedef struct MnasImgMix {            /* 32 bytes */
    int32_t mode;                      /* MNAS_IMGM_* */
    int32_t partner;                   /* index of the other image, in [0, n); the image itself is allowed */
    int32_t w16;                       /* 0..65536 (read by MIXUP) */
    int32_t y0, x0, y1, x1;            /* 0 <= y0 <= y1 <= H, 0 <= x0 <= x1 <= W (read by CUTMIX); empty boxes are allowed */
    int32_t reserved;                  /* 0 */
} MnasImgMix;
/* Host-side validation, no launch: every item's mode known, partner in [0, n), w16 in [0, 65536], box ordered and inside the
 * image, reserved 0 -- every field of every item, whatever its mode; n in [0, 65535], H, W in [1, MNAS_IMGX_MAX_OUT].  0 or
 * MNAS_EINVAL.  items_host: HOST. */
int mnas_img_mix_check(const MnasImgMix* items_host, int n, int H, int W);
/* items (n descriptors), in and out (n*3*H*W bytes each, contiguous): device.  Out of place only: partner is any index of the
 * batch, so a pass in place would read bytes it has already overwritten; in and out that overlap (in == out included) return
 * MNAS_EINVAL with no launch.  One launch; 16-byte loads and stores when H*W % 16 == 0 and both buffers are 16-byte aligned, byte
 * by byte otherwise.  Run the host check first; the kernel re-checks each descriptor it reads and writes nothing for one it
 * refuses. */
int mnas_img_mix(const MnasImgMix* items, int n, int H, int W, const void* in, void* out, void* stream);

/* ---- augmentation-policy ops on uint8 images (csrc/mnas_imga.hip; additive within ABI 8, outside the launch lists): what
 * RandAugment and the AutoAugment policies are made of, on the (n, 3, H, W) uint8 NCHW batch the stem reads.  Each item holds one
 * image's chain of up to MNAS_IMGA_MAX_OPS ops, applied in order; each op is byte for byte the Pillow call
 *     IDENTITY      copy
 *     AFFINE        img.transform(img.size, Image.AFFINE, (a, b, c, d, e, f), Image.NEAREST, fillcolor=fill), as 16.16 fixed point:
 *                   arg = {a0, a1, a2, a3, a4, a5} with FIX(v) = floor(v * 65536 + 0.5), a0, a1, a3, a4 = FIX(a, b, d, e),
 *                   a2 = FIX(c + a/2 + b/2), a5 = FIX(f + d/2 + e/2); output (x, y) takes the source pixel
 *                   ((a2 + x a0 + y a1) >> 16, (a5 + x a3 + y a4) >> 16) when it lies inside the image, the fill colour otherwise.
 *                   With a1 == a3 == 0 Pillow takes a route of its own that agrees with this one for unit scale and whole-pixel
 *                   translations, so such a matrix must have a0 == a4 == 65536 and a2, a5 = (whole pixels << 16) + 32768.
 *     BRIGHTNESS / COLOR / CONTRAST   ImageEnhance.*(img).enhance(factor): MNAS_IMGC_BRIGHTNESS / _SATURATION / _CONTRAST's arithmetic
 *     SHARPNESS     ImageEnhance.Sharpness(img).enhance(factor) = Image.blend(img.filter(ImageFilter.SMOOTH), img, factor); SMOOTH is
 *                   (1 1 1 / 1 5 1 / 1 1 1) / 13 rounded to nearest on interior pixels, the outermost rows and columns copied,
 *                   an image with H < 3 or W < 3 unchanged
 *     POSTERIZE     ImageOps.posterize(img, bits), bits = arg[0] in [1, 8]
 *     SOLARIZE      ImageOps.solarize(img, threshold), threshold = arg[0] in [0, 256]
 *     INVERT        ImageOps.invert(img)
 *     AUTOCONTRAST  ImageOps.autocontrast(img) (cutoff 0, per channel)
 *     EQUALIZE      ImageOps.equalize(img) (per channel)
 * CONTRAST, AUTOCONTRAST and EQUALIZE take their statistics (grey mean, per-channel histograms) over the image as the ops before
 * them left it. */
#define MNAS_IMGA_IDENTITY     0
#define MNAS_IMGA_AFFINE       1
#define MNAS_IMGA_BRIGHTNESS   2
#define MNAS_IMGA_COLOR        3
#define MNAS_IMGA_CONTRAST     4
#define MNAS_IMGA_SHARPNESS    5
#define MNAS_IMGA_POSTERIZE    6
#define MNAS_IMGA_SOLARIZE     7
#define MNAS_IMGA_INVERT       8
#define MNAS_IMGA_AUTOCONTRAST 9
#define MNAS_IMGA_EQUALIZE     10
#define MNAS_IMGA_MAX_OPS      4
typedef struct MnasImgAug {            /* 136 bytes */
    int32_t nops;                      /* 0..MNAS_IMGA_MAX_OPS, applied in order; 0 = copy */
    int32_t op[MNAS_IMGA_MAX_OPS];     /* MNAS_IMGA_* */
    float factor[MNAS_IMGA_MAX_OPS];   /* BRIGHTNESS / COLOR / CONTRAST / SHARPNESS: finite and >= 0; other ops: not read */
    int32_t arg[MNAS_IMGA_MAX_OPS][6]; /* AFFINE: a0..a5; POSTERIZE: bits; SOLARIZE: threshold; other ops: not read */
    int32_t reserved;                  /* 0 */
} MnasImgAug;
/* Host-side validation, no launch: every item's nops in [0, MAX_OPS], ops known, enhancer factors finite and >= 0, bits in [1, 8],
 * threshold in [0, 256], reserved 0, and every AFFINE matrix in range: a1 == a3 == 0 only in the form above, and a2 + x a0 + y a1
 * and a5 + x a3 + y a4 inside (-2^31, 2^31) at the four corners x in {0, W}, y in {0, H} (so the device's int32 arithmetic cannot
 * overflow, and Pillow, which leaves fixed point outside that range, is still what the bytes equal); n in [0, 65535], H, W in
 * [1, MNAS_IMGX_MAX_OUT].  0 or MNAS_EINVAL.  items_host: HOST. */
int mnas_img_aug_check(const MnasImgAug* items_host, int n, int H, int W);
/* Bytes of device workspace mnas_img_aug needs: one spare batch (16-byte rounded) when max_ops >= 2, plus, when need_stats != 0
 * (some item has CONTRAST, AUTOCONTRAST or EQUALIZE), 769 uint32 per (image, 16384-pixel chunk).  max_ops: the longest chain of the
 * batch, in [0, MAX_OPS].  0 is a valid answer; -1 for a bad shape or max_ops. */
int64_t mnas_img_aug_workspace_bytes(int n, int H, int W, int max_ops, int need_stats);
/* items (n descriptors), in and out (n*3*H*W bytes each, contiguous NCHW) and workspace: device; no two of the three buffers may
 * overlap (out of place only).  The ops run stage by stage, S = max(1, max_ops) stages, each one launch over the whole batch that
 * applies one op per image out of place, ping-ponging between out and the workspace so that the last stage writes out.  Chains
 * are right-aligned: an image of L ops (an empty chain counts as one IDENTITY) sits out the first S - L stages and then reads `in`,
 * so its last op lands in out with no copy stage.  stats_stages: bit s set when some image's op of stage s is CONTRAST,
 * AUTOCONTRAST or EQUALIZE; such a stage is preceded by a statistics launch over its input (LDS histograms, per (image, chunk)
 * partial tables in the workspace, no global atomics), and the apply launch reduces them into the image's mean or 3 x 256 table.
 * max_ops and stats_stages are the caller's, computed from the same descriptors it checked: a stage or statistics launch no image
 * needs is not launched.  fill_rgb: AFFINE's fill colour, r | g << 8 | b << 16.  workspace: mnas_img_aug_workspace_bytes(n, H, W,
 * max_ops, stats_stages != 0) bytes, 16-byte aligned, or null when that is 0.  16-byte loads and stores when H*W % 16 == 0 and the
 * buffers are 16-byte aligned, byte by byte otherwise.  Run the host check first; the kernels re-check each descriptor they read
 * and write nothing for one they refuse (a chain longer than max_ops, or a statistics op at a stage whose bit is clear, included). */
int mnas_img_aug(const MnasImgAug* items, int n, int H, int W, int max_ops, int stats_stages, int fill_rgb, const void* in,
                 void* out, void* workspace, void* stream);

/* ---- device random numbers (csrc/mnas_rng.h; additive within ABI 8): Philox4x32-10, a counter-based generator -- the four output
 * words are a pure function of a 128-bit counter c = {c0, c1, c2, c3} and a 64-bit key {k0, k1}, so a CPU test can state every
 * byte a kernel derives from them.  Ten rounds; each round computes, in 32-bit words with 32 x 32 -> 64-bit products,
 *     c' = {hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)},   M0 = 0xD2511F53, M1 = 0xCD9E8D57,
 * and then moves the key on: k0 += 0x9E3779B9, k1 += 0xBB67AE85.  Known answers (counter, key -> output):
 *     00000000 00000000 00000000 00000000, 00000000 00000000 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *     ffffffff ffffffff ffffffff ffffffff, ffffffff ffffffff -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *     243f6a88 85a308d3 13198a2e 03707344, a4093822 299f31d0 -> d16cfe09 94fdcceb 5001e420 24126ea1
 * The host entry below runs the header's function on the CPU (no GPU needed): ctr[4], key[2] in, out[4]. */
void mnas_philox4x32_10(const uint32_t* ctr, const uint32_t* key, uint32_t* out);

/* ---- Random Erasing on uint8 images (csrc/mnas_imge.hip; additive within ABI 8, outside the launch lists): Zhong et al. 2017 on
 * the (n, 3, H, W) uint8 NCHW batch the stem reads, IN PLACE.  One descriptor per image per launch; the box is rows [y0, y1) x
 * columns [x0, x1) of every plane:
 *     NONE   the image is not touched
 *     CONST  byte fill[c] in plane c
 *     NOISE  pixel (n, c, y, x), with k the launch's box position:
 *                r    = philox4x32_10(counter {x >> 3, y, 3 n + c, k}, key {seed & 0xffffffff, seed >> 32})
 *                word = r[(x & 7) >> 1];   half = (x & 1) ? word >> 16 : word & 0xffff
 *                byte = table[c * 4096 + (half & 4095)]
 *            one Philox call serves the eight pixels x >> 3 of a row.  y and x are coordinates in the IMAGE, not in the box: a pixel
 *            gets the same byte whichever box covers it at position k, and different k (or seeds) give independent streams.
 * table: 3 x 4096 bytes on the device, built by the caller -- erasing.erase_table carries N(mean_c, std_c) noise to byte space
 * through a 12-bit quantile table, T_c[i] = clamp(floor(255 (mean_c + std_c Phi^-1((i + 0.5) / 4096)) + 0.5), 0, 255); the kernel
 * evaluates no transcendental, so the bytes are exact.  A byte cannot hold the noise's tails: entries past 0 or 255 clamp.
 * Several boxes per image are several launches, one per box position k, in order (the scheme mnas_img_aug uses for op positions):
 * where boxes overlap the later position wins. */
#define MNAS_IMGE_NONE  0              /* not touched */
#define MNAS_IMGE_CONST 1              /* fill[c] in plane c */
#define MNAS_IMGE_NOISE 2              /* table[c][12 bits of Philox] per pixel */
typedef struct MnasImgErase {          /* 32 bytes */
    int32_t mode;                      /* MNAS_IMGE_* */
    int32_t y0, x0, y1, x1;            /* 0 <= y0 <= y1 <= H, 0 <= x0 <= x1 <= W; empty boxes are allowed */
    uint8_t fill[3];                   /* read by CONST */
    uint8_t pad;                       /* 0 */
    int32_t reserved[2];               /* 0 */
} MnasImgErase;
/* Host-side validation, no launch: every item's mode known, box ordered and inside the image, pad and reserved 0 -- every field of
 * every item, whatever its mode (fill takes any value); n in [0, 65535], H, W in [1, MNAS_IMGX_MAX_OUT].  0 or MNAS_EINVAL.
 * items_host: HOST. */
int mnas_img_erase_check(const MnasImgErase* items_host, int n, int H, int W);
/* items (n descriptors), x (n*3*H*W bytes, contiguous, ANY alignment) and table (3 * 4096 bytes, or null when no item is NOISE):
 * device.  One launch, in place on x: only the bytes inside the boxes are written and no byte of x is read.  grid (3 * bands, n)
 * with bands = ceil(H / 64): one workgroup = one plane of one image x one band of the BOX's rows (ceil(box rows / bands) each);
 * the workgroups of a NONE image, of an empty box and of bands past the box's last row return after reading the descriptor, so
 * the work is the erased area's, not the batch's.  A workgroup of a NOISE image first copies its plane's 4096 table bytes into LDS.
 * One lane = one 16-byte-aligned group of a box row: a group wholly inside the row goes out as one 16-byte store, a row's head and
 * tail as aligned 4-byte and single-byte stores; x0, W and the base address are arbitrary.  Plain vector stores, no atomics.
 * position: k above.  Run the host check first; the kernel re-checks each descriptor it reads and writes nothing for one it
 * refuses (a NOISE item with a null table included). */
int mnas_img_erase(const MnasImgErase* items, int n, int H, int W, void* x, const void* table, uint64_t seed, uint32_t position,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MNAS_H */
