// Photometric half of the training input pipeline (include/mnas.h "photometric image ops"): per image a chain of up to five
// ops -- brightness / contrast / saturation blends, a hue rotation, grey -- on uint8 RGB, byte for byte what Pillow computes
// (ImageEnhance + Image.blend, Convert.c rgb2hsv_row / hsv2rgb, convert('L')), NCHW or NHWC in, NCHW or NHWC out.
//
// Pillow's arithmetic, restated (tests/img_color_ref.py holds the restatement to Pillow over every input):
//   grey   L = (19595 r + 38470 g + 7471 b + 0x8000) >> 16
//   blend  t = (float)a + alpha * (float)(b - a) (fp32, two roundings); Pillow truncates t for 0 <= alpha <= 1 and clips it to
//          [0, 255] first otherwise.  For 0 <= alpha <= 1 and a, b in [0, 255] t already lies in [min(a, b), max(a, b)] (both
//          fp32 roundings are monotone and a, b are exact), so one clip-then-truncate serves both branches.
//   hue    rgb2hsv in fp32 / fp64 as Convert.c writes it, then hsv2rgb; the values of hsv2rgb that depend on H alone (floor and
//          fraction of H * 6 / 255) or on S alone (S / 255) come from 256-entry LDS tables built with the same fp64 expressions.
// Every function doing fp math carries `#pragma clang fp contract(off)`: no FMA contraction, as in Pillow's x86 build.
//
// Two launches.  The mean pass (only when some item has CONTRAST; the caller then passes a workspace) runs each such item's
// ops before its CONTRAST, forms L and writes one uint32 grey sum per (image, chunk of IMGC_CHUNK pixels): integer sums are
// exact, so the order does not matter, and no atomics are needed.  The apply pass reduces an image's chunk sums, takes the mean
// with Pillow's fp64 expression, runs the whole chain per pixel and stores in the output layout.  One workgroup = one image x
// one chunk; one lane = IMGC_GROUPS groups of 16 consecutive pixels, moved with 16-byte loads and stores (three per group:
// one per plane in NCHW, the 48-byte pixel run in NHWC) when H*W % 16 == 0 and the buffers are 16-byte aligned, byte by byte
// otherwise.
#include "mnas_imgc.h"

// Shared by the host check and the kernels (which re-check every descriptor they read and skip one they would refuse).
__host__ __device__ static inline bool imgc_item_ok(const MnasImgColor& t, bool have_ws) {
    if (t.nops < 0 || t.nops > MNAS_IMGC_MAX_OPS || t.hue_shift < 0 || t.hue_shift > 255 || t.reserved != 0) return false;
    int ncontrast = 0;
    for (int k = 0; k < t.nops; ++k) {
        if (t.op[k] < MNAS_IMGC_BRIGHTNESS || t.op[k] > MNAS_IMGC_GRAY) return false;
        if (!(t.factor[k] >= 0.f && t.factor[k] <= 3.402823466e38f)) return false;     // NaN, inf and negatives fail
        ncontrast += t.op[k] == MNAS_IMGC_CONTRAST;
    }
    return ncontrast == 0 || (ncontrast == 1 && have_ws);
}

// hue tables: ftab[H] = (float)(x - floor(x)), x = H * 6.0 / 255.0; fstab[S] = (float)(S / 255.0)
struct ImgcTables {
    float f[256];
    float fs[256];
};

__device__ __forceinline__ void imgc_build_tables(ImgcTables* t, int tid) {
#pragma clang fp contract(off)
    const double x = (double)tid * 6.0 / 255.0;
    t->f[tid] = (float)(x - (double)(int)floor(x));
    t->fs[tid] = (float)((double)tid / 255.0);
}

// Convert.c rgb2hsv_row, H += shift, hsv2rgb
__device__ __forceinline__ void imgc_hue(uint32_t& r, uint32_t& g, uint32_t& b, int shift, const ImgcTables* tab) {
#pragma clang fp contract(off)
    const uint32_t mx = max(r, max(g, b)), mn = min(r, min(g, b));
    if (mx == mn) return;                                   // H = S = 0: hsv2rgb gives (V, V, V), the pixel itself
    const float cr = (float)(int)(mx - mn);
    const float s = cr / (float)(int)mx;
    // h = bc - gc (r max), 2 + rc - bc (g max), 4 + gc - rc: every sum below is exact in fp64 (fp32 terms in [0, 1] with
    // exponents >= -8), so one rounding to fp32 equals Pillow's fp32 subtraction and its fp64 expressions alike
    const uint32_t cx = r == mx ? b : (g == mx ? r : g);
    const uint32_t cy = r == mx ? g : (g == mx ? b : r);
    const double base = r == mx ? 0.0 : (g == mx ? 2.0 : 4.0);
    const float xc = (float)(int)(mx - cx) / cr, yc = (float)(int)(mx - cy) / cr;
    const float h = (float)(base + (double)xc - (double)yc);
    double hd = (double)h / 6.0 + 1.0;                      // in [5/6, 11/6]: fmod(hd, 1.0) is this subtraction, exactly
    if (hd >= 1.0) hd -= 1.0;
    const int H = (imgc_clip8((int)((double)(float)hd * 255.0)) + shift) & 255;
    const int S = imgc_clip8((int)((double)s * 255.0));
    if (S == 0) {
        r = g = b = mx;
        return;
    }
    const int i = (2 * H) / 85;                             // floor(H * 6.0 / 255.0): 6H / 255 is never within 1/85 of an integer it is not
    const float f = tab->f[H], fs = tab->fs[S];
    const double V = (double)mx;
    const uint32_t p = (uint32_t)imgc_clip8((int)round(V * (1.0 - (double)fs)));
    const uint32_t q = (uint32_t)imgc_clip8((int)round(V * (1.0 - (double)(fs * f))));
    const uint32_t t = (uint32_t)imgc_clip8((int)round(V * (1.0 - (double)fs * (1.0 - (double)f))));
    switch (i) {
        case 1: r = q; g = mx; b = p; break;
        case 2: r = p; g = mx; b = t; break;
        case 3: r = p; g = q; b = mx; break;
        case 4: r = t; g = p; b = mx; break;
        case 5: r = mx; g = p; b = q; break;
        default: r = mx; g = t; b = p; break;               // i = 0 or 6 (H = 255)
    }
}

// one op on N pixels (the op is uniform over the workgroup: the switch is outside the pixel loop); `mean` is the item's
// CONTRAST degenerate
template <int N>
__device__ __forceinline__ void imgc_op(int op, float f, int shift, int mean, const ImgcTables* tab, uint32_t* r, uint32_t* g,
                                        uint32_t* b) {
    switch (op) {
        case MNAS_IMGC_BRIGHTNESS:
#pragma unroll
            for (int j = 0; j < N; ++j) {
                r[j] = imgc_blend(0u, r[j], f); g[j] = imgc_blend(0u, g[j], f); b[j] = imgc_blend(0u, b[j], f);
            }
            break;
        case MNAS_IMGC_CONTRAST:
#pragma unroll
            for (int j = 0; j < N; ++j) {
                r[j] = imgc_blend((uint32_t)mean, r[j], f); g[j] = imgc_blend((uint32_t)mean, g[j], f);
                b[j] = imgc_blend((uint32_t)mean, b[j], f);
            }
            break;
        case MNAS_IMGC_SATURATION:
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const uint32_t L = imgc_grey(r[j], g[j], b[j]);
                r[j] = imgc_blend(L, r[j], f); g[j] = imgc_blend(L, g[j], f); b[j] = imgc_blend(L, b[j], f);
            }
            break;
        case MNAS_IMGC_HUE:
#pragma unroll
            for (int j = 0; j < N; ++j) imgc_hue(r[j], g[j], b[j], shift, tab);
            break;
        default:                                            // MNAS_IMGC_GRAY
#pragma unroll
            for (int j = 0; j < N; ++j) r[j] = g[j] = b[j] = imgc_grey(r[j], g[j], b[j]);
    }
}

// Mean pass: grid (chunks, n).  partial[img * chunks + chunk] = sum of L over the chunk's pixels after the ops before CONTRAST.
template <bool VEC>
__global__ __launch_bounds__(IMGC_THREADS) void k_img_color_mean(const MnasImgColor* __restrict__ items, int64_t px,
                                                                 int in_layout, const uint8_t* __restrict__ in,
                                                                 uint32_t* __restrict__ partial) {
    __shared__ ImgcTables tab;
    __shared__ uint64_t red[IMGC_THREADS / 64];
    const int tid = threadIdx.x, img = blockIdx.y;
    const MnasImgColor it = items[img];
    if (!imgc_item_ok(it, true)) return;
    int kc = -1, hue = 0;
    for (int k = 0; k < it.nops; ++k) {
        if (it.op[k] == MNAS_IMGC_CONTRAST) kc = k;
        hue |= kc < 0 && it.op[k] == MNAS_IMGC_HUE;
    }
    if (kc < 0) return;
    if (hue) {
        imgc_build_tables(&tab, tid);
        __syncthreads();
    }
    uint32_t sum = 0;                                       // <= 64 pixels x 255
    for (int q = 0; q < IMGC_GROUPS; ++q) {
        const int64_t p0 = ((int64_t)blockIdx.x * IMGC_GROUPS * IMGC_THREADS + q * IMGC_THREADS + tid) * 16;
        if (p0 >= px) break;
        uint32_t r[16], g[16], b[16];
        imgc_load<VEC>(in, in_layout, img, px, p0, r, g, b);
        for (int k = 0; k < kc; ++k) imgc_op<16>(it.op[k], it.factor[k], it.hue_shift, 0, &tab, r, g, b);
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (VEC || p0 + j < px) sum += imgc_grey(r[j], g[j], b[j]);
    }
    const uint64_t s = imgc_block_sum(sum, red, tid);
    if (tid == 0) partial[(int64_t)img * gridDim.x + blockIdx.x] = (uint32_t)s;
}

// Apply pass: grid (chunks, n).  in == out only with equal layouts (each lane reads its pixels before it writes them).
template <bool VEC>
__global__ __launch_bounds__(IMGC_THREADS) void k_img_color(const MnasImgColor* __restrict__ items, int64_t px, int in_layout,
                                                            const uint8_t* in, int out_layout, uint8_t* out,
                                                            const uint32_t* __restrict__ partial) {
    __shared__ ImgcTables tab;
    __shared__ uint64_t red[IMGC_THREADS / 64];
    __shared__ int mean_s;
    const int tid = threadIdx.x, img = blockIdx.y;
    const MnasImgColor it = items[img];
    if (!imgc_item_ok(it, partial != nullptr)) return;
    if (it.nops == 0 && in == out) return;                  // in place, no ops: the image is left alone
    int contrast = 0, hue = 0;
    for (int k = 0; k < it.nops; ++k) {
        contrast |= it.op[k] == MNAS_IMGC_CONTRAST;
        hue |= it.op[k] == MNAS_IMGC_HUE;
    }
    if (hue) imgc_build_tables(&tab, tid);
    int mean = 0;
    if (contrast) {
        uint64_t s = 0;
        const uint32_t* pp = partial + (int64_t)img * gridDim.x;
        for (int i = tid; i < (int)gridDim.x; i += IMGC_THREADS) s += pp[i];
        s = imgc_block_sum(s, red, tid);
        if (tid == 0) mean_s = imgc_contrast_mean(s, px);
    }
    if (hue || contrast) __syncthreads();
    if (contrast) mean = mean_s;
    for (int q = 0; q < IMGC_GROUPS; ++q) {
        const int64_t p0 = ((int64_t)blockIdx.x * IMGC_GROUPS * IMGC_THREADS + q * IMGC_THREADS + tid) * 16;
        if (p0 >= px) break;
        uint32_t r[16], g[16], b[16];
        imgc_load<VEC>(in, in_layout, img, px, p0, r, g, b);
        for (int k = 0; k < it.nops; ++k) imgc_op<16>(it.op[k], it.factor[k], it.hue_shift, mean, &tab, r, g, b);
        imgc_store<VEC>(out, out_layout, img, px, p0, r, g, b);
    }
}

extern "C" int mnas_img_color_check(const MnasImgColor* items_host, int n, int H, int W) {
    if (!imgc_shape_ok(n, H, W) || (n > 0 && items_host == nullptr)) return MNAS_EINVAL;
    for (int i = 0; i < n; ++i)
        if (!imgc_item_ok(items_host[i], true)) return MNAS_EINVAL;
    return MNAS_OK;
}

extern "C" int64_t mnas_img_color_workspace_bytes(int n, int H, int W) {
    if (!imgc_shape_ok(n, H, W)) return -1;
    return (int64_t)n * imgc_chunks(H, W) * 4;
}

extern "C" int mnas_img_color(const MnasImgColor* items, int n, int H, int W, int in_layout, const void* in, int out_layout,
                              void* out, void* workspace, void* stream) {
    if (!imgc_shape_ok(n, H, W)) return MNAS_EINVAL;
    if ((in_layout != MNAS_IMGC_NCHW && in_layout != MNAS_IMGC_NHWC) || (out_layout != MNAS_IMGC_NCHW && out_layout != MNAS_IMGC_NHWC))
        return MNAS_EINVAL;
    if (n == 0) return MNAS_OK;
    if (!items || !in || !out || ((uintptr_t)workspace & 3)) return MNAS_EINVAL;
    const int64_t px = (int64_t)H * W, bytes = (int64_t)n * 3 * px;
    const uintptr_t i0 = (uintptr_t)in, o0 = (uintptr_t)out;
    if (in == out) {
        if (in_layout != out_layout) return MNAS_EINVAL;
    } else if (i0 < o0 + (uintptr_t)bytes && o0 < i0 + (uintptr_t)bytes) {
        return MNAS_EINVAL;                                 // partial overlap
    }
    const bool vec = (px & 15) == 0 && (i0 & 15) == 0 && (o0 & 15) == 0;
    const dim3 grid((unsigned)imgc_chunks(H, W), (unsigned)n);
    const hipStream_t s = (hipStream_t)stream;
    uint32_t* ws = (uint32_t*)workspace;
    if (ws) {
        if (vec)
            hipLaunchKernelGGL(k_img_color_mean<true>, grid, dim3(IMGC_THREADS), 0, s, items, px, in_layout, (const uint8_t*)in, ws);
        else
            hipLaunchKernelGGL(k_img_color_mean<false>, grid, dim3(IMGC_THREADS), 0, s, items, px, in_layout, (const uint8_t*)in, ws);
        MNAS_CHECK_LAUNCH();
    }
    if (vec)
        hipLaunchKernelGGL(k_img_color<true>, grid, dim3(IMGC_THREADS), 0, s, items, px, in_layout, (const uint8_t*)in, out_layout,
                           (uint8_t*)out, (const uint32_t*)ws);
    else
        hipLaunchKernelGGL(k_img_color<false>, grid, dim3(IMGC_THREADS), 0, s, items, px, in_layout, (const uint8_t*)in, out_layout,
                           (uint8_t*)out, (const uint32_t*)ws);
    MNAS_CHECK_LAUNCH();
    return MNAS_OK;
}
