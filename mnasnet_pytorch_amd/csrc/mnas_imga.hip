// Augmentation-policy ops of the training input pipeline (include/mnas.h "augmentation-policy ops"): per image a chain of up to
// four ops -- nearest-neighbour affine warp, brightness / color / contrast / sharpness blends, posterize, solarize, invert,
// autocontrast, equalize -- on the (n, 3, H, W) uint8 NCHW batch, byte for byte what Pillow computes (tests/randaug_ref.py holds
// the restatement to Pillow).  The blends, the grey and the contrast mean are mnas_imgc.h's, shared with mnas_imgc.hip.
//
// Stages.  An op may read pixels other than its own (AFFINE, SHARPNESS) or statistics of the whole image (CONTRAST, AUTOCONTRAST,
// EQUALIZE), so a chain is not fused: stage s of S = max(1, longest chain) is one launch that applies one op per image out of
// place, from the previous stage's buffer into the other of {out, workspace}, ordered so that the last stage writes out.  Chains
// are right-aligned: an image of L ops sits out the first S - L stages and reads `in` in its first one, so every image's last op
// lands in out and no stage copies for the sake of a shorter chain.  One workgroup = one image x one chunk of IMGC_CHUNK pixels,
// one lane = IMGC_GROUPS groups of 16 consecutive pixels; the op is uniform over the workgroup.  Pointwise ops move 16 bytes per
// plane and group (H*W % 16 == 0, aligned buffers) or single bytes; AFFINE and SHARPNESS gather bytes and store the same way.
//
// Statistics.  A stage in which some image has a statistics op is preceded by k_img_aug_stats over that stage's input: per
// (image, chunk) a partial table of IMGA_PART uint32 in the workspace -- 3 x 256 counts from one LDS histogram per wave (LDS
// atomics; counts are integers, so the order is immaterial), or the chunk's grey sum for CONTRAST.  The apply launch adds an
// image's partials in chunk order and builds its mean or its 3 x 256 byte table in LDS.  No global atomics: same bytes every run.
#include "mnas_imgc.h"

#define IMGA_PART 769                                      // uint32 per (image, chunk): 3 x 256 counts, then the grey sum
#define IMGA_WAVES (IMGC_THREADS / MNAS_WAVE)

__host__ __device__ static inline bool imga_is_stats(int op) {
    return op == MNAS_IMGA_CONTRAST || op == MNAS_IMGA_AUTOCONTRAST || op == MNAS_IMGA_EQUALIZE;
}

// stages an item takes part in: an empty chain is one IDENTITY
__host__ __device__ static inline int imga_len(const MnasImgAug& t) { return t.nops > 0 ? t.nops : 1; }

// a1 == a3 == 0: only a whole-pixel translation at unit scale; both source coordinates inside (-2^31, 2^31) at the four corners
// x in {0, W}, y in {0, H} (they are linear in x and y, so over the whole image: the int32 arithmetic below cannot overflow)
__host__ __device__ static inline bool imga_affine_ok(const int32_t* a, int H, int W) {
    if (a[1] == 0 && a[3] == 0 && (a[0] != 65536 || a[4] != 65536 || (a[2] & 0xffff) != 0x8000 || (a[5] & 0xffff) != 0x8000))
        return false;
    const int64_t lim = (int64_t)1 << 31;
    for (int k = 0; k < 4; ++k) {
        const int64_t x = (k & 1) ? W : 0, y = (k & 2) ? H : 0;
        const int64_t xv = (int64_t)a[2] + x * a[0] + y * a[1], yv = (int64_t)a[5] + x * a[3] + y * a[4];
        if (xv <= -lim || xv >= lim || yv <= -lim || yv >= lim) return false;
    }
    return true;
}

// Shared by the host check (S = MNAS_IMGA_MAX_OPS, every stage's statistics allowed) and the kernels, which re-check every
// descriptor they read and skip one they would refuse.  S: stages of the launch; stats_stages: stages with a statistics launch.
__host__ __device__ static inline bool imga_item_ok(const MnasImgAug& t, int H, int W, int S, int stats_stages) {
    if (t.nops < 0 || t.nops > MNAS_IMGA_MAX_OPS || t.reserved != 0 || imga_len(t) > S) return false;
    for (int k = 0; k < t.nops; ++k) {
        const int op = t.op[k];
        if (op < MNAS_IMGA_IDENTITY || op > MNAS_IMGA_EQUALIZE) return false;
        if (op >= MNAS_IMGA_BRIGHTNESS && op <= MNAS_IMGA_SHARPNESS && !(t.factor[k] >= 0.f && t.factor[k] <= 3.402823466e38f))
            return false;                                   // NaN, inf and negatives fail
        if (op == MNAS_IMGA_POSTERIZE && (t.arg[k][0] < 1 || t.arg[k][0] > 8)) return false;
        if (op == MNAS_IMGA_SOLARIZE && (t.arg[k][0] < 0 || t.arg[k][0] > 256)) return false;
        if (op == MNAS_IMGA_AFFINE && !imga_affine_ok(t.arg[k], H, W)) return false;
        if (imga_is_stats(op) && !((stats_stages >> (S - t.nops + k)) & 1)) return false;
    }
    return true;
}

static inline int64_t imga_batch_bytes(int n, int H, int W) { return (((int64_t)n * 3 * H * W) + 15) & ~(int64_t)15; }

// Statistics of stage `stage`: grid (chunks, n).  part[0..767] = the chunk's per-channel counts (AUTOCONTRAST, EQUALIZE) or
// part[768] = its grey sum (CONTRAST); an image whose op of this stage needs neither is left alone.
template <bool VEC>
__global__ __launch_bounds__(IMGC_THREADS) void k_img_aug_stats(const MnasImgAug* __restrict__ items, int H, int W, int stage, int S,
                                                                int stats_stages, const uint8_t* __restrict__ in,
                                                                const uint8_t* __restrict__ src, uint32_t* __restrict__ partial) {
    __shared__ uint32_t hist[IMGA_WAVES][768];
    __shared__ uint64_t red[IMGA_WAVES];
    const int tid = threadIdx.x, img = blockIdx.y;
    const int64_t px = (int64_t)H * W;
    const MnasImgAug& it = items[img];
    if (!imga_item_ok(it, H, W, S, stats_stages)) return;
    const int k = stage - (S - imga_len(it));
    if (k < 0 || it.nops == 0 || !imga_is_stats(it.op[k])) return;
    const uint8_t* s = k == 0 ? in : src;
    uint32_t* part = partial + ((int64_t)img * gridDim.x + blockIdx.x) * IMGA_PART;
    const bool grey = it.op[k] == MNAS_IMGA_CONTRAST;
    uint32_t* h = hist[tid >> 6];
    if (!grey) {
        for (int i = tid; i < IMGA_WAVES * 768; i += IMGC_THREADS) (&hist[0][0])[i] = 0u;
        __syncthreads();
    }
    uint32_t sum = 0;                                       // <= 64 pixels x 255
    for (int q = 0; q < IMGC_GROUPS; ++q) {
        const int64_t p0 = ((int64_t)blockIdx.x * IMGC_GROUPS * IMGC_THREADS + q * IMGC_THREADS + tid) * 16;
        if (p0 >= px) break;
        uint32_t r[16], g[16], b[16];
        imgc_load<VEC>(s, MNAS_IMGC_NCHW, img, px, p0, r, g, b);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (VEC || p0 + j < px) {
                if (grey) {
                    sum += imgc_grey(r[j], g[j], b[j]);
                } else {
                    atomicAdd(&h[r[j]], 1u);
                    atomicAdd(&h[256 + g[j]], 1u);
                    atomicAdd(&h[512 + b[j]], 1u);
                }
            }
        }
    }
    if (grey) {
        const uint64_t t = imgc_block_sum(sum, red, tid);
        if (tid == 0) part[768] = (uint32_t)t;
        return;
    }
    __syncthreads();
    for (int i = tid; i < 768; i += IMGC_THREADS) {
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < IMGA_WAVES; ++w) v += hist[w][i];
        part[i] = v;
    }
}

// The 3 x 256 byte table of AUTOCONTRAST / EQUALIZE from an image's partial counts.  cnt: 768 uint32 of LDS work space.
__device__ __forceinline__ void imga_build_lut(int op, const uint32_t* __restrict__ part, int chunks, uint32_t* cnt, int (*info)[4],
                                               uint8_t* lut, int tid) {
    for (int i = tid; i < 768; i += IMGC_THREADS) {
        uint32_t v = 0;
        for (int c = 0; c < chunks; ++c) v += part[(int64_t)c * IMGA_PART + i];
        cnt[i] = v;
    }
    __syncthreads();
    if (tid < 3) {
        // one lane per channel: first / last value present, bins present, and the counts turned into the sum of the bins below
        uint32_t* h = cnt + tid * 256;
        int lo = 256, hi = -1, bins = 0;
        uint32_t run = 0, last = 0;
        for (int i = 0; i < 256; ++i) {
            const uint32_t v = h[i];
            if (v) {
                if (lo == 256) lo = i;
                hi = i;
                last = v;
                ++bins;
            }
            h[i] = run;
            run += v;
        }
        info[tid][0] = lo;
        info[tid][1] = hi;
        info[tid][2] = bins > 1 ? (int)((run - last) / 255u) : 0;      // equalize's step; 0: the table is the identity
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int v = tid;
        if (op == MNAS_IMGA_AUTOCONTRAST) {
#pragma clang fp contract(off)
            const int lo = info[c][0], hi = info[c][1];
            if (hi > lo) {
                const double scale = 255.0 / (double)(hi - lo);
                const double offset = (double)(-lo) * scale;
                v = imgc_clip8((int)((double)tid * scale + offset));
            }
        } else {
            const uint32_t step = (uint32_t)info[c][2];
            if (step) v = (int)min(255u, (step / 2u + cnt[c * 256 + tid]) / step);
        }
        lut[c * 256 + tid] = (uint8_t)v;
    }
    __syncthreads();
}

// SHARPNESS on 16 aligned pixels [x0, x0 + 16) of one plane's interior row when W % 16 == 0 (t: the byte at (y, x0); v: the row's
// bytes, already loaded): rows y - 1 and y + 1 come as one 16-byte load each and the columns either side as single bytes, instead
// of nine byte loads per pixel; SMOOTH from the 18 column sums.
__device__ __forceinline__ void imga_sharpen16(const uint8_t* t, int W, int x0, float f, uint32_t (&v)[16]) {
    const uint4 up = *reinterpret_cast<const uint4*>(t - W), dn = *reinterpret_cast<const uint4*>(t + W);
    const uint32_t u[4] = {up.x, up.y, up.z, up.w}, d[4] = {dn.x, dn.y, dn.z, dn.w};
    uint32_t col[18];
    col[0] = x0 > 0 ? (uint32_t)t[-W - 1] + t[-1] + t[W - 1] : 0u;
    col[17] = x0 + 16 < W ? (uint32_t)t[-W + 16] + t[16] + t[W + 16] : 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j) col[j + 1] = ((u[j >> 2] >> (8 * (j & 3))) & 255u) + v[j] + ((d[j >> 2] >> (8 * (j & 3))) & 255u);
    uint32_t o[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t sum = col[j] + col[j + 1] + col[j + 2] + 4u * v[j];
        o[j] = (x0 + j >= 1 && x0 + j < W - 1) ? imgc_blend((2u * sum + 13u) / 26u, v[j], f) : v[j];
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = o[j];
}

// Stage `stage`: grid (chunks, n).  src: the previous stage's buffer (an image in its first stage reads `in` instead).
template <bool VEC>
__global__ __launch_bounds__(IMGC_THREADS) void k_img_aug(const MnasImgAug* __restrict__ items, int H, int W, int stage, int S,
                                                          int stats_stages, int fill, const uint8_t* __restrict__ in,
                                                          const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                          const uint32_t* __restrict__ partial) {
    __shared__ uint32_t cnt[768];
    __shared__ uint8_t lut[768];
    __shared__ int info[3][4];
    __shared__ uint64_t red[IMGA_WAVES];
    __shared__ int mean_s;
    const int tid = threadIdx.x, img = blockIdx.y;
    const int64_t px = (int64_t)H * W;
    const MnasImgAug& it = items[img];
    if (!imga_item_ok(it, H, W, S, stats_stages)) return;
    const int k = stage - (S - imga_len(it));
    if (k < 0) return;                                      // a shorter chain: not started yet
    const int op = it.nops == 0 ? MNAS_IMGA_IDENTITY : it.op[k];
    const float f = it.factor[k];
    const uint8_t* s = k == 0 ? in : src;
    const uint32_t* part = partial + (int64_t)img * gridDim.x * IMGA_PART;
    int mean = 0;
    if (op == MNAS_IMGA_CONTRAST) {
        uint64_t t = 0;
        for (int i = tid; i < (int)gridDim.x; i += IMGC_THREADS) t += part[(int64_t)i * IMGA_PART + 768];
        t = imgc_block_sum(t, red, tid);
        if (tid == 0) mean_s = imgc_contrast_mean(t, px);
        __syncthreads();
        mean = mean_s;
    } else if (op == MNAS_IMGA_AUTOCONTRAST || op == MNAS_IMGA_EQUALIZE) {
        imga_build_lut(op, part, (int)gridDim.x, cnt, info, lut, tid);
    }
    const int a0 = it.arg[k][0], a1 = it.arg[k][1], a2 = it.arg[k][2], a3 = it.arg[k][3], a4 = it.arg[k][4], a5 = it.arg[k][5];
    const uint32_t fr = fill & 255, fg = (fill >> 8) & 255, fb = (fill >> 16) & 255;
    const uint8_t* plane = s + (int64_t)img * 3 * px;
    for (int q = 0; q < IMGC_GROUPS; ++q) {
        const int64_t p0 = ((int64_t)blockIdx.x * IMGC_GROUPS * IMGC_THREADS + q * IMGC_THREADS + tid) * 16;
        if (p0 >= px) break;
        uint32_t r[16], g[16], b[16];
        if (op != MNAS_IMGA_AFFINE) imgc_load<VEC>(s, MNAS_IMGC_NCHW, img, px, p0, r, g, b);
        int y = (int)(p0 / W), x = (int)(p0 - (int64_t)y * W);         // of pixel p0 + j below (AFFINE, SHARPNESS)
        switch (op) {
            case MNAS_IMGA_AFFINE:
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    r[j] = fr; g[j] = fg; b[j] = fb;
                    if (VEC || p0 + j < px) {
                        const int xin = (a2 + x * a0 + y * a1) >> 16, yin = (a5 + x * a3 + y * a4) >> 16;
                        if (xin >= 0 && xin < W && yin >= 0 && yin < H) {
                            const uint8_t* t = plane + (int64_t)yin * W + xin;
                            r[j] = t[0]; g[j] = t[px]; b[j] = t[2 * px];
                        }
                    }
                    if (++x == W) { x = 0; ++y; }
                }
                break;
            case MNAS_IMGA_BRIGHTNESS:
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    r[j] = imgc_blend(0u, r[j], f); g[j] = imgc_blend(0u, g[j], f); b[j] = imgc_blend(0u, b[j], f);
                }
                break;
            case MNAS_IMGA_COLOR:
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const uint32_t L = imgc_grey(r[j], g[j], b[j]);
                    r[j] = imgc_blend(L, r[j], f); g[j] = imgc_blend(L, g[j], f); b[j] = imgc_blend(L, b[j], f);
                }
                break;
            case MNAS_IMGA_CONTRAST:
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    r[j] = imgc_blend((uint32_t)mean, r[j], f); g[j] = imgc_blend((uint32_t)mean, g[j], f);
                    b[j] = imgc_blend((uint32_t)mean, b[j], f);
                }
                break;
            case MNAS_IMGA_SHARPNESS:
                if (VEC && (W & 15) == 0) {                 // the group is 16 aligned pixels of row y
                    if (y >= 1 && y < H - 1) {
                        const uint8_t* t = plane + (int64_t)y * W + x;
                        imga_sharpen16(t, W, x, f, r);
                        imga_sharpen16(t + px, W, x, f, g);
                        imga_sharpen16(t + 2 * px, W, x, f, b);
                    }
                    break;
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    // SMOOTH: interior pixels of an image with both sides >= 3; elsewhere it is the pixel itself, and so is the blend
                    if ((VEC || p0 + j < px) && x >= 1 && x < W - 1 && y >= 1 && y < H - 1) {
                        const uint8_t* t = plane + (int64_t)y * W + x;
                        uint32_t sm[3];
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const uint8_t* u = t + c * px;
                            const uint32_t sum = (uint32_t)u[-W - 1] + u[-W] + u[-W + 1] + u[-1] + 5u * u[0] + u[1] + u[W - 1] + u[W] +
                                                 u[W + 1];
                            sm[c] = (2u * sum + 13u) / 26u;
                        }
                        r[j] = imgc_blend(sm[0], r[j], f); g[j] = imgc_blend(sm[1], g[j], f); b[j] = imgc_blend(sm[2], b[j], f);
                    }
                    if (++x == W) { x = 0; ++y; }
                }
                break;
            case MNAS_IMGA_POSTERIZE: {
                const uint32_t mask = ~((1u << (8 - a0)) - 1u) & 255u;
#pragma unroll
                for (int j = 0; j < 16; ++j) { r[j] &= mask; g[j] &= mask; b[j] &= mask; }
                break;
            }
            case MNAS_IMGA_SOLARIZE:
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    r[j] = (int)r[j] < a0 ? r[j] : 255u - r[j]; g[j] = (int)g[j] < a0 ? g[j] : 255u - g[j];
                    b[j] = (int)b[j] < a0 ? b[j] : 255u - b[j];
                }
                break;
            case MNAS_IMGA_INVERT:
#pragma unroll
                for (int j = 0; j < 16; ++j) { r[j] = 255u - r[j]; g[j] = 255u - g[j]; b[j] = 255u - b[j]; }
                break;
            case MNAS_IMGA_AUTOCONTRAST:
            case MNAS_IMGA_EQUALIZE:
#pragma unroll
                for (int j = 0; j < 16; ++j) { r[j] = lut[r[j]]; g[j] = lut[256 + g[j]]; b[j] = lut[512 + b[j]]; }
                break;
            default:                                        // MNAS_IMGA_IDENTITY
                break;
        }
        imgc_store<VEC>(dst, MNAS_IMGC_NCHW, img, px, p0, r, g, b);
    }
}

extern "C" int mnas_img_aug_check(const MnasImgAug* items_host, int n, int H, int W) {
    if (!imgc_shape_ok(n, H, W) || (n > 0 && items_host == nullptr)) return MNAS_EINVAL;
    for (int i = 0; i < n; ++i)
        if (!imga_item_ok(items_host[i], H, W, MNAS_IMGA_MAX_OPS, ~0)) return MNAS_EINVAL;
    return MNAS_OK;
}

extern "C" int64_t mnas_img_aug_workspace_bytes(int n, int H, int W, int max_ops, int need_stats) {
    if (!imgc_shape_ok(n, H, W) || max_ops < 0 || max_ops > MNAS_IMGA_MAX_OPS) return -1;
    return (max_ops >= 2 ? imga_batch_bytes(n, H, W) : 0) + (need_stats ? (int64_t)n * imgc_chunks(H, W) * IMGA_PART * 4 : 0);
}

extern "C" int mnas_img_aug(const MnasImgAug* items, int n, int H, int W, int max_ops, int stats_stages, int fill_rgb, const void* in,
                            void* out, void* workspace, void* stream) {
    if (!imgc_shape_ok(n, H, W) || max_ops < 0 || max_ops > MNAS_IMGA_MAX_OPS) return MNAS_EINVAL;
    const int S = max_ops > 0 ? max_ops : 1;
    if (fill_rgb < 0 || fill_rgb > 0xffffff || (stats_stages & ~((1 << S) - 1))) return MNAS_EINVAL;
    if (n == 0) return MNAS_OK;
    const int64_t px = (int64_t)H * W, bytes = (int64_t)n * 3 * px;
    const int64_t ws_bytes = mnas_img_aug_workspace_bytes(n, H, W, max_ops, stats_stages != 0);
    if (!items || !in || !out || (ws_bytes > 0 && !workspace) || ((uintptr_t)workspace & 15)) return MNAS_EINVAL;
    const uintptr_t i0 = (uintptr_t)in, o0 = (uintptr_t)out, w0 = (uintptr_t)workspace;
    if (i0 < o0 + (uintptr_t)bytes && o0 < i0 + (uintptr_t)bytes) return MNAS_EINVAL;                       // in / out overlap
    if (ws_bytes > 0 && ((i0 < w0 + (uintptr_t)ws_bytes && w0 < i0 + (uintptr_t)bytes) ||
                         (o0 < w0 + (uintptr_t)ws_bytes && w0 < o0 + (uintptr_t)bytes)))
        return MNAS_EINVAL;
    uint8_t* ping = (uint8_t*)workspace;                    // the spare batch (S >= 2), then the partial tables
    uint32_t* partial = (uint32_t*)((uint8_t*)workspace + (S >= 2 ? imga_batch_bytes(n, H, W) : 0));
    const bool vec = (px & 15) == 0 && (i0 & 15) == 0 && (o0 & 15) == 0;
    const dim3 grid((unsigned)imgc_chunks(H, W), (unsigned)n);
    const hipStream_t st = (hipStream_t)stream;
    const uint8_t* src = (const uint8_t*)in;
    for (int s = 0; s < S; ++s) {
        uint8_t* dst = ((S - 1 - s) & 1) ? ping : (uint8_t*)out;
        if ((stats_stages >> s) & 1) {
            if (vec)
                hipLaunchKernelGGL(k_img_aug_stats<true>, grid, dim3(IMGC_THREADS), 0, st, items, H, W, s, S, stats_stages,
                                   (const uint8_t*)in, src, partial);
            else
                hipLaunchKernelGGL(k_img_aug_stats<false>, grid, dim3(IMGC_THREADS), 0, st, items, H, W, s, S, stats_stages,
                                   (const uint8_t*)in, src, partial);
            MNAS_CHECK_LAUNCH();
        }
        if (vec)
            hipLaunchKernelGGL(k_img_aug<true>, grid, dim3(IMGC_THREADS), 0, st, items, H, W, s, S, stats_stages, fill_rgb,
                               (const uint8_t*)in, src, dst, (const uint32_t*)partial);
        else
            hipLaunchKernelGGL(k_img_aug<false>, grid, dim3(IMGC_THREADS), 0, st, items, H, W, s, S, stats_stages, fill_rgb,
                               (const uint8_t*)in, src, dst, (const uint32_t*)partial);
        MNAS_CHECK_LAUNCH();
        src = dst;
    }
    return MNAS_OK;
}
