// What the uint8 image kernels share (mnas_imgc.hip: the photometric ops; mnas_imga.hip: the augmentation-policy ops): the
// workgroup geometry, Pillow's grey and blend arithmetic and its contrast mean, and the 16-pixel load / store of both layouts.
// One copy, so that BRIGHTNESS / COLOR / CONTRAST are the same bytes in both kernels.
#pragma once
#include "mnas_common.h"

#define IMGC_THREADS 256
#define IMGC_GROUPS 4                                      // 16-pixel groups per lane per workgroup
#define IMGC_CHUNK (IMGC_THREADS * IMGC_GROUPS * 16)       // pixels per workgroup (16384)

static inline bool imgc_shape_ok(int n, int H, int W) {
    return n >= 0 && n <= 65535 && H >= 1 && W >= 1 && H <= MNAS_IMGX_MAX_OUT && W <= MNAS_IMGX_MAX_OUT;
}

static inline int64_t imgc_chunks(int H, int W) { return ((int64_t)H * W + IMGC_CHUNK - 1) / IMGC_CHUNK; }

__device__ __forceinline__ uint32_t imgc_grey(uint32_t r, uint32_t g, uint32_t b) {
    return (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16;
}

__device__ __forceinline__ uint32_t imgc_blend(uint32_t a, uint32_t b, float alpha) {
#pragma clang fp contract(off)
    const float t = (float)(int)a + alpha * (float)((int)b - (int)a);
    return t <= 0.f ? 0u : (t >= 255.f ? 255u : (uint32_t)t);
}

__device__ __forceinline__ int imgc_clip8(int v) { return v <= 0 ? 0 : (v < 256 ? v : 255); }

// ImageEnhance.Contrast's degenerate value from the image's grey sum: ImageStat mean (exact sum / count in fp64), int(. + 0.5)
__device__ __forceinline__ int imgc_contrast_mean(uint64_t grey_sum, int64_t px) {
#pragma clang fp contract(off)
    return (int)((double)grey_sum / (double)px + 0.5);
}

// 16 pixels [p0, p0 + 16) of image img (px pixels per plane) into r/g/b (VEC: 16-byte loads; else byte loads of those < px)
template <bool VEC>
__device__ __forceinline__ void imgc_load(const uint8_t* in, int layout, int img, int64_t px, int64_t p0, uint32_t (&r)[16],
                                          uint32_t (&g)[16], uint32_t (&b)[16]) {
    if (VEC) {
        uint4 w[3];
        if (layout == MNAS_IMGC_NCHW) {
#pragma unroll
            for (int c = 0; c < 3; ++c) w[c] = *reinterpret_cast<const uint4*>(in + ((int64_t)img * 3 + c) * px + p0);
            const uint32_t* u = reinterpret_cast<const uint32_t*>(w);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                r[j] = (u[j >> 2] >> (8 * (j & 3))) & 255u;
                g[j] = (u[4 + (j >> 2)] >> (8 * (j & 3))) & 255u;
                b[j] = (u[8 + (j >> 2)] >> (8 * (j & 3))) & 255u;
            }
        } else {
            const uint4* s = reinterpret_cast<const uint4*>(in + ((int64_t)img * px + p0) * 3);
#pragma unroll
            for (int c = 0; c < 3; ++c) w[c] = s[c];
            const uint32_t* u = reinterpret_cast<const uint32_t*>(w);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                r[j] = (u[(3 * j) >> 2] >> (8 * ((3 * j) & 3))) & 255u;
                g[j] = (u[(3 * j + 1) >> 2] >> (8 * ((3 * j + 1) & 3))) & 255u;
                b[j] = (u[(3 * j + 2) >> 2] >> (8 * ((3 * j + 2) & 3))) & 255u;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            r[j] = g[j] = b[j] = 0u;
            if (p0 + j < px) {
                if (layout == MNAS_IMGC_NCHW) {
                    const uint8_t* s = in + (int64_t)img * 3 * px + p0 + j;
                    r[j] = s[0]; g[j] = s[px]; b[j] = s[2 * px];
                } else {
                    const uint8_t* s = in + ((int64_t)img * px + p0 + j) * 3;
                    r[j] = s[0]; g[j] = s[1]; b[j] = s[2];
                }
            }
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void imgc_store(uint8_t* out, int layout, int img, int64_t px, int64_t p0, const uint32_t (&r)[16],
                                           const uint32_t (&g)[16], const uint32_t (&b)[16]) {
    if (VEC) {
        uint32_t u[12];
        if (layout == MNAS_IMGC_NCHW) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                u[q] = r[4 * q] | (r[4 * q + 1] << 8) | (r[4 * q + 2] << 16) | (r[4 * q + 3] << 24);
                u[4 + q] = g[4 * q] | (g[4 * q + 1] << 8) | (g[4 * q + 2] << 16) | (g[4 * q + 3] << 24);
                u[8 + q] = b[4 * q] | (b[4 * q + 1] << 8) | (b[4 * q + 2] << 16) | (b[4 * q + 3] << 24);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
                *reinterpret_cast<uint4*>(out + ((int64_t)img * 3 + c) * px + p0) =
                    make_uint4(u[4 * c], u[4 * c + 1], u[4 * c + 2], u[4 * c + 3]);
        } else {
#pragma unroll
            for (int q = 0; q < 12; ++q) u[q] = 0u;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                u[(3 * j) >> 2] |= r[j] << (8 * ((3 * j) & 3));
                u[(3 * j + 1) >> 2] |= g[j] << (8 * ((3 * j + 1) & 3));
                u[(3 * j + 2) >> 2] |= b[j] << (8 * ((3 * j + 2) & 3));
            }
            uint4* d = reinterpret_cast<uint4*>(out + ((int64_t)img * px + p0) * 3);
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] = make_uint4(u[4 * c], u[4 * c + 1], u[4 * c + 2], u[4 * c + 3]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (p0 + j < px) {
                if (layout == MNAS_IMGC_NCHW) {
                    uint8_t* d = out + (int64_t)img * 3 * px + p0 + j;
                    d[0] = (uint8_t)r[j]; d[px] = (uint8_t)g[j]; d[2 * px] = (uint8_t)b[j];
                } else {
                    uint8_t* d = out + ((int64_t)img * px + p0 + j) * 3;
                    d[0] = (uint8_t)r[j]; d[1] = (uint8_t)g[j]; d[2] = (uint8_t)b[j];
                }
            }
        }
    }
}

__device__ __forceinline__ uint64_t imgc_block_sum(uint64_t v, uint64_t* red, int tid) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    uint64_t s = 0;
#pragma unroll
    for (int w = 0; w < IMGC_THREADS / 64; ++w) s += red[w];
    return s;
}
