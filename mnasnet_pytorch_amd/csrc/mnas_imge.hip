// Random Erasing on uint8 training batches (include/mnas.h "Random Erasing"): a box of every chosen image of an (n, 3, H, W) NCHW
// batch is overwritten IN PLACE, with one byte per plane (CONST) or with per-pixel noise (NOISE) whose bytes are a pure function of
// (seed, box position, n, c, y, x): Philox4x32-10 (mnas_rng.h) on the counter {x >> 3, y, 3 n + c, position}, 16 bits per pixel, the
// low 12 of them an index into the caller's 3 x 4096-byte quantile table.  tests/erase_ref.py restates it in numpy.
//
// The kernel writes the boxes and nothing else, and reads no byte of x.  grid (3 * bands, n), bands = ceil(H / IMGE_BAND_ROWS):
// one workgroup = one plane of one image x one band of the box's rows (ceil(box rows / bands) of them, so at most IMGE_BAND_ROWS);
// the workgroups of an untouched image, of an empty box and of the bands past the box's last row return after the descriptor read.
// A NOISE workgroup copies its plane's 4096 table bytes into LDS first (one 16-byte load per lane).  One lane = one 16-byte-ALIGNED
// group of one box row, so consecutive lanes store consecutive 16-byte lines whatever x0, W and the base address are: a group wholly
// inside the row is one 16-byte store; a row's first and last group are clipped to the row and go out as aligned 4-byte stores and
// single bytes.  A NOISE group spans two or three Philox blocks of eight pixels (blocks are aligned in x, groups in the address), each
// computed only if one of its pixels is stored; the sixteen table bytes are gathered into two 64-bit words by shifts (no array a
// run-time index would push out of registers).
#include "mnas_common.h"
#include "mnas_rng.h"

#define IMGE_THREADS 256
#define IMGE_BAND_ROWS 64
#define IMGE_TABLE 4096                                    // table bytes per plane

// Shared by the host check and the kernel (which re-checks every descriptor it reads and skips one it would refuse).
__host__ __device__ static inline bool imge_item_ok(const MnasImgErase& t, int H, int W) {
    if (t.mode < MNAS_IMGE_NONE || t.mode > MNAS_IMGE_NOISE || t.pad != 0 || t.reserved[0] != 0 || t.reserved[1] != 0) return false;
    return 0 <= t.y0 && t.y0 <= t.y1 && t.y1 <= H && 0 <= t.x0 && t.x0 <= t.x1 && t.x1 <= W;
}

static inline bool imge_shape_ok(int n, int H, int W) {
    return n >= 0 && n <= 65535 && H >= 1 && W >= 1 && H <= MNAS_IMGX_MAX_OUT && W <= MNAS_IMGX_MAX_OUT;
}

__global__ __launch_bounds__(IMGE_THREADS) void k_img_erase(const MnasImgErase* __restrict__ items, int H, int W, int bands,
                                                            uint8_t* __restrict__ x, const uint8_t* __restrict__ table,
                                                            uint32_t key0, uint32_t key1, uint32_t position) {
    __shared__ __attribute__((aligned(16))) uint8_t tab[IMGE_TABLE];
    const int img = blockIdx.y, c = (int)(blockIdx.x % 3u), band = (int)(blockIdx.x / 3u), tid = threadIdx.x;
    const MnasImgErase it = items[img];
    // every exit below is taken by the whole workgroup
    if (it.mode == MNAS_IMGE_NONE || !imge_item_ok(it, H, W)) return;
    const bool noise = it.mode == MNAS_IMGE_NOISE;
    if (noise && table == nullptr) return;
    const int bh = it.y1 - it.y0, bw = it.x1 - it.x0;
    if (bh == 0 || bw == 0) return;
    const int per_band = (bh + bands - 1) / bands, r0 = band * per_band, rows = min(bh - r0, per_band);
    if (rows <= 0) return;
    if (noise) {
        const uint8_t* src = table + c * IMGE_TABLE;
        if (((uintptr_t)src & 15) == 0) {
            reinterpret_cast<uint4*>(tab)[tid] = reinterpret_cast<const uint4*>(src)[tid];     // IMGE_THREADS * 16 == IMGE_TABLE
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) tab[tid * 16 + j] = src[tid * 16 + j];
        }
        __syncthreads();
    }
    const int groups = (bw + 30) >> 4;                     // the most 16-byte-aligned groups bw bytes can touch
    const int work = rows * groups;
    const uint64_t fill8 = 0x0101010101010101ull * (c == 0 ? it.fill[0] : (c == 1 ? it.fill[1] : it.fill[2]));
    const int64_t plane = (int64_t)(img * 3 + c) * H * W;  // byte offsets from x; x's own low bits join them where alignment is taken
    const int base_lo = (int)((uintptr_t)x & 15);
    for (int i = tid; i < work; i += IMGE_THREADS) {
        const int r = i / groups, s = i - r * groups;
        const int y = it.y0 + r0 + r;
        const int64_t row = plane + (int64_t)y * W + it.x0;                     // the row's first box byte
        const int off = (int)((row + base_lo) & 15);
        const int g0 = 16 * s - off;                       // the group's first byte, counted from the row's first box byte
        const int jlo = max(-g0, 0), jhi = min(bw - g0, 16);                    // the group's bytes [jlo, jhi) lie in the box
        if (jhi <= jlo) continue;
        uint64_t v0 = fill8, v1 = fill8;                   // bytes 0..7 and 8..15 of the group
        if (noise) {
            v0 = v1 = 0ull;
            const int xs = it.x0 + g0;                     // image column of the group's byte 0 (outside [x0, x1) where clipped)
            const int first = (xs + jlo) >> 3, last = (xs + jhi - 1) >> 3;
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const int blk = first + b;
                if (blk > last) continue;
                uint32_t q0 = (uint32_t)blk, q1 = (uint32_t)y, q2 = (uint32_t)(3 * img + c), q3 = position;
                mnas_philox4x32_10_words(q0, q1, q2, q3, key0, key1);
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const int j = blk * 8 + t - xs;
                    if (j < jlo || j >= jhi) continue;
                    const uint32_t word = t < 2 ? q0 : (t < 4 ? q1 : (t < 6 ? q2 : q3));      // t is a constant once unrolled
                    const uint32_t half = (t & 1) ? word >> 16 : word & 0xffffu;
                    const uint64_t byte = tab[half & (IMGE_TABLE - 1)];
                    if (j < 8) v0 |= byte << (8 * j);
                    else v1 |= byte << (8 * (j - 8));
                }
            }
        }
        uint8_t* p = x + (row + g0);                       // 16-byte aligned; only [jlo, jhi) is touched
        if (jlo == 0 && jhi == 16) {
            *reinterpret_cast<uint4*>(p) = make_uint4((uint32_t)v0, (uint32_t)(v0 >> 32), (uint32_t)v1, (uint32_t)(v1 >> 32));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t w = (uint32_t)((k < 2 ? v0 : v1) >> (32 * (k & 1)));
                if (jlo <= 4 * k && 4 * k + 4 <= jhi) {
                    *reinterpret_cast<uint32_t*>(p + 4 * k) = w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (4 * k + e >= jlo && 4 * k + e < jhi) p[4 * k + e] = (uint8_t)(w >> (8 * e));
                }
            }
        }
    }
}

extern "C" void mnas_philox4x32_10(const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    mnas_philox4x32_10_words(c0, c1, c2, c3, key[0], key[1]);
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

extern "C" int mnas_img_erase_check(const MnasImgErase* items_host, int n, int H, int W) {
    if (!imge_shape_ok(n, H, W) || (n > 0 && items_host == nullptr)) return MNAS_EINVAL;
    for (int i = 0; i < n; ++i)
        if (!imge_item_ok(items_host[i], H, W)) return MNAS_EINVAL;
    return MNAS_OK;
}

extern "C" int mnas_img_erase(const MnasImgErase* items, int n, int H, int W, void* x, const void* table, uint64_t seed,
                              uint32_t position, void* stream) {
    if (!imge_shape_ok(n, H, W)) return MNAS_EINVAL;
    if (n == 0) return MNAS_OK;
    if (!items || !x) return MNAS_EINVAL;
    const int bands = (H + IMGE_BAND_ROWS - 1) / IMGE_BAND_ROWS;
    hipLaunchKernelGGL(k_img_erase, dim3((unsigned)(3 * bands), (unsigned)n), dim3(IMGE_THREADS), 0, (hipStream_t)stream, items, H, W,
                       bands, (uint8_t*)x, (const uint8_t*)table, (uint32_t)seed, (uint32_t)(seed >> 32), position);
    MNAS_CHECK_LAUNCH();
    return MNAS_OK;
}
