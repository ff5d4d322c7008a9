// Geometric half of the training input pipeline (include/mnas.h "image batch transform"): decoded HWC uint8 images ->
// crop -> PIL bilinear resize -> window -> flips -> NCHW uint8, byte for byte what
//     PIL.Image.crop(box).resize((rw, rh), Image.BILINEAR)
// produces (Pillow's 8-bit two-pass resampler, Resample.c).  The stem reads the result directly (uint8 + normalise on load).
//
// PIL's arithmetic, per axis (input length `in` = the box's, output length `out`): fp64 coefficients
//     scale = in / out, fs = max(scale, 1), support = fs, center = (xx + 0.5) * scale,
//     xmin = max((int)(center - support + 0.5), 0), xmax = min((int)(center + support + 0.5), in) - xmin,
//     w[x] = tri((x + xmin - center + 0.5) / fs) normalised by their in-order sum, kk[x] = (int)(0.5 + w[x] * 2^22);
// the horizontal pass runs first and clips to uint8 (2^21 + sum p*kk, <= 0 -> 0, >= 2^30 -> 255, else >> 22), the vertical
// pass runs the same way on that intermediate.  Both integer sums are associative (sum kk <= 2^22 + a few, 255 * that + 2^21
// < 2^31), so taps may be accumulated in any order; what must match PIL exactly is the fp64 coefficient arithmetic (no FMA
// contraction: PIL's x86 build has none) and the two clip points.
//
// One workgroup = one image x a band of IMGX_B output rows x a chunk of IMGX_CW output columns (the output size is uniform over
// the batch, so the grid is too).  It builds its columns' and rows' coefficient tables in LDS, then for the source rows its
// band needs: stages the row segments with 16-byte loads, runs the horizontal pass into a uint8 tile in LDS (exactly PIL's
// intermediate, restricted to the chunk's columns), and finally runs the vertical pass from that tile and stores 4-byte
// words per plane with the flips applied as an index mirror.
#include "mnas_common.h"

#define IMGX_CW 64           // output columns per workgroup
#define IMGX_B 16            // output rows per workgroup
#define IMGX_KMAX 65         // taps per output index at the largest supported downscale: 2 * ceil(32) + 1
#define IMGX_HR 72           // rows of the horizontal-pass tile (>= IMGX_KMAX: one output row's window always fits)
#define IMGX_SEG 16384       // bytes of the source-row staging buffer (one row segment needs <= 8.4 KB at 32x)
#define IMGX_THREADS 256

struct ImgxSmem {
    int hk[IMGX_KMAX][IMGX_CW];              // horizontal kk, tap-major: lane = column, conflict-free
    int hx0[IMGX_CW], hn[IMGX_CW];           // horizontal xmin / xmax (crop coordinates)
    int vk[IMGX_B][IMGX_KMAX];               // vertical kk of the band's rows
    int vy0[IMGX_B], vn[IMGX_B];
    uint8_t hbuf[IMGX_HR][3][IMGX_CW];       // horizontal-pass output (uint8), row-major per channel plane
    u32x4_t seg[IMGX_SEG / 16];              // staged source row segments, 16-byte aligned slots
};

// Shared by the host check and the kernel: the kernel re-checks every descriptor it reads (a device copy may differ from the
// checked host copy) and computes nothing for one it would refuse.
__host__ __device__ static inline bool imgx_item_ok(const MnasImgXform& t, int Ho, int Wo, int64_t src_bytes) {
    if (t.src_c != 1 && t.src_c != 3 && t.src_c != 4) return false;
    if (t.src_h < 1 || t.src_w < 1 || t.src_offset < 0 || (int64_t)t.src_stride < (int64_t)t.src_w * t.src_c) return false;
    if ((int64_t)t.src_h > MNAS_IMGX_MAX_DIM || (int64_t)t.src_w > MNAS_IMGX_MAX_DIM) return false;
    if (t.src_offset + (int64_t)(t.src_h - 1) * t.src_stride + (int64_t)t.src_w * t.src_c > src_bytes) return false;
    if (t.box_top < 0 || t.box_left < 0 || t.box_h < 1 || t.box_w < 1) return false;
    if (t.box_h > t.src_h - t.box_top || t.box_w > t.src_w - t.box_left) return false;
    if (t.rh < 1 || t.rw < 1 || t.rh > MNAS_IMGX_MAX_DIM || t.rw > MNAS_IMGX_MAX_DIM) return false;
    if (t.win_top < 0 || t.win_left < 0 || Ho > t.rh - t.win_top || Wo > t.rw - t.win_left) return false;
    if ((int64_t)t.box_h > (int64_t)MNAS_IMGX_MAX_DOWNSCALE * t.rh || (int64_t)t.box_w > (int64_t)MNAS_IMGX_MAX_DOWNSCALE * t.rw)
        return false;
    return (t.flags & ~3) == 0 && t.reserved == 0;
}

static inline bool imgx_shape_ok(int n, int Ho, int Wo, int64_t src_bytes) {
    return n >= 0 && n <= 65535 && Ho >= 1 && Wo >= 1 && Ho <= MNAS_IMGX_MAX_OUT && Wo <= MNAS_IMGX_MAX_OUT &&
           src_bytes >= 16 && (src_bytes & 15) == 0;
}

// Coefficient arithmetic is never contracted into FMAs (PIL's x86 build has none): contract(off) in each function below.
__device__ __forceinline__ double imgx_tri(double x) {
#pragma clang fp contract(off)
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

// PIL precompute_coeffs + normalize_coeffs_8bpc for output index xx of an axis in -> out: kk[x * kstride], x < *n.
// The weights are computed twice (once for their sum, once to normalise) rather than kept in a private array: the same
// expression evaluates to the same double both times.
__device__ __forceinline__ void imgx_coeffs(int in, int out, int xx, int* kk, int kstride, int* xmin_out, int* n_out) {
#pragma clang fp contract(off)
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = fs;                  // bilinear support 1.0 * filterscale
    const double ss = 1.0 / fs;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    if (xmax > IMGX_KMAX) xmax = IMGX_KMAX;     // unreachable for a descriptor imgx_item_ok accepts
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += imgx_tri((x + xmin - center + 0.5) * ss);
    for (int x = 0; x < xmax; ++x) {
        double w = imgx_tri((x + xmin - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        kk[x * kstride] = (int)(0.5 + w * (double)(1 << 22));
    }
    *xmin_out = xmin;
    *n_out = xmax;
}

__device__ __forceinline__ uint32_t imgx_clip8(int v) {
    return v <= 0 ? 0u : (v >= (1 << 30) ? 255u : (uint32_t)(v >> 22));
}

__global__ __launch_bounds__(IMGX_THREADS) void k_img_xform(const MnasImgXform* __restrict__ items, int Ho, int Wo,
                                                            const uint8_t* __restrict__ src, int64_t src_bytes,
                                                            uint8_t* __restrict__ out) {
    __shared__ ImgxSmem sm;
    const int tid = threadIdx.x;
    const int img = blockIdx.z;
    const MnasImgXform it = items[img];
    if (!imgx_item_ok(it, Ho, Wo, src_bytes)) return;
    const int wc0 = blockIdx.x * IMGX_CW, wr0 = blockIdx.y * IMGX_B;      // window coordinates
    const int ncol = min(IMGX_CW, Wo - wc0), nrow = min(IMGX_B, Ho - wr0);
    const int C = it.src_c;

    if (tid < ncol)
        imgx_coeffs(it.box_w, it.rw, it.win_left + wc0 + tid, &sm.hk[0][tid], IMGX_CW, &sm.hx0[tid], &sm.hn[tid]);
    else if (tid >= 64 && tid < 64 + nrow)
        imgx_coeffs(it.box_h, it.rh, it.win_top + wr0 + tid - 64, &sm.vk[tid - 64][0], 1, &sm.vy0[tid - 64], &sm.vn[tid - 64]);
    __syncthreads();

    // the chunk's source columns [sx0, sx1) of the crop (xmin and xmin + xmax grow with the output index)
    const int sx0 = sm.hx0[0], sx1 = sm.hx0[ncol - 1] + sm.hn[ncol - 1];
    const int slot = (15 + (sx1 - sx0) * C + 15) & ~15;                   // bytes per staged row, room for any misalignment
    const int n16 = slot >> 4;
    const int rpf = min(IMGX_SEG / slot, IMGX_HR);                       // >= 1: slot <= 8.4 KB for an accepted descriptor
    if (rpf < 1) return;
    const int64_t base = it.src_offset + (int64_t)it.box_top * it.src_stride + (int64_t)(it.box_left + sx0) * C;
    const int64_t last16 = (src_bytes >> 4) - 1;
    const u32x4_t* __restrict__ src16 = reinterpret_cast<const u32x4_t*>(src);
    const uint8_t* segb = reinterpret_cast<const uint8_t*>(sm.seg);
    const int hflip = it.flags & 1, vflip = (it.flags >> 1) & 1;
    const int c1 = C == 1 ? 0 : 1, c2 = C == 1 ? 0 : 2;                  // grey is replicated to RGB, alpha is dropped

    for (int b0 = 0; b0 < nrow;) {
        // the longest run of output rows [b0, b1) whose source rows [ys, ye) fit the tile
        const int ys = sm.vy0[b0];
        int b1 = b0 + 1;
        while (b1 < nrow && sm.vy0[b1] + sm.vn[b1] - ys <= IMGX_HR) ++b1;
        const int ye = sm.vy0[b1 - 1] + sm.vn[b1 - 1];

        for (int y0 = ys; y0 < ye; y0 += rpf) {
            const int nr = min(rpf, ye - y0);
            // stage rows [y0, y0 + nr): four 16-byte loads in flight per lane, every address clamped into the source buffer
            const int tot = nr * n16;
            for (int i0 = tid; i0 < tot; i0 += 4 * IMGX_THREADS) {
                u32x4_t v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = i0 + j * IMGX_THREADS;
                    if (i < tot) {
                        const int r = i / n16, q = i - r * n16;
                        int64_t c = ((base + (int64_t)(y0 + r) * it.src_stride) >> 4) + q;
                        c = c < 0 ? 0 : (c > last16 ? last16 : c);
                        v[j] = src16[c];
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = i0 + j * IMGX_THREADS;
                    if (i < tot) sm.seg[i] = v[j];
                }
            }
            __syncthreads();
            // horizontal pass: lane = output column, the three channels together
            const int col = tid & (IMGX_CW - 1);
            if (col < ncol) {
                const int xoff = (sm.hx0[col] - sx0) * C, nx = sm.hn[col];
                for (int r = tid >> 6; r < nr; r += IMGX_THREADS / IMGX_CW) {
                    const int lead = (int)((base + (int64_t)(y0 + r) * it.src_stride) & 15);
                    const uint8_t* p = segb + r * slot + lead + xoff;
                    int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
                    for (int x = 0; x < nx; ++x) {
                        const int k = sm.hk[x][col];
                        a0 += (int)p[0] * k;
                        a1 += (int)p[c1] * k;
                        a2 += (int)p[c2] * k;
                        p += C;
                    }
                    uint8_t* h = &sm.hbuf[y0 + r - ys][0][col];
                    h[0] = (uint8_t)imgx_clip8(a0);
                    h[IMGX_CW] = (uint8_t)imgx_clip8(a1);
                    h[2 * IMGX_CW] = (uint8_t)imgx_clip8(a2);
                }
            }
            __syncthreads();
        }

        // vertical pass: one item = 4 consecutive window columns of one (row, channel); stores with the flips mirrored
        for (int i = tid; i < (b1 - b0) * 3 * (IMGX_CW / 4); i += IMGX_THREADS) {
            const int qd = i & (IMGX_CW / 4 - 1), q = i >> 4, ch = q % 3, b = b0 + q / 3;
            const int wc = 4 * qd;
            if (wc >= ncol) continue;
            const uint8_t* h = &sm.hbuf[sm.vy0[b] - ys][ch][wc];
            const int ny = sm.vn[b];
            int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
            for (int y = 0; y < ny; ++y) {
                const uint32_t w4 = *reinterpret_cast<const uint32_t*>(h + y * (3 * IMGX_CW));
                const int k = sm.vk[b][y];
                a0 += (int)(w4 & 255u) * k;
                a1 += (int)((w4 >> 8) & 255u) * k;
                a2 += (int)((w4 >> 16) & 255u) * k;
                a3 += (int)(w4 >> 24) * k;
            }
            const uint32_t v0 = imgx_clip8(a0), v1 = imgx_clip8(a1), v2 = imgx_clip8(a2), v3 = imgx_clip8(a3);
            const int orow = vflip ? Ho - 1 - (wr0 + b) : wr0 + b;
            uint8_t* o = out + ((int64_t)(img * 3 + ch) * Ho + orow) * Wo;
            const int nv = min(4, ncol - wc);
            if (!hflip) {
                const int oc = wc0 + wc;
                if ((Wo & 3) == 0 && nv == 4) {
                    *reinterpret_cast<uint32_t*>(o + oc) = v0 | (v1 << 8) | (v2 << 16) | (v3 << 24);
                } else {
                    o[oc] = (uint8_t)v0;
                    if (nv > 1) o[oc + 1] = (uint8_t)v1;
                    if (nv > 2) o[oc + 2] = (uint8_t)v2;
                    if (nv > 3) o[oc + 3] = (uint8_t)v3;
                }
            } else {
                const int oc = Wo - 1 - (wc0 + wc);                       // output column of window column wc0 + wc
                if ((Wo & 3) == 0 && nv == 4) {
                    *reinterpret_cast<uint32_t*>(o + oc - 3) = v3 | (v2 << 8) | (v1 << 16) | (v0 << 24);
                } else {
                    o[oc] = (uint8_t)v0;
                    if (nv > 1) o[oc - 1] = (uint8_t)v1;
                    if (nv > 2) o[oc - 2] = (uint8_t)v2;
                    if (nv > 3) o[oc - 3] = (uint8_t)v3;
                }
            }
        }
        __syncthreads();                                                  // the tile is refilled for the next run of rows
        b0 = b1;
    }
}

extern "C" int mnas_img_xform_check(const MnasImgXform* items_host, int n, int Ho, int Wo, int64_t src_bytes) {
    if (!imgx_shape_ok(n, Ho, Wo, src_bytes) || (n > 0 && items_host == nullptr)) return MNAS_EINVAL;
    for (int i = 0; i < n; ++i)
        if (!imgx_item_ok(items_host[i], Ho, Wo, src_bytes)) return MNAS_EINVAL;
    return MNAS_OK;
}

extern "C" int mnas_img_xform(const MnasImgXform* items, int n, int Ho, int Wo, const void* src, int64_t src_bytes,
                              void* out_u8_nchw, void* stream) {
    if (!imgx_shape_ok(n, Ho, Wo, src_bytes)) return MNAS_EINVAL;
    if (n == 0) return MNAS_OK;
    if (!items || !src || !out_u8_nchw || ((uintptr_t)src & 15) || ((uintptr_t)out_u8_nchw & 3)) return MNAS_EINVAL;
    const dim3 grid((Wo + IMGX_CW - 1) / IMGX_CW, (Ho + IMGX_B - 1) / IMGX_B, n);
    hipLaunchKernelGGL(k_img_xform, grid, dim3(IMGX_THREADS), 0, (hipStream_t)stream, items, Ho, Wo, (const uint8_t*)src,
                       src_bytes, (uint8_t*)out_u8_nchw);
    MNAS_CHECK_LAUNCH();
    return MNAS_OK;
}
