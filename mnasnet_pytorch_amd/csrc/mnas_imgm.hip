// Batch mixing on uint8 training batches (include/mnas.h "batch mixing"): Mixup and CutMix of every image with a partner image
// of the same batch, (n, 3, H, W) NCHW in, the same layout out -- what the stem's uint8 input path reads, so a mixed batch
// never becomes a float batch and never visits the host.
//
//   NONE    out = x
//   MIXUP   out = (w x + (65536 - w) partner + 32768) >> 16 per byte, w = w16 in [0, 65536]: integer arithmetic, so the result is
//           defined byte for byte (tests/mix_ref.py restates it in numpy); its distance from the real-valued blend is <= 0.5
//   CUTMIX  out = partner inside rows [y0, y1) x columns [x0, x1), x elsewhere
//
// Out of place only: `partner` is any index of the batch, so a pass in place would read bytes it has already overwritten.
// One launch, a pure stream.  An image is one run of 3*H*W bytes (its three planes behind one another; MIXUP and NONE do not
// care where a plane ends); one workgroup = one image x one chunk of IMGM_CHUNK bytes; one lane = IMGM_GROUPS groups of 16
// consecutive bytes, each moved with one 16-byte load per operand and one 16-byte store when H*W % 16 == 0 and both buffers
// are 16-byte aligned (every image and plane then starts on a 16-byte boundary), byte by byte otherwise.  A CUTMIX group builds a
// byte mask -- the columns [x0, x1) clipped to the group when the group lies inside one row, byte by byte when it runs over a row
// end -- and selects through it: a box edge inside a group costs nothing extra and no lane leaves the common path; a group
// wholly outside the box does not load its partner bytes.  A lane issues the loads of all its groups before it uses the first.
#include "mnas_common.h"

#define IMGM_THREADS 256
#define IMGM_GROUPS 4                                      // 16-byte groups per lane per workgroup
#define IMGM_CHUNK (IMGM_THREADS * IMGM_GROUPS * 16)       // bytes per workgroup (16384)

// Shared by the host check and the kernel (which re-checks every descriptor it reads and skips one it would refuse).
__host__ __device__ static inline bool imgm_item_ok(const MnasImgMix& t, int n, int H, int W) {
    if (t.mode < MNAS_IMGM_NONE || t.mode > MNAS_IMGM_CUTMIX || t.reserved != 0) return false;
    if (t.partner < 0 || t.partner >= n || t.w16 < 0 || t.w16 > 65536) return false;
    return 0 <= t.y0 && t.y0 <= t.y1 && t.y1 <= H && 0 <= t.x0 && t.x0 <= t.x1 && t.x1 <= W;
}

static inline bool imgm_shape_ok(int n, int H, int W) {
    return n >= 0 && n <= 65535 && H >= 1 && W >= 1 && H <= MNAS_IMGX_MAX_OUT && W <= MNAS_IMGX_MAX_OUT;   // 3*H*W < 2^31
}

// four bytes of x against four of the partner
__device__ __forceinline__ uint32_t imgm_blend4(uint32_t a, uint32_t b, uint32_t w) {
    uint32_t r = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t xa = (a >> (8 * k)) & 255u, xb = (b >> (8 * k)) & 255u;
        r |= ((w * xa + (65536u - w) * xb + 32768u) >> 16) << (8 * k);       // <= 255 * 65536 + 32768: no overflow, result <= 255
    }
    return r;
}

// 16 bytes [q0, q0 + 16) of a run of `total` bytes as four words (VEC: one 16-byte load; else byte loads of those < total)
template <bool VEC>
__device__ __forceinline__ void imgm_load(const uint8_t* s, int q0, int total, uint32_t (&v)[4]) {
    if (VEC) {
        const uint4 t = *reinterpret_cast<const uint4*>(s + q0);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = 0u;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (q0 + j < total) v[j >> 2] |= (uint32_t)s[q0 + j] << (8 * (j & 3));
    }
}

// bytes [lo, hi) of a 16-byte group as four word masks, 0 <= lo, hi <= 16
__device__ __forceinline__ void imgm_range_mask(int lo, int hi, uint32_t (&m)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int a = min(max(lo - 4 * k, 0), 4), b = min(max(hi - 4 * k, 0), 4);
        const uint32_t upto_b = b >= 4 ? 0xffffffffu : (1u << (8 * b)) - 1u, upto_a = a >= 4 ? 0xffffffffu : (1u << (8 * a)) - 1u;
        m[k] = b > a ? upto_b & ~upto_a : 0u;
    }
}

// which bytes of the group at byte q0 of an image lie inside the box: (plane, row, column) of q0 without an integer division (the
// plane by two compares, the row from an fp32 quotient that is at most one off and is corrected), then one range per group when
// the group stays inside its row, byte by byte when it runs over a row end (or, on the byte path, into the next plane)
__device__ __forceinline__ bool imgm_box_mask(const MnasImgMix& it, int q0, int px, int H, int W, uint32_t (&m)[4]) {
    const int p = q0 - (q0 >= 2 * px ? 2 * px : (q0 >= px ? px : 0));
    int y = (int)__fdividef((float)p, (float)W), x = p - y * W;
    while (x < 0) { x += W; --y; }
    while (x >= W) { x -= W; ++y; }
    if (x + 16 <= W) {
        const bool row_in = y >= it.y0 && y < it.y1;
        imgm_range_mask(row_in ? min(max(it.x0 - x, 0), 16) : 0, row_in ? min(max(it.x1 - x, 0), 16) : 0, m);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = 0u;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const bool inside = y >= it.y0 && y < it.y1 && x >= it.x0 && x < it.x1;
            m[j >> 2] |= inside ? 255u << (8 * (j & 3)) : 0u;
            if (++x == W) {
                x = 0;
                if (++y == H) y = 0;
            }
        }
    }
    return ((m[0] | m[1]) | (m[2] | m[3])) != 0u;
}

// grid (chunks of 3*H*W, n).  All of a lane's loads are issued before the first of them is used.
template <bool VEC>
__global__ __launch_bounds__(IMGM_THREADS) void k_img_mix(const MnasImgMix* __restrict__ items, int n, int H, int W,
                                                          const uint8_t* __restrict__ in, uint8_t* __restrict__ out) {
    const int img = blockIdx.y, tid = threadIdx.x;
    const MnasImgMix it = items[img];
    if (!imgm_item_ok(it, n, H, W)) return;
    const int px = H * W, total = 3 * px;
    const uint8_t* xs = in + (int64_t)img * total;
    const uint8_t* ps = in + (int64_t)it.partner * total;
    uint8_t* d = out + (int64_t)img * total;
    const uint32_t w = (uint32_t)it.w16;
    const int base = ((int)blockIdx.x * IMGM_GROUPS * IMGM_THREADS + tid) * 16;
    uint32_t a[IMGM_GROUPS][4], b[IMGM_GROUPS][4], m[IMGM_GROUPS][4];
    bool need[IMGM_GROUPS];
#pragma unroll
    for (int g = 0; g < IMGM_GROUPS; ++g) {
        const int q0 = base + g * IMGM_THREADS * 16;
#pragma unroll
        for (int k = 0; k < 4; ++k) a[g][k] = b[g][k] = m[g][k] = 0u;
        need[g] = false;
        if (q0 >= total) continue;
        imgm_load<VEC>(xs, q0, total, a[g]);
        if (it.mode == MNAS_IMGM_MIXUP) need[g] = true;                                            // uniform over the workgroup
        else if (it.mode == MNAS_IMGM_CUTMIX) need[g] = imgm_box_mask(it, q0, px, H, W, m[g]);     // bytes taken from the partner
    }
#pragma unroll
    for (int g = 0; g < IMGM_GROUPS; ++g)
        if (need[g]) imgm_load<VEC>(ps, base + g * IMGM_THREADS * 16, total, b[g]);
#pragma unroll
    for (int g = 0; g < IMGM_GROUPS; ++g) {
        const int q0 = base + g * IMGM_THREADS * 16;
        if (q0 >= total) continue;
        uint32_t r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            r[k] = it.mode == MNAS_IMGM_MIXUP ? imgm_blend4(a[g][k], b[g][k], w) : ((b[g][k] & m[g][k]) | (a[g][k] & ~m[g][k]));
        if (VEC) {
            *reinterpret_cast<uint4*>(d + q0) = make_uint4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (q0 + j < total) d[q0 + j] = (uint8_t)(r[j >> 2] >> (8 * (j & 3)));
        }
    }
}

extern "C" int mnas_img_mix_check(const MnasImgMix* items_host, int n, int H, int W) {
    if (!imgm_shape_ok(n, H, W) || (n > 0 && items_host == nullptr)) return MNAS_EINVAL;
    for (int i = 0; i < n; ++i)
        if (!imgm_item_ok(items_host[i], n, H, W)) return MNAS_EINVAL;
    return MNAS_OK;
}

extern "C" int mnas_img_mix(const MnasImgMix* items, int n, int H, int W, const void* in, void* out, void* stream) {
    if (!imgm_shape_ok(n, H, W)) return MNAS_EINVAL;
    if (n == 0) return MNAS_OK;
    if (!items || !in || !out) return MNAS_EINVAL;
    const int64_t px = (int64_t)H * W, bytes = (int64_t)n * 3 * px;
    const uintptr_t i0 = (uintptr_t)in, o0 = (uintptr_t)out;
    if (i0 < o0 + (uintptr_t)bytes && o0 < i0 + (uintptr_t)bytes) return MNAS_EINVAL;      // any overlap, in == out included
    const bool vec = (px & 15) == 0 && (i0 & 15) == 0 && (o0 & 15) == 0;
    const dim3 grid((unsigned)((3 * px + IMGM_CHUNK - 1) / IMGM_CHUNK), (unsigned)n);
    const hipStream_t s = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(k_img_mix<true>, grid, dim3(IMGM_THREADS), 0, s, items, n, H, W, (const uint8_t*)in, (uint8_t*)out);
    else
        hipLaunchKernelGGL(k_img_mix<false>, grid, dim3(IMGM_THREADS), 0, s, items, n, H, W, (const uint8_t*)in, (uint8_t*)out);
    MNAS_CHECK_LAUNCH();
    return MNAS_OK;
}
