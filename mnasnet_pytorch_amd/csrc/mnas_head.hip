// Classifier head and loss of FineTuneModelPool: the nn.Sequential of Dropout / Linear / ReLU over the pooled features
// (classifiers.py:56-89, forward :107-111) and nn.CrossEntropyLoss (train.py:277), forward and backward, fp32.
// Replaces ATen's dropout / addmm / relu / log_softmax / nll_loss kernels (about 25 launches of 3-12 us per step) with
// 2 launches per Linear and direction plus 2 for the loss.
//
// One Linear "layer" here = the Dropout in front of it + the Linear + the optional ReLU behind it:
//     xd = u * keep(seed, idx) / (1 - p)        u: [N][I] the layer's input (pooled features or the previous layer's output)
//     z  = xd W^T + b                            W: [O][I]
//     u' = relu(z) or z
// Only u' is stored; the dropout mask is a counter-based hash of (seed, element index), recomputed wherever it is needed
// (forward operand load, weight-gradient operand load, input-gradient epilogue), never written to memory.
// Backward of a layer, given dz = dL/dz:  dW = dz^T xd,  db = sum_n dz,  du = (dz W) * keep/(1-p),  and for the layer in
// front (if it ends in a ReLU)  dz_prev = du * [u > 0].
//
// The three products are one tiled fp32 FMA GEMM with run-time strides (32x32 tile per workgroup, K split over its 8
// waves); at N = 256 these are 0.1-0.3 GFLOP launches of 80-512 workgroups; fp32 FMA (not bf16 MFMA) keeps the head
// comparable with the reference's fp32 head at 2e-5.  Deterministic:
// fixed summation order, no atomics.
#include "mnas_common.h"

// splitmix64 of (seed, index): P(keep) = 1 - p with thresh = p * 2^32  (oracle/mnasnet_oracle.py: head_dropout_keep)
__device__ __forceinline__ bool head_keep(unsigned long long seed, unsigned long long idx, unsigned int thresh) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (idx + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (unsigned int)(z >> 32) >= thresh;
}

struct HeadGemmArgs {
    int M, N, K;
    const float* A; long long sam, sak;      // A(m,k) = A[m*sam + k*sak]
    const float* B; long long sbk, sbn;      // B(k,n) = B[k*sbk + n*sbn]
    float* C; long long ldc;                 // C[m*ldc + n]
    const float* bias;                       // [N] or NULL
    int relu, accumulate;
    int drop_where;                          // 0 none, 1 on A (element m*K+k), 2 on B (element k*N+n), 3 on C (element m*N+n)
    unsigned int drop_thresh; float drop_scale; unsigned long long seed;
    const float* relu_mask; long long ldm;   // epilogue: C *= [relu_mask[m*ldm+n] > 0], or NULL
    float* rowsum; int rowsum_acc;           // rowsum[m] (+)= sum_k A(m,k)  (written by the n-tile-0 workgroups), or NULL
};

// 32x32 output tile per workgroup of 8 waves, K in steps of 128 staged through LDS (k-contiguous rows; the next step's
// operands are loaded into registers while the current one is multiplied).  Each wave multiplies an EIGHTH of every K step
// for the whole tile (4x4 outputs per lane, rows ty+8i / columns tx+8j so that the 16-byte LDS reads of a wave fall into
// distinct banks) and the eight partial tiles are added in wave order at the end: a single wave walking K = 1000 alone is
// bound by its own instruction stream (40-60 us measured), not by memory.  VEC: 16-byte global loads along whichever
// index is contiguous in memory (needs that extent and the leading strides to be multiples of 4).
template <bool VEC>
__global__ __launch_bounds__(512) void k_head_gemm(HeadGemmArgs a) {
    constexpr int BM = 32, BK = 128, LDK = 132, NV = BM * BK / 4 / 512, KW = BK / 8;
    __shared__ __attribute__((aligned(16))) float smem[2 * BM * LDK];
    float* As = smem;                         // [32 m][LDK]
    float* Bs = smem + BM * LDK;              // [32 n][LDK]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx = lane & 7, ty = lane >> 3;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BM;
    float acc[4][4], asum[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        asum[i] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    }
    const bool a_kfast = a.sak == 1, b_kfast = a.sbk == 1;
    const bool do_rowsum = a.rowsum != nullptr && blockIdx.x == 0;
    float4 ra[NV], rb[NV];
    // one operand: X(r, k) = P[r*sr + k*sk], r in [r0, r0+32) (bounded by R), dropout element index r*er + k*ek
    auto load_op = [&](float4* reg, const float* P, long long sr, long long sk, bool kfast, int r0, int R, int k0, bool drop,
                       long long er, long long ek) {
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const int q = tid + 512 * e;                     // float4 index in the 32 x 128 tile
            // kfast: 4 consecutive k of one row; else: 4 consecutive rows at one k
            const int rr = kfast ? q / (BK / 4) : (q % (BM / 4)) * 4, kk = kfast ? (q % (BK / 4)) * 4 : q / (BM / 4);
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            const int r = r0 + rr, k = k0 + kk;
            const bool full = kfast ? (r < R && k + 3 < a.K) : (r + 3 < R && k < a.K);
            if (VEC && full) {
                const float4 t = *(const float4*)(P + r * sr + k * sk);
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int ri = kfast ? r : r + i, ki = kfast ? k + i : k;
                    if (ri < R && ki < a.K) v[i] = P[ri * sr + ki * sk];
                }
            }
            if (drop) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int ri = kfast ? r : r + i, ki = kfast ? k + i : k;
                    v[i] = head_keep(a.seed, (unsigned long long)(ri * er + ki * ek), a.drop_thresh) ? v[i] * a.drop_scale : 0.f;
                }
            }
            reg[e] = make_float4(v[0], v[1], v[2], v[3]);
        }
    };
    auto store_op = [&](float* T, const float4* reg, bool kfast) {
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const int q = tid + 512 * e;
            const int rr = kfast ? q / (BK / 4) : (q % (BM / 4)) * 4, kk = kfast ? (q % (BK / 4)) * 4 : q / (BM / 4);
            if (kfast) {
                *(float4*)(T + rr * LDK + kk) = reg[e];
            } else {
                T[(rr + 0) * LDK + kk] = reg[e].x; T[(rr + 1) * LDK + kk] = reg[e].y;
                T[(rr + 2) * LDK + kk] = reg[e].z; T[(rr + 3) * LDK + kk] = reg[e].w;
            }
        }
    };
    auto load = [&](int k0) {
        load_op(ra, a.A, a.sam, a.sak, a_kfast, m0, a.M, k0, a.drop_where == 1, a.K, 1);
        load_op(rb, a.B, a.sbn, a.sbk, b_kfast, n0, a.N, k0, a.drop_where == 2, 1, a.N);
    };
    load(0);
    for (int k0 = 0; k0 < a.K; k0 += BK) {
        store_op(As, ra, a_kfast);
        store_op(Bs, rb, b_kfast);
        __syncthreads();
        if (k0 + BK < a.K) load(k0 + BK);
#pragma unroll
        for (int kq = 0; kq < KW; kq += 4) {
            const int kk = wave * KW + kq;
            float4 av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                av[i] = *(const float4*)(As + (ty + 8 * i) * LDK + kk);
                bv[i] = *(const float4*)(Bs + (tx + 8 * i) * LDK + kk);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float ar[4] = {av[i].x, av[i].y, av[i].z, av[i].w};
                if (do_rowsum) asum[i] += (ar[0] + ar[1]) + (ar[2] + ar[3]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float br[4] = {bv[j].x, bv[j].y, bv[j].z, bv[j].w};
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[i][j] = fmaf(ar[c], br[c], acc[i][j]);
                }
            }
        }
        __syncthreads();
    }
    // ---- the eight waves' partial tiles -> LDS, summed in wave order (the operand tiles are free: the loop ended with a barrier)
    float* part = smem;                      // [8][32][33] = 8448 floats (the operand tiles hold 8448)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) part[(wave * 32 + ty + 8 * i) * 33 + tx + 8 * j] = acc[i][j];
    __syncthreads();
    float outv[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int q = tid + 512 * e, mm = q >> 5, nn = q & 31;
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) v += part[(w * 32 + mm) * 33 + nn];
        outv[e] = v;
    }
    if (do_rowsum) {                          // uniform per workgroup
        __syncthreads();
        float* psum = smem;                  // [8][32]
        if (tx == 0)
#pragma unroll
            for (int i = 0; i < 4; ++i) psum[wave * 32 + ty + 8 * i] = asum[i];
        __syncthreads();
        if (tid < 32 && m0 + tid < a.M) {
            float rs = 0.f;
#pragma unroll
            for (int w = 0; w < 8; ++w) rs += psum[w * 32 + tid];
            a.rowsum[m0 + tid] = a.rowsum_acc ? a.rowsum[m0 + tid] + rs : rs;
        }
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int q = tid + 512 * e, mm = q >> 5, nn = q & 31;
        const int m = m0 + mm, n = n0 + nn;
        if (m >= a.M || n >= a.N) continue;
        float v = outv[e];
        if (a.bias) v += a.bias[n];
        if (a.relu) v = fmaxf(v, 0.f);
        if (a.drop_where == 3)
            v = head_keep(a.seed, (unsigned long long)m * a.N + n, a.drop_thresh) ? v * a.drop_scale : 0.f;
        if (a.relu_mask && !(a.relu_mask[m * a.ldm + n] > 0.f)) v = 0.f;
        float* c = a.C + m * a.ldc + n;
        *c = a.accumulate ? *c + v : v;
    }
}

static int head_drop(float p, unsigned int* thresh, float* scale) {
    if (!(p >= 0.f) || p >= 1.f) return MNAS_EINVAL;
    double t = (double)p * 4294967296.0;
    *thresh = t >= 4294967295.0 ? 4294967295u : (unsigned int)t;
    *scale = (float)(1.0 / (1.0 - (double)p));
    return MNAS_OK;
}

static int head_launch(const HeadGemmArgs& a, hipStream_t s) {
    if (a.M < 1 || a.N < 1 || a.K < 1) return MNAS_EINVAL;
    // 16-byte loads: the contiguous index of either operand must cover whole float4s at aligned addresses
    auto vec_ok = [&](const float* P, long long sr, long long sk, int R) {
        const long long lead = sk == 1 ? sr : sk;            // stride of the non-contiguous index
        const int extent = sk == 1 ? a.K : R;                // extent of the contiguous one
        return (sr == 1 || sk == 1) && (lead & 3) == 0 && (extent & 3) == 0 && ((uintptr_t)P & 15) == 0;
    };
    const dim3 grid((a.N + 31) / 32, (a.M + 31) / 32);
    if (vec_ok(a.A, a.sam, a.sak, a.M) && vec_ok(a.B, a.sbn, a.sbk, a.N)) hipLaunchKernelGGL(k_head_gemm<true>, grid, dim3(512), 0, s, a);
    else hipLaunchKernelGGL(k_head_gemm<false>, grid, dim3(512), 0, s, a);
    MNAS_CHECK_LAUNCH();
    return MNAS_OK;
}

extern "C" int mnas_head_linear_fwd(const MnasHeadLinear* c, void* stream) {
    if (!c || !c->x || !c->w || !c->y || c->N < 1 || c->I < 1 || c->O < 1) return MNAS_EINVAL;
    HeadGemmArgs a = {};
    a.M = c->N; a.N = c->O; a.K = c->I;
    a.A = (const float*)c->x; a.sam = c->I; a.sak = 1;
    a.B = (const float*)c->w; a.sbk = 1; a.sbn = c->I;
    a.C = (float*)c->y; a.ldc = c->O;
    a.bias = (const float*)c->b; a.relu = c->relu ? 1 : 0;
    a.seed = c->seed;
    if (c->drop_p > 0.f) {
        if (head_drop(c->drop_p, &a.drop_thresh, &a.drop_scale) != MNAS_OK) return MNAS_EINVAL;
        a.drop_where = 1;
    }
    return head_launch(a, (hipStream_t)stream);
}

// dW[O][I] (+)= dz^T (x * keep/(1-p)),  db[O] (+)= sum_n dz
extern "C" int mnas_head_linear_bwd_w(const MnasHeadLinear* c, void* stream) {
    if (!c || !c->x || !c->dz || !c->dw || c->N < 1 || c->I < 1 || c->O < 1) return MNAS_EINVAL;
    HeadGemmArgs a = {};
    a.M = c->O; a.N = c->I; a.K = c->N;
    a.A = (const float*)c->dz; a.sam = 1; a.sak = c->O;
    a.B = (const float*)c->x; a.sbk = c->I; a.sbn = 1;
    a.C = (float*)c->dw; a.ldc = c->I; a.accumulate = c->accumulate ? 1 : 0;
    a.rowsum = (float*)c->db; a.rowsum_acc = a.accumulate;
    a.seed = c->seed;
    if (c->drop_p > 0.f) {
        if (head_drop(c->drop_p, &a.drop_thresh, &a.drop_scale) != MNAS_OK) return MNAS_EINVAL;
        a.drop_where = 2;
    }
    return head_launch(a, (hipStream_t)stream);
}

// dx[N][I] = (dz W) * keep/(1-p) * [relu_mask > 0]   (relu_mask: this layer's input u when the layer in front ends in a ReLU)
extern "C" int mnas_head_linear_bwd_x(const MnasHeadLinear* c, void* stream) {
    if (!c || !c->dz || !c->w || !c->dx || c->N < 1 || c->I < 1 || c->O < 1) return MNAS_EINVAL;
    HeadGemmArgs a = {};
    a.M = c->N; a.N = c->I; a.K = c->O;
    a.A = (const float*)c->dz; a.sam = c->O; a.sak = 1;
    a.B = (const float*)c->w; a.sbk = c->I; a.sbn = 1;
    a.C = (float*)c->dx; a.ldc = c->I;
    a.relu_mask = (const float*)c->relu_mask; a.ldm = c->I;
    a.seed = c->seed;
    if (c->drop_p > 0.f) {
        if (head_drop(c->drop_p, &a.drop_thresh, &a.drop_scale) != MNAS_OK) return MNAS_EINVAL;
        a.drop_where = 3;
    }
    return head_launch(a, (hipStream_t)stream);
}

// keep mask of a layer as bytes (tests / oracle cross-check only)
__global__ void k_head_mask(unsigned char* out, long long n, unsigned long long seed, unsigned int thresh) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = head_keep(seed, (unsigned long long)i, thresh) ? 1 : 0;
}
extern "C" int mnas_head_dropout_mask(void* out, int64_t n, float p, uint64_t seed, void* stream) {
    unsigned int thresh; float scale;
    if (!out || n < 1 || head_drop(p, &thresh, &scale) != MNAS_OK) return MNAS_EINVAL;
    hipLaunchKernelGGL(k_head_mask, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (unsigned char*)out,
                       (long long)n, (unsigned long long)seed, thresh);
    MNAS_CHECK_LAUNCH();
    return MNAS_OK;
}

// ---- nn.CrossEntropyLoss(reduction='mean', ignore_index): one workgroup per row --------------------------------------
// loss_rows[n] = logsumexp(x[n]) - x[n][t],  dlogits[n][c] = (softmax(x[n])[c] - [c == t]) / count   (0 for ignored rows)
// count = rows whose target != ignore_index: every workgroup counts the (few hundred) targets itself.
__device__ __forceinline__ float head_wg_reduce(float v, float* red, bool is_max) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float w = __shfl_xor(v, o, 64);
        v = is_max ? fmaxf(v, w) : v + w;
    }
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return is_max ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- device-resident meters (train.py:447,465-468,575,589-592: AverageMeter.update(loss.item(), n) and accuracy(out, target,
// topk=(1, 5)) without the three host reads per step).  METRICS = true adds, to the two loss kernels, the rank of every row's
// target and the update of one MnasMeters block; METRICS = false is the code as it was (same instructions on the loss path:
// the extra work hangs off the row's max pass and the tail of the one-workgroup mean stage).
// rank_n = #{j : z[n,j] > z[n,t]} + #{j < t : z[n,j] == z[n,t]}; row n is correct@k iff rank_n < k (include/mnas.h).
#define HEAD_RANK_WRONG 0x7fffffff       // target ignored / out of range / its logit not finite: wrong for every k

struct HeadKs { int k[MNAS_METERS_MAX_K]; int nk; };

__device__ __forceinline__ int head_wg_reduce_int(int v, int* red) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// one workgroup of 256: rows correct@k from the per-row ranks (integer sums in a fixed order), then ONE thread moves the block.
// loss == NULL: only steps / samples / accuracy fields move.
__device__ __forceinline__ void head_meters_update(const int* rank_rows, int N, HeadKs ks, const float* loss, MnasMeters* m, int* redi) {
    int c[MNAS_METERS_MAX_K];
#pragma unroll
    for (int q = 0; q < MNAS_METERS_MAX_K; ++q) c[q] = 0;
    for (int i = threadIdx.x; i < N; i += 256) {
        const int r = rank_rows[i];
#pragma unroll
        for (int q = 0; q < MNAS_METERS_MAX_K; ++q) c[q] += (q < ks.nk && r < ks.k[q]) ? 1 : 0;
    }
#pragma unroll
    for (int q = 0; q < MNAS_METERS_MAX_K; ++q) c[q] = head_wg_reduce_int(c[q], redi);
    if (threadIdx.x != 0) return;
    m->steps += 1;
    m->samples += N;
    m->last_n = N;
#pragma unroll
    for (int q = 0; q < MNAS_METERS_MAX_K; ++q) {
        m->correct[q] += c[q];
        m->last_correct[q] = c[q];
    }
    if (loss) {
        // AverageMeter.update(loss.item(), n): sum += val * n in Python floats = one rounded double product and one rounded
        // double sum per step, in step order (no fused multiply-add: it would round once instead of twice)
        const float l = *loss;
        const double d = (double)l, dn = __dmul_rn(d, (double)N);
        m->loss_sum = __dadd_rn(m->loss_sum, dn);
        m->loss_samples += N;
        m->last_loss = d;
        m->last_loss_sum = dn;
        m->last_loss_n = N;
        if (!isfinite(l)) m->nonfinite_steps += 1;
    }
}

template <bool METRICS>
__global__ __launch_bounds__(256) void k_head_ce(const float* x, const long long* target, int N, int C, long long ignore_index,
                                                 float* loss_rows, float* dlogits, int* bad, int* rank_rows) {
    __shared__ float red[4];
    __shared__ int redi[4];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* row = x + (size_t)n * C;
    float cnt = 0.f;
    for (int i = tid; i < N; i += 256) cnt += target[i] != ignore_index ? 1.f : 0.f;
    cnt = head_wg_reduce(cnt, red, false);
    const long long t = target[n];
    const bool ignored = t == ignore_index;
    if (!ignored && (t < 0 || t >= C)) {            // ATen asserts on the device; here: flag it, treat the row as ignored
        if (tid == 0) atomicExch(bad, 1);
    }
    const bool valid = !ignored && t >= 0 && t < C;
    float mx = -INFINITY;
    if (METRICS) {
        const float zt = valid ? row[t] : 0.f;
        const int ti = (int)t;
        int above = 0;
        for (int c = tid; c < C; c += 256) {
            const float z = row[c];
            mx = fmaxf(mx, z);
            above += (z > zt || (z == zt && c < ti)) ? 1 : 0;
        }
        above = head_wg_reduce_int(above, redi);
        if (tid == 0) rank_rows[n] = (valid && isfinite(zt)) ? above : HEAD_RANK_WRONG;
    } else {
        for (int c = tid; c < C; c += 256) mx = fmaxf(mx, row[c]);
    }
    mx = head_wg_reduce(mx, red, true);
    float se = 0.f;
    for (int c = tid; c < C; c += 256) se += expf(row[c] - mx);
    se = head_wg_reduce(se, red, false);
    const float inv = valid && cnt > 0.f ? 1.f / cnt : 0.f, rse = 1.f / se;
    if (dlogits)
        for (int c = tid; c < C; c += 256) {
            const float p = expf(row[c] - mx) * rse;
            dlogits[(size_t)n * C + c] = valid ? (p - (c == (int)t ? 1.f : 0.f)) * inv : 0.f;
        }
    if (tid == 0) loss_rows[n] = valid ? (logf(se) + mx - row[t]) : (ignored ? 0.f : NAN);   // out-of-range target: poison the loss
}

// loss = sum(loss_rows) / count, fixed order (thread-strided partials, then a tree)
template <bool METRICS>
__global__ __launch_bounds__(256) void k_head_loss_mean(const float* loss_rows, const long long* target, int N, long long ignore_index,
                                                        float* loss, const int* rank_rows, HeadKs ks, MnasMeters* meters) {
    __shared__ float red[4];
    __shared__ int redi[4];
    float s = 0.f, cnt = 0.f;
    for (int i = threadIdx.x; i < N; i += 256) { s += loss_rows[i]; cnt += target[i] != ignore_index ? 1.f : 0.f; }
    s = head_wg_reduce(s, red, false);
    cnt = head_wg_reduce(cnt, red, false);
    if (threadIdx.x == 0) *loss = s / cnt;       // 0/0 = nan when every row is ignored, as ATen
    if (METRICS) head_meters_update(rank_rows, N, ks, loss, meters, redi);   // thread 0 reads back its own store
}

extern "C" int mnas_head_cross_entropy(const void* logits, const void* target, int N, int C, int64_t ignore_index,
                                       void* loss_rows, void* loss, void* dlogits, void* bad_flag, void* stream) {
    if (!logits || !target || !loss_rows || !loss || !bad_flag || N < 1 || C < 1) return MNAS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_head_ce<false>, dim3(N), dim3(256), 0, s, (const float*)logits, (const long long*)target, N, C,
                       (long long)ignore_index, (float*)loss_rows, (float*)dlogits, (int*)bad_flag, (int*)nullptr);
    MNAS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_head_loss_mean<false>, dim3(1), dim3(256), 0, s, (const float*)loss_rows, (const long long*)target, N,
                       (long long)ignore_index, (float*)loss, (const int*)nullptr, HeadKs{}, (MnasMeters*)nullptr);
    MNAS_CHECK_LAUNCH();
    return MNAS_OK;
}

// k of every meter clamped to [1, C] (top-k over C classes with k > C is top-C); k < 1 or more than MNAS_METERS_MAX_K of them: invalid
static int head_ks(const int* ks, int nk, int C, HeadKs* out) {
    if (!ks || nk < 1 || nk > MNAS_METERS_MAX_K) return MNAS_EINVAL;
    *out = HeadKs{};
    out->nk = nk;
    for (int i = 0; i < nk; ++i) {
        if (ks[i] < 1) return MNAS_EINVAL;
        out->k[i] = ks[i] < C ? ks[i] : C;
    }
    return MNAS_OK;
}

extern "C" int mnas_head_cross_entropy_metrics(const void* logits, const void* target, int N, int C, int64_t ignore_index,
                                               void* loss_rows, void* loss, void* dlogits, void* bad_flag, const int* ks, int nk,
                                               void* rank_rows, MnasMeters* meters, void* stream) {
    if (!logits || !target || !loss_rows || !loss || !bad_flag || !rank_rows || !meters || N < 1 || C < 1) return MNAS_EINVAL;
    HeadKs k;
    if (head_ks(ks, nk, C, &k) != MNAS_OK) return MNAS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_head_ce<true>, dim3(N), dim3(256), 0, s, (const float*)logits, (const long long*)target, N, C,
                       (long long)ignore_index, (float*)loss_rows, (float*)dlogits, (int*)bad_flag, (int*)rank_rows);
    MNAS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_head_loss_mean<true>, dim3(1), dim3(256), 0, s, (const float*)loss_rows, (const long long*)target, N,
                       (long long)ignore_index, (float*)loss, (const int*)rank_rows, k, meters);
    MNAS_CHECK_LAUNCH();
    return MNAS_OK;
}

// ---- soft-target cross-entropy: label smoothing eps and batch mixing (Mixup / CutMix: two labels a, b per row, weight lam on a) --
// target row  q = (1 - eps) (lam e[a] + (1 - lam) e[b]) + eps / C;  with lse = logsumexp(z):
//   loss_rows[n] = (1 - eps) (lam (lse - z[a]) + (1 - lam) (lse - z[b])) + eps (lse - mean_c z)
//   dlogits[n][c] = (softmax(z)[c] - q[c]) / count
// tb == NULL: no mixing (b = a, lam = 1, lam[] is not read); lam == NULL: 1.  A row is ignored when a or (with mixing) b is
// ignore_index; count = rows not ignored.  A label outside [0, C) or a lam that is NaN or outside [0, 1] raises *bad and poisons
// the loss; such a row indexes nothing.  The same launch shape as k_head_ce / k_head_loss_mean; sum_c z rides on the max pass.
// METRICS: the row is ranked against the label with the larger weight, a when lam >= 0.5.
__device__ __forceinline__ bool head_soft_counts(const long long* ta, const long long* tb, int i, long long ignore_index) {
    return ta[i] != ignore_index && (tb == nullptr || tb[i] != ignore_index);
}

template <bool METRICS>
__global__ __launch_bounds__(256) void k_head_ce_soft(const float* x, const long long* ta, const long long* tb, const float* lam,
                                                      float eps, int N, int C, long long ignore_index, float* loss_rows,
                                                      float* dlogits, int* bad, int* rank_rows) {
    __shared__ float red[4];
    __shared__ int redi[4];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* row = x + (size_t)n * C;
    float cnt = 0.f;
    for (int i = tid; i < N; i += 256) cnt += head_soft_counts(ta, tb, i, ignore_index) ? 1.f : 0.f;
    cnt = head_wg_reduce(cnt, red, false);
    const long long a = ta[n], b = tb ? tb[n] : a;
    const float l = (tb && lam) ? lam[n] : 1.f;
    const bool ignored = a == ignore_index || b == ignore_index;
    const bool valid = !ignored && a >= 0 && a < C && b >= 0 && b < C && l >= 0.f && l <= 1.f;     // a NaN lam fails both
    if (!ignored && !valid) {
        if (tid == 0) atomicExch(bad, 1);
    }
    float mx = -INFINITY, sz = 0.f;
    if (METRICS) {
        const int ti = (int)(l >= 0.5f ? a : b);
        const float zt = valid ? row[ti] : 0.f;
        int above = 0;
        for (int c = tid; c < C; c += 256) {
            const float z = row[c];
            mx = fmaxf(mx, z);
            sz += z;
            above += (z > zt || (z == zt && c < ti)) ? 1 : 0;
        }
        above = head_wg_reduce_int(above, redi);
        if (tid == 0) rank_rows[n] = (valid && isfinite(zt)) ? above : HEAD_RANK_WRONG;
    } else {
        for (int c = tid; c < C; c += 256) {
            const float z = row[c];
            mx = fmaxf(mx, z);
            sz += z;
        }
    }
    mx = head_wg_reduce(mx, red, true);
    sz = head_wg_reduce(sz, red, false);
    float se = 0.f;
    for (int c = tid; c < C; c += 256) se += expf(row[c] - mx);
    se = head_wg_reduce(se, red, false);
    const float inv = valid && cnt > 0.f ? 1.f / cnt : 0.f, rse = 1.f / se;
    // weights of e[a], e[b] and of every class.  A row whose two labels coincide has the target it would have without mixing,
    // whatever its lam: (1 - eps) on the one label, not two rounded shares of it
    const bool same = a == b;
    const float wa = same ? 1.f - eps : (1.f - eps) * l, wb = same ? 0.f : (1.f - eps) - wa, u = eps / (float)C;
    if (dlogits)
        for (int c = tid; c < C; c += 256) {
            const float p = expf(row[c] - mx) * rse;
            const float q = (c == (int)a ? wa : 0.f) + (c == (int)b && !same ? wb : 0.f) + u;
            dlogits[(size_t)n * C + c] = valid ? (p - q) * inv : 0.f;
        }
    if (tid == 0) {
        float r = ignored ? 0.f : NAN;                      // a refused row poisons the loss
        if (valid) {
            const float lse = logf(se) + mx;
            // eps == 0: no smoothing term.  A -inf logit at a class that is no label (a masked class) makes sz -inf, and 0 * inf
            // would poison a row that k_head_ce gives a finite loss; the expression itself is unchanged (0 * 0 adds nothing)
            const float sm = eps != 0.f ? lse - sz / (float)C : 0.f;
            r = wa * (lse - row[a]) + wb * (lse - row[b]) + eps * sm;
        }
        loss_rows[n] = r;
    }
}

template <bool METRICS>
__global__ __launch_bounds__(256) void k_head_loss_mean_soft(const float* loss_rows, const long long* ta, const long long* tb, int N,
                                                             long long ignore_index, float* loss, const int* rank_rows, HeadKs ks,
                                                             MnasMeters* meters) {
    __shared__ float red[4];
    __shared__ int redi[4];
    float s = 0.f, cnt = 0.f;
    for (int i = threadIdx.x; i < N; i += 256) { s += loss_rows[i]; cnt += head_soft_counts(ta, tb, i, ignore_index) ? 1.f : 0.f; }
    s = head_wg_reduce(s, red, false);
    cnt = head_wg_reduce(cnt, red, false);
    if (threadIdx.x == 0) *loss = s / cnt;       // 0/0 = nan when every row is ignored
    if (METRICS) head_meters_update(rank_rows, N, ks, loss, meters, redi);   // thread 0 reads back its own store
}

extern "C" int mnas_head_cross_entropy_soft(const void* logits, const void* target_a, const void* target_b, const float* lam,
                                            float label_smoothing, int N, int C, int64_t ignore_index, void* loss_rows, void* loss,
                                            void* dlogits, void* bad_flag, const int* ks, int nk, void* rank_rows, MnasMeters* meters,
                                            void* stream) {
    if (!logits || !target_a || !loss_rows || !loss || !bad_flag || N < 1 || C < 1) return MNAS_EINVAL;
    if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) return MNAS_EINVAL;
    HeadKs k = {};
    if (meters && (!rank_rows || head_ks(ks, nk, C, &k) != MNAS_OK)) return MNAS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const float* x = (const float*)logits;
    const long long *ta = (const long long*)target_a, *tb = (const long long*)target_b;
    if (meters) {
        hipLaunchKernelGGL(k_head_ce_soft<true>, dim3(N), dim3(256), 0, s, x, ta, tb, lam, label_smoothing, N, C, (long long)ignore_index,
                           (float*)loss_rows, (float*)dlogits, (int*)bad_flag, (int*)rank_rows);
        MNAS_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_head_loss_mean_soft<true>, dim3(1), dim3(256), 0, s, (const float*)loss_rows, ta, tb, N,
                           (long long)ignore_index, (float*)loss, (const int*)rank_rows, k, meters);
    } else {
        hipLaunchKernelGGL(k_head_ce_soft<false>, dim3(N), dim3(256), 0, s, x, ta, tb, lam, label_smoothing, N, C,
                           (long long)ignore_index, (float*)loss_rows, (float*)dlogits, (int*)bad_flag, (int*)nullptr);
        MNAS_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_head_loss_mean_soft<false>, dim3(1), dim3(256), 0, s, (const float*)loss_rows, ta, tb, N,
                           (long long)ignore_index, (float*)loss, (const int*)nullptr, HeadKs{}, (MnasMeters*)nullptr);
    }
    MNAS_CHECK_LAUNCH();
    return MNAS_OK;
}

// ---- class weights and knowledge distillation on top of the soft-target loss (include/mnas.h "distillation cross-entropy") ------------
// Labels a, b, weight l, smoothing eps and the target row q of k_head_ce_soft; class weights w[C] (NULL: all 1) and teacher logits
// t (NULL: no distillation term) are new.  The same launch shape: one workgroup per row, one workgroup for the means.
//
// Operation order (every line one fp32 operation unless it says otherwise; "sum" = the lane's strided sum, the six butterfly levels
// and the three adds of the four waves of head_wg_reduce: ceil(n / 256) + 9 adds; tests/bounds_kd.py brackets exactly this):
//   row weight   s_i = 0 for an ignored row, 1 without w, else w[a] when a == b, else fmaf(l, w[a] - w[b], w[b]);  D = sum_i s_i
//   pass 1       mx = max_c z (exact);  swz = sum_c fmaf(w_c, z_c, .) (the fma IS the add);  sw = sum_c w_c;  KD: mt = max_c t
//                Wm = sw / C (1 without w);  invT = 1 / T
//   pass 2       d_c = z_c - mx;  se = sum_c expf(d_c);   KD: eS_c = expf(d_c invT), seS = sum eS;  dt_c = t_c - mt,
//                eT_c = expf(dt_c invT), seT = sum eT;  sA = sum_c eT_c (dt_c - d_c), a class with eT_c == 0 adds exactly 0
//   scalars      rse = 1 / se, rseS = 1 / seS, rseT = 1 / seT;  wa, wb, u = eps / C as in k_head_ce_soft;
//                S = fmaf(eps, Wm - s_n, s_n)  (= sum_c w_c q_c; exactly 1 when every weight is 1);
//                invD = 1 / D (0 when the row is not valid or D is not > 0);  ch = (1 - alpha) invD;  ck = (alpha T) / N
//   gradient     p = expf(d_c) rse;  q = (qa + qb) + u;  g = (p S - w_c q) ch   (0: row not valid, or alpha == 1)
//                KD: pS = eS_c rseS, pT = eT_c rseT (both exponentials evaluated again), g = g + ck (pS - pT)
//   hard row     lse = logf(se) + mx;  sm = Wm lse - swz / C (0 when eps == 0);
//                (wa w[a]) (lse - z[a]) + (wb w[b]) (lse - z[b]) + eps sm          (0: ignored row; NaN: refused row)
//   kd row       (sA rseT) invT + (logf(seS) - logf(seT))                          (NaN: refused row; 0: no distillation term)
// The build contracts a * b + c into an fma where it likes (-ffp-contract=fast); the bracket of the uncontracted form holds either.
// Without w and t every factor above that involves them is exactly 1 or 0: the results are those of k_head_ce_soft's expressions.
__device__ __forceinline__ bool head_kd_refused(long long a, long long b, float l, int C) {
    return !(a >= 0 && a < C && b >= 0 && b < C && l >= 0.f && l <= 1.f);                   // a NaN l fails both
}

__device__ __forceinline__ float head_kd_mix_weight(float wa, float wb, float l, bool same) { return same ? wa : fmaf(l, wa - wb, wb); }

// s_i: what row i adds to the divisor D.  A refused row indexes nothing (its NaN loss row poisons the mean anyway)
__device__ __forceinline__ float head_kd_row_weight(const long long* ta, const long long* tb, const float* lam, const float* w, int i,
                                                    int C, long long ignore_index) {
    if (!head_soft_counts(ta, tb, i, ignore_index)) return 0.f;
    if (!w) return 1.f;
    const long long a = ta[i], b = tb ? tb[i] : a;
    const float l = (tb && lam) ? lam[i] : 1.f;
    if (head_kd_refused(a, b, l, C)) return 0.f;
    return head_kd_mix_weight(w[a], w[b], l, a == b);
}

template <bool METRICS>
__global__ __launch_bounds__(256) void k_head_ce_kd(const float* x, const long long* ta, const long long* tb, const float* lam, float eps,
                                                    const float* w, const float* t, float T, float alpha, int N, int C,
                                                    long long ignore_index, float* loss_rows, float* dlogits, int* bad, int* rank_rows) {
    __shared__ float red[4];
    __shared__ int redi[4];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* row = x + (size_t)n * C;
    const bool kd = t != nullptr;                       // the host passes NULL when alpha == 0: t is not read
    const float* trow = kd ? t + (size_t)n * C : nullptr;
    float D = 0.f;
    for (int i = tid; i < N; i += 256) D += head_kd_row_weight(ta, tb, lam, w, i, C, ignore_index);
    D = head_wg_reduce(D, red, false);
    const long long a = ta[n], b = tb ? tb[n] : a;
    const float l = (tb && lam) ? lam[n] : 1.f;
    const bool ignored = a == ignore_index || b == ignore_index;
    const bool refused = !ignored && head_kd_refused(a, b, l, C);
    const bool valid = !ignored && !refused;
    if (refused) {
        if (tid == 0) atomicExch(bad, 1);
    }
    float mx = -INFINITY, mt = -INFINITY, swz = 0.f, sw = 0.f;
    {
        const int ti = (int)(l >= 0.5f ? a : b);
        const float zt = (METRICS && valid) ? row[ti] : 0.f;
        int above = 0;
        for (int c = tid; c < C; c += 256) {
            const float z = row[c], wc = w ? w[c] : 1.f;
            mx = fmaxf(mx, z);
            swz = fmaf(wc, z, swz);
            sw += wc;
            if (kd) mt = fmaxf(mt, trow[c]);
            if (METRICS) above += (z > zt || (z == zt && c < ti)) ? 1 : 0;
        }
        if (METRICS) {
            above = head_wg_reduce_int(above, redi);
            if (tid == 0) rank_rows[n] = (valid && isfinite(zt)) ? above : HEAD_RANK_WRONG;
        }
    }
    mx = head_wg_reduce(mx, red, true);
    swz = head_wg_reduce(swz, red, false);
    float Wm = 1.f;
    if (w) Wm = head_wg_reduce(sw, red, false) / (float)C;
    const float invT = 1.f / T;
    float se = 0.f, seS = 0.f, seT = 0.f, sA = 0.f;
    if (kd) {
        mt = head_wg_reduce(mt, red, true);
        for (int c = tid; c < C; c += 256) {
            const float d = row[c] - mx, dt = trow[c] - mt;
            const float eT = expf(dt * invT);
            se += expf(d);
            seS += expf(d * invT);
            seT += eT;
            sA += eT > 0.f ? eT * (dt - d) : 0.f;       // pT == 0 (a masked teacher class): exactly 0, never 0 * inf
        }
        seS = head_wg_reduce(seS, red, false);
        seT = head_wg_reduce(seT, red, false);
        sA = head_wg_reduce(sA, red, false);
    } else {
        for (int c = tid; c < C; c += 256) se += expf(row[c] - mx);
    }
    se = head_wg_reduce(se, red, false);
    const float rse = 1.f / se, rseS = 1.f / seS, rseT = 1.f / seT;
    // the target row's weights, as k_head_ce_soft forms them
    const bool same = a == b;
    const float wa = same ? 1.f - eps : (1.f - eps) * l, wb = same ? 0.f : (1.f - eps) - wa, u = eps / (float)C;
    const float wA = (valid && w) ? w[a] : 1.f, wB = (valid && w) ? w[b] : 1.f;
    const float sn = head_kd_mix_weight(wA, wB, l, same), S = fmaf(eps, Wm - sn, sn);
    const bool hard_on = !(kd && alpha == 1.f);         // alpha == 1: the hard term is left out, no 0 * inf
    const float invD = valid && D > 0.f ? 1.f / D : 0.f;
    const float ch = kd ? (1.f - alpha) * invD : invD, ck = kd ? alpha * T / (float)N : 0.f;
    if (dlogits)
        for (int c = tid; c < C; c += 256) {
            const float d = row[c] - mx, wc = w ? w[c] : 1.f;
            const float p = expf(d) * rse;
            const float q = (c == (int)a ? wa : 0.f) + (c == (int)b && !same ? wb : 0.f) + u;
            float g = (valid && hard_on) ? (p * S - wc * q) * ch : 0.f;
            if (kd) {
                const float pS = expf(d * invT) * rseS, pT = expf((trow[c] - mt) * invT) * rseT;
                g = g + ck * (pS - pT);
            }
            dlogits[(size_t)n * C + c] = refused ? 0.f : g;
        }
    if (tid == 0) {
        float rh = ignored ? 0.f : NAN, rk = 0.f;          // a refused row poisons both parts
        if (valid) {
            const float lse = logf(se) + mx;
            // eps == 0: no smoothing term, as in k_head_ce_soft (a -inf logit at a class that is no label leaves the row finite)
            const float sm = eps != 0.f ? Wm * lse - swz / (float)C : 0.f;
            rh = (wa * wA) * (lse - row[a]) + (wb * wB) * (lse - row[b]) + eps * sm;
        }
        if (kd) rk = refused ? NAN : sA * rseT * invT + (logf(seS) - logf(seT));
        loss_rows[n] = rh;
        loss_rows[(size_t)N + n] = rk;
    }
}

// hard = sum(hard rows) / D, kd = (T T) (sum(kd rows) / N), loss = (1 - alpha) hard + alpha kd  (hard alone without the distillation
// term, kd alone at alpha == 1); the three sums as in k_head_loss_mean_soft
template <bool METRICS>
__global__ __launch_bounds__(256) void k_head_loss_mean_kd(const float* loss_rows, const long long* ta, const long long* tb, const float* lam,
                                                           const float* w, int N, int C, long long ignore_index, int kd, float T,
                                                           float alpha, float* loss, float* parts, const int* rank_rows, HeadKs ks,
                                                           MnasMeters* meters) {
    __shared__ float red[4];
    __shared__ int redi[4];
    float sh = 0.f, sk = 0.f, D = 0.f;
    for (int i = threadIdx.x; i < N; i += 256) {
        sh += loss_rows[i];
        sk += loss_rows[(size_t)N + i];
        D += head_kd_row_weight(ta, tb, lam, w, i, C, ignore_index);
    }
    sh = head_wg_reduce(sh, red, false);
    sk = head_wg_reduce(sk, red, false);
    D = head_wg_reduce(D, red, false);
    if (threadIdx.x == 0) {
        const float hard = sh / D;                      // 0/0 = nan when every row is ignored (or every counted weight is 0)
        const float kdv = kd ? (T * T) * (sk / (float)N) : 0.f;
        *loss = !kd ? hard : (alpha == 1.f ? kdv : (1.f - alpha) * hard + alpha * kdv);
        if (parts) { parts[0] = hard; parts[1] = kdv; }
    }
    if (METRICS) head_meters_update(rank_rows, N, ks, loss, meters, redi);   // thread 0 reads back its own store
}

extern "C" int mnas_head_cross_entropy_kd(const void* logits, const void* target_a, const void* target_b, const float* lam,
                                          float label_smoothing, const float* class_weight, const void* teacher_logits, float temperature,
                                          float alpha, int N, int C, int64_t ignore_index, void* loss_rows, void* loss, void* loss_parts,
                                          void* dlogits, void* bad_flag, const int* ks, int nk, void* rank_rows, MnasMeters* meters,
                                          void* stream) {
    if (!logits || !target_a || !loss_rows || !loss || !bad_flag || N < 1 || C < 1) return MNAS_EINVAL;
    if (!(label_smoothing >= 0.f && label_smoothing <= 1.f) || !(alpha >= 0.f && alpha <= 1.f) || !(temperature > 0.f)) return MNAS_EINVAL;
    HeadKs k = {};
    if (meters && (!rank_rows || head_ks(ks, nk, C, &k) != MNAS_OK)) return MNAS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const float* x = (const float*)logits;
    const float* t = alpha != 0.f ? (const float*)teacher_logits : nullptr;      // alpha == 0: no distillation term, t is not read
    const long long *ta = (const long long*)target_a, *tb = (const long long*)target_b;
    if (meters) {
        hipLaunchKernelGGL(k_head_ce_kd<true>, dim3(N), dim3(256), 0, s, x, ta, tb, lam, label_smoothing, class_weight, t, temperature, alpha,
                           N, C, (long long)ignore_index, (float*)loss_rows, (float*)dlogits, (int*)bad_flag, (int*)rank_rows);
        MNAS_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_head_loss_mean_kd<true>, dim3(1), dim3(256), 0, s, (const float*)loss_rows, ta, tb, lam, class_weight, N, C,
                           (long long)ignore_index, t ? 1 : 0, temperature, alpha, (float*)loss, (float*)loss_parts, (const int*)rank_rows, k,
                           meters);
    } else {
        hipLaunchKernelGGL(k_head_ce_kd<false>, dim3(N), dim3(256), 0, s, x, ta, tb, lam, label_smoothing, class_weight, t, temperature, alpha,
                           N, C, (long long)ignore_index, (float*)loss_rows, (float*)dlogits, (int*)bad_flag, (int*)nullptr);
        MNAS_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_head_loss_mean_kd<false>, dim3(1), dim3(256), 0, s, (const float*)loss_rows, ta, tb, lam, class_weight, N, C,
                           (long long)ignore_index, t ? 1 : 0, temperature, alpha, (float*)loss, (float*)loss_parts, (const int*)nullptr,
                           HeadKs{}, (MnasMeters*)nullptr);
    }
    MNAS_CHECK_LAUNCH();
    return MNAS_OK;
}

// ---- the same counts for logits from anywhere (module path, another criterion, no loss at all): one workgroup per row for the
// ranks, one workgroup for the block.  No ignore_index here: a target outside [0, C) is a wrong row.
__global__ __launch_bounds__(256) void k_head_rank(const float* x, const long long* target, int C, int* rank_rows) {
    __shared__ int redi[4];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* row = x + (size_t)n * C;
    const long long t = target[n];
    const bool valid = t >= 0 && t < C;
    const float zt = valid ? row[t] : 0.f;
    const int ti = (int)t;
    int above = 0;
    for (int c = tid; c < C; c += 256) {
        const float z = row[c];
        above += (z > zt || (z == zt && c < ti)) ? 1 : 0;
    }
    above = head_wg_reduce_int(above, redi);
    if (tid == 0) rank_rows[n] = (valid && isfinite(zt)) ? above : HEAD_RANK_WRONG;
}

__global__ __launch_bounds__(256) void k_head_meters(const int* rank_rows, int N, HeadKs ks, const float* loss, MnasMeters* meters) {
    __shared__ int redi[4];
    head_meters_update(rank_rows, N, ks, loss, meters, redi);
}

extern "C" int mnas_head_metrics(const void* logits, const void* target, int N, int C, const int* ks, int nk, const void* loss,
                                 void* rank_rows, MnasMeters* meters, void* stream) {
    if (!logits || !target || !rank_rows || !meters || N < 1 || C < 1) return MNAS_EINVAL;
    HeadKs k;
    if (head_ks(ks, nk, C, &k) != MNAS_OK) return MNAS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_head_rank, dim3(N), dim3(256), 0, s, (const float*)logits, (const long long*)target, C, (int*)rank_rows);
    MNAS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_head_meters, dim3(1), dim3(256), 0, s, (const int*)rank_rows, N, k, (const float*)loss, meters);
    MNAS_CHECK_LAUNCH();
    return MNAS_OK;
}
