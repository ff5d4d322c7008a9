// The multi-label branch of the step: MultiClassBCELoss (BCE-with-logits, optional element weights, optional focal transform of
// the MEAN), its gradient, HardDice and the per-sample macro-F1 of batch_metrics, plus the three AverageMeters of that branch in one
// MnasMultiLabelMeters block in device memory (train.py:274-279, 453-463, 577-587).  The arithmetic rule is stated once in
// include/mnas.h.  Replaces, per step, ATen's BCE forward / backward kernels, a copy of the N x C logits to the host and N
// scikit-learn calls by two launches (three with focal: the gradient needs the batch loss before it can be scaled):
//     k_mlabel_row    one 256-lane workgroup per row: the row's loss sum, its integer counts, its F1 (double) and the gradient
//                     scaled by 1/(N*C)
//     k_mlabel_batch  one workgroup: mean, focal transform, Dice, the ordered F1 sum, and the block update by one thread
//     k_mlabel_scale  focal only: dlogits *= s
// Deterministic: fixed summation order, no atomics.  fp32 throughout; the N row sums and the focal transform in double.
#include "mnas_common.h"

struct MlScratch {                        // views into the caller's scratch (mnas_mlabel_scratch_bytes)
    double* f1_rows;                      // [N] F1 of every row
    float* loss_rows;                     // [N] sum of the row's loss elements
    int* cI; int* cP; int* cT;            // [N] each, Dice rule: predicted and true / predicted / true
    float* scale;                         // [1] focal: the gradient's factor s
};

static MlScratch ml_scratch(void* p, int N) {
    char* b = (char*)p;
    MlScratch s;
    s.f1_rows = (double*)b;
    s.loss_rows = (float*)(b + (size_t)8 * N);
    s.cI = (int*)(b + (size_t)12 * N);
    s.cP = s.cI + N;
    s.cT = s.cP + N;
    s.scale = (float*)(b + (size_t)24 * N);
    return s;
}

extern "C" int64_t mnas_mlabel_scratch_bytes(int N) { return N < 1 ? 0 : (int64_t)24 * N + 16; }

struct MlRowArgs {
    const float* z; const float* t; const float* w;     // w: NULL = no weights
    float* dl;                                           // NULL = no gradient
    int C, do_loss;                                      // do_loss = 0: counts only (z and t are read, nothing else)
    float inv, thr;                                      // 1/(N*C); the Dice rule's threshold on the logit
    MlScratch s;
};

struct MlAcc { float ls; int T, P1, tp1, Pd, Id; };

// one class of one row: loss element, gradient element (returned), counts
__device__ __forceinline__ float ml_elem(float z, float t, float w, const MlRowArgs& a, MlAcc& c) {
    const bool tr = t == 1.f, p1 = z >= 0.f, pd = z > a.thr;          // NaN: both false
    c.T += tr; c.P1 += p1; c.tp1 += (p1 && tr); c.Pd += pd; c.Id += (pd && tr);
    if (!a.do_loss) return 0.f;
    const float ea = expf(-fabsf(z));
    const float e = fmaxf(z, 0.f) - z * t + log1pf(ea);
    c.ls += e * w;
    const float sg = z >= 0.f ? 1.f / (1.f + ea) : ea / (1.f + ea);
    return w * (sg - t) * a.inv;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_mlabel_row(MlRowArgs a) {
    __shared__ float redf[4];
    __shared__ int redi[4][5];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, C = a.C;
    const size_t base = (size_t)n * C;
    const float *z = a.z + base, *t = a.t + base, *w = a.w ? a.w + base : nullptr;
    float* dl = a.dl ? a.dl + base : nullptr;
    MlAcc c = {0.f, 0, 0, 0, 0, 0};
    if (VEC) {                                           // C % 4 == 0 and every pointer 16-byte aligned (checked on the host)
        for (int i = tid * 4; i < C; i += 1024) {
            const float4 zv = *(const float4*)(z + i), tv = *(const float4*)(t + i);
            const float4 wv = w ? *(const float4*)(w + i) : make_float4(1.f, 1.f, 1.f, 1.f);
            float4 g;
            g.x = ml_elem(zv.x, tv.x, wv.x, a, c);
            g.y = ml_elem(zv.y, tv.y, wv.y, a, c);
            g.z = ml_elem(zv.z, tv.z, wv.z, a, c);
            g.w = ml_elem(zv.w, tv.w, wv.w, a, c);
            if (dl) *(float4*)(dl + i) = g;
        }
    } else {
        for (int i = tid; i < C; i += 256) {
            const float g = ml_elem(z[i], t[i], w ? w[i] : 1.f, a, c);
            if (dl) dl[i] = g;
        }
    }
    // in-wave butterflies, then the four waves' partials through LDS, added in wave order
    int v[5] = {c.T, c.P1, c.tp1, c.Pd, c.Id};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c.ls += __shfl_xor(c.ls, o, 64);
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] += __shfl_xor(v[q], o, 64);
    }
    if (lane == 0) {
        redf[wave] = c.ls;
#pragma unroll
        for (int q = 0; q < 5; ++q) redi[wave][q] = v[q];
    }
    __syncthreads();
    if (tid != 0) return;
    int s[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) s[q] = ((redi[0][q] + redi[1][q]) + redi[2][q]) + redi[3][q];
    if (a.do_loss) a.s.loss_rows[n] = ((redf[0] + redf[1]) + redf[2]) + redf[3];
    a.s.cT[n] = s[0]; a.s.cP[n] = s[3]; a.s.cI[n] = s[4];
    // macro-F1 over the labels present in the row (F1 rule: predicted iff z >= 0)
    const int tp = s[2], fp = s[1] - s[2], fn = s[0] - s[2], tn = C - tp - fp - fn;
    double f = 0.0;
    int k = 0;
    if (tp + fp + fn > 0) { f = __ddiv_rn((double)(2 * (long long)tp), (double)(2 * (long long)tp + fp + fn)); ++k; }
    if (tn + fp + fn > 0) {
        const double f0 = __ddiv_rn((double)(2 * (long long)tn), (double)(2 * (long long)tn + fp + fn));
        f = k ? __dadd_rn(f, f0) * 0.5 : f0;
        ++k;
    }
    a.s.f1_rows[n] = f;
}

struct MlBatchArgs {
    MlScratch s;
    int N, C;
    int do_loss, focal, deduct;
    float gamma, balance;
    float* loss_out;                      // do_loss: the loss
    const float* ext_loss;                // !do_loss: the caller's loss for the loss meter, or NULL
    float* dice_out;                      // the HardDice value, or NULL
    MnasMultiLabelMeters* m;              // or NULL
    long long n_loss, n_dice, n_f1;
};

// clamp(1 + log(2I/U), 0, 1) in fp32; 0 when nothing was hit (the reference's log(0) = -inf, clamped)
__device__ __forceinline__ float ml_dice(long long I, long long P, long long T, int deduct) {
    if (I <= 0) return 0.f;
    const long long U = P + T - (deduct ? I : 0);
    const float v = 1.f + logf((float)(2 * I) / (float)U);
    return fminf(fmaxf(v, 0.f), 1.f);
}

// AverageMeter.update(val, n): one rounded product, one rounded sum.  The F1 value has 53 significant bits, so val * n is not
// exact and a fused multiply-add would round once where Python rounds twice.  The _rn intrinsics are plain operators to the
// compiler, and under hipcc's default -ffp-contract=fast the backend fuses them whatever the source says (a contract pragma
// included): the Makefile builds this file with -ffp-contract=on, which fuses within one expression only.
__device__ __forceinline__ void ml_meter(double val, long long n, double* sum, int64_t* cnt, double* last, double* last_sum,
                                         int64_t* last_n) {
    const double vn = __dmul_rn(val, (double)n);
    *sum = __dadd_rn(*sum, vn);
    *cnt += n;
    *last = val;
    *last_sum = vn;
    *last_n = n;
}

__global__ __launch_bounds__(256) void k_mlabel_batch(MlBatchArgs a) {
    __shared__ double redd[4];
    __shared__ long long redl[4][3];
    __shared__ double f1s[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = a.N;
    double ls = 0.0;
    long long v[3] = {0, 0, 0};
    for (int i = tid; i < N; i += 256) {
        if (a.do_loss) ls += (double)a.s.loss_rows[i];
        v[0] += a.s.cI[i]; v[1] += a.s.cP[i]; v[2] += a.s.cT[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ls += __shfl_xor(ls, o, 64);
#pragma unroll
        for (int q = 0; q < 3; ++q) v[q] += __shfl_xor(v[q], o, 64);
    }
    if (lane == 0) {
        redd[wave] = ls;
#pragma unroll
        for (int q = 0; q < 3; ++q) redl[wave][q] = v[q];
    }
    // the rows' F1 in ROW order by one thread (chunks of 256 staged through LDS by all of them)
    double fsum = 0.0;
    if (a.m) {
        for (int i0 = 0; i0 < N; i0 += 256) {
            __syncthreads();
            if (i0 + tid < N) f1s[tid] = a.s.f1_rows[i0 + tid];
            __syncthreads();
            if (tid == 0) {
                const int cnt = N - i0 < 256 ? N - i0 : 256;
                for (int j = 0; j < cnt; ++j) fsum = __dadd_rn(fsum, f1s[j]);
            }
        }
    }
    __syncthreads();
    if (tid != 0) return;
    const double S = ((redd[0] + redd[1]) + redd[2]) + redd[3];
    long long t[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) t[q] = ((redl[0][q] + redl[1][q]) + redl[2][q]) + redl[3][q];
    const long long I = t[0], P = t[1], T = t[2];
    float loss = 0.f;
    bool have_loss = false;
    if (a.do_loss) {
        const float b = (float)(S / ((double)N * (double)a.C));
        loss = b;
        if (a.focal) {
            const double bd = (double)b, g = (double)a.gamma, pt = exp(-bd), om = 1.0 - pt;
            loss = (float)((double)a.balance * pow(om, g) * bd);
            *a.s.scale = (float)((double)a.balance * pow(om, g - 1.0) * (om + g * pt * bd));
        }
        *a.loss_out = loss;
        have_loss = true;
    } else if (a.ext_loss) {
        loss = *a.ext_loss;
        have_loss = true;
    }
    const float dice = ml_dice(I, P, T, a.deduct);
    if (a.dice_out) *a.dice_out = dice;
    MnasMultiLabelMeters* m = a.m;
    if (!m) return;
    m->steps += 1;
    m->samples += N;
    m->last_n = N;
    m->tp += I; m->fp += P - I; m->fn += T - I;
    m->last_tp = I; m->last_fp = P - I; m->last_fn = T - I;
    ml_meter((double)dice, a.n_dice, &m->dice_sum, &m->dice_n, &m->last_dice, &m->last_dice_sum, &m->last_dice_n);
    ml_meter(__ddiv_rn(fsum, (double)N), a.n_f1, &m->f1_sum, &m->f1_n, &m->last_f1, &m->last_f1_sum, &m->last_f1_n);
    if (have_loss) {
        ml_meter((double)loss, a.n_loss, &m->loss_sum, &m->loss_n, &m->last_loss, &m->last_loss_sum, &m->last_loss_n);
        if (!isfinite(loss)) m->nonfinite_steps += 1;
    }
}

// focal: dlogits *= s (s from the batch stage)
__global__ __launch_bounds__(256) void k_mlabel_scale(float* dl, long long n, const float* scale) {
    const float s = *scale;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dl[i] *= s;
}

static bool ml_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int ml_launch_row(const MlRowArgs& a, int N, hipStream_t s) {
    const bool vec = (a.C & 3) == 0 && ml_al16(a.z) && ml_al16(a.t) && ml_al16(a.w) && ml_al16(a.dl);
    if (vec) hipLaunchKernelGGL(k_mlabel_row<true>, dim3(N), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_mlabel_row<false>, dim3(N), dim3(256), 0, s, a);
    MNAS_CHECK_LAUNCH();
    return MNAS_OK;
}

static bool ml_weights_ok(const MnasMultiLabelMeters* m, int64_t n_loss, int64_t n_dice, int64_t n_f1) {
    return !m || (n_loss >= 0 && n_dice >= 0 && n_f1 >= 0);
}

extern "C" int mnas_mlabel_bce(const void* logits, const void* target, const void* weights, int N, int C, int focal, float focus_param,
                               float balance_param, void* scratch, void* loss, void* dlogits, MnasMultiLabelMeters* meters,
                               int64_t n_loss, int64_t n_dice, int64_t n_f1, void* stream) {
    if (!logits || !target || !scratch || !loss || N < 1 || C < 1 || !ml_al16(scratch)) return MNAS_EINVAL;
    if (focal && !(focus_param >= 1.f)) return MNAS_EINVAL;        // (1-pt)^(gamma-1) in the gradient; also refuses NaN
    if (!ml_weights_ok(meters, n_loss, n_dice, n_f1)) return MNAS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    MlRowArgs r = {};
    r.z = (const float*)logits; r.t = (const float*)target; r.w = (const float*)weights; r.dl = (float*)dlogits;
    r.C = C; r.do_loss = 1;
    r.inv = (float)(1.0 / ((double)N * (double)C)); r.thr = 0.f;
    r.s = ml_scratch(scratch, N);
    int rc = ml_launch_row(r, N, s);
    if (rc != MNAS_OK) return rc;
    MlBatchArgs b = {};
    b.s = r.s; b.N = N; b.C = C; b.do_loss = 1; b.focal = focal ? 1 : 0;
    b.gamma = focus_param; b.balance = balance_param;
    b.loss_out = (float*)loss;
    b.m = meters; b.n_loss = n_loss; b.n_dice = n_dice; b.n_f1 = n_f1;
    hipLaunchKernelGGL(k_mlabel_batch, dim3(1), dim3(256), 0, s, b);
    MNAS_CHECK_LAUNCH();
    if (focal && dlogits) {
        const long long n = (long long)N * C;
        const long long blocks = (n + 255) / 256;
        hipLaunchKernelGGL(k_mlabel_scale, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, (float*)dlogits, n,
                           (const float*)r.s.scale);
        MNAS_CHECK_LAUNCH();
    }
    return MNAS_OK;
}

extern "C" int mnas_mlabel_metrics(const void* logits, const void* target, int N, int C, const void* loss, void* scratch,
                                   MnasMultiLabelMeters* meters, int64_t n_loss, int64_t n_dice, int64_t n_f1, void* stream) {
    if (!logits || !target || !scratch || !meters || N < 1 || C < 1 || !ml_al16(scratch)) return MNAS_EINVAL;
    if (!ml_weights_ok(meters, n_loss, n_dice, n_f1)) return MNAS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    MlRowArgs r = {};
    r.z = (const float*)logits; r.t = (const float*)target; r.C = C; r.thr = 0.f;
    r.s = ml_scratch(scratch, N);
    int rc = ml_launch_row(r, N, s);
    if (rc != MNAS_OK) return rc;
    MlBatchArgs b = {};
    b.s = r.s; b.N = N; b.C = C;
    b.ext_loss = (const float*)loss;
    b.m = meters; b.n_loss = n_loss; b.n_dice = n_dice; b.n_f1 = n_f1;
    hipLaunchKernelGGL(k_mlabel_batch, dim3(1), dim3(256), 0, s, b);
    MNAS_CHECK_LAUNCH();
    return MNAS_OK;
}

extern "C" int mnas_mlabel_hard_dice(const void* logits, const void* target, int N, int C, float threshold_logit,
                                     int deduct_intersection, void* scratch, void* out, void* stream) {
    if (!logits || !target || !scratch || !out || N < 1 || C < 1 || !ml_al16(scratch)) return MNAS_EINVAL;
    if (threshold_logit != threshold_logit) return MNAS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    MlRowArgs r = {};
    r.z = (const float*)logits; r.t = (const float*)target; r.C = C; r.thr = threshold_logit;
    r.s = ml_scratch(scratch, N);
    int rc = ml_launch_row(r, N, s);
    if (rc != MNAS_OK) return rc;
    MlBatchArgs b = {};
    b.s = r.s; b.N = N; b.C = C; b.deduct = deduct_intersection ? 1 : 0;
    b.dice_out = (float*)out;
    hipLaunchKernelGGL(k_mlabel_batch, dim3(1), dim3(256), 0, s, b);
    MNAS_CHECK_LAUNCH();
    return MNAS_OK;
}
