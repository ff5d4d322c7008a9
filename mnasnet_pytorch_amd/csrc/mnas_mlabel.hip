// The multi-label branch of the step: MultiClassBCELoss (BCE-with-logits, optional element weights, optional focal transform of
// the MEAN), its gradient, HardDice and the per-sample macro-F1 of batch_metrics, plus the three AverageMeters of that branch in one
// MnasMultiLabelMeters block in device memory (train.py:274-279, 453-463, 577-587).  The arithmetic rule is stated once in
// include/mnas.h.  Replaces, per step, ATen's BCE forward / backward kernels, a copy of the N x C logits to the host and N
// scikit-learn calls by two launches (three with focal: the gradient needs the batch loss before it can be scaled):
//     k_mlabel_row    one 256-lane workgroup per row: the row's loss sum, its integer counts, its F1 (double) and the gradient
//                     scaled by 1/(N*C)
//     k_mlabel_batch  one workgroup: mean, focal transform, Dice, the ordered F1 sum, and the block update by one thread
//     k_mlabel_scale  focal only: dlogits *= s
// mnas_mlabel_loss is the branch's current recipe on the same two launches (include/mnas.h "multi-label loss"): per-element
// asymmetric focusing with a margin, pos_weight, binary label smoothing and mixed label rows formed on load:
//     k_mlabel_row_ex<VEC, ASYM, MIX>   k_mlabel_row's twin; the gradient is final after it (nothing waits for the batch mean)
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

// one class of one row, the counts: true iff the label is exactly 1; predicted iff z >= 0 (F1) / z > thr (Dice); NaN: both false
__device__ __forceinline__ void ml_count(float z, float y, float thr, MlAcc& c) {
    const bool tr = y == 1.f, p1 = z >= 0.f, pd = z > thr;
    c.T += tr; c.P1 += p1; c.tp1 += (p1 && tr); c.Pd += pd; c.Id += (pd && tr);
}

// one class of one row, BCE-with-logits: the loss element into c.ls, the gradient element returned
__device__ __forceinline__ float ml_bce(float z, float t, float w, float inv, MlAcc& c) {
    const float ea = expf(-fabsf(z));
    const float e = fmaxf(z, 0.f) - z * t + log1pf(ea);
    c.ls += e * w;
    const float sg = z >= 0.f ? 1.f / (1.f + ea) : ea / (1.f + ea);
    return w * (sg - t) * inv;
}

// one class of one row: loss element, gradient element (returned), counts
__device__ __forceinline__ float ml_elem(float z, float t, float w, const MlRowArgs& a, MlAcc& c) {
    ml_count(z, t, a.thr, c);
    if (!a.do_loss) return 0.f;
    return ml_bce(z, t, w, a.inv, c);
}

// the end of a row's workgroup: in-wave butterflies, then the four waves' partials through LDS, added in wave order; thread 0
// stores the row's loss sum, its Dice counts and its F1
__device__ __forceinline__ void ml_row_finish(MlAcc c, float* redf, int (*redi)[5], const MlScratch& sc, int do_loss, int n, int C) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
    if (do_loss) sc.loss_rows[n] = ((redf[0] + redf[1]) + redf[2]) + redf[3];
    sc.cT[n] = s[0]; sc.cP[n] = s[3]; sc.cI[n] = s[4];
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
    sc.f1_rows[n] = f;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_mlabel_row(MlRowArgs a) {
    __shared__ float redf[4];
    __shared__ int redi[4][5];
    const int n = blockIdx.x, tid = threadIdx.x, C = a.C;
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
    ml_row_finish(c, redf, redi, a.s, a.do_loss, n, C);
}

// ---- mnas_mlabel_loss: the row launch (include/mnas.h "multi-label loss" states the rule and the forms below) ----
struct MlxRowArgs {
    MlRowArgs r;                                         // z, t = the label matrix Y, w, dl, C, inv (1/(N*C) or 1/N), s
    const long long* partner; const float* lam;          // MIX: [N] each
    const float* pw;                                     // pos_weight [C] or NULL (ASYM only)
    int N, smooth;                                       // smooth: label smoothing is on
    float gp, gn, margin;                                // gamma+, gamma-, m
    float om_eps, h_eps;                                 // smoothing: t = fmaf(1 - eps, y, eps / 2)
};

// The general element (ASYM): focusing, margin or pos_weight.  t: the smoothed label, p: the class's positive weight.  Every
// multiply that feeds an add is an explicit fmaf and everything else a statement of its own, so under -ffp-contract=on the
// roundings are exactly the ones written here.
__device__ __forceinline__ float mlx_asym(float z, float t, float w, float p, const MlxRowArgs& a, MlAcc& c) {
    const float ea = expf(-fabsf(z));
    const float l1 = log1pf(ea);
    const float spp = fmaxf(z, 0.f) + l1;                // sp(z)  = -log(1 - sigma)
    const float spn = fmaxf(-z, 0.f) + l1;               // sp(-z) = -log(sigma) = L+
    const float d = 1.f + ea;
    const float q1 = 1.f / d, qe = ea / d;
    const float sg = z >= 0.f ? q1 : qe;                 // sigma
    const float oms = z >= 0.f ? qe : q1;                // 1 - sigma, without cancellation
    // positive branch
    float Fp = 1.f, dpos = -oms;
    if (a.gp != 0.f) {
        const float ap = a.gp * spp;
        Fp = expf(-ap);                                  // (1 - sigma)^gamma+
        const float gs = a.gp * sg;
        const float ip = fmaf(gs, spn, oms);
        dpos = -(Fp * ip);
    }
    // negative branch
    float Fn = 1.f, Ln, dneg;
    if (a.margin == 0.f) {
        Ln = spp;
        if (a.gn != 0.f) {
            const float an = a.gn * spn;
            Fn = expf(-an);                              // sigma^gamma-, log(sigma) = -sp(-z)
            const float go = a.gn * oms;
            const float in = fmaf(go, spp, sg);
            dneg = Fn * in;
        } else {
            dneg = sg;
        }
    } else {
        const float sm = sg - a.margin;
        if (sm > 0.f) {                                  // strict; a NaN sigma takes the other side (the positive branch carries it)
            const float om = 1.f - sm;
            Ln = -log1pf(-sm);
            float P1 = 0.f;                              // gamma- sigma_m^(gamma- - 1); 0 for gamma- = 0
            if (a.gn != 0.f) {
                const float lsm = logf(sm);
                const float an = a.gn * lsm;
                Fn = expf(an);
                const float a1 = (a.gn - 1.f) * lsm;
                const float e1 = expf(a1);
                P1 = a.gn * e1;
            }
            const float qn = Fn / om;
            const float in = fmaf(P1, Ln, qn);
            const float so = sg * oms;
            dneg = so * in;
        } else {
            Fn = a.gn != 0.f ? 0.f : 1.f;
            Ln = 0.f;
            dneg = 0.f;
        }
    }
    const float pt = p * t;
    const float omt = 1.f - t;
    const float fl = Fp * spn;
    const float ep = pt * fl;
    const float fn = Fn * Ln;
    const float e = fmaf(omt, fn, ep);
    c.ls = fmaf(e, w, c.ls);
    const float gpos = pt * dpos;
    const float g = fmaf(omt, dneg, gpos);
    const float wg = w * g;
    return wg * a.r.inv;
}

// y: the row's raw label, y2: the partner row's; lam: the weight of y.  -> the gradient element
template <bool ASYM, bool MIX>
__device__ __forceinline__ float mlx_elem(float z, float y, float y2, float w, float p, float lam, float oml, const MlxRowArgs& a,
                                          MlAcc& c) {
    float t = y;
    if (MIX) {
        ml_count(z, lam >= 0.5f ? y : y2, 0.f, c);       // the dominant image's raw label (a bad row: lam is NaN and y2 is y)
        const float b = oml * y2;
        t = fmaf(lam, y, b);
    } else {
        ml_count(z, y, 0.f, c);
    }
    if (a.smooth) t = fmaf(a.om_eps, t, a.h_eps);
    if (ASYM) return mlx_asym(z, t, w, p, a, c);
    return ml_bce(z, t, w, a.r.inv, c);
}

template <bool VEC, bool ASYM, bool MIX>
__global__ __launch_bounds__(256) void k_mlabel_row_ex(MlxRowArgs a) {
    __shared__ float redf[4];
    __shared__ int redi[4][5];
    const int n = blockIdx.x, tid = threadIdx.x, C = a.r.C;
    const size_t base = (size_t)n * C;
    const float *z = a.r.z + base, *y = a.r.t + base, *w = a.r.w ? a.r.w + base : nullptr;
    const float* pw = ASYM ? a.pw : nullptr;
    const float* y2 = y;
    float lam = 1.f, oml = 0.f;
    if (MIX) {
        const long long p = a.partner[n];
        lam = a.lam[n];
        if (p >= 0 && p < (long long)a.N && lam >= 0.f && lam <= 1.f) {
            y2 = a.r.t + (size_t)p * C;
            oml = 1.f - lam;
        } else {                                         // a bad row reads no partner row; NaN labels make its loss and gradient NaN
            lam = __builtin_nanf("");
            oml = lam;
        }
    }
    float* dl = a.r.dl ? a.r.dl + base : nullptr;
    MlAcc c = {0.f, 0, 0, 0, 0, 0};
    if (VEC) {                                           // C % 4 == 0 and every pointer 16-byte aligned (checked on the host)
        const float4 one = make_float4(1.f, 1.f, 1.f, 1.f);
        for (int i = tid * 4; i < C; i += 1024) {
            const float4 zv = *(const float4*)(z + i), yv = *(const float4*)(y + i);
            const float4 y2v = MIX ? *(const float4*)(y2 + i) : yv;
            const float4 wv = w ? *(const float4*)(w + i) : one;
            const float4 pv = pw ? *(const float4*)(pw + i) : one;
            float4 g;
            g.x = mlx_elem<ASYM, MIX>(zv.x, yv.x, y2v.x, wv.x, pv.x, lam, oml, a, c);
            g.y = mlx_elem<ASYM, MIX>(zv.y, yv.y, y2v.y, wv.y, pv.y, lam, oml, a, c);
            g.z = mlx_elem<ASYM, MIX>(zv.z, yv.z, y2v.z, wv.z, pv.z, lam, oml, a, c);
            g.w = mlx_elem<ASYM, MIX>(zv.w, yv.w, y2v.w, wv.w, pv.w, lam, oml, a, c);
            if (dl) *(float4*)(dl + i) = g;
        }
    } else {
        for (int i = tid; i < C; i += 256) {
            const float yi = y[i];
            const float g = mlx_elem<ASYM, MIX>(z[i], yi, MIX ? y2[i] : yi, w ? w[i] : 1.f, pw ? pw[i] : 1.f, lam, oml, a, c);
            if (dl) dl[i] = g;
        }
    }
    ml_row_finish(c, redf, redi, a.r.s, 1, n, C);
}

struct MlBatchArgs {
    MlScratch s;
    int N, C;
    int do_loss, focal, deduct;
    int rows;                             // the loss is the sum of the row sums over N (mnas_mlabel_loss, reduction "rows"), not N*C
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
        const float b = (float)(S / (a.rows ? (double)N : (double)N * (double)a.C));
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

static bool ml_gamma_ok(float g) { return g == 0.f || (g >= 1.f && g <= 16.f); }          // refuses NaN

template <bool ASYM, bool MIX>
static int mlx_launch_row(const MlxRowArgs& a, bool vec, hipStream_t s) {
    if (vec) hipLaunchKernelGGL((k_mlabel_row_ex<true, ASYM, MIX>), dim3(a.N), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_mlabel_row_ex<false, ASYM, MIX>), dim3(a.N), dim3(256), 0, s, a);
    MNAS_CHECK_LAUNCH();
    return MNAS_OK;
}

extern "C" int mnas_mlabel_loss(const void* logits, const void* labels, const void* partner, const void* lam, const void* weights,
                                const void* pos_weight, int N, int C, const MnasMlabelLoss* cfg, void* scratch, void* loss,
                                void* dlogits, MnasMultiLabelMeters* meters, int64_t n_loss, int64_t n_dice, int64_t n_f1,
                                void* stream) {
    if (!logits || !labels || !cfg || !scratch || !loss || N < 1 || C < 1 || !ml_al16(scratch)) return MNAS_EINVAL;
    if ((partner == nullptr) != (lam == nullptr)) return MNAS_EINVAL;
    if (!ml_gamma_ok(cfg->gamma_pos) || !ml_gamma_ok(cfg->gamma_neg)) return MNAS_EINVAL;
    if (!(cfg->margin >= 0.f && cfg->margin <= 0.5f) || !(cfg->smoothing >= 0.f && cfg->smoothing < 1.f)) return MNAS_EINVAL;
    if (cfg->reduction != MNAS_MLABEL_MEAN && cfg->reduction != MNAS_MLABEL_ROWS) return MNAS_EINVAL;
    if (cfg->reserved[0] || cfg->reserved[1] || cfg->reserved[2]) return MNAS_EINVAL;
    if (!ml_weights_ok(meters, n_loss, n_dice, n_f1)) return MNAS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const bool rows = cfg->reduction == MNAS_MLABEL_ROWS;
    MlxRowArgs a = {};
    a.r.z = (const float*)logits; a.r.t = (const float*)labels; a.r.w = (const float*)weights; a.r.dl = (float*)dlogits;
    a.r.C = C; a.r.do_loss = 1;
    a.r.inv = rows ? (float)(1.0 / (double)N) : (float)(1.0 / ((double)N * (double)C));
    a.r.thr = 0.f;
    a.r.s = ml_scratch(scratch, N);
    a.partner = (const long long*)partner; a.lam = (const float*)lam; a.pw = (const float*)pos_weight;
    a.N = N; a.smooth = cfg->smoothing != 0.f;
    a.gp = cfg->gamma_pos; a.gn = cfg->gamma_neg; a.margin = cfg->margin;
    a.om_eps = 1.f - cfg->smoothing; a.h_eps = 0.5f * cfg->smoothing;
    const bool asym = a.gp != 0.f || a.gn != 0.f || a.margin != 0.f || pos_weight != nullptr;
    const bool vec = (C & 3) == 0 && ml_al16(logits) && ml_al16(labels) && ml_al16(weights) && ml_al16(pos_weight) && ml_al16(dlogits);
    int rc;
    if (asym) rc = partner ? mlx_launch_row<true, true>(a, vec, s) : mlx_launch_row<true, false>(a, vec, s);
    else rc = partner ? mlx_launch_row<false, true>(a, vec, s) : mlx_launch_row<false, false>(a, vec, s);
    if (rc != MNAS_OK) return rc;
    MlBatchArgs b = {};
    b.s = a.r.s; b.N = N; b.C = C; b.do_loss = 1; b.rows = rows ? 1 : 0;
    b.loss_out = (float*)loss;
    b.m = meters; b.n_loss = n_loss; b.n_dice = n_dice; b.n_f1 = n_f1;
    hipLaunchKernelGGL(k_mlabel_batch, dim3(1), dim3(256), 0, s, b);
    MNAS_CHECK_LAUNCH();
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
