// ABI glue: version query and the batched launcher (one host->library transition per forward / backward
// segment instead of ~450 ctypes calls per training step).
#include "mnas_common.h"

#define MNAS_NT_DEFAULT MNAS_NT_PWF
MNAS_SWITCH(mnas_nt_mask, mnas_diag_env("MNAS_NT", MNAS_NT_DEFAULT))

MNAS_SWITCH(mnas_pwf_enabled, mnas_diag_env("MNAS_PWF", 1))
MNAS_SWITCH(mnas_pwd_enabled, mnas_diag_env("MNAS_PWD", 1) && mnas_pwf_enabled())

MNAS_SWITCH(mnas_pws_enabled, mnas_diag_env("MNAS_PWS", 2))  // 0: off, 1: forward only, 2: forward + input gradient

extern "C" int mnas_version(void) { return 8; }
extern "C" const char* mnas_arch(void) { return "gfx950"; }

extern "C" int64_t mnas_workspace_bytes(int kind, int n, int c, int k) {
    if (n < 1 || c < 1) return -1;
    switch (kind) {
        case MNAS_WS_CONV_STATS: return (int64_t)2 * c * n * sizeof(float);
        case MNAS_WS_CONV_WGRAD:
        case MNAS_WS_PW_BWD:
        case MNAS_WS_DW_WGRAD:   return k < 1 ? -1 : (int64_t)n * c * k * sizeof(float);
        default: return -1;
    }
}

// What each slot of op.i / op.d / op.p means per opcode: OP_SLOTS in mnasnet_pytorch_amd/_lib.py, the one table, which
// tests/test_abi_cpu.py holds to the indices read below (i[14]: the stream, mnas_run_ops_multi).
static int run_one(const MnasOp& o, void* stream) {
    const int32_t* i = o.i;
    void* const* p = o.p;
    switch (o.opcode) {
        case MNAS_OP_CONV_GEMM: {
            MnasConvGemm a = {};
            a.mode = i[0]; a.N = i[1]; a.Hi = i[2]; a.Wi = i[3]; a.Ci = i[4]; a.Ho = i[5]; a.Wo = i[6]; a.Co = i[7];
            a.kh = i[8]; a.kw = i[9]; a.stride = i[10]; a.pad = i[11]; a.nparts = i[12];
            a.act.data = p[0]; a.act.scale = (const float*)p[1]; a.act.shift = (const float*)p[2];
            a.grad.g = p[3]; a.grad.y = p[4]; a.grad.coef = (const float*)p[5];
            a.w = p[6]; a.bias = (const float*)p[7]; a.resid = p[8]; a.out = p[9]; a.stats = (float*)p[10];
            a.red_y = p[11]; a.red_bn = (const float*)p[12];
            a.gate = (const float*)p[13];
            return mnas_conv_gemm(&a, stream);
        }
        case MNAS_OP_CONV_WGRAD: {
            MnasConvWgrad a = {};
            a.N = i[0]; a.Hi = i[1]; a.Wi = i[2]; a.Ci = i[3]; a.Ho = i[4]; a.Wo = i[5]; a.Co = i[6];
            a.kh = i[7]; a.kw = i[8]; a.stride = i[9]; a.pad = i[10]; a.nsplit = i[11];
            a.x.data = p[0]; a.x.scale = (const float*)p[1]; a.x.shift = (const float*)p[2];
            a.dy.g = p[3]; a.dy.y = p[4]; a.dy.coef = (const float*)p[5];
            a.partial = (float*)p[6];
#ifdef MNAS_DIAG
            {   // diagnosis build only (MNAS_ABL_NOWGRAD=1|2|3): skip the launch -- upper bound of what the side stream costs the main one
                static int skip = -1;
                if (skip < 0) skip = mnas_diag_env("MNAS_ABL_NOWGRAD", 0);
                if ((skip == 1 && a.kh == 1) || (skip == 2 && a.kh == 3) || skip == 3) return MNAS_OK;      // 1: 1x1, 2: 3x3, 3: all
            }
#endif
            return mnas_conv_wgrad(&a, stream);
        }
        case MNAS_OP_PACK_BATCH:
            return mnas_pack_weights_batch((const MnasPackDesc*)p[0], i[0], stream);
        case MNAS_OP_PW_BWD: {
            MnasPwBwd a = {};
            a.M = i[0]; a.Ci = i[1]; a.Co = i[2]; a.nparts = i[3];
            a.x.data = p[0]; a.x.scale = (const float*)p[1]; a.x.shift = (const float*)p[2];
            a.dy.g = p[3]; a.dy.y = p[4]; a.dy.coef = (const float*)p[5];
            a.w = p[6]; a.resid = p[7]; a.gin = p[8]; a.wpartial = (float*)p[9];
            a.red_partial = (float*)p[10]; a.red_y = p[11]; a.red_bn = (const float*)p[12];
            a.w_fwd = p[14]; a.b_fwd = (const float*)p[15];        // (p[13], i[6]: the retired NOGIN / RED4 forms' slots)
            a.gin_masked = i[4]; a.seg_px = i[5];
            return mnas_pw_bwd(&a, stream);
        }
        case MNAS_OP_WGRAD_FINALIZE:
            return mnas_wgrad_finalize((float*)p[0], i[0], i[1], i[2], i[3], (float*)p[1], i[4], stream);
        case MNAS_OP_DW_FWD: {
            MnasDwFwd a = {};
            a.N = i[0]; a.H = i[1]; a.W = i[2]; a.C = i[3]; a.k = i[4]; a.nparts = i[5];
            a.in.data = p[0]; a.in.scale = (const float*)p[1]; a.in.shift = (const float*)p[2];
            a.w = (const float*)p[3]; a.bias = (const float*)p[4]; a.out = p[5]; a.stats = (float*)p[6];
            a.stride = i[6];
            return mnas_dw_fwd(&a, stream);
        }
        case MNAS_OP_DW_BWD: {
            MnasDwBwd a = {};
            a.N = i[0]; a.H = i[1]; a.W = i[2]; a.C = i[3]; a.k = i[4]; a.nparts = i[5];
            a.x.data = p[0]; a.x.scale = (const float*)p[1]; a.x.shift = (const float*)p[2];
            a.dy.g = p[3]; a.dy.y = p[4]; a.dy.coef = (const float*)p[5];
            a.w = (const float*)p[6]; a.gin = p[7]; a.wpartial = (float*)p[8];
            a.red_bn = (const float*)p[9]; a.red_partial = (float*)p[10]; a.phase = i[6];
            a.g_masked = i[8]; a.stride = i[7];     // (p[11..15]: the retired SRC / g-affine forms' slots)
            return mnas_dw_bwd(&a, stream);
        }
        case MNAS_OP_DW_WGRAD_FINALIZE:
            return mnas_dw_wgrad_finalize((float*)p[0], i[0], i[1], i[2], (float*)p[1], i[3], stream);
        case MNAS_OP_STEM_FWD: {
            MnasStemFwd a = {};
            a.N = i[0]; a.H = i[1]; a.W = i[2]; a.Ho = i[3]; a.Wo = i[4]; a.Co = i[5]; a.nparts = i[6];
            a.x = (const float*)p[0]; a.w = p[1]; a.bias = (const float*)p[2]; a.out = p[3]; a.stats = (float*)p[4];
            a.in_affine = (const float*)p[5]; a.in_u8 = i[7];
            return mnas_stem_fwd(&a, stream);
        }
        case MNAS_OP_STEM_WGRAD: {
            MnasStemWgrad a = {};
            a.N = i[0]; a.H = i[1]; a.W = i[2]; a.Ho = i[3]; a.Wo = i[4]; a.Co = i[5]; a.nparts = i[6];
            a.x = (const float*)p[0];
            a.dy.g = p[1]; a.dy.y = p[2]; a.dy.coef = (const float*)p[3];
            a.partial = (float*)p[4];
            a.in_affine = (const float*)p[5]; a.in_u8 = i[7];
            return mnas_stem_wgrad(&a, stream);
        }
        case MNAS_OP_STEM_DGRAD: {
            MnasGradIn d = {p[0], p[1], (const float*)p[2]};
            return mnas_stem_dgrad(&d, (const float*)p[3], i[0], i[1], i[2], i[3], i[4], i[5], (const float*)p[4], (float*)p[5], stream);
        }
        case MNAS_OP_BN_FWD_FINALIZE:
            return mnas_bn_fwd_finalize((const float*)p[0], i[0], i[1], o.d[0], (const float*)p[1], (const float*)p[2],
                                        (float*)p[3], (float*)p[4], (int64_t*)p[5], (float)o.d[1], (float)o.d[2], i[2],
                                        (float*)p[6], stream);
        case MNAS_OP_BN_BWD_REDUCE:
            return mnas_bn_bwd_reduce(p[0], p[1], (const float*)p[2], (int64_t)o.d[0], i[0], i[1], (float*)p[3], stream);
        case MNAS_OP_BN_BWD_FINALIZE:
            return mnas_bn_bwd_finalize((const float*)p[0], i[0], i[1], o.d[0], (float*)p[1], (float*)p[2], (float*)p[3],
                                        i[2], stream);
        case MNAS_OP_ADD_ACT: {
            MnasActIn a = {p[0], (const float*)p[1], (const float*)p[2]};
            MnasActIn b = {p[3], (const float*)p[4], (const float*)p[5]};
            return mnas_add_act(&a, &b, (int64_t)o.d[0], i[0], p[6], (float*)p[7], i[1], stream);
        }
        case MNAS_OP_POOL_ACT: {
            MnasActIn a = {p[0], (const float*)p[1], (const float*)p[2]};
            return mnas_pool_act(&a, i[0], i[1], i[2], (float*)p[3], stream);
        }
        case MNAS_OP_BWD_POST: {
            MnasBwdPost a = {};
            a.bn_partial = (const float*)p[0]; a.bnbuf = (float*)p[1]; a.dgamma = (float*)p[2]; a.dbeta = (float*)p[3];
            a.count = o.d[0]; a.bn_nparts = i[0]; a.bn_C = i[1];
            a.w1 = {(float*)p[4], (float*)p[5], i[2], i[3], i[4], i[5], i[6], i[7]};
            a.w2 = {(float*)p[6], (float*)p[7], i[8], i[9], i[10], i[11], i[12], i[13]};
            return mnas_bwd_post(&a, stream);
        }
        case MNAS_OP_BWD_POST_FROZEN: {
            MnasBwdPostFrozen a = {};
            a.bn_partial = (const float*)p[0]; a.bnbuf = (const float*)p[1]; a.dgamma = (float*)p[2]; a.dbeta = (float*)p[3];
            a.count = o.d[0]; a.bn_nparts = i[0]; a.bn_C = i[1];
            a.w1 = {(float*)p[4], (float*)p[5], i[2], i[3], i[4], i[5], i[6], i[7]};
            a.w2 = {(float*)p[6], (float*)p[7], i[8], i[9], i[10], i[11], i[12], i[13]};
            a.dbias = (float*)p[8];
            return mnas_bwd_post_frozen(&a, stream);
        }
        case MNAS_OP_BN_BWD_FINALIZE_FROZEN:
            return mnas_bn_bwd_finalize_frozen((const float*)p[0], i[0], i[1], (const float*)p[1], (float*)p[2], (float*)p[3],
                                               (float*)p[4], i[2], stream);
        case MNAS_OP_BN_FROZEN_BATCH:
            return mnas_bn_frozen_tables((const MnasBnFrozenDesc*)p[0], i[0], stream);
        case MNAS_OP_TCONV_DGRAD: {
            MnasTconvDgrad a = {};
            a.N = i[0]; a.Ho = i[1]; a.Wo = i[2]; a.Co = i[3]; a.Ci = i[4]; a.nparts = i[5];
            a.dy = p[0]; a.w = p[1]; a.out = p[2]; a.stats = (float*)p[3]; a.red_y = p[4]; a.red_bn = (const float*)p[5];
            return mnas_tconv_dgrad(&a, stream);
        }
        case MNAS_OP_HEAD_LINEAR: {
            MnasHeadLinear a = {};
            a.N = i[0]; a.I = i[1]; a.O = i[2]; a.relu = i[3]; a.accumulate = i[4]; a.drop_p = 0.f; a.seed = 0;
            a.x = p[0]; a.w = p[1]; a.b = p[2]; a.y = p[3]; a.dz = p[4]; a.dw = p[5]; a.db = p[6]; a.dx = p[7]; a.relu_mask = p[8];
            if (i[5] == 0) return mnas_head_linear_fwd(&a, stream);
            if (i[5] == 1) return mnas_head_linear_bwd_w(&a, stream);
            if (i[5] == 2) return mnas_head_linear_bwd_x(&a, stream);
            return MNAS_EINVAL;
        }
        case MNAS_OP_SE_SCALE: {
            MnasActIn a = {p[0], (const float*)p[1], (const float*)p[2]};
            return mnas_se_scale(&a, (const float*)p[3], i[0], i[1], i[2], p[4], stream);
        }
        case MNAS_OP_SE_BWD_REDUCE: {
            MnasActIn a = {p[1], (const float*)p[2], (const float*)p[3]};
            return mnas_se_bwd_reduce(p[0], &a, (const float*)p[4], i[0], i[1], i[2], (float*)p[5], (float*)p[6], stream);
        }
        case MNAS_OP_SE_GATE:
            return mnas_se_gate((const float*)p[0], i[0], i[1], (float*)p[1], stream);
        case MNAS_OP_SE_PROJ_FIN:
            return mnas_se_proj_finalize((float*)p[0], i[0], i[1], i[2], i[3], (const float*)p[1], (const float*)p[2], (float*)p[3],
                                         i[4], (float*)p[4], stream);
        case MNAS_OP_SE_FC_FWD:
            return mnas_se_fc_fwd((const float*)p[0], (const float*)p[1], (const float*)p[2], (const float*)p[3], (const float*)p[4],
                                  i[0], i[1], i[2], (float*)p[5], (float*)p[6], (float*)p[7], stream);
        case MNAS_OP_SE_FC_BWD:
            return mnas_se_fc_bwd((const float*)p[0], (const float*)p[1], (const float*)p[2], (const float*)p[3], (const float*)p[4],
                                  i[0], i[1], i[2], (float*)p[5], (float*)p[6], (float*)p[7], (float*)p[8], (float*)p[9], (float*)p[10],
                                  i[3], stream);
        case MNAS_OP_SE_BWD_APPLY:
            return mnas_se_bwd_apply(p[0], (const float*)p[1], (const float*)p[2], i[0], i[1], i[2], p[3], p[4], (const float*)p[5],
                                     (float*)p[6], stream);
        case MNAS_OP_DY_MAT: {
            MnasGradIn d = {p[0], p[1], (const float*)p[2]};
            return mnas_dy_materialize(&d, (int64_t)o.d[0], i[0], p[3], stream);
        }
        case MNAS_OP_POOL_BWD:
            return mnas_pool_bwd((const float*)p[0], i[0], i[1], i[2], p[1], stream);
        case MNAS_OP_NCHW_TO_NHWC:
            return mnas_nchw_f32_to_nhwc_bf16((const float*)p[0], p[1], i[0], i[1], i[2], stream);
        case MNAS_OP_PACK_WEIGHTS:
            return mnas_pack_weights((const float*)p[0], i[0], i[1], i[2], i[3], i[4], p[1], stream);
        case MNAS_OP_EVENT_RECORD:
            // p[1] (optional): HOST int the caller owns; 0 = skip this record.  bench.py brackets the dominant kernel class with
            // events inside the timed region but only needs them in a window's last step (an event record costs ~3 us of
            // dispatch gap on either side of the launch: 17 launches x 2 per step = 1 % of the step rate when always on)
            if (p[1] && *(const volatile int*)p[1] == 0) return MNAS_OK;
            return (int)hipEventRecord((hipEvent_t)p[0], (hipStream_t)stream);
        case MNAS_OP_EVENT_WAIT:
            return (int)hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)p[0], 0);
        default:
            return MNAS_EINVAL;
    }
}

extern "C" int mnas_run_ops(const MnasOp* ops, int n, void* stream, int* failed_at) {
    for (int k = 0; k < n; ++k) {
        const int rc = run_one(ops[k], stream);
        if (rc != MNAS_OK) {
            if (failed_at) *failed_at = k;
            return rc;
        }
    }
    return MNAS_OK;
}

extern "C" int mnas_run_ops_multi(const MnasOp* ops, int n, void* const* streams, int nstreams, int* failed_at) {
    for (int k = 0; k < n; ++k) {
        const int sid = ops[k].i[14];
        if (sid < 0 || sid >= nstreams) {
            if (failed_at) *failed_at = k;
            return MNAS_EINVAL;
        }
        const int rc = run_one(ops[k], streams[sid]);
        if (rc != MNAS_OK) {
            if (failed_at) *failed_at = k;
            return rc;
        }
    }
    return MNAS_OK;
}

// ---- launch lists as hipGraphs ------------------------------------------------------------------------------------------------
// The same list, captured once (thread-local stream capture on streams[0]; the library makes no synchronising or allocating HIP
// call, so every op is capturable; ops on streams[1..] join the capture through the list's own EVENT_RECORD / EVENT_WAIT pairs) and
// replayed with one hipGraphLaunch: the host enqueues a step in a fraction of the per-launch path's time and the GPU-side gap
// between dependent kernels shrinks a little (tools/probe/graph_cost.hip: 1.3 -> 1.1 us).  The graph bakes in every pointer and
// integer of the list AND the value of gated event records at capture time: the caller re-captures when the list changes.
extern "C" int mnas_graph_create(const MnasOp* ops, int n, void* const* streams, int nstreams, void** exec_out, int* failed_at) {
    if (!ops || n < 1 || !streams || nstreams < 1 || !exec_out) return MNAS_EINVAL;
    hipStream_t s0 = (hipStream_t)streams[0];
    hipError_t e = hipStreamBeginCapture(s0, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) return (int)e;
    const int rc = mnas_run_ops_multi(ops, n, streams, nstreams, failed_at);
    hipGraph_t g = nullptr;
    e = hipStreamEndCapture(s0, &g);
    if (rc != MNAS_OK || e != hipSuccess) {
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        return rc != MNAS_OK ? rc : (int)e;
    }
    hipGraphExec_t ge = nullptr;
    e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) return (int)e;
    *exec_out = (void*)ge;
    return MNAS_OK;
}
extern "C" int mnas_graph_launch(void* exec, void* stream) {
    if (!exec) return MNAS_EINVAL;
    return (int)hipGraphLaunch((hipGraphExec_t)exec, (hipStream_t)stream);
}
extern "C" int mnas_graph_destroy(void* exec) { return exec ? (int)hipGraphExecDestroy((hipGraphExec_t)exec) : MNAS_OK; }

extern "C" int mnas_event_create(void** event) {
    hipEvent_t e;
    hipError_t rc = hipEventCreate(&e);
    if (rc == hipSuccess) *event = (void*)e;
    return (int)rc;
}
extern "C" int mnas_event_destroy(void* event) { return (int)hipEventDestroy((hipEvent_t)event); }
extern "C" int mnas_event_record(void* event, void* stream) {
    return (int)hipEventRecord((hipEvent_t)event, (hipStream_t)stream);
}
extern "C" int mnas_event_elapsed_ms(void* start, void* stop, float* ms) {
    return (int)hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop);
}
