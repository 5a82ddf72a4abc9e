// kernels_gemm.hip — precision dispatch of the GEMM-shaped stages (launch.h) onto the per-element-type launchers of
// gemm_kernels.h, whose instantiations are compiled in kernels_gemm_inst.hip, and ocm_gemm_plan.
#include "launch.h"
#include "host_common.h"

// entry templates of gemm_kernels.h (defined and explicitly instantiated in kernels_gemm_inst.hip)
template <class E>
hipError_t launch_linear_e(const E *a, const E *w, const float *bias, const float *resid, void *out, int M, int N, int K,
                           int epilogue, hipStream_t s, const LnFold &ln, const StatsOut &so);
template <class E>
hipError_t launch_linear_ld_e(const E *a, int64_t lda, const E *w, const float *bias, const float *resid, void *out,
                              int64_t ldo, int M, int N, int K, int epilogue, hipStream_t s);
template <class E>
hipError_t launch_resid_ln_e(const E *a, const E *w, const float *bias, const float *resid, float *x, const float *gamma,
                             const float *beta, void *xn, int M, int D, int K, float eps, hipStream_t s);
template <class E>
hipError_t launch_qkv_e(const E *a, const E *w, const float *bias, E *q, E *k, E *vt, float *qkv_f32, int batch,
                        int n_tokens, int n_pad, int heads, int head_dim, bool want_v, hipStream_t s, const LnFold &ln);
template <class E>
hipError_t launch_patch_e(const PatchArgs &pa, const E *w, const float *bias, const float *pos, float *x, int dim,
                          hipStream_t s, const StatsOut &so);

hipError_t launch_linear_ld(int prec, const void *a, int64_t lda, const void *w, const float *bias, const float *resid,
                            void *out, int64_t ldo, int M, int N, int K, int epilogue, hipStream_t s) {
    if (prec == 2) return hipErrorInvalidValue;  // the strided launcher serves Swin (bf16 / fp32 only)
    if (prec)
        return launch_linear_ld_e<float>((const float *)a, lda, (const float *)w, bias, resid, out, ldo, M, N, K, epilogue,
                                         s);
    return launch_linear_ld_e<bf16>((const bf16 *)a, lda, (const bf16 *)w, bias, resid, out, ldo, M, N, K, epilogue, s);
}

hipError_t launch_linear(int prec, const void *a, const void *w, const float *bias, const float *resid, void *out, int M,
                         int N, int K, int epilogue, hipStream_t s, const LnFold &ln, const StatsOut &so) {
    if (prec == 2) return launch_linear_e<sp32>((const sp32 *)a, (const sp32 *)w, bias, resid, out, M, N, K, epilogue, s, ln, so);
    if (prec) return launch_linear_e<float>((const float *)a, (const float *)w, bias, resid, out, M, N, K, epilogue, s, ln, so);
    return launch_linear_e<bf16>((const bf16 *)a, (const bf16 *)w, bias, resid, out, M, N, K, epilogue, s, ln, so);
}

// D = 512 is not offered: its split-bf16 instantiation needs more than 256 registers per lane (scratch spills)
bool linear_resid_ln_supported(int D) { return D == 128 || D == 256 || D == 384; }

// x = resid + A W^T + bias;  xn = LayerNorm(x; gamma, beta, eps) in the activation type of `prec`
hipError_t launch_linear_resid_ln(int prec, const void *a, const void *w, const float *bias, const float *resid, float *x,
                                  const float *gamma, const float *beta, void *xn, int M, int D, int K, float eps,
                                  hipStream_t s) {
    if (prec == 2)
        return launch_resid_ln_e<sp32>((const sp32 *)a, (const sp32 *)w, bias, resid, x, gamma, beta, xn, M, D, K, eps, s);
    if (prec)
        return launch_resid_ln_e<float>((const float *)a, (const float *)w, bias, resid, x, gamma, beta, xn, M, D, K, eps, s);
    return launch_resid_ln_e<bf16>((const bf16 *)a, (const bf16 *)w, bias, resid, x, gamma, beta, xn, M, D, K, eps, s);
}

hipError_t launch_qkv(int prec, const void *a, const void *w, const float *bias, void *q, void *k, void *vt,
                      float *qkv_f32, int batch, int n_tokens, int n_pad, int heads, int head_dim, bool want_v,
                      hipStream_t s, const LnFold &ln) {
    if (prec == 2)
        return launch_qkv_e<sp32>((const sp32 *)a, (const sp32 *)w, bias, (sp32 *)q, (sp32 *)k, (sp32 *)vt, qkv_f32, batch,
                                  n_tokens, n_pad, heads, head_dim, want_v, s, ln);
    if (prec)
        return launch_qkv_e<float>((const float *)a, (const float *)w, bias, (float *)q, (float *)k, (float *)vt, qkv_f32,
                                   batch, n_tokens, n_pad, heads, head_dim, want_v, s, ln);
    return launch_qkv_e<bf16>((const bf16 *)a, (const bf16 *)w, bias, (bf16 *)q, (bf16 *)k, (bf16 *)vt, qkv_f32, batch,
                              n_tokens, n_pad, heads, head_dim, want_v, s, ln);
}

hipError_t launch_patch_embed(int prec, const PatchArgs &pa, const void *w, const float *bias, const float *pos,
                              float *x, int dim, hipStream_t s, const StatsOut &so) {
    if (prec == 2) return launch_patch_e<sp32>(pa, (const sp32 *)w, bias, pos, x, dim, s, so);
    if (prec) return launch_patch_e<float>(pa, (const float *)w, bias, pos, x, dim, s, so);
    return launch_patch_e<bf16>(pa, (const bf16 *)w, bias, pos, x, dim, s, so);
}

// ocm_gemm_plan (include/ocm_vit.h): the plan functions of gemm_plan.h behind the operators' own argument checks: the very calls
// the launchers make
extern "C" int ocm_gemm_plan(int32_t family, int32_t precision, int32_t epilogue, int32_t M, int32_t N, int32_t K,
                             uint32_t flags, ocm_gemm_plan_info *plan) {
    if (!plan) return ocm_fail(OCM_EINVAL, "null argument");
    if (precision != OCM_PREC_BF16 && precision != OCM_PREC_FP32 && precision != OCM_PREC_BF16X3)
        return ocm_fail(OCM_EINVAL, "bad precision %d", precision);
    const int kq = gemm_krow(precision);
    if (M <= 0 || N <= 0 || N % 32 || K <= 0) return ocm_fail(OCM_EINVAL, "bad shape M=%d N=%d K=%d (N%%32)", M, N, K);
    if (family != OCM_GEMM_CONV && K % kq) return ocm_fail(OCM_EINVAL, "bad shape K=%d (K%%%d)", K, kq);
    GemmPlan p;
    switch (family) {
        case OCM_GEMM_LINEAR:
            if (epilogue < 0 || epilogue > 4) return ocm_fail(OCM_EINVAL, "bad epilogue %d", epilogue);
            if ((flags & OCM_PLAN_STATS_EPILOGUE) && epilogue != OCM_EPI_BIAS_RESID_F32)
                return ocm_fail(OCM_EINVAL, "the statistics epilogue is the residual one (epilogue %d)", epilogue);
            p = gemm_plan_linear(precision, epilogue, M, N, K, (flags & OCM_PLAN_STATS_EPILOGUE) != 0,
                                 (flags & OCM_PLAN_SPLITK_OFFERED) != 0);
            break;
        case OCM_GEMM_QKV:
            if (K % 64 || N != 3 * K) return ocm_fail(OCM_EINVAL, "qkv projection: N=%d K=%d (N = 3 K, K %% 64)", N, K);
            p = gemm_plan_qkv(precision, M, K);
            break;
        case OCM_GEMM_LINEAR_LD:
            if (precision == OCM_PREC_BF16X3) return ocm_fail(OCM_EINVAL, "the strided launcher serves bf16 and fp32");
            p = gemm_plan_linear_ld(precision, M, N, K);
            break;
        case OCM_GEMM_CONV:
            if ((flags & OCM_PLAN_CONV3X3) && (K % 9 || K / 9 % 32 || K / 9 > 4096))
                return ocm_fail(OCM_EINVAL, "3x3 convolution: K=%d (K = 9 C, C %% 32, C <= 4096)", K);
            p = gemm_plan_conv(precision, M, N, K, (flags & OCM_PLAN_CONV3X3) != 0);
            break;
        case OCM_GEMM_RESID_LN:
            if (!linear_resid_ln_supported(N)) return ocm_fail(OCM_EINVAL, "row width %d not in {128, 256, 384}", N);
            if (K % 64) return ocm_fail(OCM_EINVAL, "bad shape K=%d (K%%64)", K);
            p = gemm_plan_resid_ln(precision, N, K);
            break;
        default: return ocm_fail(OCM_EINVAL, "bad family %d", family);
    }
    const GemmTileInfo &t = GEMM_TILES[p.tile];
    *plan = ocm_gemm_plan_info{t.bm, t.bn, t.waves_m * t.waves_n, t.mf16, (int32_t)p.loop, p.stages, p.ksteps, p.splitk};
    return OCM_OK;
}
