// kernels_drop_path.hip — stochastic depth (DropPath, dino/vision_transformer.py:25-44,110-111) of the ViT training path. The
// residual add of an undropped branch lives in the epilogue of its attn.proj / mlp.fc2 GEMM; a branch with a per-image scale
// table runs that GEMM with the plain bias epilogue into a temporary instead, and one row kernel does the rest:
//   drop_path_ln_v4_kernel / drop_path_ln_kernel   x_out = x + branch * scale[image], y = LayerNorm(x_out): the new residual
//                                                   stream and the next LayerNorm's output from one read of the two rows
//   drop_path_bwd_kernel                           dbranch = dout * scale[image] in fp32 and in the operand type of the
//                                                   data-gradient GEMM that follows, one pass
// Row ownership is layernorm_v4_kernel's / layernorm_kernel's (kernels_misc.hip): a row sits in the registers of half a
// wavefront (dim % 128 == 0, 16-byte loads and stores) or of a whole one. Both kernels are HBM-bound: four passes over the rows
// for the forward (x, branch in; x_out, y out), plain vector loads and stores, grids sized by rows.
#include "ln_rows.h"
#include "host_common.h"

#define fail ocm_fail

namespace {

// x + branch * scale with the product rounded, then the sum: hipcc contracts a + b * c into an fma by default (and HIP's
// __fmul_rn / __fadd_rn are plain operators that contract as well), so contraction is switched off for these two statements.
__device__ __forceinline__ float scaled_sum(float x, float branch, float scale) {
#pragma clang fp contract(off)
    const float prod = branch * scale;
    return x + prod;
}

// The backward's product, rounded before anything uses it: left contractable, it would fuse with the subtraction that forms the
// lo half of a split pair (lo = bf16(v - hi)), which ocm_op_cast_split forms from the rounded fp32 value.
__device__ __forceinline__ float scaled(float v, float scale) {
#pragma clang fp contract(off)
    return v * scale;
}

// x_out is then the fp32 x + branch * scale of numpy or torch bit for bit; the statistics and y are ln_rows.h's, formed from
// x_out's values exactly as ocm_op_layernorm forms them. x_out may alias x or branch: a lane reads its columns of both rows
// before it writes them. The image of a row is row / tokens (rows fit an int: rows_ok); the rows of a workgroup may belong to
// two images.
template <int OUT, int NV>
__global__ __launch_bounds__(256) void drop_path_ln_v4_kernel(const float *x, const float *branch,
                                                              const float *__restrict__ scale,
                                                              const float *__restrict__ gamma,
                                                              const float *__restrict__ beta, float *x_out,
                                                              void *__restrict__ y, int64_t rows, int tokens, float eps) {
    constexpr int dim = NV * 128;
    const int sub = threadIdx.x & 31;
    const int64_t row = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * 8 + (threadIdx.x >> 5);
    if (row >= rows) return;
    const float sc = scale[(int)row / tokens];
    const int64_t base = row * dim + sub * 4;
    f32x4 v[NV], br[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = *(const f32x4 *)(x + base + i * 128);
#pragma unroll
    for (int i = 0; i < NV; ++i) br[i] = *(const f32x4 *)(branch + base + i * 128);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[i][e] = scaled_sum(v[i][e], br[i][e], sc);
        *(f32x4 *)(x_out + base + i * 128) = v[i];
    }
    ln_row_v4<OUT, NV>(v, gamma, beta, y, row, sub, eps);
}

// any even dim <= 1024: one wavefront per row, float2 per lane per 128 columns
template <int OUT>
__global__ __launch_bounds__(256) void drop_path_ln_kernel(const float *x, const float *branch,
                                                           const float *__restrict__ scale, const float *__restrict__ gamma,
                                                           const float *__restrict__ beta, float *x_out, void *__restrict__ y,
                                                           int64_t rows, int tokens, int dim, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float sc = scale[(int)row / tokens];
    const int64_t base = row * dim;
    f32x2 v[LN_MAXV];
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
        const int c = lane * 2 + i * 128;
        if (c < dim) {
            const f32x2 a = *(const f32x2 *)(x + base + c), b = *(const f32x2 *)(branch + base + c);
            v[i][0] = scaled_sum(a[0], b[0], sc);
            v[i][1] = scaled_sum(a[1], b[1], sc);
            *(f32x2 *)(x_out + base + c) = v[i];
        }
    }
    ln_row<OUT>(v, gamma, beta, y, row, dim, lane, eps);
}

template <int OUT>
hipError_t launch_drop_path_ln(const float *x, const float *branch, const float *scale, const float *gamma, const float *beta,
                               float *x_out, void *y, int64_t rows, int tokens, int dim, float eps, hipStream_t s) {
    const dim3 grid8((unsigned)((rows + 7) / 8)), grid4((unsigned)((rows + 3) / 4)), block(256);
#define OCM_DP_V4(NV) \
    drop_path_ln_v4_kernel<OUT, NV><<<grid8, block, 0, s>>>(x, branch, scale, gamma, beta, x_out, y, rows, tokens, eps)
    switch (dim) {  // the widths launch_layernorm gives its float4 kernel
        case 128: OCM_DP_V4(1); break;
        case 256: OCM_DP_V4(2); break;
        case 384: OCM_DP_V4(3); break;
        case 512: OCM_DP_V4(4); break;
        case 768: OCM_DP_V4(6); break;
        case 1024: OCM_DP_V4(8); break;
        default:
            drop_path_ln_kernel<OUT><<<grid4, block, 0, s>>>(x, branch, scale, gamma, beta, x_out, y, rows, tokens, dim, eps);
    }
#undef OCM_DP_V4
    return hipGetLastError();
}

// Eight consecutive elements per thread (dim % 8 == 0: they share a row, hence an image). The operand copy is what
// cast_bf16_kernel / cast_split_kernel (kernels_misc.hip) write from the fp32 values: cvt8 in place, or the [32 x hi | 32 x lo]
// groups of split8. PREC: OCM_PREC_*; with OCM_PREC_FP32 the fp32 output is the operand and op is not touched.
template <int PREC>
__global__ __launch_bounds__(256) void drop_path_bwd_kernel(const float *dout, const float *__restrict__ scale, float *dbranch,
                                                            char *__restrict__ op, size_t per_image8, size_t nvec) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvec) return;
    const float sc = scale[i / per_image8];
    f32x4 a = *(const f32x4 *)(dout + i * 8), b = *(const f32x4 *)(dout + i * 8 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        a[e] = scaled(a[e], sc);
        b[e] = scaled(b[e], sc);
    }
    *(f32x4 *)(dbranch + i * 8) = a;
    *(f32x4 *)(dbranch + i * 8 + 4) = b;
    if (PREC == OCM_PREC_BF16) {
        *(bf16x8 *)(op + i * 16) = cvt8(a, b);
    } else if (PREC == OCM_PREC_BF16X3) {
        bf16x8 hi, lo;
        split8(a, b, hi, lo);
        char *g = op + (i >> 2) * 128 + (i & 3) * 16;
        *(bf16x8 *)g = hi;
        *(bf16x8 *)(g + 64) = lo;
    }
}

int rows_ok(int32_t batch, int32_t tokens) {
    if (batch <= 0 || tokens <= 0) return fail(OCM_EINVAL, "batch %d and tokens %d must be positive", batch, tokens);
    if ((int64_t)batch * tokens > 0x7fffffffLL) return fail(OCM_EINVAL, "batch %d x tokens %d: too many rows", batch, tokens);
    return OCM_OK;
}

}  // namespace

extern "C" int ocm_op_drop_path_layernorm(const float *x, const float *branch, const float *scale, const float *gamma,
                                          const float *beta, float *x_out, void *y, int32_t out_kind, int32_t batch,
                                          int32_t tokens, int32_t dim, float eps, void *stream) {
    if (!x || !branch || !scale || !gamma || !beta || !x_out || !y) return fail(OCM_EINVAL, "null argument");
    if (int rc = rows_ok(batch, tokens)) return rc;
    if (dim <= 0 || dim % 2 || dim > 1024) return fail(OCM_EINVAL, "dim %d must be even and <= 1024", dim);
    if (out_kind < 0 || out_kind > 2) return fail(OCM_EINVAL, "out_kind %d is not one of OCM_LN_F32 / _BF16 / _SPLIT", out_kind);
    if (out_kind == OCM_LN_SPLIT && dim % 32) return fail(OCM_EINVAL, "split-pair output needs dim %% 32 == 0 (got %d)", dim);
    const int64_t rows = (int64_t)batch * tokens;
    const hipStream_t s = (hipStream_t)stream;
    if (out_kind == OCM_LN_BF16)
        HIP_TRY(launch_drop_path_ln<1>(x, branch, scale, gamma, beta, x_out, y, rows, tokens, dim, eps, s));
    else if (out_kind == OCM_LN_SPLIT)
        HIP_TRY(launch_drop_path_ln<2>(x, branch, scale, gamma, beta, x_out, y, rows, tokens, dim, eps, s));
    else
        HIP_TRY(launch_drop_path_ln<0>(x, branch, scale, gamma, beta, x_out, y, rows, tokens, dim, eps, s));
    return OCM_OK;
}

extern "C" int ocm_op_drop_path_backward(int32_t precision, const float *dout, const float *scale, float *dbranch_f32,
                                         void *dbranch_op, int32_t batch, int32_t tokens, int32_t dim, void *stream) {
    if (precision != OCM_PREC_BF16 && precision != OCM_PREC_FP32 && precision != OCM_PREC_BF16X3)
        return fail(OCM_EINVAL, "bad precision %d", precision);
    if (!dout || !scale || !dbranch_f32 || (!dbranch_op && precision != OCM_PREC_FP32)) return fail(OCM_EINVAL, "null argument");
    if (int rc = rows_ok(batch, tokens)) return rc;
    if (dim <= 0 || dim % 8) return fail(OCM_EINVAL, "dim %d must be a positive multiple of 8", dim);
    if (precision == OCM_PREC_BF16X3 && dim % 32) return fail(OCM_EINVAL, "split-pair output needs dim %% 32 == 0 (got %d)", dim);
    const size_t per8 = (size_t)tokens * dim / 8, nvec = per8 * batch, blocks = (nvec + 255) / 256;
    if (blocks > 0x7fffffffULL) return fail(OCM_EINVAL, "batch %d x tokens %d x dim %d: too many elements", batch, tokens, dim);
    const dim3 grid((unsigned)blocks), block(256);
    const hipStream_t s = (hipStream_t)stream;
    if (precision == OCM_PREC_BF16)
        drop_path_bwd_kernel<OCM_PREC_BF16><<<grid, block, 0, s>>>(dout, scale, dbranch_f32, (char *)dbranch_op, per8, nvec);
    else if (precision == OCM_PREC_BF16X3)
        drop_path_bwd_kernel<OCM_PREC_BF16X3><<<grid, block, 0, s>>>(dout, scale, dbranch_f32, (char *)dbranch_op, per8, nvec);
    else
        drop_path_bwd_kernel<OCM_PREC_FP32><<<grid, block, 0, s>>>(dout, scale, dbranch_f32, nullptr, per8, nvec);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}
