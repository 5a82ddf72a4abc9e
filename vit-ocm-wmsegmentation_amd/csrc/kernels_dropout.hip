// kernels_dropout.hip — nn.Dropout of the ViT training path (dino/vision_transformer.py: pos_drop :209, Attention.proj_drop
// :89-90, Mlp.drop after the activation and after fc2 :57-63). No mask is stored: an element's factor is a function of
// (seeds[site], flat index) through Philox4x32-10 (philox.h), formed again by the backward. `seeds` is a device array, read by
// the kernel, so a training step draws it with one torch.randint and nothing is synchronised or copied to the host.
//   dropout_mask_kernel                      the keep bytes themselves (tests, and whoever needs the mask)
//   dropout_kernel                           y = x * factor (pos_drop, both directions)
//   dropout_ln_v4_kernel / dropout_ln_kernel x_out = x + (branch * factor) * scale[image], y = LayerNorm(x_out): the sibling of
//                                            drop_path_ln_*_kernel (kernels_drop_path.hip), same row ownership
//   dropout_bwd_kernel                       dbranch = (dout * factor) * scale[image], fp32 and GEMM operand, one pass
//   gelu_dropout_kernel                      gelu(h) * factor in the operand type (fc2's operand), optionally fp32
//   gelu_dropout_bwd_kernel                  dh = (dg * factor) * gelu'(h), g = gelu(h) * factor
// Every product with a factor or a scale is one rounded fp32 multiplication (contraction off, as scaled_sum / scaled of
// kernels_drop_path.hip and for the same reason); a missing scale table multiplies by 1.0f, which changes no bit. All kernels
// are HBM-bound row or element-wise passes: plain vector loads and stores, no LDS, no atomics; one Philox block (ten rounds,
// twenty 32 x 32 -> 64 multiplications) per four elements.
//
// Compiler resource report (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage). No kernel uses scratch,
// LDS or AGPRs. VGPRs / SGPRs / waves per SIMD:
//   dropout_mask_kernel                14 / 20 / 8      dropout_kernel                     14 / 22 / 8
//   gelu_dropout_kernel bf16, fp32     27 / 28 / 8      gelu_dropout_kernel split          29 / 28 / 8
//   gelu_dropout_bwd_kernel            38 / 28 / 8      dropout_bwd_kernel (3 precisions)  25-27 / 36-38 / 8
//   dropout_ln_v4_kernel dim 128       27 / 30 / 8      dim 256  43 / 42 / 8       dim 384  51-60 / 42-44 / 8
//                        dim 512    59-60 / 42 / 8      dim 768  62-64 / 43 / 8    dim 1024 66-88 / 38-42 / 5-7
//   dropout_ln_kernel (generic)    99-107 / 58-60 / 4   (LN_MAXV = 8 float2 slots and their Philox blocks, fully unrolled)
// The 1024-wide row kernel holds 8 float4 of x and 8 of branch per lane, the generic one unrolls all eight column slots: both
// stay above the four waves per SIMD that cover HBM latency for a streaming kernel, so neither is restructured.
#include "ln_rows.h"
#include "philox.h"
#include "host_common.h"

#define fail ocm_fail

namespace {

// one rounded product; see kernels_drop_path.hip::scaled
__device__ __forceinline__ float mul_rn(float v, float f) {
#pragma clang fp contract(off)
    return v * f;
}

// x + (branch * factor) * scale: three rounded steps
__device__ __forceinline__ float dropped_sum(float x, float branch, float factor, float scale) {
#pragma clang fp contract(off)
    const float d = branch * factor;
    const float ds = d * scale;
    return x + ds;
}

__global__ __launch_bounds__(256) void dropout_mask_kernel(const int64_t *__restrict__ seeds, int site, uint32_t thresh,
                                                           uint8_t *__restrict__ keep, size_t count) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g * 4 >= count) return;
    const philox_block b = dropout_words(seeds[site], g);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (g * 4 + e < count) keep[g * 4 + e] = b.w[e] >= thresh ? 1 : 0;
}

// count % 4 == 0; y may alias x (a thread reads its four elements before it writes them)
__global__ __launch_bounds__(256) void dropout_kernel(const float *x, const int64_t *__restrict__ seeds, int site, uint32_t thresh,
                                                      float inv_keep, float *y, size_t ngroups) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= ngroups) return;
    const philox_block b = dropout_words(seeds[site], g);
    f32x4 v = *(const f32x4 *)(x + g * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = mul_rn(v[e], dropout_factor(b.w[e], thresh, inv_keep));
    *(f32x4 *)(y + g * 4) = v;
}

// Row ownership, aliasing and the LayerNorm are drop_path_ln_v4_kernel's. A lane's four columns sub * 4 + i * 128 .. + 3 are
// one group of four of the flat index row * dim + column (dim % 128 == 0).
template <int OUT, int NV>
__global__ __launch_bounds__(256) void dropout_ln_v4_kernel(const float *x, const float *branch,
                                                            const int64_t *__restrict__ seeds, int site, uint32_t thresh,
                                                            float inv_keep, const float *__restrict__ scale,
                                                            const float *__restrict__ gamma, const float *__restrict__ beta,
                                                            float *x_out, void *__restrict__ y, int64_t rows, int tokens,
                                                            float eps) {
    constexpr int dim = NV * 128;
    const int sub = threadIdx.x & 31;
    const int64_t row = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * 8 + (threadIdx.x >> 5);
    if (row >= rows) return;
    const float sc = scale ? scale[(int)row / tokens] : 1.0f;
    const int64_t seed = seeds[site];
    const int64_t base = row * dim + sub * 4;
    f32x4 v[NV], br[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = *(const f32x4 *)(x + base + i * 128);
#pragma unroll
    for (int i = 0; i < NV; ++i) br[i] = *(const f32x4 *)(branch + base + i * 128);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const philox_block b = dropout_words(seed, (uint64_t)(base + i * 128) >> 2);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[i][e] = dropped_sum(v[i][e], br[i][e], dropout_factor(b.w[e], thresh, inv_keep), sc);
        *(f32x4 *)(x_out + base + i * 128) = v[i];
    }
    ln_row_v4<OUT, NV>(v, gamma, beta, y, row, sub, eps);
}

// any even dim <= 1024: one wavefront per row. A lane's two columns have an even flat index f: it computes the block of their
// group of four and takes words f & 3 and (f & 3) + 1.
template <int OUT>
__global__ __launch_bounds__(256) void dropout_ln_kernel(const float *x, const float *branch, const int64_t *__restrict__ seeds,
                                                         int site, uint32_t thresh, float inv_keep,
                                                         const float *__restrict__ scale, const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, float *x_out, void *__restrict__ y,
                                                         int64_t rows, int tokens, int dim, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float sc = scale ? scale[(int)row / tokens] : 1.0f;
    const int64_t seed = seeds[site];
    const int64_t base = row * dim;
    f32x2 v[LN_MAXV];
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
        const int c = lane * 2 + i * 128;
        if (c < dim) {
            const uint64_t f = (uint64_t)(base + c);
            const philox_block blk = dropout_words(seed, f >> 2);
            const bool upper = f & 2;
            const uint32_t w0 = upper ? blk.w[2] : blk.w[0], w1 = upper ? blk.w[3] : blk.w[1];
            const f32x2 a = *(const f32x2 *)(x + base + c), b = *(const f32x2 *)(branch + base + c);
            v[i][0] = dropped_sum(a[0], b[0], dropout_factor(w0, thresh, inv_keep), sc);
            v[i][1] = dropped_sum(a[1], b[1], dropout_factor(w1, thresh, inv_keep), sc);
            *(f32x2 *)(x_out + base + c) = v[i];
        }
    }
    ln_row<OUT>(v, gamma, beta, y, row, dim, lane, eps);
}

template <int OUT>
hipError_t launch_dropout_ln(const float *x, const float *branch, const int64_t *seeds, int site, uint32_t thresh, float inv_keep,
                             const float *scale, const float *gamma, const float *beta, float *x_out, void *y, int64_t rows,
                             int tokens, int dim, float eps, hipStream_t s) {
    const dim3 grid8((unsigned)((rows + 7) / 8)), grid4((unsigned)((rows + 3) / 4)), block(256);
#define OCM_DO_V4(NV)                                                                                                        \
    dropout_ln_v4_kernel<OUT, NV><<<grid8, block, 0, s>>>(x, branch, seeds, site, thresh, inv_keep, scale, gamma, beta, x_out, y, \
                                                          rows, tokens, eps)
    switch (dim) {  // the widths launch_layernorm gives its float4 kernel
        case 128: OCM_DO_V4(1); break;
        case 256: OCM_DO_V4(2); break;
        case 384: OCM_DO_V4(3); break;
        case 512: OCM_DO_V4(4); break;
        case 768: OCM_DO_V4(6); break;
        case 1024: OCM_DO_V4(8); break;
        default:
            dropout_ln_kernel<OUT><<<grid4, block, 0, s>>>(x, branch, seeds, site, thresh, inv_keep, scale, gamma, beta, x_out, y,
                                                           rows, tokens, dim, eps);
    }
#undef OCM_DO_V4
    return hipGetLastError();
}

// Eight consecutive elements per thread (dim % 8 == 0: one row, one image; two Philox blocks). The operand copy is
// drop_path_bwd_kernel's: what cast_bf16_kernel / cast_split_kernel write from the fp32 values.
template <int PREC>
__global__ __launch_bounds__(256) void dropout_bwd_kernel(const float *dout, const int64_t *__restrict__ seeds, int site,
                                                          uint32_t thresh, float inv_keep, const float *__restrict__ scale,
                                                          float *dbranch, char *__restrict__ op, size_t per_image8, size_t nvec) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvec) return;
    const float sc = scale ? scale[i / per_image8] : 1.0f;
    const int64_t seed = seeds[site];
    const philox_block b0 = dropout_words(seed, 2 * i), b1 = dropout_words(seed, 2 * i + 1);
    f32x4 a = *(const f32x4 *)(dout + i * 8), b = *(const f32x4 *)(dout + i * 8 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        a[e] = mul_rn(mul_rn(a[e], dropout_factor(b0.w[e], thresh, inv_keep)), sc);
        b[e] = mul_rn(mul_rn(b[e], dropout_factor(b1.w[e], thresh, inv_keep)), sc);
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

// E: 0 bf16, 1 fp32, 2 split pairs (count % 32 == 0). One group of four per thread; the last group of a count that is no
// multiple of four goes element by element.
template <int E>
__device__ __forceinline__ void store_operand1(void *out, size_t i, float g) {
    if (E == 0) {
        ((bf16 *)out)[i] = (bf16)g;
    } else if (E == 1) {
        ((float *)out)[i] = g;
    } else {
        bf16 hi, lo;
        split1(g, hi, lo);
        char *p = (char *)out + (i >> 5) * 128 + (i & 31) * 2;
        *(bf16 *)p = hi;
        *(bf16 *)(p + 64) = lo;
    }
}

template <int E>
__global__ __launch_bounds__(256) void gelu_dropout_kernel(const float *__restrict__ hin, const int64_t *__restrict__ seeds,
                                                           int site, uint32_t thresh, float inv_keep, void *__restrict__ out,
                                                           float *__restrict__ out32, size_t count) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, f = g * 4;
    if (f >= count) return;
    const philox_block b = dropout_words(seeds[site], g);
    if (f + 4 <= count) {
        const f32x4 h = *(const f32x4 *)(hin + f);
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = mul_rn(gelu_erf(h[e]), dropout_factor(b.w[e], thresh, inv_keep));
        if (out32) *(f32x4 *)(out32 + f) = v;
        if (E == 0) {
            bf16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (bf16)v[e];
            *(bf16x4 *)((bf16 *)out + f) = o;
        } else if (E == 1) {
            *(f32x4 *)((float *)out + f) = v;
        } else {
            bf16x4 hi, lo;
            split4(v, hi, lo);
            char *p = (char *)out + (f >> 5) * 128 + (f & 31) * 2;
            *(bf16x4 *)p = hi;
            *(bf16x4 *)(p + 64) = lo;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 3; ++e)
            if (f + e < count) {
                const float v = mul_rn(gelu_erf(hin[f + e]), dropout_factor(b.w[e], thresh, inv_keep));
                if (out32) out32[f + e] = v;
                store_operand1<E>(out, f + e, v);
            }
    }
}

// gelu_bwd_kernel's derivative (kernels_train.hip) applied to the masked dg; g = the forward's gelu(h) * factor
__device__ __forceinline__ void gelu_dropout_bwd1(float dg, float x, float factor, float &dh, float &g) {
    const float cdf = 0.5f * (1.0f + erf_as(x * 0.70710678118654752f));
    const float pdf = 0.3989422804014327f * __builtin_amdgcn_exp2f(-0.7213475204444817f * x * x);  // exp(-x^2/2)/sqrt(2pi)
    g = mul_rn(gelu_erf(x), factor);
    dh = mul_rn(dg, factor) * fmaf(x, pdf, cdf);
}

// dh may alias dg
__global__ __launch_bounds__(256) void gelu_dropout_bwd_kernel(const float *dg, const float *__restrict__ hin,
                                                               const int64_t *__restrict__ seeds, int site, uint32_t thresh,
                                                               float inv_keep, float *dh, float *__restrict__ g32, size_t count) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, f = g * 4;
    if (f >= count) return;
    const philox_block b = dropout_words(seeds[site], g);
    if (f + 4 <= count) {
        const f32x4 d = *(const f32x4 *)(dg + f), h = *(const f32x4 *)(hin + f);
        f32x4 o, gv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float oe, ge;
            gelu_dropout_bwd1(d[e], h[e], dropout_factor(b.w[e], thresh, inv_keep), oe, ge);
            o[e] = oe;
            gv[e] = ge;
        }
        *(f32x4 *)(dh + f) = o;
        if (g32) *(f32x4 *)(g32 + f) = gv;
    } else {
#pragma unroll
        for (int e = 0; e < 3; ++e)
            if (f + e < count) {
                float o, gv;
                gelu_dropout_bwd1(dg[f + e], hin[f + e], dropout_factor(b.w[e], thresh, inv_keep), o, gv);
                dh[f + e] = o;
                if (g32) g32[f + e] = gv;
            }
    }
}

int rows_ok(int32_t batch, int32_t tokens) {
    if (batch <= 0 || tokens <= 0) return fail(OCM_EINVAL, "batch %d and tokens %d must be positive", batch, tokens);
    if ((int64_t)batch * tokens > 0x7fffffffLL) return fail(OCM_EINVAL, "batch %d x tokens %d: too many rows", batch, tokens);
    return OCM_OK;
}

int site_ok(const int64_t *seeds, int32_t site) {
    if (!seeds) return fail(OCM_EINVAL, "null argument");
    if (site < 0) return fail(OCM_EINVAL, "site %d must not be negative", site);
    return OCM_OK;
}

// blocks of 256 threads, four elements each
int groups_grid(size_t count, dim3 &grid) {
    if (count == 0) return fail(OCM_EINVAL, "count must be positive");
    const size_t blocks = ((count + 3) / 4 + 255) / 256;
    if (blocks > 0x7fffffffULL) return fail(OCM_EINVAL, "count %zu: too many elements", count);
    grid = dim3((unsigned)blocks);
    return OCM_OK;
}

}  // namespace

extern "C" void ocm_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    const philox_block b = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    for (int e = 0; e < 4; ++e) out[e] = b.w[e];
}

extern "C" int ocm_dropout_threshold(double p, uint32_t *thresh, float *inv_keep) {
    if (!thresh || !inv_keep) return fail(OCM_EINVAL, "null argument");
    if (!(p > 0.0 && p < 1.0)) return fail(OCM_EINVAL, "dropout rate %g is not inside (0, 1)", p);
    const double t = __builtin_floor(p * 4294967296.0 + 0.5);
    *thresh = t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
    *inv_keep = (float)(1.0 / (1.0 - p));
    return OCM_OK;
}

extern "C" int ocm_dropout_keep_host(int64_t seed, uint64_t first, uint64_t count, uint32_t thresh, uint8_t *keep) {
    if (!keep) return fail(OCM_EINVAL, "null argument");
    if (seed < 0) return fail(OCM_EINVAL, "seed must not be negative");
    if (count == 0) return fail(OCM_EINVAL, "count must be positive");
    if (first + count < first) return fail(OCM_EINVAL, "first + count overflows");
    for (uint64_t f = first; f < first + count;) {
        const philox_block b = dropout_words(seed, f >> 2);
        for (uint64_t e = f & 3; e < 4 && f < first + count; ++e, ++f) keep[f - first] = b.w[e] >= thresh ? 1 : 0;
    }
    return OCM_OK;
}

extern "C" int ocm_op_dropout_mask(const int64_t *seeds, int32_t site, size_t count, uint32_t thresh, uint8_t *keep,
                                   void *stream) {
    if (int rc = site_ok(seeds, site)) return rc;
    if (!keep) return fail(OCM_EINVAL, "null argument");
    dim3 grid;
    if (int rc = groups_grid(count, grid)) return rc;
    dropout_mask_kernel<<<grid, dim3(256), 0, (hipStream_t)stream>>>(seeds, site, thresh, keep, count);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_dropout(const float *x, const int64_t *seeds, int32_t site, uint32_t thresh, float inv_keep, float *y,
                              size_t count, void *stream) {
    if (int rc = site_ok(seeds, site)) return rc;
    if (!x || !y) return fail(OCM_EINVAL, "null argument");
    if (count % 4) return fail(OCM_EINVAL, "count %zu must be a multiple of 4", count);
    dim3 grid;
    if (int rc = groups_grid(count, grid)) return rc;
    dropout_kernel<<<grid, dim3(256), 0, (hipStream_t)stream>>>(x, seeds, site, thresh, inv_keep, y, count / 4);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_dropout_layernorm(const float *x, const float *branch, const int64_t *seeds, int32_t site, uint32_t thresh,
                                        float inv_keep, const float *scale, const float *gamma, const float *beta, float *x_out,
                                        void *y, int32_t out_kind, int32_t batch, int32_t tokens, int32_t dim, float eps,
                                        void *stream) {
    if (int rc = site_ok(seeds, site)) return rc;
    if (!x || !branch || !gamma || !beta || !x_out || !y) return fail(OCM_EINVAL, "null argument");
    if (int rc = rows_ok(batch, tokens)) return rc;
    if (dim <= 0 || dim % 2 || dim > 1024) return fail(OCM_EINVAL, "dim %d must be even and <= 1024", dim);
    if (out_kind < 0 || out_kind > 2) return fail(OCM_EINVAL, "out_kind %d is not one of OCM_LN_F32 / _BF16 / _SPLIT", out_kind);
    if (out_kind == OCM_LN_SPLIT && dim % 32) return fail(OCM_EINVAL, "split-pair output needs dim %% 32 == 0 (got %d)", dim);
    const int64_t rows = (int64_t)batch * tokens;
    const hipStream_t s = (hipStream_t)stream;
    if (out_kind == OCM_LN_BF16)
        HIP_TRY(launch_dropout_ln<1>(x, branch, seeds, site, thresh, inv_keep, scale, gamma, beta, x_out, y, rows, tokens, dim, eps,
                                     s));
    else if (out_kind == OCM_LN_SPLIT)
        HIP_TRY(launch_dropout_ln<2>(x, branch, seeds, site, thresh, inv_keep, scale, gamma, beta, x_out, y, rows, tokens, dim, eps,
                                     s));
    else
        HIP_TRY(launch_dropout_ln<0>(x, branch, seeds, site, thresh, inv_keep, scale, gamma, beta, x_out, y, rows, tokens, dim, eps,
                                     s));
    return OCM_OK;
}

extern "C" int ocm_op_dropout_backward(int32_t precision, const float *dout, const int64_t *seeds, int32_t site, uint32_t thresh,
                                       float inv_keep, const float *scale, float *dbranch_f32, void *dbranch_op, int32_t batch,
                                       int32_t tokens, int32_t dim, void *stream) {
    if (precision != OCM_PREC_BF16 && precision != OCM_PREC_FP32 && precision != OCM_PREC_BF16X3)
        return fail(OCM_EINVAL, "bad precision %d", precision);
    if (int rc = site_ok(seeds, site)) return rc;
    if (!dout || !dbranch_f32 || (!dbranch_op && precision != OCM_PREC_FP32)) return fail(OCM_EINVAL, "null argument");
    if (int rc = rows_ok(batch, tokens)) return rc;
    if (dim <= 0 || dim % 8) return fail(OCM_EINVAL, "dim %d must be a positive multiple of 8", dim);
    if (precision == OCM_PREC_BF16X3 && dim % 32) return fail(OCM_EINVAL, "split-pair output needs dim %% 32 == 0 (got %d)", dim);
    const size_t per8 = (size_t)tokens * dim / 8, nvec = per8 * batch, blocks = (nvec + 255) / 256;
    if (blocks > 0x7fffffffULL) return fail(OCM_EINVAL, "batch %d x tokens %d x dim %d: too many elements", batch, tokens, dim);
    const dim3 grid((unsigned)blocks), block(256);
    const hipStream_t s = (hipStream_t)stream;
    if (precision == OCM_PREC_BF16)
        dropout_bwd_kernel<OCM_PREC_BF16><<<grid, block, 0, s>>>(dout, seeds, site, thresh, inv_keep, scale, dbranch_f32,
                                                                 (char *)dbranch_op, per8, nvec);
    else if (precision == OCM_PREC_BF16X3)
        dropout_bwd_kernel<OCM_PREC_BF16X3><<<grid, block, 0, s>>>(dout, seeds, site, thresh, inv_keep, scale, dbranch_f32,
                                                                   (char *)dbranch_op, per8, nvec);
    else
        dropout_bwd_kernel<OCM_PREC_FP32><<<grid, block, 0, s>>>(dout, seeds, site, thresh, inv_keep, scale, dbranch_f32, nullptr,
                                                                 per8, nvec);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_gelu_dropout(int32_t precision, const float *h, const int64_t *seeds, int32_t site, uint32_t thresh,
                                   float inv_keep, void *out, float *out_f32, size_t count, void *stream) {
    if (precision != OCM_PREC_BF16 && precision != OCM_PREC_FP32 && precision != OCM_PREC_BF16X3)
        return fail(OCM_EINVAL, "bad precision %d", precision);
    if (int rc = site_ok(seeds, site)) return rc;
    if (!h || !out) return fail(OCM_EINVAL, "null argument");
    if (count == 0 || (precision == OCM_PREC_BF16X3 && count % 32)) return fail(OCM_EINVAL, "bad count %zu", count);
    dim3 grid;
    if (int rc = groups_grid(count, grid)) return rc;
    const dim3 block(256);
    const hipStream_t s = (hipStream_t)stream;
    if (precision == OCM_PREC_BF16) gelu_dropout_kernel<0><<<grid, block, 0, s>>>(h, seeds, site, thresh, inv_keep, out, out_f32, count);
    else if (precision == OCM_PREC_FP32) gelu_dropout_kernel<1><<<grid, block, 0, s>>>(h, seeds, site, thresh, inv_keep, out, out_f32, count);
    else gelu_dropout_kernel<2><<<grid, block, 0, s>>>(h, seeds, site, thresh, inv_keep, out, out_f32, count);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_gelu_dropout_backward(const float *dg, const float *h, const int64_t *seeds, int32_t site, uint32_t thresh,
                                            float inv_keep, float *dh, float *g_f32, size_t count, void *stream) {
    if (int rc = site_ok(seeds, site)) return rc;
    if (!dg || !h || !dh) return fail(OCM_EINVAL, "null argument");
    dim3 grid;
    if (int rc = groups_grid(count, grid)) return rc;
    gelu_dropout_bwd_kernel<<<grid, dim3(256), 0, (hipStream_t)stream>>>(dg, h, seeds, site, thresh, inv_keep, dh, g_f32, count);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}
