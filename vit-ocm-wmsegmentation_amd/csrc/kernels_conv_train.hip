// kernels_conv_train.hip — what training build_unet (model.py:227-320 of the reference; PGT.py's and unet.py's step) needs next
// to the operators it shares with inference (kernels_conv.hip) and with the LinearProbing decoder (kernels_train.hip):
//   ocm_op_bn_relu                   z = max(y * scale + shift, 0) into a column slice (the gate of ocm_op_bn_relu_backward: bn_pre)
//   ocm_op_maxpool2x2_backward       the pooled gradient routed to the position maxpool2x2_kernel's scan ends on, + the skip's gradient
//   ocm_op_upconv2x2_gather          the four O-wide pixel groups of a 2x2 stride-2 transposed convolution's output gradient gathered
//                                    into (M, 4 O) rows: the inverse of EpiUpconv's placement
//   ocm_op_conv1x1_planes_backward   the classifier: din = dlogits w, dw = sum dlogits in, db = sum dlogits (fixed order)
//   ocm_op_im2col3x3_image           the first layer's 27 columns (+ 5 zero columns) in fp32: the x of its weight gradient
// All of them are bound by HBM: one lane per four channels, 16-byte loads and stores, 64-bit element indices, grid-stride loops,
// every output element written exactly once, no atomics (the same inputs give the same bits on every run).
#include "host_common.h"
#include "launch.h"

#define fail ocm_fail

namespace {

constexpr int64_t MAX_BLOCKS = 2048;  // 8 192 waves: every SIMD of 256 CUs holds eight; the rest of the work is the loop's

unsigned blocks_of(int64_t lanes) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((lanes + 255) / 256, MAX_BLOCKS)); }
bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }
bool ld_ok(int64_t ld, int32_t C) { return ld >= C && ld % 4 == 0; }

__global__ __launch_bounds__(256) void bn_relu_kernel(const float *__restrict__ y, const float *__restrict__ scale,
                                                      const float *__restrict__ shift, float *__restrict__ z, int64_t ld_z,
                                                      int64_t rows, int C) {
    const int c4 = C >> 2;
    const int64_t total = rows * c4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int cc = (int)(i % c4);
        const int64_t m = i / c4;
        const f32x4 v = *(const f32x4 *)(y + m * C + cc * 4), g = *(const f32x4 *)(scale + cc * 4),
                    h = *(const f32x4 *)(shift + cc * 4);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float pre = bn_pre(v[e], g[e], h[e]);
            o[e] = pre > 0.f ? pre : 0.f;
        }
        *(f32x4 *)(z + m * ld_z + cc * 4) = o;
    }
}

// One lane per (window, four channels): maxpool2x2_kernel's scan again (a later value wins when it is greater or NaN), keeping
// the position it ends on.
__global__ __launch_bounds__(256) void maxpool2x2_bwd_kernel(const float *__restrict__ z, int64_t ld_z,
                                                             const float *__restrict__ dpool, int64_t ld_dp,
                                                             const float *__restrict__ add, int64_t ld_add,
                                                             float *__restrict__ dz, int64_t ld_dz, int B, int h, int w, int C) {
    const int c4 = C >> 2, ho = h >> 1, wo = w >> 1;
    const int64_t total = (int64_t)B * ho * wo * c4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int cc = (int)(i % c4);
        int64_t r = i / c4;
        const int x = (int)(r % wo);
        r /= wo;
        const int y = (int)(r % ho), b = (int)(r / ho);
        const int64_t row0 = ((int64_t)b * h + 2 * y) * w + 2 * x;
        const int64_t rows[4] = {row0, row0 + 1, row0 + w, row0 + w + 1};
        f32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = *(const f32x4 *)(z + rows[k] * ld_z + cc * 4);
        const f32x4 g = *(const f32x4 *)(dpool + (((int64_t)b * ho + y) * wo + x) * ld_dp + cc * 4);
        int arg[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float m = v[0][e];
            int a = 0;
#pragma unroll
            for (int k = 1; k < 4; ++k)
                if (v[k][e] > m || v[k][e] != v[k][e]) {
                    m = v[k][e];
                    a = k;
                }
            arg[e] = a;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = arg[e] == k ? g[e] : 0.f;
            if (add) {
                const f32x4 s = *(const f32x4 *)(add + rows[k] * ld_add + cc * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] += s[e];
            }
            *(f32x4 *)(dz + rows[k] * ld_dz + cc * 4) = o;
        }
    }
}

// One lane per four floats of g: (m = (b, y, x), group i*2 + j, four channels)
__global__ __launch_bounds__(256) void upconv2x2_gather_kernel(const float *__restrict__ dout, int64_t ld, float *__restrict__ g,
                                                               int B, int h, int w, int O) {
    const int o4 = O >> 2;
    const int64_t total = (int64_t)B * h * w * 4 * o4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int oc = (int)(i % o4);
        int64_t r = i / o4;
        const int grp = (int)(r & 3);
        const int64_t m = r >> 2;
        const int x = (int)(m % w);
        r = m / w;
        const int y = (int)(r % h), b = (int)(r / h);
        const int64_t src = ((int64_t)b * 2 * h + 2 * y + (grp >> 1)) * (2 * w) + 2 * x + (grp & 1);
        *(f32x4 *)(g + (m * 4 + grp) * O + oc * 4) = *(const f32x4 *)(dout + src * ld + oc * 4);
    }
}

// One lane per four columns of a row: column k = (ky*3 + kx)*3 + c, zeros outside the image and from column 27 on
__global__ __launch_bounds__(256) void im2col3x3_image_kernel(const float *__restrict__ image, int64_t sb, int64_t sc, int64_t sy,
                                                              float *__restrict__ out, int B, int h, int w) {
    const int64_t total = (int64_t)B * h * w * 8;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int q = (int)(i & 7);
        const int64_t m = i >> 3;
        const int x = (int)(m % w);
        const int64_t r = m / w;
        const int y = (int)(r % h), b = (int)(r / h);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = q * 4 + e, tap = k / 3, c = k - 3 * tap;
            const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
            float v = 0.f;
            if (k < 27 && yy >= 0 && yy < h && xx >= 0 && xx < w) v = image[(int64_t)b * sb + (int64_t)c * sc + (int64_t)yy * sy + xx];
            o[e] = v;
        }
        *(f32x4 *)(out + i * 4) = o;
    }
}

// ---- the classifier's backward ----
// Rows are cut into R chunks (a function of the row count alone), one workgroup each. A lane owns four channels of every G-th row
// of its chunk (L = lanes per row, a power of two >= C / 4; G = 256 / L row groups); the G partial sums of a channel are added
// in group order in LDS, the R chunk sums in chunk order by conv1x1_bwd_finish_kernel.
int cls_chunks(int64_t rows) { return (int)std::min<int64_t>((rows + 255) / 256, 512); }

__global__ __launch_bounds__(256) void conv1x1_bwd_kernel(const float *__restrict__ dl, const float *__restrict__ in, int64_t ld_in,
                                                          const float *__restrict__ w, float *__restrict__ din, int64_t ld_din,
                                                          float *__restrict__ part, int64_t rows, int C, int64_t chunk, int lg) {
    __shared__ float red[256 * 4];
    __shared__ float redb[256];
    const int t = threadIdx.x, L = 1 << lg, G = 256 >> lg;
    const int tc = t & (L - 1), rg = t >> lg;
    const bool active = tc * 4 < C;
    const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = std::min<int64_t>(rows, r0 + chunk);
    f32x4 wv = {0.f, 0.f, 0.f, 0.f}, acc = {0.f, 0.f, 0.f, 0.f};
    if (active) wv = *(const f32x4 *)(w + tc * 4);
    float sb = 0.f;
    for (int64_t m = r0 + rg; m < r1; m += G) {
        const float d = dl[m];
        if (active) {
            if (in) {
                const f32x4 a = *(const f32x4 *)(in + m * ld_in + tc * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = fmaf(d, a[e], acc[e]);
            }
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = d * wv[e];
            *(f32x4 *)(din + m * ld_din + tc * 4) = o;
        }
        if (tc == 0) sb += d;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[t * 4 + e] = acc[e];
    redb[t] = sb;
    __syncthreads();
    if (rg == 0 && active) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int gq = 0; gq < G; ++gq)
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += red[((gq << lg) + tc) * 4 + e];
        *(f32x4 *)(part + (int64_t)blockIdx.x * C + tc * 4) = s;
    }
    if (t == 0) {
        float s = 0.f;
        for (int gq = 0; gq < G; ++gq) s += redb[gq << lg];
        part[(int64_t)gridDim.x * C + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void conv1x1_bwd_finish_kernel(const float *__restrict__ part, int R, int C, float *__restrict__ dw,
                                                                 float *__restrict__ db) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C && dw) {
        float s = 0.f;
        for (int r = 0; r < R; ++r) s += part[(int64_t)r * C + c];
        dw[c] = s;
    }
    if (c == C && db) {
        float s = 0.f;
        for (int r = 0; r < R; ++r) s += part[(int64_t)R * C + r];
        db[0] = s;
    }
}

}  // namespace

// ---- C ABI (include/ocm_vit.h, "U-Net training") ------------------------------------------------------------------------
extern "C" int ocm_op_bn_relu(const float *y, const float *scale, const float *shift, float *z, int64_t ld_z, int64_t rows,
                              int32_t channels, void *stream) {
    if (!y || !scale || !shift || !z) return fail(OCM_EINVAL, "null argument");
    if (rows <= 0 || channels <= 0 || channels % 4)
        return fail(OCM_EINVAL, "bad shape rows=%lld channels=%d (channels %% 4)", (long long)rows, channels);
    if (!ld_ok(ld_z, channels)) return fail(OCM_EINVAL, "bad ld_z=%lld (>= channels, a multiple of 4)", (long long)ld_z);
    if (!al16(y) || !al16(scale) || !al16(shift) || !al16(z)) return fail(OCM_EINVAL, "y, scale, shift and z must be 16-byte aligned");
    bn_relu_kernel<<<dim3(blocks_of(rows * (channels / 4))), dim3(256), 0, (hipStream_t)stream>>>(y, scale, shift, z, ld_z, rows,
                                                                                                  channels);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_maxpool2x2_backward(const float *z, int64_t ld_z, const float *dpool, int64_t ld_dp, const float *add,
                                          int64_t ld_add, float *dz, int64_t ld_dz, int32_t batch, int32_t h, int32_t w,
                                          int32_t channels, void *stream) {
    if (!z || !dpool || !dz) return fail(OCM_EINVAL, "null argument");
    if (batch <= 0 || h <= 0 || w <= 0 || h % 2 || w % 2) return fail(OCM_EINVAL, "bad grid batch=%d h=%d w=%d (h, w even)", batch, h, w);
    if (channels <= 0 || channels % 4) return fail(OCM_EINVAL, "bad channels C=%d (C %% 4)", channels);
    if (!ld_ok(ld_z, channels) || !ld_ok(ld_dp, channels) || !ld_ok(ld_dz, channels) || (add && !ld_ok(ld_add, channels)))
        return fail(OCM_EINVAL, "bad leading dimensions ld_z=%lld ld_dp=%lld ld_add=%lld ld_dz=%lld (>= C, multiples of 4)",
                    (long long)ld_z, (long long)ld_dp, (long long)ld_add, (long long)ld_dz);
    if (!al16(z) || !al16(dpool) || !al16(add) || !al16(dz)) return fail(OCM_EINVAL, "z, dpool, add and dz must be 16-byte aligned");
    const int64_t lanes = (int64_t)batch * (h / 2) * (w / 2) * (channels / 4);
    maxpool2x2_bwd_kernel<<<dim3(blocks_of(lanes)), dim3(256), 0, (hipStream_t)stream>>>(z, ld_z, dpool, ld_dp, add, ld_add, dz,
                                                                                         ld_dz, batch, h, w, channels);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_upconv2x2_gather(const float *dout, int64_t ld, float *g, int32_t batch, int32_t h, int32_t w,
                                       int32_t out_channels, void *stream) {
    if (!dout || !g) return fail(OCM_EINVAL, "null argument");
    if (batch <= 0 || h <= 0 || w <= 0) return fail(OCM_EINVAL, "bad grid batch=%d h=%d w=%d", batch, h, w);
    if (out_channels <= 0 || out_channels % 4) return fail(OCM_EINVAL, "bad channels O=%d (O %% 4)", out_channels);
    if (!ld_ok(ld, out_channels)) return fail(OCM_EINVAL, "bad ld=%lld (>= O, a multiple of 4)", (long long)ld);
    if (!al16(dout) || !al16(g)) return fail(OCM_EINVAL, "dout and g must be 16-byte aligned");
    const int64_t lanes = (int64_t)batch * h * w * out_channels;
    upconv2x2_gather_kernel<<<dim3(blocks_of(lanes)), dim3(256), 0, (hipStream_t)stream>>>(dout, ld, g, batch, h, w, out_channels);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_im2col3x3_image(const float *image, int64_t stride_b, int64_t stride_c, int64_t stride_y, float *out,
                                      int32_t batch, int32_t h, int32_t w, void *stream) {
    if (!image || !out) return fail(OCM_EINVAL, "null argument");
    if (batch <= 0 || h <= 0 || w <= 0) return fail(OCM_EINVAL, "bad grid batch=%d h=%d w=%d", batch, h, w);
    if (stride_b < 0 || stride_c < 0 || stride_y < w)
        return fail(OCM_EINVAL, "bad strides b=%lld c=%lld y=%lld", (long long)stride_b, (long long)stride_c, (long long)stride_y);
    if (!al16(out)) return fail(OCM_EINVAL, "out must be 16-byte aligned");
    const int64_t lanes = (int64_t)batch * h * w * 8;
    im2col3x3_image_kernel<<<dim3(blocks_of(lanes)), dim3(256), 0, (hipStream_t)stream>>>(image, stride_b, stride_c, stride_y, out,
                                                                                          batch, h, w);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" size_t ocm_conv1x1_planes_backward_workspace_bytes(int64_t rows, int32_t channels) {
    if (rows <= 0 || channels <= 0) return 0;
    return (size_t)cls_chunks(rows) * (channels + 1) * sizeof(float);
}

extern "C" int ocm_op_conv1x1_planes_backward(const float *dlogits, const float *in, int64_t ld_in, const float *w, float *din,
                                              int64_t ld_din, float *dw, float *db, int32_t batch, int64_t hw, int32_t channels,
                                              void *workspace, size_t workspace_bytes, void *stream) {
    if (!dlogits || !w || !din || (dw && !in)) return fail(OCM_EINVAL, "null argument");
    if (batch <= 0 || hw <= 0) return fail(OCM_EINVAL, "bad shape batch=%d hw=%lld", batch, (long long)hw);
    if (channels <= 0 || channels % 4 || channels > 1024) return fail(OCM_EINVAL, "bad channels C=%d (C %% 4, C <= 1024)", channels);
    if ((in && !ld_ok(ld_in, channels)) || !ld_ok(ld_din, channels))
        return fail(OCM_EINVAL, "bad leading dimensions ld_in=%lld ld_din=%lld (>= C, multiples of 4)", (long long)ld_in,
                    (long long)ld_din);
    if (!al16(in) || !al16(w) || !al16(din)) return fail(OCM_EINVAL, "in, w and din must be 16-byte aligned");
    const int64_t rows = (int64_t)batch * hw;
    const size_t need = ocm_conv1x1_planes_backward_workspace_bytes(rows, channels);
    if (!workspace || workspace_bytes < need || !al16(workspace))
        return fail(OCM_ENOMEM, "conv1x1_planes_backward workspace: %zu bytes given, %zu needed (16-byte aligned)", workspace_bytes,
                    need);
    const hipStream_t s = (hipStream_t)stream;
    const int R = cls_chunks(rows);
    const int64_t chunk = (rows + R - 1) / R;
    int lg = 0;
    while ((4 << lg) < channels) ++lg;  // lanes per row: the power of two >= C / 4, at most 256
    conv1x1_bwd_kernel<<<dim3(R), dim3(256), 0, s>>>(dlogits, dw ? in : nullptr, ld_in, w, din, ld_din, (float *)workspace, rows,
                                                     channels, chunk, lg);
    HIP_TRY(hipGetLastError());
    if (dw || db) {
        conv1x1_bwd_finish_kernel<<<dim3(channels / 256 + 1), dim3(256), 0, s>>>((const float *)workspace, R, channels, dw, db);
        HIP_TRY(hipGetLastError());
    }
    return OCM_OK;
}
