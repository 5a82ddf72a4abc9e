// kernels_mim.hip — the row operators of Swin SimMIM pre-training (transformers' SwinForMaskedImageModeling,
// modeling_swin.py: SwinEmbeddings' mask-token blend and the masked L1 reconstruction loss).
//   mim_count_kernel          the number of nonzero mask bytes, as per-block integer partials
//   mim_l1_kernel             one pass over the decoder GEMM's rows lin (B*hp*wp, c*s*s): the pixel-shuffled reconstruction,
//                             the loss gradient in lin's own layout and a float64 partial of sum |x - rec| * m per block
//   mim_l1_final_kernel       the partials in a fixed order -> the loss
//   swin_mask_tokens_kernel   rows whose mask byte is nonzero become the mask token (the 0 / 1 blend is a row select)
//   swin_mask_tokens_bwd_*    d_rows = d at the unmasked rows, zero elsewhere; d_mask_token = the float64 column sum of the
//                             masked rows of d, per-chunk partials combined in chunk order
// All of them are HBM-bound. In mim_l1_kernel a thread owns VEC consecutive pixels of one image row (the image column is
// the fastest index), so x and rec move in whole 16-byte pieces of fully coalesced rows and lin / dlin in runs of s contiguous
// floats (128 B at s = 32). No atomics: every sum has an order fixed by the shapes, so reruns give the same bits.
#include "common.h"
#include "host_common.h"

#define fail ocm_fail

namespace {

constexpr int MIM_COUNT_BLOCKS = 64;  // integer partials of the mask count, one per lane of the wavefront that adds them up

__global__ __launch_bounds__(256) void mim_count_kernel(const uint8_t *__restrict__ mask, size_t n, unsigned *__restrict__ part) {
    __shared__ unsigned red[256];
    unsigned acc = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)MIM_COUNT_BLOCKS * 256) acc += mask[i] != 0;
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// masked pixels of one channel: p^2 times the nonzero mask bytes (an exact integer; their number fits 32 bits because the mask
// has fewer than 2^31 bytes). Called by every lane of one wavefront: lane i reads partial i, all lanes get the total.
__device__ __forceinline__ double mim_count(const unsigned *__restrict__ part, int p) {
    unsigned n = part[threadIdx.x & 63];
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    return (double)n * (double)p * (double)p;
}

// VEC pixels per thread (4 when s % 4 == 0: the four share a run of lin; 1 otherwise). nvec = B * c * S * S / VEC.
template <int VEC>
__global__ __launch_bounds__(256) void mim_l1_kernel(const float *__restrict__ lin, const float *__restrict__ x,
                                                     const uint8_t *__restrict__ mask, float *__restrict__ rec,
                                                     float *__restrict__ dlin, double *__restrict__ part,
                                                     const unsigned *__restrict__ cnt, int hp, int wp, int c, int s, int p,
                                                     size_t nvec) {
    __shared__ float sh_scale;
    __shared__ double sh_red[4];
    if (dlin && threadIdx.x < 64) {
        const double count = mim_count(cnt, p);
        if (threadIdx.x == 0) sh_scale = (float)(1.0 / ((count + 1e-5) * (double)c));
    }
    __syncthreads();
    const float scale = dlin ? sh_scale : 0.f;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    double acc = 0.0;
    if (i < nvec) {
        const int Hs = hp * s, Ws = wp * s, Wv = Ws / VEC, Wm = Ws / p;
        const int xo = (int)(i % Wv) * VEC;
        size_t r = i / Wv;
        const int yo = (int)(r % Hs);
        r /= Hs;
        const int ch = (int)(r % c), b = (int)(r / c);
        const int y = yo / s, ii = yo - y * s, xx = xo / s, jj = xo - xx * s;
        const size_t li = ((size_t)b * hp * wp + (size_t)y * wp + xx) * ((size_t)c * s * s) + (size_t)(ch * s + ii) * s + jj;
        const size_t pi = i * VEC;
        const uint8_t *mrow = mask + ((size_t)b * (Hs / p) + yo / p) * Wm;
        float rv[VEC], xv[VEC], dv[VEC];
        if (VEC == 4) {
            *(f32x4 *)rv = *(const f32x4 *)(lin + li);
            *(f32x4 *)xv = *(const f32x4 *)(x + pi);
        } else {
            rv[0] = lin[li];
            xv[0] = x[pi];
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const bool m = mrow[(xo + e) / p] != 0;
            // |x - rec| exactly (the difference of two floats is a double), so the loss carries the rounding of its sum alone
            if (m) acc += fabs((double)xv[e] - (double)rv[e]);
            dv[e] = !m ? 0.f : rv[e] > xv[e] ? scale : rv[e] < xv[e] ? -scale : 0.f;  // sign(0) = 0: torch's abs backward
        }
        if (VEC == 4) {
            if (rec) *(f32x4 *)(rec + pi) = *(const f32x4 *)rv;
            if (dlin) *(f32x4 *)(dlin + li) = *(const f32x4 *)dv;
        } else {
            if (rec) rec[pi] = rv[0];
            if (dlin) dlin[li] = dv[0];
        }
    }
    if (!part) return;
    // lanes of a wavefront in a fixed tree, then the four wavefronts in order
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) sh_red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((sh_red[0] + sh_red[1]) + sh_red[2]) + sh_red[3];
}

__global__ __launch_bounds__(256) void mim_l1_final_kernel(const double *__restrict__ part, size_t nparts,
                                                           const unsigned *__restrict__ cnt, float *__restrict__ loss, int c,
                                                           int p) {
    __shared__ double red[256];
    double acc = 0.0;
    for (size_t i = threadIdx.x; i < nparts; i += 256) acc += part[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x < 64) {
        const double count = mim_count(cnt, p);
        if (threadIdx.x == 0) loss[0] = (float)(red[0] / (count + 1e-5) / (double)c);
    }
}

// one thread per 16-byte piece of a row
__global__ __launch_bounds__(256) void swin_mask_tokens_kernel(float *__restrict__ rows, const uint8_t *__restrict__ mask,
                                                               const float *__restrict__ token, int c4, size_t nvec) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvec) return;
    const size_t row = i / c4;
    if (mask[row]) *(f32x4 *)(rows + i * 4) = *(const f32x4 *)(token + (i - row * c4) * 4);
}

constexpr int MT_ROWS = 256;  // rows per chunk of the backward: one float64 partial per (chunk, column)

// grid (chunks, ceil(C / 64)); a workgroup is 64 columns x 4 row slices. d_rows may alias d: an element is read by the thread
// that writes it, before the write.
__global__ __launch_bounds__(256) void swin_mask_tokens_bwd_kernel(const float *d, const uint8_t *__restrict__ mask,
                                                                   float *d_rows, double *__restrict__ part, int64_t T, int C) {
    __shared__ double red[4][64];
    const int col = blockIdx.y * 64 + (threadIdx.x & 63), slice = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * MT_ROWS, r1 = r0 + MT_ROWS < T ? r0 + MT_ROWS : T;
    double acc = 0.0;
    if (col < C) {
        for (int64_t r = r0 + slice; r < r1; r += 4) {
            const float v = d[r * C + col];
            const bool m = mask[r] != 0;
            if (m) acc += (double)v;
            if (d_rows) d_rows[r * C + col] = m ? 0.f : v;
        }
    }
    if (!part) return;
    red[slice][threadIdx.x & 63] = acc;
    __syncthreads();
    if (slice == 0 && col < C)
        part[(size_t)blockIdx.x * C + col] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void swin_mask_tokens_bwd_final_kernel(const double *__restrict__ part, int chunks, int C,
                                                                         float *__restrict__ d_token) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= C) return;
    double acc = 0.0;
    for (int k = 0; k < chunks; ++k) acc += part[(size_t)k * C + col];
    d_token[col] = (float)acc;  // rounded once
}

// the sizes ocm_op_mim_l1_loss accepts; pixels = B * c * S * S and the mask bytes on success
int mim_sizes(int32_t batch, int32_t hp, int32_t wp, int32_t c, int32_t s, int32_t p, size_t *pixels, size_t *mask_bytes) {
    if (batch <= 0 || hp <= 0 || wp <= 0 || c <= 0 || s <= 0 || p <= 0)
        return fail(OCM_EINVAL, "mim_l1_loss: batch %d, grid %d x %d, %d channels, stride %d and mask patch %d must be positive",
                    batch, hp, wp, c, s, p);
    const int64_t Hs = (int64_t)hp * s, Ws = (int64_t)wp * s;
    if (Hs != Ws) return fail(OCM_EINVAL, "mim_l1_loss: the image must be square (got %lld x %lld)", (long long)Hs, (long long)Ws);
    if (Hs > 0x7fffffffLL || (int64_t)c * s * s > 0x7fffffffLL) return fail(OCM_EINVAL, "mim_l1_loss: image side or row too large");
    if (Hs % p) return fail(OCM_EINVAL, "mim_l1_loss: the mask patch %d does not divide the image side %lld", p, (long long)Hs);
    const double px = (double)batch * c * (double)Hs * (double)Ws;
    if (px > 549755813888.0) return fail(OCM_EINVAL, "mim_l1_loss: too many pixels");  // 2^39: the main pass's grid fits 2^31
    *pixels = (size_t)batch * c * (size_t)Hs * (size_t)Ws;
    *mask_bytes = (size_t)batch * (size_t)(Hs / p) * (size_t)(Ws / p);
    if (*mask_bytes > 0x7fffffffULL) return fail(OCM_EINVAL, "mim_l1_loss: too many mask entries");
    return OCM_OK;
}

inline size_t mim_blocks(size_t pixels, int s) { return (pixels / (s % 4 ? 1 : 4) + 255) / 256; }

}  // namespace

hipError_t launch_swin_mask_tokens(float *rows, const uint8_t *mask, const float *token, size_t tokens, int channels,
                                   hipStream_t s) {
    const size_t nvec = tokens * (size_t)(channels / 4);
    swin_mask_tokens_kernel<<<dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, s>>>(rows, mask, token, channels / 4, nvec);
    return hipGetLastError();
}

extern "C" size_t ocm_mim_l1_loss_workspace_bytes(int32_t batch, int32_t hp, int32_t wp, int32_t c, int32_t s) {
    if (batch <= 0 || hp <= 0 || wp <= 0 || c <= 0 || s <= 0) return 0;
    const size_t pixels = (size_t)batch * c * ((size_t)hp * s) * ((size_t)wp * s);
    return MIM_COUNT_BLOCKS * sizeof(unsigned) + mim_blocks(pixels, s) * sizeof(double);
}

extern "C" int ocm_op_mim_l1_loss(const float *lin, const float *x, const uint8_t *mask, int32_t batch, int32_t hp, int32_t wp,
                                  int32_t c, int32_t s, int32_t p, float *rec, float *dlin, float *loss, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    if (!lin || !x || !mask) return fail(OCM_EINVAL, "mim_l1_loss: null argument");
    size_t pixels = 0, mask_bytes = 0;
    if (int rc = mim_sizes(batch, hp, wp, c, s, p, &pixels, &mask_bytes)) return rc;
    if (s % 4 == 0 && (((uintptr_t)lin | (uintptr_t)x | (uintptr_t)rec | (uintptr_t)dlin) & 15))
        return fail(OCM_EINVAL, "mim_l1_loss: lin, x, rec and dlin must be 16-byte aligned");
    const size_t need = ocm_mim_l1_loss_workspace_bytes(batch, hp, wp, c, s);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7))
        return fail(OCM_ENOMEM, "mim_l1_loss workspace: %zu bytes given, %zu needed (8-byte aligned)", workspace ? workspace_bytes : 0,
                    need);
    if (!rec && !dlin && !loss) return OCM_OK;
    const hipStream_t st = (hipStream_t)stream;
    unsigned *cnt = (unsigned *)workspace;
    double *part = loss ? (double *)((char *)workspace + MIM_COUNT_BLOCKS * sizeof(unsigned)) : nullptr;
    if (dlin || loss) mim_count_kernel<<<dim3(MIM_COUNT_BLOCKS), dim3(256), 0, st>>>(mask, mask_bytes, cnt);
    const size_t blocks = mim_blocks(pixels, s);
    if (s % 4 == 0)
        mim_l1_kernel<4><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(lin, x, mask, rec, dlin, part, cnt, hp, wp, c, s, p, pixels / 4);
    else
        mim_l1_kernel<1><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(lin, x, mask, rec, dlin, part, cnt, hp, wp, c, s, p, pixels);
    if (loss) mim_l1_final_kernel<<<dim3(1), dim3(256), 0, st>>>(part, blocks, cnt, loss, c, p);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

static int mask_tokens_sizes(int64_t tokens, int32_t channels) {
    if (tokens <= 0 || tokens > 0x7fffffffLL) return fail(OCM_EINVAL, "swin_mask_tokens: bad token count %lld", (long long)tokens);
    if (channels <= 0 || channels % 4 || channels > 65535 * 64)
        return fail(OCM_EINVAL, "swin_mask_tokens: channels %d must be a positive multiple of 4", channels);
    return OCM_OK;
}

extern "C" int ocm_op_swin_mask_tokens(float *rows, const uint8_t *mask, const float *mask_token, int64_t tokens, int32_t channels,
                                       void *stream) {
    if (!rows || !mask || !mask_token) return fail(OCM_EINVAL, "swin_mask_tokens: null argument");
    if (int rc = mask_tokens_sizes(tokens, channels)) return rc;
    if (((uintptr_t)rows | (uintptr_t)mask_token) & 15) return fail(OCM_EINVAL, "swin_mask_tokens: rows and mask_token must be 16-byte aligned");
    HIP_TRY(launch_swin_mask_tokens(rows, mask, mask_token, (size_t)tokens, channels, (hipStream_t)stream));
    return OCM_OK;
}

extern "C" size_t ocm_swin_mask_tokens_backward_workspace_bytes(int64_t tokens, int32_t channels) {
    if (tokens <= 0 || tokens > 0x7fffffffLL || channels <= 0) return 0;
    return (size_t)((tokens + MT_ROWS - 1) / MT_ROWS) * (size_t)channels * sizeof(double);
}

extern "C" int ocm_op_swin_mask_tokens_backward(const float *d, const uint8_t *mask, float *d_rows, float *d_mask_token,
                                                int64_t tokens, int32_t channels, void *workspace, size_t workspace_bytes,
                                                void *stream) {
    if (!d || !mask) return fail(OCM_EINVAL, "swin_mask_tokens_backward: null argument");
    if (int rc = mask_tokens_sizes(tokens, channels)) return rc;
    const size_t need = ocm_swin_mask_tokens_backward_workspace_bytes(tokens, channels);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7))
        return fail(OCM_ENOMEM, "swin_mask_tokens_backward workspace: %zu bytes given, %zu needed (8-byte aligned)",
                    workspace ? workspace_bytes : 0, need);
    if (!d_rows && !d_mask_token) return OCM_OK;
    const hipStream_t st = (hipStream_t)stream;
    const int chunks = (int)((tokens + MT_ROWS - 1) / MT_ROWS);
    double *part = d_mask_token ? (double *)workspace : nullptr;
    swin_mask_tokens_bwd_kernel<<<dim3((unsigned)chunks, (unsigned)((channels + 63) / 64)), dim3(256), 0, st>>>(d, mask, d_rows, part,
                                                                                                          tokens, channels);
    if (d_mask_token)
        swin_mask_tokens_bwd_final_kernel<<<dim3((unsigned)((channels + 255) / 256)), dim3(256), 0, st>>>(part, chunks, channels,
                                                                                                     d_mask_token);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}
