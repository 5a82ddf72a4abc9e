// kernels_roi.hip — the ROI-guided SimMIM masks of mim.py --roi_masking (reference data.py:211-233, SimMIMTransform.__call__) for a
// whole batch on device. The chain per image is
//   roi_threshold_kernel   ToPILImage + convert('L') of the float tile (the arithmetic of image_to_gray_u8_kernel, kernels_post.hip),
//                          binary = L > level as 0 / 1, white[b] = number of white pixels (exact: a count per workgroup, then one
//                          integer atomic add per workgroup)
//   ocm_op_binary_morph    twice: binary_closing(disk(2)) = dilation with border 0, erosion with border 1 (kernels_morph.hip)
//   ocm_op_label8          8-connected labels in raster order (kernels_morph.hip)
//   roi_apply_kernel       rois = resize(labels, (gh, gw), order=0) read through host-built index tables, .astype(uint8) != 0
//                          = (label & 255) != 0, cleared as a whole when white[b] < min_size (remove_small_objects on an integer
//                          image), new = mask & rois, kept unless it is empty
// Integer arithmetic only after the one fp32 multiply of ToPILImage; nothing here waits for the host.
#include "host_common.h"

#define fail ocm_fail

namespace {

constexpr int MAX_SIDE = 32768;
constexpr int64_t MAX_PIXELS = (int64_t)1 << 30;

// pic.mul(255).byte() of one channel value (truncation), exactly as image_to_gray_u8_kernel writes it
__device__ __forceinline__ unsigned int to_byte(float v) { return (uint8_t)(int)(v * 255.0f); }

// L > level of one pixel from its channel values
template <int CHANS>
__device__ __forceinline__ int above(float r, float g, float b, int level) {
    const unsigned int u = CHANS == 1 ? to_byte(r) : (19595u * to_byte(r) + 38470u * to_byte(g) + 7471u * to_byte(b) + 0x8000u) >> 16;
    return (int)u > level;  // PIL's RGB -> L; one plane is its own grey image
}

// grid (blocks, batch). Image b: planes `stride_c` elements apart, dense rows; n = h * w pixels. QUAD: a thread takes four
// consecutive pixels with 16-byte loads and one 4-byte store (the host launches it only when every plane and every mask image
// starts on such a boundary and n % 4 == 0); otherwise one pixel per thread. The same values either way.
template <int CHANS, bool QUAD>
__global__ __launch_bounds__(256) void roi_threshold_kernel(const float *__restrict__ images, int64_t stride_b, int64_t stride_c,
                                                            int n, int level, uint8_t *__restrict__ mask, int *__restrict__ white) {
    __shared__ int s_cnt[4];
    const float *img = images + (int64_t)blockIdx.y * stride_b;
    uint8_t *dst = mask + (size_t)blockIdx.y * n;
    int cnt = 0;
    if (QUAD) {
        const float4 *p0 = (const float4 *)img, *p1 = (const float4 *)(img + stride_c), *p2 = (const float4 *)(img + 2 * stride_c);
        for (int i = blockIdx.x * 256 + threadIdx.x; i < n / 4; i += gridDim.x * 256) {
            const float4 r = p0[i], g = CHANS == 3 ? p1[i] : r, b = CHANS == 3 ? p2[i] : r;
            const unsigned int o0 = above<CHANS>(r.x, g.x, b.x, level), o1 = above<CHANS>(r.y, g.y, b.y, level),
                               o2 = above<CHANS>(r.z, g.z, b.z, level), o3 = above<CHANS>(r.w, g.w, b.w, level);
            ((unsigned int *)dst)[i] = o0 | o1 << 8 | o2 << 16 | o3 << 24;
            cnt += o0 + o1 + o2 + o3;
        }
    } else {
        for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
            const int on = CHANS == 3 ? above<3>(img[i], img[stride_c + i], img[2 * stride_c + i], level)
                                      : above<1>(img[i], 0.f, 0.f, level);
            dst[i] = (uint8_t)on;
            cnt += on;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (total) atomicAdd(white + blockIdx.y, total);
    }
}

// grid (batch): one workgroup per image walks its gh * gw cells twice — "any" over new = mask & roi, then the store of new, or of
// mask != 0 when new is empty. A table entry outside the label image reads as background.
template <typename M>
__global__ __launch_bounds__(256) void roi_apply_kernel(const int *__restrict__ labels, const int *__restrict__ row_idx,
                                                        const int *__restrict__ col_idx, const int *__restrict__ white,
                                                        int min_size, const M *__restrict__ masks, M *__restrict__ out,
                                                        uint8_t *__restrict__ used, int h, int w, int gh, int gw) {
    const int b = blockIdx.x, cells = gh * gw;
    const int *lab = labels + (size_t)b * h * w;
    const M *m = masks + (size_t)b * cells;
    M *o = out + (size_t)b * cells;
    const bool kept = white[b] >= min_size;  // remove_small_objects: the white class as a whole

    auto roi = [&](int c) -> bool {
        if (!kept) return false;
        const int y = row_idx[c / gw], x = col_idx[c % gw];
        if ((unsigned)y >= (unsigned)h || (unsigned)x >= (unsigned)w) return false;
        return (lab[(size_t)y * w + x] & 255) != 0;  // float64 label -> uint8 wraps modulo 256
    };

    int any = 0;
    for (int c = threadIdx.x; c < cells; c += 256) any |= (m[c] != 0) && roi(c);
    any = __syncthreads_or(any);
    for (int c = threadIdx.x; c < cells; c += 256) {
        const bool set = m[c] != 0;
        o[c] = (M)(any ? (set && roi(c)) : set);
    }
    if (threadIdx.x == 0) used[b] = any ? 1 : 0;
}

unsigned blocks_for(size_t items, unsigned cap) {
    const size_t b = (items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

int check_batch_image(const char *what, int32_t batch, int32_t h, int32_t w) {
    if (batch < 1 || batch > 65535) return fail(OCM_EINVAL, "%s: batch = %d (1..65535)", what, batch);
    if (h < 1 || w < 1 || h > MAX_SIDE || w > MAX_SIDE || (int64_t)h * w > MAX_PIXELS)
        return fail(OCM_EINVAL, "%s: image %d x %d (sides 1..%d, at most 2^30 pixels)", what, h, w, MAX_SIDE);
    return OCM_OK;
}

}  // namespace

extern "C" int ocm_op_roi_threshold(const float *images, int64_t stride_b, int64_t stride_c, int32_t chans, int32_t batch,
                                    int32_t h, int32_t w, int32_t level, uint8_t *mask, int32_t *white, void *stream) {
    if (!images || !mask || !white) return fail(OCM_EINVAL, "roi_threshold: null argument");
    if (int rc = check_batch_image("roi_threshold", batch, h, w)) return rc;
    if (chans != 1 && chans != 3) return fail(OCM_EINVAL, "roi_threshold: chans = %d (1 or 3)", chans);
    if (level < 0 || level > 255) return fail(OCM_EINVAL, "roi_threshold: level = %d (0..255)", level);
    const int64_t n = (int64_t)h * w;
    if (stride_c < (chans == 3 ? n : 0) || stride_b < 0 || (batch > 1 && stride_b < n))
        return fail(OCM_EINVAL, "roi_threshold: stride_b = %lld, stride_c = %lld for %d planes of %lld pixels", (long long)stride_b,
                    (long long)stride_c, chans, (long long)n);
    const hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(white, 0, (size_t)batch * sizeof(int32_t), s));
    const bool quad = n % 4 == 0 && stride_b % 4 == 0 && (chans == 1 || stride_c % 4 == 0) && (uintptr_t)images % 16 == 0 &&
                      (uintptr_t)mask % 4 == 0;
    const dim3 grid(blocks_for((size_t)(quad ? n / 4 : n), 256), batch), block(256);
    auto kernel = chans == 1 ? (quad ? roi_threshold_kernel<1, true> : roi_threshold_kernel<1, false>)
                             : (quad ? roi_threshold_kernel<3, true> : roi_threshold_kernel<3, false>);
    kernel<<<grid, block, 0, s>>>(images, stride_b, stride_c, (int)n, level, mask, white);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_roi_apply(const int32_t *labels, const int32_t *row_idx, const int32_t *col_idx, const int32_t *white,
                                int32_t min_size, const void *masks, int32_t mask_bytes, void *out, uint8_t *used, int32_t batch,
                                int32_t h, int32_t w, int32_t gh, int32_t gw, void *stream) {
    if (!labels || !row_idx || !col_idx || !white || !masks || !out || !used) return fail(OCM_EINVAL, "roi_apply: null argument");
    if (int rc = check_batch_image("roi_apply", batch, h, w)) return rc;
    if (gh < 1 || gw < 1 || gh > MAX_SIDE || gw > MAX_SIDE || (int64_t)gh * gw > MAX_PIXELS)
        return fail(OCM_EINVAL, "roi_apply: grid %d x %d (sides 1..%d, at most 2^30 cells)", gh, gw, MAX_SIDE);
    if (min_size < 0) return fail(OCM_EINVAL, "roi_apply: min_size = %d < 0", min_size);
    if (mask_bytes != 1 && mask_bytes != 8) return fail(OCM_EINVAL, "roi_apply: mask_bytes = %d (1: uint8 / bool, 8: int64)", mask_bytes);
    if (masks == out) return fail(OCM_EINVAL, "roi_apply: masks and out are aliased");
    const hipStream_t s = (hipStream_t)stream;
    if (mask_bytes == 1)
        roi_apply_kernel<uint8_t><<<dim3(batch), dim3(256), 0, s>>>(labels, row_idx, col_idx, white, min_size, (const uint8_t *)masks,
                                                                    (uint8_t *)out, used, h, w, gh, gw);
    else
        roi_apply_kernel<long long><<<dim3(batch), dim3(256), 0, s>>>(labels, row_idx, col_idx, white, min_size,
                                                                      (const long long *)masks, (long long *)out, used, h, w, gh, gw);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}
