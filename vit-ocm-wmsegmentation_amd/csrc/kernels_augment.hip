// kernels_augment.hip — the per-pixel half of DINO's DataAugmentationDINO for a batch on the device, byte for byte what Pillow
// gives (dino/utils.py:36-68 GaussianBlur and Solarization; torchvision's ColorJitter and RandomGrayscale on PIL images, which are
// ImageEnhance.{Brightness, Contrast, Color}, a convert('HSV') round trip and convert('L'); ToTensor and Normalize). Restated from
// libImaging (BoxBlur.c, Blend.c, Convert.c) and pinned on the live library by tests/test_augment_host.py through the numpy
// restatement tests/augment_ref.py. Images are dense uint8 (batch, h, w, 3); every random choice is a per-image table on the device.
//   ocm_op_color_u8          color_sum_kernel<k> (k = 0..3), grid (blocks, batch): the images whose slot k is a contrast add the
//                            L values of their pixels, as they stand after the slots before k, into one 64-bit integer per image
//                            and slot (block sums first, then one integer atomic per block: exact in any order). The other
//                            images leave at once. Then color_apply_kernel runs the four slots, grey and solarize per pixel.
//   ocm_op_gaussian_blur_u8  blur_axis_kernel<false> (rows), then <true> (columns): a workgroup stages whole lines in LDS, one
//                            4-byte slot per pixel, runs Pillow's three box passes between two LDS images with the rounding to
//                            bytes after each, and stores once. The column launch stores uint8 HWC and / or float32 CHW with
//                            ToTensor and Normalize folded in, after an optional per-image solarize (upstream's second global view
//                            solarizes after the blur).
// Float arithmetic is the C statements one by one: no fused multiply-add (Image.blend is a product, then a sum).
#include <cmath>

#include "host_common.h"

#define fail ocm_fail

#pragma clang fp contract(off)

namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_MAX_AXIS = 1024;      // the longest line the blur holds in LDS
constexpr int AUG_BLUR_SLOTS = 7168;    // pixels of one LDS image: 32 lines of 224 pixels, 7 of 1024
constexpr int AUG_BLUR_MAX_LINES = 64;  // lines per workgroup
constexpr int AUG_COLOR_MAX_BLOCKS = 256;
constexpr int AUG_MAX_PIXELS = 1 << 26;
static_assert(AUG_BLUR_SLOTS >= AUG_MAX_AXIS, "one line fits");

enum { AUG_NONE = 0, AUG_BRIGHTNESS = 1, AUG_CONTRAST = 2, AUG_SATURATION = 3, AUG_HUE = 4 };

struct Rgb {
    int r, g, b;
};

__device__ __forceinline__ int aug_luma(Rgb p) { return (19595 * p.r + 38470 * p.g + 7471 * p.b + 0x8000) >> 16; }

__device__ __forceinline__ int aug_clip8(int v) { return min(max(v, 0), 255); }

// Image.blend(degenerate, image, f) of one byte: float statements, truncation inside 0..1, clip then truncation outside
__device__ __forceinline__ int aug_blend(int d, int x, float f, bool inside) {
    // plain operators under this file's contract(off): the header's __fmul_rn / __fadd_rn are parsed outside the pragma and fuse
    const float t = (float)d + f * (float)(x - d);
    if (inside) return (int)t;
    return t <= 0.0f ? 0 : t >= 255.0f ? 255 : (int)t;
}

// Convert.c rgb2hsv_row
__device__ __forceinline__ void aug_rgb2hsv(Rgb p, int &H, int &S, int &V) {
    const int mx = max(p.r, max(p.g, p.b)), mn = min(p.r, min(p.g, p.b));
    V = mx;
    if (mx == mn) {
        H = 0, S = 0;
        return;
    }
    const float cr = (float)(mx - mn);
    const float s = __fdiv_rn(cr, (float)mx);
    const float rc = __fdiv_rn((float)(mx - p.r), cr), gc = __fdiv_rn((float)(mx - p.g), cr), bc = __fdiv_rn((float)(mx - p.b), cr);
    float h;
    if (p.r == mx)
        h = bc - gc;
    else if (p.g == mx)
        h = (float)(2.0 + (double)rc - (double)bc);
    else
        h = (float)(4.0 + (double)gc - (double)rc);
    const double x = (double)h / 6.0 + 1.0;  // > 0: fmod(x, 1.0) is x - floor(x), exact
    h = (float)(x - floor(x));
    H = aug_clip8((int)((double)h * 255.0));
    S = aug_clip8((int)((double)s * 255.0));
}

// Convert.c hsv2rgb: C's round(), halves away from zero
__device__ __forceinline__ Rgb aug_hsv2rgb(int H, int S, int V) {
    if (S == 0) return Rgb{V, V, V};
    const double h6 = (double)H * 6.0 / 255.0;
    const double fl = floor(h6);
    const double f = (double)(float)(h6 - fl);
    const double fs = (double)(float)((double)S / 255.0);
    const double v = (double)V;
    const int p = aug_clip8((int)round(v * (1.0 - fs)));
    const int q = aug_clip8((int)round(v * (1.0 - fs * f)));
    const int t = aug_clip8((int)round(v * (1.0 - fs * (1.0 - f))));
    switch ((int)fl % 6) {
        case 0: return Rgb{V, t, p};
        case 1: return Rgb{q, V, p};
        case 2: return Rgb{p, V, t};
        case 3: return Rgb{p, q, V};
        case 4: return Rgb{t, p, V};
        default: return Rgb{V, p, q};
    }
}

struct ColorParams {
    int op[4];
    float f[4];
    int d[4];  // the degenerate grey of a contrast slot
};

// int(mean + 0.5) as ImageEnhance.Contrast forms it: an exact sum, a double quotient
__device__ __forceinline__ int aug_contrast_grey(unsigned long long sum, int pixels) {
    return (int)((double)sum / (double)pixels + 0.5);
}

__device__ __forceinline__ ColorParams aug_color_params(const int32_t *ops, const float *factors,
                                                        const unsigned long long *sums, int b, int pixels, int upto) {
    ColorParams c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        c.op[k] = ops[4 * b + k], c.f[k] = factors[4 * b + k];
        c.d[k] = (k < upto && c.op[k] == AUG_CONTRAST) ? aug_contrast_grey(sums[4 * b + k], pixels) : 0;
    }
    return c;
}

// slots 0 .. UPTO - 1 of one pixel
template <int UPTO>
__device__ __forceinline__ Rgb aug_slots(Rgb p, const ColorParams &c) {
#pragma unroll
    for (int k = 0; k < UPTO; ++k) {
        const int op = c.op[k];
        const float f = c.f[k];
        if (op == AUG_HUE) {
            int H, S, V;
            aug_rgb2hsv(p, H, S, V);
            p = aug_hsv2rgb((H + (int)f) & 255, S, V);
        } else if (op == AUG_BRIGHTNESS || op == AUG_CONTRAST || op == AUG_SATURATION) {
            const bool inside = f >= 0.0f && f <= 1.0f;
            const int d = op == AUG_BRIGHTNESS ? 0 : op == AUG_CONTRAST ? c.d[k] : aug_luma(p);
            p = Rgb{aug_blend(d, p.r, f, inside), aug_blend(d, p.g, f, inside), aug_blend(d, p.b, f, inside)};
        }
    }
    return p;
}

// sums: [batch][4], zeroed before the first launch of a call
template <int K>
__global__ __launch_bounds__(AUG_THREADS) void color_sum_kernel(const uint8_t *__restrict__ src, int pixels,
                                                                const int32_t *__restrict__ ops,
                                                                const float *__restrict__ factors, unsigned long long *sums) {
    __shared__ unsigned long long s_part[AUG_THREADS / 64];
    const int b = blockIdx.y;
    if (ops[4 * b + K] != AUG_CONTRAST) return;  // the whole workgroup
    const ColorParams c = aug_color_params(ops, factors, sums, b, pixels, K);
    const uint8_t *img = src + (size_t)b * pixels * 3;
    unsigned long long acc = 0;
    for (int i = blockIdx.x * AUG_THREADS + threadIdx.x; i < pixels; i += gridDim.x * AUG_THREADS) {
        const Rgb p = aug_slots<K>(Rgb{img[3 * (size_t)i], img[3 * (size_t)i + 1], img[3 * (size_t)i + 2]}, c);
        acc += (unsigned long long)aug_luma(p);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (int i = 0; i < AUG_THREADS / 64; ++i) t += s_part[i];
        atomicAdd(&sums[4 * b + K], t);
    }
}

// flags: [batch][3] = grey, solarize, threshold
__global__ __launch_bounds__(AUG_THREADS) void color_apply_kernel(const uint8_t *src, uint8_t *out, int pixels,
                                                                  const int32_t *__restrict__ ops,
                                                                  const float *__restrict__ factors,
                                                                  const int32_t *__restrict__ flags,
                                                                  const unsigned long long *__restrict__ sums) {
    const int b = blockIdx.y;
    const ColorParams c = aug_color_params(ops, factors, sums, b, pixels, 4);
    const bool grey = flags[3 * b] != 0, sol = flags[3 * b + 1] != 0;
    const int thr = flags[3 * b + 2];
    const uint8_t *img = src + (size_t)b * pixels * 3;
    uint8_t *to = out + (size_t)b * pixels * 3;
    for (int i = blockIdx.x * AUG_THREADS + threadIdx.x; i < pixels; i += gridDim.x * AUG_THREADS) {
        Rgb p = aug_slots<4>(Rgb{img[3 * (size_t)i], img[3 * (size_t)i + 1], img[3 * (size_t)i + 2]}, c);
        if (grey) p.r = p.g = p.b = aug_luma(p);
        if (sol) p = Rgb{p.r < thr ? p.r : 255 - p.r, p.g < thr ? p.g : 255 - p.g, p.b < thr ? p.b : 255 - p.b};
        to[3 * (size_t)i] = (uint8_t)p.r, to[3 * (size_t)i + 1] = (uint8_t)p.g, to[3 * (size_t)i + 2] = (uint8_t)p.b;
    }
}

struct AugNorm {
    float mean[3], std[3];
    int on;
};

// One axis of Pillow's Gaussian blur: three box passes over whole lines held in LDS. COLS false: the lines are rows, `lines`
// of them per workgroup, LDS slot = line * len + pos. COLS true: the lines are columns, LDS slot = pos * n + line, so that
// consecutive threads read consecutive slots on either axis. in and out_u8 are (batch, h, w, 3); table [batch][3] = r, ww, fw.
template <bool COLS>
__global__ __launch_bounds__(AUG_THREADS) void blur_axis_kernel(const uint8_t *__restrict__ in, int h, int w,
                                                                const uint32_t *__restrict__ table,
                                                                const int32_t *__restrict__ solarize, int lines,
                                                                uint8_t *__restrict__ out_u8, float *__restrict__ out_f32,
                                                                AugNorm norm) {
    __shared__ uint32_t s_px[2][AUG_BLUR_SLOTS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int len = COLS ? h : w, all = COLS ? w : h;
    const int l0 = blockIdx.x * lines;
    const int n = min(lines, all - l0);
    if (n <= 0 || (size_t)n * len > AUG_BLUR_SLOTS) return;  // the whole workgroup; the host sizes `lines` so that this never holds
    const int total = n * len;
    const size_t image = (size_t)b * h * w;

    // pixel of slot e in the image
    auto pixel = [&](int e) -> size_t {
        if (COLS) return (size_t)(e / n) * w + l0 + e % n;
        return (size_t)l0 * w + e;
    };
    for (int e = tid; e < total; e += AUG_THREADS) {
        const uint8_t *p = in + (image + pixel(e)) * 3;
        s_px[0][e] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    }
    __syncthreads();

    const int r = (int)min(table[3 * b], 1u << 20);  // r may exceed the line: those taps are the line's ends, counted below
    const uint32_t ww = table[3 * b + 1], fw = table[3 * b + 2];
    int cur = 0;
    if (!(r == 0 && fw == 0 && ww == 1u << 24)) {  // the identity weights of radius 0: a copy
        const int stride = COLS ? n : 1;
        for (int pass = 0; pass < 3; ++pass) {
            const uint32_t *from = s_px[cur];
            uint32_t *to = s_px[cur ^ 1];
            for (int e = tid; e < total; e += AUG_THREADS) {
                const int pos = COLS ? e / n : e % len;
                const uint32_t *line = from + (COLS ? e % n : e - pos);
                const int lo = max(pos - r, 0), hi = min(pos + r, len - 1);
                const uint32_t first = line[0], last = line[(size_t)(len - 1) * stride];
                const uint32_t nlo = (uint32_t)(lo - (pos - r)), nhi = (uint32_t)(pos + r - hi);  // taps clamped to either end
                uint32_t a0 = nlo * (first & 255u) + nhi * (last & 255u);
                uint32_t a1 = nlo * (first >> 8 & 255u) + nhi * (last >> 8 & 255u);
                uint32_t a2 = nlo * (first >> 16 & 255u) + nhi * (last >> 16 & 255u);
                for (int p = lo; p <= hi; ++p) {
                    const uint32_t v = line[(size_t)p * stride];
                    a0 += v & 255u, a1 += v >> 8 & 255u, a2 += v >> 16 & 255u;
                }
                const uint32_t fa = line[(size_t)max(pos - r - 1, 0) * stride], fb = line[(size_t)min(pos + r + 1, len - 1) * stride];
                const uint32_t o0 = (a0 * ww + ((fa & 255u) + (fb & 255u)) * fw + (1u << 23)) >> 24;
                const uint32_t o1 = (a1 * ww + ((fa >> 8 & 255u) + (fb >> 8 & 255u)) * fw + (1u << 23)) >> 24;
                const uint32_t o2 = (a2 * ww + ((fa >> 16 & 255u) + (fb >> 16 & 255u)) * fw + (1u << 23)) >> 24;
                to[e] = o0 | o1 << 8 | o2 << 16;  // each is a byte: the sums are UINT32 as Pillow's, the shift leaves 8 bits
            }
            __syncthreads();
            cur ^= 1;
        }
    }

    const int thr = (COLS && solarize) ? solarize[b] : 256;
    for (int e = tid; e < total; e += AUG_THREADS) {
        const uint32_t v = s_px[cur][e];
        int c[3] = {(int)(v & 255u), (int)(v >> 8 & 255u), (int)(v >> 16 & 255u)};
        const size_t px = pixel(e);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (c[k] >= thr) c[k] = 255 - c[k];
            if (out_u8) out_u8[(image + px) * 3 + k] = (uint8_t)c[k];
        }
        if (COLS && out_f32) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float t = __fdiv_rn((float)c[k], 255.0f);
                if (norm.on) t = __fdiv_rn(t - norm.mean[k], norm.std[k]);
                out_f32[((size_t)b * 3 + k) * h * w + px] = t;
            }
        }
    }
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

int blur_lines(int len, int all) { return std::max(1, std::min(std::min(AUG_BLUR_SLOTS / len, AUG_BLUR_MAX_LINES), all)); }

int image_check(const char *who, int32_t batch, int32_t h, int32_t w) {
    if (batch < 1 || batch > 65535) return fail(OCM_EINVAL, "%s: batch = %d (1..65535)", who, batch);
    if (h < 1 || w < 1 || (int64_t)h * w > AUG_MAX_PIXELS) return fail(OCM_EINVAL, "%s: image size %d x %d (>= 1, up to 2^26 pixels)", who, h, w);
    return OCM_OK;
}

}  // namespace

// BoxBlur.c _gaussian_blur_radius and ImagingBoxBlur's weights: float variables, the constants 12.0, 1.0 and 2.0 doubles
extern "C" int ocm_gaussian_blur_table(float radius, uint32_t *table) {
    if (!table) return fail(OCM_EINVAL, "gaussian_blur_table: null argument");
    if (!(radius >= 0.0f) || !(radius <= 4096.0f)) return fail(OCM_EINVAL, "gaussian_blur_table: radius = %g (0..4096)", (double)radius);
    const float sigma2 = radius * radius / 3;
    const float L = (float)std::sqrt(12.0 * sigma2 + 1.0);
    const float l = (float)std::floor((L - 1.0) / 2.0);
    float a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2);
    a /= 6 * (sigma2 - (l + 1) * (l + 1));
    const float fr = l + a;
    const int r = (int)fr;
    const uint32_t ww = (uint32_t)((float)(1 << 24) / (fr * 2 + 1));
    table[0] = (uint32_t)r, table[1] = ww, table[2] = ((uint32_t)(1 << 24) - (uint32_t)(r * 2 + 1) * ww) / 2;
    return OCM_OK;
}

extern "C" int32_t ocm_gaussian_blur_max_axis(void) { return AUG_MAX_AXIS; }

// [batch][4] 64-bit sums of L, one per slot
extern "C" size_t ocm_color_u8_workspace_bytes(int32_t batch) {
    return batch < 1 || batch > 65535 ? 0 : align256((size_t)batch * 4 * sizeof(unsigned long long));
}

extern "C" int ocm_op_color_u8(const uint8_t *src, uint8_t *out, int32_t batch, int32_t h, int32_t w, const int32_t *ops,
                               const float *factors, const int32_t *flags, void *workspace, size_t workspace_bytes, void *stream) {
    if (!src || !out || !ops || !factors || !flags) return fail(OCM_EINVAL, "color_u8: null argument");
    if (const int rc = image_check("color_u8", batch, h, w)) return rc;
    const size_t need = ocm_color_u8_workspace_bytes(batch);
    if (!workspace || workspace_bytes < need) return fail(OCM_ENOMEM, "color_u8 workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace & 7) return fail(OCM_EINVAL, "color_u8 workspace: not 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const int pixels = h * w;
    unsigned long long *sums = (unsigned long long *)workspace;
    const dim3 grid(std::min((pixels + AUG_THREADS - 1) / AUG_THREADS, AUG_COLOR_MAX_BLOCKS), batch), block(AUG_THREADS);
    HIP_TRY(hipMemsetAsync(sums, 0, (size_t)batch * 4 * sizeof(unsigned long long), s));
    color_sum_kernel<0><<<grid, block, 0, s>>>(src, pixels, ops, factors, sums);
    HIP_TRY(hipGetLastError());
    color_sum_kernel<1><<<grid, block, 0, s>>>(src, pixels, ops, factors, sums);
    HIP_TRY(hipGetLastError());
    color_sum_kernel<2><<<grid, block, 0, s>>>(src, pixels, ops, factors, sums);
    HIP_TRY(hipGetLastError());
    color_sum_kernel<3><<<grid, block, 0, s>>>(src, pixels, ops, factors, sums);
    HIP_TRY(hipGetLastError());
    color_apply_kernel<<<grid, block, 0, s>>>(src, out, pixels, ops, factors, flags, sums);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

// (batch, h, w, 3) bytes: the row launch's result
extern "C" size_t ocm_gaussian_blur_u8_workspace_bytes(int32_t batch, int32_t h, int32_t w) {
    if (batch < 1 || batch > 65535 || h < 1 || w < 1 || h > AUG_MAX_AXIS || w > AUG_MAX_AXIS) return 0;
    return align256((size_t)batch * h * w * 3);
}

extern "C" int ocm_op_gaussian_blur_u8(const uint8_t *src, int32_t batch, int32_t h, int32_t w, const uint32_t *table,
                                       const int32_t *solarize, uint8_t *out_u8, float *out_f32, const float *mean,
                                       const float *std, void *workspace, size_t workspace_bytes, void *stream) {
    if (!src || !table) return fail(OCM_EINVAL, "gaussian_blur_u8: null argument");
    if (!out_u8 && !out_f32) return fail(OCM_EINVAL, "gaussian_blur_u8: null outputs (uint8, float32 or both)");
    if (!mean != !std) return fail(OCM_EINVAL, "gaussian_blur_u8: mean and std come together (or both null: plain ToTensor)");
    if (const int rc = image_check("gaussian_blur_u8", batch, h, w)) return rc;
    if (h > AUG_MAX_AXIS || w > AUG_MAX_AXIS)
        return fail(OCM_EINVAL, "gaussian_blur_u8: image size %d x %d: an axis holds up to %d pixels", h, w, AUG_MAX_AXIS);
    const size_t need = ocm_gaussian_blur_u8_workspace_bytes(batch, h, w);
    if (!workspace || workspace_bytes < need)
        return fail(OCM_ENOMEM, "gaussian_blur_u8 workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    AugNorm norm = {};
    if (mean) {
        for (int c = 0; c < 3; ++c) norm.mean[c] = mean[c], norm.std[c] = std[c];
        norm.on = 1;
    }
    const hipStream_t s = (hipStream_t)stream;
    uint8_t *tmp = (uint8_t *)workspace;
    const int rows = blur_lines(w, h), cols = blur_lines(h, w);
    blur_axis_kernel<false><<<dim3((h + rows - 1) / rows, batch), dim3(AUG_THREADS), 0, s>>>(src, h, w, table, nullptr, rows, tmp,
                                                                                            nullptr, norm);
    HIP_TRY(hipGetLastError());
    blur_axis_kernel<true><<<dim3((w + cols - 1) / cols, batch), dim3(AUG_THREADS), 0, s>>>(tmp, h, w, table, solarize, cols, out_u8,
                                                                                           out_f32, norm);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}
