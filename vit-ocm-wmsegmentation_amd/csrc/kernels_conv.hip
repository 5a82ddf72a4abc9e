// kernels_conv.hip — the convolutional operators of the U-Net (model.py:227-320 of the reference: build_unet) on token-major
// (NHWC) fp32 activations, rows m = (b, y, x), each with a leading dimension in floats so that an operator reads or writes a
// channel slice of a wider buffer (torch.cat([up, skip], 1) is then two writers of one buffer, no copy):
//   ocm_op_conv3x3         Conv2d(C, O, 3, padding=1) [+ ReLU]: gemm_core.h's main loop with the A operand gathered by
//                          Conv3x3Loader — no 9 x C operand is written to HBM
//   ocm_op_conv3x3_image   the same for the network's first layer, gathered from the caller's (B, 3, H, W) planes (K = 27)
//   ocm_op_upconv2x2       ConvTranspose2d(C, O, 2, stride=2): one GEMM with N = 4 O whose epilogue scatters the four groups
//   ocm_op_maxpool2x2      MaxPool2d((2, 2)), bit exact
//   ocm_op_conv1x1_planes  Conv2d(C, 1, 1) -> (B, 1, H, W) planes: an fp32 dot per pixel
// No atomics anywhere: the same inputs give the same bits on every run.
//
// The Makefile compiles this file four times: once plain (the C ABI, the argument checks, the two fp32 kernels and the
// precision switch) and once per operand element type with -DOCM_CONV_E=0|1|2 (the GEMM instantiations of that type).
#include "host_common.h"
#include "launch.h"

struct ConvArgs {
    const float *in;
    int64_t ld_in;
    const void *w;
    const float *bias;
    float *out;
    int64_t ld_out;
    int batch, h, w_px, C, O, relu;
    // the image form: planes with element strides instead of token-major rows (in / ld_in / C unused)
    const float *image = nullptr;
    int64_t sb = 0, sc = 0, sy = 0;
};
// kind: 0 = 3x3 over token-major rows, 1 = 3x3 over image planes, 2 = 2x2 stride-2 transposed convolution
template <class E>
hipError_t launch_conv_e(int kind, const ConvArgs &a, hipStream_t s);
template <class E>
hipError_t launch_linear_relu_e(const E *a, const E *w, const float *bias, float *out, int64_t ldo, int M, int N, int K,
                                hipStream_t s);  // gemm_kernels.h

#ifdef OCM_CONV_E
// ------------------------------------------------------------------------------------------
// GEMM instantiations of one operand element type
// ------------------------------------------------------------------------------------------
#include "gemm_kernels.h"

#if OCM_CONV_E == 0
typedef bf16 ConvE;
#elif OCM_CONV_E == 1
typedef float ConvE;
#else
typedef sp32 ConvE;
#endif

typedef GatherRaw ConvRaw;  // gemm_kernels.h: gather_k_of / gather_finish are shared with PatchLoader
// bit (ky * 3 + kx) set: the tap's pixel (y + ky - 1, x + kx - 1) lies inside the h x w image
__device__ __forceinline__ unsigned tap_mask(int y, int x, int h, int w) {
    unsigned mk = 0x1FF;
    if (y == 0) mk &= ~0x007u;
    if (y == h - 1) mk &= ~0x1C0u;
    if (x == 0) mk &= ~0x049u;
    if (x == w - 1) mk &= ~0x124u;
    return mk;
}

// A operand of a 3x3 / padding-1 convolution over token-major fp32 rows: column k = (ky*3 + kx)*C + c of row (b, y, x) is
// in[(b, y + ky - 1, x + kx - 1)][c], zero outside the image. C % 32 == 0, so a 16-byte chunk (and, in fp32 and split pairs,
// a whole K step) is a contiguous channel run of ONE shifted pixel: two float4 loads, converted on the way into LDS. A row's
// handle is its centre pixel and the nine-bit mask of the taps that exist for it; a tap index past 8 (the bf16 step that
// 9 C does not fill) has no bit and loads zeros.
template <class E>
struct Conv3x3Loader {
    static constexpr bool W_TAIL = Elem<E>::MODE == 0;  // bf16: 9 C need not be a multiple of 64
    const float *in;
    int64_t ld;
    int h, w, C;
    float inv_c;  // 1 / C
    int w_row_bytes;
    struct Handle {
        const float *p;
        unsigned mask;
    };
    typedef ConvRaw Raw;
    __device__ __forceinline__ Handle row(int m) const {
        const int hw = h * w, pi = m - (m / hw) * hw;
        const int y = pi / w, x = pi - y * w;
        return Handle{in + (int64_t)m * ld, tap_mask(y, x, h, w)};
    }
    __device__ __forceinline__ Raw load(const Handle &hd, int t, int cc) const {
        const int k = gather_k_of<E>(t, cc);
        // k / C for k < 10 C, C <= 4096: (k + 0.5) / C is at least 0.5 / C >= 1.2e-4 away from an integer, the product's error below 2e-6
        const int tap = (int)(((float)k + 0.5f) * inv_c), c = k - tap * C;
        const int dy = (tap * 11) >> 5, dx = tap - 3 * dy;  // tap / 3 for tap < 32
        Raw r;
        r.lo = f32x4{0.f, 0.f, 0.f, 0.f};
        r.hi = r.lo;
        if ((hd.mask >> tap) & 1u) {
            const float *ptr = hd.p + ((int64_t)(dy - 1) * w + (dx - 1)) * ld + c;
            r.lo = *(const f32x4 *)ptr;
            if (Elem<E>::MODE != 1) r.hi = *(const f32x4 *)(ptr + 4);
        }
        return r;
    }
    __device__ __forceinline__ static typename Elem<E>::Chunk finish(const Raw &r, int cc) { return gather_finish<E>(r, cc); }
};

// The same gather from fp32 image planes (pixel (b, c, y, x) = image[b*sb + c*sc + y*sy + x]) for three channels: column
// k = (ky*3 + kx)*3 + c for k < 27; the weight rows are padded with zero columns to one K step, and so is this operand.
template <class E>
struct ConvImageLoader {
    const float *image;
    int64_t sb, sc, sy;
    int h, w;
    struct Handle {
        const float *p;
        unsigned mask;
    };
    typedef ConvRaw Raw;
    __device__ __forceinline__ Handle row(int m) const {
        const int hw = h * w, b = m / hw, pi = m - b * hw;
        const int y = pi / w, x = pi - y * w;
        return Handle{image + (int64_t)b * sb + (int64_t)y * sy + x, tap_mask(y, x, h, w)};
    }
    __device__ __forceinline__ float at(const Handle &hd, int k) const {
        const int tap = k / 3, c = k - 3 * tap;  // k >= 27: tap >= 9, no mask bit
        const int dy = (tap * 11) >> 5, dx = tap - 3 * dy;
        float v = 0.f;
        if (tap < 9 && ((hd.mask >> tap) & 1u)) v = hd.p[(int64_t)c * sc + (int64_t)(dy - 1) * sy + (dx - 1)];
        return v;
    }
    __device__ __forceinline__ Raw load(const Handle &hd, int t, int cc) const {
        const int k = gather_k_of<E>(t, cc);
        Raw r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r.lo[e] = at(hd, k + e);
        r.hi = r.lo;
        if (Elem<E>::MODE != 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) r.hi[e] = at(hd, k + 4 + e);
        }
        return r;
    }
    __device__ __forceinline__ static typename Elem<E>::Chunk finish(const Raw &r, int cc) { return gather_finish<E>(r, cc); }
};

// Plain token-major fp32 rows (the transposed convolution's input), converted on the way into LDS
template <class E>
struct F32RowLoader {
    static constexpr bool W_TAIL = Elem<E>::MODE == 0;  // bf16: C need not be a multiple of 64
    const float *in;
    int64_t ld;
    int C;
    int w_row_bytes;
    typedef const float *Handle;
    typedef ConvRaw Raw;
    __device__ __forceinline__ Handle row(int m) const { return in + (int64_t)m * ld; }
    __device__ __forceinline__ Raw load(Handle hd, int t, int cc) const {
        const int k = gather_k_of<E>(t, cc);
        Raw r;
        r.lo = f32x4{0.f, 0.f, 0.f, 0.f};
        r.hi = r.lo;
        if (k < C) {
            r.lo = *(const f32x4 *)(hd + k);
            if (Elem<E>::MODE != 1) r.hi = *(const f32x4 *)(hd + k + 4);
        }
        return r;
    }
    __device__ __forceinline__ static typename Elem<E>::Chunk finish(const Raw &r, int cc) { return gather_finish<E>(r, cc); }
};

// out[m][ldo] columns [0, N) = act(acc) (the bias is already in the accumulator), fp32, 16 bytes per lane
struct EpiConv {
    static constexpr bool ROWTAB = false;
    const float *bias;
    float *out;
    int M, N;
    int64_t ldo;
    int relu;
    template <class Cfg>
    __device__ __forceinline__ void run(const float *C, int m0, int n0, const f32x2 *, const f32x2 *) const {
        constexpr int BM = Cfg::BM, BN = Cfg::BN, NT = Cfg::NT, CPR = BN / 4;
#pragma unroll 4
        for (int q = threadIdx.x; q < BM * CPR; q += NT) {
            const int row = q / CPR, col = (q - row * CPR) * 4;
            const int m = m0 + row, n = n0 + col;
            if (m >= M || n >= N) continue;
            f32x4 v = *(const f32x4 *)(C + row * BN + col);
            if (relu) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
            }
            *(f32x4 *)(out + (int64_t)m * ldo + n) = v;
        }
    }
};

// ConvTranspose2d(C, O, 2, stride=2): GEMM column n = (i*2 + j)*O + o of input row (b, y, x) is output pixel (b, 2y + i, 2x + j),
// channel o. O % 4 == 0, so a lane's four columns stay inside one group. The bias (per o) is added here.
struct EpiUpconv {
    static constexpr bool ROWTAB = false;
    const float *bias;  // null: the main loop starts the accumulators at zero
    const float *bias_o;
    float *out;
    int M, N, O, h, w;
    int64_t ldo;
    template <class Cfg>
    __device__ __forceinline__ void run(const float *C, int m0, int n0, const f32x2 *, const f32x2 *) const {
        constexpr int BM = Cfg::BM, BN = Cfg::BN, NT = Cfg::NT, CPR = BN / 4;
#pragma unroll 4
        for (int q = threadIdx.x; q < BM * CPR; q += NT) {
            const int row = q / CPR, col = (q - row * CPR) * 4;
            const int m = m0 + row, n = n0 + col;
            if (m >= M || n >= N) continue;
            const int g = n / O, o = n - g * O;
            const int hw = h * w, b = m / hw, pi = m - b * hw;
            const int y = pi / w, x = pi - y * w;
            const int64_t orow = ((int64_t)b * (2 * h) + 2 * y + (g >> 1)) * (2 * w) + 2 * x + (g & 1);
            f32x4 v = *(const f32x4 *)(C + row * BN + col);
            v += *(const f32x4 *)(bias_o + o);
            *(f32x4 *)(out + orow * ldo + o) = v;
        }
    }
};

// The conv / up-conv GEMMs on the tile and depth gemm_plan_conv chooses (gemm_plan.h): tiles by rows and output width as the
// register-staged tail of nn.Linear; the 3x3 loader's depths of the U-Net (KsConv3x3) get gemm_mainloop's two-step prefetch, any
// other depth and every other loader the one-step pipeline. The loaders pad the last K step with zeros.
template <class E, class AL, class Epi>
static hipError_t conv_gemm(const AL &al, const E *w, int Kreal, int M, int N, const Epi &epi, hipStream_t s) {
    constexpr bool IS3X3 = std::is_same<AL, Conv3x3Loader<E>>::value;
    typedef std::conditional_t<IS3X3, KsConv3x3, KsNone> List;
    constexpr int KROW = Elem<E>::KROW;
    const int Kp = (Kreal + KROW - 1) / KROW * KROW;
    const GemmPlan p = gemm_plan_conv(Elem<E>::MODE, M, N, Kreal, IS3X3);
    switch (p.tile) {
        case T128x128: return launch_gemm<Cfg128x128, E, false, List>(al, w, Kreal, M, N, Kp, epi, s, p.ksteps);
        case T64x128: return launch_gemm<Cfg64x128, E, false, List>(al, w, Kreal, M, N, Kp, epi, s, p.ksteps);
        case T64x64: return launch_gemm<Cfg64x64, E, false, List>(al, w, Kreal, M, N, Kp, epi, s, p.ksteps);
        default: return hipErrorInvalidValue;
    }
}

template <class E>
hipError_t launch_conv_e(int kind, const ConvArgs &a, hipStream_t s) {
    const int M = a.batch * a.h * a.w_px;
    const E *w = (const E *)a.w;
    if (kind == 0) {
        const int K = 9 * a.C;
        Conv3x3Loader<E> al{a.in, a.ld_in, a.h, a.w_px, a.C, 1.0f / (float)a.C, K * (int)sizeof(E)};
        EpiConv epi{a.bias, a.out, M, a.O, a.ld_out, a.relu};
        return conv_gemm<E>(al, w, K, M, a.O, epi, s);
    }
    if (kind == 1) {
        constexpr int K = Elem<E>::KROW;  // 27 columns and zeros
        ConvImageLoader<E> al{a.image, a.sb, a.sc, a.sy, a.h, a.w_px};
        EpiConv epi{a.bias, a.out, M, a.O, a.ld_out, a.relu};
        return conv_gemm<E>(al, w, K, M, a.O, epi, s);
    }
    F32RowLoader<E> al{a.in, a.ld_in, a.C, a.C * (int)sizeof(E)};
    EpiUpconv epi{nullptr, a.bias, a.out, M, 4 * a.O, a.O, a.h, a.w_px, a.ld_out};
    return conv_gemm<E>(al, w, a.C, M, 4 * a.O, epi, s);
}
template hipError_t launch_conv_e<ConvE>(int, const ConvArgs &, hipStream_t);
template hipError_t launch_linear_relu_e<ConvE>(const ConvE *, const ConvE *, const float *, float *, int64_t, int, int, int,
                                                hipStream_t);

#else
// ------------------------------------------------------------------------------------------
// the fp32 kernels, the precision switch and the C ABI
// ------------------------------------------------------------------------------------------
#define fail ocm_fail

// nn.MaxPool2d((2, 2)) on token-major rows: one lane per (output pixel, four channels). The window is scanned in torch's order
// with torch's update rule (a later value wins when it is greater or NaN), so ties between -0 and +0 keep the first one.
__global__ __launch_bounds__(256) void maxpool2x2_kernel(const float *__restrict__ in, int64_t ld_in, float *__restrict__ out,
                                                         int64_t ld_out, int B, int h, int w, int C) {
    const int c4 = C >> 2, ho = h >> 1, wo = w >> 1;
    const int64_t total = (int64_t)B * ho * wo * c4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int cc = (int)(i % c4);
        int64_t r = i / c4;
        const int x = (int)(r % wo);
        r /= wo;
        const int y = (int)(r % ho), b = (int)(r / ho);
        const float *p = in + (((int64_t)b * h + 2 * y) * w + 2 * x) * ld_in + cc * 4;
        f32x4 m = *(const f32x4 *)p;
        const f32x4 v1 = *(const f32x4 *)(p + ld_in), v2 = *(const f32x4 *)(p + (int64_t)w * ld_in),
                    v3 = *(const f32x4 *)(p + (int64_t)(w + 1) * ld_in);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (v1[e] > m[e] || v1[e] != v1[e]) m[e] = v1[e];
            if (v2[e] > m[e] || v2[e] != v2[e]) m[e] = v2[e];
            if (v3[e] > m[e] || v3[e] != v3[e]) m[e] = v3[e];
        }
        *(f32x4 *)(out + (((int64_t)b * ho + y) * wo + x) * ld_out + cc * 4) = m;
    }
}

// Conv2d(C, 1, 1) -> planes: sixteen lanes per pixel, each a strided run of float4 chunks, added by a fixed shuffle tree
__global__ __launch_bounds__(256) void conv1x1_planes_kernel(const float *__restrict__ in, int64_t ld_in,
                                                             const float *__restrict__ w, const float *__restrict__ bias,
                                                             float *__restrict__ out, int64_t rows, int C) {
    const int sub = threadIdx.x & 15;
    const int64_t per = (int64_t)gridDim.x * 16;
    for (int64_t r0 = (int64_t)blockIdx.x * 16; r0 < rows; r0 += per) {  // every lane of a wave runs every shuffle
        const int64_t r = r0 + (threadIdx.x >> 4);
        const int64_t rc = r < rows ? r : rows - 1;
        float s = 0.f;
        for (int c = sub * 4; c < C; c += 64) {
            const f32x4 a = *(const f32x4 *)(in + rc * ld_in + c), b = *(const f32x4 *)(w + c);
            s = fmaf(a[0], b[0], fmaf(a[1], b[1], fmaf(a[2], b[2], fmaf(a[3], b[3], s))));
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (sub == 0 && r < rows) out[r] = s + (bias ? bias[0] : 0.f);
    }
}

static hipError_t launch_conv(int prec, int kind, const ConvArgs &a, hipStream_t s) {
    if (prec == 2) return launch_conv_e<sp32>(kind, a, s);
    if (prec) return launch_conv_e<float>(kind, a, s);
    return launch_conv_e<bf16>(kind, a, s);
}

static bool prec_ok(int32_t p) { return p == OCM_PREC_BF16 || p == OCM_PREC_FP32 || p == OCM_PREC_BF16X3; }
static bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }
// rows of a (batch, h, w) grid: positive and within the GEMM's 32-bit row index
static bool grid_ok(int32_t batch, int32_t h, int32_t w, int64_t scale = 1) {
    return batch > 0 && h > 0 && w > 0 && (int64_t)batch * h * w * scale <= 0x7FFFFFFFll - 256;
}

extern "C" int ocm_op_conv3x3(int32_t precision, const float *in, int64_t ld_in, const void *w, const float *bias, float *out,
                              int64_t ld_out, int32_t batch, int32_t h, int32_t w_px, int32_t C, int32_t O, int32_t relu,
                              void *stream) {
    if (!prec_ok(precision)) return fail(OCM_EINVAL, "bad precision %d", precision);
    if (!in || !w || !bias || !out) return fail(OCM_EINVAL, "null argument");
    if (!grid_ok(batch, h, w_px)) return fail(OCM_EINVAL, "bad grid batch=%d h=%d w=%d", batch, h, w_px);
    if (C <= 0 || C % 32 || C > 4096 || O <= 0 || O % 32)
        return fail(OCM_EINVAL, "bad channels C=%d O=%d (C %% 32, C <= 4096, O %% 32)", C, O);
    if (ld_in < C || ld_in % 4 || ld_out < O || ld_out % 4)
        return fail(OCM_EINVAL, "bad leading dimensions ld_in=%lld ld_out=%lld (>= C / O, multiples of 4)", (long long)ld_in,
                    (long long)ld_out);
    if (!al16(in) || !al16(w) || !al16(out)) return fail(OCM_EINVAL, "in, w and out must be 16-byte aligned");
    ConvArgs a{in, ld_in, w, bias, out, ld_out, batch, h, w_px, C, O, relu != 0};
    HIP_TRY(launch_conv(precision, 0, a, (hipStream_t)stream));
    return OCM_OK;
}

extern "C" int ocm_op_conv3x3_image(int32_t precision, const float *image, int64_t stride_b, int64_t stride_c, int64_t stride_y,
                                    const void *w, const float *bias, float *out, int64_t ld_out, int32_t batch, int32_t h,
                                    int32_t w_px, int32_t O, int32_t relu, void *stream) {
    if (!prec_ok(precision)) return fail(OCM_EINVAL, "bad precision %d", precision);
    if (!image || !w || !bias || !out) return fail(OCM_EINVAL, "null argument");
    if (!grid_ok(batch, h, w_px)) return fail(OCM_EINVAL, "bad grid batch=%d h=%d w=%d", batch, h, w_px);
    if (O <= 0 || O % 32) return fail(OCM_EINVAL, "bad channels O=%d (O %% 32)", O);
    if (stride_b < 0 || stride_c < 0 || stride_y < w_px)
        return fail(OCM_EINVAL, "bad strides b=%lld c=%lld y=%lld", (long long)stride_b, (long long)stride_c, (long long)stride_y);
    if (ld_out < O || ld_out % 4) return fail(OCM_EINVAL, "bad ld_out=%lld (>= O, a multiple of 4)", (long long)ld_out);
    if (!al16(w) || !al16(out)) return fail(OCM_EINVAL, "w and out must be 16-byte aligned");
    ConvArgs a{nullptr, 0, w, bias, out, ld_out, batch, h, w_px, 3, O, relu != 0, image, stride_b, stride_c, stride_y};
    HIP_TRY(launch_conv(precision, 1, a, (hipStream_t)stream));
    return OCM_OK;
}

extern "C" int ocm_op_upconv2x2(int32_t precision, const float *in, int64_t ld_in, const void *w, const float *bias, float *out,
                                int64_t ld_out, int32_t batch, int32_t h, int32_t w_px, int32_t C, int32_t O, void *stream) {
    if (!prec_ok(precision)) return fail(OCM_EINVAL, "bad precision %d", precision);
    if (!in || !w || !bias || !out) return fail(OCM_EINVAL, "null argument");
    if (!grid_ok(batch, h, w_px, 4)) return fail(OCM_EINVAL, "bad grid batch=%d h=%d w=%d", batch, h, w_px);
    if (C <= 0 || C % 32 || O <= 0 || O % 32) return fail(OCM_EINVAL, "bad channels C=%d O=%d (C %% 32, O %% 32)", C, O);
    if (ld_in < C || ld_in % 4 || ld_out < O || ld_out % 4)
        return fail(OCM_EINVAL, "bad leading dimensions ld_in=%lld ld_out=%lld (>= C / O, multiples of 4)", (long long)ld_in,
                    (long long)ld_out);
    if (!al16(in) || !al16(w) || !al16(out) || !al16(bias)) return fail(OCM_EINVAL, "in, w, bias and out must be 16-byte aligned");
    ConvArgs a{in, ld_in, w, bias, out, ld_out, batch, h, w_px, C, O, 0};
    HIP_TRY(launch_conv(precision, 2, a, (hipStream_t)stream));
    return OCM_OK;
}

extern "C" int ocm_op_linear_relu(int32_t precision, const void *a, const void *w, const float *bias, float *out, int64_t ld_out,
                                  int32_t M, int32_t N, int32_t K, void *stream) {
    if (!prec_ok(precision)) return fail(OCM_EINVAL, "bad precision %d", precision);
    if (!a || !w || !bias || !out) return fail(OCM_EINVAL, "null argument");
    const int kq = precision == OCM_PREC_BF16 ? 64 : 32;
    if (M <= 0 || N <= 0 || N % 32 || K <= 0 || K % kq) return fail(OCM_EINVAL, "bad shape M=%d N=%d K=%d (N%%32, K%%%d)", M, N, K, kq);
    if (ld_out < N || ld_out % 4) return fail(OCM_EINVAL, "bad ld_out=%lld (>= N, a multiple of 4)", (long long)ld_out);
    if (!al16(a) || !al16(w) || !al16(out)) return fail(OCM_EINVAL, "a, w and out must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (precision == OCM_PREC_BF16X3)
        HIP_TRY(launch_linear_relu_e<sp32>((const sp32 *)a, (const sp32 *)w, bias, out, ld_out, M, N, K, s));
    else if (precision == OCM_PREC_FP32)
        HIP_TRY(launch_linear_relu_e<float>((const float *)a, (const float *)w, bias, out, ld_out, M, N, K, s));
    else
        HIP_TRY(launch_linear_relu_e<bf16>((const bf16 *)a, (const bf16 *)w, bias, out, ld_out, M, N, K, s));
    return OCM_OK;
}

extern "C" int ocm_op_maxpool2x2(const float *in, int64_t ld_in, float *out, int64_t ld_out, int32_t batch, int32_t h, int32_t w,
                                 int32_t C, void *stream) {
    if (!in || !out) return fail(OCM_EINVAL, "null argument");
    if (batch <= 0 || h <= 0 || w <= 0 || h % 2 || w % 2) return fail(OCM_EINVAL, "bad grid batch=%d h=%d w=%d (h, w even)", batch, h, w);
    if (C <= 0 || C % 4) return fail(OCM_EINVAL, "bad channels C=%d (C %% 4)", C);
    if (ld_in < C || ld_in % 4 || ld_out < C || ld_out % 4)
        return fail(OCM_EINVAL, "bad leading dimensions ld_in=%lld ld_out=%lld (>= C, multiples of 4)", (long long)ld_in,
                    (long long)ld_out);
    if (!al16(in) || !al16(out)) return fail(OCM_EINVAL, "in and out must be 16-byte aligned");
    const int64_t total = (int64_t)batch * (h / 2) * (w / 2) * (C / 4);
    const int64_t blocks = (total + 255) / 256;
    maxpool2x2_kernel<<<dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, (hipStream_t)stream>>>(
        in, ld_in, out, ld_out, batch, h, w, C);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_conv1x1_planes(const float *in, int64_t ld_in, const float *w, const float *bias, float *out, int32_t batch,
                                     int64_t hw, int32_t C, void *stream) {
    if (!in || !w || !out) return fail(OCM_EINVAL, "null argument");
    if (batch <= 0 || hw <= 0) return fail(OCM_EINVAL, "bad shape batch=%d hw=%lld", batch, (long long)hw);
    if (C <= 0 || C % 4) return fail(OCM_EINVAL, "bad channels C=%d (C %% 4)", C);
    if (ld_in < C || ld_in % 4) return fail(OCM_EINVAL, "bad ld_in=%lld (>= C, a multiple of 4)", (long long)ld_in);
    if (!al16(in) || !al16(w)) return fail(OCM_EINVAL, "in and w must be 16-byte aligned");
    const int64_t rows = (int64_t)batch * hw, blocks = (rows + 15) / 16;
    conv1x1_planes_kernel<<<dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, (hipStream_t)stream>>>(
        in, ld_in, w, bias, out, rows, C);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}
#endif
