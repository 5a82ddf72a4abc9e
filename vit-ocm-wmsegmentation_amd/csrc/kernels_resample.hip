// kernels_resample.hip — Pillow's Image.resize of 8-bit images (libImaging Resample.c, and Geometry.c's ImagingScaleAffine for
// NEAREST) for a batch on the device: the resample every caller of the reference starts with (sw_processing.py:217-222,
// analyse_attention.py:102-111, data.py:18-122 and its SimMIMTransform), with ToTensor folded into the store.
// The host half (ocm_resample_ksize, ocm_resample_table) restates precompute_coeffs and normalize_coeffs_8bpc: for one axis,
// bounds[out][2] = (first tap, tap count) and coeffs[out][ksize_padded], weights fixed to int32 with 22 fraction bits. The
// device half is Pillow's two passes in its order, the rounding to uint8 between them included:
//   resample_h_kernel  grid (out_w / RS_HTILE_W, rows / RS_HTILE_ROWS, batch): a workgroup makes RS_HTILE_W output columns
//                      (one per lane) of RS_HTILE_ROWS source rows (each wave takes every fourth). The source pixels its
//                      columns read are staged in LDS once, RS_HSPAN pixels at a time, so a tap row of any length runs
//                      through as many stagings as it needs with the sums kept in registers; a coefficient is loaded once for
//                      a thread's four rows and all channels. A staged pixel is one LDS slot (three channels in one 4-byte
//                      word), so a tap costs one LDS read per row: against a byte per channel this halved the pass
//                      (DESIGN 3.30).
//   resample_v_kernel  grid (out_w C / RS_VTILE, out_h, batch): a thread makes RS_VPACK consecutive bytes of one output row
//                      from the intermediate rows above each other: one 4-byte load per tap where the row length is a
//                      multiple of four, byte loads otherwise. The taps and weights of an output row are the same for the
//                      whole workgroup. It stores uint8 (B, out_h, out_w, C) and / or float32 (B, C, out_h, out_w) =
//                      float(u8) / 255.0f, the IEEE quotient.
// Both passes: acc = 2^21 + sum pixel * coeff in int32, clip(acc >> 22, 0, 255). Integer arithmetic: equal inputs, equal bytes.
// Tables and crop rectangles are device data: every tap and every rectangle is clamped to the memory the call owns before it
// is used, so no table can send a load or a store outside. Workgroups never communicate and nothing synchronises with the host.
#include <climits>
#include <cmath>
#include <vector>

#include "host_common.h"

#define fail ocm_fail

// Pillow's double statements one by one: no fused multiply-add in the host tables
#pragma clang fp contract(off)

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_HTILE_W = 64;     // output columns per workgroup of the horizontal pass: one per lane
constexpr int RS_HTILE_ROWS = 16;  // source rows per workgroup of the horizontal pass
constexpr int RS_HSPAN = 256;      // source pixels staged in LDS at a time
constexpr int RS_VPACK = 4;        // bytes of an output row per thread of the vertical pass
constexpr int RS_VTILE = RS_THREADS * RS_VPACK;
constexpr int RS_WAVES = RS_THREADS / 64;
static_assert(RS_HTILE_W == 64 && RS_HTILE_ROWS % RS_WAVES == 0, "a lane per output column, the rows dealt over the waves");

constexpr int RS_PRECISION_BITS = 32 - 8 - 2;
constexpr int RS_MAX_ROWS = 1 << 19, RS_MAX_ROW_BYTES = 1 << 26;  // the grids' y extents stay below 65536

struct RsSrc {
    const uint8_t *p;
    int64_t sb, sy, sx, sc;  // bytes from image to image, row to row, pixel to pixel, channel to channel
    int h, w;
};

struct RsRect {
    int y0, x0, h, w;
};

// the rectangle of image b inside the source, and no more rows than the intermediate holds
__device__ __forceinline__ RsRect rs_rect(const int32_t *rects, int b, int src_h, int src_w, int tmp_rows) {
    RsRect r = {0, 0, src_h, src_w};
    if (rects) {
        r.y0 = min(max(rects[4 * b], 0), src_h), r.x0 = min(max(rects[4 * b + 1], 0), src_w);
        r.h = min(max(rects[4 * b + 2], 0), src_h - r.y0), r.w = min(max(rects[4 * b + 3], 0), src_w - r.x0);
    }
    r.h = min(r.h, tmp_rows);
    return r;
}

__device__ __forceinline__ uint32_t rs_clip8(int acc) { return (uint32_t)min(max(acc >> RS_PRECISION_BITS, 0), 255); }

template <int C>
struct RsPixel {
    typedef uint32_t type;  // three channels in the low bytes
};
template <>
struct RsPixel<1> {
    typedef uint8_t type;
};

// tmp: [batch][tmp_rows][out_w][C]
template <int C>
__global__ __launch_bounds__(RS_THREADS) void resample_h_kernel(RsSrc src, const int32_t *__restrict__ rects,
                                                                const int32_t *__restrict__ bounds,
                                                                const int32_t *__restrict__ coeffs, int ksize, int per_image,
                                                                uint8_t *__restrict__ tmp, int tmp_rows, int out_w) {
    typedef typename RsPixel<C>::type Px;  // a staged pixel: one LDS read per tap and row, whatever the channel count
    __shared__ Px s_px[RS_HTILE_ROWS][RS_HSPAN];
    constexpr int RPT = RS_HTILE_ROWS / RS_WAVES;  // rows per thread
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, r0 = blockIdx.y * RS_HTILE_ROWS, col = blockIdx.x * RS_HTILE_W + lane;
    const RsRect rc = rs_rect(rects, b, src.h, src.w, tmp_rows);
    if (r0 >= rc.h) return;  // the whole workgroup
    const int nrows = min(RS_HTILE_ROWS, rc.h - r0);

    int first = 0, end = 0;
    const int32_t *kk = coeffs;
    if (col < out_w) {
        const size_t row = (size_t)(per_image ? b : 0) * out_w + col;
        const int f = bounds[2 * row], n = bounds[2 * row + 1];
        if (f >= 0 && n > 0) first = f, end = min(f + min(n, ksize), rc.w);
        kk = coeffs + row * (size_t)ksize;
    }
    // the pixels this workgroup's columns read: every wave holds the same 64 columns, so every wave finds the same span
    int lo = end > first ? first : INT_MAX, hi = end > first ? end : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lo = min(lo, __shfl_xor(lo, o, 64)), hi = max(hi, __shfl_xor(hi, o, 64));

    int acc[RPT][C];
#pragma unroll
    for (int j = 0; j < RPT; ++j)
#pragma unroll
        for (int c = 0; c < C; ++c) acc[j][c] = 1 << (RS_PRECISION_BITS - 1);

    const uint8_t *base = src.p + (size_t)b * src.sb + (size_t)(rc.y0 + r0) * src.sy + (size_t)rc.x0 * src.sx;
    for (int s = lo; s < hi; s += RS_HSPAN) {
        const int npix = min(RS_HSPAN, hi - s);
        const uint8_t *from = base + (size_t)s * src.sx;
        // a wave stages the rows it sums, a lane every 64th pixel: its channels from wherever the strides put them (side by
        // side or in planes, consecutive lanes on consecutive pixels either way), packed into the pixel's slot
#pragma unroll
        for (int j = 0; j < RPT; ++j) {
            const int r = wave + RS_WAVES * j;
            if (r < nrows) {
                const uint8_t *line = from + (size_t)r * src.sy;
                for (int p = lane; p < npix; p += 64) {
                    uint32_t v = 0;
#pragma unroll
                    for (int c = 0; c < C; ++c) v |= (uint32_t)line[(size_t)p * src.sx + (size_t)c * src.sc] << (8 * c);
                    s_px[r][p] = (Px)v;
                }
            }
        }
        __syncthreads();
        const int k1 = min(end, s + npix);
        for (int k = max(first, s); k < k1; ++k) {
            const int w = kk[k - first];
#pragma unroll
            for (int j = 0; j < RPT; ++j) {
                const int r = wave + RS_WAVES * j;
                if (r < nrows) {
                    const uint32_t v = s_px[r][k - s];
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[j][c] += (int)(v >> (8 * c) & 255u) * w;
                }
            }
        }
        __syncthreads();
    }
    if (col >= out_w) return;
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        const int r = wave + RS_WAVES * j;
        if (r < nrows) {
            uint8_t *to = tmp + (((size_t)b * tmp_rows + r0 + r) * out_w + col) * C;
#pragma unroll
            for (int c = 0; c < C; ++c) to[c] = (uint8_t)rs_clip8(acc[j][c]);
        }
    }
}

template <int C>
__global__ __launch_bounds__(RS_THREADS) void resample_v_kernel(const uint8_t *__restrict__ tmp, int tmp_rows,
                                                                const int32_t *__restrict__ rects, int src_h, int src_w,
                                                                const int32_t *__restrict__ bounds,
                                                                const int32_t *__restrict__ coeffs, int ksize, int per_image,
                                                                int out_h, int out_w, uint8_t *__restrict__ out_u8,
                                                                float *__restrict__ out_f32) {
    const int b = blockIdx.z, y = blockIdx.y;
    const int L = out_w * C;  // bytes of a row
    const int i0 = (blockIdx.x * RS_THREADS + threadIdx.x) * RS_VPACK;
    if (i0 >= L) return;
    const int h = rs_rect(rects, b, src_h, src_w, tmp_rows).h;
    const size_t row = (size_t)(per_image ? b : 0) * out_h + y;  // the same taps and weights in every thread
    const int f = bounds[2 * row], n = bounds[2 * row + 1];
    int first = 0, end = 0;
    if (f >= 0 && n > 0) first = f, end = min(f + min(n, ksize), h);
    const int32_t *kk = coeffs + row * (size_t)ksize;
    const bool vec = L % RS_VPACK == 0;  // then every row of the (16-byte aligned) intermediate starts on a 4-byte boundary
    const int nb = min(RS_VPACK, L - i0);
    const uint8_t *from = tmp + (size_t)b * tmp_rows * L + i0;

    int acc[RS_VPACK];
#pragma unroll
    for (int j = 0; j < RS_VPACK; ++j) acc[j] = 1 << (RS_PRECISION_BITS - 1);
    for (int k = first; k < end; ++k) {
        const int w = kk[k - first];
        const uint8_t *p = from + (size_t)k * L;
        if (vec) {
            const uint32_t v = *(const uint32_t *)p;
#pragma unroll
            for (int j = 0; j < RS_VPACK; ++j) acc[j] += (int)(v >> (8 * j) & 255u) * w;
        } else {
#pragma unroll
            for (int j = 0; j < RS_VPACK; ++j)
                if (j < nb) acc[j] += (int)p[j] * w;
        }
    }
    uint32_t v[RS_VPACK];
#pragma unroll
    for (int j = 0; j < RS_VPACK; ++j) v[j] = rs_clip8(acc[j]);
    if (out_u8) {
        uint8_t *to = out_u8 + ((size_t)b * out_h + y) * L + i0;
        if (vec && ((uintptr_t)out_u8 & 3) == 0) {
            *(uint32_t *)to = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
        } else {
#pragma unroll
            for (int j = 0; j < RS_VPACK; ++j)
                if (j < nb) to[j] = (uint8_t)v[j];
        }
    }
    if (out_f32) {
#pragma unroll
        for (int j = 0; j < RS_VPACK; ++j)
            if (j < nb) {
                const int x = (i0 + j) / C, c = (i0 + j) - x * C;
                out_f32[(((size_t)b * C + c) * out_h + y) * out_w + x] = __fdiv_rn((float)v[j], 255.0f);
            }
    }
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// ---- Pillow's filters (Resample.c), in double ----
double bilinear_filter(double x) {
    if (x < 0.0) x = -x;
    if (x < 1.0) return 1.0 - x;
    return 0.0;
}

double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

double filter_support(int filter) { return filter == OCM_RESAMPLE_BILINEAR ? 1.0 : 2.0; }

// scale as Pillow forms it: the box edges are floats and so is their difference
double axis_scale(double in0, double in1, int out_size) { return (double)((float)in1 - (float)in0) / out_size; }

int axis_check(const char *who, int filter, int in_size, double in0, double in1, int out_size) {
    if (filter != OCM_RESAMPLE_NEAREST && filter != OCM_RESAMPLE_BILINEAR && filter != OCM_RESAMPLE_BICUBIC)
        return fail(OCM_EINVAL, "%s: filter = %d (0 nearest, 2 bilinear, 3 bicubic)", who, filter);
    if (in_size < 1) return fail(OCM_EINVAL, "%s: in_size = %d (>= 1)", who, in_size);
    if (out_size < 1) return fail(OCM_EINVAL, "%s: out_size = %d (>= 1)", who, out_size);
    if (!(in1 > in0)) return fail(OCM_EINVAL, "%s: empty box %g .. %g (in1 > in0)", who, in0, in1);
    if (!(in0 >= 0.0) || !(in1 <= (double)in_size))
        return fail(OCM_EINVAL, "%s: box %g .. %g outside 0 .. %d", who, in0, in1, in_size);
    return OCM_OK;
}

int axis_ksize(int filter, double in0, double in1, int out_size) {
    if (filter == OCM_RESAMPLE_NEAREST) return 1;
    double filterscale = axis_scale(in0, in1, out_size);
    if (filterscale < 1.0) filterscale = 1.0;
    const double k = std::ceil(filter_support(filter) * filterscale) * 2 + 1;
    return k > (double)(INT_MAX / 2) ? -1 : (int)k;
}

}  // namespace

extern "C" int32_t ocm_resample_ksize(int32_t filter, int32_t in_size, double in0, double in1, int32_t out_size) {
    if (const int rc = axis_check("resample_ksize", filter, in_size, in0, in1, out_size)) return -rc;
    const int k = axis_ksize(filter, in0, in1, out_size);
    return k < 0 ? -fail(OCM_EINVAL, "resample_ksize: the taps of %g .. %g -> %d do not fit an int", in0, in1, out_size) : k;
}

extern "C" int ocm_resample_table(int32_t filter, int32_t in_size, double in0, double in1, int32_t out_size, int32_t flip,
                                  int32_t ksize_padded, int32_t *bounds, int32_t *coeffs) {
    if (const int rc = axis_check("resample_table", filter, in_size, in0, in1, out_size)) return rc;
    if (!bounds || !coeffs) return fail(OCM_EINVAL, "resample_table: null argument");
    const int ksize = axis_ksize(filter, in0, in1, out_size);
    if (ksize < 0 || ksize_padded < ksize)
        return fail(OCM_EINVAL, "resample_table: ksize_padded = %d is too small for %d taps", ksize_padded, ksize);
    in0 = (double)(float)in0, in1 = (double)(float)in1;
    const double scale = axis_scale(in0, in1, out_size);
    auto slot = [&](int xx) { return (size_t)(flip ? out_size - 1 - xx : xx); };
    for (size_t i = 0; i < (size_t)out_size * ksize_padded; ++i) coeffs[i] = 0;

    if (filter == OCM_RESAMPLE_NEAREST) {  // ImagingScaleAffine: the position is a running sum, truncated
        double xo = in0 + scale * 0.5;
        for (int xx = 0; xx < out_size; ++xx, xo += scale) {
            const int xin = xo < 0.0 ? -1 : (int)xo;
            const bool in = xin >= 0 && xin < in_size;  // outside: no tap, the pixel is 0
            bounds[2 * slot(xx)] = in ? xin : 0, bounds[2 * slot(xx) + 1] = in;
            coeffs[slot(xx) * ksize_padded] = in ? 1 << RS_PRECISION_BITS : 0;
        }
        return OCM_OK;
    }

    double (*filt)(double) = filter == OCM_RESAMPLE_BILINEAR ? bilinear_filter : bicubic_filter;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = filter_support(filter) * filterscale;
    const double ss = 1.0 / filterscale;
    std::vector<double> k((size_t)ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = in0 + (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        if (xmax < 0) xmax = 0;
        if (xmax > ksize) xmax = ksize;
        for (int x = 0; x < xmax; ++x) {
            const double w = filt((x + xmin - center + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        int32_t *out = coeffs + slot(xx) * ksize_padded;
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) k[x] /= ww;
            out[x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << RS_PRECISION_BITS)) : (int)(0.5 + k[x] * (1 << RS_PRECISION_BITS));
        }
        bounds[2 * slot(xx)] = xmin, bounds[2 * slot(xx) + 1] = xmax;
    }
    return OCM_OK;
}

// [batch][tmp_rows][out_w][chans] bytes: the horizontal pass's result
extern "C" size_t ocm_resample_u8_workspace_bytes(int32_t batch, int32_t chans, int32_t tmp_rows, int32_t out_w) {
    if (batch < 1 || batch > 65535 || (chans != 1 && chans != 3) || tmp_rows < 1 || tmp_rows > RS_MAX_ROWS || out_w < 1 ||
        (int64_t)out_w * chans > RS_MAX_ROW_BYTES)
        return 0;
    return align256((size_t)batch * tmp_rows * out_w * chans);
}

extern "C" int ocm_op_resample_u8(const uint8_t *src, int64_t stride_b, int64_t stride_y, int64_t stride_x, int64_t stride_c,
                                  int32_t batch, int32_t chans, int32_t src_h, int32_t src_w, const int32_t *rects,
                                  int32_t tmp_rows, const int32_t *xbounds, const int32_t *xcoeffs, int32_t xksize,
                                  const int32_t *ybounds, const int32_t *ycoeffs, int32_t yksize, int32_t per_image,
                                  int32_t out_h, int32_t out_w, uint8_t *out_u8, float *out_f32, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    if (!src || !xbounds || !xcoeffs || !ybounds || !ycoeffs) return fail(OCM_EINVAL, "resample_u8: null argument");
    if (!out_u8 && !out_f32) return fail(OCM_EINVAL, "resample_u8: null outputs (uint8, float32 or both)");
    if (batch < 1 || batch > 65535) return fail(OCM_EINVAL, "resample_u8: batch = %d (1..65535)", batch);
    if (chans != 1 && chans != 3) return fail(OCM_EINVAL, "resample_u8: chans = %d (1 or 3)", chans);
    if (src_h < 1 || src_w < 1 || src_h > RS_MAX_ROWS || src_w > RS_MAX_ROW_BYTES)
        return fail(OCM_EINVAL, "resample_u8: source size %d x %d (1..2^19 rows of 1..2^26 pixels)", src_h, src_w);
    if (stride_b < 0 || stride_y < 0 || stride_x < 0 || stride_c < 0)
        return fail(OCM_EINVAL, "resample_u8: negative stride (%lld, %lld, %lld, %lld)", (long long)stride_b, (long long)stride_y,
                    (long long)stride_x, (long long)stride_c);
    if (out_h < 1 || out_h > 65535 || out_w < 1 || (int64_t)out_w * chans > RS_MAX_ROW_BYTES)
        return fail(OCM_EINVAL, "resample_u8: output size %d x %d (1..65535 rows of up to 2^26 bytes)", out_h, out_w);
    if (xksize < 1 || yksize < 1) return fail(OCM_EINVAL, "resample_u8: ksize = %d, %d (>= 1)", xksize, yksize);
    if (tmp_rows < 1 || tmp_rows > RS_MAX_ROWS || (!rects && tmp_rows < src_h))
        return fail(OCM_EINVAL, "resample_u8: tmp_rows = %d (1..2^19, and the %d source rows when there are no rectangles)", tmp_rows,
                    src_h);
    const size_t need = ocm_resample_u8_workspace_bytes(batch, chans, tmp_rows, out_w);
    if (!workspace || workspace_bytes < need)
        return fail(OCM_ENOMEM, "resample_u8 workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace & 15) return fail(OCM_EINVAL, "resample_u8 workspace: not 16-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const RsSrc in = {src, stride_b, stride_y, stride_x, stride_c, src_h, src_w};
    uint8_t *tmp = (uint8_t *)workspace;
    const dim3 gh((out_w + RS_HTILE_W - 1) / RS_HTILE_W, (tmp_rows + RS_HTILE_ROWS - 1) / RS_HTILE_ROWS, batch);
    const dim3 gv((out_w * chans + RS_VTILE - 1) / RS_VTILE, out_h, batch);
    if (chans == 1) {
        resample_h_kernel<1><<<gh, dim3(RS_THREADS), 0, s>>>(in, rects, xbounds, xcoeffs, xksize, per_image != 0, tmp, tmp_rows, out_w);
        HIP_TRY(hipGetLastError());
        resample_v_kernel<1><<<gv, dim3(RS_THREADS), 0, s>>>(tmp, tmp_rows, rects, src_h, src_w, ybounds, ycoeffs, yksize,
                                                            per_image != 0, out_h, out_w, out_u8, out_f32);
    } else {
        resample_h_kernel<3><<<gh, dim3(RS_THREADS), 0, s>>>(in, rects, xbounds, xcoeffs, xksize, per_image != 0, tmp, tmp_rows, out_w);
        HIP_TRY(hipGetLastError());
        resample_v_kernel<3><<<gv, dim3(RS_THREADS), 0, s>>>(tmp, tmp_rows, rects, src_h, src_w, ybounds, ycoeffs, yksize,
                                                            per_image != 0, out_h, out_w, out_u8, out_f32);
    }
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}
