// kernels_optim.hip — the third call of every training loop: optimizer.step() (torch.optim's AdamW, Adam and SGD, single-tensor
// rules), the global gradient norm (utils.py:363 get_grad_norm) and clip_grad_norm_'s scaling, each as ONE launch over many
// tensors instead of a pass per tensor. Everything is fp32, elementwise and memory-bound.
//   The table of a launch travels by value in the kernel arguments: up to OP_MAX_TENSORS tensors (param, grad, m, v, count) and a
//   map of up to OP_MAX_BLOCKS workgroups, one entry = (table slot, chunk of OP_CHUNK elements of that tensor). A call of N tensors
//   is a few launches (a new one whenever the slots or the map are full; a tensor may continue in the next launch). No table in
//   device memory, hence no copy, no allocation and nothing to keep alive; nothing synchronises with the host.
//   The grid of a launch is its map: one workgroup per chunk, whose threads walk the chunk's quads in steps of the workgroup
//   (there is no loop over chunks inside a workgroup).
//   optim_step_kernel<RULE>  one workgroup updates one chunk in place.
//   sumsq_kernel             one workgroup writes the float64 sum of squares of one chunk of a gradient to partial[global chunk].
//   norm_finish_kernel       one workgroup adds the partials and writes the sum (float64), the norm and the clip coefficient.
//   grad_scale_kernel        one workgroup multiplies one chunk of a gradient by the coefficient it reads from device memory.
//   ema_kernel               one workgroup moves one chunk of a teacher tensor towards its student's (DINO's momentum encoder).
// A thread owns quads of four consecutive elements (quad i of a chunk: thread i % 256, in rising i) and the chunk's tail of
// count % 4 elements goes one element per thread: 16-byte loads and stores when every pointer of the tensor is 16-byte aligned
// (OP_CHUNK is a multiple of 4, so a chunk is aligned as its tensor is), element accesses otherwise (a parameter that is a view
// at an odd offset). Both ways give a thread the same elements in the same order, and the sums are added in one fixed order (per
// thread, the xor butterfly of a wave, the waves in order, the partials by thread and the same tree): no atomics, equal inputs
// give equal bits wherever they lie. No access goes past `count` elements of any pointer.
#include <cmath>

#include "common.h"
#include "host_common.h"

#define fail ocm_fail

// the rules are torch's, operation by operation: every product and sum rounded on its own
#pragma clang fp contract(off)

namespace {

constexpr int OP_THREADS = 256;
constexpr int OP_CHUNK = 8192;         // elements per workgroup: eight quads per thread
constexpr int OP_MAX_TENSORS = 32;     // table slots per launch
constexpr int OP_MAX_BLOCKS = 512;     // map entries = workgroups per launch
constexpr int64_t OP_MAX_COUNT = (int64_t)1 << 36;  // the map holds a chunk index in 24 bits: 2^24 * 8192 = 2^37 elements
static_assert(OP_CHUNK % 4 == 0 && OP_MAX_TENSORS <= 256, "a chunk keeps its tensor's alignment; the slot takes 8 bits of a map entry");

struct OptimTable {
    float *p[OP_MAX_TENSORS];
    float *g[OP_MAX_TENSORS];
    float *m[OP_MAX_TENSORS];
    float *v[OP_MAX_TENSORS];
    int64_t count[OP_MAX_TENSORS];
    uint32_t map[OP_MAX_BLOCKS];  // slot << 24 | chunk
};

struct StepScalars {
    float decay;      // AdamW: 1 - lr * weight_decay
    float wd;         // Adam, SGD: g' = g + wd * p
    float w1;         // 1 - beta1
    float beta2, w2;  // w2 = 1 - beta2
    float step_size, bc2_sqrt, eps;
    float lr, momentum, w_damp;  // SGD; w_damp = 1 - dampening
    int32_t has_momentum, nesterov, first_step;
};
static_assert(sizeof(OptimTable) + sizeof(StepScalars) + 64 <= 4096, "the arguments of a launch must fit 4 KiB");

enum { RULE_ADAMW = OCM_OPTIM_ADAMW, RULE_ADAM = OCM_OPTIM_ADAM, RULE_SGD = OCM_OPTIM_SGD };

__device__ __forceinline__ f32x4 load4(const float *p, bool vec) {
    if (vec) return *(const f32x4 *)p;
    f32x4 v;
    v[0] = p[0], v[1] = p[1], v[2] = p[2], v[3] = p[3];
    return v;
}

__device__ __forceinline__ void store4(float *p, f32x4 v, bool vec) {
    if (vec) {
        *(f32x4 *)p = v;
    } else {
        p[0] = v[0], p[1] = v[1], p[2] = v[2], p[3] = v[3];
    }
}

// torch/optim/adam.py _single_tensor_adam and sgd.py _single_tensor_sgd, one element
template <int RULE>
__device__ __forceinline__ void update(float &p, float g, float &m, float &v, const StepScalars &s) {
    if constexpr (RULE == RULE_SGD) {
        if (s.wd != 0.f) g = g + s.wd * p;
        if (s.has_momentum) {
            m = s.first_step ? g : m * s.momentum + s.w_damp * g;
            g = s.nesterov ? g + s.momentum * m : m;
        }
        p = p + (-s.lr) * g;
    } else {
        if constexpr (RULE == RULE_ADAMW) {
            p = p * s.decay;
        } else {
            if (s.wd != 0.f) g = g + s.wd * p;
        }
        m = m + s.w1 * (g - m);            // lerp(m, g, 1 - beta1), the weight below one half
        v = v * s.beta2 + (s.w2 * g) * g;  // mul_(beta2).addcmul_(g, g, value = 1 - beta2)
        const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
        p = p + (-s.step_size) * (m / denom);
    }
}

template <int RULE>
__global__ __launch_bounds__(OP_THREADS) void optim_step_kernel(const OptimTable tab, const StepScalars s) {
    const uint32_t e = tab.map[blockIdx.x];
    const int t = (int)(e >> 24);
    const int64_t off = (int64_t)(e & 0xffffffu) * OP_CHUNK;
    const int n = (int)std::min<int64_t>(OP_CHUNK, tab.count[t] - off);
    constexpr bool ADAM = RULE != RULE_SGD;
    const bool use_m = ADAM || s.has_momentum;
    float *p = tab.p[t] + off;
    const float *g = tab.g[t] + off;
    float *m = use_m ? tab.m[t] + off : nullptr;
    float *v = ADAM ? tab.v[t] + off : nullptr;
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
    const int nq = n / 4;
    for (int i = threadIdx.x; i < nq; i += OP_THREADS) {
        f32x4 pv = load4(p + 4 * i, vec);
        const f32x4 gv = load4(g + 4 * i, vec);
        f32x4 mv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
        if (use_m && !(RULE == RULE_SGD && s.first_step)) mv = load4(m + 4 * i, vec);
        if (ADAM) vv = load4(v + 4 * i, vec);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pe = pv[k], me = mv[k], ve = vv[k];
            update<RULE>(pe, gv[k], me, ve, s);
            pv[k] = pe, mv[k] = me, vv[k] = ve;
        }
        store4(p + 4 * i, pv, vec);
        if (use_m) store4(m + 4 * i, mv, vec);
        if (ADAM) store4(v + 4 * i, vv, vec);
    }
    const int i = 4 * nq + (int)threadIdx.x;
    if (i < n) {
        float pe = p[i], me = 0.f, ve = 0.f;
        if (use_m && !(RULE == RULE_SGD && s.first_step)) me = m[i];
        if (ADAM) ve = v[i];
        update<RULE>(pe, g[i], me, ve, s);
        p[i] = pe;
        if (use_m) m[i] = me;
        if (ADAM) v[i] = ve;
    }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the workgroup's sum, valid in thread 0
__device__ __forceinline__ double block_sum(double v, double *s_wave) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        r = s_wave[0];
#pragma unroll
        for (int k = 1; k < OP_THREADS / 64; ++k) r += s_wave[k];
    }
    return r;
}

__global__ __launch_bounds__(OP_THREADS) void sumsq_kernel(const OptimTable tab, double *__restrict__ partial) {
    __shared__ double s_wave[OP_THREADS / 64];
    const uint32_t e = tab.map[blockIdx.x];
    const int t = (int)(e >> 24);
    const int64_t off = (int64_t)(e & 0xffffffu) * OP_CHUNK;
    const int n = (int)std::min<int64_t>(OP_CHUNK, tab.count[t] - off);
    const float *g = tab.g[t] + off;
    const bool vec = ((uintptr_t)g & 15) == 0;
    const int nq = n / 4;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nq; i += OP_THREADS) {
        const f32x4 gv = load4(g + 4 * i, vec);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += (double)gv[k] * (double)gv[k];
    }
    const int i = 4 * nq + (int)threadIdx.x;
    if (i < n) acc += (double)g[i] * (double)g[i];
    const double r = block_sum(acc, s_wave);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// one workgroup. coef = clamp(max_norm / (norm + 1e-6), max = 1) in fp32, as torch.nn.utils.clip_grad_norm_ forms it: a NaN norm
// gives a NaN coefficient, an infinite one 0
__global__ __launch_bounds__(OP_THREADS) void norm_finish_kernel(const double *__restrict__ partial, int64_t chunks, float max_norm,
                                                                 double *__restrict__ sumsq, float *__restrict__ norm,
                                                                 float *__restrict__ coef) {
    __shared__ double s_wave[OP_THREADS / 64];
    double acc = 0.0;
    for (int64_t c = threadIdx.x; c < chunks; c += OP_THREADS) acc += partial[c];
    const double r = block_sum(acc, s_wave);
    if (threadIdx.x != 0) return;
    const float nrm = (float)sqrt(r);
    float c = max_norm / (nrm + 1e-6f);
    if (c > 1.0f) c = 1.0f;
    *sumsq = r;
    *norm = nrm;
    *coef = c;
}

__global__ __launch_bounds__(OP_THREADS) void grad_scale_kernel(const OptimTable tab, const float *__restrict__ coef) {
    const uint32_t e = tab.map[blockIdx.x];
    const int t = (int)(e >> 24);
    const int64_t off = (int64_t)(e & 0xffffffu) * OP_CHUNK;
    const int n = (int)std::min<int64_t>(OP_CHUNK, tab.count[t] - off);
    float *g = tab.g[t] + off;
    const bool vec = ((uintptr_t)g & 15) == 0;
    const float c = *coef;
    const int nq = n / 4;
    for (int i = threadIdx.x; i < nq; i += OP_THREADS) {
        f32x4 gv = load4(g + 4 * i, vec);
#pragma unroll
        for (int k = 0; k < 4; ++k) gv[k] = gv[k] * c;
        store4(g + 4 * i, gv, vec);
    }
    const int i = 4 * nq + (int)threadIdx.x;
    if (i < n) g[i] = g[i] * c;
}

// p = p * m + g * w (torch's p.mul_(m).add_(w * q)), one chunk per workgroup
__global__ __launch_bounds__(OP_THREADS) void ema_kernel(const OptimTable tab, float m, float w) {
    const uint32_t e = tab.map[blockIdx.x];
    const int t = (int)(e >> 24);
    const int64_t off = (int64_t)(e & 0xffffffu) * OP_CHUNK;
    const int n = (int)std::min<int64_t>(OP_CHUNK, tab.count[t] - off);
    float *p = tab.p[t] + off;
    const float *g = tab.g[t] + off;
    const bool vec = (((uintptr_t)p | (uintptr_t)g) & 15) == 0;
    const int nq = n / 4;
    for (int i = threadIdx.x; i < nq; i += OP_THREADS) {
        f32x4 pv = load4(p + 4 * i, vec);
        const f32x4 gv = load4(g + 4 * i, vec);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float keep = pv[k] * m;
            const float add = gv[k] * w;
            pv[k] = keep + add;
        }
        store4(p + 4 * i, pv, vec);
    }
    const int i = 4 * nq + (int)threadIdx.x;
    if (i < n) {
        const float keep = p[i] * m;
        const float add = g[i] * w;
        p[i] = keep + add;
    }
}

int64_t chunks_of(int64_t count) { return (count + OP_CHUNK - 1) / OP_CHUNK; }

// which of a descriptor's pointers an operator dereferences
struct Needs {
    bool p, g, m, v;
};

int check_table(const char *op, const OcmOptimTensor *tensors, int32_t n, Needs need) {
    if (!tensors) return fail(OCM_EINVAL, "%s: null tensor table", op);
    if (n < 0) return fail(OCM_EINVAL, "%s: %d tensors", op, n);
    for (int32_t i = 0; i < n; ++i) {
        const OcmOptimTensor &t = tensors[i];
        if (t.count < 0 || t.count > OP_MAX_COUNT)
            return fail(OCM_EINVAL, "%s: tensor %d: count = %lld (0..2^36 elements)", op, i, (long long)t.count);
        if (t.count == 0) continue;  // an empty tensor has no address
        if (need.p && !t.param) return fail(OCM_EINVAL, "%s: tensor %d: null param", op, i);
        if (need.g && !t.grad) return fail(OCM_EINVAL, "%s: tensor %d: null grad", op, i);
        if (need.m && !t.m) return fail(OCM_EINVAL, "%s: tensor %d: null m", op, i);
        if (need.v && !t.v) return fail(OCM_EINVAL, "%s: tensor %d: null v", op, i);
        if (((uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.m | (uintptr_t)t.v) & 3)
            return fail(OCM_EINVAL, "%s: tensor %d: a pointer is not 4-byte aligned", op, i);
    }
    return OCM_OK;
}

// Cuts the table into launches and calls launch(tab, workgroups, chunks before this launch) for each, in order.
template <class F>
int for_each_launch(const OcmOptimTensor *tensors, int32_t n, F launch) {
    OptimTable tab = {};
    int nt = 0, nb = 0;
    int64_t done = 0;
    auto flush = [&]() -> int {
        if (!nb) return OCM_OK;
        const int rc = launch(tab, nb, done);
        done += nb;
        nt = nb = 0;
        return rc;
    };
    for (int32_t i = 0; i < n; ++i) {
        const OcmOptimTensor &t = tensors[i];
        const int64_t nchunks = chunks_of(t.count);
        for (int64_t c = 0; c < nchunks;) {
            if (nt == OP_MAX_TENSORS || nb == OP_MAX_BLOCKS) {
                const int rc = flush();
                if (rc != OCM_OK) return rc;
            }
            tab.p[nt] = (float *)t.param, tab.g[nt] = (float *)t.grad, tab.m[nt] = (float *)t.m, tab.v[nt] = (float *)t.v;
            tab.count[nt] = t.count;
            const int64_t k = std::min<int64_t>(nchunks - c, OP_MAX_BLOCKS - nb);
            for (int64_t j = 0; j < k; ++j) tab.map[nb + j] = (uint32_t)nt << 24 | (uint32_t)(c + j);
            nb += (int)k, c += k, ++nt;
        }
    }
    return flush();
}

int64_t total_chunks(const OcmOptimTensor *tensors, int32_t n) {
    int64_t total = 0;
    for (int32_t i = 0; i < n; ++i) total += chunks_of(tensors[i].count);
    return total;
}

bool counts_ok(const OcmOptimTensor *tensors, int32_t n) {
    if (!tensors || n < 0) return false;
    for (int32_t i = 0; i < n; ++i)
        if (tensors[i].count < 0 || tensors[i].count > OP_MAX_COUNT) return false;
    return true;
}

}  // namespace

extern "C" void ocm_optim_limits(int32_t *max_tensors, int32_t *chunk_elems) {
    if (max_tensors) *max_tensors = OP_MAX_TENSORS;
    if (chunk_elems) *chunk_elems = OP_CHUNK;
}

extern "C" int ocm_op_optim_step(const OcmOptimTensor *tensors, int32_t n, const OcmOptimHyper *hyper, void *stream) {
    if (!hyper) return fail(OCM_EINVAL, "optim_step: null hyper-parameters");
    const OcmOptimHyper &h = *hyper;
    if (h.rule != OCM_OPTIM_ADAMW && h.rule != OCM_OPTIM_ADAM && h.rule != OCM_OPTIM_SGD)
        return fail(OCM_EINVAL, "optim_step: unknown rule %d", h.rule);
    const bool adam = h.rule != OCM_OPTIM_SGD;
    if (!std::isfinite(h.lr) || !std::isfinite(h.weight_decay))
        return fail(OCM_EINVAL, "optim_step: lr = %g, weight_decay = %g (finite)", h.lr, h.weight_decay);
    if (adam && !(std::isfinite(h.step_size) && std::isfinite(h.beta1) && std::isfinite(h.beta2) && std::isfinite(h.eps) &&
                  h.bias_correction2_sqrt > 0.0 && std::isfinite(h.bias_correction2_sqrt)))
        return fail(OCM_EINVAL, "optim_step: betas (%g, %g), eps %g, step_size %g, bias_correction2_sqrt %g (finite, the last > 0)",
                    h.beta1, h.beta2, h.eps, h.step_size, h.bias_correction2_sqrt);
    if (!adam && !(std::isfinite(h.momentum) && std::isfinite(h.dampening)))
        return fail(OCM_EINVAL, "optim_step: momentum = %g, dampening = %g (finite)", h.momentum, h.dampening);
    const bool has_momentum = !adam && h.momentum != 0.0;
    const int rc = check_table("optim_step", tensors, n, Needs{true, true, adam || has_momentum, adam});
    if (rc != OCM_OK) return rc;
    // the factors in double, as torch's Python forms them, then one rounding to the tensors' type
    StepScalars s = {};
    s.decay = (float)(1.0 - h.lr * h.weight_decay);
    s.wd = (float)h.weight_decay;
    s.w1 = (float)(1.0 - h.beta1);
    s.beta2 = (float)h.beta2;
    s.w2 = (float)(1.0 - h.beta2);
    s.step_size = (float)h.step_size;
    s.bc2_sqrt = (float)h.bias_correction2_sqrt;
    s.eps = (float)h.eps;
    s.lr = (float)h.lr;
    s.momentum = (float)h.momentum;
    s.w_damp = (float)(1.0 - h.dampening);
    s.has_momentum = has_momentum, s.nesterov = h.nesterov != 0, s.first_step = h.first_step != 0;
    const hipStream_t st = (hipStream_t)stream;
    return for_each_launch(tensors, n, [&](const OptimTable &tab, int blocks, int64_t) -> int {
        if (h.rule == OCM_OPTIM_ADAMW)
            optim_step_kernel<RULE_ADAMW><<<dim3(blocks), dim3(OP_THREADS), 0, st>>>(tab, s);
        else if (h.rule == OCM_OPTIM_ADAM)
            optim_step_kernel<RULE_ADAM><<<dim3(blocks), dim3(OP_THREADS), 0, st>>>(tab, s);
        else
            optim_step_kernel<RULE_SGD><<<dim3(blocks), dim3(OP_THREADS), 0, st>>>(tab, s);
        HIP_TRY(hipGetLastError());
        return OCM_OK;
    });
}

extern "C" int ocm_op_ema_update(const OcmOptimTensor *tensors, int32_t n, double momentum, void *stream) {
    if (!std::isfinite(momentum)) return fail(OCM_EINVAL, "ema_update: momentum = %g (finite)", momentum);
    const int rc = check_table("ema_update", tensors, n, Needs{true, true, false, false});
    if (rc != OCM_OK) return rc;
    const float m = (float)momentum, w = (float)(1.0 - momentum);
    const hipStream_t st = (hipStream_t)stream;
    return for_each_launch(tensors, n, [&](const OptimTable &tab, int blocks, int64_t) -> int {
        ema_kernel<<<dim3(blocks), dim3(OP_THREADS), 0, st>>>(tab, m, w);
        HIP_TRY(hipGetLastError());
        return OCM_OK;
    });
}

// [partials: one float64 per chunk of every tensor]; 0 for a table the operator refuses
extern "C" size_t ocm_grad_norm_workspace_bytes(const OcmOptimTensor *tensors, int32_t n) {
    if (!counts_ok(tensors, n)) return 0;
    return (size_t)std::max<int64_t>(total_chunks(tensors, n), 1) * sizeof(double);
}

extern "C" int ocm_op_grad_norm(const OcmOptimTensor *tensors, int32_t n, double max_norm, double *sumsq, float *norm, float *coef,
                                void *workspace, size_t workspace_bytes, void *stream) {
    const int rc = check_table("grad_norm", tensors, n, Needs{false, true, false, false});
    if (rc != OCM_OK) return rc;
    if (!sumsq || !norm || !coef) return fail(OCM_EINVAL, "grad_norm: null output");
    const size_t need = ocm_grad_norm_workspace_bytes(tensors, n);
    if (!workspace || workspace_bytes < need)
        return fail(OCM_EINVAL, "grad_norm workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace & 7) return fail(OCM_EINVAL, "grad_norm workspace: not 8-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    double *partial = (double *)workspace;
    const int rc2 = for_each_launch(tensors, n, [&](const OptimTable &tab, int blocks, int64_t done) -> int {
        sumsq_kernel<<<dim3(blocks), dim3(OP_THREADS), 0, st>>>(tab, partial + done);
        HIP_TRY(hipGetLastError());
        return OCM_OK;
    });
    if (rc2 != OCM_OK) return rc2;
    norm_finish_kernel<<<dim3(1), dim3(OP_THREADS), 0, st>>>(partial, total_chunks(tensors, n), (float)max_norm, sumsq, norm, coef);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_grad_scale(const OcmOptimTensor *tensors, int32_t n, const float *coef, void *stream) {
    const int rc = check_table("grad_scale", tensors, n, Needs{false, true, false, false});
    if (rc != OCM_OK) return rc;
    if (!coef) return fail(OCM_EINVAL, "grad_scale: null coefficient");
    const hipStream_t st = (hipStream_t)stream;
    return for_each_launch(tensors, n, [&](const OptimTable &tab, int blocks, int64_t) -> int {
        grad_scale_kernel<<<dim3(blocks), dim3(OP_THREADS), 0, st>>>(tab, coef);
        HIP_TRY(hipGetLastError());
        return OCM_OK;
    });
}
