// kernels_morph.hip — the query-point chain of analyse_attention.py --region_query (reference analyse_attention.py:183-223,
// utils.py:237-281) and of data.py's ROI masking (data.py:216-233, get_ROIs) on device: binary masks, 8-connected component
// labelling with raster-ordered labels, exact per-region integer sums, small-object removal, binary dilation / erosion with a
// border value, and the mean over query points of head-mean attention maps.
//
// Labelling is a union-find over int32 pixel indices i = y * w + x (one array per image) whose only link operation is an integer
// atomic minimum, so that parent[i] <= i holds at every moment:
//   label_tile_kernel     one workgroup per 32 x 32 tile: union-find in LDS over the tile's pixels (links to the W, N, NW, NE
//                         neighbours inside the tile), then parent[i] = global index of the tile-local root, -1 on background
//   label_merge_kernel    every pixel on a tile's top row / left column is united with its 8-neighbours in the adjacent tiles
//                         (agent-scope atomic minimum on the global parents)
//   label_flatten_kernel  parent[i] = root(i); counts the roots (parent[i] == i) of every 1024-pixel chunk
//   label_scan_kernel     exclusive scan of the chunk counts of an image (one workgroup per image), counts[b] = their total
//   label_rank_kernel     rank[r] = 1 + number of roots before r in raster order, for every root r
//   label_relabel_kernel  labels[i] = rank[parent[i]], 0 on background
// A link always hangs the larger of two roots under the smaller one, so the root of a finished component is its smallest pixel
// index whatever order the links arrived in: the flattened parents, and therefore the labels, do not depend on scheduling. The
// rank of a root among the roots in index order is the raster order of the components' first pixels (skimage.measure.label /
// scipy.ndimage.label numbering). No workgroup waits for another one: a `find` walks strictly decreasing parents and a failed
// link retries with a strictly smaller pair of roots; everything that must be complete before the next step is separated from it
// by a kernel boundary.
#include <climits>

#include "host_common.h"

#define fail ocm_fail

// query_mean restates numpy's float32 sums: separate IEEE operations, as in kernels_post.hip
#pragma clang fp contract(off)

namespace {

constexpr int LT = 32;            // labelling tile side: 1024 pixels, four per thread
constexpr int LT_PIX = LT * LT;
constexpr int CHUNK = 1024;       // pixels per workgroup in the flatten / rank passes
constexpr int SEG = 16;           // pixels of one row a thread walks in region_stats

// ---- union-find on int32 parents with parent[i] <= i ---------------------------------------------------------------------------
template <bool GLOBAL>
__device__ __forceinline__ int load_parent(int *p, int i) {
    return GLOBAL ? __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                  : __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <bool GLOBAL>
__device__ __forceinline__ int lower_parent(int *p, int i, int v) {
    return GLOBAL ? __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                  : __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Walks parents while they strictly decrease (and stay non-negative): at most i steps, whatever other threads store meanwhile.
// On the way every visited pixel that has a grandparent is hung under it (path halving, again an atomic minimum: a non-root
// gets a smaller ancestor of its own tree), so that the long chains a thin winding component builds stay short for the next walk.
template <bool GLOBAL>
__device__ __forceinline__ int find_root(int *p, int i) {
    for (;;) {
        const int q = load_parent<GLOBAL>(p, i);
        if ((unsigned)q >= (unsigned)i) return i;  // a root (q == i); q > i or q < 0 cannot occur and would end the walk too
        const int g = load_parent<GLOBAL>(p, q);
        if ((unsigned)g < (unsigned)q) lower_parent<GLOBAL>(p, i, g);
        i = q;
    }
}

// Joins the trees of a and b: the larger root is hung under the smaller one with an atomic minimum. When the larger root b got
// another parent `old` in the meantime the minimum has kept the smaller of the two links and the other one (a — old) is made
// next: max(a, b) strictly decreases from one attempt to the next, so the loop ends after a bounded number of steps on its own.
template <bool GLOBAL>
__device__ __forceinline__ void unite(int *p, int a, int b) {
    for (;;) {
        a = find_root<GLOBAL>(p, a);
        b = find_root<GLOBAL>(p, b);
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = lower_parent<GLOBAL>(p, b, a);
        if (old == b) return;
        b = old;
    }
}

// grid (tiles_x, tiles_y, batch). Thread t owns the four pixels (row t / 8, columns 4 (t % 8) ..) of the tile.
__global__ __launch_bounds__(256) void label_tile_kernel(const uint8_t *__restrict__ mask, int *__restrict__ parent, int h, int w) {
    __shared__ int s_par[LT_PIX];
    const size_t img = (size_t)blockIdx.z * h * w;
    const int tx0 = blockIdx.x * LT, ty0 = blockIdx.y * LT;
    const int ly = threadIdx.x >> 3, lx0 = (threadIdx.x & 7) * 4;
    const int y = ty0 + ly;
    bool fg[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = tx0 + lx0 + k;
        fg[k] = y < h && x < w && mask[img + (size_t)y * w + x] != 0;
        s_par[ly * LT + lx0 + k] = fg[k] ? ly * LT + lx0 + k : -1;
    }
    __syncthreads();
    // links to the neighbours that precede a pixel in raster order. W is always linked; with N present NW and NE are reached
    // through N's and NE's own W links.
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!fg[k]) continue;
        const int lx = lx0 + k, l = ly * LT + lx;
        if (lx > 0 && load_parent<false>(s_par, l - 1) >= 0) unite<false>(s_par, l, l - 1);
        if (ly > 0) {
            if (load_parent<false>(s_par, l - LT) >= 0) {
                unite<false>(s_par, l, l - LT);
            } else {
                if (lx > 0 && load_parent<false>(s_par, l - LT - 1) >= 0) unite<false>(s_par, l, l - LT - 1);
                if (lx < LT - 1 && load_parent<false>(s_par, l - LT + 1) >= 0) unite<false>(s_par, l, l - LT + 1);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = tx0 + lx0 + k;
        if (y >= h || x >= w) continue;
        int v = -1;
        if (fg[k]) {
            const int r = find_root<false>(s_par, ly * LT + lx0 + k);  // local and global raster orders agree inside a tile
            v = (ty0 + r / LT) * w + tx0 + r % LT;
        }
        parent[img + (size_t)y * w + x] = v;
    }
}

// grid (blocks, batch). Items: the (tiles_y - 1) * w pixels on the top rows of the tile rows 1.., then the (tiles_x - 1) * h
// pixels on the left columns of the tile columns 1... Whether a pixel is foreground (parent >= 0) never changes here.
__global__ __launch_bounds__(256) void label_merge_kernel(int *parent, int h, int w, int n_top, int n_left) {
    parent += (size_t)blockIdx.y * h * w;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_top + n_left; i += gridDim.x * 256) {
        if (i < n_top) {
            const int y = (i / w + 1) * LT, x = i % w, c = y * w + x;
            if (load_parent<true>(parent, c) < 0) continue;
            for (int xx = max(x - 1, 0); xx <= min(x + 1, w - 1); ++xx)
                if (load_parent<true>(parent, (y - 1) * w + xx) >= 0) unite<true>(parent, c, (y - 1) * w + xx);
        } else {
            const int j = i - n_top;
            const int x = (j / h + 1) * LT, y = j % h, c = y * w + x;
            if (load_parent<true>(parent, c) < 0) continue;
            for (int yy = max(y - 1, 0); yy <= min(y + 1, h - 1); ++yy)
                if (load_parent<true>(parent, yy * w + x - 1) >= 0) unite<true>(parent, c, yy * w + x - 1);
        }
    }
}

// grid (nchunk, batch). Roots keep parent[i] == i throughout, so the count does not depend on how far the others have got.
__global__ __launch_bounds__(256) void label_flatten_kernel(int *parent, int n, int *__restrict__ chunk_count) {
    __shared__ int s_cnt;
    parent += (size_t)blockIdx.y * n;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    int roots = 0;
#pragma unroll
    for (int k = 0; k < CHUNK / 256; ++k) {
        const int i = blockIdx.x * CHUNK + k * 256 + threadIdx.x;
        if (i >= n || load_parent<true>(parent, i) < 0) continue;
        const int r = find_root<true>(parent, i);
        if (r != i) __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        roots += r == i;
    }
    if (roots) atomicAdd(&s_cnt, roots);
    __syncthreads();
    if (threadIdx.x == 0) chunk_count[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s_cnt;
}

// grid (batch): chunk_count -> exclusive prefix sums in place, counts[b] = number of components of image b
__global__ __launch_bounds__(256) void label_scan_kernel(int *__restrict__ chunk_count, int nchunk, int *__restrict__ counts) {
    __shared__ int s_wave[4];
    int *c = chunk_count + (size_t)blockIdx.x * nchunk;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int b0 = 0; b0 < nchunk; b0 += 256) {
        const int i = b0 + threadIdx.x;
        const int v = i < nchunk ? c[i] : 0;
        int s = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(s, o, 64);
            if (lane >= o) s += t;
        }
        if (lane == 63) s_wave[wave] = s;
        __syncthreads();
        int pre = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < wave) pre += s_wave[k];
            tot += s_wave[k];
        }
        if (i < nchunk) c[i] = carry + pre + s - v;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

// grid (nchunk, batch): rank[r] for the roots of a chunk, in index order (sub-row k of the chunk, then wave, then lane)
__global__ __launch_bounds__(256) void label_rank_kernel(const int *__restrict__ parent, int n, const int *__restrict__ chunk_offset,
                                                         int *__restrict__ rank) {
    __shared__ int s_cnt[CHUNK / 64];
    parent += (size_t)blockIdx.y * n;
    rank += (size_t)blockIdx.y * n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool root[CHUNK / 256];
    int before[CHUNK / 256];
#pragma unroll
    for (int k = 0; k < CHUNK / 256; ++k) {
        const int i = blockIdx.x * CHUNK + k * 256 + threadIdx.x;
        root[k] = i < n && parent[i] == i;
        const unsigned long long b = __ballot(root[k]);
        before[k] = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) s_cnt[k * 4 + wave] = __popcll(b);
    }
    __syncthreads();
    const int base = chunk_offset[(size_t)blockIdx.y * gridDim.x + blockIdx.x];
#pragma unroll
    for (int k = 0; k < CHUNK / 256; ++k) {
        if (!root[k]) continue;
        int pre = 0;
        for (int j = 0; j < k * 4 + wave; ++j) pre += s_cnt[j];
        rank[blockIdx.x * CHUNK + k * 256 + threadIdx.x] = base + pre + before[k] + 1;
    }
}

// grid (nchunk, batch), in place: only rank slots of roots are read, and those were all written by label_rank_kernel
__global__ __launch_bounds__(256) void label_relabel_kernel(int *__restrict__ labels, int n, const int *__restrict__ rank) {
    labels += (size_t)blockIdx.y * n;
    rank += (size_t)blockIdx.y * n;
#pragma unroll
    for (int k = 0; k < CHUNK / 256; ++k) {
        const int i = blockIdx.x * CHUNK + k * 256 + threadIdx.x;
        if (i >= n) continue;
        const int p = labels[i];
        labels[i] = p < 0 ? 0 : rank[p];
    }
}

// ---- remove_small_objects: flatten, then area[root] += 1 with one atomic per distinct root of a wave ---------------------------
__global__ __launch_bounds__(256) void label_area_kernel(int *parent, int n, int *area) {
    parent += (size_t)blockIdx.y * n;
    area += (size_t)blockIdx.y * n;
    const int lane = threadIdx.x & 63;
    for (int base = blockIdx.x * 256; base < n; base += gridDim.x * 256) {  // wave-uniform trip count
        const int i = base + threadIdx.x;
        const bool act = i < n && load_parent<true>(parent, i) >= 0;
        int r = -1;
        if (act) {
            r = find_root<true>(parent, i);
            if (r != i) __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        unsigned long long todo = __ballot(act);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int L = __shfl(r, leader, 64);
            const unsigned long long same = __ballot(act && r == L);
            if (lane == leader) atomicAdd(area + L, (int)__popcll(same));
            todo &= ~same;
        }
    }
}

__global__ __launch_bounds__(256) void keep_large_kernel(const int *__restrict__ parent, const int *__restrict__ area,
                                                         uint8_t *__restrict__ out, int n, int min_size) {
    parent += (size_t)blockIdx.y * n;
    area += (size_t)blockIdx.y * n;
    out += (size_t)blockIdx.y * n;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int p = parent[i];
        out[i] = p >= 0 && area[p] >= min_size;
    }
}

// ---- region_stats ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void region_init_kernel(long long *__restrict__ area, long long *__restrict__ sum_row,
                                                          long long *__restrict__ sum_col, int *__restrict__ bbox, size_t regions,
                                                          int h, int w) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < regions; i += (size_t)gridDim.x * 256) {
        area[i] = 0;
        sum_row[i] = 0;
        sum_col[i] = 0;
        bbox[4 * i + 0] = h;
        bbox[4 * i + 1] = w;
        bbox[4 * i + 2] = 0;
        bbox[4 * i + 3] = 0;
    }
}

struct RegionRun {
    int label, area, sumc, c0, c1;
};

__device__ __forceinline__ void region_commit(long long *area, long long *sum_row, long long *sum_col, int *bbox, size_t slot,
                                              int a, int sr, int sc, int r0, int c0, int r1, int c1) {
    atomicAdd((unsigned long long *)area + slot, (unsigned long long)a);
    atomicAdd((unsigned long long *)sum_row + slot, (unsigned long long)sr);
    atomicAdd((unsigned long long *)sum_col + slot, (unsigned long long)sc);
    atomicMin(bbox + 4 * slot + 0, r0);
    atomicMin(bbox + 4 * slot + 1, c0);
    atomicMax(bbox + 4 * slot + 2, r1 + 1);
    atomicMax(bbox + 4 * slot + 3, c1 + 1);
}

// grid (blocks, batch). A thread walks SEG pixels of one row and keeps a run per label (background does not end a run); a run
// that ends inside the segment is committed at once, the last one of every lane is first summed over the lanes of the wave that
// hold the same label. All sums are integers: the order of the atomics does not show in the result.
__global__ __launch_bounds__(256) void region_stats_kernel(const int *__restrict__ labels, int h, int w, int max_regions,
                                                           long long *__restrict__ area, long long *__restrict__ sum_row,
                                                           long long *__restrict__ sum_col, int *__restrict__ bbox) {
    labels += (size_t)blockIdx.y * h * w;
    const size_t rbase = (size_t)blockIdx.y * max_regions;
    const int segs = (w + SEG - 1) / SEG, nseg = h * segs;
    const int lane = threadIdx.x & 63;
    for (int base = blockIdx.x * 256; base < nseg; base += gridDim.x * 256) {  // wave-uniform trip count
        const int s = base + threadIdx.x;
        RegionRun run = {0, 0, 0, INT_MAX, -1};
        int y = 0;
        if (s < nseg) {
            y = s / segs;
            const int x0 = (s % segs) * SEG, x1 = min(x0 + SEG, w);
            for (int x = x0; x < x1; ++x) {
                const int l = labels[y * w + x];
                if (l <= 0 || l > max_regions) continue;
                if (l != run.label) {
                    if (run.label)
                        region_commit(area, sum_row, sum_col, bbox, rbase + run.label - 1, run.area, run.area * y, run.sumc, y,
                                      run.c0, y, run.c1);
                    run = {l, 0, 0, x, x};
                }
                ++run.area;
                run.sumc += x;
                run.c1 = x;
            }
        }
        unsigned long long todo = __ballot(run.label != 0);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int L = __shfl(run.label, leader, 64);
            const bool m = run.label == L;
            int a = m ? run.area : 0, sr = m ? run.area * y : 0, sc = m ? run.sumc : 0;
            int r0 = m ? y : INT_MAX, r1 = m ? y : -1, c0 = m ? run.c0 : INT_MAX, c1 = m ? run.c1 : -1;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                a += __shfl_xor(a, o, 64);
                sr += __shfl_xor(sr, o, 64);
                sc += __shfl_xor(sc, o, 64);
                r0 = min(r0, __shfl_xor(r0, o, 64));
                c0 = min(c0, __shfl_xor(c0, o, 64));
                r1 = max(r1, __shfl_xor(r1, o, 64));
                c1 = max(c1, __shfl_xor(c1, o, 64));
            }
            if (lane == leader) region_commit(area, sum_row, sum_col, bbox, rbase + L - 1, a, sr, sc, r0, c0, r1, c1);
            todo &= ~__ballot(m);
        }
    }
}

// ---- binary dilation / erosion ---------------------------------------------------------------------------------------------------
// Bit dy * size + dx of `fp` is footprint[dy][dx]. Erosion reads src[y + dy - r][x + dx - r], dilation the mirrored
// src[y - (dy - r)][x - (dx - r)] (scipy.ndimage's conventions); pixels outside the image read `border`.
template <bool ERODE>
__global__ __launch_bounds__(256) void binary_morph_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int h, int w,
                                                           unsigned long long fp, int size, int border, size_t total) {
    const int r = size / 2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int x = (int)(i % w);
        const size_t t = i / w;
        const int y = (int)(t % h);
        const uint8_t *img = src + (t / h) * (size_t)h * w;
        bool res = ERODE;
        for (int dy = 0; dy < size && res == ERODE; ++dy) {
            const int yy = ERODE ? y + dy - r : y - (dy - r);
            for (int dx = 0; dx < size; ++dx) {
                if (!(fp >> (dy * size + dx) & 1ull)) continue;
                const int xx = ERODE ? x + dx - r : x - (dx - r);
                const bool v = (yy < 0 || yy >= h || xx < 0 || xx >= w) ? border != 0 : img[(size_t)yy * w + xx] != 0;
                if (v != ERODE) {
                    res = !ERODE;
                    break;
                }
            }
        }
        dst[i] = res;
    }
}

// out = level <= img (utils.py:242), as 0 / 1
__global__ __launch_bounds__(256) void mask_ge_kernel(const uint8_t *__restrict__ img, uint8_t *__restrict__ out, size_t count,
                                                      int level) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) out[i] = (int)img[i] >= level;
}

// ---- mean over the query points of an image of the head means of their attention rows (analyse_attention.py:196-211) ------------
// One workgroup per image. Per pixel: for each selected row the head mean exactly as tile_post_kernel<false> computes it
// (sequential fp32 sum, / H), the maps added in selection order and divided by their number — np.mean(list, axis=0) of float32
// maps. No selection, a selection outside sel[0 .. n_sel) or a row index outside [0, R): NaN.
__global__ __launch_bounds__(256) void query_mean_kernel(const float *__restrict__ rows, const int *__restrict__ sel,
                                                         const int *__restrict__ offsets, float *__restrict__ maps, int H, int R,
                                                         int P, int n_sel) {
    const int t = blockIdx.x;
    const int q0 = offsets[t], q1 = offsets[t + 1];
    bool ok = q0 >= 0 && q1 > q0 && q1 <= n_sel;
    if (ok)
        for (int j = q0; j < q1; ++j) ok = ok && sel[j] >= 0 && sel[j] < R;
    const float *src = rows + (size_t)t * H * R * P;
    float *dst = maps + (size_t)t * P;
    const float nan = __int_as_float(0x7FC00000);
    for (int i = threadIdx.x; i < P; i += 256) {
        if (!ok) {
            dst[i] = nan;
            continue;
        }
        float acc = 0.f;
        for (int j = q0; j < q1; ++j) {
            const float *row = src + (size_t)sel[j] * P + i;
            float s = row[0];
            for (int hh = 1; hh < H; ++hh) s = s + row[(size_t)hh * R * P];
            s = s / (float)H;
            acc = j == q0 ? s : acc + s;
        }
        dst[i] = acc / (float)(q1 - q0);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
constexpr int MAX_SIDE = 32768;
constexpr int64_t MAX_PIXELS = (int64_t)1 << 30;  // int32 pixel indices with room for the neighbour offsets

int check_images(const char *what, int32_t batch, int32_t h, int32_t w) {
    if (batch < 1 || batch > 65535) return fail(OCM_EINVAL, "%s: batch = %d (1..65535)", what, batch);
    if (h < 1 || w < 1 || h > MAX_SIDE || w > MAX_SIDE || (int64_t)h * w > MAX_PIXELS)
        return fail(OCM_EINVAL, "%s: image %d x %d (sides 1..%d, at most 2^30 pixels)", what, h, w, MAX_SIDE);
    return OCM_OK;
}

int nchunks(int32_t h, int32_t w) { return (int)(((int64_t)h * w + CHUNK - 1) / CHUNK); }
size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

unsigned grid_for(size_t items, unsigned cap) {
    const size_t b = (items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// mask -> parent (roots not yet flattened): the tile pass and the border pass
hipError_t launch_components(const uint8_t *mask, int *parent, int batch, int h, int w, hipStream_t s) {
    const int tx = (w + LT - 1) / LT, ty = (h + LT - 1) / LT;
    label_tile_kernel<<<dim3(tx, ty, batch), dim3(256), 0, s>>>(mask, parent, h, w);
    const int n_top = (ty - 1) * w, n_left = (tx - 1) * h;
    if (n_top + n_left > 0)
        label_merge_kernel<<<dim3(grid_for((size_t)n_top + n_left, 4096), batch), dim3(256), 0, s>>>(parent, h, w, n_top, n_left);
    return hipGetLastError();
}

}  // namespace

extern "C" int32_t ocm_label8_tile(void) { return LT; }

extern "C" size_t ocm_label8_workspace_bytes(int32_t batch, int32_t h, int32_t w) {
    if (batch < 1 || h < 1 || w < 1 || h > MAX_SIDE || w > MAX_SIDE || (int64_t)h * w > MAX_PIXELS) return 0;
    return align256((size_t)batch * h * w * sizeof(int)) + align256((size_t)batch * nchunks(h, w) * sizeof(int));
}

extern "C" int ocm_op_label8(const uint8_t *mask, int32_t *labels, int32_t *counts, int32_t batch, int32_t h, int32_t w,
                             void *workspace, size_t workspace_bytes, void *stream) {
    if (!mask || !labels || !counts) return fail(OCM_EINVAL, "null argument");
    if (int rc = check_images("label8", batch, h, w)) return rc;
    const size_t need = ocm_label8_workspace_bytes(batch, h, w);
    if (!workspace || workspace_bytes < need)
        return fail(OCM_ENOMEM, "label8 workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    const hipStream_t s = (hipStream_t)stream;
    const int n = h * w, nc = nchunks(h, w);
    int *rank = (int *)workspace;
    int *chunk = (int *)((char *)workspace + align256((size_t)batch * n * sizeof(int)));
    HIP_TRY(launch_components(mask, labels, batch, h, w, s));
    label_flatten_kernel<<<dim3(nc, batch), dim3(256), 0, s>>>(labels, n, chunk);
    label_scan_kernel<<<dim3(batch), dim3(256), 0, s>>>(chunk, nc, counts);
    label_rank_kernel<<<dim3(nc, batch), dim3(256), 0, s>>>(labels, n, chunk, rank);
    label_relabel_kernel<<<dim3(nc, batch), dim3(256), 0, s>>>(labels, n, rank);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" size_t ocm_remove_small_objects_workspace_bytes(int32_t batch, int32_t h, int32_t w) {
    if (batch < 1 || h < 1 || w < 1 || h > MAX_SIDE || w > MAX_SIDE || (int64_t)h * w > MAX_PIXELS) return 0;
    return 2 * align256((size_t)batch * h * w * sizeof(int));
}

extern "C" int ocm_op_remove_small_objects(const uint8_t *mask, uint8_t *out, int32_t batch, int32_t h, int32_t w,
                                           int32_t min_size, void *workspace, size_t workspace_bytes, void *stream) {
    if (!mask || !out) return fail(OCM_EINVAL, "null argument");
    if (int rc = check_images("remove_small_objects", batch, h, w)) return rc;
    if (min_size < 0) return fail(OCM_EINVAL, "remove_small_objects: min_size = %d < 0", min_size);
    const size_t need = ocm_remove_small_objects_workspace_bytes(batch, h, w);
    if (!workspace || workspace_bytes < need)
        return fail(OCM_ENOMEM, "remove_small_objects workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    const hipStream_t s = (hipStream_t)stream;
    const int n = h * w;
    const size_t plane = align256((size_t)batch * n * sizeof(int));
    int *parent = (int *)workspace, *area = (int *)((char *)workspace + plane);
    HIP_TRY(hipMemsetAsync(area, 0, (size_t)batch * n * sizeof(int), s));
    HIP_TRY(launch_components(mask, parent, batch, h, w, s));
    const unsigned gx = grid_for((size_t)n, 2048);
    label_area_kernel<<<dim3(gx, batch), dim3(256), 0, s>>>(parent, n, area);
    keep_large_kernel<<<dim3(gx, batch), dim3(256), 0, s>>>(parent, area, out, n, min_size);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_region_stats(const int32_t *labels, int32_t batch, int32_t h, int32_t w, int32_t max_regions,
                                   int64_t *area, int64_t *sum_row, int64_t *sum_col, int32_t *bbox, void *stream) {
    if (!labels || !area || !sum_row || !sum_col || !bbox) return fail(OCM_EINVAL, "null argument");
    if (int rc = check_images("region_stats", batch, h, w)) return rc;
    if (max_regions < 1) return fail(OCM_EINVAL, "region_stats: max_regions = %d < 1", max_regions);
    const size_t regions = (size_t)batch * max_regions;
    const hipStream_t s = (hipStream_t)stream;
    region_init_kernel<<<dim3(grid_for(regions, 1024)), dim3(256), 0, s>>>((long long *)area, (long long *)sum_row,
                                                                           (long long *)sum_col, bbox, regions, h, w);
    const size_t nseg = (size_t)h * ((w + SEG - 1) / SEG);
    region_stats_kernel<<<dim3(grid_for(nseg, 2048), batch), dim3(256), 0, s>>>(labels, h, w, max_regions, (long long *)area,
                                                                                  (long long *)sum_row, (long long *)sum_col, bbox);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_binary_morph(const uint8_t *src, uint8_t *dst, int32_t batch, int32_t h, int32_t w, uint64_t footprint_bits,
                                   int32_t size, int32_t op, int32_t border_value, void *stream) {
    if (!src || !dst || src == dst) return fail(OCM_EINVAL, "null or aliased argument");
    if (int rc = check_images("binary_morph", batch, h, w)) return rc;
    if (size < 1 || size > 7 || !(size & 1)) return fail(OCM_EINVAL, "binary_morph: footprint size %d (odd, 1..7)", size);
    if (size * size < 64 && (footprint_bits >> (size * size))) return fail(OCM_EINVAL, "binary_morph: footprint bits beyond size^2");
    if (!footprint_bits) return fail(OCM_EINVAL, "binary_morph: empty footprint");
    if (op != 0 && op != 1) return fail(OCM_EINVAL, "binary_morph: op = %d (0 dilation, 1 erosion)", op);
    if (border_value != 0 && border_value != 1) return fail(OCM_EINVAL, "binary_morph: border_value = %d (0 or 1)", border_value);
    const hipStream_t s = (hipStream_t)stream;
    const size_t total = (size_t)batch * h * w;
    const dim3 grid(grid_for(total, 8192)), block(256);
    if (op)
        binary_morph_kernel<true><<<grid, block, 0, s>>>(src, dst, h, w, footprint_bits, size, border_value, total);
    else
        binary_morph_kernel<false><<<grid, block, 0, s>>>(src, dst, h, w, footprint_bits, size, border_value, total);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_mask_ge_u8(const uint8_t *img, uint8_t *out, int64_t count, int32_t level, void *stream) {
    if (!img || !out) return fail(OCM_EINVAL, "null argument");
    if (count <= 0) return fail(OCM_EINVAL, "bad count");
    mask_ge_kernel<<<dim3(grid_for((size_t)count, 4096)), dim3(256), 0, (hipStream_t)stream>>>(img, out, (size_t)count, level);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_query_mean(const float *rows, const int32_t *sel, const int32_t *offsets, float *maps, int32_t tiles,
                                 int32_t heads, int32_t n_rows, int32_t pixels, int32_t n_sel, void *stream) {
    if (!rows || !offsets || !maps || (n_sel > 0 && !sel)) return fail(OCM_EINVAL, "null argument");
    if (tiles <= 0 || heads <= 0 || n_rows <= 0 || pixels <= 0 || n_sel < 0) return fail(OCM_EINVAL, "bad shape");
    query_mean_kernel<<<dim3(tiles), dim3(256), 0, (hipStream_t)stream>>>(rows, sel, offsets, maps, heads, n_rows, pixels, n_sel);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}
