// swin_geom.h — the (shifted-)window geometry of Swin, shared by the forward (kernels_swin.hip) and the backward
// (kernels_swin_train.hip): which token a window position is, which mask region it lies in, which relative-position bin a
// (query, key) pair reads.
#pragma once
#include <hip/hip_runtime.h>

struct WinGeom {
    int H, W, ws, shift, nWx, nW, heads;
};
// token (row of the (B, H*W, C) stream) of position p of window (b, wy, wx): the window tiles the image rolled
// by -shift (cyclic_shift :617-626 + window_partition :486-495), so its source pixel is (+shift) mod size; the
// output goes back to the same token (window_reverse + reverse roll).
// (`ws` is passed separately: a compile-time 7 in the Swin-T instantiation turns the divisions into multiplies)
__device__ __forceinline__ size_t win_token(const WinGeom &g, int ws, int b, int wy, int wx, int p) {
    const int py = p / ws, px = p - py * ws;
    int y = wy * ws + py + g.shift, x = wx * ws + px + g.shift;
    if (y >= g.H) y -= g.H;
    if (x >= g.W) x -= g.W;
    return ((size_t)b * g.H + y) * g.W + x;
}
// region id of get_attn_mask (:584-607) for position p of the window, in the SHIFTED frame
__device__ __forceinline__ int win_region(const WinGeom &g, int ws, int wy, int wx, int p) {
    const int py = p / ws, px = p - py * ws;
    const int ys = wy * ws + py, xs = wx * ws + px;
    const int ry = (ys >= g.H - ws) + (ys >= g.H - g.shift), rx = (xs >= g.W - ws) + (xs >= g.W - g.shift);
    return ry * 3 + rx;
}
// work id = (b * nW + wy * nWx + wx) * per + head -> head, image, window row and column (per = 1: the id of a window)
struct WinId {
    int head, b, wy, wx;
};
__device__ __forceinline__ WinId win_decode(const WinGeom &g, int id, int per) {
    const int head = id % per, wlin = (id / per) % g.nW, b = id / (per * g.nW);
    const int wy = wlin / g.nWx;
    return WinId{head, b, wy, wlin - wy * g.nWx};
}
// true for the windows in which get_attn_mask separates regions: the last row and column of a shifted grid (wave-uniform)
__device__ __forceinline__ bool win_masked(const WinGeom &g, int ws, int wy, int wx) {
    return g.shift > 0 && (wy == g.H / ws - 1 || wx == g.nWx - 1);
}
// element of the (2 ws - 1)^2 x heads relative-position table (SwinRelativePositionBias :329-370) for query position i, key j
__device__ __forceinline__ int rel_bias_index(int ws, int heads, int i, int j, int head) {
    const int yi = i / ws, xi = i - yi * ws, yj = j / ws, xj = j - yj * ws;
    return ((yi - yj + ws - 1) * (2 * ws - 1) + (xi - xj + ws - 1)) * heads + head;
}
