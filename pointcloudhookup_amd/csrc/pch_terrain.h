// Terrain grid: what the kernels of pch_terrain.hip share with every other sweep that needs the ground
// under a position (pch_treefall.hip) - the row frame, the cell rule and g(X, Y), the one __device__ function that
// serves them all -, and the host's checks of a grid.  The rule is spelled out in include/pch_hip.h.
#pragma once
#include "pch_common.h"

#include <math.h>

namespace pch {

constexpr uint32_t TL_NAN = 0x7FC00000u;                    // the NaN every output carries

struct TlRow { float x, y, z; };
struct TlGrid { double x0, y0, cell; int nx, ny; };
struct TlSub { float x, y, z; int on; };

#ifdef __HIPCC__
__device__ __forceinline__ float tl_nan() { return __uint_as_float(TL_NAN); }

// P = fl32(xyz - sub3) per component; no subtraction without sub3
__device__ __forceinline__ TlRow tl_frame(TlRow q, const TlSub& s) {
    if (s.on) { q.x = q.x - s.x; q.y = q.y - s.y; q.z = q.z - s.z; }
    return q;
}

// the cell rule: false outside the grid (NaN and inf fail the comparisons)
__device__ __forceinline__ bool tl_cell(const TlGrid& g, double X, double Y, int& fx, int& fy) {
    const double qx = floor((X - g.x0) / g.cell), qy = floor((Y - g.y0) / g.cell);
    if (!(qx >= 0.0 && qx < (double)g.nx && qy >= 0.0 && qy < (double)g.ny)) return false;
    fx = (int)qx;
    fy = (int)qy;
    return true;
}

// g(X, Y) of the rule: the bilinear value between the four cell centres around the position, the position's own cell
// where one of the four has no ground, NaN outside the grid
__device__ __forceinline__ void tl_axis(double pos, double o, double cell, int nc, int& i0, int& i1, double& a) {
    const double u = ((pos - o) / cell) - 0.5;
    const int top = nc - 2 > 0 ? nc - 2 : 0;
    int f = (int)floor(u);
    f = f < 0 ? 0 : f;
    i0 = f > top ? top : f;
    i1 = i0 + 1 < nc - 1 ? i0 + 1 : nc - 1;
    a = u - (double)i0;
    if (a < 0.0) a = 0.0;
    if (a > 1.0) a = 1.0;
}
__device__ __forceinline__ double tl_ground_at(const TlGrid& g, const float* __restrict__ ground, double X, double Y) {
    int fx = 0, fy = 0;
    if (!tl_cell(g, X, Y, fx, fy)) return (double)tl_nan();
    int i0, i1, j0, j1;
    double a, b;
    tl_axis(X, g.x0, g.cell, g.nx, i0, i1, a);          // (inside the grid u lies in [-0.5, nc): the cast is safe)
    tl_axis(Y, g.y0, g.cell, g.ny, j0, j1, b);
    const double g00 = (double)ground[(size_t)j0 * g.nx + i0], g10 = (double)ground[(size_t)j0 * g.nx + i1];
    const double g01 = (double)ground[(size_t)j1 * g.nx + i0], g11 = (double)ground[(size_t)j1 * g.nx + i1];
    const double own = (double)ground[(size_t)fy * g.nx + fx];
    if (g00 != g00 || g10 != g10 || g01 != g01 || g11 != g11) return own;
    return (((g00 * (1.0 - a)) + (g10 * a)) * (1.0 - b)) + (((g01 * (1.0 - a)) + (g11 * a)) * b);
}
#endif  // __HIPCC__

static bool tl_cells_ok(int64_t ncells) { return ncells >= 1 && ncells <= PCH_TERRAIN_MAX_CELLS; }
static bool tl_rows_ok(int64_t n) { return n >= 0 && n < (int64_t(1) << 31); }
// the grid as the kernels take it; false for a grid outside the rule's limits
static bool tl_grid_of(const PchTerrainGrid* gh, TlGrid& g) {
    if (!gh || !(gh->cell > 0.0) || !isfinite(gh->cell) || gh->nx < 1 || gh->ny < 1) return false;
    if (!tl_cells_ok((int64_t)gh->nx * (int64_t)gh->ny)) return false;
    g.x0 = gh->x0; g.y0 = gh->y0; g.cell = gh->cell; g.nx = gh->nx; g.ny = gh->ny;
    return true;
}
static TlSub tl_sub_of(const float* sub3_host) {
    TlSub s = {0.0f, 0.0f, 0.0f, 0};
    if (sub3_host) { s.x = sub3_host[0]; s.y = sub3_host[1]; s.z = sub3_host[2]; s.on = 1; }
    return s;
}

}  // namespace pch
