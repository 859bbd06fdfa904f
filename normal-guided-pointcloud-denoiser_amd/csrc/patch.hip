// The GCN network input on the device: what the reference's PatchCollector.collectNetworkInput does per face
// (PatchGeneration/Modules/Mesh.py selectPaperPatch :300-307, createPatch :289-295, Patch.alignPatch :473-482,
// RotationMatrix.py:9-35, Patch.toGraph :497-506, Network/DataUtils.py file2input :41-70).
//   pcd_mesh_tta            igl.triangle_triangle_adjacency: a radix sort of the undirected edge keys
//   pcd_patch_radius        two-ring radius r = k sqrt(mean area) and the face centre, one thread per face
//   pcd_patch_select_*      faces with a vertex strictly inside the ball, as a CSR (count pass, fill pass)
//   pcd_patch_inputs        one workgroup per patch: centre, scale, the tensor T, its fp64 eigenvectors, the rotated
//                           patch's 64 x 20 rows
// Everything is fp64 with numpy's separate multiply / add roundings where a comparison decides membership.  All
// reductions are fixed LDS trees over per-thread partial sums taken in a fixed order: a run is bitwise repeatable.
// Every index read from a caller's array is checked against its range before it is used.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "pcd_knn.h"

namespace pcd {

static constexpr int kRows = 64;      // rows of the network input (file2input's num_neighbors)
static constexpr int kCols = 20;      // 17 feature columns + 3 index columns
static constexpr int kTileStride = 21;   // LDS row stride in doubles: 42 dwords, so a column walk spreads over the banks

// ---------------------------------------------------------------------------------------------- edge adjacency
// Corner c = 3 g + e stands for the edge (f[g][e], f[g][(e+1)%3]); its key is (min << 32 | max).  After the sort an
// edge's corners are adjacent: a run of exactly two gives each the other's face, anything else (boundary, an edge
// shared by more than two faces, an edge from a vertex to itself, the same face twice) gives -1.
template <class I>
__global__ __launch_bounds__(256) void k_tta_keys(const I* __restrict__ f, int64_t nc, int64_t nv,
                                                   unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals,
                                                   int* __restrict__ bad) {
    const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (c >= nc) return;
    const int64_t g = c / 3;
    const int e = (int)(c - 3 * g);
    int64_t a = (int64_t)f[c], b = (int64_t)f[3 * g + (e == 2 ? 0 : e + 1)];
    if (a < 0 || a >= nv || b < 0 || b >= nv) { atomicOr(bad, 1); a = b = 0; }
    const unsigned long long lo = (unsigned long long)(a < b ? a : b), hi = (unsigned long long)(a < b ? b : a);
    keys[c] = (lo << 32) | hi;
    vals[c] = (uint32_t)c;
}
template <class I>
__global__ __launch_bounds__(256) void k_tta_out(const unsigned long long* __restrict__ sk, const uint32_t* __restrict__ sv,
                                                  int64_t nc, I* __restrict__ tt) {
    const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (p >= nc) return;
    const unsigned long long key = sk[p];
    const bool pe = p > 0 && sk[p - 1] == key, ne = p + 1 < nc && sk[p + 1] == key;
    int64_t other = -1;
    if ((key >> 32) != (key & 0xffffffffull)) {
        if (pe && !ne && !(p > 1 && sk[p - 2] == key)) other = (int64_t)(sv[p - 1] / 3u);
        else if (ne && !pe && !(p + 2 < nc && sk[p + 2] == key)) other = (int64_t)(sv[p + 1] / 3u);
    }
    const uint32_t c = sv[p];
    if (other == (int64_t)(c / 3u)) other = -1;
    tt[c] = (I)other;
}

// ---------------------------------------------------------------------------------------------- small fp64 helpers
struct V3 { double x, y, z; };
__device__ __forceinline__ V3 sub3(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 mul3(V3 a, double s) { return V3{a.x * s, a.y * s, a.z * s}; }
// numpy.cross and numpy.linalg.norm(axis=-1): separate roundings, ((x² + y²) + z²)
__device__ __forceinline__ V3 cross3(V3 a, V3 b) {
    return V3{__dsub_rn(__dmul_rn(a.y, b.z), __dmul_rn(a.z, b.y)), __dsub_rn(__dmul_rn(a.z, b.x), __dmul_rn(a.x, b.z)),
              __dsub_rn(__dmul_rn(a.x, b.y), __dmul_rn(a.y, b.x))};
}
__device__ __forceinline__ double dot3(V3 a, V3 b) {
    return __dadd_rn(__dadd_rn(__dmul_rn(a.x, b.x), __dmul_rn(a.y, b.y)), __dmul_rn(a.z, b.z));
}
__device__ __forceinline__ double norm3(V3 a) { return sqrt(dot3(a, a)); }
__device__ __forceinline__ V3 load3(const double* __restrict__ v, int64_t i) { return V3{v[3 * i], v[3 * i + 1], v[3 * i + 2]}; }
__device__ __forceinline__ bool finite3(V3 a) {
    return fabs(a.x) < HUGE_VAL && fabs(a.y) < HUGE_VAL && fabs(a.z) < HUGE_VAL;   // (false for NaN too)
}
// the three corners of face g; false (nothing read) when a corner is outside [0, nv)
__device__ __forceinline__ bool corners(const double* __restrict__ v, int64_t nv, const int64_t* __restrict__ f, int64_t g,
                                        V3 (&p)[3]) {
    const int64_t a = f[3 * g], b = f[3 * g + 1], c = f[3 * g + 2];
    if (a < 0 || a >= nv || b < 0 || b >= nv || c < 0 || c >= nv) return false;
    p[0] = load3(v, a); p[1] = load3(v, b); p[2] = load3(v, c);
    return true;
}
// Mesh.getAreas: 0.5 |(p1 - p0) x (p2 - p0)|
__device__ __forceinline__ double area_of(const V3 (&p)[3]) { return 0.5 * norm3(cross3(sub3(p[1], p[0]), sub3(p[2], p[0]))); }
// Mesh.getFaceNormals: (p1 - p0) x (p2 - p1), normalised; the zero vector for a face of zero (or non-finite) area
__device__ __forceinline__ V3 normal_of(const V3 (&p)[3]) {
    const V3 c = cross3(sub3(p[1], p[0]), sub3(p[2], p[1]));
    const double len = norm3(c);
    if (!(len > 0.0 && len < HUGE_VAL)) return V3{0.0, 0.0, 0.0};
    return V3{c.x / len, c.y / len, c.z / len};
}
// igl.barycenter
__device__ __forceinline__ V3 centroid_of(const V3 (&p)[3]) {
    return V3{((p[0].x + p[1].x) + p[2].x) / 3.0, ((p[0].y + p[1].y) + p[2].y) / 3.0, ((p[0].z + p[1].z) + p[2].z) / 3.0};
}

// ---------------------------------------------------------------------------------------------- radius and centre
// Mesh.selectPaperPatch :301-304.  The two-ring {fi} ∪ N(fi) ∪ N(N(fi)) has at most 1 + 3 + 9 members before the
// duplicates go; absent neighbours (-1) are skipped.  The areas are summed as numpy.sum does over the ascending ring:
// in order below eight terms, else eight accumulators folded as a tree and the rest added in order.
__global__ __launch_bounds__(256) void k_patch_radius(const double* __restrict__ v, int64_t nv, const int64_t* __restrict__ f,
                                                       int64_t nf, const int64_t* __restrict__ tt,
                                                       const int64_t* __restrict__ faces, int64_t n, double k,
                                                       double* __restrict__ centre, double* __restrict__ radius,
                                                       double* __restrict__ mean_area) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t fi = faces[i];
    V3 p[3];
    if (fi < 0 || fi >= nf || !corners(v, nv, f, fi, p)) {
        centre[3 * i] = centre[3 * i + 1] = centre[3 * i + 2] = 0.0;
        radius[i] = 0.0;
        if (mean_area) mean_area[i] = 0.0;
        return;
    }
    int64_t ring[13];
    int cnt = 1;
    ring[0] = fi;
    for (int round = 0; round < 2; ++round) {
        const int have = cnt;
        for (int a = 0; a < have; ++a) {
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const int64_t g = tt[3 * ring[a] + e];
                if (g < 0 || g >= nf) continue;
                bool seen = false;
                for (int b = 0; b < cnt; ++b) seen |= (ring[b] == g);
                if (!seen && cnt < 13) ring[cnt++] = g;
            }
        }
    }
    for (int a = 1; a < cnt; ++a) {          // ascending, as numpy.union1d leaves it
        const int64_t x = ring[a];
        int b = a - 1;
        while (b >= 0 && ring[b] > x) { ring[b + 1] = ring[b]; --b; }
        ring[b + 1] = x;
    }
    double ar[13];
    for (int a = 0; a < cnt; ++a) {
        V3 q[3];
        ar[a] = corners(v, nv, f, ring[a], q) ? area_of(q) : 0.0;
    }
    double sum;
    if (cnt < 8) {
        sum = ar[0];
        for (int a = 1; a < cnt; ++a) sum = __dadd_rn(sum, ar[a]);
    } else {
        sum = __dadd_rn(__dadd_rn(__dadd_rn(ar[0], ar[1]), __dadd_rn(ar[2], ar[3])),
                        __dadd_rn(__dadd_rn(ar[4], ar[5]), __dadd_rn(ar[6], ar[7])));
        for (int a = 8; a < cnt; ++a) sum = __dadd_rn(sum, ar[a]);
    }
    const double mean = sum / (double)cnt;
    radius[i] = k * sqrt(mean);
    if (mean_area) mean_area[i] = mean;
    const V3 c = centroid_of(p);
    centre[3 * i] = c.x; centre[3 * i + 1] = c.y; centre[3 * i + 2] = c.z;
}

// ---------------------------------------------------------------------------------------------- selection
// Mesh.getFacesInRange :157-163: |v - centre| < r, strict, as numpy rounds it.
__device__ __forceinline__ bool in_ball(const double* __restrict__ v, int64_t u, V3 c, double r) {
    return norm3(sub3(load3(v, u), c)) < r;
}
struct SelectArgs {
    GridView g;               // the grid over the fp32 vertices (rows carry the vertex index in .w)
    double widen;             // added to every radius for the cell box: the fp32 rounding of vertices and centres
    const double* v; int64_t nv;
    const int64_t* f; int64_t nf;
    const int64_t* vf; const int64_t* ni;
    const double* centre; const double* radius;
    int64_t n;
};
// The patch of query p is every face with a corner inside the ball.  The candidates are the grid rows of the cells
// that overlap the widened box around the centre: a duplicate-free superset of the vertices inside, each then put to
// the exact fp64 test on the caller's vertices.  A face is taken at the vertex that is its first corner inside the
// ball, so once.  The block's threads share the cells of the box; visit(g) is called for every face of the patch, in
// no particular order.
template <int BS, class Visit>
__device__ __forceinline__ void select_walk(const SelectArgs& a, int64_t p, Visit visit) {
    const V3 c = load3(a.centre, p);
    const double r = a.radius[p];
    if (!(r > 0.0)) return;                           // (NaN too) the strict test holds for no vertex
    const GridView& g = a.g;
    const float qx = (float)c.x, qy = (float)c.y, qz = (float)c.z;
    const float rf = (float)((r + a.widen) * (1.0 + 1e-6)) + g.slack + 1e-30f;
    const int lo[3] = {max(cell_coord(qx - rf, g.ox, g.inv_h), 0), max(cell_coord(qy - rf, g.oy, g.inv_h), 0),
                       max(cell_coord(qz - rf, g.oz, g.inv_h), 0)};
    const int hi[3] = {min(cell_coord(qx + rf, g.ox, g.inv_h), g.dx - 1), min(cell_coord(qy + rf, g.oy, g.inv_h), g.dy - 1),
                       min(cell_coord(qz + rf, g.oz, g.inv_h), g.dz - 1)};
    if (hi[0] < lo[0] || hi[1] < lo[1] || hi[2] < lo[2]) return;
    const int64_t nx = hi[0] - lo[0] + 1, ny = hi[1] - lo[1] + 1, nz = hi[2] - lo[2] + 1;
    for (int64_t cell = threadIdx.x; cell < nx * ny * nz; cell += BS) {
        const int cx = lo[0] + (int)(cell % nx), cy = lo[1] + (int)((cell / nx) % ny), cz = lo[2] + (int)(cell / (nx * ny));
        uint32_t rs, re;
        if (!cell_range(g, cx, cy, cz, rs, re)) continue;
        for (uint32_t row = rs; row < re && (int64_t)row < g.n; ++row) {
            const int64_t u = (int64_t)__float_as_uint(g.pts[row].w);
            if (u >= a.nv || !in_ball(a.v, u, c, r)) continue;
            int64_t s0 = a.ni[u], s1 = a.ni[u + 1];
            if (s0 < 0) s0 = 0;
            if (s1 > 3 * a.nf) s1 = 3 * a.nf;
            for (int64_t s = s0; s < s1; ++s) {
                const int64_t gf = a.vf[s];
                if (gf < 0 || gf >= a.nf || (s > s0 && a.vf[s - 1] == gf)) continue;
                int64_t first = -1;
                for (int k = 0; k < 3 && first < 0; ++k) {
                    const int64_t w = a.f[3 * gf + k];
                    if (w >= 0 && w < a.nv && (w == u || in_ball(a.v, w, c, r))) first = w;
                }
                if (first == u) visit(gf);
            }
        }
    }
}
template <int BS>
__global__ __launch_bounds__(BS) void k_select_count(SelectArgs a, int64_t* __restrict__ counts) {
    __shared__ int sc[BS];
    const int64_t p = blockIdx.x;
    int cnt = 0;
    select_walk<BS>(a, p, [&](int64_t) { ++cnt; });
    sc[threadIdx.x] = cnt;
    __syncthreads();
    for (int w = BS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sc[threadIdx.x] += sc[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[p] = sc[0];
}
// Fill: the faces go into the row's segment of tmp in arrival order, then each takes its rank (they are distinct) as
// its slot in out.  Nothing is written unless the whole CSR fits `capacity` and the row fits its segment; a row whose
// length differs from its segment sets *status and leaves out alone.
template <int BS>
__global__ __launch_bounds__(BS) void k_select_fill(SelectArgs a, const int64_t* __restrict__ off, int64_t capacity,
                                                     int64_t* __restrict__ tmp, int64_t* __restrict__ out,
                                                     int* __restrict__ status) {
    __shared__ int fill;
    const int64_t p = blockIdx.x;
    const int64_t base = off[p], end = off[p + 1];
    if (off[a.n] > capacity || base < 0 || end < base || end > capacity || end - base > 0x7fffffff) {
        if (threadIdx.x == 0) atomicOr(status, 1);
        return;
    }
    const int cap = (int)(end - base);
    if (threadIdx.x == 0) fill = 0;
    __syncthreads();
    select_walk<BS>(a, p, [&](int64_t g) {
        const int at = atomicAdd(&fill, 1);
        if (at < cap) tmp[base + at] = g;
    });
    __threadfence_block();
    __syncthreads();
    const int cnt = fill;
    if (cnt != cap) {
        if (threadIdx.x == 0) atomicOr(status, 2);
        return;
    }
    for (int x = threadIdx.x; x < cnt; x += BS) {
        const int64_t g = tmp[base + x];
        int rank = 0;
        for (int y = 0; y < cnt; ++y) rank += (tmp[base + y] < g);
        out[base + rank] = g;
    }
}

// ---------------------------------------------------------------------------------------------- patch inputs
// local index of face g in the ascending row, or -1
__device__ __forceinline__ int64_t find_in_row(const int64_t* __restrict__ row, int64_t m, int64_t g) {
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (row[mid] < g) lo = mid + 1; else hi = mid;
    }
    return (lo < m && row[lo] == g) ? lo : -1;
}
// fixed-tree block reductions; every thread gets the result, and the scratch is free again on return
template <int BS>
__device__ __forceinline__ double block_sum(double x, double* s) {
    s[threadIdx.x] = x;
    __syncthreads();
    for (int w = BS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}
template <int BS>
__device__ __forceinline__ double block_max(double x, double* s) {
    s[threadIdx.x] = x;
    __syncthreads();
    for (int w = BS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] = fmax(s[threadIdx.x], s[threadIdx.x + w]);
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}
// Cyclic Jacobi on a symmetric 3x3 in fp64: a is destroyed, w gets the eigenvalues, the columns of V the eigenvectors.
// A bounded number of sweeps; NaN input leaves the loop at once.
__device__ void jacobi3(double (&a)[3][3], double (&w)[3], double (&V)[3][3]) {
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 24; ++sweep) {
        const double offd = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
        const double diag = fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]);
        if (!(offd > diag * 0x1p-80)) break;             // converged, zero, or NaN
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2, r = 3 - p - q;
            const double apq = a[p][q];
            if (apq == 0.0) continue;
            const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
            const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            a[p][p] -= t * apq;
            a[q][q] += t * apq;
            a[p][q] = a[q][p] = 0.0;
            const double arp = a[r][p], arq = a[r][q];
            a[r][p] = a[p][r] = c * arp - s * arq;
            a[r][q] = a[q][r] = s * arp + c * arq;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double vp = V[k][p], vq = V[k][q];
                V[k][p] = c * vp - s * vq;
                V[k][q] = s * vp + c * vq;
            }
        }
    }
    w[0] = a[0][0]; w[1] = a[1][1]; w[2] = a[2][2];
}

struct InputArgs {
    const double* v; int64_t nv;
    const int64_t* f; int64_t nf;
    const int64_t* tt; const int64_t* vf; const int64_t* ni;
    const int64_t* faces; int64_t n;
    const int64_t* off; const int64_t* rows; int64_t total;
    int adjacency;            // 0: the reference's index columns, 1: the local edge-neighbours
    int channels_first;       // 0: [n][64][20], 1: [n][20][64]
    double* rot; int64_t* centre_index; double* eig;
};

// One workgroup per patch.  The row (the patch's parent faces, ascending) is walked in strides of the block and
// re-read from global memory by every pass (it is a few hundred bytes and stays in cache); only the 64 x 20 output
// tile lives in LDS, so the rows leave as whole contiguous runs whatever the layout.
template <class OutT, int BS>
__global__ __launch_bounds__(BS) void k_patch_inputs(InputArgs a, OutT* __restrict__ out) {
    __shared__ double red[BS];
    __shared__ double tile[kRows * kTileStride];
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t fi = a.faces[p];
    int64_t base = a.off[p], m = a.off[p + 1] - base;
    if (base < 0 || m < 0 || base + m > a.total || fi < 0 || fi >= a.nf) { base = 0; m = 0; }
    const int64_t* __restrict__ row = a.rows + base;
    const int64_t pi = find_in_row(row, m, fi);
    const int64_t pe = pi >= 0 ? pi : m - 1;          // (the reference indexes with -1: the last face)

    double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    double ev[3] = {0, 0, 0};
    V3 mean{0, 0, 0};
    double scale = 1.0;
    bool keep_centre = false;
    if (m > 0) {                                      // (uniform over the block)
        // --- the mean of the patch's vertices: a corner counts when its face is the first one of the vertex's
        //     incident faces (ascending) that lies in the patch
        double sx = 0, sy = 0, sz = 0, sn = 0;
        for (int64_t j = tid; j < m; j += BS) {
            const int64_t g = row[j];
            if (g < 0 || g >= a.nf) continue;
            for (int c = 0; c < 3; ++c) {
                const int64_t u = a.f[3 * g + c];
                if (u < 0 || u >= a.nv) continue;
                bool dup = false;
                for (int c2 = 0; c2 < c; ++c2) dup |= (a.f[3 * g + c2] == u);
                if (dup) continue;
                int64_t s0 = a.ni[u], s1 = a.ni[u + 1];
                if (s0 < 0) s0 = 0;
                if (s1 > 3 * a.nf) s1 = 3 * a.nf;
                bool mine = true;                     // (a vertex whose adjacency row lacks g counts here)
                for (int64_t s = s0; s < s1; ++s) {
                    const int64_t h = a.vf[s];
                    if (h == g) break;
                    if (h >= 0 && h < g && find_in_row(row, m, h) >= 0) { mine = false; break; }
                }
                if (!mine) continue;
                sx += a.v[3 * u]; sy += a.v[3 * u + 1]; sz += a.v[3 * u + 2]; sn += 1.0;
            }
        }
        sx = block_sum<BS>(sx, red); sy = block_sum<BS>(sy, red); sz = block_sum<BS>(sz, red);
        sn = block_sum<BS>(sn, red);
        if (sn > 0.0) mean = V3{sx / sn, sy / sn, sz / sn};
        // Patch.alignPatch :474-479: no translation when the centre is (numerically) the origin, no scaling when the
        // size is (numerically) one -- numpy.allclose's 1e-8 + 1e-5 |b|.  An untranslated patch is still measured,
        // resized and rotated about its true centre (Mesh.getPCSize, resize, rotate), which it then keeps.
        keep_centre = norm3(mean) <= 1e-8;
        // --- the farthest vertex
        double d2 = 0.0;
        for (int64_t j = tid; j < m; j += BS) {
            const int64_t g = row[j];
            V3 q[3];
            if (g < 0 || g >= a.nf || !corners(a.v, a.nv, a.f, g, q)) continue;
            for (int c = 0; c < 3; ++c) { const V3 d = sub3(q[c], mean); d2 = fmax(d2, dot3(d, d)); }
        }
        const double size = sqrt(block_max<BS>(d2, red));
        if (size > 0.0 && size < HUGE_VAL && !(fabs(size - 1.0) <= 1e-8 + 1e-5)) scale = 1.0 / size;
        // --- the centre face
        V3 q[3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        const int64_t gc = row[pe];
        if (gc >= 0 && gc < a.nf) (void)corners(a.v, a.nv, a.f, gc, q);
        for (int c = 0; c < 3; ++c) q[c] = mul3(sub3(q[c], mean), scale);
        const V3 ci = centroid_of(q), ni_ = normal_of(q);
        // --- T = sum_{j != pi} (A_j / max A) exp(-|c_j - c_i| / sigma) n'_j n'_j^T, sigma = 1/3  (RotationMatrix.py)
        double t00 = 0, t01 = 0, t02 = 0, t11 = 0, t12 = 0, t22 = 0, amax = 0;
        const double sigma = 1. / 3.;
        for (int64_t j = tid; j < m; j += BS) {
            if (j == pe) continue;
            const int64_t g = row[j];
            V3 b[3];
            if (g < 0 || g >= a.nf || !corners(a.v, a.nv, a.f, g, b)) continue;
            if (!(area_of(b) > 0.0)) continue;        // a zero-area face of the mesh adds nothing
            for (int c = 0; c < 3; ++c) b[c] = mul3(sub3(b[c], mean), scale);
            const V3 nj = normal_of(b);
            const double ar = area_of(b);
            const V3 d = sub3(centroid_of(b), ci);
            const V3 raw = cross3(cross3(d, nj), d);
            const double rl = norm3(raw);
            V3 w{raw.x / rl, raw.y / rl, raw.z / rl};
            if (!finite3(w)) w = V3{0, 0, 0};         // numpy.nan_to_num of 0/0
            const double tw = 2.0 * dot3(nj, w);
            const V3 np_{tw * w.x - nj.x, tw * w.y - nj.y, tw * w.z - nj.z};
            const double mu = ar * exp(-norm3(d) / sigma);
            if (!(mu == mu) || !finite3(np_)) continue;
            amax = fmax(amax, ar);
            t00 += mu * (np_.x * np_.x); t01 += mu * (np_.x * np_.y); t02 += mu * (np_.x * np_.z);
            t11 += mu * (np_.y * np_.y); t12 += mu * (np_.y * np_.z); t22 += mu * (np_.z * np_.z);
        }
        t00 = block_sum<BS>(t00, red); t01 = block_sum<BS>(t01, red); t02 = block_sum<BS>(t02, red);
        t11 = block_sum<BS>(t11, red); t12 = block_sum<BS>(t12, red); t22 = block_sum<BS>(t22, red);
        amax = block_max<BS>(amax, red);
        const double inv = amax > 0.0 ? 1.0 / amax : 0.0;
        double T[3][3] = {{t00 * inv, t01 * inv, t02 * inv}, {t01 * inv, t11 * inv, t12 * inv}, {t02 * inv, t12 * inv, t22 * inv}};
        double w[3], V[3][3];
        jacobi3(T, w, V);                             // (every thread: the same registers, no broadcast)
        int o0 = 0, o1 = 1, o2 = 2;                   // descending eigenvalues, ties in index order
        if (w[o1] > w[o0]) { const int t = o0; o0 = o1; o1 = t; }
        if (w[o2] > w[o1]) { const int t = o1; o1 = o2; o2 = t; }
        if (w[o1] > w[o0]) { const int t = o0; o0 = o1; o1 = t; }
        ev[0] = w[o0]; ev[1] = w[o1]; ev[2] = w[o2];
        for (int k = 0; k < 3; ++k) { R[0][k] = V[k][o0]; R[1][k] = V[k][o1]; }
        if (R[0][0] * ni_.x + R[0][1] * ni_.y + R[0][2] * ni_.z < 0.0)
            for (int k = 0; k < 3; ++k) R[0][k] = -R[0][k];
        int big = 0;                                   // canonical middle axis: its largest component is positive
        if (fabs(R[1][1]) > fabs(R[1][big])) big = 1;
        if (fabs(R[1][2]) > fabs(R[1][big])) big = 2;
        if (R[1][big] < 0.0) for (int k = 0; k < 3; ++k) R[1][k] = -R[1][k];
        R[2][0] = R[0][1] * R[1][2] - R[0][2] * R[1][1];
        R[2][1] = R[0][2] * R[1][0] - R[0][0] * R[1][2];
        R[2][2] = R[0][0] * R[1][1] - R[0][1] * R[1][0];
    }
    if (tid == 0) {
        for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) a.rot[9 * p + 3 * i + k] = R[i][k];
        a.centre_index[p] = pi;
        a.eig[3 * p] = ev[0]; a.eig[3 * p + 1] = ev[1]; a.eig[3 * p + 2] = ev[2];
    }
    // --- the rows: Patch.toGraph on the rotated patch, then file2input's window of 64
    for (int i = tid; i < kRows; i += BS) {
        double* __restrict__ t = tile + i * kTileStride;
        double idx[3] = {63.0, 63.0, 63.0};
        for (int c = 0; c < 17; ++c) t[c] = 0.0;
        const int64_t g = i < m ? row[i] : -1;
        if (g >= 0 && g < a.nf) {
            V3 b[3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
            const bool ok = corners(a.v, a.nv, a.f, g, b);
            // a zero-area face of the mesh keeps a zero normal and area: the rotated corners' rounding gives neither
            const bool flat = !(area_of(b) > 0.0);
            for (int c = 0; c < 3 && ok; ++c) {
                const V3 s = mul3(sub3(b[c], mean), scale);
                b[c] = V3{(R[0][0] * s.x + R[0][1] * s.y) + R[0][2] * s.z, (R[1][0] * s.x + R[1][1] * s.y) + R[1][2] * s.z,
                          (R[2][0] * s.x + R[2][1] * s.y) + R[2][2] * s.z};
                if (keep_centre) b[c] = V3{b[c].x + mean.x, b[c].y + mean.y, b[c].z + mean.z};
            }
            const V3 cen = centroid_of(b), nrm = flat ? V3{0.0, 0.0, 0.0} : normal_of(b);
            int64_t loc[3];
            int found = 0;
            for (int e = 0; e < 3; ++e) {
                const int64_t h = a.tt[3 * g + e];
                loc[e] = (h >= 0 && h < a.nf) ? find_in_row(row, m, h) : -1;
                found += loc[e] >= 0;
            }
            t[0] = cen.x; t[1] = cen.y; t[2] = cen.z;
            t[3] = nrm.x; t[4] = nrm.y; t[5] = nrm.z;
            t[6] = flat ? 0.0 : area_of(b);
            t[7] = (double)found;
            for (int c = 0; c < 3; ++c) { t[8 + 3 * c] = b[c].x; t[9 + 3 * c] = b[c].y; t[10 + 3 * c] = b[c].z; }
            // file2input's three index columns
            double hit[3];
            int nh = 0;
            if (a.adjacency) {                        // the local edge-neighbours inside the window, in slot order
                for (int e = 0; e < 3; ++e) if (loc[e] >= 0 && loc[e] < kRows) hit[nh++] = (double)loc[e];
                if (nh == 0) { hit[0] = (double)i; nh = 1; }
            } else {                                  // the slots whose neighbour is local face 1
                for (int e = 0; e < 3; ++e) if (loc[e] == 1) hit[nh++] = (double)e;
            }
            if (nh == 1) { idx[0] = idx[1] = idx[2] = hit[0]; }
            else if (nh == 2) { idx[0] = hit[0]; idx[1] = idx[2] = hit[1]; }
            else if (nh == 3) { idx[0] = hit[0]; idx[1] = hit[1]; idx[2] = hit[2]; }
        }
        t[17] = idx[0]; t[18] = idx[1]; t[19] = idx[2];
    }
    __syncthreads();
    OutT* __restrict__ o = out + p * (int64_t)(kRows * kCols);
    for (int x = tid; x < kRows * kCols; x += BS) {
        const int r = a.channels_first ? x % kRows : x / kCols, c = a.channels_first ? x / kRows : x % kCols;
        o[x] = (OutT)tile[r * kTileStride + c];
    }
}

}  // namespace pcd

using namespace pcd;

static constexpr int kSelectBlock = 64;
static constexpr int kInputBlock = 64;

extern "C" int pcd_mesh_tta(const void* f, int f_bits, int64_t nf, int64_t nv, void* tt, int out_bits, void* stream) {
    PCD_CHECK_ARG((f_bits == 32 || f_bits == 64) && (out_bits == 32 || out_bits == 64), "bits must be 32 or 64");
    PCD_CHECK_ARG(nv >= 0 && nf >= 0 && 3 * nf < (1ll << 32) && nv < (1ll << 32), "mesh too large");
    PCD_CHECK_ARG(out_bits == 64 || nf < (1ll << 31), "int32 adjacency needs nf < 2^31");
    if (nf == 0) return PCD_OK;
    PCD_CHECK_ARG(f && tt && nv > 0, "null argument");
    hipStream_t st = as_stream(stream);
    const int64_t nc = 3 * nf;
    unsigned long long *keys = nullptr, *skeys = nullptr;
    uint32_t *vals = nullptr, *svals = nullptr;
    int* bad = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    StreamTemps tt_(st);                   // freed on every exit path
    PCD_HIP(tt_.alloc(&keys, nc * 8));
    PCD_HIP(tt_.alloc(&skeys, nc * 8));
    PCD_HIP(tt_.alloc(&vals, nc * 4));
    PCD_HIP(tt_.alloc(&svals, nc * 4));
    PCD_HIP(tt_.alloc(&bad, sizeof(int)));
    PCD_HIP(hipMemsetAsync(bad, 0, sizeof(int), st));
    const dim3 grd((unsigned)cdiv(nc, 256)), blk(256);
    if (f_bits == 64) hipLaunchKernelGGL(k_tta_keys<int64_t>, grd, blk, 0, st, (const int64_t*)f, nc, nv, keys, vals, bad);
    else hipLaunchKernelGGL(k_tta_keys<int32_t>, grd, blk, 0, st, (const int32_t*)f, nc, nv, keys, vals, bad);
    (void)rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys, skeys, vals, svals, (size_t)nc, 0u, 64u, st);
    PCD_HIP(tt_.alloc(&tmp, tmp_bytes));
    if (rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, skeys, vals, svals, (size_t)nc, 0u, 64u, st) != hipSuccess)
        return fail(PCD_ERR_HIP, "pcd_mesh_tta: rocprim::radix_sort_pairs failed");
    if (out_bits == 64) hipLaunchKernelGGL(k_tta_out<int64_t>, grd, blk, 0, st, skeys, svals, nc, (int64_t*)tt);
    else hipLaunchKernelGGL(k_tta_out<int32_t>, grd, blk, 0, st, skeys, svals, nc, (int32_t*)tt);
    PCD_LAUNCH_CHECK();
    int hbad = 0;
    PCD_HIP(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st));
    PCD_HIP(tt_.release());                // (synchronises: hbad is valid)
    PCD_CHECK_ARG(hbad == 0, "face index out of range [0, nv)");
    return PCD_OK;
}

extern "C" int pcd_patch_radius(const double* v, int64_t nv, const int64_t* f, int64_t nf, const int64_t* tt,
                                const int64_t* faces, int64_t n, double k, double* centre, double* radius,
                                double* mean_area, void* stream) {
    PCD_CHECK_ARG(nv >= 0 && nf >= 0 && n >= 0, "negative size");
    PCD_CHECK_ARG(k == k, "k is NaN");
    if (n == 0) return PCD_OK;
    PCD_CHECK_ARG(v && f && tt && faces && centre && radius && nv > 0 && nf > 0, "null argument");
    hipLaunchKernelGGL(k_patch_radius, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, as_stream(stream), v, nv, f, nf, tt,
                       faces, n, k, centre, radius, mean_area);
    PCD_LAUNCH_CHECK();
    return PCD_OK;
}

static int select_args(SelectArgs& a, const pcd_grid* g, double widen, const double* v, int64_t nv, const int64_t* f,
                       int64_t nf, const int64_t* vf, const int64_t* ni, const double* centre, const double* radius,
                       int64_t n) {
    PCD_CHECK_ARG(g != nullptr, "grid is null");
    PCD_CHECK_ARG(nv >= 0 && nf >= 0 && n >= 0, "negative size");
    PCD_CHECK_ARG(g->n == nv, "the grid must hold the mesh's nv vertices");
    PCD_CHECK_ARG(widen >= 0.0 && widen < HUGE_VAL, "widen must be finite and >= 0");
    PCD_CHECK_ARG(n < (1ll << 31), "at most 2^31 - 1 patches per call");
    PCD_CHECK_ARG(n == 0 || (v && f && vf && ni && centre && radius), "null argument");
    a = SelectArgs{g->view, widen, v, nv, f, nf, vf, ni, centre, radius, n};
    return PCD_OK;
}

extern "C" int pcd_patch_select_count(const pcd_grid* g, double widen, const double* v, int64_t nv, const int64_t* f,
                                      int64_t nf, const int64_t* vf, const int64_t* ni, const double* centre,
                                      const double* radius, int64_t n, int64_t* counts, void* stream) {
    SelectArgs a;
    const int rc = select_args(a, g, widen, v, nv, f, nf, vf, ni, centre, radius, n);
    if (rc != PCD_OK) return rc;
    if (n == 0) return PCD_OK;
    PCD_CHECK_ARG(counts, "null argument");
    hipLaunchKernelGGL(k_select_count<kSelectBlock>, dim3((unsigned)n), dim3(kSelectBlock), 0, as_stream(stream), a, counts);
    PCD_LAUNCH_CHECK();
    return PCD_OK;
}

extern "C" int pcd_patch_select_fill(const pcd_grid* g, double widen, const double* v, int64_t nv, const int64_t* f,
                                     int64_t nf, const int64_t* vf, const int64_t* ni, const double* centre,
                                     const double* radius, int64_t n, const int64_t* off, int64_t capacity,
                                     int64_t* patch_faces, void* stream) {
    SelectArgs a;
    const int rc = select_args(a, g, widen, v, nv, f, nf, vf, ni, centre, radius, n);
    if (rc != PCD_OK) return rc;
    PCD_CHECK_ARG(capacity >= 0, "negative capacity");
    if (n == 0) return PCD_OK;
    PCD_CHECK_ARG(off && (patch_faces || capacity == 0), "null argument");
    hipStream_t st = as_stream(stream);
    int64_t* tmp = nullptr;
    int* status = nullptr;
    StreamTemps tt_(st);                   // freed on every exit path
    PCD_HIP(tt_.alloc(&tmp, (size_t)std::max<int64_t>(capacity, 1) * sizeof(int64_t)));
    PCD_HIP(tt_.alloc(&status, sizeof(int)));
    PCD_HIP(hipMemsetAsync(status, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_select_fill<kSelectBlock>, dim3((unsigned)n), dim3(kSelectBlock), 0, st, a, off, capacity, tmp,
                       patch_faces, status);
    PCD_LAUNCH_CHECK();
    int h = 0;
    PCD_HIP(hipMemcpyAsync(&h, status, sizeof(int), hipMemcpyDeviceToHost, st));
    PCD_HIP(tt_.release());                // (synchronises: h is valid)
    if (h & 1) return fail(PCD_ERR_ARG, "pcd_patch_select_fill: the patches do not fit the capacity of patch_faces");
    if (h & 2) return fail(PCD_ERR_ARG, "pcd_patch_select_fill: offsets do not match the counts of pcd_patch_select_count");
    return PCD_OK;
}

// The reference's r = k * mean ** 0.5 on a numpy scalar is libm's pow, not a correctly rounded root; this is that
// call (the exponent is kept from the compiler so that it cannot become sqrt).  Host arrays.
extern "C" int pcd_host_patch_radius(const double* mean_area, int64_t n, double k, double* radius) {
    PCD_CHECK_ARG(n >= 0 && (n == 0 || (mean_area && radius)), "bad argument");
    volatile double half = 0.5;
    for (int64_t i = 0; i < n; ++i) radius[i] = k * pow(mean_area[i], half);
    return PCD_OK;
}

extern "C" int pcd_patch_inputs(const double* v, int64_t nv, const int64_t* f, int64_t nf, const int64_t* tt,
                                const int64_t* vf, const int64_t* ni, const int64_t* faces, int64_t n,
                                const int64_t* off, const int64_t* patch_faces, int64_t total, int adjacency,
                                int out_bits, int channels_first, void* out, double* rot, int64_t* centre_index,
                                double* eig, void* stream) {
    PCD_CHECK_ARG(nv >= 0 && nf >= 0 && n >= 0 && total >= 0, "negative size");
    PCD_CHECK_ARG(n < (1ll << 31), "at most 2^31 - 1 patches per call");
    PCD_CHECK_ARG(out_bits == 32 || out_bits == 64, "out_bits must be 32 or 64");
    PCD_CHECK_ARG((adjacency == 0 || adjacency == 1) && (channels_first == 0 || channels_first == 1), "bad flag");
    if (n == 0) return PCD_OK;
    PCD_CHECK_ARG(v && f && tt && vf && ni && faces && off && (patch_faces || total == 0) && out && rot &&
                  centre_index && eig && nv > 0 && nf > 0, "null argument");
    const InputArgs a{v, nv, f, nf, tt, vf, ni, faces, n, off, patch_faces, total, adjacency, channels_first, rot,
                      centre_index, eig};
    const dim3 grd((unsigned)n), blk(kInputBlock);
    if (out_bits == 64) hipLaunchKernelGGL((k_patch_inputs<double, kInputBlock>), grd, blk, 0, as_stream(stream), a, (double*)out);
    else hipLaunchKernelGGL((k_patch_inputs<float, kInputBlock>), grd, blk, 0, as_stream(stream), a, (float*)out);
    PCD_LAUNCH_CHECK();
    return PCD_OK;
}
