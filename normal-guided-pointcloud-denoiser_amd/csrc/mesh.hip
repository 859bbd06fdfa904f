// Mesh vertex update (H18): Mesh.updateVertices, PatchGeneration/Modules/Mesh.py:377-418 (= Vertex_updating.ipynb
// Algorithm 3; native twin MeshDenoisingBase::updateVertexPosition, src/GCNDenoiser/GCNDenoiser/
// MeshDenoisingBase.cpp:107-143).  One thread per vertex gathers its incident faces through the igl
// vertex->face CSR (VF, NI) instead of the reference's padded (V, max_degree, 3, 3) temporaries; fp64 like numpy;
// Jacobi sweeps (the reference adds the whole update after computing it for every vertex).
#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "pcd_device.h"
#include "pcd_host.h"

namespace pcd {

__global__ __launch_bounds__(256) void k_mesh_update(const double* __restrict__ vin, double* __restrict__ vout,
                                                      int64_t nv, const int64_t* __restrict__ f,
                                                      const double* __restrict__ fn, const int64_t* __restrict__ vf,
                                                      const int64_t* __restrict__ ni) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const double x = vin[3 * i], y = vin[3 * i + 1], z = vin[3 * i + 2];
    double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};   // [corner][axis], summed over faces first (numpy order)
    const int64_t s = ni[i], e = ni[i + 1];
    for (int64_t t = s; t < e; ++t) {
        const int64_t face = vf[t];
        const double n0 = fn[3 * face], n1 = fn[3 * face + 1], n2 = fn[3 * face + 2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t vc = f[3 * face + c];
            const double d0 = vin[3 * vc] - x, d1 = vin[3 * vc + 1] - y, d2 = vin[3 * vc + 2] - z;
            const double dot = __dadd_rn(__dadd_rn(__dmul_rn(n0, d0), __dmul_rn(n1, d1)), __dmul_rn(n2, d2));
            S[c][0] = __dadd_rn(S[c][0], __dmul_rn(dot, n0));
            S[c][1] = __dadd_rn(S[c][1], __dmul_rn(dot, n1));
            S[c][2] = __dadd_rn(S[c][2], __dmul_rn(dot, n2));
        }
    }
    const double deg3 = 3.0 * (double)(e - s);   // degree 0 -> 0/0 = NaN, as numpy
    vout[3 * i] = x + (S[0][0] + S[1][0] + S[2][0]) / deg3;
    vout[3 * i + 1] = y + (S[0][1] + S[1][1] + S[2][1]) / deg3;
    vout[3 * i + 2] = z + (S[0][2] + S[1][2] + S[2][2]) / deg3;
}

// ---------------------------------------------------------------------------------------------- fp32 path
// The same update in fp32 on MI355X-shaped buffers: vertices and face normals as float4 rows (one 16-B load per
// gather), faces as int4 (three corner ids + pad), the vertex->face CSR in int32.  Algorithmic bytes per vertex per
// sweep: own v 12 + write 12 + NI 8 + per incident face (VF 4 + normal 12 + corners 12 + 3 corner
// rows 36) = 32 + 64 deg (416 B at deg 6).  Sums in the reference's order (per corner over faces, then corners).
__global__ __launch_bounds__(256) void k_mesh_update_f32(const float4* __restrict__ vin, float4* __restrict__ vout,
                                                          int64_t nv, const int4* __restrict__ f4,
                                                          const float4* __restrict__ fn4, const int32_t* __restrict__ vf,
                                                          const int32_t* __restrict__ ni) {
    const int64_t i = xcd_block(blockIdx.x, gridDim.x) * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const float4 p = vin[i];
    float S[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    const int s = ni[i], e = ni[i + 1];
    for (int t = s; t < e; ++t) {
        const int face = vf[t];
        const float4 n = fn4[face];
        const int4 c = f4[face];
        const float4 q[3] = {vin[c.x], vin[c.y], vin[c.z]};   // the three corner rows in flight together
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float d0 = q[k].x - p.x, d1 = q[k].y - p.y, d2 = q[k].z - p.z;
            const float dot = (n.x * d0 + n.y * d1) + n.z * d2;
            S[k][0] += dot * n.x;
            S[k][1] += dot * n.y;
            S[k][2] += dot * n.z;
        }
    }
    const float deg3 = 3.f * (float)(e - s);
    vout[i] = make_float4(p.x + (S[0][0] + S[1][0] + S[2][0]) / deg3, p.y + (S[0][1] + S[1][1] + S[2][1]) / deg3,
                          p.z + (S[0][2] + S[1][2] + S[2][2]) / deg3, 0.f);
}
__global__ void k_rows3_to4(const float* __restrict__ a, int64_t n, float4* __restrict__ out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) out[i] = make_float4(a[3 * i], a[3 * i + 1], a[3 * i + 2], 0.f);
}
__global__ void k_rows4_to3(const float4* __restrict__ a, int64_t n, float* __restrict__ out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) { const float4 v = a[i]; out[3 * i] = v.x; out[3 * i + 1] = v.y; out[3 * i + 2] = v.z; }
}
template <class I>
__global__ void k_faces_to4(const I* __restrict__ f, int64_t nf, int4* __restrict__ out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < nf) out[i] = make_int4((int)f[3 * i], (int)f[3 * i + 1], (int)f[3 * i + 2], 0);
}

// ---------------------------------------------------------------------------------------------- adjacency
// igl.vertex_triangle_adjacency on the device: corners (vertex id, corner index 3f + c) radix-sorted by vertex id
// (stable: each vertex's faces in increasing face order, igl's VF), VF = corner / 3, NI = first corner of each
// vertex in the sorted order (degree-0 vertices get empty ranges).
template <class I>
__global__ void k_vta_keys(const I* __restrict__ f, int64_t nc, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                           int* __restrict__ bad, int64_t nv) {
    const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (c >= nc) return;
    const int64_t v = (int64_t)f[c];
    if (v < 0 || v >= nv) atomicOr(bad, 1);
    keys[c] = (uint32_t)(v < 0 ? 0 : v >= nv ? nv - 1 : v);
    vals[c] = (uint32_t)c;
}
template <class I>
__global__ void k_vta_out(const uint32_t* __restrict__ skeys, const uint32_t* __restrict__ svals, int64_t nc,
                          int64_t nv, I* __restrict__ vf, I* __restrict__ ni) {
    const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (p > nc) return;
    if (p < nc) vf[p] = (I)(svals[p] / 3u);
    const int64_t prev = p == 0 ? -1 : (int64_t)skeys[p - 1];
    const int64_t cur = p == nc ? nv : (int64_t)skeys[p];
    for (int64_t v = prev + 1; v <= cur && v <= nv; ++v) ni[v] = (I)p;   // first corner of v (empty runs: same p)
    if (p == nc) ni[nv] = (I)nc;
}

// ---------------------------------------------------------------------------------------------- normal filtering
// Guided bilateral filtering of the face normals (MeshNormalFiltering::updateFilteredNormalsWithPredictedNormal,
// src/GCNDenoiser/GCNDenoiser/MeshNormalFiltering.cpp:170-244).  One thread per face in every kernel.  Two layouts,
// as for the vertex update: plain fp64 rows with int64 indices (the parity path) and float4 / int4 rows with int32
// indices (the fast path); the adjacent-centroid mean is summed in fp64 in both.
struct D3 { double x, y, z; };
__device__ __forceinline__ double len3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

struct Lay64 {                       // fp64 rows, int64 indices
    using I = int64_t;
    const double* c;
    const int64_t* f;
    __device__ D3 cen(int64_t i) const { return D3{c[3 * i], c[3 * i + 1], c[3 * i + 2]}; }
    __device__ void face(int64_t i, int64_t (&v)[3]) const { v[0] = f[3 * i]; v[1] = f[3 * i + 1]; v[2] = f[3 * i + 2]; }
};
struct Lay32 {                       // float4 centroids, int4 faces, int32 indices
    using I = int32_t;
    const float4* c;
    const int4* f;
    __device__ D3 cen(int64_t i) const { const float4 q = c[i]; return D3{(double)q.x, (double)q.y, (double)q.z}; }
    __device__ void face(int64_t i, int64_t (&v)[3]) const { const int4 q = f[i]; v[0] = q.x; v[1] = q.y; v[2] = q.z; }
};

// Face geometry (MeshDenoisingBase::getFaceCentroid / getFaceArea / getFaceNormal, MeshDenoisingBase.cpp:24-65, with
// the orientation of Mesh.getFaceNormals, Mesh.py:110-114): centroid ((p0 + p1) + p2) / 3, the cross product
// (p1 − p0) × (p2 − p1), area = half its length (p1 − p2 is exactly −(p2 − p1), so this is the reference's
// 0.5 |(p1 − p0) × (p1 − p2)| bit for bit), normal = cross / length; a face of zero area gets the zero normal.
// A corner index outside [0, nv) reads nothing: the face gets zeros.
__global__ __launch_bounds__(256) void k_face_geom(const double* __restrict__ v, int64_t nv, const int64_t* __restrict__ f,
                                                    int64_t nf, double* __restrict__ cen, double* __restrict__ area,
                                                    double* __restrict__ nrm) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nf) return;
    const int64_t a = f[3 * i], b = f[3 * i + 1], c = f[3 * i + 2];
    double cx = 0, cy = 0, cz = 0, ar = 0, nx = 0, ny = 0, nz = 0;
    if (a >= 0 && a < nv && b >= 0 && b < nv && c >= 0 && c < nv) {
        const double p0x = v[3 * a], p0y = v[3 * a + 1], p0z = v[3 * a + 2];
        const double p1x = v[3 * b], p1y = v[3 * b + 1], p1z = v[3 * b + 2];
        const double p2x = v[3 * c], p2y = v[3 * c + 1], p2z = v[3 * c + 2];
        cx = ((p0x + p1x) + p2x) / 3.0; cy = ((p0y + p1y) + p2y) / 3.0; cz = ((p0z + p1z) + p2z) / 3.0;
        const double ux = p1x - p0x, uy = p1y - p0y, uz = p1z - p0z;
        const double wx = p2x - p1x, wy = p2y - p1y, wz = p2z - p1z;
        const double rx = uy * wz - uz * wy, ry = uz * wx - ux * wz, rz = ux * wy - uy * wx;
        const double len = len3(rx, ry, rz);
        ar = 0.5 * len;
        if (len > 0.0 && len < HUGE_VAL) { nx = rx / len; ny = ry / len; nz = rz / len; }
    }
    cen[3 * i] = cx; cen[3 * i + 1] = cy; cen[3 * i + 2] = cz;
    area[i] = ar;
    nrm[3 * i] = nx; nrm[3 * i + 1] = ny; nrm[3 * i + 2] = nz;
}
// The same in fp32 on float4 rows: centroid; normal with the area in .w.
__global__ __launch_bounds__(256) void k_face_geom_f32(const float4* __restrict__ v, const int4* __restrict__ f4,
                                                        int64_t nf, float4* __restrict__ cen, float4* __restrict__ nrm) {
    const int64_t i = xcd_block(blockIdx.x, gridDim.x) * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nf) return;
    const int4 q = f4[i];
    const float4 p0 = v[q.x], p1 = v[q.y], p2 = v[q.z];
    const float ux = p1.x - p0.x, uy = p1.y - p0.y, uz = p1.z - p0.z;
    const float wx = p2.x - p1.x, wy = p2.y - p1.y, wz = p2.z - p1.z;
    const float rx = uy * wz - uz * wy, ry = uz * wx - ux * wz, rz = ux * wy - uy * wx;
    const float len = sqrtf((rx * rx + ry * ry) + rz * rz);
    const bool ok = len > 0.f && len < HUGE_VALF;
    cen[i] = make_float4(((p0.x + p1.x) + p2.x) / 3.f, ((p0.y + p1.y) + p2.y) / 3.f, ((p0.z + p1.z) + p2.z) / 3.f, 0.f);
    nrm[i] = make_float4(ok ? rx / len : 0.f, ok ? ry / len : 0.f, ok ? rz / len : 0.f, 0.5f * len);
}

// Mean centroid distance over the ordered pairs of faces that share an edge (MeshNormalFiltering::getRadius /
// getSigmaS, MeshNormalFiltering.cpp:134-168: the ff_iter of every face).  Face i walks the incident faces of the
// first vertex of each of its edges (the vertex->face CSR) and takes every other face that also holds the second: a
// boundary edge gives no pair, an edge with more than two faces gives every other face on it.  Deterministic: one
// partial (sum, pair count) per block from a fixed LDS tree, then one block folds the partials in a fixed order.
template <class L>
__global__ __launch_bounds__(256) void k_adj_partial(L lay, int64_t nf, int64_t nv, const typename L::I* __restrict__ vf,
                                                      const typename L::I* __restrict__ ni, double* __restrict__ psum,
                                                      unsigned long long* __restrict__ pcnt) {
    __shared__ double ss[256];
    __shared__ unsigned long long sc[256];
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    double s = 0.0;
    unsigned long long n = 0;
    if (i < nf) {
        int64_t fv[3];
        lay.face(i, fv);
        const D3 ci = lay.cen(i);
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int64_t a = fv[e], b = fv[e == 2 ? 0 : e + 1];
            if (a < 0 || a >= nv) continue;
            const int64_t t0 = ni[a], t1 = ni[a + 1];
            for (int64_t t = t0; t < t1; ++t) {
                const int64_t g = vf[t];
                if (g == i || g < 0 || g >= nf) continue;
                int64_t gv[3];
                lay.face(g, gv);
                if (gv[0] != b && gv[1] != b && gv[2] != b) continue;
                const D3 cg = lay.cen(g);
                s += len3(cg.x - ci.x, cg.y - ci.y, cg.z - ci.z);
                ++n;
            }
        }
    }
    ss[threadIdx.x] = s;
    sc[threadIdx.x] = n;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { ss[threadIdx.x] += ss[threadIdx.x + w]; sc[threadIdx.x] += sc[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { psum[blockIdx.x] = ss[0]; pcnt[blockIdx.x] = sc[0]; }
}
// out2[0] = mean (0 when there is no pair), out2[1] = the pair count
__global__ __launch_bounds__(256) void k_adj_final(const double* __restrict__ psum, const unsigned long long* __restrict__ pcnt,
                                                    int64_t nb, double* __restrict__ out2) {
    __shared__ double ss[256];
    __shared__ unsigned long long sc[256];
    double s = 0.0;
    unsigned long long n = 0;
    for (int64_t b = threadIdx.x; b < nb; b += 256) { s += psum[b]; n += pcnt[b]; }
    ss[threadIdx.x] = s;
    sc[threadIdx.x] = n;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { ss[threadIdx.x] += ss[threadIdx.x + w]; sc[threadIdx.x] += sc[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out2[0] = sc[0] ? ss[0] / (double)sc[0] : 0.0; out2[1] = (double)sc[0]; }
}

// Face neighbourhoods (MeshNormalFiltering::getRadiusBasedFaceNeighbor, MeshNormalFiltering.cpp:47-78; mode 1:
// the vertex-based set of MeshDenoisingBase::getFaceNeighbor, MeshDenoisingBase.cpp:75-92), centre included.  The
// breadth-first search of face i runs inside its own segment [cap_off[i], cap_off[i+1]) of `rows`, which is both the
// queue and the visited set; the caller sizes the segment with an upper bound on the row (the Euclidean ball count:
// every face stepped onto lies within the radius).  Every loop is bounded before it starts: the queue walk by the
// segment's capacity, the expansion by the vertex degrees.  A row that would not fit sets bit 0 of *status and stops
// growing.  The reference marks a rejected face visited; re-testing it gives the same answer, so the set is the same.
__global__ __launch_bounds__(256) void k_nbr_bfs(const double* __restrict__ cen, const int64_t* __restrict__ f, int64_t nf, int64_t nv,
                                                  const int64_t* __restrict__ vf, const int64_t* __restrict__ ni,
                                                  int mode, double radius, const int64_t* __restrict__ cap_off,
                                                  int64_t* __restrict__ rows, int64_t* __restrict__ counts,
                                                  int* __restrict__ status) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nf) return;
    int64_t* seg = rows + cap_off[i];
    const int64_t cap = cap_off[i + 1] - cap_off[i];
    if (cap < 1) { counts[i] = 0; atomicOr(status, 1); return; }
    const double cx = cen[3 * i], cy = cen[3 * i + 1], cz = cen[3 * i + 2];
    seg[0] = i;
    int64_t cnt = 1;
    bool over = false;
    const int64_t walk = mode == 1 ? 1 : cap;            // vertex mode expands the centre only
    for (int64_t head = 0; head < walk; ++head) {
        if (head >= cnt) break;
        const int64_t g = seg[head];
        for (int c = 0; c < 3; ++c) {
            const int64_t vtx = f[3 * g + c];
            if (vtx < 0 || vtx >= nv) continue;
            const int64_t t0 = ni[vtx], t1 = ni[vtx + 1];
            for (int64_t t = t0; t < t1; ++t) {
                const int64_t h = vf[t];
                if (h < 0 || h >= nf) continue;
                bool seen = false;
                for (int64_t u = 0; u < cnt; ++u) seen |= (seg[u] == h);
                if (seen) continue;
                if (mode != 1) {
                    const double d = len3(cx - cen[3 * h], cy - cen[3 * h + 1], cz - cen[3 * h + 2]);
                    if (!(d <= radius)) continue;
                }
                if (cnt < cap) seg[cnt++] = h;
                else over = true;
            }
        }
    }
    counts[i] = cnt;
    if (over) atomicOr(status, 1);
}
// rows of the CSR in ascending face index: the members of a row are distinct, so each one's rank is its slot
__global__ __launch_bounds__(256) void k_nbr_fill(const int64_t* __restrict__ rows, const int64_t* __restrict__ cap_off,
                                                   const int64_t* __restrict__ off, int64_t nf, int64_t* __restrict__ out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nf) return;
    const int64_t* seg = rows + cap_off[i];
    const int64_t cap = cap_off[i + 1] - cap_off[i];
    const int64_t cnt = std::min<int64_t>(off[i + 1] - off[i], cap);
    for (int64_t a = 0; a < cnt; ++a) {
        const int64_t x = seg[a];
        int64_t rank = 0;
        for (int64_t b = 0; b < cnt; ++b) rank += (seg[b] < x);
        out[off[i] + rank] = x;
    }
}

// One filter pass (MeshNormalFiltering.cpp:207-236): s = Σ_j src_j A_j exp(−|c_i − c_j|² / 2σ_s²) exp(−|g_i − g_j|² / 2σ_r²)
// over the row of face i, out = s / |s|; |s| zero or not finite keeps src_i.  A neighbour of zero area has weight 0 and
// its normal is not read; a centre of zero area gets the zero normal (the vertex update then ignores it).
// σ_s = multiple_sigma_s · scale[0] is read from device memory (k_adj_final wrote it on this stream).
__global__ __launch_bounds__(256) void k_filter(const double* __restrict__ cen, const double* __restrict__ area,
                                                 const double* __restrict__ g, const double* __restrict__ src, int64_t nf,
                                                 const int64_t* __restrict__ off, const int64_t* __restrict__ nbr,
                                                 double sigma_r, double mult_s, const double* __restrict__ scale,
                                                 double* __restrict__ out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nf) return;
    const double sigma_s = mult_s * scale[0];
    const double ds = 2.0 * (sigma_s * sigma_s), dr = 2.0 * (sigma_r * sigma_r);
    const double cx = cen[3 * i], cy = cen[3 * i + 1], cz = cen[3 * i + 2];
    const double gx = g[3 * i], gy = g[3 * i + 1], gz = g[3 * i + 2];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    const int64_t t0 = off[i], t1 = off[i + 1];
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t j = nbr[t];
        const double a = area[j];
        if (!(a > 0.0)) continue;
        const double dx = cx - cen[3 * j], dy = cy - cen[3 * j + 1], dz = cz - cen[3 * j + 2];
        const double ex = gx - g[3 * j], ey = gy - g[3 * j + 1], ez = gz - g[3 * j + 2];
        const double ws = exp(-(((dx * dx + dy * dy) + dz * dz) / ds));
        const double wr = exp(-(((ex * ex + ey * ey) + ez * ez) / dr));
        const double w = (a * ws) * wr;
        sx += src[3 * j] * w; sy += src[3 * j + 1] * w; sz += src[3 * j + 2] * w;
    }
    double ox = 0.0, oy = 0.0, oz = 0.0;
    if (area[i] > 0.0) {
        const double len = len3(sx, sy, sz);
        if (len > 0.0 && len < HUGE_VAL) { ox = sx / len; oy = sy / len; oz = sz / len; }
        else { ox = src[3 * i]; oy = src[3 * i + 1]; oz = src[3 * i + 2]; }
    }
    out[3 * i] = ox; out[3 * i + 1] = oy; out[3 * i + 2] = oz;
}
// fp32 pass on float4 rows: centroid; guidance normal; source normal with the area in .w.  Algorithmic bytes per face
// and pass: own centroid, guidance and source rows 48 + offsets 8 + write 16 + per row entry (index 4 + centroid 16 +
// guidance 16 + source 16) = 72 + 52 L.  (Streaming a range weight computed once per entry instead of gathering the
// guidance row, 56 + 40 L, measured no faster: DESIGN.md's tried table.)
__global__ __launch_bounds__(256) void k_filter_f32(const float4* __restrict__ cen, const float4* __restrict__ g,
                                                     const float4* __restrict__ src, int64_t nf,
                                                     const int32_t* __restrict__ off, const int32_t* __restrict__ nbr,
                                                     float sigma_r, float mult_s, const double* __restrict__ scale,
                                                     float4* __restrict__ out) {
    const int64_t i = xcd_block(blockIdx.x, gridDim.x) * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nf) return;
    const float sigma_s = mult_s * (float)scale[0];
    const float ds = 2.f * (sigma_s * sigma_s), dr = 2.f * (sigma_r * sigma_r);
    const float4 ci = cen[i], si = src[i], gi = g[i];
    float sx = 0.f, sy = 0.f, sz = 0.f;
    const int t0 = off[i], t1 = off[i + 1];
    for (int t = t0; t < t1; ++t) {
        const int j = nbr[t];
        const float4 sj = src[j];
        if (!(sj.w > 0.f)) continue;
        const float4 cj = cen[j];
        const float dx = ci.x - cj.x, dy = ci.y - cj.y, dz = ci.z - cj.z;
        const float ws = expf(-(((dx * dx + dy * dy) + dz * dz) / ds));
        const float4 gj = g[j];
        const float ex = gi.x - gj.x, ey = gi.y - gj.y, ez = gi.z - gj.z;
        const float wr = expf(-(((ex * ex + ey * ey) + ez * ez) / dr));
        const float w = (sj.w * ws) * wr;
        sx += sj.x * w; sy += sj.y * w; sz += sj.z * w;
    }
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (si.w > 0.f) {
        const float len = sqrtf((sx * sx + sy * sy) + sz * sz);
        if (len > 0.f && len < HUGE_VALF) o = make_float4(sx / len, sy / len, sz / len, 0.f);
        else o = make_float4(si.x, si.y, si.z, 0.f);
    }
    out[i] = o;
}
// the source rows of the first iteration: the guidance normal with the current area
__global__ void k_src_from_guidance(const float4* __restrict__ g, int64_t nf, float4* __restrict__ src) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < nf) { const float4 q = g[i]; src[i] = make_float4(q.x, q.y, q.z, src[i].w); }
}
__global__ void k_rows3w_to4(const float* __restrict__ a, const float* __restrict__ w, int64_t n, float4* __restrict__ out) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) out[i] = make_float4(a[3 * i], a[3 * i + 1], a[3 * i + 2], w[i]);
}
// vertices in no face keep their input position (the sweeps give them 0/0); rows of W scalars
template <class T, int W, class I>
__global__ void k_restore_isolated(const T* __restrict__ v0, T* __restrict__ v, int64_t nv, const I* __restrict__ ni) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= nv || ni[i + 1] != ni[i]) return;
    for (int c = 0; c < W; ++c) v[W * i + c] = v0[W * i + c];
}

// one allocation cut into 256-byte aligned pieces
struct Carver {
    char* base = nullptr;
    size_t used = 0;
    size_t reserve(size_t bytes) { const size_t at = used; used += (bytes + 255) / 256 * 256; return at; }
    template <class T> T* at(size_t o) const { return reinterpret_cast<T*>(base + o); }
};

template <class L>
static void launch_scale(L lay, int64_t nf, int64_t nv, const typename L::I* vf, const typename L::I* ni, double* psum,
                         unsigned long long* pcnt, double* out2, hipStream_t st) {
    const int64_t nb = cdiv(nf, 256);
    hipLaunchKernelGGL(k_adj_partial<L>, dim3((unsigned)nb), dim3(256), 0, st, lay, nf, nv, vf, ni, psum, pcnt);
    hipLaunchKernelGGL(k_adj_final, dim3(1), dim3(256), 0, st, psum, pcnt, nb, out2);
}

}  // namespace pcd

using namespace pcd;

extern "C" int pcd_mesh_vta(const void* f, int f_bits, int64_t nf, int64_t nv, void* vf, void* ni, int out_bits,
                            void* stream) {
    PCD_CHECK_ARG((f_bits == 32 || f_bits == 64) && (out_bits == 32 || out_bits == 64), "bits must be 32 or 64");
    PCD_CHECK_ARG(nv >= 0 && nf >= 0 && 3 * nf < (1ll << 32) && nv < (1ll << 32), "mesh too large");
    PCD_CHECK_ARG(out_bits == 64 || 3 * nf < (1ll << 31), "int32 adjacency needs 3 nf < 2^31");
    hipStream_t st = as_stream(stream);
    if (nv == 0) return PCD_OK;
    PCD_CHECK_ARG(ni && (nf == 0 || (f && vf)), "null argument");
    const int64_t nc = 3 * nf;
    uint32_t *keys = nullptr, *vals = nullptr, *skeys = nullptr, *svals = nullptr;
    int* bad = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
    const size_t n = (size_t)std::max<int64_t>(nc, 1);
    StreamTemps tt(st);                    // freed on every exit path
    PCD_HIP(tt.alloc(&keys, n * 4));
    PCD_HIP(tt.alloc(&vals, n * 4));
    PCD_HIP(tt.alloc(&skeys, n * 4));
    PCD_HIP(tt.alloc(&svals, n * 4));
    PCD_HIP(tt.alloc(&bad, sizeof(int)));
    PCD_HIP(hipMemsetAsync(bad, 0, sizeof(int), st));
    const dim3 blk(256);
    if (nc > 0) {
        if (f_bits == 64) hipLaunchKernelGGL(k_vta_keys<int64_t>, dim3((unsigned)cdiv(nc, 256)), blk, 0, st, (const int64_t*)f, nc, keys, vals, bad, nv);
        else hipLaunchKernelGGL(k_vta_keys<int32_t>, dim3((unsigned)cdiv(nc, 256)), blk, 0, st, (const int32_t*)f, nc, keys, vals, bad, nv);
        unsigned end_bit = 1;
        while (end_bit < 32 && ((uint64_t)1 << end_bit) < (uint64_t)nv) ++end_bit;
        (void)rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys, skeys, vals, svals, (size_t)nc, 0u, end_bit, st);
        PCD_HIP(tt.alloc(&tmp, tmp_bytes));
        if (rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, skeys, vals, svals, (size_t)nc, 0u, end_bit, st) != hipSuccess)
            return fail(PCD_ERR_HIP, "pcd_mesh_vta: rocprim::radix_sort_pairs failed");
    }
    const dim3 grd((unsigned)cdiv(nc + 1, 256));
    if (out_bits == 64) hipLaunchKernelGGL(k_vta_out<int64_t>, grd, blk, 0, st, skeys, svals, nc, nv, (int64_t*)vf, (int64_t*)ni);
    else hipLaunchKernelGGL(k_vta_out<int32_t>, grd, blk, 0, st, skeys, svals, nc, nv, (int32_t*)vf, (int32_t*)ni);
    PCD_LAUNCH_CHECK();
    int hbad = 0;
    PCD_HIP(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, st));
    PCD_HIP(tt.release());                 // (synchronises: hbad is valid)
    PCD_CHECK_ARG(hbad == 0, "face index out of range [0, nv)");
    return PCD_OK;
}

extern "C" int pcd_mesh_update_f32(float* v, int64_t nv, const int32_t* f, const float* fn, int64_t nf,
                                   const int32_t* vf, const int32_t* ni, int k, void* stream) {
    PCD_CHECK_ARG(k >= 0, "k must be >= 0");
    if (nv == 0 || k == 0) return PCD_OK;
    PCD_CHECK_ARG(v && f && fn && vf && ni && nf > 0, "null argument");
    PCD_CHECK_ARG(nv < (1ll << 31) && 3 * nf < (1ll << 31), "fp32 path: int32 indices");
    hipStream_t st = as_stream(stream);
    float4 *a = nullptr, *b = nullptr, *fn4 = nullptr;
    int4* f4 = nullptr;
    StreamTemps tt(st);                    // freed on every exit path
    PCD_HIP(tt.alloc(&a, nv * sizeof(float4)));
    PCD_HIP(tt.alloc(&b, nv * sizeof(float4)));
    PCD_HIP(tt.alloc(&fn4, nf * sizeof(float4)));
    PCD_HIP(tt.alloc(&f4, nf * sizeof(int4)));
    const dim3 blk(256);
    hipLaunchKernelGGL(k_rows3_to4, dim3((unsigned)cdiv(nv, 256)), blk, 0, st, v, nv, a);
    hipLaunchKernelGGL(k_rows3_to4, dim3((unsigned)cdiv(nf, 256)), blk, 0, st, fn, nf, fn4);
    hipLaunchKernelGGL(k_faces_to4<int32_t>, dim3((unsigned)cdiv(nf, 256)), blk, 0, st, f, nf, f4);
    float4* buf[2] = {a, b};
    int cur = 0;
    for (int it = 0; it < k; ++it) {
        hipLaunchKernelGGL(k_mesh_update_f32, dim3((unsigned)cdiv(nv, 256)), blk, 0, st, buf[cur], buf[cur ^ 1], nv,
                           f4, fn4, vf, ni);
        cur ^= 1;
    }
    hipLaunchKernelGGL(k_rows4_to3, dim3((unsigned)cdiv(nv, 256)), blk, 0, st, buf[cur], nv, v);
    PCD_LAUNCH_CHECK();
    PCD_HIP(tt.release(false));
    return PCD_OK;
}

extern "C" int pcd_mesh_update(double* v, int64_t nv, const int64_t* f, const double* fn, int64_t nf,
                               const int64_t* vf, const int64_t* ni, int k, void* stream) {
    PCD_CHECK_ARG(k >= 0, "k must be >= 0");
    if (nv == 0 || k == 0) return PCD_OK;
    PCD_CHECK_ARG(v && f && fn && vf && ni && nf > 0, "null argument");
    hipStream_t st = as_stream(stream);
    double* tmp = nullptr;
    StreamTemps tt(st);                    // freed on every exit path
    PCD_HIP(tt.alloc(&tmp, nv * 3 * sizeof(double)));
    double* buf[2] = {v, tmp};
    int cur = 0;
    const dim3 grd((unsigned)cdiv(nv, 256)), blk(256);
    for (int it = 0; it < k; ++it) {
        hipLaunchKernelGGL(k_mesh_update, grd, blk, 0, st, buf[cur], buf[cur ^ 1], nv, f, fn, vf, ni);
        cur ^= 1;
    }
    PCD_LAUNCH_CHECK();
    if (cur != 0) PCD_HIP(hipMemcpyAsync(v, tmp, nv * 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
    PCD_HIP(tt.release(false));
    return PCD_OK;
}

// ---------------------------------------------------------------------------------------------- normal filtering ABI
extern "C" int pcd_mesh_face_geometry(const double* v, int64_t nv, const int64_t* f, int64_t nf, double* centroid,
                                      double* area, double* normal, void* stream) {
    PCD_CHECK_ARG(nv >= 0 && nf >= 0, "negative size");
    if (nf == 0) return PCD_OK;
    PCD_CHECK_ARG(v && f && centroid && area && normal && nv > 0, "null argument");
    hipLaunchKernelGGL(k_face_geom, dim3((unsigned)cdiv(nf, 256)), dim3(256), 0, as_stream(stream), v, nv, f, nf,
                       centroid, area, normal);
    PCD_LAUNCH_CHECK();
    return PCD_OK;
}

extern "C" int pcd_mesh_face_scale(const double* centroid, const int64_t* f, int64_t nf, const int64_t* vf,
                                   const int64_t* ni, int64_t nv, double* out2, void* stream) {
    PCD_CHECK_ARG(nv >= 0 && nf >= 0 && out2, "bad argument");
    hipStream_t st = as_stream(stream);
    if (nf == 0) { PCD_HIP(hipMemsetAsync(out2, 0, 2 * sizeof(double), st)); return PCD_OK; }
    PCD_CHECK_ARG(centroid && f && vf && ni && nv > 0, "null argument");
    const int64_t nb = cdiv(nf, 256);
    double* psum = nullptr;
    unsigned long long* pcnt = nullptr;
    StreamTemps tt(st);                    // freed on every exit path
    PCD_HIP(tt.alloc(&psum, nb * sizeof(double)));
    PCD_HIP(tt.alloc(&pcnt, nb * sizeof(unsigned long long)));
    launch_scale(Lay64{centroid, f}, nf, nv, vf, ni, psum, pcnt, out2, st);
    PCD_LAUNCH_CHECK();
    PCD_HIP(tt.release(false));
    return PCD_OK;
}

extern "C" int pcd_mesh_nbr_count(const double* centroid, const int64_t* f, int64_t nf, const int64_t* vf,
                                  const int64_t* ni, int64_t nv, int mode, double radius, const int64_t* cap_off,
                                  int64_t* rows, int64_t* counts, void* stream) {
    PCD_CHECK_ARG(mode == 0 || mode == 1, "mode must be 0 (radius) or 1 (vertex)");
    PCD_CHECK_ARG(mode == 1 || radius >= 0.0, "radius must be >= 0");     // (a NaN radius fails this too)
    PCD_CHECK_ARG(nv >= 0 && nf >= 0, "negative size");
    if (nf == 0) return PCD_OK;
    PCD_CHECK_ARG(centroid && f && vf && ni && cap_off && rows && counts && nv > 0, "null argument");
    hipStream_t st = as_stream(stream);
    int* status = nullptr;
    StreamTemps tt(st);                    // freed on every exit path
    PCD_HIP(tt.alloc(&status, sizeof(int)));
    PCD_HIP(hipMemsetAsync(status, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_nbr_bfs, dim3((unsigned)cdiv(nf, 256)), dim3(256), 0, st, centroid, f, nf, nv, vf, ni, mode,
                       radius, cap_off, rows, counts, status);
    PCD_LAUNCH_CHECK();
    int h = 0;
    PCD_HIP(hipMemcpyAsync(&h, status, sizeof(int), hipMemcpyDeviceToHost, st));
    PCD_HIP(tt.release());                 // (synchronises: h is valid)
    if (h != 0) return fail(PCD_ERR_ARG, "pcd_mesh_nbr_count: a neighbourhood does not fit its segment of rows");
    return PCD_OK;
}

extern "C" int pcd_mesh_nbr_fill(const int64_t* rows, const int64_t* cap_off, const int64_t* offsets, int64_t nf,
                                 int64_t* nbr_out, void* stream) {
    PCD_CHECK_ARG(nf >= 0, "negative size");
    if (nf == 0) return PCD_OK;
    PCD_CHECK_ARG(rows && cap_off && offsets && nbr_out, "null argument");
    hipLaunchKernelGGL(k_nbr_fill, dim3((unsigned)cdiv(nf, 256)), dim3(256), 0, as_stream(stream), rows, cap_off, offsets,
                       nf, nbr_out);
    PCD_LAUNCH_CHECK();
    return PCD_OK;
}

extern "C" int pcd_mesh_filter(const double* centroid, const double* area, const double* guided, const double* src,
                               int64_t nf, const int64_t* off, const int64_t* nbr, double sigma_r,
                               double multiple_sigma_s, const double* scale, double* out, void* stream) {
    PCD_CHECK_ARG(sigma_r > 0.0 && multiple_sigma_s > 0.0, "sigma_r and multiple_sigma_s must be > 0");
    PCD_CHECK_ARG(nf >= 0, "negative size");
    if (nf == 0) return PCD_OK;
    PCD_CHECK_ARG(centroid && area && guided && src && off && nbr && scale && out, "null argument");
    PCD_CHECK_ARG(out != src && out != guided, "out must not alias an input");
    hipLaunchKernelGGL(k_filter, dim3((unsigned)cdiv(nf, 256)), dim3(256), 0, as_stream(stream), centroid, area, guided,
                       src, nf, off, nbr, sigma_r, multiple_sigma_s, scale, out);
    PCD_LAUNCH_CHECK();
    return PCD_OK;
}

extern "C" int pcd_mesh_filter_f32(const float* centroid, const float* area, const float* guided, const float* src,
                                   int64_t nf, const int32_t* off, const int32_t* nbr, int64_t total, float sigma_r,
                                   float multiple_sigma_s, const double* scale, float* out, void* stream) {
    PCD_CHECK_ARG(sigma_r > 0.f && multiple_sigma_s > 0.f, "sigma_r and multiple_sigma_s must be > 0");
    PCD_CHECK_ARG(nf >= 0 && total >= 0, "negative size");
    if (nf == 0) return PCD_OK;
    PCD_CHECK_ARG(centroid && area && guided && src && off && nbr && scale && out, "null argument");
    PCD_CHECK_ARG(nf < (1ll << 31) && total < (1ll << 31), "fp32 path: int32 indices");
    hipStream_t st = as_stream(stream);
    float4 *c4 = nullptr, *g4 = nullptr, *s4 = nullptr, *o4 = nullptr;
    StreamTemps tt(st);                    // freed on every exit path
    PCD_HIP(tt.alloc(&c4, nf * sizeof(float4)));
    PCD_HIP(tt.alloc(&g4, nf * sizeof(float4)));
    PCD_HIP(tt.alloc(&s4, nf * sizeof(float4)));
    PCD_HIP(tt.alloc(&o4, nf * sizeof(float4)));
    const dim3 grd((unsigned)cdiv(nf, 256)), blk(256);
    hipLaunchKernelGGL(k_rows3_to4, grd, blk, 0, st, centroid, nf, c4);
    hipLaunchKernelGGL(k_rows3_to4, grd, blk, 0, st, guided, nf, g4);
    hipLaunchKernelGGL(k_rows3w_to4, grd, blk, 0, st, src, area, nf, s4);
    hipLaunchKernelGGL(k_filter_f32, grd, blk, 0, st, c4, g4, s4, nf, off, nbr, sigma_r, multiple_sigma_s, scale, o4);
    hipLaunchKernelGGL(k_rows4_to3, grd, blk, 0, st, o4, nf, out);
    PCD_LAUNCH_CHECK();
    PCD_HIP(tt.release(false));
    return PCD_OK;
}

// The loop of MeshNormalFiltering.cpp:191-240: normal_iterations times {face geometry of the current mesh, sigma_s,
// one filter pass, vertex_iterations sweeps of the vertex update}.  Stream-ordered: sigma_s stays on the device and
// nothing here waits for the stream.
extern "C" int pcd_mesh_denoise(double* v, int64_t nv, const int64_t* f, int64_t nf, const int64_t* vf,
                                const int64_t* ni, const int64_t* off, const int64_t* nbr, const double* guided,
                                int normal_iterations, int vertex_iterations, double sigma_r, double multiple_sigma_s,
                                double* normals_out, void* stream) {
    PCD_CHECK_ARG(normal_iterations >= 0 && vertex_iterations >= 0, "iteration counts must be >= 0");
    PCD_CHECK_ARG(sigma_r > 0.0 && multiple_sigma_s > 0.0, "sigma_r and multiple_sigma_s must be > 0");
    PCD_CHECK_ARG(nv >= 0 && nf >= 0, "negative size");
    if (nv == 0 || nf == 0 || normal_iterations == 0) return PCD_OK;
    PCD_CHECK_ARG(v && f && vf && ni && off && nbr && normals_out, "null argument");
    PCD_CHECK_ARG(normals_out != guided, "normals_out must not alias guided");
    hipStream_t st = as_stream(stream);
    const int64_t nb = cdiv(nf, 256);
    Carver cv;
    const size_t o_cen = cv.reserve(nf * 3 * sizeof(double)), o_area = cv.reserve(nf * sizeof(double));
    const size_t o_cur = cv.reserve(nf * 3 * sizeof(double)), o_g = cv.reserve(guided ? 0 : nf * 3 * sizeof(double));
    const size_t o_tmp = cv.reserve(nv * 3 * sizeof(double)), o_v0 = cv.reserve(nv * 3 * sizeof(double));
    const size_t o_ps = cv.reserve(nb * sizeof(double)), o_pc = cv.reserve(nb * sizeof(unsigned long long));
    const size_t o_sc = cv.reserve(2 * sizeof(double));
    StreamTemps tt(st);                    // freed on every exit path
    PCD_HIP(tt.alloc(&cv.base, cv.used));
    double *cen = cv.at<double>(o_cen), *area = cv.at<double>(o_area), *cur = cv.at<double>(o_cur);
    double *tmp = cv.at<double>(o_tmp), *v0 = cv.at<double>(o_v0), *scale = cv.at<double>(o_sc);
    const double* g = guided ? guided : cv.at<double>(o_g);
    PCD_HIP(hipMemcpyAsync(v0, v, nv * 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
    const dim3 gf((unsigned)nb), gv((unsigned)cdiv(nv, 256)), blk(256);
    double* buf[2] = {v, tmp};
    int at = 0;
    for (int it = 0; it < normal_iterations; ++it) {
        hipLaunchKernelGGL(k_face_geom, gf, blk, 0, st, buf[at], nv, f, nf, cen, area, cur);
        if (it == 0 && !guided)            // classic bilateral filtering: the input mesh's own normals guide
            PCD_HIP(hipMemcpyAsync(cv.at<double>(o_g), cur, nf * 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
        launch_scale(Lay64{cen, f}, nf, nv, vf, ni, cv.at<double>(o_ps), cv.at<unsigned long long>(o_pc), scale, st);
        hipLaunchKernelGGL(k_filter, gf, blk, 0, st, cen, area, g, it == 0 ? g : cur, nf, off, nbr, sigma_r,
                           multiple_sigma_s, scale, normals_out);
        for (int s = 0; s < vertex_iterations; ++s) {
            hipLaunchKernelGGL(k_mesh_update, gv, blk, 0, st, buf[at], buf[at ^ 1], nv, f, normals_out, vf, ni);
            at ^= 1;
        }
    }
    PCD_LAUNCH_CHECK();
    if (at != 0) PCD_HIP(hipMemcpyAsync(v, tmp, nv * 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL((k_restore_isolated<double, 3, int64_t>), gv, blk, 0, st, v0, v, nv, ni);
    PCD_LAUNCH_CHECK();
    PCD_HIP(tt.release(false));
    return PCD_OK;
}

extern "C" int pcd_mesh_denoise_f32(float* v, int64_t nv, const int32_t* f, int64_t nf, const int32_t* vf,
                                    const int32_t* ni, const int32_t* off, const int32_t* nbr, int64_t total,
                                    const float* guided, int normal_iterations, int vertex_iterations, float sigma_r,
                                    float multiple_sigma_s, float* normals_out, void* stream) {
    PCD_CHECK_ARG(normal_iterations >= 0 && vertex_iterations >= 0, "iteration counts must be >= 0");
    PCD_CHECK_ARG(sigma_r > 0.f && multiple_sigma_s > 0.f, "sigma_r and multiple_sigma_s must be > 0");
    PCD_CHECK_ARG(nv >= 0 && nf >= 0 && total >= 0, "negative size");
    if (nv == 0 || nf == 0 || normal_iterations == 0) return PCD_OK;
    PCD_CHECK_ARG(v && f && vf && ni && off && nbr && normals_out, "null argument");
    PCD_CHECK_ARG(nv < (1ll << 31) && 3 * nf < (1ll << 31) && total < (1ll << 31), "fp32 path: int32 indices");
    hipStream_t st = as_stream(stream);
    const int64_t nb = cdiv(nf, 256);
    Carver cv;
    const size_t o_a = cv.reserve(nv * sizeof(float4)), o_b = cv.reserve(nv * sizeof(float4));
    const size_t o_v0 = cv.reserve(nv * sizeof(float4)), o_f4 = cv.reserve(nf * sizeof(int4));
    const size_t o_cen = cv.reserve(nf * sizeof(float4)), o_g = cv.reserve(nf * sizeof(float4));
    const size_t o_cur = cv.reserve(nf * sizeof(float4)), o_out = cv.reserve(nf * sizeof(float4));
    const size_t o_ps = cv.reserve(nb * sizeof(double)), o_pc = cv.reserve(nb * sizeof(unsigned long long));
    const size_t o_sc = cv.reserve(2 * sizeof(double));
    StreamTemps tt(st);                    // freed on every exit path
    PCD_HIP(tt.alloc(&cv.base, cv.used));
    float4 *a = cv.at<float4>(o_a), *v0 = cv.at<float4>(o_v0), *cen = cv.at<float4>(o_cen), *g4 = cv.at<float4>(o_g);
    float4 *cur = cv.at<float4>(o_cur), *out = cv.at<float4>(o_out);
    int4* f4 = cv.at<int4>(o_f4);
    double* scale = cv.at<double>(o_sc);
    const dim3 gf((unsigned)nb), gv((unsigned)cdiv(nv, 256)), blk(256);
    hipLaunchKernelGGL(k_rows3_to4, gv, blk, 0, st, v, nv, a);
    PCD_HIP(hipMemcpyAsync(v0, a, nv * sizeof(float4), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_faces_to4<int32_t>, gf, blk, 0, st, f, nf, f4);
    if (guided) hipLaunchKernelGGL(k_rows3_to4, gf, blk, 0, st, guided, nf, g4);
    float4* buf[2] = {a, cv.at<float4>(o_b)};
    int at = 0;
    for (int it = 0; it < normal_iterations; ++it) {
        hipLaunchKernelGGL(k_face_geom_f32, gf, blk, 0, st, buf[at], f4, nf, cen, cur);
        if (it == 0) {
            if (guided) hipLaunchKernelGGL(k_src_from_guidance, gf, blk, 0, st, g4, nf, cur);
            else PCD_HIP(hipMemcpyAsync(g4, cur, nf * sizeof(float4), hipMemcpyDeviceToDevice, st));
        }
        launch_scale(Lay32{cen, f4}, nf, nv, vf, ni, cv.at<double>(o_ps), cv.at<unsigned long long>(o_pc), scale, st);
        hipLaunchKernelGGL(k_filter_f32, gf, blk, 0, st, cen, g4, cur, nf, off, nbr, sigma_r, multiple_sigma_s, scale, out);
        for (int s = 0; s < vertex_iterations; ++s) {
            hipLaunchKernelGGL(k_mesh_update_f32, gv, blk, 0, st, buf[at], buf[at ^ 1], nv, f4, out, vf, ni);
            at ^= 1;
        }
    }
    hipLaunchKernelGGL((k_restore_isolated<float, 4, int32_t>), gv, blk, 0, st, (const float*)v0, (float*)buf[at], nv, ni);
    hipLaunchKernelGGL(k_rows4_to3, gv, blk, 0, st, buf[at], nv, v);
    hipLaunchKernelGGL(k_rows4_to3, gf, blk, 0, st, out, nf, normals_out);
    PCD_LAUNCH_CHECK();
    PCD_HIP(tt.release(false));
    return PCD_OK;
}
