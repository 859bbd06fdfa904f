// DGCNN in train(): conv1-7 with batch-statistic batch norms and the max / mean pooling, forward and backward
// (GCNModel.py:170-207 with self.training, and what loss.backward() of NetworkController.py:135 does to it).
//
//   pack_edge_kernel        conv weight [Cout][2 Cin] -> [W_a ; W_b - W_a] as [Cin][2 Cout] (forward) and [2 Cout][Cin]
//                           (data gradient), on the stream: an optimiser step never sends a weight to the host.
//   edge_stats_kernel       per channel sum and sum of squares of y = A[nbr] + B over a chunk of patches, in double
//   row_stats_kernel        the same over the rows of conv7's product
//   bn_finalize_kernel      chunk partials, in chunk order -> (mu, var, 1 / sigma), (s, t), running buffers
//   edge_train_kernel       edge_kernel of the forward plus the arg-max slot (first maximal, one byte); the edge value,
//                           the affine and the max in double, rounded once
//   pool_train_kernel       conv7: affine (double), LeakyReLU, max (first arg-max node) and mean over the 64 nodes
//   *_bwd_reduce_kernel     d beta, d gamma partials per chunk, in double
//   bn_bwd_finalize_kernel  partials in chunk order -> d beta, d gamma
//   reverse_lists_kernel    the edges of a patch grouped by their target node, (i, j) order kept
//   edge_bwd_apply_kernel   dy on every edge -> dB (a row's own list) and dA (the target's incoming edges, in order)
//   pool_bwd_apply_kernel   conv7: dY in place of Y
//   wgrad_kernel            dW [M][K] = sum_n dY[M][n] X[K][n] on the exact-f32 MFMA, the reduction over patches split
//                           across workgroups into partial tiles; wgrad_reduce_kernel adds them in split order
//
// No float atomics; every sum has a fixed order that depends on b alone.  The forward products run on gemm_kernel<8>
// (dgcnn.hip: float32 chains of 8 k joined in double, rounded once -- the batch norms of a small batch multiply the
// forward's rounding by up to 1 / sqrt(eps)); the data gradients W^T dY on the forward's own gemm_kernel<0> with the
// add-into-Y epilogue.  -ffp-contract=off stays: fmaf where a fused multiply-add is meant.
// On the host an edge layer is three named views: where it reads and writes (EdgeLayer, pcd_dgcnn.h: the inference
// pass's wiring), what it keeps from forward to backward (EdgeState) and the scratch all layers share (EdgeScratch);
// the whole step carves them from the caller's workspace, the single-layer stage entries from a temporary allocation.
#include <math.h>

#include <algorithm>

#include "pcd_dgcnn.h"
#include "pcd_host.h"

using namespace pcd;
using namespace pcd::dgcnn;

namespace {

constexpr int CHUNK = 8;             // patches per partial of the batch statistics

// An edge value y = A[j] + B[i] and its normalised z = s y + t are formed in double from the stored float32 products
// and the double statistics (s = gamma / sigma, t = beta - s mu), and rounded once where they are stored: the forward,
// the statistics and the backward all see the same y and the same sign of z.
__device__ __forceinline__ double edge_y(float a, float b) { return (double)a + (double)b; }
__device__ __forceinline__ double affine(double y, double s, double t) { return fma(s, y, t); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);   // a fixed tree; every lane ends with the same bits
    return v;
}
// part [chunk][C][2]: the wave's two sums (lane = threadIdx.x & 63) are chunk blockIdx.x's partial of channel c
__device__ __forceinline__ void put_partial(double* part, int C, int c, double s, double q) {
    s = wave_sum(s);
    q = wave_sum(q);
    if ((threadIdx.x & 63) == 0) {
        part[((int64_t)blockIdx.x * C + c) * 2] = s;
        part[((int64_t)blockIdx.x * C + c) * 2 + 1] = q;
    }
}

// W [Cout][2 Cin] -> Wt [Cin][2 Cout] and Ws [2 Cout][Cin] (null: not wanted) of [W_a ; W_b - W_a]
__global__ void pack_edge_kernel(const float* W, int Cin, int Cout, float* Wt, float* Ws) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= Cin * Cout) return;
    const int c = e / Cin, k = e % Cin;
    const float wa = W[(int64_t)c * 2 * Cin + k];
    const float wd = W[(int64_t)c * 2 * Cin + Cin + k] - wa;
    Wt[(int64_t)k * 2 * Cout + c] = wa;
    Wt[(int64_t)k * 2 * Cout + Cout + c] = wd;
    if (Ws) {
        Ws[(int64_t)c * Cin + k] = wa;
        Ws[(int64_t)(Cout + c) * Cin + k] = wd;
    }
}

// part [chunk][C][2]: sum and sum of squares of y over the chunk's edges (lane = row i, a wave per channel)
__global__ __launch_bounds__(256) void edge_stats_kernel(const float* P, int Cout, const int32_t* lists, int kk, int64_t b,
                                                         double* part) {
    const int i = threadIdx.x & 63, c = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= Cout) return;
    const int64_t p0 = (int64_t)blockIdx.x * CHUNK, p1 = min(b, p0 + CHUNK);
    double s = 0.0, q = 0.0;
    for (int64_t p = p0; p < p1; ++p) {
        const float* A = P + (p * 2 * Cout + c) * NODES;
        const float Bi = A[(int64_t)Cout * NODES + i];
        const int32_t* row = lists + (p * NODES + i) * kk;
        for (int j = 0; j < kk; ++j) {
            const double y = edge_y(A[row[j] & 63], Bi);
            s += y;
            q = fma(y, y, q);
        }
    }
    put_partial(part, Cout, c, s, q);
}

// the same over Y [b][C][64]
__global__ __launch_bounds__(256) void row_stats_kernel(const float* Y, int C, int64_t b, double* part) {
    const int i = threadIdx.x & 63, c = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= C) return;
    const int64_t p0 = (int64_t)blockIdx.x * CHUNK, p1 = min(b, p0 + CHUNK);
    double s = 0.0, q = 0.0;
    for (int64_t p = p0; p < p1; ++p) {
        const double y = (double)Y[(p * C + c) * NODES + i];
        s += y;
        q = fma(y, y, q);
    }
    put_partial(part, C, c, s, q);
}

struct BnArgs {               // one batch norm (bn_params) and, from run_finalize, its statistics' partials and results
    const double* part;
    int nchunks, C;
    double N, eps, momentum;
    const float *gamma, *beta;
    float *rmean, *rvar;     // nullable: not updated
    int64_t* tracked;        // nullable
    double* stat;            // [3][C]: mu, biased var, 1 / sqrt(var + eps)
    double* sti;             // [2][C]: s = gamma / sigma, t = beta - s mu
};

__global__ void bn_finalize_kernel(BnArgs a) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.C) return;
    double s = 0.0, q = 0.0;
    for (int ch = 0; ch < a.nchunks; ++ch) {
        s += a.part[((int64_t)ch * a.C + c) * 2];
        q += a.part[((int64_t)ch * a.C + c) * 2 + 1];
    }
    const double mu = s / a.N;
    double var = q / a.N - mu * mu;
    if (var < 0.0) var = 0.0;
    const double istd = 1.0 / sqrt(var + a.eps);
    const double sc = (double)a.gamma[c] * istd;
    a.stat[c] = mu;
    a.stat[a.C + c] = var;
    a.stat[2 * a.C + c] = istd;
    a.sti[c] = sc;
    a.sti[a.C + c] = (double)a.beta[c] - sc * mu;
    if (a.rmean) a.rmean[c] = (float)((1.0 - a.momentum) * (double)a.rmean[c] + a.momentum * mu);
    if (a.rvar) a.rvar[c] = (float)((1.0 - a.momentum) * (double)a.rvar[c] + a.momentum * (var * (a.N / (a.N - 1.0))));
    if (c == 0 && a.tracked) *a.tracked += 1;
}

// out[c][i] = lrelu(max_j (s_c (A[c][nbr(i, j)] + B[c][i]) + t_c)), the max taken in double; arg: the first maximal slot
__global__ __launch_bounds__(256) void edge_train_kernel(const float* P, int Cout, const int32_t* lists, int kk,
                                                         const double* sti, float* out, int64_t ogs, uint8_t* arg,
                                                         int64_t ags) {
    const int i = threadIdx.x & 63, c = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= Cout) return;
    const int64_t p = blockIdx.x;
    const float* A = P + (p * 2 * Cout + c) * NODES;
    const float Bi = A[(int64_t)Cout * NODES + i];
    const double sc = sti[c], tc = sti[Cout + c];
    const int32_t* row = lists + (p * NODES + i) * kk;
    double m = -INFINITY;
    int at = 0;
    for (int j = 0; j < kk; ++j) {
        const double v = affine(edge_y(A[row[j] & 63], Bi), sc, tc);
        if (v > m || (v != v && m == m)) {               // a NaN wins once, as torch's max keeps it
            m = v;
            at = j;
        }
    }
    out[p * ogs + (int64_t)c * NODES + i] = lrelu((float)m);
    arg[p * ags + (int64_t)c * NODES + i] = (uint8_t)at;
}

// (value, node) ordered: the greater value, then the lower node; a NaN above every number
__device__ __forceinline__ bool takes(float ov, int oi, float v, int i) {
    const bool on = ov != ov, vn = v != v;
    if (on != vn) return on;
    if (on) return oi < i;
    return ov > v || (ov == v && oi < i);
}

// Y [b][C][64] -> pooled [b][2 C] (max, then mean of lrelu(s y + t)), arg7 [b][C] the first arg-max node
__global__ __launch_bounds__(256) void pool_train_kernel(const float* Y, int C, const double* sti, float* pooled,
                                                         uint8_t* arg7) {
    const int i = threadIdx.x & 63, c = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= C) return;
    const int64_t p = blockIdx.x;
    const float v = lrelu((float)affine((double)Y[(p * C + c) * NODES + i], sti[c], sti[C + c]));
    float m = v;
    double sum = (double)v;
    int at = i;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(m, off);
        const int oi = __shfl_xor(at, off);
        if (takes(ov, oi, m, at)) {
            m = ov;
            at = oi;
        }
        sum += __shfl_xor(sum, off);
    }
    if (i == 0) {
        pooled[p * 2 * C + c] = m;
        pooled[p * 2 * C + C + c] = (float)(sum * (1.0 / NODES));
        arg7[p * C + c] = (uint8_t)at;
    }
}

// ------------------------------------------------------------------------------------------------ backward
// part [chunk][C][2]: sum of dz*, sum of dz* yhat* over the chunk's rows
__global__ __launch_bounds__(256) void edge_bwd_reduce_kernel(const float* P, int Cout, const int32_t* lists, int kk,
                                                              const uint8_t* arg, int64_t ags, const float* g, int64_t ggs,
                                                              const double* stat, const double* sti, int64_t b,
                                                              double* part) {
    const int i = threadIdx.x & 63, c = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= Cout) return;
    const int64_t p0 = (int64_t)blockIdx.x * CHUNK, p1 = min(b, p0 + CHUNK);
    const double sc = sti[c], tc = sti[Cout + c];
    const double mu = stat[c], istd = stat[2 * Cout + c];
    double sb = 0.0, sg = 0.0;
    for (int64_t p = p0; p < p1; ++p) {
        const float* A = P + (p * 2 * Cout + c) * NODES;
        const float Bi = A[(int64_t)Cout * NODES + i];
        const int js = min((int)arg[p * ags + (int64_t)c * NODES + i], kk - 1);
        const double y = edge_y(A[lists[(p * NODES + i) * kk + js] & 63], Bi);
        const float gz = g[p * ggs + (int64_t)c * NODES + i];
        const float dz = (float)affine(y, sc, tc) > 0.f ? gz : 0.2f * gz;
        sb += (double)dz;
        sg = fma((double)dz, (y - mu) * istd, sg);
    }
    put_partial(part, Cout, c, sb, sg);
}

// conv7: dz[p][c][i] = (gmax [i = arg7] + gmean / 64) lrelu'(s y + t); dpooled [b][2 C]
__device__ __forceinline__ float pool_dz(float y, int i, int at, float gmax, float gmean, double sc, double tc) {
    const float gz = (i == at ? gmax : 0.f) + gmean * (1.f / NODES);
    return (float)affine((double)y, sc, tc) > 0.f ? gz : 0.2f * gz;
}

__global__ __launch_bounds__(256) void pool_bwd_reduce_kernel(const float* Y, int C, const uint8_t* arg7,
                                                              const float* dpooled, const double* stat, const double* sti,
                                                              int64_t b, double* part) {
    const int i = threadIdx.x & 63, c = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= C) return;
    const int64_t p0 = (int64_t)blockIdx.x * CHUNK, p1 = min(b, p0 + CHUNK);
    const double sc = sti[c], tc = sti[C + c];
    const double mu = stat[c], istd = stat[2 * C + c];
    double sb = 0.0, sg = 0.0;
    for (int64_t p = p0; p < p1; ++p) {
        const float y = Y[(p * C + c) * NODES + i];
        const float dz = pool_dz(y, i, arg7[p * C + c], dpooled[p * 2 * C + c], dpooled[p * 2 * C + C + c], sc, tc);
        sb += (double)dz;
        sg = fma((double)dz, ((double)y - mu) * istd, sg);
    }
    put_partial(part, C, c, sb, sg);
}

// partials in chunk order -> dstat [2][C] (d beta, d gamma, double) and the float gradients
__global__ void bn_bwd_finalize_kernel(const double* part, int nchunks, int C, double* dstat, float* dgamma, float* dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double sb = 0.0, sg = 0.0;
    for (int ch = 0; ch < nchunks; ++ch) {
        sb += part[((int64_t)ch * C + c) * 2];
        sg += part[((int64_t)ch * C + c) * 2 + 1];
    }
    dstat[c] = sb;
    dstat[C + c] = sg;
    dbeta[c] = (float)sb;
    dgamma[c] = (float)sg;
}

// Y [b][C][64] -> dY in place: s (dz - d beta / N - yhat d gamma / N)
__global__ __launch_bounds__(256) void pool_bwd_apply_kernel(float* Y, int C, const uint8_t* arg7, const float* dpooled,
                                                             const double* stat, const double* sti, const double* dstat,
                                                             double invN) {
    const int i = threadIdx.x & 63, c = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= C) return;
    const int64_t p = blockIdx.x;
    const double sc = sti[c], tc = sti[C + c];
    const double mu = stat[c], istd = stat[2 * C + c];
    const double k1 = dstat[c] * invN, k2 = dstat[C + c] * invN;
    float* at = Y + (p * C + c) * NODES + i;
    const float y = *at;
    const float dz = pool_dz(y, i, arg7[p * C + c], dpooled[p * 2 * C + c], dpooled[p * 2 * C + C + c], sc, tc);
    *at = (float)(sc * (((double)dz - k1) - ((double)y - mu) * istd * k2));
}

// lists [b][64][kk] -> rev_off [b][65], rev [b][64 kk]: the edges (i << 8 | j) grouped by target, (i, j) order kept
__global__ __launch_bounds__(64) void reverse_lists_kernel(const int32_t* lists, int kk, int32_t* rev_off, int32_t* rev) {
    __shared__ uint8_t L[NODES * NODES];
    __shared__ int cnt[NODES + 1];
    const int64_t p = blockIdx.x;
    const int v = threadIdx.x, E = NODES * kk;
    for (int e = v; e < E; e += NODES) L[e] = (uint8_t)(lists[p * E + e] & 63);
    __syncthreads();
    int n = 0;
    for (int e = 0; e < E; ++e) n += L[e] == v ? 1 : 0;
    cnt[v + 1] = n;
    __syncthreads();
    if (v == 0) {
        cnt[0] = 0;
        for (int t = 1; t <= NODES; ++t) cnt[t] += cnt[t - 1];
    }
    __syncthreads();
    int o = cnt[v];
    rev_off[p * (NODES + 1) + v] = o;
    if (v == NODES - 1) rev_off[p * (NODES + 1) + NODES] = cnt[NODES];
    int e = 0;
    for (int i = 0; i < NODES; ++i)
        for (int j = 0; j < kk; ++j, ++e)
            if (L[e] == v) rev[p * E + o++] = (i << 8) | j;
}

// dP [b][2 Cout][64]: dA rows, then dB rows
__global__ __launch_bounds__(256) void edge_bwd_apply_kernel(const float* P, int Cout, const int32_t* lists, int kk,
                                                             const int32_t* rev_off, const int32_t* rev,
                                                             const uint8_t* arg, int64_t ags, const float* g, int64_t ggs,
                                                             const double* stat, const double* sti, const double* dstat,
                                                             double invN, float* dP) {
    __shared__ float Bs[4][NODES];
    __shared__ float dzs[4][NODES];
    __shared__ uint8_t jss[4][NODES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int cr = blockIdx.y * 4 + w;
    const bool live = cr < Cout;
    const int c = live ? cr : 0;
    const int64_t p = blockIdx.x;
    const float* A = P + (p * 2 * Cout + c) * NODES;
    const float Av = A[lane], Bi = A[(int64_t)Cout * NODES + lane];
    const double sc = sti[c], tc = sti[Cout + c];
    const double mu = stat[c], istd = stat[2 * Cout + c];
    const double k1 = dstat[c] * invN, k2 = dstat[Cout + c] * invN;
    const int32_t* row = lists + (p * NODES + lane) * kk;
    const int js = min((int)arg[p * ags + (int64_t)c * NODES + lane], kk - 1);
    const double ys = edge_y(A[row[js] & 63], Bi);
    const float gz = g[p * ggs + (int64_t)c * NODES + lane];
    const float dz = (float)affine(ys, sc, tc) > 0.f ? gz : 0.2f * gz;
    Bs[w][lane] = Bi;
    dzs[w][lane] = dz;
    jss[w][lane] = (uint8_t)js;
    __syncthreads();
    // dB: lane = row i over its own list
    double accB = 0.0;
    for (int j = 0; j < kk; ++j) {
        const double yh = (edge_y(A[row[j] & 63], Bi) - mu) * istd;
        accB += ((j == js ? (double)dz : 0.0) - k1) - yh * k2;
    }
    // dA: lane = target v over its incoming edges
    double accA = 0.0;
    const int32_t* ro = rev_off + p * (NODES + 1);
    const int32_t* rv = rev + p * NODES * kk;
    const int e1 = ro[lane + 1];
    for (int e = ro[lane]; e < e1; ++e) {
        const int ij = rv[e], i = (ij >> 8) & 63, j = ij & 255;
        const double yh = (edge_y(Av, Bs[w][i]) - mu) * istd;
        accA += ((j == jss[w][i] ? (double)dzs[w][i] : 0.0) - k1) - yh * k2;
    }
    if (live) {
        dP[(p * 2 * Cout + c) * NODES + lane] = (float)(sc * accA);
        dP[(p * 2 * Cout + Cout + c) * NODES + lane] = (float)(sc * accB);
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
constexpr int WM = 128, WK = 64, WN = 32;
// LDS row strides (floats), = 33 mod 64: the 32 n rows a wave writes land in 32 banks, and the two n rows an MFMA
// reads fall in different bank halves but for one bank
constexpr int WLA = 161, WLB = 97;

struct WgradArgs {
    const float* dY;         // dY(m, n) = dY[(n / 64) * ygs + m * 64 + n % 64]
    const float* X;          // X(k, n)  = X[(n / 64) * xgs + k * 64 + n % 64]
    float* part;             // [splits][M][K]
    int64_t ygs, xgs, b, pps;
    int M, K;
};

__global__ __launch_bounds__(256) void wgrad_kernel(WgradArgs a) {
    __shared__ float As[WN * WLA];   // [n][m]
    __shared__ float Bs[WN * WLB];   // [n][k]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 32;
    const int m0 = blockIdx.y * WM, k0 = blockIdx.z * WK;
    const int64_t p0 = (int64_t)blockIdx.x * a.pps, p1 = min(a.b, p0 + a.pps);
    const int nn = tid & 31, r0 = tid >> 5;              // this thread moves column nn of rows r0 + 8 r
    const int arow = lane >> 5, acol = lane & 31;
    f32x16 acc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = 0.f;
    for (int64_t p = p0; p < p1; ++p) {
        for (int h = 0; h < NODES; h += WN) {
            float wr[16], xr[8];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + r0 + 8 * r;
                wr[r] = m < a.M ? a.dY[p * a.ygs + (int64_t)m * NODES + h + nn] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int k = k0 + r0 + 8 * r;
                xr[r] = k < a.K ? a.X[p * a.xgs + (int64_t)k * NODES + h + nn] : 0.f;
            }
            __syncthreads();                             // the previous step's MFMA reads are done
#pragma unroll
            for (int r = 0; r < 16; ++r) As[nn * WLA + r0 + 8 * r] = wr[r];
#pragma unroll
            for (int r = 0; r < 8; ++r) Bs[nn * WLB + r0 + 8 * r] = xr[r];
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < WN; kk += 2) {
                const float a0 = As[(kk + arow) * WLA + wm + acol];
                const float a1 = As[(kk + arow) * WLA + wm + 32 + acol];
                const float bv = Bs[(kk + arow) * WLB + wn + acol];
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc[1], 0, 0, 0);
            }
        }
    }
    const int k = k0 + wn + acol;
    float* out = a.part + (int64_t)blockIdx.x * a.M * a.K;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = mfma_row(m0 + wm + 32 * h, r, arow);
            if (m < a.M && k < a.K) out[(int64_t)m * a.K + k] = acc[h][r];
        }
    }
}

// mode 0: out [M][K] = sum over splits, in split order.  mode 1 (M = 2 Cout, rows dW_A then dW_B of the split weight):
// out [Cout][2 K] = [dW_A - dW_B | dW_B], the gradient of the module's [Cout][2 Cin] weight
__global__ void wgrad_reduce_kernel(const float* part, int splits, int M, int K, float* out, int mode) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t MK = (int64_t)M * K;
    if (mode == 0) {
        if (e >= MK) return;
        float s = 0.f;
        for (int sp = 0; sp < splits; ++sp) s += part[sp * MK + e];
        out[e] = s;
    } else {
        const int Cout = M / 2;
        if (e >= (int64_t)Cout * K) return;
        const int64_t c = e / K, k = e % K;
        float sa = 0.f, sd = 0.f;
        for (int sp = 0; sp < splits; ++sp) {
            sa += part[sp * MK + e];
            sd += part[sp * MK + (int64_t)Cout * K + e];
        }
        out[c * 2 * K + k] = sa - sd;
        out[c * 2 * K + K + k] = sd;
    }
}

// ------------------------------------------------------------------------------------------------ host side
// patches per split of the weight gradient's reduction: at most 32 partial tiles, 4 patches or more each
int64_t wgrad_pps(int64_t b) {
    const int64_t s = std::max<int64_t>(1, std::min<int64_t>(32, cdiv(b, 4)));
    return std::max<int64_t>(1, cdiv(b, s));
}
int64_t wgrad_splits(int64_t b) { return std::max<int64_t>(1, cdiv(b, wgrad_pps(b))); }

// a: dY, ygs, M, X, xgs, K and part are the caller's; out [M][K] (mode 0) or [M / 2][2 K] (mode 1)
int run_wgrad(WgradArgs a, int64_t b, float* out, int mode, hipStream_t st) {
    a.b = b;
    a.pps = wgrad_pps(b);
    const int splits = (int)wgrad_splits(b);
    hipLaunchKernelGGL(wgrad_kernel, dim3((unsigned)splits, (unsigned)cdiv(a.M, WM), (unsigned)cdiv(a.K, WK)), dim3(256), 0,
                       st, a);
    PCD_LAUNCH_CHECK();
    const int64_t n = mode == 0 ? (int64_t)a.M * a.K : (int64_t)(a.M / 2) * a.K;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, a.part, splits, a.M, a.K, out,
                       mode);
    PCD_LAUNCH_CHECK();
    return PCD_OK;
}

BnArgs bn_params(const float* gamma, const float* beta, float* rmean, float* rvar, int64_t* tracked, double eps,
                 double momentum) {
    BnArgs a{};
    a.gamma = gamma; a.beta = beta; a.rmean = rmean; a.rvar = rvar; a.tracked = tracked; a.eps = eps; a.momentum = momentum;
    return a;
}

int run_finalize(BnArgs a, const double* part, int64_t b, int C, double N, double* stat, double* sti, hipStream_t st) {
    a.part = part; a.nchunks = (int)cdiv(b, CHUNK); a.C = C; a.N = N; a.stat = stat; a.sti = sti;
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((unsigned)cdiv(C, 64)), dim3(64), 0, st, a);
    PCD_LAUNCH_CHECK();
    return PCD_OK;
}

struct EdgeState {           // what an edge layer keeps between its forward and its backward
    float *Wt, *Ws;          // the split weight [W_a ; W_b - W_a]: [Cin][2 Cout] (forward), [2 Cout][Cin] (data gradient)
    float* P;                // [b][2 Cout][64]: A rows, then B rows
    uint8_t* arg;            // [b][Cout][64], patch stride ags: the arg-max slot of every output
    int64_t ags;
    double *stat, *sti;      // [3][Cout]: mu, biased var, 1 / sqrt(var + eps); [2][Cout]: s, t
};
struct EdgeScratch {         // shared by all layers
    double *part, *dstat;    // [chunks][C][2]; [2][C]: d beta, d gamma
    float *dP, *wpart;       // [b][2 Cout][64]; [splits][2 Cout][Cin]
    int32_t *rev_off, *rev;  // the reversed lists of the layer at hand
};
struct EdgeGrads {           // g = dL/d out laid out as out is; dX (null: not wanted) as X is, added into or stored
    const float* g;
    float *dgamma, *dbeta, *dW, *dX;
    bool add;
};

// edge layer forward: X -> P = [A ; B], statistics, out (patch stride e.ogs) and the arg-max bytes
int edge_forward(const EdgeLayer& e, const EdgeState& s, const EdgeScratch& scr, const BnArgs& bn, float* out, int64_t b,
                 hipStream_t st) {
    const int Cout = e.Cout;
    int rc = conv_gemm(s.Wt, 2 * Cout, e.Cin, e.X, e.xgs, s.P, (int64_t)2 * Cout * NODES, b, EPI_PLAIN, true, st);
    if (rc != PCD_OK) return rc;
    const dim3 chunks((unsigned)cdiv(b, CHUNK), (unsigned)cdiv(Cout, 4));
    hipLaunchKernelGGL(edge_stats_kernel, chunks, dim3(256), 0, st, s.P, Cout, e.lists, e.kk, b, scr.part);
    PCD_LAUNCH_CHECK();
    if ((rc = run_finalize(bn, scr.part, b, Cout, (double)b * NODES * e.kk, s.stat, s.sti, st)) != PCD_OK) return rc;
    hipLaunchKernelGGL(edge_train_kernel, dim3((unsigned)b, (unsigned)cdiv(Cout, 4)), dim3(256), 0, st, s.P, Cout, e.lists,
                       e.kk, s.sti, out, e.ogs, s.arg, s.ags);
    PCD_LAUNCH_CHECK();
    return PCD_OK;
}

// edge layer backward: gr.g -> d gamma, d beta, scr.dP = [dA ; dB], dW (module layout), dX
int edge_backward(const EdgeLayer& e, const EdgeState& s, const EdgeScratch& scr, const EdgeGrads& gr, int64_t b,
                  hipStream_t st) {
    const int Cin = e.Cin, Cout = e.Cout;
    const dim3 chunks((unsigned)cdiv(b, CHUNK), (unsigned)cdiv(Cout, 4));
    hipLaunchKernelGGL(edge_bwd_reduce_kernel, chunks, dim3(256), 0, st, s.P, Cout, e.lists, e.kk, s.arg, s.ags, gr.g, e.ogs,
                       s.stat, s.sti, b, scr.part);
    PCD_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)cdiv(Cout, 64)), dim3(64), 0, st, scr.part,
                       (int)cdiv(b, CHUNK), Cout, scr.dstat, gr.dgamma, gr.dbeta);
    PCD_LAUNCH_CHECK();
    const double invN = 1.0 / ((double)b * NODES * e.kk);
    hipLaunchKernelGGL(edge_bwd_apply_kernel, dim3((unsigned)b, (unsigned)cdiv(Cout, 4)), dim3(256), 0, st, s.P, Cout, e.lists,
                       e.kk, scr.rev_off, scr.rev, s.arg, s.ags, gr.g, e.ogs, s.stat, s.sti, scr.dstat, invN, scr.dP);
    PCD_LAUNCH_CHECK();
    if (gr.dX) {   // dX (+)= [W_a ; W_b - W_a]^T dP: the split weight [2 Cout][Cin] is the GEMM's transposed operand
        const int rc = conv_gemm(s.Ws, Cin, 2 * Cout, scr.dP, (int64_t)2 * Cout * NODES, gr.dX, e.xgs, b,
                                 gr.add ? EPI_ADD : EPI_PLAIN, false, st);
        if (rc != PCD_OK) return rc;
    }
    WgradArgs a{};
    a.dY = scr.dP; a.ygs = (int64_t)2 * Cout * NODES; a.M = 2 * Cout;
    a.X = e.X; a.xgs = e.xgs; a.K = Cin; a.part = scr.wpart;
    return run_wgrad(a, b, gr.dW, 1, st);
}

int run_reverse(const int32_t* lists, int kk, int32_t* rev_off, int32_t* rev, int64_t b, hipStream_t st) {
    hipLaunchKernelGGL(reverse_lists_kernel, dim3((unsigned)b), dim3(64), 0, st, lists, kk, rev_off, rev);
    PCD_LAUNCH_CHECK();
    return PCD_OK;
}

// The whole step (TrainWs) and the single-layer stage entries (StageWs) carve their per-layer state and the shared
// scratch with the same two functions.
EdgeState carve_edge(Carver& c, int Cin, int Cout, int64_t b) {
    EdgeState s{};
    s.Wt = c.carve<float>((int64_t)2 * Cin * Cout * 4);
    s.Ws = c.carve<float>((int64_t)2 * Cin * Cout * 4);
    s.P = c.carve<float>(b * 2 * Cout * NODES * 4);
    s.arg = c.carve<uint8_t>(b * Cout * NODES);
    s.ags = (int64_t)Cout * NODES;
    s.stat = c.carve<double>((int64_t)3 * Cout * 8);
    s.sti = c.carve<double>((int64_t)2 * Cout * 8);
    return s;
}
// C channels at most, P_rows rows of dP, lists of kk at most, wfloats floats per partial of the weight gradient
EdgeScratch carve_scratch(Carver& c, int64_t b, int C, int P_rows, int kk, int64_t wfloats) {
    EdgeScratch s{};
    s.part = c.carve<double>(cdiv(b, CHUNK) * C * 2 * 8);
    s.dstat = c.carve<double>((int64_t)2 * C * 8);
    s.dP = c.carve<float>(b * P_rows * NODES * 4);
    s.wpart = c.carve<float>(wgrad_splits(b) * wfloats * 4);
    s.rev_off = c.carve<int32_t>(b * (NODES + 1) * 4);
    s.rev = c.carve<int32_t>(b * NODES * kk * 4);
    return s;
}

struct TrainWs {
    EdgeState edge[kMaxEdge];
    EdgeScratch scr;
    float *wpt, *cat, *dcat; // the pooled convolution's weight transposed [Ccat][emb]; the concatenation [b][Ccat][64]
                             // and its gradient
    float* Yp;               // [b][emb][64]: the pooled convolution's product, then its gradient
    uint8_t* argp;           // [b][emb]
    double *statp, *stip;    // as an edge layer's
    int32_t *idx3, *knn, *flag;   // [b][64][3], [l_d][b][64][k], [1]
    int64_t total;           // bytes
};
TrainWs tlayout(const Net& n, int64_t b, void* ws) {
    TrainWs w{};
    Carver c{ws};
    int64_t wfloats = (int64_t)n.emb * n.Ccat;
    for (int l = 0; l < n.E; ++l) {
        w.edge[l] = carve_edge(c, n.Cin[l], n.Cout[l], b);
        wfloats = std::max(wfloats, (int64_t)2 * n.Cout[l] * n.Cin[l]);
    }
    w.wpt = c.carve<float>((int64_t)n.Ccat * n.emb * 4);
    w.cat = c.carve<float>(b * n.cat_stride() * 4);
    w.dcat = c.carve<float>(b * n.cat_stride() * 4);
    w.idx3 = c.carve<int32_t>(b * NODES * 3 * 4);
    w.knn = c.carve<int32_t>((int64_t)n.l_d * b * NODES * n.k * 4);
    w.Yp = c.carve<float>(b * n.emb * NODES * 4);
    w.argp = c.carve<uint8_t>(b * n.emb);
    w.statp = c.carve<double>((int64_t)3 * n.emb * 8);
    w.stip = c.carve<double>((int64_t)2 * n.emb * 8);
    w.scr = carve_scratch(c, b, std::max(n.Cmax, n.emb), 2 * n.Cmax, std::max(3, n.k), wfloats);
    w.flag = c.carve<int32_t>(4);
    w.total = c.used;
    return w;
}

int check_batch(int64_t b) {
    PCD_CHECK_ARG(b >= 0 && b <= kMaxBatch, "b must be in [0, 2^20]");
    return PCD_OK;
}
int table_net(const pcd_dgcnn_table* t, Net* n) {
    PCD_CHECK_ARG(t != nullptr, "table is null");
    return make_net(n, t->l_e, t->l_d, t->l_l, t->channel_sizes, t->k, t->init_dims, t->output_channels,
                    PCD_BDGCNN_HEAD_SLOPE);
}

int check_ws(const TrainWs& w, const void* workspace, int64_t bytes) {
    PCD_CHECK_ARG(workspace != nullptr && bytes >= w.total,
                  "workspace of " + std::to_string(bytes) + " bytes is shorter than the " + std::to_string(w.total) +
                      " that pcd_dgcnn_train_workspace_bytes asks for");
    PCD_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "workspace must be 16-byte aligned");
    return PCD_OK;
}

// the parameters and gradients of either entry: arrays of E + 1
struct ParamView {
    const float *const *conv_w, *const *bn_weight, *const *bn_bias;
    float *const *bn_mean, *const *bn_var;
    int64_t* const* bn_tracked;
    const double *bn_eps, *bn_momentum;
};
struct GradView {
    float *const *conv_w, *const *bn_weight, *const *bn_bias;
};

int train_forward_impl(const Net& n, const ParamView& prm, const float* inputs, int64_t b, float* pooled,
                       void* workspace, int64_t workspace_bytes, int32_t* lists_out, void* stream) {
    int rc = check_batch(b);
    if (rc != PCD_OK) return rc;
    PCD_CHECK_ARG(b >= 1, "b must be >= 1 (batch statistics of an empty batch do not exist)");
    PCD_CHECK_ARG(inputs != nullptr && pooled != nullptr, "inputs / pooled is null");
    const int E = n.E, emb = n.emb;
    for (int l = 0; l <= E; ++l) {
        const std::string name = std::to_string(l + 1);
        PCD_CHECK_ARG(prm.conv_w[l] != nullptr, "conv" + name + " weight is null");
        PCD_CHECK_ARG(prm.bn_weight[l] != nullptr && prm.bn_bias[l] != nullptr, "bn" + name + " weight / bias is null");
        PCD_CHECK_ARG((prm.bn_mean[l] != nullptr) == (prm.bn_var[l] != nullptr),
                      "bn" + name + ": running_mean and running_var go together");
        PCD_CHECK_ARG(prm.bn_eps[l] >= 0.0, "bn" + name + " eps is invalid");
        PCD_CHECK_ARG(prm.bn_momentum[l] >= 0.0 && prm.bn_momentum[l] <= 1.0, "bn" + name + " momentum must be in [0, 1]");
    }
    const TrainWs w = tlayout(n, b, workspace);
    if ((rc = check_ws(w, workspace, workspace_bytes)) != PCD_OK) return rc;
    hipStream_t st = as_stream(stream);

    // the index columns first: a bad one ends the call before anything is computed or a buffer updated (a table
    // without static layers never reads them)
    if (n.l_e > 0) {
        int bad;
        if ((rc = index_lists_checked(inputs, b, w.idx3, w.flag, &bad, st)) != PCD_OK) return rc;
        PCD_CHECK_ARG(bad == kNoBadPatch, "patch " + std::to_string(bad) +
                                          " has an index column (rows 17:20) outside [0, 63] or NaN; nothing written");
    }
    for (int l = 0; l < E; ++l)
        if ((rc = pack_edge(prm.conv_w[l], n.Cin[l], n.Cout[l], w.edge[l].Wt, w.edge[l].Ws, st)) != PCD_OK) return rc;
    if ((rc = transpose(prm.conv_w[E], emb, n.Ccat, w.wpt, st)) != PCD_OK) return rc;

    auto bn_of = [&](int l) {
        return bn_params(prm.bn_weight[l], prm.bn_bias[l], prm.bn_mean[l], prm.bn_var[l], prm.bn_tracked[l],
                         prm.bn_eps[l], prm.bn_momentum[l]);
    };
    for (int l = 0; l < E; ++l) {
        const EdgeLayer e = edge_layer(n, l, inputs, w.cat, w.idx3, w.knn, b);
        if (e.knn && (rc = knn(e.X, e.xgs, e.Cin, e.kk, e.knn, b, st)) != PCD_OK) return rc;
        if ((rc = edge_forward(e, w.edge[l], w.scr, bn_of(l), w.cat + e.out_off, b, st)) != PCD_OK) return rc;
    }
    {   // the pooled convolution: the product is stored (the backward turns it into dY in place), then statistics and
        // pooling
        rc = conv_gemm(w.wpt, emb, n.Ccat, w.cat, n.cat_stride(), w.Yp, (int64_t)emb * NODES, b, EPI_PLAIN, true, st);
        if (rc != PCD_OK) return rc;
        const dim3 chunks((unsigned)cdiv(b, CHUNK), (unsigned)cdiv(emb, 4));
        hipLaunchKernelGGL(row_stats_kernel, chunks, dim3(256), 0, st, w.Yp, emb, b, w.scr.part);
        PCD_LAUNCH_CHECK();
        rc = run_finalize(bn_of(E), w.scr.part, b, emb, (double)b * NODES, w.statp, w.stip, st);
        if (rc != PCD_OK) return rc;
        hipLaunchKernelGGL(pool_train_kernel, dim3((unsigned)b, (unsigned)cdiv(emb, 4)), dim3(256), 0, st, w.Yp, emb,
                           w.stip, pooled, w.argp);
        PCD_LAUNCH_CHECK();
    }
    if (lists_out && n.l_d > 0)
        PCD_HIP(hipMemcpyAsync(lists_out, w.knn, (int64_t)n.l_d * b * NODES * n.k * 4, hipMemcpyDeviceToDevice, st));
    return PCD_OK;
}

int train_backward_impl(const Net& n, const float* inputs, int64_t b, const float* d_pooled, const float* pool_w,
                        void* workspace, int64_t workspace_bytes, const GradView& grads, void* stream) {
    int rc = check_batch(b);
    if (rc != PCD_OK) return rc;
    PCD_CHECK_ARG(b >= 1, "b must be >= 1");
    PCD_CHECK_ARG(inputs != nullptr && d_pooled != nullptr && pool_w != nullptr,
                  "inputs / d_pooled / the pooled convolution's weight is null");
    const int E = n.E, emb = n.emb;
    for (int l = 0; l <= E; ++l)
        PCD_CHECK_ARG(grads.conv_w[l] && grads.bn_weight[l] && grads.bn_bias[l],
                      "gradient " + std::to_string(l + 1) + " has a null pointer");
    const TrainWs w = tlayout(n, b, workspace);
    if ((rc = check_ws(w, workspace, workspace_bytes)) != PCD_OK) return rc;
    hipStream_t st = as_stream(stream);
    const EdgeScratch& scr = w.scr;
    {   // the pooled convolution: pooling, LeakyReLU and batch norm, dY in place of the stored product
        const dim3 chunks((unsigned)cdiv(b, CHUNK), (unsigned)cdiv(emb, 4));
        hipLaunchKernelGGL(pool_bwd_reduce_kernel, chunks, dim3(256), 0, st, w.Yp, emb, w.argp, d_pooled, w.statp, w.stip, b,
                           scr.part);
        PCD_LAUNCH_CHECK();
        hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)cdiv(emb, 64)), dim3(64), 0, st, scr.part,
                           (int)cdiv(b, CHUNK), emb, scr.dstat, grads.bn_weight[E], grads.bn_bias[E]);
        PCD_LAUNCH_CHECK();
        hipLaunchKernelGGL(pool_bwd_apply_kernel, dim3((unsigned)b, (unsigned)cdiv(emb, 4)), dim3(256), 0, st, w.Yp, emb,
                           w.argp, d_pooled, w.statp, w.stip, scr.dstat, 1.0 / ((double)b * NODES));
        PCD_LAUNCH_CHECK();
        // dcat = W^T dY: W [emb][Ccat] itself is the GEMM's transposed operand; every slice's first contribution
        rc = conv_gemm(pool_w, n.Ccat, emb, w.Yp, (int64_t)emb * NODES, w.dcat, n.cat_stride(), b, EPI_PLAIN, false, st);
        if (rc != PCD_OK) return rc;
        WgradArgs a{};
        a.dY = w.Yp; a.ygs = (int64_t)emb * NODES; a.M = emb;
        a.X = w.cat; a.xgs = n.cat_stride(); a.K = n.Ccat; a.part = scr.wpart;
        if ((rc = run_wgrad(a, b, grads.conv_w[E], 0, st)) != PCD_OK) return rc;
    }
    const int32_t* reversed = nullptr;   // the lists scr.rev holds: the static layers share theirs
    for (int l = E - 1; l >= 0; --l) {
        const EdgeLayer e = edge_layer(n, l, inputs, w.cat, w.idx3, w.knn, b);
        if (e.lists != reversed) {
            if ((rc = run_reverse(e.lists, e.kk, scr.rev_off, scr.rev, b, st)) != PCD_OK) return rc;
            reversed = e.lists;
        }
        // the gradient of a slice of cat is that slice of dcat, which already holds the pooled convolution's
        // contribution: this layer's is added second.  The network's inputs take none.
        EdgeGrads gr{};
        gr.g = w.dcat + e.out_off; gr.dX = e.X == inputs ? nullptr : w.dcat + (e.X - w.cat); gr.add = true;
        gr.dgamma = grads.bn_weight[l]; gr.dbeta = grads.bn_bias[l]; gr.dW = grads.conv_w[l];
        if ((rc = edge_backward(e, w.edge[l], scr, gr, b, st)) != PCD_OK) return rc;
    }
    return PCD_OK;
}

}  // namespace

namespace pcd {
namespace dgcnn {
int pack_edge(const float* W, int Cin, int Cout, float* Wt, float* Ws, hipStream_t st) {
    hipLaunchKernelGGL(pack_edge_kernel, dim3((unsigned)cdiv(Cin * Cout, 256)), dim3(256), 0, st, W, Cin, Cout, Wt, Ws);
    PCD_LAUNCH_CHECK();
    return PCD_OK;
}
}  // namespace dgcnn
}  // namespace pcd

extern "C" {

int pcd_dgcnn_train_workspace_bytes(int k, int emb_dims, int64_t b, int64_t* bytes) {
    PCD_CHECK_ARG(bytes != nullptr, "bytes is null");
    Net n;
    int rc = fixed_net(&n, k, emb_dims, 1);
    if (rc != PCD_OK || (rc = check_batch(b)) != PCD_OK) return rc;
    *bytes = tlayout(n, b, nullptr).total;
    return PCD_OK;
}

int pcd_dgcnn_train_forward(const pcd_dgcnn_train_params* prm, int k, int emb_dims, const float* inputs, int64_t b,
                            float* pooled, void* workspace, int64_t workspace_bytes, int32_t* lists_out, void* stream) {
    PCD_CHECK_ARG(prm != nullptr, "params is null");
    Net n;
    const int rc = fixed_net(&n, k, emb_dims, 1);
    if (rc != PCD_OK) return rc;
    const ParamView v{prm->conv_w, prm->bn_weight, prm->bn_bias, prm->bn_mean, prm->bn_var, prm->bn_tracked, prm->bn_eps,
                      prm->bn_momentum};
    return train_forward_impl(n, v, inputs, b, pooled, workspace, workspace_bytes, lists_out, stream);
}

int pcd_dgcnn_train_backward(int k, int emb_dims, const float* inputs, int64_t b, const float* d_pooled,
                             const float* conv7_w, void* workspace, int64_t workspace_bytes,
                             const pcd_dgcnn_train_grads* grads, void* stream) {
    Net n;
    const int rc = fixed_net(&n, k, emb_dims, 1);
    if (rc != PCD_OK) return rc;
    PCD_CHECK_ARG(grads != nullptr, "grads is null");
    const GradView v{grads->conv_w, grads->bn_weight, grads->bn_bias};
    return train_backward_impl(n, inputs, b, d_pooled, conv7_w, workspace, workspace_bytes, v, stream);
}

int pcd_bdgcnn_train_workspace_bytes(const pcd_dgcnn_table* table, int64_t b, int64_t* bytes) {
    PCD_CHECK_ARG(bytes != nullptr, "bytes is null");
    Net n;
    int rc = table_net(table, &n);
    if (rc != PCD_OK || (rc = check_batch(b)) != PCD_OK) return rc;
    *bytes = tlayout(n, b, nullptr).total;
    return PCD_OK;
}

int pcd_bdgcnn_train_forward(const pcd_dgcnn_table* table, const pcd_bdgcnn_train_params* prm, const float* inputs,
                             int64_t b, float* pooled, void* workspace, int64_t workspace_bytes, int32_t* lists_out,
                             void* stream) {
    Net n;
    const int rc = table_net(table, &n);
    if (rc != PCD_OK) return rc;
    PCD_CHECK_ARG(prm != nullptr, "params is null");
    PCD_CHECK_ARG(prm->conv_w && prm->bn_weight && prm->bn_bias && prm->bn_mean && prm->bn_var && prm->bn_tracked &&
                      prm->bn_eps && prm->bn_momentum, "params has a null array");
    const ParamView v{prm->conv_w, prm->bn_weight, prm->bn_bias, prm->bn_mean, prm->bn_var, prm->bn_tracked, prm->bn_eps,
                      prm->bn_momentum};
    return train_forward_impl(n, v, inputs, b, pooled, workspace, workspace_bytes, lists_out, stream);
}

int pcd_bdgcnn_train_backward(const pcd_dgcnn_table* table, const float* inputs, int64_t b, const float* d_pooled,
                              const float* pool_conv_w, void* workspace, int64_t workspace_bytes,
                              const pcd_bdgcnn_train_grads* grads, void* stream) {
    Net n;
    const int rc = table_net(table, &n);
    if (rc != PCD_OK) return rc;
    PCD_CHECK_ARG(grads != nullptr, "grads is null");
    PCD_CHECK_ARG(grads->conv_w && grads->bn_weight && grads->bn_bias, "grads has a null array");
    const GradView v{grads->conv_w, grads->bn_weight, grads->bn_bias};
    return train_backward_impl(n, inputs, b, d_pooled, pool_conv_w, workspace, workspace_bytes, v, stream);
}

int pcd_dgcnn_wgrad_split(int64_t b, int64_t* patches_per_split) {
    PCD_CHECK_ARG(patches_per_split != nullptr, "patches_per_split is null");
    PCD_CHECK_ARG(b >= 0 && b <= kMaxBatch, "b must be in [0, 2^20]");
    *patches_per_split = wgrad_pps(b);
    return PCD_OK;
}

int pcd_dgcnn_wgrad(const float* dy, const float* x, int m_rows, int k_cols, int64_t b, float* dw, void* stream) {
    PCD_CHECK_ARG(m_rows >= 1 && k_cols >= 1, "M and K must be >= 1");
    PCD_CHECK_ARG(m_rows <= (1 << 16) && k_cols <= (1 << 16), "M and K must be <= 65536");
    PCD_CHECK_ARG(b >= 1 && b <= kMaxBatch, "b must be in [1, 2^20]");
    PCD_CHECK_ARG(dy != nullptr && x != nullptr && dw != nullptr, "dy / x / dw is null");
    hipStream_t st = as_stream(stream);
    StreamTemps tmp(st);
    WgradArgs a{};
    a.dY = dy; a.ygs = (int64_t)m_rows * NODES; a.M = m_rows;
    a.X = x; a.xgs = (int64_t)k_cols * NODES; a.K = k_cols;
    PCD_HIP(tmp.alloc(&a.part, wgrad_splits(b) * (int64_t)m_rows * k_cols * sizeof(float)));
    const int rc = run_wgrad(a, b, dw, 0, st);
    if (rc != PCD_OK) return rc;
    PCD_HIP(tmp.release());
    return PCD_OK;
}

// the edge stage's scratch: one allocation, carved as the whole step's workspace is
namespace {
struct StageWs {
    EdgeState edge;
    EdgeScratch scr;
    int64_t total;
};
struct StageDims { int Cin, Cout; };
StageWs slayout(StageDims d, int n, int64_t b, void* ws) {
    StageWs w{};
    Carver c{ws};
    w.edge = carve_edge(c, d.Cin, d.Cout, b);
    w.scr = carve_scratch(c, b, d.Cout, 2 * d.Cout, n, (int64_t)2 * d.Cout * d.Cin);
    w.total = c.used;
    return w;
}
// the arguments of a stage entry; d: edge layer `layer` (1-based) of the fixed network
int check_stage(int layer, int64_t b, int n, StageDims* d) {
    Net net;
    const int rc = fixed_net(&net, 1, 1, 1);
    if (rc != PCD_OK) return rc;
    PCD_CHECK_ARG(layer >= 1 && layer <= net.E, "layer must be in [1, 6]");
    PCD_CHECK_ARG(b >= 1 && b <= kMaxBatch, "b must be in [1, 2^20]");
    PCD_CHECK_ARG(n >= 1 && n <= NODES, "list_len must be in [1, 64]");
    *d = {net.Cin[layer - 1], net.Cout[layer - 1]};
    return PCD_OK;
}
}  // namespace

int pcd_dgcnn_edgeconv_train(const float* w, const float* gamma, const float* beta, double eps, double momentum,
                             float* running_mean, float* running_var, int64_t* tracked, int layer, const float* x,
                             int64_t b, const int32_t* lists, int list_len, float* out, uint8_t* argmax, double* stats,
                             void* stream) {
    StageDims d;
    int rc = check_stage(layer, b, list_len, &d);
    if (rc != PCD_OK) return rc;
    PCD_CHECK_ARG(w && gamma && beta && x && lists && out && argmax && stats, "a pointer is null");
    PCD_CHECK_ARG((running_mean != nullptr) == (running_var != nullptr), "running_mean and running_var go together");
    PCD_CHECK_ARG(eps >= 0.0 && momentum >= 0.0 && momentum <= 1.0, "eps / momentum is invalid");
    hipStream_t st = as_stream(stream);
    StreamTemps tmp(st);
    char* ws;
    PCD_HIP(tmp.alloc(&ws, slayout(d, list_len, b, nullptr).total));
    const StageWs sw = slayout(d, list_len, b, ws);
    EdgeState s = sw.edge;
    s.arg = argmax;          // the caller's, [b][Cout][64] as the carved ones are
    s.stat = stats;
    if ((rc = pack_edge(w, d.Cin, d.Cout, s.Wt, s.Ws, st)) != PCD_OK) return rc;
    const BnArgs bn = bn_params(gamma, beta, running_mean, running_var, tracked, eps, momentum);
    rc = edge_forward(edge_layer_alone(d.Cin, d.Cout, x, lists, list_len), s, sw.scr, bn, out, b, st);
    if (rc != PCD_OK) return rc;
    PCD_HIP(tmp.release());
    return PCD_OK;
}

int pcd_dgcnn_edgeconv_train_backward(const float* w, const float* gamma, const float* beta, double eps, int layer,
                                      const float* x, int64_t b, const int32_t* lists, int list_len, const float* g,
                                      float* dab, float* dgamma, float* dbeta, float* dw, float* dx, void* stream) {
    StageDims d;
    int rc = check_stage(layer, b, list_len, &d);
    if (rc != PCD_OK) return rc;
    PCD_CHECK_ARG(w && gamma && beta && x && lists && g && dab && dgamma && dbeta && dw, "a pointer is null");
    PCD_CHECK_ARG(eps >= 0.0, "eps is invalid");
    hipStream_t st = as_stream(stream);
    StreamTemps tmp(st);
    char* ws;
    PCD_HIP(tmp.alloc(&ws, slayout(d, list_len, b, nullptr).total + (int64_t)b * d.Cout * NODES * 4));
    const StageWs sw = slayout(d, list_len, b, ws);
    float* out = at<float>(ws, sw.total);
    const EdgeLayer e = edge_layer_alone(d.Cin, d.Cout, x, lists, list_len);
    const EdgeState& s = sw.edge;
    EdgeScratch scr = sw.scr;
    scr.dP = dab;            // the caller's
    if ((rc = pack_edge(w, d.Cin, d.Cout, s.Wt, s.Ws, st)) != PCD_OK) return rc;
    const BnArgs bn = bn_params(gamma, beta, nullptr, nullptr, nullptr, eps, 0.0);
    // the forward again (no buffer is touched), then the backward on what it left
    if ((rc = edge_forward(e, s, scr, bn, out, b, st)) != PCD_OK) return rc;
    if ((rc = run_reverse(lists, list_len, scr.rev_off, scr.rev, b, st)) != PCD_OK) return rc;
    EdgeGrads gr{};
    gr.g = g; gr.dX = dx; gr.add = false;
    gr.dgamma = dgamma; gr.dbeta = dbeta; gr.dW = dw;
    if ((rc = edge_backward(e, s, scr, gr, b, st)) != PCD_OK) return rc;
    PCD_HIP(tmp.release());
    return PCD_OK;
}

}  // extern "C"
