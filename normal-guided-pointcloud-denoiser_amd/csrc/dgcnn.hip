// The DGCNN / BetterDGCNN forward pass (inference, fp32): GCNModel.py:121-297 of the reference as five kernels over a
// runtime layer table (pcd_dgcnn.h: Net; DGCNN is the fixed instance of it).
//
//   gemm_kernel    Y = W . X on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain per output), 128 x 64
//                  tiles, W shared by all patches, X the patches' columns.  Epilogues: plain store, per-row affine
//                  (+ LeakyReLU 0.2), or affine + LeakyReLU + max / mean over the 64 columns of a patch (conv7:
//                  [b, emb, 64] is never stored); or added into Y (the data gradients of csrc/dgcnn_train.hip).
//                  gemm_kernel<0> is the inference kernel; gemm_kernel<8> (train-mode forward products) joins float32
//                  chains of 8 k in double.
//   index_kernel   the three index columns (floats) -> int32 lists, truncating as .long() does; a value outside
//                  [0, 63] or a NaN is clamped to 0 and the lowest such patch raised in a device flag.
//   knn_kernel     one workgroup per patch: 64 x 64 squared distances of the layer's input, the k smallest per row,
//                  ascending, ties to the lower index (self included, as topk includes it).
//   edge_kernel    out[c, i] = lrelu(max_j s_c (A[c, j] + B[c, i]) + t_c) over row i's list, where A = W_a X and
//                  B = (W_b - W_a) X come from one GEMM: W [x_j - x_i ; x_i] = W_a x_j + (W_b - W_a) x_i.
//   fused_edge_kernel   that GEMM and edge_kernel in one launch for a layer with 2 Cout <= 128: the patch's [A ; B]
//                  tile stays in LDS (BetterDGCNN's narrow layers; DGCNN keeps the two kernels).  The same bits.
//   gemm_bf16_kernel, fused_edge_bf16_kernel   the opt-in bf16-operand mode (pcd_dgcnn_set_operands): the conv-form
//                  GEMM and the fused layer on v_mfma_f32_32x32x16_bf16 -- operands rounded to bf16, float32 sums,
//                  the float32 epilogues unchanged.  Edge layers with Cin >= 32 and the pooled convolution use them;
//                  the first layer, the head, the searches and train() stay float32.
//
// Every output element depends on its own patch only and is summed in a fixed order: a patch's output bits do not
// depend on the batch, its place in it, or the run.  No float atomics.  The library's -ffp-contract=off stays; where a
// fused multiply-add is meant the code says fmaf (or is the MFMA).
// The layer table, an edge layer's wiring (edge_layer) and the workspace carver are in pcd_dgcnn.h, shared with
// csrc/dgcnn_train.hip, which also launches this file's GEMM, k-NN, index and transpose kernels through pcd::dgcnn.
#include <limits.h>
#include <math.h>

#include <vector>

#include "pcd_dgcnn.h"
#include "pcd_host.h"

using namespace pcd;
using namespace pcd::dgcnn;

namespace {

constexpr int BM = 128, BN = 64, BK = 32;
// LDS row strides (floats) of the W and X tiles: = 32 mod 64, so the two k rows an MFMA reads fall in different bank halves
constexpr int LDA = 160, LDB = 96;

struct GemmArgs {
    const float* Wt;        // [K][M]: the weight, transposed (rows are contiguous in m)
    const float* X;         // X(k, n) = X[(n / G) * xgs + k * xks + n % G]
    float* Y;               // Y(m, n) = Y[(n / G) * ygs + m * yms + n % G]
    const float* s;         // [M] (affine epilogues)
    const float* t;
    float* poolT;           // EPI_POOL: [2 M][b]  (max rows, then mean rows)
    float* pool_dbg;        // EPI_POOL, nullable: [b][2 M]
    int64_t N, G, xgs, xks, ygs, yms, b;
    int M, K, epi;
    float slope;            // of the LeakyReLU epilogues
};

// max that keeps a NaN (torch's max does)
__device__ __forceinline__ float nanmax(float a, float b) { return (b > a || b != b) ? b : a; }

// FLUSH = 0: the forward's kernel, one float32 chain over all of K.  FLUSH > 0 (the train-mode forward products, whose
// rounding the batch norms of a small batch amplify): every FLUSH k the MFMA accumulators are added into double
// accumulators and cleared, so no float32 chain is longer than FLUSH terms; plain epilogue only.
template <int FLUSH>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs a) {
    // K-tiles of W [BK][BM] and X [BK][BN]; afterwards the pooling epilogue's [BM][65] staging
    __shared__ float lds[BM * 65];
    static_assert(BM * 65 >= BK * (LDA + LDB), "the pooling staging must cover the k tiles");
    float* As = lds;
    float* Bs = lds + BK * LDA;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 32;   // a wave owns 64 x 32: two 32 x 32 accumulators sharing b
    const int m0 = blockIdx.y * BM;
    const int64_t n0 = (int64_t)blockIdx.x * BN;
    // global -> LDS: this thread always moves column tid & 127 of the W tile (rows (tid >> 7) + 2 r) and column
    // tid & 63 of the X tile (rows (tid >> 6) + 4 r)
    const int wcol = tid & 127, wrow0 = tid >> 7, xcol = tid & 63, xrow0 = tid >> 6;
    const int mg = m0 + wcol;
    const int64_t ng = n0 + xcol;
    const bool m_ok = mg < a.M, n_ok = ng < a.N;
    const int64_t xoff = n_ok ? (ng / a.G) * a.xgs + ng % a.G : 0;
    float wr[16], xr[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = k0 + wrow0 + 2 * r;
            wr[r] = (m_ok && k < a.K) ? a.Wt[(int64_t)k * a.M + mg] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int k = k0 + xrow0 + 4 * r;
            xr[r] = (n_ok && k < a.K) ? a.X[xoff + (int64_t)k * a.xks] : 0.f;
        }
    };
    f32x16 acc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = 0.f;
    double wide[FLUSH > 0 ? 2 : 1][FLUSH > 0 ? 16 : 1];
    if constexpr (FLUSH > 0) {
        static_assert(FLUSH % 2 == 0 && BK % FLUSH == 0, "a K tile is a whole number of flushes");
#pragma unroll
        for (int r = 0; r < 16; ++r) wide[0][r] = wide[1][r] = 0.0;
    }
    fetch(0);
    const int arow = lane >> 5, acol = lane & 31;
    for (int k0 = 0; k0 < a.K; k0 += BK) {
#pragma unroll
        for (int r = 0; r < 16; ++r) As[(wrow0 + 2 * r) * LDA + wcol] = wr[r];
#pragma unroll
        for (int r = 0; r < 8; ++r) Bs[(xrow0 + 4 * r) * LDB + xcol] = xr[r];
        __syncthreads();
        if (k0 + BK < a.K) fetch(k0 + BK);
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            const float a0 = As[(kk + arow) * LDA + wm + acol];
            const float a1 = As[(kk + arow) * LDA + wm + 32 + acol];
            const float bv = Bs[(kk + arow) * LDB + wn + acol];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc[1], 0, 0, 0);
            if constexpr (FLUSH > 0) {
                if ((kk + 2) % FLUSH == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        wide[0][r] += (double)acc[0][r];
                        wide[1][r] += (double)acc[1][r];
                        acc[0][r] = acc[1][r] = 0.f;
                    }
                }
            }
        }
        __syncthreads();
    }
    if constexpr (FLUSH > 0) {                         // (every tile ends on a flush: the float accumulators are zero)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[0][r] = (float)wide[0][r];
            acc[1][r] = (float)wide[1][r];
        }
    }
    const int cn = wn + acol;
    const int64_t n = n0 + cn;
    float* Ps = lds;                                   // EPI_POOL: [BM][65] staging (every wave is past the k loop)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rm = mfma_row(wm + 32 * h, r, arow);
            const int m = m0 + rm;
            float v = acc[h][r];
            if (a.epi != EPI_PLAIN && a.epi != EPI_ADD && m < a.M) {
                v = fmaf(a.s[m], v, a.t[m]);
                if (a.epi != EPI_AFFINE) v = lrelu(v, a.slope);
            }
            if (a.epi == EPI_POOL) {
                Ps[rm * 65 + cn] = v;
            } else if (m < a.M && n < a.N) {
                float* y = a.Y + (n / a.G) * a.ygs + (int64_t)m * a.yms + n % a.G;
                *y = a.epi == EPI_ADD ? *y + v : v;
            }
        }
    }
    if (a.epi != EPI_POOL) return;
    __syncthreads();
    // one row per 4 threads, 16 columns each in column order, then ((q0 + q1) + (q2 + q3)): a fixed-order sum
    const int q = tid & 3;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int pr = half * 64 + (tid >> 2);
        float sum = 0.f, mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const float v = Ps[pr * 65 + q * 16 + c];
            sum += v;
            mx = nanmax(mx, v);
        }
        sum += __shfl_xor(sum, 1);
        mx = nanmax(mx, __shfl_xor(mx, 1));
        sum += __shfl_xor(sum, 2);
        mx = nanmax(mx, __shfl_xor(mx, 2));
        const int m = m0 + pr;
        if (q == 0 && m < a.M) {
            const int64_t p = blockIdx.x;              // G == BN: one patch per column tile
            const float mean = sum * (1.f / NODES);
            a.poolT[(int64_t)m * a.b + p] = mx;
            a.poolT[((int64_t)a.M + m) * a.b + p] = mean;
            if (a.pool_dbg) {
                a.pool_dbg[p * 2 * a.M + m] = mx;
                a.pool_dbg[p * 2 * a.M + a.M + m] = mean;
            }
        }
    }
}

__global__ void transpose_kernel(const float* W, int M, int K, float* Wt) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)M * K) return;
    const int k = (int)(e / M), m = (int)(e % M);
    Wt[e] = W[(int64_t)m * K + k];
}

// inputs [b][20][64] -> lists [b][64][3]; flag: lowest patch with an index column outside [0, 63] (or NaN)
__global__ void index_kernel(const float* inputs, int64_t b, int32_t* lists, int* flag, int patch_base) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= b * NODES * 3) return;
    const int64_t p = e / (NODES * 3);
    const int rem = (int)(e % (NODES * 3));
    const int c = rem / NODES, i = rem % NODES;
    const float f = inputs[p * (20 * NODES) + (17 + c) * NODES + i];
    const bool ok = f > -1.0f && f < 64.0f;            // (int)f in [0, 63]; a NaN fails both
    lists[(p * NODES + i) * 3 + c] = ok ? (int)f : 0;
    if (!ok) atomicMin(flag, patch_base + (int)p);
}

// x [b] patches of [C][64] (patch stride xgs floats) -> lists [b][64][k]
__global__ __launch_bounds__(256) void knn_kernel(const float* x, int64_t xgs, int C, int k, int32_t* lists) {
    __shared__ float Xs[64 * NODES];
    __shared__ float Ds[NODES * 65];
    const int tid = threadIdx.x, i = tid & 63, j0 = (tid >> 6) * 16;
    const float* xp = x + (int64_t)blockIdx.x * xgs;
    float acc[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) acc[jj] = 0.f;
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int cc = min(64, C - c0);
        for (int e = tid; e < cc * NODES; e += 256) Xs[e] = xp[(int64_t)c0 * NODES + e];
        __syncthreads();
        for (int c = 0; c < cc; ++c) {
            const float xi = Xs[c * NODES + i];
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) {
                const float d = xi - Xs[c * NODES + j0 + jj];
                acc[jj] = fmaf(d, d, acc[jj]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) Ds[i * 65 + j0 + jj] = acc[jj] != acc[jj] ? INFINITY : acc[jj];   // NaN sorts last
    __syncthreads();
    // (distance, index) is a strict total order, so the ranks of a row are a permutation of 0..63
    int rank[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) rank[jj] = 0;
    for (int j = 0; j < NODES; ++j) {
        const float d = Ds[i * 65 + j];
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
            const float dj = Ds[i * 65 + j0 + jj];
            rank[jj] += (d < dj || (d == dj && j < j0 + jj)) ? 1 : 0;
        }
    }
    int32_t* out = lists + ((int64_t)blockIdx.x * NODES + i) * k;
#pragma unroll
    for (int jj = 0; jj < 16; ++jj)
        if (rank[jj] < k) out[rank[jj]] = j0 + jj;
}

// P [b][2 Cout][64] (A rows, then B rows) -> out[c][i] = lrelu(max_j fmaf(s_c, A[c][j] + B[c][i], t_c))
__global__ __launch_bounds__(256) void edge_kernel(const float* P, int Cout, const int32_t* lists, int kk, const float* s,
                                                   const float* t, float* out, int64_t ogs) {
    const int i = threadIdx.x & 63, c = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= Cout) return;
    const int64_t p = blockIdx.x;
    const float* A = P + (p * 2 * Cout + c) * NODES;
    const float Bi = A[(int64_t)Cout * NODES + i];
    const float sc = s[c], tc = t[c];
    const int32_t* row = lists + (p * NODES + i) * kk;
    float m = -INFINITY;
    for (int j = 0; j < kk; ++j) {
        const int nb = row[j] & 63;                    // (lists are made by index_kernel / knn_kernel: in range)
        m = nanmax(m, fmaf(sc, A[nb] + Bi, tc));
    }
    out[p * ogs + (int64_t)c * NODES + i] = lrelu(m);
}

// A narrow edge layer (2 Cout <= BM) in one launch: workgroup p forms patch p's whole [A ; B] = Wt^T X tile as
// gemm_kernel<0> does -- its k loop, statement for statement: the same fmaf chain per element -- stages it in LDS as
// the pooling epilogue stages its tile, and applies edge_kernel's max over the lists from there.  P never reaches
// memory; the output is edge_kernel's, bit for bit.
struct FusedEdgeArgs {
    const float* Wt;        // [Cin][2 Cout]
    const float* X;         // [b][Cin][64], patch stride xgs
    const int32_t* lists;   // [b][64][kk]
    const float *s, *t;     // [Cout]
    float* out;             // [b][Cout][64], patch stride ogs
    int64_t xgs, ogs;
    int Cin, Cout, kk;
};

__global__ __launch_bounds__(256) void fused_edge_kernel(FusedEdgeArgs a) {
    __shared__ float lds[BM * 65];                     // the K tiles; afterwards the [BM][65] tile of P
    __shared__ uint8_t nbr[NODES * NODES];             // the patch's lists [64][kk]
    float* As = lds;
    float* Bs = lds + BK * LDA;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 32;
    const int64_t p = blockIdx.x;
    const int M = 2 * a.Cout, K = a.Cin;
    const int wcol = tid & 127, wrow0 = tid >> 7, xcol = tid & 63, xrow0 = tid >> 6;
    const bool m_ok = wcol < M;
    const float* Xp = a.X + p * a.xgs + xcol;
    for (int e = tid; e < NODES * a.kk; e += 256) nbr[e] = (uint8_t)(a.lists[p * NODES * a.kk + e] & 63);
    float wr[16], xr[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = k0 + wrow0 + 2 * r;
            wr[r] = (m_ok && k < K) ? a.Wt[(int64_t)k * M + wcol] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int k = k0 + xrow0 + 4 * r;
            xr[r] = k < K ? Xp[(int64_t)k * NODES] : 0.f;
        }
    };
    f32x16 acc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = 0.f;
    fetch(0);
    const int arow = lane >> 5, acol = lane & 31;
    for (int k0 = 0; k0 < K; k0 += BK) {
#pragma unroll
        for (int r = 0; r < 16; ++r) As[(wrow0 + 2 * r) * LDA + wcol] = wr[r];
#pragma unroll
        for (int r = 0; r < 8; ++r) Bs[(xrow0 + 4 * r) * LDB + xcol] = xr[r];
        __syncthreads();
        if (k0 + BK < K) fetch(k0 + BK);
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            const float a0 = As[(kk + arow) * LDA + wm + acol];
            const float a1 = As[(kk + arow) * LDA + wm + 32 + acol];
            const float bv = Bs[(kk + arow) * LDB + wn + acol];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc[1], 0, 0, 0);
        }
        __syncthreads();
    }
    // the tile to LDS: a lane's 16 registers are 16 rows of one column, so a wave's store covers 32 consecutive
    // columns of two rows 4 apart -- 65 = 1 mod 32: no two lanes of a half-wave meet in a bank
    float* Ps = lds;
    const int cn = wn + acol;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 16; ++r) Ps[mfma_row(wm + 32 * h, r, arow) * 65 + cn] = acc[h][r];
    __syncthreads();
    // edge_kernel from LDS: lane = row i, a wave per channel, four channels a pass
    const uint8_t* row = nbr + lane * a.kk;
    for (int c = wave; c < a.Cout; c += 4) {
        const float* A = Ps + c * 65;
        const float Bi = Ps[(a.Cout + c) * 65 + lane];
        const float sc = a.s[c], tc = a.t[c];
        float m = -INFINITY;
        for (int j = 0; j < a.kk; ++j) m = nanmax(m, fmaf(sc, A[row[j]] + Bi, tc));
        a.out[p * a.ogs + (int64_t)c * NODES + lane] = lrelu(m);
    }
}

// ------------------------------------------------------------------------------- bf16 operands, float32 accumulation
// The opt-in arm of the conv-form GEMM on v_mfma_f32_32x32x16_bf16: the same 128 x 64 output tile (one column tile =
// one patch), K tiles of 64.  The weight is rounded once on the host side of the mode switch into Wb [M][Kp], k
// contiguous and zero-padded to Kp = 8 ceil(K / 8), so a lane's 8-k fragment is one 16-byte load; X stays float32 in
// memory and is rounded (the plain cast: nearest even, NaN and Inf kept) on its way into LDS.  LDS rows are 72 bf16
// (144 bytes = 36 banks): the 16-byte fragment reads of 16 consecutive rows start in 16 different groups of 4 banks.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
constexpr int BKH = 64, LDH = 72;
static_assert(BM * 65 * 4 >= (BM + BN) * LDH * 2, "the pooling staging must cover the bf16 k tiles");

struct GemmBf16Args {
    const __bf16* Wb;       // [M][Kp]
    const float* X;         // [b][K][64], patch stride xgs
    float* Y;               // [b][M][64], patch stride ygs
    const float* s;         // [M] (affine epilogues)
    const float* t;
    float* poolT;           // EPI_POOL: [2 M][b]
    float* pool_dbg;        // EPI_POOL, nullable: [b][2 M]
    int64_t xgs, ygs, b;
    int M, K, Kp, epi;
    float slope;
};

// float32 src(m, k) = src[m * sm + k * sk] -> Wb [M][Kp], zeros for k >= K
__global__ void pack_bf16_kernel(const float* src, int64_t sm, int64_t sk, int M, int K, int Kp, __bf16* Wb) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)M * Kp) return;
    const int m = (int)(e / Kp), k = (int)(e % Kp);
    Wb[e] = k < K ? (__bf16)src[m * sm + k * sk] : (__bf16)0.f;
}

// conv weight W [Cout][2 Cin] -> the float32 [W_a ; W_b - W_a] of pack_edge, rounded, as Wb [2 Cout][Kp]
__global__ void pack_edge_bf16_kernel(const float* W, int Cin, int Cout, int Kp, __bf16* Wb) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)2 * Cout * Kp) return;
    const int m = (int)(e / Kp), k = (int)(e % Kp), c = m < Cout ? m : m - Cout;
    float v = 0.f;
    if (k < Cin) {
        const float wa = W[(int64_t)c * 2 * Cin + k];
        v = m < Cout ? wa : W[(int64_t)c * 2 * Cin + Cin + k] - wa;
    }
    Wb[e] = (__bf16)v;
}

// acc = rows m0 .. m0 + 127 of Wb times patch Xp [K][64]: the k loop both bf16 kernels run, so a fused layer has the
// two-kernel path's bits.  lds: (BM + BN) * LDH bf16.  Every access past M or K is predicated: zeros enter the sum.
__device__ __forceinline__ void bf16_tile(const __bf16* Wb, int M, int K, int Kp, int m0, const float* Xp, __bf16* lds,
                                          f32x16 (&acc)[2]) {
    __bf16* As = lds;                                  // [BM][LDH]
    __bf16* Bs = lds + BM * LDH;                       // [BN][LDH]: X transposed, k contiguous
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 32;
    // global -> LDS: 16-byte chunk tid + 256 r of the W tile (row chunk >> 3, k group chunk & 7); column tid & 63 of
    // the X tile, k groups (tid >> 6) and (tid >> 6) + 4
    const int xcol = tid & 63, xg0 = tid >> 6;
    bf16x8 wr[4];
    float xr[16];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = tid + 256 * r, m = m0 + (c >> 3), k = k0 + (c & 7) * 8;
            bf16x8 z = {};
            wr[r] = (m < M && k < Kp) ? *reinterpret_cast<const bf16x8*>(Wb + (int64_t)m * Kp + k) : z;
        }
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k0 + (xg0 + 4 * g) * 8 + j;
                xr[8 * g + j] = k < K ? Xp[(int64_t)k * NODES + xcol] : 0.f;
            }
    };
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = 0.f;
    fetch(0);
    const int arow = lane >> 5, acol = lane & 31;
    for (int k0 = 0; k0 < K; k0 += BKH) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = tid + 256 * r;
            *reinterpret_cast<bf16x8*>(As + (c >> 3) * LDH + (c & 7) * 8) = wr[r];
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            bf16x8 v;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (__bf16)xr[8 * g + j];
            *reinterpret_cast<bf16x8*>(Bs + xcol * LDH + (xg0 + 4 * g) * 8) = v;
        }
        __syncthreads();
        if (k0 + BKH < K) fetch(k0 + BKH);
#pragma unroll
        for (int ks = 0; ks < BKH; ks += 16) {
            if (k0 + ks >= K) break;                   // (uniform: the rest of the tile is zeros)
            const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(As + (wm + acol) * LDH + ks + 8 * arow);
            const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(As + (wm + 32 + acol) * LDH + ks + 8 * arow);
            const bf16x8 bv = *reinterpret_cast<const bf16x8*>(Bs + (wn + acol) * LDH + ks + 8 * arow);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, bv, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bv, acc[1], 0, 0, 0);
        }
        __syncthreads();
    }
}

// gemm_kernel<0>'s epilogues on the bf16 product (plain, affine, affine + LeakyReLU, pool): float32, the same order
__global__ __launch_bounds__(256) void gemm_bf16_kernel(GemmBf16Args a) {
    __shared__ __attribute__((aligned(16))) float lds[BM * 65];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 32;
    // one patch per column tile; the row tiles of a patch are neighbours in the grid, so they run together and the
    // patch's X is read from memory once (patch-major order streamed X once per row tile: 8 GB for conv7 on 4096
    // patches, which bounded the kernel)
    const int mtiles = (a.M + BM - 1) / BM;
    const int m0 = (int)(blockIdx.x % mtiles) * BM;
    const int64_t p = blockIdx.x / mtiles;
    f32x16 acc[2];
    bf16_tile(a.Wb, a.M, a.K, a.Kp, m0, a.X + p * a.xgs, reinterpret_cast<__bf16*>(lds), acc);
    const int arow = lane >> 5, acol = lane & 31;
    const int cn = wn + acol;
    float* Ps = lds;                                   // EPI_POOL: [BM][65] staging (every wave is past the k loop)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rm = mfma_row(wm + 32 * h, r, arow);
            const int m = m0 + rm;
            float v = acc[h][r];
            if (a.epi != EPI_PLAIN && m < a.M) {
                v = fmaf(a.s[m], v, a.t[m]);
                if (a.epi != EPI_AFFINE) v = lrelu(v, a.slope);
            }
            if (a.epi == EPI_POOL)
                Ps[rm * 65 + cn] = v;
            else if (m < a.M)
                a.Y[p * a.ygs + (int64_t)m * NODES + cn] = v;
        }
    }
    if (a.epi != EPI_POOL) return;
    __syncthreads();
    // one row per 4 threads, 16 columns each in column order, then ((q0 + q1) + (q2 + q3)): a fixed-order sum
    const int q = tid & 3;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int pr = half * 64 + (tid >> 2);
        float sum = 0.f, mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const float v = Ps[pr * 65 + q * 16 + c];
            sum += v;
            mx = nanmax(mx, v);
        }
        sum += __shfl_xor(sum, 1);
        mx = nanmax(mx, __shfl_xor(mx, 1));
        sum += __shfl_xor(sum, 2);
        mx = nanmax(mx, __shfl_xor(mx, 2));
        const int m = m0 + pr;
        if (q == 0 && m < a.M) {
            const float mean = sum * (1.f / NODES);
            a.poolT[(int64_t)m * a.b + p] = mx;
            a.poolT[((int64_t)a.M + m) * a.b + p] = mean;
            if (a.pool_dbg) {
                a.pool_dbg[p * 2 * a.M + m] = mx;
                a.pool_dbg[p * 2 * a.M + a.M + m] = mean;
            }
        }
    }
}

// fused_edge_kernel on the bf16 product: Wb [2 Cout][Kp]
struct FusedEdgeBf16Args {
    const __bf16* Wb;
    const float* X;
    const int32_t* lists;
    const float *s, *t;
    float* out;
    int64_t xgs, ogs;
    int Cin, Kp, Cout, kk;
};

__global__ __launch_bounds__(256) void fused_edge_bf16_kernel(FusedEdgeBf16Args a) {
    __shared__ __attribute__((aligned(16))) float lds[BM * 65];   // the K tiles; afterwards the [BM][65] tile of P
    __shared__ uint8_t nbr[NODES * NODES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 32;
    const int64_t p = blockIdx.x;
    for (int e = tid; e < NODES * a.kk; e += 256) nbr[e] = (uint8_t)(a.lists[p * NODES * a.kk + e] & 63);
    f32x16 acc[2];
    bf16_tile(a.Wb, 2 * a.Cout, a.Cin, a.Kp, 0, a.X + p * a.xgs, reinterpret_cast<__bf16*>(lds), acc);
    float* Ps = lds;
    const int arow = lane >> 5, cn = wn + (lane & 31);
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 16; ++r) Ps[mfma_row(wm + 32 * h, r, arow) * 65 + cn] = acc[h][r];
    __syncthreads();
    const uint8_t* row = nbr + lane * a.kk;
    for (int c = wave; c < a.Cout; c += 4) {
        const float* A = Ps + c * 65;
        const float Bi = Ps[(a.Cout + c) * 65 + lane];
        const float sc = a.s[c], tc = a.t[c];
        float m = -INFINITY;
        for (int j = 0; j < a.kk; ++j) m = nanmax(m, fmaf(sc, A[row[j]] + Bi, tc));
        a.out[p * a.ogs + (int64_t)c * NODES + lane] = lrelu(m);
    }
}

// ---------------------------------------------------------------------------------------------- host side
constexpr int kWideFlush = 8;      // k per float32 chain of the train-mode forward products

int launch_gemm(const GemmArgs& a, hipStream_t st, bool wide = false) {
    if (a.N <= 0 || a.M <= 0) return PCD_OK;
    dim3 grid((unsigned)cdiv(a.N, BN), (unsigned)cdiv(a.M, BM));
    if (wide)
        hipLaunchKernelGGL(gemm_kernel<kWideFlush>, grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(gemm_kernel<0>, grid, dim3(256), 0, st, a);
    PCD_LAUNCH_CHECK();
    return PCD_OK;
}

int launch_gemm_bf16(const GemmBf16Args& a, hipStream_t st) {
    if (a.b <= 0 || a.M <= 0) return PCD_OK;
    // (b <= 2^20 patches x at most 512 row tiles: the grid stays below 2^31)
    hipLaunchKernelGGL(gemm_bf16_kernel, dim3((unsigned)(a.b * cdiv(a.M, BM))), dim3(256), 0, st, a);
    PCD_LAUNCH_CHECK();
    return PCD_OK;
}
int padded_k(int K) { return (K + 7) / 8 * 8; }
// float32 src(m, k) = src[m * sm + k * sk] -> Wb [M][padded_k(K)], rounded to nearest even
int pack_bf16(const float* src, int64_t sm, int64_t sk, int M, int K, __bf16* Wb, hipStream_t st) {
    const int Kp = padded_k(K);
    hipLaunchKernelGGL(pack_bf16_kernel, dim3((unsigned)cdiv((int64_t)M * Kp, 256)), dim3(256), 0, st, src, sm, sk, M,
                       K, Kp, Wb);
    PCD_LAUNCH_CHECK();
    return PCD_OK;
}
GemmBf16Args conv_args_bf16(const __bf16* Wb, int M, int K, const float* X, int64_t xgs, float* Y, int64_t ygs,
                            int64_t b) {
    GemmBf16Args a{};
    a.Wb = Wb; a.X = X; a.Y = Y; a.M = M; a.K = K; a.Kp = padded_k(K); a.b = b; a.xgs = xgs; a.ygs = ygs;
    a.epi = EPI_PLAIN; a.slope = kTrunkSlope;
    return a;
}

// conv form: X [b][K][64] (patch stride xgs) -> Y [b][M][64] (patch stride ygs)
GemmArgs conv_args(const float* Wt, int M, int K, const float* X, int64_t xgs, float* Y, int64_t ygs, int64_t b) {
    GemmArgs a{};
    a.Wt = Wt; a.X = X; a.Y = Y; a.M = M; a.K = K; a.b = b;
    a.N = b * NODES; a.G = NODES; a.xgs = xgs; a.xks = NODES; a.ygs = ygs; a.yms = NODES;
    a.epi = EPI_PLAIN; a.slope = kTrunkSlope;
    return a;
}
// head form: X [K][b] -> Y [M][b]
GemmArgs head_args(const float* Wt, int M, int K, const float* X, float* Y, int64_t b) {
    GemmArgs a{};
    a.Wt = Wt; a.X = X; a.Y = Y; a.M = M; a.K = K; a.b = b;
    a.N = b; a.G = b; a.xgs = 0; a.xks = b; a.ygs = 0; a.yms = b;
    a.epi = EPI_PLAIN; a.slope = kTrunkSlope;
    return a;
}

}  // namespace

struct pcd_dgcnn {
    Net net;
    float* dev = nullptr;          // every packed weight in one allocation
    // transposed weights and folded batch norms (s, t), in network order: the E edge layers [Cin][2 Cout], the pooled
    // convolution [Ccat][emb], the l_l linears; the last linear's (s, t) is (1, bias)
    std::vector<const float*> wt, s, t;
    // PCD_OPERANDS_BF16: the trunk's weights rounded to bf16, [M][padded_k(K)] each, made at the first switch; null
    // for a layer that stays on the float32 kernel
    int operands = PCD_OPERANDS_F32;
    __bf16* dev16 = nullptr;
    std::vector<const __bf16*> wb;
    const __bf16* bf16_weight(int l) const { return operands == PCD_OPERANDS_BF16 ? wb[l] : nullptr; }
};

namespace {

struct Workspace {
    float *cat, *P, *pooled;          // [b][Ccat][64], [b][2 product_rows][64], [2 emb][b]
    float* h[kMaxLin];                // the head's hidden layers [width][b]
    int32_t *idx3, *knn, *flag;       // [b][64][3], [l_d][b][64][k], [1]
    int64_t total;                    // bytes
};
// Where the fused kernel runs when the caller leaves the choice to the library (PCD_FUSED_AUTO): what
// tools/better_dgcnn_probe.py measured -- faster than the two kernels at every list length from 3 to 64 for Cin from
// 17 to 1024, by less the wider the input (1.4 x at Cin = 1024, k = 8).  Wider inputs were not measured and keep the
// two kernels.
constexpr int kFusedMaxCin = 1024;
bool fused_wins(int Cin, int Cout, int /* kk */) { return 2 * Cout <= BM && Cin <= kFusedMaxCin; }
bool fused_layer(const Net& n, int l) { return n.fuse && fused_wins(n.Cin[l], n.Cout[l], l < n.l_e ? 3 : n.k); }
// the widest Cout whose [A ; B] product goes through memory (0: every layer is fused)
int product_rows(const Net& n) {
    int c = 0;
    for (int l = 0; l < n.E; ++l)
        if (!fused_layer(n, l) && n.Cout[l] > c) c = n.Cout[l];
    return c;
}

Workspace layout(const Net& n, int64_t b, void* ws) {
    Workspace w{};
    Carver c{ws};
    w.cat = c.carve<float>(b * n.cat_stride() * 4);
    w.P = c.carve<float>(b * 2 * product_rows(n) * NODES * 4);
    w.idx3 = c.carve<int32_t>(b * NODES * 3 * 4);
    w.knn = c.carve<int32_t>((int64_t)n.l_d * b * NODES * n.k * 4);
    w.pooled = c.carve<float>(2 * (int64_t)n.emb * b * 4);
    for (int l = 0; l + 1 < n.l_l; ++l) w.h[l] = c.carve<float>((int64_t)n.head[l] * b * 4);
    w.flag = c.carve<int32_t>(4);
    w.total = c.used;
    return w;
}

// The smallest Cin of an edge layer that the bf16 mode moves to the bf16 kernel: below it (the first layer's 17 rows)
// K does not fill one bf16 k-step and the layer keeps the float32 kernel.
constexpr int kBf16MinCin = 32;

// out: the layer's output [b][Cout][64], patch stride e.ogs.  fused: P is not touched.  wb not null: the product on
// the bf16 kernel from wb [2 Cout][padded_k(Cin)]; wt is not read.
int run_edge(const float* wt, const __bf16* wb, const float* s, const float* t, const EdgeLayer& e, float* P,
             float* out, int64_t b, bool fused, hipStream_t st) {
    if (fused && wb) {
        FusedEdgeBf16Args a{wb, e.X, e.lists, s, t, out, e.xgs, e.ogs, e.Cin, padded_k(e.Cin), e.Cout, e.kk};
        hipLaunchKernelGGL(fused_edge_bf16_kernel, dim3((unsigned)b), dim3(256), 0, st, a);
        PCD_LAUNCH_CHECK();
        return PCD_OK;
    }
    if (fused) {
        FusedEdgeArgs a{wt, e.X, e.lists, s, t, out, e.xgs, e.ogs, e.Cin, e.Cout, e.kk};
        hipLaunchKernelGGL(fused_edge_kernel, dim3((unsigned)b), dim3(256), 0, st, a);
        PCD_LAUNCH_CHECK();
        return PCD_OK;
    }
    const int64_t pgs = (int64_t)2 * e.Cout * NODES;
    const int rc = wb ? launch_gemm_bf16(conv_args_bf16(wb, 2 * e.Cout, e.Cin, e.X, e.xgs, P, pgs, b), st)
                      : launch_gemm(conv_args(wt, 2 * e.Cout, e.Cin, e.X, e.xgs, P, pgs, b), st);
    if (rc != PCD_OK) return rc;
    hipLaunchKernelGGL(edge_kernel, dim3((unsigned)b, (unsigned)cdiv(e.Cout, 4)), dim3(256), 0, st, P, e.Cout, e.lists,
                       e.kk, s, t, out, e.ogs);
    PCD_LAUNCH_CHECK();
    return PCD_OK;
}

// the weights of either create entry: arrays of the table's lengths
struct WeightView {
    const float* const* conv_w;  const int32_t *conv_rows, *conv_cols;                      // [E + 1]
    const float *const *bn_weight, *const *bn_bias, *const *bn_mean, *const *bn_var;        // [E + l_l - 1]
    const double* bn_eps;  const int32_t* bn_len;
    const float *const *lin_w, *const *lin_b;  const int32_t *lin_rows, *lin_cols;          // [l_l]
};

int create_impl(const Net& n, const WeightView& w, pcd_dgcnn** out) {
    const int E = n.E, L = n.l_l, nb = n.nbn();    // batch norms: E + 1 convolutions, L - 1 hidden linears
    // the shapes of the layer table
    std::vector<int> cr(E + 1), cc(E + 1), bl(nb), lr(L), lc(L);
    for (int l = 0; l < E; ++l) { cr[l] = n.Cout[l]; cc[l] = 2 * n.Cin[l]; bl[l] = n.Cout[l]; }
    cr[E] = n.emb; cc[E] = n.Ccat; bl[E] = n.emb;
    for (int l = 0; l < L; ++l) { lr[l] = n.out_of_linear(l); lc[l] = n.in_of_linear(l); }
    for (int l = 0; l + 1 < L; ++l) bl[E + 1 + l] = n.head[l];
    for (int l = 0; l <= E; ++l) {
        PCD_CHECK_ARG(w.conv_w[l] != nullptr, "conv" + std::to_string(l + 1) + " weight is null");
        PCD_CHECK_ARG(w.conv_rows[l] == cr[l] && w.conv_cols[l] == cc[l],
                      "conv" + std::to_string(l + 1) + " weight must be [" + std::to_string(cr[l]) + ", " +
                          std::to_string(cc[l]) + "], got [" + std::to_string(w.conv_rows[l]) + ", " +
                          std::to_string(w.conv_cols[l]) + "]");
    }
    for (int l = 0; l < nb; ++l) {
        PCD_CHECK_ARG(w.bn_weight[l] && w.bn_bias[l] && w.bn_mean[l] && w.bn_var[l],
                      "bn" + std::to_string(l + 1) + " has a null pointer");
        PCD_CHECK_ARG(w.bn_len[l] == bl[l], "bn" + std::to_string(l + 1) + " must have " + std::to_string(bl[l]) +
                                                " channels, got " + std::to_string(w.bn_len[l]));
        PCD_CHECK_ARG(w.bn_eps[l] >= 0.0 && w.bn_eps[l] == w.bn_eps[l], "bn" + std::to_string(l + 1) + " eps is invalid");
    }
    for (int l = 0; l < L; ++l) {
        PCD_CHECK_ARG(w.lin_w[l] != nullptr, "linear" + std::to_string(l + 1) + " weight is null");
        PCD_CHECK_ARG(w.lin_rows[l] == lr[l] && w.lin_cols[l] == lc[l],
                      "linear" + std::to_string(l + 1) + " weight must be [" + std::to_string(lr[l]) + ", " +
                          std::to_string(lc[l]) + "], got [" + std::to_string(w.lin_rows[l]) + ", " +
                          std::to_string(w.lin_cols[l]) + "]");
        PCD_CHECK_ARG((w.lin_b[l] != nullptr) == (l > 0),
                      l == 0 ? std::string("linear1 has no bias") : "linear" + std::to_string(l + 1) + " bias is null");
    }
    // everything to the host (the pointers may be host or device memory), folded in double, rounded once
    auto pull = [](const float* src, int64_t cnt, std::vector<float>& dst) {
        dst.resize(cnt);
        return hipMemcpy(dst.data(), src, cnt * sizeof(float), hipMemcpyDefault);
    };
    const int total = E + 1 + L;
    std::vector<float> packed;
    std::vector<int64_t> wt_off(total), s_off(total), t_off(total);
    std::vector<float> W, g, be, mu, var, bias;
    // batch norm l -> (s, t) at slot `at`
    auto fold = [&](int l, int at, const std::vector<float>* lin_bias) {
        const int cnt = bl[l];
        s_off[at] = (int64_t)packed.size();
        for (int c = 0; c < cnt; ++c) packed.push_back((float)((double)g[c] / sqrt((double)var[c] + w.bn_eps[l])));
        t_off[at] = (int64_t)packed.size();
        for (int c = 0; c < cnt; ++c) {
            const double sc = (double)g[c] / sqrt((double)var[c] + w.bn_eps[l]);
            const double shift = (lin_bias ? (double)(*lin_bias)[c] : 0.0) - (double)mu[c];
            packed.push_back((float)((double)be[c] + sc * shift));
        }
    };
    auto pull_bn = [&](int l) -> hipError_t {
        hipError_t e = pull(w.bn_weight[l], bl[l], g);
        if (e == hipSuccess) e = pull(w.bn_bias[l], bl[l], be);
        if (e == hipSuccess) e = pull(w.bn_mean[l], bl[l], mu);
        if (e == hipSuccess) e = pull(w.bn_var[l], bl[l], var);
        return e;
    };
    for (int l = 0; l <= E; ++l) {
        PCD_HIP(pull(w.conv_w[l], (int64_t)cr[l] * cc[l], W));
        PCD_HIP(pull_bn(l));
        wt_off[l] = (int64_t)packed.size();
        if (l < E) {                                   // [W_a ; W_b - W_a], transposed to [Cin][2 Cout]
            const int Cin = n.Cin[l], Cout = n.Cout[l];
            for (int kq = 0; kq < Cin; ++kq) {
                for (int c = 0; c < Cout; ++c) packed.push_back(W[(int64_t)c * 2 * Cin + kq]);
                for (int c = 0; c < Cout; ++c)
                    packed.push_back((float)((double)W[(int64_t)c * 2 * Cin + Cin + kq] - (double)W[(int64_t)c * 2 * Cin + kq]));
            }
        } else {
            for (int kq = 0; kq < n.Ccat; ++kq)
                for (int c = 0; c < n.emb; ++c) packed.push_back(W[(int64_t)c * n.Ccat + kq]);
        }
        fold(l, l, nullptr);
    }
    for (int l = 0; l < L; ++l) {
        const int at = E + 1 + l;
        PCD_HIP(pull(w.lin_w[l], (int64_t)lr[l] * lc[l], W));
        if (l > 0) PCD_HIP(pull(w.lin_b[l], lr[l], bias));
        wt_off[at] = (int64_t)packed.size();
        for (int kq = 0; kq < lc[l]; ++kq)
            for (int c = 0; c < lr[l]; ++c) packed.push_back(W[(int64_t)c * lc[l] + kq]);
        if (l + 1 < L) {
            PCD_HIP(pull_bn(at));
            fold(at, at, l > 0 ? &bias : nullptr);
        } else {
            s_off[at] = (int64_t)packed.size();
            for (int c = 0; c < lr[l]; ++c) packed.push_back(1.f);
            t_off[at] = (int64_t)packed.size();
            for (int c = 0; c < lr[l]; ++c) packed.push_back(bias[c]);
        }
    }
    pcd_dgcnn* m = new pcd_dgcnn();
    m->net = n;
    hipError_t e = hipMalloc((void**)&m->dev, packed.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(m->dev, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (m->dev) (void)hipFree(m->dev);
        delete m;
        return fail(e == hipErrorOutOfMemory ? PCD_ERR_OOM : PCD_ERR_HIP,
                    std::string("pcd_dgcnn_create: ") + hipGetErrorString(e));
    }
    m->wt.resize(total); m->s.resize(total); m->t.resize(total);
    for (int l = 0; l < total; ++l) {
        m->wt[l] = m->dev + wt_off[l];
        m->s[l] = m->dev + s_off[l];
        m->t[l] = m->dev + t_off[l];
    }
    *out = m;
    return PCD_OK;
}

// what a debug struct of either entry asks for
struct DebugView {
    float* cat;  int32_t* lists;  float* pooled;
    float* h[kMaxLin];
};

}  // namespace

// the launchers csrc/dgcnn_train.hip uses too (declared in pcd_dgcnn.h)
namespace pcd {
namespace dgcnn {

int make_net(Net* n, int l_e, int l_d, int l_l, const int* cs, int k, int init_dims, int output_channels,
             float head_slope) {
    PCD_CHECK_ARG(l_e >= 0 && l_d >= 0, "l_e and l_d must be >= 0");
    PCD_CHECK_ARG(l_e <= kMaxEdge && l_d <= kMaxEdge && l_e + l_d >= 1 && l_e + l_d <= kMaxEdge,
                  "l_e + l_d must be in [1, " + std::to_string(kMaxEdge) + "] (there is nothing to concatenate without an "
                  "edge layer), got " + std::to_string(l_e) + " + " + std::to_string(l_d));
    PCD_CHECK_ARG(l_l >= 2 && l_l <= kMaxLin, "l_l must be in [2, " + std::to_string(kMaxLin) + "] (the last linear reads "
                  "channel_sizes[-1], a hidden width), got " + std::to_string(l_l));
    PCD_CHECK_ARG(cs != nullptr, "channel_sizes is null");
    PCD_CHECK_ARG(init_dims == 17, "init_dims must be 17 (the network's forward slices rows 0:17 of its input)");
    PCD_CHECK_ARG(k >= 1 && k <= NODES, "k must be in [1, 64]");
    PCD_CHECK_ARG(output_channels >= 1 && output_channels <= 4096, "output_channels must be in [1, 4096]");
    *n = Net{};
    n->l_e = l_e; n->l_d = l_d; n->l_l = l_l; n->E = l_e + l_d; n->k = k; n->out_ch = output_channels;
    n->head_slope = head_slope;
    for (int i = 0; i < n->E + l_l; ++i) {
        const int lim = i < n->E ? kMaxEdgeWidth : kMaxWidth;
        PCD_CHECK_ARG(cs[i] >= 1 && cs[i] <= lim, "channel_sizes[" + std::to_string(i) + "] must be in [1, " +
                                                      std::to_string(lim) + "], got " + std::to_string(cs[i]));
    }
    for (int l = 0; l < n->E; ++l) {
        n->Cin[l] = l == 0 ? 17 : cs[l - 1];
        n->Cout[l] = cs[l];
        n->cat_off[l] = n->Ccat;
        n->Ccat += cs[l];
        n->Cmax = cs[l] > n->Cmax ? cs[l] : n->Cmax;
    }
    n->emb = cs[n->E];
    for (int j = 0; j + 1 < l_l; ++j) n->head[j] = cs[n->E + 1 + j];
    return PCD_OK;
}

int fixed_net(Net* n, int k, int emb, int output_channels) {
    PCD_CHECK_ARG(emb >= 1 && emb <= (1 << 16), "emb_dims must be in [1, 65536]");
    const int cs[10] = {64, 64, 128, 256, 256, 256, emb, 512, 256, 64};
    return make_net(n, 3, 3, 4, cs, k, 17, output_channels, 0.2f);
}

int conv_gemm(const float* Wt, int M, int K, const float* X, int64_t xgs, float* Y, int64_t ygs, int64_t b, int epi,
              bool wide, hipStream_t st) {
    GemmArgs a = conv_args(Wt, M, K, X, xgs, Y, ygs, b);
    a.epi = epi;
    return launch_gemm(a, st, wide && epi == EPI_PLAIN);
}

int knn(const float* x, int64_t xgs, int C, int k, int32_t* lists, int64_t b, hipStream_t st) {
    hipLaunchKernelGGL(knn_kernel, dim3((unsigned)b), dim3(256), 0, st, x, xgs, C, k, lists);
    PCD_LAUNCH_CHECK();
    return PCD_OK;
}

int index_lists(const float* inputs, int64_t b, int32_t* lists, int* flag, int patch_base, hipStream_t st) {
    hipLaunchKernelGGL(index_kernel, dim3((unsigned)cdiv(b * NODES * 3, 256)), dim3(256), 0, st, inputs, b, lists, flag,
                       patch_base);
    PCD_LAUNCH_CHECK();
    return PCD_OK;
}

int index_lists_checked(const float* inputs, int64_t b, int32_t* lists, int* flag, int* bad, hipStream_t st) {
    *bad = kNoBadPatch;
    PCD_HIP(hipMemsetAsync(flag, 0x7f, sizeof(int), st));
    const int rc = index_lists(inputs, b, lists, flag, 0, st);
    if (rc != PCD_OK) return rc;
    PCD_HIP(hipMemcpyAsync(bad, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    PCD_HIP(hipStreamSynchronize(st));
    return PCD_OK;
}

int transpose(const float* W, int M, int K, float* Wt, hipStream_t st) {
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)cdiv((int64_t)M * K, 256)), dim3(256), 0, st, W, M, K, Wt);
    PCD_LAUNCH_CHECK();
    return PCD_OK;
}

}  // namespace dgcnn
}  // namespace pcd

// first_bad null: the index flag lives in the workspace, is read after the index kernel (one stream synchronise) and
// a bad index column refuses the call.  Otherwise the caller's device flag takes atomicMin(patch_base + patch), the
// clamped indices are used and nothing waits for the device.  A table without static layers (l_e = 0) never reads the
// index columns: they are not checked.
static int forward_impl(const pcd_dgcnn* m, const float* inputs, int64_t b, float* out, void* workspace,
                        int64_t workspace_bytes, const DebugView* debug, int32_t* first_bad, int64_t patch_base,
                        void* stream) {
    PCD_CHECK_ARG(m != nullptr, "model is null");
    PCD_CHECK_ARG(b >= 0 && b <= kMaxBatch, "b must be in [0, 2^20]");
    if (b == 0) return PCD_OK;
    PCD_CHECK_ARG(inputs != nullptr && out != nullptr, "inputs / out is null");
    const Net& n = m->net;
    const Workspace w = layout(n, b, workspace);
    PCD_CHECK_ARG(workspace != nullptr && workspace_bytes >= w.total,
                  "workspace of " + std::to_string(workspace_bytes) + " bytes is shorter than the " +
                      std::to_string(w.total) + " that " + (n.fuse ? "pcd_bdgcnn_workspace_bytes" : "pcd_dgcnn_workspace_bytes") +
                      " asks for");
    PCD_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "workspace must be 16-byte aligned");
    PCD_CHECK_ARG(patch_base >= 0 && patch_base + b < kNoBadPatch, "patch_base + b must be in [0, 0x7f7f7f7f)");
    hipStream_t st = as_stream(stream);

    // the index columns first: a bad one ends the call before anything is computed from it (or, deferred, is
    // recorded in the caller's flag while the clamped index is used)
    int rc;
    if (n.l_e > 0 && first_bad) {
        if ((rc = index_lists(inputs, b, w.idx3, first_bad, (int)patch_base, st)) != PCD_OK) return rc;
    } else if (n.l_e > 0) {
        int bad;
        if ((rc = index_lists_checked(inputs, b, w.idx3, w.flag, &bad, st)) != PCD_OK) return rc;
        PCD_CHECK_ARG(bad == kNoBadPatch, "patch " + std::to_string(bad) +
                                          " has an index column (rows 17:20) outside [0, 63] or NaN; no output written");
    }

    const int E = n.E;
    for (int l = 0; l < E; ++l) {
        const EdgeLayer e = edge_layer(n, l, inputs, w.cat, w.idx3, w.knn, b);
        if (e.knn && (rc = dgcnn::knn(e.X, e.xgs, e.Cin, e.kk, e.knn, b, st)) != PCD_OK) return rc;
        const bool fused = fused_layer(n, l);
        rc = run_edge(m->wt[l], m->bf16_weight(l), m->s[l], m->t[l], e, w.P, w.cat + e.out_off, b, fused, st);
        if (rc != PCD_OK) return rc;
    }
    // the pooled convolution + batch norm + LeakyReLU + max / mean over the nodes -> pooled [2 emb][b]
    if (const __bf16* wb = m->bf16_weight(E)) {
        GemmBf16Args a = conv_args_bf16(wb, n.emb, n.Ccat, w.cat, n.cat_stride(), nullptr, 0, b);
        a.epi = EPI_POOL; a.s = m->s[E]; a.t = m->t[E]; a.poolT = w.pooled;
        a.pool_dbg = debug ? debug->pooled : nullptr;
        if ((rc = launch_gemm_bf16(a, st)) != PCD_OK) return rc;
    } else {
        GemmArgs a = conv_args(m->wt[E], n.emb, n.Ccat, w.cat, n.cat_stride(), nullptr, 0, b);
        a.epi = EPI_POOL; a.s = m->s[E]; a.t = m->t[E]; a.poolT = w.pooled;
        a.pool_dbg = debug ? debug->pooled : nullptr;
        if ((rc = launch_gemm(a, st)) != PCD_OK) return rc;
    }
    const int H = n.l_l - 1;                            // hidden linears
    for (int l = 0; l < H; ++l) {
        GemmArgs a = head_args(m->wt[E + 1 + l], n.head[l], n.in_of_linear(l), l ? w.h[l - 1] : w.pooled, w.h[l], b);
        a.epi = EPI_AFFINE_LRELU; a.s = m->s[E + 1 + l]; a.t = m->t[E + 1 + l]; a.slope = n.head_slope;
        if ((rc = launch_gemm(a, st)) != PCD_OK) return rc;
    }
    {   // the last linear (+ bias) -> out [b][out_ch]
        GemmArgs a = head_args(m->wt[E + 1 + H], n.out_ch, n.head[H - 1], w.h[H - 1], out, b);
        a.G = 1; a.ygs = n.out_ch; a.yms = 1;           // Y(m, n) = out[n * out_ch + m]
        a.xgs = 1; a.xks = b;                           // X(k, n) = h[k * b + n]
        a.epi = EPI_AFFINE; a.s = m->s[E + 1 + H]; a.t = m->t[E + 1 + H];
        if ((rc = launch_gemm(a, st)) != PCD_OK) return rc;
    }
    if (debug) {
        if (debug->cat) PCD_HIP(hipMemcpyAsync(debug->cat, w.cat, b * n.cat_stride() * 4, hipMemcpyDeviceToDevice, st));
        if (debug->lists && n.l_d > 0)
            PCD_HIP(hipMemcpyAsync(debug->lists, w.knn, (int64_t)n.l_d * b * NODES * n.k * 4, hipMemcpyDeviceToDevice, st));
        for (int l = 0; l < H; ++l)
            if (debug->h[l])
                PCD_HIP(hipMemcpyAsync(debug->h[l], w.h[l], (int64_t)n.head[l] * b * 4, hipMemcpyDeviceToDevice, st));
    }
    return PCD_OK;
}

static bool fixed_debug(const pcd_dgcnn_debug* d, DebugView* v) {
    if (!d) return false;
    *v = DebugView{};
    v->cat = d->cat; v->lists = d->lists; v->pooled = d->pooled;
    v->h[0] = d->h1; v->h[1] = d->h2; v->h[2] = d->h3;
    return true;
}
static bool table_debug(const pcd_dgcnn* m, const pcd_bdgcnn_debug* d, DebugView* v) {
    if (!d) return false;
    *v = DebugView{};
    v->cat = d->cat; v->lists = d->lists; v->pooled = d->pooled;
    if (m && d->h)
        for (int l = 0; l + 1 < m->net.l_l; ++l) v->h[l] = d->h[l];
    return true;
}

extern "C" {

int pcd_dgcnn_create(const pcd_dgcnn_weights* w, int k, int init_dims, int emb_dims, int output_channels,
                     pcd_dgcnn** out) {
    PCD_CHECK_ARG(out != nullptr, "out is null");
    *out = nullptr;
    PCD_CHECK_ARG(w != nullptr, "weights is null");
    PCD_CHECK_ARG(init_dims == 17, "init_dims must be 17 (the network's forward slices rows 0:17 of its input)");
    Net n;
    const int rc = fixed_net(&n, k, emb_dims, output_channels);
    if (rc != PCD_OK) return rc;
    const WeightView v{w->conv_w, w->conv_rows, w->conv_cols, w->bn_weight, w->bn_bias, w->bn_mean, w->bn_var,
                       w->bn_eps, w->bn_len, w->lin_w, w->lin_b, w->lin_rows, w->lin_cols};
    return create_impl(n, v, out);
}

int pcd_bdgcnn_create(const pcd_dgcnn_table* t, const pcd_bdgcnn_weights* w, pcd_dgcnn** out) {
    PCD_CHECK_ARG(out != nullptr, "out is null");
    *out = nullptr;
    PCD_CHECK_ARG(t != nullptr, "table is null");
    Net n;
    const int rc = make_net(&n, t->l_e, t->l_d, t->l_l, t->channel_sizes, t->k, t->init_dims, t->output_channels,
                            PCD_BDGCNN_HEAD_SLOPE);
    if (rc != PCD_OK) return rc;
    n.fuse = true;
    PCD_CHECK_ARG(w != nullptr, "weights is null");
    PCD_CHECK_ARG(w->conv_w && w->conv_rows && w->conv_cols && w->bn_weight && w->bn_bias && w->bn_mean && w->bn_var &&
                      w->bn_eps && w->bn_len && w->lin_w && w->lin_b && w->lin_rows && w->lin_cols,
                  "weights has a null array");
    const WeightView v{w->conv_w, w->conv_rows, w->conv_cols, w->bn_weight, w->bn_bias, w->bn_mean, w->bn_var,
                       w->bn_eps, w->bn_len, w->lin_w, w->lin_b, w->lin_rows, w->lin_cols};
    return create_impl(n, v, out);
}

int pcd_dgcnn_destroy(pcd_dgcnn* m) {
    if (!m) return PCD_OK;
    if (m->dev) (void)hipFree(m->dev);
    if (m->dev16) (void)hipFree(m->dev16);
    delete m;
    return PCD_OK;
}

int pcd_dgcnn_set_operands(pcd_dgcnn* m, int operands) {
    PCD_CHECK_ARG(operands == PCD_OPERANDS_F32 || operands == PCD_OPERANDS_BF16,
                  "operands must be PCD_OPERANDS_F32 or PCD_OPERANDS_BF16");
    PCD_CHECK_ARG(m != nullptr, "model is null");
    if (operands == PCD_OPERANDS_BF16 && !m->dev16) {
        // the packed float32 [W_a ; W_b - W_a] of every edge layer with Cin >= 32, and W7, rounded once
        const Net& n = m->net;
        const int E = n.E;
        std::vector<int64_t> off(E + 1, -1);
        Carver c{nullptr};
        for (int l = 0; l <= E; ++l) {
            if (l < E && n.Cin[l] < kBf16MinCin) continue;
            const int M = l < E ? 2 * n.Cout[l] : n.emb, K = l < E ? n.Cin[l] : n.Ccat;
            off[l] = c.take((int64_t)M * padded_k(K) * 2);
        }
        __bf16* dev16 = nullptr;
        hipError_t e = hipMalloc((void**)&dev16, c.used > 0 ? c.used : 256);
        if (e != hipSuccess)
            return fail(e == hipErrorOutOfMemory ? PCD_ERR_OOM : PCD_ERR_HIP,
                        std::string("pcd_dgcnn_set_operands: ") + hipGetErrorString(e));
        std::vector<const __bf16*> wb(E + 1, nullptr);
        int rc = PCD_OK;
        for (int l = 0; l <= E && rc == PCD_OK; ++l) {
            if (off[l] < 0) continue;
            const int M = l < E ? 2 * n.Cout[l] : n.emb, K = l < E ? n.Cin[l] : n.Ccat;
            __bf16* dst = at<__bf16>(dev16, off[l]);
            rc = pack_bf16(m->wt[l], 1, M, M, K, dst, nullptr);      // Wt [K][M]
            wb[l] = dst;
        }
        if (rc == PCD_OK && (e = hipStreamSynchronize(nullptr)) != hipSuccess)
            rc = fail(PCD_ERR_HIP, std::string("pcd_dgcnn_set_operands: ") + hipGetErrorString(e));
        if (rc != PCD_OK) {
            (void)hipFree(dev16);
            return rc;
        }
        m->dev16 = dev16;
        m->wb = wb;
    }
    m->operands = operands;
    return PCD_OK;
}

int pcd_dgcnn_operands(const pcd_dgcnn* m, int* operands) {
    PCD_CHECK_ARG(m != nullptr, "model is null");
    PCD_CHECK_ARG(operands != nullptr, "operands is null");
    *operands = m->operands;
    return PCD_OK;
}
int pcd_bdgcnn_destroy(pcd_dgcnn* m) { return pcd_dgcnn_destroy(m); }

int pcd_dgcnn_workspace_bytes(const pcd_dgcnn* m, int64_t b, int64_t* bytes) {
    PCD_CHECK_ARG(m != nullptr, "model is null");
    PCD_CHECK_ARG(bytes != nullptr, "bytes is null");
    PCD_CHECK_ARG(b >= 0 && b <= kMaxBatch, "b must be in [0, 2^20]");
    *bytes = layout(m->net, b, nullptr).total;
    return PCD_OK;
}
int pcd_bdgcnn_workspace_bytes(const pcd_dgcnn* m, int64_t b, int64_t* bytes) {
    return pcd_dgcnn_workspace_bytes(m, b, bytes);
}

int pcd_dgcnn_forward(const pcd_dgcnn* m, const float* inputs, int64_t b, float* out, void* workspace,
                      int64_t workspace_bytes, const pcd_dgcnn_debug* debug, void* stream) {
    DebugView v;
    return forward_impl(m, inputs, b, out, workspace, workspace_bytes, fixed_debug(debug, &v) ? &v : nullptr, nullptr, 0,
                        stream);
}

int pcd_dgcnn_forward_deferred(const pcd_dgcnn* m, const float* inputs, int64_t b, float* out, void* workspace,
                               int64_t workspace_bytes, const pcd_dgcnn_debug* debug, int32_t* first_bad,
                               int64_t patch_base, void* stream) {
    PCD_CHECK_ARG(first_bad != nullptr, "first_bad is null");
    DebugView v;
    return forward_impl(m, inputs, b, out, workspace, workspace_bytes, fixed_debug(debug, &v) ? &v : nullptr, first_bad,
                        patch_base, stream);
}

int pcd_bdgcnn_forward(const pcd_dgcnn* m, const float* inputs, int64_t b, float* out, void* workspace,
                       int64_t workspace_bytes, const pcd_bdgcnn_debug* debug, void* stream) {
    DebugView v;
    return forward_impl(m, inputs, b, out, workspace, workspace_bytes, table_debug(m, debug, &v) ? &v : nullptr, nullptr,
                        0, stream);
}

int pcd_bdgcnn_forward_deferred(const pcd_dgcnn* m, const float* inputs, int64_t b, float* out, void* workspace,
                                int64_t workspace_bytes, const pcd_bdgcnn_debug* debug, int32_t* first_bad,
                                int64_t patch_base, void* stream) {
    PCD_CHECK_ARG(first_bad != nullptr, "first_bad is null");
    DebugView v;
    return forward_impl(m, inputs, b, out, workspace, workspace_bytes, table_debug(m, debug, &v) ? &v : nullptr,
                        first_bad, patch_base, stream);
}

int pcd_dgcnn_knn(const float* x, int64_t b, int channels, int k, int32_t* lists, void* stream) {
    PCD_CHECK_ARG(b >= 0 && b <= kMaxBatch, "b must be in [0, 2^20]");
    PCD_CHECK_ARG(channels >= 1, "channels must be >= 1");
    PCD_CHECK_ARG(k >= 1 && k <= NODES, "k must be in [1, 64]");
    if (b == 0) return PCD_OK;
    PCD_CHECK_ARG(x != nullptr && lists != nullptr, "x / lists is null");
    return dgcnn::knn(x, (int64_t)channels * NODES, channels, k, lists, b, as_stream(stream));
}

int pcd_dgcnn_edgeconv(const pcd_dgcnn* m, int layer, const float* x, int64_t b, const int32_t* lists, int list_len,
                       float* out, void* stream) {
    PCD_CHECK_ARG(m != nullptr, "model is null");
    PCD_CHECK_ARG(layer >= 1 && layer <= m->net.E, "layer must be in [1, " + std::to_string(m->net.E) + "]");
    PCD_CHECK_ARG(b >= 0 && b <= kMaxBatch, "b must be in [0, 2^20]");
    PCD_CHECK_ARG(list_len >= 1 && list_len <= NODES, "list_len must be in [1, 64]");
    if (b == 0) return PCD_OK;
    PCD_CHECK_ARG(x != nullptr && lists != nullptr && out != nullptr, "x / lists / out is null");
    const int l = layer - 1, Cin = m->net.Cin[l], Cout = m->net.Cout[l];
    hipStream_t st = as_stream(stream);
    StreamTemps tmp(st);
    float* P;
    PCD_HIP(tmp.alloc(&P, b * 2 * Cout * NODES * sizeof(float)));
    const int rc = run_edge(m->wt[l], m->bf16_weight(l), m->s[l], m->t[l],
                            edge_layer_alone(Cin, Cout, x, lists, list_len), P, out, b, false, st);
    if (rc != PCD_OK) return rc;
    PCD_HIP(tmp.release());
    return PCD_OK;
}

// the stage entry's scratch: the packed weight [c_in][2 c_out], then (two kernels) P [b][2 c_out][64]
static int64_t edgeconv_scratch(int c_in, int c_out, int64_t b, bool fused, void* base, float** wt, float** P) {
    Carver c{base};
    *wt = c.carve<float>((int64_t)2 * c_in * c_out * 4);
    *P = fused ? nullptr : c.carve<float>(b * 2 * c_out * NODES * 4);
    return c.used;
}
// the bf16 stage entry's: the rounded weight [2 c_out][padded_k(c_in)] in the packed weight's place, then P
static int64_t edgeconv_scratch_bf16(int c_in, int c_out, int64_t b, bool fused, void* base, __bf16** wb, float** P) {
    Carver c{base};
    *wb = c.carve<__bf16>((int64_t)2 * c_out * padded_k(c_in) * 2);
    *P = fused ? nullptr : c.carve<float>(b * 2 * c_out * NODES * 4);
    return c.used;
}

int pcd_bdgcnn_edgeconv_scratch_bytes(int c_in, int c_out, int64_t b, int64_t* bytes) {
    PCD_CHECK_ARG(bytes != nullptr, "bytes is null");
    PCD_CHECK_ARG(c_in >= 1 && c_in <= kMaxEdgeWidth && c_out >= 1 && c_out <= kMaxEdgeWidth,
                  "c_in and c_out must be in [1, " + std::to_string(kMaxEdgeWidth) + "]");
    PCD_CHECK_ARG(b >= 0 && b <= kMaxBatch, "b must be in [0, 2^20]");
    float *wt, *P;
    __bf16* wb;
    *bytes = edgeconv_scratch(c_in, c_out, b, false, nullptr, &wt, &P);
    // (the bf16 weight's rows are padded to 8 k: longer than the float32 weight only where c_in < 7)
    const int64_t bf = edgeconv_scratch_bf16(c_in, c_out, b, false, nullptr, &wb, &P);
    if (bf > *bytes) *bytes = bf;
    return PCD_OK;
}

int pcd_bdgcnn_edgeconv(const float* w, const float* s, const float* t, int c_in, int c_out, const float* x, int64_t b,
                        const int32_t* lists, int list_len, int fused, float* out, void* scratch, int64_t scratch_bytes,
                        void* stream) {
    PCD_CHECK_ARG(fused == PCD_FUSED_OFF || fused == PCD_FUSED_ON || fused == PCD_FUSED_AUTO,
                  "fused must be PCD_FUSED_OFF, PCD_FUSED_ON or PCD_FUSED_AUTO");
    PCD_CHECK_ARG(fused != PCD_FUSED_ON || 2 * c_out <= BM,
                  "fused = PCD_FUSED_ON needs 2 c_out <= " + std::to_string(BM) + " (one GEMM tile holds the patch's [A ; B])");
    PCD_CHECK_ARG(c_in >= 1 && c_in <= kMaxEdgeWidth && c_out >= 1 && c_out <= kMaxEdgeWidth,
                  "c_in and c_out must be in [1, " + std::to_string(kMaxEdgeWidth) + "]");
    PCD_CHECK_ARG(b >= 0 && b <= kMaxBatch, "b must be in [0, 2^20]");
    PCD_CHECK_ARG(list_len >= 1 && list_len <= NODES, "list_len must be in [1, 64]");
    if (b == 0) return PCD_OK;
    PCD_CHECK_ARG(w && s && t && x && lists && out, "a pointer is null");
    const bool fuse = fused == PCD_FUSED_ON || (fused == PCD_FUSED_AUTO && fused_wins(c_in, c_out, list_len));
    hipStream_t st = as_stream(stream);
    StreamTemps tmp(st);
    float *wt, *P;
    const int64_t need = edgeconv_scratch(c_in, c_out, b, fuse, scratch, &wt, &P);
    if (scratch) {
        PCD_CHECK_ARG(scratch_bytes >= need && reinterpret_cast<uintptr_t>(scratch) % 16 == 0,
                      "scratch must be 16-byte aligned and hold the " + std::to_string(need) +
                          " bytes that pcd_bdgcnn_edgeconv_scratch_bytes asks for at most, got " +
                          std::to_string(scratch_bytes));
    } else {
        char* own;
        PCD_HIP(tmp.alloc(&own, need));
        edgeconv_scratch(c_in, c_out, b, fuse, own, &wt, &P);
    }
    int rc = dgcnn::pack_edge(w, c_in, c_out, wt, nullptr, st);
    if (rc != PCD_OK) return rc;
    rc = run_edge(wt, nullptr, s, t, edge_layer_alone(c_in, c_out, x, lists, list_len), P, out, b, fuse, st);
    if (rc != PCD_OK) return rc;
    if (!scratch) PCD_HIP(tmp.release());
    return PCD_OK;
}

int pcd_bdgcnn_edgeconv_bf16(const float* w, const float* s, const float* t, int c_in, int c_out, const float* x,
                             int64_t b, const int32_t* lists, int list_len, int fused, float* out, void* scratch,
                             int64_t scratch_bytes, void* stream) {
    PCD_CHECK_ARG(fused == PCD_FUSED_OFF || fused == PCD_FUSED_ON || fused == PCD_FUSED_AUTO,
                  "fused must be PCD_FUSED_OFF, PCD_FUSED_ON or PCD_FUSED_AUTO");
    PCD_CHECK_ARG(fused != PCD_FUSED_ON || 2 * c_out <= BM,
                  "fused = PCD_FUSED_ON needs 2 c_out <= " + std::to_string(BM) + " (one GEMM tile holds the patch's [A ; B])");
    PCD_CHECK_ARG(c_in >= 1 && c_in <= kMaxEdgeWidth && c_out >= 1 && c_out <= kMaxEdgeWidth,
                  "c_in and c_out must be in [1, " + std::to_string(kMaxEdgeWidth) + "]");
    PCD_CHECK_ARG(b >= 0 && b <= kMaxBatch, "b must be in [0, 2^20]");
    PCD_CHECK_ARG(list_len >= 1 && list_len <= NODES, "list_len must be in [1, 64]");
    if (b == 0) return PCD_OK;
    PCD_CHECK_ARG(w && s && t && x && lists && out, "a pointer is null");
    const bool fuse = fused == PCD_FUSED_ON || (fused == PCD_FUSED_AUTO && fused_wins(c_in, c_out, list_len));
    hipStream_t st = as_stream(stream);
    StreamTemps tmp(st);
    __bf16* wb;
    float* P;
    const int64_t need = edgeconv_scratch_bf16(c_in, c_out, b, fuse, scratch, &wb, &P);
    if (scratch) {
        PCD_CHECK_ARG(scratch_bytes >= need && reinterpret_cast<uintptr_t>(scratch) % 16 == 0,
                      "scratch must be 16-byte aligned and hold the " + std::to_string(need) +
                          " bytes that pcd_bdgcnn_edgeconv_scratch_bytes asks for at most, got " +
                          std::to_string(scratch_bytes));
    } else {
        char* own;
        PCD_HIP(tmp.alloc(&own, need));
        edgeconv_scratch_bf16(c_in, c_out, b, fuse, own, &wb, &P);
    }
    const int Kp = padded_k(c_in);
    hipLaunchKernelGGL(pack_edge_bf16_kernel, dim3((unsigned)cdiv((int64_t)2 * c_out * Kp, 256)), dim3(256), 0, st, w,
                       c_in, c_out, Kp, wb);
    PCD_LAUNCH_CHECK();
    const int rc = run_edge(nullptr, wb, s, t, edge_layer_alone(c_in, c_out, x, lists, list_len), P, out, b, fuse, st);
    if (rc != PCD_OK) return rc;
    if (!scratch) PCD_HIP(tmp.release());
    return PCD_OK;
}

int pcd_dgcnn_gemm_bf16(const float* w, const float* x, int m_rows, int k_cols, int64_t b, int epilogue, const float* s,
                        const float* t, float* y, void* stream) {
    PCD_CHECK_ARG(m_rows >= 1 && k_cols >= 1, "M and K must be >= 1");
    PCD_CHECK_ARG(b >= 0 && b <= kMaxBatch, "b must be in [0, 2^20]");
    PCD_CHECK_ARG(epilogue >= EPI_PLAIN && epilogue <= EPI_AFFINE, "epilogue must be in [0, 3]");
    PCD_CHECK_ARG(epilogue == EPI_PLAIN || (s != nullptr && t != nullptr), "s / t is null");
    if (b == 0) return PCD_OK;
    PCD_CHECK_ARG(w != nullptr && x != nullptr && y != nullptr, "w / x / y is null");
    hipStream_t st = as_stream(stream);
    StreamTemps tmp(st);
    __bf16* Wb;
    float* poolT = nullptr;
    PCD_HIP(tmp.alloc(&Wb, (int64_t)m_rows * padded_k(k_cols) * 2));
    int rc = pack_bf16(w, k_cols, 1, m_rows, k_cols, Wb, st);
    if (rc != PCD_OK) return rc;
    GemmBf16Args a = conv_args_bf16(Wb, m_rows, k_cols, x, (int64_t)k_cols * NODES, y, (int64_t)m_rows * NODES, b);
    a.epi = epilogue; a.s = s; a.t = t;
    if (epilogue == EPI_POOL) {                        // y [b][2 M]
        PCD_HIP(tmp.alloc(&poolT, 2 * (int64_t)m_rows * b * sizeof(float)));
        a.poolT = poolT; a.pool_dbg = y; a.Y = nullptr;
    }
    if ((rc = launch_gemm_bf16(a, st)) != PCD_OK) return rc;
    PCD_HIP(tmp.release());
    return PCD_OK;
}

int pcd_dgcnn_gemm(const float* w, const float* x, int m_rows, int k_cols, int64_t b, int nodes, int epilogue,
                   const float* s, const float* t, float* y, void* stream) {
    PCD_CHECK_ARG(m_rows >= 1 && k_cols >= 1, "M and K must be >= 1");
    PCD_CHECK_ARG(b >= 0 && b <= kMaxBatch, "b must be in [0, 2^20]");
    PCD_CHECK_ARG(nodes == NODES || nodes == 1, "nodes must be 64 (x [b][K][64]) or 1 (x [K][b])");
    PCD_CHECK_ARG(epilogue >= EPI_PLAIN && epilogue <= EPI_ADD, "epilogue must be in [0, 4]");
    PCD_CHECK_ARG(epilogue != EPI_POOL || nodes == NODES, "the pooling epilogue needs nodes = 64");
    PCD_CHECK_ARG(epilogue == EPI_PLAIN || epilogue == EPI_ADD || (s != nullptr && t != nullptr), "s / t is null");
    if (b == 0) return PCD_OK;
    PCD_CHECK_ARG(w != nullptr && x != nullptr && y != nullptr, "w / x / y is null");
    hipStream_t st = as_stream(stream);
    StreamTemps tmp(st);
    float *Wt, *poolT = nullptr;
    const int64_t wn = (int64_t)m_rows * k_cols;
    PCD_HIP(tmp.alloc(&Wt, wn * sizeof(float)));
    int rc = dgcnn::transpose(w, m_rows, k_cols, Wt, st);
    if (rc != PCD_OK) return rc;
    GemmArgs a = nodes == NODES
                     ? conv_args(Wt, m_rows, k_cols, x, (int64_t)k_cols * NODES, y, (int64_t)m_rows * NODES, b)
                     : head_args(Wt, m_rows, k_cols, x, y, b);
    a.epi = epilogue; a.s = s; a.t = t;
    if (epilogue == EPI_POOL) {                        // y [b][2 M]
        PCD_HIP(tmp.alloc(&poolT, 2 * (int64_t)m_rows * b * sizeof(float)));
        a.poolT = poolT; a.pool_dbg = y; a.Y = nullptr;
    }
    if ((rc = launch_gemm(a, st)) != PCD_OK) return rc;
    PCD_HIP(tmp.release());
    return PCD_OK;
}

}  // extern "C"
