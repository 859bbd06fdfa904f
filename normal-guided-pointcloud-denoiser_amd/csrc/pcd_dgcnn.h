// What the DGCNN forward (dgcnn.hip) and the train-mode forward / backward (dgcnn_train.hip) share: the layer table,
// the wiring of an edge layer (EdgeLayer), the workspace carver, the C layout of the MFMA both GEMM kernels use, and
// the launchers dgcnn.hip defines for the training file too.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pcd_host.h"

namespace pcd {
namespace dgcnn {

constexpr int NODES = 64;                                  // rows of a patch
constexpr int64_t kMaxBatch = 1 << 20;   // 2^31 / (64 x 20) patches and more would pass int32 in the index flag
constexpr int kNoBadPatch = PCD_DGCNN_NO_BAD_PATCH;
constexpr float kTrunkSlope = 0.2f;      // LeakyReLU of every convolution; the head's is the table's
// the bounds of a table (pcd.h states them): with them no int32 product of two widths, and no int32 grid size, overflows
constexpr int kMaxEdge = PCD_DGCNN_MAX_EDGE_LAYERS, kMaxLin = PCD_DGCNN_MAX_LINEARS;
constexpr int kMaxEdgeWidth = PCD_DGCNN_MAX_EDGE_WIDTH, kMaxWidth = PCD_DGCNN_MAX_WIDTH;

// The layer table, on the host.  DGCNN is fixed_net(); BetterDGCNN's comes from the caller (make_net).
struct Net {
    int l_e = 0, l_d = 0, l_l = 0;   // static edge layers (over the index columns), dynamic ones (k-NN), linears
    int E = 0;                       // l_e + l_d
    int k = 0;
    int Cin[kMaxEdge] = {}, Cout[kMaxEdge] = {};
    int cat_off[kMaxEdge] = {};      // the layer's slice of the [Ccat][64] concatenation
    int Ccat = 0;                    // sum of Cout
    int Cmax = 0;                    // the widest edge layer
    int emb = 0;                     // the pooled convolution's width
    int head[kMaxLin] = {};          // the l_l - 1 hidden widths of the head
    int out_ch = 0;
    float head_slope = 0.2f;         // LeakyReLU of the head (DGCNN 0.2; BetterDGCNN F.leaky_relu's default 0.01)
    bool fuse = false;               // eval(): narrow edge layers in one kernel where it measured faster (BetterDGCNN)
    int64_t cat_stride() const { return (int64_t)Ccat * NODES; }   // floats per patch of the concatenation
    int nbn() const { return E + l_l; }                            // batch norms
    int in_of_linear(int j) const { return j == 0 ? 2 * emb : head[j - 1]; }
    int out_of_linear(int j) const { return j < l_l - 1 ? head[j] : out_ch; }
};
// channel_sizes [l_e + l_d + l_l]; PCD_ERR_ARG (naming the argument) for what GCNModel.py:217-256 cannot build
int make_net(Net* n, int l_e, int l_d, int l_l, const int* channel_sizes, int k, int init_dims, int output_channels,
             float head_slope);
// DGCNN(k, 17, emb, ., out_ch): 3, 3, 4, [64, 64, 128, 256, 256, 256, emb, 512, 256, 64], head slope 0.2
int fixed_net(Net* n, int k, int emb, int output_channels);

// Where edge layer l reads and writes.  g, the arg-max bytes and dL/d out are laid out as out is; dL/dX as X is.
struct EdgeLayer {
    int Cin, Cout;
    const float* X;          // [b][Cin][64], patch stride xgs
    int64_t xgs;
    const int32_t* lists;    // [b][64][kk]
    int kk;
    int32_t* knn;            // null, or lists: the layer's own k-NN lists, to be made from X before they are read
    int64_t out_off, ogs;    // the output is [b][Cout][64] at out_off floats into a buffer of patch stride ogs
};

// layer l of the network: the first reads rows 0:17 of inputs [b][20][64], the others the slice before theirs of cat
// [b][Ccat][64]; the static ones go over the index lists idx3 [b][64][3], dynamic layer d over block d of knn
// [l_d][b][64][k]
inline EdgeLayer edge_layer(const Net& n, int l, const float* inputs, const float* cat, const int32_t* idx3, int32_t* knn,
                            int64_t b) {
    EdgeLayer e{};
    e.Cin = n.Cin[l]; e.Cout = n.Cout[l];
    e.X = l == 0 ? inputs : cat + (int64_t)n.cat_off[l - 1] * NODES;
    e.xgs = l == 0 ? 20 * NODES : n.cat_stride();
    e.knn = l >= n.l_e ? knn + (int64_t)(l - n.l_e) * b * NODES * n.k : nullptr;
    e.lists = l >= n.l_e ? e.knn : idx3;
    e.kk = l >= n.l_e ? n.k : 3;
    e.out_off = (int64_t)n.cat_off[l] * NODES; e.ogs = n.cat_stride();
    return e;
}
// a layer on its own (the stage entries): x [b][Cin][64] -> [b][Cout][64] over the caller's lists
inline EdgeLayer edge_layer_alone(int Cin, int Cout, const float* x, const int32_t* lists, int kk) {
    EdgeLayer e{};
    e.Cin = Cin; e.Cout = Cout;
    e.X = x; e.xgs = (int64_t)e.Cin * NODES; e.ogs = (int64_t)e.Cout * NODES;
    e.lists = lists; e.kk = kk;
    return e;
}

template <class T>
T* at(void* base, int64_t off) { return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) + off); }
// Carves one allocation into pieces whose offsets are multiples of 256.  A layout function runs the same carve<T>
// calls to size a workspace (base null: only `used` means anything) and to unpack one.
struct Carver {
    void* base;
    int64_t used = 0;
    int64_t take(int64_t bytes) { const int64_t o = used; used += (bytes + 255) / 256 * 256; return o; }
    template <class T> T* carve(int64_t bytes) { return at<T>(base, take(bytes)); }
};

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : 0.2f * v; }
__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : slope * v; }

// C layout of v_mfma_f32_32x32x2_f32: column = lane & 31; register r of a lane holds the tile's row (r & 3) +
// 8 (r >> 2) + 4 (lane >> 5).  tile_row: the first row of the 32 x 32 tile, half = lane >> 5.
__device__ __forceinline__ int mfma_row(int tile_row, int r, int half) {
    return tile_row + (r & 3) + 8 * (r >> 2) + 4 * half;
}

// epilogues of the GEMM; EPI_ADD: Y += W . X (plain product added into what Y holds)
constexpr int EPI_PLAIN = 0, EPI_AFFINE_LRELU = 1, EPI_POOL = 2, EPI_AFFINE = 3, EPI_ADD = 4;

// Y [b][M][64] (patch stride ygs) = or += W . X, X [b][K][64] (patch stride xgs); Wt [K][M] is W transposed.
// epi: EPI_PLAIN or EPI_ADD.  wide (EPI_PLAIN only): float32 chains of 8 k joined in double, rounded once.
int conv_gemm(const float* Wt, int M, int K, const float* X, int64_t xgs, float* Y, int64_t ygs, int64_t b, int epi,
              bool wide, hipStream_t st);
// x [b] patches of [C][64] (patch stride xgs) -> lists [b][64][k]
int knn(const float* x, int64_t xgs, int C, int k, int32_t* lists, int64_t b, hipStream_t st);
// inputs [b][20][64] -> lists [b][64][3]; flag takes the lowest patch_base + patch with a bad index column
int index_lists(const float* inputs, int64_t b, int32_t* lists, int* flag, int patch_base, hipStream_t st);
// the same, waiting for it (one stream synchronise): *bad = the lowest patch with a bad index column or kNoBadPatch
int index_lists_checked(const float* inputs, int64_t b, int32_t* lists, int* flag, int* bad, hipStream_t st);
// W [M][K] -> Wt [K][M]
int transpose(const float* W, int M, int K, float* Wt, hipStream_t st);
// conv weight W [Cout][2 Cin] -> [W_a ; W_b - W_a] as Wt [Cin][2 Cout] and, if not null, Ws [2 Cout][Cin]
// (csrc/dgcnn_train.hip)
int pack_edge(const float* W, int Cin, int Cout, float* Wt, float* Ws, hipStream_t st);

}  // namespace dgcnn
}  // namespace pcd
