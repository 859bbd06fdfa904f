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
constexpr int kCin[6] = {17, 64, 64, 128, 256, 256};       // edge layers conv1-6
constexpr int kCout[6] = {64, 64, 128, 256, 256, 256};
constexpr int kCatOff[6] = {0, 64, 128, 256, 512, 768};    // the layer's slice of the [1024][64] concatenation
constexpr int64_t kCatStride = 1024 * NODES;               // floats per patch of the concatenation
constexpr int kHead[3] = {512, 256, 64};                   // linear1-3
constexpr int64_t kMaxBatch = 1 << 20;   // 2^31 / (64 x 20) patches and more would pass int32 in the index flag
constexpr int kNoBadPatch = PCD_DGCNN_NO_BAD_PATCH;

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

// layer l of the network: conv1 reads inputs [b][20][64], the others the slice before theirs of cat [b][1024][64];
// conv1-3 go over the index lists idx3 [b][64][3], conv4-6 over their third of knn [3][b][64][k]
inline EdgeLayer edge_layer(int l, const float* inputs, const float* cat, const int32_t* idx3, int32_t* knn, int k,
                            int64_t b) {
    EdgeLayer e{};
    e.Cin = kCin[l]; e.Cout = kCout[l];
    e.X = l == 0 ? inputs : cat + (int64_t)kCatOff[l - 1] * NODES;
    e.xgs = l == 0 ? 20 * NODES : kCatStride;
    e.knn = l >= 3 ? knn + (int64_t)(l - 3) * b * NODES * k : nullptr;
    e.lists = l >= 3 ? e.knn : idx3;
    e.kk = l >= 3 ? k : 3;
    e.out_off = (int64_t)kCatOff[l] * NODES; e.ogs = kCatStride;
    return e;
}
// layer l on its own (the stage entries): x [b][Cin][64] -> [b][Cout][64] over the caller's lists
inline EdgeLayer edge_layer_alone(int l, const float* x, const int32_t* lists, int kk) {
    EdgeLayer e{};
    e.Cin = kCin[l]; e.Cout = kCout[l];
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

}  // namespace dgcnn
}  // namespace pcd
