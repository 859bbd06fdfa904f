// What the DGCNN forward (dgcnn.hip) shares with the train-mode forward / backward (dgcnn_train.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pcd {
namespace dgcnn {

// epilogues of the GEMM; EPI_ADD: Y += W . X (plain product added into what Y holds)
constexpr int EPI_PLAIN = 0, EPI_AFFINE_LRELU = 1, EPI_POOL = 2, EPI_AFFINE = 3, EPI_ADD = 4;

// Y [b][M][64] (patch stride ygs) = or += W . X, X [b][K][64] (patch stride xgs); Wt [K][M] is W transposed.
// epi: EPI_PLAIN or EPI_ADD.  wide (EPI_PLAIN only): float32 chains of 8 k joined in double, rounded once.
int conv_gemm(const float* Wt, int M, int K, const float* X, int64_t xgs, float* Y, int64_t ygs, int64_t b, int epi,
              bool wide, hipStream_t st);
// x [b] patches of [C][64] (patch stride xgs) -> lists [b][64][k]
int knn(const float* x, int64_t xgs, int C, int k, int32_t* lists, int64_t b, hipStream_t st);
// inputs [b][20][64] -> lists [b][64][3]; flag takes the lowest patch with a bad index column
int index_lists(const float* inputs, int64_t b, int32_t* lists, int* flag, hipStream_t st);
// W [M][K] -> Wt [K][M]
int transpose(const float* W, int M, int K, float* Wt, hipStream_t st);

}  // namespace dgcnn
}  // namespace pcd
