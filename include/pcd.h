/*
 * pcd.h -- C-ABI of libpcd.so, the MI355X-native (gfx950) hot path of the normal-guided point-cloud denoiser.
 *
 * Every entry point takes raw DEVICE pointers + sizes + an opaque hipStream_t (passed as void*), never torch
 * types.  Calls are stream-ordered; the library never frees caller memory.  Every entry returns an int status
 * (PCD_OK = 0, negative on error) and pcd_last_error() returns a thread-local description of the last failure.
 * Numerical guards of the reference (Σw = 0 fallbacks, singular 3x3 masks, displacement clamps) are reproduced
 * and never raised.
 *
 * Reference interface each entry replaces (paths relative to the reference repository root):
 *   pcd_grid_build / pcd_grid_*    Selector.__init__ KDTree snapshot          Pointcloud/Modules/Selector.py:138-141
 *   pcd_knn                         Selector.getKNNSelection                   Pointcloud/Modules/Selector.py:235-246
 *                                   torch_cluster.knn_graph (loop=False)       Pointcloud/Modules/GraphBuilder.py:60-63
 *                                   torch_geometric.nn.pool.knn (k=1)          Pointcloud/Modules/Utils.py:253-295
 *   pcd_radius_count / _fill        Selector.getPointsInRangeSelection(Vectorized)  Pointcloud/Modules/Selector.py:214-233
 *   pcd_nvt_csr                     Decompositionor.getBetterFilteredNVT       Pointcloud/Modules/Decompositionor.py:278-300
 *   pcd_nvt_normal_csr              Decompositionor.getNormalFilteredNVT       Pointcloud/Modules/Decompositionor.py:260-276
 *   pcd_pvt_normal_csr              Decompositionor.getNormalFilteredPVT       Pointcloud/Modules/Decompositionor.py:172-211
 *   pcd_vu_smooth                   Decomposition.getVUSmoothedNormals         Pointcloud/Modules/Decompositionor.py:92-106
 *   pcd_classify                    Decomposition.getNVTFeatures/getClasses    Pointcloud/Modules/Decompositionor.py:57-69
 *   pcd_pca_dense                   GraphBuilder.getPVTDecompositionWithKNN    Pointcloud/Modules/GraphBuilder.py:99-111
 *   pcd_step_csr                    Denoiser.{flat,edge,feature,corner,new,dummy}_step  Pointcloud/Modules/Denoiser.py:26-232
 *   pcd_edge_length_sum             TorchUtils.averageEdgeLength               Pointcloud/Modules/Utils.py:297-299
 *   pcd_nn_dist                     TorchUtils.Chamfer/Paper/HausdorffDistance Pointcloud/Modules/Utils.py:253-295
 *   pcd_mesh_update(_f32)           Mesh.updateVertices                        PatchGeneration/Modules/Mesh.py:377-418
 *   pcd_mesh_vta                    igl.vertex_triangle_adjacency (Mesh.__init__) PatchGeneration/Modules/Mesh.py:26
 *   pcd_mesh_tta / pcd_patch_radius / _select_count / _select_fill / _inputs
 *                                   PatchCollector.collectNetworkInput         PatchGeneration/Modules/PatchCollector.py:161-166
 *   pcd_mesh_face_geometry / _face_scale / _nbr_count / _nbr_fill / _filter(_f32) / _denoise(_f32)
 *                                   MeshNormalFiltering::updateFilteredNormalsWithPredictedNormal and its helpers
 *                                                       src/GCNDenoiser/GCNDenoiser/MeshNormalFiltering.cpp:47-244
 *   pcd_dgcnn_*                     DGCNN.forward (eval)                       PatchGeneration/Modules/Network/GCNModel.py:121-215
 *   pcd_dgcnn_train_* / _wgrad / _edgeconv_train(_backward)
 *                                   DGCNN.forward (train) and loss.backward()  PatchGeneration/Modules/Network/GCNModel.py:170-207
 *                                                                              PatchGeneration/Modules/NetworkController.py:120-136
 *   pcd_bdgcnn_create / _destroy / _workspace_bytes
 *                                   BetterDGCNN.__init__                       PatchGeneration/Modules/Network/GCNModel.py:217-256
 *   pcd_bdgcnn_forward(_deferred)   BetterDGCNN.forward (eval)                 PatchGeneration/Modules/Network/GCNModel.py:258-297
 *   pcd_bdgcnn_edgeconv(_scratch_bytes)
 *                                   one edge layer of it: convN + max          PatchGeneration/Modules/Network/GCNModel.py:270-281
 *   pcd_dgcnn_set_operands / _operands / _gemm_bf16, pcd_bdgcnn_edgeconv_bf16
 *                                   the opt-in bf16-operand inference mode of both networks (no counterpart)
 *   pcd_bdgcnn_train_workspace_bytes / _train_forward / _train_backward
 *                                   BetterDGCNN.forward (train) up to the pooling, and loss.backward() below it
 *                                                                              PatchGeneration/Modules/Network/GCNModel.py:258-287
 *                                                                              PatchGeneration/Modules/NetworkController.py:120-136
 *   pcd_denoiser_*                  Processor.denoise / getMyFeatureDecomposition / denoiseUntilMinimumError loop body
 *                                                                              Pointcloud/Modules/Processor.py:110-185
 *   pcd_orient_normals_mst          GraphBuilder.flipNormals (MST + DFS, host) Pointcloud/Modules/GraphBuilder.py:129-209
 *   pcd_orient_normals_mst_gpu      GraphBuilder.flipNormals (Borůvka MST + Euler-tour rooting + sign pointer jumping,
 *                                   device)                                    Pointcloud/Modules/GraphBuilder.py:129-209
 */
#ifndef PCD_H
#define PCD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status */
enum {
    PCD_OK = 0,
    PCD_ERR_ARG = -1,      /* bad argument (null pointer, size, unsupported k)     -> AssertionError/ValueError */
    PCD_ERR_OOM = -2,      /* device allocation failed                               */
    PCD_ERR_HIP = -3,      /* HIP runtime error                                      */
    PCD_ERR_STATE = -4,    /* object used in the wrong state                          */
    PCD_ERR_RCCL = -5      /* collective failure (multi-GPU slab mode)                */
};
const char* pcd_last_error(void);
int pcd_version(void);
/* hash of the sources and flags this library was built from (16 hex digits), e.g. to match profiles to builds */
const char* pcd_build_id(void);
/* Largest k supported by the kNN kernels (register top-k lists). */
int pcd_max_k(void);

/* ------------------------------------------------------------------ frozen snapshot (H1) */
typedef struct pcd_grid pcd_grid;
typedef struct {
    int64_t n;           /* snapshot points                           */
    int64_t cells;       /* occupied cells                            */
    int64_t table_slots; /* hash-table slots                          */
    float cell;          /* cell edge length                          */
    float origin[3];     /* cell (0,0,0) lower corner                  */
    int32_t dims[3];     /* cells per axis over the snapshot bbox       */
} pcd_grid_info_t;

/* Build the kNN index over a private copy of xyz[n][3] (fp32 device rows).  cell <= 0 picks the cell edge
 * so an occupied cell holds ~k_hint/2 points.  origin3 (host, nullable; needs cell > 0) pins the cell lattice:
 * grids of subsets built on one lattice order their points as subsequences of the full set's order (used by
 * the spatial slabs, so every rank breaks distance ties like one GPU would).  Synchronises `stream`.
 * Replaces the KDTree construction of Selector.__init__ (Pointcloud/Modules/Selector.py:138-141). */
int pcd_grid_build(const float* xyz, int64_t n, int k_hint, float cell, const float* origin3, void* stream,
                   pcd_grid** out);
/* The cell lattice pcd_grid_build would pick for xyz (origin = bbox minimum, cell edge), without building. */
int pcd_grid_params(const float* xyz, int64_t n, int k_hint, float cell, float* origin3, float* cell_out,
                    void* stream);
/* Another index over the SAME frozen snapshot as `src` (its points, in caller order) with another cell size (cell <= 0:
 * ~k_hint/2 points per occupied cell).  The fused loop indexes its snapshot with cells of about its list cap
 * (Processor picks k_hint = 2 x the cap): the re-anchoring searches then resolve fewer, fuller cells per query.
 * Synchronises `stream`. */
int pcd_grid_rebuild(const pcd_grid* src, int k_hint, float cell, void* stream, pcd_grid** out);
int pcd_grid_destroy(pcd_grid* g);
int pcd_grid_get_info(const pcd_grid* g, pcd_grid_info_t* out);
/* perm[r] = original index of the r-th point in the grid's spatial (Morton) order; int32 device [n]. */
int pcd_grid_perm(const pcd_grid* g, int32_t* perm, void* stream);

/* ------------------------------------------------------------------ kNN (H2) */
/* For each query row q[nq][3] the k nearest snapshot points, ascending (d², index): d² is the fp32
 * ((dx·dx) + (dy·dy)) + (dz·dz) of dx = q.x - p.x, ..., every step rounded, whatever the grid's cell size.
 *   idx_bits    32 or 64: element type of idx_out ([nq][k] row-major)
 *   sorted_ids  0: indices in the caller's original order, equal d² in ascending original index; 1: indices are ranks
 *               in the grid's spatial order (pcd_grid_perm maps them back), and equal d² come in ascending RANK --
 *               so the points of perm[rank] can differ from the sorted_ids = 0 list inside a group of exact ties
 *   exclude_self  1: query i is snapshot point i; drop it (torch_cluster.knn_graph loop=False semantics).  Entry i is
 *               dropped from the k + 1 best; a point with k + 1 or more exact duplicates of smaller index is not
 *               among them and loses the last of them instead.  Needs k + 1 <= min(n, pcd_max_k()), sorted_ids = 0
 *   d2_out      nullable fp32 [nq][k] squared distances
 * Tested bit for bit against brute force on every row of translated, degenerate (line, plane, one point, n = 1),
 * clustered, tied and 1e-18-scaled clouds for every k of the capacity ladder's rungs (tests/test_gpu_knn_edges.py). */
int pcd_knn(const pcd_grid* g, const float* q, int64_t nq, int k, void* idx_out, int idx_bits, int sorted_ids,
            int exclude_self, float* d2_out, void* stream);

/* Radius selection over the frozen snapshot (scipy query_ball_point semantics: float64 ((dx²+dy²)+dz²) <= r²,
 * members in ascending ORIGINAL index).  Two calls: count [nq] (int64), then, with the caller's exclusive prefix
 * sums offsets [nq+1] and total = offsets[nq], fill idx_out [total] (int64).  fill synchronises `stream`.
 * radii: fp32 [nq] per query (the reference builds a torch.float radius tensor, Selector.py:233), r = the fp32 value
 * converted exactly: r < 0 or NaN selects nobody, r = 0 the exact duplicates of q, r = +inf every point.  The kernels walk
 * every cell of the grid that the ball's box overlaps, occupied or not: a ball much larger than a sparse cloud's
 * occupied region costs its box's cell count. */
int pcd_radius_count(const pcd_grid* g, const float* q, int64_t nq, const float* radii, int64_t* counts,
                     void* stream);
int pcd_radius_fill(const pcd_grid* g, const float* q, int64_t nq, const float* radii, const int64_t* offsets,
                    int64_t total, int64_t* idx_out, void* stream);

/* Diagnostic: total work of a kNN(k) pass over q (spatial-order ids), summed over queries into out6 (device u64):
 * cells considered, cells probed in the hash, cells found, candidates scanned, sorted inserts (variant 0:
 * per-candidate insertion) or batch merges (variant 1: batched search, k > 8), extra rings. */
int pcd_knn_stats(const pcd_grid* g, const float* q, int64_t nq, int k, int variant, unsigned long long* out6,
                  void* stream);

/* ------------------------------------------------------------------ tensor voting (H5-H7, H15) */
/* CSR selection: segment r has centre ci[r] and neighbours nbr[off[r] .. off[r+1]); all int64 (torch long).
 * Better-filtered NVT: w_ij = acos(|clamp(normalize(v_j - v_i) . n_j)|) > rho, T_i = sum w n_j n_j^T / sum w, every
 * w := 1 when none votes; eigval [m][3] ascending, eigvec [m][3][3] columns.
 *   - a member coincident with the centre (v_j == v_i, e.g. the centre itself) has c = 0: it votes iff
 *     acos(0) > rho, i.e. for every rho < pi/2;  rho < 0: every member votes;  rho >= pi/2: none does (fallback)
 *   - the weight is multiplied in (w n_j) n_j^T as in the reference, so a member with a NaN or infinite normal makes
 *     the tensor of EVERY row that lists it NaN whether it votes or not (a NaN pair itself never votes for rho >= 0);
 *     a zero normal votes like any other (c = 0) and adds nothing but its count to sum w
 *   - an empty segment (off[r] == off[r+1]) is 0 / 0: NaN eigenvalues (and the eigenvectors eigh makes of a NaN
 *     tensor: first row (1, 0, 0), the rest NaN) */
int pcd_nvt_csr(const float* pos, const float* n, int64_t npts, const int64_t* ci, const int64_t* off,
                const int64_t* nbr, int64_t m, float rho, float* eigval, float* eigvec, void* stream);
/* Normal-filtered NVT (CPSD): w_ij = acos(clamp(n_i . n_j)) <= rho; T_i = sum w n_j n_j^T / sum w, or n_i n_i^T when
 * no neighbour votes.  Same CSR and outputs as pcd_nvt_csr. */
int pcd_nvt_normal_csr(const float* n, int64_t npts, const int64_t* ci, const int64_t* off, const int64_t* nbr,
                       int64_t m, float rho, float* eigval, float* eigvec, void* stream);
/* Normal-filtered PVT (CPSD): same vote; every w := 1 when none votes; weighted covariance of v_j about their
 * weighted mean / sum w; an empty neighbourhood gets the reference's cross-product samples.  Outputs as above. */
int pcd_pvt_normal_csr(const float* pos, const float* n, int64_t npts, const int64_t* ci, const int64_t* off,
                       const int64_t* nbr, int64_t m, float rho, float* eigval, float* eigvec, void* stream);
/* eigval [m][3] ascending, eigvec [m][3][3] (columns), n [m][3] -> f_n [m][3] */
int pcd_vu_smooth(const float* eigval, const float* eigvec, const float* n, int64_t m, float tau, float damp,
                  float* out, void* stream);
/* features nullable [m][3] = (planarity, linearity, sphericity); classes int64 [m] */
int pcd_classify(const float* eigval, int64_t m, float scale, float* features, int64_t* classes, void* stream);
/* The kernels' two 3x3 symmetric eigen-solvers on DEVICE tensors t6 [m][6] = (a00, a01, a02, a11, a12, a22), as
 * the fused loop compiles them (torch.linalg.eigh at Decompositionor.py:300 is what both replace):
 *   solver 0: the LAPACK ssyevd restatement (NVT1, the public ops) -> w [m][3] ascending, vec [m][3][3] columns
 *   solver 1: NVT2's fixed-sweep Jacobi on the hardware rcp/sqrt estimates -> w [m][3] ascending, vec [m][3] = the
 *             smallest eigenvalue's unit eigenvector (sign arbitrary; classes and edge_step use it through y yᵀ)
 *             Its rotations use 1 / a_pq: an off-diagonal below ~2^-128 is skipped as negligible, which holds for
 *             NVT2's tensors (sums of unit normals, trace >= 1) and not for a tensor that is subnormal as a whole;
 *             the eigenvector is defined for lambda_max >= 2^-30 (below, any tensor, the zero one included, can give NaN).
 *             NaN in -> all three eigenvalues NaN.
 * For tests: pins NVT2's solver against the LAPACK one on the same tensors. */
int pcd_eigh3_batch(const float* t6, int64_t m, int solver, float* w, float* vec, void* stream);
/* Covariance of the k neighbours nbr[i*k .. i*k+k) about their own mean; eigval [n][3], eigvec [n][3][3]. */
int pcd_pca_dense(const float* pos, int64_t n, const int64_t* nbr, int k, float* eigval, float* eigvec,
                  void* stream);

/* ------------------------------------------------------------------ position updates (H9-H12) */
enum { PCD_STEP_FLAT = 0, PCD_STEP_EDGE = 1, PCD_STEP_FEATURE = 2, PCD_STEP_CORNER = 3, PCD_STEP_NEW = 4,
       PCD_STEP_DUMMY = 5 };
/* One Denoiser.*_step over a CSR selection: out [m][3] new positions of the centres.
 * edge_vectors [npts][3] is required for PCD_STEP_EDGE only.  Uses a device workspace it allocates
 * internally for the global (flat/new) reductions; stream-ordered.
 *   - the step di = alpha (x - v_i) is taken iff |di| < d for edge, feature, corner and new (strict) and iff
 *     |di| <= d for flat; a NaN step is never taken; a system with an exactly zero pivot (inv_ex's info != 0) keeps v_i
 *   - flat and new reduce their global centre and delta over nbr[0 .. off[m]): off[0] must be 0.  delta = 0 (every
 *     row one point) and a NaN position among the rows (NaN centre; the NaN distances are dropped, delta = 0) give
 *     weights of 0 or NaN: flat moves nobody, new keeps v_i to rounding
 *   - an empty segment: flat (0 / 0), edge and corner (zero system) keep v_i; feature and new solve (I + n n^T) x =
 *     (I + n n^T) v_i, i.e. v_i to rounding */
int pcd_step_csr(int kind, const float* pos, const float* n, const float* edge_vectors, int64_t npts,
                 const int64_t* ci, const int64_t* off, const int64_t* nbr, int64_t m, float d, float alpha,
                 float* out, void* stream);

/* ------------------------------------------------------------------ metrics (H4, H17) */
/* sum over rows of ||pos[b[e]] - pos[a[e]]|| in fp64 -> *sum_out (device double) */
int pcd_edge_length_sum(const float* pos, const int64_t* a, const int64_t* b, int64_t e, double* sum_out,
                        void* stream);
/* for each query: squared distance to / index of its nearest snapshot point (k = 1) */
int pcd_nn_dist(const pcd_grid* g, const float* q, int64_t nq, float* d2_out, int64_t* idx_out, void* stream);

/* ------------------------------------------------------------------ mesh vertex update (H18) */
/* k Jacobi sweeps of v_i += Σ_{f∋i} Σ_{c∈f} n_f (n_f·(v_c − v_i)) / (3 deg_i), fp64, in place on v [nv][3].
 * f [nf][3] int64, fn [nf][3] f64, vf/ni = igl vertex_triangle_adjacency (VF [3nf], NI [nv+1]) int64. */
int pcd_mesh_update(double* v, int64_t nv, const int64_t* f, const double* fn, int64_t nf, const int64_t* vf,
                    const int64_t* ni, int k, void* stream);
/* The same k Jacobi sweeps in fp32 (v [nv][3] f32 in place, f [nf][3] int32, fn [nf][3] f32, vf / ni int32): vertex and
 * normal rows as float4 and faces as int4 internally, one thread per vertex.  Not bitwise the fp64 path: within fp32
 * rounding of it (tests/test_gpu_mesh.py). */
int pcd_mesh_update_f32(float* v, int64_t nv, const int32_t* f, const float* fn, int64_t nf, const int32_t* vf,
                        const int32_t* ni, int k, void* stream);
/* igl.vertex_triangle_adjacency (the reference's Mesh.__init__, PatchGeneration/Modules/Mesh.py:26) on the device:
 * f [nf][3] (int32 or int64 per f_bits) -> vf [3 nf] (the incident faces of each vertex in increasing face order) and
 * ni [nv + 1] offsets, int32 or int64 per out_bits.  PCD_ERR_ARG for a face index outside [0, nv).  Synchronises. */
int pcd_mesh_vta(const void* f, int f_bits, int64_t nf, int64_t nv, void* vf, void* ni, int out_bits, void* stream);

/* ------------------------------------------------------------------ guided bilateral normal filtering (mesh) */
/* The reference's network-free mesh denoiser, src/GCNDenoiser/GCNDenoiser/MeshNormalFiltering.cpp:170-244.  fp64
 * entries take plain rows and int64 indices; the _f32 entries take fp32 rows and int32 indices (float4 internally).
 * vf / ni are the vertex->face CSR of pcd_mesh_vta.  Nothing here synchronises unless it says so. */
/* MeshDenoisingBase::getFaceCentroid / getFaceArea / getFaceNormal (MeshDenoisingBase.cpp:24-65), normals oriented as
 * Mesh.getFaceNormals (PatchGeneration/Modules/Mesh.py:110-114): centroid [nf][3] = ((p0+p1)+p2)/3, area [nf] =
 * 0.5 |(p1-p0) x (p2-p1)|, normal [nf][3] = the unit cross product, zero for a face of zero area. */
int pcd_mesh_face_geometry(const double* v, int64_t nv, const int64_t* f, int64_t nf, double* centroid, double* area,
                           double* normal, void* stream);
/* MeshNormalFiltering::getRadius / getSigmaS with multiple = 1 (MeshNormalFiltering.cpp:134-168): out2 (device) =
 * {mean |c_f - c_g| over the ordered pairs of faces sharing an edge, the number of pairs}; {0, 0} without a pair.
 * Deterministic fp64 reduction (block partials, then one block). */
int pcd_mesh_face_scale(const double* centroid, const int64_t* f, int64_t nf, const int64_t* vf, const int64_t* ni,
                        int64_t nv, double* out2, void* stream);
/* MeshNormalFiltering::getRadiusBasedFaceNeighbor (MeshNormalFiltering.cpp:47-78; mode 0) or the vertex-based set of
 * MeshDenoisingBase::getFaceNeighbor (MeshDenoisingBase.cpp:75-92; mode 1), centre included (include_central_face).
 * Count: the search of face i runs inside rows[cap_off[i] .. cap_off[i+1]), which the caller sizes with an upper bound
 * on the row (radius mode: the number of centroids within the radius; vertex mode: the degrees of its corners), and
 * counts [nf] gets the row lengths.  PCD_ERR_ARG when a row does not fit (nothing is written past a segment).
 * Synchronises.  Fill: with offsets [nf+1] = the exclusive prefix sums of counts, nbr_out [offsets[nf]] gets every
 * row in ascending face index (the reference keeps its search order instead). */
int pcd_mesh_nbr_count(const double* centroid, const int64_t* f, int64_t nf, const int64_t* vf, const int64_t* ni,
                       int64_t nv, int mode, double radius, const int64_t* cap_off, int64_t* rows, int64_t* counts,
                       void* stream);
int pcd_mesh_nbr_fill(const int64_t* rows, const int64_t* cap_off, const int64_t* offsets, int64_t nf,
                      int64_t* nbr_out, void* stream);
/* One pass of the filter (MeshNormalFiltering.cpp:207-236) over the CSR (off, nbr): out_i = normalize(sum_j src_j A_j
 * exp(-|c_i-c_j|^2 / 2 sigma_s^2) exp(-|g_i-g_j|^2 / 2 sigma_r^2)), sigma_s = multiple_sigma_s * scale[0] with scale
 * the device output of pcd_mesh_face_scale.  A zero or non-finite sum keeps src_i; a neighbour of zero area weighs 0
 * and is not read; a centre of zero area gets the zero normal.  _f32: total = off[nf]. */
int pcd_mesh_filter(const double* centroid, const double* area, const double* guided, const double* src, int64_t nf,
                    const int64_t* off, const int64_t* nbr, double sigma_r, double multiple_sigma_s,
                    const double* scale, double* out, void* stream);
int pcd_mesh_filter_f32(const float* centroid, const float* area, const float* guided, const float* src, int64_t nf,
                        const int32_t* off, const int32_t* nbr, int64_t total, float sigma_r, float multiple_sigma_s,
                        const double* scale, float* out, void* stream);
/* MeshNormalFiltering::updateFilteredNormalsWithPredictedNormal (MeshNormalFiltering.cpp:170-244): normal_iterations
 * times {face geometry of the current mesh, sigma_s, one filter pass (src = guided in the first iteration, the current
 * face normals afterwards), vertex_iterations sweeps of pcd_mesh_update}, in place on v; normals_out [nf][3] gets the
 * last filtered normals.  guided null: the input mesh's own face normals guide (bilateral normal filtering).  The
 * neighbourhoods (off, nbr) are the caller's, built once on the input mesh.  Vertices in no face keep their position.
 * normal_iterations == 0 or an empty mesh: PCD_OK, nothing written. */
int pcd_mesh_denoise(double* v, int64_t nv, const int64_t* f, int64_t nf, const int64_t* vf, const int64_t* ni,
                     const int64_t* off, const int64_t* nbr, const double* guided, int normal_iterations,
                     int vertex_iterations, double sigma_r, double multiple_sigma_s, double* normals_out, void* stream);
int pcd_mesh_denoise_f32(float* v, int64_t nv, const int32_t* f, int64_t nf, const int32_t* vf, const int32_t* ni,
                         const int32_t* off, const int32_t* nbr, int64_t total, const float* guided,
                         int normal_iterations, int vertex_iterations, float sigma_r, float multiple_sigma_s,
                         float* normals_out, void* stream);

/* ------------------------------------------------------------------ GCN network input (patches) */
/* The reference's PatchCollector.collectNetworkInput per face: selectPaperPatch / createPatch / Patch.alignPatch /
 * Patch.toGraph (PatchGeneration/Modules/Mesh.py:289-307, 473-506), RotationMatrix (RotationMatrix.py:9-35) and
 * FileDataset.file2input (Network/DataUtils.py:41-70).  Everything is fp64 with int64 indices; vf / ni are the
 * vertex->face CSR of pcd_mesh_vta, tt the edge adjacency of pcd_mesh_tta.  Nothing synchronises unless it says so. */
/* igl.triangle_triangle_adjacency(f)[0]: tt [nf][3], slot e = the face across the edge (f[e], f[(e+1)%3]), -1 on a
 * boundary edge and on an edge shared by more than two faces.  f int32 / int64 per f_bits, tt per out_bits.
 * PCD_ERR_ARG for a face index outside [0, nv).  Synchronises. */
int pcd_mesh_tta(const void* f, int f_bits, int64_t nf, int64_t nv, void* tt, int out_bits, void* stream);
/* Per requested face faces[i] (Mesh.py:300-304): centre [n][3] = the mean of its corners, radius [n] =
 * k sqrt(mean area of {face} U edge-neighbours U their edge-neighbours), absent neighbours skipped, the areas summed
 * as numpy.sum does.  mean_area [n] (may be null) gets that mean: the reference takes the root with libm's
 * pow(x, 0.5), which is not correctly rounded, so a caller that needs its last bit redoes k * pow(mean, 0.5) on the
 * host (pcd_host_patch_radius); radius holds k * sqrt(mean), correctly rounded.  A face outside [0, nf) gets radius 0. */
int pcd_patch_radius(const double* v, int64_t nv, const int64_t* f, int64_t nf, const int64_t* tt,
                     const int64_t* faces, int64_t n, double k, double* centre, double* radius, double* mean_area,
                     void* stream);
/* Patch selection (Mesh.py:157-163, 242-251): patch i = every face with a vertex u, |v_u - centre_i| < radius_i
 * (strict, rounded as numpy.linalg.norm rounds), rows ascending and duplicate-free.  g: a grid built over the nv
 * vertices rounded to fp32; the kernels walk the cells that overlap the box of half-width radius_i + widen around the
 * centre (widen: a bound on the fp32 rounding of the vertices and the centres, e.g. 4e-7 max|coordinate|) and put
 * every row found there to the exact fp64 test on v.  Count: counts [n].  Fill: off [n+1] = the exclusive prefix sums
 * of counts, patch_faces [capacity].  PCD_ERR_ARG when off[n] > capacity or a row does not have its counted length,
 * and then nothing is written to patch_faces.  Fill synchronises. */
int pcd_patch_select_count(const pcd_grid* g, double widen, const double* v, int64_t nv, const int64_t* f, int64_t nf,
                           const int64_t* vf, const int64_t* ni, const double* centre, const double* radius, int64_t n,
                           int64_t* counts, void* stream);
int pcd_patch_select_fill(const pcd_grid* g, double widen, const double* v, int64_t nv, const int64_t* f, int64_t nf,
                          const int64_t* vf, const int64_t* ni, const double* centre, const double* radius, int64_t n,
                          const int64_t* off, int64_t capacity, int64_t* patch_faces, void* stream);
/* radius[i] = k * pow(mean_area[i], 0.5) with the C library's pow on host arrays: the reference's `k * mean ** 0.5`
 * on a numpy scalar, bit for bit (see pcd_patch_radius). */
int pcd_host_patch_radius(const double* mean_area, int64_t n, double k, double* radius);
/* Alignment and graph rows of the patches (off [n+1], patch_faces [total]) of faces [n], one workgroup per patch:
 * centre on the mean of the patch's vertices, scale the farthest one to distance 1, T = sum_{j != centre} (A_j / max A)
 * exp(-3 |c_j - c_i|) n'_j n'_j^T, rot [n][3][3] = its eigenvectors as rows in descending eigenvalue order (fp64 Jacobi),
 * row 0 agreeing with the centre face's normal, row 1 with its largest component positive, row 2 = row 0 x row 1; then
 * per patch the first 64 faces' rows of 20 columns {centroid 3, normal 3, area, edge-neighbours in the patch, corners
 * 9, index columns 3}, zero-padded, of the rotated patch.  adjacency 0: the reference's index columns (the slot whose
 * neighbour is local face 1, else 63); 1: the local edge-neighbours inside the window.  out: [n][64][20] (or
 * [n][20][64] with channels_first) float64 / float32 per out_bits, the float32 being the float64 value rounded.
 * centre_index [n]: the local index of the face in its own patch, -1 if absent; eig [n][3]: the eigenvalues,
 * descending.  A face outside [0, nf) or an empty patch gives padding rows and the identity.  Bitwise repeatable. */
int pcd_patch_inputs(const double* v, int64_t nv, const int64_t* f, int64_t nf, const int64_t* tt, const int64_t* vf,
                     const int64_t* ni, const int64_t* faces, int64_t n, const int64_t* off, const int64_t* patch_faces,
                     int64_t total, int adjacency, int out_bits, int channels_first, void* out, double* rot,
                     int64_t* centre_index, double* eig, void* stream);

/* ------------------------------------------------------------------ fused denoise loop (H8, H13, H14) */
typedef struct pcd_denoiser pcd_denoiser;
typedef struct {
    int k;               /* feature kNN size (getMyFeatureDecomposition N), reference default 16       */
    int k_update;        /* update kNN size, reference 8                                                 */
    float rho;           /* NVT angle threshold, reference 5*pi/12                                       */
    float tau;           /* VU smoothing eigenvalue threshold, reference 0.3                             */
    float damp;          /* VU smoothing dampening d, reference 3                                        */
    float class_scale;   /* planarity scale in getClasses, reference 0.2                                 */
    float d;             /* displacement clamp (2 * mean edge length in Processor.denoise)              */
    int nphases;         /* number of (class, step, alpha) phases, Gauss-Seidel in this order           */
    int phase_class[3];  /* 0 flat, 1 edge, 2 corner                                                     */
    int phase_kind[3];   /* PCD_STEP_*                                                                   */
    float phase_alpha[3];
    int jacobi;          /* 0: Gauss-Seidel across the phases (Processor.denoise, Processor.py:127-138); 1: every phase
                            reads the iteration's input positions (Jacobi across classes: temp_pos, the thesis driver
                            "Ours", PostProcessing.ipynb:1069-1090)                                          */
    float clamp_global;  /* > 0: a moved point keeps its new position only while it lies within clamp_global of its
                            position at pcd_denoiser_load, else it keeps the previous iteration's position
                            (PostProcessing.ipynb:1088-1089, mask = ||temp_pos - original_pos|| < d); 0: off */
} pcd_denoise_params;

/* sizeof(pcd_denoise_params) as this library was built: a binding checks its mirror against it (a struct that
 * is shorter than the library's would be read past its end). */
int pcd_denoise_params_size(void);
/* g: the frozen snapshot, fewer than 2^27 points (134M; larger clouds run as spatial slabs, pcd_slab). */
int pcd_denoiser_create(const pcd_grid* g, int k_max, pcd_denoiser** out);
int pcd_denoiser_destroy(pcd_denoiser* dn);
/* pos, n: caller rows [N][3] (original order, N = grid n) -> internal spatial order */
int pcd_denoiser_load(pcd_denoiser* dn, const float* pos, const float* n, void* stream);
int pcd_denoiser_iterate(pcd_denoiser* dn, const pcd_denoise_params* p, int iterations, void* stream);
/* back to original order; any output pointer may be null.  classes int64 [N] and edge vectors [N][3]
 * are those of the LAST iteration's NVT2; f_n is the last smoothed normal field (= n after iterate). */
int pcd_denoiser_store(pcd_denoiser* dn, float* pos, float* n, int64_t* classes, float* edge_vectors,
                       void* stream);
/* Seeded search (default ON): iterations after the first cap the acceptance threshold at the largest key of
 * the previous iteration's stored list (re-keyed at the current positions) and run the capped search (LDS row
 * buffer, one sorted drain).  Results are identical either way (tested bitwise); it only changes the work done.
 * reset_seed forgets the stored list, so the next iterate() runs unseeded. */
int pcd_denoiser_set_seeding(pcd_denoiser* dn, int enable);
/* LDS row windows (default ON): NVT1, NVT2 and the flat phase stage a window of rows around each block's own rows
 * in LDS and read neighbours from it when they fall inside.  OFF reads every neighbour from global memory: same
 * results bit for bit (the parity tests check this); a diagnostic / reference switch. */
int pcd_denoiser_set_windows(pcd_denoiser* dn, int enable);
int pcd_denoiser_reset_seed(pcd_denoiser* dn);
/* Anchored search (default ON, applies to seeded searches with k, k_update <= 32): each point keeps an anchor --
 * a position, the exact 2K nearest snapshot points there (K = the list cap 8/16/32) and their 2K-th distance D.
 * When the current k-th distance over that list is below D - |q - anchor|, the list's top k IS the snapshot's
 * k-NN (no grid search); the few queries that fail are re-anchored by a wave-per-query grid search (the rare
 * query whose quantised ordering is ambiguous by the exact-key search).  Same results (tested bitwise).  Anchors depend only on the snapshot: they survive load(); reset_seed drops them. */
int pcd_denoiser_set_anchoring(pcd_denoiser* dn, int enable);
/* Diagnostics: rows re-anchored by the last anchored kNN stage (-1: none ran).  Synchronises `stream`. */
int pcd_denoiser_anchor_stats(pcd_denoiser* dn, int64_t* redo_rows, void* stream);
/* Diagnostics of the last anchored kNN stage: out4 = {rows re-anchored, of which spilled from the quantised-key
 * search to the exact-key wave search, of those: with a cap box over 4096 cells, with an ambiguous quantised order
 * or too few points under a dense cap}; -1 when no anchored stage ran.  Synchronises `stream`. */
int pcd_denoiser_tile_stats(pcd_denoiser* dn, int64_t* out4, void* stream);
/* Profiling aid: with timing enabled, every iteration (up to 256) records HIP events on its stream between the
 * stages; get_timing returns each stage's elapsed ms AVERAGED over the iterations recorded since set_timing or
 * the previous get_timing, then starts over.  Slots: anchor test (+ redo-list select), re-anchoring search, exact-key
 * spill search, NVT1 (the four make up K1: kNN + NVT1; a non-anchored K1 reports its whole time in the NVT1 slot),
 * NVT2, phase 0, phase 1, phase 2, finish, -.  enable = 2 records the K1 stage's two events only (one slot: K1's
 * ms), for a timed region that needs K1's time without the other stages' events (~4 us each on the stream). */
int pcd_denoiser_set_timing(pcd_denoiser* dn, int enable);
int pcd_denoiser_get_timing(pcd_denoiser* dn, float* ms_out, int n_slots, int* n_written);
/* Device error word -> status: PCD_ERR_STATE if a kNN list held an invalid entry or (spatial slabs) a query's
 * k-ball left the coverage box.  Synchronises `stream`.  store() calls it. */
int pcd_denoiser_check(pcd_denoiser* dn, void* stream);
/* The raw device error word behind check (bit 0: invalid list entry, bit 1: a k-ball left the coverage box; with bit
 * 1, bit 2: a row without a coverage sphere failed -- the band -- and bit 3: a sphere row failed), without raising:
 * the spatial-slab driver re-plans on bit 1.  Synchronises `stream`. */
int pcd_denoiser_status(pcd_denoiser* dn, int* bits, void* stream);
/* What the failed coverage checks lacked, for a re-plan that grows only that (spatial slabs; no reference
 * counterpart): band_excess = the farthest any sphere-less row's k-ball reached past the coverage box
 * (0: none failed), sphere_ratio = the largest (|q - centre| + d_k) / R over the sphere rows that failed (0: none).
 * Synchronises `stream`. */
int pcd_denoiser_coverage_excess(pcd_denoiser* dn, float* band_excess, float* sphere_ratio, void* stream);
/* The kNN list the last K1 stage stored (the snapshot's `cols` nearest of each point's current position, in
 * (distance, index) order = getKNNSelection's columns, Selector.py:235-246), in caller order with ORIGINAL snapshot
 * indices: out int64 [N][cols], cols <= the stored list length (max(k, k_update) of the last iteration).  The loop
 * works in its grid's spatial order: exactly equal fp32 d² come in ascending RANK of that grid (pcd_grid_perm), as
 * pcd_knn's sorted_ids = 1 gives them, not in ascending original index. */
int pcd_denoiser_lists(pcd_denoiser* dn, int64_t* out, int cols, void* stream);
/* Parity probe of the fused NVT2 stage (off by default; enabling allocates [N] float4).  While on, every NVT2 stage
 * also writes, per row, the eigenvalues of the reference's normalised tensor T / Σw (Decompositionor.py:299-300:
 * getBetterFilteredNVT's eigval, ascending) and Σw, as that kernel computes them.  probe_store copies them out in
 * caller order: nvt2_eig4 [N][4] = (λ0, λ1, λ2, Σw); rows no NVT2 stage wrote hold NaN.  The edge vectors (the
 * smallest eigenvalue's eigenvector) come out through pcd_denoiser_store. */
int pcd_denoiser_set_probe(pcd_denoiser* dn, int enable);
int pcd_denoiser_probe_store(pcd_denoiser* dn, float* nvt2_eig4, void* stream);
/* Exact NVT2 (default OFF; no allocation).  The default NVT2 stage leaves the tensor unnormalised and solves it with
 * a fixed-sweep Jacobi: its classes match the reference, its edge vectors are LAPACK's only to ~5e-7/gap, with an
 * arbitrary sign.  While ON, every NVT2 stage (iterate, pcd_denoiser_stage, pcd_slab_iterate) runs the reference's
 * second vote as it runs the first (Processor.py:110-117: getBetterFilteredNVT on the filtered normals,
 * Decompositionor.py:278-300): T / Σw and LAPACK's ssyevd, the arithmetic of NVT1, bit for bit.  store()'s
 * edge_vectors are then eigvec[..., 0] with LAPACK's sign, and probe_store's eigenvalues are those of T / Σw as
 * computed, not a quotient.  Costs NVT2 time; pcd_denoise_params is unchanged. */
int pcd_denoiser_set_exact_nvt2(pcd_denoiser* dn, int enable);
/* Processor.getMyFeatureDecomposition (Processor.py:110-117) on the loaded state from the fused stages: K1 (the kNN
 * of the current positions, NVT1, VU smoothing -> f_n) and the exact NVT2 on f_n (Decompositionor.py:278-300),
 * whatever set_exact_nvt2 says.  Outputs in caller order, each nullable: eigval [N][3] ascending, eigvec [N][3][3]
 * (columns: eigvec[i][r][c] = component r of eigenvector c, pcd_nvt_csr's layout), f_n [N][3], classes int64 [N]
 * (p->class_scale).  Uses p->k, k_update (the stored list length), rho, tau, damp, class_scale; same limits and
 * argument checks as iterate.  It moves no position, does not rebind the normals and leaves the classes / edge
 * vectors of the last iteration alone: an iterate() after it computes what it would have computed without it.
 * pcd_denoiser_lists then returns this call's kNN lists, and the probe (when on) its eigenvalues and Σw.  Working buffers ([N] x 49 B) are allocated on the first
 * call and freed at destroy.  Ends with pcd_denoiser_check (synchronises `stream`). */
int pcd_denoiser_decompose(pcd_denoiser* dn, const pcd_denoise_params* p, float* eigval, float* eigvec, float* f_n,
                           int64_t* classes, void* stream);

/* ---- spatial slabs (multi-GPU): the same loop over a rank's own points with a halo ----
 * The grid holds the rank's points plus halo snapshot points owned by other ranks.  Only the ACTIVE rows are
 * queried and updated; the caller keeps the halo rows' state current with pack/unpack + its own transport
 * (RCCL) between stages, and all-reduces the flat-phase sums (sum) and delta (max) between the PHASE_* stages:
 *   per iteration: KNN_NVT1 -> exchange FN -> NVT2 -> per phase [flat/new: PHASE_SUM(red=double[4]) ->
 *   all-reduce sum -> PHASE_CENTRE(red) -> PHASE_MAXDIST(red=float[1]) -> all-reduce max] -> PHASE_APPLY(red or
 *   null) -> exchange POS -> FINISH.  pcd_denoiser_iterate runs the same sequence with no exchange. */
enum { PCD_FIELD_POS = 0, PCD_FIELD_NRM = 1, PCD_FIELD_FN = 2, PCD_FIELD_EDGE = 3 };
enum { PCD_STAGE_KNN_NVT1 = 0, PCD_STAGE_NVT2 = 1, PCD_STAGE_PHASE_SUM = 2, PCD_STAGE_PHASE_CENTRE = 3,
       PCD_STAGE_PHASE_MAXDIST = 4, PCD_STAGE_PHASE_APPLY = 5, PCD_STAGE_FINISH = 6 };
/* rows: device int32 [n_rows] of spatial-order rows (ascending), kept by the caller; null = all rows. */
int pcd_denoiser_set_rows(pcd_denoiser* dn, const int32_t* rows, int64_t n_rows);
/* host lo3/hi3: the box the local snapshot covers (null: no check). */
int pcd_denoiser_set_coverage(pcd_denoiser* dn, const float* lo3, const float* hi3);
/* Spatial slabs: per-point coverage spheres (DEVICE float [n], caller order; 0 = none; null: clear).  A point whose
 * k-ball leaves the coverage box is still covered when the ball lies inside the sphere of radius radii[i] around its
 * position at load -- the slab driver adds every snapshot point of such a sphere to the local snapshot (the sparse
 * points near a cut, whose balls would otherwise widen every rank's halo).  Replaces nothing in the reference (it is
 * the exactness condition of Selector.getKNNSelection's KD-tree query over a partitioned snapshot, Selector.py:243). */
int pcd_denoiser_set_coverage_spheres(pcd_denoiser* dn, const float* radii, void* stream);
/* one stage; red: device scalars as above (SUM/CENTRE: double[4] Σx,Σy,Σz,count; MAXDIST out / APPLY in:
 * float[1] delta, nullable = local value). */
int pcd_denoiser_stage(pcd_denoiser* dn, const pcd_denoise_params* p, int stage, int phase, void* red,
                       void* stream);
/* state rows <-> packed device float4 buffers (field PCD_FIELD_*; POS = current positions, EDGE = NVT2's edge vectors,
 * written by a test to feed the edge phase the reference's own).  FN rows unpacked
 * between K1 and NVT2 must be another rank's K1 output (unit vectors: NVT2's vote margin assumes it). */
int pcd_denoiser_pack(pcd_denoiser* dn, int field, const int32_t* rows, int64_t n, float* out4, void* stream);
int pcd_denoiser_unpack(pcd_denoiser* dn, int field, const int32_t* rows, int64_t n, const float* in4,
                        void* stream);

/* ---- the CPSD ("Martin") comparison driver in one call (PostProcessing.ipynb:1041-1062) ----
 * Per iteration on the loaded state: kNN(k_update) lists of the current positions, the radius-r selection over the
 * frozen snapshot (scipy query_ball_point membership, Selector.py:214-233) with the normal-filtered NVT + VU smoothing
 * (Processor.getMartinFeatureDecomposition, Processor.py:102-108) and PVT, VU features (Decompositionor.py:84-85), then
 * flat_step / edge_step / corner_step with alpha[3] and the per-step clamp, Jacobi across classes, the global clamp
 * ||pos - pos at load|| < d, n := f_n.  No host synchronisation per iteration; one at the end of the call. */
typedef struct {
    float r;             /* radius of the selection, the notebook's r = d                               */
    float rho;           /* vote angle of both normal filters, 0.9                                      */
    float tau;           /* VU smoothing and VU-feature threshold, 0.3                                  */
    float damp;          /* VU smoothing dampening, 3                                                   */
    float d;             /* global clamp (PostProcessing.ipynb:1060)                                    */
    float step_clamp;    /* per-step displacement clamp, d * 20000                                      */
    float alpha[3];      /* flat, edge, corner step: 0.1, 1, 1                                          */
    int k_update;        /* update kNN size, 8                                                          */
} pcd_cpsd_params;
int pcd_cpsd_iterate(pcd_denoiser* dn, const pcd_cpsd_params* p, int iterations, void* stream);

/* ---- spatial slabs in one call per iteration (the RCCL communicator, halo exchange and scalar
 * all-reduces live in the library; PyTorch only sets up the ranks) ----
 * A pcd_comm is the slab transport: RCCL over xGMI (pcd_comm_create from a unique id rank 0 made with pcd_comm_id and
 * the caller broadcast), or host callbacks (pcd_comm_create_host: any transport the caller has, e.g. gloo in tests;
 * every exchange is staged through pinned host memory and handed to the callback). */
typedef struct pcd_comm pcd_comm;
enum { PCD_DT_F32 = 0, PCD_DT_F64 = 1, PCD_DT_I32 = 2 };
enum { PCD_OP_SUM = 0, PCD_OP_MAX = 1 };
typedef struct {
    void* user;
    /* Exchange float4 rows with npeers peers: to peers[q] send rows [send_off[q], send_off[q+1]) of `send`, from it
     * receive rows [recv_off[q], recv_off[q+1]) into `recv` (HOST memory, 4 floats a row).  Return 0 on success. */
    int (*exchange)(void* user, int npeers, const int* peers, const float* send, const int64_t* send_off, float* recv,
                    const int64_t* recv_off);
    /* In-place all-reduce of count elements of dtype PCD_DT_* with PCD_OP_* over every rank (HOST memory). */
    int (*allreduce)(void* user, void* buf, int count, int dtype, int op);
} pcd_host_transport;
/* bytes of an RCCL unique id (ncclUniqueId) */
int pcd_comm_id_bytes(void);
/* rank 0: a fresh RCCL unique id into id_out [pcd_comm_id_bytes()] for the caller to broadcast */
int pcd_comm_id(void* id_out);
/* every rank (collective, on its own HIP device): the RCCL communicator of `world` ranks from rank 0's id */
int pcd_comm_create(const void* id, int world, int rank, pcd_comm** out);
int pcd_comm_create_host(const pcd_host_transport* t, int world, int rank, pcd_comm** out);
int pcd_comm_destroy(pcd_comm* c);
/* world size, this rank, and the transport (PCD_COMM_RCCL / PCD_COMM_HOST) the communicator was made with */
enum { PCD_COMM_HOST = 0, PCD_COMM_RCCL = 1 };
int pcd_comm_info(const pcd_comm* c, int* world, int* rank, int* transport);
/* Point-to-point bulk copy of DEVICE memory, stream-ordered: send send_bytes from `send` to rank send_peer and
 * receive recv_bytes into `recv` from rank recv_peer (a peer of -1: nothing that way).  Byte counts are multiples of
 * 4.  The slab driver's coordinator (rank 0, the only rank holding the whole cloud, as the reference's single process
 * does: Processor.py:115-121) hands each rank its slab + halo of the snapshot with it, and collects the owned state
 * for a re-plan.  RCCL: ncclSend / ncclRecv in one group.  Host transport: staged through host memory and handed to
 * the exchange callback as ceil(bytes / 16) float4 rows.  Synchronises `stream` on the host transport only. */
int pcd_comm_sendrecv(pcd_comm* c, int send_peer, const void* send, int64_t send_bytes, int recv_peer, void* recv,
                      int64_t recv_bytes, void* stream);
/* in-place all-reduce of device scalars (the flat phase's Σ and δ, Denoiser.py:106-107), stream-ordered */
int pcd_allreduce_scalars(pcd_comm* c, void* buf, int count, int dtype, int op, void* stream);
/* Halo routes of this rank's denoiser: for each of npeers peers (host arrays), n_send[q] own rows to send and
 * n_recv[q] halo rows to receive; send_rows / recv_rows: device int32 spatial-order rows, peer after peer (copied).
 * own_lo3 / own_hi3 (host, nullable): the OWNED slab (no halo) -- with it, NVT2 and the phases run the rows whose
 * k-ball stays strictly inside it while an exchange is in flight.  Synchronises `stream`. */
int pcd_denoiser_set_routes(pcd_denoiser* dn, int npeers, const int* peers, const int64_t* n_send,
                            const int32_t* send_rows, const int64_t* n_recv, const int32_t* recv_rows,
                            const float* own_lo3, const float* own_hi3, void* stream);
/* one field (PCD_FIELD_*) of the send rows -> the peers' halo rows, stream-ordered */
int pcd_halo_exchange(pcd_denoiser* dn, pcd_comm* c, int field, void* stream);
/* `iterations` slab iterations of Processor.denoise's body (Processor.py:123-139) over the active rows: K1, f_n
 * exchange, NVT2, the phases with their all-reduces and position exchanges, n := f_n -- one call, every exchange
 * overlapped with the rows that need no halo data (the exchange runs on a stream of the library's own; later
 * calls on this denoiser wait for it).  Same result bit for bit as the staged sequence above. */
int pcd_slab_iterate(pcd_denoiser* dn, pcd_comm* c, const pcd_denoise_params* p, int iterations, void* stream);
/* Read-set exchange (on by default; PCD_SLAB_READSET=0 in the environment at pcd_denoiser_set_routes, or on = 0
 * here: every halo row in every exchange).  pcd_slab_iterate's K1 stores the kNN lists first; each rank marks the
 * halo rows the lists of its band rows (k-ball not inside the owned slab) hold, sends that mask to each peer (one bit
 * per route row), and the peers send position + normal of exactly those rows while NVT1 runs the no-halo rows; the
 * iteration's f_n and position exchanges move the same rows, and no exchange trails the iteration.  The halo rows a
 * list does not hold are not kept current (pcd_halo_exchange refreshes every one).  Needs the anchored K1 (list cap
 * <= 32, seeding and anchoring on) and >= 2k local rows on every rank. */
int pcd_denoiser_set_readset(pcd_denoiser* dn, int on);
/* since pcd_denoiser_set_routes: read-set iterations and the send / receive rows they moved, summed */
int pcd_denoiser_readset_stats(const pcd_denoiser* dn, int64_t* iterations, int64_t* send_rows, int64_t* recv_rows);

/* ------------------------------------------------------------------ DGCNN forward (inference, fp32) */
/* DGCNN(k, init_dims = 17, emb_dims, dropout, output_channels) in eval(): three edge convolutions over the input's
 * three index columns (17 -> 64 -> 64 -> 128), three over a k-nearest-neighbour graph rebuilt in feature space before
 * each (128 -> 256 -> 256 -> 256), conv7 (1024 -> emb) over the concatenation, max and mean over the 64 nodes, and the
 * head 2 emb -> 512 -> 256 -> 64 -> output_channels.  Batch norms use their running statistics (folded on the host in
 * double with each layer's own eps, rounded once); dropout is the identity.  A patch's output depends on that patch
 * only and is the same bits in any batch, at any place in it, in every run.  Neighbour ties go to the lower index. */
typedef struct pcd_dgcnn pcd_dgcnn;
typedef struct {
    /* HOST or DEVICE pointers, row-major fp32.  conv 1-7: [rows][cols] = [out][2 in] (conv7: [emb][1024]);
     * batch norms 1-10 (weight, bias, running mean, running var, eps, channels); linear 1-4: [out][in], bias [out]
     * (linear1 has none: lin_b[0] must be null). */
    const float* conv_w[7];
    int32_t conv_rows[7], conv_cols[7];
    const float* bn_weight[10];
    const float* bn_bias[10];
    const float* bn_mean[10];
    const float* bn_var[10];
    double bn_eps[10];
    int32_t bn_len[10];
    const float* lin_w[4];
    const float* lin_b[4];
    int32_t lin_rows[4], lin_cols[4];
} pcd_dgcnn_weights;
typedef struct {
    /* optional DEVICE outputs of pcd_dgcnn_forward (null: not wanted) */
    float* cat;          /* [b][1024][64] the six layer outputs, concatenated (conv7's input)        */
    int32_t* lists;      /* [3][b][64][k] the neighbour lists of layers 4-6, ascending distance      */
    float* pooled;       /* [b][2 emb]    max, then mean over the nodes                              */
    float* h1;           /* [512][b], [256][b], [64][b]: the head's hidden layers, channels first    */
    float* h2;
    float* h3;
} pcd_dgcnn_debug;
/* Packs the weights on the device (copies; the caller's arrays are not kept).  PCD_ERR_ARG for init_dims != 17 (the
 * forward slices rows 0:17), k outside [1, 64] and every shape that does not fit the layer table.  Synchronous. */
int pcd_dgcnn_create(const pcd_dgcnn_weights* w, int k, int init_dims, int emb_dims, int output_channels,
                     pcd_dgcnn** out);
int pcd_dgcnn_destroy(pcd_dgcnn* m);
/* bytes of caller-owned device scratch a forward of b patches needs (about 393 KB a patch) */
int pcd_dgcnn_workspace_bytes(const pcd_dgcnn* m, int64_t b, int64_t* bytes);
/* inputs [b][20][64] fp32 (rows 0:17 features, 17:20 the index columns as floats, truncated as .long() does) ->
 * out [b][output_channels].  An index outside [0, 63] or NaN is never used as an address: PCD_ERR_ARG naming the
 * first such patch, nothing computed.  NaN / Inf features propagate to their own patch's output only.  A short
 * or not 16-byte-aligned workspace is PCD_ERR_ARG and nothing is written.  Stream-ordered; synchronises `stream` once, after the index
 * check.  Replaces DGCNN.forward (PatchGeneration/Modules/Network/GCNModel.py:170-215). */
int pcd_dgcnn_forward(const pcd_dgcnn* m, const float* inputs, int64_t b, float* out, void* workspace,
                      int64_t workspace_bytes, const pcd_dgcnn_debug* debug, void* stream);
/* The same without waiting for the device: a bad index column is not refused but recorded -- first_bad (DEVICE
 * int32[1], set to PCD_DGCNN_NO_BAD_PATCH by the caller before the first chunk) takes the minimum of
 * patch_base + patch over the bad patches, whose outputs are then computed from the clamped index 0 (no address is
 * ever formed from a bad value).  The caller reads first_bad once, after its last chunk (predictNormals does).  The
 * launches can be captured in a graph. */
#define PCD_DGCNN_NO_BAD_PATCH 0x7f7f7f7f
int pcd_dgcnn_forward_deferred(const pcd_dgcnn* m, const float* inputs, int64_t b, float* out, void* workspace,
                               int64_t workspace_bytes, const pcd_dgcnn_debug* debug, int32_t* first_bad,
                               int64_t patch_base, void* stream);
/* Stages, for tests.  knn: x [b][channels][64] -> lists [b][64][k] (the k nearest rows in feature space, self
 * included, ascending (d2, index)).  edgeconv: layer 1-6 of the model on x [b][Cin][64] with the given lists
 * [b][64][list_len] (entries are taken mod 64) -> out [b][Cout][64]; synchronises `stream`. */
int pcd_dgcnn_knn(const float* x, int64_t b, int channels, int k, int32_t* lists, void* stream);
int pcd_dgcnn_edgeconv(const pcd_dgcnn* m, int layer, const float* x, int64_t b, const int32_t* lists, int list_len,
                       float* out, void* stream);
/* The network's GEMM y = w . x on the exact-f32 MFMA: w [M][K]; nodes = 64: x [b][K][64] -> y [b][M][64]; nodes = 1:
 * x [K][b] -> y [M][b].  epilogue 0: plain; 1: LeakyReLU_0.2(s[m] y + t[m]); 2 (nodes = 64): that, then max and mean
 * over each patch's 64 columns -> y [b][2 M]; 3: s[m] y + t[m].  Synchronises `stream`. */
int pcd_dgcnn_gemm(const float* w, const float* x, int m_rows, int k_cols, int64_t b, int nodes, int epilogue,
                   const float* s, const float* t, float* y, void* stream);
/* epilogue 4 of pcd_dgcnn_gemm: y += w . x, added into what y holds (the data gradients of the training step) */

/* ------------------------------------------------------------------ BetterDGCNN (the layer table from the caller) */
/* BetterDGCNN(l_e, l_d, l_l, channel_sizes, k, init_dims = 17, dropout, output_channels) of GCNModel.py:217-297: the
 * network above with every count and width from the caller.  Convolution i (1-based, i <= l_e + l_d) is an edge
 * convolution 2 C_{i-1} -> C_i with C_0 = 17 and C_i = channel_sizes[i - 1]; the first l_e run over the three index
 * columns, the next l_d over the k nearest rows of their own input (with l_e = 0 the first search is on rows 0:17 of
 * the input, and the index columns are never read nor checked).  Their outputs are concatenated ([Ccat][64], Ccat =
 * C_1 + .. + C_{l_e + l_d}); convolution l_e + l_d + 1 maps Ccat -> C, followed by max and mean over the nodes; linear
 * j < l_l maps C -> C' (input doubled for j = 1, a bias for j > 1) with batch norm l_e + l_d + 1 + j, the last linear
 * channel_sizes[-1] -> output_channels.  The trunk's LeakyReLU slope is 0.2; the head's is F.leaky_relu's default
 * 0.01 (GCNModel.py:291).  DGCNN is the table 3, 3, 4, [64, 64, 128, 256, 256, 256, emb, 512, 256, 64] with head slope
 * 0.2, and runs through the same code.  The guarantees on bits are those of pcd_dgcnn_forward / pcd_dgcnn_train_*.
 * Bounds (PCD_ERR_ARG naming the argument otherwise): l_e + l_d in [1, 16], l_l in [2, 16] (the reference fails
 * outside the lower ones), channel_sizes[i] in [1, 4096] for the edge layers (so Ccat <= 65536) and [1, 65536] after
 * them, k in [1, 64], init_dims = 17, output_channels in [1, 4096].  With them 2 Cin Cout <= 2^25 and every width times
 * 64 nodes stay far inside int32; everything multiplied by the batch (b <= 2^20) is computed in int64. */
#define PCD_DGCNN_MAX_EDGE_LAYERS 16
#define PCD_DGCNN_MAX_LINEARS 16
#define PCD_DGCNN_MAX_EDGE_WIDTH 4096
#define PCD_DGCNN_MAX_WIDTH 65536
#define PCD_BDGCNN_HEAD_SLOPE 0.01f
typedef struct {
    int32_t l_e, l_d, l_l;
    const int32_t* channel_sizes;    /* HOST, [l_e + l_d + l_l] */
    int32_t k, init_dims, output_channels;
} pcd_dgcnn_table;
typedef struct {
    /* HOST arrays of the table's lengths; what they point to as in pcd_dgcnn_weights (HOST or DEVICE, row-major fp32).
     * conv [l_e + l_d + 1]: [out][2 in], the last [C][Ccat]; batch norms [l_e + l_d + l_l]; linears [l_l] (lin_b[0]
     * must be null). */
    const float* const* conv_w;
    const int32_t *conv_rows, *conv_cols;
    const float* const* bn_weight;
    const float* const* bn_bias;
    const float* const* bn_mean;
    const float* const* bn_var;
    const double* bn_eps;
    const int32_t* bn_len;
    const float* const* lin_w;
    const float* const* lin_b;
    const int32_t *lin_rows, *lin_cols;
} pcd_bdgcnn_weights;
typedef struct {
    /* optional DEVICE outputs (null: not wanted) */
    float* cat;          /* [b][Ccat][64]                                                            */
    int32_t* lists;      /* [l_d][b][64][k] the neighbour lists of the dynamic layers                */
    float* pooled;       /* [b][2 C]                                                                 */
    float* const* h;     /* HOST array of l_l - 1 DEVICE pointers: the hidden layers [width][b]      */
} pcd_bdgcnn_debug;
/* As pcd_dgcnn_create / _destroy / _workspace_bytes / _forward / _forward_deferred, for a table from the caller
 * (BetterDGCNN.__init__ and .forward, GCNModel.py:217-297).  The handle is a pcd_dgcnn. */
int pcd_bdgcnn_create(const pcd_dgcnn_table* table, const pcd_bdgcnn_weights* w, pcd_dgcnn** out);
int pcd_bdgcnn_destroy(pcd_dgcnn* m);
int pcd_bdgcnn_workspace_bytes(const pcd_dgcnn* m, int64_t b, int64_t* bytes);
int pcd_bdgcnn_forward(const pcd_dgcnn* m, const float* inputs, int64_t b, float* out, void* workspace,
                       int64_t workspace_bytes, const pcd_bdgcnn_debug* debug, void* stream);
int pcd_bdgcnn_forward_deferred(const pcd_dgcnn* m, const float* inputs, int64_t b, float* out, void* workspace,
                                int64_t workspace_bytes, const pcd_bdgcnn_debug* debug, int32_t* first_bad,
                                int64_t patch_base, void* stream);
/* Stage, for tests: one edge layer by (c_in, c_out) in eval() -- DEVICE w [c_out][2 c_in], the folded batch norm s, t
 * [c_out], x [b][c_in][64], lists [b][64][list_len] (entries taken mod 64) -> out [b][c_out][64]
 * (convN + max of GCNModel.py:270-281).  fused: PCD_FUSED_OFF runs the GEMM and the max over the lists as two kernels
 * (DGCNN's path), PCD_FUSED_ON as one kernel that keeps the product in LDS -- the same bits; PCD_ERR_ARG unless
 * 2 c_out <= 128, the GEMM's tile height -- and PCD_FUSED_AUTO as pcd_bdgcnn_forward chooses.  scratch: null -- the
 * packed weight and the product come from the stream's memory pool and the call synchronises `stream`; or DEVICE
 * memory, 16-byte aligned, of pcd_bdgcnn_edgeconv_scratch_bytes(c_in, c_out, b) bytes or more -- nothing is allocated
 * and nothing waits (what tools/better_dgcnn_probe.py times). */
#define PCD_FUSED_OFF 0
#define PCD_FUSED_ON 1
#define PCD_FUSED_AUTO 2
int pcd_bdgcnn_edgeconv(const float* w, const float* s, const float* t, int c_in, int c_out, const float* x, int64_t b,
                        const int32_t* lists, int list_len, int fused, float* out, void* scratch, int64_t scratch_bytes,
                        void* stream);
/* The size serves pcd_bdgcnn_edgeconv and pcd_bdgcnn_edgeconv_bf16 alike (the bf16 weight lies where the packed
 * float32 weight would; its rows are padded to 8 k, which shows in the size only for c_in < 7). */
int pcd_bdgcnn_edgeconv_scratch_bytes(int c_in, int c_out, int64_t b, int64_t* bytes);

/* ------------------------------------------------------------------ bf16 operands (opt-in, inference only) */
/* With PCD_OPERANDS_BF16 the trunk's GEMMs -- every edge layer with Cin >= 32 and the pooled convolution -- run on
 * v_mfma_f32_32x32x16_bf16: the activations (float32 in memory, as before: workspace sizes do not change) and the
 * packed float32 weights [W_a ; W_b - W_a], W7 are rounded to bf16 (nearest even; NaN and Inf kept) and the products
 * are accumulated in float32.  The folded batch norms, LeakyReLU, max over the lists and the pooling stay float32,
 * in the order of the float32 mode; edge layers with Cin < 32 (the first) and the head stay on the float32 kernel.
 * A patch's output still depends on that patch alone: the same bits in any batch, at any place in it, in every run.
 * What is lost is precision: the outputs differ from the float32 mode's at the 1e-2 level.
 * set_operands serves handles of either create entry; the first switch to bf16 allocates and rounds the weights
 * (synchronous); switching back uses the float32 weights again, bit for bit.  PCD_ERR_ARG for any other value.
 * pcd_dgcnn_forward(_deferred), pcd_bdgcnn_forward(_deferred) and pcd_dgcnn_edgeconv follow the handle's setting; the
 * training entries take no handle and are float32. */
#define PCD_OPERANDS_F32 0
#define PCD_OPERANDS_BF16 1
int pcd_dgcnn_set_operands(pcd_dgcnn* m, int operands);
int pcd_dgcnn_operands(const pcd_dgcnn* m, int* operands);
/* Stages, for tests.  gemm_bf16: pcd_dgcnn_gemm with nodes = 64 on the bf16 kernel -- float32 w [M][K] and
 * x [b][K][64] are rounded as the forward rounds them; epilogues 0-3; any K >= 1 (no Cin < 32 exception).
 * edgeconv_bf16: pcd_bdgcnn_edgeconv on the bf16 kernel, whatever c_in is; fused ON = OFF bit for bit. */
int pcd_dgcnn_gemm_bf16(const float* w, const float* x, int m_rows, int k_cols, int64_t b, int epilogue, const float* s,
                        const float* t, float* y, void* stream);
int pcd_bdgcnn_edgeconv_bf16(const float* w, const float* s, const float* t, int c_in, int c_out, const float* x,
                             int64_t b, const int32_t* lists, int list_len, int fused, float* out, void* scratch,
                             int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------ DGCNN training (train(), fp32) */
/* conv1-7 and the max / mean pooling of DGCNN.forward with self.training (GCNModel.py:170-207): batch norms take the
 * batch's statistics (biased variance over every edge of the batch; sums in double, fixed order) and update their
 * running buffers as nn.BatchNorm does (momentum, unbiased variance, num_batches_tracked).  The head (linear1-4,
 * bn8-10, dropout) is not here.  Neighbour lists are constants of the backward; there is no gradient with respect
 * to the inputs.  The same batch, weights and buffers give the same bits in every run; the bits depend on the batch. */
typedef struct {
    /* DEVICE pointers.  conv 1-7 weights as pcd_dgcnn_weights; batch norms 1-7.  bn_mean / bn_var / bn_tracked are
     * updated in place (null: not updated; mean and var go together). */
    const float* conv_w[7];
    const float* bn_weight[7];
    const float* bn_bias[7];
    float* bn_mean[7];
    float* bn_var[7];
    int64_t* bn_tracked[7];
    double bn_eps[7];
    double bn_momentum[7];
} pcd_dgcnn_train_params;
typedef struct {
    /* DEVICE outputs, overwritten: conv [out][2 in] (conv7 [emb][1024]), batch norm weight and bias gradients */
    float* conv_w[7];
    float* bn_weight[7];
    float* bn_bias[7];
} pcd_dgcnn_train_grads;
/* bytes of caller-owned device scratch a training step of b patches needs: the packed weights plus about
 * (1.2 MB + 260 B x emb) a patch; it carries the forward's state to the backward */
int pcd_dgcnn_train_workspace_bytes(int k, int emb_dims, int64_t b, int64_t* bytes);
/* inputs [b][20][64] -> pooled [b][2 emb] (max, then mean over the nodes, of conv7's activations).  Packs the split
 * weights from prm on the stream (nothing goes to the host), keeps what the backward needs in the workspace and, if
 * lists is not null, copies the neighbour lists of layers 4-6 to it ([3][b][64][k]).  A bad index column is
 * PCD_ERR_ARG as in pcd_dgcnn_forward, before any buffer is updated; a short or misaligned workspace is PCD_ERR_ARG
 * with nothing written.  Synchronises `stream` once, after the index check.
 * Replaces dgcnn.train(); dgcnn(inputs) up to GCNModel.py:207 (NetworkController.py:120-122). */
int pcd_dgcnn_train_forward(const pcd_dgcnn_train_params* prm, int k, int emb_dims, const float* inputs, int64_t b,
                            float* pooled, void* workspace, int64_t workspace_bytes, int32_t* lists, void* stream);
/* d_pooled [b][2 emb] -> the gradients of conv1-7's weights and bn1-7's weight and bias, from the workspace the
 * forward of the same (k, emb_dims, inputs, b) left.  conv7_w: the weight the forward ran with.  Consumes the
 * workspace (conv7's stored product becomes its gradient in place): one backward per forward.  Stream-ordered, never
 * waits.  Replaces loss.backward() below the pooling (NetworkController.py:135). */
int pcd_dgcnn_train_backward(int k, int emb_dims, const float* inputs, int64_t b, const float* d_pooled,
                             const float* conv7_w, void* workspace, int64_t workspace_bytes,
                             const pcd_dgcnn_train_grads* grads, void* stream);
/* Stages, for tests.  wgrad: dw [M][K] = sum over the b x 64 columns of dy [b][M][64] x [b][K][64]^T on the exact-f32
 * MFMA; the patches are split into runs of pcd_dgcnn_wgrad_split(b) whose partial products are added in run order
 * (the conv weight gradients of loss.backward()).  Synchronises `stream`. */
int pcd_dgcnn_wgrad(const float* dy, const float* x, int m_rows, int k_cols, int64_t b, float* dw, void* stream);
int pcd_dgcnn_wgrad_split(int64_t b, int64_t* patches_per_split);
/* One edge layer (1-6) in train() on x [b][Cin][64] with the given lists [b][64][list_len] (entries taken mod 64):
 * w [Cout][2 Cin], gamma / beta [Cout] -> out [b][Cout][64], argmax [b][Cout][64] (the first maximal list slot),
 * stats [3][Cout] doubles (mean, biased variance, 1 / sqrt(var + eps)); running_mean / running_var / tracked (null:
 * none) are updated.  convN + max of GCNModel.py:178-200.  Synchronises `stream`. */
int pcd_dgcnn_edgeconv_train(const float* w, const float* gamma, const float* beta, double eps, double momentum,
                             float* running_mean, float* running_var, int64_t* tracked, int layer, const float* x,
                             int64_t b, const int32_t* lists, int list_len, float* out, uint8_t* argmax, double* stats,
                             void* stream);
/* Its backward (the forward is run again inside; no buffer is touched): g [b][Cout][64] = dL/d out -> dab
 * [b][2 Cout][64] (dA rows, then dB rows), dgamma / dbeta [Cout], dw [Cout][2 Cin], and, if dx is not null,
 * dx [b][Cin][64] with the lists held constant.  Synchronises `stream`. */
int pcd_dgcnn_edgeconv_train_backward(const float* w, const float* gamma, const float* beta, double eps, int layer,
                                      const float* x, int64_t b, const int32_t* lists, int list_len, const float* g,
                                      float* dab, float* dgamma, float* dbeta, float* dw, float* dx, void* stream);
/* The training step for a table from the caller (BetterDGCNN.forward with self.training, GCNModel.py:258-287, and
 * loss.backward() below the pooling): as pcd_dgcnn_train_workspace_bytes / _forward / _backward, the arrays of
 * l_e + l_d + 1 entries.  Batch statistics run over N = b x 64 x 3 edges in a static layer, b x 64 x k in a dynamic
 * one and b x 64 in the pooled convolution.  lists: [l_d][b][64][k]. */
typedef struct {
    const float* const* conv_w;
    const float* const* bn_weight;
    const float* const* bn_bias;
    float* const* bn_mean;
    float* const* bn_var;
    int64_t* const* bn_tracked;
    const double* bn_eps;
    const double* bn_momentum;
} pcd_bdgcnn_train_params;
typedef struct {
    float* const* conv_w;
    float* const* bn_weight;
    float* const* bn_bias;
} pcd_bdgcnn_train_grads;
int pcd_bdgcnn_train_workspace_bytes(const pcd_dgcnn_table* table, int64_t b, int64_t* bytes);
int pcd_bdgcnn_train_forward(const pcd_dgcnn_table* table, const pcd_bdgcnn_train_params* prm, const float* inputs,
                             int64_t b, float* pooled, void* workspace, int64_t workspace_bytes, int32_t* lists,
                             void* stream);
/* pool_conv_w: the weight of convolution l_e + l_d + 1 the forward ran with */
int pcd_bdgcnn_train_backward(const pcd_dgcnn_table* table, const float* inputs, int64_t b, const float* d_pooled,
                              const float* pool_conv_w, void* workspace, int64_t workspace_bytes,
                              const pcd_bdgcnn_train_grads* grads, void* stream);

/* ------------------------------------------------------------------ normal orientation (host) */
/* GraphBuilder.flipNormals: Kruskal MST on cost 1-|n_i·n_j| over the directed edge list (a[e] -> b[e],
 * host int64 arrays), then DFS from argmax z flipping n_dst when n_src·n_dst < cos(7π/12).  HOST memory,
 * n [npts][3] fp32 modified in place. */
int pcd_orient_normals_mst(const float* pos, float* n, int64_t npts, const int64_t* a, const int64_t* b,
                           int64_t e);
/* Same contract and bit-identical result on DEVICE memory (pos [npts][3], n [npts][3] in place, a/b [e] int64),
 * ordered on `stream`; synchronises the stream before returning.  The minimum spanning forest is unique under
 * keys (cost, edge index), which is the host's stable Kruskal order, and each node's sign is a composition of
 * per-edge maps {identity, negate, +1} from the root's sign, so the DFS visit order never matters.
 * PCD_ERR_ARG for an out-of-range edge index; npts and e must be < 2^32. */
int pcd_orient_normals_mst_gpu(const float* pos, float* n, int64_t npts, const int64_t* a, const int64_t* b,
                               int64_t e, void* stream);

/* ------------------------------------------------------------------ host builds of the per-point math */
/* The exact __host__ __device__ code the kernels run, compiled for the CPU (HOST pointers); for tests.
 *   t6 [m][6] = (a00, a01, a02, a11, a12, a22) -> w [m][3] ascending, v [m][3][3] columns (LAPACK ssyevd signs) */
int pcd_host_eigh3(const float* t6, int64_t m, float* w, float* v);
int pcd_host_vu_smooth(const float* w, const float* v, const float* n, int64_t m, float tau, float damp, float* out);
/* getBetterFilteredNVT's tensor T (before eigh) for CSR rows: centres ci [m], neighbours nbr[off[r] .. off[r+1]),
 * pos / n [.][3] -> t6 [m][6] (a00, a01, a02, a11, a12, a22); the fused kernels' vote and sums, on the host. */
int pcd_host_nvt_tensor(const float* pos, const float* n, const int64_t* ci, const int64_t* off, const int64_t* nbr,
                        int64_t m, float rho, float* t6);
/* a9 [m][3][3] row-major, b3 [m][3] -> x3 [m][3] = inv_ex(A) b as the position steps compute it, ok [m] (0 when
 * inv_ex reports info != 0, i.e. an exactly zero pivot; x untouched = 0) */
int pcd_host_solve3(const float* a9, const float* b3, int64_t m, float* x3, int32_t* ok);
/* torch.linalg.inv_ex (Denoiser.py:43, 80, 163, 210) restated for 3x3: a9 [m][3][3] -> inv9 [m][3][3], ok [m] as
 * above (inv untouched = 0 where ok = 0).  The position steps' arithmetic (pcd_device.h inv3_ref), on the host. */
int pcd_host_inv3(const float* a9, int64_t m, float* inv9, int32_t* ok);
/* Denoiser.*_step (PCD_STEP_*) over CSR rows, the kernels' step functions on the host: out [m][3]; delta = the global
 * flat / new-step delta (Denoiser.py:107, 138). */
int pcd_host_step_csr(int kind, const float* pos, const float* n, const float* edge_vectors, const int64_t* ci,
                      const int64_t* off, const int64_t* nbr, int64_t m, float delta, float d, float alpha, float* out);

#ifdef __cplusplus
}
#endif
#endif /* PCD_H */
