/*
 * bevfusion_hip.h -- C ABI of libbevfusion_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the native operators of the reference
 * (lhn0323/BEVFUSION-3D_object_detection, paths relative to the reference root,
 *  BF/ = projects/BEVFusion/bevfusion/).  Each entry point names the reference interface it
 * replaces.  The reference binds its ops with pybind11 + at::Tensor
 * (BF/ops/bev_pool/src/bev_pool.cpp:89-94, BF/ops/voxel/src/voxelization.cpp:6-11); this
 * library exposes the same operations with plain pointers and sizes so that any host
 * (ctypes, pybind, C++) can bind them.  See INTEGRATION.md for the reference-side stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter name ends in _host
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream)
 *   - return value: 0 = ok, negative = error (BFHIP_E_*); message via bfhip_last_error()
 *   - no entry point allocates, frees or synchronises the device; temporaries live in the
 *     caller-provided workspace (size from the matching *_workspace_bytes()).  All entry
 *     points are therefore hipGraph-capturable.
 *   - outputs are caller-allocated and written in place, like the reference's
 *     hard_voxelize/dynamic_voxelize (BF/ops/voxel/voxelize.py:47-66)
 */
#ifndef BEVFUSION_HIP_H_
#define BEVFUSION_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BFHIP_OK 0
#define BFHIP_E_INVALID (-1)   /* bad argument (shape, alignment, unsupported size) */
#define BFHIP_E_WORKSPACE (-2) /* workspace too small */
#define BFHIP_E_LAUNCH (-3)    /* hipGetLastError() after a launch was not hipSuccess */

#define BFHIP_REDUCE_SUM 0  /* enum order of BF/ops/voxel/src/scatter_points_cuda.cu:7 */
#define BFHIP_REDUCE_MEAN 1
#define BFHIP_REDUCE_MAX 2

/* op ids of the optional profiler */
#define BFHIP_OP_BEV_POOL_FWD 0
#define BFHIP_OP_BEV_POOL_BWD 1
#define BFHIP_OP_HARD_VOXELIZE 2 /* whole 7-launch pipeline */
#define BFHIP_OP_DYNAMIC_VOXELIZE 3
#define BFHIP_OP_LIFT_SPLAT_FWD 4
#define BFHIP_OP_LIFT_SPLAT_BWD 5
#define BFHIP_OP_SPCONV_FWD 6
#define BFHIP_OP_SPCONV_BWD 7 /* dgrad */
#define BFHIP_OP_RULEBOOK 8
#define BFHIP_OP_BEV_AUX 9
#define BFHIP_OP_SCATTER_FWD 10
#define BFHIP_OP_SCATTER_BWD 11
#define BFHIP_OP_SPCONV_WGRAD 12 /* whole op: offset counts + main kernel + partial-slab reduce */
#define BFHIP_OP_RASTER 13
#define BFHIP_OP_SPCONV_WGRAD_MAIN 14 /* the dominant kernel alone (what rocprofv3 lists as spconv_wgrad64p_kernel) */
/* dense ops: recorded only at profile level 2 (bfhip_profile_enable(2)): ~280 scopes per training step */
#define BFHIP_OP_CONV2D_FWD 15   /* bfhip_conv2d_fwd */
#define BFHIP_OP_CONV2D_DGRAD 16 /* bfhip_conv2d_dgrad: weight transpose + implicit GEMM */
#define BFHIP_OP_CONV2D_WGRAD 17 /* bfhip_conv2d_wgrad: main kernel + slab reduce */
#define BFHIP_OP_BN2D_FWD 18     /* bfhip_bn2d_fwd / _fwd_partials: statistics, finalize, apply */
#define BFHIP_OP_BN2D_BWD 19     /* bfhip_bn2d_bwd: reduce, finalize, apply */
#define BFHIP_OP_CONV2D_PW_FWD 20   /* bfhip_conv2d_fwd calls served by the pointwise kernel (1x1, stride 1): HBM-bound GEMMs over the pixel matrix */
#define BFHIP_OP_CONV2D_PW_DGRAD 21 /* bfhip_conv2d_dgrad(_wt) calls served by the pointwise kernel */
#define BFHIP_OP_COUNT 24

int bfhip_abi_version(void);
/* thread-local, valid until the next failing call on the same thread */
const char *bfhip_last_error(void);

/* Optional profiler used by bench.py for the roofline line: when enabled, every entry point
 * records a HIP event pair ON ITS OWN STREAM around its dominant kernel launch (memsets and
 * helper launches excluded).  bfhip_profile_read() synchronises the recorded events (the only
 * call in this library that blocks) and returns the accumulated milliseconds and launch count. */
void bfhip_profile_enable(int on);
int bfhip_profile_read(int op, double *sum_ms_host, long long *count_host, int reset);

/* ---------------------------------------------------------------------------------------
 * bev_pool  (replaces bev_pool_ext.bev_pool_forward / bev_pool_backward,
 *            BF/ops/bev_pool/src/bev_pool.cpp:22-87, kernels BF/ops/bev_pool/src/bev_pool_cuda.cu:20-98)
 *   x        f32[n, c]   rows sorted so that each interval is contiguous
 *   geom     i32[n, 4]   (x, y, z, b) per row; only the first row of an interval is read
 *   starts   i32[m], lengths i32[m]
 *   out      f32[b, d, h, w, c]  cell (b, z, x, y) <- sum of the interval's rows, other cells 0
 * fwd zero-fills `out` itself (the reference's wrapper does torch::zeros, bev_pool.cpp:38-40).
 * bwd: x_grad[row] = out_grad[cell(interval(row))].  If `intervals_cover_all_rows` is 0 the
 * whole x_grad is zero-filled first (reference: torch::zeros, bev_pool.cpp:76-78); pass 1 when
 * starts/lengths partition [0, n) (always true for intervals built from ranks) to skip it.
 * m_dev: optional device int holding the live interval count (<= m); NULL = use m.
 * --------------------------------------------------------------------------------------- */
int bfhip_bev_pool_fwd(const float *x, const int32_t *geom, const int32_t *starts,
                       const int32_t *lengths, float *out, int n, int c, int m, int b, int d,
                       int h, int w, const int32_t *m_dev, void *stream);
int bfhip_bev_pool_bwd(const float *out_grad, const int32_t *geom, const int32_t *starts,
                       const int32_t *lengths, float *x_grad, int n, int c, int m, int b, int d,
                       int h, int w, int intervals_cover_all_rows, const int32_t *m_dev,
                       void *stream);

/* ---------------------------------------------------------------------------------------
 * voxelization  (replaces voxel_layer.dynamic_voxelize / hard_voxelize,
 *                BF/ops/voxel/src/voxelization.h:58-96; CPU kernels voxelization_cpu.cpp:8-144,
 *                CUDA kernels voxelization_cuda.cu:24-373)
 *   points f32[n, f] (f >= 3), voxel_size_host f32[3], coors_range_host f32[6] (xyzxyz min,max)
 * dynamic: coors i32[n,3] = floor((p - min)/voxel) per axis in IEEE fp32 (subtract, divide),
 *          (-1,-1,-1) when any axis is outside [0, grid) -- the CPU path's convention
 *          (voxelization_cpu.cpp:34-39).
 * hard   : first-come grouping, deterministic, identical to hard_voxelize_cpu:
 *          voxel id = order of the voxel's first point; <= max_points points kept per voxel in
 *          point order; voxels beyond max_voxels dropped.  voxels f32[max_voxels, max_points, f]
 *          and num_points_per_voxel must be zero-filled by the caller (voxelize.py:51-53);
 *          coors i32[max_voxels,3] in (x,y,z).  The voxel count is written to *voxel_num_dev.
 * --------------------------------------------------------------------------------------- */
int bfhip_dynamic_voxelize(const float *points, int32_t *coors, int n, int f,
                           const float *voxel_size_host, const float *coors_range_host,
                           void *stream);
size_t bfhip_hard_voxelize_workspace_bytes(int n, int max_points, int max_voxels);
int bfhip_hard_voxelize(const float *points, int n, int f, float *voxels, int32_t *coors,
                        int32_t *num_points_per_voxel, const float *voxel_size_host,
                        const float *coors_range_host, int max_points, int max_voxels,
                        void *workspace, size_t workspace_bytes, int32_t *voxel_num_dev,
                        void *stream);

/* ---------------------------------------------------------------------------------------
 * dynamic scatter  (replaces voxel_layer.dynamic_point_to_voxel_forward / _backward,
 *   BF/ops/voxel/src/scatter_points_cuda.cu:183-308) and the hard-voxel mean (BF/bevfusion.py:251-253)
 *   feats f32[N,C], coors i32[N,3]; rows with any negative coordinate are dropped (:202).
 *   voxel rows come out in ascending lexicographic (c0,c1,c2) order, like at::unique_dim(sorted).
 *   fwd outputs are sized for N rows; counts_dev i32[3] = {M voxels, valid points, key-overflow flag
 *   (coordinates must be < 2^21)}.  Sums run in point order (deterministic).
 *   bwd: sum/mean -> gather (mean divides by count); max -> gradient to the lowest-index arg-max.
 * --------------------------------------------------------------------------------------- */
size_t bfhip_dynamic_scatter_workspace_bytes(int N);
int bfhip_dynamic_scatter_fwd(const float *feats, const int32_t *coors, int N, int C, int reduce_type,
                              float *voxel_feats, int32_t *voxel_coors, int32_t *point2voxel,
                              int32_t *voxel_count, int32_t *counts_dev, void *workspace,
                              size_t workspace_bytes, void *stream);
size_t bfhip_dynamic_scatter_bwd_workspace_bytes(int M, int C);
int bfhip_dynamic_scatter_bwd(float *grad_feats, const float *grad_voxel_feats, const float *feats,
                              const float *voxel_feats, const int32_t *point2voxel,
                              const int32_t *voxel_count, int N, int M, int C, int reduce_type,
                              void *workspace, size_t workspace_bytes, void *stream);
int bfhip_voxel_mean(const float *voxels, const int32_t *num_points, int M, int P, int F, float *out,
                     void *stream);

/* ---------------------------------------------------------------------------------------
 * camera frustum -> BEV plan  (replaces BaseViewTransform.get_geometry + bev_pool_aux,
 *   BF/depth_lss.py:68-112,118-176, and the interval construction of
 *   BF/ops/bev_pool/bev_pool.py:48-54; sync-free: all counts stay on the device)
 *   frustum        f32[D*HW, 3]  pixel-depth grid (depth_lss.py:53-66)
 *   per camera (B*N rows): post_trans f32[3], post_rots_inv f32[9], combine f32[9]
 *                          (= camera2lidar_rots @ intrins_inverse, depth_lss.py:93), c2l_trans f32[3]
 *   per sample (B rows)  : extra_rots f32[9], extra_trans f32[3]   (identity / 0 when absent)
 *   origin_host = bx - dx/2, dx_host, nx_host = (nx[0], nx[1], nx[2])   (depth_lss.py:14-18)
 * geometry is evaluated per point in fp32 with the fixed association ((m0*p0+m1*p1)+m2*p2), no
 * fma; cell = trunc((p - origin)/dx); kept = inside the grid; rank = x*(nx1*nx2*B) + y*(nx2*B)
 * + z*B + b; kept points are STABLY sorted by rank (the reference's argsort is unstable).
 * outputs (N' = B*N*D*HW rows where sized by points; mmax rows where sized by intervals):
 *   sorted_pd        u32[N']  (pixel_index << 8 | depth_bin) of the k-th sorted kept point
 *   starts, lengths  i32[mmax], cell_of_interval i32[mmax] (offset of the cell in out[b][z][x][y])
 *   counts_dev       i32[2] = {n_kept, n_intervals}
 *   interval_order   i32[mmax] (may be NULL): the intervals in camera-major order -- stably sorted by (sample, camera) of
 *                    their first member; bfhip_lift_splat_fwd walks them in this order so that every XCD gathers the feature
 *                    rows of "its" cameras from its own L2 (the cells' sums are unchanged, only their production order)
 *   optional (may be NULL): cell_of_point i32[N'] (out cell of every frustum point or -1; needed by
 *   lift_splat_bwd), geom_sorted i32[N',4] (x,y,z,b), ranks_sorted i64[N'], kept u8[N'],
 *   geom_xyz f32[N',3] (the materialised get_geometry output, for parity tests)
 * --------------------------------------------------------------------------------------- */
size_t bfhip_bev_plan_workspace_bytes(long long nprime, long long ncells_times_b);
int bfhip_bev_plan(const float *frustum, const float *post_trans, const float *post_rots_inv,
                   const float *combine, const float *c2l_trans, const float *extra_rots,
                   const float *extra_trans, int B, int N, int D, int HW,
                   const float *origin_host, const float *dx_host, const int32_t *nx_host,
                   uint32_t *sorted_pd, int32_t *starts, int32_t *lengths,
                   int32_t *cell_of_interval, int32_t *interval_order, int32_t *counts_dev, int32_t *cell_of_point,
                   int32_t *geom_sorted, int64_t *ranks_sorted, uint8_t *kept, float *geom_xyz,
                   int mmax, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * fused lift-splat  (replaces the outer product BF/depth_lss.py:723-725, the two gathers
 *   x[kept][indices] :190-194 and the bev_pool op, without materialising x[N', C])
 *   depth f32[P, depth_pitch] (softmax over D bins, pixel-major), feat f32[P, feat_pitch]
 *   (C channels, pixel-major), P = B*N*HW pixels; plan arrays from bfhip_bev_plan.
 *   out f32[out_cells, C] (out_bf16 = 1: bf16[out_cells, C], the fp32 sums rounded once on store) with
 *   out_cells = B*nx2*nx0*nx1, zero-filled by the call.
 * bwd: d_depth[p,d] = <out_grad[cell(p,d)], feat[p]>, d_feat[p] = sum_d depth[p,d]*out_grad[cell(p,d)]
 * feat_bf16 = 1: feat is bf16[P, feat_pitch] (pitches in ELEMENTS, C % 8 == 0) -- the depthnet's output as the bf16
 *   convolution left it (the reference widens it with x.float(), BF/depth_lss.py:467-468: same values); the gathered rows are
 *   half as long, the arithmetic is unchanged (fp32 products and sums in the same order), and the backward writes d_feat as
 *   bf16[P, d_feat_pitch] (the fp32 sums rounded once, what the backward of that x.float() does).
 * --------------------------------------------------------------------------------------- */
int bfhip_lift_splat_fwd(const float *depth, int depth_pitch, const void *feat, int feat_bf16, int feat_pitch,
                         const uint32_t *sorted_pd, const int32_t *starts, const int32_t *lengths,
                         const int32_t *cell_of_interval, const int32_t *interval_order /* may be NULL: rank order */,
                         const int32_t *counts_dev, int mmax, int C, long long out_cells, void *out, int out_bf16,
                         void *stream);
int bfhip_lift_splat_bwd(const void *out_grad, int grad_bf16 /* out_grad is bf16[out_cells, C] */, const float *depth,
                         int depth_pitch,
                         const void *feat, int feat_bf16, int feat_pitch, const int32_t *cell_of_point,
                         int num_cams, int D, int HW, int C, float *d_depth, int d_depth_pitch,
                         void *d_feat, int d_feat_pitch, void *stream);

/* ---------------------------------------------------------------------------------------
 * sparse 3-D convolution  (replaces what the reference delegates to spconv 2.x:
 *   SpconvOps.get_indice_pairs_implicit_gemm, projects/SparseConvolution/sparse_functional.py:118-137;
 *   ConvGemmOps.implicit_gemm :287-314; SparseConvTensor.dense(), BF/sparse_encoder.py:147)
 *   indices i32[N,4] = (b, x, y, z), 16-byte aligned; shapes/ksize/stride/padding/dilation are host int[3]
 *   pair table i32[KV, ld]: pair[k*ld + out_row] = input row or -1; offset k = (i*k1 + j)*k2 + l
 *   weights f32 (Cout, k0, k1, k2, Cin) (mmdet3d/models/layers/spconv/overwrite_spconv/write_spconv2.py:50-51)
 * SubM    : out rows = in rows; pad = dil*(k//2).
 * strided : out shape (in + 2p - d(k-1) - 1)//s + 1 (projects/SparseConvolution/sparse_conv.py:88-90);
 *           output rows in ASCENDING LINEAR ORDER ((b*X+x)*Y+y)*Z+z (canonical; spconv's is hash order).
 *           Two phases because N_out must reach the host: _count writes counts_dev[0] = N_out;
 *           _fill (same workspace, untouched in between) writes out_indices i32[n_out,4],
 *           pair_fwd i32[KV,n_out], pair_bwd i32[KV,N]; the number of pairs is sum(counts_dev[1..64])
 *           (counts_dev is i32[65]; rulebook_subm's n_pairs_dev is i32[64], same convention: 64 spread
 *           counters, because one hot word serialises the atomics).
 * duplicate input coordinates (never produced by the voxelizers; the reference's own encoder test feeds them,
 *           tests/test_models/test_middle_encoders/test_sparse_encoders.py:22-25, where spconv's result is whichever
 *           row its hash insert kept): every duplicate stays a row; a neighbour lookup resolves a coordinate to its LOWEST
 *           row (SubM table) / a strided output takes the HIGHEST row per (offset, output) slot -- deterministic both.
 * gemm    : out[n_rows, Ndim] = sum_k M_k . in[pairs[k][row]];  transpose=0 forward (M_k = W[:,k,:]^T),
 *           transpose=1 dgrad (M_k = W[:,k',:], k' = KV-1-k when flip else k; flip=1 lets a SubM layer
 *           reuse pair_fwd as its backward table).  Exact-fp32 MFMA, deterministic, no atomics.
 * wgrad   : dW (Cout,KV,Cin) = sum_n dout[n] (x) in[pairs[k][n]], fixed-order reduction.
 * sparse_to_bev: out f32[B, C*Z, X, Y] (zero-filled here) <- feats[n][c] at (b, c*Z+z, x, y);
 * bev_to_sparse: its gather (backward).
 * --------------------------------------------------------------------------------------- */
int bfhip_conv_out_shape(const int *in_shape, const int *ksize, const int *stride,
                         const int *padding, const int *dilation, int *out_shape);
size_t bfhip_rulebook_subm_workspace_bytes(int N);
int bfhip_rulebook_subm(const int32_t *indices, int N, int B, const int *in_shape, const int *ksize,
                        const int *dilation, int32_t *pair_fwd, int32_t *n_pairs_dev, uint32_t *row_mask,
                        int32_t *perm, void *workspace, size_t workspace_bytes, void *stream);
/* row_mask / perm (optional, kernel volume <= 32): the table's row masks and sorted row order (see
 * bfhip_rulebook_sort_rows below), produced by the launch that fills the table instead of a second pass over it.
 * n_pairs_dev is optional (NULL: no pair statistics). */
size_t bfhip_rulebook_sparse_workspace_bytes(int B, const int *in_shape, const int *ksize,
                                             const int *stride, const int *padding,
                                             const int *dilation);
/* n_in_dev (optional): the true number of input rows on the device; N is then only the launch bound.  With
 * bfhip_rulebook_sparse_out_indices (output coordinates into a buffer of `cap` rows, no host-side N_out) a chain of strided
 * layers is counted back to back and all N_out values are read in ONE host read. */
int bfhip_rulebook_sparse_count(const int32_t *indices, int N, const int32_t *n_in_dev, int B, const int *in_shape,
                                const int *ksize, const int *stride, const int *padding, const int *dilation,
                                int32_t *counts_dev, void *workspace, size_t workspace_bytes, void *stream);
int bfhip_rulebook_sparse_out_indices(int B, const int *in_shape, const int *ksize, const int *stride,
                                      const int *padding, const int *dilation, int cap, int32_t *out_indices,
                                      void *workspace, size_t workspace_bytes, void *stream);
int bfhip_rulebook_sparse_fill(const int32_t *indices, int N, int B, const int *in_shape,
                               const int *ksize, const int *stride, const int *padding,
                               const int *dilation, int n_out, int32_t *out_indices,
                               int32_t *pair_fwd, int32_t *pair_bwd, int32_t *counts_dev,
                               uint32_t *mask_fwd, int32_t *perm_fwd, uint32_t *mask_bwd, int32_t *perm_bwd,
                               void *sort_workspace, size_t sort_workspace_bytes,
                               void *workspace, size_t workspace_bytes, void *stream);
/* mask_fwd / perm_fwd (over the output rows, from pair_fwd) and mask_bwd / perm_bwd (over the input rows, from pair_bwd):
 * optional, kernel volume <= 32; sort_workspace = bfhip_rulebook_sort_rows_workspace_bytes(max(N, n_out), KV) bytes. */
/* row_mask[n] bit k = (pairs[k][n] >= 0); perm = rows stably sorted by mask inside consecutive chunks of 4096 rows
 * (key = (n / 4096, mask); one LDS sort per chunk, one launch), so that the 16 rows of an MFMA tile share their kernel
 * offsets and whole offsets are skipped per tile (cf. spconv's mask_argsort,
 * projects/SparseConvolution/sparse_functional.py:139-162) while consecutive tiles stay in one slab of space (the
 * gather-GEMM deals contiguous eighths of the tiles to the 8 XCDs).  BFHIP_SPCONV_CHUNK_SORT=0: the round-2 order
 * (eighth of the row range, mask) from a device-wide sort.  perm/row_mask are optional
 * (NULL) inputs of gemm / wgrad; results do not depend on them (only the fp32 summation order of wgrad). */
size_t bfhip_rulebook_sort_rows_workspace_bytes(int n_rows, int KV);
int bfhip_rulebook_sort_rows(const int32_t *pairs, int ld, int KV, int n_rows, uint32_t *row_mask,
                             int32_t *perm, void *workspace, size_t workspace_bytes, void *stream);
/* Debug guard: the gather kernels below dereference pairs[k*ld + perm[i]] and in + pairs[..]*K unchecked (an index that is
 * out of range is a memory-aperture fault).  Counts into status_dev i32[4]: [0] pair entries outside
 * [-1, n_src), [1] perm entries outside [0, n_rows), [2] rows not occurring exactly once in perm, [3] rows whose row_mask
 * disagrees with the table.  perm / row_mask optional.  The Python host runs it before every gather launch under
 * BFHIP_SPCONV_VALIDATE=1 and in the parity tests; it is not part of the timed path. */
size_t bfhip_rulebook_validate_workspace_bytes(int n_rows);
int bfhip_rulebook_validate(const int32_t *pairs, int ld, int KV, int n_rows, int n_src, const int32_t *perm,
                            const uint32_t *row_mask, int32_t *status_dev, void *workspace, size_t workspace_bytes,
                            void *stream);
size_t bfhip_spconv_workspace_bytes(int KV, int Cin, int Cout);
int bfhip_spconv_gemm(const float *in, const float *W, const int32_t *pairs, int ld, int KV,
                      int n_rows, int Cin, int Cout, int transpose, int flip, const int32_t *perm,
                      const uint32_t *row_mask, float *out, void *workspace, size_t workspace_bytes,
                      void *stream);
/* bf16-MFMA variant of bfhip_spconv_gemm (same workspace size): features and weights enter the MFMA as bf16, products
 * accumulate in fp32.  io_bf16 = 0: features f32 (rounded on load), output f32.  io_bf16 = 1: features STORED in bf16
 * (the gathered 16-byte row segments are the MFMA operand as they are: half the gather traffic) and the output rounded
 * to bf16 once -- the reference runs spconv in half precision under AMP.  Requires K % 8 == 0. */
int bfhip_spconv_gemm_bf16(const void *in, const float *W, const int32_t *pairs, int ld, int KV,
                           int n_rows, int Cin, int Cout, int transpose, int flip, const int32_t *perm,
                           const uint32_t *row_mask, void *out, int io_bf16, void *workspace, size_t workspace_bytes,
                           void *stream);
size_t bfhip_spconv_wgrad_workspace_bytes(int KV, int Cin, int Cout, int n_rows);
/* io_bf16 = 1: `in` and `dout` are bf16 feature matrices (widened on load; Cin, Cout multiples of 4); dW is always f32 */
int bfhip_spconv_wgrad(const void *in, const void *dout, const int32_t *pairs, int ld, int KV,
                       int n_rows, int Cin, int Cout, const int32_t *perm, float *dW, int io_bf16, void *workspace,
                       size_t workspace_bytes, void *stream);
int bfhip_sparse_to_bev(const float *feats, const int32_t *indices, int N, int C, int B, int X,
                        int Y, int Z, float *out, void *stream);
int bfhip_bev_to_sparse(const float *grad_out, const int32_t *indices, int N, int C, int B, int X,
                        int Y, int Z, float *grad_feats, void *stream);
/* channels-last variants: out (f32 | bf16, dtype 0 | 1) is the NHWC memory of the [B, C*Z, X, Y] map, out[b][x][y][c*Z+z];
 * the backward reads element (b, ch, x, y) at grad_out[b*stride_b + x*stride_x + y*stride_y + ch] (strides in elements,
 * channel stride 1), so a channel slice of a wider channels-last gradient is consumed in place. */
int bfhip_sparse_to_bev_nhwc(const float *feats, const int32_t *indices, int N, int C, int B, int X, int Y, int Z,
                             int dtype, void *out, void *stream);
int bfhip_bev_nhwc_to_sparse(const void *grad_out, long long stride_b, long long stride_x, long long stride_y,
                             int dtype, const int32_t *indices, int N, int C, int Z, float *grad_feats, void *stream);

/* ---------------------------------------------------------------------------------------
 * sparse LiDAR depth images + GT depth histogram  (replaces the per-sample torch loop of
 *   BaseDepthTransform.forward, BF/depth_lss.py:372-449, and the scatter_add_ histogram of
 *   DepthLSSTransform.get_cam_feats, :636-686)
 *   points f32[n,f]; inv_rot f32[9] = lidar_aug_matrix_inverse[:3,:3]; aug_trans f32[3] = lidar_aug_matrix[:3,3];
 *   lidar2image, img_aug f32[ncam,16] (row-major 4x4).  depth f32[ncam,iH,iW] is fully written.
 *   A pixel hit by several points keeps the LAST point (torch's scatter_ leaves it unspecified, :410-417).
 *   counts (optional, f32[ncam,fH,fW,D], cleared by the caller) receives the depth-bin histogram of the hit
 *   pixels; bfhip_depth_histogram normalises it (bin 0 excluded, as :670-674) or rebuilds it from a depth image.
 * --------------------------------------------------------------------------------------- */
/* Gradient of the first dtransform layer, Conv2d(1, 8, 1) on the one-channel depth image (BF/depth_lss.py:592-594; its
 * autograd backward in the reference): y[m][c] = b[c] + d[m] * w[c] over the M = BN * iH * iW pixels.  dy bf16 [M][8] dense,
 * d bf16 [M] -> out f32[16] = {db[0..8), dw[0..8)}; fp32 accumulation, fixed-order sums (deterministic). */
size_t bfhip_depth_lift_bwd_workspace_bytes(void);
int bfhip_depth_lift_bwd(const void *dy, const void *d, long long M, float *out, void *workspace, size_t workspace_bytes, void *stream);
size_t bfhip_rasterise_depth_workspace_bytes(int ncam, int iH, int iW);
int bfhip_rasterise_depth(const float *points, int n, int f, const float *inv_rot, const float *aug_trans,
                          const float *lidar2image, const float *img_aug, int ncam, int iH, int iW,
                          float *depth, float *counts, int fH, int fW, int D, const float *dbound_host,
                          void *workspace, size_t workspace_bytes, void *stream);
int bfhip_depth_histogram(const float *depth, int BN, int iH, int iW, int fH, int fW, int D,
                          const float *dbound_host, float *counts, float *distr, void *stream);

/* ---------------------------------------------------------------------------------------
 * BatchNorm1d (+ residual) (+ ReLU) on sparse feature matrices f32[N, C], training mode  (SURVEY 8 f-4;
 *   replaces the BN1d / add / ReLU torch kernels after every sparse conv,
 *   mmdet3d/models/layers/sparse_block.py:135-154,157-224; norm_cfg BN1d eps 1e-3 momentum 0.01)
 *   fwd: stats f32[2C] <- (batch mean, 1/sqrt(biased var + eps)); running stats updated like torch
 *        (running_var with the unbiased variance); y = act(gamma * (x - mean) * invstd + beta [+ residual])
 *   bwd: dgb f32[2C] <- (dgamma, dbeta); dx; dres (optional) = gradient of the residual input
 *   C must divide 256 and be a multiple of 4; tensors 16-byte aligned.
 * --------------------------------------------------------------------------------------- */
size_t bfhip_bn1d_workspace_bytes(int N, int C);
/* n_rows_dev / m_dev (optional, both BatchNorm families): the number of ACTIVE rows when N / M is only a capacity (feature
 * matrices of the sparse encoder sized by bounds, true counts on the device: no host read); the rows beyond it must be zero. */
int bfhip_bn1d_fwd(const float *x, const float *residual, const float *gamma, const float *beta, int N, int C,
                   float eps, float momentum, int relu, float *running_mean, float *running_var, float *stats,
                   float *y, const int32_t *n_rows_dev, void *workspace, size_t workspace_bytes, void *stream);
int bfhip_bn1d_bwd(const float *dy, const float *y, const float *x, const float *stats, const float *gamma, int N,
                   int C, int relu, float *dx, float *dres, float *dgb, const int32_t *n_rows_dev, void *workspace,
                   size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * BatchNorm2d (+ residual) (+ ReLU), training mode, on channels-last activations viewed as [M = N*H*W, C]
 *   (the BN / add / ReLU after every dense conv: ResNet bottlenecks, BF/depth_lss.py:581-620,
 *    BF/bevfusion_head.py:25-38,104-126, mmdet3d/models/backbones/second.py:70-95, necks/second_fpn.py:60-84)
 *   dtype: 0 = f32, 1 = bf16 (x, residual, y, dy, dx, dres share it); gamma/beta/stats/running stats are f32.
 *   C must be a multiple of the 16-byte vector (4 f32 / 8 bf16) with at most 256 vectors per row:
 *   bfhip_bn2d_supported() tells.  stats f32[4C] <- (mean, invstd, a = gamma*invstd, b = beta - mean*a).
 *   bwd: pass y only for layers that added a residual before the ReLU (otherwise the ReLU mask is recomputed
 *   from x and y may be NULL); dgb f32[2C] <- (dgamma, dbeta); dres optional.
 * --------------------------------------------------------------------------------------- */
int bfhip_bn2d_supported(long long M, int C, int dtype);
/* out f32[C] = column sums of x [M][C] (dtype 0 f32 | 1 bf16, dense; shapes as bfhip_bn2d_supported, workspace as
 * bfhip_bn2d_workspace_bytes): the bias gradient of a convolution / linear layer (sum of dy over pixels / rows), fixed order. */
int bfhip_colsum(const void *x, long long M, int C, int dtype, float *out, void *workspace, size_t workspace_bytes, void *stream);
size_t bfhip_bn2d_workspace_bytes(long long M, int C, int dtype);
int bfhip_bn2d_fwd(const void *x, const void *residual, const float *gamma, const float *beta, long long M, int C,
                   int dtype, float eps, float momentum, int relu, float *running_mean, float *running_var,
                   float *stats, void *y, const int32_t *m_dev, void *workspace, size_t workspace_bytes, void *stream);
int bfhip_bn2d_bwd(const void *dy, const void *x, const void *y, const float *stats, const float *gamma, long long M,
                   int C, int dtype, int relu, void *dx, void *dres, float *dgb, const int32_t *m_dev, void *workspace,
                   size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * out f32[M, N] = X^T Y for tall-skinny row-major X [K, M], Y [K, N] (f32 | bf16, dtype 0 | 1), K >> M, N: the weight
 *   gradient of the linear layers that act on every BEV cell (cross-attention K / V projections and the position
 *   embedding MLP of the TransFusion decoder layer, BF/transformer.py:10-23,60-105: dW = dY^T X with K = B*180*180).
 *   K is split over the chip, products and sums in fp32, fixed-order combine (deterministic).
 * --------------------------------------------------------------------------------------- */
size_t bfhip_xty_workspace_bytes(long long K, int M, int N);
int bfhip_xty(const void *X, const void *Y, long long K, int M, int N, int dtype, float *out, void *workspace,
              size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Cross attention of few queries over very many keys (the TransFusion decoder layer: 200 queries x 32 400 BEV cells,
 *   8 heads of 16 channels, dropout on the attention weights; BF/transformer.py:60-105, mmcv MultiheadAttention ->
 *   torch scaled_dot_product_attention).  Q [B, Lq, H*16], K / V [B, Lk, H*16], O, dO, dQ, dK, dV alike: bf16, row-major;
 *   head h = channels 16h..16h+15; Lq <= bfhip_attn_max_queries() = 512 (host-only; up to 256 queries one workgroup per
 *   key chunk keeps them all, above that the forward adds a query-block grid axis and the backward walks 32 query tiles per
 *   key tile: dK / dV are still final per key, no extra workspace).  lse f32[B*H, Lq] (log-sum-exp of the scaled scores) links fwd and bwd.
 *   The key axis is split over the chip; combines run in a fixed order (bit-reproducible).  dropout_p in [0, 1): keep
 *   mask = counter hash of (seed, b, h, query, key), regenerated in the backward; bfhip_attn_dropout_mask writes it
 *   out (u8[B*H, Lq, Lk]) for tests.  The hashed element index is 32-bit: with dropout_p > 0 all three refuse
 *   B*H*Lq*Lk > 2^32 (BFHIP_E_INVALID, before any launch).  The workspace is shared by fwd and bwd.
 * --------------------------------------------------------------------------------------- */
int bfhip_attn_max_queries(void);
size_t bfhip_attn_workspace_bytes(int B, int H, int Lq, int Lk);
int bfhip_attn_fwd(const void *Q, const void *K, const void *V, int B, int H, int Lq, int Lk, float scale,
                   float dropout_p, unsigned long long seed, const unsigned long long *seed_dev, void *O, float *lse,
                   void *workspace, size_t workspace_bytes, void *stream);
int bfhip_attn_bwd(const void *Q, const void *K, const void *V, const void *O, const void *dO, const float *lse, int B,
                   int H, int Lq, int Lk, float scale, float dropout_p, unsigned long long seed,
                   const unsigned long long *seed_dev, void *dQ, void *dK, void *dV, void *workspace, size_t workspace_bytes,
                   void *stream);
/* seed_dev (optional, all three): device u64 call counter mixed into the seed (a replayed hipGraph repeats its host arguments) */
int bfhip_attn_dropout_mask(int B, int H, int Lq, int Lk, float dropout_p, unsigned long long seed,
                            const unsigned long long *seed_dev, unsigned char *mask, void *stream);

/* ---------------------------------------------------------------------------------------
 * Bilinear 2x upsampling of channels-last maps [B, H, W, C] -> [B, 2H, 2W, C] (f32 | bf16), torch's align_corners=False
 *   index rule; the LSS-FPN's top-down path (BF/bevfusion_necks.py:76-88).  dir 0 = forward; dir 1 = backward as a gather
 *   (src = grad of the output, dst = grad of the input): no atomics, deterministic.  C % (4 | 8) == 0.
 * --------------------------------------------------------------------------------------- */
int bfhip_upsample2x_nhwc(const void *src, void *dst, int B, int H, int W, int C, int dtype, int dir, void *stream);

/* ---------------------------------------------------------------------------------------
 * 3x3 stride-2 pad-1 max pooling of a channels-last bf16 map [N, H, W, C] -> [N, OH, OW, C], OH = (H - 1) / 2 + 1 (the ResNet-50
 *   stem's nn.MaxPool2d(3, 2, 1); img_backbone = mmdet.ResNet, an external dependency of the reference).  Forward stores the
 *   winning tap (0..8, torch's scan order and tie / NaN rule) of every element in `tap` (u8, same shape as y); backward is a
 *   gather over the <= 2 x 2 windows of each input pixel: no atomics, no zero-fill, deterministic.  C % 8 == 0.
 * --------------------------------------------------------------------------------------- */
int bfhip_maxpool3x3s2_fwd(const void *x, int N, int H, int W, int C, void *y, unsigned char *tap, void *stream);
int bfhip_maxpool3x3s2_bwd(const void *dy, const unsigned char *tap, int N, int H, int W, int C, void *dx, void *stream);

/* ---------------------------------------------------------------------------------------
 * TransFusion head: box decoding, target assignment and losses on the device  (SURVEY 8 f-3).
 *   Replaces TransFusionBBoxCoder.decode/encode (BF/utils.py:33-96), HungarianAssigner3D.assign with its three costs
 *   and the `.cpu()` + scipy.optimize.linear_sum_assignment round trip (BF/utils.py:128-151,241-284; IoU as
 *   mmdet3d/structures/bbox_3d/base_box3d.py:529-590), the target scatter and the box-by-box heat-map drawing of
 *   BEVFusionHead.get_targets_single (BF/bevfusion_head.py:514-674, mmdet3d/models/utils/gaussian.py:9-92) and the
 *   three loss terms of loss_by_feat (:696-796: mmdet GaussianFocalLoss / FocalLoss / L1Loss).
 *   Head outputs keep the reference layout [B, channels, ld] (ld = proposals of all decoder layers concatenated);
 *   one call handles the P proposals starting at p_off.  Ground truth is padded to G boxes per sample:
 *   gt_boxes f32[B,G,Wg] = (x, y, z_bottom, dx, dy, dz, yaw[, vx, vy]), gt_labels i32[B,G], n_gt i32[B].
 *
 *   decode_boxes   cfg_host = {out_size_factor, voxel_x, voxel_y, pc_x0, pc_y0}; vel may be NULL (-> 7 columns);
 *                  boxes f32[B,P,7|9] bottom-centre
 *   assign_cost    cfg_host = {cls_weight, alpha, gamma, eps, reg_weight, iou_weight, pc_x0, pc_y0, pc_x1, pc_y1};
 *                  cost, iou f32[B,P,G] (columns >= n_gt[b] are written as 0 and never read)
 *   hungarian      minimum-cost assignment per sample, fp64, max(P, G) <= 1024.  assigned i32[B,P]: 0 = background,
 *                  g + 1 = matched (AssignResult.gt_inds); status i32[B]: 0 ok, 1 = non-finite costs (all background)
 *   assign_targets cfg_host = {pc_x0, pc_y0, (float)(out_size_factor*voxel_x), (float)(out_size_factor*voxel_y),
 *                  pos_weight}; labels i32[B,P] (num_classes = background), label_weights f32[B,P],
 *                  bbox_targets / bbox_weights f32[B,P,code_size], ious f32[B,P] (clamped matched IoU)
 *   draw_heatmap   cfg_host = {pc_x0, pc_y0, voxel_x, voxel_y, out_size_factor}; heatmap f32[B,num_classes,H,W] is
 *                  cleared and drawn; box (x, y) lands at [cls][x cell][y cell] (the `center_int[[1, 0]]` fix, :662)
 *   gaussian_focal_loss  loss_sum_npos f32[2] <- (sum of element losses on clip_sigmoid(logits), count of target == 1);
 *                  grad f32[n] <- d element loss / d logit (unscaled)
 *   query_losses   loss_sums f32[2] <- (weighted focal sum over [B,P,C], weighted L1 sum over [B,P,K]); grad_cls /
 *                  grad_box in the layout of the inputs (entries outside [p_off, p_off+P) untouched)
 *   predict_compact  the filter of TransFusionBBoxCoder.decode (BF/utils.py:100-124) with the counts left on the device:
 *                  boxes f32[B,P,W] (W = 7 | 9, decoded), scores f32[B,P], labels i64[B,P] (what max(1) returns), P <= 4096;
 *                  range_host = post_center_range {x0, y0, z0, x1, y1, z1}.  A row is kept iff lo <= centre <= hi on all three
 *                  axes and, when use_threshold != 0, score > threshold; NaN fails every comparison.  Kept rows go, in
 *                  ascending proposal order, to out_boxes f32[B,P,W], out_scores f32[B,P], out_labels i32[B,P]; rows >=
 *                  counts[b] are zeros with label -1; counts i32[B].  One launch, one workgroup per sample, no atomics, no
 *                  host read.  The outputs must not alias the inputs.
 * --------------------------------------------------------------------------------------- */
int bfhip_decode_boxes(const float *center, const float *height, const float *dim, const float *rot,
                       const float *vel, int B, int P, int ld, int p_off, const float *cfg_host, float *boxes,
                       void *stream);
int bfhip_predict_compact(const float *boxes, const float *scores, const long long *labels, int B, int P, int W,
                          const float *range_host, int use_threshold, float threshold, float *out_boxes, float *out_scores,
                          int32_t *out_labels, int32_t *counts, void *stream);
int bfhip_assign_cost(const float *boxes, int W, const float *cls_logits, int C, int ld, int p_off,
                      const float *gt_boxes, int Wg, const int32_t *gt_labels, const int32_t *n_gt, int B, int P,
                      int G, const float *cfg_host, float *cost, float *iou, void *stream);
int bfhip_hungarian(const float *cost, const int32_t *n_gt, int B, int P, int G, int32_t *assigned,
                    int32_t *status, void *stream);
int bfhip_assign_targets(const int32_t *assigned, const float *iou, const float *gt_boxes, int Wg,
                         const int32_t *gt_labels, int B, int P, int G, int num_classes, int code_size,
                         const float *cfg_host, int32_t *labels, float *label_weights, float *bbox_targets,
                         float *bbox_weights, float *ious, void *stream);
int bfhip_draw_heatmap(const float *gt_boxes, int Wg, const int32_t *gt_labels, const int32_t *n_gt, int B, int G,
                       int num_classes, int H, int W, const float *cfg_host, double gaussian_overlap,
                       int min_radius, float *heatmap, void *stream);
size_t bfhip_gaussian_focal_loss_workspace_bytes(long long n);
int bfhip_gaussian_focal_loss(const float *logits, const float *target, long long n, float clip_eps,
                              float *loss_sum_npos, float *grad, void *workspace, size_t workspace_bytes,
                              void *stream);
/* circle NMS (mmdet3d/models/layers/box3d_nms.py:186-228, called from BEVFusionHead.predict_by_feat :399-413 on the CPU):
 * dets f32[n,3] = (x, y, score); keep i32[min(n, post_max_size)] receives the kept indices, highest score first;
 * n_keep i32[1].  n <= 4096. */
int bfhip_circle_nms(const float *dets, int n, float thresh, int post_max_size, int32_t *keep, int32_t *n_keep,
                     void *stream);
/* rotate NMS: nms_bev (mmdet3d/models/layers/box3d_nms.py:234-275) -> mmcv.ops.nms_rotated, called from
 * BEVFusionHead.predict_by_feat :414-423 when test_cfg.nms_type is neither None nor 'circle'.
 * boxes f32[n,5] = (x, y, w, h, angle), scores f32[n]; the min(n, pre_max_size) highest-scoring boxes take part, box j is
 * dropped when an earlier kept box overlaps it with IoU > thresh; keep i32[min(n, pre_max_size, post_max_size)] receives
 * the kept indices (into boxes), highest score first; n_keep i32[1].  Equal scores: lower index first.
 * n <= 16384, min(n, pre_max_size) <= 4096. */
size_t bfhip_rotate_nms_workspace_bytes(int n, int pre_max_size);
int bfhip_rotate_nms(const float *boxes, const float *scores, int n, float thresh, int pre_max_size, int post_max_size,
                     int32_t *keep, int32_t *n_keep, void *workspace, size_t workspace_bytes, void *stream);
int bfhip_query_losses(const float *cls_logits, const int32_t *labels, const float *label_weights,
                       const float *box_pred, const float *bbox_targets, const float *bbox_weights,
                       const float *code_weights, int B, int C, int P, int K, int ld, int p_off, float gamma,
                       float alpha, float *grad_cls, float *grad_box, float *loss_sums, void *stream);

/* BEVFusion.voxelize (projects/BEVFusion/bevfusion/bevfusion.py:227-255: per-sample voxelize, F.pad batch id, cat, mean) for B
 * samples without the per-sample host reads: voxels f32[B][max_voxels][P][F], coors i32[B][max_voxels][3], num_points
 * i32[B][max_voxels], counts_dev i32[B] (what bfhip_hard_voxelize left on the device) -> feats f32[cap][F] (per-voxel means),
 * out_coords i32[cap][4] = (b, x, y, z); active rows are the prefix, the rest are zeros with b = -1 (inactive rows: every
 * index-driven kernel of this library skips them); n_total_dev i32[2] = (active rows, sum of counts). */
int bfhip_voxel_compact_mean(const float *voxels, const int32_t *coors, const int32_t *num_points, const int32_t *counts_dev,
                             int B, int max_voxels, int P, int F, int cap, float *feats, int32_t *out_coords,
                             int32_t *n_total_dev, void *stream);

/* ---- dense 2-D convolution, channels-last bf16, implicit GEMM on the matrix cores (csrc/conv2d.hip).
 * Replaces the cuDNN convolutions behind torch.nn.Conv2d of ConvFuser (projects/BEVFusion/bevfusion/bevfusion_head.py:26-38),
 * SECOND / SECONDFPN (mmdet3d/models/backbones/second.py:27-95, necks/second_fpn.py:30-94), shared_conv (:95-102),
 * depthnet / downsample (projects/BEVFusion/bevfusion/depth_lss.py:592-620) and GeneralizedLSSFPN
 * (projects/BEVFusion/bevfusion/bevfusion_necks.py:50-72).  x bf16 [N,H,W,Cin] with pixel pitch ldx, w bf16
 * [Cout][KH][KW][Cin] (the memory of a channels-last Conv2d weight), y bf16|f32 [N,OH,OW,Cout] with pixel pitch ldy; Cin, Cout
 * multiples of 8.  stat_partial (optional) f32[bfhip_conv2d_stat_rows()][2][Cout]: per-row-block column sums and sums of
 * squares of the fp32 accumulators (without bias) = the `partial` input of bfhip_bn2d_fwd_partials. */
int bfhip_conv2d_supported(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil);
int bfhip_conv2d_stat_rows(int N, int OH, int OW);
int bfhip_conv2d_fwd(const void *x, int ldx, const void *w, const float *bias, void *y, int ldy, int N, int H, int W, int Cin,
                     int Cout, int KH, int KW, int stride, int pad, int dil, int out_f32, float *stat_partial, void *stream);
size_t bfhip_conv2d_dgrad_workspace_bytes(int Cin, int Cout, int KH, int KW);
int bfhip_conv2d_dgrad(const void *dy, int ldg, const void *w, void *dx, int ldx, int N, int H, int W, int Cin, int Cout,
                       int KH, int KW, int stride, int pad, int dil, int out_f32, void *workspace, size_t workspace_bytes,
                       void *stream);
/* The data gradient with the weight already transposed (wt bf16 [Cin][KH][KW][Cout], read-only), and the transposition of a
 * whole table of weights in one launch -- a training step refreshes all layers' copies once, after the optimizer, instead of
 * paying a transpose launch inside every bfhip_conv2d_dgrad.  segs_dev: nseg device records of bfhip_conv2d_wt_segment_bytes()
 * bytes each {u64 src ([Cout][taps][Cin], bf16 or f32), u64 dst, i32 Cout, i32 taps, i32 Cin, i32 src_f32, i64 first_block};
 * a segment owns ceil(Cin/32) * ceil(Cout/32) * taps blocks, first_block ascending from 0, total_blocks = their sum. */
int bfhip_conv2d_dgrad_wt(const void *dy, int ldg, const void *wt, const void *addend, int addend_stride, void *dx, int ldx, int N,
                          int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil, int out_f32, void *stream);
/* addend (optional, bf16, dense with pixel pitch Cin): dx = data gradient + addend in the kernel's epilogue (the second gradient path
 * of a residual connection).  addend_stride 1: [N,H,W,Cin]; 2: [N,ceil(H/2),ceil(W/2),Cin], the gradient of a stride-2 1x1 shortcut
 * over the same tensor -- it reaches the pixels with even h and w only.  Accepted only when bfhip_conv2d_dgrad_fuses_addend() says
 * so (1x1, stride 1, no padding, bf16 output) */
int bfhip_conv2d_dgrad_fuses_addend(int KH, int KW, int stride, int pad, int out_f32);
int bfhip_conv2d_wt_segment_bytes(void);
int bfhip_conv2d_weight_transpose_batched(const void *segs_dev, int nseg, long long total_blocks, void *stream);
/* fp32 operand -> bf16 pair hi = bf16(v), lo = bf16(v - hi) (v = hi + lo to 2^-16 relative), in the layouts of the three-product
 * fp32 convolution (a*b ~ a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on the bf16 matrix cores, fp32 accumulation): src f32 [P][C] dense ->
 * chan (optional) bf16 [P][3C] and batch (optional) bf16 [3][P][C]; bit k of order_* set = block k holds lo.  C % 8 == 0. */
int bfhip_split_bf16x3(const float *src, long long P, int C, void *chan, int order_chan, void *batch, int order_batch, void *stream);
/* Host-only queries of the launch decision (no launch, no device needed; the same functions, knobs and CU count as the launch
 * path).  launch_choice: dir 0 = bfhip_conv2d_fwd, 1 = bfhip_conv2d_dgrad(_wt); out_host[8] = {pointwise kernel (0 | 1), tile shape
 * (0 = 128x64, 1 = 128x128, 2 = 256x256; pointwise: the tile width), LDS stages, gather mode (0 forward, 1 transposed, 2 parity
 * classes), tile rows, tile columns, row tiles, column tiles}.  wgrad_choice: out_host[4] = {tile shape (0 = 128x128, 1 = 128 co x
 * 256 k, 2 = 256 co x 128 k), tiles along Cout, tiles along K, pixel-range splits}. */
int bfhip_conv2d_launch_choice(int dir, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil,
                               int out_f32, int32_t *out_host);
int bfhip_conv2d_wgrad_choice(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil,
                              int32_t *out_host);
size_t bfhip_conv2d_wgrad_workspace_bytes(int N, int OH, int OW, int Cin, int Cout, int KH, int KW);
int bfhip_conv2d_wgrad(const void *x, int ldx, const void *dy, int ldg, void *dw, int N, int H, int W, int Cin, int Cout,
                       int KH, int KW, int stride, int pad, int dil, int dw_bf16, void *workspace, size_t workspace_bytes,
                       void *stream);
/* Grouped weight gradients: dW of MANY layers in one launch per tile shape plus one slab-sum launch.  dW of a layer is a leaf of
 * the backward graph (torch/nn/modules/conv.py's weight gradient, reached through BF/bevfusion.py:143-171 and every ConvModule of
 * the dense path), so a caller may collect (x, dy, dW) during the backward and launch the group at its end: every workgroup then
 * runs ~target_steps 64-pixel steps of its layer instead of the 6-9 a one-residency-round launch of a small layer leaves it,
 * and the fp32 split slabs shrink with the split count.  Same kernels, same fixed-order slab sum as bfhip_conv2d_wgrad; only the
 * number of splits (= the fp32 summation order) differs.
 *   bfhip_wgrad_layer                    one record per layer, host memory, filled by the caller
 *   bfhip_conv2d_wgrad_groupable()       1 if the layer's geometry can join a group (else: bfhip_conv2d_wgrad)
 *   bfhip_conv2d_wgrad_group_table_bytes size of the table image for n layers
 *   bfhip_conv2d_wgrad_group_plan()      host only: plans splits / XCD chunks, writes the table image into table_host (host memory,
 *                                        e.g. pinned) and the slab workspace size into *slab_bytes; target_steps <= 0: default 96
 *   bfhip_conv2d_wgrad_group_launch()    table_dev = device copy of the image (copied by the caller, stream-ordered before this
 *                                        call); slab: 256-byte aligned device workspace of >= *slab_bytes */
typedef struct bfhip_wgrad_layer {
  const void *x, *dy; /* bf16 [N,H,W,ldx] and bf16 [N,OH,OW,ldg], 16-byte aligned */
  void *dw;           /* [Cout][KH][KW][Cin], fp32 or bf16 (dw_bf16) */
  int32_t ldx, ldg, N, H, W, Cin, Cout, KH, KW, stride, pad, dil, dw_bf16, reserved;
} bfhip_wgrad_layer;
size_t bfhip_conv2d_wgrad_group_table_bytes(int n_layers);
int bfhip_conv2d_wgrad_groupable(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil);
int bfhip_conv2d_wgrad_group_plan(const void *layers, int n_layers, int target_steps, void *table_host, size_t table_bytes,
                                  size_t *slab_bytes);
int bfhip_conv2d_wgrad_group_launch(const void *table_host, const void *table_dev, void *slab, size_t slab_bytes, void *stream);
/* BatchNorm2d forward whose statistics pass already happened in the producing convolution's epilogue: `partial`
 * f32[nblk][2][C] (column sums, sums of squares per row block).  Otherwise as bfhip_bn2d_fwd. */
int bfhip_bn2d_fwd_partials(const void *x, const void *residual, const float *gamma, const float *beta, long long M, int C,
                            int dtype, float eps, float momentum, int relu, float *running_mean, float *running_var,
                            float *stats, void *y, const float *partial, int nblk, const int32_t *m_dev, void *stream);
/* The same, also storing the ReLU decision of every element as one bit (relu_mask u8[M][C/8]; bf16 with residual and ReLU only),
 * and the backward that reads those bits instead of the saved output y (1/16 of its bytes, in both passes of the backward). */
int bfhip_bn2d_fwd_partials_mask(const void *x, const void *residual, const float *gamma, const float *beta, long long M, int C,
                                 int dtype, float eps, float momentum, int relu, float *running_mean, float *running_var,
                                 float *stats, void *y, const float *partial, int nblk, const int32_t *m_dev,
                                 unsigned char *relu_mask, void *stream);
int bfhip_bn2d_bwd_mask(const void *dy, const void *x, const unsigned char *relu_mask, const float *stats, const float *gamma,
                        long long M, int C, int dtype, void *dx, void *dres, float *dgb, const int32_t *m_dev, void *workspace,
                        size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * gradient clipping + AdamW + bf16 parameter refresh of all parameter tensors in three launches
 *   (replaces, in the benchmarked training step, clip_grad_norm_ + torch.optim.AdamW of the reference's optim_wrapper,
 *   projects/BEVFusion/configs/nuscenes/bevfusion_lidar_voxel0075_second_secfpn_8xb4-cyclic-20e_nus-3d.py:369-372)
 *   segs_dev      : n_tensors records of bfhip_adamw_segment_bytes() bytes each:
 *                   { float *master, *m, *v; uint16_t *lowp (bf16 copy or NULL); int64 n; int32 grad_bf16, group }
 *                   (group: row of the group table of bfhip_adamw_step_groups, 0 = the single group; ignored by
 *                   bfhip_adamw_step)
 *   grad_ptrs_dev : int64[n_tensors] device addresses of this step's gradients (0: no gradient = zero gradient), element
 *                   order = the parameter's own memory order
 *   chunks_dev    : int32[n_chunks][2] = (tensor, chunk index) covering every tensor in chunks of bfhip_adamw_chunk_elems()
 *   partial_dev   : f32[n_chunks] scratch; scalars_dev : f32[8] persistent state ([2] = step count; zero it once):
 *                   after the call [0] clip scale, [1] 1 if the gradient norm was NaN / inf (nothing was updated), [5] the norm
 *   max_norm <= 0 : no clipping.  Arithmetic: torch's fused AdamW (decoupled weight decay, fp32), bf16 copy rounded once.
 * --------------------------------------------------------------------------------------- */
int bfhip_adamw_segment_bytes(void);
int bfhip_adamw_chunk_elems(void);
int bfhip_adamw_step(const void *segs_dev, const int64_t *grad_ptrs_dev, const int32_t *chunks_dev, int n_chunks,
                     float *partial_dev, float *scalars_dev, float lr, float beta1, float beta2, float eps,
                     float weight_decay, float max_norm, void *stream);
/* ---------------------------------------------------------------------------------------
 * the same step with parameter groups and per-step hyper-parameters (mmengine's paramwise_cfg: a smaller lr for the backbone,
 *   no weight decay on norms and biases; the reference's LinearLR / CosineAnnealingLR / CosineAnnealingMomentum schedules,
 *   projects/BEVFusion/configs/nuscenes/bevfusion_lidar_voxel0075_second_secfpn_8xb4-cyclic-20e_nus-3d.py:328-372)
 *   segs_dev, grad_ptrs_dev, chunks_dev, partial_dev, scalars_dev, max_norm : as bfhip_adamw_step; a tensor's `group` field
 *                   selects its record.  After the call also scalars[6] = 1 if some tensor named a group >= n_groups (that
 *                   tensor was not updated; nothing is read past the table)
 *   groups_dev    : f32[n_groups][8] device records; the caller writes [0] lr, [1] beta1, [2] beta2, [3] eps, [4] weight_decay
 *                   before every call (stream-ordered, e.g. in the same upload as grad_ptrs_dev); the call fills
 *                   [5] 1 - beta1^step and [6] sqrt(1 - beta2^step); [7] unused
 *   groups_host   : the same n_groups records in host memory, read during the call only: every group is checked here
 *                   (lr >= 0, 0 <= beta < 1, eps > 0; BFHIP_E_INVALID names the group), no device read
 *   The gradient norm, the clip scale, found_inf and the step counter (scalars[2]) are global, over all groups, as
 *   clip_grad_norm_ over all parameters.  Three launches.  With n_groups = 1 the results are bit-identical to bfhip_adamw_step
 *   with the same values by value.
 * --------------------------------------------------------------------------------------- */
int bfhip_adamw_step_groups(const void *segs_dev, const int64_t *grad_ptrs_dev, const int32_t *chunks_dev, int n_chunks,
                            float *partial_dev, float *scalars_dev, float *groups_dev, const float *groups_host, int n_groups,
                            float max_norm, void *stream);

/* ---------------------------------------------------------------------------------------
 * Shifted-window multi-head self-attention of the Swin image backbone (csrc/swin_attn.hip; the reference's camera configs build
 *   img_backbone = mmdet.SwinTransformer, whose ShiftWindowMSA pads, rolls, partitions, masks and un-partitions through copies).
 *   Window 7, head dim 32, bf16 with fp32 softmax statistics; roll, partition, bias, mask and softmax are inside the kernel.
 *   qkv   bf16 [B, Hp, Wp, 3C] with token pitch qkv_pitch (elements, >= 3C, multiple of 8), C = heads * 32, channel =
 *         which * C + head * 32 + d (which: 0 q, 1 k, 2 v) -- the qkv Linear's output as it is; Hp, Wp multiples of 7
 *   bias  f32 [heads, 49, 49]: the relative-position table gathered to (query, key) pairs
 *   shift 0 | 3: token (h, w) sits in the window of ((h - shift) mod Hp, (w - shift) mod Wp); with shift > 0 a -100 is added
 *         where query and key lie in different regions ([0, L-7), [L-7, L-3), [L-3, L) of the shifted coordinate, per axis)
 *   out   bf16 [B, Hp, Wp, C] dense; lse f32 [B, Hp, Wp, heads]
 *   bwd   recomputes the probabilities from lse; dqkv bf16 [B, Hp, Wp, 3C] dense, every element written; dbias_partial f32
 *         [parts, heads, 49, 49] with parts = bfhip_swin_attn_parts(): one slab per workgroup column, each summed in a fixed
 *         order; the caller adds the slabs.  No floating-point atomics: forward and backward are run-to-run reproducible.
 *   bfhip_swin_attn_supported / _parts are host-only (no device needed); supported answers 0 for any other window, head dim,
 *   shift, or an Hp / Wp that is not a multiple of 7.
 * --------------------------------------------------------------------------------------- */
int bfhip_swin_attn_supported(int B, int Hp, int Wp, int heads, int window, int head_dim, int shift);
int bfhip_swin_attn_parts(int B, int Hp, int Wp, int heads);
int bfhip_swin_attn_fwd(const void *qkv, long long qkv_pitch, const float *bias, int B, int Hp, int Wp, int heads, int shift,
                        float scale, void *out, float *lse, void *stream);
int bfhip_swin_attn_bwd(const void *qkv, long long qkv_pitch, const float *bias, const void *out, const void *dout,
                        const float *lse, int B, int Hp, int Wp, int heads, int shift, float scale, void *dqkv,
                        float *dbias_partial, int parts, void *stream);

/* ---------------------------------------------------------------------------------------
 * Row-wise LayerNorm with the residual update in front of it (csrc/layernorm.hip): the token-wise glue of a transformer block
 *   (mmdet's SwinBlock: LayerNorm, cast, drop path, residual add, twice per block) over a row-major [M, C] matrix.
 *   dtypes 0 = f32, 1 = bf16: x_dtype for x / s / dsum / dx, branch_dtype for branch / dbranch, y_dtype for y / dy; gamma, beta,
 *   scale and the statistics are f32 and all arithmetic is fp32.  C a multiple of 8, C <= 1536, M < 2^31, every tensor dense and
 *   16-byte aligned.  The mode is which pointers are given:
 *     norm        branch = s = NULL:  y = LN(x) * gamma + beta, mean_rstd f32 [M, 2] = (mean, 1 / sqrt(var + eps)) per row
 *     add + norm  branch, s, y:       s = x + scale[row / rows_per_sample] * branch, stored in x's dtype; y = LN(s as stored) ...
 *     add         branch, s, y = NULL: s only (gamma, beta, mean_rstd unused)
 *   scale f32 [M / rows_per_sample] or NULL (= 1): the per-sample drop-path factor.  The variance is the biased two-pass form.
 *   bwd   with g = dy * gamma and x_hat recomputed from the saved s: dLN = rstd * (g - mean_C(g) - x_hat * mean_C(g * x_hat));
 *         ds = dLN + dsum, where dsum (the gradient of the s output) or dy may be NULL; dx = ds, dbranch = scale * ds, each
 *         written only when its pointer is given.  dgamma = sum_rows dy * x_hat and dbeta = sum_rows dy (f32 [C]) are produced
 *         when partial (f32 [parts, 2, C], parts = bfhip_layernorm_parts()), dgamma and dbeta are given, NULL all three
 *         otherwise: one partial row per workgroup, added by a second small launch in a fixed order.  No atomics: forward and
 *         backward are run-to-run reproducible.  No allocation, no synchronisation; everything runs on `stream`.
 *   bfhip_layernorm_supported / _parts are host-only (no device needed); supported answers 0 for a C that is not a multiple of 8
 *   or exceeds 1536, an M outside [1, 2^31) or a dtype other than 0 / 1.
 * --------------------------------------------------------------------------------------- */
int bfhip_layernorm_supported(long long M, int C, int x_dtype, int y_dtype);
int bfhip_layernorm_parts(long long M, int C);
int bfhip_layernorm_fwd(const void *x, const void *branch, const float *scale, long long rows_per_sample, const float *gamma,
                        const float *beta, long long M, int C, float eps, int x_dtype, int branch_dtype, int y_dtype, void *s,
                        void *y, float *mean_rstd, void *stream);
int bfhip_layernorm_bwd(const void *s, const float *mean_rstd, const float *gamma, const void *dy, const void *dsum,
                        const float *scale, long long rows_per_sample, long long M, int C, int x_dtype, int branch_dtype,
                        int y_dtype, void *dx, void *dbranch, float *partial, int parts, float *dgamma, float *dbeta,
                        void *stream);

/* ---------------------------------------------------------------------------------------
 * Eval-mode BatchNorm (+ residual add) (+ ReLU) over a dense row-major [M, C] matrix (csrc/bn_eval.hip): BatchNorm on its
 *   RUNNING statistics -- inference, mmdet's norm_eval, frozen backbone stages -- for a channels-last [N, C, H, W] activation
 *   (M = N*H*W) or a feature matrix [M, C].
 *   dtype: 0 = f32, 1 = bf16 (x, residual, y, dy, dx, dres share it); gamma, beta and the running statistics are f32 and are
 *   only read.  C must be a multiple of the 16-byte vector (4 f32 / 8 bf16) with at most 512 vectors per row, M in [1, 2^31)
 *   (M = 1 is legal: there are no batch statistics): bfhip_bn_eval_supported() tells.  All arithmetic is fp32, one rounding
 *   at the store.
 *   fwd   y = act((x - running_mean) * a + beta [+ residual]), a = gamma / sqrt(running_var + eps); one launch, no workspace.
 *   bwd   g = dy * [y > 0] with relu (y is read only then and may be NULL otherwise), g = dy without; dx = g * a and dres = g,
 *         each written only when its pointer is given.  dgb f32[2C] <- (dgamma, dbeta) = (sum_rows g * x_hat, sum_rows g) with
 *         x_hat = (x - running_mean) / sqrt(running_var + eps) when x, partial (f32 [bfhip_bn_eval_parts()][2][C]) and dgb are
 *         given, NULL all three otherwise: one partial row per workgroup, added by a second small launch in a fixed order.  No
 *         atomics: run-to-run reproducible.  No allocation, no synchronisation; everything runs on `stream`.
 *   bfhip_bn_eval_supported / _parts are host-only (no device needed).
 * --------------------------------------------------------------------------------------- */
int bfhip_bn_eval_supported(long long M, int C, int dtype);
int bfhip_bn_eval_parts(long long M, int C, int dtype);
int bfhip_bn_eval_fwd(const void *x, const void *residual, const float *gamma, const float *beta, const float *running_mean,
                      const float *running_var, long long M, int C, int dtype, float eps, int relu, void *y, void *stream);
int bfhip_bn_eval_bwd(const void *dy, const void *y, const void *x, const float *gamma, const float *running_mean,
                      const float *running_var, long long M, int C, int dtype, float eps, int relu, void *dx, void *dres,
                      float *partial, float *dgb, void *stream);

/* ---------------------------------------------------------------------------------------
 * Eval-mode BatchNorm over a CAPACITY-sized [M, C] matrix whose active rows are a prefix counted on the device
 *   (csrc/bn_eval.hip; the static capacity mode of the sparse encoder in eval).  Same arguments and shapes as
 *   bfhip_bn_eval_fwd / _bwd plus rows_dev, a device i32[1]; with n = min(max(*rows_dev, 0), M):
 *   fwd   rows < n get what bfhip_bn_eval_fwd computes, bit for bit; rows [n, M) are WRITTEN AS ZEROS whatever x and residual
 *         hold there (NaN included).
 *   bwd   rows < n as bfhip_bn_eval_bwd; rows >= n get dx = dres = 0 and add nothing to dgamma / dbeta.  partial has
 *         bfhip_bn_eval_parts(M, C, dtype) rows (the partition of the capacity), so dgb equals, bit for bit, what
 *         bfhip_bn_eval_bwd gives on the same matrix with dy zeroed beyond n.  No atomics: run-to-run reproducible.
 *   The kernels read the count themselves (one uniform load per workgroup): no extra launch, workspace, allocation or
 *   synchronisation; everything runs on `stream`.  bfhip_bn_eval_supported(M, C, dtype) decides the shapes.
 * --------------------------------------------------------------------------------------- */
int bfhip_bn_eval_rows_fwd(const void *x, const void *residual, const float *gamma, const float *beta,
                           const float *running_mean, const float *running_var, long long M, int C, int dtype, float eps,
                           int relu, void *y, const int32_t *rows_dev, void *stream);
int bfhip_bn_eval_rows_bwd(const void *dy, const void *y, const void *x, const float *gamma, const float *running_mean,
                           const float *running_var, long long M, int C, int dtype, float eps, int relu, void *dx, void *dres,
                           float *partial, float *dgb, const int32_t *rows_dev, void *stream);

/* ---------------------------------------------------------------------------------------
 * Camera-image preprocessing (csrc/preprocess.hip): the image path of the reference's Det3DDataPreprocessor
 *   (M3D/models/data_preprocessors/data_preprocessor.py:126-330: channel swap, .float(), (x - mean) / std, pad to the size
 *   divisor at the bottom and right, stack) in one pass that also writes the dtype and memory format the backbone reads.
 *   samples_host: n_samples descriptors in HOST memory; sample i is a dense DEVICE block [views, 3, h_i, w_i] of raw pixel
 *     values, src_dtype 0 = uint8, 1 = float32 (one dtype and one view count for all samples; h and w may differ).  The
 *     descriptors travel in the kernel arguments, bfhip_img_preprocess_max_samples() per launch; a longer list is cut into
 *     that many launches.  No device table, no copy.
 *   out[b, v, c, y, x] = (float(src_b[v, c', y, x]) - mean_host[c]) / std_host[c] inside the image (c' = 2 - c with swap_rb, else
 *     c; with normalise = 0 just the float value, mean_host / std_host may be NULL) and pad_value itself outside (y >= h_b or
 *     x >= w_b).  fp32 arithmetic in that order with a true division: bit-identical to the IEEE result.  out_dtype 0 = f32,
 *     1 = bf16 (that fp32 value rounded to nearest even once).  Hp >= max h and Wp >= max w, or BFHIP_E_INVALID.
 *   out layout: pixel_major = 0: [n_samples, views, 3, Hp, Wp] contiguous; 1: [n_samples * views, Hp, Wp, 3] (the storage of
 *     a channels-last [n_samples * views, 3, Hp, Wp] tensor).  Every element of out is written exactly once, padding included.
 *     16-byte stores are used when Wp is a multiple of 8 and out is 16-byte aligned; any other Wp or alignment is legal.
 *   No allocation, no synchronisation; everything runs on `stream`.
 * --------------------------------------------------------------------------------------- */
typedef struct bfhip_img_desc {
  const void *data; /* device pointer of the [views, 3, h, w] block */
  int h, w;
} bfhip_img_desc;
int bfhip_img_preprocess_max_samples(void);
int bfhip_img_preprocess(const bfhip_img_desc *samples_host, int n_samples, int views, int src_dtype, int swap_rb, int normalise,
                         const float *mean_host, const float *std_host, float pad_value, int Hp, int Wp, int out_dtype,
                         int pixel_major, void *out, void *stream);

/* ---------------------------------------------------------------------------------------
 * ImageAug3D on the device (csrc/image_aug.hip): PIL's bicubic antialiased resize, crop (zero outside), mirror and nearest
 *   rotation of raw uint8 frames, bit for bit, followed by everything bfhip_img_preprocess does.  Two launches per
 *   bfhip_image_aug_max_cams() cameras: resize + crop + flip into the uint8 intermediate `mid` [n_samples * views, 3, fH, fW],
 *   then rotate + swap + normalise + pad + cast into `out` (when no camera rotates the second launch is bfhip_img_preprocess).
 *   cams_host: n_samples * views descriptors in HOST memory.  data: DEVICE pointer of the camera's frame, uint8 [h, w, 3]
 *     pixel-major; crop: left / top of the fH x fW crop in the resized image (may hang over any edge: zero there); flip: mirror
 *     left-right after the crop; rotates != 0: gather out[Y, X] = in[(a5 + X a3 + Y a4) >> 16, (a2 + X a0 + Y a1) >> 16], int32,
 *     zero outside.  The crop's overlap with the resized image is [h_first, h_first + h_count) x [v_first, v_first + v_count)
 *     in resized coordinates (a count of 0: the whole output is zero); its resampling tables start at int h_off / v_off of the
 *     tables: per output one entry (lo, n, k_0 .. k_{taps-1}): out = clamp((2^21 + sum_{j < n} px[lo + j] * k_j) >> 22, 0, 255),
 *     horizontal pass first with a uint8 result in between, int32 accumulators.
 *   tables_host / tables_dev: the same table_ints int32 values in host and in device memory.  The host copy is validated
 *     before anything is launched (every entry inside its source, bounds not decreasing, taps <= bfhip_image_aug_max_taps(),
 *     no 64-column / 16-row tile over more source than the kernel stages): BFHIP_E_INVALID otherwise.
 *   bfhip_image_aug_supported: 1 when an axis pair with these sizes and tap counts is within those bounds (taps <= 24 and
 *     source / resized <= 6.25 per axis: every resize >= 0.2 of a source of 39 pixels or more a side).
 *   swap_rb .. pixel_major, out: as bfhip_img_preprocess with h = fH and w = fW; every element of out and of mid is written
 *     exactly once.  No allocation, no synchronisation; everything runs on `stream`.
 * --------------------------------------------------------------------------------------- */
typedef struct bfhip_image_aug_cam {
  const void *data;
  int h, w;
  int crop[2];
  int flip, rotates;
  int a[6];
  int h_off, h_taps, h_first, h_count;
  int v_off, v_taps, v_first, v_count;
} bfhip_image_aug_cam;
int bfhip_image_aug_max_taps(void);
int bfhip_image_aug_max_cams(void);
int bfhip_image_aug_supported(int src_h, int src_w, int new_h, int new_w, int fH, int fW, int h_taps, int v_taps);
int bfhip_image_aug(const bfhip_image_aug_cam *cams_host, int n_samples, int views, const int32_t *tables_host,
                    const int32_t *tables_dev, long long table_ints, int fH, int fW, void *mid, int swap_rb, int normalise,
                    const float *mean_host, const float *std_host, float pad_value, int Hp, int Wp, int out_dtype,
                    int pixel_major, void *out, void *stream);

/* ---------------------------------------------------------------------------------------
 * GridMask fused into ImageAug3D on the device: bfhip_image_aug with one mask record per sample.
 *   masks_host: NULL, or n_samples records in HOST memory; they travel in the kernel arguments.  active == 0: the sample has
 *     no mask.  The mask is defined on an hh x ww canvas of ones; with use_h canvas row Y is 0 when t = Y - st_h >= 0,
 *     t / d < hh / d and t % d < length, with use_w column X likewise with st_w and ww.  Output pixel (y, x), y < fH, x < fW, of
 *     every camera of the sample reads the canvas at (Y, X) = (y + crop[0], x + crop[1]); rotates != 0: at
 *     ((a5 + X a3 + Y a4) >> 16, (a2 + X a0 + Y a1) >> 16) instead, int32, 0 outside the canvas (PIL's nearest rotate(r)).
 *     mode != 0 inverts.  Where the mask is 0 the pixel's three channels are 0 before the normalisation; padding keeps
 *     pad_value.  r is the angle in degrees the terms were made from and is not read.
 *   Validated before anything is launched: d >= 2, 1 <= length < d, 0 <= st_h, st_w < d, hh, ww >= 1 and the fH x fW window
 *     from crop inside the canvas: BFHIP_E_INVALID otherwise.
 *   With masks_host NULL or no active record the launches are those of bfhip_image_aug.  Otherwise the second launch is the
 *     finish kernel whether or not a camera rotates; no further launch, upload or buffer.
 * --------------------------------------------------------------------------------------- */
typedef struct bfhip_grid_mask {
  int active;
  int d, length, st_h, st_w;
  int use_h, use_w, mode;
  int hh, ww;
  int crop[2]; /* top, left of the window in the canvas */
  int r, rotates;
  int a[6];
} bfhip_grid_mask;
int bfhip_image_aug_masked(const bfhip_image_aug_cam *cams_host, const bfhip_grid_mask *masks_host, int n_samples, int views,
                           const int32_t *tables_host, const int32_t *tables_dev, long long table_ints, int fH, int fW, void *mid,
                           int swap_rb, int normalise, const float *mean_host, const float *std_host, float pad_value, int Hp,
                           int Wp, int out_dtype, int pixel_major, void *out, void *stream);

/* ---------------------------------------------------------------------------------------
 * The point half of the LiDAR augmentation chain on the device (csrc/points_aug.hip): GlobalRotScaleTrans /
 *   BEVFusionGlobalRotScaleTrans, BEVFusionRandomFlip3D, PointsRangeFilter and PointShuffle
 *   (M3D/datasets/transforms/transforms_3d.py:631-956, BF/transforms_3d.py:130-201) of a whole batch in three launches per 16
 *   samples: count per block, one-block scan, ranked write.
 *   samples_host: n_samples descriptors in HOST memory.  points: DEVICE float32 [n, C], 4-byte aligned, 3 <= C <= 8.
 *     flags: 1 rotate + translate + scale present; 2 scale before translate (R,S,T; otherwise R,T,S); 4 negate y (horizontal
 *     flip); 8 negate x (vertical flip); 16 range filter present; 32 shuffle.  rot: rot_mat_T row-major,
 *     x' = (x rot[0] + y rot[3]) + z rot[6], y' with rot[1], rot[4], rot[7], z' with rot[2], rot[5], rot[8]; then (v + trans) *
 *     scale, or v * scale + trans; every product and sum one float32 operation, never fused.  range: (x, y, z) minimum and
 *     maximum, a row is kept when every transformed coordinate is strictly inside.  keys: the round keys of the shuffle, a
 *     balanced Feistel network of BFHIP_POINTS_AUG_ROUNDS rounds on the next even power of two with cycle walking
 *     (bevfusion_amd/points_aug.py: shuffle_permutation is its definition).
 *   out: float32 [sum n, C]; sample i owns the rows from sum_{j < i} n_j on and its first kept[i] rows are written: the kept
 *     rows in input order, or, with the shuffle, the r-th kept row at row perm(r).  Columns 3 .. C-1 are copied.
 *   kept: int32 [n_samples], written for every sample (0 for an empty one).  sum n < 2^31.
 *   No allocation, no synchronisation; everything runs on `stream`.  bfhip_points_aug_block: rows per workgroup.
 * --------------------------------------------------------------------------------------- */
#define BFHIP_POINTS_AUG_ROUNDS 6
typedef struct bfhip_points_aug_sample {
  const float *points;
  int n;
  int flags;
  float rot[9];
  float trans[3];
  float scale;
  float range[6];
  uint32_t keys[BFHIP_POINTS_AUG_ROUNDS];
} bfhip_points_aug_sample;
int bfhip_points_aug_block(void);
size_t bfhip_points_aug_workspace_bytes(long long total_rows, int n_samples);
int bfhip_points_aug(const bfhip_points_aug_sample *samples_host, int n_samples, int C, float *out, int32_t *kept,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * bfhip_points_aug with ObjectSample's paste (M3D/datasets/transforms/transforms_3d.py:328-460) as the step in front: the
 *   original points inside any pasted box are dropped, the sampled objects' points are put in front of the rest, and the
 *   chain above runs on all rows.  Same three launches per 16 samples.
 *   pastes: n_samples descriptors in HOST memory, pastes[i] beside samples_host[i].  points: DEVICE float32 [n_points, C], the
 *     pasted rows (already translated to their boxes).  planes: DEVICE float32 [n_boxes, 6, 4], per box six inward plane
 *     equations (n0, n1, n2, d) (bevfusion_amd/points_aug.py: paste_planes); n_boxes <= bfhip_points_aug_max_boxes() = 64.
 *     An original row (x, y, z) is inside box j when ((x n0 + y n1) + z n2) + d < 0 for its six planes, every product and sum
 *     one float32 operation, on the UNtransformed coordinates; it is dropped when it is inside any box.  Pasted rows skip
 *     that test.  Both then pass through rotate / translate / scale, the flips and the range test.
 *   The row space of sample i is its n_points pasted rows, then its n original rows: its region of `out` starts at row
 *     sum_{j < i} (n_j + n_points_j), kept[i] counts pasted and original rows, and without the shuffle the kept pasted rows
 *     come first.  A sample with n_points = n_boxes = 0 behaves as in bfhip_points_aug.  sum (n + n_points) < 2^31; the
 *     workspace is bfhip_points_aug_workspace_bytes(that sum, n_samples).
 * --------------------------------------------------------------------------------------- */
typedef struct bfhip_points_aug_paste_desc {
  const float *points;
  int n_points;
  const float *planes;
  int n_boxes;
} bfhip_points_aug_paste_desc;
int bfhip_points_aug_max_boxes(void);
int bfhip_points_aug_paste(const bfhip_points_aug_sample *samples_host, const bfhip_points_aug_paste_desc *pastes_host,
                           int n_samples, int C, float *out, int32_t *kept, void *workspace, size_t workspace_bytes,
                           void *stream);

/* ---------------------------------------------------------------------------------------
 * bfhip_points_aug / bfhip_points_aug_paste with LoadPointsFromMultiSweeps (M3D/datasets/transforms/loading.py:316-453) as the
 *   step in front of everything: a sample's n rows are its keyframe and its sweeps as they were read from their files, one
 *   contiguous buffer [keyframe ; sweep 1 ; ... ; sweep S], cut into n_segments <= bfhip_points_aug_max_sweeps() = 16 segments
 *   (the keyframe is segment 0).  Same three launches per 16 samples; needs C >= 5.
 *   segment: first = its first row (of the sample's n); flags: 1 = remove close rows, 2 = transform; dt, radius; m = the 3 x 3
 *     of lidar2sensor, row-major; t = its translation column.  For a row (x, y, z) of the segment:
 *       flags & 1: the row is dropped when |x| < radius and |y| < radius, on the raw float32 x, y (a NaN keeps the row);
 *       flags & 2: v_j = (float)(((double)x * m[j] + (double)y * m[3 + j]) + (double)z * m[6 + j]), every product and sum one
 *                  float64 operation, then v_j = (float)((double)v_j - t[j]);
 *       column 4 = dt.
 *     Then the box test of a paste (on these xyz; pasted rows take no part in the sweep step), then the chain.
 *   sweeps: n_samples descriptors in HOST memory.  segments: DEVICE, 8-byte aligned, n_segments entries; first[]: the HOST copy of
 *     the boundaries, first[0] = 0 <= first[1] <= ... <= first[n_segments] = n, which the entry checks.  n_segments = 0: the
 *     sample has no sweep step and behaves as in bfhip_points_aug / bfhip_points_aug_paste.
 *   pastes: NULL (no sample has a paste) or as in bfhip_points_aug_paste; row space, `out`, `kept` and the workspace as there.
 * --------------------------------------------------------------------------------------- */
#define BFHIP_POINTS_AUG_MAX_SEGMENTS 16
typedef struct bfhip_points_aug_segment {
  int first;
  int flags;
  float dt;
  float radius;
  double m[9];
  double t[3];
} bfhip_points_aug_segment;
typedef struct bfhip_points_aug_sweeps_desc {
  const bfhip_points_aug_segment *segments;
  int n_segments;
  int first[BFHIP_POINTS_AUG_MAX_SEGMENTS + 1];
} bfhip_points_aug_sweeps_desc;
int bfhip_points_aug_max_sweeps(void);
int bfhip_points_aug_sweeps(const bfhip_points_aug_sample *samples_host, const bfhip_points_aug_paste_desc *pastes_host,
                            const bfhip_points_aug_sweeps_desc *sweeps_host, int n_samples, int C, float *out, int32_t *kept,
                            void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Query initialisation of the TransFusion head (csrc/query_init.hip; BF/bevfusion_head.py:221-260,278-281): 3x3 peak test,
 *   the K best masked scores of a sample and the gather of what the head reads at them.  Three launches, no host read.
 *   h: float32 score map [B, C, H, W] with element strides h_sb, h_sc, h_sy, h_sx (NCHW or channels-last; nothing is copied).
 *   m(b, c, y, x) = h where h > 0 and (bit c of nms_free_mask is set, or the cell is interior, 1 <= y <= H-2, 1 <= x <= W-2,
 *     and h >= each of its 8 neighbours in its class plane); 0 elsewhere.  A NaN is never a peak and fails every comparison.
 *   The picks of a sample are the first K of its C*H*W cells ordered by (m descending, flat = c*H*W + y*W + x ascending): equal
 *     scores go to the lower index, and with fewer than K positive cells the zero-valued cells follow in ascending flat index
 *     (NaN cells after all of those).  The order is a property of the input alone: the results are bit-reproducible.
 *   flat: the BEV feature rows, element (b, cell, ch) at flat + (b * flat_sb + cell * flat_sr + ch) elements, float32
 *     (row_dtype 0) or bf16 (1), 16-byte aligned rows.
 *   top_class, top_index: int64 [B, K] (flat / HW, flat % HW).  query_pos: float32 [B, K, 2] =
 *     (top_index / pos_w + 0.5, top_index % pos_w + 0.5).  query_heatmap_score: float32 [B, C, K], m of every class at the
 *     picked cell.  rows: [B, K, Ch] dense, row_dtype.
 *   bfhip_query_init_supported: 1 when nms_kernel_size == 3, 1 <= K <= 512, K <= C*H*W < 2^31, C <= 32, H, W >= 3 and Ch is a
 *     whole number of 16-byte vectors of row_dtype.  workspace: bfhip_query_init_workspace_bytes(B, C, H, W), 16-byte aligned
 *     (it holds the worst case, a constant map, where every cell is a candidate).
 *   bfhip_query_init_bwd: d_flat [B, HW, Ch] dense = 0, then d_flat[b, top_index[b, p], :] = sum of d_rows[b, p', :] over the
 *     picks p' of that cell in ascending p', summed in float32 and rounded once to row_dtype (memset + one launch, no atomics).
 *     d_rows [B, K, Ch] dense, 16-byte aligned.
 * --------------------------------------------------------------------------------------- */
int bfhip_query_init_supported(int B, int C, int H, int W, int K, int Ch, int nms_kernel_size, int row_dtype);
size_t bfhip_query_init_workspace_bytes(int B, int C, int H, int W);
int bfhip_query_init_fwd(const float *h, long long h_sb, long long h_sc, long long h_sy, long long h_sx, int B, int C, int H, int W,
                         unsigned nms_free_mask, const void *flat, long long flat_sb, long long flat_sr, int Ch, int row_dtype,
                         int K, int pos_w, long long *top_class, long long *top_index, float *query_pos,
                         float *query_heatmap_score, void *rows, void *workspace, size_t workspace_bytes, void *stream);
int bfhip_query_init_bwd(const long long *top_index, const void *d_rows, int B, int K, int Ch, long long HW, int row_dtype,
                         void *d_flat, void *stream);

/* ---------------------------------------------------------------------------------------
 * JPEG decode in two halves (csrc/jpeg_host.h, csrc/jpeg.hip): the serial entropy stage on the host, everything after it
 *   (dequantise, 8x8 inverse DCT, chroma upsampling, YCbCr -> RGB) on the device, bit for bit what libjpeg's default decode
 *   (accurate integer IDCT, fancy upsampling) gives.
 *   bfhip_jpeg_parse / bfhip_jpeg_entropy_decode: HOST ONLY -- no HIP call, safe in a loader's worker; they take untrusted
 *     bytes and neither read outside [bytes, bytes + n) nor write outside [coef, coef + coef_bytes).
 *   bfhip_jpeg_parse reads the markers up to the first scan.  0 with `supported` set or cleared (reason: BFHIP_JPEG_R_*), or
 *     BFHIP_E_INVALID for a malformed stream.  The fused path takes baseline sequential (SOF0) 8-bit files of three
 *     components in one scan, luma sampled 1x1, 2x1, 1x2 or 2x2 and chroma 1x1, 8-bit quantisation tables, no EXIF
 *     orientation tag.  For a supported stream: block_cols / block_rows per component padded to whole MCUs, quant per
 *     component in natural (row-major) order, coef_offset in int16 elements, coef_bytes the size of the coefficient buffer.
 *   bfhip_jpeg_entropy_decode writes, per component at coef_offset, [block_rows, block_cols, 64] int16 coefficients in natural
 *     order with the DC prediction undone, not dequantised.  Restart intervals, byte stuffing and the file's own Huffman
 *     tables are handled; a scan that ends early leaves the remaining blocks zero, as libjpeg does.  `header` must be what
 *     bfhip_jpeg_parse gave for the same bytes; coef_bytes >= header->coef_bytes.  0 or BFHIP_E_INVALID.
 *   bfhip_jpeg_decode: n_frames frames in TWO launches.  frames_host / frames_dev: the same descriptors in host and in device
 *     memory; the host copy is validated against coef_elems, planes_bytes and rgb_bytes before anything is launched.
 *     coef_off: int16 elements from coef_dev (a multiple of 8), the component's [block_rows, block_cols, 64] block.  plane_off:
 *     bytes from planes_dev (a multiple of 8), the component's uint8 plane [block_rows * 8, block_cols * 8], written by the
 *     first launch (dequantise + IDCT: 32-bit wrap-around arithmetic, column pass descaled by 11, row pass by 18, + 128,
 *     clamped) and read by the second (triangle-filter upsampling whose neighbours outside the component's real extent
 *     ceil(width / hs) x ceil(height / vs) are the nearest real sample; 16-bit fixed-point colour conversion).  rgb_off: bytes
 *     from rgb_dev of the frame's uint8 [height, width, 3] block; exactly those bytes are written.  hs, vs: luma sampling,
 *     1 or 2 each; chroma is 1x1.  Frames must not overlap in planes_dev or rgb_dev.  n_frames <= 65535.
 *     No allocation, no synchronisation; everything runs on `stream`.
 * --------------------------------------------------------------------------------------- */
#define BFHIP_JPEG_R_OK 0
#define BFHIP_JPEG_R_PROGRESSIVE 1
#define BFHIP_JPEG_R_ARITHMETIC 2
#define BFHIP_JPEG_R_PRECISION 3        /* not 8 bits per sample */
#define BFHIP_JPEG_R_COMPONENTS 4       /* not three components */
#define BFHIP_JPEG_R_MULTI_SCAN 5       /* the first scan does not hold every component */
#define BFHIP_JPEG_R_QUANT16 6          /* a 16-bit quantisation table */
#define BFHIP_JPEG_R_SAMPLING 7
#define BFHIP_JPEG_R_EXIF_ORIENTATION 8
#define BFHIP_JPEG_R_NOT_BASELINE 9     /* extended sequential, lossless or hierarchical */
#define BFHIP_JPEG_R_COLOUR_SPACE 10    /* the components are not YCbCr (no JFIF marker and Adobe / the ids say RGB) */
typedef struct bfhip_jpeg_header {
  int32_t width, height, ncomp;
  int32_t supported, reason;
  int32_t restart_interval;
  int32_t mcus_x, mcus_y;
  int32_t hs[3], vs[3];
  int32_t block_cols[3], block_rows[3];
  int64_t coef_offset[3];
  int64_t coef_bytes;
  uint16_t quant[3][64];
} bfhip_jpeg_header;
typedef struct bfhip_jpeg_frame {
  int64_t coef_off[3];
  int64_t plane_off[3];
  int64_t rgb_off;
  int32_t width, height;
  int32_t hs, vs;
  int32_t block_cols[3], block_rows[3];
  uint16_t quant[3][64];
} bfhip_jpeg_frame;
int bfhip_jpeg_parse(const uint8_t *bytes, size_t n, bfhip_jpeg_header *header);
int bfhip_jpeg_entropy_decode(const uint8_t *bytes, size_t n, const bfhip_jpeg_header *header, int16_t *coef, size_t coef_bytes);
int bfhip_jpeg_decode(const bfhip_jpeg_frame *frames_host, const bfhip_jpeg_frame *frames_dev, int n_frames,
                      const int16_t *coef_dev, size_t coef_elems, uint8_t *planes_dev, size_t planes_bytes, uint8_t *rgb_dev,
                      size_t rgb_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Baseline JPEG encode (csrc/jpeg_encode_host.h, csrc/jpeg_encode.hip): the decoder turned round.  RGB -> YCbCr, edge padding,
 *   chroma downsampling, libjpeg's accurate integer forward DCT (jfdctint) and quantisation leave int16 coefficients in the
 *   decoder's layout (per component [block_rows, block_cols, 64], natural order, DC not differenced); the Huffman stage codes
 *   them with the Annex K tables.  bevfusion_amd/jpeg_encode.py: torch_jpeg_forward defines the coefficients in int32
 *   wrap-around arithmetic, and the host entropy encoder defines the bytes.  Luma sampling hs x vs is 1x1, 2x1 or 2x2.
 *   bfhip_jpeg_entropy_encode: HOST ONLY, no HIP call.  header: geometry as bfhip_jpeg_parse leaves it (width, height, hs, vs,
 *     mcus, block_cols / block_rows, coef_offset, coef_bytes; the quantisation tables are not read); coef_bytes >=
 *     header->coef_bytes.  restart_interval: MCUs between restart markers, 0 = none, at most 65535.  Writes the scan --
 *     interleaved MCUs, DC differences per component reset at every restart, zigzag order, ZRL for runs above 15, EOB unless
 *     coefficient 63 is non-zero, FF stuffed with 00, the last byte of every interval padded with 1-bits, RSTm with m counting
 *     modulo 8 -- and the EOI marker behind it into out[0 .. capacity).  BFHIP_E_INVALID, with not one byte written at or past
 *     `capacity`, when the stream is longer than capacity (stats->bytes then holds the needed length), when an AC coefficient
 *     lies outside +-1023 or a DC difference outside +-2047 (neither has a Huffman code) or when the header is inconsistent.
 *     stats (may be NULL): bytes written (the needed length on overflow), stuffed bytes, ZRL symbols, EOBs and the largest AC
 *     and DC categories met.
 *   The device entry points take a descriptor table, one bfhip_jpeg_enc_frame per frame, in host and in device memory (the same
 *     bytes; frames_dev 16-byte aligned); the host copy is validated before anything is launched: dimensions 1 .. 65535, a
 *     sampling bfhip_jpeg_encode_supported takes, block counts that fit the frame, no zero quantisation entry, every range
 *     inside its buffer, frames in ascending order of out_off and ws_off without overlap, n_frames 1 ..
 *     bfhip_jpeg_encode_max_frames() = 65535.  Frames of different sizes, samplings and tables share the launches.
 *     rgb_off: bytes from rgb_dev of the frame's uint8 [height, width, 3] pixels.  coef_off: int16 elements from coef_dev (a
 *     multiple of 8; coef_dev 16-byte aligned).  out_off / capacity: bytes from out_dev of the frame's stream and how many it
 *     may take.  ws_off: bytes from the workspace (a multiple of 256) of the frame's bfhip_jpeg_encode_workspace_bytes(width,
 *     height, hs, vs) bytes.  quant: natural order, components 1 and 2 usually equal.
 *   bfhip_jpeg_forward (one launch): pixels -> coefficients: jccolor's 16-bit fixed-point colour conversion; components
 *     extended by repeating their last column and row, the downsampled chroma plane extended by its last downsampled row; h2v2
 *     (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2 ..., h2v1 (a + b + bias) >> 1 with bias 0, 1, 0, 1 ...; - 128; rows
 *     first (outputs 0 and 4 shifted left by 2, the rest descaled by 11), columns second (0 and 4 descaled by 2, the rest by
 *     15); (|x| + (8 q >> 1)) / (8 q) truncated, sign restored.  A luma block wholly outside ceil(W / 8) x ceil(H / 8) is zero
 *     but for its DC, which is the DC of the block to its left, or -- in a block row below the last real one -- of the rightmost
 *     block of the row above within the same MCU (libjpeg's dummy blocks).
 *   bfhip_jpeg_entropy_encode_device (two launches): coefficients -> each frame's scan with a restart marker after EVERY MCU
 *     row (the unit of parallelism) and EOI, the bytes the host encoder gives with restart_interval = mcus_x.  result: int64
 *     [n_frames, 2]: the stream's length -- the NEEDED length when it exceeds the capacity -- and flags: BFHIP_JPEG_ENC_OVERFLOW
 *     (nothing was written at or past out_off + capacity), BFHIP_JPEG_ENC_BAD_COEF (a coefficient without a Huffman code was met
 *     and clamped: the stream is not to be used).
 *   bfhip_jpeg_encode: both (three launches).  The markers in front of the scan are the caller's (jpeg_encode.py).
 *   Integer arithmetic only (the slab's boundary words are completed with integer atomic OR, which commutes): the same bytes on
 *   every run.  No allocation, no synchronisation; everything runs on `stream`.
 * --------------------------------------------------------------------------------------- */
#define BFHIP_JPEG_ENC_OVERFLOW 1
#define BFHIP_JPEG_ENC_BAD_COEF 2
typedef struct bfhip_jpeg_enc_stats {
  int64_t bytes;
  int64_t stuffed;
  int64_t zrl;
  int64_t eob;
  int32_t max_ac_category, max_dc_category;
} bfhip_jpeg_enc_stats;
typedef struct bfhip_jpeg_enc_frame {
  int64_t rgb_off;
  int64_t coef_off[3];
  int64_t out_off, capacity;
  int64_t ws_off;
  int32_t width, height;
  int32_t hs, vs;
  int32_t block_cols[3], block_rows[3];
  uint16_t quant[3][64];
} bfhip_jpeg_enc_frame;
int bfhip_jpeg_entropy_encode(const bfhip_jpeg_header *header, const int16_t *coef, size_t coef_bytes, int restart_interval,
                              uint8_t *out, size_t capacity, bfhip_jpeg_enc_stats *stats);
int bfhip_jpeg_encode_supported(int width, int height, int hs, int vs);
size_t bfhip_jpeg_encode_workspace_bytes(int width, int height, int hs, int vs);
int bfhip_jpeg_encode_max_frames(void);
int bfhip_jpeg_forward(const bfhip_jpeg_enc_frame *frames_host, const bfhip_jpeg_enc_frame *frames_dev, int n_frames,
                       const uint8_t *rgb_dev, size_t rgb_bytes, int16_t *coef_dev, size_t coef_elems, void *stream);
int bfhip_jpeg_entropy_encode_device(const bfhip_jpeg_enc_frame *frames_host, const bfhip_jpeg_enc_frame *frames_dev, int n_frames,
                                     const int16_t *coef_dev, size_t coef_elems, void *workspace, size_t workspace_bytes,
                                     uint8_t *out_dev, size_t out_bytes, int64_t *result_dev, void *stream);
int bfhip_jpeg_encode(const bfhip_jpeg_enc_frame *frames_host, const bfhip_jpeg_enc_frame *frames_dev, int n_frames,
                      const uint8_t *rgb_dev, size_t rgb_bytes, int16_t *coef_dev, size_t coef_elems, void *workspace,
                      size_t workspace_bytes, uint8_t *out_dev, size_t out_bytes, int64_t *result_dev, void *stream);

/* ---------------------------------------------------------------------------------------
 * Lossless PNG encode (csrc/png_encode_host.h, csrc/png_encode.hip): 8-bit RGB frames -> the zlib stream of a PNG file's IDAT
 *   chunk, in a restricted DEFLATE that runs in parallel.  bevfusion_amd/png_encode.py defines the format byte for byte.
 *   Filter: per row the type (None, Sub, Up, Average, Paeth over the RAW row above) with the least sum of v < 128 ? v : 256 - v
 *     over its filtered bytes, the lowest type on a tie; the row above the first and the bytes left of the first pixel are
 *     zero.  Filtered data: [height, 1 + 3 width], the type in front of each row.
 *   Stream: 78 01, then one DEFLATE block per band of band_bytes filtered bytes, each band on a byte boundary.  Tokens: a
 *     maximal stretch of equal bytes inside a band is a literal, matches of distance 1 and length min(r, 258) while r >= 3
 *     bytes remain, then 0-2 literals.  A band is a dynamic block (HLIT 29, HDIST 0, HCLEN 15; code-length symbols 0-15 on four
 *     bits; a 15-bit length-limited code from package-merge over the band's 286-symbol histogram, ties by symbol index; one
 *     distance code of one bit when the band has a match) followed, unless it is the last, by an empty stored block (00 00 FF
 *     FF); or, when that is not smaller than n + 5 ceil(n / 65535) bytes, stored blocks.  A stream therefore never exceeds
 *     bfhip_png_capacity(n_bytes, band_bytes) = 2 + the sum of that bound over its bands.  The Adler-32 trailer is NOT written:
 *     the caller combines it from the per-band (A, B, n) triples and appends it, as it writes the PNG chunks and their CRCs.
 *   bfhip_png_frame: src_off: bytes from rgb_dev of the uint8 [height, width, 3] pixels (encode) or from data_dev of the bytes
 *     (deflate: width and height are not read).  out_off / capacity: bytes from out_dev of the stream and how many it may take.
 *     ws_off: bytes from the workspace, a multiple of 256, of bfhip_png_workspace_bytes(n_bytes, band_bytes, with_filter) bytes.
 *     res_off: uint32 words from result_dev of the job's bfhip_png_result_words(n_bytes, band_bytes) words: stream length (low,
 *     high word; the NEEDED length on overflow), flags (BFHIP_PNG_OVERFLOW: nothing was written at or past out_off + capacity),
 *     stored bands, dynamic bands, longest code, bands, 0; then per band Adler A, B of the band alone, its length, its bytes in
 *     the stream | stored << 31.  n_bytes: 1 .. 2^31 - 1, for encode height (1 + 3 width).  band_bytes: 1 .. 2^26, for encode
 *     a whole number of rows.  Jobs in ascending order of out_off, ws_off and res_off without overlap; at most
 *     bfhip_png_encode_max_frames() = 65535 of them; the host copy of the table is validated before anything is launched.
 *   bfhip_png_encode: four launches whatever the batch (filter; per band histogram, Adler sums, code construction, decision and
 *     emission into the band's slab, which the kernel zeroes itself; band offsets and results; compaction).  bfhip_png_deflate:
 *     the last three over bytes already on the device.  Integer arithmetic only (integer atomic OR and LDS adds, which
 *     commute): the same bytes on every run.  No allocation, no synchronisation; everything runs on `stream`.
 *   HOST ONLY, no HIP call: bfhip_png_filter_host, bfhip_png_huffman_lengths (lens[n_symbols], n_symbols <= 286, max_len <= 15)
 *     and bfhip_png_deflate_host (bands: 4 words per band as above, may be NULL; BFHIP_E_INVALID with nothing written at or past
 *     `capacity` when the stream is longer, stats->bytes then holds the needed length).
 * --------------------------------------------------------------------------------------- */
#define BFHIP_PNG_OVERFLOW 1
typedef struct bfhip_png_stats {
  int64_t bytes;
  int64_t bands, stored_bands, dynamic_bands;
  int64_t tokens;
  int32_t max_code_length, overflow;
} bfhip_png_stats;
typedef struct bfhip_png_frame {
  int64_t src_off;
  int64_t out_off, capacity;
  int64_t ws_off, res_off;
  int64_t n_bytes, band_bytes;
  int32_t width, height;
} bfhip_png_frame;
int bfhip_png_encode_supported(int width, int height, int band_rows);
int bfhip_png_encode_max_frames(void);
size_t bfhip_png_workspace_bytes(int64_t n_bytes, int64_t band_bytes, int with_filter);
size_t bfhip_png_capacity(int64_t n_bytes, int64_t band_bytes);
size_t bfhip_png_result_words(int64_t n_bytes, int64_t band_bytes);
int bfhip_png_encode(const bfhip_png_frame *frames_host, const bfhip_png_frame *frames_dev, int n_frames, const uint8_t *rgb_dev,
                     size_t rgb_bytes, void *workspace, size_t workspace_bytes, uint8_t *out_dev, size_t out_bytes,
                     uint32_t *result_dev, size_t result_words, void *stream);
int bfhip_png_deflate(const bfhip_png_frame *jobs_host, const bfhip_png_frame *jobs_dev, int n_jobs, const uint8_t *data_dev,
                      size_t data_bytes, void *workspace, size_t workspace_bytes, uint8_t *out_dev, size_t out_bytes,
                      uint32_t *result_dev, size_t result_words, void *stream);
int bfhip_png_filter_host(const uint8_t *rgb, int width, int height, uint8_t *out, size_t out_bytes);
int bfhip_png_huffman_lengths(const uint32_t *hist, int n_symbols, int max_len, uint8_t *lens);
int bfhip_png_deflate_host(const uint8_t *data, size_t n, size_t band_bytes, uint8_t *out, size_t capacity, uint32_t *bands,
                           size_t band_slots, bfhip_png_stats *stats);

/* ---------------------------------------------------------------------------------------
 * Points in rotated boxes, per box (csrc/points_in_boxes.hip): box_np_ops.points_in_rbbox (M3D/structures/ops/box_np_ops.py
 *   :354-377, 643-677) and the per-box gathers of the ground-truth database builder (tools/dataset_converters/
 *   create_gt_database.py:257, 296-297), as bevfusion_amd/box_ops.py: torch_points_in_boxes defines them.
 *   points: float32 [n, C], 4-byte aligned, 3 <= C <= 8, n < 2^31.  planes: float32 [K, 6, 4], per box six inward plane equations
 *     (n0, n1, n2, d) (bevfusion_amd/points_aug.py: paste_planes); K <= bfhip_points_in_boxes_max_boxes() = 256.  Row i is in box
 *     j unless ((x n0 + y n1) + z n2) + d >= 0 for one of its planes, every product and sum one float32 operation, never fused;
 *     a NaN sign therefore leaves the row inside.
 *   bfhip_points_in_boxes_count (two launches): counts int32 [K], the rows in each box.  member: NULL, or uint64 [n, ceil(K /
 *     64)], 8-byte aligned: bit j % 64 of word j / 64 of row i is set when row i is in box j (with NULL the words live in the
 *     workspace).  The workspace, 256-byte aligned, bfhip_points_in_boxes_workspace_bytes(n, K) bytes, also keeps the row
 *     offsets per (box, workgroup of bfhip_points_in_boxes_block() rows) and must reach the gather unchanged.
 *   bfhip_points_in_boxes_gather (one launch): out float32 [capacity, C]; the rows of box j, in ascending row index, at rows
 *     [start_j, start_j + counts_j), start the exclusive prefix sum of counts; a row in two boxes is written once for each.
 *     centers: NULL, or float32 [K, 3]: columns 0..2 of a row of box j are point - centers[j], one float32 subtraction each; the
 *     other columns are copied.  total: the sum of counts, which the caller has read; total < 2^31 and capacity >= total, or
 *     the call is rejected.  n, C, K, counts, member and the workspace as they were given to the count call.
 *   No allocation, no synchronisation, no atomics: every output is the same bytes on every run.
 * --------------------------------------------------------------------------------------- */
int bfhip_points_in_boxes_block(void);
int bfhip_points_in_boxes_max_boxes(void);
size_t bfhip_points_in_boxes_workspace_bytes(long long n, int K);
int bfhip_points_in_boxes_count(const float *points, long long n, int C, const float *planes, int K, int32_t *counts,
                                uint64_t *member, void *workspace, size_t workspace_bytes, void *stream);
int bfhip_points_in_boxes_gather(const float *points, long long n, int C, const float *centers, int K, const int32_t *counts,
                                 const uint64_t *member, long long total, float *out, long long capacity, const void *workspace,
                                 size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * nuScenes detection protocol (csrc/detection_eval.hip): greedy centre-distance matching, PR curves, AP and TP errors, as
 *   bevfusion_amd/evaluation.py: numpy_detection_eval defines them (the reference's NuScenesCustomMetric, projects/BEVFusion/
 *   evaluation/, runs the nuScenes devkit's accumulate / calc_ap / calc_tp on the host).  Two launches for any number of samples.
 *   Boxes are float32 rows of 9: x, y, z, dx, dy, dz, yaw, vx, vy.  pred_off / gt_off: int32 [n_samples + 1], the first row of
 *     each sample; at most bfhip_detection_eval_max_preds() = 512 predictions per sample.  pred_cls / gt_cls: int32, the index into
 *     the evaluated classes, or -1 (ignored); n_classes <= bfhip_detection_eval_max_classes() = 64; at most
 *     bfhip_detection_eval_max_gt() = 1024 GT boxes per (sample, class) -- further ones are not seen; the caller checks.
 *   bfhip_detection_match (one launch): per (sample, class, threshold) the class's predictions of the sample, by (score descending,
 *     row descending), each take the nearest not yet taken GT of the class in the sample (float64 sqrt(dx dx + dy dy) of the x, y
 *     centres; equal distance: the lower row) when its distance is < the threshold.  dist_ths: HOST float64 [n_ths], n_ths <=
 *     bfhip_detection_eval_max_thresholds() = 8.  match: int32 [n_ths, n_pred], the GT row or -1, written for every prediction with
 *     a class (the caller presets the others).  pred_err: float64 [n_pred, 5], the errors (translation, scale, orientation,
 *     velocity, attribute) of the match at threshold tp_index, NaN where unmatched.  Bit c of half_period_mask: class c's
 *     orientation error has period pi, not 2 pi; bit c of attr_empty_mask: its attribute error is NaN, not 0.
 *   bfhip_detection_curves (one launch): order: int32 [n_pred], the prediction rows by (class ascending, score descending, row
 *     descending), the ignored class last; cls_off: int32 [n_classes + 1], each class's first position in it.  npos: int32
 *     [n_classes], the GT boxes of each class.  levels: float64 [101], the recall levels.  Out: precision and confidence float64
 *     [n_classes, n_ths, 101], err_curves float64 [n_classes, 5, 101] (at tp_index), ap float64 [n_classes, n_ths], tp_err float64
 *     [n_classes, 5], max_recall_ind int32 [n_classes].  The workspace, 256-byte aligned, has
 *     bfhip_detection_curves_workspace_bytes(n_pred, n_ths) bytes.
 *   No allocation, no synchronisation, no atomics: the same bytes on every run.  All pointers but dist_ths are device pointers.
 * --------------------------------------------------------------------------------------- */
int bfhip_detection_eval_max_preds(void);
int bfhip_detection_eval_max_gt(void);
int bfhip_detection_eval_max_thresholds(void);
int bfhip_detection_eval_max_classes(void);
int bfhip_detection_match(const float *pred, const float *score, const int32_t *pred_cls, const int32_t *pred_off, long long n_pred,
                          const float *gt, const int32_t *gt_cls, const int32_t *gt_off, long long n_gt, int n_samples,
                          int n_classes, const double *dist_ths, int n_ths, int tp_index, uint64_t half_period_mask,
                          uint64_t attr_empty_mask, int32_t *match, double *pred_err, void *stream);
size_t bfhip_detection_curves_workspace_bytes(long long n_pred, int n_ths);
int bfhip_detection_curves(const float *score, const int32_t *order, const int32_t *cls_off, const int32_t *match,
                           const double *pred_err, long long n_pred, int n_classes, int n_ths, int tp_index, const int32_t *npos,
                           const double *levels, double min_precision, int first_level, uint64_t attr_empty_mask,
                           double *precision, double *confidence, double *err_curves, double *ap, double *tp_err,
                           int32_t *max_recall_ind, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Prediction visualiser (csrc/visualize.hip): 3D boxes drawn on the camera frames and tiled into a mosaic, and a bird's-eye
 *   canvas of the cloud with the box footprints, as bevfusion_amd/visualize.py defines them bit for bit (the reference's
 *   tools/visualize/visualize_bboxes_bevfusion.py and visualize_bev.py go through matplotlib).
 *   table: float32 [n_boxes, 8]: x, y, z (bottom centre), dx, dy, dz, cos(yaw), sin(yaw); a row with a non-finite entry is not
 *     drawn.  lidar2cam, cam2img: float32 [n_views, 3, 4], row-major.  thickness: 1/16 pixel, 1 .. bfhip_vis_max_thickness() =
 *     2048.  Frames and canvases have 1 .. bfhip_vis_max_dim() = 8192 pixels a side.
 *   bfhip_vis_camera_segments (one launch): one 32-byte record per (view, box, edge of the reference's 12) into the workspace:
 *     corners, camera transform, clip against z_cam = near, projection and perspective divide in float32 (every operation
 *     rounded once, none fused), ends in 1/16-pixel fixed point, clipped in int64 to a guard rectangle round the frame.  The
 *     pixel box of every record is kept a second time, as a dense 8-byte array behind the records, for the composite's cull.
 *   bfhip_vis_bev_segments (one launch): the same for the 4 footprint edges on a canvas with u = (x - x0) px_per_m,
 *     v = (y1 - y) px_per_m (y1 the upper y limit: row 0 is the top).
 *   bfhip_vis_composite (one launch): src uint8 [n_views, H, W, 3]; out uint8 [rows h, cols w, 3], h = H / scale, w = W / scale,
 *     scale 1 .. bfhip_vis_max_scale() = 4.  Cell i of the rows x cols grid shows view cell_view[i] (int32 [rows cols]; outside
 *     0 .. n_views - 1: black).  A source pixel whose centre lies within thickness / 2 of an edge (a capsule, exact in int64)
 *     takes colors[box] (int32 [n_boxes]: r | g << 8 | b << 16) of the highest such box index; an output pixel is the rounded
 *     mean (sum + scale^2 / 2) / scale^2 of its scale x scale source pixels.  n_boxes and edges (12 or 4) as given to the
 *     segment call that filled the workspace; src and out must not overlap.
 *   bfhip_vis_bev_points (one launch): points float32 [n, C], C >= 2; a point with 0 <= floor((x - x0) px_per_m) < W and
 *     0 <= floor((y - y0) px_per_m) < H (y0 the lower limit; float32, a NaN fails) stores a white point_size x point_size
 *     square round (col, H - 1 - that row), cut at the canvas, into canvas uint8 [H, W, 3], which the caller has zeroed.
 *   The workspace, 256-byte aligned, has bfhip_vis_workspace_bytes(n_views, n_boxes, edges) bytes (n_views = 1 for the BEV).
 *   No allocation, no synchronisation, no atomics: the same bytes on every run.  All pointers are device pointers.
 * --------------------------------------------------------------------------------------- */
int bfhip_vis_max_dim(void);
int bfhip_vis_max_thickness(void);
int bfhip_vis_max_scale(void);
size_t bfhip_vis_workspace_bytes(int n_views, int n_boxes, int edges);
int bfhip_vis_camera_segments(const float *table, int n_boxes, const float *lidar2cam, const float *cam2img, int n_views,
                              float near, int thickness, int H, int W, void *workspace, size_t workspace_bytes, void *stream);
int bfhip_vis_bev_segments(const float *table, int n_boxes, float x0, float y1, float px_per_m, int thickness, int H, int W,
                           void *workspace, size_t workspace_bytes, void *stream);
int bfhip_vis_composite(const uint8_t *src, int n_views, int H, int W, const void *workspace, size_t workspace_bytes, int n_boxes,
                        int edges, const int32_t *colors, const int32_t *cell_view, int rows, int cols, int scale, uint8_t *out,
                        void *stream);
int bfhip_vis_bev_points(const float *points, long long n, int C, float x0, float y0, float px_per_m, int point_size,
                         uint8_t *canvas, int H, int W, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BEVFUSION_HIP_H_ */
