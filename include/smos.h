/*
 * smos.h -- C ABI of libsmos_hip.so: the MI355X (gfx950) kernels of the StreamMOS
 * streaming-inference path.
 *
 * This is the drop-in boundary.  Plain pointers and sizes only; no torch types.  Every entry point
 *   - takes DEVICE pointers for tensors (HBM resident), HOST pointers for small shape/stride/scale
 *     vectors unless the comment says "device",
 *   - launches asynchronously on the hipStream_t passed as `stream` (never on the legacy default
 *     stream, unlike the reference's deep_point launches, point_deep_cuda_kernel.cu:153-160),
 *   - allocates nothing, synchronises nothing, keeps no global state (graph-capturable; the one exception is the test
 *     hook smos_debug_set_conv_grid_cap below),
 *   - returns SMOS_OK or an error code; smos_last_error() gives the thread-local message that the
 *     Python shims turn into RuntimeError (the reference raises c10::Error -> RuntimeError,
 *     point_deep_cuda.cpp:11-13).
 *
 * Each function names the reference interface it replaces (paths relative to the reference root).
 */
#ifndef SMOS_H_
#define SMOS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMOS_ABI_VERSION 4

enum smos_status {
  SMOS_OK = 0,
  SMOS_ERR_ARG = 1,          /* null pointer, bad size, unsupported rank */
  SMOS_ERR_UNSUPPORTED = 2,  /* dtype / shape outside what this build implements */
  SMOS_ERR_LAUNCH = 3        /* the HIP runtime reported a launch error */
};

enum smos_dtype { SMOS_F32 = 0, SMOS_F16 = 1, SMOS_F64 = 2 };

typedef void* smos_stream_t; /* hipStream_t */

int smos_abi_version(void);
const char* smos_last_error(void);
/* Test hook (process-wide, not part of the data path; the one piece of state the library keeps): caps the grid of the
 * persistent convolution kernels (smos_conv_cl / _rows_cl / _wino_cl / _wino1d_cl / _bf16_cl), of smos_stem_gemm, of
 * smos_pointnet_scatter / _rows, of smos_gather_scatter_cl, of the three smos_gather_scatter_train_* entries, of smos_point_head / _gather, of smos_tta_argmax and of the emit, copy, start and sum
 * kernels of smos_bilinear_gather_bwd_det / smos_msda_bwd_det and of smos_train_prep_build / _draws and smos_copy_paste_* at `blocks`, 0 = no cap.  It makes one block walk several work items -- the
 * item-boundary code paths, a wave's whole-tile / head / tail units of the stem, the scatter's software pipeline -- on shapes
 * small enough to check against float64.  The results do not depend on it. */
int smos_debug_set_conv_grid_cap(int32_t blocks);

/* --------------------------------------------------------------------------------------------
 * Point -> grid max-pool scatter.
 * Replaces point_deep.cuda_kernel.voxel_maxpooling_forward (deep_point/src/point_deep_cuda.cpp:20-37,
 * kernels deep_point/src/point_deep_cuda_kernel.cu:24-99) -- three launches, an int64 index scratch
 * and CAS-loop float atomics there; one fused launch with native integer atomic max here.
 *
 *   feat   [BS, C, N]      element strides feat_stride[3] (reference layout: {C*N, N, 1})
 *   ind    [BS, N, D]      contiguous, same dtype as feat; D <= 4
 *   out    [BS, C, D1..Dn] element strides out_stride[2+D]; MUST be zero-filled by the caller
 *                          (the reference's caller does so, deep_point/__init__.py:26)
 *   voxel_max_idx [BS, N]  int64, pre-filled with -1 by the caller, or NULL to skip it; receives
 *                          bs*out_stride[0] + sum_d cell_d*out_stride[2+d] for kept points
 *   out_size[D], scale[D]  host
 *   flag_ws                device int32 scratch (4 bytes); used to detect negative features, which take
 *                          a slower exact path (see DESIGN.md "VoxelMaxPool")
 * cell_d = (int64)((float)ind_d * scale_d) truncated toward zero; a point is kept iff every
 * 0 <= cell_d < out_size[d].  Occupied cell = max over its members; empty cell stays 0.
 */
int smos_voxel_maxpool_fwd(const void* feat, const int64_t* feat_stride, const void* ind, void* out,
                           const int64_t* out_stride, int64_t* voxel_max_idx, int64_t BS, int64_t C,
                           int64_t N, int32_t D, const int64_t* out_size, const float* scale,
                           int32_t dtype, int32_t* flag_ws, smos_stream_t stream);

/* Replaces point_deep.cuda_kernel.voxel_maxpooling_backward (point_deep_cuda.cpp:39-57, kernel
 * point_deep_cuda_kernel.cu:109-132): grad_feat[b,c,n] = grad_out[cell] iff out[cell] == feat[b,c,n].
 * grad_feat must be zero-filled by the caller; grad_out uses out's strides. */
int smos_voxel_maxpool_bwd(const void* feat, const int64_t* feat_stride, const void* ind, const void* out,
                           const void* grad_out, const int64_t* out_stride, void* grad_feat, int64_t BS,
                           int64_t C, int64_t N, int32_t D, const int64_t* out_size, const float* scale,
                           int32_t dtype, smos_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Grid -> point bilinear gather.
 * Replaces networks/backbone.py:453-475 (BilinearSample = F.grid_sample, bilinear, zeros padding,
 * align_corners=True) including its float32 normalise / un-normalise round trip.
 *   grid  [B, C, H, W]  element strides grid_stride[4]  (NCHW or NHWC both fine)
 *   coord [B, N, K]     contiguous, K >= 2; row = coord[...,0]*scale[0], col = coord[...,1]*scale[1]
 *   out   [B, C, N]     element strides out_stride[3]
 */
int smos_bilinear_gather_fwd(const float* grid, const int64_t* grid_stride, const float* coord, int32_t K,
                             float* out, const int64_t* out_stride, int64_t B, int64_t C, int64_t H,
                             int64_t W, int64_t N, const float* scale, smos_stream_t stream);

/* Its gradient with respect to grid: grad_grid[b, c, y, x] = sum over the points and their four taps of
 * w_tap * grad_out[b, c, n], with the taps, weights and range rules of the forward (a tap outside the map, a NaN
 * coordinate or a padding row adds nothing).  There is no gradient with respect to coord.  Float32 only.
 *   grad_out  [B, C, N]     element strides grad_out_stride[3]   (channel-major or point-major)
 *   coord     [B, N, K]     contiguous, as in the forward
 *   grad_grid [B, C, H, W]  element strides grad_grid_stride[4]; may arrive uninitialised: the call zeroes it itself.
 * A destination with channel stride 1 (channels-last) and C >= 8 is added to in whole row segments; any other takes
 * one 4-byte atomic per (point, tap, channel).  The sums depend on the arrival order of the atomics.
 */
int smos_bilinear_gather_bwd(const float* grad_out, const int64_t* grad_out_stride, const float* coord, int32_t K,
                             float* grad_grid, const int64_t* grad_grid_stride, int64_t B, int64_t C, int64_t H,
                             int64_t W, int64_t N, const float* scale, smos_stream_t stream);

/* The same gradient summed in a FIXED order, without atomics on the data (csrc/segsum.hip): every (point, tap) pair is
 * written out with its destination row (b * H + y) * W + x as a 32-bit key, one stable radix sort brings the pairs of a
 * row together in ascending pair index (b * N + n) * 4 + k, k = nw, ne, sw, se, and a row is then summed as a defined
 * float32 number: term j = w_j * grad_out_j (one rounding); chunks of smos_segsum_chunk() consecutive terms are summed
 * left to right from their first term; the chunk partials are added left to right (round-to-nearest additions, no FMA).
 * A pixel no pair reaches is exactly 0.  Two calls give the same bits, on any grid and any device.
 * Arguments as smos_bilinear_gather_bwd (any strides on both tensors; grad_grid may arrive uninitialised), then
 *   work   smos_bilinear_gather_bwd_det_work_bytes(B, C, H, W, N) bytes of device scratch, 256-byte aligned, free again
 *          when the call's launches have run.  The query returns 0 for an empty problem (no scratch is touched) and -1
 *          where the 32-bit keys do not reach: it needs B * N < 2^29 and B * H * W < 2^31 - 1.
 * Float32 only. */
int32_t smos_segsum_chunk(void);
int64_t smos_bilinear_gather_bwd_det_work_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int64_t N);
int smos_bilinear_gather_bwd_det(const float* grad_out, const int64_t* grad_out_stride, const float* coord, int32_t K,
                                 float* grad_grid, const int64_t* grad_grid_stride, int64_t B, int64_t C, int64_t H,
                                 int64_t W, int64_t N, const float* scale, void* work, int64_t work_bytes,
                                 smos_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Training form of a cross-view transfer: smos_bilinear_gather_fwd followed by smos_voxel_maxpool_fwd (D = 2) without the
 * [B, C, N] tensor between them, and the gradient of the pair with respect to grid (csrc/gather_scatter_train.hip).  Float32.
 *   grid    [B, C, Hg, Wg]  element strides grid_stride[4]
 *   gcoord  [B, N, Kg]      contiguous, Kg >= 2: the gather's coordinates, scaled by gscale[2] as in smos_bilinear_gather_fwd
 *   scoord  [B, N, Ks]      contiguous, Ks >= 2: the scatter's, cell = trunc(coord * sscale[2]) as in smos_voxel_maxpool_fwd
 *   out     [B, C, Ho, Wo]  element strides out_stride[4]; MUST be zero-filled by the caller
 *   pts     [B, C, N]       element strides pts_stride[3], or NULL: the gathered values, the bits of smos_bilinear_gather_fwd
 *   flag_ws                 device int32 scratch (4 bytes), as in smos_voxel_maxpool_fwd
 * out has the bits of the two calls it stands for, for every finite grid: a negative value takes the same exact path
 * (two more launches that return at once otherwise). */
int smos_gather_scatter_train_fwd(const float* grid, const int64_t* grid_stride, const float* gcoord, int32_t Kg,
                                  const float* gscale, const float* scoord, int32_t Ks, const float* sscale, float* out,
                                  const int64_t* out_stride, float* pts, const int64_t* pts_stride, int64_t B, int64_t C,
                                  int64_t Hg, int64_t Wg, int64_t N, int64_t Ho, int64_t Wo, int32_t* flag_ws,
                                  smos_stream_t stream);

/* Its backward.  The gradient of the point values is
 *   x[b, c, n] = grad_out[b, c, cell(n)] if the point is kept and its gathered value (recomputed, the forward's bits) equals
 *                out[b, c, cell(n)], else 0 -- every tie wins, a 0 in a cell whose maximum is 0 wins, as in
 *                smos_voxel_maxpool_bwd -- plus grad_pts[b, c, n] (one float32 addition) where grad_pts is not NULL,
 * and grad_grid is smos_bilinear_gather_bwd of x: the same taps, weights, wave tiles and row atomics, except that a run
 * of points whose sum is exactly 0 issues no atomic.  The sums depend on the arrival order of the atomics.
 *   out       [B, C, Ho, Wo]  the forward's result, element strides out_stride[4]
 *   grad_out  [B, C, Ho, Wo]  element strides grad_out_stride[4] (e.g. a channel slice of a wider tensor)
 *   grad_pts  [B, C, N]       element strides grad_pts_stride[3], or NULL
 *   grad_grid [B, C, Hg, Wg]  element strides grad_grid_stride[4]; may arrive uninitialised: the call zeroes it itself.
 *                             Channel stride 1 and C >= 8: whole row segments; anything else: 4-byte atomics. */
int smos_gather_scatter_train_bwd(const float* grid, const int64_t* grid_stride, const float* gcoord, int32_t Kg,
                                  const float* gscale, const float* scoord, int32_t Ks, const float* sscale, const float* out,
                                  const int64_t* out_stride, const float* grad_out, const int64_t* grad_out_stride,
                                  const float* grad_pts, const int64_t* grad_pts_stride, float* grad_grid,
                                  const int64_t* grad_grid_stride, int64_t B, int64_t C, int64_t Hg, int64_t Wg, int64_t N,
                                  int64_t Ho, int64_t Wo, smos_stream_t stream);

/* x itself, [B, C, N] at element strides x_stride[3], every element written and nothing else: the input of
 * smos_bilinear_gather_bwd_det for a fixed-order backward.  Other arguments as smos_gather_scatter_train_bwd. */
int smos_gather_scatter_train_point_grad(const float* grid, const int64_t* grid_stride, const float* gcoord, int32_t Kg,
                                         const float* gscale, const float* scoord, int32_t Ks, const float* sscale,
                                         const float* out, const int64_t* out_stride, const float* grad_out,
                                         const int64_t* grad_out_stride, const float* grad_pts, const int64_t* grad_pts_stride,
                                         float* x, const int64_t* x_stride, int64_t B, int64_t C, int64_t Hg, int64_t Wg,
                                         int64_t N, int64_t Ho, int64_t Wo, smos_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Training loss: OHEM cross-entropy + lovasz_weight * Lovasz-softmax (classes = present, one image), one scalar.
 * Replaces utils/criterion.py:10-28 and utils/lovasz_losses.py:147-222 as AttNet calls them (`ce + 3 * lovasz`).
 * See csrc/seg_loss.hip.  Nothing is read back: the all-ignored case yields exactly 0 on the device.
 *   pred    [B, C, P]   float32, element strides pred_stride[3]; C = 2 or 3
 *   target  [B, P]      int64, contiguous; ignore_index, and any label outside [0, C), takes part as an ignored position
 *   k                   size of the OHEM top-k, max(int(top_ratio * B * P), 1), from the caller
 *   coef    [C + 1, B*P] float32 out: rows 0..C-1 the Lovasz coefficient d of each position in class c's sorted order
 *                       (0 for an ignored position or an absent class), row C the top-k flag (1.0 / 0.0)
 *   loss    [1]         float32 out
 *   stats   [2]         float32 out: 1 / number of present classes (0 when there is none), that number
 *   work                smos_seg_loss_work_bytes(B*P, C) bytes of device scratch (0 from the query: sizes not supported),
 *                       free again when the call's launches have run
 * smos_seg_loss_fwd enqueues every launch of the forward (prep, one radix sort over C + 1 segments, tile counts, tile
 * scan, apply, finish); smos_seg_loss_bwd is one launch that recomputes the softmax and writes
 *   grad[b, j, p] = grad_out * [ (1/n + top_weight/k * top) * (p_j - [j == y])
 *                                + lovasz_weight / present * sum_c s_c * coef[c] * p_c * ([c == j] - p_j) ],   s_c = -1 if y == c else 1
 * (0 at an ignored position) through grad_stride[3]; grad_out is a DEVICE scalar.  Ties between sort keys are broken by
 * position (a stable sort), sums are float64 partials added in a fixed order: two runs give the same bits.
 * smos_seg_loss_tile(): elements per block of the scan kernels (tests place their edge cases around it). */
int32_t smos_seg_loss_tile(void);
int64_t smos_seg_loss_work_bytes(int64_t n, int32_t C);
int smos_seg_loss_fwd(const float* pred, const int64_t* pred_stride, const int64_t* target, int64_t B, int32_t C,
                      int64_t P, int64_t k, float top_weight, float lovasz_weight, int64_t ignore_index, float* coef,
                      float* loss, float* stats, void* work, int64_t work_bytes, smos_stream_t stream);
int smos_seg_loss_bwd(const float* pred, const int64_t* pred_stride, const int64_t* target, const float* coef,
                      const float* stats, const float* grad_out, int64_t B, int32_t C, int64_t P, int64_t k,
                      float top_weight, float lovasz_weight, int64_t ignore_index, float* grad,
                      const int64_t* grad_stride, smos_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Multi-scale deformable attention sampler, forward.
 * Replaces MultiScaleDeformableAttention.ms_deform_attn_forward (deformattn/src/vision.cpp:13-16 ->
 * deformattn/src/cuda/ms_deform_attn_cuda.cu:20-80, kernel ms_deform_im2col_cuda.cuh:237-299).
 *   value [N, S, M, D]; spatial_shapes [L,2] int64 DEVICE; level_start_index [L] int64 DEVICE
 *   sampling_loc [N, Lq, M, L, P, 2]; attn_weight [N, Lq, M, L, P]; out [N, Lq, M*D]  (all contiguous)
 * dtype: SMOS_F32 or SMOS_F64 (the reference dispatches float/double only, ms_deform_attn_cuda.cu:64).
 */
int smos_msda_fwd(const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                  const void* sampling_loc, const void* attn_weight, void* out, int64_t N, int64_t S,
                  int64_t M, int64_t D, int64_t L, int64_t Lq, int64_t P, int32_t dtype,
                  smos_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * TTA reduce: softmax over classes, mean over the B test-time-augmentation variants, argmax.
 * Replaces val_StreamMOS.py:97-98,113.  pred [B, K, N] float32 contiguous (K <= 8) -> labels [N] uint8,
 * prob [N, K] float32 (optional, may be NULL).
 */
int smos_tta_argmax(const float* pred, int64_t B, int64_t K, int64_t N, uint8_t* labels, float* prob,
                    smos_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Voxel voting (voxel_voting.py:38-91,214-242).  The vote table is a dense array of
 * SMOS_VOTE_CELLS packed 64-bit words (three 21-bit class counters per voxel) that stays in HBM;
 * the caller zero-fills it per frame (smos_vote_clear), accumulates the 8 history frames and the
 * current frame, then resolves the current frame's labels.
 *
 *   pts [n, pt_stride] float32 rows (x, y, z, ...) in the frame's OWN sensor coordinates
 *   labels [n] uint8 in {0,1,2}
 *   pose_diff: host, 16 doubles row-major = inv(P_cur) * P_frame, or NULL for the current frame;
 *              applied in float64 then rounded to float32 (datasets/utils.py:116-126)
 *   recip_quantize: 0 = float32 true division (numpy / torch-CPU behaviour, the pinned one),
 *                   1 = multiply by the float32 reciprocal of the cell size (what torch's CUDA div by a
 *                       Python scalar does in voxel_voting.py:86-88 when run on a GPU)
 * Crop (utils/transforms.py:151-161) and Quantize (voxel_voting.py:77-91) are fused in.
 */
#define SMOS_VOTE_NX 512
#define SMOS_VOTE_NY 512
#define SMOS_VOTE_NZ 30
#define SMOS_VOTE_CELLS (512LL * 512LL * 30LL)

int smos_vote_clear(uint64_t* table, smos_stream_t stream);
int smos_vote_accumulate(const float* pts, int64_t n, int64_t pt_stride, const uint8_t* labels,
                         const double* pose_diff, int32_t recip_quantize, uint64_t* table,
                         smos_stream_t stream);
/* The same accumulation for a whole voting window in one launch (voxel_voting.py:214-238 loops over the 8 history frames
 * and the current one): host arrays of `count` device pointers / sizes; pose_diff[f] = 16 host doubles or NULL (identity,
 * the current frame).  Integer adds commute, so the table equals the one `count` single-frame calls produce. */
int smos_vote_accumulate_frames(int32_t count, const float* const* pts, const int64_t* n, const int64_t* pt_stride,
                                const uint8_t* const* labels, const double* const* pose_diff, int32_t recip_quantize,
                                uint64_t* table, smos_stream_t stream);
/* out_labels[i] = argmax of the voxel of point i (ties -> lowest class) if the point survives the crop,
 * else labels[i]; lut (device, 256 int32 entries, e.g. {0:0,1:9,2:251}) is applied when non-NULL. */
int smos_vote_resolve(const float* pts, int64_t n, int64_t pt_stride, const uint8_t* labels,
                      int32_t recip_quantize, const uint64_t* table, const int32_t* lut,
                      int32_t* out_labels, smos_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Instance-level voting (voxel_instance_voting.py:144-193): the two heavy steps of cluster().
 *
 * smos_dbscan: sklearn.cluster.DBSCAN(eps, min_samples).fit_predict(pts[:, :3]) (:150-153) on the device.
 *   labels[i] (device, int32[n]) = NAME of point i's cluster = index of the cluster's lowest-index core point, or -1 for
 *   noise.  scikit-learn numbers clusters 0,1,2.. in the order of exactly that index, so ranking the distinct names
 *   gives its labels; a border point gets the smallest name among the clusters it touches (the one scikit-learn expands
 *   first).  Distances: float32 coordinates widened to float64, d2 = dx*dx + dy*dy + dz*dz, d2 <= eps*eps.
 *   work: device scratch of smos_dbscan_work_bytes(n) bytes, 256-byte aligned (x-sorted copy of the points, the
 *   permutation, labels, hipCUB sort space).  The call synchronises `stream` once per 4 propagation sweeps (it reads
 *   back a "changed" flag); max_sweeps bounds the loop.
 * smos_box_vote: counts[k*3 + c] (device, uint32, caller zero-fills) += number of points of class c in {1,2} of one
 *   frame that survive the voting crop (utils/transforms.py:151-161) and lie inside the closed axis-aligned box
 *   boxes[k] = (lo_x, lo_y, lo_z, hi_x, hi_y, hi_z) float32 -- in_hull() of :62-76 for a box.  pose_diff as in
 *   smos_vote_accumulate (NULL for the current frame).  At most 2048 boxes per call.
 */
int64_t smos_dbscan_work_bytes(int64_t n);   /* 0 for n == 0, -1 on failure */
int smos_dbscan(const float* pts, int64_t n, int64_t pt_stride, double eps, int32_t min_samples, int32_t* labels,
                void* work, int64_t work_bytes, int32_t max_sweeps, smos_stream_t stream);
int smos_box_vote(const float* pts, int64_t n, int64_t pt_stride, const uint8_t* labels, const double* pose_diff,
                  const float* boxes, int32_t K, uint32_t* counts, smos_stream_t stream);

/* The same instance vote with nothing read back: a fixed sequence of launches whose grids depend on n alone.  The
 * foreground count and the cluster count K exist only in device memory.  None of these calls synchronises.
 *
 * smos_instance_cluster: DBSCAN(eps, min_samples) of the points of the WHOLE scan pts[n] whose bf[i] (device, uint8[n])
 *   is 2, then InstanceVoter.cluster_boxes on the device.  A point with bf != 2 is nobody's neighbour.
 *   names[i] (device, int32[n]): scan index of the lowest core point of point i's cluster; -1 for noise and for every
 *     non-foreground point (smos_dbscan's names of the compacted foreground, mapped back to scan indices).
 *   Clusters of more than min_points points are kept: boxes[slot] (device, float32[max_boxes][6]) = (lo_x, lo_y, z0,
 *     hi_x, hi_y, z1) with lifted = lo_z + floor_lift in float32, z0 / z1 = min / max(lifted, hi_z); a box with hi_z == lo_z
 *     or any hi == lo gets lo = +inf (it contains nothing).  slot_of[name] (device, int32[n]) = the cluster's slot, -1
 *     for every other index.  *k_dev (device int32) = number of slots used; slot order is unspecified.  If more than
 *     max_boxes (1..2048) clusters are kept, bit 0 of *status (device int32, written by every call) is set, *k_dev =
 *     max_boxes and the clusters beyond keep slot -1.
 *   work: smos_instance_work_bytes(n) bytes of device scratch, 256-byte aligned; a larger one does as well, and nothing
 *     in it has to survive between calls.  n == 0: *k_dev = *status = 0, nothing else is touched.
 * smos_box_vote_dev: smos_box_vote for the `count` frames of a window in one launch, on the first *k_dev boxes:
 *   host arrays of `count` device pointers / sizes, pose_diff[f] = 16 host doubles or NULL (identity, the current frame).
 *   counts (device, uint32[max_boxes][3], caller zero-fills).  max_boxes (1..2048) sizes the kernel's LDS.
 * smos_instance_apply: labels[i] (device int32[n], in place) = 2 if 2 * counts[s][2] > counts[s][1] else 1 for every
 *   point whose names[i] has a slot s = slot_of[names[i]] < *k_dev (voxel_instance_voting.py:178-183); others are kept.
 *   max_boxes = rows of counts.
 */
int64_t smos_instance_work_bytes(int64_t n);   /* 0 for n <= 0 (or n >= 2^31); needs no device */
int smos_instance_cluster(const float* pts, int64_t n, int64_t pt_stride, const uint8_t* bf, double eps,
                          int32_t min_samples, int32_t min_points, float floor_lift, int32_t max_boxes, int32_t* names,
                          float* boxes, int32_t* slot_of, int32_t* k_dev, int32_t* status, void* work, int64_t work_bytes,
                          smos_stream_t stream);
int smos_box_vote_dev(int32_t count, const float* const* pts, const int64_t* n, const int64_t* pt_stride,
                      const uint8_t* const* labels, const double* const* pose_diff, const float* boxes,
                      const int32_t* k_dev, int32_t max_boxes, uint32_t* counts, smos_stream_t stream);
int smos_instance_apply(const int32_t* names, const int32_t* slot_of, const uint32_t* counts, const int32_t* k_dev,
                        int32_t max_boxes, int32_t* labels, int64_t n, smos_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Fused point-side kernels of the inference engine (csrc/point_fused.hip).  Scatter targets are
 * channels-last and zero-filled by the caller; features are assumed >= 0 (post-ReLU), as on every call
 * site of the model.
 */
/* point_pre + input scatter (models/StreamMOS.py:101-103): per-point MLP cin->cmid->cout (BatchNorm folded
 * into w/b, ReLU after both layers; only 7->64->64 is built) on xyzi [B*T, cin, N], max-scattered into
 * bev [B, H, W, T*cout] at cell (int(coord0), int(coord1)), coord [B*T, N, K].  pts_out (optional): the
 * features of the t == 0 scan as rows pts_out[b*po_b + n*po_n + c]. */
int smos_pointnet_scatter(const float* xyzi, const float* coord, int32_t K, const float* w1, const float* b1,
                          const float* w2, const float* b2, float* bev, float* pts_out, int64_t po_b, int64_t po_n,
                          int64_t B, int64_t T, int64_t N, int64_t H, int64_t W, int32_t cin, int32_t cmid,
                          int32_t cout, smos_stream_t stream);
/* Sparse DownSample2D on the input grid (networks/backbone.py:136-159 as used by header_bev[0],
 * multi_view_encoder.py:340-347): see csrc/stem.hip.  All buffers are device memory owned by the caller; no call reads
 * anything back to the host (row counts stay in `meta`), so the sequence is graph-capturable.
 *   smos_stem_mark    flags (int32 [4, B, H/2, W/2]; index = parity class (y&1)*2+(x&1), sample, y>>1, x>>1) <- 1 for
 *                     every cell a point of coord [B, T, N, K] falls into.  flags must be all zero on entry (zero it once;
 *                     smos_stem_scan leaves it all zero again).  Also re-arms scan_state (uint64
 *                     [smos_stem_scan_state_words(B*H*W)]) for the smos_stem_scan call that follows on the stream.
 *   smos_stem_scan    one pass over the flags: row_cell[row] <- natural cell id (b*H + y)*W + x; row_of [B,H,W] <- row id
 *                     or -1; meta (12 x int32): [4..7] first row of each class, [8..11] one past its last row (meta[11] =
 *                     number of rows); flags cleared; if rows != NULL, rows[0 .. meta[11]) (row_floats floats each: the
 *                     compact table of smos_pointnet_scatter_rows) zero-filled.
 *   smos_stem_gemm    y4[cls] (device, capacity B*(H/2)*(W/2) rows of (taps+1)*Cout floats; taps = 1,2,2,4) <-
 *                     occupied rows of bev [B*H*W, Cin] times the class weights; with row_cell == NULL, bev is the
 *                     compact row table itself (row r of the table = global row r).  wprep4[cls]: weights of the class in
 *                     MFMA operand order [(taps+1)][Cin/2][64]: entry (mt, s, lane) = W[mt*32 + (lane & 31)][(lane >> 5) *
 *                     (Cin/2) + s], where W stacks the class's 3x3 taps (ky-major over the kernel rows / columns that
 *                     reach an output pixel) and the 1x1 pool-branch weights last.  Built for Cin = 192, Cout = 32.
 *   smos_stem_epilogue out[b,ho,wo,c] <- relu(sum_taps Y[cell][slot][c] + max_window(occupied ? Y[cell][q][c] : 0) +
 *                     bias[c]); out is channels-last [B, H/2, W/2, *] with row pitch out_pitch; C must be 32.
 * y4 / wprep4 are HOST arrays of 4 device pointers. */
int64_t smos_stem_scan_state_words(int64_t cells);
int smos_stem_mark(const float* coord, int32_t K, int64_t B, int64_t T, int64_t N, int64_t H, int64_t W, int32_t* flags,
                   uint64_t* scan_state, smos_stream_t stream);
int smos_stem_scan(int32_t* flags, int64_t B, int64_t H, int64_t W, uint64_t* scan_state, int32_t* row_cell, int32_t* row_of,
                   int32_t* meta, float* rows, int64_t row_floats, smos_stream_t stream);
int smos_stem_gemm(const float* bev, const int32_t* row_cell, const int32_t* meta, const float* const* wprep4, float* const* y4,
                   int64_t Cin, int64_t Cout, smos_stream_t stream);
int smos_stem_epilogue(const float* const* y4, const int32_t* meta, const int32_t* row_of, const float* bias, float* out,
                       int64_t out_pitch, int64_t B, int64_t H, int64_t W, int64_t C, smos_stream_t stream);
/* The sampler of smos_msda_fwd fed by the raw query projection of a DeformAttnLayer (multi_view_encoder.py:300-316):
 * qp [N, H*W, M*P*2 + M*P] = per token the sampling offsets (x, y per head and point) followed by the attention logits;
 * single level H x W, queries on the same H x W lattice with the cell centres as reference points.  Folds softmax over the
 * P logits, off / (W, H) and + reference point into the kernel.  value [N, H*W, M, D], out [N, H*W, M*D]; D == 32, P <= 8. */
int smos_msda_fwd_qp(const float* value, const float* qp, float* out, int64_t N, int64_t H, int64_t W, int64_t M, int64_t D,
                     int64_t P, smos_stream_t stream);

/* Temporal fusion on the matrix cores (csrc/tfusion.hip; networks/multi_view_encoder.py:285-321 DeformAttnLayer,
 * deformattn/modules/ms_deform_attn.py:94-115 MSDeformAttn's projections).  d_model = 128.
 * smos_tfusion_project: up to eight token-wise Linear jobs y = W x (+ b) in one launch -- the projections of a frame that depend
 *   on no previous layer (value_proj of every layer, the first layer's [sampling_offsets | attention_weights]) and the
 *   decoder's tap products (the [B Hs Ws, 128] x [128, 9 * 128] GEMMs in front of smos_upconv_xy).  Host arrays of n_jobs
 *   entries; x[j] [tokens[j], *] rows of pitch x_pitch[j] floats (>= 128); wstream[j] = the weights as 16 x 16 blocks in MFMA
 *   operand order (streammos_amd.ops.tfusion_pack_linear: cout rounded up to a multiple of 64, zero padded); bias[j] [cout]
 *   or NULL; out[j] [tokens[j], *] rows of pitch out_pitch[j] >= cout (a job may fill a column range of a wider matrix); cout a
 *   multiple of 4, <= 2048.
 * smos_tfusion_layer: everything of one layer behind its sampler in one launch:
 *   q1 = norm1(query + output_proj(sampled)); out = norm2(q1 + linear2(relu(linear1(q1)))); and, if qp_next != NULL,
 *   qp_next = W_q out + b_q -- the NEXT layer's offset / logit projection (nq <= 64 channels), so that the following
 *   smos_msda_fwd_qp can start at once.  wstream / params = streammos_amd.ops.TfusionLayer (sizes:
 *   smos_tfusion_layer_stream_floats / _param_floats); ffn a multiple of 32. */
int smos_tfusion_project(int32_t n_jobs, const float* const* x, const int64_t* x_pitch, const float* const* wstream,
                         const float* const* bias, float* const* out, const int64_t* out_pitch, const int64_t* cout,
                         const int64_t* tokens, smos_stream_t stream);
int64_t smos_tfusion_layer_param_floats(int64_t ffn);
int64_t smos_tfusion_layer_stream_floats(int64_t ffn, int32_t has_next);
int smos_tfusion_layer(const float* sampled, const float* query, int64_t q_pitch, const float* wstream, const float* params,
                       float* out, int64_t o_pitch, float* qp_next, int64_t nq, int64_t tokens, int64_t ffn, float eps1,
                       float eps2, smos_stream_t stream);

/* The decoder's tap products on the bf16 matrix pipe at fp32 accuracy (csrc/tap_bf16x3.hip): out[j] = x[j] W[j]^T for up to
 * eight jobs in one launch, every fp32 operand split exactly into three bf16 limbs (hi = bf16(v), mid = bf16(v - hi), lo =
 * bf16(v - hi - mid), round-to-nearest-even) and the six leading limb products summed in fp32 in a fixed order.  The job
 * contract of smos_tfusion_project without a bias: x[j] [tokens[j], *] rows of 128 channels, pitch x_pitch[j] floats;
 * wlimbs[j] = streammos_amd.ops.tap_limbs_pack(W[j]): the limbs of W as bf16 MFMA fragments in the kernel's stream order
 * [tile of 32 outputs][k step 0..7][lo, mid, hi][lane 0..63][8] -- lane (r = lane & 31, h = lane >> 5), element j holds
 * W_limb[32 tile + r][16 step + 8 h + j], cout rounded up to a multiple of 32 with zero rows; out[j] [tokens[j], *] rows of pitch out_pitch[j] >= cout[j] (a job may fill a column range of a wider matrix);
 * cout a multiple of 4, <= 2048; 0 < tokens < 2^22; operands below 2 GiB.  Inputs: finite, and large enough for the low limb
 * to stay a normal number (|v| >~ 2^-110, or 0); a non-finite input gives a non-finite output (NaN where fp32 gives Inf).
 * Deterministic; a column range of W gives the bits of the whole matrix. */
int smos_tap_products_bf16x3(int32_t n_jobs, const float* const* x, const int64_t* x_pitch, const void* const* wlimbs,
                             float* const* out, const int64_t* out_pitch, const int64_t* cout, const int64_t* tokens,
                             smos_stream_t stream);

/* out = LayerNorm(x + res) over rows of C floats (res may be NULL): the residual + norm steps of a DeformAttnLayer
 * (multi_view_encoder.py:314-320).  C in {64, 128, 256, 512}; biased variance, eps inside the square root (torch). */
int smos_add_layer_norm(const float* x, const float* res, const float* gamma, const float* beta, float* out, int64_t rows,
                        int64_t C, float eps, smos_stream_t stream);

/* General channels-last convolution on the matrix cores with the epilogue fused (csrc/conv_igemm.hip):
 *   out = act(conv_{KH x KW, stride, pad}(x) + bias [+ res]);  act 0 none, 1 ReLU, 2 LeakyReLU(0.01).
 * Replaces every conv2d -> BatchNorm (folded by the caller) -> ReLU / LeakyReLU (-> + residual -> ReLU) chain of
 * networks/backbone.py:9-34,136-159 and networks/multi_view_encoder.py:460-497 (cuDNN in the reference).
 * x [B, H, W, *], res / out [B, Ho, Wo, *]: row pitches in floats (multiples of 4; channel slices of wider buffers are
 * fine), 16-byte aligned, each tensor < 2 GiB.  Cin % 32 == 0, Cout % (32 * mt) == 0, mt in {1, 2, 4} = 32-channel output
 * blocks per wave (a tuning knob), KH, KW <= 7, stride 1 or 2.  bias / res may be NULL.
 * The window has to fit the padded image (KH <= H + 2 pad_h, KW <= W + 2 pad_w); act(NaN) is NaN, as in the reference.
 * wprep: Cout * Cin * KH * KW floats in MFMA operand order for the chosen mt; with stage = (ky * KW + kx) * (Cin / 32) + cc:
 *   wprep[((((ct * n_stage + stage) * 4 + i4) * mt + m) * 64 + lane) * 4 + c]
 *       = w[ct * 32 * mt + m * 32 + (lane & 31)][cc * 32 + 8 * i4 + 4 * (lane >> 5) + c][ky][kx].
 * chan_sums (may be NULL; needs res == NULL): [B][chunks][Cout] with chunks = smos_conv_cl_sum_chunks(Ho, Wo); entry
 *   (b, chunk, c) = sum of out[b, y, x, c] over one output row segment of 32 pixels (chunk = ((y / 4) * ceil(Wo / 32) +
 *   x / 32) * 4 + y % 4; segments outside the image hold 0): the global-average-pool input of a ChannelAtt block
 *   (networks/backbone.py:57-73) without another pass over the map.  Summation order is fixed (run-to-run identical). */
int64_t smos_conv_cl_sum_chunks(int64_t Ho, int64_t Wo);
/* smos_conv_cl for stride 1, "same" padding (pad = K / 2), KW in {3, 5, 7}, odd KH <= 7, mt in {1, 2} (32 / 64 output
 * channels per block), with the input rows staged through LDS once per kernel row and 32-channel chunk
 * (csrc/conv_rows.hip): one coalesced request per row instead of one per tap.  Same operands and epilogue; the weight block
 * is ordered (ky, cin chunk, kx) inside a tile:
 *   wprep[((((ct * KH + ky) * (Cin / 32) + cc) * KW + kx) * 4 + i4) * mt + m][lane][c]
 *       = w[ct * 32 * mt + m * 32 + (lane & 31)][cc * 32 + 8 * i4 + 4 * (lane >> 5) + c][ky][kx]. */
int smos_conv_rows_cl(const float* x, int64_t x_pitch, const float* wprep, const float* bias, const float* res, int64_t res_pitch,
                      float* out, int64_t out_pitch, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int32_t KH,
                      int32_t KW, int32_t mt, int32_t act, float* chan_sums, smos_stream_t stream);
int smos_conv_cl(const float* x, int64_t x_pitch, const float* wprep, const float* bias, const float* res, int64_t res_pitch,
                 float* out, int64_t out_pitch, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int32_t KH,
                 int32_t KW, int32_t stride, int32_t pad_h, int32_t pad_w, int32_t mt, int32_t act, float* chan_sums,
                 smos_stream_t stream);
/* smos_conv_cl on the bf16 matrix cores (csrc/conv_bf16.hip; the engine's opt-in conv_precision "bf16"):
 *   out = act(sum bf16(w) * bf16(x) + bias [+ res]);  products exact, sums / bias / residual / activation / chan_sums fp32.
 * x is fp32 and rounded to bf16 (round-to-nearest-even) as the kernel stages it.  Same operands, pitches, alignment, act
 * codes and chan_sums layout (smos_conv_cl_sum_chunks) as smos_conv_cl; Cin % 32 == 0, Cout % 32 == 0, Cout <= 2048,
 * KH, KW <= 7, stride 1 or 2, explicit padding; the block shape is chosen inside.  Shapes whose staged input region does
 * not fit are refused: ask smos_conv_bf16_cl_supported (1 / 0) first.
 * wprep: Cout * Cin * KH * KW bf16 (uint16 bit patterns, rounded to nearest even) in MFMA operand order; with
 * stage = ((cc * KH) + ky) * KW + kx (the 32-channel chunk outermost):
 *   wprep[(((stage * (Cout / 32) + q) * 2 + s) * 64 + lane) * 8 + j]
 *       = bf16(w[q * 32 + (lane & 31)][cc * 32 + 16 * s + 8 * (lane >> 5) + j][ky][kx]).
 * Deterministic: bit-identical from run to run, whatever the grid, the stream or the batch size. */
int smos_conv_bf16_cl_supported(int64_t Cin, int64_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t has_res);
int smos_conv_bf16_cl(const float* x, int64_t x_pitch, const uint16_t* wprep, const float* bias, const float* res,
                      int64_t res_pitch, float* out, int64_t out_pitch, int64_t B, int64_t H, int64_t W, int64_t Cin,
                      int64_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad_h, int32_t pad_w, int32_t act,
                      float* chan_sums, smos_stream_t stream);
/* smos_conv_cl for the stride-1 3x3 "same" layers in the Winograd F(2x2, 3x3) form (csrc/conv_wino.hip): 4 instead of 9
 * multiply-adds per output and channel pair, arithmetic still plain fp32 -- the weights are transformed on the host in
 * float64 (U = G g G^T, rounded once), the input and output transforms are additions.  Replaces the same reference layers as
 * smos_conv_cl (networks/backbone.py:136-159, networks/multi_view_encoder.py:446-447,478-497) where the kernel is 3x3 and
 * the stride 1.  Cin % 16 == 0, mb in {1, 2}: 16 * mb output channels per block, Cout % (16 * mb) == 0.  Operand order:
 *   wprep[((((ct * (Cin / 16) + cc) * 4 + i) * mb + m) * 4 + xi) * 64 + lane][nu]
 *       = U[xi][nu] of w[ct * 16 * mb + m * 16 + (lane & 15)][cc * 16 + 4 * (lane >> 4) + i],  U = G w G^T (4 x 4),
 *   G = [[1, 0, 0], [1/2, 1/2, 1/2], [1/2, -1/2, 1/2], [0, 0, 1]].
 * chan_sums (may be NULL; needs res == NULL): [B][chunks][Cout], chunks = smos_conv_wino_sum_chunks(H, W); entry
 *   (b, chunk, c) = sum of out[b, y, x, c] over two output rows x 32 columns (chunk = ((y / 8) * ceil(W / 32) + x / 32) * 4
 *   + (y % 8) / 2; parts outside the image contribute 0).  Summation order is fixed (run-to-run identical). */
int64_t smos_conv_wino_sum_chunks(int64_t H, int64_t W);
int smos_conv_wino_cl(const float* x, int64_t x_pitch, const float* wprep, const float* bias, const float* res, int64_t res_pitch,
                      float* out, int64_t out_pitch, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int32_t mb,
                      int32_t act, float* chan_sums, smos_stream_t stream);

/* act(conv(x, w) + bias) for a stride-1 KH x KW kernel with one extent 3 and the other 5 or 7 ("same" padding) in the 1-D
 * Winograd F(2, 3) form along the 3-tap axis (csrc/conv_wino1d.hip): 4 instead of 6 multiply-adds per pair of outputs, long-
 * axis tap and channel pair, fp32 throughout.  wprep = U = G g per long-axis tap, computed in float64 and rounded once, in
 * operand order [cout tile][cin chunk of 16][k-step i][long tap][mb][lane = q * 16 + m][position] (ops.conv_wino1d_prepare);
 * Cin % 16 == 0, Cout % (16 * mb) == 0, mb in {1, 2}; channels-last maps with row pitches in floats, 16-byte aligned.
 * Replaces nn.Conv2d + BatchNorm2d + ReLU of the two parallel branches of an Unbalance_BasicBlock
 * (networks/multi_view_encoder.py:478-497). */
int smos_conv_wino1d_cl(const float* x, int64_t x_pitch, const float* wprep, const float* bias, float* out, int64_t out_pitch,
                        int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t KH, int64_t KW, int32_t mb, int32_t act,
                        smos_stream_t stream);

/* conv3x3(bilinear_up(x)) without upsampling x (decoder conv_1, multi_view_encoder.py:441-453; csrc/upconv.hip).
 * z [B, Hs, Ws, 9*C] = the nine tap products W_{ky,kx} x at the source resolution (tap t = 3 ky + kx occupies channels
 * [t*C, (t+1)*C)), computed by the caller with one GEMM.
 *   smos_upconv_xpass  t [B, 3, Hs, Wo, C] <- sum_kx up_x(z tap (ky,kx))[X + kx - 1]   (taps leaving [0, Wo) dropped)
 *   smos_upconv_ypass  out [B, Ho, Wo, *] (row pitch out_pitch) <- act(conv_a + bias + sum_src sum_ky up_y(t_src)[Y + ky - 1]);
 *                      conv_a [B, Ho, Wo, *] (row pitch a_pitch) is the direct convolution of the channels that are not
 *                      upsampled; t2 may be NULL; act 0 none, 1 ReLU, 2 LeakyReLU(0.01); interpolation with ATen's
 *                      align_corners=True weights.
 *   smos_upconv_xy     the two passes in one launch, t kept on the CU (same operations in the same order: same
 *                      results): out <- act(conv_a + bias + sum over z1 [B, H1, W1, 9*C], z2 [B, H2, W2, 9*C] (one may
 *                      be NULL)).  Only for sources of at most half the output height: smos_upconv_xy_ok(Hs, Ho) != 0.
 *                      Refused as well (the kernel addresses a row with 32-bit byte offsets): a_pitch or out_pitch below C,
 *                      a row of conv_a, out (Wo * pitch) or z (Ws * 9 * C) of 2^29 floats = 2 GiB or more. */
int smos_upconv_xy_ok(int64_t Hs, int64_t Ho);
int smos_upconv_xy(const float* conv_a, int64_t a_pitch, const float* bias, const float* z1, int64_t H1, int64_t W1, const float* z2,
                   int64_t H2, int64_t W2, float* out, int64_t out_pitch, int64_t B, int64_t Ho, int64_t Wo, int64_t C, int32_t act,
                   smos_stream_t stream);
/*   smos_upconv_xy_units  smos_upconv_xy with the unit geometry given: `strip` output rows per unit of work (8, 16 or 32;
 *                      smos_upconv_xy chooses it from the sizes) and at most `max_blocks` blocks (0: no cap; fewer blocks
 *                      than units make a block walk several units).  Same results for every choice. */
int smos_upconv_xy_units(const float* conv_a, int64_t a_pitch, const float* bias, const float* z1, int64_t H1, int64_t W1,
                         const float* z2, int64_t H2, int64_t W2, float* out, int64_t out_pitch, int64_t B, int64_t Ho, int64_t Wo,
                         int64_t C, int32_t act, int32_t strip, int64_t max_blocks, smos_stream_t stream);
int smos_upconv_xpass(const float* z, float* t, int64_t B, int64_t Hs, int64_t Ws, int64_t C, int64_t Wo, smos_stream_t stream);
int smos_upconv_ypass(const float* conv_a, int64_t a_pitch, const float* bias, const float* t1, int64_t H1, const float* t2,
                      int64_t H2, float* out, int64_t out_pitch, int64_t B, int64_t Ho, int64_t Wo, int64_t C, int32_t act,
                      smos_stream_t stream);
/* The adjoint of the two passes (csrc/upconv_bwd.hip; the backward of ops.upconv3x3_train): from the output gradient
 * g [B, Ho, Wo, *] (row pitch g_pitch >= C) the gradient of one source's tap products,
 *     gz[b, ys, xs, (3 ky + kx) C + c] = sum_{Y, X} wy(Y + ky - 1 -> ys) wx(X + kx - 1 -> xs) g[b, Y, X, c]
 * with the float32 weights the forward applies and the taps that leave the Ho x Wo image dropped, in two launches:
 *   smos_upconv_bwd_ypass  s [B, 3, Hs, Wo, C] <- sum over the fine rows D that read source row ys of wy * g[b, D - ky + 1, X, c]
 *   smos_upconv_bwd_xpass  gz [B * Hs * Ws, *] (row pitch gz_pitch >= 9 * C; the layout of z) <- sum over the fine columns D
 *                          that read source column xs of wx * s[b, ky, ys, D - kx + 1, c]
 * Gather form: every element is summed by one thread in ascending D over smos_upconv_bwd_window(n_src, n_dst) candidates --
 * no atomics, the same bits on every run and for every grid.  max_blocks caps the grid (0: no cap; fewer blocks walk
 * the same elements in several trips).  The element-count limits of the forward passes, and n_src * n_dst <= 2^22 per axis. */
int smos_upconv_bwd_window(int64_t n_src, int64_t n_dst);
int smos_upconv_bwd_ypass(const float* g, int64_t g_pitch, float* s, int64_t B, int64_t Ho, int64_t Wo, int64_t C, int64_t Hs,
                          int64_t max_blocks, smos_stream_t stream);
int smos_upconv_bwd_xpass(const float* s, float* gz, int64_t gz_pitch, int64_t B, int64_t Hs, int64_t Ws, int64_t C, int64_t Wo,
                          int64_t max_blocks, smos_stream_t stream);

/* CatFusion + PredBranch (networks/backbone.py:387-413, 188-196): rows [B*N, K1] (row pitch in floats) ->
 * 1x1 K1->M1 + ReLU -> 1x1 M1->M2 + ReLU -> 1x1 M2->M3 + bias, out [B, M3, N]; one kernel, intermediates in registers
 * (csrc/point_head.hip).  Built for 192 -> 96 -> 64 -> M3 <= 32.  wprep: smos_point_head_weight_floats() floats =
 * the three weight matrices in MFMA operand order followed by the biases (b3 padded to 32):
 *   A1[(mt*96 + s)*64 + lane] = W1[mt*32 + (lane&31)][64*(s>>5) + 32*(lane>>5) + (s&31)]   (a row is three 64-channel
 *       segments; k-steps [32t, 32t+32) walk segment t, lane half h its channels [32h, 32h+32))
 *   A2[(mt*48 + s)*64 + lane] = W2[mt*32 + (lane&31)][ch(s, lane>>5)],  A3[s*64 + lane] = W3[lane&31][ch(s, lane>>5)] (0 beyond M3)
 *   with ch(s, h) = 32 (s >> 4) + 8 ((s & 15) >> 2) + 4 h + (s & 3)   (the accumulator order of the previous layer). */
int64_t smos_point_head_weight_floats(void);
/* The scan's padding tail can be left out: n_live (DEVICE int32, may be NULL = no tail) says how many points at the
 * front of every sample are real -- the reference pads every scan to frame_point_num with points at -1000
 * (datasets/data_StreamMOS.py:568-571) and cuts their predictions off again (val_StreamMOS.py:113); the logits of points
 * [*n_live, N) are written as zeros without being computed.  The streaming runner passes a count; AttNet.infer computes all N. */
int smos_point_head(const float* rows, int64_t row_pitch, const float* wprep, float* out, int64_t B, int64_t N, int64_t K1,
                    int64_t M1, int64_t M2, int64_t M3, const int32_t* n_live, smos_stream_t stream);

/* smos_point_head with the middle 64-channel segment of every row gathered from a channels-last map instead of read from
 * the row: channel 64 + c of point (b, n) = BilinearSample of grid [B, Hg, Wg, *] (pixel pitch grid_pitch floats, channels
 * [0, 64) read, 16-byte aligned, < 2 GiB) at gcoord * gscale, with the position arithmetic, tap order and absent-tap rule of
 * smos_gather_scatter_cl (gcoord, Kg, g_batch_stride, gscale as there).  Floats [64, 128) of `rows` are neither read nor
 * written; the logits equal those of smos_gather_scatter_cl(pts_out = rows + 64) followed by smos_point_head bit
 * for bit.  Replaces networks/backbone.py:453-475 (bev_grid2point) + :387-413,188-196 of the decoder's tail in one launch. */
int smos_point_head_gather(const float* rows, int64_t row_pitch, const float* wprep, float* out, int64_t B, int64_t N,
                           int64_t K1, int64_t M1, int64_t M2, int64_t M3, const int32_t* n_live, const float* grid,
                           int64_t grid_pitch, int64_t Hg, int64_t Wg, const float* gcoord, int32_t Kg,
                           int64_t g_batch_stride, const float* gscale, smos_stream_t stream);

/* smos_pointnet_scatter with a COMPACT target: rows [n_rows, T*cout] (zero-filled by smos_stem_scan) instead of
 * the dense [B,H,W,T*cout] grid; the features of cell (b, y, x) go to row row_of[b][y][x] (smos_stem_scan).
 * It can be told how many points of the current scan are real (n_live: DEVICE int32 or NULL; see smos_point_head): the point
 * rows of the padding tail [*n_live, N) are not computed and not written.  The scatter itself is unaffected (padding points lie
 * outside the grid). */
int smos_pointnet_scatter_rows(const float* xyzi, const float* coord, int32_t K, const float* w1, const float* b1,
                               const float* w2, const float* b2, float* rows, const int32_t* row_of, float* pts_out,
                               int64_t po_b, int64_t po_n, int64_t B, int64_t T, int64_t N, int64_t H, int64_t W, int32_t cin,
                               int32_t cmid, int32_t cout, const int32_t* n_live, smos_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Device-side validation preprocessing (csrc/preprocess.hip): what DataloadVal does with
 * numpy per sample (datasets/data_StreamMOS.py:397-599, datasets/utils.py:98-192).
 *   range6     host doubles {x_lo, x_hi, y_lo, y_hi, z_lo, z_hi}     (config Voxel.range_*)
 *   bev_size3  host int64   {512, 512, 30}                            (config Voxel.bev_shape)
 *   rv4        host doubles {phi_hi, dphi, theta_hi, dtheta} in radians (datasets/utils.py:176-181)
 */
/* moved[i] = (float32)(pose_diff * (x, y, z, 1)) computed in float64, intensity carried; mask[i] = lo <= p < hi.
 * pose_diff: host, 16 doubles row-major, or NULL (identity, the current scan). */
int smos_prep_transform_mask(const float* scan, int64_t n, const double* pose_diff, const double* range6, float* moved,
                             int32_t* mask, smos_stream_t stream);
/* Writes scan t of every TTA variant v (x *= tta_sx[v], y *= tta_sy[v]; V <= 4):
 *   xyzi [V,T,7,N] = (x, y, z, intensity, dist, frac(x_quan), frac(y_quan)), coord [V,T,N,3] = (x,y,z)_quan,
 *   sphere [V,T,N,2] = (theta_quan, phi_quan); kept points are compacted in order (slot prefix[i]-1, prefix = inclusive
 * prefix sum of mask), slots >= count hold the reference's padding point (-1000, -1000, -4000, -1000). */
int smos_prep_emit(const float* moved, const int32_t* mask, const int32_t* prefix, int64_t n, int32_t t, int32_t T, int64_t N,
                   int32_t V, const float* tta_sx, const float* tta_sy, const double* range6, const int64_t* bev_size3,
                   const double* rv4, float* xyzi, float* coord, float* sphere, smos_stream_t stream);
/* raw[i] = mask[i] ? labels[prefix[i]-1] : 0   (val_StreamMOS.py:112-118) */
int smos_prep_unpad_labels(const uint8_t* labels, int64_t N, const int32_t* mask, const int32_t* prefix, int64_t n,
                           uint8_t* raw, smos_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Device-side training sample builder (csrc/train_prep.hip): what DataloadTrain.__getitem__
 * does with numpy per sample (datasets/data_StreamMOS.py:292-364, datasets/utils.py:116-126,280-343) without copy-paste:
 * 5 scans -> 3 chained windows of 3 frames (window w, frame t = scan w + t), each aligned (twice for w > 0, one float32
 * rounding per alignment), range-filtered, resampled with replacement to N points, augmented, quantised; the targets of
 * frame 0 and its BEV label grid.  range6 / bev_size3 / rv4 as in the validation block above.  Four launches, no host read.
 *
 *   scans[5], label_words[5]  host arrays of device pointers: [n_k, 4] float32 rows (16-byte aligned), [n_k] uint32 words
 *   n[5]                      host, 1 <= n_k <= 2^30
 *   first_pose  [5][16]       host doubles, inv(P_0) P_k row-major (applied to every scan, frame 0 included)
 *   second_pose [3][16]       host doubles, inv(P_w) P_0 (entry 0 is not read)
 *   words, noise              device draws, uint32 [3, 3, N] and float64 [3, 3*N, 3], or both NULL: the seeded generator
 *   seed, sample_index, noise_mean, noise_std   read by the seeded generator only
 *   shift3, scale, v_flip, h_flip, rot_cos, rot_sin   the sample's augmentation scalars (host); shift and scale are rounded
 *                             to float32, cos / sin of theta_z * pi / 180 stay float64; v_flip negates x, h_flip negates y
 *   lut [n_maps][lut_len]     device int32; target m = lut[m][word & 0xFFFF], 0 for an id >= lut_len; 1 <= n_maps <= 4
 *   xyzi[3], coord[3], sphere[3]   host arrays of device pointers, per window: [3,7,N], [3,N,3], [3,N,2] float32
 *   targets[n_maps * 3]       device pointers [N] int64, entry m * 3 + w
 *   bev[3]                    device pointers [bev_size3[0]/2, bev_size3[1]/2] int64: max label of map 0 over the cells
 *                             (int)(x_quan * 0.5), (int)(y_quan * 0.5) of frame 0 with the cell rule of
 *                             smos_voxel_maxpool_fwd, empty cell 0; zero-filled here
 *   counts [9]                device int32: in-range points of job 3 w + t.  A job with none is written as the validation
 *                             padding point (-1000, -1000, -4000, -1000) with label 0 (the reference raises there)
 *   work                      smos_train_prep_work_bytes(max n_k) bytes of device scratch, 256-byte aligned (-1: bad size)
 * Resampling: slot j takes kept point ((uint64)r * n_valid) >> 32 of its 32-bit draw r.
 * Augmentation per slot: p = f32(f64(p) + noise); p += f32(shift); p *= f32(scale); flips;
 *   x' = f32(f64(x) * cos + f64(y) * sin), y' = f32(f64(y) * cos - f64(x) * sin).  Out-of-range results are kept.
 * Seeded draws: Philox4x32-10, key = (seed low word, seed high word), counter = (j, call << 16 | w << 8 | t,
 *   sample_index low word, sample_index high word).  Call 0 yields (r, unused, x1, x2), call 1 yields (y1, y2, z1, z2);
 *   noise_d = f64(f32(z_d * f32(noise_std)) + f32(noise_mean)) with the float32 Box-Muller
 *   z_d = sqrt(-2 ln(((d1 >> 8) + 1) * 2^-24)) * cos(2 pi * (d2 >> 8) * 2^-24).
 * The results depend on neither the grid size nor smos_debug_set_conv_grid_cap, which caps these launches too. */
int64_t smos_train_prep_work_bytes(int64_t n_max);
int smos_train_prep_build(const void* const* scans, const void* const* label_words, const int64_t* n, const double* first_pose,
                          const double* second_pose, const double* range6, const int64_t* bev_size3, const double* rv4,
                          int64_t N, const uint32_t* words, const double* noise, uint64_t seed, uint64_t sample_index,
                          double noise_mean, double noise_std, const double* shift3, double scale, int32_t v_flip,
                          int32_t h_flip, double rot_cos, double rot_sin, const int32_t* lut, int32_t n_maps, int32_t lut_len,
                          void* const* xyzi, void* const* coord, void* const* sphere, void* const* targets, void* const* bev,
                          int32_t* counts, void* work, int64_t work_bytes, smos_stream_t stream);
/* words [3, 3, N] uint32 and noise [3, 3*N, 3] float64 (device): exactly what smos_train_prep_build generates for
 * (seed, sample_index) when it is given no draws. */
int smos_train_prep_draws(uint64_t seed, uint64_t sample_index, int64_t N, double noise_mean, double noise_std,
                          uint32_t* words, double* noise, smos_stream_t stream);

/*
 * Copy-paste augmentation on the device (csrc/copy_paste.hip): SequenceCutPaste of the reference
 * (datasets/copy_paste.py, copy_paste_seg.py) on the five scans of a training sample; host restatement:
 * streammos_amd.preprocess.copy_paste_sample.  All pointers but the small host arrays named so are DEVICE pointers; everything
 * runs on `stream`, nothing is read back.
 *   state of a sample   frame k owns rows off_k .. off_k + n[k] + slots of four flat arrays, off_k = sum over the frames before
 *                       it: pts [rows, 4] float32, words [rows] uint32, angles [rows, 2] float32 (phi, theta), flags [rows]
 *                       uint8 (bit 0 alive, bit 1 object class).  A frame's rows are its scan points in their order, then one
 *                       slot range per object in paste order (`slots` = the points of all objects).  A removed point and an
 *                       unused slot hold the padding point (-1000, -1000, -4000, -1000); every row keeps its word.
 *   status [count]      int32: the accepted trial of each object, -1 if none (or skipped)
 * smos_copy_paste_begin: one launch.  scans[k] [n[k], 4] float32 raw, label_words[k] [n[k]] uint32, first_pose (HOST) five
 * row-major 4x4 float64 inv(P_0) P_k: the first alignment (float64, rounded once), the angles, the flags, padded slots,
 * status = -1.
 * smos_copy_paste_object: four launches for object `number` (0-based, in paste order) of m >= 10 points (the caller skips
 * smaller ones, copy_paste.py:195) whose slot range starts at row n[k] + slot of every frame.  scan0 / label_words0 /
 * first_pose0: scan 0 again (the road points, semantic id 40, as form_seq takes them: never edited).  object_points [m, 4]
 * float32 and footprint [4, 2] float64 (the x, y of the first four corners of the box scaled by 1.05) lie in the object bank.
 * HOST arrays: shift_x5 / shift_y5 = velo_x * t * 0.1, velo_y * t * 0.1; order20 a permutation of 0..19 (trial j turns by
 * 18 * order20[j] degrees on top of the trials before it); cos20 / sin20 of 18 i degrees.  noise [5, m, 3] float64 or NULL:
 * generated in the kernels, Philox4x32-10 with key = seed and counter (point, 1 << 24 | call << 16 | number << 8 | frame,
 * sample_index lo, hi), call 0 words 2, 3 -> x, call 1 words 0, 1 -> y and 2, 3 -> z through the float32 Box-Muller of
 * smos_train_prep_build, times 0.001.  paste_word: the label word of the pasted points (label base + motion label).
 * work: smos_copy_paste_work_bytes(n[0]) bytes of device scratch, 256-byte aligned (-1: bad size); a stream's objects share it.
 * smos_copy_paste_draws: noise [5, m, 3] float64 exactly as the kernels generate it.
 * Grids are capped by smos_debug_set_conv_grid_cap; the bits do not depend on the grid.
 */
int64_t smos_copy_paste_work_bytes(int64_t n0);
int smos_copy_paste_begin(const void* const* scans, const void* const* label_words, const int64_t* n, const double* first_pose,
                          int64_t slots, int32_t count, void* pts, void* words, void* angles, void* flags, int32_t* status,
                          smos_stream_t stream);
int smos_copy_paste_object(const void* scan0, const void* label_words0, const double* first_pose0, const int64_t* n, int64_t slots,
                           void* pts, void* words, void* angles, void* flags, int32_t* status, int32_t count, int32_t number,
                           const void* object_points, int32_t m, int64_t slot, const double* footprint, const double* shift_x5,
                           const double* shift_y5, const uint8_t* order20, const double* cos20, const double* sin20,
                           const double* noise, uint64_t seed, uint64_t sample_index, uint32_t paste_word, void* work,
                           int64_t work_bytes, smos_stream_t stream);
int smos_copy_paste_draws(uint64_t seed, uint64_t sample_index, int32_t number, int32_t m, double* noise, smos_stream_t stream);

/* Multi-scale deformable attention, backward (training row f2).  Replaces
 * MultiScaleDeformableAttention.ms_deform_attn_backward (deformattn/src/cuda/ms_deform_attn_cuda.cu:83-153, kernels
 * ms_deform_im2col_cuda.cuh:87-159,301-920).  grad_out [N,Lq,M*D]; grad_value [N,S,M,D] MUST be zero-filled by the
 * caller (accumulated with atomic adds); grad_sampling_loc [N,Lq,M,L,P,2] and grad_attn_weight [N,Lq,M,L,P] are
 * fully written. */
int smos_msda_bwd(const void* grad_out, const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                  const void* sampling_loc, const void* attn_weight, void* grad_value, void* grad_sampling_loc,
                  void* grad_attn_weight, int64_t N, int64_t S, int64_t M, int64_t D, int64_t L, int64_t Lq, int64_t P,
                  int32_t dtype, smos_stream_t stream);

/* smos_msda_bwd for float32 with grad_value summed in a fixed order (csrc/segsum.hip; the scheme and the definition of
 * the sum are those of smos_bilinear_gather_bwd_det).  Pair index ((((b * Lq + q) * M + m) * L + l) * P + p) * 4 + corner,
 * corners in the order of the atomic kernel (top-left, top-right, bottom-left, bottom-right); key = the row
 * (b * S + level_start[l] + y * W + x) * M + m of grad_value; pair weight (w_y * w_x) * attn, two float32 products in that
 * order; term = weight * grad_out[b, q, m, :].  grad_value may arrive uninitialised and is fully written (0 where no
 * sample reaches).  grad_sampling_loc and grad_attn_weight come from the arithmetic of smos_msda_bwd: the same bits.
 *   work   smos_msda_bwd_det_work_bytes(N, S, M, D, L, Lq, P) bytes of device scratch, 256-byte aligned (0: an empty
 *          problem, -1: more than 2^29 - 1 samples or 2^31 - 2 value rows). */
int64_t smos_msda_bwd_det_work_bytes(int64_t N, int64_t S, int64_t M, int64_t D, int64_t L, int64_t Lq, int64_t P);
int smos_msda_bwd_det(const float* grad_out, const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                      const float* sampling_loc, const float* attn_weight, float* grad_value, float* grad_sampling_loc,
                      float* grad_attn_weight, int64_t N, int64_t S, int64_t M, int64_t D, int64_t L, int64_t Lq, int64_t P,
                      void* work, int64_t work_bytes, smos_stream_t stream);

/* --------------------------------------------------------------------------------------------
 * Channels-last ("cl") engine kernels (csrc/cl_kernels.hip).  A map is [B, H, W, C] with C innermost; every tensor
 * argument has its own row pitch (elements between consecutive pixels / points), so it may be a channel slice of a
 * wider buffer.  P = number of rows (B*H*W).  All pointers 16-byte aligned, C and pitches multiples of 4.
 */
int smos_bias_act_cl(const float* x, int64_t x_pitch, const float* bias, const float* res, int64_t res_pitch, float* out,
                     int64_t out_pitch, int64_t P, int64_t C, int32_t act, smos_stream_t stream);
int smos_downsample_epilogue_cl(const float* a, int64_t a_pitch, const float* p, int64_t p_pitch, const float* bias, float* out,
                                int64_t out_pitch, int64_t B, int64_t C, int64_t H, int64_t W, int32_t stride,
                                smos_stream_t stream);
/* ws: device scratch of at least B*C*(ceil(HW/512)+1) floats (deterministic two-stage column sums + the gates). */
int smos_channel_gate_residual_cl(const float* y, int64_t y_pitch, const float* bias, const float* w1, const float* b1,
                                  const float* w2, const float* b2, const float* xres, int64_t res_pitch, float* out,
                                  int64_t out_pitch, float* ws, int64_t ws_floats, int64_t B, int64_t C, int64_t Cr, int64_t HW,
                                  smos_stream_t stream);
/* The same block fed by the channel sums a smos_conv_cl launch left behind (chan_sums [B][chunks][C], see smos_conv_cl):
 * gate MLP + out = relu((y + bias) * gate + xres), no pass over y for the average pool.  gate_ws: B*C floats of scratch. */
int smos_channel_gate_apply_cl(const float* y, int64_t y_pitch, const float* bias, const float* w1, const float* b1,
                               const float* w2, const float* b2, const float* xres, int64_t res_pitch, float* out,
                               int64_t out_pitch, const float* chan_sums, int64_t chunks, float* gate_ws, int64_t B, int64_t C,
                               int64_t Cr, int64_t HW, smos_stream_t stream);
/* BasicBlock.forward (networks/backbone.py:136-159: conv3x3-BN-ReLU, conv3x3-BN, optional ChannelAtt gate, + x, ReLU) on
 * channels-last maps as ONE foreign call: enqueues smos_conv_wino_cl twice (+ smos_channel_gate_apply_cl when gw1 != NULL) on
 * `stream` -- the same launches with the same arguments as the separate calls, so results are bit-identical; what is saved is
 * the host's per-call marshalling (csrc/blocks.hip).  u1 / u2: the Winograd weight blocks of the two convs (BN folded,
 * ops.conv_wino_prepare, same mb); b1 / b2 their biases; gw1 [Cr, C], gb1 [Cr], gw2 [C, Cr], gb2 [C]: the gate MLP or all NULL;
 * y: scratch map [B,H,W,*] (pitch y_pitch) for the first conv's output; out may not alias x or y; ws: smos_basic_block_ws_floats
 * floats of scratch, needed with a gate only.  Shape limits are those of smos_conv_wino_cl with Cin == Cout == C. */
int64_t smos_basic_block_ws_floats(int64_t B, int64_t H, int64_t W, int64_t C);
int smos_basic_block_cl(const float* x, int64_t x_pitch, const float* u1, const float* b1, const float* u2, const float* b2,
                        const float* gw1, const float* gb1, const float* gw2, const float* gb2, int64_t Cr, float* y,
                        int64_t y_pitch, float* out, int64_t out_pitch, float* ws, int64_t B, int64_t H, int64_t W, int64_t C,
                        int32_t mb, smos_stream_t stream);
/* Unbalance_BasicBlock.forward (networks/multi_view_encoder.py:478-497) as one foreign call: smos_conv_wino1d_cl for the
 * (kha x kwa) and (khb x kwb) branches into channels [0, C) and [C, 2C) of `both` (ReLU), then smos_conv_wino_cl 2C -> C over
 * `both` with residual x and ReLU into out.  ua / ub = ops.conv_wino1d_prepare, uc = ops.conv_wino_prepare, all with the same mb.
 * Same launches and arguments as the separate calls (bit-identical). */
int smos_unbalance_block_cl(const float* x, int64_t x_pitch, const float* ua, const float* ba, int64_t kha, int64_t kwa,
                            const float* ub, const float* bb, int64_t khb, int64_t kwb, const float* uc, const float* bc,
                            float* both, int64_t both_pitch, float* out, int64_t out_pitch, int64_t B, int64_t H, int64_t W,
                            int64_t C, int32_t mb, smos_stream_t stream);
/* Zero fill of n <= 4 channels-last views (rows[i] rows of row_floats[i] floats at pitch pitches[i], 16-byte aligned) in one
 * launch: the zero-initialised scatter-max targets of the cross-view transfers (networks/multi_view_encoder.py:395-420 create
 * theirs with torch.zeros inside VoxelMaxPool, deep_point/point_deep.py:27). */
int smos_zero_views_cl(int32_t n, float* const* ptrs, const int64_t* rows, const int64_t* row_floats, const int64_t* pitches,
                       smos_stream_t stream);
/* Bilinear (align_corners=True) resize of n_src <= 3 channels-last sources to Ho x Wo, concatenated along C into the dense
 * out [B, Ho, Wo, sum src_c].  Every source: 16-byte aligned, src_c % 4 == 0, src_h, src_w > 0, src_pitch % 4 == 0 and
 * src_pitch >= src_c; out 16-byte aligned. */
int smos_upsample_concat_cl(const float* const* src, const int64_t* src_c, const int64_t* src_h, const int64_t* src_w,
                            const int64_t* src_pitch, int32_t n_src, float* out, int64_t B, int64_t Ho, int64_t Wo,
                            smos_stream_t stream);
/* DownSample2D's tail with the pool branch computed on the fly (networks/backbone.py:105-134; csrc/downsample.hip):
 * out = relu(a + bias + maxpool3x3(conv1x1(x, w); stride, pad 1)) -- replaces smos_conv_cl (1x1, full resolution) +
 * smos_downsample_epilogue_cl; q = W x stays in LDS.  x [B,H,W,*] pitch x_pitch; wpairs = the [Cout, Cin] weights (BN folded) as
 * 16 x 16 blocks in MFMA operand order (streammos_amd.ops.pool_branch_prepare); a / out [B,Ho,Wo,*]; Cin == Cout in {32, 64, 128}
 * (128 at stride 2 only); stride 1 or 2. */
int smos_downsample_pool_branch(const float* x, int64_t x_pitch, const float* wpairs, const float* a, int64_t a_pitch,
                                const float* bias, float* out, int64_t out_pitch, int64_t B, int64_t H, int64_t W, int64_t Cin,
                                int64_t Cout, int32_t stride, smos_stream_t stream);
/* BilinearSample (networks/backbone.py:453-475) of the channels-last grid [B,Hg,Wg,*] (pixel pitch grid_pitch, C channels read)
 * at gcoord*gscale, fused with VoxelMaxPool of the result into the zero-filled channels-last out [B,Ho,Wo,*] (pixel pitch
 * out_pitch) at int(scoord*sscale) (networks/multi_view_encoder.py:395-404,410-419).  out may be NULL (gather only); pts_out
 * (optional) receives the gathered features as rows pts_out[b*po_b + n*po_n + c].  C is 32 or 64.
 * n_live (DEVICE int32 or NULL; see smos_point_head): point rows of the padding tail are not written.
 * The coordinates are strided views: sample b, point n at coord + b * batch_stride + n * K floats (the first two of a point's
 * K values are read; a dense [B, N, K] tensor has batch_stride N * K).  Lets a caller pass pcds_coord[:, 0, :, :, 0] of the
 * reference's [B, T, N, 3, 1] tensor (networks/multi_view_encoder.py:395-420 slice it the same way) without a compacting copy. */
int smos_gather_scatter_cl(const float* grid, int64_t grid_pitch, const float* gcoord, int32_t Kg, int64_t g_batch_stride,
                           const float* gscale, const float* scoord, int32_t Ks, int64_t s_batch_stride, const float* sscale,
                           float* out, int64_t out_pitch, float* pts_out, int64_t po_b, int64_t po_n, int64_t B, int64_t C,
                           int64_t Hg, int64_t Wg, int64_t N, int64_t Ho, int64_t Wo, const int32_t* n_live,
                           smos_stream_t stream);

/* Per-frame label outputs of the overlapped sequence loop (streammos_amd/run_sequence.py).  labels [n] uint8 in {0,1,2}
 * (4-byte aligned) -> words [n] int32 (16-byte aligned; NULL: not written): lut != 0 the learning_map_inv value 0 / 9 / 251
 * (predictions/), lut == 0 the label itself (predictions_bf/).  gt [n] uint32 (16-byte aligned; NULL: nothing counted) holds
 * SemanticKITTI label words, mapped through gt_map[word & 0xFFFF] (map_n int32 entries; ids >= map_n count as 0); counts[6]
 * (device uint64) += tp1, tp2, pred1, pred2, gt1, gt2 over the points whose mapped gt is not 0 (kitti.MovingIoU.add). */
int smos_label_words(const uint8_t* labels, int64_t n, int32_t lut, int32_t* words, const uint32_t* gt, const int32_t* gt_map,
                     int32_t map_n, uint64_t* counts, smos_stream_t stream);
/* The same for voted LUT words (int32 [n], 16-byte aligned): class 2 for 251, 1 for 9, 0 otherwise; words gets a copy. */
int smos_label_count_voted(const int32_t* voted, int64_t n, int32_t* words, const uint32_t* gt, const int32_t* gt_map,
                           int32_t map_n, uint64_t* counts, smos_stream_t stream);

/* Training point MLP (csrc/point_mlp_train.hip): BN0 -> conv1x1 7->64 -> BN1 -> ReLU -> conv1x1 64->64 -> BN2 ->
 * ReLU of PointNetStacker(7, 64, pre_bn=True, stack_num=2) on x [S,7,N] -> y [S,64,N], both channel-major float32.
 *   params     HOST array of 14 DEVICE float pointers: gamma0, beta0, running_mean0, running_var0, W1 [64,7], gamma1, beta1,
 *              running_mean1, running_var1, W2 [64,64], gamma2, beta2, running_mean2, running_var2
 *   eps_mom    HOST array of 6 doubles: eps of BN0..2, then momentum of BN0..2
 *   training   != 0: batch statistics over the S*N points (biased variance), the six running buffers updated in place
 *              (running_var with the unbiased variance); S*N must exceed 1.  0: the running buffers are the statistics.
 *   fold       smos_point_mlp_fold_floats() floats, dstat smos_point_mlp_stat_doubles() doubles: written by the forward, read
 *              by the backward; together with x they are all the backward needs from the forward.
 *   grads      HOST array of 8 DEVICE float pointers, NULL where no gradient is wanted: gamma0, beta0, W1, gamma1, beta1, W2,
 *              gamma2, beta2.  Work that only a NULL entry needs is not done.  There is no gradient for x.
 *   work       smos_point_mlp_work_bytes(S*N) bytes of device scratch (-1 from the query: too many points).
 * Every sum over points is formed per chunk of smos_point_mlp_chunk() points and added in chunk order in float64: the bits of
 * y, of the buffers and of every gradient depend on the data alone, not on the grid (smos_debug_set_conv_grid_cap bounds the
 * grids of the chunk walks) or the run.  Nothing is read back to the host. */
int32_t smos_point_mlp_chunk(void);
int32_t smos_point_mlp_fold_floats(void);
int32_t smos_point_mlp_stat_doubles(void);
int64_t smos_point_mlp_work_bytes(int64_t P);
int smos_point_mlp_fwd(const float* x, int64_t S, int64_t N, int32_t training, const void* const* params, const double* eps_mom,
                       float* y, float* fold, double* dstat, void* work, int64_t work_bytes, smos_stream_t stream);
int smos_point_mlp_bwd(const float* x, const float* grad_y, int64_t S, int64_t N, int32_t training, const void* const* params,
                       const double* eps_mom, const float* fold, const double* dstat, void* const* grads, void* work,
                       int64_t work_bytes, smos_stream_t stream);

/* Training point head (csrc/point_head_train.hip): cat(a, b, c) -> dropout -> conv1x1 192->96 -> BN1 -> ReLU ->
 * conv1x1 96->64 -> BN2 -> ReLU -> dropout -> conv1x1 64->3 + bias (CatFusion + PredBranch) on three [B,64,N] channel-major float32
 * inputs -> logits [B,3,N] float32.
 *   pitch      HOST array of 3: floats between two channels of a / b / c (>= N; a sample is 64 channels).  Outputs are dense.
 *   masks      smos_point_head_train_mask_words(B*N) uint32 of packed keep bits, 8 word planes of B*N: bit k & 31 of word k >> 5
 *              keeps input channel k (k < 192), bit j & 31 of word 6 + (j >> 5) keeps channel j of the second dropout.  NULL:
 *              nothing is dropped and nothing scaled.  scale = 1 / keep probability (1.25), applied to kept values only.
 *   smos_point_head_train_masks fills them: from keep1 [B,192,N] and keep2 [B,64,N] bytes (non-zero: keep) when both are
 *              given, else from Philox4x32-10 keyed by the two DEVICE int64 words at seed (read on the device): key = the
 *              halves of seed[0], counter (point, 8 * word + i, halves of seed[1]); output v of call i decides bit 4 i + v; a
 *              value is kept iff its 32-bit draw is below 3435973837 = ceil(0.8 * 2^32): keep probability 0.8 + 4.7e-11.
 *   params     HOST array of 12 DEVICE float pointers: W1 [96,192], gamma1, beta1, running_mean1, running_var1, W2 [64,96],
 *              gamma2, beta2, running_mean2, running_var2, W3 [3,64], b3
 *   eps_mom    HOST array of 4 doubles: eps of BN1, BN2, then momentum of BN1, BN2
 *   training   != 0: batch statistics over the B*N points (biased variance), the four running buffers updated in place
 *              (running_var with the unbiased variance); B*N must exceed 1.  0: the running buffers are the statistics.
 *   fold       smos_point_head_train_fold_floats() floats written by the forward and read by the backward (the weights as
 *              the forward saw them and the folded statistics); with the inputs and the masks it is all the backward needs.  dstat: smos_point_head_train_stat_doubles() doubles, the float64 mean
 *              and biased variance of both batch norms as the forward normalised with them.
 *   grads      HOST array of 11 DEVICE float pointers, NULL where no gradient is wanted: d_a, d_b, d_c [B,64,N] (all three or
 *              none), dW1, dgamma1, dbeta1, dW2, dgamma2, dbeta2, dW3, db3.  Work that only a NULL entry needs is not done.
 *   work       smos_point_head_train_work_bytes(B*N) bytes of device scratch (-1 from the queries: too many points).
 * Every sum over points is formed per chunk of smos_point_head_train_chunk() points and added in chunk order in float64: the bits
 * of every result depend on the data alone, not on the grid (smos_debug_set_conv_grid_cap bounds the grids of the chunk walks)
 * or the run.  Nothing is read back to the host. */
int32_t smos_point_head_train_chunk(void);
int32_t smos_point_head_train_fold_floats(void);
int32_t smos_point_head_train_stat_doubles(void);
int64_t smos_point_head_train_work_bytes(int64_t P);
int64_t smos_point_head_train_mask_words(int64_t P);
int smos_point_head_train_masks(const uint8_t* keep1, const uint8_t* keep2, const int64_t* seed, int64_t B, int64_t N,
                                uint32_t* masks, smos_stream_t stream);
int smos_point_head_train_fwd(const float* a, const float* b, const float* c, const int64_t* pitch, const uint32_t* masks,
                              double scale, int64_t B, int64_t N, int32_t training, const void* const* params,
                              const double* eps_mom, float* logits, float* fold, double* dstat, void* work, int64_t work_bytes,
                              smos_stream_t stream);
int smos_point_head_train_bwd(const float* a, const float* b, const float* c, const int64_t* pitch, const uint32_t* masks,
                              double scale, const float* grad_logits, int64_t B, int64_t N, int32_t training, const float* fold,
                              void* const* grads, void* work, int64_t work_bytes, smos_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SMOS_H_ */
