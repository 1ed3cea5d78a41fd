/*
 * rpe.h -- C ABI of librpe_hip.so: the MI355X (gfx950) hot path of the per-frame stereo pose solve.
 *
 * Drop-in boundary for aimi-lab/robust-pose-estimator (reference paths are relative to its repo root).
 * Every entry point takes raw DEVICE pointers, explicit shapes and a HIP stream (passed as void*, a
 * hipStream_t; NULL = the default stream).  All tensors are caller-owned, contiguous, NCHW, row-major,
 * x fastest.  Inputs are const; outputs and scratch are pre-allocated by the caller (size-query
 * functions below).  The library keeps no mutable global state and is re-entrant (one host thread per
 * GPU).  Return value: 0 = ok; <0 = RPE_E_* below.  No C++ exception crosses this boundary.  Numerical
 * failure is signalled in-band exactly like the reference (NaN pose -> caller's failure gate,
 * core/pose/pose_estimator.py:81-87).
 */
#ifndef RPE_H
#define RPE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPE_OK 0
#define RPE_E_BADARG (-1)  /* null pointer, non-positive size, unsupported dtype / radius / level count */
#define RPE_E_LAUNCH (-2)  /* hipGetLastError() != hipSuccess after a launch                            */
#define RPE_E_UNSUPPORTED (-3)

#define RPE_F32 0
#define RPE_F64 1
#define RPE_F16 2      /* rpe_corr_build_ex and the rpe_corr_alt_*_ex / _dt entry points only: feature maps rounded to fp16 */
#define RPE_F32X3 3    /* rpe_corr_build_ex only: f32 feature maps, every f32 product evaluated as six bf16 products (3-way exact split) */

/* solver modes of rpe_pose_solve */
#define RPE_SOLVER_LBFGS 0 /* reference-faithful: torch.optim.LBFGS(lr=1, line_search_fn=None) iterates */
#define RPE_SOLVER_GN 1    /* Gauss-Newton: 6x6 normal equations, Cholesky in f64                        */

/* stop reasons written to info[.][2] by rpe_pose_solve (0 = still running / not started) */
#define RPE_STOP_OPT_AT_START 1 /* max|g| <= 1e-7 at the first evaluation                                */
#define RPE_STOP_GTD 2          /* directional derivative g.d > -1e-9                                    */
#define RPE_STOP_MAX_ITER 3
#define RPE_STOP_MAX_EVAL 4     /* evals >= max_iter*5/4                                                 */
#define RPE_STOP_OPT 5          /* max|g| <= 1e-7                                                        */
#define RPE_STOP_STEP 6         /* max|t*d| <= 1e-9                                                      */
#define RPE_STOP_LOSS 7         /* |loss - prev_loss| < 1e-9                                             */
#define RPE_STOP_NOT_PD 8       /* GN only: H not positive definite or g not finite; pose left unchanged */

/* Library / build identification, e.g. "rpe-hip 0.1 gfx950". */
const char *rpe_version(void);
/* Layout version of this header's structs (rpe_conv_desc, rpe_solve_opts) and signatures: a binding compares it with the
 * RPE_ABI_VERSION it was written against before the first call (the ctypes binding does, robust-pose-estimator_amd/_lib.py).
 * 5: rpe_conv_desc is 200 bytes (stats_tiles), stride-2 statistics are one record per 32 output pixels, rpe_pose_solve_ex, rpe_pose_gate_chain.
 * Entry points are only ever ADDED under one RPE_ABI_VERSION (they change no struct and no existing signature); RPE_ABI_MINOR counts those
 * additions, so a binding can require "version 5, minor >= m" for the newest entry point it calls -- or probe with dlsym:
 *   minor 0: the 68 entry points of round 4;  1: rpe_conv_wino_x3*, rpe_conv1x1_x3*, rpe_conv_wino1d_x3* (9, round 5);  2: rpe_run_ops and
 *   the rpe_*_args structs of the prepared launch lists, rpe_corr_lookup_conv1x1* (round 6);  3: struct rpe_surfel_map and the
 *   rpe_surfel_* entry points of frame-to-model tracking (7);  4: rpe_surfel_*_many (K maps per launch, RPE_SURFEL_MAX_MAPS) and
 *   rpe_pose_gate_chain_rows, for tracking several sequences frame to model in one batch (8).  rpe_conv_wino24* and RPE_OP_CONV_WINO24
 *   (Winograd F(2x4,3x3)) were added without a new minor: probe for them with dlsym.  So were rpe_flow_forward_interpolate, rpe_flow_seed
 *   and RPE_OP_FLOW_SEED (warm start of the update loop), rpe_ingest_stereo (the one-call input side) and rpe_pose_quality /
 *   rpe_pose_quality_workspace_bytes (the solve-quality report), and rpe_conv_fused_m96 with RPE_OP_CONV_FUSED_M96 (the 96-row tile class
 *   of the stride-2 3x3 layers), and rpe_corr_alt_bytes / rpe_corr_alt_prepare / rpe_corr_alt_lookup with RPE_OP_CORR_ALT_PREPARE /
 *   RPE_OP_CORR_ALT_LOOKUP (correlation without the all-pairs volume), and the entry points of the update loop on zero-padded maps:
 *   rpe_conv_wino_v, rpe_conv_wino24_v, rpe_conv_wino1d_v, rpe_conv1x1_v (struct rpe_conv_desc_v), rpe_stem_conv_v, rpe_conv3x3_to2_flow_v,
 *   rpe_corr_lookup_ex, rpe_corr_alt_lookup_ex, rpe_upsample_convex_ex, rpe_copy_rect with RPE_OP_* kinds 22-31, and the entry points of the
 *   encoders on zero-padded maps: rpe_enc_conv_wino_v, rpe_enc_conv_wino24_v, rpe_enc_conv_s2_v, rpe_enc_conv_s2_m96_v, rpe_instnorm_apply_v
 *   with RPE_OP_* kinds 34-38 (32 and 33 are the event ops), and the fp16 feature maps of the correlation without the volume:
 *   rpe_corr_alt_bytes_ex, rpe_corr_alt_prepare_ex, rpe_corr_alt_lookup_dt with RPE_OP_CORR_ALT_PREPARE_EX / RPE_OP_CORR_ALT_LOOKUP_DT (39, 40),
 *   and the update block's convolutions with fp16 operands: rpe_conv_f16_packed_bytes, rpe_conv_f16_pack, rpe_conv_f16 with RPE_OP_CONV_F16 (41);
 *   and the backward of the geometry stage: rpe_depth_backproject_warp_backward, rpe_depth_backproject_warp_backward_workspace_bytes,
 *   rpe_flow2depth_backward;
 *   and the backward of RAFT's output heads: rpe_upsample_convex_backward, rpe_conv_bwd_weight, rpe_conv_bwd_weight_workspace_bytes,
 *   rpe_conv3x3_to2_bwd_data, rpe_relu_backward, rpe_sum_groups;
 *   and the backward of one update-block application: rpe_gru_gates_zr_recompute, rpe_gru_gates_h_recompute,
 *   rpe_gru_gates_zq_backward, rpe_gru_gates_r_backward (rpe_conv_bwd_weight also takes
 *   (1,5), (5,1) and (7,7) since then: rpe_conv_bwd_weight_workspace_bytes returns 0 for them in a library that does not);
 *   and the backward of the correlation: rpe_corr_grad_volume_floats, rpe_corr_lookup_backward, rpe_corr_build_backward_workspace_bytes,
 *   rpe_corr_build_backward;
 *   and the backward of the encoders: rpe_conv_s2_bwd_weight, rpe_conv_s2_bwd_weight_workspace_bytes, rpe_conv_s2_bwd_data,
 *   rpe_bn_frozen_backward, rpe_bn_frozen_backward_workspace_bytes, rpe_instnorm_backward, rpe_split_act_backward;
 *   and the training step's update: rpe_optim_chunk_floats, rpe_optim_chunk_offsets, rpe_optim_workspace_bytes, rpe_grad_norm,
 *   rpe_adamw_step (structs rpe_optim_row, rpe_optim_chunk, rpe_optim_record);
 *   and RAFT's sequence loss on ground-truth flow: rpe_flow_sequence_loss_workspace_bytes, rpe_flow_sequence_loss,
 *   rpe_flow_sequence_loss_backward;
 *   the next RPE_ABI_MINOR bump counts them and rpe_conv_wino24*. */
#define RPE_ABI_VERSION 5
#define RPE_ABI_MINOR 4
int rpe_abi_minor(void);
int rpe_abi_version(void);

/* ---------------------------------------------------------------------------------------------------------
 * SE(3) group ops -- replace the lietorch C++/CUDA kernels the reference calls through
 * `from lietorch import SE3` (core/geometry/pinhole_transforms.py:3,29,51; core/pose/pose_estimator.py:81-91;
 * core/optimization/declerative_node_lie.py:233-234).  Pose = 7 scalars [tx ty tz qx qy qz qw]; tangent =
 * 6 scalars [tau(3) phi(3)].  dtype = RPE_F32 | RPE_F64 for every pointer of the call.
 * --------------------------------------------------------------------------------------------------------- */
int rpe_se3_exp(const void *xi, void *T, int64_t n, int dtype, void *stream);            /* (n,6) -> (n,7)   */
int rpe_se3_log(const void *T, void *xi, int64_t n, int dtype, void *stream);            /* (n,7) -> (n,6)   */
int rpe_se3_mul(const void *A, const void *B, void *C, int64_t n, int dtype, void *stream); /* C = A * B     */
int rpe_se3_inv(const void *T, void *Tinv, int64_t n, int dtype, void *stream);
/* T (n,7) acts on pts (n,m,3) -> out (n,m,3): `T * pts` with the (n,1) pose broadcast over m points.      */
int rpe_se3_act(const void *T, const void *pts, void *out, int64_t n, int64_t m, int dtype, void *stream);
/* Trajectory chaining of core/pose/pose_estimator.py:90-91 as an inclusive scan over m relative poses:
 * P_k = P_{k-1} * inv(scale(rel_k, s)), P_{-1} = init (7 scalars, may be NULL = identity). f64 or f32.    */
int rpe_se3_chain(const void *rel, const void *init, void *out, int64_t m, double scale, int dtype, void *stream);
/* The whole per-frame bookkeeping of PoseEstimator.forward (core/pose/pose_estimator.py:81-91) for m consecutive relative poses:
 * row k fails when any of its 7 scalars is NaN or any |log(rel_k)| > thr (:81) and is replaced by the identity (:83); then the chain
 * of rpe_se3_chain.  rel_out (m,7) = the gated relative poses (may be NULL), abs_out (m,7) = the chained absolute poses, ok (m) int32 =
 * 1 where the row passed (may be NULL).  Same arithmetic as rpe_se3_log / _inv / _mul step by step: bit-identical poses.            */
int rpe_pose_gate_chain(const void *rel, const void *init, void *rel_out, void *abs_out, int32_t *ok, int64_t m, double scale,
                        double thr, int dtype, void *stream);
/* rpe_pose_gate_chain for m INDEPENDENT rows (m sequences tracked side by side): row k is gated and chained onto ITS OWN init row,
 * init (m,7) (may be NULL = identity for every row), and gives the bits a rpe_pose_gate_chain call with m = 1 gives for it.          */
int rpe_pose_gate_chain_rows(const void *rel, const void *init, void *rel_out, void *abs_out, int32_t *ok, int64_t m, double scale,
                             double thr, int dtype, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Pose layer -- replaces DPoseSE3Head.objective / .solve (core/pose/pose_head.py:12-79) together with
 * torch.optim.LBFGS, transform/project (core/geometry/pinhole_transforms.py:28-30,90-99) and
 * DeclarativeFunctionLie.forward (core/optimization/declerative_node_lie.py:223-247).
 *
 * Inputs (all float32 unless noted), n rows, H*W pixels each:
 *   flow (n,2,H,W)  pcl1 (n,3,H,W)  pcl2 (n,3,H,W)  w1 (n,1,H,W)  w2 (n,1,H,W)
 *   mask1, mask2 (n,1,H,W) uint8 (torch.bool storage, 0/1)   K (n,3,3)   loss_weight (n,2) = [w3d, w2d]
 * All arithmetic is float64, as in the reference (pose_head.py:64).
 * --------------------------------------------------------------------------------------------------------- */
/* Scratch bytes needed by rpe_pose_reduce / rpe_pose_solve for n rows of h*w pixels. */
size_t rpe_pose_workspace_bytes(int n, int h, int w);

/* One objective evaluation at poses T (n,7) f64.  out (n,32) f64 per row:
 *   [0] loss2d  [1] loss3d  [2] f = lw[1]*loss2d + lw[0]*loss3d  [3..8] g = df/dxi (left perturbation,
 *   unclipped)  [9..29] upper triangle of the Gauss-Newton Hessian H (row-major: 00 01 .. 05 11 12 .. 55;
 *   zeros unless need_hessian != 0)  [30],[31] reserved.                                                  */
int rpe_pose_reduce(const float *flow, const float *pcl1, const float *pcl2, const float *w1, const float *w2,
                    const uint8_t *mask1, const uint8_t *mask2, const float *K, const float *loss_weight,
                    const double *T, int n, int h, int w, int need_hessian, double *out, void *workspace,
                    void *stream);

/* Whole solve on the device, no host synchronisation: start at identity, run `iters` iterations of
 * `mode`, n independent rows.  Outputs: T_out (n,7) f64 group element; vec7 (n,7) f32 and log6 (n,6) f32
 * (the two tensors DeclarativeFunctionLie.forward returns); info (n,4) int32 = [n_iter, func_evals,
 * stop_reason, 0].  Any output pointer except T_out may be NULL.                                          */
int rpe_pose_solve(const float *flow, const float *pcl1, const float *pcl2, const float *w1, const float *w2,
                   const uint8_t *mask1, const uint8_t *mask2, const float *K, const float *loss_weight,
                   int n, int h, int w, int mode, int iters, double *T_out, float *vec7, float *log6,
                   int32_t *info, void *workspace, void *stream);

/* Same with torch.optim.LBFGS's remaining constructor arguments exposed (rpe_pose_solve uses its defaults
 * tolerance_grad=1e-7, tolerance_change=1e-9, history_size=100, which is how pose_head.py:70 builds the optimiser).
 * 1 <= history_size <= 100.  The tolerances also drive the Gauss-Newton step test. */
int rpe_pose_solve_opts(const float *flow, const float *pcl1, const float *pcl2, const float *w1, const float *w2,
                        const uint8_t *mask1, const uint8_t *mask2, const float *K, const float *loss_weight,
                        int n, int h, int w, int mode, int iters, double tolerance_grad, double tolerance_change,
                        int history_size, double *T_out, float *vec7, float *log6, int32_t *info, void *workspace,
                        void *stream);

/* The same with the options in a sized struct: struct_size = sizeof(rpe_solve_opts) of the header the caller was built against.  The library
 * accepts any struct_size >= the layout it knows (fields are only ever appended, so a newer caller's longer struct carries this layout as
 * its prefix) and returns RPE_E_BADARG for a shorter one; a field appended later is read only when struct_size covers it and takes its
 * documented default otherwise.
 *   partition_rows: the pixel reduction sums per-block partials in a fixed order, and the number of blocks per row is chosen so that
 *   ONE round of workgroups covers the batch -- so a row's float64 sums are grouped differently in a 16-row launch than alone.
 *   0 = that default; p > 0 = the partition a p-row batch would get.  With p = 1 every row's iterates are bit-identical to solving
 *   it alone, whatever the batch (what the chunked sequence tracker asks for: core/pose/pose_estimator.py:98-125 solves one frame at
 *   a time).  rpe_pose_workspace_bytes covers every choice. */
typedef struct rpe_solve_opts {
    int struct_size;             /* sizeof(rpe_solve_opts) */
    int history_size;            /* 1..100 (torch.optim.LBFGS default 100) */
    double tolerance_grad;       /* 1e-7 */
    double tolerance_change;     /* 1e-9 */
    int partition_rows;          /* 0 = n */
    int reserved;                /* flags; 0 = defaults.  RPE_SOLVE_LAUNCH_PER_EVALUATION (bit 0): one launch per evaluation even where the whole
                                  * solve would run as one persistent launch (identical results; for A/B measurements) */
} rpe_solve_opts;
/* Concurrent solves.  The one persistent launch is chosen when ITS grid fits the device's resident workgroups; its workgroups then wait
 * for their row's tail without giving up their slots.  Persistent solves running at the same time (on several streams, in this process or
 * in another) whose grids TOGETHER exceed the device can each hold part of a row with no row of either complete, and starve each other
 * until the wait's bound gives up -- with a wrong pose and a normal stop code.  A caller that runs several solves at once passes
 * RPE_SOLVE_LAUNCH_PER_EVALUATION (bit-identical results), unless it keeps their combined grids within the device. */
#define RPE_SOLVE_LAUNCH_PER_EVALUATION 1
int rpe_pose_solve_ex(const float *flow, const float *pcl1, const float *pcl2, const float *w1, const float *w2,
                      const uint8_t *mask1, const uint8_t *mask2, const float *K, const float *loss_weight,
                      int n, int h, int w, int mode, int iters, const rpe_solve_opts *opts, double *T_out, float *vec7,
                      float *log6, int32_t *info, void *workspace, void *stream);

/* Solve-quality report (opt-in; not part of any solve): everything a consumer of the pose needs to judge HOW WELL a frame was solved,
 * evaluated in float64 at a given pose T (n,7) f64 -- normally the pose rpe_pose_solve* returned.  Inputs as rpe_pose_reduce; the gates are
 * those of the objective (core/pose/pose_head.py:12-58): the reprojection term keeps a pixel unless its weighted residual is NaN / Inf, its
 * flow target leaves the image or mask1 is false; the 3-D term keeps mask1 & mask2; depth is clamped at 1e-12 -- handled exactly as
 * rpe_pose_reduce handles them.  out (n,64) f64 per row:
 *   [0]      n2d   pixels the reprojection term keeps
 *   [1]      n3d   pixels the 3-D term keeps
 *   [2] [3]  sum of w1 over the kept 2-D pixels, sum of w2 over the kept 3-D pixels
 *   [4] [5]  sum w1 (ex^2 + ey^2), sum w2 |e3|^2 over the kept pixels (= loss2d (hw)^2, loss3d hw)
 *   [6] [7]  unweighted RMS of the kept residuals: sqrt(sum (ex^2 + ey^2) / n2d) in pixels, sqrt(sum |e3|^2 / n3d) in the solve's
 *            (normalised) units; 0 / 0 gives NaN
 *   [8]      f = lw[1] loss2d + lw[0] loss3d
 *   [9]      max |g|, g unclipped
 *   [10..15] g = df/dxi (left perturbation, xi = (tau, phi))
 *   [16..51] C (6x6, row-major), see below
 *   [52]     pd: 1 if the Cholesky factorisation of H succeeded and m > 6 and f is finite, else 0; when 0, C is all NaN
 *   [53]     m = 2 n2d + 3 n3d, the number of scalar residuals
 *   [54..63] zero, reserved
 * C = (2 f / (m - 6)) H^-1 with H the Gauss-Newton Hessian of rpe_pose_reduce (H = 2 J^T W J, f = sum W r^2): the usual
 * sigma^2 (J^T W J)^-1 with sigma^2 = f / (m - 6), i.e. the FORMAL covariance of the weighted least-squares fit in the left tangent
 * (tau, phi) of T.  It is invariant to a common scale of the weights and says how well the data constrain the pose under the fit's own
 * noise model; how it is calibrated against true pose error depends on the trained weight heads and cannot be measured with the seeded
 * weights this repository ships -- treat it as a relative measure between frames until it has been calibrated on real weights.
 * A NaN residual that the gate removes still reaches g (0 * NaN, as in the reference's autograd), not f, H or C.
 * Two launches on `stream`: a streaming pass whose workgroups write partial sums, and one workgroup per row that adds them in index order,
 * factors and inverts H.  The pixel partition depends on (h, w) only, so a row's 64 slots do not depend on the batch, bit for bit.
 * workspace: rpe_pose_quality_workspace_bytes(n, h, w) bytes.  Status codes as rpe_pose_reduce. */
size_t rpe_pose_quality_workspace_bytes(int n, int h, int w);
int rpe_pose_quality(const float *flow, const float *pcl1, const float *pcl2, const float *w1, const float *w2,
                     const uint8_t *mask1, const uint8_t *mask2, const float *K, const float *loss_weight,
                     const double *T, int n, int h, int w, double *out, void *workspace, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Backward of the declarative pose layer (training): replaces DeclarativeNodeLie.gradient /
 * _get_objective_derivatives (core/optimization/declerative_node_lie.py:13-82,106-126; called from
 * DeclarativeFunctionLie.backward :249-267), which differentiates the objective twice with autograd, by the closed
 * forms of fY, fYY and fXY^T u (csrc/pose_backward.hip).  Inputs as rpe_pose_reduce; T (n,7) f64 = the layer's output
 * pose (the reference uses its float32 vec7).
 *   rpe_pose_backward_moments: out (n,48) f64 = [g2u(6) | g3u(6) | H(6x6 row-major)]: tangent gradients of the
 *       reprojection / 3-D terms with unit loss weight (fY = lw[1] g2u + lw[0] g3u; d fY/d loss_weight) and
 *       H = (fYY + fYY^T)/2 as the reference forms it (:51).  workspace: rpe_pose_backward_workspace_bytes(n,h,w).
 *   rpe_pose_backward_grads:   given u (n,6) f64 = -H^-1 v, writes fXY^T u for flow (n,2,h,w), pcl1, pcl2 (n,3,h,w),
 *       w1, w2 (n,1,h,w), float32, NaN -> 0 (:76); any output pointer may be NULL.
 * The 6x6 solve, the optimality test |fY| <= eps (:43-47) and d/d loss_weight = (u.g3u, u.g2u) stay on the host side. */
size_t rpe_pose_backward_workspace_bytes(int n, int h, int w);
int rpe_pose_backward_moments(const float *flow, const float *pcl1, const float *pcl2, const float *w1, const float *w2,
                              const uint8_t *mask1, const uint8_t *mask2, const float *K, const float *loss_weight,
                              const double *T, int n, int h, int w, double *out, void *workspace, void *stream);
int rpe_pose_backward_grads(const float *flow, const float *pcl1, const float *pcl2, const float *w1, const float *w2,
                            const uint8_t *mask1, const uint8_t *mask2, const float *K, const float *loss_weight,
                            const double *T, const double *u, int n, int h, int w, float *grad_flow, float *grad_pcl1,
                            float *grad_pcl2, float *grad_w1, float *grad_w2, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Stereo depth, back-projection, flow warps and the 1/8 stacks of the weight heads -- replaces
 * core/pose/pose_net.py:73-79 (depth from disparity, validity, proj), :104-108 (remap_from_flow x3,
 * remap_from_flow_nearest; core/interpol/flow_utils.py:4-26) and :110-113 (bilinear x0.125 of the two
 * 8-channel stacks) in ONE pass.  h and w must be multiples of 8.
 *
 *   in : stereo_flow2 (n,2,h,w)  time_flow (n,2,h,w)  baseline (n)  K (n,3,3)  depth1 (n,1,h,w)
 *        image1l, image2l (n,3,h,w)  stereo_flow1 (n,2,h,w)  mask2 (n,1,h,w) u8
 *   out: depth2 (n,1,h,w)  mask2_valid (n,1,h,w) u8 = mask2 & (0 < depth <= 1)   [pose_net.py:75-77]
 *        pcl1 (n,3,h,w)  pcl2w (n,3,h,w) = remap_from_flow(proj(depth2), time_flow)
 *        mask2w (n,1,h,w) u8 = valid_mapping & remap_nearest(mask2_valid)           [pose_net.py:107-108]
 *        inp1 (n,8,h/8,w/8) = down8(cat(stereo_flow1, image1l, pcl1))
 *        inp2 (n,8,h/8,w/8) = down8(cat(warp(stereo_flow2), warp(image2l), pcl2w))
 *        pcl2 (n,3,h,w) un-warped cloud, may be NULL
 * --------------------------------------------------------------------------------------------------------- */
int rpe_depth_backproject_warp(const float *stereo_flow2, const float *time_flow, const float *baseline,
                               const float *K, const float *depth1, const float *image1l, const float *image2l,
                               const float *stereo_flow1, const uint8_t *mask2, int n, int h, int w,
                               float *depth2, uint8_t *mask2_valid, float *pcl1, float *pcl2w, uint8_t *mask2w,
                               float *inp1, float *inp2, float *pcl2, void *stream);

/* flow2depth of core/pose/pose_net.py:127-135 (first frame): depth (n,1,h,w), valid (n,1,h,w) u8. */
int rpe_flow2depth(const float *stereo_flow, const float *baseline, int n, int h, int w, float *depth,
                   uint8_t *valid, void *stream);

/* Integer sampling taps of the two warps for index-parity tests: x0,y0 = floor (bilinear), xn,yn =
 * round-half-even (nearest) of the un-normalised grid_sample position.  Each (n,h,w) int32.            */
int rpe_warp_taps(const float *flow, int n, int h, int w, int32_t *x0, int32_t *y0, int32_t *xn, int32_t *yn,
                  void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Backward of rpe_depth_backproject_warp (training): the adjoint of core/pose/pose_net.py:73-79,104-113 and
 * core/interpol/flow_utils.py:4-14, from the gradients of pcl1, pcl2w, inp1 and inp2 to the three flows and depth1.
 *
 *   in : the forward's stereo_flow2, time_flow, baseline, K, depth1, image2l, stereo_flow1, mask2 and n, h, w (h, w multiples of 8).
 *        depth1, stereo_flow1 and mask2 are not read (the stage is linear in the first two, and masks carry no gradient); they are
 *        required all the same, so that the call names the forward it differentiates.
 *        grad_pcl1, grad_pcl2w (n,3,h,w), grad_inp1, grad_inp2 (n,8,h/8,w/8): the incoming gradients; any may be NULL = zero.
 *   out: grad_time_flow, grad_stereo_flow2, grad_stereo_flow1 (n,2,h,w), grad_depth1 (n,1,h,w); any may be NULL = not wanted (the
 *        others are the same bits).  Every wanted output is written in full.
 *   - down8: grad_inp* / 4 lands on the 2x2 pixels at offsets 3, 4 of each 8x8 cell.  inp1 channels 0-1 -> grad_stereo_flow1, 2-4 (the
 *     image) nowhere, 5-7 join grad_pcl1; grad_depth1 = <that, K^-1 [x+.5, y+.5, 1]>.
 *   - the bilinear warp by time_flow (grid_sample, align_corners=True, zero padding) of stereo_flow2 (2), image2l (3), pcl2 (3):
 *     grad_time_flow = sum over the 8 channels of g * d(sample)/d(ix, iy), torch's convention (tap differences, a tap outside the image
 *     reads as zero, d ix / d flow.x = 1); a position that does not read (NaN, or beyond +-1e6: rpe_warp_taps) gives 0.
 *     The value gradient g * tap weight is summed per SOURCE pixel into grad_stereo_flow2 (both channels) and the pcl2 gradient.
 *   - pcl2 = depth2 * ray, depth2 = baseline / -sf2.x, replaced by 1 where !(0 < depth2 <= 1) (the forward's float32 test):
 *     grad_stereo_flow2.x += <grad pcl2, ray> * baseline / sf2.x^2 where valid, 0 where clamped.  mask2 does not gate this.
 *   Sampling positions and taps are the forward's (float32, rpe_warp_taps); the sums behind them are float64, rounded once.
 *   The scatter uses no float atomics: taps are counted per source pixel (integer atomics), the counts scanned, the per-source lists
 *   filled and each list sorted and summed in destination-index order -- bit-identical from run to run, and a row's result does not
 *   depend on its batch.  One source pixel's list is sorted and summed by one thread: a flow that sends a large share of an image to
 *   one pixel serialises on it (n log n in the list length).
 *   workspace: rpe_depth_backproject_warp_backward_workspace_bytes(n, h, w) bytes (0 for non-positive sizes), 16-byte aligned like every
 *   (n,2|3,h,w) pointer of the call (RPE_E_BADARG otherwise).  NULL required pointers, h % 8, w % 8, non-positive h / w, n < 0 and n > 65535 (a row is
 *   one grid line of the launches; rpe_flow2depth_backward has the same limit) return RPE_E_BADARG before any launch; h*w >= 2^29 returns RPE_E_UNSUPPORTED; n == 0 is RPE_OK.
 * rpe_flow2depth_backward: the same disparity adjoint for rpe_flow2depth (the first frame's depth1): grad_stereo_flow (n,2,h,w) with
 *   .x = grad_depth * baseline / sf.x^2 where the depth is valid, 0 where it was clamped, .y = 0.  Any h, w.
 * --------------------------------------------------------------------------------------------------------- */
size_t rpe_depth_backproject_warp_backward_workspace_bytes(int n, int h, int w);
int rpe_depth_backproject_warp_backward(const float *stereo_flow2, const float *time_flow, const float *baseline,
                                        const float *K, const float *depth1, const float *image2l,
                                        const float *stereo_flow1, const uint8_t *mask2, int n, int h, int w,
                                        const float *grad_pcl1, const float *grad_pcl2w, const float *grad_inp1,
                                        const float *grad_inp2, float *grad_time_flow, float *grad_stereo_flow2,
                                        float *grad_stereo_flow1, float *grad_depth1, void *workspace, void *stream);
int rpe_flow2depth_backward(const float *stereo_flow, const float *baseline, const float *grad_depth, int n, int h, int w,
                            float *grad_stereo_flow, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Backward of RAFT's output heads (csrc/raft_backward.hip): the tail of the last update iteration,
 *     t_f = relu(conv3x3(net; fh.conv1)), delta = conv3x3(t_f; fh.conv2), t_m = relu(conv3x3(net; mask.0)),
 *     m = 0.25 conv1x1(t_m; mask.2), flow_up = upsample_convex(flow_prev + delta, m)
 * (core/RAFT/core/update.py FlowHead, BasicUpdateBlock.mask; core/RAFT/core/raft.py upsample_flow).  f32, NCHW.  No float atomics; every
 * sum runs in an order fixed by the shapes alone: two runs give the same bits, on any device.
 * rpe_upsample_convex_backward: from grad_up (b,2,8 h8,8 w8; 16-byte aligned), flow (b,2,h8,w8) and mask (b,576,h8,w8) -- the logits exactly
 *   as rpe_upsample_convex reads them -- d_flow (b,2,h8,w8) and d_mask (b,576,h8,w8), both written in full.  Gather form: d_flow at a cell
 *   collects from the nine cells whose 3x3 window (zero padded, as the forward's unfold) holds it; d_mask_k = p_k (g_k - sum_k' p_k' g_k') per
 *   sub-pixel with the forward's softmax code (double).  Dense tensors; any h8, w8; b == 0 is RPE_OK, b > 65535 RPE_E_BADARG.
 * rpe_conv_bwd_weight: d_weight (cout,cin,kh,kw) and d_bias (cout) (either may be NULL) of y = conv(x; W) + bias, stride 1, 'same' zero
 *   padding, (kh,kw) = (3,3), (1,1), (1,5), (5,1) or (7,7), from x (b,cin,h,w) and dy (b,cout,h,w) at ANY h, w; x and dy may be channel slices (batch strides in
 *   floats, at least the slice).  A GEMM on the f32 matrix cores (v_mfma_f32_32x32x2_f32) with M = cout, N = cin kh kw, K = b h w; layers of one
 *   or two output channels run a plain kernel (3x3 and 1x1; the other sizes run the GEMM at any cout).  K is split into chunks of c(K) = max(1024, round_up(ceil(K / 64), 32)) pixels -- at most 64, a
 *   function of b h w alone --, each chunk writes a partial and the partials are added in index order in f64; d_bias is dy's channel sum under
 *   the same rule; both leave multiplied by ``scale`` (the mask head's 0.25; 1 otherwise), applied to the f64 sum.  workspace: rpe_conv_bwd_weight_workspace_bytes(...) bytes (0 for a shape it refuses), 16-byte aligned.  Non-positive
 *   sizes, other kernels, NULL x / dy / workspace: RPE_E_BADARG; b h w, cin h w, cout h w or the weight's size >= 2^31: RPE_E_UNSUPPORTED.
 * rpe_conv3x3_to2_bwd_data: the data gradient of rpe_conv3x3_to2 (weight (2,c,3,3)): dx (b,c,h,w) = conv(dy (b,2,h,w); W transposed and
 *   flipped), multiplied by [act > 0] when act (b,c,h,w: the ReLU output that was the layer's input) is given.  Channel slices throughout.
 * rpe_relu_backward: out = act > 0 ? grad : 0 on (b,c,hw) channel slices; out may be grad.
 * rpe_sum_groups: out (b,c,hw; a channel slice) = act(sum_g parts[g] + bias[c]) for parts (groups,b,c,hw) dense, added in group order in f64,
 *   bias may be NULL, relu 0 / 1.  The forward convolution kernels add in one k-ordered f32 chain; the tail runs them on groups of input
 *   channels and adds the groups here, which keeps its results at the error of a blocked float32 sum.
 * --------------------------------------------------------------------------------------------------------- */
int rpe_upsample_convex_backward(const float *grad_up, const float *flow, const float *mask, int b, int h8, int w8, float *d_flow,
                                 float *d_mask, void *stream);
size_t rpe_conv_bwd_weight_workspace_bytes(int b, int cin, int cout, int h, int w, int kh, int kw);
int rpe_conv_bwd_weight(const float *x, long long x_batch_stride, const float *dy, long long dy_batch_stride, int b, int cin, int cout,
                        int h, int w, int kh, int kw, float scale, float *d_weight, float *d_bias, void *workspace, void *stream);
int rpe_conv3x3_to2_bwd_data(const float *dy, long long dy_batch_stride, const float *weight, const float *act,
                             long long act_batch_stride, int b, int c, int h, int w, float *dx, long long dx_batch_stride, void *stream);
int rpe_relu_backward(const float *grad, long long grad_batch_stride, const float *act, long long act_batch_stride, int b, int c, int hw,
                      float *out, long long out_batch_stride, void *stream);
int rpe_sum_groups(const float *parts, int groups, int b, int c, int hw, const float *bias, int relu, float *out, long long out_batch_stride,
                   void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Backward of one update-block application (csrc/update_backward.hip; core/RAFT/core/update.py SepConvGRU): the adjoints of the gate
 * epilogues rpe_gru_gates_zr / rpe_gru_gates_h for ONE half,  h' = (1 - z) h + z q,  z = s(z_pre), r = s(r_pre), q = tanh(q_pre), rh = r h.
 * All operands are (b,c,hw) f32 channel slices (batch strides in floats, at least c hw); z, r, q are the POST-activation values.
 * rpe_gru_gates_zq_backward: from d_h_new = d loss / d h':  d_z_pre = d (q - h) z (1 - z),  d_q_pre = d z (1 - q^2),  d_h = d (1 - z).
 * rpe_gru_gates_r_backward: from d_rh = d loss / d (r h) (convq's data gradient):  d_r_pre = d_rh h r (1 - r),  d_h_out = d_h_in + d_rh r;
 *   d_h_out may be d_h_in or d_rh (in place).  Products in double, one rounding per result; a saturated gate gives exact zeros.
 * rpe_gru_gates_zr_recompute / _h_recompute: the gates again with everything the adjoints read kept (the forward's epilogues keep z and r h
 *   only): from zr_pre (b,2c,hw: z | r, bias added) and h:  z, r, rh = r h;  from q_pre, z and h:  q = tanh(q_pre), h_new = (1 - z) h + z q.
 *   Activations in double, rounded once.
 * The weight and data gradients of the step's convolutions are rpe_conv_bwd_weight and forward convolutions on transposed weights.
 * b == 0 is RPE_OK; NULL, b > 65535, c or hw <= 0, a batch stride shorter than the slice: RPE_E_BADARG.
 * --------------------------------------------------------------------------------------------------------- */
int rpe_gru_gates_zr_recompute(const float *zr_pre, long long zr_batch_stride, const float *h, long long h_batch_stride, int b, int c, int hw,
                               float *z, long long z_batch_stride, float *r, long long r_batch_stride, float *rh, long long rh_batch_stride,
                               void *stream);
int rpe_gru_gates_h_recompute(const float *q_pre, long long qp_batch_stride, const float *z, long long z_batch_stride, const float *h,
                              long long h_batch_stride, int b, int c, int hw, float *q, long long q_batch_stride, float *h_new,
                              long long hn_batch_stride, void *stream);
int rpe_gru_gates_zq_backward(const float *d_h_new, long long d_batch_stride, const float *h, long long h_batch_stride, const float *z,
                              long long z_batch_stride, const float *q, long long q_batch_stride, int b, int c, int hw, float *d_z_pre,
                              long long dz_batch_stride, float *d_q_pre, long long dq_batch_stride, float *d_h, long long dh_batch_stride,
                              void *stream);
int rpe_gru_gates_r_backward(const float *d_rh, long long drh_batch_stride, const float *h, long long h_batch_stride, const float *r,
                             long long r_batch_stride, const float *d_h_in, long long dhi_batch_stride, int b, int c, int hw, float *d_r_pre,
                             long long dr_batch_stride, float *d_h_out, long long dho_batch_stride, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Backward of the correlation (csrc/corr_backward.hip; core/RAFT/core/corr.py CorrBlock), f32 pyramid route.  Upstream detaches coords1, so
 * the lookup coordinates are constants: the window is linear in the pyramid, the pyramid bilinear in (fmap1, fmap2); the gradient is exact.
 * The gradient volume G = d loss / d pyramid is a dense f32 (b, h8 w8, S) tensor, S = sum_l h_l w_l with h_l = h8 >> l, w_l = w8 >> l (the
 *   pyramid's level sizes, every level at least 2 x 2): row p holds the levels' maps of query p one after the other, each row-major.
 *   S h8 w8 4 bytes per pair: 139 MB at 640 x 512 (h8 w8 = 5120, S = 6800), 2.2 GB at 1280 x 1024.  rpe_corr_grad_volume_floats: its size,
 *   0 for a geometry the pyramid refuses.
 * rpe_corr_lookup_backward: G += the adjoint of ONE rpe_corr_lookup at coords (b,2,h8,w8) from d_corr (b, levels 81, h8, w8), the gradient
 *   of the looked-up window (channel l 81 + i 9 + j samples level l at (x + i - r, y + j - r): upstream's transposed window order).  The
 *   integer taps and fractions are the forward's (the function behind rpe_corr_lookup_taps); a cell is the sum of its (at most four non-zero)
 *   weight x gradient terms in one fixed order; cells outside a level are dropped (zero padding).  One wave owns a query's row: no atomics;
 *   calls accumulate in stream order; bit-identical from run to run and independent of the batch.  The caller zero-fills G.  radius == 4.
 * rpe_corr_build_backward: d_fmap1, d_fmap2 (b,c,h8,w8) from G and the feature maps.  With F2cat (c x S) = fmap2 followed by its
 *   successively 2x2-pooled copies (floor: a last odd row / column is dropped, as avg_pool2d does):
 *       d_fmap1 = F2cat G^T / sqrt(c),   dF2cat = fmap1 G / sqrt(c),   d_fmap2 = dF2cat's level 0 + the pool adjoints of the levels above,
 *   applied from the last level down to 0 (a quarter to each covered cell, nothing to a dropped row or column).  The GEMMs run on the f32
 *   matrix cores (v_mfma_f32_32x32x2_f32); the contraction axis K (S, then h8 w8) is split into chunks of max(512, round_up(ceil(K / 8), 32))
 *   -- a function of the shape alone --, the partials are added in chunk order in f64 and scaled there.  No float atomics.  c: a multiple of
 *   4 up to 256.  d_f2cat (b,c,S) may be NULL (it then lives in the workspace).  workspace: rpe_corr_build_backward_workspace_bytes(...) bytes
 *   (0 for a shape it refuses), 16-byte aligned.
 * NULL, a refused geometry or c, radius != 4, b > 65535: RPE_E_BADARG.
 * --------------------------------------------------------------------------------------------------------- */
size_t rpe_corr_grad_volume_floats(int b, int h8, int w8, int levels);
int rpe_corr_lookup_backward(const float *coords, const float *d_corr, int b, int h8, int w8, int levels, int radius, float *grad_volume,
                             void *stream);
size_t rpe_corr_build_backward_workspace_bytes(int b, int c, int h8, int w8, int levels);
int rpe_corr_build_backward(const float *grad_volume, const float *fmap1, const float *fmap2, int b, int c, int h8, int w8, int levels,
                            float *d_fmap1, float *d_fmap2, float *d_f2cat, void *workspace, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Backward of RAFT's encoders (csrc/encoder_backward.hip; core/RAFT/core/extractor.py BasicEncoder, ResidualBlock): what the stride-1
 * entry points above do not cover.  f32, NCHW, channel slices (batch strides in floats, at least the slice).  No float atomics; every sum
 * runs in an order fixed by the shapes alone: two runs give the same bits, on any device.  Any map size.
 * The three STRIDE-2 forms: kernel k = 3 (padding 1), 1 (padding 0) and 7 (padding 3, the stem), ho = (hi + 2 (k / 2) - k) / 2 + 1 and
 *   wo likewise; any other k, or ho / wo that do not follow from hi / wi: RPE_E_BADARG (workspace query: 0).
 * rpe_conv_s2_bwd_weight: d_weight (cout,cin,k,k) and d_bias (cout) (either may be NULL) of y = conv(x; W, stride 2) + bias from
 *   x (b,cin,hi,wi) and dy (b,cout,ho,wo): rpe_conv_bwd_weight's GEMM (v_mfma_f32_32x32x2_f32, the same tile) with M = cout, N = cin k k,
 *   K = b ho wo, the same chunks c(K) = max(1024, round_up(ceil(K / 64), 32)) added in index order in f64, ``scale`` applied to the f64
 *   sum; a staged pixel reads x at (2 py + ty - k/2, 2 px + tx - k/2), border taps from a clamped address, selected to zero.  d_bias is
 *   rpe_conv_bwd_weight's bias sum on dy.  workspace: rpe_conv_s2_bwd_weight_workspace_bytes(...) bytes, 16-byte aligned.  NULL x / dy /
 *   workspace, non-positive sizes: RPE_E_BADARG; b ho wo, cin hi wi, cout ho wo or the weight's size >= 2^31: RPE_E_UNSUPPORTED.
 * rpe_conv_s2_bwd_data: dx (b,cin,hi,wi) of the k = 3 and k = 1 forms from dy and weight (cout,cin,k,k), in gather form: an input pixel
 *   adds only the taps whose parity reaches it (1, 2, 2 or 4 at 3x3; one pixel in four at 1x1) and is an exact zero where none does; no
 *   zero-inserted copy of dy exists.  The sum over (cout, taps) runs in f64 in one fixed order and is rounded once.  k = 7: RPE_E_BADARG
 *   (images are not trained).  b == 0 is RPE_OK.
 * rpe_bn_frozen_backward: the adjoint of y = s (z + conv_bias - mean) + beta, s = gamma / sqrt(var + eps), with (mean, var) the running
 *   statistics (constants), from dy (b,c,hw; behind the ReLU mask) and the raw convolution output z:  d_beta = S0 = sum dy,
 *   d_gamma = (sum dy z + (conv_bias - mean) S0) / sqrt(var + eps),  d_conv_bias = s S0,  dz (b,c,hw) = s dy (may be dy).  The two sums run
 *   over K = b hw in chunks of c(K), threads and waves in a fixed tree, chunks in index order, all f64.  conv_bias and every output may be
 *   NULL.  workspace: rpe_bn_frozen_backward_workspace_bytes(b, c, hw) bytes, 16-byte aligned.  b <= 0 or > 65535, c > 65535: RPE_E_BADARG.
 * rpe_instnorm_backward: the adjoint of y = (z - mean) / sigma per (b,c) plane, sigma = sqrt(biased var + eps), no affine parameters:
 *   dz = (dy - mean(dy) - xh mean(dy xh)) / sigma, xh = (z - mean) / sigma.  The four plane moments in f64 (one workgroup per plane, fixed
 *   tree), then a pass that applies them; a NaN stays inside its plane.  dz may be dy.  (A bias added in front of the norm cancels: its
 *   gradient is zero.)  b == 0 is RPE_OK.
 * rpe_split_act_backward: out = grad (1 - act^2) on channels [0, half) (tanh) and act > 0 ? grad : 0 on [half, c) (ReLU), act = the
 *   activated output (the context encoder's net | inp); products in f64, rounded once; out may be grad.
 * --------------------------------------------------------------------------------------------------------- */
size_t rpe_conv_s2_bwd_weight_workspace_bytes(int b, int cin, int cout, int hi, int wi, int ho, int wo, int k);
int rpe_conv_s2_bwd_weight(const float *x, long long x_batch_stride, const float *dy, long long dy_batch_stride, int b, int cin, int cout,
                           int hi, int wi, int ho, int wo, int k, float scale, float *d_weight, float *d_bias, void *workspace,
                           void *stream);
int rpe_conv_s2_bwd_data(const float *dy, long long dy_batch_stride, const float *weight, int b, int cin, int cout, int hi, int wi, int ho,
                         int wo, int k, float *dx, long long dx_batch_stride, void *stream);
size_t rpe_bn_frozen_backward_workspace_bytes(int b, int c, int hw);
int rpe_bn_frozen_backward(const float *dy, long long dy_batch_stride, const float *z, long long z_batch_stride, const float *gamma,
                           const float *conv_bias, const float *mean, const float *var, double eps, int b, int c, int hw, float *d_gamma,
                           float *d_beta, float *d_conv_bias, float *dz, long long dz_batch_stride, void *workspace, void *stream);
int rpe_instnorm_backward(const float *dy, long long dy_batch_stride, const float *z, long long z_batch_stride, int b, int c, int hw,
                          double eps, float *dz, long long dz_batch_stride, void *stream);
int rpe_split_act_backward(const float *grad, long long grad_batch_stride, const float *act, long long act_batch_stride, int b, int c,
                           int half, int hw, float *out, long long out_batch_stride, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * RAFT correlation -- replaces CorrBlock (core/RAFT/core/corr.py of the aimi-lab/RAFT submodule: all-pairs
 * correlation / sqrt(C), 4-level 2x2 average-pool pyramid, radius-r bilinear window lookup), called from
 * RAFT.forward (call sites core/pose/pose_net.py:47,65,129).
 *
 * The pyramid is an opaque device buffer owned by the caller; its internal layout (f32; the maps of 8 x-neighbouring
 * queries interleaved and skewed) is private to build/lookup.
 * --------------------------------------------------------------------------------------------------------- */
size_t rpe_corr_pyramid_bytes(int b, int h8, int w8, int levels);
/* the same for a given feature_dtype of rpe_corr_build_ex: RPE_F32 / RPE_F16 need rpe_corr_pyramid_bytes; the RPE_F32X3 experiment keeps
 * both feature maps as three bf16 planes and needs more scratch -- a pyramid that rpe_corr_build_ex(..., RPE_F32X3) writes MUST have been
 * sized with this function and RPE_F32X3 (the library sees only the pointer; the Python binding checks the buffer length) */
size_t rpe_corr_pyramid_bytes_ex(int b, int h8, int w8, int levels, int feature_dtype);
/* fmap1, fmap2: (b,c,h8,w8) f32.  Computes corr[b,q1,q2] = <fmap1[:,q1], fmap2[:,q2]> / sqrt(c) and the
 * average-pooled levels. */
int rpe_corr_build(const float *fmap1, const float *fmap2, int b, int c, int h8, int w8, int levels,
                   void *pyramid, void *stream);
/* Same with the precision of the feature maps selectable: feature_dtype = RPE_F32 (as rpe_corr_build) or RPE_F16 =
 * "fp16 features" (BASELINE config 5; RAFT's mixed_precision encoders hand fp16 feature maps to corr.py, which calls
 * .float() on them): both maps are rounded to fp16 (round to nearest even), the products run on the 16-bit matrix cores
 * with f32 accumulation (exact products, f32 sums) and the pyramid stays f32.  c % 16 == 0.
 * RPE_F32X3 (experiment switch): f32 maps, each f32 product evaluated as six bf16 products of an exact three-way split of both factors,
 * f32 accumulation -- f32-equivalent results (csrc/corr.hip, k_corr_build_x3). */
int rpe_corr_build_ex(const float *fmap1, const float *fmap2, int b, int c, int h8, int w8, int levels, int feature_dtype,
                      void *pyramid, void *stream);
/* coords (b,2,h8,w8) f32 (channel 0 = x, 1 = y) -> out (b, levels*(2r+1)^2, h8, w8) f32, channel order
 * level-major then window index i*(2r+1)+j with x offset (i-r) and y offset (j-r) (upstream's transposed
 * window).  radius must be 4, levels <= 4. */
int rpe_corr_lookup(const void *pyramid, const float *coords, int b, int h8, int w8, int levels, int radius,
                    float *out, void *stream);
/* The same lookup with coords and out living in LARGER maps: coords is the top-left h8 x w8 of (b, 2, map_h, map_w), out the top-left
 * h8 x w8 of (b, levels*(2r+1)^2, map_h, map_w); nothing outside that rectangle is read or written, so a zero-filled out keeps its zero
 * padding.  The pyramid, the taps and every value are those of rpe_corr_lookup on the true (h8, w8): bit-identical inside the rectangle.
 * map_h < h8 or map_w < w8 -> RPE_E_BADARG.  (The update loop on maps padded to the tuned kernels' sizes, core/RAFT/core/raft.py's loop.) */
int rpe_corr_lookup_ex(const void *pyramid, const float *coords, int b, int h8, int w8, int levels, int radius, int map_h, int map_w,
                       float *out, void *stream);
/* The lookup FUSED into the convolution that consumes it: out (b, 256, h8, w8) = act(convc1(lookup(coords))) without the 324-channel
 * tensor ever reaching memory -- BasicMotionEncoder.forward's first layer (upstream core/RAFT/core/update.py: cor = F.relu(self.convc1(corr)),
 * 1x1, 324 -> 256; the reference's call site is core/pose/pose_net.py:65).  A workgroup looks the four levels of 64 queries up into LDS
 * and contracts them on the f32 matrix cores; the products are added in rpe_conv1x1's order, so the result is BIT-IDENTICAL to
 * rpe_corr_lookup followed by rpe_conv1x1 (or rpe_conv_fused) with the same weights.  packed = rpe_corr_lookup_conv1x1_pack of the
 * (256, 324, 1, 1) weight (rpe_corr_lookup_conv1x1_packed_floats floats; 0 for any other shape); bias (256) or NULL; relu != 0: ReLU;
 * out / out2 (may be NULL): channel slices given by their batch strides (floats).  levels must be 4, radius 4, w8 % 8 == 0; anything else
 * -> RPE_E_UNSUPPORTED (the caller runs the two entry points).  Launches of at most one 64-query tile per compute unit run one workgroup per
 * tile (35 us against 45 for the two kernels at 2 pairs of 640x512); larger ones run persistent workgroups that look tile n + 1 up under the
 * matrix phase of tile n (315 us against 307 at 32 pairs: the f32 matrix pipe bounds both, so the two entry points remain the route for
 * large batches; measured in NOTES.md, round 6).  rpe_corr_lookup stays the stand-alone entry point (and the kernel the HBM roofline of
 * bench.py is stated on). */
size_t rpe_corr_lookup_conv1x1_packed_floats(int cout, int cin);
int rpe_corr_lookup_conv1x1_pack(const float *weight, int cout, int cin, float *packed, void *stream);
int rpe_corr_lookup_conv1x1(const void *pyramid, const float *coords, int b, int h8, int w8, int levels, int radius, const float *packed,
                            const float *bias, int relu, float *out, long long out_batch_stride, float *out2, long long out2_batch_stride,
                            void *stream);
/* Integer taps of the lookup for index-parity tests: x0,y0 (b,levels,2r+1,h8*w8) int32 = floor of the
 * un-normalised grid_sample position of window tap i on each axis (x0[..,i,q] pairs with x offset i-r,
 * y0[..,j,q] with y offset j-r) -- the very indices rpe_corr_lookup reads.  -1000000 marks a non-finite tap. */
int rpe_corr_lookup_taps(const float *coords, int b, int h8, int w8, int levels, int32_t *x0, int32_t *y0,
                         void *stream);
/* Diagnostic for the roofline claim of rpe_corr_lookup (bench.py): for these coordinates, per (batch item, level, group of 8
 * x-neighbouring queries) the number of staging rounds the lookup takes (1 = the group's eight windows fit one 12 x 16 box:
 * smooth flow) and the 128-B pyramid lines its loader requests.  rounds, lines: (b, levels, h8 * ceil(w8/8)) int32.  Same
 * tap / round arithmetic as the lookup kernel (shared device code), no pyramid access. */
int rpe_corr_lookup_rounds(const float *coords, int b, int h8, int w8, int levels, int32_t *rounds, int32_t *lines,
                           void *stream);
/* Copy one level of the pyramid out as a dense (b*h8*w8, h8>>l, w8>>l) f32 tensor (tests only). */
int rpe_corr_export_level(const void *pyramid, int b, int h8, int w8, int levels, int level, float *dense,
                          void *stream);

/* ---- Correlation WITHOUT the all-pairs volume (upstream RAFT's alternate_corr; csrc/corr_alt.hip).  The window of every query is
 * recomputed from the two feature maps at every lookup; what is kept between lookups is a scratch of pixel-major feature maps:
 * fmap1 / sqrt(c) and fmap2 with its levels - 1 pooled copies (2x2 mean, stride 2, sizes floored) -- pooling fmap2 and pooling the
 * correlation over its target axes are the same linear map.  f32 (fp16: the _ex / _dt forms below); c as rpe_corr_build takes it (a multiple of 16, <= 256).
 * rpe_corr_alt_bytes: bytes of the scratch; 0 for exactly the (b, h8, w8, levels) for which rpe_corr_pyramid_bytes_ex(.., RPE_F32) is 0
 * (and for a c the route does not take).  At most b c h8 w8 4 (1 + 4/3) bytes plus RPE_CORR_ALT_PAD bytes per level. */
#define RPE_CORR_ALT_PAD 512
size_t rpe_corr_alt_bytes(int b, int c, int h8, int w8, int levels);
/* Once per pass: fmap1, fmap2 (b,c,h8,w8) f32 -> scratch (rpe_corr_alt_bytes bytes, 16-byte aligned). */
int rpe_corr_alt_prepare(const float *fmap1, const float *fmap2, int b, int c, int h8, int w8, int levels, void *scratch, void *stream);
/* rpe_corr_lookup's contract on that scratch: coords (b,2,h8,w8) -> out (b, levels*(2r+1)^2, h8, w8) f32, the same channel order
 * (transposed window), zero for taps outside the level's map, integer taps and fractions from the arithmetic of rpe_corr_lookup_taps.
 * A query's values depend on its own coordinate and the feature maps of its pair only -- bit for bit, whatever its neighbours' flow
 * and whichever batch it is part of.  radius must be 4. */
int rpe_corr_alt_lookup(const void *scratch, const float *coords, int b, int c, int h8, int w8, int levels, int radius, float *out,
                        void *stream);
/* rpe_corr_alt_lookup with coords and out in (map_h, map_w) maps, as rpe_corr_lookup_ex. */
int rpe_corr_alt_lookup_ex(const void *scratch, const float *coords, int b, int c, int h8, int w8, int levels, int radius, int map_h, int map_w,
                           float *out, void *stream);
/* The same route with the precision of the scratch selectable (BASELINE config 5 on this route; upstream's AlternateCorrBlock under
 * autocast): feature_dtype = RPE_F32 forwards to the three functions above, bit for bit; RPE_F16 keeps the scratch in fp16 and runs the
 * window products on the 16-bit matrix cores (v_mfma_f32_32x32x16_f16, f32 accumulation); anything else -> RPE_E_BADARG (0 bytes).
 *   Layout (RPE_F16): as above -- pixel-major, a pixel's c channels contiguous and now 2 c bytes apart, the blocks F1, F2_0 .. F2_{levels-1}
 *     each rounded up to 256 bytes.
 *   Rounding: F1 = half(fmap1) and F2_0 = half(fmap2), round to nearest even, UNSCALED; F2_l (l >= 1) is pooled from the STORED fp16 F2_{l-1}:
 *     the four values converted to f32, summed in row-major order, times 0.25, rounded once to fp16 (upstream pools its fp16 maps level
 *     after level; sizes floored).  The lookup accumulates the c products of a window value in f32 in a fixed order and multiplies the sum by
 *     1 / sqrt(c) in f32, so a c that is no power of 4 loses nothing in the features.  Blend, taps, zeros outside the map, channel order
 *     and the bit-for-bit independence of a query from its neighbours and its batch are those of rpe_corr_alt_lookup.
 *   Bytes (RPE_F16): 0 exactly where rpe_corr_alt_bytes is 0; otherwise at least 2 (b c h8 w8 2) and at most b c h8 w8 2 (1 + 4/3) plus
 *     RPE_CORR_ALT_PAD bytes per level -- half of the f32 scratch up to that padding.
 * The argument checks are those of the f32 forms (null pointers, 16-byte alignment of the scratch, radius 4, the geometry rule,
 * map_h >= h8, map_w >= w8; b > 65535 -> RPE_E_UNSUPPORTED).  rpe_corr_alt_lookup_dt with map_h = h8, map_w = w8 is the dense lookup. */
size_t rpe_corr_alt_bytes_ex(int b, int c, int h8, int w8, int levels, int feature_dtype);
int rpe_corr_alt_prepare_ex(const float *fmap1, const float *fmap2, int b, int c, int h8, int w8, int levels, int feature_dtype, void *scratch,
                            void *stream);
int rpe_corr_alt_lookup_dt(const void *scratch, const float *coords, int b, int c, int h8, int w8, int levels, int radius, int map_h, int map_w,
                           int feature_dtype, float *out, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * RAFT update block, element-wise halves of SepConvGRU (core/RAFT/core/update.py) fused around the
 * convolutions, and the convex 8x up-sampling of RAFT.upsample_flow (core/RAFT/core/raft.py).
 * --------------------------------------------------------------------------------------------------------- */
/* zr_pre (b,2c,hw): pre-activations (WITHOUT bias; zr_bias (2c) and the tensor zr_add (b,2c,hw) are added here, either
 * may be NULL) of the z and r convolutions stacked on the channel axis.  zr_add carries the loop-invariant part of
 * the convolution: the context features `inp` are the same in all GRU iterations, so conv(inp-channels) is computed
 * once per RAFT pass and added here instead of being recomputed 12 times.  h is read from
 * channels [0,c) of a (b,h_channels,hw) buffer.  Writes z = sigmoid(zr_pre[:, :c]) to z_out (b,c,hw) and
 * r*h = sigmoid(zr_pre[:, c:]) * h into channels [0,c) of rh_out (b,rh_channels,hw), so rh_out can be the
 * (r*h | x) buffer the q convolution reads. */
int rpe_gru_gates_zr(const float *zr_pre, const float *zr_bias, const float *zr_add, const float *h, int h_channels,
                     int b, int c, int hw, float *z_out, float *rh_out, int rh_channels, void *stream);
/* h_out = (1 - z) * h + z * tanh(q_pre + q_add + q_bias[c]) (q_bias (c), q_add (b,c,hw) may be NULL); h_out may alias h.  h / h_out are channels [0,c) of buffers with
 * h_channels / hout_channels channels per batch row, so the new state lands straight in the (h|x) buffer. */
int rpe_gru_gates_h(const float *z, const float *q_pre, const float *q_bias, const float *q_add, const float *h,
                    int h_channels, int b, int c, int hw, float *h_out, int hout_channels, void *stream);
/* y = act(x + bias[c]) for x (b,c,hw): the bias add, ReLU (relu != 0) and the torch.cat / copy_ that follow a
 * convolution of the update block (core/RAFT/core/update.py BasicMotionEncoder / FlowHead), in one pass.  The result
 * goes to channels [out1_offset, out1_offset+c) of out1 (b,out1_channels,hw) and, if out2 != NULL, also to out2.
 * bias may be NULL; out1 may alias x when out1_channels == c. */
int rpe_bias_act(const float *x, const float *bias, int b, int c, int hw, int relu, float *out1, int out1_channels,
                 int out1_offset, float *out2, int out2_channels, int out2_offset, void *stream);
/* Encoder epilogues (core/RAFT/core/extractor.py ResidualBlock.forward / BasicEncoder.forward): for x (b,c,hw)
 *   y = norm(x + bias[c]);  if (relu) y = max(y,0);  if (residual != NULL) y = max(residual + y, 0)
 * rpe_instnorm_act: per-(b,c) instance norm, biased variance, eps inside the root (torch.nn.InstanceNorm2d, fnet).
 * rpe_affine_act:   y = x*scale[c] + shift[c], i.e. an eval-mode BatchNorm2d folded with the conv bias (cnet).
 * out may alias x.  bias / residual may be NULL. */
int rpe_instnorm_act(const float *x, const float *bias, int b, int c, int hw, float eps, int relu,
                     const float *residual, float *out, void *stream);
int rpe_affine_act(const float *x, const float *scale, const float *shift, int b, int c, int hw, int relu,
                   const float *residual, float *out, void *stream);
/* dst[:, 0:c] = src[:, 0:c] for channel slices of NCHW buffers (pointer to the slice's first plane in batch item 0 + batch stride
 * in floats): the slice assignments / clones around RAFT's update loop (core/RAFT/core/raft.py: net = tanh(net), coords1 = coords0
 * .clone(), the returned hidden state) without a library copy kernel. */
int rpe_copy_planes(const float *src, long long src_batch_stride, float *dst, long long dst_batch_stride, int b, int c, int hw,
                    void *stream);
/* FlowHead.conv2 (core/RAFT/core/update.py) + the coordinate update of RAFT.forward (core/RAFT/core/raft.py):
 * out (b,2,h,w) = conv3x3(x (b,c,h,w), weight (2,c,3,3), padding 1) + bias (2) [+ add (b,2,h,w), may be NULL = plain
 * convolution; pass coords1 to get coords1 + delta_flow].  out may alias add.  Two output channels make this a
 * streaming problem, not a GEMM. */
int rpe_conv3x3_to2(const float *x, const float *weight, const float *bias, int b, int c, int h, int w,
                    const float *add, float *out, void *stream);
/* The same with the flow bookkeeping of RAFT.forward's loop (core/RAFT/core/raft.py: coords1 = coords1 + delta_flow;
 * flow = coords1 - coords0 with coords0 the integer pixel grid; the motion encoder concatenates flow behind its output) fused in:
 * coords_out = conv + bias + coords, and flow = coords_out - grid is written to flow_out (b,2,h,w) and to the two-plane channel
 * slices dst1 / dst2 (pointer to the first plane in batch item 0 + batch stride in floats; any of the three may be NULL). */
int rpe_conv3x3_to2_flow(const float *x, const float *weight, const float *bias, int b, int c, int h, int w,
                         const float *coords, float *coords_out, float *flow_out, float *dst1, long long dst1_batch_stride,
                         float *dst2, long long dst2_batch_stride, void *stream);
/* Warm start of the update loop from a previous flow (upstream RAFT.forward(..., flow_init): coords1 = coords0 + flow_init, and
 * core/RAFT/core/utils/utils.py::forward_interpolate).
 * rpe_flow_forward_interpolate: flow, out (b,2,h,w) f32, out must not overlap flow.  Per batch row, each source pixel (x0, y0) lands at
 * x1 = x0 + dx, y1 = y0 + dy (f64); it is valid iff 0 < x1 < w and 0 < y1 < h (strict, as upstream's mask).  Output point (x, y) takes the
 * (dx, dy) of the nearest valid point, distance (x - x1)^2 + (y - y1)^2 in f64 (two rounded squares, then their rounded sum, no fused
 * multiply-add), ties to the lowest source index y0 * w + x0 (upstream's scipy griddata(method='nearest') leaves ties undefined).  A row
 * without a valid point gives zeros (upstream's scipy raises).  Outputs are copies of input values; a row's result does not depend on the
 * batch or the launch (no atomics); no allocation, no synchronisation.  b <= 65535.
 * rpe_flow_seed: the front of a warm pass -- coords_out = pixel grid + flow_init (one f32 addition), flow_out = flow_init, and flow_init
 * into the two-plane channel slices dst1 / dst2 (pointer to the first plane in batch item 0 + batch stride in floats); every output may
 * be NULL.  flow_init (b,2,h,w). */
int rpe_flow_forward_interpolate(const float *flow, int b, int h, int w, float *out, void *stream);
int rpe_flow_seed(const float *flow_init, int b, int h, int w, float *coords_out, float *flow_out, float *dst1, long long dst1_batch_stride,
                  float *dst2, long long dst2_batch_stride, void *stream);
/* flow (b,2,h8,w8), mask (b,576,h8,w8) raw logits already scaled by .25 -> out (b,2,8*h8,8*w8). */
int rpe_upsample_convex(const float *flow, const float *mask, int b, int h8, int w8, float *out, void *stream);
/* The same with flow (b,2,map_h,map_w) and mask (b,576,map_h,map_w) in larger maps whose top-left h8 x w8 is read (a zero padding beyond it
 * is F.unfold's own zero border); out stays the true-size (b,2,8*h8,8*w8).  map_h < h8 or map_w < w8 -> RPE_E_BADARG. */
int rpe_upsample_convex_ex(const float *flow, const float *mask, int b, int h8, int w8, int map_h, int map_w, float *out, void *stream);
/* rpe_conv3x3_to2_flow on a zero-padded map whose real content is h_valid x w_valid: outside that extent coords_out is the pixel grid and
 * the flow written to flow_out / dst1 / dst2 is exactly zero (not conv + bias); inside it the results are those of rpe_conv3x3_to2_flow,
 * bit for bit.  h_valid > h or w_valid > w (or < 1) -> RPE_E_BADARG. */
int rpe_conv3x3_to2_flow_v(const float *x, const float *weight, const float *bias, int b, int c, int h, int w,
                           const float *coords, float *coords_out, float *flow_out, float *dst1, long long dst1_batch_stride,
                           float *dst2, long long dst2_batch_stride, int h_valid, int w_valid, void *stream);
/* dst[:, :, :h, :w] = src[:, :, :h, :w] for (b, c) stacks of maps with their own row pitch, plane stride and batch stride (floats): the way
 * into and out of a padded workspace (core/RAFT/core/raft.py: net, inp, flow_init in; the hidden state and the 1/8 flow out).  A pitch below
 * w or a plane stride below (h - 1) pitch + w -> RPE_E_BADARG. */
int rpe_copy_rect(const float *src, long long src_batch_stride, long long src_plane_stride, int src_pitch, float *dst,
                  long long dst_batch_stride, long long dst_plane_stride, int dst_pitch, int b, int c, int h, int w, void *stream);

/* ---- update-block convolutions (core/RAFT/core/update.py: BasicMotionEncoder convc1/convc2/convf2/conv, SepConvGRU
 * convz|convr/convq of both halves, FlowHead.conv1) as implicit GEMMs on the f32 matrix cores with their epilogues
 * fused.  Stride 1 (stride 2: see the descriptor), zero padding k/2 ("same"), NCHW, kernel height odd, kernel width 1, 3 or 5, w % 4 == 0
 * (otherwise RPE_E_UNSUPPORTED: the caller keeps the library convolution + rpe_bias_act / rpe_gru_gates_*).
 * Every tensor argument is a pointer to channel 0 of a channel slice plus the batch stride (in floats) of the
 * buffer it lives in, so inputs and outputs can be slices of the concatenated (h | motion | flow) buffers.
 *   v = conv(x)[co][p] * scale[co] + add[co][p] + bias[co]           (scale, add, bias: each may be NULL)
 *   RPE_CONV_LINEAR : y = v;  RPE_CONV_RELU : y = max(v, 0);  then, if residual != NULL, y = max(residual + y, 0)
 *   RPE_CONV_TANH   : y = tanh(v)   (rpe_conv_fused, plain epilogue only: no scale / residual / stats / stride 2)
 *                     (the encoder's ResidualBlock tail, core/RAFT/core/extractor.py); out = y (and out2 = y when
 *                     out2 != NULL).  If stats != NULL the kernel also writes per-tile moments of v,
 *                     stats[b][cout][rpe_conv_stats_tiles(cout,h,w,stride)][3] = (count, mean, sum of squared deviations
 *                     from that mean; taken about a pivot so that |mean| >> std loses no digits), for rpe_instnorm_apply
 *                     (instance norm in one further read + write pass instead of three).
 *   RPE_CONV_GATE_ZR: cout = 2*gate_channels; co <  gate_channels: out[co]  = sigmoid(v)                 (z)
 *                                             co >= gate_channels: out2[co-gate_channels] = sigmoid(v) * hidden[co-gate_channels]  (r*h)
 *   RPE_CONV_GATE_H : out[co] = (1 - zgate[co]) * hidden[co] + zgate[co] * tanh(v);  out may alias hidden.        */
#define RPE_CONV_LINEAR 0
#define RPE_CONV_RELU 1
#define RPE_CONV_GATE_ZR 2
#define RPE_CONV_GATE_H 3
#define RPE_CONV_TANH 4     /* y = tanh(v): the hidden-state half of the context encoder's output (core/RAFT/core/raft.py: net = tanh(net)) */
typedef struct rpe_conv_desc {
    const float *x;      long long x_batch_stride;      /* input slice (b, cin, h, w)                              */
    const float *packed;                                 /* weights from rpe_conv_pack                              */
    const float *bias;                                   /* (cout) or NULL                                          */
    const float *add;    long long add_batch_stride;    /* (b, cout, h, w) pre-activation addend or NULL           */
    float *out;          long long out_batch_stride;
    float *out2;         long long out2_batch_stride;   /* NULL unless described above                             */
    const float *hidden; long long hidden_batch_stride; /* gates only                                              */
    const float *zgate;  long long zgate_batch_stride;  /* RPE_CONV_GATE_H only                                    */
    const float *scale;                                  /* (cout) or NULL (folded batch norm: scale, bias = shift) */
    const float *residual; long long residual_batch_stride; /* LINEAR / RELU only                                   */
    float *stats;                                        /* LINEAR / RELU only                                      */
    const float *pre_norm;                               /* (b, cin, 2) = (mean, 1/std) from rpe_instnorm_finalize or NULL: x is the RAW output
                                                          * of the previous convolution and is normalised + ReLU'd while it is staged (3x3, stride 1) */
    int b, cin, cout, h, w, kh, kw, mode, gate_channels;  /* h, w: INPUT map                                       */
    int stride;                                          /* 0 or 1: stride 1; 2: the encoders' down-sampling convolutions (3x3 pad 1 or 1x1 pad 0,
                                                          * even h and w, LINEAR / RELU only); the output map is (h/2, w/2)                        */
    int stats_tiles;                                     /* records per (b, cout) plane of `stats`: 0 or rpe_conv_stats_tiles(cout,h,w,stride)
                                                          * (checked when non-zero; it selects nothing) */
} rpe_conv_desc;
/* A descriptor with a VALID EXTENT beside the map extent (rpe_conv_*_v): d.h x d.w is a zero-padded workspace map whose real content is the
 * top-left h_valid x w_valid.  The kernels read the whole map (its padding is zero, i.e. the convolution's own border) and their epilogues
 * store ZERO, not the computed value, at every output with y >= h_valid or x >= w_valid -- relu(bias), and for the GRU gates sigmoid(.) and
 * tanh(.) of the bias and the context term, would otherwise leak into the padding the next layer reads.  Inside the extent the result is
 * that of the plain entry point on the same map, bit for bit; h_valid == d.h and w_valid == d.w IS the plain entry point's launch.
 * h_valid > d.h or w_valid > d.w (or < 1), or a NULL pointer -> RPE_E_BADARG.  Supported: what the update loop uses -- rpe_conv_wino_v /
 * rpe_conv_wino24_v with the plain epilogue (bias, ReLU, out2; w % 4 == 0), rpe_conv_wino1d_v with every mode, rpe_conv1x1_v; anything
 * else the plain entry point takes -> RPE_E_UNSUPPORTED.  (core/RAFT/core/update.py's layers at any img_size, infer_f2f.yaml:13.)
 * The encoders' layers use the same struct through entry points of their own, rpe_enc_conv_wino_v, rpe_enc_conv_wino24_v, rpe_enc_conv_s2_v
 * and rpe_enc_conv_s2_m96_v (below), which also take scale, residual, stats and pre_norm. */
typedef struct rpe_conv_desc_v { rpe_conv_desc d; int h_valid, w_valid; } rpe_conv_desc_v;
int rpe_conv_wino_v(const rpe_conv_desc_v *desc, void *stream);
int rpe_conv_wino24_v(const rpe_conv_desc_v *desc, void *stream);
int rpe_conv_wino1d_v(const rpe_conv_desc_v *desc, void *stream);
int rpe_conv1x1_v(const rpe_conv_desc_v *desc, void *stream);
/* The ENCODERS' valid-extent forms (core/RAFT/core/extractor.py's layer2, layer3 at any img_size), the same struct rpe_conv_desc_v:
 *   rpe_enc_conv_wino_v / rpe_enc_conv_wino24_v: rpe_conv_wino / rpe_conv_wino24 with every descriptor field the encoders use -- bias,
 *     scale, residual, stats, pre_norm, LINEAR / RELU -- on a map with w % 4 == 0 and 16-byte aligned slices.  Beside the zero stored
 *     outside the extent: the `stats` records cover the outputs inside it only (a tile wholly outside leaves the record (0, 0, 0), which
 *     rpe_instnorm_finalize skips), and with `pre_norm` the input counts as zero outside the extent AFTER normalising
 *     (relu((0 - mean) / std) is not zero), so the result inside is that of the convolution on the cropped, normalised input.
 *   rpe_enc_conv_s2_v / rpe_enc_conv_s2_m96_v: what rpe_conv_fused / rpe_conv_fused_m96 do at stride 2 (3x3 pad 1, the 1x1 shortcut; bias /
 *     scale, stats, LINEAR / RELU); h_valid x w_valid is the extent of the OUTPUT map (d.h / 2 x d.w / 2).  The records (one per 32
 *     output pixels) count and sum the pixels inside it; the two tile classes stay bit-identical.
 * Extent == map is literally the plain entry point's launch (same kernel, same bits, records included).  Extent beyond the map or < 1,
 * or a NULL pointer -> RPE_E_BADARG (checked before anything is dereferenced); a field the form does not take -> RPE_E_UNSUPPORTED. */
int rpe_enc_conv_wino_v(const rpe_conv_desc_v *desc, void *stream);
int rpe_enc_conv_wino24_v(const rpe_conv_desc_v *desc, void *stream);
int rpe_enc_conv_s2_v(const rpe_conv_desc_v *desc, void *stream);
int rpe_enc_conv_s2_m96_v(const rpe_conv_desc_v *desc, void *stream);
/* number of floats of the packed form of a (cout, cin, kh, kw) weight tensor (0 on bad arguments) */
size_t rpe_conv_packed_floats(int cout, int cin, int kh, int kw);
/* weight (cout, cin, kh, kw) contiguous -> packed (tap-major 16-channel steps, output channels padded to 128) */
int rpe_conv_pack(const float *weight, int cout, int cin, int kh, int kw, float *packed, void *stream);
int rpe_conv_fused(const rpe_conv_desc *desc, void *stream);
/* rpe_conv_fused with one more tile class: a stride-2 3x3 launch of 96 output channels without residual / add / out2 runs 96(co) x
 * 128(px) tiles in which no wave idles (csrc/conv_s2.hip) instead of 128-row tiles a quarter of whose rows do not exist -- whatever the
 * launch size, so the caller picks this entry point for launches that fill the chip (rpe_conv_fused turns to 64 x 64 tiles below 512
 * workgroups).  Bit-identical to rpe_conv_fused, the statistics records included; every other descriptor runs exactly as
 * rpe_conv_fused (same rules, same codes). */
int rpe_conv_fused_m96(const rpe_conv_desc *desc, void *stream);
/* The same operation for 3x3 stride-1 convolutions with LINEAR / RELU epilogues (even h and w, cin % 4 == 0) as Winograd
 * F(2x2,3x3) on the f32 matrix cores: 2.25x fewer matrix FLOPs than the direct form (csrc/conv_wino.hip; the update block's
 * convc2, convf2, conv and FlowHead.conv1, core/RAFT/core/update.py, and the encoders' residual blocks,
 * core/RAFT/core/extractor.py).  Supported descriptor fields: bias, scale, out, out2, residual, stats, pre_norm (cin <= 128
 * with the last four: the encoders' widths); stats then holds T = rpe_conv_wino_stats_tiles(h, w) records per plane laid out (b, T, cout, 3) -- pass
 * tiles = -T to rpe_instnorm_apply / rpe_instnorm_finalize (negative = tile-major layout).  desc->packed must come from
 * rpe_conv_wino_pack (rpe_conv_wino_packed_floats floats; 0 = unsupported shape).  add / gates -> RPE_E_UNSUPPORTED
 * (the caller uses rpe_conv_fused). */
size_t rpe_conv_wino_packed_floats(int cout, int cin);
int rpe_conv_wino_stats_tiles(int h, int w);
int rpe_conv_wino_pack(const float *weight, int cout, int cin, float *packed, void *stream);
int rpe_conv_wino(const rpe_conv_desc *desc, void *stream);
/* The same convolution as Winograd F(2x4,3x3): F(2,3) along H, F(4,3) along W at the points {0, 1, -1, 1/2, -2}; 1/3 product per output
 * against F(2x2)'s 4/9, at about a serial direct f32 sum's error (csrc/conv_wino24.hip; the layers of rpe_conv_wino).  Same descriptor
 * fields, epilogues and moment records (rpe_conv_wino_stats_tiles, (b, T, cout, 3)).  Needs cin % 4 == 0, even h, w % 4 == 0 and
 * 16-byte aligned x / out / out2 / residual planes (batch strides % 4 == 0); anything else -> RPE_E_UNSUPPORTED (the caller uses
 * rpe_conv_wino).  desc->packed must come from rpe_conv_wino24_pack (rpe_conv_wino24_packed_floats floats, 0 = unsupported shape;
 * 16-byte aligned). */
size_t rpe_conv_wino24_packed_floats(int cout, int cin);
int rpe_conv_wino24_pack(const float *weight, int cout, int cin, float *packed, void *stream);
int rpe_conv_wino24(const rpe_conv_desc *desc, void *stream);
/* LABELLED VARIANT of rpe_conv_wino (never in a headline number; bench.py --conv-bf16x3): the same convolution, descriptor fields,
 * epilogues and moment records, with every f32 product of the Winograd domain evaluated as six bf16 products of an exact three-way
 * split (x = hi + mid + lo) on the 16-bit matrix cores, f32 accumulation: f32-equivalent error (tests/test_gpu_conv_x3.py holds it to
 * 1.25x the f32 kernels'), 3/8 of the matrix time (csrc/conv_wino_x3.hip).  Needs cin % 16 == 0, w % 4 == 0, even h, 16-byte
 * aligned tensors; anything else -> RPE_E_UNSUPPORTED (the caller uses rpe_conv_wino).  desc->packed must come from
 * rpe_conv_wino_x3_pack (rpe_conv_wino_x3_packed_bytes bytes, 0 = unsupported shape; 16-byte aligned).  Same reference layers as
 * rpe_conv_wino (core/RAFT/core/update.py, extractor.py; call sites core/pose/pose_net.py:47,65,129). */
size_t rpe_conv_wino_x3_packed_bytes(int cout, int cin);
int rpe_conv_wino_x3_pack(const float *weight, int cout, int cin, void *packed, void *stream);
int rpe_conv_wino_x3(const rpe_conv_desc *desc, void *stream);
/* The same operation for 1x5 / 5x1 stride-1 convolutions (w % 4 == 0, cin % 4 == 0; tensors 16-byte aligned) with every
 * epilogue mode of rpe_conv_fused incl. the GRU gates (add, hidden, zgate, out2, gate_channels), as Winograd F(4,5) along the
 * filter axis on the f32 matrix cores: 8 products per 4 outputs instead of 20 (csrc/conv_wino1d.hip; SepConvGRU's convz|convr
 * and convq, core/RAFT/core/update.py).  desc->packed must come from rpe_conv_wino1d_pack (weight (cout, cin, 5) = the
 * contiguous (cout, cin, 1, 5) or (cout, cin, 5, 1) tensor; rpe_conv_wino1d_packed_floats floats, 0 = unsupported shape);
 * kh, kw select the axis.  scale / residual / stats / pre_norm -> RPE_E_UNSUPPORTED. */
size_t rpe_conv_wino1d_packed_floats(int cout, int cin);
int rpe_conv_wino1d_pack(const float *weight, int cout, int cin, float *packed, void *stream);
int rpe_conv_wino1d(const rpe_conv_desc *desc, void *stream);
/* LABELLED VARIANT of rpe_conv_wino1d (never in a headline number; bench.py --conv-bf16x3): the same convolution, descriptor fields
 * and epilogue modes incl. the GRU gates, with every f32 product of the Winograd domain evaluated as six bf16 products of an exact
 * three-way split on the 16-bit matrix cores, f32 accumulation (csrc/conv_wino1d_x3.hip; error held to the f32 kernels' by
 * tests/test_gpu_conv_x3.py).  Needs cin % 16 == 0, w % 4 == 0, 16-byte aligned tensors; anything else -> RPE_E_UNSUPPORTED (the
 * caller uses rpe_conv_wino1d).  desc->packed must come from rpe_conv_wino1d_x3_pack (rpe_conv_wino1d_x3_packed_bytes bytes, 0 =
 * unsupported shape; 16-byte aligned).  Same reference layers as rpe_conv_wino1d (SepConvGRU, core/RAFT/core/update.py; call sites
 * core/pose/pose_net.py:47,65,129). */
size_t rpe_conv_wino1d_x3_packed_bytes(int cout, int cin);
int rpe_conv_wino1d_x3_pack(const float *weight, int cout, int cin, void *packed, void *stream);
int rpe_conv_wino1d_x3(const rpe_conv_desc *desc, void *stream);
/* 1x1 stride-1 convolutions as plain GEMMs with LDS-DMA operand rings (csrc/conv1x1.hip; BasicMotionEncoder.convc1 behind the
 * correlation lookup, the mask head's and the encoders' 1x1 output layers, core/RAFT/core/update.py / extractor.py).  Same
 * descriptor; supported fields: bias, out, out2, mode LINEAR / RELU / TANH; h * w % 4 == 0, 16-byte aligned input slice.  desc->packed
 * must come from rpe_conv1x1_pack (rpe_conv1x1_packed_floats floats).  Anything else -> RPE_E_UNSUPPORTED (use rpe_conv_fused). */
size_t rpe_conv1x1_packed_floats(int cout, int cin);
int rpe_conv1x1_pack(const float *weight, int cout, int cin, float *packed, void *stream);
int rpe_conv1x1(const rpe_conv_desc *desc, void *stream);
/* LABELLED VARIANT of rpe_conv1x1 (never in a headline number; bench.py --conv-bf16x3): the same GEMM with every f32 product as six bf16
 * products of a three-way split on the 16-bit matrix cores, f32 accumulation (csrc/conv1x1_x3.hip; BasicMotionEncoder.convc1,
 * core/RAFT/core/update.py; call sites core/pose/pose_net.py:47,65,129).  Same descriptor; supported: bias, out, out2, mode LINEAR / RELU;
 * h * w % 4 == 0, 16-byte aligned input and output slices; anything else -> RPE_E_UNSUPPORTED (use rpe_conv1x1).  desc->packed must come from
 * rpe_conv1x1_x3_pack (rpe_conv1x1_x3_packed_bytes bytes; 16-byte aligned).
 * SPECIAL VALUES (all three bf16x3 entry points; the f32 kernels do not share this): the split x = hi + mid + lo turns an infinite input into
 * hi = +-Inf, mid = Inf - Inf = NaN, so +-Inf in an activation or weight gives NaN in every output it reaches, where the f32 kernels give
 * +-Inf (or NaN only for Inf - Inf / 0 * Inf).  NaN inputs give NaN in both.  rpe_conv1x1_x3 with cin % 16 != 0 additionally reads channel
 * cin - 1 a second time against zero weights in its padded last K step: a NaN there is harmless (it is NaN anyway), an Inf falls under the
 * rule above.  Finite inputs, including denormals and values up to FLT_MAX / 4, are unaffected (tests/test_gpu_conv_x3.py). */
size_t rpe_conv1x1_x3_packed_bytes(int cout, int cin);
int rpe_conv1x1_x3_pack(const float *weight, int cout, int cin, void *packed, void *stream);
int rpe_conv1x1_x3(const rpe_conv_desc *desc, void *stream);
/* OPT-IN PRECISION CONTRACT (RAFT's ``update_fp16``; never in a headline number): rpe_conv_fused's operation for stride-1 "same" convolutions
 * with (kh, kw) in {1x1, 3x3, 1x5, 5x1} and fp16 OPERANDS on the 16-bit matrix cores (v_mfma_f32_32x32x16_f16; csrc/conv_f16.hip) -- what
 * upstream RAFT's mixed_precision (autocast) does to the update block, core/RAFT/core/update.py; call sites core/pose/pose_net.py:47,65,129.
 *   - every input activation and every weight is rounded to IEEE fp16, round to nearest even, unscaled; the products are exact in f32;
 *   - the sum is f32 in one fixed order (no atomics, no split K over workgroups), the same for every batch size and launch size: a batch
 *     row's result does not depend on the batch it is launched in, bit for bit;
 *   - everything after the sum is f32 exactly as rpe_conv_fused defines it above: bias, add, ReLU / tanh, the GRU gates with hidden / zgate,
 *     out2 (the kernels share the epilogue's code); activations stay f32 in memory -- only the operands are rounded, while they are staged.
 * Supported: any cin >= 1 (the pack pads the K tail with zero weights and the kernel stages channels >= cin as zero WITHOUT reading them: what
 * lies behind the slice cannot enter, not even a NaN through 0 * NaN), any cout, w % 4 == 0, 16-byte aligned slices with batch strides
 * % 4 == 0, b <= 65535, every mode of rpe_conv_fused (LINEAR, RELU, TANH, GATE_ZR, GATE_H) with bias, add, hidden, zgate, out2, gate_channels;
 * out may alias hidden.  scale / residual / stats / pre_norm, stride 2, another kernel shape or a misaligned slice -> RPE_E_UNSUPPORTED; a NULL
 * pointer or a non-positive extent -> RPE_E_BADARG, checked before anything is dereferenced.  desc->packed must come from rpe_conv_f16_pack
 * (rpe_conv_f16_packed_bytes bytes, 0 = unsupported shape; 16-byte aligned): fp16 in matrix-fragment order, packed on the device.
 * SPECIAL VALUES (this entry point; the f32 kernels do not share it): an activation or weight with |x| > 65504 becomes +-Inf where round to
 * nearest even says so (from 65520 on), and +-Inf then follows IEEE through the sum (Inf - Inf, 0 * Inf -> NaN); NaN operands give NaN in
 * every output they reach, and only there.  Values below the smallest fp16 normal (2^-14) round to fp16 subnormals or zero.
 * FP16 SUBNORMAL OPERANDS (observed once on an MI355X with a 1x1 identity layer; no test asserts it): they are NOT flushed.  Activations of
 * 2^-15, 2^-24, 3 * 2^-24 came back exactly, 2^-25 as 0 and 1.5 * 2^-24 as 2^-23 (the ties-to-even roundings into the subnormal range), and
 * a subnormal weight 2^-20 against 1024 gave 2^-10 exactly: v_cvt_f16_f32 produces subnormals and v_mfma_f32_32x32x16_f16 multiplies them. */
size_t rpe_conv_f16_packed_bytes(int cout, int cin, int kh, int kw);
int rpe_conv_f16_pack(const float *weight, int cout, int cin, int kh, int kw, void *packed, void *stream);
int rpe_conv_f16(const rpe_conv_desc *desc, void *stream);
/* Generic convolution for every shape the tuned kernels above refuse (odd maps, rows that are not whole 16-byte quads): replaces
 * torch.nn.functional.conv2d(x, weight, bias, stride, padding) as the host code's fallback route, so that every convolution of the
 * reference's RAFT (core/RAFT/core/extractor.py, update.py) runs in this library for any img_size (configuration/infer_f2f.yaml:13).
 * x (b, cin, h, w) and out (b, cout, ho, wo) are channel slices given by their batch strides (floats); weight (cout, cin, kh, kw)
 * contiguous, bias (cout) or NULL; kh, kw <= 7; stride 1 or 2; zero padding (pad_h, pad_w); ho = (h + 2 pad_h - kh) / stride + 1;
 * relu != 0: out = max(., 0).  f32 matrix cores with element-wise operand gathers: robust, 2-3x slower than the tuned kernels. */
int rpe_conv_direct(const float *x, long long x_batch_stride, const float *weight, const float *bias, int b, int cin, int cout,
                    int h, int w, int kh, int kw, int stride, int pad_h, int pad_w, int relu, float *out,
                    long long out_batch_stride, void *stream);
/* number of moment records per (b, channel) plane rpe_conv_fused leaves for this shape (h, w: input): stride 1 one per pixel
 * tile (the launcher and this function share one tile-width rule); stride 2 one per 32 output pixels -- in both of its tile
 * classes (128 x 128, or 64 x 64 for launches too small to fill the chip), bit-identical between them, so an image's statistics
 * do not depend on how many images share the launch */
int rpe_conv_stats_tiles(int cout, int h, int w, int stride);
/* round-3 name, kept: the count no longer depends on the batch (returns rpe_conv_stats_tiles; 0 for b <= 0) */
int rpe_conv_stats_tiles_batch(int cout, int h, int w, int stride, int b);
/* Instance norm (torch.nn.InstanceNorm2d, affine=False; fnet of core/RAFT/core/extractor.py) of x (b,c,hw) given the
 * per-tile (count, mean, M2) records rpe_conv_fused / rpe_stem_conv left in `partials` (b,c,tiles,3) -- or rpe_conv_wino in
 * (b,|tiles|,c,3) when tiles < 0 --, merged in f64 with the parallel-variance formula:
 *   y = (x - mean) / sqrt(var + eps); if (relu) y = max(y,0); if (residual) y = max(residual + y, 0).  out may alias x. */
int rpe_instnorm_apply(const float *x, const float *partials, int tiles, int b, int c, int hw, float eps, int relu,
                       const float *residual, float *out, void *stream);
/* The same with a residual that is itself the RAW output of an instance-normalised convolution: residual_mean_inv (b,c,2) =
 * (mean, 1/sqrt(var + eps)) from rpe_instnorm_finalize, and the residual term becomes relu((residual - mean) * inv) -- the first
 * residual block of fnet then reads the stem's raw output twice (as input through `pre_norm`, as shortcut through this) and the
 * stem's normalised output is never written (BasicEncoder.forward: relu1(norm1(conv1 x)) -> layer1, core/RAFT/core/extractor.py).
 * relu: bit 0 = ReLU on y (as above); bit 1 = the raw residual is normalised WITHOUT a ReLU -- the shortcut of a stride-2 ResidualBlock,
 * norm3(conv1x1 x) (extractor.py), whose normalised output then never exists as a tensor either.
 * tiles == 0: `partials` is not records but the (b,c,2) (mean, 1/sqrt(var + eps)) pairs rpe_instnorm_finalize made of them (eps is
 * then unused): the pass is a pure stream, several workgroups per plane -- the faster form behind large maps. */
int rpe_instnorm_apply_ex(const float *x, const float *partials, int tiles, int b, int c, int hw, float eps, int relu,
                          const float *residual, const float *residual_mean_inv, float *out, void *stream);
/* mean_inv (b,c,2) = (mean, 1/sqrt(var + eps)) of each plane from the same partial sums: the `pre_norm` input of the
 * next rpe_conv_fused, which then normalises its input on the fly (no separate pass for norm1 + ReLU of a ResidualBlock). */
int rpe_instnorm_finalize(const float *partials, int tiles, int b, int c, int hw, float eps, float *mean_inv, void *stream);
/* rpe_instnorm_apply_ex's pass (tiles == 0 form: mean_inv (b,c,2) from rpe_instnorm_finalize, whose merge weighs every record by its
 * own count and so takes the valid-extent records as they are) on a zero-padded (h, w) map with h_valid x w_valid of content: the same
 * bits inside the extent, ZERO outside it (relu((0 - mean) * inv) is not zero).  relu bits, residual and residual_mean_inv as there; out
 * may alias x.  w % 4 == 0, 16-byte aligned tensors, else RPE_E_UNSUPPORTED; an extent beyond the map or < 1, NULL -> RPE_E_BADARG. */
int rpe_instnorm_apply_v(const float *x, const float *mean_inv, int b, int c, int h, int w, int h_valid, int w_valid, int relu,
                         const float *residual, const float *residual_mean_inv, float *out, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Prepared launch lists -- replace the HOST loop around the kernels above: RAFT.forward's `for itr in range(iters)` over lookup ->
 * motion encoder -> SepConvGRU -> flow head (core/RAFT/core/raft.py; call sites core/pose/pose_net.py:47,65,129) and the encoders'
 * layer-by-layer walk (core/RAFT/core/extractor.py), which the reference runs as hundreds of Python-dispatched launches per frame
 * (scripts/infer_trajectory.py:57,71-77 tracks one frame at a time: ~330 launches of 10-50 us each, i.e. the host decides the frame rate).
 * A list is an array of rpe_op in caller-owned host memory: each op names an entry point of this header (`kind`), the argument block that
 * entry point would be called with (`args`: the rpe_conv_desc of the convolutions, one of the rpe_*_args structs below for the others --
 * the same values in the same order as the function's parameters) and the stream it goes to (`stream` = index into the `streams` array of
 * the call).  rpe_run_ops walks the list once, calling the SAME entry points -- same checks, same kernels, same bits as calling them one
 * by one -- and stops at the first op that fails (its index goes to *failed_op, its status is returned).  The list and everything it
 * points to must stay alive and unchanged for the duration of the call only (launches are asynchronous; the argument blocks are consumed
 * at enqueue time); the caller may patch pointers inside the argument blocks between calls (new input / output buffers).
 * Fork / join between the streams of a list: RPE_OP_EVENT_RECORD records, RPE_OP_STREAM_WAIT makes streams[op.stream] wait for, the
 * hipEvent_t whose handle is stored at `args` (args = address of a void* cell holding the handle; a NULL handle makes the op a no-op, so a
 * caller can keep timing events in a list and arm them only when it measures).  No state is kept between calls. */
#define RPE_OP_CONV_FUSED 1        /* args: const rpe_conv_desc *  -> rpe_conv_fused       */
#define RPE_OP_CONV_WINO 2         /*       const rpe_conv_desc *  -> rpe_conv_wino        */
#define RPE_OP_CONV_WINO1D 3       /*       const rpe_conv_desc *  -> rpe_conv_wino1d      */
#define RPE_OP_CONV1X1 4           /*       const rpe_conv_desc *  -> rpe_conv1x1          */
#define RPE_OP_CONV_WINO_X3 5      /*       const rpe_conv_desc *  -> rpe_conv_wino_x3     */
#define RPE_OP_CONV_WINO1D_X3 6    /*       const rpe_conv_desc *  -> rpe_conv_wino1d_x3   */
#define RPE_OP_CONV1X1_X3 7        /*       const rpe_conv_desc *  -> rpe_conv1x1_x3       */
#define RPE_OP_CORR_LOOKUP 8       /*       const rpe_corr_lookup_args *                   */
#define RPE_OP_STEM_CONV 9         /*       const rpe_stem_conv_args *                     */
#define RPE_OP_FLOW_UPDATE 10      /*       const rpe_flow_update_args * -> rpe_conv3x3_to2_flow */
#define RPE_OP_COPY_PLANES 11      /*       const rpe_copy_planes_args *                   */
#define RPE_OP_INSTNORM_FINALIZE 12 /*      const rpe_instnorm_finalize_args *             */
#define RPE_OP_INSTNORM_APPLY 13   /*       const rpe_instnorm_apply_args * -> rpe_instnorm_apply_ex */
#define RPE_OP_UPSAMPLE_CONVEX 14  /*       const rpe_upsample_convex_args *               */
#define RPE_OP_CORR_BUILD 15       /*       const rpe_corr_build_args * -> rpe_corr_build_ex */
#define RPE_OP_LOOKUP_CONV1X1 16    /*       const rpe_lookup_conv1x1_args * -> rpe_corr_lookup_conv1x1 */
#define RPE_OP_CONV_WINO24 17      /*       const rpe_conv_desc *  -> rpe_conv_wino24      */
#define RPE_OP_FLOW_SEED 18        /*       const rpe_flow_seed_args * -> rpe_flow_seed    */
#define RPE_OP_CONV_FUSED_M96 19   /*       const rpe_conv_desc *  -> rpe_conv_fused_m96   */
#define RPE_OP_CORR_ALT_PREPARE 20 /*       const rpe_corr_alt_prepare_args *              */
#define RPE_OP_CORR_ALT_LOOKUP 21  /*       const rpe_corr_alt_lookup_args *               */
#define RPE_OP_CONV_WINO_V 22      /*       const rpe_conv_desc_v * -> rpe_conv_wino_v     */
#define RPE_OP_CONV_WINO24_V 23    /*       const rpe_conv_desc_v * -> rpe_conv_wino24_v   */
#define RPE_OP_CONV_WINO1D_V 24    /*       const rpe_conv_desc_v * -> rpe_conv_wino1d_v   */
#define RPE_OP_CONV1X1_V 25        /*       const rpe_conv_desc_v * -> rpe_conv1x1_v       */
#define RPE_OP_STEM_CONV_V 26      /*       const rpe_stem_conv_v_args *                   */
#define RPE_OP_FLOW_UPDATE_V 27    /*       const rpe_flow_update_v_args * -> rpe_conv3x3_to2_flow_v */
#define RPE_OP_CORR_LOOKUP_EX 28   /*       const rpe_corr_lookup_ex_args *                */
#define RPE_OP_CORR_ALT_LOOKUP_EX 29 /*     const rpe_corr_alt_lookup_ex_args *            */
#define RPE_OP_UPSAMPLE_CONVEX_EX 30 /*     const rpe_upsample_convex_ex_args *            */
#define RPE_OP_COPY_RECT 31        /*       const rpe_copy_rect_args *                     */
#define RPE_OP_EVENT_RECORD 32     /*       void *const * (address of a hipEvent_t handle; NULL handle = no-op) */
#define RPE_OP_STREAM_WAIT 33      /*       void *const * (the same)                       */
#define RPE_OP_ENC_CONV_WINO_V 34  /*       const rpe_conv_desc_v * -> rpe_enc_conv_wino_v */
#define RPE_OP_ENC_CONV_WINO24_V 35 /*      const rpe_conv_desc_v * -> rpe_enc_conv_wino24_v */
#define RPE_OP_ENC_CONV_S2_V 36    /*       const rpe_conv_desc_v * -> rpe_enc_conv_s2_v   */
#define RPE_OP_ENC_CONV_S2_M96_V 37 /*      const rpe_conv_desc_v * -> rpe_enc_conv_s2_m96_v */
#define RPE_OP_INSTNORM_APPLY_V 38 /*       const rpe_instnorm_apply_v_args *              */
#define RPE_OP_CORR_ALT_PREPARE_EX 39 /*    const rpe_corr_alt_prepare_ex_args *           */
#define RPE_OP_CORR_ALT_LOOKUP_DT 40 /*     const rpe_corr_alt_lookup_dt_args *            */
#define RPE_OP_CONV_F16 (RPE_OP_CORR_ALT_LOOKUP_DT + 1) /* = 41: const rpe_conv_desc * -> rpe_conv_f16 (the kind after the last one) */
typedef struct rpe_op {
    int kind;                      /* RPE_OP_*                                             */
    int stream;                    /* index into rpe_run_ops' streams[]                    */
    const void *args;
} rpe_op;
typedef struct rpe_corr_lookup_args { const void *pyramid; const float *coords; int b, h8, w8, levels, radius; float *out; } rpe_corr_lookup_args;
typedef struct rpe_lookup_conv1x1_args {
    const void *pyramid; const float *coords; int b, h8, w8, levels, radius; const float *packed, *bias; int relu; float *out;
    long long out_batch_stride; float *out2; long long out2_batch_stride;
} rpe_lookup_conv1x1_args;
typedef struct rpe_corr_build_args { const float *fmap1, *fmap2; int b, c, h8, w8, levels, feature_dtype; void *pyramid; } rpe_corr_build_args;
typedef struct rpe_corr_alt_prepare_args { const float *fmap1, *fmap2; int b, c, h8, w8, levels; void *scratch; } rpe_corr_alt_prepare_args;
typedef struct rpe_corr_alt_lookup_args { const void *scratch; const float *coords; int b, c, h8, w8, levels, radius; float *out; } rpe_corr_alt_lookup_args;
typedef struct rpe_stem_conv_args {
    const float *image; int b, cin, h, w, stride; float div, mul, sub; const float *packed; int cout; const float *bias, *scale; int relu;
    float *out, *stats;
} rpe_stem_conv_args;
typedef struct rpe_flow_update_args {
    const float *x, *weight, *bias; int b, c, h, w; const float *coords; float *coords_out, *flow_out, *dst1; long long dst1_batch_stride;
    float *dst2; long long dst2_batch_stride;
} rpe_flow_update_args;
typedef struct rpe_flow_seed_args {
    const float *flow_init; int b, h, w; float *coords_out, *flow_out, *dst1; long long dst1_batch_stride; float *dst2; long long dst2_batch_stride;
} rpe_flow_seed_args;
typedef struct rpe_copy_planes_args { const float *src; long long src_batch_stride; float *dst; long long dst_batch_stride; int b, c, hw; } rpe_copy_planes_args;
typedef struct rpe_instnorm_finalize_args { const float *partials; int tiles, b, c, hw; float eps; float *mean_inv; } rpe_instnorm_finalize_args;
typedef struct rpe_instnorm_apply_args {
    const float *x, *partials; int tiles, b, c, hw; float eps; int relu; const float *residual, *residual_mean_inv; float *out;
} rpe_instnorm_apply_args;
typedef struct rpe_upsample_convex_args { const float *flow, *mask; int b, h8, w8; float *out; } rpe_upsample_convex_args;
typedef struct rpe_corr_lookup_ex_args { const void *pyramid; const float *coords; int b, h8, w8, levels, radius, map_h, map_w; float *out; } rpe_corr_lookup_ex_args;
typedef struct rpe_corr_alt_lookup_ex_args {
    const void *scratch; const float *coords; int b, c, h8, w8, levels, radius, map_h, map_w; float *out;
} rpe_corr_alt_lookup_ex_args;
typedef struct rpe_stem_conv_v_args {
    const float *image; int b, cin, h, w, stride; float div, mul, sub; const float *packed; int cout; const float *bias, *scale; int relu;
    float *out, *stats; int h_valid, w_valid;
} rpe_stem_conv_v_args;
typedef struct rpe_flow_update_v_args {
    const float *x, *weight, *bias; int b, c, h, w; const float *coords; float *coords_out, *flow_out, *dst1; long long dst1_batch_stride;
    float *dst2; long long dst2_batch_stride; int h_valid, w_valid;
} rpe_flow_update_v_args;
typedef struct rpe_upsample_convex_ex_args { const float *flow, *mask; int b, h8, w8, map_h, map_w; float *out; } rpe_upsample_convex_ex_args;
typedef struct rpe_copy_rect_args {
    const float *src; long long src_batch_stride, src_plane_stride; int src_pitch; float *dst; long long dst_batch_stride, dst_plane_stride;
    int dst_pitch, b, c, h, w;
} rpe_copy_rect_args;
typedef struct rpe_instnorm_apply_v_args {
    const float *x, *mean_inv; int b, c, h, w, h_valid, w_valid, relu; const float *residual, *residual_mean_inv; float *out;
} rpe_instnorm_apply_v_args;
typedef struct rpe_corr_alt_prepare_ex_args {
    const float *fmap1, *fmap2; int b, c, h8, w8, levels, feature_dtype; void *scratch;
} rpe_corr_alt_prepare_ex_args;
typedef struct rpe_corr_alt_lookup_dt_args {
    const void *scratch; const float *coords; int b, c, h8, w8, levels, radius, map_h, map_w, feature_dtype; float *out;
} rpe_corr_alt_lookup_dt_args;
/* streams: n_streams hipStream_t handles (NULL = the default stream).  failed_op may be NULL. */
int rpe_run_ops(const rpe_op *ops, int n_ops, void *const *streams, int n_streams, int *failed_op);

/* ---- The two weight heads of PoseNet (core/pose/pose_net.py:109-115: torch.cat of the 1/8 stacks with the GRU hidden
 * state and the context -> TinyUNet(264) / TinyUNet(272), core/unet/unet.py:7-82 -> bilinear resize to (H, W) -> Sigmoid)
 * as one chain of 15 launches for both heads and all frames (csrc/unet.hip), inference-mode batch norm folded.
 *   inp1, inp2 (b,8,h8,w8) from rpe_depth_backproject_warp; hidden, context: channel 0 of (b,128,h8,w8) slices with their
 *   batch strides (floats); params2d / params3d: rpe_unet_params_floats(264 / 272) floats in the layout documented in
 *   csrc/unet.hip (3x3 weights as [cin][9][cout], batch norm as per-channel scale/shift); out2d, out3d (b,1,H,W) in (0,1).
 *   The 1/8 grid must be at least 44x44 (valid convolutions), as in the reference; otherwise RPE_E_UNSUPPORTED. */
size_t rpe_unet_params_floats(int in_channels);
size_t rpe_unet_workspace_bytes(int b, int h8, int w8);
int rpe_unet_heads(const float *inp1, const float *inp2, const float *hidden, const float *context, long long hidden_batch_stride,
                   long long context_batch_stride, const float *params2d, const float *params3d, int b, int h8, int w8, int H, int W,
                   float *out2d, float *out3d, void *workspace, void *stream);

/* ---- Training route of ONE TinyUNet head (csrc/unet_train.hip): what F.conv2d / F.batch_norm / F.max_pool2d / F.conv_transpose2d /
 * F.interpolate and their backward kernels do under autograd while the reference trains the heads (scripts/train_posenet.py),
 * as hand-written kernels, one per operation.  f32 NCHW; every reduction in a fixed order (no float atomics): bit-reproducible.
 *   input: the channel concatenation of nsrc <= 4 maps (n, src_channels[k], h8, w8), never materialised: src[k] points at channel 0 of
 *     row 0, src_batch_strides[k] is the distance between rows in floats (so a channel slice of a wider tensor is fine); every
 *     src_channels[k] must be a multiple of 8 (RPE_E_UNSUPPORTED otherwise).  src, src_channels, src_batch_strides, params,
 *     running_mean, running_var, num_batches_tracked, momentum and eps are HOST arrays (of device pointers / of values).
 *   params: the 36 parameter tensors in torch's own layouts, in the order documented in csrc/unet_train_host.h (per encoder stage
 *     conv1.weight, conv1.bias, norm.weight, norm.bias, conv2.weight, conv2.bias; per decoder stage upconv.weight, upconv.bias,
 *     conv1.weight, conv1.bias, norm.weight, norm.bias, conv2.weight, conv2.bias; head.weight, head.bias).
 *   norms (3 encoder, then 2 decoder): bit k of train_mask set = batch statistics (biased variance) and running_mean[k] / running_var[k]
 *     (momentum[k], unbiased variance) and *num_batches_tracked[k] (int64; the array or an entry may be NULL) updated exactly once, as
 *     F.batch_norm(training=True) does; bit clear = the running statistics are used and left alone.
 *   out (n,1,out_h,out_w): the head map resized bilinearly (align_corners=False), through a sigmoid if `sigmoid` is set.
 *   workspace: rpe_unet_train_workspace_bytes(n, cin, h8, w8, out_h, out_w) bytes (cin = sum of src_channels; 0 = unsupported size);
 *     the forward leaves the saved activations in it, rpe_unet_train_backward must get the same, untouched workspace and the same
 *     src / params / train_mask / sizes.  It writes the parameter gradients back to back in the params order into grad_params
 *     (rpe_unet_train_grad_floats(cin) floats; tensor k starts at rpe_unet_train_grad_offset(cin, k), k = 36 gives the total) and the
 *     gradient of the concatenated input (n,cin,h8,w8) into grad_input unless that is NULL.  `out` (the forward's output) is read
 *     only with `sigmoid`.  The 1/8 grid must be at least 44x44, otherwise RPE_E_UNSUPPORTED.
 *   Where the buffers of the workspace lie (for tests and tools that read a saved activation or an activation gradient):
 *     rpe_unet_train_workspace_offset gives the first float of buffer `index` counted from the workspace pointer rounded up to 256
 *     bytes, (size_t)-1 for an unsupported shape or an index outside [0, 46); rpe_unet_train_workspace_extent writes
 *     (rows, channels, h, w) of that buffer into extent[4] (RPE_E_BADARG for such an index, RPE_E_UNSUPPORTED for such a shape).
 *     Index order = order in memory (documented with the plan in csrc/unet_train_host.h): per encoder stage a1, r1, g_r1, skip,
 *     g_skip, [pool, g_pool,] mean, invstd; per decoder stage up, g_up, r, nrm, g_nrm, dout, g_dout, mean, invstd; hm, g_hm, wpart
 *     (doubles: 2 rows channels floats). */
size_t rpe_unet_train_workspace_bytes(int n, int cin, int h8, int w8, int out_h, int out_w);
size_t rpe_unet_train_workspace_offset(int n, int cin, int h8, int w8, int index);
int rpe_unet_train_workspace_extent(int n, int cin, int h8, int w8, int index, int *extent);
size_t rpe_unet_train_grad_floats(int cin);
size_t rpe_unet_train_grad_offset(int cin, int index);
int rpe_unet_train_forward(const float *const *src, const int *src_channels, const long long *src_batch_strides, int nsrc,
                           const float *const *params, float *const *running_mean, float *const *running_var,
                           long long *const *num_batches_tracked, const float *momentum, const float *eps, int train_mask,
                           int n, int h8, int w8, int out_h, int out_w, int sigmoid, float *out, void *workspace, void *stream);
int rpe_unet_train_backward(const float *grad_out, const float *out, const float *const *src, const int *src_channels,
                            const long long *src_batch_strides, int nsrc, const float *const *params, int train_mask, int n, int h8, int w8,
                            int out_h, int out_w, int sigmoid, float *grad_params, float *grad_input, void *workspace, void *stream);

/* ---- 7x7 convolutions of few input channels as patch-staged implicit GEMMs (csrc/stem.hip):
 *   cin = 3, stride 2: the encoders' first layer (core/RAFT/core/extractor.py BasicEncoder.conv1/norm1/relu1) on the RAW
 *                      0..255 image with RAFT.forward's normalisation image = 2 * (image / 255) - 1 (core/RAFT/core/raft.py)
 *                      applied while the input patch is staged (zero padding of the NORMALISED image, as the reference);
 *   cin = 2, stride 1: the motion encoder's convf1 on the flow (core/RAFT/core/update.py), div = mul = 1, sub = 0.
 * xn = mul * (x / div) - sub;  v = conv7x7(xn; pad 3) * scale[co] + bias[co] (scale NULL = 1: folded batch norm for cnet);
 * optional ReLU; stats (b,cout,rpe_stem_tiles(h,w,stride),3) receives per-tile (count, mean, M2) of v for
 * rpe_instnorm_apply (fnet).  cout % 64 == 0; stride 2 needs even h, w.  packed = rpe_stem_pack of the (cout,cin,7,7)
 * weight (rpe_stem_packed_floats floats). */
int rpe_stem_tiles(int h, int w, int stride);
size_t rpe_stem_packed_floats(int cout, int cin);
int rpe_stem_pack(const float *weight, int cout, int cin, float *packed, void *stream);
int rpe_stem_conv(const float *image, int b, int cin, int h, int w, int stride, float div, float mul, float sub,
                  const float *packed, int cout, const float *bias, const float *scale, int relu, float *out,
                  float *stats, void *stream);
/* rpe_stem_conv with a valid extent of the OUTPUT map (cin = 2, stride 1, no stats: convf1 on a zero-padded flow map): outputs with
 * y >= h_valid or x >= w_valid are stored as zero, not relu(bias); inside, rpe_stem_conv's bits.  An extent beyond the map -> RPE_E_BADARG. */
int rpe_stem_conv_v(const float *image, int b, int cin, int h, int w, int stride, float div, float mul, float sub,
                    const float *packed, int cout, const float *bias, const float *scale, int relu, float *out,
                    float *stats, int h_valid, int w_valid, void *stream);

/* ---- input side: what the reference's datasets do on the CPU before a frame reaches
 * PoseEstimator (dataset/stereo_dataset.py:12-16,35-40, dataset/video_dataset.py:59-63, dataset/transforms.py:20-39).
 * mask_specularities: out (h,w) u8 = erode_11x11((r+g+b < sum_threshold) & mask) on the decoded uint8 (h,w,3) image;
 * mask may be NULL; sum_threshold = ceil(3*255*spec_thr) (numpy compares the integer sum with a float); pixels outside
 * the image never erode (cv2.erode's default border value). */
int rpe_mask_specularities(const uint8_t *img_hwc, const uint8_t *mask, int h, int w, int sum_threshold, uint8_t *out,
                           void *stream);
/* ResizeStereo on one image: bilinear resize (torchvision 0.14 on tensors: align_corners=False, no antialias) of the
 * input to (resized_h, resized_w), then the centre crop [top, top+out_h) x [left, left+out_w); out (c,out_h,out_w) f32.
 * Input: float32 (c,h,w), or -- in_is_u8_hwc -- the decoded uint8 (h,w,c) image (fuses .permute(2,0,1).float()). */
int rpe_resize_crop(const void *in, int in_is_u8_hwc, int c, int h, int w, int resized_h, int resized_w, int top, int left,
                    int out_h, int out_w, float *out, void *stream);
/* the same with nearest sampling for the (h,w) u8 mask (InterpolationMode.NEAREST) */
int rpe_resize_crop_mask(const uint8_t *in, int h, int w, int resized_h, int resized_w, int top, int left, int out_h,
                         int out_w, uint8_t *out, void *stream);
/* Rectification of one image with precomputed maps: cv2.remap(src, mapx, mapy, INTER_NEAREST) with the default constant-0
 * border (dataset/preprocess/stereo_rectify.py:44-51, called per frame by StereoRectifier.__call__,
 * dataset/rectification.py:52-65): dst(ch,y,x) = src(ch, cvRound(mapy[y,x]), cvRound(mapx[y,x])), cvRound = round half to
 * even, saturated to int16; 0 outside the image.  src / dst planar (c,h,w) / (c,out_h,out_w), uint8 or float32
 * (src_is_u8); the maps are the CV_32FC1 pair initUndistortRectifyMap produces (preprocess.StereoRectifier builds them). */
int rpe_remap_nearest(const void *src, int src_is_u8, int c, int h, int w, const float *mapx, const float *mapy, int out_h,
                      int out_w, void *dst, void *stream);

/* Pseudo-rectification of the right image (dataset/rectification.py:55-58 mode='pseudo' -> dataset/preprocess/stereo_rectify.py:
 * 52-59 pseudo_rectify_2d): dst = cv2.warpAffine(src, [[1,0,tx],[0,1,ty]], (w,h)), i.e. INTER_LINEAR with source coordinates
 * rounded to 1/32 pixel (fixed point, AB_BITS = 10), OpenCV's 5-bit bilinear table (uint8: integer weights summing to 2^15,
 * (sum + 2^14) >> 15; float32: float weights), BORDER_CONSTANT 0.  tx = lkmat[0][2] - rkmat[0][2], ty = lkmat[1][2] - rkmat[1][2]
 * as float32 (the reference builds the matrix with .astype(np.float32)).  Planar (c,h,w) uint8 or float32.
 * RESTATED, UNPINNED: the arithmetic above is OpenCV 4.x's imgwarp.cpp as published, restated without cv2 in the build image; it is
 * tested bit for bit against a scalar restatement of the same description (oracle/rectify.py), NOT against cv2.warpAffine itself --
 * a 1-LSB difference to a particular OpenCV build (other interpolation tables, FMA contraction in remapBilinear<float>) would go
 * unnoticed until a golden from real cv2 (oracle/gen_golden.py on a machine that has it) pins both. */
int rpe_shift_bilinear(const void *src, int src_is_u8, int c, int h, int w, float tx, float ty, void *dst, void *stream);

/* The whole input side in one call: n decoded stereo frames -> the tracker's inputs, bit for bit what the chain
 * rpe_mask_specularities (left image) -> rpe_resize_crop (both images) + rpe_resize_crop_mask -> rpe_remap_nearest (both images) or
 * rpe_shift_bilinear (right image) gives frame by frame (dataset/video_dataset.py:55-66; the mask is not rectified there either),
 * without its intermediates: one launch reads the frames and writes limg, rimg (n,3,out_h,out_w) f32 0..255 and mask (n,1,out_h,out_w)
 * u8, nothing else.
 * frames: uint8 HWC.  right == NULL: stacked (n,2h,w,3), the left eye in the upper half (StereoVideoDataset._split_stereo_img);
 * else frames is the left eye (n,h,w,3) and right the other one.  bgr != 0: the channels are stored B,G,R (as a decoder hands them
 * over) and are swapped on load.  user_mask: NULL or (n,h,w) u8, non-zero = valid (rpe_mask_specularities' mask argument).
 * sum_threshold and (resized_h, resized_w, top, left, out_h, out_w) as rpe_mask_specularities / rpe_resize_crop take them.
 * rect_mode: RPE_INGEST_RECT_NONE; RPE_INGEST_RECT_MAPS with the four (out_h,out_w) f32 maps of rpe_remap_nearest (left x, y, right
 * x, y); RPE_INGEST_RECT_SHIFT with rpe_shift_bilinear's (tx, ty) for the right image.  Maps and shift are ignored in other modes.
 * out_w % 4 == 0 (16-byte stores) needs limg / rimg 16-byte and mask 4-byte aligned: RPE_E_BADARG otherwise.  RPE_E_UNSUPPORTED for
 * a reduction so strong (beyond about 8:1 per axis) that a 64x16 output tile's source footprint does not fit 64 KiB of LDS, n > 65535
 * is RPE_E_BADARG.  Frames whose base is not 4-byte aligned are read byte by byte (slower, same result). */
#define RPE_INGEST_RECT_NONE 0
#define RPE_INGEST_RECT_MAPS 1
#define RPE_INGEST_RECT_SHIFT 2
int rpe_ingest_stereo(const uint8_t *frames, const uint8_t *right, int n, int h, int w, int bgr, const uint8_t *user_mask,
                      int sum_threshold, int resized_h, int resized_w, int top, int left, int out_h, int out_w, int rect_mode,
                      const float *lmapx, const float *lmapy, const float *rmapx, const float *rmapy, float tx, float ty,
                      float *limg, float *rimg, uint8_t *mask, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Surfel map of frame-to-model tracking (core/fusion/surfel_map.py; configuration/infer_scared.yaml: frame2frame False).
 *
 * Layout: SoA f32 with capacity cap -- opts (3,cap) world points in mm, rgb (3,cap), conf (cap), t_created (cap) -- so that
 * [:, :n] views are the reference's (3,N) tensors.  The count n lives in a device int32 (*count); *overflow is a device int32 that a
 * kernel ORs with 1 when it would have written past cap (it then writes nothing past cap, stores n = cap and returns normally) and
 * with 2 when n exceeded the caller's n_bound (surfels past the bound are not updated, and source or pixel items past the last
 * launched tile of 1024 are dropped: beyond n <= cap and writes staying inside the destination, the result is then unspecified).
 * No entry point synchronises the host: every kernel reads n from *count and is launched over n_bound, a host-side upper bound
 * of n (the caller tracks n + h*w per fuse).
 * Compactions (init, fuse, prune) preserve order and are deterministic (block counts -> scan -> scatter): the map's order is the
 * reference's (boolean-mask gathers, torch.cat appends).  They read a source map and write a DIFFERENT destination map (the caller
 * ping-pongs two buffers); fuse also updates the source's matched surfels in place before compacting.
 * Frame inputs: depth (h,w) f32 in mm, img (3,h,w) f32, mask (h,w) u8 (nonzero = valid), confidence (h,w) f32.  kmat, kinv: device
 * f32 3x3 row-major (kinv = torch.linalg.inv(kmat), computed once on the host as the reference does per call); poses: device f32
 * 7-vectors [t, q] (lietorch layout).  Arithmetic follows the reference's operation order without FMA contraction: reproject
 * p = depth * (Kinv . (x+.5, y+.5, 1)), transform R p + t, project (K p).xy / clamp((K p).z, 1e-12) (NaN stays NaN).
 * Workspace: rpe_surfel_workspace_bytes(n_bound, h, w) bytes, any alignment of 256. */
typedef struct rpe_surfel_map {
    float *opts;          /* (3, cap) */
    float *rgb;           /* (3, cap) */
    float *conf;          /* (cap) */
    float *t_created;     /* (cap), f32 as in the reference */
    int64_t cap;
    int32_t *count;       /* device: n */
    int32_t *overflow;    /* device: 0, or the OR of 1 (cap reached) and 2 (n > n_bound) */
} rpe_surfel_map;

size_t rpe_surfel_workspace_bytes(int64_t n_bound, int h, int w);
/* SurfelMap(frame=, kmat=, pmat=) (surfel_map.py:45-70): every pixel with mask != 0, in raster order, at pmat . reproject(depth);
 * rgb from img, conf = confidence / conf_thr, t_created = 0.  Writes *dst->count. */
int rpe_surfel_init(const float *depth, const float *img, const uint8_t *mask, const float *confidence, int h, int w, const float *kinv,
                    const float *pmat, float conf_thr, const rpe_surfel_map *dst, void *workspace, void *stream);
/* SurfelMap.fuse(frame, pose) with upscale 1 (surfel_map.py:73-158; other upscales: RPE_E_UNSUPPORTED), then the prune:
 *  1. every surfel i < n of src: (u,v) = project(K, pose^-1 . opts_i); associated when 0 <= u < w-1 and 0 <= v < h-1, pixel
 *     m = round(v - .5) * w + round(u - .5) (half to even, flattened in f32), |z(pose . reproject(depth)[m]) - z_i| < d_thresh and
 *     mask[m]; then conf_i = clamp(conf_i + 1/conf_thr, 0, 1) and, with average_pts, opts_i / rgb_i = (conf_i old * old + 1/conf_thr *
 *     frame) / (conf_i old + 1/conf_thr) -- in place in src;
 *  2. dst = [surfels of src | every pixel with mask != 0 that no surfel associated with, raster order: world point, rgb, conf 1/conf_thr,
 *     t_created = tick], keeping only conf >= 1 | (tick + 1 - t_created) < t_max (the prune after tick += 1).
 * The caller's tick becomes tick + 1.  n_bound >= n of src; dst needs cap >= n + h*w to be safe. */
int rpe_surfel_fuse(const rpe_surfel_map *src, int64_t n_bound, const float *depth, const float *img, const uint8_t *mask, int h, int w,
                    const float *kmat, const float *kinv, const float *pose, float d_thresh, int average_pts, int upscale, float conf_thr,
                    int tick, int t_max, const rpe_surfel_map *dst, void *workspace, void *stream);
/* remove_surfels_by_confidence_and_time (surfel_map.py:150-158) alone: dst = the surfels of src with conf >= 1 | (tick - t_created) < t_max */
int rpe_surfel_prune(const rpe_surfel_map *src, int64_t n_bound, int tick, int t_max, const rpe_surfel_map *dst, void *workspace, void *stream);
/* SurfelMap.render (surfel_map.py:230-264) under extrinsics T: every surfel projects to (u,v) = project(K, T . opts_i); in the image
 * when 0 <= u < w and 0 <= v < h; pixel (int)v * w + (int)u (.long() truncation).  Per pixel the WINNER is the surfel with the largest
 * conf in torch.sort's order (-inf < ... < -0 == +0 < ... < +inf < NaN), ties going to the LARGEST surfel index -- what a stable
 * argsort of conf followed by last-write-wins scattering gives (the reference's own CPU argsort is not stable and its CUDA index_put
 * has no defined winner, so this rule is the deterministic one).  Implemented as one 64-bit atomicMax per in-image surfel on
 * (order-preserving conf bits << 32 | index), then a resolve pass.  Outputs (empty pixels 0): img (3,h,w) = winner's rgb, depth (h,w)
 * = winner's z -- of T . opts when depth_transformed (transform_cpy(T).render(), the tracker's pair in one launch: the identity act of
 * the copy's render is exact), of opts itself otherwise (render(extrinsics=T) writes the untransformed z) --, confidence (h,w) = winner's
 * conf, mask (h,w) u8 = confidence != 0.  Then SparseImgInterpolator(5, 2, 0) on depth and each colour plane
 * (core/interpol/sparse_img_interpolation.py:19-31): NaN pixels become the 5x5 Gaussian (sigma 2, centre weight 0, normalised) of the
 * reflect-padded plane with NaNs read as 0; other pixels are untouched.  Needs h, w >= 3. */
int rpe_surfel_render(const rpe_surfel_map *m, int64_t n_bound, const float *kmat, const float *T, int depth_transformed, int h, int w,
                      float *img, float *depth, float *confidence, uint8_t *mask, void *workspace, void *stream);
/* SurfelMap.transform / transform_cpy (surfel_map.py:205-219): opts_out[:, i] = T . opts_in[:, i] for i < *count (in place allowed);
 * in_cap / out_cap are the row strides of the two (3, cap) arrays. */
int rpe_surfel_transform(const float *opts_in, int64_t in_cap, float *opts_out, int64_t out_cap, const int32_t *count, int64_t n_bound,
                         const float *T, void *stream);

/* K maps per call (ABI minor 4): several sequences tracked frame to model in one batch.  Map k of a call gets bit for bit what the
 * single-map entry point gives it alone -- count, order, t_created, overflow word, render outputs, render tie winners -- but each
 * stage is ONE launch over all K maps (a compaction's scan: one workgroup per map).  maps / dst / src are HOST arrays of K
 * descriptors, n_bounds HOST int64 arrays, kmat / kinv of the fuse and init HOST arrays of K device pointers (each map's own 3x3);
 * batched frame inputs are device tensors of K (or `batch`) rows: depth / mask / confidence (.,1,h,w), img (.,3,h,w), poses (.,7).
 * 0 <= K <= RPE_SURFEL_MAX_MAPS (K = 0: nothing to do, RPE_OK); the maps of one call must not share storage.  The per-map argument
 * table goes into the head of the workspace with small kernel launches (no host copy, no allocation, no synchronisation: the calls
 * can be captured into a graph).  Workspace: rpe_surfel_workspace_bytes_many(K, n_bounds, h, w) bytes (>= the sum of the single-map
 * sizes; 0 on bad arguments), 256-aligned; render and fuse need the K n_bounds of the call, init K zeros. */
#define RPE_SURFEL_MAX_MAPS 64
size_t rpe_surfel_workspace_bytes_many(int nmaps, const int64_t *n_bounds, int h, int w);
/* rpe_surfel_init for K frames: map dst[k] from row k of depth / img / mask / confidence at pmat row k, with kinv[k]. */
int rpe_surfel_init_many(int nmaps, const float *depth, const float *img, const uint8_t *mask, const float *confidence, int h, int w,
                         const float *const *kinv, const float *pmat, float conf_thr, const rpe_surfel_map *dst, void *workspace,
                         void *stream);
/* rpe_surfel_render of map k with n_bounds[k], kmat row k (K,3,3) and T row k (K,7), into row k of img (K,3,h,w), depth /
 * confidence (K,1,h,w) and mask (K,1,h,w) u8: the rows of one batch, no concatenation.  One splat and one resolve launch. */
int rpe_surfel_render_many(int nmaps, const rpe_surfel_map *maps, const int64_t *n_bounds, const float *kmat, const float *T,
                           int depth_transformed, int h, int w, float *img, float *depth, float *confidence, uint8_t *mask, void *workspace,
                           void *stream);
/* rpe_surfel_fuse of map k (src[k] -> dst[k], n_bounds[k], ticks[k], kmat[k], kinv[k]) with frame row rows[k] (0 <= rows[k] < batch) of
 * depth / img / mask and of pose (batch,7): a caller fuses the subset of its maps whose frame passed the gate.  d_thresh, average_pts,
 * upscale, conf_thr and t_max are shared.  Update, block counts, scan and scatter: one launch each. */
int rpe_surfel_fuse_many(int nmaps, const rpe_surfel_map *src, const int64_t *n_bounds, const rpe_surfel_map *dst, const int32_t *ticks,
                         const int32_t *rows, int batch, const float *depth, const float *img, const uint8_t *mask, int h, int w,
                         const float *const *kmat, const float *const *kinv, const float *pose, float d_thresh, int average_pts, int upscale,
                         float conf_thr, int t_max, void *workspace, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * The training step's update (csrc/optim.hip): the global gradient norm and a clipped AdamW step over ANY number of float32 tensors,
 * one launch each -- what torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW.step (amsgrad = False, maximize = False) do in a chain of
 * per-tensor-list launches and, behind a GradScaler, one host synchronisation.  Neither call synchronises the host.
 *
 * table: DEVICE array of n_rows rpe_optim_row, one per tensor (any numel >= 1, < 2^31; the four pointers 4-byte aligned, nothing more).
 * chunks: DEVICE array of n_chunks rpe_optim_chunk, the tensors cut into pieces of RPE_OPTIM_CHUNK elements in table order -- exactly what
 *   rpe_optim_chunk_offsets writes (into HOST memory: the caller uploads it beside the table).  It returns the number of chunks (with
 *   out = NULL: only that), RPE_E_BADARG for a numel < 1, a negative n_rows or cap < the count, RPE_E_UNSUPPORTED for a numel >= 2^31: this
 *   is where sizes are checked, since the calls below see device memory only.  The split is a function of the sizes alone.
 * workspace: rpe_optim_workspace_bytes(n_chunks) bytes, 16-byte aligned, ZEROED ONCE by the caller before its first use (the two tickets in
 *   its head are counted back to zero by every launch); not shared between streams.
 * rpe_grad_norm: record <- {sqrt(sum of squares of every gradient element) in f64, the same rounded to f32, the number of non-finite
 *   gradient elements}.  One f64 partial per chunk (products of floats are exact in f64), the partials added in index order in f64 by
 *   the launch's last workgroup: no float atomics, the same bits on every run.
 * rpe_adamw_step: reads the record on the device.  skip_nonfinite != 0 and record->nonfinite != 0: nothing is written but state[1]
 *   (skipped steps) += 1.  Otherwise state[0] (the step counter t) += 1 and per element, in f32 with the scalars evaluated in f64,
 *     g' = c g, c = min(1, max_norm / (norm + 1e-6)) (max_norm <= 0: c = 1);   p *= 1 - lr weight_decay;
 *     m += (1 - beta1)(g' - m);   v = beta2 v + (1 - beta2) g' g';   p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps).
 *   The gradients are only read.  state: DEVICE long long[2], zero at first.
 * n_rows == 0 (or n_chunks == 0): RPE_OK, nothing launched.  NULL table / chunks / workspace / record / state, negative counts, n_chunks <
 * n_rows: RPE_E_BADARG.
 * --------------------------------------------------------------------------------------------------------- */
#define RPE_OPTIM_CHUNK 4096
typedef struct rpe_optim_row { float *param; const float *grad; float *exp_avg; float *exp_avg_sq; long long numel; } rpe_optim_row;
typedef struct rpe_optim_chunk { int row; int offset; } rpe_optim_chunk;          /* elements [offset, offset + RPE_OPTIM_CHUNK) of tensor `row` */
typedef struct rpe_optim_record { double norm; float norm_f32; int reserved; long long nonfinite; long long reserved2; } rpe_optim_record;
size_t rpe_optim_chunk_floats(void);                                              /* RPE_OPTIM_CHUNK of the loaded library */
int rpe_optim_chunk_offsets(const long long *numel, int n_rows, rpe_optim_chunk *out, int cap);
size_t rpe_optim_workspace_bytes(int n_chunks);
int rpe_grad_norm(const rpe_optim_row *table, int n_rows, const rpe_optim_chunk *chunks, int n_chunks, void *workspace,
                  rpe_optim_record *record, void *stream);
int rpe_adamw_step(const rpe_optim_row *table, int n_rows, const rpe_optim_chunk *chunks, int n_chunks, void *workspace,
                   const rpe_optim_record *record, long long *state, double lr, double beta1, double beta2, double eps, double weight_decay,
                   double max_norm, int skip_nonfinite, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * RAFT's sequence loss on ground-truth flow and its gradient (csrc/flow_loss.hip): what trains the flow network as RAFT itself is trained.
 *     mask   = valid & !(|gt| >= max_flow)             |gt| = the per-pixel Euclidean norm, formed in f64
 *     term_k = (1 / M) sum_{b,c,y,x} mask |pred_k - gt|,   M = b 2 h w: the mean runs over ALL elements, not over the valid ones
 *     loss   = sum_k weights[k] term_k,  k = 0 .. n_preds - 1   (RAFT: weights[k] = gamma^(n_preds - 1 - k), computed by the caller)
 *   and, on the LAST prediction over the mask pixels, the mean end-point error and the fractions with an error below 1, 3 and 5 px.
 * One deliberate departure from upstream RAFT: a masked pixel contributes EXACTLY ZERO to the loss and to the gradient, whatever pred
 * and gt hold there, NaN and inf included (upstream's valid * i_loss makes 0 * NaN = NaN of such a pixel).  A NaN in gt under a valid
 * pixel is not masked (it fails |gt| >= max_flow): loss and that pixel's gradient are NaN, and rpe_adamw_step's non-finite test skips.
 *
 * preds: DEVICE array of n_preds pointers (1 <= n_preds <= 1024), each a contiguous f32 (b,2,h,w) tensor; gt f32 (b,2,h,w); valid uint8
 * (b,h,w), non-zero = valid; weights: DEVICE array of n_preds doubles; any h and w; pointers need the alignment of their element only.
 * rpe_flow_sequence_loss: two launches, no host synchronisation.  The first reads gt and valid once per pixel and every prediction
 *   once, forms differences and magnitudes in f64 and writes one f64 partial per quantity and workgroup (RPE_FLOW_LOSS_TILE pixels each)
 *   into workspace (rpe_flow_sequence_loss_workspace_bytes, 8-byte aligned, no initial state); the second adds the partials in workgroup
 *   order: no float atomics, the same bits on every run.  record: DEVICE double[RPE_FLOW_LOSS_TERMS + n_preds] -- [RPE_FLOW_LOSS_LOSS]
 *   the loss, [_EPE], [_1PX], [_3PX], [_5PX] the metrics (NaN when no pixel is in the mask), [_COUNT] the number of mask pixels as a
 *   long long in that slot, [_TERMS + k] = term_k (unweighted); loss_f32: the loss rounded to f32.
 * rpe_flow_sequence_loss_backward: one launch; g: DEVICE float, d L / d loss.  grads: DEVICE array of n_preds pointers to f32 (b,2,h,w)
 *   buffers, every element of which is written:  grads[k] = float32(weights[k] g / M) sign(pred_k - gt)  on mask pixels (NaN where the
 *   difference is NaN), exact 0 on masked pixels and where pred_k == gt.  The mask is formed again: nothing but the inputs is kept.
 * NULL pointers, n_preds < 1, b, h or w < 1, max_flow not > 0: RPE_E_BADARG; n_preds > 1024 or h w >= 2^30: RPE_E_UNSUPPORTED.
 * --------------------------------------------------------------------------------------------------------- */
#define RPE_FLOW_LOSS_TILE 1024
#define RPE_FLOW_LOSS_LOSS 0
#define RPE_FLOW_LOSS_EPE 1
#define RPE_FLOW_LOSS_1PX 2
#define RPE_FLOW_LOSS_3PX 3
#define RPE_FLOW_LOSS_5PX 4
#define RPE_FLOW_LOSS_COUNT 5
#define RPE_FLOW_LOSS_TERMS 6
size_t rpe_flow_sequence_loss_workspace_bytes(int n_preds, int b, int h, int w);
int rpe_flow_sequence_loss(const float *const *preds, int n_preds, const float *gt, const uint8_t *valid, const double *weights, int b, int h,
                           int w, double max_flow, void *workspace, double *record, float *loss_f32, void *stream);
int rpe_flow_sequence_loss_backward(const float *const *preds, int n_preds, const float *gt, const uint8_t *valid, const double *weights,
                                    const float *g, int b, int h, int w, double max_flow, float *const *grads, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RPE_H */
