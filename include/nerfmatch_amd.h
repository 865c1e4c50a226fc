/*
 * nerfmatch_amd -- C ABI of the MI355X (gfx950) implementation of the NeRFMatch hot path.
 *
 * The reference (nv-dvl/nerfmatch) has no FFI layer: its boundary is the Python class API
 * (SURVEY.md section 8b).  Every entry point below replaces a stack of eager torch ops inside one of
 * those classes; the reference location each one replaces is cited as file:line relative to the
 * reference tree.  the nerfmatch_amd python modules bind these with ctypes.
 *
 * Conventions
 *   - all tensors are contiguous row-major fp32 unless stated; `dev` = device (HBM) pointer,
 *     `host` = host pointer;
 *   - no allocation, no global state, no synchronisation inside: work is enqueued on `stream`
 *     (a hipStream_t passed as void*) and the call returns immediately;
 *   - return value: NM_OK or an NM_ERR_* code (nm_error_string() gives text).  Nothing is enqueued
 *     when an error is returned.
 */
#ifndef NERFMATCH_AMD_H
#define NERFMATCH_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* nmStream_t; /* hipStream_t */

enum {
  NM_OK = 0,
  NM_ERR_ARG = 1,         /* null pointer / non-positive size */
  NM_ERR_UNSUPPORTED = 2, /* shape outside what the kernels are built for */
  NM_ERR_LAUNCH = 3,      /* HIP reported a launch error */
  NM_ERR_WORKSPACE = 4    /* workspace too small */
};

/* Bumped on every removed or re-signed symbol; nm_abi_version() of a loaded library must equal the binding's own number. */
#define NM_ABI_VERSION 3
int nm_abi_version(void);
const char* nm_error_string(int code);

/* Measurement aid (bench.py's `roofline.peak_sustained`; no reference counterpart): a bare v_mfma_f32_32x32x16_f16 stream,
 * `workgroups` x 4 wavefronts x `rounds` x 24 MFMAs of 32768 FLOP; sink: workgroups * 256 floats. */
int nm_probe_mfma_f16(float* sink, int workgroups, int rounds, nmStream_t stream);

/* Compute-unit partitions (round 6; no reference counterpart -- the reference runs render and matcher of its batch-1 loop one after the
 * other on torch's default stream, nerfmatch/nerfmatch_evaluator.py:556-574, :660-679).  nm_stream_create_cu_mask returns a HIP stream
 * whose kernels run on the compute units whose bits are set in mask_host (n_words 32-bit words, bit i = unit i / 8 of XCD i % 8), so that
 * one query's render (persistent workgroups, one per CU of the partition) and the previous query's matcher (many short dependent launches
 * on the rest of the chip) run side by side.  nm_stream_cus(stream) = the number of CUs a persistent kernel on `stream` sizes its grid to
 * (the partition's size; the whole device for any other stream).  Results never depend on it: tiles are independent.
 * The registry of such streams (at most 16) is the library's only process-wide state.  nm_stream_destroy takes only streams made here. */
int nm_stream_create_cu_mask(const uint32_t* mask_host, int n_words, nmStream_t* stream);
int nm_stream_destroy(nmStream_t stream);
int nm_stream_cus(nmStream_t stream);

/* Parameter fingerprints (round 6; no reference counterpart: the reference keeps no derived copies of its parameters).  One launch sums
 * the 32-bit words of n_tensors device tensors (ptrs_dev[i], words_dev[i] words; 64-bit wrap-around sums with position-dependent odd
 * multipliers: exact in any order) over n_blocks workgroups of 16384 words (blk_tensor_dev / blk_off_dev: tensor and first word of each)
 * into cur_dev[n_tensors] (zero before the first launch; left zero by every launch).  baseline != 0: ref_dev := the sums, ctrl_dev[1] := 0;
 * baseline == 0: ctrl_dev[1] := 1 when some tensor's sum differs from ref_dev (sticky).  ctrl_dev: int32[2], zero before the first launch.
 * The python classes use it to notice parameters that were modified through `.data` behind their packed copies (ops.ParamGuard). */
int nm_params_fingerprint(const void* const* ptrs_dev, const long long* words_dev, const int* blk_tensor_dev, const long long* blk_off_dev,
                          int n_tensors, int n_blocks, unsigned long long* cur_dev, unsigned long long* ref_dev, int* ctrl_dev, int baseline,
                          nmStream_t stream);

/* ------------------------------------------------------------------------------------------------
 * NeRF render half
 * ---------------------------------------------------------------------------------------------- */

/* Ray bundle for the pixels (ds/2 + i*ds, ds/2 + j*ds) of an H x W image.
 * Replaces sample_nerf_rays + get_ray_dirs + get_rays_c2w + rays_intersect_sphere + prepare_rays_data
 * (nerfmatch/nerf/render_utils.py:23-41, :56-104; nerfmatch/nerf/scene_utils.py:101-120), which run on
 * the CPU at full resolution in the reference.
 *   Kinv_host   : 9 floats, inverse intrinsics (row-major)
 *   c2w_host    : 16 floats, NORMALISED camera-to-world (row-major 4x4)
 *   rays (dev)  : [R,12] = o(3) viewdir(3) near far viewdir(3) radius, R = nm_raygen_count(H,W,ds)
 *   fallback (dev): one int; set to 1 when some ray misses the unit sphere, in which case EVERY ray
 *                 gets far = 1 (the reference's assert -> except path, render_utils.py:62-68). */
int nm_raygen_count(int H, int W, int ds);
int nm_raygen(const float* Kinv_host, const float* c2w_host, int H, int W, int ds, float near_plane,
              float* rays, int* fallback, nmStream_t stream);
/* Q poses in one launch: c2w_host = Q row-major 4x4 matrices (16 floats each), rays [Q*R,12], fallback [Q].  Same arithmetic as
 * Q calls of nm_raygen (the batched renderer render_novel_views uses this). */
int nm_raygen_batch(const float* Kinv_host, const float* c2w_host, int Q, int H, int W, int ds, float near_plane,
                    float* rays, int* fallback, nmStream_t stream);

/* Stratified fence posts t[R,S+1] from rays[R,12] and t_rand[R,S+1] ~ U[0,1).
 * Replaces sample_gaus_along_rays' t_vals (nerfmatch/nerf/render_utils.py:434-445). */
int nm_sample_coarse(const float* rays, const float* t_rand, int R, int S, float* t_out, nmStream_t stream);

/* Hierarchical re-sampling: t_out[R,S+1] from t_in[R,S+1], weights[R,S], jitter[R,S+1].
 * Replaces resample_gaus_along_rays + sorted_piecewise_constant_pdf
 * (nerfmatch/nerf/render_utils.py:453-552, :583-597) including the `u + u + jitter` behaviour of the
 * randomized branch.  jitter may be NULL when randomized == 0.  The jitter is given UNSCALED: the kernel multiplies it by
 * `jitter_scale` where it reads it (one fp32 product, what the reference's `torch.rand_like(u) * (1 / n - eps)` computes,
 * render_utils.py:472-476) -- saves the caller an elementwise launch; 1.0f for a jitter that is already scaled.
 * The call also reports whether the result has the zero-width tail NM_NERF_ZERO_TAIL relies on:
 * *zero_tail_violation (device int, may be NULL) is set to 0 before the launch and raised (non-zero) when some fence post
 * j > S/2 does not sit at u = 1 - eps (cannot happen for 0 <= jitter; always raised when randomized == 0).  Hand the same
 * pointer to nm_nerf_fwd_bf16x3: the decision "skip the tail or evaluate everything" is then taken on the device, with
 * no host synchronisation and no promise by the caller. */
int nm_resample(const float* t_in, const float* weights, const float* jitter, float jitter_scale, int R, int S, float padding,
                int randomized, float* t_out, int* zero_tail_violation, nmStream_t stream);

/* Weights of one NeRF MLP in the reference's (torch nn.Linear, [out,in]) layout, HOST pointers.
 * Keys: {nerf_coarse|nerf_fine}.{pts_linears.i, alpha_linear, feature_linear, views_linears.0, rgb_linear}
 * (nerfmatch/nerf/models/nerf.py:45-63). */
typedef struct {
  const float* pts_w[8]; /* [256,90] [256,256]x4 [256,346] [256,256]x2 */
  const float* pts_b[8]; /* [256] */
  const float* alpha_w;  /* [1,256] */
  const float* alpha_b;  /* [1] */
  const float* feat_w;   /* [256,256] */
  const float* feat_b;   /* [256] */
  const float* views_w;  /* [128, 283 + app_dim] */
  const float* views_b;  /* [128] */
  const float* rgb_w;    /* [3,128] */
  const float* rgb_b;    /* [3] */
  int app_dim;           /* 0 or 16 */
} nmNerfWeights;

/* Pack into the MFMA-operand-ordered blob nm_nerf_fwd consumes (host -> host; upload it once). */
size_t nm_nerf_blob_floats(void);
int nm_nerf_pack(const nmNerfWeights* w, float* blob_host);

enum {
  NM_NERF_SKIP_RGB = 1, /* do not evaluate the views layer (with feature_linear folded into it) and the rgb head; rgb output is not written */
  NM_NERF_FEAT_MAX = 2, /* feat/pts of the max-weight sample instead of the weighted sum (feat_comb == "max") */
  /* Premise: every interval s > S/2 of every ray has zero width (t[s+1] == t[s]) -- what nm_resample with
   * randomized = 1 produces for any jitter >= 0 (a promise of the caller when the split kernels get zero_tail_violation == NULL;
   * verified on the device when they are handed the flag nm_resample wrote), because the reference's `u + u + jitter` saturates at the upper half of the fence posts
   * (nerfmatch/nerf/render_utils.py:477-496).  Such samples have alpha = 0, i.e. weight exactly 0 in every output, so
   * nm_nerf_fwd_bf16x3 evaluates samples 0 .. S/2 only and writes weight 0 for the rest: same results, ~half the
   * matrix work.  Honoured for S in {64, 128} and multiples of 256, raw == sample_feat == NULL, without NM_NERF_FEAT_MAX; ignored otherwise and by
   * nm_nerf_fwd (which evaluates everything). */
  NM_NERF_ZERO_TAIL = 4
};

/* One pass (coarse or fine) of the fused conical-frustum -> IPE -> 8x256 MLP -> alpha-composite pipeline.
 * Replaces cast_rays/conical_frustum_to_gaussian/lift_gaussian (nerfmatch/nerf/render_utils.py:326-402),
 * PositionalEncodingMIP.forward (nerfmatch/nerf/embedding.py:66-84), NeRF.forward
 * (nerfmatch/nerf/models/nerf.py:94-144), the chunked forward_nerf loop (nerfmatch/nerf/renderer.py:119-180),
 * volume_render_radiance_field (nerfmatch/nerf/render_utils.py:176-230) and the weighted feature / point sums
 * of render_rays (nerfmatch/nerf/renderer.py:250-281).
 *   blob (dev)      nm_nerf_pack output                     rays (dev) [R,12]      t (dev) [R,S+1]
 *   app_row (dev)   [16] appearance embedding row or NULL   tap_layer  0..7, or -1 = last pts layer
 *   var_scale       <= 0: off (mip_var_scale)               S in {32,64,128} or a multiple of 128
 * outputs (dev; any may be NULL = not wanted, except weights):
 *   weights [R,S]  feat [R,256]  pts [R,3]  rgb [R,3]  depth [R]  acc [R]
 *   raw [R,S,4] (rgb, raw sigma per sample)   sample_feat [R,S,256] (tapped activation per sample) */
int nm_nerf_fwd(const float* blob, const float* rays, const float* t, const float* app_row, int R, int S,
                int tap_layer, int white_bg, float var_scale, int flags, float* weights, float* feat, float* pts,
                float* rgb, float* depth, float* acc, float* raw, float* sample_feat, nmStream_t stream);
/* Guarded form: the launch does nothing unless bit 0 of run_if[0] (device int32[16], required) is set when the kernel starts --
 * the decision is taken on the device, no host synchronisation.  Used as the fall-back of nm_nerf_fwd_fp16x3: hand it the
 * same outputs and that call's `status`; when an fp16 operand saturated there, this pass rewrites every output in fp32.
 * The flag is CONSUMED: after the rewrite bit 0 of run_if[0] is cleared and run_if[11] (a count of such events, sticky) goes up
 * by one; run_if[12] is scratch of this call.  NM_NERF_ZERO_TAIL is ignored (every sample is evaluated).
 * ONE STREAM PER STATUS BLOCK: launches that share a run_if / status block must not overlap (the completion counter in run_if[12]
 * and the clearing of bit 0 assume the fp16x3 launch and this one are the only users until this one has finished); concurrent renders
 * on different streams each need their own block. */
int nm_nerf_fwd_guarded(const float* blob, const float* rays, const float* t, const float* app_row, int R, int S,
                        int tap_layer, int white_bg, float var_scale, int flags, float* weights, float* feat, float* pts,
                        float* rgb, float* depth, float* acc, float* raw, float* sample_feat, int* run_if,
                        nmStream_t stream);

/* Same pass on the bf16 matrix cores with fp32-accurate operand splitting (every product = w_hi*x_hi + w_hi*x_lo +
 * w_lo*x_hi, fp32 accumulation): identical arguments and outputs, its own packed blob.  Differences to the fp32
 * oracle are < 1e-6 on the rendered features (tolerance 1e-4); see DESIGN.md section 3.1b.
 * The kernel is persistent (one workgroup per CU) and parks the tapped activations of the tile in flight in
 * `workspace` (device, nm_nerf_workspace_bytes_bf16x3() bytes, L2-resident; may be NULL when neither feat nor
 * sample_feat is requested).  One workspace per stream: calls that may overlap in time must not share it. */
size_t nm_nerf_blob_bytes_bf16x3(void);
size_t nm_nerf_workspace_bytes_bf16x3(void);
int nm_nerf_pack_bf16x3(const nmNerfWeights* w, void* blob_host);
/* The zero-tail decision can be taken on the device: `zero_tail_violation` is the flag nm_resample wrote for the very `t` passed here
 * (device int, may be NULL = trust the NM_NERF_ZERO_TAIL flag, a promise of the caller).  With NM_NERF_ZERO_TAIL set and the flag
 * raised the kernel evaluates every sample. */
int nm_nerf_fwd_bf16x3(const void* blob, const float* rays, const float* t, const float* app_row, int R, int S,
                       int tap_layer, int white_bg, float var_scale, int flags, float* weights, float* feat, float* pts,
                       float* rgb, float* depth, float* acc, float* raw, float* sample_feat, void* workspace,
                       const int* zero_tail_violation, nmStream_t stream);

/* Same pass with the operands split into fp16 hi / lo parts instead of bf16 ones (22 mantissa bits instead of 16; the three
 * products run on v_mfma_f32_32x32x16_f16 at the bf16 rate; operands beyond +-65504 saturate): fp32-class results also on
 * trained-like scenes (densities of +-1e4, opacity saturating within a few samples), where the bf16 split leaves the
 * compositing weights 7e-4 off -- tests/golden/nerf_surface_r512_s128.npz, DESIGN.md section 3.1b.  Same blob size, workspace
 * and arguments as nm_nerf_fwd_bf16x3, plus `status`; the blob comes from nm_nerf_pack_fp16x3.  Replaces the same reference lines:
 * nerfmatch/nerf/renderer.py:119-180, nerf/models/nerf.py:94-144, nerf/render_utils.py:176-230.
 * Power-of-two operand scaling, range telemetry and a saturation flag for the fp16 split:
 * an fp16 hi/lo pair carries 22 significant bits only while its lo part is a normal fp16 number (|x| >~ 2^-3); the pack step
 * therefore multiplies every weight group by a power of two chosen from its own maximum (constants: cannot saturate) and the
 * kernel carries the hidden activations of layer l at 2^act_log2[l] times their value; the re-packing of a finished layer
 * folds the change of scale into its bias add (one fma, exact) and every output leaves the kernel in true units.
 *   act_log2 (host, 12 ints, NULL = {12, 0,...,0, 12, 0}: scaled weights, activations as they are): [0] IPE input (|x| <= 1, <= 15),
 *   [1..7] hidden input of pts layers 1..7, [8] layer 7's output = input of the density head and of the views layer (feature_linear
 *   has no activation: the pack step multiplies it into the views layer's hidden columns, the kernels never run it as a layer),
 *   [9] ignored (kept for the 12-int layout), [10] direction PE (<= 15), [11] appearance row.
 * `status` (device int32[16], zeroed by the caller, may be NULL):
 *   status[0] |= 1   when some operand of the launch reached +-65504 (it was clamped): the results are NOT to be trusted --
 *                    launch nm_nerf_fwd_guarded(fp32 blob, same arguments, run_if = status) behind it (which clears the bit again
 *                    and counts the event in status[11]);
 *   status[1 + k]    = max over the launch of the bit pattern of |value| re-packed to fp16 in range slot k (k = 0..7: output of
 *                    pts layer k at the scale act_log2[k + 1]; k = 8: unused, stays 0; k = 9: views-layer extra inputs): divide by
 *                    2^act_log2 to get activation ranges, choose act_log2 with >= 2^4 headroom (NeRF.calibrate does). */
int nm_nerf_pack_fp16x3(const nmNerfWeights* w, const int* act_log2, void* blob_host);
int nm_nerf_fwd_fp16x3(const void* blob, const float* rays, const float* t, const float* app_row, int R, int S,
                       int tap_layer, int white_bg, float var_scale, int flags, float* weights, float* feat, float* pts,
                       float* rgb, float* depth, float* acc, float* raw, float* sample_feat, void* workspace,
                       const int* zero_tail_violation, int* status, nmStream_t stream);

/* Pointwise forward / backward of ONE NeRF MLP on the fused kernel's K-loop machinery (round 4): the fine pass of the iNeRF
 * refinement (nerfmatch/nerfmatch_evaluator.py:348-430), where only d loss / d (ray origin, view
 * direction) is needed -- dX of every layer, no dW.  bf16 hi/lo split (three products, fp32 accumulate).
 *   forward : xi [n,96] (IPE, nm_inerf_encode), xd [n,48] -> out4 [n,4] = (rgb logits r g b, raw sigma) for nm_inerf_composite
 *             (logit = out4, sig = out4 + 3, ld = 4) and `gates` (device, nm_nerf_points_gate_bytes(n)): one bit per ReLU
 *             activation of the nine layers -- all the backward pass needs from the forward one;  blob: nm_nerf_pack_bf16x3
 *   backward: g4 [n,4] = d loss / d (logits, sigma) (nm_inerf_composite_bwd with ld = 4) -> g_xi0, g_xi5 [n,96]: the two
 *             contributions to d loss / d xi (through layer 0 and through the skip connection; their sum feeds
 *             nm_inerf_encode_bwd), g_xd [n,48];  blob_bwd: the transposed weights, nm_nerf_pack_bwd_bf16x3 (host -> host). */
size_t nm_nerf_blob_bytes_bwd_bf16x3(void);
size_t nm_nerf_points_gate_bytes(int n);
int nm_nerf_pack_bwd_bf16x3(const nmNerfWeights* w, void* blob_host);
int nm_nerf_points_fwd_bf16x3(const void* blob, const float* xi, const float* xd, int n, float* out4, void* gates, nmStream_t stream);
/* forward, "from rays" form: sample n = (ray n / S_act, interval n % S_act) is encoded inside the kernel (nm_inerf_encode's formulas:
 * frustum Gaussian of [z[s], z[s+1]], IPE with exact sine / exponential, direction PE, appearance row) -- no xi / xd arrays.
 * With a TAPPED layer (the matching term of the refinement, `use_match_loss`, nerfmatch/nerfmatch_evaluator.py:420-441, reads the rendered
 * features pt_feat = sum_s w_s h_tap(s)): additionally feats [R S_act, 256] row-major <- the post-ReLU activations of pts layer `tap_layer`
 * (0..7): the `feats` operand of nm_inerf_ray_sums / nm_inerf_ray_sums_bwd.  No tap: feats NULL and tap_layer -1 (any other mix: NM_ERR_ARG). */
int nm_nerf_points_fwd_rays_bf16x3(const void* blob, const float* rays, const float* z, int R, int S, int S_act, const float* app_row,
                                   int tap_layer, float* out4, void* gates, float* feats, nmStream_t stream);
int nm_nerf_points_bwd_bf16x3(const void* blob_bwd, const float* g4, const void* gates, int n, float* g_xi0, float* g_xi5, float* g_xd,
                              nmStream_t stream);
/* The backward pass with the TAPPED layer of nm_nerf_points_fwd_rays_bf16x3, which sends a gradient back into the rendered features:
 * d loss / d h_tap(n) += tap_weights[n] * g_pt_feat[n / S_act][:] (product, then sum) before that layer's ReLU gate, i.e. what the
 * GEMM chain receives as nm_inerf_ray_sums_bwd's g_feats -- which then need not exist (pass g_feats NULL there). */
int nm_nerf_points_bwd_tap_bf16x3(const void* blob_bwd, const float* g4, const void* gates, int R, int S_act, int tap_layer,
                                  const float* tap_weights, const float* g_pt_feat, float* g_xi0, float* g_xi5, float* g_xd, nmStream_t stream);

/* Same pass with ONE fp16 MFMA per product block (operands rounded once to fp16, fp32 accumulation; its own blob with 8 KiB
 * weight slots): a third of the matrix work of the split-bf16 kernel.  Meant for the COARSE pass of render_rays when only its
 * compositing weights are consumed (they feed nothing but the resampler, render_utils.py:449-505): measured effect on the FINE
 * outputs of a render: features 3.8e-7 from the fp64 result against 3.2e-7 with the split-bf16 coarse pass (fence posts
 * 1.3e-6 against 4.8e-7) -- DESIGN.md section 3.1d; its own outputs carry ~3e-4 relative error, outside the 1e-4 class. */
size_t nm_nerf_blob_bytes_fp16x1(void);
int nm_nerf_pack_fp16x1(const nmNerfWeights* w, void* blob_host);
int nm_nerf_fwd_fp16x1(const void* blob, const float* rays, const float* t, const float* app_row, int R, int S,
                       int tap_layer, int white_bg, float var_scale, int flags, float* weights, float* feat, float* pts,
                       float* rgb, float* depth, float* acc, float* raw, float* sample_feat, void* workspace,
                       const int* zero_tail_violation, nmStream_t stream);

/* pt3d[n,3] = (unnorm[4,4] . [pts,1])[:3]   (nerfmatch/utils/geometry.py:76-85); unnorm_host: 16 floats. */
int nm_unnormalize_points(const float* pts, const float* unnorm_host, int n, float* out, nmStream_t stream);

/* ------------------------------------------------------------------------------------------------
 * iNeRF pose refinement: the differentiable fine pass of NeRFMatchEvaluator.inerf_refinement
 * (nerfmatch/nerfmatch_evaluator.py:348-430).  Forward / backward pairs around the MLP, which runs through nm_linear /
 * nm_linear_bf16x3 (forward and, with transposed weights, backward).  n = R * S_act rows, row r * S_act + s = sample s of
 * ray r; S_act <= S: only the first S_act samples of a ray are evaluated (S/2 + 1 suffices after the randomized
 * resampler: later intervals have zero width, hence zero weight and zero gradient).
 *   nm_inerf_encode      xi [n,96] = IPE(o + t_mean * viewdir, var) (90 columns + zero padding),
 *                        xd [n,48] = [dir PE (27) | appearance row (16) | zero padding]; var from the (detached) frustum
 *   nm_inerf_encode_bwd  d loss / d xi, d loss / d xd  ->  g_o [R,3] (ray origins), g_v [R,3] (rays[:, 8:11])
 *   nm_inerf_composite   rgb logits / raw sigma (column 0..2 / 0 of row-major [n, ld] buffers) -> rgb_map [R,3],
 *                        white background, delta = dz * |rays[:, 3:6]| (render_utils.py:187-230); also writes the
 *                        compositing weights [R, S_act] (may be NULL: not wanted)
 *   nm_inerf_composite_bwd  G = d loss / d rgb_map -> g_logit [n,ld], g_sigma [n,ld] (unused columns zeroed),
 *                        g_d [R,3] (rays[:, 3:6], through |d|); g_weights [R, S_act] is added to the weights' gradient (NULL: none)
 * Matching term (`use_match_loss`, nerfmatch_evaluator.py:420-441): the fine weights also feed the matcher.
 *   nm_inerf_ray_sums          pt_feat [R,C] = sum_s w_s feats[r S_act + s], pts [R,3] = sum_s w_s (o + t_mean d): :423-425
 *                              (the Gaussian means are the detached sampler's: constants of the backward pass)
 *   nm_inerf_ray_sums_bwd      d loss / d pt_feat [R,C], d loss / d pts [R,3] -> g_feats [n,C] (may be NULL: not written), g_weights [R, S_act]
 * ---------------------------------------------------------------------------------------------- */
int nm_inerf_encode(const float* rays, const float* z, int R, int S, int S_act, const float* app_row, float* xi, float* xd,
                    nmStream_t stream);
int nm_inerf_encode_bwd(const float* rays, const float* z, int R, int S, int S_act, const float* g_xi, const float* g_xd,
                        float* g_o, float* g_v, nmStream_t stream);
/* Same with d loss / d xi given as the sum of two arrays (nm_nerf_points_bwd_bf16x3's layer-0 and skip-connection parts). */
int nm_inerf_encode_bwd2(const float* rays, const float* z, int R, int S, int S_act, const float* g_xi_a, const float* g_xi_b,
                         const float* g_xd, float* g_o, float* g_v, nmStream_t stream);
/* d loss / d pose (row-major 4x4 on the device, homogeneous row zero) from the per-ray gradients: origin = pose[:3,3] for every
 * ray, view direction = normalise(pose[:3,:3] . Kinv . (x, y, 1)) on the ds-sub-sampled pixel grid (reference gen_rays,
 * nerfmatch/nerfmatch_evaluator.py:268-286).  g_d (may be NULL): a second gradient w.r.t. the same direction tensor (rays[:, 3:6]).
 * Kinv_host (9), pose_host (16): host, row-major. */
int nm_inerf_pose_grad(const float* Kinv_host, const float* pose_host, int H, int W, int ds, const float* g_o, const float* g_v,
                       const float* g_d, int R, float* g_pose, nmStream_t stream);
int nm_inerf_composite(const float* logit_rgb, const float* sigma_raw, int ld, const float* z, const float* rays, int R, int S,
                       int S_act, float* rgb_map, float* weights, nmStream_t stream);
int nm_inerf_composite_bwd(const float* logit_rgb, const float* sigma_raw, int ld, const float* z, const float* rays,
                           const float* g_rgb_map, const float* g_weights, int R, int S, int S_act, float* g_logit,
                           float* g_sigma, float* g_d, nmStream_t stream);
int nm_inerf_ray_sums(const float* weights, const float* feats, int C, const float* rays, const float* z, int R, int S, int S_act,
                      float* pt_feat, float* pts, nmStream_t stream);
int nm_inerf_ray_sums_bwd(const float* weights, const float* feats, int C, const float* rays, const float* z, const float* g_pt_feat,
                          const float* g_pts, int R, int S, int S_act, float* g_feats, float* g_weights, nmStream_t stream);

/* ---- Compositing along a ray and its backward, one wavefront per ray (csrc/nerf_composite.hip) -------------------------------
 * volume_render_radiance_field (render_utils.py:176-230) on the MLP's own output rows, for the refinement's fused fine pass and for scene
 * training: out4 [R*S_act, 4] = rgb logits | raw sigma per sample (what nm_nerf_points_fwd*_bf16x3 and the GEMM chain write), t [R, S+1]
 * fence posts, delta = dz * |rays[:, 3:6]|; only the first S_act <= S samples of a ray exist (see above).  density = relu(raw sigma +
 * noise [R, S_act] * noise_std) (noise NULL: none), white_bg either way, the +1e-10 in the transmittance product
 *   -> rgb [R,3], depth [R], acc [R], weights [R, S_act] (the last three may be NULL).
 * _bwd: g_rgb [R,3], g_weights [R, S_act] (NULL = none) -> g_out4 [R*S_act, 4] = d loss / d (logits, sigma), what
 * nm_nerf_points_bwd*_bf16x3 reads (the density gate is raw sigma + noise * noise_std > 0), and g_d [R,3] = d loss / d rays[:, 3:6]
 * through |d| (NULL: not wanted).  Prefix product / suffix sum over lanes, 16-byte accesses.  1 <= S_act <= S; S_act > 1024 is
 * NM_ERR_UNSUPPORTED from both. */
int nm_nerf_composite4(const float* out4, const float* t, const float* rays, const float* noise, float noise_std, int white_bg, int R, int S,
                       int S_act, float* rgb, float* depth, float* acc, float* weights, nmStream_t stream);
int nm_nerf_composite4_bwd(const float* out4, const float* t, const float* rays, const float* noise, float noise_std, int white_bg,
                           const float* g_rgb, const float* g_weights, int R, int S, int S_act, float* g_out4, float* g_d, nmStream_t stream);

/* ---- NeRF scene training (csrc/nerf_train.hip) ---------------------------------------------------------------------------
 * The per-ray kernels of one training step of NerfRenderer.render_rays(validation=False) (nerfmatch/nerf/renderer.py:182-295) and
 * compute_nerf_metrics (nerfmatch/utils/metrics.py:59-96); the two MLPs run on nm_linear* / nm_linear_wgrad*.  No gradient flows
 * through t, the frustum Gaussians or the encodings (render_utils.py:299-310, :581-597: sampling under no_grad, stop_grad=True). */

/* rays[R,12], t[R,S+1] -> xi[R*S,96], xd[R*S,48] in the layout of nm_inerf_encode, with the forward render kernels' mean d * t_mean + o
 * (d = rays[:,3:6]; the direction PE from rays[:,8:11]) and var_scale as in nm_nerf_fwd.  Appearance: row ray_id[r] (int64, device) of
 * table[V,16] per ray (embedding_a(ray_id), renderer.py:225); table NULL = none, ray_id NULL = id 1 for every ray (renderer.py:298-299).
 * ray_id_host (may be NULL): the same ids on the host -- an id outside [0, V) is then NM_ERR_ARG before anything is enqueued.  On the
 * device such an id is clamped into the table and counted in *status (int, device, may be NULL; add-only). */
int nm_nerf_train_encode(const float* rays, const float* t, int R, int S, const long long* ray_id, const long long* ray_id_host,
                         const float* table, int V, float var_scale, float* xi, float* xd, int* status, nmStream_t stream);
/* s[R,S+1] = t_to_s(t, min t, max t) (render_utils.py:618-636; minimum and maximum over the WHOLE batch, reduced on the device; g's
 * in-place eps as the reference applies it) and, with weights[R,S], lossfun_distortion (metrics.py:453-465) per ray -> loss_ray[R] and
 * its mean -> loss_mean[1] (may be NULL).  t_is_s != 0: `t` already holds s (s and workspace may then be NULL).
 * workspace: nm_nerf_distortion_workspace_bytes() bytes.  S <= 1024.
 * _bwd: g_weights[R,S] = scale / R * (2 sum_j w_j |u_i - u_j| + 2 w_i (s_{i+1} - s_i) / 3), u the interval midpoints of s. */
size_t nm_nerf_distortion_workspace_bytes(void);
int nm_nerf_distortion(const float* t, int t_is_s, const float* weights, int R, int S, void* workspace, float* s, float* loss_ray,
                       float* loss_mean, nmStream_t stream);
int nm_nerf_distortion_bwd(const float* s, const float* weights, int R, int S, float scale, float* g_weights, nmStream_t stream);
/* acc[0] = 0.5 mean(mask (rgb_c - gt)^2), acc[1] = the same of rgb_f (double, fixed summation order; mask[R] NULL = 1; metrics.py:74, :80);
 * g_rgb_c / g_rgb_f [R,3] (may be NULL) = the gradients of coarse_weight * acc[0] + acc[1]. */
int nm_nerf_photo_loss(const float* rgb_c, const float* rgb_f, const float* gt, const float* mask, float coarse_weight, int R, double* acc,
                       float* g_rgb_c, float* g_rgb_f, nmStream_t stream);
/* d loss / d appearance table: columns 27..42 of g_xd_a (+ g_xd_b, may be NULL) [R*S,48] summed per ray into g_ray[R,16] (scratch), then
 * ADDED into g_table[V,16] rows by ray_id (clamped as in nm_nerf_train_encode; NULL = id 1) in a fixed order: no float atomics, two
 * runs give the same bits, and the row of an id that does not occur is left as it is. */
int nm_nerf_app_grad(const float* g_xd_a, const float* g_xd_b, const long long* ray_id, int R, int S, int V, float* g_ray, float* g_table,
                     nmStream_t stream);

/* ---- Training ray batches from device-resident frames (csrc/ray_bank.hip) ---------------------------------------------------
 * Replaces the pre-expanded host ray table of NerfBaseDataset (load_sample + process_train_data, nerfmatch/datasets/nerfbase.py:255-321,
 * :351-385; get_ray_dirs / get_rays_c2w / prepare_rays_data, nerfmatch/nerf/render_utils.py:23-41, :81-104) and the shuffling DataLoader
 * over it.  The bank: images [F,H,W,3] uint8, masks [F,H,W] uint8 or NULL, cams [F,21] = row-major Kinv (9) | rows 0..2 of the normalised
 * camera-to-world (12), flags [F] int32, ts_table [F] int64 (the frame's appearance id) -- all on the device.  Pixel g = (f H + y) W + x.
 * The per-pixel expressions are nm_raygen's: rows of pixels outside the last image row, norm_ray_dir != 0, equal nm_raygen's at ds = 1
 * bit for bit.  The last row's radius is the reference's (the value of row H-3, `dx[-2:-1]`, render_utils.py:94-95), which nm_raygen's is
 * not; hence H >= 3. */

/* flags[f] = 1 iff some pixel of frame f has a unit-sphere discriminant that is not >= 0: every ray of that frame gets far = 1
 * (the try / except around rays_intersect_sphere, nerfbase.py:287-293).  Once per bank. */
int nm_raybank_frame_flags(const float* cams, int F, int H, int W, int* flags, nmStream_t stream);

/* n rays, one thread each.  Ray i's index j comes from ids[i] (int64, device) or, ids == NULL, from the epoch permutation
 * j = perm(pos0 + i * pos_stride); its pixel is g = valid[j] (valid: int64 [n_src], device) or, valid == NULL, g = j.
 *   n_src: the size of the index space of j (the length of `valid`; F*H*W without it).
 *   perm: a keyed bijection of [0, n_src): a balanced 4-round Feistel network on 2 * perm_half_bits bits (the smallest even number with
 *     2^bits >= n_src; <= 40), halves (l, r) -> (r, l ^ (mix(r + key_k) & (2^half_bits - 1))) with nm_pnp_ransac's 32-bit mix, re-applied
 *     while the value is >= n_src (cycle walking).  perm_keys_host: the 4 round keys (host; derived from (seed, epoch) by the caller).
 *     Every position must lie in [0, n_src) (NM_ERR_ARG otherwise).  nerfmatch_amd.nerf.ray_bank.epoch_ids states it in torch.
 * Outputs (device): rays [n,12] = o(3) d(3) near far viewdir(3) radius (16-byte aligned) with d = viewdir (norm_ray_dir != 0) or the
 *   unnormalised dirs . R^T, whose row neighbours then give the radius (nerfbase.py:284); far = (sqrt(disc) - o.v) / v.v from the unit
 *   directions, or 1 where flags[f]; rgbs [n,3] = uint8 / 255 (true division); ts [n] int64 = ts_table[f]; mask [n] (may be NULL; needs
 *   masks) = 1 - round(m / 255) (mask_transient, nerfbase.py:225-228).
 * An index outside its table (ids[i] or valid[j]) is clamped into it and counted in *bad (device int, add-only; zeroed by the caller):
 *   no id can make the kernel leave the tables. */
int nm_raybank_gather(const uint8_t* images, const uint8_t* masks, const float* cams, const int* flags, const long long* ts_table, int F, int H,
                      int W, const long long* ids, const long long* valid, long long n_src, const uint32_t* perm_keys_host, int perm_half_bits,
                      long long pos0, long long pos_stride, int n, int norm_ray_dir, float near_plane, float* rays, float* rgbs, long long* ts,
                      float* mask, int* bad, nmStream_t stream);

/* ---- Reference point sets from a device-resident scene cache (csrc/ref_bank.hip) ----------------------------------------------
 * Replaces NeRFMatchMultiPair.load_ref_pts (nerfmatch/datasets/nerfmatch_dataset.py:441-518) with its reader load_frame_3d
 * (nerfmatch/datasets/data_loading.py:36-80): k cache files unpickled and stacked per query, k projections of all k n points, the
 * co-visibility rule, a randperm draw and a copy to the device.  The bank: pt3d [F,n,3] world, pt_feat [F,n,D], pt_mask [F,n] uint8,
 * cams [F,21] = row-major diag(W / w_f, H / h_f, 1) K_f (9; :486-490) | rows 0..2 of the world-to-camera matrix (12) -- all on the
 * device.  ref_ids [B,k] int64 (device): the frames of each query; candidate c = s n + r of query b is row r of frame ref_ids[b,s].
 * A frame id outside [0, F) is clamped into the bank by every kernel and counted by nm_refbank_gather.
 * Limits (NM_ERR_UNSUPPORTED beyond): k <= 32, k n <= 2^20, P <= 2^20, D % 4 == 0, D <= 1024; B <= 65535.
 * nerfmatch_amd.ref_bank states the rule in torch. */

/* words [B,k n] uint32: bit j of a candidate's word is set iff its projection into camera j of its query's row satisfies
 * x >= 0 && y >= 0 && x < img_w && y < img_h (:498): p = R X + t, q = p / p.z, pix = K q in fp32 in nm_gt_supervision's operation order,
 * no contraction; no depth test; a projection that is not finite sets no bit.  One thread per (query, candidate). */
int nm_refbank_visibility(const float* pt3d, const float* cams, const long long* ref_ids, int F, int n, int B, int k, int img_w, int img_h,
                          uint32_t* words, nmStream_t stream);

/* The co-visibility rule (:478, :499-506), one workgroup per query over its N = k n words.  visible = all; for j = 0 .. k-1:
 * I = |visible & bit_j|, V = |visible|; visible = visible | bit_j if 3 I < V, else visible & bit_j.  decisions [B] int32: bit j = 1 where
 * the union was taken; n_visible [B] int32 = Nv >= 1; list [B,N] int32: the visible candidates in ascending order, then -1. */
int nm_refbank_select(const uint32_t* words, int B, int k, int N, int* list, int* n_visible, int* decisions, nmStream_t stream);

/* Output row q of query b (one wavefront each): candidate list[b, perm_b(q mod Nv)], Nv = n_visible[b] (:509-516 with the randperm replaced):
 * perm_b is nm_raybank_gather's permutation of [0, Nv) with the 4 round keys perm_keys[b] (device uint32 [B,4]; derived by the caller)
 * and 2 * half_bits = the smallest even number of bits with 2^bits >= Nv, taken from Nv on the device.  list == NULL (then P == k n;
 * n_visible and perm_keys unused): row q is candidate q, the stacked layout of :585-590.
 * out_pt3d [B,P,3], out_feat [B,P,D] (bank and output feature rows are copied as 16-byte vectors: both bases 16-byte aligned),
 * out_mask [B,P] uint8.  *bad (device int, add-only; zeroed by the caller) += the entries of ref_ids outside [0, F). */
int nm_refbank_gather(const float* pt3d, const float* pt_feat, const uint8_t* pt_mask, const long long* ref_ids, int F, int n, int D, int B,
                      int k, const int* list, const int* n_visible, const uint32_t* perm_keys, int P, float* out_pt3d, float* out_feat,
                      uint8_t* out_mask, int* bad, nmStream_t stream);

/* ---- Covisibility pair lists from a device-resident scene cache (csrc/covis_pairs.hip) ----------------------------------------
 * Replaces the downloaded `train_pair_txt` lists (pairs-db-covis20.txt; parsed by load_retrieval_pairs / load_topk_retrieval_pairs,
 * nerfmatch/datasets/data_loading.py:94-127), which an SfM toolchain made from a sparse model: which frames see each other follows from
 * the cached renders alone.  The bank is the one of the section above without its features: pt3d [F,n,3] world points in ray order,
 * pt_mask [F,n] uint8, cams [F,21] -- all on the device.  rows [Q] int32 (device; may be NULL: Q == F and row q is frame q): the query
 * frames; an id outside [0, F) is clamped into the bank.  nerfmatch_amd.covis_pairs states the rule in torch.
 * Projection: p = R X + t, q = p / p.z, pix = K q in fp32 in nm_gt_supervision's operation order, no contraction.  A point is SEEN by a
 * camera iff pix is finite, p.z > 0 (a depth-sign test, unlike nm_refbank_visibility), 0 <= x < img_w and 0 <= y < img_h; with the
 * depth test (zself != NULL; the frames' points are one per cell of a gw x gh grid over the image, gw gh == n) also: for the cell
 * c = ((int)y gh / img_h) gw + (int)x gw / img_w of the query frame i, pt_mask[i,c] != 0, zq = zself[i,c] > 0 and
 * fabsf(p.z - zq) <= depth_tol * zq (one fp32 product).
 * Limits (NM_ERR_UNSUPPORTED beyond): F <= 2^20, n <= 2^20, Q <= 2^20, Q F <= 2^31, k <= 64, image and grid sides <= 8192.
 * Every check is made before anything is enqueued.  Integer counts, one writer per element: two runs give the same bytes. */
#define NM_COVIS_QUERY_TILE 32 /* query cameras per workgroup of nm_covis_scores */

/* zself [F,n]: p.z of point (f, r) under camera f -- frame f's own depth map.  pt_mask (may be NULL): where it is 0 the cell holds NaN
 * instead, which fails nm_covis_scores' test zq > 0 like the mask itself.  One thread per point. */
int nm_covis_self_depth(const float* pt3d, const uint8_t* pt_mask, const float* cams, int F, int n, float* zself, nmStream_t stream);

/* scores [Q,F] int32: scores[q,j] = #{ r : pt_mask[j,r] != 0 and point (j, r) is seen by frame rows[q] }, the diagonal like any other
 * entry.  zself == NULL: no depth test (then gw == gh == 0; depth_tol unused); otherwise nm_covis_self_depth's output WITH the bank's
 * pt_mask (the kernel gathers 4 bytes per point from it and reads no mask of the query frame), gw gh == n and
 * 0 <= depth_tol < inf (NM_ERR_ARG otherwise).  One workgroup per (frame j, tile of NM_COVIS_QUERY_TILE rows). */
int nm_covis_scores(const float* pt3d, const uint8_t* pt_mask, const float* cams, const int* rows, const float* zself, int F, int n, int Q,
                    int img_w, int img_h, int gw, int gh, float depth_tol, int* scores, nmStream_t stream);

/* ids [Q,k] int32: row q lists the frames j != rows[q] with scores[q,j] >= min_score (and >= 0) by score descending, then index
 * ascending, padded with -1; n_pairs [Q] int32: how many it lists.  One workgroup per row, k rounds of an arg-max over the packed key
 * (score << 32) | (F - 1 - j). */
int nm_covis_topk(const int* scores, const int* rows, int Q, int F, int k, int min_score, int* ids, int* n_pairs, nmStream_t stream);

/* ---- Pillow-exact Lanczos resize of 8-bit images (csrc/image_prep.hip) --------------------------------------------------------
 * Replaces PIL.Image.resize(img_wh, Image.LANCZOS) and the arithmetic behind it in the reference's process_img
 * (nerfmatch/datasets/nerfmatch_dataset.py:36-61; nerfbase.py:197-237): every output byte equals Pillow's.
 * src [F,H,W,C] uint8, C in {1, 3} -> out_u8 [F,h,w,C] and / or out_f32 [F,C,h,w] = lut[c * 256 + byte] (lut: device float [C,256],
 * needed with out_f32); each output may be NULL, not both.  One launch for all frames; a tile of NM_IMAGE_TILE_W x NM_IMAGE_TILE_H
 * output pixels per workgroup.
 * Tables of an axis in -> out (device int32, made on the host: nerfmatch_amd.image_prep.lanczos_tables states the arithmetic):
 *   bounds [out,2] = (first source index, number of taps) of every output; coefficients in fixed point with 22 fractional bits,
 *   coef_x [ksize_x, w] TAP-major (row x holds tap x of every output column), coef_y [h, ksize_y] output-major.
 *   ksize = ceil(3 max(in / out, 1)) * 2 + 1 (anything else: NM_ERR_ARG), or 0 with NULL tables for an axis that keeps its size.
 * The horizontal pass runs first and is rounded and clipped to uint8; the vertical pass filters those bytes; a pixel is
 * clip((2^21 + sum_x k[x] src[first + x]) >> 22, 0, 255) in int32.
 * white_where (may be NULL): [F,h,w] uint8 at OUTPUT resolution; where it is >= 128 the pixel is 255 in every channel in both outputs.
 * Limits (NM_ERR_UNSUPPORTED beyond): C in {1, 3}; every side <= 8192; a reduction of at most 8 x per axis (ksize <= 51), any
 * enlargement; F <= 65535.  src, out_u8 and out_f32 must be 16-byte aligned (NM_ERR_ARG).  Every check is made before anything is
 * enqueued. */
#define NM_IMAGE_TILE_W 64
#define NM_IMAGE_TILE_H 32
int nm_image_resize_u8(const uint8_t* src, int F, int H, int W, int C, const int* coef_x, const int* bounds_x, int ksize_x,
                       const int* coef_y, const int* bounds_y, int ksize_y, int h, int w, const uint8_t* white_where, const float* lut,
                       uint8_t* out_u8, float* out_f32, nmStream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Matcher half
 * ---------------------------------------------------------------------------------------------- */

enum { NM_ACT_NONE = 0, NM_ACT_RELU = 1, NM_ACT_GELU = 2 };

/* y[M,N] = (act(x[M,K] . w[N,K]^T + bias[N] + pre[M,N]) + residual[M,N]) * [gate[M,N] > 0]   (bias / pre / residual / gate may be NULL).
 * The nn.Linear calls of MultiHeadAttention / FeedForwardNetwork / pt_pe_proj / pt_ffeat_proj
 * (nerfmatch/modules/attention.py:101-103,114,145-147; nerfmatch/nerfmatch_c2f_trainer.py:152-160).
 * `pre` lets a layer with a concatenated input be two GEMMs (the NeRF skip layer, the views layer); `gate` applies the ReLU
 * derivative of a saved activation in the backward GEMMs of the iNeRF refinement. */
int nm_linear(const float* x, const float* w, const float* bias, const float* pre, const float* residual, const float* gate,
              int M, int N, int K, int act, float* y, nmStream_t stream);

/* The same layer (same epilogue) on the bf16 matrix cores with fp32-accurate hi/lo operand splitting (cf. nm_nerf_fwd_bf16x3).
 * The weight matrix is split and laid out once: nm_linear_pack_bf16x3(w [N,K] device, blob device of
 * nm_linear_blob_bytes_bf16x3(N, K) bytes) -- a device-side kernel, asynchronous on `stream`.
 * Requires K % 8 == 0 and N % 8 == 0 (NM_ERR_UNSUPPORTED otherwise; use nm_linear). */
int nm_linear_bf16x3(const float* x, const void* blob, const float* bias, const float* pre, const float* residual,
                     const float* gate, int M, int N, int K, int act, float* y, nmStream_t stream);
size_t nm_linear_blob_bytes_bf16x3(int N, int K);
/* Fused q|k|v (n_q = 32 heads) or k|v (n_q = 0) projection of an attention layer, head_dim 32, split-bf16 path: the weight
 * blob packs the [n_q + 64 heads, K] stack of proj_q / proj_k / proj_v (attention.py:150-166); the q columns are written as
 * fp32 rows q_out[M, n_q], the keys and values go straight into the operand slots of the attention kernel
 * (nm_attention_workspace_bytes(B, S, heads) bytes, B = M / S sequences of S tokens) without ever existing as fp32 rows.
 * nm_attention_presplit then runs the attention over those slots.  n_q and 32 heads multiples of 128, S of 32. */
int nm_linear_qkv_bf16x3(const float* x, const void* blob, int M, int K, int n_q, int heads, int S, float* q_out, void* kv_slots,
                         nmStream_t stream);
int nm_attention_presplit(const float* q, int ldq, const void* kv_slots, int B, int L, int S, int heads, float scale, float* out,
                          nmStream_t stream);
int nm_linear_pack_bf16x3(const float* w, int N, int K, void* blob, nmStream_t stream);
/* Round 6: the blob of the TRANSPOSE -- w is stored (K, N) (an nn.Linear weight (out = K, in = N)); the blob is that of the (N, K) matrix
 * w^T, so that nm_linear_bf16x3(dy, blob) = dy . w is the layer's input gradient (autograd's dx = dy @ W, done by torch in the reference)
 * without a transposed copy of the weight in between.  nm_linear_blob_bytes_bf16x3(N, K) bytes. */
int nm_linear_pack_t_bf16x3(const float* w, int N, int K, void* blob, nmStream_t stream);

/* Row-wise LayerNorm over `dim` in {64,128,256,512} (NM_ERR_UNSUPPORTED otherwise), eps as nn.LayerNorm (1e-5).
 * (nerfmatch/modules/attention.py:196-207, :229-230, :238). */
int nm_layernorm(const float* x, const float* gamma, const float* beta, int rows, int dim, float eps, float* y,
                 nmStream_t stream);
/* Two LayerNorms of equal width in one launch (the two pre-norms of a cross-attention layer, attention.py:229-233): y0 = LN(x0; gamma0, beta0),
 * y1 = LN(x1; gamma1, beta1); row arithmetic identical to nm_layernorm (bit-identical results). */
int nm_layernorm2(const float* x0, const float* gamma0, const float* beta0, int rows0, float eps0, float* y0, const float* x1,
                  const float* gamma1, const float* beta1, int rows1, float eps1, float* y1, int dim, nmStream_t stream);

/* Softmax multi-head attention without materialising the (L,S,H) score tensor.
 * q [B,L,H*D], k,v [B,S,H*D], out [B,L,H*D]; D in {16,32}; scores are (q*scale).k.
 * Replaces FullAttention.forward / LocalitySelfAttention.forward (nerfmatch/modules/attention.py:53-57, :71-81).
 * ldq / ldk / ldv: row strides in floats (>= H*D, multiples of 4): q/k/v may be column slices of one fused projection
 * buffer, e.g. [B*L, 3*H*D] written by a single nm_linear with the concatenated proj_q|proj_k|proj_v weights.
 * flags: NM_ATTN_BF16X3 evaluates QK^T and PV on the bf16 matrix cores with hi/lo operand splitting (fp32-accurate: ~1e-6 on
 * the tokens; head_dim 32 only; ignored for head_dim 16 and for the small-sequence kernel of <= 64-token windows).  On that
 * route K and V are split into bf16 hi/lo MFMA operands once per call into `workspace` (device,
 * nm_attention_workspace_bytes(B, S, heads) bytes; one per stream) and streamed from there by LDS DMA (attention_v2.hip);
 * workspace == NULL where the split kernel applies: NM_ERR_WORKSPACE.  The other routes take no workspace (may be NULL).
 * nlse_out (may be NULL): the forward pass keeps what the backward pass needs -- the split-bf16 kernel also writes
 * nlse_out[B][heads][L] = -(log-sum-exp of the query's scaled scores) in the log2 domain, for nm_attention_bwd's `nlse`.
 * Only that route produces it: nlse_out != NULL on any other route is NM_ERR_UNSUPPORTED. */
enum { NM_ATTN_BF16X3 = 1 };
size_t nm_attention_workspace_bytes(int B, int S, int heads);
int nm_attention(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, int B, int L, int S, int heads,
                 int head_dim, float scale, int flags, void* workspace, float* out, float* nlse_out, nmStream_t stream);

/* The part of a pre-norm encoder layer behind the attention as ONE launch:
 *     y = xh + W2 . gelu(W1 . LN2(xh + att . Wo^T) + b1) + b2          (rows x 256 everywhere, split-bf16 products)
 * replaces the tail of GenericEncoderLayer.forward_pre_norm (nerfmatch/modules/attention.py:229-241: proj_out :131-133, norm2,
 * FeedForwardNetwork :136-154) = nm_linear_bf16x3 + nm_layernorm + 2 x nm_linear_bf16x3.  att / xh / y: device [rows, 256];
 * wo_blob from nm_linear_pack_bf16x3, w1 / w2 blobs from nm_linear_pack_perm_bf16x3 (same size, K in accumulator order: the
 * three products are chained in registers); gamma2 / beta2 / b1 / b2: device [256].  dim != 256: NM_ERR_UNSUPPORTED. */
int nm_linear_pack_perm_bf16x3(const float* w, int N, int K, void* blob, nmStream_t stream);
int nm_encoder_tail_bf16x3(const float* att, const float* xh, const void* wo_blob, const void* w1_perm_blob, const void* w2_perm_blob,
                           const float* gamma2, const float* beta2, const float* b1, const float* b2, int rows, int dim, float eps,
                           float* y, nmStream_t stream);
/* Round 6: the backward of that tail for FROZEN parameters (input gradients only) as one launch -- torch autograd through the same reference
 * lines when the matcher's parameters do not require gradients (the matching term of the iNeRF refinement, nerfmatch_evaluator.py:429-441):
 *   g1 = dy . W2;  du = g1 o gelu'(u_pre);  g2 = du . W1;  d_a = LayerNorm2'(a_pre; g2);  d_xh = dy + d_a;  d_att = d_a . Wo
 * a_pre = xh + att . Wo^T and u_pre = W1 . LN2(a_pre) + b1 are the forward pass's intermediates [rows, 256]; w2t_blob = nm_linear_pack_bf16x3 of
 * W2^T, w1t_perm_blob / wot_perm_blob = nm_linear_pack_perm_bf16x3 of W1^T / Wo^T.  dim must be 256. */
int nm_encoder_tail_bwd_bf16x3(const float* dy, const float* a_pre, const float* u_pre, const void* w2t_blob, const void* w1t_perm_blob,
                               const void* wot_perm_blob, const float* gamma2, int rows, int dim, float eps, float* d_att, float* d_xh,
                               nmStream_t stream);
/* ... and the forward of the same passes as one launch that KEEPS those two intermediates: nm_encoder_tail_bf16x3 (same arithmetic, same order:
 * y is bit-identical) with a_out = xh + att . Wo^T and u_out = W1 . LN2(a) + b1 written on the way, [rows, 256] each. */
int nm_encoder_tail_save_bf16x3(const float* att, const float* xh, const void* wo_blob, const void* w1_perm_blob, const void* w2_perm_blob,
                                const float* gamma2, const float* beta2, const float* b1, const float* b2, int rows, int dim, float eps,
                                float* y, float* a_out, float* u_out, nmStream_t stream);

/* THROUGHPUT configuration (BASELINE.json config 5, "fp8 MFMA attention"), head_dim 32: both contractions with ONE
 * v_mfma_f32_32x32x16_fp8_fp8 per product block on OCP e4m3 operands -- keys / values scaled per (batch, head), queries per
 * query, probabilities by 2^8 after the shift by the running maximum (all powers of two); fp32 accumulation and row sums.
 * NOT a parity arithmetic: 3 mantissa bits; the error against nm_attention is reported by bench.py (variants.attention_fp8)
 * and bounded by tests/test_matcher_gpu.py::test_attention_fp8_error_bound.  Approximates FullAttention.forward
 * (nerfmatch/modules/attention.py:44-57).  workspace: device, nm_attention_fp8_workspace_bytes(B, S, heads) bytes. */
size_t nm_attention_fp8_workspace_bytes(int B, int S, int heads);
int nm_attention_fp8(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, int B, int L, int S, int heads,
                     float scale, void* workspace, float* out, nmStream_t stream);

/* tokens y[B, h*w, C] = transpose(cfeat x[B,C,h,w]) (+ pe_table[C,table_h,table_w][:, :h, :w] when pe_table != NULL).
 * Replaces flatten/permute + PositionEncodingSine.forward + rearrange (nerfmatch_c2f_trainer.py:240,249-252;
 * third_party/loftr/position_encoding.py:45-50). */
int nm_add_sine_pe(const float* x, const float* pe_table, int B, int h, int w, int C, int table_h, int table_w,
                   float* y, nmStream_t stream);

/* ---- ConvFormer image backbone: the memory-bound kernels (csrc/convformer.hip) -----------------------------------------------
 * The backbone of the reference (MetaFormer_MS / init_backbone, nerfmatch/modules/__init__.py:14-113) is the stem plus stages 0 and 1
 * of timm's convformer_b36 / caformer_b36.  Activations are channel-last rows; its 1x1 convolutions are nm_linear, its LayerNorms
 * nm_layernorm.  All four: fp32, caller's buffers, 16-byte aligned (NM_ERR_ARG otherwise; the one exception: nm_conv_patches' NCHW
 * input, see there), every check before anything is enqueued.
 *
 * nm_dwconv7_nhwc: y[b,h,w,c] = sum_(ky,kx) w49c[ky*7+kx, c] * a(x[b, h+ky-3, w+kx-3, c]), x, y [B,H,W,C], w49c [49,C] tap-major.
 *   a = StarReLU (below) when act_scale / act_bias (device pointers to one float each; both or neither) are given, else the identity;
 *   a tap outside the image contributes 0 (the padding is applied BEHIND the activation).  Per output one fmaf chain over the 49 taps in
 *   (ky, kx) order from 0: independent of tile and batch position.  x != y.
 *   Limits (NM_ERR_UNSUPPORTED beyond): C a multiple of 64 up to 1024, H, W <= 8192, B <= 65535.  A workgroup makes
 *   NM_DWCONV_TILE_H x NM_DWCONV_TILE_W outputs of 32 channels.
 * nm_star_relu: y[i] = scale[0] * relu(x[i])^2 + bias[0] as r = x < 0 ? 0 : x; t = r * r; t = scale * t; y = t + bias (three roundings; a NaN
 *   passes through).  scale, bias: device pointers.  In place (y == x) allowed.
 * nm_conv_patches: rows [B*Ho*Wo, ld], Ho = (H + 2 pad - k) / stride + 1 (Wo alike): column (ky*k + kx)*C + c of row (b, oy, ox) is
 *   x[b, c, oy*stride - pad + ky, ox*stride - pad + kx], zero outside the image; columns k*k*C .. ld-1 are written as zero.
 *   layout 0: x [B,C,H,W], read as single floats and therefore only 4-byte aligned (image q of a batch of odd-sized images);
 *   layout 1: x [B,H,W,C], 16-byte aligned.  ld % 8 == 0 and ld >= k*k*C (NM_ERR_ARG otherwise).  The convolution is then
 *   nm_linear(rows, w [N, ld] in the same column order, bias).  Limits: k <= 7, stride <= 8, pad < k, C <= 1024, H, W <= 8192.
 * nm_nhwc_to_nchw: y[b,c,p] = x[b,p,c] for x [B,HW,C] (the inverse direction of nm_add_sine_pe).  Limits: C % 4 == 0, B <= 65535. */
#define NM_DWCONV_TILE_H 16
#define NM_DWCONV_TILE_W 16
int nm_dwconv7_nhwc(const float* x, const float* w49c, const float* act_scale, const float* act_bias, int B, int H, int W, int C, float* y,
                    nmStream_t stream);
int nm_star_relu(const float* x, const float* scale, const float* bias, size_t n, float* y, nmStream_t stream);
int nm_conv_patches(const float* x, int layout, int B, int C, int H, int W, int k, int stride, int pad, int ld, float* rows,
                    nmStream_t stream);
int nm_nhwc_to_nchw(const float* x, int B, int HW, int C, float* y, nmStream_t stream);

/* ---- ConvFormer image backbone: the kernels of the fp16 inference walk (csrc/gemm_f16.hip and, beside their fp32 forms, convformer.hip /
 * matcher_misc.hip) -------------------------------------------------------------------------------------------------
 * fp16 buffers are `void*` (IEEE binary16 rows).  A value is stored as fp16 by ONE rounding to nearest even that overflows to infinity:
 * nothing saturates.  `overflow` (device int32, may be NULL): every kernel that stores fp16 adds the number of stored values that are
 * not finite while the fp32 value they were rounded from was (the GEMM: while the accumulator, before the activation, was) -- by
 * ordinary vector atomic adds.  Operands 16-byte aligned unless stated (NM_ERR_ARG), every check before anything is enqueued.
 *
 * nm_linear_f16: y[M,N] = epi(x[M,K] . w^T), x fp16 rows, the weight a blob of nm_linear_blob_bytes_f16(N, K) bytes written by
 *   nm_linear_pack_f16 (w [N,K] fp32 on the device, each value rounded to fp16; asynchronous on `stream`), one product per K-step on
 *   v_mfma_f32_32x32x16_f16 with fp32 accumulation.  epi(v) = a(v + bias) + residual: bias [N] fp32 or NULL; a = StarReLU on the fp32
 *   accumulator, op for op nm_star_relu, when star_scale / star_bias (device pointers to one float each; both or neither) are given;
 *   residual [M,N] fp32 or NULL.  out_f16 = 1: y is fp16 rows (residual must be NULL: NM_ERR_ARG); 0: fp32 rows.  Row m's result does not
 *   depend on M.  K % 8 == 0 and N % 8 == 0 (NM_ERR_UNSUPPORTED otherwise).
 * nm_layernorm_f16: nm_layernorm's rows (the same arithmetic: the result is nm_layernorm's, rounded) stored as fp16; dim in {128,256,512};
 *   y 4-byte aligned.
 * nm_dwconv7_nhwc_f16: nm_dwconv7_nhwc with x and y fp16: the input widens exactly, activation and sums are the fp32 kernel's, the sum is
 *   rounded once -- the result is nm_dwconv7_nhwc's on the widened input, rounded.  Same limits.
 * nm_conv_patches_f16: nm_conv_patches with fp16 rows.  layout 0: x fp32 [B,C,H,W] (4-byte aligned), rounded as it is gathered;
 *   layout 1: x fp16 [B,H,W,C], C % 8 == 0 (NM_ERR_UNSUPPORTED otherwise), copied.  ld % 8 == 0 and ld >= k*k*C. */
size_t nm_linear_blob_bytes_f16(int N, int K);
int nm_linear_pack_f16(const float* w, int N, int K, void* blob, nmStream_t stream);
int nm_linear_f16(const void* x, const void* blob, const float* bias, const float* star_scale, const float* star_bias,
                  const float* residual, int M, int N, int K, int out_f16, void* y, int* overflow, nmStream_t stream);
int nm_layernorm_f16(const float* x, const float* gamma, const float* beta, int rows, int dim, float eps, void* y, int* overflow,
                     nmStream_t stream);
int nm_dwconv7_nhwc_f16(const void* x, const float* w49c, const float* act_scale, const float* act_bias, int B, int H, int W, int C,
                        void* y, int* overflow, nmStream_t stream);
int nm_conv_patches_f16(const void* x, int layout, int B, int C, int H, int W, int k, int stride, int pad, int ld, void* rows,
                        int* overflow, nmStream_t stream);

/* ---- NeRF scene training: the kernels of the fp16 mixed-precision walk (csrc/gemm_f16_train.hip, nerf_train.hip) ----------
 * Same conventions as the section above: fp16 buffers are `void*`, one rounding to nearest even that overflows to infinity, `overflow`
 * (device int32, may be NULL) counts stored fp16 values that are not finite while the fp32 value they were rounded from was; operands
 * 16-byte aligned, every check before anything is enqueued.
 *
 * nm_linear_chain_f16: y[M,N] = alpha * [gate > 0] * (act(x[M,K] . w^T + x2[M,K2] . w2^T + bias) + residual): x, x2 fp16 rows; blob, blob2
 *   in nm_linear_pack_f16's layout (nm_linear_blob_bytes_f16(N, K) / (N, K2) bytes; written by nm_linear_pack_f16 or nm_linear_pack_t_f16);
 *   x2 / blob2 both or neither (K2 = 0 without); bias [N] fp32 (the accumulators' start value) or NULL; act = ReLU on the fp32 accumulator
 *   when relu = 1; residual, gate [M,N] fp16 or NULL.  out_f16 = 1: y fp16 rows, counted; 0: fp32 rows, never counted.  One product per
 *   K-step on v_mfma_f32_32x32x16_f16, fp32 accumulation.  Row m's result does not depend on M.  K, K2, N multiples of 8
 *   (NM_ERR_UNSUPPORTED otherwise).
 * nm_linear_pack_t_f16: the blob of w^T (N, K) from the stored w [K,N] fp32: the dX product dy . w of a linear layer.
 * nm_linear_wgrad_f16: dw[N,K] (+)= alpha * dy[M,N]^T . x[M,K] and, db not NULL, db[N] (+)= alpha * column sums of dy, from one pass over
 *   dy: fp16 operands, fp32 accumulation, fp32 results; accumulate = 1 adds onto dw / db.  M is split into slices of
 *   nm_linear_wgrad_f16_slice_rows(M) rows (a multiple of 64; 64 up to M = 16384), one workgroup each per 128 x 128 tile of dw, whose
 *   partials are kept in `workspace` (nm_linear_wgrad_f16_workspace_bytes, else NM_ERR_WORKSPACE) and added in slice order: no atomics,
 *   the same bits on every run.  N, K multiples of 8, dy / x / dw 16-byte aligned (NM_ERR_UNSUPPORTED otherwise).
 * nm_nerf_g4_split_f16: g4[n,4] fp32 (d loss / d (rgb logits, sigma), nm_nerf_composite4_bwd) times the loss scale -> the two zero-padded
 *   fp16 operand rows g_logit[n,8] (columns 0..2) and g_sig[n,8] (column 0) of the backward chain; counted.
 * nm_nerf_train_encode_f16: nm_nerf_train_encode with xi / xd stored as fp16: the fp32 kernel's values, each rounded once. */
int nm_linear_pack_t_f16(const float* w, int N, int K, void* blob, nmStream_t stream);
int nm_linear_chain_f16(const void* x, const void* blob, int K, const void* x2, const void* blob2, int K2, const float* bias,
                        const void* residual, const void* gate, float alpha, int relu, int M, int N, int out_f16, void* y, int* overflow,
                        nmStream_t stream);
int nm_linear_wgrad_f16_slice_rows(int M);
size_t nm_linear_wgrad_f16_workspace_bytes(int M, int N, int K);
int nm_linear_wgrad_f16(const void* dy, const void* x, int M, int N, int K, float alpha, int accumulate, float* dw, float* db,
                        void* workspace, size_t workspace_bytes, nmStream_t stream);
int nm_nerf_g4_split_f16(const float* g4, size_t n, float scale, void* g_logit, void* g_sig, int* overflow, nmStream_t stream);
int nm_nerf_train_encode_f16(const float* rays, const float* t, int R, int S, const long long* ray_id, const long long* ray_id_host,
                             const float* table, int V, float var_scale, void* xi, void* xd, int* status, nmStream_t stream);

/* ---- ConvFormer image backbone: backward of the kernels above (csrc/convformer_bwd.hip) ----------------------------------------
 * Same conventions: fp32, caller's buffers, 16-byte aligned, every check before anything is enqueued, NM_ERR_UNSUPPORTED beyond the
 * forward kernel's limits.  a(x) = scale * relu(x)^2 + bias, r = relu(x).  Every reduction (dw49c, dscale, dbias) is the sum, in a fixed
 * order, of per-workgroup partial sums kept in `workspace` (at least *_workspace_bytes(...) bytes, else NM_ERR_WORKSPACE): no atomics, the
 * same bits on every run.  dscale_dbias: two floats, {dscale, dbias}; NULL = not wanted (no reduction, no workspace).
 *
 * nm_dwconv7_nhwc_bwd_input: da[b,h,w,c] = sum_(ky,kx) w49c[ky*7+kx, c] * dy[b, h-ky+3, w-kx+3, c] (dy zero outside the image), one fmaf
 *   chain per element.  With x and act_scale (both or neither): dx = da * (2 * (scale * r(x))) in that order of roundings,
 *   dscale = sum da * r(x)^2, dbias = sum da over all elements; without: dx = da, and dscale_dbias must be NULL.  dx != dy, dx != x.
 * nm_dwconv7_nhwc_bwd_weight: dw49c[t,c] = sum_(b,h,w) dy[b,h,w,c] * a(x[b, h+ky-3, w+kx-3, c]) over the in-image terms, t = ky*7 + kx,
 *   tap-major [49,C] like the forward's w49c; a = the identity without act_scale / act_bias (both or neither).
 * nm_star_relu_bwd: dx[i] = dy[i] * (2 * (scale * r(x[i]))), dscale = sum dy * r(x)^2, dbias = sum dy; any n >= 1; out of place.
 * nm_conv_patches_bwd: the adjoint of nm_conv_patches for layout 1 with C % 4 == 0 (anything else: NM_ERR_UNSUPPORTED):
 *   dx[b,iy,ix,c] = sum of drows[(b,oy,ox), (ky*k+kx)*C + c] over the (ky, kx) with oy*stride - pad + ky = iy and ox*stride - pad + kx = ix,
 *   added in ascending (ky, kx) order; the columns k*k*C .. ld-1 of drows are not read.  Same limits as nm_conv_patches. */
size_t nm_dwconv7_nhwc_bwd_input_workspace_bytes(int B, int H, int W, int C);
int nm_dwconv7_nhwc_bwd_input(const float* dy, const float* w49c, const float* x, const float* act_scale, int B, int H, int W, int C, float* dx,
                              float* dscale_dbias, void* workspace, size_t workspace_bytes, nmStream_t stream);
size_t nm_dwconv7_nhwc_bwd_weight_workspace_bytes(int B, int H, int W, int C);
int nm_dwconv7_nhwc_bwd_weight(const float* dy, const float* x, const float* act_scale, const float* act_bias, int B, int H, int W, int C,
                               float* dw49c, void* workspace, size_t workspace_bytes, nmStream_t stream);
size_t nm_star_relu_bwd_workspace_bytes(size_t n);
int nm_star_relu_bwd(const float* x, const float* dy, const float* scale, size_t n, float* dx, float* dscale_dbias, void* workspace,
                     size_t workspace_bytes, nmStream_t stream);
int nm_conv_patches_bwd(const float* drows, int layout, int B, int C, int H, int W, int k, int stride, int pad, int ld, float* dx,
                        nmStream_t stream);

/* The reference's encoding MODULES as callable entry points (its evaluator reaches into renderer.xyz_encoder / dirs_encoder directly,
 * nerfmatch/nerfmatch_evaluator.py:385-393).  The fused kernels never call these: they produce the same encodings as MFMA operands.
 *   nm_mip_encode: PositionalEncodingMIP.forward(x, y) (nerfmatch/nerf/embedding.py:66-84) for x, y [n, D], scales 2^min_deg .. 2^(min_deg +
 *     num_freqs - 1).  y != NULL (integrated PE): x_ret [n, 2*num_freqs*D] = exp(-y_enc/2) sin(x_enc) and, when y_ret != NULL,
 *     y_ret = max(0, (1 - exp(-2 y_enc) cos(2 x_enc))/2 - x_ret^2); column = part*num_freqs*D + scale*D + axis, part 1 = phase + fl32(pi/2).
 *     y == NULL (plain PE): x_ret [n, 2*num_freqs*D + D] = [sin(x_enc) | x].
 *     arith 0: expf + fp64-reduced sine (correctly rounded class; the arithmetic of nm_nerf_fwd, the iNeRF kernels and nm_inerf_encode);
 *     arith 1: the exp2 / fp32 Cody-Waite sine device functions the split render kernels (nm_nerf_fwd_fp16x3 / _bf16x3) inline for x_ret.
 *   nm_fourier_embed: FourierEmbedding.forward(x) (embedding.py:35-46, log-scale, scale 1): out [n, D + 2*num_freqs*D] =
 *     [x | sin(2^0 x) | cos(2^0 x) | sin(2^1 x) | ...]. */
int nm_mip_encode(const float* x, const float* y, size_t n, int D, int min_deg, int num_freqs, int arith, float* x_ret, float* y_ret,
                  nmStream_t stream);
int nm_fourier_embed(const float* x, size_t n, int D, int num_freqs, float* out, nmStream_t stream);

/* feature_normalization of NeRFMatcherCoarse's `pt_feat_norm` option (nerfmatch/nerfmatch_coarse_trainer.py:42-47, called on pt_feat and
 * pt3d at :198-200): per set b of x[B,N,D], centroid = mean over the N rows; x -= centroid IN PLACE (the reference's `x -= ...` changes the
 * caller's tensor as well); y[B,N,D] = x / max_r ||x_r||_2.  D <= 1024. */
int nm_feature_normalize(float* x, int B, int N, int D, float* y, nmStream_t stream);

/* out[n, C + 3 + 6*num_freqs] = [feat[n,C] | x | sin(2^0 x) cos(2^0 x) sin(2^1 x) ...]
 * (FourierEmbedding.forward nerfmatch/nerf/embedding.py:35-46 + the cat of cat_pe, nerfmatch_c2f_trainer.py:258-261). */
int nm_cat_fourier(const float* feat, const float* pt3d, int n, int C, int num_freqs, float* out, nmStream_t stream);
/* d loss / d pt3d [n,3] from dy [n, ld] (ld as above, padded to a multiple of 8): the gradient the iNeRF matching term sends
 * to the rendered points (autograd of the same embedding in the reference). */
int nm_cat_fourier_bwd(const float* dy, const float* pt3d, int n, int C, int num_freqs, float* g_pt3d, nmStream_t stream);

/* The same matching for a BATCH of P pairs when the confidence matrix itself is not wanted (inference): the similarity /
 * confidence values exist only in accumulator registers -- two passes of the 128 x 128 tile GEMM on the split-bf16 matrix
 * cores (sums of exp(sim - |scale|), then conf + per-tile row maxima / first columns + column maxima), an exact tie pass for
 * rows whose maximum is attained more than once, ordered compaction -- seven launches per batch instead of nine per pair
 * (csrc/match_fused.hip).  Same reference lines as nm_dual_softmax_match: nerfmatch_c2f_trainer.py:289-300,
 * modules/extract_matches.py:21-36.
 *   im [P,M,C], pt [P,N,C], im_mask [P,M] / pt_mask [P,N] uint8 or NULL; out_i / out_j / out_conf [P,M] (valid prefix:
 *   counts[p]; the slots behind it are written as index 0 / confidence 0); C in {64,128,256,512}; |scale| log2(e) <= 60 (cosine similarities are bounded by |scale|: one fixed shift
 *   serves both soft-maxes) -- otherwise NM_ERR_UNSUPPORTED: use nm_dual_softmax_match per pair.
 * What tests/test_match_fused_routes_gpu.py pins down (case table: tests/match_fused_util.py):
 *   - selection is the reference's mask on EQUAL BITS: row i is matched iff conf[i, j] > threshold (strictly) for a column j that attains the
 *     row maximum (and, mutual != 0, the maximum of column j); among several such columns the FIRST one is returned.  Bit-identical point rows
 *     get bit-identical confidences wherever their columns sit (so do bit-identical image rows), so the lowest unmasked copy is the answer;
 *   - out_i is strictly increasing within a pair; every slot of out_i / out_j / out_conf at or behind counts[p] holds 0 / 0 / 0.0f, so the
 *     buffers may be read as indices before the counts are known;
 *   - the masks are bytes, [P][M] and [P][N], 0 = masked; a masked entry is the reference's fill of -1e9 before both soft-maxes: conf 0, except
 *     that a row AND column without any unmasked entry meet in the uniform value (1/M)(1/N) -- with one side entirely masked every row returns
 *     column 0 at that confidence (threshold permitting);
 *   - scale has either sign (the reference's temp_type "div" arrives as 1 / temperature); fabsf(scale) * log2(e), evaluated in float, must be
 *     <= 60 (the largest such float is accepted, the next one, NaN and infinities are not); P <= 65535; anything else NM_ERR_UNSUPPORTED, and
 *     like every error it is returned before anything is written;
 *   - the workspace needs no initialisation and keeps no state between calls: nm_match_fused_workspace_bytes(P, M, N, C) bytes of any content,
 *     one byte less is NM_ERR_WORKSPACE; pair p of a batch returns the bits it returns alone. */
size_t nm_match_fused_workspace_bytes(int P, int M, int N, int C);
int nm_dual_softmax_match_fused(const float* im, const float* pt, int P, int M, int N, int C, float scale, const uint8_t* im_mask,
                                const uint8_t* pt_mask, float threshold, int mutual, int64_t* out_i, int64_t* out_j,
                                float* out_conf, int* counts, void* workspace, size_t workspace_bytes, nmStream_t stream);

/* Cosine mutual nearest neighbours of two descriptor sets (csrc/match_fused.hip): the reference's mutual_nn_matching
 * (nerfmatch/utils/geometry.py:160-180), which the two-view pose metrics of a NeRF validation step call on the rendered point features.
 *   desc1 [N1,C], desc2 [N2,C] fp32; d = desc / (|desc| + eps) per row, sim = d1 d2^T (split-bf16 matrix cores, only in registers).
 *   nn12[i] = argmax_j sim[i,j], nn21[j] = argmax_i sim[i,j]; where the kernel's own values are exactly equal the LOWEST index wins.
 *   Row i is a match iff nn21[nn12[i]] == i, with score sim[i, nn12[i]]; use_threshold != 0 keeps only score > threshold (strictly).
 *   An all-zero row normalises to zero: its similarities are exactly 0 and take part like any other value.  Non-finite inputs are
 *   outside the contract (the indices stay inside the arrays).
 * Outputs (device): matches [N1,2] int64 (i, nn12[i]) in ascending i and scores [N1] fp32 -- valid prefix: count[0] entries, the rest is
 *   not written; count [1] int32; nn12 [N1] / nn21 [N2] int32, or NULL.  Deterministic: the same inputs give the same bytes.
 * C in {64,128,256,512}, 1 <= N1, N2 <= 2^20 -- otherwise NM_ERR_UNSUPPORTED; N1 or N2 < 1, a negative / non-finite eps or a NaN
 * threshold: NM_ERR_ARG.  workspace: nm_feature_mutual_nn_workspace_bytes(N1,N2,C) bytes (0 for an unsupported shape), else
 * NM_ERR_WORKSPACE.  Every check is made before anything is enqueued. */
size_t nm_feature_mutual_nn_workspace_bytes(int N1, int N2, int C);
int nm_feature_mutual_nn(const float* desc1, const float* desc2, int N1, int N2, int C, float eps, float threshold, int use_threshold,
                         int64_t* matches, float* scores, int* count, int* nn12, int* nn21, void* workspace, size_t workspace_bytes,
                         nmStream_t stream);

/* Dual-softmax matching + (mutual) nearest-neighbour selection for ONE image/point-set pair.
 * Replaces coarse_matching (nerfmatch/nerfmatch_c2f_trainer.py:289-300) + extract_mutual_matches inference branch
 * (nerfmatch/modules/extract_matches.py:21-36).
 *   im [M,C], pt [N,C] raw token features (normalised inside as f/(|f|+1e-6))
 *   scale      multiplies the cosine similarity (temperature for temp_type "mul", 1/temperature for "div")
 *   im_mask[M], pt_mask[N] : uint8 0/1 or NULL
 *   conf [M,N] or NULL (not materialised in HBM when NULL... see DESIGN.md)
 *   im_norm [M,C], pt_norm[N,C] or NULL: the normalised features (ret_feats)
 *   out_i[M], out_j[M] int64, out_conf[M] f32: compacted matches sorted by i; count (dev int): number of matches
 *   workspace: nm_match_workspace_bytes(M,N,C) bytes of device scratch
 * flags: NM_MATCH_BF16X3 computes the similarity matrix on the split-bf16 matrix-core path (cf.
 * nm_linear_bf16x3; needs N % 8 == 0, otherwise the fp32 path is taken).  The softmax sweeps and the equality tests of the
 * selection are unchanged.  NM_MATCH_STATS_ONLY stops behind the similarity matrix and the four soft-max statistics -- what
 * nm_match_focal_loss / nm_match_focal_loss_bwd read from the workspace: the loss of iNeRF's matching term consumes neither the confidence
 * matrix nor a match list (nerfmatch_evaluator.py:429-441) --; conf / out_i / out_j / out_conf / count may be NULL and are not written. */
enum { NM_MATCH_BF16X3 = 1, NM_MATCH_STATS_ONLY = 2 };
size_t nm_match_workspace_bytes(int M, int N, int C);
int nm_dual_softmax_match(const float* im, const float* pt, int M, int N, int C, float scale, const uint8_t* im_mask,
                          const uint8_t* pt_mask, float threshold, int mutual, int flags, float* conf, float* im_norm,
                          float* pt_norm, int64_t* out_i, int64_t* out_j, float* out_conf, int* count, void* workspace,
                          size_t workspace_bytes, nmStream_t stream);

/* 5x5 (win x win) windows, stride 4, zero padding win/2, of the fine map ffeat[C,Hf,Wf] gathered at coarse cells
 * i_ids[K] (row-major over (Hf/4, Wf/4)): out[K, win*win, C].
 * Replaces F.unfold + rearrange + gather (third_party/loftr/fine_matching.py:46-55) without the full unfold. */
int nm_fine_windows(const float* ffeat, int C, int Hf, int Wf, const int64_t* i_ids, const int* count, int max_k,
                    int win, int stride, float* out, nmStream_t stream);

/* Batched form: ffeat[B,C,Hf,Wf], match k reads map map_ids[k] (int64, < B).  One launch for the matches of a whole batch. */
int nm_fine_windows_batch(const float* ffeat, int B, int C, int Hf, int Wf, const int64_t* map_ids, const int64_t* i_ids,
                          const int* count, int max_k, int win, int stride, float* out, nmStream_t stream);

/* Match assembly of one image / point-set pair (nerfmatch_c2f_trainer.py:457-483) as one launch over K match slots:
 * mpt2d_c[k] = pt2d[i_ids[k]] ([M,2]), mpt3d[k] = pt3d[j_ids[k]] ([N,3]), mpt2d_f[k] = mpt2d_c[k] + expec_f[k,:2] * win / 2 * fine_ds
 * (the reference's expression, every intermediate rounded to fp32), pred_mask[k] = (mconf[k] != 0) as bytes.  All K slots are computed:
 * ids must be valid indices in every slot (the match lists of this library are zero-initialised behind their count). */
int nm_assemble_matches(const float* pt2d, const float* pt3d, const int64_t* i_ids, const int64_t* j_ids, const float* expec_f,
                        const float* mconf, int K, float win, float fine_ds, float* mpt2d_c, float* mpt2d_f, float* mpt3d,
                        uint8_t* pred_mask, nmStream_t stream);

/* rows gather: out[k,:] = src[ids[k],:] for k < *count. */
int nm_gather_rows(const float* src, const int64_t* ids, const int* count, int max_k, int dim, float* out,
                   nmStream_t stream);
/* Image side of the fine stage in one launch on the matrix cores (round 5): the 5 x 5 window of every match (FinePreprocess,
 * third_party/loftr/fine_matching.py:58-71) through ONE pre-norm self-attention encoder layer of width 128 with 8 heads of 16 (`fine_sa`:
 * GenericEncoderLayer.forward_pre_norm, nerfmatch/modules/attention.py:229-241; bias-free q / k / v / out projections, exact-erf GELU
 * feed-forward with biases):
 *   out [max_k, 25, 128] = xh + W2 gelu(W1 LN2(xh + MHA(xh)) + b1) + b2,  xh = LN1(window)
 * for the first min(*count, max_k) matches (the rest stays unwritten).  ffeat [B, 128, Hf, Wf]; map_ids / i_ids as nm_fine_windows_batch.
 * The six 128 x 128 weight matrices as nm_linear_pack_perm_bf16x3 blobs (64 KiB each); split-bf16 products, fp32 accumulate.
 * With pt_f [max_k, 128] (the point-side fine features, nm_fine_pt_proj) and expec_f [max_k, 3]: FineMatching's expectation of every match
 * (nm_fine_expectation's arithmetic on the layer's output) is written as well; `out` may then be NULL (the layer's output is not stored).
 * Other shapes: NM_ERR_UNSUPPORTED (use nm_fine_windows_batch + the generic layer kernels). */
int nm_fine_window_layer(const float* ffeat, int B, int C, int Hf, int Wf, const int64_t* map_ids, const int64_t* i_ids, const int* count,
                         int max_k, int win, int stride, int heads, const float* ln1_gamma, const float* ln1_beta, float ln1_eps,
                         const void* wq_perm, const void* wk_perm, const void* wv_perm, const void* wo_perm, const float* ln2_gamma,
                         const float* ln2_beta, float ln2_eps, const void* w1_perm, const float* b1, const void* w2_perm, const float* b2,
                         float scale, float* out, const float* pt_f, float* expec_f, nmStream_t stream);
/* The WHOLE fine stage of the matches in one launch: nm_fine_window_layer with the point side computed inside as well -- pt_f[k] = W1 (W0
 * pt_src[pt_ids[k]] + b0) + b1 (nm_fine_pt_proj's arithmetic; pt_src [rows, pt_c0], transposed weights pt_w0t [pt_c0, 128], pt_w1t [128, 128],
 * biases may be NULL) instead of being read from `pt_f` (give one of the two).  reference: pt_ffeat_proj + FinePreprocess + fine_sa +
 * FineMatching, nerfmatch_c2f_trainer.py:344-350. */
int nm_fine_stage(const float* ffeat, int B, int C, int Hf, int Wf, const int64_t* map_ids, const int64_t* i_ids, const int* count, int max_k,
                  int win, int stride, int heads, const float* ln1_gamma, const float* ln1_beta, float ln1_eps, const void* wq_perm,
                  const void* wk_perm, const void* wv_perm, const void* wo_perm, const float* ln2_gamma, const float* ln2_beta, float ln2_eps,
                  const void* w1_perm, const float* b1, const void* w2_perm, const float* b2, float scale, float* out, const float* pt_f,
                  const float* pt_src, const int64_t* pt_ids, int pt_c0, const float* pt_w0t, const float* pt_b0, const float* pt_w1t,
                  const float* pt_b1, float* expec_f, nmStream_t stream);
/* Point side of the fine stage in one launch (round 5): out[k, :C1] = W1 (W0 src[ids[k]] + b0) + b1 for the first min(*count, max_k) slots, zeros
 * for the rest -- `pt_ffeat_proj` (two Linear layers, no activation between) on the matched points' coarse tokens,
 * nerfmatch/nerfmatch_c2f_trainer.py:344-346.  w0t [C0, C1], w1t [C1, C1]: the TRANSPOSED weights (row k = the weights of input k); biases may be
 * NULL.  fp32 FMAs in K order.  C1 = 128, C0 a multiple of 4 up to 512; other shapes: NM_ERR_UNSUPPORTED (use nm_gather_rows + nm_linear). */
int nm_fine_pt_proj(const float* src, const int64_t* ids, const int* count, int max_k, int C0, int C1, const float* w0t, const float* b0,
                    const float* w1t, const float* b1, float* out, nmStream_t stream);

/* expec_f[K,3] = (E[x], E[y], std) of softmax(<pt_f[k], win_f[k,r]> / sqrt(C)) over the win x win window.
 * Replaces FineMatching.forward (third_party/loftr/fine_matching.py:88-121). */
int nm_fine_expectation(const float* pt_f, const float* win_f, const int* count, int max_k, int win, int C,
                        float* expec_f, nmStream_t stream);

/* ---- training side of the matcher head ---------------------------------------------------
 * The reference trains through torch autograd (NeRFMatcherMS.forward_with_metrics, nerfmatch_c2f_trainer.py:490-551); these
 * are the backward passes of the layers above, called from nerfmatch_amd/autograd.py.  All fp32. */

/* nn.Linear weight gradient dw[N,K] (+)= dy[M,N]^T . x[M,K] (fp32 matrix cores; row slices summed in a fixed order).
 * workspace: nm_linear_wgrad_workspace_bytes(M,N,K) bytes (may be NULL when the whole of M fits one slice and
 * accumulate == 0: NM_ERR_WORKSPACE is returned when it was needed).  N and K multiples of 4, dy / x / dw on 16-byte boundaries
 * (rows move in 16-byte pieces), else NM_ERR_UNSUPPORTED. */
size_t nm_linear_wgrad_workspace_bytes(int M, int N, int K);
int nm_linear_wgrad(const float* dy, const float* x, int M, int N, int K, int accumulate, float* dw, void* workspace,
                    size_t workspace_bytes, nmStream_t stream);
/* The same product on the bf16 matrix cores with hi/lo operand splitting (the arithmetic of nm_linear_bf16x3, i.e. of the dX GEMMs of
 * the same backward pass): N even, K a multiple of 4; same workspace function.  dW of nn.Linear under loss.backward() with the split arithmetic selected.
 * db (may be NULL): the bias gradient db [N] = column sums of dy from the same launch (dy is read once for both; accumulate applies to dw and db alike). */
int nm_linear_wgrad_bf16x3(const float* dy, const float* x, int M, int N, int K, int accumulate, float* dw, float* db, void* workspace,
                           size_t workspace_bytes, nmStream_t stream);
/* bias gradient out[N] (+)= sum_m dy[m,:] (float atomics: order-dependent in the last bits). */
int nm_col_sum(const float* dy, int M, int N, int accumulate, float* out, nmStream_t stream);
/* nm_col_sum with the row chunks' partial sums written to `workspace` (nm_col_sum_workspace_bytes(M,N) bytes, else NM_ERR_WORKSPACE) and added
 * in a fixed order: the same bits on every run. */
size_t nm_col_sum_workspace_bytes(int M, int N);
int nm_col_sum_ordered(const float* dy, int M, int N, int accumulate, float* out, void* workspace, size_t workspace_bytes, nmStream_t stream);
/* exact-erf GELU (nn.GELU(), modules/attention.py:136-154) as a separate pass over the pre-activations u (training keeps
 * u for the backward pass), and du = dh * gelu'(u).  n % 4 == 0. */
int nm_gelu(const float* u, size_t n, float* h, nmStream_t stream);
int nm_gelu_bwd(const float* u, const float* dh, size_t n, float* du, nmStream_t stream);
/* nn.ReLU backward (FeedForwardNetwork with act_fn "relu", nerfmatch/modules/attention.py:136-154): du = dh where the forward's OUTPUT h > 0, else 0.
 * n % 4 == 0.  (The forward is nm_linear's fused NM_ACT_RELU.) */
int nm_relu_bwd(const float* h, const float* dh, size_t n, float* du, nmStream_t stream);
/* nn.LayerNorm backward: dx[rows,dim]; dgamma[dim] and dbeta[dim] are ADDED onto (zero them first) -- or both NULL: input gradient only
 * (frozen parameters: the matching term of the iNeRF refinement, nerfmatch_evaluator.py:429-441).  dim in {64,128,256,512}. */
int nm_layernorm_bwd(const float* x, const float* gamma, const float* dy, int rows, int dim, float eps, float* dx,
                     float* dgamma, float* dbeta, nmStream_t stream);
/* nm_layernorm_bwd with parameter gradients (dgamma, dbeta not NULL; ADDED onto) whose per-workgroup partial sums go through `workspace`
 * (nm_layernorm_bwd_workspace_bytes(rows,dim) bytes, else NM_ERR_WORKSPACE) and are added in a fixed order instead of with float atomics: the
 * same bits on every run.  dx is that of nm_layernorm_bwd. */
size_t nm_layernorm_bwd_workspace_bytes(int rows, int dim);
int nm_layernorm_bwd_ordered(const float* x, const float* gamma, const float* dy, int rows, int dim, float eps, float* dx, float* dgamma,
                             float* dbeta, void* workspace, size_t workspace_bytes, nmStream_t stream);
/* backward of y = f / (|f| + 1e-6) (coarse_matching, nerfmatch_c2f_trainer.py:290-291). dim in {64,128,256,512}. */
int nm_l2norm_bwd(const float* f, const float* dy, int rows, int dim, float* df, nmStream_t stream);

/* Backward of softmax attention (autograd through FullAttention.forward, modules/attention.py:44-57).  q/k/v/o/d_o and the
 * three gradients are row-pitched like nm_attention's q/k/v.  head_dim 32: flash-style recomputation on the fp32 matrix cores
 * (workspace: nm_attention_bwd_workspace_bytes(B,L,S,heads,flags)); flags & NM_ATTN_BF16X3: the same contractions on the
 * bf16 matrix cores with hi/lo operand splitting (attention_bwd_v2.hip; operands pre-split into the workspace);
 * head_dim 16 with L,S <= 64 (fine windows): one thread per row.
 * nlse (may be NULL): the array nm_attention wrote as nlse_out for the same q / k / scale (split-bf16 route only: NM_ERR_UNSUPPORTED
 * with the fp32 kernels): the dQ kernel then makes ONE pass over the keys instead of two (7 instead of 8 tile products per key /
 * query tile pair). */
size_t nm_attention_bwd_workspace_bytes(int B, int L, int S, int heads, int flags);
int nm_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* d_o, int ldq, int ldk, int ldv,
                     int ldo, int lddo, int B, int L, int S, int heads, int head_dim, float scale, float* dq, float* dk, float* dv,
                     int lddq, int lddk, int lddv, int flags, const float* nlse, void* workspace, size_t workspace_bytes,
                     nmStream_t stream);

/* Backward of nm_fine_windows (scatter-add of d out[K,win*win,C] into dffeat[C,Hf,Wf], which the caller zeroes or accumulates
 * onto; float atomics) and of nm_fine_expectation (d_expec[K,3] -> d_pt[K,C], d_win[K,win*win,C]); autograd through
 * third_party/loftr/fine_matching.py:46-55 and :88-121. */
int nm_fine_windows_bwd(const float* dwin, int C, int Hf, int Wf, const int64_t* i_ids, const int* count, int max_k, int win,
                        int stride, float* dffeat, nmStream_t stream);
int nm_fine_expectation_bwd(const float* pt_f, const float* win_f, const float* d_expec, const int* count, int max_k, int win,
                            int C, float* d_pt, float* d_win, nmStream_t stream);

/* Focal loss on the dual-softmax confidence (compute_matching_loss, nerfmatch/utils/metrics.py:372-380) and its gradient.
 * Protocol per training step:  zero acc[4] (double: sum_pos, sum_neg, n_pos, n_neg);  nm_focal_count over the WHOLE batch's
 * conf_gt (uint8 0/1, other values ignored);  then per batch element, right after nm_dual_softmax_match on `workspace`
 * (which still holds the similarity matrix and the soft-max statistics):  nm_match_focal_loss adds the element's loss sums to
 * acc and writes row_t[M] / col_t[N];  loss = acc[0]/acc[2] + acc[1]/acc[3].  nm_match_focal_loss_bwd (same workspace
 * contents) writes ddot[M,N] = grad_loss * d loss / d (im_n . pt_n) and adds d loss / d scale to *dscale (double, may be
 * NULL); grad_loss is a device scalar (NULL = 1).  clamp != 0: conf is clamped to [1e-6, 1 - 1e-6] first (c2f model);
 * clamp == 0: not (NeRFMatcherCoarse.forward_with_metrics, nerfmatch_coarse_trainer.py:380) -- a positive at conf == 0 (a masked entry) is then
 * log 0, an infinite loss and NaN gradients, as in the reference.  A conf_gt byte above 1 is in neither mean and neither count and has
 * t = 0; its ddot is the soft-max coupling alone.  conf_gt, pt_mask and N need no alignment (4-byte aligned pointers and N % 4 == 0 take
 * the faster kernels).  row_t, col_t, ddot and the loss sums are the same bytes on every call when N % 4 == 0, conf_gt is 4-byte aligned
 * and the partial sums fit the workspace (4 nx M rounded up to 256, plus 1024 nx, at most 256 N bytes, nx = ceil(N / 256): not for a tall,
 * narrow pair such as 300 x 8); otherwise col_t and the loss sums are accumulated with atomics.  *dscale always is. */
int nm_focal_count(const uint8_t* conf_gt, size_t total, double* acc, nmStream_t stream);
int nm_match_focal_loss(const uint8_t* conf_gt, int M, int N, int C, float alpha, float gamma, int clamp, void* workspace,
                        size_t workspace_bytes, double* acc, float* row_t, float* col_t, nmStream_t stream);
int nm_match_focal_loss_bwd(const uint8_t* conf_gt, const uint8_t* im_mask, const uint8_t* pt_mask, int M, int N, int C,
                            float alpha, float gamma, int clamp, float scale, const float* grad_loss, void* workspace,
                            size_t workspace_bytes, const double* acc, const float* row_t, const float* col_t, float* ddot,
                            double* dscale, nmStream_t stream);

/* Coarse match supervision of a training batch, built on the device (supervision.hip).  Replaces the numpy code of the reference's
 * dataset classes (nerfmatch/datasets/nerfmatch_dataset.py:302-353 and :553-583; project_points3d, nerfmatch/utils/geometry.py:119-136),
 * which makes a dense float32 M x N matrix per pair on the host.
 *   pt3d [B,N,3], K [B,3,3], w2c [B,3,4] (world-to-camera [R|t]); pt_mask [B,N] / im_mask [B,M] uint8, non-zero = valid, may be NULL;
 *   H, W: image size in pixels, ds: the coarse stride; M: the number of coarse cells (image tokens), (H/ds)*(W/ds) in the reference.
 * Outputs (all caller-allocated, device):
 *   pt2d_proj [B,N,2]  = (K (p / p.z))[:2] with p = R X + t, plain fp32 multiplies / adds and a true division, in the reference's order;
 *   gt_cell   [B,N] int32: with c = floor(pix / ds), the cell is visible iff min(cx, cy) > 0 && cx < W/ds && cy < H/ds; i = cx + cy * (W/ds)
 *             clipped to [0, M-1]; gt_cell = i iff visible && pt_mask[b,j] && im_mask[b,i], else -1.  As in the reference, the strict `> 0`
 *             excludes cell row 0 and cell column 0, and there is no depth test (a point behind the camera whose flipped projection lands
 *             in the image counts).  p.z == 0 or a non-finite projection (undefined in the reference): invisible.
 *             NULL: projection only (every argument after pt2d_proj must be NULL then; M, H, W, ds are ignored);
 *   conf_gt   [B,M,N] uint8 (may be NULL): zero-filled on the stream, 1 at [b, gt_cell[b,j], j] -- what nm_focal_count / nm_match_focal_loss read;
 *   b_ids, i_ids, j_ids [B*N] int64 and counts [B] int32 (all four or none): the entries of conf_gt in torch.where order (ascending b,
 *             then i, then j), sum(counts) of them, the rest of the arrays is left unwritten; counts[b] = entries of batch element b.
 *             Deterministic: the same inputs give the same bytes.  M <= 6400 (a per-cell histogram in LDS), else NM_ERR_UNSUPPORTED.
 *   fallback  [B,2] int32 (i, j) (may be NULL; needs the triple): a batch element WITHOUT any entry gets row b of it as its only entry, in
 *             conf_gt and in the triple (the reference's `if match_gt.sum() < 1`, nerfmatch_dataset.py:347-351; the caller draws the pair);
 *             a row outside [0,M) x [0,N) is ignored.  gt_cell is geometry only and does not show the fallback entry.
 * H % ds != 0 or W % ds != 0: NM_ERR_UNSUPPORTED.  workspace: nm_gt_supervision_workspace_bytes(B,M,N) bytes, needed for the triple only
 * (NM_ERR_WORKSPACE).  Every check is made before anything is enqueued. */
size_t nm_gt_supervision_workspace_bytes(int B, int M, int N);
int nm_gt_supervision(const float* pt3d, const float* K, const float* w2c, const uint8_t* pt_mask, const uint8_t* im_mask, const int* fallback,
                      int B, int M, int N, int H, int W, int ds, float* pt2d_proj, int* gt_cell, uint8_t* conf_gt, int64_t* b_ids,
                      int64_t* i_ids, int64_t* j_ids, int* counts, void* workspace, size_t workspace_bytes, nmStream_t stream);

/* Batched PnP-RANSAC (pnp.hip): the 2D-3D matches of Q queries -> Q world-to-camera poses, three launches, no host round trip.
 *   pt2d [K,2] pixels, pt3d [K,3], grouped by query: query q owns matches [offsets[q], offsets[q+1]); offsets [Q+1] int32 on the DEVICE
 *   (the kernels clamp every range to [0, K], so no offset value can make them leave the arrays); offsets_host: the same Q+1 values on the
 *   host, or NULL -- when given they are checked (non-decreasing, inside [0, K]) before anything is enqueued.  Kmat [Q,3,3], upper
 *   triangular (fx, skew, cx; fy, cy; the last row is taken as 0 0 1).  thr_px: inlier threshold in pixels; n_hyps: hypotheses per query,
 *   a multiple of 64, at most 4096; refine_iters >= 0 Levenberg-Marquardt steps; add_half_px != 0: 0.5 is added to every pixel coordinate
 *   (in fp32) before use.  pt2d / pt3d may be NULL only if K == 0.
 * Outputs (device, caller-allocated): pose [Q,12] fp32 row-major [R | t] (world to camera); n_inliers [Q] int32 -- a value below 4 means
 *   NO POSE (pose is then the identity): fewer than four matches, no hypothesis with four inliers, or a refined pose that keeps fewer than
 *   four in the final fp64 recount; inlier_mask [K] uint8 or NULL (zero outside every query's range and for a query without a pose).
 *   Study outputs, NULL in production: hyp_pose [Q,n_hyps,12] fp32, the hypotheses as K [R | t] (all NaN: the sample gave none), and
 *   hyp_count [Q,n_hyps] int32, their inlier counts.
 * Sampling.  Hypothesis h of a query with n >= 4 matches draws four distinct indices; slot s = 0..3 takes
 *       hash4(seed, h, s, attempt) % n,   attempt = 0, 1, ... until the index differs from the earlier slots'
 *   (after 64 attempts: the smallest unused index), where, in 32-bit unsigned arithmetic,
 *       mix(x):  x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16
 *       hash4(seed, h, s, a) = mix(mix(mix(mix(seed ^ 0x9E3779B9) + h) + s) + a).
 *   The hash does not see the query's position in the batch.  Slots 0..2 feed a P3P minimal solve in fp64; of its up to four roots the one
 *   that reprojects slot 3 best (in front of the camera) is the hypothesis.  A point is an inlier of a hypothesis iff its depth is positive
 *   and its squared pixel residual is <= thr_px^2 (fp32).  The winner maximises (count << 32) | (0xFFFFFFFF - h): most inliers, ties to
 *   the lowest h.  It is refined in fp64 with the inlier set re-evaluated at every step; a step is taken iff the inlier count does not
 *   fall and the cost of the step's inlier set falls.  All sums run in an order fixed by the query's own matches: the outputs of a query
 *   are the same bits alone, in any batch, and on every run.
 * workspace: nm_pnp_ransac_workspace_bytes(Q, n_hyps) bytes (NM_ERR_WORKSPACE).  Every check is made before anything is enqueued. */
size_t nm_pnp_ransac_workspace_bytes(int Q, int n_hyps);
int nm_pnp_ransac(const float* pt2d, const float* pt3d, const int* offsets, const int* offsets_host, const float* Kmat, int Q, int K,
                  float thr_px, int n_hyps, int refine_iters, uint32_t seed, int add_half_px, float* pose, int* n_inliers,
                  uint8_t* inlier_mask, float* hyp_pose, int* hyp_count, void* workspace, size_t workspace_bytes, nmStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NERFMATCH_AMD_H */
